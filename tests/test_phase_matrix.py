"""The matrix layer of the phase calls (phase_matrix.py) on its host path, against the per-cell
oracle of tests/_phase_cases.py and against predict_cycle_phase on the long table."""
import inspect

import numpy as np
import pandas as pd
import pytest

from scdna_replication_tools_amd import phase_matrix as PM
from scdna_replication_tools_amd.phase_matrix import PhaseMatrix, phase_calls
from scdna_replication_tools_amd.predict_cycle_phase import predict_cycle_phase
from tests import _phase_cases as C


def _matrix(device="cpu"):
    rep, cn, reads, ids, _ = C.case()
    return PhaseMatrix(rep, cn, reads, ids, device=device)


def test_host_features_against_the_oracle():
    rep, cn, reads, ids, orc = C.case()
    got = _matrix().features()
    assert list(got.columns) == PM.FEATURE_COLUMNS
    C.assert_features(got, rep, cn, reads, ids, orc)
    assert np.isnan(got['rep_auto']).sum() == 2                     # the all-0 and the all-1 cell
    assert got['cn_bk'].dtype == np.int64 and got['rep_bk'].dtype == np.int64


def test_float64_reads_and_any_positive_scaling():
    rep, cn, reads, ids, orc = C.case()
    r64 = reads.astype(np.float64)
    C.assert_features(PhaseMatrix(rep, cn, r64, ids, device="cpu").features(), rep, cn, r64, ids, orc)
    rpm = r64 / r64.sum(axis=0) * 1e6                               # the reference's rpm column
    got = PhaseMatrix(rep, cn, rpm, ids, device="cpu").features()
    assert np.all(np.abs(got['rpm_auto'].to_numpy() - orc['rpm_auto'].to_numpy())
                  <= C.auto_bound(reads)[np.argsort(ids, kind="stable")])


def test_phase_calls_equal_predict_cycle_phase_on_the_long_table():
    rep, cn, reads, ids, orc = C.case()
    table = phase_calls(_matrix())
    s_, g_, lq_ = predict_cycle_phase(C.long_table(rep, cn, reads, ids), device="cpu")
    ref = pd.concat([s_, g_, lq_]).drop_duplicates("cell_id").set_index("cell_id")["PERT_phase"]
    assert list(table['PERT_phase']) == list(ref.loc[table['cell_id']])
    assert list(table['PERT_phase']) == list(C.oracle_phase(orc))
    assert set(table['PERT_phase']) == {'S', 'G1/2', 'LQ'}
    for col in ('rpm_auto', 'rep_auto'):
        assert np.allclose(table[col + '_norm'], table[col] - np.mean(table[col].values), rtol=0, atol=0,
                           equal_nan=True)


def test_exact_threshold_decision():
    """``exceeds`` decides rep_auto > thresh on the integers: at a threshold equal to a cell's own
    (rounded) rep_auto the answer is the sign of the rounding, which the fp64 comparison cannot see.
    ``phase_calls`` uses it at the reference's 0.2 and compares the fp64 column otherwise."""
    m = _matrix()
    raw, f = m.raw(), m.features()
    num, den = raw["rep_auto_num"][m.order()], raw["rep_auto_den"][m.order()]
    from fractions import Fraction
    live = np.flatnonzero(den != 0)
    for i in live[:6]:
        t = float(f['rep_auto'][i])
        want = Fraction(int(num[i]), int(den[i])) > Fraction(t)
        assert bool(PM.exceeds(num[i:i + 1], den[i:i + 1], t)[0]) == want
    assert not PM.exceeds(num, den, 0.2)[den == 0].any()
    # phase_calls' rule: exact at the reference's threshold, the fp64 column at any other
    assert np.array_equal(PM.rep_auto_exceeds(num, den, 0.2), PM.exceeds(num, den, 0.2))
    for t in (0.1, 0.25, float(f['rep_auto'][live[0]])):
        with np.errstate(invalid="ignore"):
            assert np.array_equal(PM.rep_auto_exceeds(num, den, t), f['rep_auto'].to_numpy() > t)
    calls = phase_calls(m, rep_auto_thresh=0.1)
    low = (calls['rep_auto'] > 0.1) | (calls['frac_cn0'] > 0.05)
    assert np.array_equal((calls['PERT_phase'] == 'LQ').to_numpy(), (low & (calls['PERT_phase'] != 'G1/2')).to_numpy())


def test_two_matrices_concatenate_with_norms_over_both():
    rep, cn, reads, ids, _ = C.case()
    a = PhaseMatrix(rep[:, :10], cn[:, :10], reads[:, :10], ids[:10], device="cpu")
    b = PhaseMatrix(rep[:, 10:], cn[:, 10:], reads[:, 10:], ids[10:], device="cpu")
    both, whole = phase_calls([a, b]), phase_calls(_matrix())
    assert len(both) == len(whole) and list(both['cell_id'][:10]) == sorted(ids[:10])
    merged = both.set_index('cell_id').loc[whole['cell_id']].reset_index()
    assert list(merged['PERT_phase']) == list(whole['PERT_phase'])
    for col in ('rep_auto', 'rpm_auto'):                            # centred over all the cells of both
        centre = np.mean(both[col].values)
        assert np.array_equal(both[col + '_norm'].to_numpy(), (both[col] - centre).to_numpy(), equal_nan=True)
        assert np.array_equal(merged[col].to_numpy(), whole[col].to_numpy(), equal_nan=True)


def test_from_frame_round_trip_and_refusals():
    rep, cn, reads, ids, _ = C.case()
    long = C.long_table(rep, cn, reads, ids)
    got = PhaseMatrix.from_frame(long, device="cpu").features()
    pd.testing.assert_frame_equal(got, _matrix().features())
    shuffled = long.sample(frac=1.0, random_state=0).sort_values('cell_id', kind="stable")   # per-cell orders differ
    for bad in (long.iloc[:-3], shuffled):
        with pytest.raises(ValueError, match="predict_cycle_phase"):
            PhaseMatrix.from_frame(bad, device="cpu")


def test_argument_checks():
    rep, cn, reads, ids, _ = C.case()
    with pytest.raises(ValueError, match="max_lag"):
        PhaseMatrix(rep[:50], cn[:50], reads[:50], ids, device="cpu")           # L = max_lag
    PhaseMatrix(rep[:51], cn[:51], reads[:51], ids, device="cpu").features()    # the shortest legal series
    with pytest.raises(ValueError):
        PhaseMatrix(rep, cn, reads, ids, device="cpu", max_lag=65)
    with pytest.raises(ValueError):
        PhaseMatrix(rep, cn[:, :5], reads, ids, device="cpu")
    with pytest.raises(ValueError):
        PhaseMatrix(rep * 2, cn, reads, ids, device="cpu")
    with pytest.raises(ValueError):
        phase_calls([])


def test_other_lags_and_lag_zero():
    """min_lag = 1 averages lag 0 (= 1) too: the exact rational against the oracle."""
    rep, cn, reads, ids, _ = C.case()
    for min_lag, max_lag in ((1, 50), (5, 64), (50, 50)):
        got = PhaseMatrix(rep, cn, reads, ids, device="cpu", min_lag=min_lag, max_lag=max_lag).features()
        orc = C.oracle_features(rep, cn, reads, ids, min_lag, max_lag)
        for col, x in (('rep_auto', rep), ('rpm_auto', reads)):
            ok = ~np.isnan(orc[col].to_numpy())
            err = np.abs(got[col].to_numpy() - orc[col].to_numpy())[ok]
            assert np.all(err <= C.auto_bound(x)[np.argsort(ids, kind="stable")][ok]), (col, min_lag, max_lag)


def test_posterior_draws_phase_table_on_numpy_planes():
    from scdna_replication_tools_amd.posterior_draws import PosteriorDraws
    rep, cn, reads, ids, _ = C.case()
    L, N = rep.shape
    rng = np.random.default_rng(3)
    planes_rep = np.stack([rep, rep ^ (rng.random(rep.shape) < 0.02), rep ^ (rng.random(rep.shape) < 0.2)]).astype(np.uint8)
    planes_cn = np.stack([cn, cn, np.where(rng.random(cn.shape) < 0.1, 0, cn)]).astype(np.uint8)
    labels = dict(cell_ids=ids, chr=np.repeat('1', L), start=np.arange(L))
    d = PosteriorDraws(planes_rep, cn=planes_cn, reads=reads, device="cpu", **labels)
    t = d.phase_table()
    shares = t[['share_S', 'share_G1/2', 'share_LQ']].to_numpy()
    assert list(t['cell_id']) == list(ids) and np.allclose(shares.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    assert set(np.unique(np.round(shares * 3))) <= {0, 1, 2, 3}
    for col in ('rep_auto_mean', 'rep_auto_q5', 'rep_auto_q50', 'rep_auto_q95', 'cell_frac_rep_mean', 'rpm_auto'):
        assert col in t.columns
    # a single plane equal to the decode reproduces phase_calls
    one = PosteriorDraws(rep[None], cn=cn[None], reads=reads, device="cpu", **labels).phase_table().set_index('cell_id')
    calls = phase_calls(_matrix()).set_index('cell_id').loc[one.index]
    for name in ('S', 'G1/2', 'LQ'):
        assert np.array_equal(one['share_' + name].to_numpy() == 1.0, (calls['PERT_phase'] == name).to_numpy())
    for col, src in (('rep_auto_mean', 'rep_auto'), ('cell_frac_rep_mean', 'cell_frac_rep'), ('rpm_auto', 'rpm_auto')):
        assert np.array_equal(one[col].to_numpy(), calls[src].to_numpy(), equal_nan=True)
    with pytest.raises(ValueError):
        PosteriorDraws(planes_rep, cn=planes_cn, device="cpu", **labels).phase_table()       # no reads
    with pytest.raises(ValueError):
        PosteriorDraws(planes_rep, cn=planes_cn, reads=reads[:-1], device="cpu", **labels)


def test_pert_infer_scrt_validates_phase_calls():
    from scdna_replication_tools_amd.pert_model import pert_infer_scRT
    p = inspect.signature(pert_infer_scRT.__init__).parameters["phase_calls"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    rep, cn, reads, ids, _ = C.case()
    df = C.long_table(rep[:, :8], cn[:, :8], reads[:, :8], ids[:8])
    kw = dict(input_col='reads', clone_col=None, device='cpu')
    assert pert_infer_scRT(df, df, **kw).phase_calls is False
    m = pert_infer_scRT(df, df, phase_calls=True, **kw)
    assert m.phase_calls is True and m.phase_table is None
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError):
            pert_infer_scRT(df, df, phase_calls=bad, **kw)
