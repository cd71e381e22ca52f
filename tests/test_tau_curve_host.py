"""The likelihood curve over tau without a GPU: the per-element arithmetic (pert_math.h
enum_evidence / tau_mix, compiled for the host) against the fp64 oracle within the derived bounds
of tests/_curve_bounds.py, TauCurve.table on hand-made curves with exact expected values, the grid
validation, and the argument checks of the two C entry points.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _curve_bounds as cb
from tests._problems import make_problem

EPS32 = cb.EPS32


@pytest.fixture(scope="module")
def nat():
    from scdna_replication_tools_amd import build, _native
    build.build()
    _native.lib()
    return _native


def _element_inputs(prob, z):
    """x, logits, D of every (bin, cell) of an oracle problem, flattened over (L, N): D = u omega
    (1 - lam) / lam in fp64, rounded once to fp32 (a relative eps32 of delta, which the score
    error's delta dpsi term covers eight times over)."""
    from oracle import pert_oracle as po
    with torch.no_grad():
        c = po.constrain(prob.kind, z)
        L, N = prob.reads.shape
        gcf = po.gc_features(prob.gc, prob.K).reshape(L, 1, prob.K + 1)
        omega = torch.exp(torch.sum(torch.mul(c["expose_betas"], gcf), 2))
        D = c["expose_u"] * omega * (1 - prob.lamb) / prob.lamb
    return (prob.reads.numpy().reshape(-1), z["expose_pi"].numpy().reshape(L * N, prob.P), D.numpy().reshape(-1),
            float(torch.log1p(-prob.lamb)))


@pytest.mark.parametrize("P,low", [(2, False), (7, True), (13, False), (13, True), (16, True)])
def test_enum_evidence_host_within_element_bound_of_oracle(nat, P, low):
    prob, _, z = make_problem("step2", L=12, N=9, P=P, K=2 if P == 2 else 4, seed=20 + P, low_reads=low)
    ref = cb.oracle_evidence(prob, z)
    x, zl, D, l1m = _element_inputs(prob, z)
    ev0, ev1 = nat.selftest_enum_evidence_host(P, x, zl, l1m, D)
    shape = ref["e"][0].shape
    worst = 0.0
    for r, dev in enumerate((ev0, ev1)):
        d = np.abs(dev.astype(np.float64).reshape(shape) - ref["e"][r])
        assert np.isfinite(dev).all()
        ratio = d / ref["B"][r]
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (r, float(ratio.max()))
    print("P={} low={}: worst |delta e| / bound {:.3f}; median bound {:.3g}, median |e| {:.3g}".format(
        P, low, worst, float(np.median(ref["B"])), float(np.median(np.abs(ref["e"])))))
    # the check has power: the bound is far below the separation of the two branches
    assert np.median(ref["B"]) < 1e-2 * np.median(np.abs(ref["e"][1] - ref["e"][0]))


def test_tau_mix_host_matches_fp64_logaddexp(nat):
    """m within 6 eps32 (1 + |m|) of the fp64 logaddexp at phi clamped as the model clamps it:
    random points, differences of +-300, phi at and beyond both clamps, evidences near 2,000."""
    rng = np.random.default_rng(7)
    n = 400
    e0 = rng.uniform(-300, 50, n).astype(np.float32)
    e1 = (e0 + rng.normal(size=n).astype(np.float32) * 8).astype(np.float32)
    phi = rng.uniform(0.0005, 0.9995, n).astype(np.float32)
    e1[0:20] = e0[0:20] + 300
    e1[20:40] = e0[20:40] - 300
    phi[40:50] = np.float32(0.001)
    phi[50:60] = np.float32(0.999)
    phi[60:70] = rng.uniform(0, 0.001, 10).astype(np.float32)
    phi[70:80] = rng.uniform(0.999, 1.0, 10).astype(np.float32)
    phi[80], phi[81] = 0.0, 1.0
    e0[90:110] = rng.uniform(1990, 2010, 20).astype(np.float32)
    e1[90:110] = e0[90:110] + rng.normal(size=20).astype(np.float32) * 3
    e0[110:120] = -e0[90:100]
    e1[110:120] = e0[110:120] + 300
    e1[120:130] = e0[120:130]                                   # equal branches
    m = nat.selftest_tau_mix_host(e0, e1, phi).astype(np.float64)
    phic = np.clip(phi, np.float32(0.001), np.float32(0.999)).astype(np.float64)
    ref, _ = cb.mix(e0.astype(np.float64), e1.astype(np.float64), phic)
    assert np.isfinite(m).all()
    ratio = np.abs(m - ref) / (6 * EPS32 * (1 + np.abs(ref)))
    print("tau_mix: worst |delta m| / (6 eps32 (1 + |m|)) = {:.3f}".format(float(ratio.max())))
    assert (ratio <= 1.0).all(), (int(ratio.argmax()), float(ratio.max()))


def _curve(grid, cols, fit, tau=None):
    from scdna_replication_tools_amd.tau_curve import TauCurve
    ll = np.asarray(cols, np.float64).T                         # (G, N)
    N = ll.shape[1]
    return TauCurve(np.asarray(grid, np.float32), ll, np.asarray(fit, np.float64),
                    np.full(N, 0.5, np.float32) if tau is None else np.asarray(tau, np.float32))


GRID7 = [0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875]           # exact in fp32


def _row(t, i=0):
    return {k: t[k].iloc[i] for k in t.columns}


def test_table_unimodal():
    t = _curve(GRID7, [[-10, -3, -1, 0, -1.5, -4, -9]], [-0.25], tau=[0.46875]).table()
    r = _row(t)
    assert list(t.columns) == ["model_tau", "curve_at_fit", "curve_tau", "curve_gain", "tau_lo", "tau_hi", "n_modes",
                               "alt_tau", "alt_drop"]
    assert r["model_tau"] == np.float32(0.46875) and r["curve_at_fit"] == -0.25
    assert r["curve_tau"] == 0.5 and r["curve_gain"] == 0.25
    assert r["tau_lo"] == 0.375 and r["tau_hi"] == 0.625 and r["n_modes"] == 1      # S = {-1, 0, -1.5}
    assert np.isnan(r["alt_tau"]) and np.isnan(r["alt_drop"])


def test_table_two_separated_modes():
    t = _curve(GRID7, [[0, -1, -5, -6, -5, -1.5, -0.5]], [-0.125]).table(cell_ids=["c0"])
    r = _row(t)
    assert list(t.columns)[0] == "cell_id" and r["cell_id"] == "c0"
    assert r["curve_tau"] == 0.125 and r["curve_gain"] == 0.125
    assert r["tau_lo"] == 0.125 and r["tau_hi"] == 0.875 and r["n_modes"] == 2      # S = {0,1} u {5,6}
    assert r["alt_tau"] == 0.875 and r["alt_drop"] == 0.5
    # a tighter cut splits off nothing new but drops the second basin
    r = _row(_curve(GRID7, [[0, -1, -5, -6, -5, -1.5, -0.5]], [-0.125]).table(drop=0.25))
    assert r["n_modes"] == 1 and r["tau_lo"] == 0.125 and r["tau_hi"] == 0.125 and np.isnan(r["alt_tau"])


def test_table_plateau_tie():
    """Equal maxima: curve_tau is the first; the second, in another run, is the alternative at
    drop 0 from the best."""
    r = _row(_curve(GRID7, [[-4, 0, 0, -3, 0, -4, -5]], [-1.0]).table())
    assert r["curve_tau"] == 0.25 and r["curve_gain"] == 1.0
    assert r["tau_lo"] == 0.25 and r["tau_hi"] == 0.625 and r["n_modes"] == 2       # S = {1,2} u {4}
    assert r["alt_tau"] == 0.625 and r["alt_drop"] == 0.0


def test_table_empty_set():
    """The fitted tau beats every grid point by more than the drop: S is empty."""
    r = _row(_curve(GRID7, [[-9, -8, -5, -4, -5, -8, -9]], [0.0]).table())
    assert r["curve_tau"] == 0.5 and r["curve_gain"] == -4.0 and r["n_modes"] == 0
    assert all(np.isnan(r[k]) for k in ("tau_lo", "tau_hi", "alt_tau", "alt_drop"))


def test_table_fit_better_than_every_grid_point():
    """l* is the fit's value: the cut is taken from it, not from the best grid point."""
    r = _row(_curve(GRID7, [[-9, -3, -1.5, -1, -2, -3, -9]], [0.0]).table())
    assert r["curve_tau"] == 0.5 and r["curve_gain"] == -1.0
    assert r["tau_lo"] == 0.375 and r["tau_hi"] == 0.5 and r["n_modes"] == 1        # S = {-1.5, -1}: -2 < -1.92
    assert np.isnan(r["alt_tau"]) and np.isnan(r["alt_drop"])


def test_table_single_grid_point_and_several_cells():
    t = _curve([0.5], [[-2.0], [-7.0]], [-2.5, -1.0]).table()
    a, b = _row(t, 0), _row(t, 1)
    assert a["curve_tau"] == 0.5 and a["curve_gain"] == 0.5 and a["tau_lo"] == 0.5 and a["tau_hi"] == 0.5
    assert a["n_modes"] == 1 and np.isnan(a["alt_tau"])
    assert b["curve_gain"] == -6.0 and b["n_modes"] == 0 and np.isnan(b["tau_lo"])
    assert t["n_modes"].dtype == np.int64 and len(t) == 2


def test_grid_validation():
    from scdna_replication_tools_amd.tau_curve import DEFAULT_GRID, validate_grid
    g = validate_grid(None)
    assert g.dtype == np.float32 and g.shape == (99,) and np.array_equal(g, np.linspace(0.01, 0.99, 99).astype(np.float32))
    assert np.array_equal(g, DEFAULT_GRID)
    assert validate_grid([0.25]).shape == (1,)
    for bad in ([], [0.5, 0.25], [0.25, 0.25], [0.0, 0.5], [0.5, 1.0], [0.5, np.nan], [[0.2, 0.4]],
                np.linspace(0.01, 0.99, 1025), [0.5, 0.5 + 1e-9]):       # (the last: equal after the cast)
        with pytest.raises(ValueError):
            validate_grid(bad)


def _problem(nat, **kw):
    d = dict(kind=2, L=10, N=10, P=13, K1=5, n_libs=1, ldn=256)
    d.update(kw)
    return nat.PertProblem(**d)


def test_abi_and_argument_checks(nat):
    """The four names are exported, and every argument error returns before any launch (no GPU
    here): the pointers below are host buffers that are never dereferenced."""
    names = {"pert_enum_evidence", "pert_tau_curve", "pert_selftest_enum_evidence_host", "pert_selftest_tau_mix_host"}
    assert names <= set(nat.EXPORTED_SYMBOLS)
    lib = nat.lib()
    assert nat.TAU_MAX_GRID == 1024
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    st = nat.PertState(params=p, z_pi=p)
    good = dict(reads=p, gcf=p)
    E_ARG, E_P, E_K = 1, 2, 3
    ev = lambda pr, out=p, s=st: lib.pert_enum_evidence(ctypes.byref(pr), ctypes.byref(s), out, None)
    assert ev(_problem(nat, **good), None) == E_ARG                            # null ev
    assert lib.pert_enum_evidence(None, ctypes.byref(st), p, None) == E_ARG
    assert lib.pert_enum_evidence(ctypes.byref(_problem(nat, **good)), None, p, None) == E_ARG
    assert ev(_problem(nat, kind=1, **good)) == E_ARG                          # step 1
    assert ev(_problem(nat, P=17, **good)) == E_P
    assert ev(_problem(nat, P=1, **good)) == E_P
    assert ev(_problem(nat, K1=9, **good)) == E_K
    assert ev(_problem(nat, L=0, **good)) == E_ARG
    assert ev(_problem(nat, ldn=100, **good)) == E_ARG                         # not a multiple of PERT_BLOCK
    assert ev(_problem(nat, N=300, **good)) == E_ARG                           # ldn < N
    assert ev(_problem(nat, N=0, **good)) == E_ARG
    assert ev(_problem(nat)) == E_ARG                                          # null reads / gcf
    assert ev(_problem(nat, **good), s=nat.PertState(params=p)) == E_ARG       # null z_pi
    assert ev(_problem(nat, kind=3, **good)) == E_ARG                          # step 3 without rho_fixed
    assert ev(_problem(nat, P=17, L=0, **good)) == E_ARG                       # the order: shape before P

    def tc(pr, e=p, g=p, G=5, c=p, a=p, s=st):
        return lib.pert_tau_curve(ctypes.byref(pr), ctypes.byref(s), e, g, G, c, a, None)
    ok = _problem(nat, **good)
    for k in ("e", "g", "c", "a"):
        assert tc(ok, **{k: None}) == E_ARG                                    # each null buffer
    assert lib.pert_tau_curve(None, ctypes.byref(st), p, p, 5, p, p, None) == E_ARG
    assert lib.pert_tau_curve(ctypes.byref(ok), None, p, p, 5, p, p, None) == E_ARG
    assert tc(_problem(nat, kind=1, **good)) == E_ARG
    assert tc(ok, G=0) == E_ARG and tc(ok, G=-1) == E_ARG and tc(ok, G=1025) == E_ARG
    assert tc(_problem(nat, L=0, **good)) == E_ARG
    assert tc(_problem(nat, N=0, **good)) == E_ARG
    assert tc(_problem(nat, N=300, **good)) == E_ARG
    assert tc(_problem(nat, ldn=100, **good)) == E_ARG
    assert tc(ok, s=nat.PertState(z_pi=p)) == E_ARG                            # null params
    assert tc(_problem(nat, kind=3, **good)) == E_ARG                          # step 3 without rho_fixed
    assert lib.pert_selftest_enum_evidence_host(17, 0, None, None, 0.0, None, None, None) == E_P
    assert lib.pert_selftest_enum_evidence_host(13, 1, None, None, 0.0, None, None, None) == E_ARG
    assert lib.pert_selftest_tau_mix_host(1, None, None, None, None) == E_ARG
    assert lib.pert_selftest_tau_mix_host(0, None, None, None, None) == 0


def test_model_argument_and_process_group_guard():
    """tau_curve=False keeps the model as it was; True / a grid is validated at construction."""
    import pandas as pd
    from scdna_replication_tools_amd.pert_model import pert_infer_scRT
    df = pd.DataFrame({})
    assert pert_infer_scRT(df, df, device="cpu").tau_grid is None
    m = pert_infer_scRT(df, df, device="cpu", tau_curve=True)
    assert m.tau_grid.shape == (99,) and m.tau_curve_s is None and m.tau_table_g is None
    assert np.array_equal(pert_infer_scRT(df, df, device="cpu", tau_curve=[0.25, 0.5]).tau_grid,
                          np.array([0.25, 0.5], np.float32))
    with pytest.raises(ValueError):
        pert_infer_scRT(df, df, device="cpu", tau_curve=[0.5, 0.25])
