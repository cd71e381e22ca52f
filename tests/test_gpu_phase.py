"""pert_phase_counts / pert_phase_acf (csrc/phase_kernels.hip) against a numpy restatement, the
matrix layer on the device against the per-cell oracle, and pert_infer_scRT(phase_calls=True)."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from scdna_replication_tools_amd import _native as nat
from scdna_replication_tools_amd.phase_matrix import PhaseMatrix, host_counts, phase_calls
from tests import _phase_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E_ARG = 1

# (L, N, ldn, planes, max_lag).  At these sizes the kernels cut the bins into chunks of 128 (two
# 64-bin words, the least chunk); a chunk's halo is the word before it; pert_phase_acf sweeps 4 bins
# at a time.
SHAPES = [
    (51, 1, 256, 1, 50),       # the shortest legal series: lag 50 has one pair
    (130, 300, 512, 2, 50),    # tail masking (300 = 4 waves + 44 lanes), a second plane, a 2-bin last sweep
    (63, 70, 256, 1, 50),      # the 64-bin word edge - 1: one partial word
    (64, 70, 256, 1, 50),      # exactly one word
    (65, 70, 256, 2, 64),      # the word edge + 1, and the largest lag (the whole halo word)
    (127, 70, 256, 1, 50),     # chunk length - 1
    (128, 70, 256, 1, 50),     # exactly one chunk
    (129, 70, 256, 2, 64),     # chunk length + 1: a second chunk of one bin, all of its pairs in the halo
    (178, 70, 256, 1, 50),     # chunk + max_lag: the last pair of the second chunk reaches its first bin
    (192, 70, 256, 1, 50),     # chunk + halo word
    (193, 70, 256, 1, 50),     # chunk + halo word + 1
    (257, 70, 256, 2, 7),      # three chunks, a short lag window
]


def _inputs(L, N, planes, seed):
    rng = np.random.default_rng(seed)
    rep = (np.cumsum(rng.random((planes, L, N)) < 0.08, axis=1) % 2).astype(np.uint8)
    cn = (np.cumsum(rng.random((planes, L, N)) < 0.03, axis=1) % 5).astype(np.uint8)
    if N >= 3:
        rep[:, :, 0], rep[:, :, 1] = 1, 0
    return rep, cn, C.make_reads(rng, L, N, np.float64)


def _ref_counts(rep, cn, max_lag):
    """The integer outputs of one plane, restated: rep, cn (L, N)."""
    x = (rep != 0).astype(np.int64)
    L = x.shape[0]
    out = dict(T=x.sum(0), rep_bk=(x[1:] != x[:-1]).sum(0), cn_bk=(cn[1:] != cn[:-1]).sum(0), cn0=(cn == 0).sum(0))
    out["S"] = np.stack([(x[:L - k] * x[k:]).sum(0) for k in range(1, max_lag + 1)])
    out["head"] = np.stack([x[:k].sum(0) for k in range(1, max_lag + 1)])
    out["tail"] = np.stack([x[L - k:].sum(0) for k in range(1, max_lag + 1)])
    return out


def _ref_acf(x, max_lag):
    x = np.asarray(x, np.float64)
    L = x.shape[0]
    m = x.mean(axis=0)
    d = x - m
    return m, np.stack([(d[:L - k] * d[k:]).sum(0) for k in range(max_lag + 1)])


def _padded(a, ldn, fill, dtype):
    """a (..., L, N) on the device with rows ldn apart; the padding columns hold ``fill``."""
    buf = torch.full(a.shape[:-1] + (ldn,), fill, dtype=dtype, device=DEV)
    buf[..., :a.shape[-1]] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return buf


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _counts(rep_d, cn_d, L, N, ldn, planes, max_lag):
    pc = torch.zeros((4, planes, N), dtype=torch.int32, device=DEV)
    pl = torch.zeros((3, planes, max_lag, N), dtype=torch.int32, device=DEV)
    nat.check(nat.lib().pert_phase_counts(L, N, ldn, planes, L * ldn, rep_d.data_ptr(), cn_d.data_ptr(), max_lag,
                                          pc[0].data_ptr(), pc[1].data_ptr(), pc[2].data_ptr(), pc[3].data_ptr(),
                                          pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), _stream()),
              "pert_phase_counts")
    pc, pl = pc.cpu().numpy().astype(np.int64), pl.cpu().numpy().astype(np.int64)
    return dict(T=pc[0], rep_bk=pc[1], cn_bk=pc[2], cn0=pc[3], S=pl[0], head=pl[1], tail=pl[2])


def _acf(x_d, L, N, ldn, max_lag):
    need = ctypes.c_int64()
    nat.check(nat.lib().pert_phase_acf_workspace(L, N, max_lag, ctypes.byref(need)), "pert_phase_acf_workspace")
    ws = torch.full((need.value // 8,), float("nan"), dtype=torch.float64, device=DEV)    # need not be initialised
    mean = torch.empty(N, dtype=torch.float64, device=DEV)
    c = torch.empty((max_lag + 1, N), dtype=torch.float64, device=DEV)
    nat.check(nat.lib().pert_phase_acf(L, N, ldn, x_d.data_ptr(), int(x_d.dtype == torch.float64), max_lag,
                                       mean.data_ptr(), c.data_ptr(), ws.data_ptr(), need.value, _stream()),
              "pert_phase_acf")
    return mean.cpu().numpy(), c.cpu().numpy()


@pytest.mark.parametrize("L,N,ldn,planes,max_lag", SHAPES)
def test_counts_abi(L, N, ldn, planes, max_lag):
    rep, cn, _ = _inputs(L, N, planes, seed=L)
    rep_d, cn_d = _padded(rep, ldn, 0xFF, torch.uint8), _padded(cn, ldn, 0xFF, torch.uint8)
    got = _counts(rep_d, cn_d, L, N, ldn, planes, max_lag)
    for p in range(planes):
        want = _ref_counts(rep[p], cn[p], max_lag)
        for k, v in want.items():
            assert np.array_equal(got[k][p], v), (k, p)
    again = _counts(rep_d, cn_d, L, N, ldn, planes, max_lag)
    assert all(np.array_equal(got[k], again[k]) for k in got)
    # without cn the cn outputs are not touched (null pointers are accepted)
    pc = torch.zeros((2, planes, N), dtype=torch.int32, device=DEV)
    pl = torch.zeros((3, planes, max_lag, N), dtype=torch.int32, device=DEV)
    nat.check(nat.lib().pert_phase_counts(L, N, ldn, planes, L * ldn, rep_d.data_ptr(), None, max_lag, pc[0].data_ptr(),
                                          pc[1].data_ptr(), None, None, pl[0].data_ptr(), pl[1].data_ptr(),
                                          pl[2].data_ptr(), _stream()), "pert_phase_counts")
    assert np.array_equal(pc.cpu().numpy()[0], got["T"]) and np.array_equal(pl.cpu().numpy()[0], got["S"])


@pytest.mark.parametrize("is_f64", [0, 1])
@pytest.mark.parametrize("L,N,ldn,planes,max_lag", SHAPES)
def test_acf_abi(L, N, ldn, planes, max_lag, is_f64):
    _, _, reads = _inputs(L, N, 1, seed=L)
    x = reads if is_f64 else reads.astype(np.float32)
    x_d = _padded(x, ldn, float("nan"), torch.float64 if is_f64 else torch.float32)
    mean, c = _acf(x_d, L, N, ldn, max_lag)
    want_m, want_c = _ref_acf(x, max_lag)
    err_m, err_c = np.abs(mean - want_m), np.abs(c - want_c)
    print("mean: largest error {:.3e}; c: largest error / c_0 {:.3e}".format(err_m.max(), (err_c / want_c[0]).max()))
    assert np.all(err_m <= C.mean_bound(x)) and np.all(err_c <= C.c_bound(x)[None, :])
    mean2, c2 = _acf(x_d, L, N, ldn, max_lag)
    assert np.array_equal(mean, mean2) and np.array_equal(c, c2)                # bit for bit
    # a NaN, and an Inf, in one cell's series: that cell's outputs are NaN, the others' do not move
    for bad in (float("nan"), float("inf")):
        n_bad, t_bad = N // 2, L // 2
        y_d = x_d.clone()
        y_d[t_bad, n_bad] = bad
        mean3, c3 = _acf(y_d, L, N, ldn, max_lag)
        keep = np.arange(N) != n_bad
        assert np.isnan(mean3[n_bad]) and np.isnan(c3[:, n_bad]).all()
        assert np.array_equal(mean3[keep], mean[keep]) and np.array_equal(c3[:, keep], c[:, keep])


def test_argument_errors():
    L, N, ldn = 130, 70, 256
    rep, cn, reads = _inputs(L, N, 1, seed=1)
    rep_d, cn_d = _padded(rep, ldn, 0xFF, torch.uint8), _padded(cn, ldn, 0xFF, torch.uint8)
    x_d = _padded(reads, ldn, float("nan"), torch.float64)
    out = torch.zeros((8, 64 * N), dtype=torch.int32, device=DEV)
    o = [out[i].data_ptr() for i in range(7)]
    ws = torch.zeros(1 << 16, dtype=torch.float64, device=DEV)
    fo = torch.zeros((66, N), dtype=torch.float64, device=DEV)
    lib = nat.lib()

    def counts(L=L, ldn=ldn, max_lag=50, rep=rep_d.data_ptr(), outs=o):
        return lib.pert_phase_counts(L, N, ldn, 1, 0, rep, cn_d.data_ptr(), max_lag, *outs, _stream())

    def acf(L=L, ldn=ldn, max_lag=50, x=x_d.data_ptr(), mean=fo[0].data_ptr(), ws_bytes=ws.numel() * 8):
        return lib.pert_phase_acf(L, N, ldn, x, 1, max_lag, mean, fo[1:].data_ptr(), ws.data_ptr(), ws_bytes, _stream())

    assert counts() == 0 and acf() == 0
    for f in (counts, acf):
        assert f(L=50) == E_ARG                       # L = max_lag
        assert f(max_lag=65) == E_ARG and f(max_lag=0) == E_ARG
        assert f(ldn=ldn + 8) == E_ARG                # not a multiple of 16
        assert f(L=1 << 20) == E_ARG
    assert counts(rep=rep_d.data_ptr() + 4) == E_ARG and acf(x=x_d.data_ptr() + 8) == E_ARG
    assert counts(rep=None) == E_ARG and acf(x=None) == E_ARG
    for i in (0, 1, 4, 5, 6, 2, 3):                   # each output null in turn (cn's: cn is given)
        assert counts(outs=[None if j == i else p for j, p in enumerate(o)]) == E_ARG
    assert acf(mean=None) == E_ARG and acf(ws_bytes=8) == E_ARG
    need = ctypes.c_int64()
    assert lib.pert_phase_acf_workspace(L, N, 50, None) == E_ARG
    assert lib.pert_phase_acf_workspace(50, N, 50, ctypes.byref(need)) == E_ARG
    torch.cuda.synchronize()


def test_phase_matrix_over_strided_device_tensors_in_place():
    rep, cn, reads, ids, orc = C.case()
    L, N = rep.shape
    rep_d, cn_d = _padded(rep, 256, 0xFF, torch.uint8), _padded(cn, 256, 0xFF, torch.uint8)
    x_d = _padded(reads, 256, float("nan"), torch.float32)
    pm = PhaseMatrix(rep_d[:, :N], cn_d[:, :N], x_d[:, :N], ids)
    assert pm.device.type == "cuda" and pm.ldn == 256
    assert (pm._rep.data_ptr(), pm._cn.data_ptr(), pm._reads.data_ptr()) == (rep_d.data_ptr(), cn_d.data_ptr(),
                                                                            x_d.data_ptr())
    want = host_counts(rep, cn, pm.max_lag)
    got = pm.raw()["counts"]
    assert all(np.array_equal(got[k], want[k]) for k in want)
    C.assert_features(pm.features(), rep, cn, reads, ids, orc)
    host = phase_calls(PhaseMatrix(rep, cn, reads, ids, device="cpu"))
    dev = phase_calls(pm)
    assert list(dev['PERT_phase']) == list(host['PERT_phase']) == list(C.oracle_phase(orc))
    # numpy inputs are uploaded; float64 reads take the double kernel
    up = PhaseMatrix(rep, cn, reads.astype(np.float64), ids, device=DEV)
    C.assert_features(up.features(), rep, cn, reads, ids, orc)


def test_an_indexless_cuda_device_keeps_the_callers_buffers():
    """device='cuda' (what pert_infer_scRT passes without a process group) names the current
    device: tensors that live there are used in place, not copied, by every entry of the layer."""
    from scdna_replication_tools_amd import phase_matrix as PM
    rep, cn, reads, ids, _ = C.case()
    L, N = rep.shape
    rep_d, cn_d = _padded(rep, 256, 0xFF, torch.uint8), _padded(cn, 256, 0xFF, torch.uint8)
    x_d = _padded(reads, 256, float("nan"), torch.float32)
    assert PM.pick_device("cuda") == rep_d.device == PM.pick_device(None, rep, x_d)
    for device in ("cuda", torch.device("cuda"), DEV):
        pm = PhaseMatrix(rep_d[:, :N], cn_d[:, :N], x_d[:, :N], ids, device=device)
        assert (pm._rep.data_ptr(), pm._cn.data_ptr(), pm._reads.data_ptr()) == (
            rep_d.data_ptr(), cn_d.data_ptr(), x_d.data_ptr())
    dev = PM.pick_device("cuda")
    planes = torch.stack([rep_d, rep_d])[:, :, :N]
    assert PM.device_planes(planes, dev)[0].data_ptr() == planes.data_ptr()
    assert PM.device_matrix(x_d[:, :N], dev, torch.float32)[0].data_ptr() == x_d.data_ptr()
    want = PhaseMatrix(rep, cn, reads, ids, device="cpu").features()
    assert np.array_equal(PM.reads_auto(x_d[:, :N], device="cuda"), PM.reads_auto(x_d[:, :N]))
    got = PM.counts_of_planes(planes, torch.stack([cn_d, cn_d])[:, :, :N], device="cuda")
    assert np.array_equal(got["T"][1] / float(L), want.set_index('cell_id').loc[ids, 'cell_frac_rep'].to_numpy())


def _matrices(frame):
    """(rep, cn, reads, cell ids) of a returned frame: each cell's rows in table order."""
    d = frame.sort_values('cell_id', kind="stable")
    ids = d['cell_id'].unique()
    N = len(ids)
    mat = lambda col, dt: np.ascontiguousarray(d[col].to_numpy().reshape(N, len(d) // N).T.astype(dt))
    return mat('model_rep_state', np.uint8), mat('model_cn_state', np.uint8), mat('reads', np.float64), ids


def test_pipeline_phase_calls():
    """pert_infer_scRT(phase_calls=True, posterior_draws=4): the returned frames are those of a run
    without the keyword; phase_table equals predict_cycle_phase on them, cell for cell."""
    from scdna_replication_tools_amd.pert_model import pert_infer_scRT
    from scdna_replication_tools_amd.predict_cycle_phase import predict_cycle_phase
    from scdna_replication_tools_amd.simulator import simulate, to_long_form
    sim = simulate(n_s=40, n_g=40, n_bins=300, num_reads=183 * 300, seed=2)
    kw = dict(input_col='reads', clone_col='clone_id', cn_prior_method='g1_clones', max_iter=300, min_iter=50,
              rel_tol=1e-6, max_iter_step1=200, max_iter_step3=100)
    runs, in_place = [], []
    real = pert_infer_scRT._phase_matrix

    def watched(self, shard, cell_ids):
        # the matrices are dropped once the features are computed: look while they are alive
        from scdna_replication_tools_amd import phase_matrix as PM
        made = PM.PhaseMatrix(shard.rep_out[:, :shard.N], shard.cn_out[:, :shard.N], shard.reads[:, :shard.N],
                              cell_ids, device=self.device)
        in_place.append((made._rep.data_ptr(), made._cn.data_ptr(), made._reads.data_ptr()) ==
                        (shard.rep_out.data_ptr(), shard.cn_out.data_ptr(), shard.reads.data_ptr()))
        return real(self, shard, cell_ids)

    for extra in (dict(), dict(phase_calls=True, posterior_draws=4)):
        df_s, df_g = to_long_form(sim, n_libs=1)
        m = pert_infer_scRT(df_s, df_g, **kw, **extra)
        m._phase_matrix = watched.__get__(m)
        runs.append((m, m.run_pert_model()))
    assert in_place == [True, True]            # step 2's and step 3's decode and reads, not copies
    (m0, out0), (m, out) = runs
    assert m0.phase_table is None
    for a, b in zip(out0, out):
        pd.testing.assert_frame_equal(a, b)
    cn_s_out, _, cn_g1_out, _ = out
    table = m.phase_table
    assert list(table['fitted_as']) == ['S'] * 40 + ['G1/2'] * 40

    parts = [_matrices(cn_s_out), _matrices(cn_g1_out)]
    orcs = [C.oracle_features(*p) for p in parts]
    orc = pd.concat(orcs, ignore_index=True)
    ra, fr, f0 = (orc[c].to_numpy() for c in ('rep_auto', 'cell_frac_rep', 'frac_cn0'))
    margin = min(np.nanmin(np.abs(ra - C.REP_AUTO_THRESH)), np.abs(fr - C.FRAC_THRESH).min(),
                 np.abs(fr - (1 - C.FRAC_THRESH)).min(), np.abs(f0 - C.FRAC_CN0_THRESH).min())
    assert margin > C.MARGIN, "this fit has a cell on a threshold: pick another simulation seed"

    cn = pd.concat([cn_s_out, cn_g1_out], ignore_index=True)
    cn["rpm"] = cn["reads"] / cn.groupby("cell_id")["reads"].transform("sum") * 1e6
    s_, g_, lq_ = predict_cycle_phase(cn, device="cpu")
    ref = pd.concat([s_, g_, lq_]).drop_duplicates("cell_id").set_index("cell_id")["PERT_phase"]
    assert list(table['PERT_phase']) == list(ref.loc[table['cell_id']])
    for (rep, cnm, reads, ids), o, name in zip(parts, orcs, ('S', 'G1/2')):
        got = table.loc[table['fitted_as'] == name, list(o.columns)].reset_index(drop=True)
        C.assert_features(got, rep, cnm, reads, ids, o)
    for col in ('rpm_auto', 'rep_auto'):
        assert np.array_equal(table[col + '_norm'].to_numpy(), (table[col] - np.mean(table[col].values)).to_numpy(),
                              equal_nan=True)

    draws = m.draws_s.phase_table()
    assert len(draws) == 40 and sorted(draws['cell_id']) == sorted(parts[0][3])
    shares = draws[['share_S', 'share_G1/2', 'share_LQ']].to_numpy()
    assert np.allclose(shares.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    s_rows = table[table['fitted_as'] == 'S'].set_index('cell_id').loc[draws['cell_id']]
    assert np.array_equal(draws['rpm_auto'].to_numpy(), s_rows['rpm_auto'].to_numpy(), equal_nan=True)
