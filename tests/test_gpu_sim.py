"""The read-count simulator on the GPU: the generator against known answers and an independent
numpy Philox, the counter rule (geometry, sharding), and the samplers' distributions against
scipy with derived thresholds.  Pyro is not a dependency, so parity with the reference's own
simulator is distributional and structural (tests/_sim_ref.py holds the numpy side)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _sim_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
PERT_E_ARG = 1


@pytest.fixture(scope="module")
def nat():
    from scdna_replication_tools_amd import _native
    _native.lib()
    return _native


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a, dtype), device=DEV)


def sim_raw(nat, counter, key, n):
    out = torch.zeros((n, 4), dtype=torch.int32, device=DEV)
    nat.check(nat.lib().pert_sim_raw(key[0], key[1], *counter, n, out.data_ptr(), stream()), "pert_sim_raw")
    return out.cpu().numpy().view(np.uint32)


def sim_cells(nat, libs, means, stds, seed, cell0=0, want_tau=True):
    N, (n_libs, K1) = len(libs), means.shape
    tau = torch.full((N,), -1.0, dtype=torch.float32, device=DEV) if want_tau else None
    betas = torch.full((K1, N), np.nan, dtype=torch.float32, device=DEV)
    libs_d, means_d, stds_d = dev(libs, np.int32), dev(means, np.float32), dev(stds, np.float32)   # alive over the call
    nat.check(nat.lib().pert_sim_cells(N, K1, n_libs, cell0, ctypes.c_uint64(seed), libs_d.data_ptr(),
                                       means_d.data_ptr(), stds_d.data_ptr(), tau.data_ptr() if want_tau else 0,
                                       betas.data_ptr(), stream()), "pert_sim_cells")
    torch.cuda.synchronize()
    return (tau.cpu().numpy() if want_tau else None), betas.cpu().numpy()


def sim_reads(nat, cn, gc, betas, u, lamb, seed, rho=None, tau=None, a=0.0, cell0=0, want_p=True, expect=0):
    """pert_sim_reads through the C ABI.  Outputs are pre-filled with junk so the padding columns
    show whether the kernel wrote them."""
    L, N = cn.shape
    ldn = -(-N // 256) * 256
    cn_d = torch.zeros((L, ldn), dtype=torch.float32, device=DEV)
    cn_d[:, :N] = dev(cn, np.float32)
    counts = torch.full((L, ldn), -7, dtype=torch.int32, device=DEV)
    rep = torch.full((L, ldn), 9, dtype=torch.uint8, device=DEV)
    p_rep = torch.full((L, ldn), -3.0, dtype=torch.float32, device=DEV) if want_p else None
    colsum = torch.zeros(N, dtype=torch.int64, device=DEV)
    exhausted = torch.zeros(1, dtype=torch.int32, device=DEV)
    gc_d, betas_d = dev(gc, np.float32), dev(betas, np.float32)
    rho_d = dev(rho, np.float32) if rho is not None else None
    tau_d = dev(tau, np.float32) if tau is not None else None
    code = nat.lib().pert_sim_reads(L, N, ldn, betas.shape[0], cell0, ctypes.c_uint64(seed), cn_d.data_ptr(),
                                    gc_d.data_ptr(), rho_d.data_ptr() if rho is not None else 0,
                                    tau_d.data_ptr() if tau is not None else 0, betas_d.data_ptr(), float(u), float(a),
                                    float(lamb), counts.data_ptr(), rep.data_ptr(),
                                    p_rep.data_ptr() if want_p else 0, colsum.data_ptr(), exhausted.data_ptr(), stream())
    assert code == expect
    torch.cuda.synchronize()
    return dict(L=L, N=N, ldn=ldn, counts_d=counts, colsum_d=colsum, counts=counts.cpu().numpy().view(np.uint32),
                rep=rep.cpu().numpy(), p_rep=p_rep.cpu().numpy() if want_p else None,
                colsum=colsum.cpu().numpy(), exhausted=int(exhausted.item()))


# ---------------------------------------------------------------------------- 1. generator

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
          "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,words", KNOWN)
def test_generator_known_answers(nat, counter, key, words):
    want = np.array([int(w, 16) for w in words.split()], np.uint32)
    np.testing.assert_array_equal(R.philox(np.array(counter, np.uint32), key), want)      # the numpy side itself
    np.testing.assert_array_equal(sim_raw(nat, counter, key, 1)[0], want)


def test_generator_consecutive_counters(nat):
    start, key, n = (0xFFFFFE00, 0xFFFFFFFF, 7, 1), (0x12345678, 0x9ABCDEF0), 1024     # the low word carries
    value = sum(w << (32 * i) for i, w in enumerate(start)) + np.arange(n, dtype=object)
    ctr = np.array([[(int(v) >> (32 * i)) & 0xFFFFFFFF for i in range(4)] for v in value], np.uint32)
    assert ctr[-1, 1] == 0 and ctr[-1, 2] == 8
    np.testing.assert_array_equal(sim_raw(nat, start, key, n), R.philox(ctr, key))


# ---------------------------------------------------------------------------- 2. per-cell draws

def test_cell_draws(nat):
    N, seed, cell0 = 300, 0x1234567890ABCDEF, 5
    libs = (np.arange(N) * 7 % 2).astype(np.int32)
    means = np.array([[0.5, 0.0], [0.7, 0.1]], np.float32)
    stds = np.array([[1.0, 0.1], [0.5, 0.2]], np.float32)
    tau, betas = sim_cells(nat, libs, means, stds, seed, cell0=cell0)
    want_tau, want_betas = R.cell_draws(seed, cell0, libs, means, stds)
    np.testing.assert_array_equal(tau, want_tau)
    assert (tau > 0).all() and (tau < 1).all()
    np.testing.assert_allclose(betas, want_betas, rtol=1e-5, atol=0)
    _, fixed = sim_cells(nat, libs, means, np.zeros_like(stds), seed, want_tau=False)     # zero spread: the means
    np.testing.assert_array_equal(fixed, means[libs].T)


# ---------------------------------------------------------------------------- 3 / 4. geometry, Bernoulli

class Shape37x300:
    L, N, K1, seed, a, lamb, u = 37, 300, 2, 20240611, 10.0, 0.75, 40.0


@pytest.fixture(scope="module")
def s_case(nat):
    c = Shape37x300
    rng = np.random.default_rng(5)
    cn = rng.choice([1.0, 2.0, 3.0, 5.0], size=(c.L, c.N))
    gc = rng.uniform(0.3, 0.65, c.L).astype(np.float32)
    rho = rng.uniform(0, 1, c.L).astype(np.float32)
    libs = (np.arange(c.N) % 2).astype(np.int32)
    means = np.array([[0.5, 0.0]] * 2, np.float32)
    stds = np.array([[1.0, 0.1]] * 2, np.float32)
    tau, betas = sim_cells(nat, libs, means, stds, c.seed)
    args = dict(cn=cn, gc=gc, rho=rho, libs=libs, means=means, stds=stds, tau=tau, betas=betas)
    run = lambda seed: sim_reads(nat, cn, gc, betas, c.u, c.lamb, seed, rho=rho, tau=tau, a=c.a)
    return args, run(c.seed), run


def test_geometry_and_sharding(nat, s_case):
    c = Shape37x300
    args, one, run = s_case
    assert one["ldn"] == 512 and one["exhausted"] == 0
    again = run(c.seed)
    for k in ("counts", "rep", "p_rep", "colsum"):
        np.testing.assert_array_equal(again[k], one[k])
    for k in ("counts", "rep", "p_rep"):
        assert (one[k][:, c.N:] == 0).all()                                   # padding columns written as zero
    np.testing.assert_array_equal(one["colsum"], one["counts"][:, :c.N].astype(np.int64).sum(0))
    for lo, hi in ((0, 130), (130, c.N)):
        tau, betas = sim_cells(nat, args["libs"][lo:hi], args["means"], args["stds"], c.seed, cell0=lo)
        np.testing.assert_array_equal(tau, args["tau"][lo:hi])
        np.testing.assert_array_equal(betas, args["betas"][:, lo:hi])
        part = sim_reads(nat, args["cn"][:, lo:hi], args["gc"], betas, c.u, c.lamb, c.seed, rho=args["rho"], tau=tau,
                         a=c.a, cell0=lo)
        assert part["ldn"] == 256 and part["exhausted"] == 0
        for k in ("counts", "rep", "p_rep"):
            np.testing.assert_array_equal(part[k][:, :hi - lo], one[k][:, lo:hi])
            assert (part[k][:, hi - lo:] == 0).all()
        np.testing.assert_array_equal(part["colsum"], one["colsum"][lo:hi])
    other = run(c.seed + 1)
    assert (other["counts"][:, :c.N] != one["counts"][:, :c.N]).mean() > 0.9
    no_p = sim_reads(nat, args["cn"], args["gc"], args["betas"], c.u, c.lamb, c.seed, rho=args["rho"],
                     tau=args["tau"], a=c.a, want_p=False)
    np.testing.assert_array_equal(no_p["counts"], one["counts"])


def test_bernoulli(nat, s_case):
    c = Shape37x300
    args, one, _ = s_case
    phi = 1.0 / (1.0 + np.exp(-c.a * (args["tau"].astype(np.float64)[None, :] - args["rho"].astype(np.float64)[:, None])))
    w = R.draw(c.seed, R.TAG_READS, np.arange(c.L)[:, None], np.arange(c.N)[None, :], 0)
    u = R.uniform32(w[..., 0]).astype(np.float64)
    rep = one["rep"][:, :c.N]
    assert set(np.unique(rep)) <= {0, 1}
    differ = rep != (u < phi)
    print("bernoulli: {} of {} differ, max |u - phi| there {}".format(
        differ.sum(), differ.size, np.abs(u - phi)[differ].max() if differ.any() else 0.0))
    assert (np.abs(u - phi)[differ] <= 1e-6).all()
    assert differ.sum() <= 2
    np.testing.assert_allclose(one["p_rep"][:, :c.N], phi, atol=1e-6, rtol=0)
    g = sim_reads(nat, args["cn"], args["gc"], args["betas"], c.u, c.lamb, c.seed)           # G1/2 mode
    assert (g["rep"] == 0).all() and (g["p_rep"] == 0).all() and g["exhausted"] == 0


# ---------------------------------------------------------------------------- 5. negative binomial

NB_CASES = [(1.0, 0.75), (2.5, 0.75), (9.0, 0.75), (11.0, 0.75), (61.0, 0.75), (400.0, 0.75), (5000.0, 0.75),
            (61.0, 0.3), (61.0, 0.95)]


@pytest.mark.parametrize("delta,lamb", NB_CASES)
def test_negative_binomial_distribution(nat, delta, lamb):
    """65,536 draws at one delta (G1/2 mode, constant cn, zero betas) against scipy's nbinom.
    Thresholds: chi-square at its 1 - 1e-6 quantile; mean and variance within 5 standard errors
    (the variance's from the fourth central moment).  Power: the same sample against delta * 1.03
    must fail the chi-square wherever delta >= 9."""
    L, N = 64, 1024
    cn_value = 0.0 if delta == 1.0 else 2.0                       # cn 0: theta 0, the clamp gives delta 1
    u = delta * lamb / ((1.0 - lamb) * 2.0)
    out = sim_reads(nat, np.full((L, N), cn_value), np.full(L, 0.45), np.zeros((2, N)), u, lamb, seed=int(delta * 100))
    x = out["counts"][:, :N].astype(np.float64).reshape(-1)
    assert out["exhausted"] == 0
    stat, df, smallest = R.nb_chi2(x, delta, lamb)
    threshold = R.chi2_threshold(df)
    mean, var, m4 = R.nb_moments(delta, lamb)
    n = x.size
    z_mean = (x.mean() - mean) / np.sqrt(var / n)
    z_var = (x.var(ddof=1) - var) / np.sqrt((m4 - var ** 2 * (n - 3) / (n - 1)) / n)
    shifted, df_s, _ = R.nb_chi2(x, delta * 1.03, lamb)
    print("delta {} lamb {}: chi2 {:.1f} (df {}, threshold {:.1f}, smallest expected {:.0f}), z mean {:.2f}, "
          "z var {:.2f}, against 1.03 delta chi2 {:.1f}".format(delta, lamb, stat, df, threshold, smallest, z_mean,
                                                                 z_var, shifted))
    assert smallest >= 20 and df <= 33
    assert stat < threshold
    assert abs(z_mean) < 5 and abs(z_var) < 5
    if delta >= 9:
        assert shifted > R.chi2_threshold(df_s)


# ---------------------------------------------------------------------------- 6. heterogeneous elements

def test_heterogeneous_elements(nat):
    L, N, a, lamb, u, seed = 64, 512, 10.0, 0.75, 30.0, 77
    rng = np.random.default_rng(8)
    cn = rng.choice([1.0, 2.0, 3.0, 5.0], size=(L, N))
    gc = rng.uniform(0.3, 0.65, L).astype(np.float32)
    rho = rng.uniform(0, 1, L).astype(np.float32)
    tau = rng.uniform(0, 1, N).astype(np.float32)
    betas = np.stack([rng.normal(0.5, 1.0, N), rng.normal(0.0, 0.1, N)]).astype(np.float32)
    out = sim_reads(nat, cn, gc, betas, u, lamb, seed, rho=rho, tau=tau, a=a)
    assert out["exhausted"] == 0
    f = lambda v: np.asarray(v, np.float64)
    phi = 1.0 / (1.0 + np.exp(-a * (f(tau)[None, :] - f(rho)[:, None])))
    un = R.uniform32(R.draw(seed, R.TAG_READS, np.arange(L)[:, None], np.arange(N)[None, :], 0)[..., 0])
    rep = (f(un) < phi).astype(np.float64)
    omega = np.exp(f(betas[0])[None, :] * f(gc)[:, None] + f(betas[1])[None, :])
    delta = np.maximum(f(np.float32(u)) * cn * (1.0 + rep) * omega * (1 - lamb) / lamb, 1.0)
    mean, var, m4 = R.nb_moments(delta, lamb)         # mean theta and variance theta / (1 - lamb) where delta > 1
    z = (out["counts"][:, :N].astype(np.float64) - mean) / np.sqrt(var)
    n = z.size
    se_square = np.sqrt((m4 / var ** 2 - 1.0).sum()) / n
    print("heterogeneous: mean z {:.4f} (5/sqrt(n) = {:.4f}), mean z^2 {:.4f} (5 se = {:.4f}), rep differs in {}".format(
        z.mean(), 5 / np.sqrt(n), (z ** 2).mean(), 5 * se_square, int((rep != out["rep"][:, :N]).sum())))
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs((z ** 2).mean() - 1.0) < 5 * se_square


# ---------------------------------------------------------------------------- 7. normalisation

def test_normalisation(nat, s_case):
    c = Shape37x300
    _, one, _ = s_case
    L, N, ldn, num_reads = c.L, c.N, one["ldn"], 20000
    out = torch.full((L, ldn), -1.0, dtype=torch.float32, device=DEV)
    call = lambda r: nat.lib().pert_sim_normalise(L, N, ldn, float(r), one["counts_d"].data_ptr(),
                                                  one["colsum_d"].data_ptr(), out.data_ptr(), stream())
    assert call(num_reads) == 0
    got = out.cpu().numpy()
    raw = one["counts"][:, :N].astype(np.float64)
    colsum = raw.sum(0)
    np.testing.assert_array_equal(one["colsum"], colsum.astype(np.int64))
    want = (raw / colsum * num_reads).astype(np.int64)
    np.testing.assert_array_equal(got[:, :N], want.astype(np.float32))
    assert (got[:, N:] == 0).all()
    totals = got[:, :N].astype(np.int64).sum(0)
    assert (totals > num_reads - L).all() and (totals <= num_reads).all()
    assert call(2 ** 24) == PERT_E_ARG
    assert call(2 ** 24 - 1) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- 8. the reference's own test

def test_reference_simulator_test():
    """test_pert_simulator of the reference's test_with_pytest.py as written, its bin table taken
    from simulator.load_bins() instead of the csv path."""
    import pandas as pd
    from scipy import stats
    from scdna_replication_tools.pert_simulator import pert_simulator
    from scdna_replication_tools_amd.simulator import load_bins

    df = load_bins()
    df = df.loc[df['chr'] == '1']
    assert df.shape[1] == 6
    num_cells, num_cells_with_CNA, CNA_start, CNA_end, CNA_state = 100, 30, 0, 100, 3.0
    cn_g = []
    for i in range(num_cells):
        temp_cn = df.copy()
        temp_cn['cell_id'] = 'cell_{}_g'.format(i)
        temp_cn['library_id'] = 'ABCD'
        temp_cn['true_somatic_cn'] = 2.0
        if i < num_cells_with_CNA:
            temp_cn.iloc[CNA_start:CNA_end, temp_cn.columns.get_loc('true_somatic_cn')] = CNA_state
            temp_cn['clone_id'] = 'A'
        else:
            temp_cn['clone_id'] = 'B'
        cn_g.append(temp_cn)
    cn_g = pd.concat(cn_g, ignore_index=True)
    assert len(cn_g['cell_id'].unique()) == num_cells
    assert len(cn_g['clone_id'].unique()) == 2
    cn_s = cn_g.copy()
    cn_s['cell_id'] = cn_s['cell_id'].str.replace('_g', '_s')

    num_reads = int(1e6 / 20)
    clones = ['A', 'B']
    rt_cols = ['mcf7rt', 'mcf7rt']
    lamb = 0.75
    betas = [0.5, 0.0]
    a = 10.0
    torch.manual_seed(0)
    cn_s, cn_g = pert_simulator(cn_s, cn_g, num_reads, rt_cols, clones, lamb, betas, a, gc_col='gc',
                                input_cn_col='true_somatic_cn')

    assert 'true_reads_norm' in cn_s.columns
    assert 'true_t' in cn_s.columns
    assert 'true_rep' in cn_s.columns
    assert 'true_reads_norm' in cn_g.columns
    assert 'true_t' in cn_g.columns
    assert 'true_rep' in cn_g.columns
    assert np.all(cn_g['true_rep'] == 0)

    L = len(df)
    assert len(cn_s) == len(cn_g) == num_cells * L
    assert set(np.unique(cn_s['true_rep'])) <= {0.0, 1.0}
    assert ((cn_s['true_t'] > 0) & (cn_s['true_t'] < 1)).all()
    per_cell = cn_s.groupby('cell_id')
    assert (per_cell['true_t'].nunique() == 1).all()
    assert (cn_s['true_total_cn'] == cn_s['true_somatic_cn'] * (1 + cn_s['true_rep'])).all()
    assert (cn_g['true_total_cn'] == cn_g['true_somatic_cn']).all()
    assert cn_s['true_reads_norm'].dtype == np.int64
    totals = per_cell['true_reads_norm'].sum()
    assert ((totals > num_reads - L) & (totals <= num_reads)).all()
    rho = stats.spearmanr(per_cell['true_t'].first(), per_cell['true_rep'].mean())[0]
    print("reference test: spearman(true_t, replicated fraction) = {:.4f}".format(rho))
    assert rho > 0.9


def test_reference_helpers_return_cpu_tensors():
    """simulate_s_cells / simulate_g_cells with the reference's arguments (:201, :252): the same
    tuples, as CPU tensors of the reference's dtypes."""
    import pandas as pd
    from scdna_replication_tools.pert_simulator import (convert_rt_units, get_libraries_tensor, simulate_g_cells,
                                                         simulate_s_cells)
    from scdna_replication_tools_amd.simulator import load_bins
    bins = load_bins().iloc[:50]
    L, N, num_reads = len(bins), 7, 9000
    cells = ['c{}'.format(i) for i in range(N)]
    cn = pd.DataFrame(np.full((L, N), 2.0), columns=cells)
    long = pd.DataFrame({'cell_id': np.repeat(cells, L), 'library_id': np.repeat(['X', 'Y', 'X', 'X', 'Y', 'X', 'Y'], L)})
    libs, n_libs = get_libraries_tensor(long)
    assert n_libs == 2 and libs.tolist() == [0, 1, 0, 0, 1, 0, 1]
    out = simulate_s_cells(bins['gc'], libs, cn, bins['mcf7rt'], n_libs, num_reads, 0.75, [0.5, 0.0], 10.0, seed=3)
    reads_norm, reads, rep, p_rep, t = out
    assert [x.dtype for x in out] == [torch.int64, torch.float64, torch.float64, torch.float64, torch.float32]
    assert all(x.device.type == 'cpu' for x in out)
    assert [tuple(x.shape) for x in out] == [(L, N)] * 4 + [(N,)]
    rho = convert_rt_units(bins['mcf7rt'].to_numpy())
    want_p = 1 / (1 + np.exp(-10.0 * (t.numpy().astype(np.float64)[None, :] - rho[:, None])))
    np.testing.assert_allclose(p_rep.numpy(), want_p, atol=1e-6, rtol=0)
    np.testing.assert_array_equal(reads_norm.numpy(), (reads.numpy() / reads.numpy().sum(0) * num_reads).astype(np.int64))
    again = simulate_s_cells(bins['gc'], libs, cn, bins['mcf7rt'], n_libs, num_reads, 0.75, [0.5, 0.0], 10.0, seed=3)
    assert all(torch.equal(x, y) for x, y in zip(out, again))
    g = simulate_g_cells(bins['gc'], libs, cn, n_libs, num_reads, 0.75, [0.5, 0.0], seed=3)
    assert len(g) == 2 and g[0].dtype == torch.int64 and g[1].dtype == torch.float64 and g[0].shape == (L, N)
    # u = num_reads / (L mean(cn)): G1/2 cells carry 1.5 times the S cells' reads per copy
    assert 1.2 < g[1].mean().item() / (reads.numpy() / (1 + rep.numpy())).mean() < 1.8


# ---------------------------------------------------------------------------- 9. into the fit

# Recovery of the fit on pert_simulator data with the reference's per-cell beta spread
# (beta_stds = logspace(0, -K, K + 1)), measured once on an MI355X with the seed below
# (with beta_stds zeros the same run gave 1.0000 and 0.9952).  The test
# asserts 0.02 below: the spread seen between seeds of the existing recovery tests.
MEASURED_ACC_CN_DEFAULT_SPREAD = 1.0000
MEASURED_ACC_REP_DEFAULT_SPREAD = 0.9912
SEED_MARGIN = 0.02


def fit_accuracies(beta_stds):
    import pandas as pd
    from scdna_replication_tools.pert_simulator import pert_simulator
    from scdna_replication_tools_amd.pert_model import pert_infer_scRT
    from scdna_replication_tools_amd.simulator import clone_profiles, load_bins

    n_bins, n_cells = 300, 40
    bins = load_bins().iloc[:n_bins][['chr', 'start', 'end', 'gc', 'mcf7rt']]
    prof = clone_profiles(n_bins, 3)

    def cells(suffix):
        frames = []
        for i in range(n_cells):
            f = bins.copy()
            f['cell_id'] = 'cell_{}_{}'.format(suffix, i)
            f['library_id'] = 'LIB0'
            f['clone_id'] = 'ABC'[i % 3]
            f['true_somatic_cn'] = prof[:, i % 3]
            frames.append(f)
        return pd.concat(frames, ignore_index=True)

    df_s, df_g = pert_simulator(cells('S'), cells('G'), 183 * n_bins, ['mcf7rt'] * 3, ['A', 'B', 'C'], 0.75,
                                [0.5, 0.0], 10.0, seed=2, beta_stds=beta_stds)
    for df in (df_s, df_g):
        df['state'] = df['true_somatic_cn'].astype(np.int64)
        df['copy'] = df['true_somatic_cn']
    m = pert_infer_scRT(df_s, df_g, input_col='true_reads_norm', clone_col='clone_id', cn_prior_method='g1_clones',
                        max_iter=300, min_iter=50, rel_tol=1e-6, max_iter_step1=200, max_iter_step3=100)
    cn_s_out, supp_s, cn_g1_out, supp_g1 = m.run_pert_model()
    assert len(cn_s_out) == len(df_s)
    acc_cn = (cn_s_out["model_cn_state"] == cn_s_out["true_somatic_cn"]).mean()
    acc_rep = (cn_s_out["model_rep_state"] == cn_s_out["true_rep"]).mean()
    return float(acc_cn), float(acc_rep)


def test_into_the_fit_fixed_betas():
    """beta_stds zeros: the model simulator.simulate draws from, so test_pipeline_end_to_end's
    thresholds apply."""
    acc_cn, acc_rep = fit_accuracies(np.zeros(2))
    print("fit on pert_simulator data, fixed betas: acc_cn {:.4f} acc_rep {:.4f}".format(acc_cn, acc_rep))
    assert acc_cn > 0.97 and acc_rep > 0.9, (acc_cn, acc_rep)


def test_into_the_fit_default_beta_spread():
    acc_cn, acc_rep = fit_accuracies(None)
    print("fit on pert_simulator data, default beta spread: acc_cn {:.4f} acc_rep {:.4f}".format(acc_cn, acc_rep))
    assert acc_cn > MEASURED_ACC_CN_DEFAULT_SPREAD - SEED_MARGIN, acc_cn
    assert acc_rep > MEASURED_ACC_REP_DEFAULT_SPREAD - SEED_MARGIN, acc_rep
