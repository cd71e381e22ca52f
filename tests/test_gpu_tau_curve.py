"""GPU: per-cell likelihood curves over tau (pert_enum_evidence, pert_tau_curve,
PertShard.evidence / tau_curve, pert_infer_scRT(tau_curve=True)) against the fp64 oracle.

The branch evidences must lie within the element bound, and the curves and the values at the
fitted tau within the cell bound, of tests/_curve_bounds.py; the curve kernel alone is checked
against an fp64 evaluation of the device's own evidences; the evidences must reproduce the
posterior pass's P(rep = 1); padding stays untouched, reruns and chunked grids are bit-identical.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _curve_bounds as cb
from tests import _post_bounds as pb
from tests._problems import KIND_OF, init_constrained, make_problem

pytestmark = pytest.mark.gpu

EPS32 = cb.EPS32

# (kind, L, N, P, make_problem arguments, bounded)
CASES = {
    "step2_deep": ("step2", 40, 70, 13, dict(seed=0), True),                  # second cell tile: 6 real lanes
    "step2_low": ("step2", 40, 70, 13, dict(seed=0, low_reads=True), True),
    "step3_low": ("step3", 33, 65, 5, dict(seed=2, low_reads=True), True),   # frozen rho / a; one real lane
    "bin_tiles": ("step2", 150, 64, 13, dict(seed=4, low_reads=True, prior="composite"), True),   # > one bin tile
    "P16": ("step2", 24, 300, 16, dict(low_reads=True, prior="uniform", z_scale=0.3), False),     # ldn 512
    # (one cell holds one library: make_problem's default of two cannot be built at N = 1)
    "tiny_P2": ("step2", 2, 1, 2, dict(K=2, n_libs=1), False),
}
GRIDS = {"default": None, "G1": np.array([0.3], np.float32), "G17": np.linspace(0.05, 0.95, 17).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The problem, its oracle evidences (computed once, never modified) and the device runs."""
    from scdna_replication_tools_amd.engine import PertShard
    kind, L, N, P, extra, bounded = CASES[name]
    prob, kw, z = make_problem(kind, L=L, N=N, P=P, **extra)
    sh = PertShard(KIND_OF[kind], init=init_constrained(kind, z), device="cuda", dirichlet_mode="exact", **kw)
    sh.set_unconstrained({k: v.numpy() for k, v in z.items()})
    if name == "bin_tiles":
        assert -(-L // min(sh.bins_per_tile, 64)) >= 2
    if name == "P16":
        assert sh.ldn == 512
    ref = cb.oracle_evidence(prob, z)
    assert np.isfinite(ref["e"]).all()
    ev = {k: v.cpu().numpy().astype(np.float64) for k, v in sh.evidence().items()}
    curves = {g: sh.tau_curve(grid) for g, grid in GRIDS.items()}
    torch.cuda.synchronize()
    return dict(prob=prob, z=z, sh=sh, ref=ref, ev=ev, curves=curves, L=L, N=N, P=P, bounded=bounded)


@pytest.mark.parametrize("name", list(CASES))
def test_evidence_within_element_bound_of_oracle(name):
    c = _case(name)
    out = c["sh"].evidence()
    assert set(out) == {"ev0", "ev1"}
    for r, k in enumerate(("ev0", "ev1")):
        assert out[k].shape == (c["L"], c["N"]) and out[k].dtype == torch.float32
        worst = pb.check(k, c["ev"][k], c["ref"]["e"][r], c["ref"]["B"][r])
        print("{} {}: worst |delta| / bound {:.3f}; median bound {:.3g}".format(
            name, k, worst, float(np.median(c["ref"]["B"][r]))))


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][5]])
def test_the_cell_bound_is_sharp(name):
    """From the oracle alone: every cell's bound is at most 0.1 of that cell's curve range over
    the default grid, so a curve within the bound has the oracle's shape."""
    ratio = cb.sharpness(_case(name)["ref"])
    print("{}: worst cell bound / curve range {:.4f}".format(name, float(ratio.max())))
    assert (ratio <= 0.1).all(), float(ratio.max())


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("name", list(CASES))
def test_curve_within_cell_bound_of_oracle(name, grid):
    c = _case(name)
    tc, ref = c["curves"][grid], c["ref"]
    g = cb.DEFAULT_GRID if GRIDS[grid] is None else GRIDS[grid]
    assert np.array_equal(tc.grid, g) and tc.loglik.shape == (g.size, c["N"]) and tc.loglik.dtype == np.float64
    assert tc.at_fit.shape == (c["N"],) and tc.tau.shape == (c["N"],)
    want, bound = cb.curve(ref, g.astype(np.float64))
    r_curve = pb.check("likelihood_only.loglik", tc.likelihood_only.loglik, want, bound)
    # the fitted tau: the oracle's constrained value of the same fp32 parameter
    assert np.abs(tc.tau.astype(np.float64) - ref["tau"]).max() <= 4 * EPS32
    want_fit, bound_fit = cb.curve_at(ref, ref["tau"])
    r_fit = pb.check("likelihood_only.at_fit", tc.likelihood_only.at_fit, want_fit, bound_fit)
    print("{} {}: worst |delta| / cell bound  curve {:.3f}  at_fit {:.3f}; median bound {:.3g}".format(
        name, grid, r_curve, r_fit, float(np.median(bound))))
    # the u prior, the one other term tau enters, in fp64 on the host
    from scdna_replication_tools_amd.tau_curve import u_prior_logpdf
    sh = c["sh"]
    u = sh.params[sh.lay.off_u:sh.lay.off_u + c["N"]].cpu().numpy()
    args = (u, sh.mean_reads.cpu().numpy(), sh.ploidy.cpu().numpy())
    # (the uniform prior's argmax state is 0 in every bin: ploidy 0, where the model's own u prior
    # is undefined and so is this term; everywhere else it is finite)
    defined = args[2] > 0
    assert defined.all() or name == "P16"
    with np.errstate(all="ignore"):
        prior, prior_fit = u_prior_logpdf(*args, g.astype(np.float64)[:, None]), u_prior_logpdf(*args, tc.tau.astype(np.float64))
    assert np.isfinite(prior[:, defined]).all() and np.isfinite(prior_fit[defined]).all()
    assert np.array_equal(tc.loglik, tc.likelihood_only.loglik + prior, equal_nan=True)
    assert np.array_equal(tc.at_fit, tc.likelihood_only.at_fit + prior_fit, equal_nan=True)
    if defined.all():
        from torch.distributions import Normal
        gm = torch.tensor(args[1], dtype=torch.float64) / ((1 + 0.3) * torch.tensor(args[2], dtype=torch.float64))
        lp = Normal(gm, gm / 10).log_prob(torch.tensor(u, dtype=torch.float64)).numpy()
        assert np.allclose(u_prior_logpdf(*args, 0.3), lp, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", list(CASES))
def test_curve_kernel_alone_against_fp64_of_the_device_evidence(name):
    """The device's own ev through an fp64 evaluation of m: each (g, n) within
    sum_l 6 eps32 (1 + |m|) -- tau_mix's own error, with kernel 1's taken out."""
    c = _case(name)
    sh, tc = c["sh"], c["curves"]["default"]
    con = sh.constrained()
    frozen = c["prob"].kind == "step3"
    a = float(np.asarray(c["prob"].a_fixed).reshape(-1)[0]) if frozen else float(np.asarray(con["expose_a"])[0])
    rho = (np.asarray(c["prob"].rho_fixed, np.float64) if frozen else np.asarray(con["expose_rho"], np.float64)).reshape(-1, 1)
    e0, e1 = c["ev"]["ev0"], c["ev"]["ev1"]
    worst = 0.0
    taus = [np.full(c["N"], t, np.float64) for t in tc.grid.astype(np.float64)] + [tc.tau.astype(np.float64)]
    devs = list(tc.likelihood_only.loglik) + [tc.likelihood_only.at_fit]
    for t, dev in zip(taus, devs):
        m, _ = cb.mix(e0, e1, cb.phi_of(a, t[None, :], rho))
        bound = (6 * EPS32 * (1 + np.abs(m))).sum(0)
        ratio = np.abs(dev - m.sum(0)) / bound
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (float(t[0]), float(ratio.max()))
    print("{}: worst |delta| / sum_l 6 eps32 (1 + |m|) = {:.3f}".format(name, worst))


@pytest.mark.parametrize("name", list(CASES))
def test_evidence_reproduces_the_posterior_pass(name):
    """P(rep = 1) of posterior() equals phi e^{e_1} / ((1 - phi) e^{e_0} + phi e^{e_1}) at the
    fitted tau, within _post_bounds' b_rep (the posterior pass's own error, its fp32 phi included)
    plus the element bounds propagated through the weight: gamma_1 (1 - gamma_1) (B_0 + B_1)."""
    c = _case(name)
    ref = c["ref"]
    rep_prob = c["sh"].posterior()["rep_prob"].cpu().numpy().astype(np.float64)
    marg = pb.oracle_marginals(c["prob"], c["z"])
    phi = cb.phi_of(ref["a"], ref["tau"][None, :], ref["rho"][:, None])
    _, g1 = cb.mix(c["ev"]["ev0"], c["ev"]["ev1"], phi)
    _, g1_ref = cb.mix(ref["e"][0], ref["e"][1], phi)
    assert np.abs(g1_ref - marg["p_rep"]).max() < 1e-9          # the factorisation itself, in fp64
    bound = marg["b_rep"] + g1_ref * (1 - g1_ref) * (ref["B"][0] + ref["B"][1]) + 4 * EPS32
    worst = pb.check("rep_prob from ev", g1, rep_prob, bound)
    print("{}: worst |delta| / bound {:.3f}; 0.01 < P(rep) < 0.99 on {:.0%}".format(
        name, worst, float(((marg["p_rep"] > 0.01) & (marg["p_rep"] < 0.99)).mean())))


@pytest.mark.parametrize("name", list(CASES))
def test_padding_untouched_reruns_and_chunks_bit_identical(name):
    """Through the C entry points on raw buffers pre-filled with NaN: columns n >= N of ev keep
    the fill's bits and the real ones are finite; a second launch of either kernel writes the same
    bytes; a grid evaluated in two chunks equals the one-call result bit for bit; nothing of the
    state moves."""
    c = _case(name)
    sh, L, N = c["sh"], c["L"], c["N"]
    ldn, dev = sh.ldn, sh.device
    z0, p0 = sh.z_pi.clone(), sh.params.clone()
    grid = torch.as_tensor(cb.DEFAULT_GRID, device=dev)
    G = grid.numel()
    nan = float("nan")

    def run_ev():
        ev = torch.full((2, L, ldn), nan, dtype=torch.float32, device=dev)
        assert sh.lib.pert_enum_evidence(ctypes.byref(sh._prob), ctypes.byref(sh._state), ev.data_ptr(), sh._stream()) == 0
        return ev

    def run_curve(ev, g):
        curve = torch.full((g.numel(), N), nan, dtype=torch.float64, device=dev)
        fit = torch.full((N,), nan, dtype=torch.float64, device=dev)
        assert sh.lib.pert_tau_curve(ctypes.byref(sh._prob), ctypes.byref(sh._state), ev.data_ptr(), g.data_ptr(),
                                     g.numel(), curve.data_ptr(), fit.data_ptr(), sh._stream()) == 0
        return curve, fit
    ev_a, ev_b = run_ev(), run_ev()
    fill = torch.full((1,), nan, dtype=torch.float32).view(torch.int32).item()
    real, pad = ev_a[..., :N], ev_a[..., N:]
    assert torch.isfinite(real).all()
    assert pad.numel() > 0 and (pad.contiguous().view(torch.int32) == fill).all()
    assert torch.equal(ev_a.view(torch.int32), ev_b.view(torch.int32))
    (c1, f1), (c2, f2) = run_curve(ev_a, grid), run_curve(ev_a, grid)
    assert torch.isfinite(c1).all() and torch.isfinite(f1).all()
    assert torch.equal(c1.view(torch.int64), c2.view(torch.int64)) and torch.equal(f1.view(torch.int64), f2.view(torch.int64))
    for cut in (37, 8, 1):                                      # off and on the kernel's chunk of grid points
        (ca, fa), (cb_, fb) = run_curve(ev_a, grid[:cut].contiguous()), run_curve(ev_a, grid[cut:].contiguous())
        assert torch.equal(torch.cat([ca, cb_]).view(torch.int64), c1.view(torch.int64)), cut
        assert torch.equal(fa.view(torch.int64), f1.view(torch.int64)) and torch.equal(fb.view(torch.int64), f1.view(torch.int64))
    torch.cuda.synchronize()
    # the Python path is these launches
    tc = c["curves"]["default"]
    assert np.array_equal(tc.likelihood_only.loglik, c1.cpu().numpy())
    assert np.array_equal(tc.likelihood_only.at_fit, f1.cpu().numpy())
    assert torch.equal(sh.z_pi.view(torch.int32), z0.view(torch.int32))
    assert torch.equal(sh.params.view(torch.int32), p0.view(torch.int32))


def test_argument_errors_before_any_launch():
    c = _case("step3_low")
    sh = c["sh"]
    N = c["N"]
    ev = sh.ev
    grid = torch.as_tensor(cb.DEFAULT_GRID, device=sh.device)
    curve = torch.zeros((grid.numel(), N), dtype=torch.float64, device=sh.device)
    fit = torch.zeros(N, dtype=torch.float64, device=sh.device)
    lib, pr, st = sh.lib, sh._prob, sh._state
    E_ARG = 1

    def tc(prob=pr, state=st, e=ev.data_ptr(), g=grid.data_ptr(), G=grid.numel(), cu=curve.data_ptr(), f=fit.data_ptr()):
        return lib.pert_tau_curve(ctypes.byref(prob), ctypes.byref(state), e, g, G, cu, f, sh._stream())
    assert tc() == 0
    for k in ("e", "g", "cu", "f"):
        assert tc(**{k: None}) == E_ARG
    for G in (0, -3, 1025):
        assert tc(G=G) == E_ARG

    def changed(**kw):
        p2 = type(pr)()
        ctypes.memmove(ctypes.byref(p2), ctypes.byref(pr), ctypes.sizeof(pr))
        for k, v in kw.items():
            setattr(p2, k, v)
        return p2
    for kw in (dict(kind=1), dict(L=0), dict(N=0), dict(N=sh.ldn + 1), dict(ldn=sh.ldn - 1), dict(rho_fixed=None)):
        assert tc(prob=changed(**kw)) == E_ARG, kw
        assert lib.pert_enum_evidence(ctypes.byref(changed(**kw)), ctypes.byref(st), ev.data_ptr(), sh._stream()) == E_ARG, kw
    assert lib.pert_enum_evidence(ctypes.byref(changed(P=17)), ctypes.byref(st), ev.data_ptr(), sh._stream()) == 2
    assert lib.pert_enum_evidence(ctypes.byref(changed(K1=9)), ctypes.byref(st), ev.data_ptr(), sh._stream()) == 3
    assert lib.pert_enum_evidence(ctypes.byref(pr), ctypes.byref(st), None, sh._stream()) == E_ARG
    torch.cuda.synchronize()
    # the Python wrapper validates the grid, which the library cannot read
    for bad in ([0.6, 0.4], [0.0, 0.5], [0.5, 1.0], [0.5, 0.5], [float("nan")], []):
        with pytest.raises(ValueError):
            sh.tau_curve(bad)


def test_step1_has_no_curve():
    from scdna_replication_tools_amd.engine import PertShard
    prob, kw, z = make_problem("step1", L=8, N=6, seed=1)
    sh = PertShard(1, init=init_constrained("step1", z), device="cuda", **kw)
    with pytest.raises(ValueError):
        sh.evidence()
    with pytest.raises(ValueError):
        sh.tau_curve()


def test_pipeline_tau_tables():
    """pert_infer_scRT(tau_curve=True) against tau_curve=False on the tables and limits of
    test_gpu_fit's pipeline test: the four returned frames are equal, and the model carries one
    table row per S cell and per G1/2 cell."""
    from scdna_replication_tools_amd.pert_model import pert_infer_scRT
    from scdna_replication_tools_amd.simulator import simulate, to_long_form
    from scdna_replication_tools_amd.tau_curve import TABLE_COLUMNS
    sim = simulate(n_s=40, n_g=40, n_bins=300, num_reads=183 * 300, seed=2)
    df_s, df_g = to_long_form(sim, n_libs=1)
    runs, models = {}, {}
    for flag in (False, True):
        m = pert_infer_scRT(df_s.copy(), df_g.copy(), input_col='reads', clone_col='clone_id',
                            cn_prior_method='g1_clones', max_iter=300, min_iter=50, rel_tol=1e-6, max_iter_step1=200,
                            max_iter_step3=100, tau_curve=flag)
        runs[flag] = m.run_pert_model()
        models[flag] = m
    for a, b in zip(runs[False], runs[True]):
        assert a.equals(b)
    off = models[False]
    assert off.tau_curve_s is None and off.tau_table_s is None and off.tau_curve_g is None and off.tau_table_g is None
    m = models[True]
    for curve, table, out in ((m.tau_curve_s, m.tau_table_s, runs[True][0]), (m.tau_curve_g, m.tau_table_g, runs[True][2])):
        assert list(table.columns) == ["cell_id"] + TABLE_COLUMNS
        assert len(table) == 40 and curve.loglik.shape == (99, 40)
        assert sorted(table["cell_id"].astype(str)) == sorted(out["cell_id"].astype(str).unique())
        assert np.isfinite(curve.loglik).all() and np.isfinite(curve.at_fit).all()
        assert np.array_equal(table["curve_at_fit"].to_numpy(), curve.at_fit)
        for col in ("model_tau", "curve_at_fit", "curve_tau", "curve_gain"):
            assert np.isfinite(table[col].to_numpy(np.float64)).all(), col
        n_modes = table["n_modes"].to_numpy()
        empty, single = n_modes == 0, n_modes < 2
        for col in ("tau_lo", "tau_hi"):
            assert (np.isnan(table[col].to_numpy()) == empty).all(), col
        for col in ("alt_tau", "alt_drop"):
            assert (np.isnan(table[col].to_numpy()) == single).all(), col
        # the table's model_tau is the frame's
        tau_frame = out.groupby(out["cell_id"].astype(str))["model_tau"].first()
        got = table.set_index(table["cell_id"].astype(str))["model_tau"]
        assert np.array_equal(got.loc[tau_frame.index].to_numpy(np.float32), tau_frame.to_numpy(np.float32))
