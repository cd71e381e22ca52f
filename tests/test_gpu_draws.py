"""GPU: posterior draws of replication and copy-number state (pert_enum_draw,
PertShard.draw_states, pert_infer_scRT(posterior_draws=...)) against the fp64 oracle.

Every draw must satisfy the conditions of tests/_draw_ref.py at the oracle's posterior of the same
point with the uniform of the documented counter rule; the draws must not depend on how they are
chunked or on which cells a launch holds, must leave the padding and the fit's state untouched,
and must be bit-identical from run to run.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _draw_ref as dr
from tests import _post_bounds as pb
from tests import _sim_ref as sr
from tests._problems import KIND_OF, init_constrained, make_problem

pytestmark = pytest.mark.gpu

# test_gpu_posterior's CASES, by value: (kind, L, N, P, make_problem arguments)
CASES = {
    "step2_deep": ("step2", 40, 70, 13, dict(seed=0)),                       # second cell tile: 6 real lanes
    "step2_low": ("step2", 40, 70, 13, dict(seed=0, low_reads=True)),
    "step3_low": ("step3", 33, 65, 5, dict(seed=2, low_reads=True)),        # frozen rho / a; one real lane
    "bin_tiles": ("step2", 150, 64, 13, dict(seed=4, low_reads=True, prior="composite")),   # L > kMaxLT = 64
    "P16": ("step2", 24, 130, 16, dict(seed=7, low_reads=True, prior="uniform", z_scale=0.3)),
    "tiny": ("step2", 2, 1, 13, dict(seed=6, n_libs=1, low_reads=True)),
    "tiny_P2": ("step2", 2, 1, 2, dict(seed=5, K=2, n_libs=1)),              # smallest P and K, saturated
}
N_DRAWS = 8
SEED = (5 << 32) | 77        # a high word: the key's second word is not the tag's alone
SENTINEL = 0xEE


def _shard(kind, prob_kw, z, **extra):
    from scdna_replication_tools_amd.engine import PertShard
    sh = PertShard(KIND_OF[kind], init=init_constrained(kind, z), device="cuda", dirichlet_mode="exact",
                   **prob_kw, **extra)
    sh.set_unconstrained({k: v.numpy() for k, v in z.items()})
    return sh


@functools.lru_cache(maxsize=None)
def _case(name):
    """The problem, its oracle posterior (computed once, never modified) and the device draws."""
    kind, L, N, P, extra = CASES[name]
    prob, kw, z = make_problem(kind, L=L, N=N, P=P, **extra)
    sh = _shard(kind, kw, z)
    if name == "bin_tiles":
        assert -(-L // min(sh.bins_per_tile, 64)) >= 2
    ref = pb.oracle_marginals(prob, z)
    for v in ref.values():
        v.setflags(write=False)
    out = {k: v.clone() for k, v in sh.draw_states(N_DRAWS, seed=SEED).items()}
    torch.cuda.synchronize()
    u = dr.uniforms(SEED, np.arange(L)[:, None], np.arange(N)[None, :], 0, N_DRAWS)
    u.setflags(write=False)
    return dict(prob=prob, kw=kw, z=z, sh=sh, ref=ref, out=out, u=u, kind=kind, L=L, N=N, P=P)


def _raw(sh, n_draws, seed=SEED, first=0, cell0=0, want_cn=True):
    """pert_enum_draw on sentinel-filled raw [n_draws][L][ldn] buffers."""
    shape = (n_draws, sh.L, sh.ldn)
    rep = torch.full(shape, SENTINEL, dtype=torch.uint8, device=sh.device)
    cn = torch.full(shape, SENTINEL, dtype=torch.uint8, device=sh.device) if want_cn else None
    rc = sh.lib.pert_enum_draw(ctypes.byref(sh._prob), ctypes.byref(sh._state), seed, cell0, first, n_draws,
                               rep.data_ptr(), 0 if cn is None else cn.data_ptr(), sh._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return rep, cn


@pytest.mark.parametrize("name", list(CASES))
def test_draws_within_oracle_condition(name):
    c = _case(name)
    rep, cn = c["out"]["rep"], c["out"]["cn"]
    assert rep.shape == cn.shape == (N_DRAWS, c["L"], c["N"]) and rep.dtype == cn.dtype == torch.uint8
    assert int(rep.max()) <= 1 and int(cn.max()) < c["P"]
    j_dev = 2 * cn.cpu().numpy().astype(np.int64) + rep.cpu().numpy()
    share = dr.check(name, c["ref"], c["u"], j_dev)
    _, _, b = dr.prefix(c["ref"])
    top = dr.joint_order(c["ref"]["gamma"]).max(0)
    print("{}: {:.3%} of {} draws differ from the fp64 draw (cap {:.0%}); median prefix bound {:.3g}; "
          "top state < 0.99 on {:.0%}".format(name, share, j_dev.size, dr.CAP, float(np.median(b)),
                                              float((top < 0.99).mean())))
    # cn_draw = NULL gives the same rep planes
    only = c["sh"].draw_states(N_DRAWS, seed=SEED, want_cn=False)
    assert set(only) == {"rep"} and torch.equal(only["rep"], rep)


@pytest.mark.parametrize("name", list(CASES))
def test_chunks_padding_and_reruns(name):
    """Draws 0..7 in one call equal draws 0..2 and then 3..7 (across a Philox word group); the
    padding columns keep the sentinel; a second launch writes the same bytes; the raw entry point
    agrees with draw_states, with and without the cn planes."""
    c = _case(name)
    sh, N = c["sh"], c["N"]
    rep, cn = _raw(sh, N_DRAWS)
    for b in (rep, cn):
        assert b[..., N:].numel() > 0 and (b[..., N:] == SENTINEL).all() and (b[..., :N] != SENTINEL).all()
    assert torch.equal(rep[..., :N], c["out"]["rep"]) and torch.equal(cn[..., :N], c["out"]["cn"])
    rep2, cn2 = _raw(sh, N_DRAWS)
    assert torch.equal(rep, rep2) and torch.equal(cn, cn2)
    ra, ca = _raw(sh, 3, first=0)
    rb, cb = _raw(sh, 5, first=3)
    assert torch.equal(torch.cat([ra, rb]), rep) and torch.equal(torch.cat([ca, cb]), cn)
    rn, none = _raw(sh, N_DRAWS, want_cn=False)
    assert none is None and torch.equal(rn, rep)


def test_cell0_shards_reproduce_the_whole():
    """Cells [0, 64) and [64, 70) of step2_deep as shards of their own, the second with
    cell0 = 64, give the 70-cell shard's columns bit for bit."""
    c = _case("step2_deep")
    kind, prob, kw, z = c["kind"], c["prob"], c["kw"], c["z"]
    parts = []
    for a, b in ((0, 64), (64, 70)):
        sub = dict(kw, reads=kw["reads"][:, a:b], libs=kw["libs"][a:b], eta=kw["eta"].cells(slice(a, b)))
        zs = {k: (v[a:b] if k in ("expose_tau", "expose_u", "expose_betas") else v[:, a:b] if k == "expose_pi" else v)
              for k, v in z.items()}
        sh = _shard(kind, sub, zs)
        parts.append({k: v.clone() for k, v in sh.draw_states(N_DRAWS, seed=SEED, cell0=a).items()})
        # the shard against the oracle of ITS cells, under the uniforms of their global indices
        j_dev = 2 * parts[-1]["cn"].cpu().numpy().astype(np.int64) + parts[-1]["rep"].cpu().numpy()
        dr.check("cells [{}, {})".format(a, b), pb.oracle_marginals(prob.cells(slice(a, b)), zs), c["u"][:, :, a:b],
                 j_dev)
    for k in ("rep", "cn"):
        assert torch.equal(torch.cat([p[k] for p in parts], dim=2), c["out"][k]), k
    # and without cell0 the second shard draws other numbers
    other = sh.draw_states(N_DRAWS, seed=SEED, cell0=0)
    assert not (torch.equal(other["rep"], parts[1]["rep"]) and torch.equal(other["cn"], parts[1]["cn"]))


def test_seed_high_word_and_draw_index_matter():
    c = _case("step2_low")
    sh = c["sh"]
    low = {k: v.clone() for k, v in sh.draw_states(N_DRAWS, seed=SEED & 0xFFFFFFFF).items()}
    assert not torch.equal(low["rep"], c["out"]["rep"]) and not torch.equal(low["cn"], c["out"]["cn"])
    # the low word alone is itself within the oracle condition under ITS uniforms
    u = dr.uniforms(SEED & 0xFFFFFFFF, np.arange(c["L"])[:, None], np.arange(c["N"])[None, :], 0, N_DRAWS)
    dr.check("low word", c["ref"], u, 2 * low["cn"].cpu().numpy().astype(np.int64) + low["rep"].cpu().numpy())
    planes = c["out"]["rep"]
    assert len({planes[d].cpu().numpy().tobytes() for d in range(N_DRAWS)}) == N_DRAWS


@pytest.mark.parametrize("name", ["step2_deep", "step3_low"])
def test_nothing_of_the_fit_moves(name):
    c = _case(name)
    sh = c["sh"]
    cn0, rep0 = (t.clone() for t in sh.decode())
    keep = {k: getattr(sh, k).clone() for k in ("params", "z_pi", "m_pi", "v_pi", "adam_m", "adam_v")
            if getattr(sh, k, None) is not None}
    assert {"params", "z_pi"} <= set(keep)
    first = {k: v.clone() for k, v in sh.draw_states(N_DRAWS, seed=SEED).items()}
    buf = sh.rep_draw.data_ptr()
    second = sh.draw_states(N_DRAWS, seed=SEED)
    assert sh.rep_draw.data_ptr() == buf                      # the buffers are reused while the shape holds
    for k in first:
        assert torch.equal(first[k], second[k]) and torch.equal(first[k], c["out"][k]), k
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(getattr(sh, k).view(torch.int32), v.view(torch.int32)), k
    assert torch.equal(sh.cn_out[:, :c["N"]], cn0) and torch.equal(sh.rep_out[:, :c["N"]], rep0)
    assert sh.draw_states(3, seed=SEED)["rep"].shape[0] == 3   # another shape: new buffers
    assert torch.equal(sh.draw_states(3, seed=SEED, first_draw=2)["cn"], c["out"]["cn"][2:5])


def test_step1_has_no_draws():
    from scdna_replication_tools_amd.engine import PertShard
    prob, kw, z = make_problem("step1", L=8, N=6, seed=1)
    sh = PertShard(1, init=init_constrained("step1", z), device="cuda", **kw)
    with pytest.raises(ValueError):
        sh.draw_states(4)
    assert sh.rep_draw is None


def _pooled_chi2(observed, expected, min_expected=20.0):
    """Pearson chi-square of counts against expected counts, the states with an expected count
    below ``min_expected`` pooled into one class (and that class, if still small, into the smallest
    of the others).  Returns (statistic, degrees of freedom)."""
    big = expected >= min_expected
    exp_, obs_ = list(expected[big]), list(observed[big])
    if (~big).any():
        exp_.append(expected[~big].sum())
        obs_.append(observed[~big].sum())
        if exp_[-1] < min_expected and len(exp_) > 1:
            k = int(np.argmin(exp_[:-1]))
            exp_[k] += exp_.pop()
            obs_[k] += obs_.pop()
    exp_, obs_ = np.asarray(exp_), np.asarray(obs_)
    assert obs_.sum() == observed.sum() and abs(exp_.sum() - observed.sum()) < 1e-6 * observed.sum()
    return float(((obs_ - exp_) ** 2 / exp_).sum()), len(exp_) - 1


@pytest.mark.parametrize("name", ["tiny", "P16"])
def test_distribution_of_many_draws(name):
    """2,048 draws (tiny: 2 bins x 1 cell; and P16, whose uniform prior leaves most elements
    uncertain): per element the Pearson chi-square of the joint-state counts against the fp64
    gamma, states with an expected count under 20 pooled, stays below the 1e-6 quantile of its
    chi-square law."""
    c = _case(name)
    n = 2048
    out = c["sh"].draw_states(n, seed=SEED)
    j = (2 * out["cn"].cpu().numpy().astype(np.int64) + out["rep"].cpu().numpy()).reshape(n, -1)
    g = dr.joint_order(c["ref"]["gamma"]).reshape(2 * c["P"], -1)
    worst, dfs = 0.0, []
    for e in range(j.shape[1]):
        stat, df = _pooled_chi2(np.bincount(j[:, e], minlength=2 * c["P"]).astype(np.float64), g[:, e] * n)
        dfs.append(df)
        if df > 0:
            thr = sr.chi2_threshold(df, alpha=1e-6)
            assert stat < thr, (e, stat, df)
            worst = max(worst, stat / thr)
        else:
            assert stat < 1e-3, (e, stat)       # one class holds every draw but an expected < 1e-3 of them
    print("{}: {} elements x {} draws, df {}..{}, worst chi2 / threshold {:.3f}".format(
        name, j.shape[1], n, min(dfs), max(dfs), worst))
    assert max(dfs) >= 1
    # the draws of the first 8 indices are the case's
    assert torch.equal(out["rep"][:N_DRAWS], c["out"]["rep"])


def test_pipeline_posterior_draws():
    """pert_infer_scRT(posterior_draws=4) against a run without the keyword on the tables and
    limits of test_gpu_posterior's pipeline test: the frames are unchanged, and draws_s holds 4
    planes shaped and ordered like the MAP matrix."""
    import pandas as pd
    from scdna_replication_tools_amd.pert_model import pert_infer_scRT
    from scdna_replication_tools_amd.posterior_draws import PosteriorDraws
    from scdna_replication_tools_amd.simulator import simulate, to_long_form
    sim = simulate(n_s=40, n_g=40, n_bins=300, num_reads=183 * 300, seed=2)
    df_s, df_g = to_long_form(sim, n_libs=1)
    runs, models = {}, {}
    for n in (0, 4):
        m = pert_infer_scRT(df_s.copy(), df_g.copy(), input_col='reads', clone_col='clone_id',
                            cn_prior_method='g1_clones', max_iter=300, min_iter=50, rel_tol=1e-6, max_iter_step1=200,
                            max_iter_step3=100, posterior_draws=n)
        runs[n], models[n] = m.run_pert_model(), m
    for a, b in zip(runs[0], runs[4]):
        pd.testing.assert_frame_equal(a, b)
    assert models[0].draws_s is None
    d = models[4].draws_s
    assert isinstance(d, PosteriorDraws) and d.n_draws == 4 and d.cn.shape == d.rep.shape
    out = runs[4][0]
    inp = models[4]._prepare()
    assert list(d.cell_ids) == list(inp.cells_s) and (d.L, d.N) == (len(inp.loci_start), len(inp.cells_s))
    assert d.L * d.N == len(out)
    # the MAP matrix in the planes' order, from the output's own labels
    ci = pd.Index(d.cell_ids.astype(str)).get_indexer(out["cell_id"].astype(str).to_numpy())
    li = pd.MultiIndex.from_arrays([d.chr.astype(str), d.start]).get_indexer(
        pd.MultiIndex.from_arrays([out["chr"].astype(str).to_numpy(), out["start"].to_numpy()]))
    assert (ci >= 0).all() and (li >= 0).all()
    rep_map = np.zeros((d.L, d.N), np.int64)
    rep_map[li, ci] = out["model_rep_state"].to_numpy().astype(np.int64)
    clone_of = np.empty(d.N, object)
    clone_of[ci] = out["clone_id"].to_numpy()
    assert list(d.clone_ids) == list(clone_of)
    # draws of the posterior the MAP is the argmax of
    rep = np.asarray(d.rep)
    assert rep.shape == (4,) + rep_map.shape and rep.max() <= 1 and np.asarray(d.cn).max() < 13
    # coin flips would agree with the MAP calls on half the elements, and planes in another cell
    # order on as many as a neighbouring cell's calls do
    for i in range(4):
        agree = float((rep[i] == rep_map).mean())
        assert agree > 0.6 and agree > float((rep[i] == np.roll(rep_map, 1, axis=1)).mean()), (i, agree)
    assert len({rep[i].tobytes() for i in range(4)}) == 4
    tw = d.twidth()
    assert len(tw) == 4 and np.isfinite(tw["t_width"]).all()
    assert d.frac_rt().shape == (4, d.N) and len(d.cell_table()) == d.N and len(d.pseudobulk()) == d.L
