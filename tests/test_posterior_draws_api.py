"""PosteriorDraws on hand-made host planes (no GPU): every statistic against the same quantity
computed draw by draw through the existing RTMatrix host path, and against plain numpy."""
import numpy as np
import pytest
import torch

from scdna_replication_tools_amd.posterior_draws import PosteriorDraws
from scdna_replication_tools_amd.rt_profiles import RTMatrix

N_DRAWS, L, N = 3, 6, 5
CELLS = np.array(["c3", "c0", "c4", "c1", "c2"])
CLONES = np.array(["B", "A", "A", "B", "A"])
CHR = np.array(["2", "1", "1", "2", "1", "10"])
START = np.array([500, 1000, 0, 0, 500, 0])
Q = (0.05, 0.5, 0.95)


def _planes():
    rng = np.random.default_rng(3)
    # cells replicate a draw-dependent early part of a per-locus timing, so profiles are not constant
    timing = rng.permutation(L)[:, None]
    depth = np.array([1, 2, 3, 4, 5])[None, :]
    rep = np.stack([(timing < np.clip(depth + s, 0, L)).astype(np.uint8) for s in (-1, 0, 1)])
    rep[1, 0, 0] ^= 1
    rep[2, 3, 4] ^= 1
    cn = rng.integers(0, 13, rep.shape).astype(np.uint8)
    return rep, cn


@pytest.fixture(scope="module", params=["numpy", "torch"])
def draws(request):
    rep, cn = _planes()
    if request.param == "torch":
        rep, cn = torch.from_numpy(rep), torch.from_numpy(cn)
    return PosteriorDraws(rep, CELLS, CHR, START, clone_ids=CLONES, cn=cn, device="cpu"), _planes()[0]


def _mats(rep):
    return [RTMatrix(rep[d].copy(), CELLS, CHR, START, clone_ids=CLONES, device="cpu") for d in range(N_DRAWS)]


def test_shapes_and_rt_matrix_in_place(draws):
    pd_, rep = draws
    assert len(pd_) == pd_.n_draws == N_DRAWS and (pd_.L, pd_.N) == (L, N) and pd_.cn.shape == pd_.rep.shape
    base = pd_.rep.numpy() if torch.is_tensor(pd_.rep) else pd_.rep
    for d in range(N_DRAWS):
        m = pd_.rt_matrix(d)
        assert isinstance(m, RTMatrix) and m is pd_.rt_matrix(d)
        assert np.shares_memory(m._rep_host, base[d]) and not np.shares_memory(m._rep_host, base[(d + 1) % N_DRAWS])
        np.testing.assert_array_equal(m._rep_host, rep[d])
    with pytest.raises(IndexError):
        pd_.rt_matrix(N_DRAWS)
    with pytest.raises(ValueError):
        PosteriorDraws(rep[0], CELLS, CHR, START)
    with pytest.raises(ValueError):
        PosteriorDraws(rep, CELLS[:-1], CHR, START, device="cpu")
    with pytest.raises(ValueError):
        PosteriorDraws(rep, CELLS, CHR, START, cn=rep[:2], device="cpu")


def test_frac_rt_and_cell_table(draws):
    pd_, rep = draws
    f = pd_.frac_rt()
    assert f.shape == (N_DRAWS, N) and f.dtype == np.float32
    np.testing.assert_array_equal(f, np.stack([m.cell_fractions() for m in _mats(rep)]))
    np.testing.assert_array_equal(f, (rep.sum(1).astype(np.float32) / np.float32(L)))
    t = pd_.cell_table(q=Q)
    assert list(t.columns) == ["cell_id", "clone_id", "frac_rt_mean", "frac_rt_q5", "frac_rt_q50", "frac_rt_q95"]
    assert list(t["cell_id"]) == list(CELLS) and list(t["clone_id"]) == list(CLONES)
    f64 = f.astype(np.float64)
    np.testing.assert_array_equal(t["frac_rt_mean"].to_numpy(), f64.mean(0))
    for q in Q:
        np.testing.assert_array_equal(t["frac_rt_q{:g}".format(100 * q)].to_numpy(), np.quantile(f64, q, axis=0))
    assert (t["frac_rt_q5"] <= t["frac_rt_q50"]).all() and (t["frac_rt_q50"] <= t["frac_rt_q95"]).all()
    assert (t["frac_rt_q5"] < t["frac_rt_q95"]).any()
    assert list(pd_.cell_table(q=()).columns) == ["cell_id", "clone_id", "frac_rt_mean"]


def test_pseudobulk(draws):
    pd_, rep = draws
    t = pd_.pseudobulk(q=Q)
    order = np.lexsort((START, CHR))
    assert list(t["chr"]) == list(CHR[order]) and list(t["start"]) == list(START[order])
    pbs = [m.pseudobulk() for m in _mats(rep)]
    groups = {"pseudobulk": (lambda p: p["population"][0], np.ones(N, bool))}
    for c in ("A", "B"):
        groups["pseudobulk_clone" + c] = ((lambda p, c=c: p["clones"][c][0]), CLONES == c)
    cols = ["chr", "start"]
    for name, (get, sel) in groups.items():
        per_draw = np.stack([get(p) for p in pbs]).astype(np.float64)                     # the RTMatrix path
        plain = np.stack([rep[d][order][:, sel].astype(np.float32).mean(1) for d in range(N_DRAWS)])
        np.testing.assert_array_equal(per_draw, plain.astype(np.float64))                 # plain numpy
        np.testing.assert_array_equal(t[name + "_mean"].to_numpy(), per_draw.mean(0))
        for q in Q:
            np.testing.assert_array_equal(t["{}_q{:g}".format(name, 100 * q)].to_numpy(),
                                          np.quantile(per_draw, q, axis=0))
        cols += [name + "_mean"] + ["{}_q{:g}".format(name, 100 * q) for q in Q]
    assert list(t.columns) == cols
    # without clones: the population alone
    t0 = PosteriorDraws(rep, CELLS, CHR, START, device="cpu").pseudobulk(q=(0.5,))
    assert list(t0.columns) == ["chr", "start", "pseudobulk_mean", "pseudobulk_q50"]
    np.testing.assert_array_equal(t0["pseudobulk_mean"].to_numpy(), t["pseudobulk_mean"].to_numpy())


@pytest.mark.parametrize("curve,kw", [("linear", {}), ("linear", dict(by="clone", per_cell=True)), ("sigmoid", {})])
def test_twidth(draws, curve, kw):
    pd_, rep = draws
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # curve_fit's covariance warning on few points
        t = pd_.twidth(curve=curve, **kw)
        want = [m.twidth(curve=curve, **kw) for m in _mats(rep)]
    n_par = 2 if curve == "linear" else 3
    assert list(t.columns) == ["draw", "t_width", "right_time", "left_time"] + ["popt_%d" % i for i in range(n_par)]
    assert list(t["draw"]) == list(range(N_DRAWS))
    for d, (t_width, right_time, left_time, popt, _, _) in enumerate(want):
        np.testing.assert_array_equal(t.loc[d, ["t_width", "right_time", "left_time"]].to_numpy(np.float64),
                                      np.array([t_width, right_time, left_time], np.float64))
        np.testing.assert_array_equal(t.loc[d, ["popt_%d" % i for i in range(n_par)]].to_numpy(np.float64),
                                      np.asarray(popt, np.float64))
    assert t["t_width"].nunique() > 1                         # the draws differ, and so do their T-widths
