"""Posterior marginals of the enumerated states without a GPU: the per-element arithmetic
(pert_math.h enum_posterior, compiled for the host) against fp64 torch within the derived
bound of tests/_post_bounds.py, its tie to the hot path's responsibilities, the argument
checks of pert_enum_posterior, and the two output columns of package_s_output.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from tests import _post_bounds as pb

EPS32 = pb.EPS32
LAM = 0.75


@pytest.fixture(scope="module")
def nat():
    from scdna_replication_tools_amd import build, _native
    build.build()
    _native.lib()
    return _native


def _inputs(P, n=300):
    """The input ranges of test_enum_cellbin_host_matches_autograd, plus rows with x = 0, with
    D < 1 and 1 <= D < kAsymMin = 3, with phi outside [0.001, 0.999] and with one logit + 40
    (fp32 pi rounds to 1: both clamps of log pi~ bind)."""
    rng = np.random.default_rng(100 + P)
    x = rng.integers(0, 400, n).astype(np.float32)
    st = rng.integers(0, P, n)
    z = (rng.normal(size=(n, P)) * 2).astype(np.float32)
    z[np.arange(n), st] += 5
    D = rng.uniform(0.3, 60, n).astype(np.float32)
    phi = rng.uniform(0.0002, 0.9998, n).astype(np.float32)
    x[0:40:4] = 0
    D[0:20] = rng.uniform(0.05, 1.0, 20).astype(np.float32)
    D[20:40] = rng.uniform(1.0, 3.0, 20).astype(np.float32)
    x[40:60] = rng.integers(0, 12, 20).astype(np.float32)          # few reads at any D
    phi[60:70] = rng.uniform(0.0, 0.001, 10).astype(np.float32)
    phi[70:80] = rng.uniform(0.999, 1.0, 10).astype(np.float32)
    z[80:100, :] = (rng.normal(size=(20, P)) * 0.5).astype(np.float32)
    z[np.arange(80, 100), st[80:100]] += 40
    assert (D < 1).sum() >= 20 and ((D >= 1) & (D < 3)).sum() >= 20 and (x == 0).sum() >= 10
    return x, z, D, phi


def _reference(P, x, z, D, phi):
    """fp64 torch, as test_enum_cellbin_host_matches_autograd builds its reference: scores
    (2, P, n) and their fp32 error E_s.  log pi~ is log(clamp(pi, eps32, 1 - eps32)): the model
    is defined by the reference's fp32 run, whose Categorical clamps at the fp32 eps (an fp64
    Categorical would clamp at 2.2e-16 and describe another model where pi < 1.2e-7).
    The threshold is not copied from the code under test: it is torch's own clamp_probs
    (torch/distributions/utils.py: eps = finfo(probs.dtype).eps, applied by Categorical's
    probs_to_logits, categorical.py:67-71) at the dtype the reference runs in, float32
    (pert_model.py:156-166 builds float32 tensors); EPS32 here is numpy's finfo(float32).eps."""
    assert EPS32 == torch.finfo(torch.float32).eps
    from torch.distributions import Bernoulli, NegativeBinomial
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    zt, Dt, pt, X = t64(z), t64(D), t64(phi), t64(x)
    pi = torch.softmax(zt, -1)
    lp_cn = torch.log(pi.clamp(EPS32, 1.0 - EPS32)).T.reshape(1, P, -1)
    phic = pt.clamp(0.001, 0.999)
    cn = torch.arange(P).reshape(P, 1)
    rep = torch.tensor([0., 1.], dtype=torch.float64).reshape(2, 1, 1)
    lp_rep = Bernoulli(phic).log_prob(rep)                          # (2, 1, n)
    delta = cn * (1 + rep) * Dt
    clamped = delta < 1
    delta = torch.where(clamped, torch.ones_like(delta), delta)
    lam = torch.tensor(LAM, dtype=torch.float64)
    lp_reads = NegativeBinomial(delta, probs=lam).log_prob(X)       # (2, P, n)
    xlx = torch.where(X > 0, X * torch.log(torch.where(X > 0, X, torch.ones_like(X))), torch.zeros_like(X))
    kappa = X * np.log(LAM) + xlx - X - torch.lgamma(1 + X)
    dpsi = torch.where(clamped, torch.zeros_like(delta),
                       torch.log1p(-lam) + torch.digamma(delta + X) - torch.digamma(delta))
    score = (lp_cn + lp_rep + lp_reads).numpy()
    E = pb.score_error(np.broadcast_to(lp_cn.numpy(), score.shape), np.broadcast_to(lp_rep.numpy(), score.shape),
                       (lp_reads - kappa).numpy(), delta.numpy(), dpsi.numpy())
    return pb.marginals(score, E), phic.numpy()


@pytest.mark.parametrize("P", [13, 5, 2])
def test_enum_posterior_host_matches_fp64(nat, P):
    x, z, D, phi = _inputs(P)
    out = nat.selftest_enum_posterior_host(P, x, z, np.log1p(-LAM), D, phi)
    ref, _ = _reference(P, x, z, D, phi)
    r_rep = pb.check("p_rep", out["p_rep"], ref["p_rep"], ref["b_rep"])
    r_cn = pb.check("p_cn", out["p_cn"].T, ref["p_cn"], ref["b_cn"])
    print("P={}: worst |delta| / bound  rep {:.3f}  cn {:.3f}; median bound {:.3g}".format(
        P, r_rep, r_cn, float(np.median(ref["b_rep"]))))
    p_cn = out["p_cn"].astype(np.float64)
    assert np.abs(p_cn.sum(1) - 1.0).max() <= pb.additive(P)
    for v in (out["p_rep"], out["p_cn"]):
        assert np.isfinite(v).all() and v.min() >= 0.0 and v.max() <= 1.0
    # the test has power: uncertain elements exist, and the bound is far below them
    assert ((ref["p_rep"] > 0.01) & (ref["p_rep"] < 0.99)).mean() > 0.1
    assert np.median(ref["b_rep"]) < 1e-4


@pytest.mark.parametrize("P", [13, 5, 2])
def test_posterior_ties_to_the_hot_path_responsibilities(nat, P):
    """Where the phi mask is open, enum_forward's gt (the hot path's d E / d t / a) is
    sum_c gamma(c, 1) - clamp(phi) = p_rep - phi.  gt carries its own fp32 score rounding, so the
    two sides are compared within the derived bound plus (2P + 4) eps32, not to a few ulp."""
    x, z, D, phi = _inputs(P)
    n = x.size
    em1 = np.zeros((n, P), np.float32)
    fwd = nat.selftest_enum_cellbin_host(P, x, em1, em1.sum(1), z, np.log1p(-LAM), D, phi)
    out = nat.selftest_enum_posterior_host(P, x, z, np.log1p(-LAM), D, phi)
    ref, phic = _reference(P, x, z, D, phi)
    open_ = (phi >= 0.001) & (phi <= 0.999)
    assert open_.sum() > 200 and (~open_).sum() >= 10
    got = out["p_rep"].astype(np.float64) - phi.astype(np.float64)
    bound = ref["b_rep"] + pb.additive(P)
    d = np.abs(fwd["gt"].astype(np.float64) - got)
    assert (d[open_] <= bound[open_]).all(), float((d[open_] / bound[open_]).max())
    assert (fwd["gt"][~open_] == 0).all()                # masked there: not the posterior


@pytest.mark.parametrize("P", [2, 5, 13, 16])
def test_joint_argmax_carries_its_share_of_the_posterior(nat, P):
    """The decode's joint argmax a = r* P + c* (enum_forward) and the marginals (enum_posterior)
    come from one score: the largest of 2P softmax weights is at least 1 / (2P), and each
    marginal that contains the argmax state is at least that weight, less the (P + 2) eps32 of
    the normalisation (sum_k p_cn[k] = 1 within that much)."""
    x, z, D, phi = _inputs(P)
    n = x.size
    em1 = np.zeros((n, P), np.float32)
    fwd = nat.selftest_enum_cellbin_host(P, x, em1, em1.sum(1), z, np.log1p(-LAM), D, phi)
    out = nat.selftest_enum_posterior_host(P, x, z, np.log1p(-LAM), D, phi)
    a = fwd["argmax"]
    assert a.min() >= 0 and a.max() < 2 * P
    c, r = a % P, a // P
    assert (r == 1).any() and (r == 0).any() and np.unique(c).size > 1
    floor = 1.0 / (2 * P) - (P + 2) * 2.0 ** -23
    p_c = out["p_cn"].astype(np.float64)[np.arange(n), c]
    p_rep = out["p_rep"].astype(np.float64)
    p_r = np.where(r == 1, p_rep, 1.0 - p_rep)
    assert (p_c >= floor).all(), (float(p_c.min()), floor)
    assert (p_r >= floor).all(), (float(p_r.min()), floor)


def _problem(nat, **kw):
    d = dict(kind=2, L=10, N=10, P=13, K1=5, n_libs=1, ldn=256)
    d.update(kw)
    return nat.PertProblem(**d)


def test_enum_posterior_abi_and_argument_checks(nat):
    """Both names are exported and every argument error returns before any launch (no GPU
    here): the pointers below are host buffers that are never dereferenced."""
    assert {"pert_enum_posterior", "pert_selftest_enum_posterior_host"} <= set(nat.EXPORTED_SYMBOLS)
    lib = nat.lib()
    assert hasattr(lib, "pert_enum_posterior") and hasattr(lib, "pert_selftest_enum_posterior_host")
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    st = nat.PertState(params=p, z_pi=p)
    call = lambda pr, cs, rp, cp, cm: lib.pert_enum_posterior(ctypes.byref(pr), ctypes.byref(st), cs, rp, cp, cm, None)
    good = dict(reads=p, gcf=p)
    E_ARG, E_P, E_K = 1, 2, 3
    assert call(_problem(nat, **good), p, None, p, None) == E_ARG              # null rep_prob
    assert call(_problem(nat, **good), None, p, p, None) == E_ARG              # cn_prob without cn_state
    assert call(_problem(nat, **good), p, p, None, None) == E_ARG              # cn_state without cn_prob
    assert call(_problem(nat, kind=1, **good), p, p, p, None) == E_ARG         # step 1
    assert call(_problem(nat, P=17, **good), p, p, p, None) == E_P
    assert call(_problem(nat, P=1, **good), p, p, p, None) == E_P
    assert call(_problem(nat, K1=9, **good), p, p, p, None) == E_K
    assert call(_problem(nat, L=0, **good), p, p, p, None) == E_ARG
    assert call(_problem(nat, ldn=100, **good), p, p, p, None) == E_ARG        # not a multiple of PERT_BLOCK
    assert call(_problem(nat, N=300, **good), p, p, p, None) == E_ARG          # ldn < N
    assert call(_problem(nat, N=0, **good), p, p, p, None) == E_ARG
    assert call(_problem(nat), p, p, p, None) == E_ARG                         # null reads / gcf
    assert call(_problem(nat, kind=3, **good), p, p, p, None) == E_ARG         # step 3 without rho_fixed
    assert lib.pert_enum_posterior(None, ctypes.byref(st), None, p, None, None, None) == E_ARG
    assert lib.pert_selftest_enum_posterior_host(17, 0, None, None, 0.0, None, None, None, None) == E_P


def _tables(seed=6):
    from tests.test_reference_boundary import _model
    m, s, g = _model(seed=seed)
    cn_s_reads_df = m.process_input_data()[2]
    L, N = cn_s_reads_df.shape
    rng = np.random.default_rng(1)
    tr = {"cn": rng.integers(0, 13, (L, N)), "rep": rng.integers(0, 2, (L, N)).astype(np.float32),
          "expose_tau": rng.uniform(size=N).astype(np.float32), "expose_u": rng.uniform(50, 90, N).astype(np.float32),
          "expose_rho": rng.uniform(size=(L, 1)).astype(np.float32), "expose_a": np.array([7.5], np.float32)}
    post = {"rep_prob": rng.uniform(size=(L, N)).astype(np.float32),
            "cn_prob": rng.uniform(size=(L, N)).astype(np.float32)}
    return m, cn_s_reads_df, tr, post


def _expected(out, df, a, cell_col="cell_id"):
    """a (loci x cells) looked up per output row through the frame's own labels."""
    ci = pd.Index(np.asarray(df.columns).astype(str)).get_indexer(out[cell_col].astype(str).to_numpy())
    li = pd.MultiIndex.from_arrays([np.asarray(df.index.get_level_values(0)).astype(str),
                                    np.asarray(df.index.get_level_values(1))]).get_indexer(
        pd.MultiIndex.from_arrays([out["chr"].astype(str).to_numpy(), out["start"].to_numpy()]))
    assert (ci >= 0).all() and (li >= 0).all()
    return a[li, ci]


def test_package_s_output_posterior_columns():
    from scdna_replication_tools_amd.pert_model import MapTrace, PivotAxes
    m, df, tr, post = _tables()
    lam, lg, ls = np.array([0.71], np.float32), [3.0, 2.0], [9.0]
    inp = m._prepare()
    axes = PivotAxes(inp.loci_chr, inp.loci_start, inp.cells_s, keys=inp.keys_s)
    assert inp.keys_s.is_grid(np.asarray(axes.columns), np.asarray(axes.index.get_level_values(0)).astype(str),
                              np.asarray(axes.index.get_level_values(1)))
    base, bsupp = m.package_s_output(m.cn_s, MapTrace(**tr), axes, lam, lg, ls)
    # the grid path
    got, gsupp = m.package_s_output(m.cn_s, MapTrace(**tr, **post), axes, lam, lg, ls)
    assert list(got.columns) == list(base.columns) + ["model_rep_prob", "model_cn_prob"]
    pd.testing.assert_frame_equal(got[list(base.columns)], base)
    pd.testing.assert_frame_equal(gsupp, bsupp)
    for node, col in (("rep_prob", "model_rep_prob"), ("cn_prob", "model_cn_prob")):
        assert got[col].dtype == np.float32
        np.testing.assert_array_equal(got[col].to_numpy(), _expected(got, df, post[node]))
    # the indexed path: shuffled rows, some removed, located through the frame's labels
    sub = m.cn_s.sample(frac=0.8, random_state=3)
    assert len(sub) < len(m.cn_s)
    base2, _ = m.package_s_output(sub, MapTrace(**tr), df, lam, lg, ls)
    got2, _ = m.package_s_output(sub, MapTrace(**{k: torch.as_tensor(v) for k, v in {**tr, **post}.items()}), df,
                                 lam, lg, ls)
    assert len(got2) == len(sub)
    assert list(got2.columns) == list(base2.columns) + ["model_rep_prob", "model_cn_prob"]
    pd.testing.assert_frame_equal(got2[list(base2.columns)], base2)
    for node, col in (("rep_prob", "model_rep_prob"), ("cn_prob", "model_cn_prob")):
        assert got2[col].dtype == np.float32
        np.testing.assert_array_equal(got2[col].to_numpy(), _expected(got2, df, post[node]))
    np.testing.assert_array_equal(got2["model_cn_state"].to_numpy(), _expected(got2, df, tr["cn"]))
    # without the nodes: today's columns, in today's order
    assert list(base.columns) == list(m.cn_s.columns) + ["model_cn_state", "model_rep_state", "model_tau", "model_u",
                                                         "model_rho"]


def test_constructor_takes_posterior_keyword_only():
    import inspect
    from scdna_replication_tools_amd.pert_model import pert_infer_scRT
    p = inspect.signature(pert_infer_scRT.__init__).parameters["posterior"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert list(inspect.signature(pert_infer_scRT.__init__).parameters)[-1] == "posterior"
