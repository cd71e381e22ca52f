"""Elementwise error bound of the posterior marginals (test infrastructure).

The posterior over the 2P joint states of one (bin, cell) is gamma = softmax(s) of the joint
scores, and a marginal is p = sum_{s in A} gamma_s.  A score error ds moves it, to first order,
by sum_s gamma_s (1[s in A] - p) ds_s, so an fp32 evaluation whose scores are within E_s of the
exact ones satisfies, per element,

    |p_dev - p64| <= sum_s gamma_s |1[s in A] - p64| E_s + (2P + 4) eps32.

E_s is the per-score fp32 bound ``tests/_bounds.decode_mismatches`` uses (c = 8, nb_rel = 5e-6,
the same terms); gamma and p64 are fp64.  The additive term covers the roundings of the two
sequential sums over the 2P exponentials, the reciprocal and the product.  The bound is derived,
not tuned: nothing in it comes from the code under test.
"""
from __future__ import annotations

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
SCORE_C = 8.0            # decode_mismatches' c
NB_REL = 5e-6            # decode_mismatches' nb_rel


def score_error(lp_cn, lp_rep, nbp, delta, dpsi, c: float = SCORE_C, nb_rel: float = NB_REL):
    """E_s of every joint state (broadcast of the terms): decode_mismatches' expression."""
    a = lambda v: np.abs(np.asarray(v, np.float64))
    nbp = a(nbp)
    return c * EPS32 * (a(lp_cn) + a(lp_rep) + nbp + a(delta) * a(dpsi)) + nb_rel * np.maximum(nbp, 1.0)


def additive(P: int) -> float:
    return (2 * P + 4) * EPS32


def marginals(score, E):
    """score, E: (2, P, ...) fp64.  Returns the fp64 marginals and their bounds:
    dict(gamma (2, P, ...), p_rep (...), p_cn (P, ...), b_rep (...), b_cn (P, ...))."""
    score = np.asarray(score, np.float64)
    E = np.broadcast_to(np.asarray(E, np.float64), score.shape)
    P = score.shape[1]
    flat = score.reshape((2 * P,) + score.shape[2:])
    g = np.exp(flat - flat.max(0, keepdims=True))
    g = (g / g.sum(0, keepdims=True)).reshape(score.shape)
    p_rep = g[1].sum(0)
    p_cn = g[0] + g[1]
    gE = g * E
    tot = gE.sum((0, 1))                                   # sum_s gamma_s E_s
    in_rep = gE[1].sum(0)
    b_rep = in_rep * (1.0 - p_rep) + (tot - in_rep) * p_rep + additive(P)
    in_cn = gE[0] + gE[1]                                  # (P, ...)
    b_cn = in_cn * (1.0 - p_cn) + (tot[None] - in_cn) * p_cn + additive(P)
    return dict(gamma=g, p_rep=p_rep, p_cn=p_cn, b_rep=b_rep, b_cn=b_cn, E=E)


def oracle_marginals(prob, z):
    """``marginals`` of an oracle problem at the point z: gamma = softmax(oracle.enum_scores) in
    fp64, E_s from oracle.enum_score_terms -- arrays over (L, N)."""
    from oracle import pert_oracle as po
    with torch.no_grad():
        t = po.enum_score_terms(prob, z)
    nbp = (t["lp_reads"] - t["kappa"]).numpy()
    score = t["score"].numpy()
    E = score_error(np.broadcast_to(t["lp_cn"].numpy(), score.shape), np.broadcast_to(t["lp_rep"].numpy(), score.shape),
                    nbp, t["delta"].numpy(), t["dpsi"].numpy())
    return marginals(score, E)


def check(name: str, dev, ref, bound) -> float:
    """Largest |dev - ref| / bound (<= 1 passes); raises naming the worst element."""
    dev = np.asarray(dev, np.float64).reshape(np.shape(ref))
    ratio = np.abs(dev - ref) / bound
    worst = float(ratio.max()) if ratio.size else 0.0
    if not np.isfinite(dev).all() or worst > 1.0:
        i = np.unravel_index(int(np.nanargmax(np.where(np.isfinite(ratio), ratio, np.inf))), ratio.shape)
        raise AssertionError("{}: |delta| / bound = {:.3g} at {} (dev {:.9g}, fp64 {:.9g}, bound {:.3g})".format(
            name, worst, i, dev[i], ref[i], bound[i]))
    return worst
