"""Error bounds of the likelihood curve over tau (test infrastructure).

With the fp64 oracle terms of one (bin, cell) (oracle.enum_score_terms), the part of a joint score
that tau does not enter is ``base = lp_cn + (lp_reads - kappa)`` and the branch evidences are
``e_r = logsumexp_c base[r]``.

Element bound.  A score error ds moves a logsumexp by sum_c softmax_c ds_c, so an fp32 evaluation
whose scores are within E of the exact ones gives

    |e_r,dev - e_r| <= B_r = sum_c softmax_c(base[r]) E + (P + 6) eps32 + 3 eps32 |e_r|

E is ``_post_bounds.score_error`` with the lp_rep argument 0 (the Bernoulli term is not part of
these scores); the additive terms cover the P exponentials and their sequential sum, the logarithm
and the final addition.

Bound on m.  m = log((1 - phi) e^{e_0} + phi e^{e_1}) has d m / d e_r = the posterior weight of
branch r, so with gamma_1 the fp64 weight of the replicated branch

    |m_dev - m| <= (1 - gamma_1) (B_0 + 8 eps32 |log(1 - phi)|) + gamma_1 (B_1 + 8 eps32 |log phi|)
                   + 6 eps32 + eps32 |m|

(8 eps32 |log .|: the c = 8 of score_error on the Bernoulli term, which covers the fp32 phi).
Cell bound: the sum of the m bound over the bins.

The bounds are derived, not tuned: nothing here comes from the code under test.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import _post_bounds as pb

EPS32 = pb.EPS32
DEFAULT_GRID = np.linspace(0.01, 0.99, 99).astype(np.float32)


def logsumexp0(a):
    mx = a.max(0)
    return mx + np.log(np.exp(a - mx[None]).sum(0))


def evidence_from_terms(lp_cn, nbp, delta, dpsi):
    """lp_cn (P, ...) and nbp, delta, dpsi (2, P, ...) fp64 -> e (2, ...) and B (2, ...)."""
    nbp = np.asarray(nbp, np.float64)
    base = np.asarray(lp_cn, np.float64)[None] + nbp
    P = base.shape[1]
    E = pb.score_error(np.broadcast_to(np.asarray(lp_cn)[None], base.shape), 0.0, nbp, delta, dpsi)
    e = np.stack([logsumexp0(base[r]) for r in (0, 1)])
    w = np.exp(base - e[:, None])                              # softmax_c per branch
    B = (w * E).sum(1) + (P + 6) * EPS32 + 3 * EPS32 * np.abs(e)
    return e, B


def oracle_evidence(prob, z):
    """The oracle problem at the point z: dict(e (2, L, N), B (2, L, N), a, rho (L,), tau (N,))
    in fp64, computed once and never modified."""
    from oracle import pert_oracle as po
    with torch.no_grad():
        t = po.enum_score_terms(prob, z)
        c = po.constrain(prob.kind, z)
    e, B = evidence_from_terms(t["lp_cn"].numpy(), (t["lp_reads"] - t["kappa"]).numpy(), t["delta"].numpy(),
                               t["dpsi"].numpy())
    a = c["expose_a"] if prob.kind != "step3" else prob.a_fixed
    rho = c["expose_rho"] if prob.kind != "step3" else prob.rho_fixed
    out = dict(e=e, B=B, a=float(np.asarray(a).reshape(-1)[0]), rho=np.asarray(rho, np.float64).reshape(-1),
               tau=np.asarray(c["expose_tau"], np.float64).reshape(-1))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def phi_of(a, tau, rho):
    """clamp(1 / (1 + exp(-a (tau - rho))), 0.001, 0.999) in fp64; tau and rho broadcast."""
    return np.clip(1.0 / (1.0 + np.exp(-a * (np.asarray(tau, np.float64) - np.asarray(rho, np.float64)))),
                   0.001, 0.999)


def mix(e0, e1, phi):
    """fp64 m = log((1 - phi) e^{e0} + phi e^{e1}) and gamma_1, the replicated branch's weight."""
    b0 = np.asarray(e0, np.float64) + np.log1p(-phi)
    b1 = np.asarray(e1, np.float64) + np.log(phi)
    m = np.logaddexp(b0, b1)
    return m, np.exp(b1 - m)


def mix_bound(B0, B1, phi, m, g1):
    return ((1.0 - g1) * (B0 + 8 * EPS32 * np.abs(np.log1p(-phi))) + g1 * (B1 + 8 * EPS32 * np.abs(np.log(phi)))
            + 6 * EPS32 + EPS32 * np.abs(m))


def curve(ev, taus):
    """The oracle's curve and its cell bound: ``taus`` (G,), one value of tau per row for every
    cell, or (G, N), a value per row and cell -> two (G, N) arrays."""
    e, B = ev["e"], ev["B"]
    taus = np.asarray(taus, np.float64)
    rho = ev["rho"][:, None]                                    # (L, 1)
    rows, bounds = [], []
    for t in taus:
        phi = phi_of(ev["a"], t, rho)                           # (L, 1) or (L, N)
        phi = np.broadcast_to(phi, e[0].shape)
        m, g1 = mix(e[0], e[1], phi)
        rows.append(m.sum(0))
        bounds.append(mix_bound(B[0], B[1], phi, m, g1).sum(0))
    return np.stack(rows), np.stack(bounds)


def curve_at(ev, tau_cells):
    """The curve at one tau per cell: (N,) value and bound."""
    c, b = curve(ev, np.asarray(tau_cells, np.float64).reshape(1, -1))
    return c[0], b[0]


def sharpness(ev):
    """Per cell: the largest cell bound over the default grid divided by the curve's range over
    it.  From the oracle alone; the check is sharp where this is small."""
    c, b = curve(ev, DEFAULT_GRID.astype(np.float64))
    return b.max(0) / (c.max(0) - c.min(0))
