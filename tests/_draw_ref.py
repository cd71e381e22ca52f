"""The check of posterior draws against the fp64 oracle (test infrastructure).

A draw of one (bin, cell) is the first joint state j (j = 2 cn + rep) whose inclusive CDF value
exceeds the element's uniform.  The fp64 side: gamma from ``tests/_post_bounds`` (the oracle's
softmax of the joint scores, re-ordered to j), its prefix sums F_j, and the uniform from the
independent Philox of ``tests/_sim_ref`` under the documented counter rule.  A CDF prefix
{0..j} is a marginal like any other, so ``_post_bounds``' elementwise bound applies to it:

    b_j = in_A (1 - F_j) + (tot - in_A) F_j + additive(P) + 2 eps32,
    in_A = sum_{s <= j} gamma_s E_s,   tot = sum_s gamma_s E_s,

the last term for the fp32 product u S.  Three conditions, none of which uses anything from the
code under test:

* per draw: F_{j-1} - b_{j-1} <= u < F_j + b_j at the device's j (F_{-1} = b_{-1} = 0);
* a state with gamma below 2^-149 (2P) -- its fp32 weight is zero -- is never drawn;
* the share of draws that differ from the fp64 draw (the first j with u < F_j) is at most
  ``CAP``: the bound excuses a draw only next to a CDF edge, so a large share is a failure the
  per-draw condition would hide, not rounding.
"""
from __future__ import annotations

import numpy as np

from tests import _post_bounds as pb
from tests import _sim_ref as sr

TAG_DRAWS = 3
CAP = 0.01
ZERO_WEIGHT = 2.0 ** -149


def joint_order(a):
    """(2, P, ...) in the oracle's (rep, cn) layout -> (2P, ...) with j = 2 cn + rep."""
    a = np.asarray(a)
    return np.swapaxes(a, 0, 1).reshape((2 * a.shape[1],) + a.shape[2:])


def uniforms(seed, bins, cells, first_draw, n_draws):
    """The fp32 uniforms of draws first_draw .. first_draw + n_draws - 1 of the elements
    (bins, cells) (broadcast; cells are GLOBAL indices): word g & 3 of draw round g >> 2 of the
    stream PERT_TAG_DRAWS.  float32 (n_draws, ...)."""
    out = []
    words = {}
    for g in range(first_draw, first_draw + n_draws):
        if g >> 2 not in words:
            words = {g >> 2: sr.draw(seed, TAG_DRAWS, bins, cells, g >> 2)}
        out.append(sr.uniform32(words[g >> 2][..., g & 3]))
    return np.stack(out)


def prefix(ref):
    """From ``_post_bounds.marginals`` / ``oracle_marginals`` output: gamma (2P, ...) in joint
    order, F (2P, ...) its inclusive prefix sums and b (2P, ...) their bounds, all fp64."""
    g = joint_order(ref["gamma"]).astype(np.float64)
    P = g.shape[0] // 2
    gE = g * joint_order(ref["E"])
    F = np.cumsum(g, axis=0)
    in_a = np.cumsum(gE, axis=0)
    tot = gE.sum(axis=0)
    b = in_a * (1.0 - F) + (tot[None] - in_a) * F + pb.additive(P) + 2.0 * pb.EPS32
    return g, F, b


def check(name, ref, u, j_dev):
    """ref: ``_post_bounds`` marginals of the elements (...); u float32 and j_dev integer
    (n_draws, ...).  Asserts the three conditions and returns the share of draws that differ from
    the fp64 draw."""
    g, F, b = prefix(ref)
    n_states = g.shape[0]
    j_dev = np.asarray(j_dev).astype(np.int64)
    u = np.asarray(u, np.float64)
    assert j_dev.shape == u.shape and u.shape[1:] == g.shape[1:], (j_dev.shape, u.shape, g.shape)
    assert j_dev.min() >= 0 and j_dev.max() < n_states, (name, int(j_dev.min()), int(j_dev.max()))
    pad = lambda a: np.concatenate([np.zeros((1,) + a.shape[1:]), a])          # index j -> value at j - 1
    take = lambda a, j: np.take_along_axis(a, j, axis=0)
    lo = take(pad(F), j_dev) - take(pad(b), j_dev)
    hi = take(F, j_dev) + take(b, j_dev)
    bad = ~((lo <= u) & (u < hi))
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("{}: {} of {} draws outside their bounded CDF interval; first at {}: j {} u {:.9g} "
                             "not in [{:.9g}, {:.9g})".format(name, int(bad.sum()), bad.size, i, j_dev[i], u[i], lo[i],
                                                              hi[i]))
    zero = take(g, j_dev) < ZERO_WEIGHT * n_states
    assert not zero.any(), "{}: {} draws of a state whose weight is zero".format(name, int(zero.sum()))
    j64 = (F[None] <= u[:, None]).sum(axis=1)                # the first j with u < F_j
    j64 = np.minimum(j64, n_states - 1)
    share = float((j64 != j_dev).mean())
    assert share <= CAP, "{}: {:.3%} of the draws differ from the fp64 draw (cap {:.0%})".format(name, share, CAP)
    return share
