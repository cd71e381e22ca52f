"""Shared by tests/test_cell_level.py and tests/test_gpu_cpd.py: the reference fixture of the cell
level (tests/golden/cell_level_reference.npz, made by make_cell_level_reference_golden.py), an
independent triple-loop oracle of the change-point search, and the search's test profiles."""
import functools
import os

import numpy as np
import pandas as pd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_level_reference.npz")
# normalize_by_cell against the reference.  Every column is the reference's bit for bit: the same
# numpy / sklearn operations in the same order.  G1_match_pearsonr alone goes through a BLAS dot
# product (scipy's pearsonr), whose summation order is the BLAS build's: it is held to the bound of a
# sum of a few hundred unit-scale fp64 terms (eps * L ~ 1e-13) with two to three orders of margin.
RTOL, ATOL = 1e-10, 1e-12


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(GOLDEN))


def frame(fx, key):
    cols = [str(c) for c in fx[key + "_columns"]]
    data = {}
    for i, (c, dt) in enumerate(zip(cols, fx[key + "_dtypes"])):
        v = fx["{}_col{}".format(key, i)]
        data[c] = v.astype(object) if str(dt) == "object" else v.astype(str(dt))
    return pd.DataFrame(data, index=fx[key + "_index"])[cols]


VARIANT_COLS = ("start", "cell_id", "G1_match_cell_id", "changepoint_segments", "rt_value")


def variants(cn_s, cn_g1):
    """Edge cases made from the fixture's tables (the generator records the reference's result for the
    same tables): a G1/2 cell whose rows name two clones, S rows on a chromosome outside 1..22, X, Y,
    and tables without a clone column."""
    g2 = cn_g1.copy()
    cell = g2["cell_id"].iloc[0]
    rows = np.flatnonzero((g2["cell_id"] == cell).to_numpy())[:50]
    other = [c for c in g2["clone_id"].unique() if c != g2["clone_id"].iloc[0]][0]
    g2.loc[rows, "clone_id"] = other
    s2 = cn_s.copy()
    s2.loc[s2.index[100:104], "chr"] = "MT"
    return {"mixed": (cn_s, g2), "MT": (s2, cn_g1), "noclone": (cn_s.drop(columns="clone_id"), cn_g1)}


def check_against_reference(out, fx):
    """The comparison of both the CPU and the device test: names, order, dtypes, rows, then values."""
    want = frame(fx, "out")
    assert list(out.columns) == list(want.columns)
    assert [str(out[c].dtype) for c in out.columns] == [str(d) for d in fx["out_dtypes"]]
    assert len(out) == len(want) and (out.index.to_numpy() == want.index.to_numpy()).all()
    for c in want.columns:
        a, b = out[c].to_numpy(), want[c].to_numpy()
        if c == "G1_match_pearsonr":
            np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, err_msg=c)
        else:
            assert (a == b).all(), c


def triple_loop(y, mode):
    """The definition, candidate by candidate in Python floats: (a, b, gain), the first maximum."""
    n = len(y)
    S = [0.0]
    for v in y:
        S.append(S[-1] + float(v))
    best = (-1, -1, 0.0)
    found = False
    if mode == 2:
        for a in range(2, n - 3):
            for b in range(a + 2, n - 1):
                g = (S[a] * S[a]) * (1.0 / a) + ((S[b] - S[a]) * (S[b] - S[a])) * (1.0 / (b - a))
                g = g + ((S[n] - S[b]) * (S[n] - S[b])) * (1.0 / (n - b))
                if not found or g > best[2]:
                    best, found = (a, b, g), True
    else:
        for a in range(2, n - 1):
            g = (S[a] * S[a]) * (1.0 / a) + ((S[n] - S[a]) * (S[n] - S[a])) * (1.0 / (n - a))
            if not found or g > best[2]:
                best, found = (a, n, g), True
    return best


def noisy_steps(rng, n, n_steps=2):
    """A unit-noise profile with a few level shifts."""
    y = rng.standard_normal(n)
    for _ in range(n_steps):
        lo = int(rng.integers(0, max(n - 2, 1)))
        y[lo:lo + int(rng.integers(2, max(n // 3, 3)))] += rng.choice([-2.0, 1.5, 3.0])
    return y


def ragged(profiles):
    """(Y (N, ld) zero padded, lens int32) of a list of profiles."""
    lens = np.array([len(p) for p in profiles], dtype=np.int32)
    Y = np.zeros((len(profiles), int(lens.max())))
    for i, p in enumerate(profiles):
        Y[i, :len(p)] = p
    return Y, lens


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)
