"""The reference's compute_ccc_features outputs (tests/golden/ccc_reference.npz, written by
tests/golden/make_ccc_reference_golden.py from the reference's own module) and the comparisons the
CPU and GPU tests share."""
import os
import warnings

import numpy as np
import pandas as pd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ccc_reference.npz")
FEATURE_CASES = ("A_alone", "B", "C", "D", "E", "F")     # calculate_features alone
IN_COLS = ["cell_id", "chr", "start", "rpm_clone_norm", "state", "clone_id"]

# Tolerances, as tests/_bin_cases.py sets them: the measured worst difference, times 64 for the
# kernel's other, fixed summation order; anything above 1e-9 would mean something other than
# rounding differs.
#
# score1, score2 and lrs are compared scaled by |score1| + |score2| (lrs is a difference of the
# two and sits near 0 for a unimodal cell: a test relative to lrs itself is meaningless).  The
# worst such difference of the kernel from per-cell sklearn fed the same draws, on the unflagged
# cells of cases A, B, D, E and the 5,451-bin genome case in the kernel's first run on an MI355X,
# was 7.2e-15 (score2 of case A; lrs 4.9e-15 there, 2.6e-15 at genome length).  The host path's
# own difference from the golden is 0 (it makes sklearn's calls on the reference's stream).
MEASURED_WORST_SCORE = 7.2e-15
SCORE_TOL = 64 * MEASURED_WORST_SCORE
# rpm_clone_norm, total_mapped_reads_hmmcopy and corrected_madn against the golden on the CPU:
# equal bit for bit (the same pandas / numpy / sklearn calls on the same values), so the floor of
# one rounding of each, 2^-52, stands in as the measured value.
MEASURED_WORST_REL = 2.0 ** -52
RTOL = 64 * MEASURED_WORST_REL
assert SCORE_TOL < 1e-9 and RTOL < 1e-9

_npz = None


def golden():
    global _npz
    if _npz is None:
        _npz = np.load(GOLDEN)
    return _npz


def frame(key: str, base: pd.DataFrame = None) -> pd.DataFrame:
    """A stored frame.  The columns the generator found equal to its input's (``<key>_same``)
    come from ``base``, at the stored row positions when the frame holds a subset of its rows."""
    g = golden()
    cols, dtypes = list(g[key + "_columns"]), list(g[key + "_dtypes"])
    same = set(g[key + "_same"]) if key + "_same" in g else set()
    if key + "_rows" in g:
        base = base.iloc[g[key + "_rows"]]
    data = {}
    for i, (c, dt) in enumerate(zip(cols, dtypes)):
        v = base[c].to_numpy() if c in same else g["{}_col{}".format(key, i)]
        data[c] = v.astype(object) if dt == "object" else v.astype(dt)
    index = pd.RangeIndex(int(g[key + "_index_range"])) if key + "_index_range" in g else pd.Index(g[key + "_index"])
    return pd.DataFrame(data, index=index)[cols]


def table(case: str) -> pd.DataFrame:
    """The case's input table, as the generator passed it to the reference."""
    if case == "A_alone":
        return frame("A_cn_out", table("A"))[IN_COLS].copy()
    if case == "H":
        return table("A")[golden()["H_keep"]].reset_index(drop=True)
    return frame(case + "_in")


def seed(case: str) -> int:
    return int(golden()[case + "_seed"])


def groups(case: str):
    """The input of ``features_matrix`` per profile length of a calculate_features case: a list of
    (the cells' places in sorted-cell order, X, state, chromosome codes), the three (L, N)."""
    from scdna_replication_tools_amd import ccc_features as F
    t = table(case)
    _, order, offs = F._cells(t, "cell_id")
    x, st = t["rpm_clone_norm"].to_numpy(), t["state"].to_numpy()
    ch = pd.factorize(t["chr"].to_numpy())[0]
    return [(sel, np.ascontiguousarray(x[pos].T), st[pos].T, ch[pos].T) for _, sel, pos in F._by_length(order, offs)]


def n_cells(case: str) -> int:
    return table(case)["cell_id"].nunique()


def sklearn_cells(X: np.ndarray, stream) -> dict:
    """Per-cell sklearn on the stream's draws (ccc_features.exact_scores: GaussianMixture(1) and
    GaussianMixture(2) on a private RandomState placed at the cell's draws) and numpy's median,
    for every column of X."""
    from scdna_replication_tools_amd import ccc_features as F
    rs_at = stream.walker()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sc = np.array([F.exact_scores(X[:, n], rs_at(int(stream.index[n]))) for n in range(X.shape[1])])
    return dict(score1=sc[:, 0], score2=sc[:, 1], lrs=sc[:, 2], madn=np.median(np.abs(np.diff(X, axis=0)), axis=0))


def score_diff(got: dict, ref: dict, ok=None) -> dict:
    """Worst |difference| of score1, score2 and lrs, scaled by |score1| + |score2| of the reference."""
    ok = slice(None) if ok is None else ok
    scale = (np.abs(ref["score1"]) + np.abs(ref["score2"]))[ok]
    return {k: float(np.max(np.abs(got[k][ok] - ref[k][ok]) / scale)) for k in ("score1", "score2", "lrs")}


def closed_form_score1(x: np.ndarray) -> float:
    """GaussianMixture(1).fit(x).score(x): the mean log density at the M step of all-one
    responsibilities (the scale of the lrs comparison, from the profile alone)."""
    nk = x.size + 10 * np.finfo(np.float64).eps
    mean = x.sum() / nk
    var = ((x - mean) ** 2).sum() / nk + 1e-6
    return float(np.mean(-0.5 * (np.log(2 * np.pi) + (x - mean) ** 2 / var) - 0.5 * np.log(var)))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(d == 0, 0.0, d / np.abs(b)))) if a.size else 0.0


def assert_frame_is(got: pd.DataFrame, want: pd.DataFrame, what="", profiles: pd.DataFrame = None,
                    norm_col="rpm_clone_norm"):
    """A result frame against the reference's: columns, order, dtypes and index equal; every
    column equal, except lrs (within SCORE_TOL of the reference's, scaled by |score1| + |score2|
    of the cell's profile) and rpm_clone_norm / total_mapped_reads_hmmcopy / corrected_madn
    (within RTOL).  ``profiles``: the frame that holds the cells' profiles when ``want`` does not
    (cell_features).  Returns the worst differences."""
    assert list(got.columns) == list(want.columns), (what, list(got.columns))
    assert [str(got[c].dtype) for c in got.columns] == [str(want[c].dtype) for c in want.columns], what
    assert got.index.equals(want.index), what
    worst = {}
    for c in want.columns:
        g, w = got[c].to_numpy(), want[c].to_numpy()
        if c == "lrs":
            prof = want if profiles is None else profiles
            s1 = prof.groupby("cell_id")[norm_col].agg(lambda s: closed_form_score1(s.to_numpy()))
            s1 = want["cell_id"].map(s1).to_numpy()
            scale = np.abs(s1) + np.abs(s1 + w / 2)
            worst[c] = float(np.max(np.abs(g - w) / scale))
            assert worst[c] <= SCORE_TOL, (what, c, worst[c])
        elif c in (norm_col, "total_mapped_reads_hmmcopy", "corrected_madn") and w.dtype.kind == "f":
            worst[c] = rel(g, w)
            assert worst[c] <= RTOL, (what, c, worst[c])
        elif w.dtype.kind == "f":
            np.testing.assert_array_equal(g, w, err_msg="{} {}".format(what, c))
        else:
            assert (g == w).all(), (what, c)
    print(what, "worst differences", worst)
    return worst
