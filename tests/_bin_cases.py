"""The reference's binarisation and clone-normalisation outputs (tests/golden/binarize_reference.npz,
written by tests/golden/make_binarize_reference_golden.py from the reference's own functions)
and the comparisons the CPU and GPU tests share."""
import os

import numpy as np
import pandas as pd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binarize_reference.npz")
CASES = ("A", "B", "C", "D", "E", "F")
OUT_COLS = ["mean_0", "covariance_0", "mean_1", "covariance_1", "gmm_state", "rt_state", "frac_rt", "binary_thresh"]
# The worst relative difference of the CPU tensor program (no host path) from the reference on
# cases A-F is 3.8e-14 (a mean of case B; covariances 1.8e-14 and distances 1.6e-14, both case
# E: DESIGN.md section 6h); the tests grant 64 times that for the kernel's other, fixed
# summation order.  Anything above 1e-9 would mean something other than rounding differs.
MEASURED_WORST_REL = 3.8e-14
RTOL = 64 * MEASURED_WORST_REL
assert RTOL < 1e-9

_npz = None


def golden():
    global _npz
    if _npz is None:
        _npz = np.load(GOLDEN)
    return _npz


def table(case: str) -> pd.DataFrame:
    """The case's input table: cell_id (object) and x (float64), in the fixture's row order."""
    g = golden()
    return pd.DataFrame({"cell_id": g[case + "_cell_id"].astype(object), "x": g[case + "_x"]})


def matrix(case: str) -> np.ndarray:
    """(L, N) float64 matrix of a case whose cells all have one length, columns in sorted-cell
    order (the cases' tables are grouped by cell already)."""
    t = table(case)
    cells = pd.unique(t["cell_id"])
    assert list(cells) == sorted(cells)
    L = len(t) // len(cells)
    return np.ascontiguousarray(t["x"].to_numpy().reshape(len(cells), L).T)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


def assert_profiles_are(case: str, cn: pd.DataFrame, man: pd.DataFrame, rtol: float = RTOL):
    """``binarize_profiles``' two frames against the reference's: columns, order and dtypes, the
    discrete columns and frac_rt equal on every row, the continuous ones within rtol, and the
    distance table's layout."""
    g = golden()
    assert list(cn.columns) == list(g[case + "_columns"])
    assert [str(cn[c].dtype) for c in cn.columns] == list(g[case + "_dtypes"])
    for c in ("gmm_state", "rt_state", "binary_thresh", "frac_rt"):
        np.testing.assert_array_equal(cn[c].to_numpy(), g["{}_{}".format(case, c)], err_msg=case + " " + c)
    worst = {}
    for c in ("mean_0", "mean_1", "covariance_0", "covariance_1"):
        worst[c] = rel(cn[c].to_numpy(), g["{}_{}".format(case, c)])
    assert list(man.columns) == list(g[case + "_man_columns"])
    assert [str(man[c].dtype) for c in man.columns] == list(g[case + "_man_dtypes"])
    np.testing.assert_array_equal(man.index.to_numpy(), g[case + "_man_index"])
    np.testing.assert_array_equal(man["thresh"].to_numpy(), g[case + "_man_thresh"])
    np.testing.assert_array_equal(man["cell_id"].to_numpy().astype("U"), g[case + "_man_cell_id"])
    np.testing.assert_array_equal(man["best_thresh"].to_numpy(), g[case + "_man_best_thresh"])
    worst["manhattan_dist"] = rel(man["manhattan_dist"].to_numpy(), g[case + "_man_manhattan_dist"])
    print("case", case, "worst relative differences", worst)
    assert max(worst.values()) <= rtol, worst
    return worst


def sklearn_cells(X: np.ndarray):
    """The per-cell restatement (binarize.exact_cell: sklearn's GaussianMixture, scipy's skew,
    numpy's percentiles and sums) of every column of X, stacked like ``binarize_matrix``'s result."""
    import warnings
    from scdna_replication_tools_amd import binarize as B
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ex = [B.exact_cell(X[:, n]) for n in range(X.shape[1])]
    return dict(means=np.array([e[0] for e in ex]), covariances=np.array([e[1] for e in ex]),
                gmm_state=np.array([e[2] for e in ex]).T, rt_state=np.array([e[3] for e in ex]).T.astype(np.uint8),
                manhattan=np.array([e[4] for e in ex]), best=np.array([e[5] for e in ex]))


def simulated_ratio(L: int, N: int, seed: int) -> np.ndarray:
    """(L, N) float64: simulated S-phase reads over the G1/2 pseudobulk median, the bulk level's
    own input."""
    from scdna_replication_tools_amd import simulator
    sim = simulator.simulate(N, N, n_bins=L, seed=seed)
    return sim.reads_s.astype(np.float64) / np.median(sim.reads_g.astype(np.float64), axis=1)[:, None]
