"""compute_ccc_features on the CPU (the host path serves every cell): the reference's import path,
every golden case of tests/golden/ccc_reference.npz, the random-stream contract, and the C ABI of
pert_ccc_features without a launch."""
import ctypes
import warnings

import numpy as np
import pandas as pd
import pytest

from scdna_replication_tools_amd import ccc_features as F
from tests import _ccc_cases as C


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


def _state_after(start, n_doubles):
    rs = np.random.RandomState()
    rs.set_state(start)
    rs.random_sample(n_doubles)
    return rs.get_state()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_shim_is_the_reference_import_path():
    import scdna_replication_tools.compute_ccc_features as shim
    for name in ("calculate_features", "calculate_breakpoints", "breakpoints", "correct_breakpoints", "correct_madn",
                 "compute_clone_normalization", "compute_read_count", "compute_cell_frac", "compute_ccc_features",
                 "autocorr", "get_args", "main"):
        assert getattr(shim, name) is getattr(F, name), name
    assert shim.breakpoints([2, 2, 3, 3, 2]) == 2


@pytest.mark.parametrize("case", C.FEATURE_CASES)
def test_calculate_features_matches_reference(case):
    """Columns, order, dtypes, index, madn and breakpoints equal, lrs within tolerance; and numpy's
    global generator is left where the reference leaves it: 4 doubles per cell further."""
    t = C.table(case)
    np.random.seed(C.seed(case))
    start = np.random.get_state()
    got = _quiet(F.calculate_features, t.copy(), device="cpu")
    C.assert_frame_is(got, C.frame(case + "_out", t), what=case)
    assert _same_state(np.random.get_state(), _state_after(start, 4 * C.n_cells(case)))


@pytest.mark.parametrize("case", ["A", "G1"])
def test_compute_ccc_features_matches_reference(case):
    t = C.table(case)
    np.random.seed(C.seed(case))
    cn_out, cell_features = _quiet(F.compute_ccc_features, t.copy(), device="cpu")
    want = C.frame(case + "_cn_out", t)
    C.assert_frame_is(cn_out, want, what=case + " cn_out")
    C.assert_frame_is(cell_features, C.frame(case + "_cell_features"), what=case + " cell_features", profiles=want)
    if case == "G1":                                     # the caller's breakpoints are kept
        np.testing.assert_array_equal(cn_out["breakpoints"].to_numpy(), t["breakpoints"].to_numpy())


@pytest.mark.parametrize("key", ["G2", "G2w"])
def test_correct_breakpoints_matches_reference(key):
    """Fractional clone means make the column float64; whole ones leave it int64."""
    t = C.frame(key + "_in")
    C.assert_frame_is(F.correct_breakpoints(t.copy()), C.frame(key + "_out", t), what=key)


def test_clone_normalization_with_missing_rows_matches_reference():
    t = C.table("H")
    want = C.frame("H_out", t)
    assert len(want) < len(t)                            # loci were dropped
    C.assert_frame_is(F.compute_clone_normalization(t.copy()), want, what="H")


def test_breakpoints_of_scattered_chromosomes_and_read_count_and_cell_frac():
    """Whole-column restatements against the per-cell definitions written out here."""
    rng = np.random.default_rng(3)
    n = 400
    t = pd.DataFrame({"cell_id": rng.choice(np.array(["x", "y", "z"], dtype=object), n),
                      "chr": rng.choice(np.array(["1", "2", "X"], dtype=object), n),
                      "state": rng.integers(1, 4, n), "reads": rng.uniform(0, 9, n),
                      "model_rep_state": (rng.uniform(size=n) < np.where(np.arange(n) % 3 == 0, 0.99, 0.5)) * 1.0})
    t.loc[t["cell_id"] == "z", "model_rep_state"] = 1.0
    got = F.compute_cell_frac(F.compute_read_count(F.calculate_breakpoints(t.copy())))
    for cell, rows in t.groupby("cell_id"):
        bk = sum(int((np.diff(r["state"].to_numpy()) != 0).sum()) for _, r in rows.groupby("chr"))
        g = got.loc[rows.index]
        assert (g["breakpoints"] == bk).all()
        np.testing.assert_array_equal(g["total_mapped_reads_hmmcopy"].to_numpy(), rows["reads"].sum())
        frac = rows["model_rep_state"].sum() / len(rows)
        np.testing.assert_array_equal(g["cell_frac_rep"].to_numpy(), frac)
        assert (g["extreme_cell_frac"] == (frac > 0.95 or frac < 0.05)).all()
    assert got["breakpoints"].dtype == np.int64 and got["extreme_cell_frac"].dtype == bool


def test_drawn_stream_reproduces_public_sklearn():
    """The (first2, u) this module derives from a cell's doubles are what public sklearn draws from
    a generator placed there: its KMeans(2, n_init=1) ends at the centres Lloyd reaches from the
    k-means++ centres those draws select (pins the stream on the installed sklearn)."""
    from sklearn.cluster import KMeans, kmeans_plusplus
    (sel, X, state, chrom), = C.groups("B")
    L, N = X.shape
    stream = F._Stream(23, N)
    first = F.first_centres(stream.draws[:, :2].reshape(-1), L).reshape(N, 2)
    rs_at = stream.walker()
    for n in range(N):
        x = X[:, n:n + 1]
        rs = rs_at(n)
        _, i1 = kmeans_plusplus(x, 1, random_state=rs)              # the 1-component fit's draw
        assert i1[0] == first[n, 0]
        before = rs.get_state()
        _, i2 = kmeans_plusplus(x, 2, random_state=rs)              # the 2-component fit's three draws
        assert i2[0] == first[n, 1]
        assert _same_state(rs.get_state(), _state_after(before, 3))
        # the second centre from this module's uniforms: the better of the two trials
        d0 = (x[:, 0] - x[first[n, 1], 0]) ** 2
        cand = np.minimum(np.searchsorted(np.cumsum(d0), stream.draws[n, 2:] * d0.sum()), L - 1)
        pots = [np.minimum(d0, (x[:, 0] - x[c, 0]) ** 2).sum() for c in cand]
        assert i2[1] == cand[int(np.argmin(pots))]


def test_features_matrix_random_state_and_errors():
    (sel, X, state, chrom), = C.groups("B")
    a = _quiet(F.features_matrix, X, state, chrom, random_state=5, device="cpu")
    b = _quiet(F.features_matrix, X, state, chrom, random_state=np.random.RandomState(5), device="cpu")
    for k in ("madn", "lrs", "score1", "score2", "breakpoints"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    assert a.flagged.all() and not a.flags.any()         # the host path served every cell
    np.testing.assert_array_equal(a.lrs, -2 * (a.score1 - a.score2))
    bad = X.copy()
    bad[7, 3] = np.inf
    with pytest.raises(ValueError):
        _quiet(F.features_matrix, bad, random_state=5, device="cpu")
    with pytest.raises(ValueError):
        _quiet(F.features_matrix, X[:1], random_state=5, device="cpu")       # one bin: sklearn's own error
    with pytest.raises(TypeError):
        F.features_matrix(X.astype(np.float32), device="cpu")
    with pytest.raises(TypeError):
        F.features_matrix(X, random_state="seed", device="cpu")
    with pytest.raises(ValueError):
        F.features_matrix(X, state, None, device="cpu")


def test_native_entry_point_rejects_bad_arguments_without_launching():
    from scdna_replication_tools_amd import _native, build
    build.build()
    lib = _native.lib()
    assert "pert_ccc_features" in _native.EXPORTED_SYMBOLS and hasattr(lib, "pert_ccc_features")
    assert ctypes.sizeof(_native.PertCccParams) == 2 * 4 + 6 * 8
    p = F.ccc_params(96)
    assert (p.lloyd_max_iter, p.em_max_iter, p.em_tol, p.reg_covar) == (300, 100, 1e-3, 1e-6)
    buf = (ctypes.c_double * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    # x, first1, first2, u | state, chrom | p | scratch, score1, score2, lrs, madn, breakpoints, flags
    args = [ptr] * 4 + [ptr, ptr] + [ctypes.byref(p)] + [ptr] * 7

    def call(L, N, a):
        return lib.pert_ccc_features(L, N, *a, None)
    assert call(1, 4, args) == 1                                     # PERT_E_ARG: L < 2
    assert call(96, 0, args) == 1                                    # N < 1
    for k in (0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 12, 13):               # each required buffer null
        assert call(96, 4, args[:k] + [None] + args[k + 1:]) == 1, k
    assert call(96, 4, args[:4] + [None, ptr] + args[6:]) == 1       # exactly one of state / chrom
    assert call(96, 4, args[:4] + [ptr, None] + args[6:]) == 1
    for field in ("lloyd_max_iter", "em_max_iter"):
        bad = F.ccc_params(96)
        setattr(bad, field, 0)
        assert call(96, 4, args[:6] + [ctypes.byref(bad)] + args[7:]) == 1, field
