"""Threshold binarisation of RT profiles, clone normalisation and scRT's bulk level on the CPU,
against the reference's own outputs (tests/golden/binarize_reference.npz)."""
import ctypes
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

from scdna_replication_tools_amd import binarize as B
from tests import _bin_cases as C


def test_import_paths():
    from scdna_replication_tools.binarize_rt_profiles import binarize_profiles
    from scdna_replication_tools.normalize_by_clone import cell_clone_norm, normalize_by_clone
    assert binarize_profiles is B.binarize_profiles
    assert normalize_by_clone is B.normalize_by_clone and cell_clone_norm is B.cell_clone_norm


@pytest.mark.parametrize("case", C.CASES)
def test_profiles_match_reference(case, capsys):
    t = C.table(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # sklearn's convergence warnings, as in the reference
        cn, man = B.binarize_profiles(t, "x", device="cpu")
    assert cn is t                                            # written in place, like the reference
    assert "cell_skew" not in capsys.readouterr().out         # the reference's prints are not made
    C.assert_profiles_are(case, cn, man)


def test_case_b_takes_all_three_percentile_branches():
    from scipy.stats import skew
    X = C.matrix("B")
    res = B.binarize_matrix(X, device="cpu")
    assert (np.abs(res.means[:, 0] - res.means[:, 1]) < 0.7).all()
    sk = np.array([skew(X[:, n]) for n in range(X.shape[1])])
    assert (sk > 0.2).sum() >= 10 and (sk < -0.2).sum() >= 10 and ((sk >= -0.2) & (sk <= 0.2)).sum() >= 10


def test_one_sided_cells_take_the_first_threshold():
    res = B.binarize_matrix(C.matrix("F"), device="cpu")
    assert (res.best_thresh == -3.0).all()
    np.testing.assert_array_equal(res.frac_rt, np.r_[np.ones(8), np.zeros(8)])
    assert not res.flagged.any()                              # equal distances of one binarisation are no near-tie


@pytest.mark.parametrize("case", ["A", "C"])
def test_tensor_program_flags_at_most_a_tenth(case):
    """The cap on flagged cells (the margins are not so wide that the host path does the work),
    and the tensor program alone, before the host path, already equals the reference."""
    X = C.matrix(case)
    res = B.binarize_matrix(X, device="cpu", exact=False)
    assert res.flagged.mean() <= 0.10, res.flags
    g = C.golden()
    L, N = X.shape
    ok = ~res.flagged
    np.testing.assert_array_equal(res.rt_state.T[ok], g[case + "_rt_state"].reshape(N, L)[ok])
    np.testing.assert_array_equal(res.gmm_state.T[ok], g[case + "_gmm_state"].reshape(N, L)[ok])
    np.testing.assert_array_equal(res.best_thresh[ok], g[case + "_binary_thresh"].reshape(N, L)[ok, 0])


def test_matrix_result_and_input_checks():
    X = C.matrix("C")
    res = B.binarize_matrix(torch.from_numpy(X), device="cpu")
    L, N = X.shape
    assert res.means.shape == (N, 2) and res.covariances.shape == (N, 2) and res.manhattan.shape == (N, 100)
    assert res.gmm_state.shape == (L, N) and res.rt_state.shape == (L, N) and res.flagged.shape == (N,)
    np.testing.assert_array_equal(res.thresholds, np.linspace(-3, 3, 100))
    np.testing.assert_array_equal(res.frac_rt, res.rt_state.sum(0) / L)
    np.testing.assert_array_equal(res.rt_state, X > res.best_thresh[None, :])
    np.testing.assert_array_equal(res.manhattan.argmin(1), np.searchsorted(res.thresholds, res.best_thresh))
    with pytest.raises(TypeError):
        B.binarize_matrix(X.astype(np.float32), device="cpu")
    bad = X.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError):
        B.binarize_matrix(bad, device="cpu")
    t = C.table("C")
    t.loc[5, "x"] = np.inf
    with pytest.raises(ValueError):
        B.binarize_profiles(t, "x", device="cpu")


def test_existing_columns_are_overwritten_and_thresholds_passed():
    t = C.table("C")
    t["rt_state"] = 7
    t["mean_1"] = "old"
    cn, _ = B.binarize_profiles(t, "x", device="cpu")
    assert list(cn.columns) == ["cell_id", "x", "rt_state", "mean_1", "mean_0", "covariance_0", "covariance_1",
                                "gmm_state", "frac_rt", "binary_thresh"]
    assert cn["rt_state"].dtype == np.float64 and cn["mean_1"].dtype == np.float64
    np.testing.assert_array_equal(cn["rt_state"].to_numpy(), C.golden()["C_rt_state"])
    # a mean-gap threshold above every cell's gap sends every cell to the percentile levels
    ref, _ = B.binarize_profiles(C.table("C"), "x", device="cpu")
    pct, _ = B.binarize_profiles(C.table("C"), "x", 'rt_state', 'frac_rt', 'binary_thresh', 'cell_id', 10.0, 0.2, -0.2,
                                 device="cpu")
    np.testing.assert_array_equal(pct["mean_0"].to_numpy(), ref["mean_0"].to_numpy())
    X = C.matrix("C")
    ex = [B.exact_cell(X[:, n], 10.0) for n in range(X.shape[1])]
    np.testing.assert_array_equal(pct["binary_thresh"].to_numpy().reshape(X.shape[1], -1)[:, 0],
                                  np.linspace(-3, 3, 100)[[e[5] for e in ex]])


def _clone_inputs():
    g = C.golden()
    cn_s = pd.DataFrame({c: (g["G_in_" + c].astype(object) if g["G_in_" + c].dtype.kind == "U" else g["G_in_" + c])
                         for c in g["G_in_columns"]})
    prof = pd.DataFrame(g["G_prof_values"], columns=pd.Index(g["G_prof_columns"].astype(object), name="clone_id"),
                        index=pd.MultiIndex.from_arrays([g["G_prof_chr"].astype(object), g["G_prof_start"]],
                                                        names=["chr", "start"]))
    return cn_s, prof


def test_normalize_by_clone_equals_reference():
    g = C.golden()
    cn_s, prof = _clone_inputs()
    before_s, before_p = cn_s.copy(), prof.copy()
    out = B.normalize_by_clone(cn_s, prof, input_col="reads")
    pd.testing.assert_frame_equal(cn_s, before_s)             # the caller's frames are not modified
    pd.testing.assert_frame_equal(prof, before_p)
    assert list(out.columns) == list(g["G_columns"])
    assert [str(out[c].dtype) for c in out.columns] == list(g["G_dtypes"])
    np.testing.assert_array_equal(out.index.to_numpy(), g["G_index"])
    for i, c in enumerate(out.columns):
        v = out[c].to_numpy()
        np.testing.assert_array_equal(v.astype("U") if v.dtype == object else v, g["G_col{}".format(i)], err_msg=c)
    # the profile handed over with chr / start as columns, as a table read from a file has them
    out2 = B.normalize_by_clone(cn_s, prof.reset_index(), input_col="reads")
    pd.testing.assert_frame_equal(out2, out)
    # one cell through cell_clone_norm
    cell = cn_s[cn_s["cell_id"] == "cell_S_3"].set_index(["chr", "start"])
    one = B.cell_clone_norm(prof.dropna(), cell, cell["clone_id"].iloc[0], "reads", "rt_value")
    want = out[out["cell_id"] == "cell_S_3"].drop(columns="ploidy").reset_index(drop=True)
    pd.testing.assert_frame_equal(one[want.columns], want)


@pytest.fixture(scope="module")
def bulk_tables():
    from scdna_replication_tools_amd import simulator
    sim = simulator.simulate(12, 10, n_bins=96, seed=3, n_clones=2)
    return simulator.to_long_form(sim)


def test_bulk_level_is_the_chain_of_the_three_functions(bulk_tables):
    from scdna_replication_tools.infer_scRT import scRT
    from scdna_replication_tools_amd.infer_scRT import consensus_profiles
    cn_s, cn_g1 = bulk_tables
    cols_s, cols_g = list(cn_s.columns), list(cn_g1.columns)
    obj = scRT(cn_s, cn_g1, device="cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, supp_s, g1_out, supp_g1 = obj.infer(level="bulk")
        bulk = consensus_profiles(cn_g1.assign(dummy_clone_id="1"), "reads", clone_col="dummy_clone_id", cn_state_col=None)
        norm = B.normalize_by_clone(cn_s.assign(dummy_clone_id="1"), bulk, input_col="reads", clone_col="dummy_clone_id",
                                    output_col="rt_value")
        want, man = B.binarize_profiles(norm, "rt_value", device="cpu")
    assert supp_s.empty and g1_out.empty and supp_g1.empty
    assert list(cn_s.columns) == cols_s and list(cn_g1.columns) == cols_g
    pd.testing.assert_frame_equal(obj.bulk_profile, bulk)
    pd.testing.assert_frame_equal(out, want.drop(columns="dummy_clone_id"))
    pd.testing.assert_frame_equal(obj.manhattan_df, man)
    assert out is obj.cn_s and "dummy_clone_id" not in out.columns
    assert set(out["rt_state"].unique()) <= {0.0, 1.0} and 0.0 < out["frac_rt"].mean() < 1.0
    # the bulk-level result flows into the downstream analyses
    pb = obj.compute_pseudobulk_rt_profiles()
    assert "pseduobulk_hours" in pb.columns and obj.bulk_cn is pb
    tw = obj.calculate_twidth(pseudobulk_col="pseduobulk_hours")
    assert len(tw) == 6 and np.isfinite(tw[0])


def test_cell_and_clone_levels_still_raise(bulk_tables):
    from scdna_replication_tools_amd.infer_scRT import scRT
    cn_s, cn_g1 = bulk_tables
    for level in ("cell", "clone"):
        with pytest.raises(NotImplementedError, match="statsmodels.*ruptures"):
            scRT(cn_s, cn_g1).infer(level=level)


def test_native_entry_point_rejects_bad_arguments_without_launching():
    from scdna_replication_tools_amd import _native, build
    build.build()
    lib = _native.lib()
    assert "pert_rt_binarize" in _native.EXPORTED_SYMBOLS and hasattr(lib, "pert_rt_binarize")
    assert ctypes.sizeof(_native.PertBinParams) == 14 * 4 + (5 + 2 + 5 + 100 + 9) * 8
    p = B.bin_params(96)
    buf = (ctypes.c_double * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    args = [ptr] * 8
    call = lambda L, N, x, pp, a: lib.pert_rt_binarize(L, N, x, pp, *a, None)
    assert call(1, 4, ptr, ctypes.byref(p), args) == 1               # PERT_E_ARG: L < 2
    assert call(96, 0, ptr, ctypes.byref(p), args) == 1              # N < 1
    assert call(96, 4, None, ctypes.byref(p), args) == 1             # null input
    assert call(96, 4, ptr, None, args) == 1                         # null parameters
    for k in range(8):
        assert call(96, 4, ptr, ctypes.byref(p), args[:k] + [None] + args[k + 1:]) == 1
    assert call(50, 4, ptr, ctypes.byref(p), args) == 1              # percentile positions of another length
