"""rt_profiles on the host: the DataFrame layer against fixtures the reference's own
compute_pseudobulk_rt_profiles.py / calculate_twidth.py produced (bit for bit: values, dtypes,
column names, row order), the matrix layer (chunked numpy path) against the DataFrame layer,
the curve fits against scipy called as the reference calls it, and the import shims."""
import numpy as np
import pandas as pd
import pytest
import scipy
from scipy.optimize import curve_fit

from scdna_replication_tools_amd import rt_profiles as rt
from tests._rt_cases import FRAC, QUERY, STATE, TFS, assert_frame_is, assert_hist_is, golden, same_bits, table


def merged_with_tfs(case):
    cn = table(case)
    merged = pd.merge(cn, rt.compute_pseudobulk_rt_profiles(cn, STATE))
    out = rt.compute_time_from_scheduled_column(merged, pseudobulk_col="pseudobulk_hours", frac_rt_col=FRAC,
                                                tfs_col=TFS)
    assert out is merged                                       # in place, as the reference
    return merged


@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_frame_layer_equals_reference(case):
    z = golden()
    assert_frame_is(rt.compute_pseudobulk_rt_profiles(table(case), STATE), case + "_pb")
    merged = merged_with_tfs(case)
    assert same_bits(merged[TFS].to_numpy(), z[case + "_tfs"])
    assert_hist_is(rt.calc_pct_replicated_per_time_bin(merged, tfs_col=TFS, rs_col=STATE), case + "_hist")


def test_cases_cover_what_they_claim():
    z = golden()
    assert z["A_tfs"].dtype == np.float32 and z["B_tfs"].dtype == np.float64
    assert len(z["A_pb_col0"]) == 64 and len(z["C_pb_col0"]) == 61          # the inner merge lost clone B's loci
    names = list(z["D_pb_columns"])
    assert np.isnan(z["D_pb_col%d" % names.index("pseudobulk_cloneB_hours")]).all()
    assert not np.isnan(z["D_pb_col%d" % names.index("pseudobulk_hours")]).any()
    assert list(z["A_pb_col0"][:2]) == ["1", "1"] and z["A_pb_col0"][-1] == "10"


def test_calc_population_rt_columns_and_order():
    cn = table("C")
    got = rt.calc_population_rt(cn, STATE, "avg", time_col="t", chr_col="chr", start_col="start")
    assert list(got.columns) == ["chr", "start", "avg", "t"]
    assert got["avg"].dtype == np.float32 and got["t"].dtype == np.float32
    keys = list(zip(got["chr"], got["start"]))
    assert keys == sorted(keys) and len(keys) == 64
    # a column of arbitrary floats takes numpy's own mean per locus
    cn["x"] = np.random.default_rng(0).normal(size=len(cn)).astype(np.float32)
    got = rt.calc_population_rt(cn, "x", "avg")
    want = [np.mean(g["x"].values) for _, g in cn.groupby(["chr", "start"])]
    assert same_bits(got["avg"].to_numpy(), np.asarray(want, np.float32))


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_interval_edges_equal_reference(name):
    z = golden()
    df = pd.DataFrame({TFS: z["E_%s_tfs" % name], STATE: z["E_%s_state" % name],
                       "cell_id": z["E_%s_cell_id" % name].astype(object)})
    assert_hist_is(rt.calc_pct_replicated_per_time_bin(df, tfs_col=TFS, rs_col=STATE), "E_%s_hist" % name)
    assert_hist_is(rt.calc_pct_replicated_per_time_bin(df, tfs_col=TFS, rs_col=STATE, per_cell=True),
                   "E_%s_hist_cell" % name)


def test_query_and_per_cell_equal_reference():
    merged = merged_with_tfs("A")
    kw = dict(tfs_col=TFS, rs_col=STATE)
    assert_hist_is(rt.calc_pct_replicated_per_time_bin(merged, query2=QUERY, **kw), "F_query")
    assert_hist_is(rt.calc_pct_replicated_per_time_bin(merged, per_cell=True, **kw), "F_cell")
    assert_hist_is(rt.calc_pct_replicated_per_time_bin(merged, per_cell=True, query2=QUERY, **kw), "F_cell_query")


def _scipy_fit(curve, x, y):
    """scipy called as the reference calls it (calculate_twidth.py:84-87, :104-107)."""
    if curve == "sigmoid":
        popt, _ = curve_fit(rt.sigmoid, x, y, [np.median(x), 1, 0.0], method="dogbox")
        lo, hi = rt.inv_sigmoid(0.25, *popt), rt.inv_sigmoid(0.75, *popt)
    else:
        popt, _ = curve_fit(rt.linear, x, y, [-1.0, -1.0])
        lo, hi = rt.inv_linear(0.25, *popt), rt.inv_linear(0.75, *popt)
    return popt, (lo - hi, hi, lo)          # what the reference's caller names t_width, right_time, left_time


@pytest.mark.parametrize("curve", ["sigmoid", "linear"])
@pytest.mark.parametrize("per_cell", [False, True])
def test_calculate_twidth(curve, per_cell):
    z = golden()
    key = "G_{}_{}".format(curve, "cell" if per_cell else "agg")
    t_width, right_time, left_time, popt, time_bins, pct_reps = rt.calculate_twidth(
        merged_with_tfs("A"), tfs_col=TFS, rs_col=STATE, per_cell=per_cell, curve=curve)
    assert_hist_is((time_bins, pct_reps), key)
    want_popt, want_times = _scipy_fit(curve, list(z[key + "_time_bins"]), list(z[key + "_pct_reps"]))
    assert same_bits(np.asarray(popt), np.asarray(want_popt))
    assert same_bits(np.array([t_width, right_time, left_time]), np.array(want_times))
    if scipy.__version__ == str(z["scipy_version"]):            # another scipy may end its optimiser elsewhere
        np.testing.assert_allclose(popt, z[key + "_popt"], rtol=1e-8)
        np.testing.assert_allclose([t_width, right_time, left_time], z[key + "_times"], rtol=1e-8)


def test_t_width_helpers_return_order():
    popt = [0.5, -1.2, 0.01]
    t_width, left_time, right_time = rt.calc_t_width(popt)
    assert left_time == rt.inv_sigmoid(0.75, *popt) and right_time == rt.inv_sigmoid(0.25, *popt)
    assert t_width == right_time - left_time
    np.testing.assert_allclose(rt.sigmoid(rt.inv_sigmoid(0.3, *popt), *popt), 0.3, rtol=1e-12)
    t_width, left_time, right_time = rt.calc_linear_t_width([-0.1, 0.5])
    assert (left_time, right_time) == (rt.inv_linear(0.75, -0.1, 0.5), rt.inv_linear(0.25, -0.1, 0.5))
    assert rt.linear(rt.inv_linear(0.3, -0.1, 0.5), -0.1, 0.5) == pytest.approx(0.3)


# ---- matrix layer, host path -------------------------------------------------------------------

def _matrix(case, **kw):
    return rt.RTMatrix.from_frame(table(case), rs_col=STATE, device="cpu", **kw)


@pytest.mark.parametrize("case", ["A", "B", "D"])
def test_matrix_equals_frame_layer(case):
    z = golden()
    m = _matrix(case)
    assert (m.L, m.N) == (64, 40) and list(m.clones) == ["A", "B"]
    frame = rt.compute_pseudobulk_rt_profiles(table(case), STATE)
    got = m.pseudobulk_frame(STATE)
    assert list(got.columns) == list(frame.columns)
    for c in frame.columns:
        assert got[c].dtype == frame[c].dtype and same_bits(got[c].to_numpy(), frame[c].to_numpy()), c
    assert_frame_is(got, case + "_pb")
    frac_dtype = np.float64 if case == "B" else np.float32
    cn = table(case)
    first = cn.drop_duplicates("cell_id").set_index("cell_id")[FRAC]
    if case != "D":                                            # D's table keeps A's fraction column
        assert same_bits(m.cell_fractions(frac_dtype), first.loc[list(m.cell_ids)].to_numpy())
        assert_hist_is(m.tfs_histogram(frac_dtype=frac_dtype), case + "_hist")
    merged = pd.merge(cn, frame)
    merged[FRAC] = pd.Series(m.cell_fractions(frac_dtype), index=m.cell_ids).loc[merged["cell_id"]].to_numpy()
    rt.compute_time_from_scheduled_column(merged, "pseudobulk_hours", FRAC, TFS)
    for per_cell in (False, True):
        want = rt.calc_pct_replicated_per_time_bin(merged, tfs_col=TFS, rs_col=STATE, per_cell=per_cell)
        assert m.tfs_histogram(per_cell=per_cell, frac_dtype=frac_dtype) == want


def test_matrix_query_per_cell_and_clone_hours():
    m = _matrix("A")
    chr1 = m.chr == "1"
    assert_hist_is(m.tfs_histogram(loci=chr1), "F_query")
    assert_hist_is(m.tfs_histogram(per_cell=True), "F_cell")
    assert_hist_is(m.tfs_histogram(per_cell=True, loci=np.flatnonzero(chr1)), "F_cell_query")
    # each cell against its own clone's profile, and a subset of cells, against the frame layer
    cn = table("A")
    merged = pd.merge(cn, rt.compute_pseudobulk_rt_profiles(cn, STATE))
    merged["own"] = np.where(merged["clone_id"] == "A", merged["pseudobulk_cloneA_hours"],
                             merged["pseudobulk_cloneB_hours"]).astype(np.float32)
    rt.compute_time_from_scheduled_column(merged, "own", FRAC, TFS)
    assert m.tfs_histogram(by="clone") == rt.calc_pct_replicated_per_time_bin(merged, tfs_col=TFS, rs_col=STATE)
    some = ["cell_03", "cell_30", "cell_31"]
    want = rt.calc_pct_replicated_per_time_bin(merged, tfs_col=TFS, rs_col=STATE, per_cell=True,
                                               query2="cell_id in {}".format(some))
    assert m.tfs_histogram(by="clone", per_cell=True, cells=some) == want
    t_width = m.twidth(curve="sigmoid")[0]
    assert t_width == rt.calculate_twidth(merged_with_tfs("A"), tfs_col=TFS, rs_col=STATE)[0]


def test_matrix_rows_in_any_order_and_chunked(monkeypatch):
    cn = table("A")
    base = _matrix("A")
    perm = np.random.default_rng(1).permutation(base.L)
    rep = cn[STATE].to_numpy().reshape(64, 40)                 # the fixture's table is bin-major
    assert (rep == base._rep_host).all()
    monkeypatch.setattr(rt, "_CHUNK_ELEMS", 40 * 5)            # 5 bins per chunk: 13 chunks
    m = rt.RTMatrix(rep[perm], base.cell_ids, base.chr[perm], base.start[perm], clone_ids=base.clone_ids,
                    device="cpu")
    assert_frame_is(m.pseudobulk_frame(STATE), "A_pb")
    assert_hist_is(m.tfs_histogram(), "A_hist")
    assert_hist_is(m.tfs_histogram(per_cell=True), "F_cell")


def test_from_frame_rejects_bad_tables():
    with pytest.raises(ValueError, match="full bins x cells grid"):
        rt.RTMatrix.from_frame(table("C"), rs_col=STATE, device="cpu")
    cn = table("A")
    cn.loc[5, STATE] = 2.0
    with pytest.raises(ValueError, match="other than 0 and 1"):
        rt.RTMatrix.from_frame(cn, rs_col=STATE, device="cpu")
    cn = table("A")
    cn = pd.concat([cn.iloc[1:], cn.iloc[[7]]], ignore_index=True)      # right size, one pair twice
    with pytest.raises(ValueError, match="full bins x cells grid"):
        rt.RTMatrix.from_frame(cn, rs_col=STATE, device="cpu")


def test_shims_expose_reference_names():
    from scdna_replication_tools import calculate_twidth as tw
    from scdna_replication_tools import compute_pseudobulk_rt_profiles as pb
    for name in ("calc_population_rt", "compute_pseudobulk_rt_profiles"):
        assert getattr(pb, name) is getattr(rt, name)
    for name in ("compute_time_from_scheduled_column", "calc_pct_replicated_per_time_bin", "sigmoid", "inv_sigmoid",
                 "fit_sigmoid", "calc_t_width", "linear", "inv_linear", "fit_linear", "calc_linear_t_width",
                 "plot_cell_variability", "calculate_twidth", "compute_and_plot_twidth"):
        assert getattr(tw, name) is getattr(rt, name)


def test_plot_runs_headless():
    import matplotlib
    matplotlib.use("Agg")
    ax, t_width = rt.compute_and_plot_twidth(merged_with_tfs("A"), tfs_col=TFS, rs_col=STATE)
    assert t_width == pytest.approx(float(golden()["G_sigmoid_agg_times"][0]), rel=1e-6)
    assert ax.get_xlabel().startswith("time from scheduled")


def test_native_entry_points_validate_before_launching():
    """PERT_E_ARG without a GPU: bad strides, too many groups or edges, counters that could wrap."""
    from scdna_replication_tools_amd import _native as nat
    lib, p = nat.lib(), 4096                                   # a 16-byte aligned non-null address, never read
    assert lib.pert_rt_counts(10, 20, 16, 1, p, p, p, p, None) == 1             # ldn < N
    assert lib.pert_rt_counts(10, 20, 40, 1, p, p, p, p, None) == 1             # ldn not a multiple of 16
    assert lib.pert_rt_counts(10, 20, 32, 1, p + 4, p, p, p, None) == 1         # rows not 16-byte aligned
    assert lib.pert_rt_counts(10, 20, 32, 0, p, p, p, p, None) == 1
    assert lib.pert_rt_counts(10, 20, 32, 1, p, p, None, p, None) == 1
    hist = lambda L, N, ldn, G, n_edges, per_cell: lib.pert_rt_tfs_hist(L, N, ldn, G, p, p, p, p, p, n_edges, 0,
                                                                        per_cell, p, p, None)
    assert hist(1 << 16, 1 << 16, 1 << 16, 1, 201, 0) == 1                      # L N = 2^32
    assert hist(10, 20, 32, nat.RT_MAX_GROUPS + 1, 201, 0) == 1
    assert hist(10, 20, 32, 1, nat.RT_MAX_EDGES + 1, 0) == 1
    assert hist(10, 20, 32, 1, 1, 0) == 1
    assert hist(10, 20, 32, 1, 201, 3) == 1
