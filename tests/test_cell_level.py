"""The deterministic cell level without a GPU: normalize_by_cell's host path against the reference's
own module (tests/golden/cell_level_reference.npz), the numpy change-point search against an
independent triple loop, scRT.infer_cell_level as the chain of its parts, the C entry point's
argument checks, and the shim's import paths and signatures."""
import ctypes
import inspect
import os
import re
import warnings

import numpy as np
import pandas as pd
import pytest

from scdna_replication_tools_amd import normalize_cell as NC
from tests import _cell_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reference_tables():
    fx = CC.fixture()
    return fx, CC.frame(fx, "in_s"), CC.frame(fx, "in_g")


# ---- normalize_by_cell against the reference

def test_host_path_equals_the_reference_module(reference_tables):
    fx, cn_s, cn_g1 = reference_tables
    before_s, before_g = cn_s.copy(), cn_g1.copy()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)            # the round cap's warning
        out = NC.normalize_by_cell(cn_s, cn_g1, device="cpu")
    CC.check_against_reference(out, fx)
    pd.testing.assert_frame_equal(cn_s, before_s)                 # the caller's frames are left alone
    pd.testing.assert_frame_equal(cn_g1, before_g)


@pytest.mark.parametrize("name", ["mixed", "MT", "noclone"])
def test_edge_cases_equal_the_reference_module(reference_tables, name):
    """A G1/2 cell whose rows name two clones (a candidate with its rows of the clone only), S rows on
    a chromosome outside the category list (in the profile, absent from the result) and tables without
    a clone column (every G1/2 cell is a candidate): the reference's own result for the same tables."""
    fx, cn_s, cn_g1 = reference_tables
    vs, vg = CC.variants(cn_s, cn_g1)[name]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = NC.normalize_by_cell(vs, vg, device="cpu")
    assert list(out.columns) == [str(c) for c in fx["variant_{}_columns".format(name)]]
    assert len(out) != len(CC.frame(fx, "out"))                   # the case does change the result
    for c in CC.VARIANT_COLS:
        want = fx["variant_{}_{}".format(name, c)]
        got = out[c].to_numpy()
        assert len(got) == len(want) and (got.astype(want.dtype) == want).all(), c


def test_fixture_covers_what_it_claims(reference_tables):
    fx, cn_s, cn_g1 = reference_tables
    want = CC.frame(fx, "out")
    assert cn_s["cell_id"].nunique() == 24 and cn_g1["cell_id"].nunique() == 24
    assert set(cn_s["chr"].unique()) == {"1", "2", "X"}
    assert cn_s.groupby("cell_id").size().nunique() > 1           # ragged
    assert cn_s["rpm_gc_norm"].isna().sum() == 1 and cn_g1["rpm_gc_norm"].isna().sum() == 1
    segs = want.groupby("cell_id")["changepoint_segments"].max()
    assert (segs > 0).sum() >= 6 and segs.max() >= 4
    # both loops nominate: an interior segment, one from the start of chr 1 and one to the end of chr X
    first = want.groupby("cell_id").head(1)
    last = want.groupby("cell_id").tail(1)
    assert (first["changepoint_segments"] > 0).any() and (last["changepoint_segments"] > 0).any()
    assert (last["chr"] == "X").all() and (first["chr"] == "1").all()
    # no cell of the committed fixture comes near the round cap, and every decision had a margin
    assert int(fx["round_cap"]) == NC.MAX_ROUNDS and fx["n_searches"].max() < NC.MAX_ROUNDS // 2
    gain, ratio, pval = fx["worst_margins"]
    assert gain > 1e-9 and ratio > 1e-6 and pval > 1e-6
    modes = set(fx["searches"][:, 1].tolist())
    assert modes == {1, 2}


def test_single_cell_functions_are_the_batched_path(reference_tables):
    fx, cn_s, cn_g1 = reference_tables
    want = CC.frame(fx, "out")
    cell = want.loc[want["changepoint_segments"] > 0, "cell_id"].iloc[0]
    w = want[want["cell_id"] == cell].reset_index(drop=True)
    one = w[["chr", "start", "cell_id", "temp_rt"]].sample(frac=1.0, random_state=1)     # unsorted on purpose
    got = NC.remove_cell_specific_CNAs(one, input_col="temp_rt", device="cpu").reset_index(drop=True)
    assert isinstance(got["chr"].dtype, pd.CategoricalDtype)
    assert list(got["chr"].cat.categories) == [str(i + 1) for i in range(22)] + ["X", "Y"]
    for c in ("temp_rt_2", "changepoint_segments", "temp_rt_3", "temp_rt_4", "rt_value"):
        assert (got[c].to_numpy() == w[c].to_numpy()).all(), c
    srt = NC.sort_by_cell_and_loci(one)
    assert (srt["start"].to_numpy() == w["start"].to_numpy()).all()
    srt["temp_rt_2"] = w["temp_rt_2"].to_numpy()
    Y, chng = NC.identify_changepoint_segs(srt, "temp_rt_2", device="cpu")
    assert (Y == w["temp_rt_3"].to_numpy()).all() and (chng == w["changepoint_segments"].to_numpy()).all()
    # g1_cell_norm: the S cell against its recorded match
    match = w["G1_match_cell_id"].iloc[0]
    s_cell = cn_s[cn_s["cell_id"] == cell].dropna().copy()
    g_cell = cn_g1[cn_g1["cell_id"] == match].dropna().copy()
    s_cell["ploidy"] = float(s_cell["state"].mode().min())
    g_cell["ploidy"] = float(g_cell["state"].mode().min())
    norm = NC.g1_cell_norm(s_cell, g_cell, output_col="temp_rt")
    assert list(norm.columns) == ["chr", "start", "cell_id", "temp_rt"]
    norm = NC.sort_by_cell_and_loci(norm)
    assert (norm["temp_rt"].to_numpy() == w["temp_rt"].to_numpy()).all()


def test_round_cap_warns(monkeypatch, reference_tables):
    fx, cn_s, cn_g1 = reference_tables
    monkeypatch.setattr(NC, "MAX_ROUNDS", 2)
    with pytest.warns(RuntimeWarning, match="reached 2 change-point searches"):
        NC.normalize_by_cell(cn_s, cn_g1, device="cpu")


def test_mirror_image_background_and_chromosome_rule():
    """The reference's quirks by hand: Y[~idx] is the mirror image of the region, and in the
    one-breakpoint loop the label AT the breakpoint is left_chr, the one before it right_chr."""
    Y = np.arange(10.0)
    idx = np.arange(2, 5)
    assert (Y[~idx] == np.array([7.0, 6.0, 5.0])).all()              # Y[n - 1 - a] down to Y[n - b]
    rng = np.random.default_rng(3)
    y = rng.standard_normal(60) * 0.05 + 1.0
    y[:12] *= 0.5                                                    # a loss at the start of chr 1
    loop = NC._CellLoop(y, np.array(["1"] * 30 + ["X"] * 30, dtype=object))
    loop.mode = 1
    a, b, _ = NC.cpd_search_host(y, mode=1)
    assert (a[0], b[0]) == (12, 60)
    assert loop.step(12, 60) and (loop.chng[:12] == 1).all() and (loop.chng[12:] == 0).all()
    # the same loss at the start of a cell whose first chromosome is '2' is not touched
    loop = NC._CellLoop(y, np.array(["2"] * 30 + ["X"] * 30, dtype=object))
    loop.mode = 1
    assert not loop.step(12, 60) and loop.done and not loop.chng.any()


# ---- the search's host twin

@pytest.mark.parametrize("n", [6, 7, 12])
@pytest.mark.parametrize("mode", [1, 2])
def test_host_search_equals_the_triple_loop(n, mode):
    rng = np.random.default_rng(100 * n + mode)
    profiles = [CC.noisy_steps(rng, n) for _ in range(6)] + [np.round(rng.integers(0, 3, n)).astype(float)]
    Y, lens = CC.ragged(profiles)
    a, b, g = NC.cpd_search_host(Y, lens, mode=mode)
    for i, p in enumerate(profiles):
        wa, wb, wg = CC.triple_loop(p, mode)
        assert (a[i], b[i]) == (wa, wb) and CC.bits(g[i]) == CC.bits(wg), (i, a[i], b[i], wa, wb)


def test_host_search_ties_steps_and_infeasible():
    a, b, g = NC.cpd_search_host(np.zeros(12))
    assert (a[0], b[0], g[0]) == (2, 4, 0.0)                         # every gain ties: smallest a, then b
    a, b, g = NC.cpd_search_host(np.zeros(12), mode=1)
    assert (a[0], b[0], g[0]) == (2, 12, 0.0)
    y = np.ones(40)
    y[11:23] = 3.0                                                   # a planted step
    a, b, g = NC.cpd_search_host(y)
    assert (a[0], b[0]) == (11, 23) and (a[0], b[0], g[0]) == CC.triple_loop(y, 2)
    a, b, _ = NC.cpd_search_host(y[:23], mode=1)
    assert (a[0], b[0]) == (11, 23)
    # ragged rows, mixed modes, an inactive row, the infeasible lengths
    rng = np.random.default_rng(9)
    Y, lens = CC.ragged([CC.noisy_steps(rng, n) for n in (5, 6, 3, 4, 30, 30)])
    mode = np.array([2, 2, 1, 1, 2, 1], np.int32)
    a, b, g = NC.cpd_search_host(Y, lens, mode, active=[1, 1, 1, 1, 0, 1])
    assert (a[0], b[0], g[0]) == (-1, -1, 0.0) and (a[2], b[2], g[2]) == (-1, -1, 0.0)
    assert (a[1], b[1]) == (2, 4) and (a[3], b[3]) == (2, 4)         # the only candidates
    assert (a[4], b[4]) == (-1, -1) and np.isnan(g[4])               # inactive
    assert (a[5], b[5], g[5]) == CC.triple_loop(Y[5, :30], 1)
    with pytest.raises(ValueError, match="finite"):
        NC.cpd_search_host(np.array([1.0, np.nan, 2.0, 3.0, 1.0, 0.0]))
    with pytest.raises(ValueError, match="modes"):
        NC.cpd_search_host(np.zeros(8), mode=3)
    with pytest.raises(ValueError, match="GPU"):
        NC.cpd_search(np.zeros(8), device="cpu")                     # no quiet fall-back to the host


# ---- scRT's cell level

def test_cell_level_is_the_chain_of_the_public_functions():
    from scdna_replication_tools.infer_scRT import scRT
    from scdna_replication_tools_amd import binarize as B
    from scdna_replication_tools_amd import gc_correction as G
    from scdna_replication_tools_amd import simulator
    from scdna_replication_tools_amd.infer_scRT import assign_s_to_clones, consensus_profiles
    cn_s, cn_g1 = simulator.to_long_form(simulator.simulate(12, 10, n_bins=96, seed=3, n_clones=2))
    cols_s, cols_g = list(cn_s.columns), list(cn_g1.columns)
    obj = scRT(cn_s, cn_g1, device="cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = obj.infer_cell_level()
        prof = consensus_profiles(cn_g1, "copy", clone_col="clone_id")
        s = assign_s_to_clones(cn_s, prof, col_name="copy", clone_col="clone_id")
        s, g = G.bulk_g1_gc_correction(s, cn_g1, input_col="reads", output_col="rpm_gc_norm", device="cpu")
        s = NC.normalize_by_cell(s, g, input_col="rpm_gc_norm", clone_col="clone_id", temp_col="temp_rt",
                                 output_col="rt_value", seg_col="changepoint_segments", device="cpu")
        want, man = B.binarize_profiles(s, "rt_value", device="cpu")
    assert list(cn_s.columns) == cols_s and list(cn_g1.columns) == cols_g
    pd.testing.assert_frame_equal(obj.clone_profiles, prof)
    pd.testing.assert_frame_equal(out, want)
    pd.testing.assert_frame_equal(obj.manhattan_df, man)
    assert out is obj.cn_s
    assert {"rpm_gc_norm", "temp_rt", "changepoint_segments", "G1_match_cell_id", "rt_value", "rt_state"} <= set(out.columns)
    assert len(out) == len(cn_s) and set(out["G1_match_cell_id"]) <= set(cn_g1["cell_id"])
    assert set(out["rt_state"].unique()) <= {0.0, 1.0} and 0.0 < out["frac_rt"].mean() < 1.0
    pb = obj.compute_pseudobulk_rt_profiles()                        # flows into the downstream analyses
    assert "pseduobulk_hours" in pb.columns and obj.bulk_cn is pb


# ---- the shim

def test_import_paths_and_signatures_match_the_reference():
    import scdna_replication_tools.normalize_by_cell as shim
    from scdna_replication_tools.infer_scRT import scRT
    cols = ["cell_col", "chr_col", "start_col"]
    ref = {
        "sort_by_cell_and_loci": (["cn"] + cols, dict(cell_col="cell_id", chr_col="chr", start_col="start")),
        "identify_changepoint_segs": (["cell_cn", "col", "chr_col"], dict(chr_col="chr")),
        "remove_cell_specific_CNAs": (["cell_cn", "input_col", "output_col", "seg_col"] + cols,
                                      dict(input_col="copy_norm", output_col="rt_value", seg_col="changepoint_segments")),
        "compute_cell_corrs": (["s_cell_cn", "clone_cn_g1", "s_cell_id", "col"] + cols, dict(col="rpm_gc_norm")),
        "g1_cell_norm": (["s_cell_cn", "g1_cell_cn", "input_col", "output_col"] + cols + ["cn_state_col", "ploidy_col"],
                         dict(input_col="rpm_gc_norm", output_col="state_norm", cn_state_col="state", ploidy_col="ploidy")),
        "normalize_by_cell": (["cn_s", "cn_g1", "input_col", "clone_col", "cell_col", "temp_col", "output_col", "seg_col",
                               "chr_col", "start_col", "cn_state_col", "ploidy_col"],
                              dict(input_col="rpm_gc_norm", clone_col="clone_id", temp_col="temp_rt", output_col="rt_value",
                                   seg_col="changepoint_segments", cn_state_col="state", ploidy_col="ploidy")),
    }
    for name, (params, defaults) in ref.items():
        sig = inspect.signature(getattr(shim, name))
        positional = [p for p, v in sig.parameters.items() if v.kind == v.POSITIONAL_OR_KEYWORD]
        assert positional == params, name
        for p, d in defaults.items():
            assert sig.parameters[p].default == d, (name, p)
        assert name in shim.__all__
    assert shim.normalize_by_cell is NC.normalize_by_cell
    assert [p for p in inspect.signature(scRT.infer_cell_level).parameters] == ["self"]


# ---- the C ABI

def test_cpd_symbols_and_argument_checks():
    from scdna_replication_tools_amd import _native, build
    build.build()
    lib = _native.lib()
    with open(os.path.join(ROOT, "include", "pert_hip.h")) as fh:
        header = fh.read()
    for sym in ("pert_cpd_workspace", "pert_cpd_search"):
        assert sym in _native.EXPORTED_SYMBOLS and hasattr(lib, sym)
        assert re.search(r"\bint {}\(".format(sym), header)
    assert os.path.join(build.HERE, "csrc", "cpd_kernels.hip") in build.SOURCES
    max_n = int(re.search(r"#define PERT_CPD_MAX_N (\d+)", header).group(1))
    assert max_n == _native.CPD_MAX_N and max_n >= 5451
    assert 16 * (max_n + 1) + 256 <= 160 * 1024                     # the two tables and the winners in LDS
    nbytes = ctypes.c_int64()
    N, ld = 3, 8
    assert lib.pert_cpd_workspace(N, ld, ctypes.byref(nbytes)) == 0 and nbytes.value > 0
    assert lib.pert_cpd_workspace(N, ld, None) == 1
    assert lib.pert_cpd_workspace(0, ld, ctypes.byref(nbytes)) == 1
    assert lib.pert_cpd_workspace(65536, ld, ctypes.byref(nbytes)) == 1          # cells are one grid dimension
    assert lib.pert_cpd_workspace(N, 0, ctypes.byref(nbytes)) == 1
    assert lib.pert_cpd_workspace(N, max_n + 1, ctypes.byref(nbytes)) == 1       # over the LDS budget
    assert lib.pert_cpd_workspace(N, max_n, ctypes.byref(nbytes)) == 0
    assert lib.pert_cpd_workspace(1, 5451, ctypes.byref(nbytes)) == 0
    assert lib.pert_cpd_workspace(N, ld, ctypes.byref(nbytes)) == 0
    # nothing below may launch or copy: the device pointers are not device memory
    buf = ctypes.create_string_buffer(int(nbytes.value) + 64)
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    ip = ctypes.POINTER(ctypes.c_int32)
    lens, mode, active = np.array([8, 6, 3], np.int32), np.array([2, 1, 2], np.int32), np.array([1, 1, 0], np.int32)

    def search(N=N, ld=ld, y=ptr, lens=lens, mode=mode, active=active, a=ptr, b=ptr, g=ptr, ws=ptr, nb=None):
        P = lambda v: None if v is None else v.ctypes.data_as(ip)
        return lib.pert_cpd_search(N, ld, y, P(lens), P(mode), P(active), a, b, g, ws,
                                   int(nbytes.value) if nb is None else nb, None)
    for kw in (dict(y=None), dict(lens=None), dict(mode=None), dict(active=None), dict(a=None), dict(b=None),
               dict(g=None), dict(ws=None), dict(N=0), dict(ld=0), dict(ld=max_n + 1), dict(nb=8),
               dict(ws=ctypes.c_void_p(ptr.value + 8)), dict(y=ctypes.c_void_p(ptr.value + 4)),
               dict(lens=np.array([9, 6, 3], np.int32)), dict(lens=np.array([8, -1, 3], np.int32)),
               dict(mode=np.array([2, 0, 2], np.int32)), dict(mode=np.array([3, 1, 2], np.int32)),
               dict(active=np.array([1, 2, 0], np.int32))):
        assert search(**kw) == 1, kw
    # no active cell: nothing to do, and nothing launched
    assert search(active=np.zeros(3, np.int32)) == 0
