"""Golden vectors from the REFERENCE's normalize_by_cell.py, run by hand in the build container only
(the reference does not travel to the GPU box; the committed .npz is data).

The module is imported from the reference tree with a stand-in ``ruptures`` whose ``KernelCPD`` is
the change-point search's definition by brute force: the full table of gains
G(a, b) of a profile, its first maximum in (a, b) order.  ``add_cell_ploidies`` is rebound to
make_binarize_reference_golden.own_cell_ploidies (the reference's raises on this scipy).  The
module's ``identify_changepoint_segs`` and ``ttest_ind`` are wrapped to RECORD every round of every
cell; they return what the reference's own return.

Input: 24 + 24 cells x 300 bins from simulator.simulate(n_clones=2), the bins relabelled into
chromosomes 1, 2 and X, reads per million as the input column, 3 % of the rows of both tables
dropped (ragged lengths after the merge with the G1 match), one NaN in each table, and planted
copy-number changes in six cells: two interior gains, two losses at the start of chr 1 and two gains
at the end of chr X.

The generator asserts that every decision of the run has a margin, so a test needs to exclude
nothing: in every round of every cell |median_ratio - 1.1|, |median_ratio - 0.9| and |pval - 0.05|
exceed 1e-6, the winning gain exceeds the best gain at any other (a, b) by more than 1e-9 relative,
and no cell comes near the round cap.  Pick another seed if an assertion fails.  Three edge cases made
from the same tables (tests/_cell_cases.py::variants) are recorded with the columns that carry the
decisions; the margins are asserted over their rounds too.

    python tests/golden/make_cell_level_reference_golden.py
"""
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_binarize_reference_golden import REF_PARENT, own_cell_ploidies  # noqa: E402

SEED = 31
N_CELLS, N_BINS = 24, 300
CHR_EDGES = (0, 120, 220, 300)                  # bins [0, 120) -> '1', [120, 220) -> '2', [220, 300) -> 'X'
CHR_NAMES = ("1", "2", "X")
ROUND_CAP = 64                                  # normalize_cell.MAX_ROUNDS (asserted equal in the test)

LOG = []                                        # one dict per cell: searches and decisions


def gains_table(y, n_bkps):
    """Every feasible candidate's gain, by the definition: (a, b, G) arrays in (a, b) order."""
    n = len(y)
    S = np.zeros(n + 1)
    for i in range(n):
        S[i + 1] = S[i] + y[i]
    rinv = np.zeros(n + 1)
    rinv[1:] = 1.0 / np.arange(1, n + 1)
    cand = []
    if n_bkps == 2:
        for a in range(2, n - 3):
            for b in range(a + 2, n - 1):
                g = (S[a] * S[a]) * rinv[a] + ((S[b] - S[a]) * (S[b] - S[a])) * rinv[b - a]
                g = g + ((S[n] - S[b]) * (S[n] - S[b])) * rinv[n - b]
                cand.append((a, b, g))
    else:
        for a in range(2, n - 1):
            g = (S[a] * S[a]) * rinv[a] + ((S[n] - S[a]) * (S[n] - S[a])) * rinv[n - a]
            cand.append((a, n, g))
    return cand


class KernelCPD:
    """The stand-in: fit(Y).predict(n_bkps) -> [a, b, n] or [a, n], first maximum of the gains."""

    def __init__(self, kernel="linear", min_size=2):
        assert kernel == "linear" and min_size == 2

    def fit(self, y):
        self.y = np.array(y, dtype=np.float64)
        return self

    def predict(self, n_bkps):
        n = len(self.y)
        cand = gains_table(self.y, n_bkps)
        assert cand, "infeasible search in the fixture"
        g = np.array([c[2] for c in cand])
        best = int(np.argmax(g))
        rest = np.delete(g, best)
        margin = (g[best] - rest.max()) / abs(g[best]) if rest.size else np.inf
        a, b, _ = cand[best]
        LOG[-1]["searches"].append(dict(n_bkps=n_bkps, a=a, b=b, gain=g[best], margin=margin, n=n))
        return [a, b, n] if n_bkps == 2 else [a, n]


def reference_module():
    rpt = types.ModuleType("ruptures")
    rpt.KernelCPD = KernelCPD
    sys.modules["ruptures"] = rpt
    assert "scdna_replication_tools" not in sys.modules
    sys.path.insert(0, REF_PARENT)
    import scdna_replication_tools.normalize_by_cell as nbc
    assert nbc.__file__.startswith(REF_PARENT)
    sys.path.remove(REF_PARENT)
    nbc.add_cell_ploidies = own_cell_ploidies
    ref_segs, ref_ttest = nbc.identify_changepoint_segs, nbc.ttest_ind

    def segs(cell_cn, col, chr_col='chr'):
        LOG.append(dict(searches=[], tests=[]))
        return ref_segs(cell_cn, col, chr_col=chr_col)

    def ttest(region, background):
        res = ref_ttest(region, background)
        with np.errstate(all="ignore"):
            LOG[-1]["tests"].append(dict(ratio=np.median(region) / np.median(background), pval=res[1],
                                         n_region=len(region), n_background=len(background)))
        return res

    nbc.identify_changepoint_segs, nbc.ttest_ind = segs, ttest
    return nbc


def tables():
    sys.path.insert(0, ROOT)
    from scdna_replication_tools_amd import simulator
    sim = simulator.simulate(N_CELLS, N_CELLS, n_bins=N_BINS, seed=SEED, n_clones=2)
    df_s, df_g = simulator.to_long_form(sim)
    chrom = np.empty(N_BINS, dtype=object)
    for k, name in enumerate(CHR_NAMES):
        chrom[CHR_EDGES[k]:CHR_EDGES[k + 1]] = name
    out = []
    for df in (df_s, df_g):
        df = df[["clone_id", "cell_id", "start", "chr", "state", "reads", "library_id"]].copy()
        df["chr"] = np.tile(chrom, N_CELLS)
        df["reads"] = df["reads"].astype(np.float64)
        out.append(df)
    cn_s, cn_g = out
    # the planted cell-specific changes, in the S-phase cells' reads (bin positions of the full table)
    cells = cn_s["cell_id"].unique()
    bins = np.tile(np.arange(N_BINS), N_CELLS)
    for cell, lo, hi, factor in ((cells[2], 150, 190, 1.6), (cells[5], 0, 30, 0.45), (cells[9], 265, 300, 1.7),
                                 (cells[14], 40, 75, 1.5), (cells[17], 0, 25, 0.5), (cells[20], 270, 300, 1.6)):
        hit = (cn_s["cell_id"].to_numpy() == cell) & (bins >= lo) & (bins < hi)
        cn_s.loc[hit, "reads"] = np.round(cn_s.loc[hit, "reads"] * factor)
    for df in (cn_s, cn_g):
        tot = df.groupby("cell_id")["reads"].transform("sum")
        df["rpm_gc_norm"] = df["reads"] / tot * 1e6
    rng = np.random.default_rng(SEED)
    cn_s = cn_s[rng.uniform(size=len(cn_s)) >= 0.03].reset_index(drop=True)
    cn_g = cn_g[rng.uniform(size=len(cn_g)) >= 0.03].reset_index(drop=True)
    cn_s.loc[777, "rpm_gc_norm"] = np.nan
    cn_g.loc[4321, "rpm_gc_norm"] = np.nan
    return cn_s, cn_g


def store(out, key, df):
    out[key + "_columns"] = np.asarray(df.columns).astype("U")
    out[key + "_dtypes"] = np.asarray([str(df[c].dtype) for c in df.columns]).astype("U")
    out[key + "_index"] = df.index.to_numpy()
    for i, c in enumerate(df.columns):
        v = df[c]
        if isinstance(v.dtype, pd.CategoricalDtype):
            out["{}_cat{}".format(key, i)] = np.asarray(v.cat.categories).astype("U")
            v = v.astype(object)
        v = v.to_numpy()
        out["{}_col{}".format(key, i)] = v.astype("U") if v.dtype == object else v


def main():
    import scipy
    import sklearn
    nbc = reference_module()
    cn_s, cn_g = tables()
    out = dict(numpy_version=np.array(np.__version__), pandas_version=np.array(pd.__version__),
               scipy_version=np.array(scipy.__version__), sklearn_version=np.array(sklearn.__version__))
    store(out, "in_s", cn_s)
    store(out, "in_g", cn_g)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = nbc.normalize_by_cell(cn_s.copy(), cn_g.copy())
    store(out, "out", res)
    n_main = len(LOG)
    assert n_main == cn_s["cell_id"].nunique()

    # edge cases made from the same tables (tests/_cell_cases.py::variants): the reference's result,
    # the columns that carry the decisions
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _cell_cases
    for name, (vs, vg) in _cell_cases.variants(cn_s, cn_g).items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            vres = nbc.normalize_by_cell(vs.copy(), vg.copy())
        out["variant_{}_columns".format(name)] = np.asarray(vres.columns).astype("U")
        for c in _cell_cases.VARIANT_COLS:
            v = vres[c].to_numpy()
            out["variant_{}_{}".format(name, c)] = v.astype("U") if v.dtype == object else v

    # every decision has a margin, in the main run and in the edge cases
    assert max(len(c["searches"]) for c in LOG) < ROUND_CAP // 2
    n_search = np.array([len(c["searches"]) for c in LOG[:n_main]])
    worst = dict(ratio=np.inf, pval=np.inf, gain=np.inf)
    for c in LOG:
        for s in c["searches"]:
            worst["gain"] = min(worst["gain"], s["margin"])
        for t in c["tests"]:
            worst["ratio"] = min(worst["ratio"], abs(t["ratio"] - 1.1), abs(t["ratio"] - 0.9))
            worst["pval"] = min(worst["pval"], abs(t["pval"] - 0.05))
            assert t["n_region"] == t["n_background"]            # the mirror image, not the complement
    assert worst["gain"] > 1e-9 and worst["ratio"] > 1e-6 and worst["pval"] > 1e-6, worst
    flat = [(ci, s["n_bkps"], s["n"], s["a"], s["b"], s["gain"]) for ci, c in enumerate(LOG[:n_main])
            for s in c["searches"]]
    out["searches"] = np.array([f[:5] for f in flat], dtype=np.int64)       # cell, n_bkps, n, a, b
    out["search_gains"] = np.array([f[5] for f in flat])
    out["n_searches"] = n_search
    out["round_cap"] = np.array(ROUND_CAP)
    out["worst_margins"] = np.array([worst["gain"], worst["ratio"], worst["pval"]])
    segs = res.groupby("cell_id")["changepoint_segments"].max().to_numpy()
    assert (segs > 0).sum() >= 6, segs

    path = os.path.join(HERE, "cell_level_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    print("columns:", list(res.columns))
    print("dtypes:", [str(res[c].dtype) for c in res.columns])
    print("rows:", len(res), "of", len(cn_s), "index", res.index[:3].tolist())
    print("searches per cell: mean {:.2f}, max {}".format(n_search.mean(), n_search.max()))
    print("nominated segments per cell:", segs.astype(int).tolist())
    print("worst margins (gain rel, ratio, pval):", worst)


if __name__ == "__main__":
    main()
