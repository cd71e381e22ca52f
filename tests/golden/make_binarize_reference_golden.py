"""Golden vectors from the REFERENCE's binarize_rt_profiles.py and normalize_by_clone.py, run by
hand in the build container only (the reference does not travel to the GPU box; the committed
.npz is data).  Both modules are imported from the reference tree with ``ruptures`` (unused by
anything under test) stubbed.  ``normalize_by_clone.add_cell_ploidies`` is REBOUND to a ploidy
function of this generator's own: the reference's raises on this scipy (``stats.mode`` returns a
scalar, see make_reference_golden.py); the replacement writes the same column (per-cell mode of
the state, float64) and leaves the columns in the order the reference's set_index / reset_index
round trip leaves them (cell column first, ploidy last).

Cases (tests/test_binarize.py, tests/test_gpu_binarize.py), float64 profiles:
  A  48 cells x 271 bins from simulator.simulate: reads / G1 pseudobulk median
  B  60 cells x 600 bins, the scale-mixture construction of tests/test_gpu_tau.py rescaled into
     (-3, 3): GMM means closer than 0.7, >= 10 cells in each of the early / mid / late branches
  C  24 cells x 96 bins (fewer bins than the kernel's 256 threads)
  D  ragged: 10 cells of 271 bins, 10 of 263, 4 of 300, rows shuffled
  E  32 cells x 1,000 bins at 8 reads per bin: many identical values
  F  8 cells all above 3 and 8 all below -3: every threshold gives one side
  G  normalize_by_clone on A's long tables: two clones, 3 % of the rows dropped, one locus missing
     from one clone's profile, one inf in a cell

    python tests/golden/make_binarize_reference_golden.py
"""
import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_PARENT = "/root/reference"
OUT_COLS = ["mean_0", "covariance_0", "mean_1", "covariance_1", "gmm_state", "rt_state", "frac_rt", "binary_thresh"]


def own_cell_ploidies(cn, cell_col='cell_id', cn_state_col='state', ploidy_col='ploidy'):
    """Per-cell mode of the state (ties to the smallest value) as a float64 column, written in
    place; the cell column moves to the front as the reference's index round trip leaves it."""
    mode = cn.groupby(cell_col)[cn_state_col].agg(lambda s: s.value_counts().sort_index().idxmax())
    ploidy = cn[cell_col].map(mode).astype(np.float64)
    cells = cn.pop(cell_col)
    cn.insert(0, cell_col, cells)
    cn[ploidy_col] = ploidy
    return cn


def reference_modules():
    """The reference's two modules, imported before the project's own package of the same name can
    be found (the repository root is put on the path afterwards)."""
    sys.modules.setdefault("ruptures", types.ModuleType("ruptures"))
    assert "scdna_replication_tools" not in sys.modules
    sys.path.insert(0, REF_PARENT)
    import scdna_replication_tools.binarize_rt_profiles as brp
    import scdna_replication_tools.normalize_by_clone as nbc
    assert brp.__file__.startswith(REF_PARENT) and nbc.__file__.startswith(REF_PARENT)
    sys.path.remove(REF_PARENT)
    nbc.add_cell_ploidies = own_cell_ploidies
    return brp, nbc


def long_table(X, prefix):
    """(L, N) matrix -> rows grouped by cell."""
    L, N = X.shape
    cells = np.array(["{}_{:03d}".format(prefix, n) for n in range(N)], dtype=object)
    return pd.DataFrame({"cell_id": np.repeat(cells, L), "x": X.T.reshape(-1)})


def scale_mixture(L=600, N=60, seed=5):
    """tests/test_gpu_tau.py::_scale_mixture's construction."""
    rng = np.random.default_rng(seed)
    cols = []
    for n in range(N):
        x = rng.standard_normal(L) * np.where(rng.random(L) < 0.2, 4.0, 1.0)
        if n % 3 == 1:
            x = x + rng.exponential(3.0, L) * (rng.random(L) < 0.3)
        elif n % 3 == 2:
            x = x - rng.exponential(3.0, L) * (rng.random(L) < 0.3)
        cols.append(np.round(200 + 20 * x))
    return np.stack(cols, 1).astype(np.float64)


def run_binarize(out, key, brp, table):
    out[key + "_cell_id"] = table["cell_id"].to_numpy().astype("U")
    out[key + "_x"] = table["x"].to_numpy(np.float64)
    cn = table.copy()
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cn, man = brp.binarize_profiles(cn, "x")
    out[key + "_columns"] = np.asarray(cn.columns).astype("U")
    out[key + "_dtypes"] = np.asarray([str(cn[c].dtype) for c in cn.columns]).astype("U")
    for c in OUT_COLS:
        out["{}_{}".format(key, c)] = cn[c].to_numpy()
    out[key + "_man_columns"] = np.asarray(man.columns).astype("U")
    out[key + "_man_dtypes"] = np.asarray([str(man[c].dtype) for c in man.columns]).astype("U")
    out[key + "_man_index"] = man.index.to_numpy()
    for c in man.columns:
        v = man[c].to_numpy()
        out["{}_man_{}".format(key, c)] = v.astype("U") if v.dtype == object else v
    return cn, man


def ratio_profiles(simulator, n_cells, n_bins, seed, num_reads=1e6):
    sim = simulator.simulate(n_cells, n_cells, n_bins=n_bins, seed=seed, num_reads=num_reads)
    return sim, sim.reads_s.astype(np.float64) / np.median(sim.reads_g.astype(np.float64), axis=1)[:, None]


def main():
    import scipy
    import sklearn
    brp, nbc = reference_modules()
    sys.path.insert(0, ROOT)
    from scdna_replication_tools_amd import simulator
    out = dict(numpy_version=np.array(np.__version__), pandas_version=np.array(pd.__version__),
               scipy_version=np.array(scipy.__version__), sklearn_version=np.array(sklearn.__version__))

    sim_a, XA = ratio_profiles(simulator, 48, 271, seed=11)
    run_binarize(out, "A", brp, long_table(XA, "a"))

    reads = scale_mixture(seed=4)              # 25 early, 12 mid, 23 late (seed 5: only 9 mid)
    XB = (reads - 200.0) / 20.0
    XB = XB * (2.9 / np.abs(XB).max())
    cnb, _ = run_binarize(out, "B", brp, long_table(XB, "b"))
    from scipy.stats import skew
    per = cnb.groupby("cell_id").first()
    assert ((per["mean_0"] - per["mean_1"]).abs() < 0.7).all()
    sk = np.array([skew(XB[:, n]) for n in range(XB.shape[1])])
    branches = [(sk > 0.2).sum(), ((sk <= 0.2) & (sk >= -0.2)).sum(), (sk < -0.2).sum()]
    assert min(branches) >= 10, branches
    out["B_branches"] = np.array(branches)

    _, XC = ratio_profiles(simulator, 24, 96, seed=12)
    run_binarize(out, "C", brp, long_table(XC, "c"))

    _, XD = ratio_profiles(simulator, 24, 300, seed=13)
    lens = [271] * 10 + [263] * 10 + [300] * 4
    parts = []
    for n, ln in enumerate(lens):
        parts.append(pd.DataFrame({"cell_id": "d_{:03d}".format((n * 7) % 24), "x": XD[:ln, n]}))
    td = pd.concat(parts, ignore_index=True).sample(frac=1.0, random_state=4).reset_index(drop=True)
    run_binarize(out, "D", brp, td)

    sim_e = simulator.simulate(32, 32, n_bins=1000, seed=14, num_reads=8 * 1000)
    XE = sim_e.reads_s.astype(np.float64) / 8.0
    run_binarize(out, "E", brp, long_table(XE, "e"))

    _, XF = ratio_profiles(simulator, 16, 120, seed=15)
    XF[:, :8] = 3.5 + XF[:, :8]
    XF[:, 8:] = -3.5 - XF[:, 8:]
    assert XF[:, :8].min() > 3 and XF[:, 8:].max() < -3
    cnf, _ = run_binarize(out, "F", brp, long_table(XF, "f"))
    assert set(cnf["frac_rt"].unique()) == {0.0, 1.0} and (cnf["binary_thresh"] == -3.0).all()

    # G: normalize_by_clone
    sim_g = simulator.simulate(48, 48, n_bins=271, seed=11, n_clones=2)
    df_s, df_g = simulator.to_long_form(sim_g)
    df_s["reads"] = df_s["reads"].astype(np.float64)
    df_g["reads"] = df_g["reads"].astype(np.float64)
    rng = np.random.default_rng(21)
    cn_s = df_s[["clone_id", "cell_id", "start", "chr", "state", "reads", "gc"]]
    cn_s = cn_s[rng.uniform(size=len(cn_s)) >= 0.03].reset_index(drop=True)
    cn_s.loc[1234, "reads"] = np.inf
    prof = df_g.pivot_table(index=["chr", "start"], columns="clone_id", values="reads", aggfunc="median")
    prof.iloc[17, 1] = np.nan                        # one locus missing from clone B's profile
    for c in cn_s.columns:
        v = cn_s[c].to_numpy()
        out["G_in_" + c] = v.astype("U") if v.dtype == object else v
    out["G_in_columns"] = np.asarray(cn_s.columns).astype("U")
    out["G_prof_chr"] = prof.index.get_level_values(0).to_numpy().astype("U")
    out["G_prof_start"] = prof.index.get_level_values(1).to_numpy(np.int64)
    out["G_prof_columns"] = np.asarray(prof.columns).astype("U")
    out["G_prof_values"] = prof.to_numpy(np.float64)
    res = nbc.normalize_by_clone(cn_s.copy(), prof.copy(), input_col="reads")
    out["G_columns"] = np.asarray(res.columns).astype("U")
    out["G_dtypes"] = np.asarray([str(res[c].dtype) for c in res.columns]).astype("U")
    out["G_index"] = res.index.to_numpy()
    for i, c in enumerate(res.columns):
        v = res[c].to_numpy()
        out["G_col{}".format(i)] = v.astype("U") if v.dtype == object else v

    path = os.path.join(HERE, "binarize_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    print("A columns:", list(out["A_columns"]), list(out["A_dtypes"]))
    print("manhattan:", list(out["A_man_columns"]), list(out["A_man_dtypes"]), out["A_man_index"][:3], out["A_man_index"][98:102])
    print("B branches (early, mid, late):", branches)
    print("G columns:", list(out["G_columns"]), list(out["G_dtypes"]), "rows", len(res), "of", len(cn_s))


if __name__ == "__main__":
    main()
