"""Golden vectors from the REFERENCE's compute_pseudobulk_rt_profiles.py and calculate_twidth.py,
run in the build container only (the reference does not travel to the GPU box; the committed
.npz is data).  Both modules import here once ``seaborn`` (unused by anything under test) is
stubbed; matplotlib runs on the Agg backend.

Cases (tests/test_rt_profiles.py, tests/test_gpu_rt.py):
  A  grid, 64 loci on chromosomes '1' and '10' x 40 cells, clones A/B, float32 state and fraction
  B  A with a float64 fraction column holding the float32 quotients widened
  C  A shuffled, 3 % of the rows dropped, clone B missing three loci (inner-merge loss of loci)
  D  A with clone B fully replicated: a constant clone profile, NaN hours for that clone
  E  calc_pct_replicated_per_time_bin on hand-made tfs columns (float32 and float64) holding
     every float32(edge), every float64 edge, -10, 10, nextafter(10, 0), NaN and a value < -10
  F  query2 = "chr == '1'" and per_cell=True on A
  G  calculate_twidth, sigmoid and linear, aggregated and per cell, on A

    python tests/golden/make_rt_reference_golden.py
"""
import os
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/scdna_replication_tools"
STATE, FRAC, TFS = "model_rep_state", "cell_frac_rep", "time_from_scheduled_rt"


def reference_modules():
    import matplotlib
    matplotlib.use("Agg")
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    sys.path.insert(0, REF)
    import calculate_twidth as tw                       # the reference modules
    import compute_pseudobulk_rt_profiles as pb
    return pb, tw


def base_table(seed=5):
    rng = np.random.default_rng(seed)
    chrom = np.array(["1"] * 34 + ["10"] * 30)
    start = np.concatenate([np.arange(34), np.arange(30)]).astype(np.int64) * 500000 + 1
    L, N = 64, 40
    cells = np.array(["cell_%02d" % i for i in range(N)])
    clones = np.array(["A"] * 25 + ["B"] * 15)
    rt = rng.uniform(0.0, 1.0, L)                                        # locus timing, 0 = early
    tau = rng.uniform(0.1, 0.9, N)
    state = ((rt[:, None] + rng.normal(0.0, 0.15, (L, N))) < tau[None, :]).astype(np.float32)
    state[:, clones == "B"] = ((rt[::-1, None] * 0.7 + rng.normal(0.0, 0.2, (L, 15))) < tau[None, 25:]).astype(np.float32)
    frac = (state.sum(axis=0, dtype=np.float32) / np.float32(L)).astype(np.float32)
    ll, nn = np.meshgrid(np.arange(L), np.arange(N), indexing="ij")
    ll, nn = ll.ravel(), nn.ravel()
    return pd.DataFrame({"cell_id": cells[nn], "chr": chrom[ll], "start": start[ll], "clone_id": clones[nn],
                         STATE: state[ll, nn], FRAC: frac[nn]})


def save_table(out, key, cn):
    out[key + "_cell_id"] = cn["cell_id"].to_numpy().astype("U")
    out[key + "_chr"] = cn["chr"].to_numpy().astype("U")
    out[key + "_start"] = cn["start"].to_numpy(np.int64)
    out[key + "_clone_id"] = cn["clone_id"].to_numpy().astype("U")
    out[key + "_state"] = cn[STATE].to_numpy()
    out[key + "_frac"] = cn[FRAC].to_numpy()


def save_frame(out, key, df):
    out[key + "_columns"] = np.asarray(df.columns).astype("U")
    out[key + "_dtypes"] = np.asarray([str(df[c].dtype) for c in df.columns]).astype("U")
    for i, c in enumerate(df.columns):
        v = df[c].to_numpy()
        out["{}_col{}".format(key, i)] = v.astype("U") if v.dtype == object else v


def save_hist(out, key, res):
    tb, pct = res
    assert all(type(p) is float for p in pct)
    out[key + "_time_bins"] = np.asarray(tb, np.float64)
    out[key + "_pct_reps"] = np.asarray(pct, np.float64)


def run_case(out, key, cn, pb, tw, hist=True):
    """pseudobulk -> merge -> tfs column -> aggregated histogram, as the reference's main() chains them."""
    bulk = pb.compute_pseudobulk_rt_profiles(cn, STATE)
    save_frame(out, key + "_pb", bulk)
    merged = pd.merge(cn, bulk)
    merged = tw.compute_time_from_scheduled_column(merged, pseudobulk_col="pseudobulk_hours", frac_rt_col=FRAC, tfs_col=TFS)
    out[key + "_tfs"] = merged[TFS].to_numpy()
    if hist:
        save_hist(out, key + "_hist", tw.calc_pct_replicated_per_time_bin(merged, tfs_col=TFS, rs_col=STATE))
    return merged


def main():
    import scipy
    pb, tw = reference_modules()
    out = dict(numpy_version=np.array(np.__version__), pandas_version=np.array(pd.__version__),
               scipy_version=np.array(scipy.__version__))
    cn = base_table()
    save_table(out, "A", cn)
    merged = run_case(out, "A", cn, pb, tw)

    cn_b = cn.copy()
    cn_b[FRAC] = cn_b[FRAC].astype(np.float64)
    out["B_frac"] = cn_b[FRAC].to_numpy()
    run_case(out, "B", cn_b, pb, tw)

    rng = np.random.default_rng(9)
    cn_c = cn.sample(frac=1.0, random_state=3).reset_index(drop=True)
    cn_c = cn_c[rng.uniform(size=len(cn_c)) >= 0.03]
    gone = (cn_c["clone_id"] == "B") & (((cn_c["chr"] == "1") & cn_c["start"].isin([1, 2500001])) |
                                        ((cn_c["chr"] == "10") & (cn_c["start"] == 1000001)))
    cn_c = cn_c[~gone].reset_index(drop=True)
    save_table(out, "C", cn_c)
    run_case(out, "C", cn_c, pb, tw)

    cn_d = cn.copy()
    cn_d.loc[cn_d["clone_id"] == "B", STATE] = np.float32(1.0)
    out["D_state"] = cn_d[STATE].to_numpy()
    run_case(out, "D", cn_d, pb, tw)

    edges = np.linspace(-10, 10, 201)
    for name, dt in (("f32", np.float32), ("f64", np.float64)):
        special = np.array([-10.0, 10.0, np.nextafter(dt(10), dt(0)), np.nan, -10.5, np.nextafter(dt(-10), dt(-11))])
        t = np.concatenate([edges.astype(np.float32).astype(dt), edges.astype(dt), special.astype(dt),
                            rng.uniform(-11, 11, 300).astype(dt)])
        assert t.dtype == dt
        df = pd.DataFrame({TFS: t, STATE: (rng.uniform(size=t.size) < 0.5).astype(np.float32),
                           "cell_id": np.array(["c%d" % (i % 7) for i in range(t.size)])})
        out["E_{}_tfs".format(name)] = t
        out["E_{}_state".format(name)] = df[STATE].to_numpy()
        out["E_{}_cell_id".format(name)] = df["cell_id"].to_numpy().astype("U")
        save_hist(out, "E_{}_hist".format(name), tw.calc_pct_replicated_per_time_bin(df, tfs_col=TFS, rs_col=STATE))
        save_hist(out, "E_{}_hist_cell".format(name),
                  tw.calc_pct_replicated_per_time_bin(df, tfs_col=TFS, rs_col=STATE, per_cell=True))

    q = "chr == '1'"
    save_hist(out, "F_query", tw.calc_pct_replicated_per_time_bin(merged, tfs_col=TFS, rs_col=STATE, query2=q))
    save_hist(out, "F_cell", tw.calc_pct_replicated_per_time_bin(merged, tfs_col=TFS, rs_col=STATE, per_cell=True))
    save_hist(out, "F_cell_query",
              tw.calc_pct_replicated_per_time_bin(merged, tfs_col=TFS, rs_col=STATE, per_cell=True, query2=q))

    for curve in ("sigmoid", "linear"):
        for per_cell in (False, True):
            t_width, right_time, left_time, popt, tb, pct = tw.calculate_twidth(
                merged, tfs_col=TFS, rs_col=STATE, per_cell=per_cell, curve=curve)
            key = "G_{}_{}".format(curve, "cell" if per_cell else "agg")
            out[key + "_times"] = np.array([t_width, right_time, left_time], np.float64)
            out[key + "_popt"] = np.asarray(popt, np.float64)
            save_hist(out, key, (tb, pct))

    path = os.path.join(HERE, "rt_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    print("A pseudobulk columns:", list(out["A_pb_columns"]), [out["A_pb_col%d" % i].dtype for i in range(len(out["A_pb_columns"]))])
    print("tfs dtypes:", out["A_tfs"].dtype, out["B_tfs"].dtype, "C loci:", len(out["C_pb_col0"]),
          "D NaN hours:", int(np.isnan(out["D_pb_col7"]).sum()) if "D_pb_col7" in out else None)
    print("G sigmoid:", out["G_sigmoid_agg_times"], out["G_sigmoid_cell_times"])


if __name__ == "__main__":
    main()
