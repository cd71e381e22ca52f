"""The reference-produced fixture of the pseudobulk / T-width analyses
(tests/golden/rt_reference.npz, written by tests/golden/make_rt_reference_golden.py) as the
tables the reference ran on, and exact comparisons against what it recorded."""
import os

import numpy as np
import pandas as pd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rt_reference.npz")
STATE, FRAC, TFS = "model_rep_state", "cell_frac_rep", "time_from_scheduled_rt"
QUERY = "chr == '1'"
_cache = {}


def golden():
    if "z" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def table(case):
    """The input long table of case A, B, C or D (B and D are A with one column replaced)."""
    z = golden()
    key = "C" if case == "C" else "A"
    cn = pd.DataFrame({"cell_id": z[key + "_cell_id"].astype(object), "chr": z[key + "_chr"].astype(object),
                       "start": z[key + "_start"], "clone_id": z[key + "_clone_id"].astype(object),
                       STATE: z[key + "_state"], FRAC: z[key + "_frac"]})
    if case == "B":
        cn[FRAC] = z["B_frac"]
    if case == "D":
        cn[STATE] = z["D_state"]
    return cn


def same_bits(a, b):
    """Equal dtype, shape and bit patterns (so NaNs compare equal positionally, -0.0 != 0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind in "OU" or b.dtype.kind in "OU":
        return a.shape == b.shape and bool((a.astype("U") == b.astype("U")).all())
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_frame_is(df, key):
    z = golden()
    assert list(df.columns) == list(z[key + "_columns"])
    assert [str(df[c].dtype) for c in df.columns] == list(z[key + "_dtypes"])
    for i, c in enumerate(df.columns):
        assert same_bits(df[c].to_numpy(), z["{}_col{}".format(key, i)]), (key, c)
    assert list(df.index) == list(range(len(df)))


def assert_hist_is(res, key):
    z = golden()
    time_bins, pct_reps = res
    assert all(type(p) is float for p in pct_reps)
    assert same_bits(np.asarray(time_bins, np.float64), z[key + "_time_bins"]), key
    assert same_bits(np.asarray(pct_reps, np.float64), z[key + "_pct_reps"]), key
