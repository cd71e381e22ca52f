"""The LOWESS curve's oracle: the point-by-point definition, no regrouping,
one ``np.partition`` per fit, in fp64 or ``np.longdouble``; the first-order rounding bound of the
tests; and the cases the host path and the kernel are checked on."""
import numpy as np
import pandas as pd

EPS = float(np.finfo(np.float64).eps)
SAFETY = 8                       # binarize.margins' safety factor


def _fit(x0, x, y, d, k, stats=None):
    """The fit at x0 of the points (x, y) with robustness weights d."""
    dt = x.dtype.type
    dist = np.abs(x - x0)
    h = np.partition(dist, k - 1)[k - 1]
    inside = dist < h
    if h == 0 or not inside.any():
        raise ValueError("zero bandwidth")
    t = np.where(inside, dist / np.where(h > 0, h, 1), dt(0))
    t = np.where(inside, (1 - t ** 3) ** 3, dt(0))
    td = t * d
    tot = td.sum()
    if not tot > 0:
        return dt(np.nan)
    w = td / tot
    xbar = (w * x).sum()
    var = (w * (x - xbar) ** 2).sum()
    lev = 1 + (x0 - xbar) * (x - xbar) / var if var > 0 else np.ones_like(x)
    p = w * lev
    terms = p * y
    f = terms.sum()
    if stats is not None:
        # the condition of the sum; and what a change of the robustness weights does to the fit:
        # d fit / d delta_i = (t_i / tot) lev_i (y_i - line(x_i)), line the local line of this fit
        slope = (w * (x - xbar) * y).sum() / var if var > 0 else dt(0)
        line = (w * y).sum() + slope * (x - xbar)
        af = abs(f)
        stats["kappa"] = max(stats.get("kappa", 0.0), float(np.abs(terms).sum() / af) if af > 0 else 0.0)
        stats["sens"] = max(stats.get("sens", 0.0),
                            float((t / tot * np.abs(lev) * np.abs(y - line)).sum() / af) if af > 0 else 0.0)
        stats["lam"] = max(stats.get("lam", 0.0), float((t / tot * np.abs(lev)).sum()))
        stats["fmax"] = max(stats.get("fmax", 0.0), float(af))
    return f


def lowess_ref(x, y, xvals, frac=2.0 / 3.0, it=3, dtype=np.float64, with_bound=False):
    """The curve at ``xvals`` of the points (x, y), non-finite points dropped.  ``with_bound``:
    also the relative rounding bound of an fp64 evaluation (see ``bound`` below)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ok = np.isfinite(x) & np.isfinite(y)
    x, y = x[ok].astype(dtype), y[ok].astype(dtype)
    xvals = np.asarray(xvals, dtype=np.float64).astype(dtype)
    n = len(x)
    k = int(frac * n + 1e-10)
    if k < 1:
        raise ValueError("no neighbours")
    xs, back = np.unique(x, return_inverse=True)
    d = np.ones(n, dtype=dtype)
    err = 0.0                                   # the relative error carried by the fits of the last round
    for _ in range(it + 1):
        st = {} if with_bound else None
        fu = np.array([_fit(x0, x, y, d, k, st) for x0 in xs], dtype=dtype)
        r = np.abs(y - fu[back.reshape(-1)])
        m = np.median(r)
        if m == 0:
            u = np.where(r > 0, dtype(1), dtype(0))
        else:
            u = np.minimum(r / (6 * m), dtype(1))
        d = (1 - u * u) ** 2
        if with_bound:
            err = _carry(err, st, n)
            # residuals and their median move by err * fmax; u = r / (6 m), u <= 1 where it matters:
            # |du| <= (1/6 + 1) err fmax / m;  |d delta / du| = 4 u (1 - u^2) <= 8 / (3 sqrt 3);
            # a weight cannot move by more than 1 (m = 0: the weights are 0 / 1 by r > 0)
            derr = min(1.0, (8 / (3 * np.sqrt(3))) * (7 / 6) * err * st.get("fmax", 0.0) / float(m)) if m > 0 else 1.0
            err = (err, derr)
    st = {} if with_bound else None
    out = np.array([_fit(x0, x, y, d, k, st) for x0 in xvals], dtype=dtype)
    if with_bound:
        return out, SAFETY * _carry(err, st, n)
    return out


def _carry(err, st, n):
    """The relative error of a round's fits: the n-term sums' own rounding, n eps kappa, plus what
    the errors of the robustness weights (from the round before) do to them.  ``sens`` is
    sum |d fit / d delta_i| / |fit| at exact residuals; residuals known to ``e`` (relative to the
    fit) add ``lam * e`` to it."""
    own = n * EPS * st.get("kappa", 0.0)          # no entry: every fit of the round was NaN
    if not isinstance(err, tuple):
        return own                              # the first round: delta = 1 exactly
    e_fit, e_delta = err
    return own + (st.get("sens", 0.0) + st.get("lam", 0.0) * e_fit) * e_delta


# ----------------------------------------------------------------------------------------------
# cases: name -> (gc (L,), Y (C, L), xvals, frac, it)
# ----------------------------------------------------------------------------------------------

def _curve(gc):
    return 180.0 * (1.0 - 8.0 * (gc - 0.45) ** 2)


def make_case(C, L, seed, digits=3, frac=2.0 / 3.0, it=3, outliers=0.0, kind="gamma", nan=0):
    rng = np.random.default_rng(seed)
    gc = np.round(rng.uniform(0.3, 0.65, L), digits)
    if kind == "gamma":
        Y = _curve(gc)[None, :] * rng.gamma(20.0, 1.0 / 20.0, (C, L))
    elif kind == "rows":                        # identical rows of one constant: residuals 0 up to rounding
        Y = np.full((C, L), 100.0)
    elif kind == "zeros":                       # every residual exactly 0: m = 0
        Y = np.zeros((C, L))
    elif kind == "spike":
        # zeros, but for one bin where every cell reads 1: the fits away from it are exactly 0, so
        # more than half the residuals are exactly 0 (m = 0) and the points near the bin, whose
        # residuals are not, get u = 1 and weight 0 -- the curve there depends on that branch
        Y = np.zeros((C, L))
        Y[:, np.argsort(gc)[L // 2]] = 1.0
    elif kind == "split":
        # tiny noise, but at the two lowest gc values the cells read +1000 and -1000 in turn: their
        # first fit is near 0, their residuals 1000 get weight 0, and with a window of two distinct
        # x the next fit at the lowest one has zero weights only: NaN, which the median propagates
        Y = 1e-3 * rng.normal(size=(C, L))
        low = np.argsort(gc)[:2]
        Y[:, low] = np.where(np.arange(C) % 2 == 0, 1000.0, -1000.0)[:, None]
    else:
        raise ValueError(kind)
    if outliers:
        Y[rng.uniform(size=Y.shape) < outliers] *= 4.0
    for _ in range(nan):
        Y[rng.integers(C), rng.integers(L)] = np.nan
    return gc, Y, np.unique(gc), frac, it


CASES = {
    "3x5": dict(C=3, L=5, seed=1, digits=9),                                 # n odd, all gc distinct
    "7x96_ties": dict(C=7, L=96, seed=2, digits=2),                          # n even, U < L
    "12x40": dict(C=12, L=40, seed=3, digits=3),
    "12x40_distinct": dict(C=12, L=40, seed=4, digits=9),
    "7x96_frac": dict(C=7, L=96, seed=5, digits=3, frac=0.3),
    "7x96_it0": dict(C=7, L=96, seed=6, digits=3, it=0),
    "7x96_outliers": dict(C=7, L=96, seed=7, digits=3, outliers=0.02),       # 2 % of the points x 4: some delta = 0
    "12x40_rows": dict(C=12, L=40, seed=8, digits=3, kind="rows"),           # identical rows
    "12x40_zeros": dict(C=12, L=40, seed=9, digits=3, kind="zeros"),         # m = 0 exactly
    "7x96_nan": dict(C=7, L=96, seed=10, digits=3, nan=5),
    "1x400": dict(C=1, L=400, seed=11, digits=3, outliers=0.02),             # one cell: one chunk, one histogram row
    "9x65": dict(C=9, L=65, seed=12, digits=3, outliers=0.02),               # one lane past a wave of bins
}

# cases whose curve holds NaN: compared by ``agrees`` (the NaN where the oracle's are, the rest
# inside the bound)
SPECIAL = {
    "m0_branch": dict(C=6, L=40, seed=13, digits=9, frac=0.2, it=0, kind="spike"),
    "nan_fit": dict(C=8, L=10, seed=14, digits=9, frac=0.2, it=3, kind="split"),
}

_cache = {}


def case(name):
    """(gc, Y, xvals, frac, it, ref_long as float64, ref_f64, bound): computed once per session."""
    if name not in _cache:
        gc, Y, xv, frac, it = make_case(**(CASES[name] if name in CASES else SPECIAL[name]))
        x = np.tile(gc, Y.shape[0])
        long_, bound = lowess_ref(x, Y.ravel(), xv, frac, it, dtype=np.longdouble, with_bound=True)
        f64 = lowess_ref(x, Y.ravel(), xv, frac, it, dtype=np.float64)
        for a in (gc, Y, xv):
            a.setflags(write=False)
        _cache[name] = (gc, Y, xv, frac, it, long_, f64, bound)
    return _cache[name]


def scaled_error(got, long_, bound):
    """max |got - ref| / (bound |ref|): inside the bound when <= 1 (0 / 0 counts as 0)."""
    got = np.asarray(got, dtype=np.longdouble)
    diff = np.abs(got - long_)
    den = bound * np.abs(long_)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(diff == 0, 0.0, diff / den)
    return float(np.max(s))


def agrees(got, long_, bound):
    """NaN exactly where the oracle's curve is NaN, and the rest inside the bound."""
    got = np.asarray(got)
    nan = np.isnan(np.asarray(long_, dtype=np.float64))
    if not np.array_equal(np.isnan(got), nan):
        return False
    return bool(nan.all()) or scaled_error(got[~nan], long_[~nan], bound) <= 1.0


def host_curve(gc, Y, xv, frac, it, cond=None):
    from scdna_replication_tools_amd import gc_correction
    ux, inv = np.unique(gc, return_inverse=True)
    return gc_correction.lowess_host(ux, np.tile(inv.reshape(-1), Y.shape[0]), Y.ravel(), xv, frac=frac, it=it,
                                     cond=cond)


def tables(seed=0, C_s=3, C_g=5, L=24):
    """Two libraries with different GC curves; library B's cells hold fewer bins."""
    rng = np.random.default_rng(seed)
    rows_s, rows_g = [], []
    for lib, a, n_bins in (("A", 6.0, L), ("B", -4.0, L - 5)):
        gc = np.round(rng.uniform(0.3, 0.65, n_bins), 3)
        lam = 60.0 * (1.0 + a * (gc - 0.45) ** 2 + 0.5 * a * (gc - 0.45))
        for rows, C, tag in ((rows_s, C_s, "s"), (rows_g, C_g, "g")):
            for c in range(C):
                rows.append(pd.DataFrame({"cell_id": "{}_{}{}".format(lib, tag, c), "library_id": lib, "chr": "1",
                                          "start": np.arange(n_bins) * 500000, "gc": gc,
                                          "reads": rng.poisson(lam)}))
    return pd.concat(rows_s, ignore_index=True), pd.concat(rows_g, ignore_index=True)
