"""The bulk G1 GC correction (reference scdna_replication_tools/bulk_gc_correction.py): reads per
million per cell, one LOWESS curve of rpm on GC per library over every (G1/2 cell, bin) point, and
every row's rpm divided by the curve at its GC.

The reference calls ``statsmodels.nonparametric.lowess(rpm, gc, xvals=unique gc)`` (frac = 2/3,
it = 3, delta = 0) on the long table -- a weighted regression over two thirds of all points for
every distinct GC value, four times over -- and then looks the curve up row by row through
``DataFrame.apply``.  GC is a property of the bin: x takes U distinct values, each repeated once
per cell, and the tricube weight depends on x alone.  So a fit needs two sums per distinct x,
S0 = sum delta and S1 = sum delta y (delta the robustness weights), and a robustness round is one
pass over the rpm matrix, an exact median of the absolute residuals and a U x U local regression.

``lowess_matrix`` is that on a GPU (csrc/lowess_kernels.hip, ``pert_lowess_curve``: every round
queued at once, fp64, bit-identical from run to run); ``lowess_host`` is the same regrouped
algorithm in numpy with an inverse index per point, the CPU path, the path of a table whose cells
do not share one list of bins, and the kernel's check.  The curve's definition (DESIGN.md section
6n): k = int(frac n + 1e-10); the bandwidth h of a fit at x0 is the k-th smallest |x - x0|;
t = (1 - (|x - x0| / h)^3)^3 inside h; weights t delta / sum t delta; the weighted local line at x0.
Robustness runs it + 1 rounds from delta = 1: fits at every data x, m = np.median |residual|,
u = min(r / (6 m), 1), delta = (1 - u^2)^2 (m = 0: u = 1 where r > 0).  h = 0 raises ValueError; a
window of zero delta only gives NaN.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pandas as pd
import torch

from .ccc_features import _by_length, _cells

FRAC, IT = 2.0 / 3.0, 3          # statsmodels' defaults, the reference's call
_BLOCK = 256                     # fit points per block of the host regression


def lowess_k(n: int, frac: float) -> int:
    """The number of neighbours of a fit among n points (statsmodels: int(frac * n + 1e-10))."""
    return int(frac * n + 1e-10)


def _check_bandwidth(ux, cnt, k, x0s):
    """ValueError unless every fit has a point strictly inside its bandwidth: the points at the
    nearest populated x must be fewer than k (else h = 0, or every tricube weight is 0)."""
    if k < 1:
        raise ValueError("lowess: frac * n < 1, no neighbour in a fit's window")
    pos = np.flatnonzero(cnt > 0)
    xp, cp = ux[pos], cnt[pos]
    i = np.searchsorted(xp, x0s)
    lo, hi = np.clip(i - 1, 0, len(xp) - 1), np.clip(i, 0, len(xp) - 1)
    dl, dh = np.abs(xp[lo] - x0s), np.abs(xp[hi] - x0s)
    near = np.where(dl < dh, cp[lo], np.where(dh < dl, cp[hi], np.where(lo == hi, cp[lo], cp[lo] + cp[hi])))
    if (near >= k).any():
        raise ValueError("lowess: the {} neighbours of a fit all sit at one x (a single distinct x, or frac too "
                         "small): the bandwidth is 0".format(k))


def _regress(ux, cnt, S0, S1, k, x0s, cond=None):
    """The local regression at x0s from the per-distinct-x sums.  ``cond``: a list that receives
    the largest condition of the fits' sums, sum |terms| / |sum of terms| (for y of one sign, where
    a distinct x's terms share their sign, it is the point-by-point sum's)."""
    out = np.empty(len(x0s))
    worst = 0.0
    for b in range(0, len(x0s), _BLOCK):
        x0 = x0s[b:b + _BLOCK, None]
        dist = np.abs(ux[None, :] - x0)
        o = np.argsort(dist, axis=1, kind="stable")
        cs = np.cumsum(cnt[o], axis=1)
        at = (cs >= k).argmax(axis=1)
        rows = np.arange(dist.shape[0])
        h = dist[rows, o[rows, at]][:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            t = dist / h
            T = np.where(dist < h, (1.0 - t * t * t) ** 3, 0.0)
            W = (T * S0).sum(axis=1)[:, None]
            w = T * S0 / W
            xb = (w * ux).sum(axis=1)[:, None]
            e = ux[None, :] - xb
            v = (w * e * e).sum(axis=1)[:, None]
            lev = np.where(v > 0, 1.0 + (x0 - xb) * e / v, 1.0)
            terms = (T / W) * lev * S1
            f = terms.sum(axis=1)
            if cond is not None:
                kap = np.abs(terms).sum(axis=1) / np.abs(f)
                kap = kap[np.isfinite(kap)]
                worst = max(worst, float(kap.max())) if kap.size else worst
        out[b:b + _BLOCK] = np.where(W[:, 0] > 0, f, np.nan)
    if cond is not None:
        cond.append(worst)
    return out


def robustness_weights(y, f):
    """The bisquare weights of the residuals |y - f| against their median."""
    r = np.abs(y - f)
    m = np.median(r)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(r > 0, 1.0, 0.0) if m == 0 else np.minimum(r / (6 * m), 1.0)
    return (1 - u * u) ** 2


def lowess_host(ux, inv, y, xvals, frac=FRAC, it=IT, cond=None):
    """The curve at ``xvals`` of the points (ux[inv[i]], y[i]): ``ux`` the sorted distinct x,
    ``inv`` one index per point, ``y`` the points' values (a non-finite y is no point).  A fit at a
    data x whose window carries zero robustness weights only is NaN, and so are its points'
    residuals, their median and every later fit: the whole curve is NaN (numpy's propagation; the
    kernel does the same).  ``cond``: a list that receives the condition of every round's fits."""
    ux = np.ascontiguousarray(ux, dtype=np.float64)
    inv = np.asarray(inv).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    xvals = np.asarray(xvals, dtype=np.float64).reshape(-1)
    if inv.shape != y.shape:
        raise ValueError("one index per point")
    if ux.size == 0 or not np.isfinite(ux).all() or (np.diff(ux) <= 0).any():
        raise ValueError("ux must be finite and strictly increasing")
    if not np.isfinite(xvals).all():
        raise ValueError("xvals must be finite")
    ok = np.isfinite(y)
    inv, y = inv[ok], y[ok]
    U = len(ux)
    cnt = np.bincount(inv, minlength=U).astype(np.float64)
    k = lowess_k(len(y), frac)
    _check_bandwidth(ux, cnt, k, np.concatenate([ux, xvals]))
    d = np.ones_like(y)
    for _ in range(it + 1):
        fu = _regress(ux, cnt, np.bincount(inv, d, U), np.bincount(inv, d * y, U), k, ux, cond)
        d = robustness_weights(y, fu[inv])
    return _regress(ux, cnt, np.bincount(inv, d, U), np.bincount(inv, d * y, U), k, xvals, cond)


def _distinct(gc):
    gc = np.asarray(gc, dtype=np.float64).reshape(-1)
    if not np.isfinite(gc).all():
        raise ValueError("gc must be finite")
    ux, inv = np.unique(gc, return_inverse=True)
    return ux, inv.reshape(-1).astype(np.int32)


def lowess_matrix(gc, Y, xvals, frac=FRAC, it=IT, device=None):
    """The curve at ``xvals`` of the points (gc[l], Y[c, l]) on a GPU: ``gc`` (L,) finite, ``Y``
    (C, L) float64, array or tensor (one row per cell).  One call of ``pert_lowess_curve`` on
    ``device`` (default: Y's for a GPU tensor, else cuda) and its current stream; returns a numpy
    array.  There is no fallback: without the kernel this raises (``lowess_host`` is the CPU path)."""
    from . import _native
    if isinstance(Y, torch.Tensor):
        dev = torch.device(device) if device is not None else (Y.device if Y.is_cuda else torch.device("cuda"))
        Yt = Y
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda")
        Yt = torch.from_numpy(np.require(Y, dtype=np.float64, requirements=["C", "W"]))
    if dev.type != "cuda":
        raise ValueError("lowess_matrix is the kernel path and runs on a GPU; lowess_host is the CPU path")
    if Yt.dtype != torch.float64 or Yt.dim() != 2 or Yt.shape[0] < 1 or Yt.shape[1] < 1:
        raise ValueError("Y must be (C, L) float64 with at least one cell and one bin")
    ux, inv = _distinct(gc)
    C, L = Yt.shape
    if inv.shape[0] != L:
        raise ValueError("one gc value per column of Y")
    xv = np.ascontiguousarray(xvals, dtype=np.float64).reshape(-1)
    if not np.isfinite(xv).all():
        raise ValueError("xvals must be finite")
    if xv.size == 0:
        return np.empty(0)
    Yd = Yt.to(dev).contiguous()
    per_bin = torch.isfinite(Yd).sum(dim=0).cpu().numpy()
    cnt = np.bincount(inv, weights=per_bin, minlength=len(ux))
    k = lowess_k(int(per_bin.sum()), frac)
    _check_bandwidth(ux, cnt, k, np.concatenate([ux, xv]))
    lib = _native.lib()
    U, M = len(ux), len(xv)
    nbytes = ctypes.c_int64()
    _native.check(lib.pert_lowess_workspace(C, L, U, M, ctypes.byref(nbytes)), "pert_lowess_workspace")
    ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    out = torch.empty(M, dtype=torch.float64, device=dev)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _native.check(lib.pert_lowess_curve(C, L, U, M, Yd.data_ptr(), inv.ctypes.data_as(ip), ux.ctypes.data_as(dp),
                                            xv.ctypes.data_as(dp), k, int(it), out.data_ptr(), ws.data_ptr(),
                                            int(nbytes.value), ctypes.c_void_p(stream)), "pert_lowess_curve")
        res = out.cpu().numpy()               # the host arrays stay alive until the stream is through
    return res


def native_absmed(Y, inv, fit, device="cuda"):
    """``pert_lowess_absmed``: (lo, hi, n), the two middle order statistics of |Y[c, l] - fit[inv[l]]|
    over the finite Y and their number.  Y (C, L) float64, inv (L,) int32, fit (U,) float64."""
    from . import _native
    dev = torch.device(device)
    Yd = torch.as_tensor(np.ascontiguousarray(Y, dtype=np.float64)).to(dev).contiguous()
    inv = np.ascontiguousarray(inv, dtype=np.int32)
    fd = torch.as_tensor(np.ascontiguousarray(fit, dtype=np.float64)).to(dev)
    C, L = Yd.shape
    U = fd.shape[0]
    lib = _native.lib()
    nbytes = ctypes.c_int64()
    _native.check(lib.pert_lowess_workspace(C, L, U, 0, ctypes.byref(nbytes)), "pert_lowess_workspace")
    ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    med = torch.empty(2, dtype=torch.float64, device=dev)
    n = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _native.check(lib.pert_lowess_absmed(C, L, U, Yd.data_ptr(), inv.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                             fd.data_ptr(), med.data_ptr(), n.data_ptr(), ws.data_ptr(),
                                             int(nbytes.value), ctypes.c_void_p(stream)), "pert_lowess_absmed")
        m = med.cpu().numpy()
    return float(m[0]), float(m[1]), int(n.item())


# ----------------------------------------------------------------------------------------------
# the reference's functions on whole columns
# ----------------------------------------------------------------------------------------------

def compute_reads_per_million(cn, input_col='reads', rpm_col='rpm', cell_col='cell_id'):
    """bulk_gc_correction.py:21-26 on whole columns (in place, and returned): ``rpm_col`` float64 =
    (reads / the cell's total) * 1e6, the total summed in row order as the reference's ``sum()``
    does (exact for integer reads); -1 for a row without a cell."""
    v = cn[input_col].to_numpy()
    integral = v.dtype.kind in "iub"
    v = v.astype(np.int64) if integral else v.astype(np.float64)
    cells, order, offs = _cells(cn, cell_col)
    out = np.full(len(cn), -1.0)
    for L, sel, pos in _by_length(order, offs):
        if L == 0:
            continue
        vals = v[pos]                                        # (cells of this length, L)
        total = vals.sum(axis=1) if integral else np.cumsum(vals, axis=1)[:, -1]
        with np.errstate(invalid="ignore", divide="ignore"):
            out[pos] = (vals / total[:, None]) * 1E6
    cn[rpm_col] = out
    return cn


def predict_gc(curve, gc, gc_col='gc', pred_rpm_col='pred_rpm'):
    """bulk_gc_correction.py:29-31: the curve's value at ``gc`` (IndexError when it has none)."""
    at = np.flatnonzero(curve[gc_col].to_numpy() == gc)
    return curve[pred_rpm_col].to_numpy()[at[0]]


def _library_matrix(chunk, rpm_col, gc_col, cell_col):
    """(gc (L,), Y (C, L)) when every cell of the chunk holds the same GC values in the same row
    order, else None."""
    cells, order, offs = _cells(chunk, cell_col)
    lens = np.diff(offs)
    if len(cells) == 0 or lens[0] == 0 or (lens != lens[0]).any() or offs[-1] != len(chunk):
        return None
    C, L = len(cells), int(lens[0])
    gc = chunk[gc_col].to_numpy(dtype=np.float64)[order].reshape(C, L)
    if not np.isfinite(gc[0]).all() or (gc != gc[0]).any():
        return None
    return gc[0], np.ascontiguousarray(chunk[rpm_col].to_numpy(dtype=np.float64)[order].reshape(C, L))


def gc_curve(cn_g1_chunk, gc_vec, rpm_col='rpm', gc_col='gc', cell_col='cell_id', device=None, frac=FRAC, it=IT):
    """The LOWESS curve of one library's G1/2 rows at ``gc_vec`` (bulk_gc_correction.py:64-66).
    On a GPU a table whose cells share one list of bins is one ``lowess_matrix`` call; any other
    table, and the CPU, take ``lowess_host`` with one index per row."""
    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    gc_vec = np.asarray(gc_vec, dtype=np.float64)
    mat = _library_matrix(cn_g1_chunk, rpm_col, gc_col, cell_col) if dev.type == "cuda" else None
    if mat is not None:
        return lowess_matrix(mat[0], mat[1], gc_vec, frac=frac, it=it, device=dev)
    x = cn_g1_chunk[gc_col].to_numpy(dtype=np.float64)
    y = cn_g1_chunk[rpm_col].to_numpy(dtype=np.float64)
    ok = np.isfinite(x) & np.isfinite(y)                     # a non-finite x or y is no point
    if not ok.any():
        raise ValueError("no finite (gc, rpm) point to fit the curve to")
    ux, inv = np.unique(x[ok], return_inverse=True)
    return lowess_host(ux, inv.reshape(-1), y[ok], gc_vec, frac=frac, it=it)


def _corrected(chunk, gc_vec, pred, rpm_col, gc_col):
    """rpm / the curve at each row's gc.  A gc the curve has no value for is the reference's
    IndexError (predict_gc's ``values[0]`` of an empty selection)."""
    gc = chunk[gc_col].to_numpy(dtype=np.float64)
    at = pd.Index(gc_vec).get_indexer(gc)
    if (at < 0).any() or np.isnan(gc).any():
        raise IndexError("a row's {} value is not among the S-phase cells' of its library: the curve has no "
                         "prediction for it".format(gc_col))
    with np.errstate(invalid="ignore", divide="ignore"):
        return chunk[rpm_col].to_numpy(dtype=np.float64) / pred[at]


def bulk_g1_gc_correction(cn_s, cn_g1, input_col='reads', library_col='library_id', output_col='rpm_gc_norm',
                          gc_col='gc', cell_col='cell_id', device=None):
    """bulk_gc_correction.py:34-74: per library, the LOWESS curve of the G1/2 cells' rpm on GC,
    evaluated at the S-phase cells' distinct GC values, divides every row's rpm.  Returns
    (cn_s, cn_g1) with float64 ``rpm`` and ``output_col`` added (-1 in ``output_col`` for a row
    whose library has no S-phase cell); the caller's frames are not modified.  ``device``: where
    the curve is fitted (default: the GPU when there is one)."""
    rpm_col = 'rpm'
    cn_s = compute_reads_per_million(cn_s.copy(deep=False), input_col=input_col, rpm_col=rpm_col, cell_col=cell_col)
    cn_g1 = compute_reads_per_million(cn_g1.copy(deep=False), input_col=input_col, rpm_col=rpm_col, cell_col=cell_col)
    out_s, out_g = np.full(len(cn_s), -1.0), np.full(len(cn_g1), -1.0)
    lib_g = cn_g1[library_col].to_numpy()
    for lib_id, rows in cn_s.groupby(library_col, sort=True).indices.items():
        rows = np.sort(rows)
        s_chunk = cn_s.iloc[rows]
        g_rows = np.flatnonzero(lib_g == lib_id)
        g_chunk = cn_g1.iloc[g_rows]
        gc_vec = s_chunk[gc_col].unique()
        fin = np.isfinite(gc_vec)
        pred = np.full(len(gc_vec), np.nan)
        pred[fin] = gc_curve(g_chunk, gc_vec[fin], rpm_col=rpm_col, gc_col=gc_col, cell_col=cell_col, device=device)
        out_s[rows] = _corrected(s_chunk, gc_vec, pred, rpm_col, gc_col)
        out_g[g_rows] = _corrected(g_chunk, gc_vec, pred, rpm_col, gc_col)
    cn_s[output_col] = out_s
    cn_g1[output_col] = out_g
    return cn_s, cn_g1
