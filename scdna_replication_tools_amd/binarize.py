"""Threshold binarisation of RT profiles (Dileep & Gilbert, Nat. Commun. 2018; reference
scdna_replication_tools/binarize_rt_profiles.py:22-121) and the per-clone normalisation that
feeds it (normalize_by_clone.py:22-77), for every cell at once.

The reference loops over cells: one ``GaussianMixture(n_components=2, random_state=0)`` fit of
the cell's float64 profile, the two binary levels (the GMM means, or percentiles chosen by the
skew when the means are closer than MEAN_GAP_THRESH), a scan of ``np.linspace(-3, 3, 100)`` for
the first threshold of least Manhattan distance between the profile and its binarisation, and a
dozen ``cn.loc`` column writes -- about 90 ms per cell.

Here (``binarize_matrix``) all cells of one length are one launch of ``pert_rt_binarize``
(csrc/bin_kernels.hip, fp64, one workgroup per cell) on a GPU, or the same algorithm as a tensor
program on the CPU (``tensor_binarize``: tau_init's k-means++ / Lloyd / EM functions on the raw
profile, with this module's margins).  Both mark every cell in which a decision sits within its
rounding margin of flipping under another summation order (``margins``); those cells are
recomputed on the host with the reference's own library calls (``exact_cell``), so every cell's
discrete outputs are the reference's.  ``binarize_profiles`` is the reference's DataFrame entry
point on top: rows grouped by cell, cells grouped by length, whole-column writes.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import pandas as pd
import torch

from . import tau_init
from ._native import (BIN_F_EM, BIN_F_LEVELS, BIN_F_LLOYD, BIN_F_POINT, BIN_F_PP, BIN_F_RESP, BIN_F_SCAN,
                      BIN_THRESHOLDS)

EPS = float(np.finfo(np.float64).eps)
OUT_COLS = ("mean_0", "covariance_0", "mean_1", "covariance_1", "gmm_state")


def thresholds() -> np.ndarray:
    """The reference's fixed thresholds (binarize_rt_profiles.py:89)."""
    return np.linspace(-3, 3, BIN_THRESHOLDS)


def margins(L: int) -> dict:
    """Margins of an fp64-vs-fp64 comparison at L bins: sklearn / numpy
    and this module sum the same fp64 terms in different orders, so a sum of L terms differs by at
    most L eps of the sum of their magnitudes (first order), and each margin is that bound times
    the quantity's sensitivity, times a safety factor of 8."""
    le = L * EPS
    return dict(
        pp_margin=8 * le,          # cumulative sum / potential: L terms, relative to the potential
        tie_margin=64 * le,        # label rule c^2 - 2 x c: centres carry L eps, three terms, cancellation <= 8
        lloyd_margin=4096 * le,    # shift ~ tol = 1e-4 var: d shift / tol <= 2 |dc| L eps max|x| / tol ~ 200 (max|x| / sd) L eps
        em_margin=1024 * le,       # lower bound: a mean of L O(1..10) terms + parameters carrying ~10 L eps each
        gap_margin=256 * le,       # EM means after <= 100 iterations, relative to max(1, |mu0| + |mu1|)
        skew_margin=256 * le,      # m3 / m2^1.5: two sums of L terms, O(1) value
        resp_margin=256 * le,      # (x - mu)^2 / var with parameters carrying ~10 L eps, relative to 1 + |l0| + |l1|
        thresh_margin=0.0,         # X and np.linspace's thresholds are the reference's bits: X > t is exact
        dist_margin=64 * le,       # sum of L terms, levels moved by ~10 L eps: relative to least + L max|level|
    )


def bin_params(L: int, MEAN_GAP_THRESH=0.7, EARLY_S_SKEW_THRESH=0.2, LATE_S_SKEW_THRESH=-0.2):
    """The pert_bin_params at L bins: the RandomState(0) draws and percentile positions of this
    length, the reference's thresholds and sklearn's defaults, and ``margins(L)``."""
    from ._native import PertBinParams
    first, u = tau_init._rng_draws(L)
    p = PertBinParams()
    p.first, p.lloyd_max_iter, p.em_max_iter = first, 300, 100
    tau_init.set_percentile_positions(p, L)
    p.u[0], p.u[1] = float(u[0]), float(u[1])
    p.em_tol, p.reg_covar = 1e-3, 1e-6
    p.mean_gap, p.early_skew, p.late_skew = float(MEAN_GAP_THRESH), float(EARLY_S_SKEW_THRESH), float(LATE_S_SKEW_THRESH)
    for i, t in enumerate(thresholds()):
        p.thresh[i] = float(t)
    for k, v in margins(L).items():
        setattr(p, k, v)
    return p


def native_binarize(X: torch.Tensor, p) -> dict:
    """One launch of pert_rt_binarize on X's device and current stream.  X (L, N) float64 on a
    GPU; returns device tensors: means, covs (N, 2), gmm_state int8 and rt_state uint8 (N, L),
    dist (N, 100), best, n_rep, flags int32 (N,)."""
    from . import _native
    L, N = X.shape
    dev = X.device
    rows = X.T.contiguous()                                          # (N, L): one row per cell
    out = dict(means=torch.empty((N, 2), dtype=torch.float64, device=dev),
               covs=torch.empty((N, 2), dtype=torch.float64, device=dev),
               gmm_state=torch.empty((N, L), dtype=torch.int8, device=dev),
               rt_state=torch.empty((N, L), dtype=torch.uint8, device=dev),
               dist=torch.empty((N, BIN_THRESHOLDS), dtype=torch.float64, device=dev),
               best=torch.empty(N, dtype=torch.int32, device=dev),
               n_rep=torch.empty(N, dtype=torch.int32, device=dev),
               flags=torch.empty(N, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _native.check(_native.lib().pert_rt_binarize(
            L, N, rows.data_ptr(), ctypes.byref(p), out["means"].data_ptr(), out["covs"].data_ptr(),
            out["gmm_state"].data_ptr(), out["rt_state"].data_ptr(), out["dist"].data_ptr(), out["best"].data_ptr(),
            out["n_rep"].data_ptr(), out["flags"].data_ptr(), ctypes.c_void_p(stream)), "pert_rt_binarize")
    return out


def tensor_binarize(X: torch.Tensor, p, return_kmeans: bool = False) -> dict:
    """What pert_rt_binarize computes, as one tensor program over the columns of X (L, N)
    float64 on any device (the CPU path of ``binarize_matrix``, and the kernel's check): the
    same stages, decisions, margins and flag bits, the same layout of the results."""
    L, N = X.shape
    dev = X.device
    flags = torch.zeros(N, dtype=torch.int32, device=dev)

    def mark(mask, bit):
        flags.bitwise_or_(mask.to(torch.int32) * bit)

    # KMeans: tolerance from the uncentred data, centring, k-means++, Lloyd
    Xc = X - X.mean(0)
    tol = Xc.pow(2).mean(0) * 1e-4
    u = np.array([p.u[0], p.u[1]])
    frag = torch.zeros(N, dtype=torch.bool, device=dev)
    cen = tau_init._kmeans_pp(Xc, int(p.first), u, frag, None, pp_margin=p.pp_margin)
    mark(frag, BIN_F_PP)
    frag = torch.zeros(N, dtype=torch.bool, device=dev)
    lab1 = tau_init._lloyd(Xc, cen, tol, max_iter=int(p.lloyd_max_iter), fragile=frag, fragile_rel=p.lloyd_margin,
                           boundary=p.tie_margin)
    mark(frag, BIN_F_LLOYD)
    # EM and fit_predict's final E step
    frag = torch.zeros(N, dtype=torch.bool, device=dev)
    w, mu, var = tau_init._gmm_fit(X, lab1, max_iter=int(p.em_max_iter), tol=p.em_tol, reg_covar=p.reg_covar,
                                   fragile=frag, em_margin=p.em_margin)
    mark(frag, BIN_F_EM)
    wlp = tau_init._gmm_log_prob(X, w, mu, var)
    gmm_state = (wlp[1] > wlp[0]).to(torch.int8)
    mark(((wlp[1] - wlp[0]).abs() <= p.resp_margin * (1 + wlp[0].abs() + wlp[1].abs())).any(0), BIN_F_RESP)
    # levels
    gap = (mu[0] - mu[1]).abs()
    b0, b1 = torch.minimum(mu[0], mu[1]), torch.maximum(mu[0], mu[1])
    close = gap < p.mean_gap
    mark((gap - p.mean_gap).abs() <= p.gap_margin * (mu[0].abs() + mu[1].abs()).clamp(min=1.0), BIN_F_LEVELS)
    if bool(close.any()):
        skew = Xc.pow(3).mean(0) / Xc.pow(2).mean(0) ** 1.5
        mark(close & (((skew - p.early_skew).abs() <= p.skew_margin) | ((skew - p.late_skew).abs() <= p.skew_margin)),
             BIN_F_LEVELS)
        early = close & (skew > p.early_skew)
        late = close & ~early & (skew < p.late_skew)
        mid = close & ~early & ~late
        qs = tau_init._percentiles(X, tau_init.QS)
        b0 = torch.where(early, qs[2], torch.where(late, qs[0], torch.where(mid, qs[1], b0)))
        b1 = torch.where(early, qs[4], torch.where(late, qs[2], torch.where(mid, qs[3], b1)))
    # the scan
    th = torch.as_tensor(np.array(p.thresh[:]), dtype=X.dtype, device=dev)
    dist = torch.empty((BIN_THRESHOLDS, N), dtype=X.dtype, device=dev)
    cnt = torch.empty((BIN_THRESHOLDS, N), dtype=torch.int64, device=dev)
    chunk = max(1, int(5e7 // (BIN_THRESHOLDS * L)))
    for s in range(0, N, chunk):
        xs = X[:, s:s + chunk]
        hi = xs[None] > th[:, None, None]                                # (100, L, n)
        dist[:, s:s + chunk] = torch.where(hi, (xs - b1[s:s + chunk]).abs()[None], (xs - b0[s:s + chunk]).abs()[None]).sum(1)
        cnt[:, s:s + chunk] = hi.sum(1)
    best = dist.argmin(0)                                                # first minimum
    dmin = dist.gather(0, best[None])[0]
    cbest = cnt.gather(0, best[None])[0]
    slack = p.dist_margin * (dmin + L * torch.maximum(b0.abs(), b1.abs()))
    mark(((cnt != cbest[None]) & (dist - dmin[None] <= slack[None])).any(0), BIN_F_SCAN)
    tbest = th[best]
    if p.thresh_margin > 0.0:
        mark(((X - tbest[None]).abs() <= p.thresh_margin).any(0), BIN_F_POINT)
    out = dict(means=mu.T.contiguous(), covs=var.T.contiguous(), gmm_state=gmm_state.T.contiguous(),
               rt_state=(X > tbest[None]).to(torch.uint8).T.contiguous(), dist=dist.T.contiguous(),
               best=best.to(torch.int32), n_rep=cbest.to(torch.int32), flags=flags)
    if return_kmeans:
        out["kmeans"] = lab1.T.contiguous()
    return out


def exact_cell(x: np.ndarray, MEAN_GAP_THRESH=0.7, EARLY_S_SKEW_THRESH=0.2, LATE_S_SKEW_THRESH=-0.2):
    """One cell the reference's way (binarize_rt_profiles.py:46-113), with the library calls it
    makes: sklearn's GaussianMixture on the float64 column, scipy's skew, numpy's percentiles and
    the scan's fp64 sums.  Returns (means (2,), covariances (2,), gmm_state, rt_state, distances
    (100,), index of the chosen threshold)."""
    from scipy.stats import skew
    from sklearn.mixture import GaussianMixture
    x = np.ascontiguousarray(x, dtype=np.float64)
    gm = GaussianMixture(n_components=2, random_state=0)
    states = gm.fit_predict(x.reshape(-1, 1))
    mu = gm.means_[:, 0].copy()
    lo, hi = min(mu[0], mu[1]), max(mu[0], mu[1])
    if abs(mu[0] - mu[1]) < MEAN_GAP_THRESH:
        sk = skew(x)
        qa, qb = (50, 95) if sk > EARLY_S_SKEW_THRESH else ((5, 50) if sk < LATE_S_SKEW_THRESH else (25, 75))
        lo, hi = np.percentile(x, qa), np.percentile(x, qb)
    d = np.array([np.abs(x - np.where(x > t, hi, lo)).sum() for t in thresholds()])
    bi = int(np.argmin(d))                                               # first strict minimum
    return mu, gm.covariances_[:, 0, 0].copy(), states, (x > thresholds()[bi]), d, bi


@dataclass
class Binarized:
    """``binarize_matrix``'s result for the N cells (columns) of an (L, N) matrix."""
    means: np.ndarray          # (N, 2) GMM means, sklearn's component order (unsorted)
    covariances: np.ndarray    # (N, 2) GMM variances, reg_covar included
    gmm_state: np.ndarray      # (L, N) int8, the GMM's label per bin
    rt_state: np.ndarray       # (L, N) uint8, the binary replication state
    frac_rt: np.ndarray        # (N,) replicated bins / L
    best_thresh: np.ndarray    # (N,) the chosen threshold
    manhattan: np.ndarray      # (N, 100) distance per threshold
    thresholds: np.ndarray     # (100,)
    flagged: np.ndarray        # (N,) bool: recomputed on the host
    flags: np.ndarray          # (N,) int32: the batched pass's flag bits


def binarize_matrix(X, *, MEAN_GAP_THRESH=0.7, EARLY_S_SKEW_THRESH=0.2, LATE_S_SKEW_THRESH=-0.2, device=None,
                    exact: bool = True) -> Binarized:
    """binarize_rt_profiles.py:44-117 for every column (cell) of X, an (L, N) float64 tensor or
    array.  ``device``: where the batched pass runs (default: X's device for a tensor, else the
    GPU when there is one); on a GPU it is one launch of pert_rt_binarize, on the CPU the tensor
    program.  Flagged cells are then recomputed by ``exact_cell`` (``exact=False`` leaves the
    batched pass's results: measurement and tests)."""
    if isinstance(X, torch.Tensor):
        if X.dtype != torch.float64:
            raise TypeError("binarize_matrix compares float64 values against the thresholds: X must be float64")
        dev = torch.device(device) if device is not None else X.device
        Xt = X.to(dev)
    else:
        X = np.asarray(X)
        if X.dtype != np.float64:
            raise TypeError("binarize_matrix compares float64 values against the thresholds: X must be float64")
        dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        Xt = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    if Xt.ndim != 2 or Xt.shape[0] < 2 or Xt.shape[1] < 1:
        raise ValueError("X must be (L, N) with L >= 2 bins and N >= 1 cells")
    if not bool(torch.isfinite(Xt).all()):
        raise ValueError("Input X contains NaN or infinity")
    L, N = Xt.shape
    p = bin_params(L, MEAN_GAP_THRESH, EARLY_S_SKEW_THRESH, LATE_S_SKEW_THRESH)
    raw = native_binarize(Xt, p) if dev.type == "cuda" else tensor_binarize(Xt, p)
    r = {k: v.cpu().numpy() for k, v in raw.items()}
    th = thresholds()
    means, covs, dist, best = r["means"], r["covs"], r["dist"], r["best"].astype(np.int64)
    gmm_state, rt_state, n_rep = r["gmm_state"].T.copy(), r["rt_state"].T.copy(), r["n_rep"].astype(np.int64)
    flagged = r["flags"] != 0
    if exact and flagged.any():
        idx = np.flatnonzero(flagged)
        cols = Xt[:, torch.as_tensor(idx, device=dev)].T.cpu().numpy()
        with tau_init.host_threads():                # library scans up front; sklearn on this one thread
            for j, n in enumerate(idx):
                mu, cv, gs, rs, d, bi = exact_cell(cols[j], MEAN_GAP_THRESH, EARLY_S_SKEW_THRESH, LATE_S_SKEW_THRESH)
                means[n], covs[n], dist[n], best[n] = mu, cv, d, bi
                gmm_state[:, n], rt_state[:, n], n_rep[n] = gs, rs, int(rs.sum())
    return Binarized(means=means, covariances=covs, gmm_state=gmm_state, rt_state=rt_state,
                     frac_rt=n_rep / L, best_thresh=th[best], manhattan=dist, thresholds=th, flagged=flagged,
                     flags=r["flags"])


def binarize_profiles(cn, input_col, rs_col='rt_state', frac_rt_col='frac_rt', thresh_col='binary_thresh',
                      cell_col='cell_id', MEAN_GAP_THRESH=0.7, EARLY_S_SKEW_THRESH=0.2, LATE_S_SKEW_THRESH=-0.2, *,
                      device=None):
    """binarize_rt_profiles.py:22-121: adds to ``cn`` (in place, as the reference does, and
    returns it) the float64 columns mean_0, covariance_0, mean_1, covariance_1, gmm_state,
    ``rs_col``, ``frac_rt_col`` and ``thresh_col``, and returns with it the table of Manhattan
    distances (thresh, manhattan_dist, cell_id, best_thresh; 100 rows per cell, cells in sorted
    order, index 0..99 repeating).  Rows are grouped by cell in row order (groupby semantics; rows
    whose cell is NaN belong to no cell and keep NaN); cells of one length are one batched pass.
    The reference's ``cell_skew`` prints are not made."""
    from .predict_cycle_phase import _segments
    vals = cn[input_col].to_numpy(dtype=np.float64)
    ids = cn[cell_col].to_numpy()
    has = ~pd.isna(ids)
    rows_all = np.flatnonzero(has)
    if not np.isfinite(vals[rows_all]).all():
        raise ValueError("Input X contains NaN or infinity ('{}')".format(input_col))
    cells, codes, order, offs = _segments(ids[rows_all])
    order = rows_all[order]                                   # row positions grouped by sorted cell
    lens = np.diff(offs)
    if len(lens) and lens.min() < 2:
        raise ValueError("a cell with fewer than 2 rows cannot be binarised (2 mixture components)")
    n_cells, n_rows = len(cells), len(cn)
    cols = {c: np.full(n_rows, np.nan) for c in OUT_COLS + (rs_col, frac_rt_col, thresh_col)}
    man = np.empty((n_cells, BIN_THRESHOLDS))
    best_t = np.empty(n_cells)
    for L in np.unique(lens):
        sel = np.flatnonzero(lens == L)
        pos = order[offs[sel][:, None] + np.arange(L)[None, :]]           # (n, L) row positions
        res = binarize_matrix(np.ascontiguousarray(vals[pos].T), MEAN_GAP_THRESH=MEAN_GAP_THRESH,
                              EARLY_S_SKEW_THRESH=EARLY_S_SKEW_THRESH, LATE_S_SKEW_THRESH=LATE_S_SKEW_THRESH,
                              device=device)
        per_cell = lambda a: np.broadcast_to(np.asarray(a, np.float64)[:, None], pos.shape)
        cols["mean_0"][pos], cols["mean_1"][pos] = per_cell(res.means[:, 0]), per_cell(res.means[:, 1])
        cols["covariance_0"][pos], cols["covariance_1"][pos] = per_cell(res.covariances[:, 0]), per_cell(res.covariances[:, 1])
        cols["gmm_state"][pos] = res.gmm_state.T
        cols[rs_col][pos] = res.rt_state.T
        cols[frac_rt_col][pos] = per_cell(res.frac_rt)
        cols[thresh_col][pos] = per_cell(res.best_thresh)
        man[sel], best_t[sel] = res.manhattan, res.best_thresh
    for c in ("mean_0", "covariance_0", "mean_1", "covariance_1", "gmm_state", rs_col, frac_rt_col, thresh_col):
        cn[c] = cols[c]
    manhattan_df = pd.DataFrame({"thresh": np.tile(thresholds(), n_cells), "manhattan_dist": man.reshape(-1),
                                 "cell_id": np.repeat(np.asarray(cells), BIN_THRESHOLDS),
                                 "best_thresh": np.repeat(best_t, BIN_THRESHOLDS)},
                                index=np.tile(np.arange(BIN_THRESHOLDS), n_cells))
    return cn, manhattan_df


# ----------------------------------------------------------------------------------------------
# normalize_by_clone.py
# ----------------------------------------------------------------------------------------------

def _clone_quotient(values: np.ndarray, profile: np.ndarray) -> np.ndarray:
    return values / (profile + np.finfo(float).eps)


def cell_clone_norm(clone_profiles, cell_cn, clone_id, input_col, output_col, chr_col='chr', start_col='start'):
    """normalize_by_clone.py:22-48 for one cell: ``cell_cn`` and ``clone_profiles`` indexed by
    (chr, start); the cell's rows whose ``input_col`` is finite and whose locus the clone's
    profile has (not NaN), in the cell's row order, with ``output_col`` = value / (profile + eps)
    and the index back as the first columns.  Neither argument is modified."""
    li = clone_profiles.index.get_indexer(cell_cn.index)
    v = cell_cn[input_col].to_numpy(dtype=np.float64)
    prof = clone_profiles[clone_id].to_numpy(dtype=np.float64)[np.where(li >= 0, li, 0)]
    keep = (li >= 0) & np.isfinite(v) & ~np.isnan(prof)
    out = cell_cn[keep].copy()
    out[output_col] = _clone_quotient(v[keep], prof[keep])
    return out.reset_index()


def normalize_by_clone(cn_s, clone_profiles, input_col='rpm_gc_norm', clone_col='clone_id', cell_col='cell_id',
                       output_col='rt_value', chr_col='chr', start_col='start', cn_state_col='state',
                       ploidy_col='ploidy'):
    """normalize_by_clone.py:51-77 on whole columns: rows with a NaN dropped from both tables,
    ``ploidy_col`` = the cell's most frequent ``cn_state_col``, every cell's ``input_col`` divided
    by its clone's profile at the same (chr, start) (inner join; non-finite cell values dropped),
    cells concatenated in sorted order with a fresh index.  Columns come out as the reference
    leaves them: chr, start, cell, the other columns in their order, ploidy, ``output_col``.  The
    caller's frames are not modified (the reference drops their NaN rows in place)."""
    from . import prep
    s = cn_s.dropna()
    prof = clone_profiles.dropna()
    if not set([chr_col, start_col]).issubset(set(prof.index.names)):
        prof = prof.reset_index().set_index([chr_col, start_col])
    codes, cells = pd.factorize(s[cell_col].to_numpy(), sort=True)
    order = np.argsort(codes, kind="stable")                  # rows grouped by sorted cell, in row order
    s = s.iloc[order]
    codes = codes[order]
    ploidy = prep._cell_mode(codes, len(cells), s[cn_state_col].to_numpy())
    # the cell's clone is its first row's (normalize_by_clone.py:68)
    starts = np.flatnonzero(np.r_[True, codes[1:] != codes[:-1]])
    clone_of_cell = s[clone_col].to_numpy()[starts]
    missing = [c for c in pd.unique(clone_of_cell) if c not in prof.columns]
    if missing:
        raise KeyError(missing[0])
    ccol = prof.columns.get_indexer(clone_of_cell)[codes]
    li = prof.index.get_indexer(pd.MultiIndex.from_arrays([s[chr_col].to_numpy(), s[start_col].to_numpy()]))
    v = s[input_col].to_numpy(dtype=np.float64)
    pv = prof.to_numpy(dtype=np.float64)[np.where(li >= 0, li, 0), ccol]
    keep = (li >= 0) & np.isfinite(v) & ~np.isnan(pv)
    rest = [c for c in s.columns if c not in (chr_col, start_col, cell_col)]
    out = s[[chr_col, start_col, cell_col] + rest][keep].reset_index(drop=True)
    out[ploidy_col] = ploidy[codes][keep].astype(np.float64)      # appended, or overwritten in its place
    out[output_col] = _clone_quotient(v[keep], pv[keep])
    return out
