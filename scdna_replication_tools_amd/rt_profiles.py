"""Pseudobulk replication-timing profiles and T-width from the decoded replication states.

Reference: scdna_replication_tools/compute_pseudobulk_rt_profiles.py (population and per-clone
mean of the state per locus, rescaled to 0-10 h) and calculate_twidth.py (the share of
replicated rows in each of 200 intervals of time from scheduled replication, and the width of
its sigmoid or linear fit).  The reference builds one DataFrame per locus and scans the long
table once per interval; here

* the DataFrame layer (same names, arguments, defaults, return values, column names, row
  order and dtypes) factorises the keys once and works on ``bincount`` / ``searchsorted`` of
  the whole columns -- any table the reference accepts, on the host;
* the matrix layer, ``RTMatrix``, holds the bins x cells state matrix itself (the decode's
  ``uint8 [L][ldn]`` on the GPU, or a numpy array) and never forms the long table: every row's
  time from scheduled replication is ``hours[group(cell)][bin] - 10 frac[cell]``, so the two
  O(L N) passes are the HIP kernels ``pert_rt_counts`` / ``pert_rt_tfs_hist`` (integer counts;
  csrc/rt_kernels.hip), or a chunked numpy pass with the same counts when there is no GPU.
  The host turns the counts into fractions and hours with the reference's own operations.

Both layers reproduce the reference's rounding: the mean of a float32 state column is the
float32 count over the row count (numpy divides in float64 and rounds once more, which for a
quotient of two float32 values equals the directly rounded float32 quotient), the 0-10 h scale
is evaluated in the column's dtype, and an interval test ``a <= t < b`` compares in the
dtype of ``t`` with the edge rounded to it.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import pandas as pd

N_INTERVALS = 200
_CHUNK_ELEMS = 1 << 22          # (bin, cell) pairs per chunk of the host passes


def interval_edges() -> np.ndarray:
    """The 201 fp64 edges of the time-from-scheduled-replication intervals (calculate_twidth.py:51)."""
    return np.linspace(-10, 10, N_INTERVALS + 1)


# ----------------------------------------------------------------------------------------------
# shared arithmetic: counts -> the reference's values
# ----------------------------------------------------------------------------------------------

def _mean_from_sums(sums: np.ndarray, counts: np.ndarray, dtype) -> np.ndarray:
    """np.mean of a column of ``dtype`` per group, from the groups' exact sums and sizes:
    numpy forms ``dtype(sum) / intp(count)`` in float64 and rounds to ``dtype``."""
    dtype = np.dtype(dtype)
    acc = dtype if dtype.kind == "f" else np.dtype(np.float64)           # integer columns are averaged in float64
    s = np.asarray(sums).astype(acc).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (s / np.asarray(counts, np.float64)).astype(acc)


def _hours_from_profile(values: np.ndarray) -> np.ndarray:
    """The 0-10 h scale of a pseudobulk profile (latest locus = 10), in the profile's dtype; a
    constant profile gives NaN, as the reference's division by zero does."""
    v = np.asarray(values)
    if v.size == 0:
        return v.copy()
    late = v - max(v)                     # builtin max, as the reference: <= 0
    late *= -1
    with np.errstate(invalid="ignore", divide="ignore"):
        late = late / max(late)
    late *= 10
    return late


def _tfs_dtype(hours_dtype, frac_dtype):
    return np.result_type(np.dtype(hours_dtype), np.dtype(frac_dtype))


def _lists_from_hist(hist_n, hist_rep, left_edges, cell_order=None):
    """(time_bins, pct_reps) as the reference lists them: the left edge of every non-empty
    interval (interval-major, then cells in sorted id order) and sum / count as Python floats."""
    hist_n, hist_rep = np.asarray(hist_n), np.asarray(hist_rep)
    if hist_n.ndim == 1:
        keep = np.flatnonzero(hist_n > 0)
        tb = left_edges[keep]
        num, den = hist_rep[keep], hist_n[keep]
    else:                                                               # [cells][intervals]
        hn, hr = hist_n[cell_order].T, hist_rep[cell_order].T           # -> [intervals][sorted cells]
        ii, cc = np.nonzero(hn > 0)
        tb = left_edges[ii]
        num, den = hr[ii, cc], hn[ii, cc]
    pct = np.asarray(num, np.float64) / np.asarray(den, np.float64)
    return list(tb), pct.tolist()


# ----------------------------------------------------------------------------------------------
# DataFrame layer: compute_pseudobulk_rt_profiles.py
# ----------------------------------------------------------------------------------------------

def _is_small_integers(v: np.ndarray) -> bool:
    if v.dtype.kind in "biu":
        return v.size == 0 or int(np.abs(v.astype(np.int64)).max()) < (1 << 20)
    if v.dtype.kind != "f" or v.size == 0:
        return v.dtype.kind == "f"
    return bool(np.all(np.isfinite(v)) and np.all(v == np.rint(v)) and np.abs(v).max() < (1 << 20))


def _locus_codes(cn: pd.DataFrame, chr_col: str, start_col: str):
    """Row -> locus index in the reference's groupby order (sorted by chr, then start; rows with a
    missing key dropped, code -1), and the loci's key values."""
    c_codes, c_uni = pd.factorize(cn[chr_col], sort=True)
    s_codes, s_uni = pd.factorize(cn[start_col], sort=True)
    ok = (c_codes >= 0) & (s_codes >= 0)
    key = c_codes.astype(np.int64) * max(len(s_uni), 1) + s_codes
    uni, inv = np.unique(key[ok], return_inverse=True)
    codes = np.full(len(cn), -1, np.int64)
    codes[ok] = inv
    chrom = np.asarray(c_uni)[uni // max(len(s_uni), 1)] if len(uni) else np.asarray(c_uni)[:0]
    start = np.asarray(s_uni)[uni % max(len(s_uni), 1)] if len(uni) else np.asarray(s_uni)[:0]
    return codes, chrom, start


def _group_means(values: np.ndarray, codes: np.ndarray, n_groups: int):
    """np.mean(values[codes == k]) for every k that occurs, bit for bit: exact integer sums where
    the column holds small integers (a 0/1 state), else numpy's own mean of each group's rows
    in their table order.  Returns (means over the occurring groups, their indices)."""
    sel = codes >= 0
    v, c = values[sel], codes[sel]
    counts = np.bincount(c, minlength=n_groups)
    present = np.flatnonzero(counts > 0)
    if _is_small_integers(v):
        sums = np.bincount(c, weights=v.astype(np.float64), minlength=n_groups)      # exact
        return _mean_from_sums(sums[present], counts[present], v.dtype), present
    order = np.argsort(c, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(counts[present])])
    vs = v[order]
    means = [np.mean(vs[bounds[i]:bounds[i + 1]]) for i in range(len(present))]
    return np.asarray(means, dtype=np.result_type(*means) if means else v.dtype), present


def _population_rt(values, codes, chrom, start, output_col, time_col, chr_col, start_col):
    means, present = _group_means(values, codes, len(chrom))
    out = pd.DataFrame({chr_col: chrom[present], start_col: start[present], output_col: means})
    out[time_col] = _hours_from_profile(means)
    return out


def calc_population_rt(cn, input_col, output_col, time_col='rt_hours', chr_col='chr', start_col='start'):
    """Mean of ``input_col`` per locus, sorted by (chr, start), and its 0-10 h timing scale
    (compute_pseudobulk_rt_profiles.py:16-38)."""
    codes, chrom, start = _locus_codes(cn, chr_col, start_col)
    return _population_rt(cn[input_col].to_numpy(), codes, chrom, start, output_col, time_col, chr_col, start_col)


def compute_pseudobulk_rt_profiles(cn, input_col, output_col='pseudobulk', time_col='hours', clone_col='clone_id',
                                   chr_col='chr', start_col='start'):
    """Population- and clone-level pseudobulk replication timing profiles
    (compute_pseudobulk_rt_profiles.py:41-69).  As in the reference, the loci are keyed by the
    columns 'chr' and 'start' whatever ``chr_col`` / ``start_col`` say, and each clone's table is
    inner-merged, so a locus missing from any clone leaves the result."""
    chr_col, start_col = 'chr', 'start'
    codes, chrom, start = _locus_codes(cn, chr_col, start_col)
    values = cn[input_col].to_numpy()
    bulk_cn = _population_rt(values, codes, chrom, start, '{}_{}'.format(output_col, input_col),
                             '{}_{}'.format(output_col, time_col), chr_col, start_col)
    if clone_col is not None:
        k_codes, k_uni = pd.factorize(cn[clone_col], sort=True)
        for k, clone_id in enumerate(k_uni):
            clone_codes = np.where(k_codes == k, codes, -1)
            clone_cn = _population_rt(values, clone_codes, chrom, start,
                                      '{}_clone{}_{}'.format(output_col, clone_id, input_col),
                                      '{}_clone{}_{}'.format(output_col, clone_id, time_col), chr_col, start_col)
            bulk_cn = pd.merge(bulk_cn, clone_cn)
    return bulk_cn


# ----------------------------------------------------------------------------------------------
# DataFrame layer: calculate_twidth.py
# ----------------------------------------------------------------------------------------------

def compute_time_from_scheduled_column(cn, pseudobulk_col='pseudobulk_hours', frac_rt_col='frac_rt',
                                       tfs_col='time_from_scheduled_rt'):
    """Adds ``tfs_col`` = hours of the locus in pseudobulk - 10 x the cell's replicated fraction,
    in place (calculate_twidth.py:23-34)."""
    elapsed = cn[frac_rt_col] * 10.0
    cn[tfs_col] = cn[pseudobulk_col] - elapsed
    return cn


def _interval_index(t: np.ndarray) -> np.ndarray:
    """Interval of each value (edges[i] <= t < edges[i+1], compared in t's dtype), -1 for none."""
    t = np.asarray(t)
    edges = interval_edges()
    if t.dtype.kind == "f":
        edges = edges.astype(t.dtype)
    idx = np.searchsorted(edges, t, side="right") - 1
    idx[(idx >= N_INTERVALS) | np.isnan(t.astype(np.float64, copy=False))] = -1
    return idx


def calc_pct_replicated_per_time_bin(cn, tfs_col='time_from_scheduled_rt', rs_col='rt_state', per_cell=False,
                                     query2=None, cell_col='cell_id',):
    """Share of replicated rows in each 0.1 h interval of time from scheduled replication
    (calculate_twidth.py:37-71): (time_bins, pct_reps), empty intervals omitted; with
    ``per_cell`` one point per (interval, cell).  ``query2`` is evaluated once on the whole
    table (a row-wise condition selects the same rows as the reference's per-interval query)."""
    idx = _interval_index(cn[tfs_col].to_numpy())
    keep = idx >= 0
    if query2:
        keep &= np.asarray(cn.eval(query2), dtype=bool)
    rs = cn[rs_col].to_numpy()
    left = interval_edges()[:-1]
    if not per_cell:
        hist_n = np.bincount(idx[keep], minlength=N_INTERVALS)
        hist_rep = np.bincount(idx[keep], weights=rs[keep].astype(np.float64), minlength=N_INTERVALS)
        return _lists_from_hist(hist_n, hist_rep, left)
    cells, cell_uni = pd.factorize(cn[cell_col], sort=True)
    keep &= cells >= 0
    n_cells = max(len(cell_uni), 1)
    key = cells[keep].astype(np.int64) * N_INTERVALS + idx[keep]
    hist_n = np.bincount(key, minlength=n_cells * N_INTERVALS).reshape(n_cells, N_INTERVALS)
    hist_rep = np.bincount(key, weights=rs[keep].astype(np.float64),
                           minlength=n_cells * N_INTERVALS).reshape(n_cells, N_INTERVALS)
    return _lists_from_hist(hist_n, hist_rep, left, cell_order=np.arange(n_cells))


def sigmoid(x, x0, k, b):
    """Logistic curve with midpoint x0, rate k and offset b."""
    return 1 / (1 + np.exp(-k * (x - x0))) + b


def inv_sigmoid(y, x0, k, b):
    odds = (1 / (y - b)) - 1
    return (np.log(odds) / -k) + x0


def fit_sigmoid(xdata, ydata):
    from scipy.optimize import curve_fit
    start = [np.median(xdata), 1, 0.0]
    return curve_fit(sigmoid, xdata, ydata, start, method='dogbox')


def calc_t_width(popt, low=0.25, high=0.75):
    """(t_width, left_time, right_time): where the fitted sigmoid crosses ``high`` and ``low``."""
    right_time = inv_sigmoid(low, *popt)
    left_time = inv_sigmoid(high, *popt)
    return right_time - left_time, left_time, right_time


def linear(x, m, b):
    return m * x + b


def inv_linear(y, m, b):
    return (y - b) / m


def fit_linear(xdata, ydata):
    from scipy.optimize import curve_fit
    return curve_fit(linear, xdata, ydata, [-1.0, -1.0])


def calc_linear_t_width(popt, low=0.25, high=0.75):
    right_time = inv_linear(low, *popt)
    left_time = inv_linear(high, *popt)
    return right_time - left_time, left_time, right_time


def twidth_from_points(time_bins, pct_reps, curve='sigmoid'):
    """The fit and T-width of calculate_twidth on points already computed (by either layer).
    The second and third values are named as the reference's caller receives them: it unpacks
    (t_width, left_time, right_time) as t_width, right_time, left_time."""
    if curve == 'sigmoid':
        popt, _ = fit_sigmoid(time_bins, pct_reps)
        t_width, right_time, left_time = calc_t_width(popt)
    elif curve == 'linear':
        popt, _ = fit_linear(time_bins, pct_reps)
        t_width, right_time, left_time = calc_linear_t_width(popt)
    else:
        raise ValueError("curve must be 'sigmoid' or 'linear'")
    return t_width, right_time, left_time, popt, time_bins, pct_reps


def calculate_twidth(cn, tfs_col='time_from_scheduled_rt', rs_col='rt_state', per_cell=False, query2=None,
                     curve='sigmoid', cell_col='cell_id'):
    """T-width of a set of S-phase cells (calculate_twidth.py:142-170):
    (t_width, right_time, left_time, popt, time_bins, pct_reps)."""
    time_bins, pct_reps = calc_pct_replicated_per_time_bin(cn, tfs_col=tfs_col, rs_col=rs_col, per_cell=per_cell,
                                                           query2=query2, cell_col=cell_col)
    return twidth_from_points(time_bins, pct_reps, curve=curve)


def plot_cell_variability(xdata, ydata, popt=None, left_time=None, right_time=None, t_width=None, alpha=1,
                          title='Cell-to-cell variabilty', curve='sigmoid', ax=None):
    """Scatter of the histogram points with the fitted curve and the T-width guides."""
    import matplotlib.pyplot as plt
    if ax is None:
        _, ax = plt.subplots(1, 1, figsize=(6, 6))
    ax.scatter(xdata, ydata, label='data', alpha=alpha)
    if popt is not None:
        grid = np.linspace(-10, 10, 1000)
        fitted = sigmoid(grid, *popt) if curve == 'sigmoid' else linear(grid, *popt)
        ax.plot(grid, fitted, color='r', label='fit')
        for level in (0.75, 0.25):
            ax.axhline(y=level, color='k', linestyle='--')
        ax.axvline(x=left_time, color='k', linestyle='--')
        ax.axvline(x=right_time, color='k', linestyle='--', label='T_width={}'.format(round(t_width, 3)))
    ax.set_xlabel('time from scheduled replication (h)')
    ax.set_ylabel('% replicated')
    ax.set_title(title)
    ax.legend(loc='best')
    return ax


def compute_and_plot_twidth(cn, tfs_col='time_from_scheduled_rt', rs_col='rt_state', per_cell=False, query2=None,
                            cell_col='cell_id', alpha=1, title='Cell-to-cell variabilty', curve='sigmoid', ax=None):
    """calculate_twidth, then plot_cell_variability of its result: (ax, t_width)."""
    t_width, right_time, left_time, popt, time_bins, pct_reps = calculate_twidth(
        cn, tfs_col=tfs_col, rs_col=rs_col, per_cell=per_cell, query2=query2, curve=curve, cell_col=cell_col)
    ax = plot_cell_variability(time_bins, pct_reps, popt, left_time, right_time, t_width, alpha=alpha, title=title,
                               curve=curve, ax=ax)
    return ax, t_width


# ----------------------------------------------------------------------------------------------
# matrix layer
# ----------------------------------------------------------------------------------------------

class RTMatrix:
    """The bins x cells replication-state matrix with its row and column labels.

    ``rep``: a ``(L, N)`` numpy array of 0 / 1, or a CUDA ``uint8`` tensor of shape ``(L, N)``
    whose rows are ``ldn`` apart (a ``PertShard.decode()`` result: used in place, no host copy).
    ``cell_ids [N]``, ``chr [L]``, ``start [L]``, ``clone_ids [N]`` (optional) label it; rows may
    be in any order, results list the loci sorted by (chr, start) as the reference does.
    ``device=None`` runs the two O(L N) passes on the GPU when there is one (always, for a CUDA
    tensor), else in chunked numpy; the counts, and so every result, are the same."""

    def __init__(self, rep, cell_ids, chr, start, clone_ids=None, device: Optional[str] = None):
        import torch
        self.cell_ids = np.asarray(cell_ids)
        self.chr, self.start = np.asarray(chr), np.asarray(start)
        self.clone_ids = None if clone_ids is None else np.asarray(clone_ids)
        if torch.is_tensor(rep):
            if rep.dtype != torch.uint8 or rep.dim() != 2:
                raise ValueError("a tensor rep must be uint8 [L][N]")
            self.device = rep.device if device is None else torch.device(device)
            if rep.device != self.device:
                rep = rep.to(self.device)
            if self.device.type == "cpu":
                rep = rep.numpy()
        if not torch.is_tensor(rep):
            rep = np.asarray(rep)
            if rep.ndim != 2:
                raise ValueError("rep must be a (bins, cells) matrix")
            if rep.dtype != np.uint8:
                if rep.size and not np.all((rep == 0) | (rep == 1)):
                    raise ValueError("rep holds values other than 0 and 1")
                rep = rep.astype(np.uint8)
            self.device = (torch.device(device) if device is not None
                           else torch.device("cuda" if torch.cuda.is_available() else "cpu"))
        self.L, self.N = int(rep.shape[0]), int(rep.shape[1])
        if self.L < 1 or self.N < 1:
            raise ValueError("rep must hold at least one bin and one cell")
        if len(self.cell_ids) != self.N or len(self.chr) != self.L or len(self.start) != self.L or (
                self.clone_ids is not None and len(self.clone_ids) != self.N):
            raise ValueError("labels do not match rep's shape {}".format((self.L, self.N)))
        if self.device.type == "cuda":
            self._rep_dev, self.ldn = self._device_matrix(rep)
            self._rep_host = None
        else:
            self._rep_dev, self.ldn, self._rep_host = None, self.N, np.ascontiguousarray(rep)
        # loci in the reference's order: sorted by chr (as stored: strings sort as strings), then start
        self.locus_order = np.lexsort((self.start, self.chr))
        if self.clone_ids is None:
            self.clones, self._clone_of = np.asarray([]), np.full(self.N, -1, np.int64)
        else:
            codes, uni = pd.factorize(self.clone_ids, sort=True)
            self.clones, self._clone_of = np.asarray(uni), codes.astype(np.int64)
        self._counts = None

    # ---- construction from a long table -------------------------------------------------------

    @classmethod
    def from_frame(cls, cn, rs_col='model_rep_state', cell_col='cell_id', chr_col='chr', start_col='start',
                   clone_col='clone_id', device: Optional[str] = None):
        """From a complete bins x cells long table (every cell has every locus exactly once).
        ValueError if the table is not a full grid or ``rs_col`` holds values other than 0 / 1."""
        codes, chrom, start = _locus_codes(cn, chr_col, start_col)
        cells, cell_uni = pd.factorize(cn[cell_col], sort=True)
        L, N = len(chrom), len(cell_uni)
        if L == 0 or N == 0 or len(cn) != L * N or (codes < 0).any() or (cells < 0).any():
            raise ValueError("the table is not a full bins x cells grid ({} rows, {} loci x {} cells)".format(
                len(cn), L, N))
        flat = codes * N + cells
        if len(np.unique(flat)) != L * N:
            raise ValueError("the table is not a full bins x cells grid (repeated (locus, cell) rows)")
        state = cn[rs_col].to_numpy()
        if not np.all((state == 0) | (state == 1)):
            raise ValueError("{} holds values other than 0 and 1".format(rs_col))
        rep = np.empty(L * N, np.uint8)
        rep[flat] = state.astype(np.uint8)
        clone_ids = None
        if clone_col is not None:
            k_codes, k_uni = pd.factorize(cn[clone_col], sort=True)      # -1: no clone
            of_cell = np.empty(N, np.int64)
            of_cell[cells] = k_codes
            if (of_cell[cells] != k_codes).any():
                raise ValueError("{} varies within a cell".format(clone_col))
            clone_ids = np.asarray(k_uni, dtype=object)[of_cell] if len(k_uni) else np.full(N, None, object)
            clone_ids[of_cell < 0] = None
        return cls(rep.reshape(L, N), np.asarray(cell_uni), chrom, start, clone_ids=clone_ids, device=device)

    # ---- device plumbing -----------------------------------------------------------------------

    def _device_matrix(self, rep):
        import torch
        if torch.is_tensor(rep):
            ldn = int(rep.stride(0)) if rep.shape[0] > 1 else int(rep.shape[1])
            if rep.stride(1) == 1 and ldn >= rep.shape[1] and ldn % 16 == 0 and rep.data_ptr() % 16 == 0:
                return rep, ldn
        L, N = int(rep.shape[0]), int(rep.shape[1])
        ldn = -(-N // 256) * 256
        buf = torch.zeros((L, ldn), dtype=torch.uint8, device=self.device)
        buf[:, :N] = rep if torch.is_tensor(rep) else torch.from_numpy(np.ascontiguousarray(rep))
        return buf[:, :N], ldn

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _device_counts(self, group, G):
        import torch
        from . import _native as nat
        with torch.cuda.device(self.device):
            grp = torch.as_tensor(group.astype(np.int32), device=self.device)
            bins = torch.zeros((G, self.L), dtype=torch.int32, device=self.device)
            cells = torch.zeros(self.N, dtype=torch.int32, device=self.device)
            nat.check(nat.lib().pert_rt_counts(self.L, self.N, self.ldn, G, self._rep_dev.data_ptr(), grp.data_ptr(),
                                               bins.data_ptr(), cells.data_ptr(), self._stream()), "pert_rt_counts")
            return (bins.cpu().numpy().view(np.uint32).astype(np.int64),
                    cells.cpu().numpy().view(np.uint32).astype(np.int64))

    def _device_hist(self, group, hours, f10, edges, per_cell, strategy=1):
        import torch
        from . import _native as nat
        T = hours.dtype
        nb = len(edges) - 1
        shape = (self.N, nb) if per_cell else (nb,)
        with torch.cuda.device(self.device):
            hist_n = torch.zeros(shape, dtype=torch.int32, device=self.device)
            hist_rep = torch.zeros(shape, dtype=torch.int32, device=self.device)
            f10_d = torch.as_tensor(f10, device=self.device)
            edges_d = torch.as_tensor(edges, device=self.device)
            # the kernel keeps a tile's hours rows of every group in LDS: launches of at most
            # RT_MAX_GROUPS groups each, whose counts add up in the same outputs
            for g0 in range(0, hours.shape[0], nat.RT_MAX_GROUPS):
                part = np.ascontiguousarray(hours[g0:g0 + nat.RT_MAX_GROUPS])
                sub = np.where((group >= g0) & (group < g0 + len(part)), group - g0, -1).astype(np.int32)
                grp = torch.as_tensor(sub, device=self.device)
                hours_d = torch.as_tensor(part, device=self.device)
                nat.check(nat.lib().pert_rt_tfs_hist(
                    self.L, self.N, self.ldn, len(part), self._rep_dev.data_ptr(), grp.data_ptr(), hours_d.data_ptr(),
                    f10_d.data_ptr(), edges_d.data_ptr(), len(edges), int(T == np.float64),
                    int(strategy) if per_cell else 0, hist_n.data_ptr(), hist_rep.data_ptr(), self._stream()),
                    "pert_rt_tfs_hist")
            return (hist_n.cpu().numpy().view(np.uint32).astype(np.int64),
                    hist_rep.cpu().numpy().view(np.uint32).astype(np.int64))

    # ---- the chunked numpy passes (same counts as the kernels) -----------------------------------

    def _host_counts(self, group, G):
        rep = self._rep_host
        onehot = np.zeros((self.N, G), np.float32)
        sel = np.flatnonzero((group >= 0) & (group < G))
        onehot[sel, group[sel]] = 1.0
        bins = np.zeros((G, self.L), np.int64)
        cells = np.zeros(self.N, np.int64)
        step = max(1, _CHUNK_ELEMS // self.N)
        for l0 in range(0, self.L, step):
            blk = rep[l0:l0 + step]
            cells += blk.sum(axis=0, dtype=np.int64)
            bins[:, l0:l0 + step] = np.rint(blk.astype(np.float32) @ onehot).astype(np.int64).T   # exact: < 2^24
        return bins, cells

    def _host_hist(self, group, hours, f10, edges, per_cell):
        rep, nb = self._rep_host, len(edges) - 1
        sel = np.flatnonzero((group >= 0) & (group < hours.shape[0]))
        n_out = self.N if per_cell else 1
        hist_n = np.zeros(n_out * nb, np.int64)
        hist_rep = np.zeros(n_out * nb, np.int64)
        if len(sel):
            step = max(1, _CHUNK_ELEMS // len(sel))
            rows_of = hours[group[sel]]                                     # [cells][L]
            for l0 in range(0, self.L, step):
                t = rows_of[:, l0:l0 + step].T - f10[sel][None, :]          # one subtraction in T
                idx = np.searchsorted(edges, t.ravel(), side="right") - 1
                ok = (idx >= 0) & (idx < nb) & ~np.isnan(t.ravel())
                key = idx[ok]
                if per_cell:
                    key = key + np.broadcast_to(sel[None, :] * nb, t.shape).ravel()[ok]
                hist_n += np.bincount(key, minlength=n_out * nb)
                hist_rep += np.bincount(key, weights=rep[l0:l0 + step][:, sel].ravel()[ok].astype(np.float64),
                                        minlength=n_out * nb).astype(np.int64)
        shape = (self.N, nb) if per_cell else (nb,)
        return hist_n.reshape(shape), hist_rep.reshape(shape)

    # ---- results --------------------------------------------------------------------------------

    def counts(self):
        """(clone_count int64 [n_clones + 1][L], cell_count int64 [N]): replicated cells per bin
        for each clone (sorted clone ids; the last row collects the cells without a clone) and
        replicated bins per cell.  One pass, cached."""
        if self._counts is None:
            G = len(self.clones) + 1
            group = np.where(self._clone_of >= 0, self._clone_of, G - 1)
            self._counts = (self._device_counts if self.device.type == "cuda" else self._host_counts)(group, G)
        return self._counts

    def cell_fractions(self, dtype=np.float32, state_dtype=np.float32) -> np.ndarray:
        """Replicated fraction of each cell: the quotient count / L formed in ``state_dtype`` (the
        state column's; the reference's compute_cell_frac divides float32 values) and stored as ``dtype``."""
        st = np.dtype(state_dtype).type
        return (self.counts()[1].astype(st) / st(self.L)).astype(dtype)

    def pseudobulk(self, dtype=np.float32) -> dict:
        """The pseudobulk profiles of a state column of ``dtype``: a dict with ``chr`` / ``start``
        (the loci sorted by (chr, start)), ``population`` = (values, hours) and ``clones`` =
        {clone id: (values, hours)}, values being the mean state and hours its 0-10 h scale."""
        clone_count, _ = self.counts()
        order = self.locus_order
        sizes = np.bincount(np.where(self._clone_of >= 0, self._clone_of, len(self.clones)),
                            minlength=len(self.clones) + 1)

        def profile(count, size):
            values = _mean_from_sums(count[order], np.full(self.L, size), dtype)
            return values, _hours_from_profile(values)

        return dict(chr=self.chr[order], start=self.start[order],
                    population=profile(clone_count.sum(axis=0), self.N),
                    clones={c: profile(clone_count[k], sizes[k]) for k, c in enumerate(self.clones)})

    def pseudobulk_frame(self, input_col='model_rep_state', output_col='pseudobulk', time_col='hours',
                         dtype=np.float32) -> pd.DataFrame:
        """``pseudobulk`` laid out as compute_pseudobulk_rt_profiles returns it."""
        pb = self.pseudobulk(dtype)
        chrom = pb["chr"].astype(object) if pb["chr"].dtype.kind in "US" else pb["chr"]
        out = pd.DataFrame({'chr': chrom, 'start': pb["start"],
                            '{}_{}'.format(output_col, input_col): pb["population"][0],
                            '{}_{}'.format(output_col, time_col): pb["population"][1]})
        for clone_id, (values, hours) in pb["clones"].items():
            out['{}_clone{}_{}'.format(output_col, clone_id, input_col)] = values
            out['{}_clone{}_{}'.format(output_col, clone_id, time_col)] = hours
        return out

    def tfs_counts(self, by='population', per_cell=False, cells=None, loci=None, dtype=np.float32, frac_dtype=None,
                   strategy=1):
        """The integer histogram behind ``tfs_histogram``: (hist_n, hist_rep), int64 [200] or
        [N][200] with ``per_cell`` (rows in ``cell_ids`` order)."""
        frac_dtype = dtype if frac_dtype is None else frac_dtype
        T = np.dtype(_tfs_dtype(dtype, frac_dtype))
        pb = self.pseudobulk(dtype)
        inv = np.empty(self.L, np.int64)
        inv[self.locus_order] = np.arange(self.L)                          # sorted loci -> matrix rows
        if by == 'population':
            hours = pb["population"][1][inv][None, :]
            group = np.zeros(self.N, np.int64)
        elif by == 'clone':
            if not len(self.clones):
                raise ValueError("by='clone' needs clone_ids")
            hours = np.stack([pb["clones"][c][1][inv] for c in self.clones])
            group = self._clone_of.copy()
        else:
            raise ValueError("by must be 'population' or 'clone'")
        hours = hours.astype(T)
        if loci is not None:                                               # bins left out count nowhere
            keep = np.zeros(self.L, bool)
            keep[np.asarray(loci)] = True
            hours[:, ~keep] = np.nan
        if cells is not None:
            group = np.where(np.isin(self.cell_ids, np.asarray(cells)), group, -1)
        # cn[frac] * 10.0 in the fraction column's dtype, then one subtraction in the common dtype
        f10 = (self.cell_fractions(frac_dtype, state_dtype=dtype) * 10.0).astype(T)
        edges = interval_edges().astype(T)
        if self.device.type == "cuda":
            return self._device_hist(group, hours, f10, edges, per_cell, strategy)
        return self._host_hist(group, hours, f10, edges, per_cell)

    def tfs_histogram(self, by='population', per_cell=False, cells=None, loci=None, dtype=np.float32, frac_dtype=None):
        """calc_pct_replicated_per_time_bin of the long table this matrix stands for, with
        time from scheduled replication = hours of the bin (the population's profile, or with
        ``by='clone'`` the cell's clone's) - 10 x the cell's replicated fraction.  ``dtype`` is the
        state (and so hours) column's, ``frac_dtype`` the fraction column's (default ``dtype``;
        float64 reproduces a float64 column of widened float32 quotients).  ``cells`` (ids) and
        ``loci`` (row indices or a mask) restrict the rows, as ``query2`` does.
        Returns (time_bins, pct_reps)."""
        hist_n, hist_rep = self.tfs_counts(by, per_cell, cells, loci, dtype, frac_dtype)
        order = np.argsort(self.cell_ids, kind="stable") if per_cell else None
        return _lists_from_hist(hist_n, hist_rep, interval_edges()[:-1], cell_order=order)

    def twidth(self, curve='sigmoid', **kw):
        """calculate_twidth on ``tfs_histogram(**kw)``."""
        return twidth_from_points(*self.tfs_histogram(**kw), curve=curve)

    def bootstrap(self, n_boot=200, seed=0, **kw):
        """A ``CellBootstrap`` of this matrix (cell_bootstrap.py): the sampling spread over cells of
        the pseudobulk profiles and of T-width."""
        from .cell_bootstrap import CellBootstrap
        return CellBootstrap(self, n_boot=n_boot, seed=seed, **kw)
