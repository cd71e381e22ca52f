"""The deterministic cell level's normalisation (reference scdna_replication_tools/normalize_by_cell.py):
every S-phase cell divided by its best-correlated G1/2 cell of the same clone, then cell-specific
copy-number changes removed by a change-point search, then scaled.

The reference finds its change points with ``ruptures.KernelCPD(kernel='linear', min_size=2)``.  For
the linear kernel a segment's cost is sum y^2 - (sum y)^2 / len, so ``predict(n_bkps)`` returns the
breakpoints that maximise a sum of (segment sum)^2 / len terms: a closed form, defined in DESIGN.md
section 6o and built here twice.  ``cpd_search`` is that on a GPU (csrc/cpd_kernels.hip,
``pert_cpd_search``: all cells of a round in one call, fp64, bit-identical from run to run);
``cpd_search_host`` is the same definition in numpy, the CPU path and the kernel's check: the two
agree bit for bit on the breakpoints and on the gain.  The definition, for a profile Y[0..n):

    S[0] = 0, S[i] = S[i-1] + Y[i-1] (in bin order);  rinv[k] = 1.0 / k
    two breakpoints, 2 <= a, a + 2 <= b <= n - 2:
        G(a, b) = (S[a] S[a]) rinv[a] + ((S[b] - S[a]) (S[b] - S[a])) rinv[b - a]
                  + ((S[n] - S[b]) (S[n] - S[b])) rinv[n - b]
    one breakpoint, 2 <= a <= n - 2:
        G(a) = (S[a] S[a]) rinv[a] + ((S[n] - S[a]) (S[n] - S[a])) rinv[n - a]

every operation one fp64 operation, the terms added left to right; the largest G wins and a tie goes
to the smallest a, then the smallest b.  A search without a candidate (n < 6, n < 4) reports
a = b = -1 and ends that cell's loop.

The reference's loop runs one cell at a time; here it runs in rounds over all cells at once: one
search call per round for the cells still looping, then the reference's per-cell decisions (a median
ratio, a t-test, the chromosome test) on the host.  Its ``while`` loops have no bound; a cell's loop is
ended after ``MAX_ROUNDS`` searches with a warning.
"""
from __future__ import annotations

import ctypes
import warnings

import numpy as np
import pandas as pd
import torch

from . import prep

MAX_ROUNDS = 64                  # searches per cell before its loop is ended with a warning
_BLOCK = 1 << 21                 # candidates per block of the host search
EPS = float(np.finfo(float).eps)


# ----------------------------------------------------------------------------------------------
# the search
# ----------------------------------------------------------------------------------------------

def _feasible(n: int, mode: int) -> bool:
    return n >= 6 if mode == 2 else n >= 4


def _search_one(y: np.ndarray, mode: int):
    """(a, b, gain) of one profile by the definition, rows of a against a vector of b."""
    n = len(y)
    if not _feasible(n, mode):
        return -1, -1, 0.0
    S = np.concatenate([[0.0], np.cumsum(y, dtype=np.float64)])          # cumsum adds in order
    rinv = np.zeros(n + 1)
    rinv[1:] = 1.0 / np.arange(1, n + 1, dtype=np.float64)
    Sn = S[n]
    if mode == 1:
        a = np.arange(2, n - 1)
        g = (S[a] * S[a]) * rinv[a] + ((Sn - S[a]) * (Sn - S[a])) * rinv[n - a]
        i = int(np.argmax(g))                                            # the first maximum
        return int(a[i]), n, float(g[i])
    b = np.arange(n + 1)
    t3 = ((Sn - S) * (Sn - S)) * rinv[n - b]                             # the third term, per b
    best = (-1.0, -1, -1)
    rows = max(1, _BLOCK // (n + 1))
    for a0 in range(2, n - 3, rows):
        a = np.arange(a0, min(a0 + rows, n - 3))[:, None]
        ok = (b[None, :] >= a + 2) & (b[None, :] <= n - 2)
        d = S[None, :] - S[a]
        t1 = (S[a] * S[a]) * rinv[a]
        g = (t1 + (d * d) * rinv[np.where(ok, b[None, :] - a, 0)]) + t3[None, :]
        g = np.where(ok, g, -1.0)
        i = int(np.argmax(g))                                            # row-major: smallest a, then b
        ia, ib = divmod(i, n + 1)
        if g[ia, ib] > best[0]:                                          # a later block wins only if larger
            best = (float(g[ia, ib]), int(a[ia, 0]), ib)
    if best[1] < 0:
        return -1, -1, 0.0
    return best[1], best[2], best[0]


def _search_args(Y, lens, mode, active):
    Y = np.asarray(Y, dtype=np.float64) if not isinstance(Y, torch.Tensor) else Y
    if Y.ndim == 1:
        Y = Y[None, :]
    N, ld = Y.shape
    lens = np.full(N, ld, np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    mode = np.full(N, mode, np.int32) if np.ndim(mode) == 0 else np.ascontiguousarray(mode, dtype=np.int32)
    active = np.ones(N, np.int32) if active is None else np.ascontiguousarray(np.asarray(active) != 0, dtype=np.int32)
    if lens.shape != (N,) or mode.shape != (N,) or active.shape != (N,):
        raise ValueError("one length, one mode and one active flag per profile")
    if ((lens < 0) | (lens > ld)).any() or not np.isin(mode, (1, 2)).all():
        raise ValueError("lengths must lie in [0, {}] and modes be 1 or 2".format(ld))
    return Y, lens, mode, active


def cpd_search_host(Y, lens=None, mode=2, active=None):
    """The change-point search of every active row of ``Y`` (N, ld) float64 (row c's first
    ``lens[c]`` entries are its profile) in numpy: ``mode`` 2 or 1 breakpoints (a scalar or one per
    row).  Returns (a, b, gain): int32, int32, float64 arrays; b = the length in mode 1; a = b = -1
    and gain 0 where the search is infeasible; an inactive row holds -1, -1, NaN."""
    Y, lens, mode, active = _search_args(Y, lens, mode, active)
    N = Y.shape[0]
    a, b, g = np.full(N, -1, np.int32), np.full(N, -1, np.int32), np.full(N, np.nan)
    for c in np.flatnonzero(active):
        y = np.asarray(Y[c, :lens[c]], dtype=np.float64)
        if not np.isfinite(y).all():
            raise ValueError("the change-point search needs finite profiles (row {})".format(c))
        a[c], b[c], g[c] = _search_one(y, int(mode[c]))
    return a, b, g


class _DeviceSearch:
    """``pert_cpd_search`` on the rows of one device matrix, its workspace and outputs allocated once
    for all rounds."""

    def __init__(self, Y, device):
        from . import _native
        self.native = _native
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise ValueError("cpd_search is the kernel path and runs on a GPU; cpd_search_host is the CPU path")
        Yt = Y if isinstance(Y, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(Y, dtype=np.float64))
        if Yt.dtype != torch.float64 or Yt.dim() != 2 or Yt.shape[0] < 1 or Yt.shape[1] < 1:
            raise ValueError("Y must be (N, ld) float64 with at least one row and one column")
        if Yt.shape[1] > _native.CPD_MAX_N:
            raise ValueError("a profile of {} bins exceeds the search's {} (its tables live in LDS)".format(
                Yt.shape[1], _native.CPD_MAX_N))
        self.Y = Yt.to(self.dev).contiguous()
        self.N, self.ld = self.Y.shape
        self.lib = _native.lib()
        nbytes = ctypes.c_int64()
        _native.check(self.lib.pert_cpd_workspace(self.N, self.ld, ctypes.byref(nbytes)), "pert_cpd_workspace")
        self.nbytes = int(nbytes.value)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=self.dev)
        self.a = torch.full((self.N,), -1, dtype=torch.int32, device=self.dev)
        self.b = torch.full((self.N,), -1, dtype=torch.int32, device=self.dev)
        self.g = torch.full((self.N,), float("nan"), dtype=torch.float64, device=self.dev)

    def update_rows(self, rows, values):
        self.Y[torch.as_tensor(rows, device=self.dev)] = torch.from_numpy(np.ascontiguousarray(values)).to(self.dev)

    def __call__(self, lens, mode, active):
        ip = ctypes.POINTER(ctypes.c_int32)
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            self.native.check(self.lib.pert_cpd_search(
                self.N, self.ld, self.Y.data_ptr(), lens.ctypes.data_as(ip), mode.ctypes.data_as(ip),
                active.ctypes.data_as(ip), self.a.data_ptr(), self.b.data_ptr(), self.g.data_ptr(), self.ws.data_ptr(),
                self.nbytes, ctypes.c_void_p(stream)), "pert_cpd_search")
            out = self.a.cpu().numpy(), self.b.cpu().numpy(), self.g.cpu().numpy()   # the host arrays outlive the call
        return out


def cpd_search(Y, lens=None, mode=2, active=None, device="cuda"):
    """``cpd_search_host`` on a GPU: one ``pert_cpd_search`` call on ``device`` and its current stream.
    ``Y``: array or tensor (N, ld) float64, ld <= 10,000.  An inactive row holds -1, -1, NaN.  There is
    no fallback: without the kernel this raises."""
    Y, lens, mode, active = _search_args(Y, lens, mode, active)
    return _DeviceSearch(Y, device)(lens, mode, active)


# ----------------------------------------------------------------------------------------------
# the reference's per-cell decisions
# ----------------------------------------------------------------------------------------------

def _scale(v: np.ndarray) -> np.ndarray:
    """sklearn.preprocessing.scale of one column (a copy): its two-step centring included."""
    from sklearn import preprocessing
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # "numerical issues were encountered when centering"
        return preprocessing.scale(np.asarray(v, dtype=np.float64))


def _ratio_and_pval(Y: np.ndarray, idx: np.ndarray):
    """normalize_by_cell.py:48-55: the region's median over the 'background's, and the two-sided
    t-test of the two.  The reference's background is ``Y[~temp_indices]`` on INTEGER indices: not the
    complement but the mirror image Y[-1 - i], as many values as the region holds."""
    from scipy.stats import ttest_ind
    region = Y[idx]
    background = Y[~idx]
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ratio = np.median(region) / np.median(background)
        pval = ttest_ind(region, background)[1]
    return ratio, pval


class _CellLoop:
    """One cell's state in identify_changepoint_segs (normalize_by_cell.py:35-113)."""

    def __init__(self, y, chrom):
        self.Y = np.array(y, dtype=np.float64)
        self.chrom = chrom                               # the sorted table's labels: str, or None (NaN)
        self.chng = np.zeros(len(self.Y))
        self.j = 1
        self.mode = 2
        self.done = False
        self.rounds = 0

    def _same(self, l, r):
        return l is not None and r is not None and l == r

    def step(self, a, b):
        """The decision after a search returned (a, b); True when Y changed."""
        self.rounds += 1
        if a < 0:                                        # no candidate: the loop ends (section 6o)
            self.done = True
            return False
        Y, n = self.Y, len(self.Y)
        if self.mode == 2:
            idx = np.arange(a, b)
            ratio, pval = _ratio_and_pval(Y, idx)
            left, right = self.chrom[a], self.chrom[b - 1]
            if (ratio > 1.1 or ratio < 0.9) and pval < 0.05 and self._same(left, right):
                self.chng[idx] = self.j
                self.j += 1
                Y[idx] /= ratio
                return True
            self.mode = 1
            return False
        # one breakpoint: the label AT the breakpoint is the reference's left_chr, the one before it
        # its right_chr (:78-79)
        left, right = self.chrom[a], self.chrom[a - 1]
        if right == '1':
            idx = np.arange(0, a)
        elif left == 'X':
            idx = np.arange(a, n)
        else:
            self.done = True
            return False
        ratio, pval = _ratio_and_pval(Y, idx)
        if ((ratio > 1.1 and left == 'X') or (ratio < 0.9 and right == '1')) and pval < 0.05:
            self.chng[idx] = self.j
            self.j += 1
            Y[idx] /= ratio
            return True
        self.done = True
        return False


def changepoint_rounds(profiles, chroms, device=None):
    """identify_changepoint_segs for many cells at once: ``profiles`` a list of 1-D float64 arrays,
    ``chroms`` their per-bin chromosome labels (str, or None for a label outside 1..22, X, Y).
    Every round is one search over the cells still looping (``pert_cpd_search`` on a GPU ``device``,
    ``cpd_search_host`` on the CPU), then each cell's decision.  Returns (Y list, chng list, rounds
    array); a cell that reaches MAX_ROUNDS searches is ended with a warning."""
    N = len(profiles)
    if N == 0:
        return [], [], np.zeros(0, np.int64)
    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    cells = [_CellLoop(y, c) for y, c in zip(profiles, chroms)]
    lens = np.array([len(c.Y) for c in cells], dtype=np.int32)
    ld = max(int(lens.max()), 1)
    Y = np.zeros((N, ld))
    for i, c in enumerate(cells):
        if not np.isfinite(c.Y).all():
            raise ValueError("the change-point search needs finite profiles")
        Y[i, :lens[i]] = c.Y
    search = _DeviceSearch(Y, dev) if dev.type == "cuda" else None
    capped = 0
    while True:
        active = np.array([not c.done for c in cells], dtype=np.int32)
        if not active.any():
            break
        mode = np.array([c.mode for c in cells], dtype=np.int32)
        a, b, _ = search(lens, mode, active) if search is not None else cpd_search_host(Y, lens, mode, active)
        changed = []
        for i in np.flatnonzero(active):
            c = cells[i]
            if c.step(int(a[i]), int(b[i])):
                if not np.isfinite(c.Y).all():           # a zero or non-finite ratio: nothing left to search
                    c.done = True
                    continue
                Y[i, :lens[i]] = c.Y
                changed.append(i)
            if not c.done and c.rounds >= MAX_ROUNDS:
                c.done = True
                capped += 1
        if search is not None and changed:
            search.update_rows(changed, Y[changed])
    if capped:
        warnings.warn("{} cell(s) reached {} change-point searches; their loops were ended there (the "
                      "reference's have no bound)".format(capped, MAX_ROUNDS), RuntimeWarning)
    return [c.Y for c in cells], [c.chng for c in cells], np.array([c.rounds for c in cells], dtype=np.int64)


def _chr_labels(cn, chr_col):
    """The labels of a table sorted by ``sort_by_cell_and_loci``: str of 1..22, X, Y, None otherwise."""
    col = cn[chr_col]
    codes = col.cat.codes.to_numpy() if isinstance(col.dtype, pd.CategoricalDtype) else prep._chr_codes(col)
    cats = np.asarray(col.cat.categories, dtype=object) if isinstance(col.dtype, pd.CategoricalDtype) \
        else np.asarray(prep.CHR_ORDER, dtype=object)
    lab = np.empty(len(codes), dtype=object)
    ok = codes >= 0
    lab[ok] = cats[codes[ok]]
    return lab


def sort_by_cell_and_loci(cn, cell_col='cell_id', chr_col='chr', start_col='start'):
    """normalize_by_cell.py:24-32: ``chr_col`` as a category in the order 1..22, X, Y (any other label
    becomes NaN and sorts last), rows sorted by (cell, chr, start).  A new frame is returned."""
    return prep.sort_by_cell_and_loci(cn, cell_col=cell_col, chr_col=chr_col, start_col=start_col)


def identify_changepoint_segs(cell_cn, col, chr_col='chr', *, device=None):
    """normalize_by_cell.py:35-113 for one cell's sorted table: (Y, chng), the profile with every
    nominated region divided by its median ratio, and the regions numbered from 1 (0: none)."""
    Y, chng, _ = changepoint_rounds([cell_cn[col].to_numpy(dtype=np.float64)], [_chr_labels(cell_cn, chr_col)],
                                    device=device)
    return Y[0], chng[0]


def _trim_tails(v: np.ndarray) -> np.ndarray:
    """normalize_by_cell.py:121-128: values 4 sigma above the mean become the 95th percentile, then
    values 4 sigma below the 5th."""
    v2 = np.where(_scale(v) < 4, v, np.percentile(v, 95))
    return np.where(_scale(v2) > -4, v2, np.percentile(v2, 5))


def _scale_segments(Y3: np.ndarray, chng: np.ndarray) -> tuple:
    """normalize_by_cell.py:137-143: scaled within every nominated segment, then overall."""
    v4 = np.empty(len(Y3))
    for seg in np.unique(chng):
        at = chng == seg
        v4[at] = _scale(Y3[at])
    return v4, _scale(v4)


def _finish_cells(frames, input_col, output_col, seg_col, chr_col, device):
    """remove_cell_specific_CNAs on sorted per-cell frames, the change-point loop batched over them."""
    trimmed = [_trim_tails(f[input_col].to_numpy(dtype=np.float64)) if len(f) else np.zeros(0) for f in frames]
    Ys, chngs, rounds = changepoint_rounds(trimmed, [_chr_labels(f, chr_col) for f in frames], device=device)
    for f, v2, Y3, chng in zip(frames, trimmed, Ys, chngs):
        f[input_col + '_2'] = v2
        f[seg_col] = chng
        f[input_col + '_3'] = Y3
        v4, v5 = _scale_segments(Y3, chng) if len(f) else (np.zeros(0), np.zeros(0))
        f[input_col + '_4'] = v4
        f[output_col] = v5
    return frames, rounds


def remove_cell_specific_CNAs(cell_cn, input_col='copy_norm', output_col='rt_value', seg_col='changepoint_segments',
                              cell_col='cell_id', chr_col='chr', start_col='start', *, device=None):
    """normalize_by_cell.py:116-145 for one cell's table: sorted by (cell, chr, start); the tails
    trimmed into ``input_col + '_2'``; the change-point loop's regions in ``seg_col`` and its profile
    in ``input_col + '_3'``; scaled within every region (``input_col + '_4'``) and overall
    (``output_col``).  A new frame is returned."""
    out = sort_by_cell_and_loci(cell_cn, cell_col=cell_col, chr_col=chr_col, start_col=start_col)
    out = out.copy()
    return _finish_cells([out], input_col, output_col, seg_col, chr_col, device)[0][0]


def _g1_quotient(s_val, ploidy_g1, state_g1, ploidy_s):
    return (s_val * ploidy_g1) / ((state_g1 * ploidy_s) + EPS)


def g1_cell_norm(s_cell_cn, g1_cell_cn, input_col='rpm_gc_norm', output_col='state_norm',
                 cell_col='cell_id', chr_col='chr', start_col='start', cn_state_col='state', ploidy_col='ploidy'):
    """normalize_by_cell.py:183-213: the S-phase cell's ``input_col`` times the G1 cell's ploidy over
    (the G1 cell's state times the S cell's ploidy, + eps), at the loci both cells have, in the S
    cell's row order, then centred and scaled.  Returns [chr, start, cell, ``output_col``].  The S
    cell's values are read from ``input_col + '_s'`` when the table has it (the reference's
    compute_cell_corrs renames the column in place) and from ``input_col`` otherwise; neither frame is
    modified."""
    s_col = '{}_s'.format(input_col)
    s_val = s_cell_cn[s_col if s_col in s_cell_cn.columns else input_col].to_numpy(dtype=np.float64)
    g_key = pd.MultiIndex.from_arrays([g1_cell_cn[chr_col].to_numpy(), g1_cell_cn[start_col].to_numpy()])
    s_key = pd.MultiIndex.from_arrays([s_cell_cn[chr_col].to_numpy(), s_cell_cn[start_col].to_numpy()])
    if g_key.has_duplicates or s_key.has_duplicates:
        raise ValueError("a cell holds a locus twice")
    pos = g_key.get_indexer(s_key)
    hit = pos >= 0
    q = _g1_quotient(s_val[hit], g1_cell_cn[ploidy_col].to_numpy(dtype=np.float64)[pos[hit]],
                     g1_cell_cn[cn_state_col].to_numpy(dtype=np.float64)[pos[hit]],
                     s_cell_cn[ploidy_col].to_numpy(dtype=np.float64)[hit])
    out = s_cell_cn[[chr_col, start_col, cell_col]][hit].reset_index(drop=True)
    out[output_col] = _scale(q) if len(q) else q
    return out


# ----------------------------------------------------------------------------------------------
# normalize_by_cell on whole tables
# ----------------------------------------------------------------------------------------------

def _with_ploidy(cn, cell_col, cn_state_col, ploidy_col):
    """add_cell_ploidies as the reference leaves the table: rows with a NaN already dropped, the
    cell column first, ``ploidy_col`` (float64, the mode of the cell's states) last or in its place.
    Returns the frame, the sorted cells and every row's cell code."""
    codes, cells = pd.factorize(cn[cell_col].to_numpy(), sort=True)
    ploidy = prep._cell_mode(codes, len(cells), cn[cn_state_col].to_numpy())
    rest = [c for c in cn.columns if c != cell_col]
    out = cn[[cell_col] + rest].copy()
    out[ploidy_col] = ploidy[codes].astype(np.float64)
    return out, cells, codes


def _masked_pearson(Xs, Ms, Xg, Mg, dev):
    """Pearson r of every S column with every G1 column over the loci both have (mask 1), from sums
    of the columns shifted by their own means (r does not change; the raw moments then hold no large
    common offset)."""
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)
    Xs, Ms, Xg, Mg = t(Xs), t(Ms), t(Xg), t(Mg)
    Xs = (Xs - (Xs * Ms).sum(0) / Ms.sum(0).clamp(min=1)) * Ms
    Xg = (Xg - (Xg * Mg).sum(0) / Mg.sum(0).clamp(min=1)) * Mg
    n = Ms.T @ Mg
    sx, sy = Xs.T @ Mg, Ms.T @ Xg
    sxy, sxx, syy = Xs.T @ Xg, (Xs * Xs).T @ Mg, Ms.T @ (Xg * Xg)
    r = (n * sxy - sx * sy) / torch.sqrt((n * sxx - sx * sx) * (n * syy - sy * sy))
    return r.cpu().numpy()


def normalize_by_cell(cn_s, cn_g1, input_col='rpm_gc_norm', clone_col='clone_id', cell_col='cell_id',
                      temp_col='temp_rt', output_col='rt_value', seg_col='changepoint_segments',
                      chr_col='chr', start_col='start', cn_state_col='state', ploidy_col='ploidy', *, device=None):
    """normalize_by_cell.py:216-267 on whole tables.  Rows with a NaN are dropped from both; every
    cell gets ``ploidy_col``; every S-phase cell is matched with the G1/2 cell of its clone (its first
    row's ``clone_col``; all G1/2 cells when either table lacks the column) whose ``input_col`` has the
    highest Pearson r with its own over the loci both have (the reference's descending sort, ties
    included); ``temp_col`` is g1_cell_norm against that cell; remove_cell_specific_CNAs then runs
    with the reference's DEFAULT cell / chr / start column names, as the reference calls it, its
    change-point loop in rounds over all cells (``device``: a GPU runs ``pert_cpd_search``, the CPU
    ``cpd_search_host``; default: the GPU when there is one).  Returns the cells in sorted order, each
    sorted by (chr, start): chr, start, cell, ``temp_col``, G1_match_cell_id, G1_match_pearsonr,
    ``temp_col``_2, ``seg_col``, ``temp_col``_3, ``temp_col``_4, ``output_col``, then the S table's other
    columns and ``ploidy_col``.  A row whose chromosome is not one of 1..22, X, Y takes part in the
    cell's profile (sorted last) and is absent from the result, as the reference's final merge leaves
    it.  The caller's frames are not modified (the reference drops their NaN rows in place)."""
    from scipy.stats import pearsonr
    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    s, s_cells, s_code = _with_ploidy(cn_s.dropna(), cell_col, cn_state_col, ploidy_col)
    g, g_cells, g_code = _with_ploidy(cn_g1.dropna(), cell_col, cn_state_col, ploidy_col)
    if len(s_cells) == 0:
        raise ValueError("No objects to concatenate")
    # one integer key per (chr, start) over both tables
    ch_code, _ = pd.factorize(np.concatenate([s[chr_col].to_numpy(dtype=object), g[chr_col].to_numpy(dtype=object)]))
    st_code, st_u = pd.factorize(np.concatenate([s[start_col].to_numpy(), g[start_col].to_numpy()]))
    lkey, loci = pd.factorize(ch_code.astype(np.int64) * max(len(st_u), 1) + st_code)
    ks, kg = lkey[:len(s)], lkey[len(s):]
    L, Ns, Ng = len(loci), len(s_cells), len(g_cells)
    vs, vg = s[input_col].to_numpy(dtype=np.float64), g[input_col].to_numpy(dtype=np.float64)
    Xs, Ms, Xg, Mg = np.zeros((L, Ns)), np.zeros((L, Ns)), np.zeros((L, Ng)), np.zeros((L, Ng))
    np.add.at(Ms, (ks, s_code), 1.0)
    np.add.at(Mg, (kg, g_code), 1.0)
    if Ms.max() > 1 or (Ng and Mg.max() > 1):
        raise ValueError("a cell holds a locus twice")
    Xs[ks, s_code], Xg[kg, g_code] = vs, vg
    rows_s = np.argsort(s_code, kind="stable")
    off_s = np.searchsorted(s_code[rows_s], np.arange(Ns + 1))
    by_clone = clone_col in g.columns and clone_col in s.columns
    if by_clone:
        clone_s = s[clone_col].to_numpy()[rows_s[off_s[:-1]]]
        clone_g_rows = g[clone_col].to_numpy()
        # a G1 cell whose rows name more than one clone is a candidate with its rows of the clone only
        cl_code = pd.factorize(clone_g_rows)[0]
        lo, hi = np.full(Ng, np.iinfo(np.int64).max), np.full(Ng, -1)
        np.minimum.at(lo, g_code, cl_code)
        np.maximum.at(hi, g_code, cl_code)
        mixed = lo != hi
    R = _masked_pearson(Xs, Ms, Xg, Mg, dev) if Ng else np.zeros((Ns, 0))

    g_state, g_ploidy = g[cn_state_col].to_numpy(dtype=np.float64), g[ploidy_col].to_numpy(dtype=np.float64)
    s_ploidy = s[ploidy_col].to_numpy(dtype=np.float64)
    g_pos = np.full((L, Ng), -1, dtype=np.int64)                       # the G1 row of (locus, cell)
    g_pos[kg, g_code] = np.arange(len(g))
    frames, full = [], []
    for i in range(Ns):
        rows = rows_s[off_s[i]:off_s[i + 1]]                            # the cell's rows, in table order
        if by_clone:
            # the reference's candidates: the G1 ROWS of the clone, grouped by (sorted) cell
            cand = np.unique(g_code[clone_g_rows == clone_s[i]])
        else:
            cand = np.arange(Ng)
        if cand.size == 0:
            raise ValueError("No objects to concatenate: S cell {} has no G1 cell of its clone to correlate "
                             "with (compute_cell_corrs)".format(s_cells[i]))

        def exact_r(j):
            """scipy's pearsonr over the shared loci of S cell i and the rows of G1 cell j that belong
            to the candidates' table, the S cell's order."""
            gr = g_pos[ks[rows], j]
            hit = gr >= 0
            if by_clone:
                hit &= clone_g_rows[np.where(hit, gr, 0)] == clone_s[i]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return float(pearsonr(vs[rows[hit]], vg[gr[hit]])[0]), hit, gr

        r = R[i, cand].copy()
        split = by_clone and bool(mixed[cand].any())
        top = np.sort(r)[-2:]
        if split or not np.isfinite(r).all() or (len(r) > 1 and abs(top[1] - top[0]) <= 1e-9 * abs(top[1])):
            r = np.array([exact_r(j)[0] for j in cand])                 # a near tie: the reference's own numbers
        j = int(cand[prep.rank_desc_like_pandas(r[None, :])[0, 0]])
        r_best, hit, gr = exact_r(j)
        cols = {chr_col: s[chr_col].to_numpy()[rows[hit]], start_col: s[start_col].to_numpy()[rows[hit]],
                cell_col: s[cell_col].to_numpy()[rows[hit]]}
        q = _g1_quotient(vs[rows[hit]], g_ploidy[gr[hit]], g_state[gr[hit]], s_ploidy[rows[hit]])
        f = pd.DataFrame(cols)
        f[temp_col] = _scale(q) if len(q) else q
        f['G1_match_cell_id'] = g_cells[j]
        f['G1_match_pearsonr'] = r_best
        f['_row'] = rows[hit]
        # remove_cell_specific_CNAs is called without the column names (:257): the defaults
        f = sort_by_cell_and_loci(f, cell_col='cell_id', chr_col='chr', start_col='start').copy()
        frames.append(f)
    frames, _ = _finish_cells(frames, temp_col, output_col, seg_col, 'chr', dev)

    rest = [c for c in s.columns if c not in (chr_col, start_col, cell_col)]
    for f in frames:
        # pd.merge(temp_merged_cn, cell_cn) (:260): the keys come back as the S table's labels, and a
        # row whose category is NaN finds no partner
        keep = f['chr'].notna().to_numpy() if isinstance(f['chr'].dtype, pd.CategoricalDtype) else np.ones(len(f), bool)
        f = f[keep]
        src = s.iloc[f.pop('_row').to_numpy()]
        f = f.reset_index(drop=True)
        f[chr_col] = src[chr_col].to_numpy()
        for c in rest:
            f[c] = src[c].to_numpy()
        full.append(f)
    return pd.concat(full, ignore_index=True)
