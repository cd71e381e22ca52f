"""The cell-cycle-classifier features (reference scdna_replication_tools/compute_ccc_features.py):
per cell the bimodality score ``lrs`` (the log likelihood ratio statistic of a 1-component against
a 2-component Gaussian mixture of the clone-normalised read depth), ``madn`` (the median absolute
difference of adjacent bins) and ``breakpoints`` (copy-number changes within chromosomes), with
the per-clone normalisation before them and the read-count / clone corrections after them.

The reference loops over cells: two sklearn ``GaussianMixture`` fits, a median, a nested
``groupby('chr')`` and three ``cn.loc`` writes each.  Here (``features_matrix``) all cells of one
length are one launch of ``pert_ccc_features`` (csrc/ccc_kernels.hip, fp64, one workgroup per
cell).  The kernel marks every cell in which a k-means / EM decision sits within its rounding
margin of flipping under another summation order (``binarize.margins``); those cells' scores are
recomputed on the host with sklearn itself, so they are the reference's own.  Without a GPU the
host path serves every cell.

The random stream.  The reference fits with ``random_state=None``: every cell, in sorted-cell
order, consumes exactly 4 doubles of numpy's global generator -- d0 the 1-component k-means++
``choice``, d1 the 2-component ``choice``, d2 and d3 its two local-trial uniforms.  This module
draws ``random_sample(4 N)`` once from the same generator (``random_state=None``; an int or a
``RandomState`` is also accepted), so the generator is left where the reference leaves it and
``np.random.seed(s)`` before a call reproduces the reference seeded the same way; the host path
fits cell n on a private ``RandomState`` set to the start state and advanced by 4 n doubles.
"""
from __future__ import annotations

import ctypes
from argparse import ArgumentParser
from dataclasses import dataclass
from typing import Optional

import numpy as np
import pandas as pd
import torch

from . import binarize, tau_init
from .predict_cycle_phase import _segments, autocorr  # noqa: F401  (autocorr: the reference's name here)

DRAWS_PER_CELL = 4


# ----------------------------------------------------------------------------------------------
# the random stream
# ----------------------------------------------------------------------------------------------

class _Stream:
    """The draws of ``n_cells`` cells taken at once from the caller's generator, and the
    generator's state before them (what a private generator of the host path starts from)."""

    def __init__(self, random_state, n_cells: int):
        if random_state is None:
            self.start = np.random.get_state()
            d = np.random.random_sample(DRAWS_PER_CELL * n_cells)
        else:
            if isinstance(random_state, (int, np.integer)):
                random_state = np.random.RandomState(int(random_state))
            if not isinstance(random_state, np.random.RandomState):
                raise TypeError("random_state must be None, an int or a numpy.random.RandomState")
            self.start = random_state.get_state()
            d = random_state.random_sample(DRAWS_PER_CELL * n_cells)
        self.draws = d.reshape(n_cells, DRAWS_PER_CELL)
        self.index = np.arange(n_cells)            # the cells' places in the stream

    def subset(self, sel) -> "_Stream":
        s = object.__new__(_Stream)
        s.start, s.draws, s.index = self.start, self.draws[sel], self.index[sel]
        return s

    def walker(self):
        """rs_at(n), for increasing n: a private RandomState placed at cell n's first draw."""
        rs = np.random.RandomState()
        rs.set_state(self.start)
        at = [0]

        def rs_at(n: int):
            assert n >= at[0]
            if n > at[0]:
                rs.random_sample(DRAWS_PER_CELL * (n - at[0]))
            at[0] = n + 1                          # the cell's two fits consume its 4 draws
            return rs
        return rs_at


def first_centres(d: np.ndarray, L: int) -> np.ndarray:
    """``RandomState.choice(L, p=ones(L) / L)`` for each double of ``d`` (what sklearn's
    k-means++ does with float64 unit sample weights): searchsorted(cdf, d, 'right')."""
    w = np.ones(L, dtype=np.float64)
    cdf = (w / w.sum()).cumsum()
    cdf /= cdf[-1]
    return cdf.searchsorted(d, side="right").astype(np.int32)


# ----------------------------------------------------------------------------------------------
# one length: the launch, and the host path
# ----------------------------------------------------------------------------------------------

def ccc_params(L: int):
    """The pert_ccc_params at L bins: sklearn's defaults and ``binarize.margins(L)``."""
    from ._native import PertCccParams
    p = PertCccParams()
    p.lloyd_max_iter, p.em_max_iter, p.em_tol, p.reg_covar = 300, 100, 1e-3, 1e-6
    m = binarize.margins(L)
    p.pp_margin, p.tie_margin, p.lloyd_margin, p.em_margin = (m["pp_margin"], m["tie_margin"], m["lloyd_margin"],
                                                              m["em_margin"])
    return p


def native_features(X: torch.Tensor, draws: np.ndarray, p, state: Optional[torch.Tensor] = None,
                    chrom: Optional[torch.Tensor] = None) -> dict:
    """One launch of pert_ccc_features on X's device and current stream.  X (L, N) float64 on a
    GPU, ``draws`` (N, 4) the cells' doubles, ``state`` / ``chrom`` (L, N) integer tensors or both
    None; returns device tensors score1, score2, lrs, madn float64 and breakpoints, flags int32,
    all (N,)."""
    from . import _native
    L, N = X.shape
    dev = X.device
    rows = X.T.contiguous()                                          # (N, L): one row per cell
    draws = np.ascontiguousarray(draws, dtype=np.float64).reshape(N, DRAWS_PER_CELL)
    first = torch.from_numpy(first_centres(draws[:, :2].reshape(-1), L).reshape(N, 2).T.copy()).to(dev)   # (2, N)
    u = torch.from_numpy(np.ascontiguousarray(draws[:, 2:])).to(dev)
    if (state is None) != (chrom is None):
        raise ValueError("state and chrom come together")
    st = state.T.to(torch.int32).contiguous() if state is not None else None
    ch = chrom.T.to(torch.int32).contiguous() if chrom is not None else None
    scratch = torch.empty((2, N, L), dtype=torch.int8, device=dev)
    out = {k: torch.empty(N, dtype=torch.float64, device=dev) for k in ("score1", "score2", "lrs", "madn")}
    out.update({k: torch.empty(N, dtype=torch.int32, device=dev) for k in ("breakpoints", "flags")})
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _native.check(_native.lib().pert_ccc_features(
            L, N, rows.data_ptr(), first[0].data_ptr(), first[1].data_ptr(), u.data_ptr(),
            st.data_ptr() if st is not None else None, ch.data_ptr() if ch is not None else None, ctypes.byref(p),
            scratch.data_ptr(), out["score1"].data_ptr(), out["score2"].data_ptr(), out["lrs"].data_ptr(),
            out["madn"].data_ptr(), out["breakpoints"].data_ptr(), out["flags"].data_ptr(), ctypes.c_void_p(stream)),
            "pert_ccc_features")
    return out


def exact_scores(x: np.ndarray, rs: np.random.RandomState):
    """One cell's two fits the reference's way (compute_ccc_features.py:22-27) on ``rs``, a
    generator placed at the cell's first draw: (score1, score2, lrs)."""
    from sklearn.mixture import GaussianMixture
    X = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 1)
    s1 = GaussianMixture(n_components=1, random_state=rs).fit(X).score(X)
    s2 = GaussianMixture(n_components=2, random_state=rs).fit(X).score(X)
    return s1, s2, -2 * (s1 - s2)


def adjacent_breakpoints(state: np.ndarray, chrom: np.ndarray) -> np.ndarray:
    """What the kernel counts, for the columns of (L, N) arrays: rows whose state differs from
    the row before on the same chromosome."""
    return ((state[1:] != state[:-1]) & (chrom[1:] == chrom[:-1])).sum(0).astype(np.int64)


@dataclass
class CccFeatures:
    """``features_matrix``'s result for the N cells (columns) of an (L, N) matrix."""
    madn: np.ndarray           # (N,) median |x[i+1] - x[i]|
    lrs: np.ndarray            # (N,) -2 (score1 - score2)
    score1: np.ndarray         # (N,) mean log-likelihood of the 1-component mixture
    score2: np.ndarray         # (N,) of the 2-component mixture
    breakpoints: Optional[np.ndarray]   # (N,) int64, or None without state / chrom
    flags: np.ndarray          # (N,) int32: the kernel's flag bits (0 on the host path)
    flagged: np.ndarray        # (N,) bool: scores recomputed on the host


def features_matrix(X, state=None, chrom=None, *, random_state=None, device=None,
                    _stream: Optional[_Stream] = None) -> CccFeatures:
    """compute_ccc_features.py:19-34 for every column (cell) of X, an (L, N) float64 tensor or
    array, columns in the reference's (sorted-cell) order; with ``state`` and ``chrom`` (L, N)
    integer arrays also the breakpoints between adjacent rows of one chromosome.  ``device``:
    where it runs (default: X's device for a tensor, else the GPU when there is one); on a GPU it
    is one launch of pert_ccc_features and the flagged cells' scores are then recomputed by
    ``exact_scores``; on the CPU, and for non-finite input or fewer than 2 bins (sklearn's
    ValueError surfaces), every cell is.  ``_stream``: the cells' draws when the caller (a ragged
    table's ``calculate_features``) has drawn them for all its cells at once."""
    if isinstance(X, torch.Tensor):
        dev = torch.device(device) if device is not None else X.device
        Xn = X.detach().cpu().numpy()
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        Xn = np.asarray(X)
    if Xn.dtype != np.float64:
        raise TypeError("features_matrix fits float64 profiles, as the reference does: X must be float64")
    if Xn.ndim != 2 or Xn.shape[0] < 1 or Xn.shape[1] < 1:
        raise ValueError("X must be (L, N) with N >= 1 cells")
    if (state is None) != (chrom is None):
        raise ValueError("state and chrom come together")
    L, N = Xn.shape
    stream = _stream if _stream is not None else _Stream(random_state, N)
    assert stream.draws.shape == (N, DRAWS_PER_CELL)
    on_gpu = dev.type == "cuda" and L >= 2 and bool(np.isfinite(Xn).all())
    if on_gpu:
        as_dev = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dev)
        Xt = X.to(dev) if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(Xn)).to(dev)
        raw = native_features(Xt, stream.draws, ccc_params(L), as_dev(state), as_dev(chrom))
        r = {k: v.cpu().numpy() for k, v in raw.items()}
        madn, lrs, score1, score2, flags = r["madn"], r["lrs"], r["score1"], r["score2"], r["flags"]
        bk = r["breakpoints"].astype(np.int64) if state is not None else None
        flagged = flags != 0
        todo = np.flatnonzero(flagged)
    else:
        madn = np.median(np.abs(np.diff(Xn, axis=0)), axis=0) if L >= 2 else np.full(N, np.nan)
        lrs, score1, score2 = np.empty(N), np.empty(N), np.empty(N)
        flags = np.zeros(N, dtype=np.int32)
        bk = adjacent_breakpoints(np.asarray(state), np.asarray(chrom)) if state is not None else None
        flagged = np.ones(N, dtype=bool)
        todo = np.arange(N)
    if todo.size:
        rs_at = stream.walker()
        todo = todo[np.argsort(stream.index[todo], kind="stable")]
        with tau_init.host_threads():                # library scans up front; sklearn on this one thread
            for n in todo:
                score1[n], score2[n], lrs[n] = exact_scores(Xn[:, n], rs_at(int(stream.index[n])))
    return CccFeatures(madn=madn, lrs=lrs, score1=score1, score2=score2, breakpoints=bk, flags=flags, flagged=flagged)


# ----------------------------------------------------------------------------------------------
# the reference's functions on whole columns
# ----------------------------------------------------------------------------------------------

def get_args():
    p = ArgumentParser()
    p.add_argument('input', help='copynumber tsv file with the columns the cell cycle classifier features need')
    p.add_argument('output', help='the input with the features added as new columns')
    return p.parse_args()


def _cells(cn, cell_col):
    """Rows grouped by sorted cell in row order (groupby semantics; a NaN cell is no cell):
    (cells, row positions grouped, offsets)."""
    ids = cn[cell_col].to_numpy()
    rows = np.flatnonzero(~pd.isna(ids))
    cells, _, order, offs = _segments(ids[rows])
    return cells, rows[order], offs


def _by_length(order, offs):
    """Per profile length L: (L, the cells of that length, their (n, L) row positions)."""
    lens = np.diff(offs)
    for L in np.unique(lens):
        sel = np.flatnonzero(lens == L)
        yield int(L), sel, order[offs[sel][:, None] + np.arange(L)[None, :]]


def _set_int_column(frame, col, values):
    """``frame[col] = 0`` followed by the reference's ``.loc`` writes of ``values``: the column
    stays int64 while every value written is whole, else it becomes float64."""
    v = np.asarray(values)
    if v.dtype.kind == "f" and np.isfinite(v).all() and (v == np.round(v)).all() and np.abs(v).max(initial=0) < 2.0 ** 63:
        v = v.astype(np.int64)
    frame[col] = v


def _sorted_breakpoints(codes: np.ndarray, chr_col: np.ndarray, state: np.ndarray, n_cells: int) -> np.ndarray:
    """calculate_breakpoints for rows grouped by cell (``codes`` ascending) whose chromosomes are
    not contiguous: a stable sort by (cell, chromosome) gathers each chromosome's rows in row order,
    as the reference's groupby('chr') does; rows without a chromosome belong to none."""
    cc, _ = pd.factorize(chr_col)
    keep = cc >= 0
    codes, cc, state = codes[keep], cc[keep], state[keep]
    o = np.lexsort((cc, codes))
    codes, cc, state = codes[o], cc[o], state[o]
    hit = (codes[1:] == codes[:-1]) & (cc[1:] == cc[:-1]) & (state[1:] != state[:-1])
    return np.bincount(codes[1:][hit], minlength=n_cells).astype(np.int64)


def _contiguous_chromosomes(codes: np.ndarray, cc: np.ndarray) -> bool:
    """Whether, in rows grouped by cell, every cell's rows of one chromosome are one run."""
    if codes.size == 0:
        return True
    runs = 1 + int(((codes[1:] != codes[:-1]) | (cc[1:] != cc[:-1])).sum())
    pairs = np.unique(codes.astype(np.int64) * (int(cc.max()) + 1) + cc).size
    return runs == pairs


def breakpoints(data):
    """The number of adjacent elements of ``data`` that differ."""
    return int(np.sum(np.diff(np.asarray(data)) != 0))


def calculate_breakpoints(cn, cell_col='cell_id', cn_col='state', bk_col='breakpoints'):
    """compute_ccc_features.py:43-56 on whole columns (in place, and returned): ``bk_col`` int64,
    per cell the state changes between adjacent rows of each chromosome."""
    cells, order, offs = _cells(cn, cell_col)
    codes = np.repeat(np.arange(len(cells)), np.diff(offs))
    per_cell = _sorted_breakpoints(codes, cn['chr'].to_numpy()[order], cn[cn_col].to_numpy()[order], len(cells))
    out = np.zeros(len(cn), dtype=np.int64)
    out[order] = per_cell[codes]
    cn[bk_col] = out
    return cn


def calculate_features(cn, cell_col='cell_id', rpm_norm_col='rpm_clone_norm', madn_col='madn', lrs_col='lrs',
                       bk_col='breakpoints', cn_col='state', *, random_state=None, device=None):
    """compute_ccc_features.py:18-40 on whole columns (in place, and returned): ``madn_col`` and
    ``lrs_col`` float64 per row, and ``bk_col`` when the table lacks it.  Cells of one length are
    one ``features_matrix`` pass (one launch on a GPU); the breakpoints ride in that launch when
    every cell's chromosomes are contiguous and its states are integers, else they are counted on
    the host by a stable sort."""
    vals = cn[rpm_norm_col].to_numpy(dtype=np.float64)
    cells, order, offs = _cells(cn, cell_col)
    n_cells, n_rows = len(cells), len(cn)
    codes = np.repeat(np.arange(n_cells), np.diff(offs))
    want_bk = bk_col not in cn.columns
    st = ch = None
    if want_bk:
        state = cn[cn_col].to_numpy()
        cc, _ = pd.factorize(cn['chr'].to_numpy())
        in_launch = (state.dtype.kind in "iub" or (state.dtype.kind == "f" and np.isfinite(state[order]).all()
                                                   and (state[order] == np.round(state[order])).all()))
        in_launch = in_launch and (cc[order] >= 0).all() and _contiguous_chromosomes(codes, cc[order])
        in_launch = in_launch and (state.size == 0 or np.abs(state[order]).max(initial=0) < 2 ** 31)
        if in_launch:
            st, ch = state.astype(np.int64), cc.astype(np.int64)
    stream = _Stream(random_state, n_cells)
    madn, lrs, bk = np.empty(n_cells), np.empty(n_cells), np.zeros(n_cells, dtype=np.int64)
    for L, sel, pos in _by_length(order, offs):
        res = features_matrix(np.ascontiguousarray(vals[pos].T), None if st is None else st[pos].T,
                              None if ch is None else ch[pos].T, device=device, _stream=stream.subset(sel))
        madn[sel], lrs[sel] = res.madn, res.lrs
        if st is not None:
            bk[sel] = res.breakpoints
    for col, per_cell in ((madn_col, madn), (lrs_col, lrs)):
        out = cn[col].to_numpy(dtype=np.float64).copy() if col in cn.columns else np.full(n_rows, np.nan)
        out[order] = per_cell[codes]
        cn[col] = out
    if want_bk:
        if st is None:
            bk = _sorted_breakpoints(codes, cn['chr'].to_numpy()[order], cn[cn_col].to_numpy()[order], n_cells)
        out = np.zeros(n_rows, dtype=np.int64)
        out[order] = bk[codes]
        cn[bk_col] = out
    return cn


def correct_breakpoints(cell_features, bk_col='breakpoints', clone_col='clone_id', output_col='corrected_breakpoints'):
    """compute_ccc_features.py:59-67 (in place, and returned): each cell's breakpoints minus its
    clone's mean; rows without a clone keep 0."""
    bk = cell_features[bk_col].to_numpy()
    codes, clones = pd.factorize(cell_features[clone_col].to_numpy(), sort=True)
    out = np.zeros(len(cell_features), dtype=np.float64)
    for k in range(len(clones)):                        # per clone: np.mean's own summation
        m = codes == k
        out[m] = bk[m] - np.mean(bk[m])
    _set_int_column(cell_features, output_col, out)
    return cell_features


def correct_madn(cell_features, madn_col='madn', num_reads_col='total_mapped_reads_hmmcopy', output_col='corrected_madn'):
    """compute_ccc_features.py:70-79 (in place, and returned): the residual of a linear regression
    of madn on the cell's read count."""
    from sklearn.linear_model import LinearRegression
    reads = cell_features[num_reads_col].to_numpy().reshape(-1, 1)
    fitted = LinearRegression().fit(reads, cell_features[madn_col].to_numpy()).predict(reads)
    cell_features[output_col] = cell_features[madn_col] - fitted
    return cell_features


def compute_clone_normalization(cn, rpm_col='rpm', rpm_norm_col='rpm_clone_norm', clone_col='clone_id', cell_col='cell_id'):
    """compute_ccc_features.py:82-100: per clone the (chr, start) x cell matrix of ``rpm_col``
    (pandas' pivot: sorted loci, duplicates averaged), gaps interpolated linearly down the loci,
    every cell divided by the clone's mean profile; loci that are not finite in every cell of every
    clone are dropped; returns the rows of ``cn`` (in order, fresh index) that are left, with
    ``rpm_norm_col`` appended -- an inner join, without the melt and merge."""
    mats = []
    for _, chunk in cn.groupby(clone_col):
        mat = chunk.pivot_table(values=rpm_col, index=['chr', 'start'], columns=cell_col).interpolate(method='linear', axis=0)
        mats.append(mat.divide(mat.mean(axis=1), axis=0))
    full = pd.concat(mats, axis=1).dropna(axis=0)
    li = full.index.get_indexer(pd.MultiIndex.from_arrays([cn['chr'].to_numpy(), cn['start'].to_numpy()]))
    ci = full.columns.get_indexer(cn[cell_col].to_numpy())
    keep = (li >= 0) & (ci >= 0)
    out = cn[keep].reset_index(drop=True)
    out[rpm_norm_col] = full.to_numpy(dtype=np.float64)[li[keep], ci[keep]]
    return out


def compute_read_count(cn, input_col='reads', output_col='total_mapped_reads_hmmcopy'):
    """compute_ccc_features.py:114-119 (in place, and returned): the sum of ``input_col`` over
    each cell's rows (NaN skipped)."""
    v = cn[input_col].to_numpy()
    if v.dtype.kind == "f":
        v = np.where(np.isnan(v), 0.0, v)
    cells, order, offs = _cells(cn, 'cell_id')
    total = np.zeros(len(cells), dtype=v.dtype if v.dtype.kind in "iuf" else np.float64)
    for L, sel, pos in _by_length(order, offs):
        total[sel] = v[pos].sum(axis=1)                  # each row pairwise, as the reference's per-cell sum
    out = np.zeros(len(cn), dtype=total.dtype)
    out[order] = np.repeat(total, np.diff(offs))
    _set_int_column(cn, output_col, out)
    return cn


def compute_cell_frac(cn, frac_rt_col='cell_frac_rep', rep_state_col='model_rep_state'):
    """compute_ccc_features.py:121-131 (in place, and returned): each cell's fraction of
    replicated bins, and whether it is beyond 0.05 / 0.95."""
    cells, order, offs = _cells(cn, 'cell_id')
    lens = np.diff(offs)
    codes = np.repeat(np.arange(len(cells)), lens)
    rep = cn[rep_state_col].to_numpy()[order].astype(np.float64)
    frac = np.bincount(codes, weights=rep, minlength=len(cells)) / lens
    extreme = np.zeros(len(cn), dtype=bool)
    extreme[order] = ((frac > 0.95) | (frac < 0.05))[codes]
    cn['extreme_cell_frac'] = extreme
    out = cn[frac_rt_col].to_numpy(dtype=np.float64).copy() if frac_rt_col in cn.columns else np.full(len(cn), np.nan)
    out[order] = frac[codes]
    cn[frac_rt_col] = out
    return cn


def compute_ccc_features(cn, cell_col='cell_id', rpm_col='rpm', cn_col='state', clone_col='clone_id', madn_col='madn',
                         lrs_col='lrs', num_reads_col='total_mapped_reads_hmmcopy', bk_col='breakpoints', *,
                         random_state=None, device=None):
    """compute_ccc_features.py:134-186: the per-cell features of the cell cycle classifier.

    ``cn`` holds ``cell_col``, chr, start, ``rpm_col`` (read depth), ``cn_col`` (copy-number
    state) and ``clone_col``; ``num_reads_col`` and ``bk_col`` are computed when absent.  Returns
    (cn_out, cell_features): the rows that survive the clone normalisation with
    ``<rpm_col>_clone_norm``, ``madn_col``, ``lrs_col``, ``bk_col``, ``num_reads_col`` and the
    corrected madn / breakpoints, and one row per cell of those features."""
    rpm_norm_col = '{}_clone_norm'.format(rpm_col)
    cn = compute_clone_normalization(cn, rpm_col=rpm_col, rpm_norm_col=rpm_norm_col, clone_col=clone_col, cell_col=cell_col)
    cn = calculate_features(cn, rpm_norm_col=rpm_norm_col, madn_col=madn_col, lrs_col=lrs_col, cell_col=cell_col,
                            bk_col=bk_col, cn_col=cn_col, random_state=random_state, device=device)
    if num_reads_col not in cn.columns:
        cn = compute_read_count(cn, input_col=rpm_col, output_col=num_reads_col)
    cell_features = cn[[cell_col, clone_col, madn_col, lrs_col, num_reads_col, bk_col]].drop_duplicates()
    cell_features = correct_madn(cell_features, madn_col=madn_col, num_reads_col=num_reads_col,
                                 output_col='corrected_{}'.format(madn_col))
    cell_features = correct_breakpoints(cell_features, bk_col=bk_col, clone_col=clone_col,
                                        output_col='corrected_{}'.format(bk_col))
    return pd.merge(cn, cell_features), cell_features


def main():
    argv = get_args()
    cn = pd.read_csv(argv.input, sep='\t')
    cn, _ = compute_ccc_features(cn)
    cn.to_csv(argv.output, sep='\t', index=False)


if __name__ == '__main__':
    main()
