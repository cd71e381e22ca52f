"""Phase calls from the decode's state matrices: the matrix layer beside predict_cycle_phase.py.

The DataFrame functions of ``predict_cycle_phase`` need the long table, scatter its columns into
padded fp64 tensors and run one slice-multiply-sum per lag.  ``PhaseMatrix`` holds the bins x cells
matrices themselves -- the decode's ``uint8 [L][ldn]`` replication and copy-number states and the
shard's ``reads``, on the GPU in place, or numpy arrays -- and never forms the long table:

* ``pert_phase_counts`` (csrc/phase_kernels.hip) gives, per cell, the integer counts every feature
  of the 0 / 1 replication state follows from: T = sum x_t, the breakpoints, the bins with cn 0,
  S_k = #{t : x_t = x_{t+k} = 1} and the sums of the first and last k states;
* ``pert_phase_acf`` gives the mean and the centred lag products of the read depth in fp64;
* without a GPU a chunked numpy path produces the same integers.

Exactness.  With n = L, m = T / n, A_k = T - tail_k and B_k = T - head_k (the sums of the first and
last n - k states), n^2 c_k = n^2 S_k - n T (A_k + B_k) + (n - k) T^2 and n^2 c_0 = n T (n - T) are
integers, so ``rep_auto`` (the mean of c_k / c_0 over lags min_lag - 1 .. max_lag, lag 0 counting as
1) is one exact rational per cell: it is rounded to fp64 once, and at the reference's threshold
``rep_auto > 0.2`` is decided on the rational itself against the exact value of the fp64 0.2.  ``cell_frac_rep = T / L`` and
``frac_cn0 = cn0 / L`` are single fp64 divisions, as the reference's are.  Any positive scaling of
the reads gives the same autocorrelation, so no ``rpm`` column is formed.

``rpm_auto`` is two-pass fp64 like the reference's acf, summed in another order: it agrees with a
per-cell loop of ``predict_cycle_phase.autocorr`` to 8 (n + 2) u (1 + r)^2, r = max|x| sqrt(n / c_0)
(DESIGN.md section 6l).  statsmodels is not part of this stack; parity with it is not claimed.
"""
from __future__ import annotations

import ctypes
from fractions import Fraction
from typing import Optional

import numpy as np
import pandas as pd

from .predict_cycle_phase import MAX_LAG, MIN_LAG, _segments

__all__ = ["PhaseMatrix", "phase_calls", "FEATURE_COLUMNS", "REP_AUTO_THRESH"]

_CHUNK_ELEMS = 1 << 22          # (bin, cell) pairs per chunk of the host passes
REP_AUTO_THRESH = 0.2           # the reference's threshold: the one decided exactly on the integers
FEATURE_COLUMNS = ['cell_id', 'cell_frac_rep', 'rpm_auto', 'rep_auto', 'cn_bk', 'rep_bk', 'frac_cn0']
_RAGGED = ("PhaseMatrix needs a full bins x cells grid in which every cell lists its loci in the same order ({}); "
           "for other tables use the DataFrame functions of predict_cycle_phase (compute_cell_frac, "
           "compute_quality_features, predict_cycle_phase)")


def _check_lags(L: int, min_lag: int, max_lag: int):
    from ._native import PHASE_MAX_LAG
    if not 1 <= min_lag <= max_lag + 1 or not 1 <= max_lag <= PHASE_MAX_LAG:
        raise ValueError("lags must satisfy 1 <= min_lag <= max_lag + 1 and max_lag <= {}".format(PHASE_MAX_LAG))
    if L <= max_lag:
        raise ValueError("a series of {} bins has no pair at lag {}: L must exceed max_lag".format(L, max_lag))
    if L >= 1 << 20:
        raise ValueError("L must be below 2^20")


def pick_device(device, *mats):
    """Where the passes run: ``device`` when given, else the device of the first CUDA tensor among
    ``mats``, else the GPU when there is one, else the CPU.  A CUDA device without an index is
    resolved to the current one, so that it compares equal to the device of the tensors that live
    there (``torch.device('cuda') != torch.device('cuda:0')``) and they are used in place."""
    import torch
    if device is not None:
        dev = torch.device(device)
    else:
        dev = next((m.device for m in mats if torch.is_tensor(m) and m.device.type == "cuda"), None)
        if dev is None:
            dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if dev.type == "cuda" and dev.index is None and torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


# ----------------------------------------------------------------------------------------------
# the two O(L N) passes: device, and chunked numpy with the same integers
# ----------------------------------------------------------------------------------------------

def device_matrix(a, device, dtype):
    """``a`` (L, N) as a tensor of ``dtype`` on ``device`` whose rows are ``ldn`` elements apart
    (ldn >= N a multiple of 16, base 16-byte aligned): a tensor that already is one is used in
    place, anything else is copied into a zero-padded buffer.  Returns (the (L, N) view, ldn)."""
    import torch
    if torch.is_tensor(a) and a.device == device and a.dtype == dtype:
        ldn = int(a.stride(0)) if a.shape[0] > 1 else int(a.shape[1])
        if a.stride(1) == 1 and ldn >= a.shape[1] and ldn % 16 == 0 and a.data_ptr() % 16 == 0:
            return a, ldn
    L, N = int(a.shape[0]), int(a.shape[1])
    ldn = -(-N // 256) * 256
    buf = torch.zeros((L, ldn), dtype=dtype, device=device)
    buf[:, :N] = a.to(device=device, dtype=dtype) if torch.is_tensor(a) else torch.from_numpy(
        np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    return buf[:, :N], ldn


def device_planes(a, device):
    """``a`` (D, L, N) uint8 as a device tensor with the layout pert_phase_counts reads: used in place
    when it has it.  Returns (the (D, L, N) view, ldn, plane stride in bytes)."""
    import torch
    D, L, N = (int(v) for v in a.shape)
    if torch.is_tensor(a) and a.device == device and a.dtype == torch.uint8:
        ldn, ps = int(a.stride(1)), int(a.stride(0))
        if (a.stride(2) == 1 and ldn >= N and ldn % 16 == 0 and a.data_ptr() % 16 == 0 and ps >= L * ldn
                and ps % 16 == 0):
            return a, ldn, ps
    ldn = -(-N // 256) * 256
    buf = torch.zeros((D, L, ldn), dtype=torch.uint8, device=device)
    buf[:, :, :N] = a.to(device) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return buf[:, :, :N], ldn, L * ldn


def device_counts(rep, cn, ldn: int, plane_stride: int, max_lag: int) -> dict:
    """One pert_phase_counts launch over ``rep`` / ``cn`` (D, L, N) uint8 device views of one layout
    (``cn`` may be None): int64 arrays ``T``, ``rep_bk``, ``cn_bk``, ``cn0`` (D, N) and ``S``, ``head``,
    ``tail`` (D, max_lag, N)."""
    import torch
    from . import _native as nat
    D, L, N = (int(v) for v in rep.shape)
    dev = rep.device
    with torch.cuda.device(dev):
        per_cell = torch.zeros((4, D, N), dtype=torch.int32, device=dev)
        per_lag = torch.zeros((3, D, max_lag, N), dtype=torch.int32, device=dev)
        nat.check(nat.lib().pert_phase_counts(
            L, N, ldn, D, plane_stride, rep.data_ptr(), cn.data_ptr() if cn is not None else None, max_lag,
            per_cell[0].data_ptr(), per_cell[1].data_ptr(), per_cell[2].data_ptr(), per_cell[3].data_ptr(),
            per_lag[0].data_ptr(), per_lag[1].data_ptr(), per_lag[2].data_ptr(),
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "pert_phase_counts")
        pc = per_cell.cpu().numpy().view(np.uint32).astype(np.int64)
        pl = per_lag.cpu().numpy().view(np.uint32).astype(np.int64)
    return dict(T=pc[0], rep_bk=pc[1], cn_bk=pc[2], cn0=pc[3], S=pl[0], head=pl[1], tail=pl[2])


def device_acf(x, ldn: int, max_lag: int):
    """pert_phase_acf over ``x`` (L, N), a float32 / float64 device view: (mean (N,), c (max_lag + 1, N))
    float64 numpy arrays."""
    import torch
    from . import _native as nat
    L, N = int(x.shape[0]), int(x.shape[1])
    dev = x.device
    with torch.cuda.device(dev):
        need = ctypes.c_int64()
        nat.check(nat.lib().pert_phase_acf_workspace(L, N, max_lag, ctypes.byref(need)), "pert_phase_acf_workspace")
        ws = torch.empty(max(int(need.value) // 8, 1), dtype=torch.float64, device=dev)
        mean = torch.empty(N, dtype=torch.float64, device=dev)
        c = torch.empty((max_lag + 1, N), dtype=torch.float64, device=dev)
        nat.check(nat.lib().pert_phase_acf(
            L, N, ldn, x.data_ptr(), int(x.dtype == torch.float64), max_lag, mean.data_ptr(), c.data_ptr(),
            ws.data_ptr(), int(need.value), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
            "pert_phase_acf")
        return mean.cpu().numpy(), c.cpu().numpy()


def host_counts(rep: np.ndarray, cn: Optional[np.ndarray], max_lag: int) -> dict:
    """``device_counts`` for one (L, N) plane in chunked numpy (no plane axis)."""
    L, N = rep.shape
    out = dict(T=np.zeros(N, np.int64), rep_bk=np.zeros(N, np.int64), cn_bk=np.zeros(N, np.int64),
               cn0=np.zeros(N, np.int64), S=np.zeros((max_lag, N), np.int64), head=np.zeros((max_lag, N), np.int64),
               tail=np.zeros((max_lag, N), np.int64))
    step = max(1, _CHUNK_ELEMS // L)
    for n0 in range(0, N, step):
        sl = slice(n0, n0 + step)
        x = rep[:, sl] != 0
        out["T"][sl] = x.sum(axis=0, dtype=np.int64)
        out["rep_bk"][sl] = (x[1:] != x[:-1]).sum(axis=0, dtype=np.int64)
        for k in range(1, max_lag + 1):
            out["S"][k - 1, sl] = (x[:L - k] & x[k:]).sum(axis=0, dtype=np.int64)
        out["head"][:, sl] = np.cumsum(x[:max_lag], axis=0, dtype=np.int64)
        out["tail"][:, sl] = np.cumsum(x[::-1][:max_lag], axis=0, dtype=np.int64)
        if cn is not None:
            c = cn[:, sl]
            out["cn_bk"][sl] = (c[1:] != c[:-1]).sum(axis=0, dtype=np.int64)
            out["cn0"][sl] = (c == 0).sum(axis=0, dtype=np.int64)
    return out


def host_acf(x: np.ndarray, max_lag: int):
    """``device_acf`` in chunked numpy: two passes in fp64 (the mean, then the centred products)."""
    L, N = x.shape
    mean, c = np.empty(N), np.empty((max_lag + 1, N))
    step = max(1, _CHUNK_ELEMS // L)
    with np.errstate(invalid="ignore", over="ignore"):
        for n0 in range(0, N, step):
            sl = slice(n0, n0 + step)
            v = x[:, sl].astype(np.float64)
            m = v.sum(axis=0) / L
            m[~np.isfinite(m)] = np.nan
            d = v - m
            mean[sl] = m
            for k in range(max_lag + 1):
                c[k, sl] = (d[:L - k] * d[k:]).sum(axis=0)
    return mean, c


# ----------------------------------------------------------------------------------------------
# counts -> features
# ----------------------------------------------------------------------------------------------

def rep_auto_rational(counts: dict, L: int, min_lag: int, max_lag: int):
    """The exact ``rep_auto`` of every cell as (numerator, denominator), object arrays of Python
    ints shaped like ``counts['T']``; the denominator is 0 where the series is constant (T = 0 or
    T = L: the reference's NaN), else positive."""
    lo = min_lag - 1                                     # acf[min_lag - 1:]: lags lo .. max_lag
    ks = np.arange(max(lo, 1), max_lag + 1)
    T = counts["T"]
    lag = lambda a: a[..., ks - 1, :].sum(axis=-2)       # sums over the lags: < 2^27, int64
    sS = lag(counts["S"])
    sAB = 2 * len(ks) * T - lag(counts["head"]) - lag(counts["tail"])
    sNK = int((L - ks).sum())
    n = int(L)
    To, c0 = T.astype(object), (n * T.astype(object)) * (n - T.astype(object))     # n^2 c_0 = n T (n - T)
    num = (n * n) * sS.astype(object) - (n * To) * sAB.astype(object) + sNK * (To * To)
    if lo == 0:
        num = num + c0                                   # lag 0: c_0 / c_0 = 1
    return num, c0 * (max_lag - lo + 1)


def _ratio(num, den) -> np.ndarray:
    """num / den rounded to fp64 once (Python's int / int is correctly rounded); NaN where den = 0."""
    out = np.full(num.shape, np.nan)
    ok = den != 0
    out[ok] = [a / b for a, b in zip(num[ok], den[ok])]
    return out


def exceeds(num, den, thresh: float) -> np.ndarray:
    """num / den > thresh, decided on the integers against the exact value of the fp64 ``thresh``
    (False where den = 0, as NaN > thresh is)."""
    t = Fraction(float(thresh))
    out = np.zeros(num.shape, bool)
    ok = den != 0
    out[ok] = [a * t.denominator > t.numerator * b for a, b in zip(num[ok], den[ok])]
    return out


def rep_auto_exceeds(num, den, thresh: float) -> np.ndarray:
    """The low-quality test ``rep_auto > thresh`` per cell.  At the reference's threshold
    (REP_AUTO_THRESH) it is decided exactly, on the integers; at any other threshold it is the fp64
    comparison of the rounded ``rep_auto`` column, so it agrees with ``table['rep_auto'] > thresh``."""
    if float(thresh) == REP_AUTO_THRESH:
        return exceeds(num, den, thresh)
    with np.errstate(invalid="ignore"):
        return _ratio(num, den) > thresh


def rpm_auto_from(c: np.ndarray, min_lag: int) -> np.ndarray:
    """np.mean(acf[min_lag - 1:]) per cell from the lag products c (max_lag + 1, N)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        ac = c / c[0]
        ac[0] = np.where(np.isnan(ac[0]), np.nan, 1.0)
        return ac[min_lag - 1:].mean(axis=0)


def call_phases(frac, lq_auto, frac_cn0, frac_thresh=0.05, frac_cn0_thresh=0.05) -> np.ndarray:
    """predict_cycle_phase.py:106-115 per cell: 'G1/2' unless thresh < frac < 1 - thresh, then 'LQ'
    where ``lq_auto`` (rep_auto > its threshold) or frac_cn0 > its threshold, else 'S'."""
    assert frac_thresh < 0.5
    replicating = (frac > frac_thresh) & (frac < (1 - frac_thresh))
    low = lq_auto | (frac_cn0 > frac_cn0_thresh)
    return np.where(~replicating, 'G1/2', np.where(low, 'LQ', 'S')).astype(object)


# ----------------------------------------------------------------------------------------------
# the matrix layer
# ----------------------------------------------------------------------------------------------

class PhaseMatrix:
    """The bins x cells matrices the phase calls are made from.

    ``rep`` / ``cn``: ``(L, N)`` numpy arrays, or CUDA ``uint8`` tensors used in place (a
    ``PertShard.decode()`` result; rows ``ldn`` apart, as ``RTMatrix`` accepts).  ``reads``: an
    ``(L, N)`` float32 or float64 array or tensor (the shard's ``reads[:, :N]`` works in place).
    ``cell_ids [N]`` label the columns.  ``device=None`` runs the passes on the GPU when there is one
    (always, for CUDA tensors), else in chunked numpy; the integers are the same.  ``min_lag`` /
    ``max_lag``: the reference's 10 and 50 (``np.mean(acf(x, nlags=50)[9:])``)."""

    def __init__(self, rep, cn, reads, cell_ids, device: Optional[str] = None, *, min_lag: int = MIN_LAG,
                 max_lag: int = MAX_LAG):
        import torch
        self.cell_ids = np.asarray(cell_ids)
        self.min_lag, self.max_lag = int(min_lag), int(max_lag)
        mats = dict(rep=rep, cn=cn, reads=reads)
        self.device = pick_device(device, rep, cn, reads)
        shape = tuple(int(v) for v in rep.shape)
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise ValueError("rep must be a (bins, cells) matrix")
        for name, m in mats.items():
            if tuple(int(v) for v in m.shape) != shape:
                raise ValueError("{} does not match rep's shape {}".format(name, shape))
        self.L, self.N = shape
        if len(self.cell_ids) != self.N:
            raise ValueError("cell_ids do not match rep's shape {}".format(shape))
        _check_lags(self.L, self.min_lag, self.max_lag)
        is_f64 = (reads.dtype == torch.float64) if torch.is_tensor(reads) else np.asarray(reads).dtype == np.float64
        if self.device.type == "cuda":
            self._rep, self.ldn = device_matrix(self._states(rep, "rep"), self.device, torch.uint8)
            self._cn, ldn_cn = device_matrix(self._states(cn, "cn"), self.device, torch.uint8)
            if ldn_cn != self.ldn:                       # one launch reads both with one row stride
                self._cn = torch.zeros((self.L, self.ldn), dtype=torch.uint8, device=self.device)[:, :self.N].copy_(
                    self._cn)
            self._reads, self.ldn_reads = device_matrix(reads, self.device,
                                                        torch.float64 if is_f64 else torch.float32)
        else:
            host = lambda m: m.detach().cpu().numpy() if torch.is_tensor(m) else np.asarray(m)
            self._rep, self._cn = self._states(host(rep), "rep"), self._states(host(cn), "cn")
            self._reads = host(reads)
            if self._reads.dtype not in (np.float32, np.float64):
                self._reads = self._reads.astype(np.float64)
            self.ldn = self.ldn_reads = self.N
        self._raw = None

    @staticmethod
    def _states(m, name):
        """A state matrix as uint8 (a tensor stays one); rep must hold 0 / 1."""
        import torch
        if torch.is_tensor(m):
            if m.dtype != torch.uint8:
                raise ValueError("a tensor {} must be uint8 [L][N]".format(name))
            return m
        m = np.asarray(m)
        if m.dtype != np.uint8:
            if m.size and (not np.all(m == np.rint(m)) or m.min() < 0 or m.max() > 255):
                raise ValueError("{} holds values that are not states".format(name))
            m = m.astype(np.uint8)
        if name == "rep" and m.size and m.max() > 1:
            raise ValueError("rep holds values other than 0 and 1")
        return m

    @classmethod
    def from_frame(cls, cn, rep_state_col='model_rep_state', cn_state_col='model_cn_state', reads_col='reads',
                   cell_col='cell_id', chr_col='chr', start_col='start', device: Optional[str] = None, **kw):
        """From a long table that is a full grid: every cell has the same number of rows and lists
        its loci (``chr_col``, ``start_col``) in the same order -- each cell's series is its rows in
        table order, as the reference's groupby sees them.  ValueError otherwise."""
        cells, codes, order, offs = _segments(cn[cell_col].to_numpy())
        lens = np.diff(offs)
        if len(cells) == 0 or (lens != lens[0]).any():
            raise ValueError(_RAGGED.format("the cells differ in their number of rows"))
        N, L = len(cells), int(lens[0])
        for col in (chr_col, start_col):
            key = cn[col].to_numpy()[order].reshape(N, L)
            if (key != key[0]).any():
                raise ValueError(_RAGGED.format("the cells list their loci in different orders"))
        mat = lambda col: np.ascontiguousarray(cn[col].to_numpy()[order].reshape(N, L).T)
        reads = mat(reads_col)
        if reads.dtype not in (np.float32, np.float64):
            reads = reads.astype(np.float64)
        return cls(mat(rep_state_col), mat(cn_state_col), reads, np.asarray(cells), device=device, **kw)

    def release(self):
        """Compute and keep the per-cell results, then drop the matrices (a decode's buffers are
        overwritten by the shard's next call)."""
        self.raw()
        self._rep = self._cn = self._reads = None
        return self

    def raw(self) -> dict:
        """The per-cell results in ``cell_ids`` order (one pass over each matrix, cached): the
        integer ``counts``, the reads' ``mean`` and lag products ``c``, and ``rep_auto`` as an exact
        (numerator, denominator)."""
        if self._raw is None:
            if self.device.type == "cuda":
                counts = {k: v[0] for k, v in device_counts(self._rep[None], self._cn[None], self.ldn, 0,
                                                            self.max_lag).items()}
                mean, c = device_acf(self._reads, self.ldn_reads, self.max_lag)
            else:
                counts = host_counts(self._rep, self._cn, self.max_lag)
                mean, c = host_acf(self._reads, self.max_lag)
            num, den = rep_auto_rational(counts, self.L, self.min_lag, self.max_lag)
            self._raw = dict(counts=counts, mean=mean, c=c, rep_auto_num=num, rep_auto_den=den)
        return self._raw

    def features(self) -> pd.DataFrame:
        """One row per cell, sorted by cell id as the reference's ``cell_metrics`` is: ``cell_id``,
        ``cell_frac_rep``, ``rpm_auto``, ``rep_auto``, ``cn_bk``, ``rep_bk``, ``frac_cn0``."""
        r = self.raw()
        k = r["counts"]
        order = self.order()
        table = pd.DataFrame({
            'cell_id': self.cell_ids, 'cell_frac_rep': k["T"] / float(self.L),
            'rpm_auto': rpm_auto_from(r["c"], self.min_lag), 'rep_auto': _ratio(r["rep_auto_num"], r["rep_auto_den"]),
            'cn_bk': k["cn_bk"], 'rep_bk': k["rep_bk"], 'frac_cn0': k["cn0"] / float(self.L)})
        return table.iloc[order].reset_index(drop=True)

    def order(self) -> np.ndarray:
        """The cells' positions in sorted-id order (the rows of ``features``)."""
        return np.argsort(self.cell_ids, kind="stable")


def phase_calls(mats, frac_thresh=0.05, rep_auto_thresh=0.2, frac_cn0_thresh=0.05) -> pd.DataFrame:
    """predict_cycle_phase on one ``PhaseMatrix`` or several (the S and the G1/2 fit's): their
    feature tables one after the other, ``rpm_auto_norm`` / ``rep_auto_norm`` centred over all cells
    (compute_quality_features) and ``PERT_phase`` in {'S', 'G1/2', 'LQ'} by the reference's order of
    tests.  At the default ``rep_auto_thresh`` the test ``rep_auto > 0.2`` is decided on the exact
    rational against the exact value of the fp64 0.2 (what comparing an unrounded ``rep_auto`` would
    give: it can differ from ``table['rep_auto'] > 0.2`` only where the rounded value equals the
    threshold); at any other threshold the fp64 column is compared."""
    if isinstance(mats, PhaseMatrix):
        mats = [mats]
    mats = list(mats)
    if not mats:
        raise ValueError("phase_calls needs at least one PhaseMatrix")
    table = pd.concat([m.features() for m in mats], ignore_index=True)
    lq_auto = np.concatenate([rep_auto_exceeds(m.raw()["rep_auto_num"], m.raw()["rep_auto_den"], rep_auto_thresh)[m.order()]
                              for m in mats])
    table['rpm_auto_norm'] = table['rpm_auto'] - np.mean(table['rpm_auto'].values)
    table['rep_auto_norm'] = table['rep_auto'] - np.mean(table['rep_auto'].values)
    table['PERT_phase'] = call_phases(table['cell_frac_rep'].to_numpy(), lq_auto, table['frac_cn0'].to_numpy(),
                                      frac_thresh, frac_cn0_thresh)
    return table


def counts_of_planes(rep, cn, max_lag: int = MAX_LAG, device: Optional[str] = None) -> dict:
    """The integer counts of ``rep`` / ``cn`` (n_draws, L, N) uint8 planes with a leading draw axis:
    one pert_phase_counts launch over all of them on a GPU (tensors with the layout of
    ``draw_states`` are used in place), else the chunked numpy pass per plane."""
    import torch
    D, L, N = (int(v) for v in rep.shape)
    dev = pick_device(device, rep, cn)
    if dev.type == "cuda":
        rep_d, ldn, ps = device_planes(rep, dev)
        cn_d, ldn_c, ps_c = device_planes(cn, dev)
        if (ldn_c, ps_c) != (ldn, ps):                   # one launch reads both with one layout
            cn_d = torch.zeros((D, ps), dtype=torch.uint8, device=dev)[:, :L * ldn].view(D, L, ldn)[:, :, :N].copy_(
                cn_d)
        return device_counts(rep_d, cn_d, ldn, ps, max_lag)
    host = lambda m: m.detach().cpu().numpy() if torch.is_tensor(m) else np.asarray(m)
    rep_h, cn_h = host(rep), host(cn)
    per = [host_counts(rep_h[d], cn_h[d], max_lag) for d in range(D)]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def reads_auto(reads, min_lag: int = MIN_LAG, max_lag: int = MAX_LAG, device: Optional[str] = None) -> np.ndarray:
    """``rpm_auto`` of every column of ``reads`` (L, N) float32 / float64: one pert_phase_acf call on
    a GPU (a device tensor with padded rows is used in place), else the numpy pass."""
    import torch
    _check_lags(int(reads.shape[0]), min_lag, max_lag)
    dev = pick_device(device, reads)
    if dev.type == "cuda":
        f64 = (reads.dtype == torch.float64) if torch.is_tensor(reads) else np.asarray(reads).dtype == np.float64
        x, ldn = device_matrix(reads, dev, torch.float64 if f64 else torch.float32)
        _, c = device_acf(x, ldn, max_lag)
    else:
        x = reads.detach().cpu().numpy() if torch.is_tensor(reads) else np.asarray(reads)
        _, c = host_acf(x, max_lag)
    return rpm_auto_from(c, min_lag)
