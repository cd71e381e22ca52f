"""Cell-bootstrap intervals of the pseudobulk replication-timing profiles and of T-width.

``PosteriorDraws`` gives the posterior spread of these statistics; this module gives their
sampling spread over the cells that happened to be sequenced.  A replicate is an integer weight
per cell (how often a resampling picked it), so

* its per-bin counts are ``rep . w`` (``pert_boot_counts``: one weight row per (replicate, group)),
* its histogram of time from scheduled replication is ``RTMatrix``'s rank-1 histogram with every
  (bin, cell) row counted ``w[n]`` times (``pert_boot_tfs_hist``),

and all replicates share one read of the one byte per (bin, cell).  Every replicate equals
``RTMatrix`` run on the matrix whose columns are the original's cells, each repeated ``w[n]``
times: the counts are integers and the host turns them into profiles and hours with
``RTMatrix``'s own operations, so that identity is exact.  Without a GPU (or with an ``RTMatrix``
built with ``device='cpu'``) chunked numpy passes give the same numbers.

Generated weights are a bootstrap stratified by clone, drawn from Philox4x32-10 words by the
rule include/pert_hip.h states for ``pert_boot_weights`` (not numpy's stream); explicit weights
serve subsampling without replacement (0 / 1 rows) and the jackknife.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import pandas as pd

from .posterior_draws import DEFAULT_Q, _summary
from .rt_profiles import (_CHUNK_ELEMS, RTMatrix, _lists_from_hist, _mean_from_sums, _tfs_dtype, interval_edges,
                          twidth_from_points)

TAG_BOOT = 4                            # PERT_TAG_BOOT
_BUDGET_BYTES = 256 << 20               # count + hours of one chunk of replicates (and the resampler's scratch)
_M0, _M1, _W0, _W1, _TAG_MUL = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0x9E3779B9
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


# ----------------------------------------------------------------------------------------------
# the resampler on the host
# ----------------------------------------------------------------------------------------------

def _philox4x32_10(c, k0: int, k1: int):
    """Philox4x32-10 of the counter words ``c`` (four uint64 arrays holding 32-bit values)."""
    c = list(c)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def stratum_layout(strata):
    """(order, pos_lo, pos_n), int32 [N] each: the cell at every position of the cells sorted stably
    by stratum, and the first position and the size of that position's stratum."""
    strata = np.asarray(strata)
    if strata.ndim != 1 or len(strata) < 1:
        raise ValueError("strata must label at least one cell")
    order = np.argsort(strata, kind="stable")
    s = strata[order]
    first = np.concatenate([[True], s[1:] != s[:-1]])
    starts = np.flatnonzero(first)
    sid = np.cumsum(first) - 1
    sizes = np.diff(np.concatenate([starts, [len(s)]]))
    return order.astype(np.int32), starts[sid].astype(np.int32), sizes[sid].astype(np.int32)


def boot_weights_host(strata, n_boot: int, seed: int = 0, b0: int = 0) -> np.ndarray:
    """Replicates ``b0 .. b0 + n_boot - 1`` of the stratified bootstrap, uint8 ``(n_boot, N)``: the
    draws of ``pert_boot_weights`` in numpy.  OverflowError if a cell is picked more than 255 times."""
    order, pos_lo, pos_n = stratum_layout(strata)
    N = len(order)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) ^ ((TAG_BOOT * _TAG_MUL) & 0xFFFFFFFF)
    j = np.arange(N, dtype=np.uint64)
    n_g, lo = pos_n.astype(np.uint64), pos_lo.astype(np.int64)
    out = np.empty((n_boot, N), np.uint8)
    step = max(1, _CHUNK_ELEMS // (4 * N))
    for r0 in range(0, n_boot, step):
        b = (np.arange(r0, min(r0 + step, n_boot), dtype=np.uint64) + np.uint64(b0))[:, None]
        shape = (len(b), N)
        w = _philox4x32_10([np.broadcast_to(j, shape), np.broadcast_to(b & _MASK, shape),
                            np.full(shape, TAG_BOOT, np.uint64), np.broadcast_to(b >> _S32, shape)], k0, k1)
        # mulhi64(w[1] << 32 | w[0], n_g) with n_g < 2^31: both partial products stay below 2^63
        off = (w[1] * n_g + ((w[0] * n_g) >> _S32)) >> _S32
        cell = order[lo[None, :] + off.astype(np.int64)]
        key = np.arange(len(b), dtype=np.int64)[:, None] * N + cell
        counts = np.bincount(key.ravel(), minlength=len(b) * N).reshape(shape)
        if counts.max() > 255:
            raise OverflowError("a cell was drawn more than 255 times in one replicate")
        out[r0:r0 + len(b)] = counts
    return out


# ----------------------------------------------------------------------------------------------
# counts -> hours, all rows at once
# ----------------------------------------------------------------------------------------------

def _hours_from_profiles(values: np.ndarray) -> np.ndarray:
    """``_hours_from_profile`` of every row of ``values [..., L]`` (no NaN, or all NaN, per row),
    bit for bit: the same operations with the row maxima taken by numpy instead of the builtin."""
    v = np.asarray(values)
    if v.size == 0:
        return v.copy()
    late = v - v.max(axis=-1, keepdims=True)
    late *= -1
    with np.errstate(invalid="ignore", divide="ignore"):
        late = late / late.max(axis=-1, keepdims=True)
    late *= 10
    return late


def _sd(a: np.ndarray) -> np.ndarray:
    """Standard deviation over the replicates (axis 0), n - 1 in the denominator."""
    a = np.asarray(a, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return a.std(axis=0, ddof=1) if a.shape[0] > 1 else np.full(a.shape[1:], np.nan)


class CellBootstrap:
    """Resampled cells of an ``RTMatrix``: ``n_boot`` replicates of the bootstrap stratified by
    clone (a clone of ``n`` cells receives ``n`` draws with replacement from itself; the cells
    without a clone form one more stratum; no clone ids: one stratum), generated from ``seed`` --
    or the explicit ``weights``, an integer ``(B, N)`` array in [0, 255] (how often each replicate
    counts each cell).  The passes run where ``rt`` runs.  ``chunk`` bounds the replicates of one
    launch (default: as many as keep a launch's counts and hours within 256 MiB); results do not
    depend on it."""

    def __init__(self, rt: RTMatrix, n_boot: int = 200, seed: int = 0, weights=None, chunk: Optional[int] = None):
        self.rt = rt
        self.L, self.N = rt.L, rt.N
        self.clones = rt.clones
        n_groups = len(rt.clones) + 1
        self._group = np.where(rt._clone_of >= 0, rt._clone_of, n_groups - 1).astype(np.int64)
        if chunk is not None and int(chunk) < 1:
            raise ValueError("chunk must be at least 1")
        self.chunk = None if chunk is None else int(chunk)
        self._w_dev = None
        self.ldw = -(-self.N // 256) * 256
        if weights is not None:
            w = np.asarray(weights)
            if w.ndim != 2 or w.shape[0] < 1 or w.shape[1] != self.N:
                raise ValueError("weights must be (replicates, {} cells), not {}".format(self.N, w.shape))
            if w.dtype.kind not in "biu":
                raise ValueError("weights must be integers")
            if w.dtype.kind != "b" and (int(w.min()) < 0 or int(w.max()) > 255):
                raise ValueError("weights must lie in [0, 255]")
            self.seed, self.weights = None, np.ascontiguousarray(w.astype(np.uint8))
        else:
            if int(n_boot) < 1:
                raise ValueError("n_boot must be at least 1")
            self.seed = int(seed)
            strata = self._group if len(rt.clones) else np.zeros(self.N, np.int64)
            if rt.device.type == "cuda":
                self.weights = self._device_weights(strata, int(n_boot))
            else:
                self.weights = boot_weights_host(strata, int(n_boot), self.seed)
        self.n_boot = int(self.weights.shape[0])
        if self.L * int(self.weights.sum(axis=1, dtype=np.int64).max()) >= 1 << 32:
            raise ValueError("bins x a replicate's total weight reaches 2^32: a 32-bit counter could wrap")
        self._counts = self._population = None

    def __len__(self):
        return self.n_boot

    # ---- device plumbing -----------------------------------------------------------------------

    def _device_weights(self, strata, n_boot):
        import torch
        from . import _native as nat
        rt = self.rt
        order, pos_lo, pos_n = stratum_layout(strata)
        with torch.cuda.device(rt.device):
            order_d, lo_d, n_d = (torch.as_tensor(a, device=rt.device) for a in (order, pos_lo, pos_n))
            w = torch.zeros((n_boot, self.ldw), dtype=torch.uint8, device=rt.device)
            flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
            step = min(nat.BOOT_MAX_LAUNCH, self.chunk or max(1, _BUDGET_BYTES // (4 * self.N)))
            for b0 in range(0, n_boot, step):
                bc = min(step, n_boot - b0)
                scratch = torch.zeros((bc, self.N), dtype=torch.int32, device=rt.device)
                nat.check(nat.lib().pert_boot_weights(
                    self.N, self.ldw, lo_d.data_ptr(), n_d.data_ptr(), order_d.data_ptr(),
                    self.seed & 0xFFFFFFFFFFFFFFFF, b0, bc, scratch.data_ptr(), w[b0:].data_ptr(), flag.data_ptr(),
                    rt._stream()), "pert_boot_weights")
            bits = int(flag.item())
            if bits & 2:
                raise RuntimeError("pert_boot_weights: the stratum layout is inconsistent")
            if bits & 1:
                raise OverflowError("a cell was drawn more than 255 times in one replicate")
            self._w_dev = w
            return w[:, :self.N].cpu().numpy()

    def _weights_on_device(self):
        import torch
        if self._w_dev is None:
            w = torch.zeros((self.n_boot, self.ldw), dtype=torch.uint8, device=self.rt.device)
            w[:, :self.N] = torch.from_numpy(self.weights)
            self._w_dev = w
        return self._w_dev

    def _chunk_of(self, n_groups: int) -> int:
        """Replicates per launch: count (uint32) and hours (at most fp64) [chunk][groups][L]."""
        if self.chunk is not None:
            return self.chunk
        return max(1, min(self.n_boot, _BUDGET_BYTES // (12 * n_groups * self.L)))

    def _device_counts(self, group, G):
        import torch
        from . import _native as nat
        rt = self.rt
        out = np.empty((self.n_boot, G, self.L), np.int64)
        with torch.cuda.device(rt.device):
            w = self._weights_on_device()
            member = torch.zeros((G, self.ldw), dtype=torch.uint8, device=rt.device)
            member[torch.as_tensor(group, device=rt.device), torch.arange(self.N, device=rt.device)] = 1
            step = self._chunk_of(G)
            for b0 in range(0, self.n_boot, step):
                wg = (w[b0:b0 + step, None, :] * member[None]).contiguous()          # [Bc][G][ldw], masked by group
                bc = wg.shape[0]
                count = torch.zeros((bc * G, self.L), dtype=torch.int32, device=rt.device)
                nat.check(nat.lib().pert_boot_counts(self.L, self.N, rt.ldn, rt._rep_dev.data_ptr(), bc * G, self.ldw,
                                                     wg.data_ptr(), count.data_ptr(), rt._stream()),
                          "pert_boot_counts")
                out[b0:b0 + bc] = count.cpu().numpy().view(np.uint32).reshape(bc, G, self.L)
        return out

    def _device_hist(self, group, hours_of, G, f10, edges):
        import torch
        from . import _native as nat
        rt = self.rt
        T, nb = f10.dtype, len(edges) - 1
        hist_n = np.zeros((self.n_boot, G, nb), np.int64)
        hist_rep = np.zeros((self.n_boot, G, nb), np.int64)
        with torch.cuda.device(rt.device):
            w = self._weights_on_device()
            f10_d = torch.as_tensor(f10, device=rt.device)
            edges_d = torch.as_tensor(edges, device=rt.device)
            # the kernel keeps a tile's hours rows of every group in LDS: launches of at most
            # RT_MAX_GROUPS groups each
            for g0 in range(0, G, nat.RT_MAX_GROUPS):
                gs = min(nat.RT_MAX_GROUPS, G - g0)
                sub = np.where((group >= g0) & (group < g0 + gs), group - g0, -1).astype(np.int32)
                grp = torch.as_tensor(sub, device=rt.device)
                step = self._chunk_of(gs)
                for b0 in range(0, self.n_boot, step):
                    hours = np.ascontiguousarray(hours_of(b0, min(b0 + step, self.n_boot))[:, g0:g0 + gs])
                    bc = hours.shape[0]
                    hours_d = torch.as_tensor(hours, device=rt.device)
                    hn = torch.zeros((bc, gs, nb), dtype=torch.int32, device=rt.device)
                    hr = torch.zeros((bc, gs, nb), dtype=torch.int32, device=rt.device)
                    nat.check(nat.lib().pert_boot_tfs_hist(
                        self.L, self.N, rt.ldn, gs, rt._rep_dev.data_ptr(), grp.data_ptr(), bc, self.ldw,
                        w[b0:].data_ptr(), hours_d.data_ptr(), f10_d.data_ptr(), edges_d.data_ptr(), len(edges),
                        int(T == np.float64), hn.data_ptr(), hr.data_ptr(), rt._stream()), "pert_boot_tfs_hist")
                    hist_n[b0:b0 + bc, g0:g0 + gs] = hn.cpu().numpy().view(np.uint32)
                    hist_rep[b0:b0 + bc, g0:g0 + gs] = hr.cpu().numpy().view(np.uint32)
        return hist_n, hist_rep

    # ---- the chunked numpy passes (same counts as the kernels) -----------------------------------

    def _host_counts(self, group, G):
        rep = self.rt._rep_host
        member = np.zeros((G, self.N), np.float64)
        member[group, np.arange(self.N)] = 1.0
        out = np.empty((self.n_boot, G, self.L), np.int64)
        step_b = self._chunk_of(G)
        for b0 in range(0, self.n_boot, step_b):
            wg = (self.weights[b0:b0 + step_b, None, :].astype(np.float64) * member[None]).reshape(-1, self.N)
            step = max(1, _CHUNK_ELEMS // self.N)
            for l0 in range(0, self.L, step):
                blk = rep[l0:l0 + step].astype(np.float64)                   # sums below 2^53: exact
                out[b0:b0 + step_b, :, l0:l0 + step] = np.rint(wg @ blk.T).astype(np.int64).reshape(-1, G, len(blk))
        return out

    def _host_hist(self, group, hours_of, G, f10, edges):
        rep, nb = self.rt._rep_host, len(edges) - 1
        hist_n = np.zeros((self.n_boot, G * nb), np.int64)
        hist_rep = np.zeros((self.n_boot, G * nb), np.int64)
        step_b = self._chunk_of(G)
        for b0 in range(0, self.n_boot, step_b):
            hours = hours_of(b0, min(b0 + step_b, self.n_boot))
            for b in range(b0, b0 + len(hours)):
                sel = np.flatnonzero((group >= 0) & (group < G) & (self.weights[b] > 0))
                if not len(sel):
                    continue
                wb = self.weights[b, sel].astype(np.float64)
                rows_of = hours[b - b0][group[sel]]                          # [cells][L]
                step = max(1, _CHUNK_ELEMS // len(sel))
                for l0 in range(0, self.L, step):
                    t = rows_of[:, l0:l0 + step].T - f10[sel][None, :]       # one subtraction in T
                    idx = np.searchsorted(edges, t.ravel(), side="right") - 1
                    ok = (idx >= 0) & (idx < nb) & ~np.isnan(t.ravel())
                    key = idx[ok] + np.broadcast_to(group[sel][None, :] * nb, t.shape).ravel()[ok]
                    wt = np.broadcast_to(wb[None, :], t.shape).ravel()[ok]
                    state = (rep[l0:l0 + step][:, sel] != 0).ravel()[ok]
                    hist_n[b] += np.rint(np.bincount(key, weights=wt, minlength=G * nb)).astype(np.int64)
                    hist_rep[b] += np.rint(np.bincount(key, weights=wt * state, minlength=G * nb)).astype(np.int64)
        return hist_n.reshape(-1, G, nb), hist_rep.reshape(-1, G, nb)

    # ---- results --------------------------------------------------------------------------------

    def _clone_counts(self):
        if self._counts is None:
            G = len(self.clones) + 1
            count = (self._device_counts if self.rt.device.type == "cuda" else self._host_counts)(self._group, G)
            member = np.zeros((self.N, G), np.int64)
            member[np.arange(self.N), self._group] = 1
            self._counts = (count, self.weights.astype(np.int64) @ member)
        return self._counts

    def counts(self, by='clone'):
        """(count int64 [B][G][L], size int64 [B][G]): the weighted number of replicated cells per
        bin and the total weight of each group in every replicate.  ``by='clone'``: the groups of
        ``RTMatrix.counts`` (sorted clone ids; the last collects the cells without a clone);
        ``by='population'``: one group.  One pass over the matrix, cached."""
        count, size = self._clone_counts()
        if by == 'clone':
            return count, size
        if by == 'population':
            if self._population is None:
                self._population = (count.sum(axis=1, keepdims=True), size.sum(axis=1, keepdims=True))
            return self._population
        raise ValueError("by must be 'population' or 'clone'")

    def profiles(self, by='clone', dtype=np.float32, rows=None):
        """(values, hours) ``[B][G][L]`` in the matrix's row order: every replicate's pseudobulk mean
        state per group (``size`` 0: NaN) and its 0-10 h scale, formed as ``RTMatrix.pseudobulk``
        forms them.  ``rows = (b0, b1)`` restricts the replicates."""
        count, size = self.counts(by)
        if rows is not None:
            count, size = count[rows[0]:rows[1]], size[rows[0]:rows[1]]
        values = _mean_from_sums(count, size[..., None], dtype)
        return values, _hours_from_profiles(values)

    def pseudobulk(self, q: Sequence[float] = DEFAULT_Q, dtype=np.float32) -> pd.DataFrame:
        """One row per locus, sorted by (chr, start), laid out as ``PosteriorDraws.pseudobulk``: the
        mean and the quantiles ``q`` over the replicates of the pseudobulk replicated fraction, for
        the population (``pseudobulk_mean``, ``pseudobulk_q<percent>``) and for each clone
        (``pseudobulk_clone<id>_...``), each with its standard deviation (``..._sd``)."""
        order = self.rt.locus_order
        chrom = self.rt.chr[order]
        out = {"chr": chrom.astype(object) if chrom.dtype.kind in "US" else chrom, "start": self.rt.start[order]}

        def add(values, prefix):
            out.update(_summary(values, q, prefix))
            out[prefix + "_sd"] = _sd(values)

        add(self.profiles('population', dtype)[0][:, 0][:, order], "pseudobulk")
        if len(self.clones):
            per_clone = self.profiles('clone', dtype)[0]
            for k, c in enumerate(self.clones):
                add(per_clone[:, k][:, order], "pseudobulk_clone{}".format(c))
        return pd.DataFrame(out)

    def tfs_counts(self, by='population', cells=None, loci=None, dtype=np.float32, frac_dtype=None):
        """(hist_n, hist_rep), int64 ``[B][G][200]``: ``RTMatrix.tfs_counts`` of every replicate, per
        group (``by='population'``: G = 1; ``by='clone'``: one per clone, the cells without a clone
        left out as there).  Hours are the replicate's own; a cell's replicated fraction is its own
        in the unweighted matrix.  ``cells`` / ``loci`` / ``dtype`` / ``frac_dtype`` as there."""
        rt = self.rt
        frac_dtype = dtype if frac_dtype is None else frac_dtype
        T = np.dtype(_tfs_dtype(dtype, frac_dtype))
        if by == 'population':
            G, group = 1, np.zeros(self.N, np.int64)
        elif by == 'clone':
            if not len(self.clones):
                raise ValueError("by='clone' needs clone_ids")
            G, group = len(self.clones), rt._clone_of.copy()
        else:
            raise ValueError("by must be 'population' or 'clone'")
        keep = None
        if loci is not None:                                               # bins left out count nowhere
            keep = np.zeros(self.L, bool)
            keep[np.asarray(loci)] = True
        if cells is not None:
            group = np.where(np.isin(rt.cell_ids, np.asarray(cells)), group, -1)

        def hours_of(b0, b1):
            hours = self.profiles(by, dtype, rows=(b0, b1))[1][:, :G].astype(T)
            if keep is not None:
                hours[..., ~keep] = np.nan
            return hours

        f10 = (rt.cell_fractions(frac_dtype, state_dtype=dtype) * 10.0).astype(T)
        edges = interval_edges().astype(T)
        return (self._device_hist if rt.device.type == "cuda" else self._host_hist)(group, hours_of, G, f10, edges)

    def twidth(self, curve='sigmoid', by='population', per_clone=False, **kw) -> pd.DataFrame:
        """One row per replicate -- or, with ``per_clone``, per (replicate, clone), each clone's own
        profile giving its hours: ``t_width``, ``right_time``, ``left_time`` and the fit parameters
        ``popt_0`` ... of ``twidth_from_points`` on that replicate's histogram (``**kw``:
        ``tfs_counts``' restrictions and dtypes)."""
        hist_n, hist_rep = self.tfs_counts(by='clone' if per_clone else by, **kw)
        if not per_clone:
            hist_n, hist_rep = hist_n.sum(axis=1, keepdims=True), hist_rep.sum(axis=1, keepdims=True)
        left = interval_edges()[:-1]
        rows = []
        for b in range(self.n_boot):
            for g in range(hist_n.shape[1]):
                t_width, right_time, left_time, popt, _, _ = twidth_from_points(
                    *_lists_from_hist(hist_n[b, g], hist_rep[b, g], left), curve=curve)
                row = {"replicate": b}
                if per_clone:
                    row["clone_id"] = self.clones[g]
                row.update({"t_width": float(t_width), "right_time": float(right_time),
                            "left_time": float(left_time)})
                row.update({"popt_{}".format(i): float(v) for i, v in enumerate(popt)})
                rows.append(row)
        return pd.DataFrame(rows)

    def twidth_interval(self, q: Sequence[float] = DEFAULT_Q, curve='sigmoid', by='population', per_clone=False,
                        **kw) -> pd.DataFrame:
        """One row -- or one per clone with ``per_clone``: ``t_width`` of the unweighted matrix
        next to the mean, the quantiles ``q`` and the standard deviation of ``t_width`` over the
        replicates (``t_width_mean``, ``t_width_q<percent>``, ``t_width_sd``)."""
        tw = self.twidth(curve=curve, by=by, per_clone=per_clone, **kw)
        rows = []
        for c in (self.clones if per_clone else [None]):
            if per_clone:
                user_cells = kw.get("cells")
                ids = self.rt.cell_ids[self.rt.clone_ids == c]
                ids = ids if user_cells is None else ids[np.isin(ids, np.asarray(user_cells))]
                own = self.rt.twidth(curve=curve, by='clone', **dict(kw, cells=ids))[0]
                values = tw.loc[tw["clone_id"] == c, "t_width"].to_numpy()
                row = {"clone_id": c}
            else:
                own = self.rt.twidth(curve=curve, by=by, **kw)[0]
                values, row = tw["t_width"].to_numpy(), {}
            row["t_width"] = float(own)
            row.update({k: float(v) for k, v in _summary(values, q, "t_width").items()})
            row["t_width_sd"] = float(_sd(values))
            rows.append(row)
        return pd.DataFrame(rows)
