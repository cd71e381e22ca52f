"""Distributions of the replication-timing statistics over posterior draws of the states.

``PertShard.draw_states`` (pert_enum_draw) gives whole-matrix realisations of the (cn, rep) states
from the posterior the decode is the argmax of.  ``PosteriorDraws`` holds those planes with the
labels of the S-phase output and turns them into what a user reads: the replicated fraction of
each cell, the pseudobulk profiles and the T-width, each with its spread over the draws.  Every
statistic goes through ``RTMatrix`` over one plane in place (the integer-count kernels on the GPU,
the chunked numpy passes on the host); the long table is never formed.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import pandas as pd

from .rt_profiles import RTMatrix

DEFAULT_Q = (0.05, 0.5, 0.95)


def _q_name(q: float) -> str:
    return "q{:g}".format(100.0 * q).replace(".", "_")


def _summary(a: np.ndarray, q: Sequence[float], prefix: str) -> dict:
    """Mean and quantiles over axis 0 (the draws) of ``a``, in float64."""
    a = np.asarray(a, np.float64)
    out = {prefix + "_mean": a.mean(axis=0)}
    if len(q):
        qs = np.quantile(a, np.asarray(q, np.float64), axis=0)
        for qi, v in zip(q, qs):
            out["{}_{}".format(prefix, _q_name(qi))] = v
    return out


class PosteriorDraws:
    """``rep`` (and optionally ``cn``): ``(n_draws, L, N)`` uint8 planes, numpy arrays or torch
    tensors on any device (``draw_states``' result: used in place, each plane a ``(L, N)`` view
    whose rows are ``ldn`` apart).  ``cell_ids [N]``, ``chr [L]``, ``start [L]`` and ``clone_ids [N]``
    (optional) label them as they label an ``RTMatrix``.  ``device`` is passed on to ``RTMatrix``.
    ``reads`` (optional): the cells' ``(L, N)`` float32 / float64 read depth, which ``phase_table``
    needs beside the ``cn`` planes."""

    def __init__(self, rep, cell_ids, chr, start, clone_ids=None, cn=None, device: Optional[str] = None, reads=None):
        if len(rep.shape) != 3 or rep.shape[0] < 1:
            raise ValueError("rep must be (n_draws, bins, cells) planes")
        if cn is not None and tuple(cn.shape) != tuple(rep.shape):
            raise ValueError("cn planes do not match rep's shape {}".format(tuple(rep.shape)))
        if reads is not None and tuple(reads.shape) != tuple(rep.shape[1:]):
            raise ValueError("reads do not match the planes' shape {}".format(tuple(rep.shape[1:])))
        self.rep, self.cn, self.reads = rep, cn, reads
        self.n_draws, self.L, self.N = (int(v) for v in rep.shape)
        self.cell_ids = np.asarray(cell_ids)
        self.chr, self.start = np.asarray(chr), np.asarray(start)
        self.clone_ids = None if clone_ids is None else np.asarray(clone_ids)
        self.device = device
        self._mats = {}
        self.rt_matrix(0)                       # checks the labels against the planes

    def __len__(self):
        return self.n_draws

    def rt_matrix(self, d: int) -> RTMatrix:
        """The ``RTMatrix`` of draw ``d`` over that plane in place (its counts are cached)."""
        d = int(d)
        if not 0 <= d < self.n_draws:
            raise IndexError("draw {} of {}".format(d, self.n_draws))
        if d not in self._mats:
            self._mats[d] = RTMatrix(self.rep[d], self.cell_ids, self.chr, self.start, clone_ids=self.clone_ids,
                                     device=self.device)
        return self._mats[d]

    def frac_rt(self, dtype=np.float32) -> np.ndarray:
        """``(n_draws, N)``: the replicated fraction of every cell in every draw
        (``RTMatrix.cell_fractions``)."""
        return np.stack([self.rt_matrix(d).cell_fractions(dtype) for d in range(self.n_draws)])

    def cell_table(self, q: Sequence[float] = DEFAULT_Q, cell_col="cell_id") -> pd.DataFrame:
        """One row per cell (in ``cell_ids`` order): the mean and the quantiles ``q`` of its
        replicated fraction over the draws, columns ``frac_rt_mean`` and ``frac_rt_q<percent>``."""
        out = {cell_col: self.cell_ids}
        if self.clone_ids is not None:
            out["clone_id"] = self.clone_ids
        out.update(_summary(self.frac_rt(), q, "frac_rt"))
        return pd.DataFrame(out)

    def pseudobulk(self, q: Sequence[float] = DEFAULT_Q, dtype=np.float32) -> pd.DataFrame:
        """One row per locus, sorted by (chr, start): the mean and quantiles over the draws of the
        pseudobulk replicated fraction (``RTMatrix.pseudobulk``), for the population (columns
        ``pseudobulk_mean``, ``pseudobulk_q<percent>``) and, when clones are known, for each clone
        (``pseudobulk_clone<id>_...``)."""
        pbs = [self.rt_matrix(d).pseudobulk(dtype) for d in range(self.n_draws)]
        chrom = pbs[0]["chr"]
        out = {"chr": chrom.astype(object) if chrom.dtype.kind in "US" else chrom, "start": pbs[0]["start"]}
        out.update(_summary(np.stack([p["population"][0] for p in pbs]), q, "pseudobulk"))
        for c in pbs[0]["clones"]:
            out.update(_summary(np.stack([p["clones"][c][0] for p in pbs]), q, "pseudobulk_clone{}".format(c)))
        return pd.DataFrame(out)

    def twidth(self, curve='sigmoid', **kw) -> pd.DataFrame:
        """One row per draw: ``RTMatrix.twidth(curve, **kw)`` of that draw -- ``t_width``,
        ``right_time``, ``left_time`` and the fit parameters ``popt_0`` ..."""
        rows = []
        for d in range(self.n_draws):
            t_width, right_time, left_time, popt, _, _ = self.rt_matrix(d).twidth(curve=curve, **kw)
            row = {"draw": d, "t_width": float(t_width), "right_time": float(right_time),
                   "left_time": float(left_time)}
            row.update({"popt_{}".format(i): float(v) for i, v in enumerate(popt)})
            rows.append(row)
        return pd.DataFrame(rows)

    def phase_table(self, q: Sequence[float] = DEFAULT_Q, cell_col="cell_id", frac_thresh=0.05, rep_auto_thresh=0.2,
                    frac_cn0_thresh=0.05) -> pd.DataFrame:
        """One row per cell (in ``cell_ids`` order): the share of draws in which ``phase_calls`` calls
        it S / G1/2 / LQ (``share_S``, ``share_G1/2``, ``share_LQ``), the mean and the quantiles ``q``
        over the draws of ``rep_auto`` and ``cell_frac_rep`` (NaN-propagating: a draw in which the
        cell's states are constant has no ``rep_auto``), and ``rpm_auto``, which no draw changes.
        Needs the ``cn`` planes and ``reads``.  One pert_phase_counts launch over all planes and one
        pert_phase_acf call (phase_matrix.py)."""
        from . import phase_matrix as pm
        if self.cn is None or self.reads is None:
            raise ValueError("phase_table needs the cn planes and reads")
        counts = pm.counts_of_planes(self.rep, self.cn, pm.MAX_LAG, device=self.device)
        num, den = pm.rep_auto_rational(counts, self.L, pm.MIN_LAG, pm.MAX_LAG)
        frac = counts["T"] / float(self.L)
        phase = pm.call_phases(frac, pm.rep_auto_exceeds(num, den, rep_auto_thresh), counts["cn0"] / float(self.L),
                               frac_thresh, frac_cn0_thresh)
        out = {cell_col: self.cell_ids}
        for name in ('S', 'G1/2', 'LQ'):
            out["share_" + name] = (phase == name).mean(axis=0)
        with np.errstate(invalid="ignore"):
            out.update(_summary(pm._ratio(num, den), q, "rep_auto"))
        out.update(_summary(frac, q, "cell_frac_rep"))
        out["rpm_auto"] = pm.reads_auto(self.reads, device=self.device)
        return pd.DataFrame(out)
