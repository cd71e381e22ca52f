"""Read-count simulator: the PERT generative model run forwards on the GPU.

Reference: ``scdna_replication_tools/pert_simulator.py`` -- ``pert_simulator`` (:285-418),
``simulate_s_cells`` (:201-249), ``simulate_g_cells`` (:252-282), ``convert_rt_units``
(:177-179), ``get_libraries_tensor`` (:182-198), with the same names, positional arguments,
defaults and return values.  The reference conditions its Pyro models ``model_s`` / ``model_g1``
on lambda, u, a, rho and the beta means and traces one sample of the rest; the same draws are
made here by the HIP kernels of csrc/sim_kernels.hip (``pert_sim_cells``, ``pert_sim_reads``,
``pert_sim_normalise``; there is no CPU sampler):

  per cell         tau ~ U(0, 1), betas ~ Normal(beta_means[lib], beta_stds[lib])
  per (bin, cell)  rep ~ Bernoulli(1 / (1 + exp(-a (tau - rho)))), chi = cn (1 + rep),
                   delta = max(u chi exp(sum_k beta_k gc^(K-k)) (1 - lamb) / lamb, 1),
                   reads ~ NegativeBinomial(delta, probs=lamb)
  then             reads_norm = int64(reads / sum(reads) * num_reads)

The random numbers are Philox4x32-10 words addressed by (seed, bin, global cell, draw round)
(include/pert_hip.h), not torch's or Pyro's stream: a run reproduces from its seed, and
parity with the reference is in distribution, not draw for draw.  ``seed=None`` takes the
seed from torch's global generator, so ``torch.manual_seed(s)`` before a call reproduces it
as it does with the reference.  Cells are numbered globally -- the S cells clone by clone in
``clones`` order, then the G1/2 cells -- so no two cells of a call share random numbers.

The output frames are built by index gather from the simulated matrices
(``assemble_frames``), not by the reference's melt / merge rounds; rows, row order, columns,
column order and dtypes are the reference's.

One deliberate deviation.  The reference takes ``gc`` and ``rt`` in order of first appearance
(``drop_duplicates``, :331 / :348) but the CN matrix in ``pivot_table`` order (chromosome as a
string, then start).  For a table with several chromosomes in natural order the two
disagree, and the reference simulates with gc and rho attached to the wrong loci.  Here both
are looked up per locus of the pivot.  On single-chromosome tables (the tutorial, the
reference's test) and on string-sorted tables the two coincide.  (``simulate_s_cells`` /
``simulate_g_cells`` take the profiles as given, row i for locus i of ``cn``, like the
reference's.)
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import pandas as pd

BLOCK = 256
MAX_NUM_READS = 1 << 24


# ----------------------------------------------------------------------------------------------
# the reference's helpers
# ----------------------------------------------------------------------------------------------

def convert_rt_units(rt):
    """pert_simulator.py:177-179: RT on 0-1 with the largest values the latest times."""
    return 1 - ((rt - rt.min()) / (rt.max() - rt.min()))


def _library_codes(cn: pd.DataFrame):
    libs = cn[['cell_id', 'library_id']].drop_duplicates()
    codes, uniques = pd.factorize(libs['library_id'])           # order of first appearance
    return np.asarray(codes, np.int64), int(len(uniques))


def get_libraries_tensor(cn):
    """pert_simulator.py:182-198: the library index of each (cell_id, library_id) pair in order
    of first appearance, as an int64 tensor, and the number of libraries."""
    import torch
    codes, n_libs = _library_codes(cn)
    return torch.from_numpy(codes), n_libs


# ----------------------------------------------------------------------------------------------
# device layer
# ----------------------------------------------------------------------------------------------

@dataclass
class SimMatrix:
    """One simulated (bins x cells) matrix, on the device.  Row stride ``ldn`` = N rounded up to
    256 as in ``pert_problem``; columns [N, ldn) are zero."""
    L: int
    N: int
    ldn: int
    counts: "object"                  # int32 [L][ldn] holding uint32 raw counts
    rep: "object"                     # uint8 [L][ldn]
    p_rep: "object"                   # float32 [L][ldn] or None
    colsum: "object"                  # int64 [N] exact column sums of counts
    tau: "object"                     # float32 [N] or None (G1/2)
    betas: "object"                   # float32 [K1][N]
    reads_norm: "object"              # float32 [L][ldn] or None: pert_problem.reads' layout
    exhausted: int                    # lanes that used up a sampler's rounds (expected 0)
    seed: int
    cell0: int

    def raw(self) -> np.ndarray:
        """uint32 [L][N] on the host."""
        return self.counts[:, :self.N].cpu().numpy().view(np.uint32)


def default_beta_stds(K1: int) -> np.ndarray:
    """The reference's expose_beta_stds: logspace(0, -K, K + 1) (pert_simulator.py:53)."""
    return np.logspace(0, -(K1 - 1), K1)


def _per_library(values, n_libs: int, K1: int, name: str) -> np.ndarray:
    v = np.asarray(values, np.float64)
    if v.ndim == 1:
        v = np.broadcast_to(v.reshape(1, -1), (n_libs, v.shape[0]))
    if v.shape != (n_libs, K1):
        raise ValueError("{} must have shape ({},) or ({}, {}), got {}".format(name, K1, n_libs, K1, v.shape))
    return np.ascontiguousarray(v, np.float32)


def new_seed() -> int:
    """A seed from torch's global generator (follows torch.manual_seed; advances it)."""
    import torch
    return int(torch.randint(0, (1 << 63) - 1, (1,), dtype=torch.int64).item())


def simulate_matrix(cn, gc, libs, n_libs: int, betas: Sequence[float], u: float, lamb: float, seed: int,
                    rho=None, a: float = 0.0, num_reads: Optional[float] = None, beta_stds=None, cell0: int = 0,
                    want_p_rep: bool = True, device=None) -> SimMatrix:
    """Simulate the (L, N) matrix of global cells [cell0, cell0 + N) on the GPU.  ``cn`` (L, N)
    array or device tensor, ``gc`` (L,), ``libs`` (N,) library indices, ``betas`` the K + 1
    beta means shared by the libraries, ``rho`` (L,) for S-phase cells or None for the G1/2
    model.  ``num_reads`` given: also the normalised counts (``reads_norm``)."""
    import torch
    from . import _native as nat
    lib = nat.lib()                                           # raises if the extension is not built
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError("the simulator runs on the GPU (device={!r}); there is no CPU sampler".format(device))
    L, N = int(cn.shape[0]), int(cn.shape[1])
    K1 = len(betas)
    if L < 1 or N < 1:
        raise ValueError("empty CN matrix {}".format((L, N)))
    if not 1 <= K1 <= nat.MAX_K1:
        raise ValueError("betas needs 1 to {} coefficients".format(nat.MAX_K1))
    if num_reads is not None and not 0 <= float(num_reads) < MAX_NUM_READS:
        raise ValueError("num_reads must be below 2^24 (the fp32 matrix of normalised counts is exact up to there)")
    means = _per_library(np.asarray(betas, np.float64), n_libs, K1, "betas")
    stds = _per_library(default_beta_stds(K1) if beta_stds is None else beta_stds, n_libs, K1, "beta_stds")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ldn = -(-N // BLOCK) * BLOCK
    s_mode = rho is not None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        f32 = lambda x: torch.as_tensor(np.ascontiguousarray(x, np.float32), device=dev)
        cn_d = torch.zeros((L, ldn), dtype=torch.float32, device=dev)
        cn_d[:, :N] = cn.to(dev, torch.float32) if torch.is_tensor(cn) else f32(cn)
        gc_d = f32(np.asarray(gc, np.float64).reshape(-1))
        rho_d = f32(np.asarray(rho, np.float64).reshape(-1)) if s_mode else None
        if gc_d.numel() != L or (s_mode and rho_d.numel() != L):
            raise ValueError("gc and rho need one value per locus ({})".format(L))
        libs_d = torch.as_tensor(np.ascontiguousarray(np.asarray(libs).reshape(-1), np.int32), device=dev)
        if libs_d.numel() != N:
            raise ValueError("libs needs one entry per cell ({})".format(N))
        means_d, stds_d = f32(means), f32(stds)
        tau = torch.empty(N, dtype=torch.float32, device=dev) if s_mode else None
        betas_d = torch.empty((K1, N), dtype=torch.float32, device=dev)
        counts = torch.empty((L, ldn), dtype=torch.int32, device=dev)
        rep = torch.empty((L, ldn), dtype=torch.uint8, device=dev)
        p_rep = torch.empty((L, ldn), dtype=torch.float32, device=dev) if (want_p_rep and s_mode) else None
        colsum = torch.zeros(N, dtype=torch.int64, device=dev)
        exhausted = torch.zeros(1, dtype=torch.int32, device=dev)
        ptr = lambda t: 0 if t is None else t.data_ptr()
        nat.check(lib.pert_sim_cells(N, K1, n_libs, int(cell0), ctypes.c_uint64(seed), ptr(libs_d), ptr(means_d),
                                     ptr(stds_d), ptr(tau), ptr(betas_d), stream), "pert_sim_cells")
        nat.check(lib.pert_sim_reads(L, N, ldn, K1, int(cell0), ctypes.c_uint64(seed), ptr(cn_d), ptr(gc_d),
                                     ptr(rho_d), ptr(tau), ptr(betas_d), float(u), float(a), float(lamb),
                                     ptr(counts), ptr(rep), ptr(p_rep), ptr(colsum), ptr(exhausted), stream),
                  "pert_sim_reads")
        reads_norm = None
        if num_reads is not None:
            reads_norm = torch.empty((L, ldn), dtype=torch.float32, device=dev)
            nat.check(lib.pert_sim_normalise(L, N, ldn, float(num_reads), ptr(counts), ptr(colsum),
                                             ptr(reads_norm), stream), "pert_sim_normalise")
        n_exhausted = int(exhausted.item())                   # synchronises: the inputs above stay alive
    return SimMatrix(L=L, N=N, ldn=ldn, counts=counts, rep=rep, p_rep=p_rep, colsum=colsum, tau=tau,
                     betas=betas_d, reads_norm=reads_norm, exhausted=n_exhausted, seed=seed, cell0=int(cell0))


def _sample(cn, gc, libs, n_libs, betas, u, lamb, seed, rho, a, num_reads, beta_stds, cell0, device):
    """Host view of one simulated matrix, in the reference's dtypes: (reads_norm int64, reads
    float64, rep float64, p_rep float64, t float32) as numpy arrays (rep, p_rep, t None for G1/2).
    The one place the frame layer touches the device."""
    m = simulate_matrix(cn, gc, libs, n_libs, betas, u, lamb, seed, rho=rho, a=a, num_reads=num_reads,
                        beta_stds=beta_stds, cell0=cell0, device=device)
    reads = m.raw().astype(np.float64)
    reads_norm = m.reads_norm[:, :m.N].cpu().numpy().astype(np.int64)
    if rho is None:
        return reads_norm, reads, None, None, None
    return (reads_norm, reads, m.rep[:, :m.N].cpu().numpy().astype(np.float64),
            m.p_rep[:, :m.N].cpu().numpy().astype(np.float64), m.tau.cpu().numpy())


def simulate_s_cells(gc_profile, libs, cn, rt, L_val, num_reads, lamb, betas, a, *, seed=None, beta_stds=None,
                     device=None, cell0=0):
    """pert_simulator.py:201-249: (reads_norm, reads, rep, p_rep, t) as CPU tensors."""
    import torch
    cn_v = np.asarray(getattr(cn, "values", cn), np.float64)
    num_loci = cn_v.shape[0]
    rho = convert_rt_units(np.asarray(getattr(rt, "values", rt), np.float64))
    u_guess = float(num_reads) / (1.5 * num_loci * float(np.mean(cn_v)))
    out = _sample(cn_v, np.asarray(getattr(gc_profile, "values", gc_profile), np.float64), np.asarray(libs),
                  int(L_val), betas, u_guess, lamb, new_seed() if seed is None else seed, rho, a, num_reads,
                  beta_stds, cell0, device)
    return tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in out)


def simulate_g_cells(gc_profile, libs, cn, L_val, num_reads, lamb, betas, *, seed=None, beta_stds=None,
                     device=None, cell0=0):
    """pert_simulator.py:252-282: (reads_norm, reads) as CPU tensors."""
    import torch
    cn_v = np.asarray(getattr(cn, "values", cn), np.float64)
    u_guess = float(num_reads) / (1. * cn_v.shape[0] * float(np.mean(cn_v)))
    out = _sample(cn_v, np.asarray(getattr(gc_profile, "values", gc_profile), np.float64), np.asarray(libs),
                  int(L_val), betas, u_guess, lamb, new_seed() if seed is None else seed, None, 0.0, num_reads,
                  beta_stds, cell0, device)
    return tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in out[:2])


# ----------------------------------------------------------------------------------------------
# frame layer
# ----------------------------------------------------------------------------------------------

@dataclass
class Pivot:
    """``pd.pivot_table(df, index=['chr', 'start'], columns='cell_id', values=col)`` as arrays:
    loci sorted by (chr as a string, start), cells sorted by id, plus each table row's position."""
    chr: np.ndarray                   # (L,) str
    start: np.ndarray                 # (L,)
    cells: np.ndarray                 # (N,)
    values: np.ndarray                # (L, N) float64, NaN where the table has no row
    li: np.ndarray                    # (rows,) locus of each table row
    ci: np.ndarray                    # (rows,) cell of each table row
    first_row: np.ndarray             # (L,) the first table row of each locus

    def per_locus(self, column) -> np.ndarray:
        """A per-locus column of the table (gc, rt) in the pivot's locus order."""
        return np.asarray(column)[self.first_row]


def pivot(df: pd.DataFrame, value_col: str) -> Pivot:
    c_codes, c_uni = pd.factorize(df['chr'].astype(str), sort=True)
    s_codes, s_uni = pd.factorize(df['start'], sort=True)
    n_codes, n_uni = pd.factorize(df['cell_id'], sort=True)
    if (c_codes < 0).any() or (s_codes < 0).any() or (n_codes < 0).any():
        raise ValueError("missing chr, start or cell_id values")
    key = c_codes.astype(np.int64) * max(len(s_uni), 1) + s_codes
    uni, first_row, li = np.unique(key, return_index=True, return_inverse=True)
    L, N = len(uni), len(n_uni)
    flat = li.astype(np.int64) * N + n_codes
    v = df[value_col].to_numpy(np.float64)
    ok = ~np.isnan(v)
    cnt = np.bincount(flat[ok], minlength=L * N)
    with np.errstate(invalid="ignore", divide="ignore"):
        values = np.bincount(flat[ok], weights=v[ok], minlength=L * N) / cnt        # the mean, as pivot_table
    return Pivot(chr=np.asarray(c_uni).astype(str)[uni // max(len(s_uni), 1)],
                 start=np.asarray(s_uni)[uni % max(len(s_uni), 1)], cells=np.asarray(n_uni),
                 values=values.reshape(L, N), li=li, ci=n_codes, first_row=first_row)


def _locus_table(df: pd.DataFrame, col: str):
    """(chr, start) -> the first value of ``col`` at that locus in ``df``."""
    index = pd.MultiIndex.from_arrays([df['chr'].astype(str).to_numpy(), df['start'].to_numpy()])
    first = ~index.duplicated()
    return index[first], df[col].to_numpy(np.float64)[first]


def _at_loci(table, pv: Pivot, what: str) -> np.ndarray:
    index, values = table
    at = index.get_indexer(pd.MultiIndex.from_arrays([pv.chr, pv.start]))
    if (at < 0).any():
        raise ValueError("{}: loci without a value in the S-phase table".format(what))
    return values[at]


def assemble_frames(df_s, df_g, clones, s_parts, g_part, input_cn_col='true_somatic_cn', pivots=None):
    """The output frames of pert_simulator.py:336-418 from the simulated matrices.
    ``s_parts[i]``: (reads_norm, reads, rep, p_rep, t) of clone ``clones[i]`` as arrays in that
    clone's pivot order (``pivot(clone rows)``: loci x cells, t per cell); ``g_part``:
    (reads_norm, reads) in the pivot order of ``df_g``.  ``chr`` must already be a string column.
    ``pivots``: (the clones' Pivots, df_g's Pivot) where the caller has them already."""
    out = []
    for i, (clone_id, part) in enumerate(zip(clones, s_parts)):
        clone_df = df_s.loc[(df_s['clone_id'] == str(clone_id)).to_numpy()]
        pv = pivot(clone_df, input_cn_col) if pivots is None else pivots[0][i]
        reads_norm, reads, rep, p_rep, t = (np.asarray(x) for x in part)
        frame = clone_df.copy(deep=False)
        frame.index = pd.RangeIndex(len(frame))
        frame['true_reads_norm'] = reads_norm[pv.li, pv.ci].astype(np.int64)
        frame['true_reads_raw'] = reads[pv.li, pv.ci].astype(np.float64)
        frame['true_rep'] = rep[pv.li, pv.ci].astype(np.float64)
        frame['true_p_rep'] = p_rep[pv.li, pv.ci].astype(np.float64)
        frame['true_t'] = t.reshape(-1)[pv.ci]
        out.append(frame)
    df_s_out = pd.concat(out, ignore_index=True)

    pv = pivot(df_g, input_cn_col) if pivots is None else pivots[1]
    reads_norm, reads = (np.asarray(x) for x in g_part)
    df_g_out = df_g.copy(deep=False)
    df_g_out.index = pd.RangeIndex(len(df_g_out))
    df_g_out['true_reads_norm'] = reads_norm[pv.li, pv.ci].astype(np.int64)
    df_g_out['true_reads_raw'] = reads[pv.li, pv.ci].astype(np.float64)
    df_g_out['true_t'] = 0.0
    df_g_out['true_rep'] = 0.0
    df_g_out['true_p_rep'] = 0.0
    df_s_out['true_total_cn'] = df_s_out[input_cn_col] * (df_s_out['true_rep'] + 1)
    df_g_out['true_total_cn'] = df_g_out[input_cn_col] * (df_g_out['true_rep'] + 1)
    return df_s_out, df_g_out


def _complete(pv: Pivot, what: str):
    if np.isnan(pv.values).any():
        raise ValueError("{}: every cell needs a copy number at every locus".format(what))


def pert_simulator(df_s, df_g, num_reads, rt_cols, clones, lamb, betas, a, gc_col='gc',
                   input_cn_col='true_somatic_cn', *, seed=None, beta_stds=None, device=None):
    """Simulate S-phase and G1/2-phase read counts for cells with known copy number
    (pert_simulator.py:285-418; the parameters are the reference's).  Returns (df_s, df_g) with
    ``true_reads_norm``, ``true_reads_raw``, ``true_rep``, ``true_p_rep``, ``true_t`` and
    ``true_total_cn`` added; S-phase cells of clones not in ``clones`` are dropped.

    ``seed``: None takes one from torch's global generator (``torch.manual_seed`` reproduces a
    run); an integer is used as given.  ``beta_stds``: the spread of each cell's GC coefficients
    around ``betas``; None is the reference's ``logspace(0, -K, K + 1)``, zeros give every cell
    exactly ``betas``.  ``device``: the GPU to run on (default the current one)."""
    df_s.chr = df_s.chr.astype(str)
    df_g.chr = df_g.chr.astype(str)
    assert len(rt_cols) == len(clones)
    seed = new_seed() if seed is None else int(seed)

    gc_table = _locus_table(df_s, gc_col)         # one gc profile for all cells, as the reference's (:331)
    cell0 = 0
    s_parts, s_pivots = [], []
    for rt_col, clone_id in zip(rt_cols, clones):
        clone_df = df_s.loc[(df_s['clone_id'] == str(clone_id)).to_numpy()]
        if len(clone_df) == 0:
            raise ValueError("no S-phase cells of clone {!r}".format(clone_id))
        libs, n_libs = _library_codes(clone_df)
        pv = pivot(clone_df, input_cn_col)
        _complete(pv, "S-phase cells of clone {!r}".format(clone_id))
        L, N = pv.values.shape
        rho = convert_rt_units(pv.per_locus(clone_df[rt_col].to_numpy(np.float64)))
        u = float(num_reads) / (1.5 * L * float(np.mean(pv.values)))
        s_parts.append(_sample(pv.values, _at_loci(gc_table, pv, gc_col), libs, n_libs, betas, u, lamb, seed, rho, a,
                               num_reads, beta_stds, cell0, device))
        s_pivots.append(pv)
        cell0 += N

    libs, n_libs = _library_codes(df_g)
    pv = pivot(df_g, input_cn_col)
    _complete(pv, "G1/2-phase cells")
    L, N = pv.values.shape
    u = float(num_reads) / (1. * L * float(np.mean(pv.values)))
    g_part = _sample(pv.values, _at_loci(gc_table, pv, gc_col), libs, n_libs, betas, u, lamb, seed, None, 0.0,
                     num_reads, beta_stds, cell0, device)[:2]
    return assemble_frames(df_s, df_g, clones, s_parts, g_part, input_cn_col, pivots=(s_pivots, pv))
