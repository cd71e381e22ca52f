"""Time of the threshold binarisation (binarize.py): the pert_rt_binarize launch, binarize_matrix
end to end, the host path per flagged cell, the CPU tensor program and the per-cell sklearn loop;
and the launch of the kernel it shares its stages with, pert_tau_binarize (tau_init.py).

    python tools/binarize_timing.py [--shapes small,genome] [--out profiles/binarize_timing.jsonl]

One process.  Per shape (bins x cells of simulated S-phase reads over the G1/2 pseudobulk median,
float64): the kernel timed with device events (3 warm-up launches, 10 timed ones into the same buffers, median and min),
``binarize_matrix(device='cuda')`` once from a host array (upload, launch, download, host path),
the share of cells the kernel flags and which bits, ``exact_cell`` on a slice of up to 16 cells
(the host path's cost per flagged cell, flagged or not), the CPU tensor program on the same input
and the reference-style per-cell loop on a 64-cell slice; then pert_tau_binarize timed the same way
on fp32 simulated reads of the same shape.  Prints one JSON line per measurement."""
import argparse
import ctypes
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scdna_replication_tools_amd import _native as nat        # noqa: E402
from scdna_replication_tools_amd import binarize as B           # noqa: E402
from scdna_replication_tools_amd import simulator               # noqa: E402
from scdna_replication_tools_amd import tau_init                # noqa: E402

SHAPES = {"small": (271, 400), "genome": (5451, 2000), "tiny": (96, 32)}
WARMUP, REPS = 3, 10
SLICE = 64


def profiles(L, N, seed=0):
    sim = simulator.simulate(N, min(N, 256), n_bins=L, seed=seed)
    return sim.reads_s.astype(np.float64) / np.median(sim.reads_g.astype(np.float64), axis=1)[:, None]


def launch_ms(launch):
    """The device-event times (ms) of REPS calls of launch() after WARMUP untimed ones."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for i in range(WARMUP + REPS):
        if i >= WARMUP:
            ev[i - WARMUP][0].record()
        launch()
        if i >= WARMUP:
            ev[i - WARMUP][1].record()
    torch.cuda.synchronize()
    return np.array([s.elapsed_time(e) for s, e in ev])


def tau_launch(L, N, seed=0):
    """A closure that launches pert_tau_binarize on tau_init.binarize_native's inputs (fp32
    simulated reads, one row per cell) into buffers allocated once."""
    sim = simulator.simulate(N, 1, n_bins=L, seed=seed)
    norm = torch.from_numpy(sim.reads_s.astype(np.float32)).cuda().T.contiguous()
    bufs = [torch.empty(shape, dtype=dt, device="cuda") for shape, dt in
            (((2, N, L), torch.int8), ((2, N, L), torch.int8), ((2, N, 2), torch.float64), ((2, N), torch.int32),
             ((2, N), torch.float64), ((2, N), torch.float64))]
    p = tau_init.tau_params(L)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: nat.check(nat.lib().pert_tau_binarize(L, N, norm.data_ptr(), ctypes.byref(p),
                                                         *[b.data_ptr() for b in bufs], stream), "pert_tau_binarize")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,genome")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("binarize_timing needs a GPU")
    warnings.simplefilter("ignore")
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    for name in a.shapes.split(","):
        L, N = SHAPES[name]
        X = profiles(L, N)
        base = dict(shape=name, L=L, N=N)
        Xd = torch.from_numpy(X).cuda()
        p = B.bin_params(L)
        rows_d = Xd.T.contiguous()                               # (N, L): one row per cell
        raw = B.native_binarize(Xd, p)                           # the output buffers, reused by the timed launches
        outs = [raw[k].data_ptr() for k in ("means", "covs", "gmm_state", "rt_state", "dist", "best", "n_rep", "flags")]
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        ms = launch_ms(lambda: nat.check(nat.lib().pert_rt_binarize(L, N, rows_d.data_ptr(), ctypes.byref(p), *outs,
                                                                    stream), "pert_rt_binarize"))
        flags = raw["flags"].cpu().numpy()
        emit(what="pert_rt_binarize launch", median_ms=round(float(np.median(ms)), 3),
             min_ms=round(float(ms.min()), 3), us_per_cell=round(float(np.median(ms)) * 1e3 / N, 2), **base)
        bits = {str(b): int(((flags & b) != 0).sum()) for b in (1, 2, 4, 8, 16, 32, 64)}
        emit(what="flagged cells", flagged=int((flags != 0).sum()), share=round(float((flags != 0).mean()), 4),
             by_bit=bits, **base)

        t0 = time.perf_counter()
        res = B.binarize_matrix(X, device="cuda")
        t1 = time.perf_counter()
        emit(what="binarize_matrix cuda end to end", seconds=round(t1 - t0, 4), host_path_cells=int(res.flagged.sum()),
             **base)

        n_ex = min(16, N)
        t0 = time.perf_counter()
        for n in range(n_ex):
            B.exact_cell(X[:, n])
        t1 = time.perf_counter()
        emit(what="host path (exact_cell)", cells=n_ex, ms_per_cell=round((t1 - t0) * 1e3 / n_ex, 2), **base)

        t0 = time.perf_counter()
        cpu = B.binarize_matrix(X, device="cpu", exact=False)
        t1 = time.perf_counter()
        same = bool((cpu.rt_state == res.rt_state)[:, ~(cpu.flagged | res.flagged)].all())
        emit(what="CPU tensor program (no host path)", seconds=round(t1 - t0, 3), flagged=int(cpu.flagged.sum()),
             threads=torch.get_num_threads(), states_equal_device=same, **base)

        import pandas as pd
        sl = min(SLICE, N)
        cn = pd.DataFrame({"cell_id": np.repeat(np.arange(sl), L), "x": X[:, :sl].T.reshape(-1)})
        t0 = time.perf_counter()
        for _, cell in cn.groupby("cell_id"):
            out = B.exact_cell(cell["x"].values)
            for col, v in (("mean_0", out[0][0]), ("covariance_0", out[1][0]), ("mean_1", out[0][1]),
                           ("covariance_1", out[1][1]), ("gmm_state", out[2]), ("rt_state", out[3])):
                cn.loc[cell.index, col] = v
        t1 = time.perf_counter()
        emit(what="per-cell sklearn loop with per-cell column writes", cells=sl, seconds=round(t1 - t0, 3),
             ms_per_cell=round((t1 - t0) * 1e3 / sl, 2), **base)
        del Xd, rows_d, raw
        torch.cuda.empty_cache()

        ms = launch_ms(tau_launch(L, N))
        emit(what="pert_tau_binarize launch", median_ms=round(float(np.median(ms)), 3),
             min_ms=round(float(ms.min()), 3), us_per_cell=round(float(np.median(ms)) * 1e3 / N, 2), **base)
        torch.cuda.empty_cache()

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
