"""Time of the bulk G1 GC correction (gc_correction.py): the queued launches of pert_lowess_curve,
and bulk_g1_gc_correction end to end on the long tables.

    python tools/lowess_timing.py [--shapes genome] [--bench-json FILE] [--out profiles/lowess_timing.jsonl]

One process.  Per shape (G1/2 cells x bins of gamma-distributed rpm around a GC curve, 2 % of the
points x 4; GC rounded to 3 decimals, U ~ 350 distinct values, and to 9, every bin its own): one
call of pert_lowess_curve (frac 2/3, it 3: 5 sums passes, 4 medians of 6 histogram passes, 5 local
regressions) timed with device events around the call (2 warm-up calls, 5 timed, median and min);
the bytes its 29 streaming passes read from the rpm matrix divided by that time -- a floor of their
rate, the regressions and the small kernels are inside the time -- next to the HBM figures of a
bench.py result line (``--bench-json``, a ``bench.py --full`` record from the same device: its pattern
ceiling and achieved GB/s; the committed record is profiles/lowess_timing_bench.json);
and ``bulk_g1_gc_correction(device='cuda')`` once on DataFrames of the same cells plus --s-cells
S-phase cells.  Nothing here is a gate.  The reference's own time (statsmodels over the same points,
then a per-row DataFrame.apply) is not measured: statsmodels is not a dependency of this project.
Prints one JSON line per measurement."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scdna_replication_tools_amd import _native as nat        # noqa: E402
from scdna_replication_tools_amd import gc_correction as G      # noqa: E402

SHAPES = {"tiny": (64, 96), "small": (400, 271), "genome": (2000, 5451)}
WARMUP, REPS = 2, 5
HIST_PASSES = 6


def table(C, L, digits, seed=0):
    rng = np.random.default_rng(seed)
    gc = np.round(rng.uniform(0.3, 0.65, L), digits)
    Y = (180.0 * (1.0 - 8.0 * (gc - 0.45) ** 2))[None, :] * rng.gamma(20.0, 1.0 / 20.0, (C, L))
    Y[rng.uniform(size=Y.shape) < 0.02] *= 4.0
    return gc, Y


def frames(gc, Y, s_cells, seed=1):
    import pandas as pd
    rng = np.random.default_rng(seed)
    C, L = Y.shape
    reads_g = rng.poisson(Y)
    reads_s = rng.poisson(Y[:s_cells] * rng.choice([1.0, 2.0], size=(s_cells, L)))

    def long(reads, tag):
        n = reads.shape[0]
        return pd.DataFrame({"cell_id": np.repeat(np.array(["{}{:05d}".format(tag, i) for i in range(n)], dtype=object), L),
                             "library_id": "A", "chr": "1", "start": np.tile(np.arange(L) * 500000, n),
                             "gc": np.tile(gc, n), "reads": reads.reshape(-1)})
    return long(reads_s, "s"), long(reads_g, "g")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="genome")
    ap.add_argument("--s-cells", type=int, default=200)
    ap.add_argument("--bench-json", default=None, help="a file holding a bench.py --full result line from the same device")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lowess_timing needs a GPU")
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    hbm = None
    if a.bench_json:
        with open(a.bench_json) as fh:
            rec = [json.loads(ln) for ln in fh if ln.lstrip().startswith("{")][-1]
        roof = rec.get("roofline", {})
        hbm = dict(bench_achieved_GBs=roof.get("achieved"), bench_pattern_ceiling_GBs=(roof.get("pattern_ceiling") or {}).get("GB/s"))
    lib = nat.lib()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    for name in a.shapes.split(","):
        C, L = SHAPES[name]
        for digits in (3, 9):
            gc, Y = table(C, L, digits)
            ux, inv = G._distinct(gc)
            U = len(ux)
            base = dict(shape=name, cells=C, bins=L, distinct_gc=U)
            Yd = torch.from_numpy(Y).cuda()
            k = G.lowess_k(C * L, G.FRAC)
            nbytes = ctypes.c_int64()
            nat.check(lib.pert_lowess_workspace(C, L, U, U, ctypes.byref(nbytes)), "pert_lowess_workspace")
            ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device="cuda")
            out = torch.empty(U, dtype=torch.float64, device="cuda")
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
            host = []
            for i in range(WARMUP + REPS):
                if i >= WARMUP:
                    ev[i - WARMUP][0].record()
                t0 = time.perf_counter()
                nat.check(lib.pert_lowess_curve(C, L, U, U, Yd.data_ptr(), inv.ctypes.data_as(ip), ux.ctypes.data_as(dp),
                                                ux.ctypes.data_as(dp), k, G.IT, out.data_ptr(), ws.data_ptr(),
                                                int(nbytes.value), stream), "pert_lowess_curve")
                host.append(time.perf_counter() - t0)
                if i >= WARMUP:
                    ev[i - WARMUP][1].record()
                torch.cuda.synchronize()
            ms = np.array([s.elapsed_time(e) for s, e in ev])
            passes = (G.IT + 2) + HIST_PASSES * (G.IT + 1)
            streamed = passes * C * L * 8
            emit(what="pert_lowess_curve queued launches (device events)", median_ms=round(float(np.median(ms)), 3),
                 min_ms=round(float(ms.min()), 3), queue_ms_host=round(float(np.median(host[WARMUP:])) * 1e3, 3),
                 workspace_MiB=round(nbytes.value / 2 ** 20, 2), **base)
            emit(what="streaming passes: bytes read from the rpm matrix / whole call time", passes=passes,
                 GB=round(streamed / 1e9, 3), GBs=round(streamed / (float(np.median(ms)) * 1e-3) / 1e9, 1),
                 **dict(hbm or {}), **base)
            del Yd, ws
            torch.cuda.empty_cache()
            if digits == 9:
                cn_s, cn_g1 = frames(gc, Y, min(a.s_cells, C))
                t0 = time.perf_counter()
                out_s, out_g = G.bulk_g1_gc_correction(cn_s, cn_g1, device="cuda")
                t1 = time.perf_counter()
                emit(what="bulk_g1_gc_correction cuda end to end (DataFrames in, DataFrames out)",
                     seconds=round(t1 - t0, 3), rows_g1=len(cn_g1), rows_s=len(cn_s),
                     mean_corrected_g1=round(float(out_g["rpm_gc_norm"].mean()), 4), **base)
    emit(what="note", text="no gate on these numbers; the reference's own time (statsmodels, then a per-row "
                           "DataFrame.apply) is not measured here")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
