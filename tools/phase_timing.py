"""Time of the phase-call features (phase_matrix.py): the pert_phase_counts and pert_phase_acf
launches, ``PhaseMatrix.features()`` end to end, and the DataFrame path it stands beside.

    python tools/phase_timing.py [--shapes c3,c4] [--frame-shapes c3,c4] [--out profiles/phase_timing.jsonl]

One process, one GPU.  Per shape (bins x cells; states that switch about every 50 bins, copy-number
states with a few changes, Poisson reads under a slow AR(1) envelope, all generated on the device
from a seed): each kernel timed with device events (3 warm-up launches, 10 timed ones into the same
buffers, so the inputs stay in the Infinity Cache where they fit; median and min) with the bytes it
has to read (one byte per state, two passes over the float reads) and the rate that is of them; ``PhaseMatrix(...).features()`` over the device matrices in place
(launches, downloads of the per-cell outputs, the exact rationals, the table), median of 3; then,
for ``--frame-shapes``, the DataFrame path on the equivalent long table in the same process:
building that table from the matrices (with the ``rpm`` column by groupby-transform), then
``compute_cell_frac`` + ``compute_quality_features`` on the GPU.  Prints one JSON line per
measurement and writes them to ``--out`` as it goes."""
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

from scdna_replication_tools_amd import _native as nat                                    # noqa: E402
from scdna_replication_tools_amd import predict_cycle_phase as pcp                        # noqa: E402
from scdna_replication_tools_amd.phase_matrix import PhaseMatrix                          # noqa: E402

SHAPES = {"tiny": (300, 96), "c3": (5451, 2000), "c4": (5451, 10000)}
WARMUP, REPS = 3, 10
MAX_LAG = pcp.MAX_LAG


def matrices(L, N, seed=0):
    """rep, cn uint8 [L][ldn] and reads float32 [L][ldn] on the device, ldn = N rounded up to 256."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ldn = -(-N // 256) * 256
    u = lambda: torch.rand((L, ldn), device="cuda", generator=g)
    rep = (torch.cumsum((u() < 0.02).to(torch.int32), dim=0) % 2).to(torch.uint8)
    cn = (2 + torch.cumsum((u() < 0.001).to(torch.int32), dim=0) % 3).to(torch.uint8)
    z = torch.empty((L, ldn), device="cuda")
    z[0] = torch.randn(ldn, device="cuda", generator=g)
    for t in range(1, L):
        z[t] = 0.97 * z[t - 1] + (1 - 0.97 ** 2) ** 0.5 * torch.randn(ldn, device="cuda", generator=g)
    reads = torch.poisson(60.0 * torch.exp(0.5 * z), generator=g)
    return rep, cn, reads, ldn


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


def long_table(rep, cn, reads, N):
    """The long table the matrices stand for (cell-major), as a caller of the DataFrame path builds it."""
    import pandas as pd
    L = rep.shape[0]
    host = lambda m, dt: np.ascontiguousarray(m[:, :N].T.cpu().numpy().astype(dt)).reshape(-1)
    frame = pd.DataFrame({"cell_id": np.repeat(np.arange(N), L), "model_rep_state": host(rep, np.float64),
                          "model_cn_state": host(cn, np.float64), "reads": host(reads, np.float64)})
    frame["rpm"] = frame["reads"] / frame.groupby("cell_id")["reads"].transform("sum") * 1e6
    return frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c3,c4")
    ap.add_argument("--frame-shapes", default="c3,c4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("phase_timing needs a GPU")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")

    lib = nat.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    frame_shapes = [s for s in a.frame_shapes.split(",") if s]
    for name in a.shapes.split(","):
        L, N = SHAPES[name]
        base = dict(shape=name, L=L, N=N)
        rep, cn, reads, ldn = matrices(L, N)

        pc = torch.zeros((4, N), dtype=torch.int32, device="cuda")
        pl = torch.zeros((3, MAX_LAG, N), dtype=torch.int32, device="cuda")
        ms = launch_ms(lambda: nat.check(lib.pert_phase_counts(
            L, N, ldn, 1, 0, rep.data_ptr(), cn.data_ptr(), MAX_LAG, pc[0].data_ptr(), pc[1].data_ptr(), pc[2].data_ptr(),
            pc[3].data_ptr(), pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), stream), "pert_phase_counts"))
        nbytes = 2 * L * N
        emit(what="pert_phase_counts launch (rep + cn)", median_ms=round(float(np.median(ms)), 4),
             min_ms=round(float(ms.min()), 4), bytes_read=nbytes,
             gb_per_s=round(nbytes / (float(np.median(ms)) * 1e-3) / 1e9, 1), **base)

        need = ctypes.c_int64()
        nat.check(lib.pert_phase_acf_workspace(L, N, MAX_LAG, ctypes.byref(need)), "pert_phase_acf_workspace")
        ws = torch.empty(need.value // 8, dtype=torch.float64, device="cuda")
        mean = torch.empty(N, dtype=torch.float64, device="cuda")
        c = torch.empty((MAX_LAG + 1, N), dtype=torch.float64, device="cuda")
        ms = launch_ms(lambda: nat.check(lib.pert_phase_acf(
            L, N, ldn, reads.data_ptr(), 0, MAX_LAG, mean.data_ptr(), c.data_ptr(), ws.data_ptr(), need.value, stream),
            "pert_phase_acf"))
        nbytes = 2 * 4 * L * N
        emit(what="pert_phase_acf call (float32 reads, 3 kernels)", median_ms=round(float(np.median(ms)), 4),
             min_ms=round(float(ms.min()), 4), bytes_read=nbytes, workspace_bytes=int(need.value),
             fma_f64=L * N * (MAX_LAG + 1), gb_per_s=round(nbytes / (float(np.median(ms)) * 1e-3) / 1e9, 1), **base)

        ids = np.arange(N)
        secs = []
        for _ in range(4):                               # the first is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            table = PhaseMatrix(rep[:, :N], cn[:, :N], reads[:, :N], ids).features()
            secs.append(time.perf_counter() - t0)
        emit(what="PhaseMatrix.features() end to end, device matrices in place",
             median_s=round(float(np.median(secs[1:])), 4), first_s=round(secs[0], 4), **base)

        if name in frame_shapes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            frame = long_table(rep, cn, reads, N)
            t1 = time.perf_counter()
            frame = pcp.compute_cell_frac(frame)
            frame = pcp.compute_quality_features(frame, device="cuda")
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            per = frame.iloc[::L]
            emit(what="DataFrame path: long table, then compute_cell_frac + compute_quality_features (cuda)",
                 rows=len(frame), build_table_s=round(t1 - t0, 3), features_s=round(t2 - t1, 3),
                 total_s=round(t2 - t0, 3),
                 rep_auto_max_abs_diff=float(np.nanmax(np.abs(per["rep_auto"].to_numpy() - table["rep_auto"].to_numpy()))),
                 rpm_auto_max_abs_diff=float(np.nanmax(np.abs(per["rpm_auto"].to_numpy() - table["rpm_auto"].to_numpy()))),
                 **base)
            del frame, per
        del rep, cn, reads, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
