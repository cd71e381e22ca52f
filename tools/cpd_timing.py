"""Time of the cell level's change-point search (normalize_cell.py): one two-breakpoint round of
pert_cpd_search over all cells, the numpy twin on a slice of the same cells, and normalize_by_cell
end to end on long tables.

    python tools/cpd_timing.py [--shapes genome] [--host-cells 4] [--table-cells 400] [--out profiles/cpd_timing.jsonl]

One process.  Per shape (cells x bins of unit noise with a few level shifts): one call of
pert_cpd_search in mode 2 for every cell (its three launches and the upload of the per-cell arrays),
timed with device events around the call (1 warm-up call, 3 timed, median and min), and the
candidates (a, b) it evaluates per second; ``cpd_search_host`` on the first --host-cells cells of the
same matrix on this machine's CPU (one thread of numpy), its time per cell and what all cells would
take at that rate -- an extrapolation, and recorded as one; then ``normalize_by_cell(device='cuda')``
once on DataFrames of --table-cells S-phase and as many G1/2 cells over the same bins (23 chromosomes,
Poisson reads, a planted gain in every tenth S cell), with the number of rounds it ran.  Nothing here
is a gate.  ruptures' own time is not measured: it is not a dependency of this project.
Prints one JSON line per measurement."""
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

from scdna_replication_tools_amd import normalize_cell as NC     # noqa: E402

SHAPES = {"tiny": (48, 300), "small": (400, 271), "genome": (2000, 5451)}
WARMUP, REPS = 1, 3


def profiles(N, L, seed=0):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((N, L))
    for c in range(N):
        for _ in range(2):
            lo = int(rng.integers(0, L - 4))
            Y[c, lo:lo + int(rng.integers(2, max(L // 8, 3)))] += rng.choice([-1.0, 1.0])
    return Y


def candidates(n):
    m = n - 5                                  # a in [2, n - 4], b in [a + 2, n - 2]
    return m * (m + 1) // 2 if m > 0 else 0


def frames(n_cells, L, seed=1):
    import pandas as pd
    rng = np.random.default_rng(seed)
    names = [str(i + 1) for i in range(22)] + ["X"]
    edges = np.linspace(0, L, len(names) + 1).astype(int)
    chrom = np.empty(L, dtype=object)
    for k, nm in enumerate(names):
        chrom[edges[k]:edges[k + 1]] = nm
    base = rng.gamma(40.0, 5.0, L)

    def long(tag, planted):
        reads = rng.poisson(np.broadcast_to(base, (n_cells, L))).astype(np.float64)
        if planted:
            for c in range(0, n_cells, 10):
                lo = int(rng.integers(0, L - L // 20))
                reads[c, lo:lo + L // 40] *= 1.6
        cells = np.array(["{}{:05d}".format(tag, i) for i in range(n_cells)], dtype=object)
        rpm = reads / reads.sum(1, keepdims=True) * 1e6
        return pd.DataFrame({"cell_id": np.repeat(cells, L), "chr": np.tile(chrom, n_cells),
                             "start": np.tile(np.arange(L) * 500000, n_cells), "clone_id": "A", "state": 2,
                             "reads": reads.reshape(-1), "rpm_gc_norm": rpm.reshape(-1)})
    return long("s", True), long("g", False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="genome")
    ap.add_argument("--host-cells", type=int, default=4)
    ap.add_argument("--table-cells", type=int, default=400)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cpd_timing needs a GPU")
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    ip = ctypes.POINTER(ctypes.c_int32)
    for name in a.shapes.split(","):
        N, L = SHAPES[name]
        base = dict(shape=name, cells=N, bins=L)
        Y = profiles(N, L)
        s = NC._DeviceSearch(Y, "cuda")
        lens, mode, active = np.full(N, L, np.int32), np.full(N, 2, np.int32), np.ones(N, np.int32)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
        for i in range(WARMUP + REPS):
            if i >= WARMUP:
                ev[i - WARMUP][0].record()
            s.native.check(s.lib.pert_cpd_search(N, L, s.Y.data_ptr(), lens.ctypes.data_as(ip), mode.ctypes.data_as(ip),
                                                 active.ctypes.data_as(ip), s.a.data_ptr(), s.b.data_ptr(),
                                                 s.g.data_ptr(), s.ws.data_ptr(), s.nbytes, stream), "pert_cpd_search")
            if i >= WARMUP:
                ev[i - WARMUP][1].record()
            torch.cuda.synchronize()
        ms = np.array([u.elapsed_time(v) for u, v in ev])
        total = candidates(L) * N
        emit(what="pert_cpd_search, one two-breakpoint round over all cells (device events)",
             median_ms=round(float(np.median(ms)), 3), min_ms=round(float(ms.min()), 3), candidates=total,
             candidates_per_s=round(total / (float(np.median(ms)) * 1e-3), 0),
             workspace_MiB=round(s.nbytes / 2 ** 20, 2), **base)
        k = min(a.host_cells, N)
        t0 = time.perf_counter()
        ha, hb, hg = NC.cpd_search_host(Y[:k])
        t1 = time.perf_counter()
        da, db, dg = s.a.cpu().numpy()[:k], s.b.cpu().numpy()[:k], s.g.cpu().numpy()[:k]
        emit(what="cpd_search_host on a slice of the same cells (numpy, this machine's CPU)", slice_cells=k,
             seconds=round(t1 - t0, 3), seconds_per_cell=round((t1 - t0) / k, 4),
             extrapolated_seconds_all_cells=round((t1 - t0) / k * N, 1),
             bit_equal_to_kernel=bool((ha == da).all() and (hb == db).all() and (hg.view(np.uint64) == dg.view(np.uint64)).all()),
             **base)
        del s
        torch.cuda.empty_cache()
        n_tab = min(a.table_cells, N)
        cn_s, cn_g1 = frames(n_tab, L)
        seen = []
        inner = NC.changepoint_rounds

        def counting(*args, **kw):
            res = inner(*args, **kw)
            seen.append(res[2])
            return res
        NC.changepoint_rounds = counting
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t0 = time.perf_counter()
                out = NC.normalize_by_cell(cn_s, cn_g1, device="cuda")
                t1 = time.perf_counter()
        finally:
            NC.changepoint_rounds = inner
        r = seen[0]
        emit(what="normalize_by_cell cuda end to end (DataFrames in, DataFrame out)", seconds=round(t1 - t0, 2),
             s_cells=n_tab, g1_cells=n_tab, rows_s=len(cn_s), rows_out=len(out), rounds=int(r.max()),
             searches_per_cell_mean=round(float(r.mean()), 2),
             cells_with_segments=int((out.groupby("cell_id")["changepoint_segments"].max() > 0).sum()),
             shape=name, bins=L)
    emit(what="note", text="no gate on these numbers; ruptures' own time (one cell at a time, an O(n^2) dynamic "
                           "programme) is not measured here")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
