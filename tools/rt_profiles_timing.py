"""Device time of pert_rt_counts / pert_rt_tfs_hist against the chunked numpy path.

    python tools/rt_profiles_timing.py [--shapes c4,shard20kb] [--no-host] [--out FILE]

One process.  Per shape: a synthetic decode (bins x cells uint8 on the GPU, replication state =
locus timing + noise < the cell's S-phase time), the hours rows and fractions RTMatrix derives
from it, then each kernel timed with device events: 3 warm-up launches, 20 timed ones (each into
re-zeroed outputs; the memset is outside the events), median and min.  ``GB/s`` is the state
matrix's bytes (L x ldn) over the median, ``of_spec`` that over the 8 TB/s HBM3E spec.  The host
rows time RTMatrix's chunked numpy passes once on the same matrix.  Prints one JSON line per
measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scdna_replication_tools_amd import _native as nat          # noqa: E402
from scdna_replication_tools_amd import rt_profiles as rt       # noqa: E402

SHAPES = {"c4": (5451, 10000, 4), "shard20kb": (136000, 2000, 4), "tiny": (300, 500, 2)}
HBM_SPEC = 8.0e12
WARMUP, REPS = 3, 20


def synthetic_decode(L, N, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ldn = -(-N // 256) * 256
    rep = torch.zeros((L, ldn), dtype=torch.uint8, device="cuda")
    locus = torch.rand(L, generator=g, device="cuda")
    tau = torch.rand(N, generator=g, device="cuda") * 0.8 + 0.1
    step = max(1, (1 << 26) // N)
    for l0 in range(0, L, step):
        noise = torch.randn((min(step, L - l0), N), generator=g, device="cuda") * 0.15
        rep[l0:l0 + step, :N] = (locus[l0:l0 + step, None] + noise < tau[None, :]).to(torch.uint8)
    return rep[:, :N], ldn


def timed(launch, zero):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for i in range(WARMUP + REPS):
        zero()
        if i >= WARMUP:
            ev[i - WARMUP][0].record()
        launch()
        if i >= WARMUP:
            ev[i - WARMUP][1].record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3
    return float(np.median(us)), float(us.min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4,shard20kb")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rt_profiles_timing needs a GPU")
    lib, rows = nat.lib(), []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    for name in a.shapes.split(","):
        L, N, n_clones = SHAPES[name]
        rep, ldn = synthetic_decode(L, N)
        labels = dict(cell_ids=np.arange(N), chr=np.zeros(L, np.int64), start=np.arange(L),
                      clone_ids=np.arange(N) % n_clones)
        m = rt.RTMatrix(rep, **labels)
        stream = torch.cuda.current_stream().cuda_stream
        nbytes = L * ldn
        base = dict(shape=name, L=L, N=N, ldn=ldn, clones=n_clones, state_bytes=nbytes)

        def report(kernel, med, mn):
            emit(kernel=kernel, median_us=round(med, 2), min_us=round(mn, 2), GBps=round(nbytes / med / 1e3, 1),
                 of_spec=round(nbytes / (med * 1e-6) / HBM_SPEC, 4), **base)

        group = torch.as_tensor((np.arange(N) % n_clones).astype(np.int32), device="cuda")
        bins = torch.zeros((n_clones, L), dtype=torch.int32, device="cuda")
        cells = torch.zeros(N, dtype=torch.int32, device="cuda")
        report("pert_rt_counts", *timed(
            lambda: nat.check(lib.pert_rt_counts(L, N, ldn, n_clones, rep.data_ptr(), group.data_ptr(),
                                                 bins.data_ptr(), cells.data_ptr(), stream), "pert_rt_counts"),
            lambda: (bins.zero_(), cells.zero_())))

        pb = m.pseudobulk(np.float32)
        for T in (np.float32, np.float64):
            hours = torch.as_tensor(np.stack([pb["clones"][c][1] for c in m.clones]).astype(T), device="cuda")
            f10 = torch.as_tensor((m.cell_fractions(np.float32) * 10.0).astype(T), device="cuda")
            edges = torch.as_tensor(rt.interval_edges().astype(T), device="cuda")
            for per_cell, label in ((0, "aggregate"), (1, "per_cell_lds_tile"), (2, "per_cell_global_adds")):
                shape = (N, 200) if per_cell else (200,)
                hn = torch.zeros(shape, dtype=torch.int32, device="cuda")
                hr = torch.zeros(shape, dtype=torch.int32, device="cuda")
                report("pert_rt_tfs_hist {} {}".format(label, np.dtype(T).name), *timed(
                    lambda: nat.check(lib.pert_rt_tfs_hist(
                        L, N, ldn, n_clones, rep.data_ptr(), group.data_ptr(), hours.data_ptr(), f10.data_ptr(),
                        edges.data_ptr(), 201, int(T == np.float64), per_cell, hn.data_ptr(), hr.data_ptr(), stream),
                        "pert_rt_tfs_hist"),
                    lambda: (hn.zero_(), hr.zero_())))

        # end to end through RTMatrix on the device (uploads, launches, downloads, host arithmetic)
        m2 = rt.RTMatrix(rep, **labels)
        t0 = time.perf_counter()
        m2.pseudobulk(np.float32)
        t1 = time.perf_counter()
        dev_hist = m2.tfs_counts(by="clone")
        t2 = time.perf_counter()
        dev_cell = m2.tfs_counts(by="clone", per_cell=True)
        t3 = time.perf_counter()
        emit(kernel="RTMatrix device end to end", pseudobulk_s=round(t1 - t0, 4), hist_s=round(t2 - t1, 4),
             hist_per_cell_s=round(t3 - t2, 4), **base)
        if not a.no_host:
            h = rt.RTMatrix(rep.cpu().numpy(), device="cpu", **labels)
            t0 = time.perf_counter()
            h.pseudobulk(np.float32)
            t1 = time.perf_counter()
            host_hist = h.tfs_counts(by="clone")
            t2 = time.perf_counter()
            host_cell = h.tfs_counts(by="clone", per_cell=True)
            t3 = time.perf_counter()
            same = all((x == y).all() for x, y in zip(dev_hist + dev_cell, host_hist + host_cell))
            emit(kernel="RTMatrix chunked numpy", pseudobulk_s=round(t1 - t0, 3), hist_s=round(t2 - t1, 3),
                 hist_per_cell_s=round(t3 - t2, 3), equals_device=bool(same), **base)
        del rep, m, m2
        torch.cuda.empty_cache()

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
