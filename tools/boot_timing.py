"""Device time of the cell bootstrap's three launches, CellBootstrap end to end, and the same
replicates taken one at a time through RTMatrix (what the matrix layer offered before).

    python tools/boot_timing.py [--shapes c2k,c4] [--boot 200] [--out profiles/boot_timing.jsonl]

One process, one GPU.  Per shape: a synthetic decode (as tools/rt_profiles_timing.py), 3 clones,
B replicates.
* kernels: pert_boot_weights, pert_boot_counts (B x 4 weight rows: 3 clones and the group of
  cells without one) and pert_boot_tfs_hist (population hours, fp32; and per clone) each timed
  with device events: 2 warm-up launches, 10 timed ones into re-zeroed outputs (the memset is
  outside the events), median and min.  ``counts_share`` is the counts launch's median over the
  sum of the three medians (weights + counts + population histogram).
* ``CellBootstrap passes``: host clock (ends in downloads, so synchronised) around
  construction (the resampler), ``counts()`` and ``tfs_counts()``; ``twidth_interval`` adds the B
  curve fits on the host.
* ``RTMatrix per replicate``: for the same weights, B times: gather the resampled columns on the
  device, build an RTMatrix on them, ``counts()`` and ``tfs_counts()``.  ``ratio`` is that time
  over the CellBootstrap passes' time; ``equal`` says the histograms agree.
Prints one JSON line per measurement."""
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
from scdna_replication_tools_amd import cell_bootstrap as cb    # noqa: E402
from scdna_replication_tools_amd import rt_profiles as rt       # noqa: E402

SHAPES = {"c2k": (5451, 2000), "c4": (5451, 10000), "tiny": (300, 500)}
N_CLONES = 3
WARMUP, REPS = 2, 10


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
    ap.add_argument("--shapes", default="c2k,c4")
    ap.add_argument("--boot", type=int, default=200)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-fits", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("boot_timing needs a GPU")
    lib, rows, B = nat.lib(), [], a.boot

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    # warm: code objects loaded, torch's allocator primed, before any host clock starts
    rep, _ = synthetic_decode(130, 300)
    small = rt.RTMatrix(rep, cell_ids=np.arange(300), chr=np.zeros(130, np.int64), start=np.arange(130),
                        clone_ids=np.arange(300) % N_CLONES)
    small.tfs_counts(by='population')
    small.bootstrap(n_boot=3).tfs_counts(by='population')

    for name in a.shapes.split(","):
        L, N = SHAPES[name]
        rep, ldn = synthetic_decode(L, N)
        labels = dict(cell_ids=np.arange(N), chr=np.zeros(L, np.int64), start=np.arange(L),
                      clone_ids=np.arange(N) % N_CLONES)
        m = rt.RTMatrix(rep, **labels)
        stream = torch.cuda.current_stream().cuda_stream
        base = dict(shape=name, L=L, N=N, clones=N_CLONES, B=B)

        # ---- end to end: the passes, then with the fits
        t0 = time.perf_counter()
        boot = cb.CellBootstrap(m, n_boot=B, seed=1)
        t1 = time.perf_counter()
        boot.counts('clone')
        t2 = time.perf_counter()
        hist = boot.tfs_counts(by='population')
        t3 = time.perf_counter()
        passes_s = t3 - t0
        emit(what="CellBootstrap passes", weights_s=round(t1 - t0, 4), counts_s=round(t2 - t1, 4),
             hist_s=round(t3 - t2, 4), total_s=round(passes_s, 4), **base)
        if not a.no_fits:
            t0 = time.perf_counter()
            try:
                iv = cb.CellBootstrap(m, n_boot=B, seed=1).twidth_interval()
                emit(what="CellBootstrap twidth_interval end to end", total_s=round(time.perf_counter() - t0, 4),
                     t_width=round(float(iv["t_width"][0]), 4), t_width_sd=round(float(iv["t_width_sd"][0]), 5), **base)
            except RuntimeError as e:                           # a curve fit that did not converge
                emit(what="CellBootstrap twidth_interval end to end", error=str(e), **base)

        # ---- the three launches
        G = N_CLONES + 1
        ldw = boot.ldw
        order, pos_lo, pos_n = (torch.as_tensor(x, device="cuda") for x in cb.stratum_layout(boot._group))
        scratch = torch.zeros((B, N), dtype=torch.int32, device="cuda")
        w = torch.zeros((B, ldw), dtype=torch.uint8, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        med = {}
        med["weights"], mn = timed(
            lambda: nat.check(lib.pert_boot_weights(N, ldw, pos_lo.data_ptr(), pos_n.data_ptr(), order.data_ptr(), 1, 0,
                                                    B, scratch.data_ptr(), w.data_ptr(), flag.data_ptr(), stream),
                              "pert_boot_weights"), lambda: scratch.zero_())
        emit(what="pert_boot_weights", median_us=round(med["weights"], 2), min_us=round(mn, 2), **base)
        member = torch.zeros((G, ldw), dtype=torch.uint8, device="cuda")
        member[torch.as_tensor(boot._group, device="cuda"), torch.arange(N, device="cuda")] = 1
        wg = (w[:, None, :] * member[None]).contiguous()
        count = torch.zeros((B * G, L), dtype=torch.int32, device="cuda")
        med["counts"], mn = timed(
            lambda: nat.check(lib.pert_boot_counts(L, N, ldn, rep.data_ptr(), B * G, ldw, wg.data_ptr(),
                                                   count.data_ptr(), stream), "pert_boot_counts"),
            lambda: count.zero_())
        emit(what="pert_boot_counts", rows=B * G, median_us=round(med["counts"], 2), min_us=round(mn, 2), **base)
        f10 = torch.as_tensor((m.cell_fractions(np.float32) * 10.0).astype(np.float32), device="cuda")
        edges = torch.as_tensor(rt.interval_edges().astype(np.float32), device="cuda")
        for by, g_hist in (("population", 1), ("clone", N_CLONES)):
            hours = torch.as_tensor(np.ascontiguousarray(boot.profiles(by)[1][:, :g_hist]), device="cuda")
            group = np.zeros(N, np.int32) if by == "population" else m._clone_of.astype(np.int32)
            grp = torch.as_tensor(group, device="cuda")
            hn = torch.zeros((B, g_hist, 200), dtype=torch.int32, device="cuda")
            hr = torch.zeros_like(hn)
            med[by], mn = timed(
                lambda: nat.check(lib.pert_boot_tfs_hist(L, N, ldn, g_hist, rep.data_ptr(), grp.data_ptr(), B, ldw,
                                                         w.data_ptr(), hours.data_ptr(), f10.data_ptr(),
                                                         edges.data_ptr(), 201, 0, hn.data_ptr(), hr.data_ptr(),
                                                         stream), "pert_boot_tfs_hist"),
                lambda: (hn.zero_(), hr.zero_()))
            emit(what="pert_boot_tfs_hist {} float32".format(by), groups=g_hist, median_us=round(med[by], 2),
                 min_us=round(mn, 2), decisions_per_ns=round(B * L * N / med[by] / 1e3, 2), **base)
        emit(what="launch shares", counts_share=round(med["counts"] / (med["weights"] + med["counts"] +
                                                                       med["population"]), 4), **base)

        # ---- the same replicates one at a time through RTMatrix
        if not a.no_baseline:
            weights = torch.from_numpy(boot.weights).cuda()
            cells = torch.arange(N, device="cuda")
            equal = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in range(B):
                cols = torch.repeat_interleave(cells, weights[b].long())
                cols_h = cols.cpu().numpy()
                one = rt.RTMatrix(rep.index_select(1, cols), cell_ids=labels["cell_ids"][cols_h], chr=labels["chr"],
                                  start=labels["start"], clone_ids=labels["clone_ids"][cols_h])
                one.counts()
                got = one.tfs_counts(by='population')
                equal = equal and bool((got[0] == hist[0][b, 0]).all() and (got[1] == hist[1][b, 0]).all())
            base_s = time.perf_counter() - t0
            emit(what="RTMatrix per replicate", total_s=round(base_s, 4), ratio=round(base_s / passes_s, 2),
                 equal=equal, **base)
        del rep, m, boot
        torch.cuda.empty_cache()

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
