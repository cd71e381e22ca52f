"""Time pert_enum_posterior against the decode pass of the same shard (device events).

    python tools/posterior_timing.py [--cells 10000 1250] [--launches 12] [--out profiles/posterior_timing.jsonl]

The decode (pert_enum_pass, PERT_MODE_DECODE) is the yardstick: it streams the same reads and
pi logits and evaluates the same 2P scores.  For each shape -- seeded simulator.simulate
inputs on the 5,451-bin grid, P = 13, the g1_clones prior, 20 SVI steps from the initial values
so the logits are no longer uniform -- the two kernels are warmed up and then launched
alternately, each launch between its own pair of events; the posterior once with cn_prob
alone and once more with the P-plane cn_marg.  One JSON row per (shape, run) is appended to
--out: median and range in milliseconds of both kernels, and their ratio.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

P, K = 13, 4


def make_shard(n_cells: int, seed: int):
    from scdna_replication_tools_amd import _native as nat
    from scdna_replication_tools_amd.engine import EtaCodebook, PertShard
    from scdna_replication_tools_amd.init import init_params
    from scdna_replication_tools_amd.simulator import simulate
    sim = simulate(n_s=n_cells, n_g=1, num_reads=1e6, seed=seed)
    reads = sim.reads_s.astype(np.float32)
    states = np.minimum(sim.cn_s.astype(np.int64), P - 1)
    eta = EtaCodebook.from_states(states, 1e6, P)
    bm = np.zeros((1, K + 1))
    bm[0, K - 1] = 0.5
    libs = np.zeros(n_cells, int)
    t_init = np.clip(sim.tau_s, 0.05, 0.95)
    init = init_params(nat.KIND_STEP2, reads, libs, 1, P, K, ploidy=eta.argmax_states().mean(0), t_init=t_init,
                       beta_means=bm, seed=0)
    return PertShard(nat.KIND_STEP2, reads, sim.gc, libs, 1, P, K, init, eta=eta, lamb=0.75, beta_means=bm,
                     device="cuda")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[10000, 1250])
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_timing.jsonl"))
    a = ap.parse_args()
    if a.launches < 10:
        raise SystemExit("--launches: at least 10 per kernel")
    from scdna_replication_tools_amd import _native as nat
    for n_cells in a.cells:
        sh = make_shard(n_cells, a.seed)
        for _ in range(20):
            sh.step_async()
        sh.decode()
        L, ldn = sh.L, sh.ldn
        rep_prob = torch.zeros((L, ldn), dtype=torch.float32, device=sh.device)
        cn_prob = torch.zeros_like(rep_prob)
        cn_marg = torch.zeros((P, L, ldn), dtype=torch.float32, device=sh.device)
        stream = sh._stream()
        for run, marg in (("cn_prob", None), ("cn_prob+cn_marg", cn_marg)):
            def post():
                nat.check(sh.lib.pert_enum_posterior(ctypes.byref(sh._prob), ctypes.byref(sh._state),
                                                     sh.cn_out.data_ptr(), rep_prob.data_ptr(), cn_prob.data_ptr(),
                                                     0 if marg is None else marg.data_ptr(), stream),
                          "pert_enum_posterior")

            def dec():
                sh._pass(nat.MODE_DECODE)
            for _ in range(a.warmup):
                dec()
                post()
            ev = {"decode": [], "posterior": []}
            for _ in range(a.launches):
                ev["decode"].append(timed(dec))
                ev["posterior"].append(timed(post))
            torch.cuda.synchronize()
            ms = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}
            row = {"tool": "posterior_timing", "device": torch.cuda.get_device_name(sh.device), "cells": n_cells,
                   "bins": L, "P": P, "bins_per_tile": sh.bins_per_tile, "run": run, "launches": a.launches,
                   "decode": stats(ms["decode"]), "posterior": stats(ms["posterior"]),
                   "posterior_over_decode": round(float(np.median(ms["posterior"]) / np.median(ms["decode"])), 3),
                   "lib": sh.lib.pert_version().decode()}
            print(json.dumps(row), flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(row) + "\n")
        del sh, rep_prob, cn_prob, cn_marg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
