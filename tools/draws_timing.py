"""Time pert_enum_draw against pert_enum_posterior on the same shard (device events).

    python tools/draws_timing.py [--cells 10000 1250] [--draws 1 16 64] [--launches 12]
                                 [--out profiles/draws_timing.jsonl]

The posterior pass with cn_prob (pert_enum_posterior) is the yardstick: it streams the same reads
and pi logits and evaluates the same 2P scores, once per element.  The shapes, inputs and protocol
are tools/posterior_timing.py's: seeded simulator.simulate inputs on the 5,451-bin grid, P = 13, 20
SVI steps from the initial values; per run the two kernels are warmed up and then launched
alternately, each launch between its own pair of events.  The draw pass runs at each number of
draws with and without the cn planes.  One JSON row per (shape, draws, planes) is appended to
--out: median and range in milliseconds of both kernels, their ratio, the bytes the draw pass
stores and its stored bytes per millisecond.
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

from tools.posterior_timing import P, make_shard, stats, timed   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[10000, 1250])
    ap.add_argument("--draws", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--layout", default="byte_rows", help="label of the store layout the library was built with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draws_timing.jsonl"))
    a = ap.parse_args()
    if a.launches < 10:
        raise SystemExit("--launches: at least 10 per kernel")
    from scdna_replication_tools_amd import _native as nat
    for n_cells in a.cells:
        sh = make_shard(n_cells, a.seed)
        for _ in range(20):
            sh.step_async()
        sh.decode()
        L, N, ldn = sh.L, sh.N, sh.ldn
        rep_prob = torch.zeros((L, ldn), dtype=torch.float32, device=sh.device)
        cn_prob = torch.zeros_like(rep_prob)
        stream = sh._stream()

        def post():
            nat.check(sh.lib.pert_enum_posterior(ctypes.byref(sh._prob), ctypes.byref(sh._state),
                                                 sh.cn_out.data_ptr(), rep_prob.data_ptr(), cn_prob.data_ptr(), 0,
                                                 stream), "pert_enum_posterior")

        for n_draws in a.draws:
            rep = torch.zeros((n_draws, L, ldn), dtype=torch.uint8, device=sh.device)
            cn = torch.zeros_like(rep)
            for planes, cn_ptr in (("rep", 0), ("rep+cn", cn.data_ptr())):
                def draw():
                    nat.check(sh.lib.pert_enum_draw(ctypes.byref(sh._prob), ctypes.byref(sh._state), a.seed, 0, 0,
                                                    n_draws, rep.data_ptr(), cn_ptr, stream), "pert_enum_draw")
                for _ in range(a.warmup):
                    post()
                    draw()
                ev = {"posterior": [], "draw": []}
                for _ in range(a.launches):
                    ev["posterior"].append(timed(post))
                    ev["draw"].append(timed(draw))
                torch.cuda.synchronize()
                ms = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}
                stored = n_draws * L * N * (2 if cn_ptr else 1)
                med = float(np.median(ms["draw"]))
                row = {"tool": "draws_timing", "device": torch.cuda.get_device_name(sh.device), "cells": n_cells,
                       "bins": L, "P": P, "bins_per_tile": sh.bins_per_tile, "layout": a.layout, "draws": n_draws,
                       "planes": planes, "launches": a.launches, "posterior": stats(ms["posterior"]),
                       "draw": stats(ms["draw"]), "draw_over_posterior": round(med / float(np.median(ms["posterior"])), 3),
                       "stored_bytes": stored, "stored_mb_per_ms": round(stored / med / 1e6, 3),
                       "lib": sh.lib.pert_version().decode()}
                print(json.dumps(row), flush=True)
                os.makedirs(os.path.dirname(a.out), exist_ok=True)
                with open(a.out, "a") as fh:
                    fh.write(json.dumps(row) + "\n")
            del rep, cn
            torch.cuda.empty_cache()
        del sh, rep_prob, cn_prob
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
