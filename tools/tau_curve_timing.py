"""Time pert_enum_evidence and pert_tau_curve against pert_enum_posterior on the same shard
(device events), and measure the curve's error at genome length.

    python tools/tau_curve_timing.py [--cells 10000 1250] [--launches 12] [--grid 99]
                                     [--out profiles/tau_curve_timing.jsonl]

The posterior pass is the yardstick of the evidence pass: it streams the same reads and pi
logits and evaluates the same scores.  For each shape -- seeded simulator.simulate inputs on the
5,451-bin grid, P = 13, the g1_clones prior, 20 SVI steps from the initial values so the logits
are no longer uniform -- the three kernels are warmed up and then launched alternately, each
launch between its own pair of events.  One JSON row per shape is appended to --out: median and
range in milliseconds of the three kernels, the evidence pass over the posterior pass, the curve
kernel's (element, grid point) rate, the bytes it re-reads, and its time over the floor of its
instruction count.

Accuracy: on 64 sampled cells of the full-length shard (the first, the last and 62 seeded ones,
as test_gpu_configs samples cells) the row records max |curve_dev - curve_fp64| over the grid,
where curve_fp64 is the fp64 oracle (oracle.enum_score_terms) at the shard's parameters, next
to the worst-case cell bound of tests/_curve_bounds.py.
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
CURVE_CHUNK = 4            # curve_kernels.hip kCurveChunk: grid points per wave
# MI355X: 256 CUs x 4 SIMDs at 2.4 GHz; a SIMD issues a wave64 fp32 VALU instruction (fma, convert)
# over 2 cycles, a transcendental (v_log_f32) and an fp64 add over 4 (half the fp32 rate: 78.6 of
# 157.3 vector TFLOP/s).  The floor is the instruction count the factorisation allows per
# (element, grid point) -- one fma, one transcendental log, one convert, one fp64 add -- not the
# count of tau_mix's overflow-safe form, which the kernel runs.
SIMD_RATE = 256 * 4 * 2.4e9
FLOOR_CYCLES_PER_WAVE = 2 + 4 + 2 + 4


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
    sh = PertShard(nat.KIND_STEP2, reads, sim.gc, libs, 1, P, K, init, eta=eta, lamb=0.75, beta_means=bm,
                   device="cuda")
    return sh, dict(reads=reads, gc=sim.gc, libs=libs, states=states, bm=bm, t_init=t_init)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def accuracy(sh, data, grid, curve_dev, n_sample: int, seed: int):
    """max |curve_dev - curve_fp64| over the grid on sampled cells, and the worst cell bound."""
    from oracle import pert_oracle as po
    from tests import _curve_bounds as cb
    N = sh.N
    rng = np.random.default_rng(seed)
    cells = np.unique(np.r_[0, N - 1, rng.choice(N, size=min(n_sample, N) - 2, replace=False)])
    z = sh.unconstrained(pi_cells=cells)
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    etas = np.ones((sh.L, cells.size, P), np.float32)
    np.put_along_axis(etas, data["states"][:, cells][..., None], 1e6, axis=2)
    prob = po.OracleProblem(kind="step2", reads=t64(data["reads"][:, cells]), gc=t64(np.asarray(data["gc"], np.float32)),
                            libs=torch.tensor(data["libs"][cells], dtype=torch.long), n_libs=1, P=P, K=K,
                            etas=t64(etas), lamb=t64([np.float32(0.75)]), beta_means=t64(data["bm"]),
                            t_init=t64(data["t_init"][cells]))
    zs = {k: t64(v) for k, v in z.items()}
    for k in ("expose_u", "expose_tau"):
        zs[k] = zs[k][cells]
    zs["expose_betas"] = zs["expose_betas"][cells]
    ref = cb.oracle_evidence(prob, zs)
    want, bound = cb.curve(ref, grid.astype(np.float64))
    err = np.abs(curve_dev[:, cells] - want)
    rng_cell = want.max(0) - want.min(0)
    return {"sampled_cells": int(cells.size), "max_abs_err": float(err.max()), "median_abs_err": float(np.median(err.max(0))),
            "worst_cell_bound": float(bound.max()), "median_curve_range": float(np.median(rng_cell)),
            "max_err_over_range": float((err.max(0) / rng_cell).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[10000, 1250])
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", type=int, default=99)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tau_curve_timing.jsonl"))
    a = ap.parse_args()
    if a.launches < 10:
        raise SystemExit("--launches: at least 10 per kernel")
    if not torch.cuda.is_available():
        raise SystemExit("tau_curve_timing needs a GPU")
    from scdna_replication_tools_amd import _native as nat
    for n_cells in a.cells:
        sh, data = make_shard(n_cells, a.seed)
        for _ in range(20):
            sh.step_async()
        sh.decode()
        L, N, ldn, dev = sh.L, sh.N, sh.ldn, sh.device
        rep_prob = torch.zeros((L, ldn), dtype=torch.float32, device=dev)
        cn_prob = torch.zeros_like(rep_prob)
        ev = torch.zeros((2, L, ldn), dtype=torch.float32, device=dev)
        grid = np.linspace(0.01, 0.99, a.grid).astype(np.float32)
        grid_d = torch.as_tensor(grid, device=dev)
        curve = torch.zeros((a.grid, N), dtype=torch.float64, device=dev)
        at_fit = torch.zeros(N, dtype=torch.float64, device=dev)
        stream = sh._stream()
        prob, state = ctypes.byref(sh._prob), ctypes.byref(sh._state)

        def post():
            nat.check(sh.lib.pert_enum_posterior(prob, state, sh.cn_out.data_ptr(), rep_prob.data_ptr(),
                                                 cn_prob.data_ptr(), 0, stream), "pert_enum_posterior")

        def evid():
            nat.check(sh.lib.pert_enum_evidence(prob, state, ev.data_ptr(), stream), "pert_enum_evidence")

        def curv():
            nat.check(sh.lib.pert_tau_curve(prob, state, ev.data_ptr(), grid_d.data_ptr(), a.grid, curve.data_ptr(),
                                            at_fit.data_ptr(), stream), "pert_tau_curve")
        fns = {"posterior": post, "evidence": evid, "curve": curv}
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        evs = {k: [] for k in fns}
        for _ in range(a.launches):
            for k, fn in fns.items():
                evs[k].append(timed(fn))
        torch.cuda.synchronize()
        ms = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in evs.items()}
        med = {k: float(np.median(v)) for k, v in ms.items()}
        points = float(L) * N * a.grid
        chunks = -(-a.grid // CURVE_CHUNK)
        floor_ms = points / 64 * FLOOR_CYCLES_PER_WAVE / SIMD_RATE * 1e3
        row = {"tool": "tau_curve_timing", "device": torch.cuda.get_device_name(dev), "cells": n_cells, "bins": L,
               "P": P, "G": a.grid, "bins_per_tile": sh.bins_per_tile, "launches": a.launches,
               "posterior": stats(ms["posterior"]), "evidence": stats(ms["evidence"]), "curve": stats(ms["curve"]),
               "evidence_over_posterior": round(med["evidence"] / med["posterior"], 3),
               "curve_points_per_s": round(points / (med["curve"] * 1e-3), 1),
               "curve_bytes_reread": int(chunks * 8 * L * ldn),
               "curve_floor_ms": round(floor_ms, 4), "curve_floor_fraction": round(floor_ms / med["curve"], 4),
               "lib": sh.lib.pert_version().decode()}
        if not a.no_accuracy:
            row["accuracy"] = accuracy(sh, data, grid, curve.cpu().numpy(), a.sample, a.seed)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
        del sh, rep_prob, cn_prob, ev, curve, at_fit
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
