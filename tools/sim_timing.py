"""Time the device simulator against simulator.simulate (numpy, one core) on the same shapes in
one process, and append the result to profiles/sim_timing.jsonl.

    python tools/sim_timing.py [--launches 12] [--sizes c4,1250] [--out profiles/sim_timing.jsonl]

Shapes: C4 (5,451 bins x 10,000 S + 10,000 G1/2 cells) and 1,250 + 1,250 cells.  Device times are
host clocks around work that ends in a device synchronise, after one warm-up launch:
``kernels`` = pert_sim_cells + pert_sim_reads + pert_sim_normalise for the S and the G1/2
matrix with the inputs already on the device; ``end_to_end`` = simulate_matrix for both from
host arrays (uploads, allocation, the exhausted word read back).  The numpy time is one call
of simulate() (it has no warm-up to speak of).  There is no fallback: without a GPU it fails."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = {"c4": 10000, "1250": 1250}


def spread(ts):
    ts = np.asarray(ts) * 1e3
    return dict(n=len(ts), median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()),
                mean_ms=float(ts.mean()), std_ms=float(ts.std(ddof=1)) if len(ts) > 1 else 0.0)


def one_size(name, n_cells, launches):
    import torch
    from scdna_replication_tools_amd import _native as nat
    from scdna_replication_tools_amd import pert_simulator as ps
    from scdna_replication_tools_amd import simulator as sim

    lamb, betas, a, num_reads = 0.75, (0.5, 0.0), 10.0, 1e6
    t0 = time.perf_counter()
    ref = sim.simulate(n_s=n_cells, n_g=n_cells, num_reads=num_reads, lamb=lamb, betas=betas, a=a, seed=0)
    t_numpy = time.perf_counter() - t0
    L = ref.n_bins
    libs = np.zeros(n_cells, np.int32)
    u_s = num_reads / (1.5 * L * ref.cn_s.mean())
    u_g = num_reads / (L * ref.cn_g.mean())

    def end_to_end(seed):
        s = ps.simulate_matrix(ref.cn_s, ref.gc, libs, 1, betas, u_s, lamb, seed, rho=ref.rho_true, a=a,
                               num_reads=num_reads, cell0=0)
        g = ps.simulate_matrix(ref.cn_g, ref.gc, libs, 1, betas, u_g, lamb, seed, num_reads=num_reads, cell0=n_cells)
        torch.cuda.synchronize()
        return s, g

    s, g = end_to_end(1)                                                   # warm-up; its buffers serve the kernel timing
    assert s.exhausted == 0 and g.exhausted == 0
    t_e2e = []
    for i in range(launches):
        t0 = time.perf_counter()
        end_to_end(2 + i)
        t_e2e.append(time.perf_counter() - t0)

    lib, dev = nat.lib(), s.counts.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    f32 = lambda x: torch.as_tensor(np.ascontiguousarray(x, np.float32), device=dev)
    ldn = s.ldn
    cn_s, cn_g = torch.zeros((L, ldn), device=dev), torch.zeros((L, ldn), device=dev)
    cn_s[:, :n_cells], cn_g[:, :n_cells] = f32(ref.cn_s), f32(ref.cn_g)
    gc, rho, libs_d = f32(ref.gc), f32(ref.rho_true), torch.as_tensor(libs, device=dev)
    means, stds = f32([betas]), f32([ps.default_beta_stds(2)])
    exhausted = torch.zeros(1, dtype=torch.int32, device=dev)

    def kernels(seed):
        for m, cn, u, tau, rho_d, cell0 in ((s, cn_s, u_s, s.tau, rho, 0), (g, cn_g, u_g, None, None, n_cells)):
            m.colsum.zero_()
            p = lambda t: 0 if t is None else t.data_ptr()
            nat.check(lib.pert_sim_cells(n_cells, 2, 1, cell0, ctypes.c_uint64(seed), p(libs_d), p(means), p(stds),
                                         p(tau), p(m.betas), stream), "pert_sim_cells")
            nat.check(lib.pert_sim_reads(L, n_cells, ldn, 2, cell0, ctypes.c_uint64(seed), p(cn), p(gc), p(rho_d), p(tau),
                                         p(m.betas), float(u), a, lamb, p(m.counts), p(m.rep), p(m.p_rep), p(m.colsum),
                                         p(exhausted), stream), "pert_sim_reads")
            nat.check(lib.pert_sim_normalise(L, n_cells, ldn, num_reads, p(m.counts), p(m.colsum), p(m.reads_norm),
                                             stream), "pert_sim_normalise")
        torch.cuda.synchronize()

    kernels(1)
    t_k = []
    for i in range(launches):
        t0 = time.perf_counter()
        kernels(2 + i)
        t_k.append(time.perf_counter() - t0)
    assert int(exhausted.item()) == 0
    elements = 2 * L * n_cells
    rec = dict(size=name, bins=L, s_cells=n_cells, g_cells=n_cells, elements=elements, numpy_simulate_s=t_numpy,
               device_kernels=spread(t_k), device_end_to_end=spread(t_e2e),
               kernels_elements_per_s=elements / float(np.median(t_k)),
               speedup_kernels=t_numpy / float(np.median(t_k)), speedup_end_to_end=t_numpy / float(np.median(t_e2e)),
               mean_count_s=float(s.colsum.double().mean().item() / L), device=torch.cuda.get_device_name(dev))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--sizes", default="c4,1250")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_timing.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sim_timing needs a GPU: a time taken elsewhere says nothing about it")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.sizes.split(","):
        rec = one_size(name, SIZES[name], args.launches)
        rec["launches"] = args.launches
        rec["when"] = time.strftime("%Y-%m-%dT%H:%M:%S")
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
