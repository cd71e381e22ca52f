"""Time of the cell-cycle-classifier features (ccc_features.py): the pert_ccc_features launch,
features_matrix end to end, the share of flagged cells, and the per-cell sklearn loop.

    python tools/ccc_timing.py [--shapes genome] [--out profiles/ccc_timing.jsonl]

One process.  Per shape (bins x cells of simulated S-phase reads over the G1/2 pseudobulk median,
float64, with random copy-number states on 23 chromosomes): the kernel timed with device events (3
warm-up launches, 10 timed ones into the same buffers, median and min), the share of cells it flags
and which bits, ``features_matrix(device='cuda')`` once from host arrays (upload, launch, download,
host path for the flagged cells), and the reference-style per-cell loop (two GaussianMixture fits,
the median, the per-chromosome breakpoints, three column writes) on a slice of the same cells.
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

from scdna_replication_tools_amd import _native as nat        # noqa: E402
from scdna_replication_tools_amd import ccc_features as F      # noqa: E402
from scdna_replication_tools_amd import simulator               # noqa: E402

SHAPES = {"small": (271, 400), "genome": (5451, 2000), "tiny": (96, 32)}
WARMUP, REPS = 3, 10
SLICE = 32


def profiles(L, N, seed=0):
    sim = simulator.simulate(N, min(N, 256), n_bins=L, seed=seed)
    X = sim.reads_s.astype(np.float64) / np.median(sim.reads_g.astype(np.float64), axis=1)[:, None]
    rng = np.random.default_rng(seed + 1)
    state = 2 + (rng.uniform(size=(L, N)) < 0.002).cumsum(0) % 3
    chrom = np.repeat((np.arange(L) * 23 // L)[:, None], N, 1)
    return X, state, chrom


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="genome")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ccc_timing needs a GPU")
    warnings.simplefilter("ignore")
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    for name in a.shapes.split(","):
        L, N = SHAPES[name]
        X, state, chrom = profiles(L, N)
        base = dict(shape=name, L=L, N=N)
        stream_draws = F._Stream(0, N)
        p = F.ccc_params(L)
        rows_d = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()                   # (N, L): one row per cell
        st_d = torch.from_numpy(np.ascontiguousarray(state.T)).to(torch.int32).cuda()
        ch_d = torch.from_numpy(np.ascontiguousarray(chrom.T)).to(torch.int32).cuda()
        first = torch.from_numpy(F.first_centres(stream_draws.draws[:, :2].reshape(-1), L).reshape(N, 2).T.copy()).cuda()
        u = torch.from_numpy(np.ascontiguousarray(stream_draws.draws[:, 2:])).cuda()
        scratch = torch.empty((2, N, L), dtype=torch.int8, device="cuda")
        outs = [torch.empty(N, dtype=torch.float64, device="cuda") for _ in range(4)]
        outs += [torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(2)]
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        ms = launch_ms(lambda: nat.check(nat.lib().pert_ccc_features(
            L, N, rows_d.data_ptr(), first[0].data_ptr(), first[1].data_ptr(), u.data_ptr(), st_d.data_ptr(),
            ch_d.data_ptr(), ctypes.byref(p), scratch.data_ptr(), *[o.data_ptr() for o in outs], stream),
            "pert_ccc_features"))
        flags = outs[5].cpu().numpy()
        emit(what="pert_ccc_features launch", median_ms=round(float(np.median(ms)), 3),
             min_ms=round(float(ms.min()), 3), us_per_cell=round(float(np.median(ms)) * 1e3 / N, 2), **base)
        emit(what="flagged cells", flagged=int((flags != 0).sum()), share=round(float((flags != 0).mean()), 4),
             by_bit={str(b): int(((flags & b) != 0).sum()) for b in (1, 2, 4)}, **base)
        del rows_d, st_d, ch_d, scratch
        torch.cuda.empty_cache()

        t0 = time.perf_counter()
        res = F.features_matrix(X, state, chrom, random_state=0, device="cuda")
        t1 = time.perf_counter()
        emit(what="features_matrix cuda end to end", seconds=round(t1 - t0, 4), host_path_cells=int(res.flagged.sum()),
             **base)

        import pandas as pd
        from sklearn.mixture import GaussianMixture
        sl = min(SLICE, N)
        cn = pd.DataFrame({"cell_id": np.repeat(np.arange(sl), L), "chr": chrom[:, :sl].T.reshape(-1),
                           "x": X[:, :sl].T.reshape(-1), "state": state[:, :sl].T.reshape(-1)})
        np.random.seed(0)
        t0 = time.perf_counter()
        for _, cell in cn.groupby("cell_id"):
            x = cell["x"].values.reshape(-1, 1)
            s1 = GaussianMixture(n_components=1).fit(x).score(x)
            s2 = GaussianMixture(n_components=2).fit(x).score(x)
            cn.loc[cell.index, "madn"] = np.median(np.abs(np.diff(cell["x"].values)))
            cn.loc[cell.index, "lrs"] = -2 * (s1 - s2)
            cn.loc[cell.index, "breakpoints"] = sum(int((np.diff(c["state"].values) != 0).sum())
                                                    for _, c in cell.groupby("chr"))
        t1 = time.perf_counter()
        emit(what="per-cell sklearn loop with per-cell column writes", cells=sl, seconds=round(t1 - t0, 3),
             ms_per_cell=round((t1 - t0) * 1e3 / sl, 2), **base)
        per = cn.groupby("cell_id").first()
        emit(what="loop vs features_matrix on the slice", madn_equal=bool((per["madn"].to_numpy() == res.madn[:sl]).all()),
             breakpoints_equal=bool((per["breakpoints"].to_numpy() == res.breakpoints[:sl]).all()),
             lrs_max_abs_diff=float(np.max(np.abs(per["lrs"].to_numpy() - res.lrs[:sl]))), **base)

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
