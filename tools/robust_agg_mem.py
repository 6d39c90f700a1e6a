"""Time and peak transient memory of ``FLRunner.aggregate_robust`` alone, on synthetic client rows of a given size.

    python tools/robust_agg_mem.py --aggregator median --clients 128 [--params 2583873 --buffers 1928]

A bare runner (no engine, no data) gets ``clients`` rows of ``params`` + ``buffers`` fp32 (defaults: AlexNet3D) near a
common model, then aggregates ``--reps`` times.  Prints one JSON line: milliseconds per aggregation (CUDA events,
after one warm-up call) and the peak of ``torch.cuda.max_memory_allocated()`` above what the rows themselves hold.
Goes through the runner's method only, so it measures whichever implementation the tree has."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aggregator", default="median", choices=["krum", "multikrum", "median", "trimmed_mean"])
    ap.add_argument("--clients", type=int, default=128)
    ap.add_argument("--params", type=int, default=0)
    ap.add_argument("--buffers", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from neuroimagedisttraining_amd.engine.executor import FLConfig, FLRunner, padded_rows
    from neuroimagedisttraining_amd.engine.runner import StatInfo
    from neuroimagedisttraining_amd.parallel import runtime as rt
    if not args.params:
        from neuroimagedisttraining_amd.models.alexnet3d import AlexNet3D_Dropout
        with torch.device("meta"):
            m = AlexNet3D_Dropout(num_classes=1)
        args.params = sum(p.numel() for p in m.parameters())
        args.buffers = sum(b.numel() for b in m.buffers())
    dev = torch.device("cuda:0")
    N, P, Q = args.clients, args.params, args.buffers
    r = FLRunner.__new__(FLRunner)
    r.device, r.N, r.P, r.Q = dev, N, P, Q
    r.info = rt.DistInfo(0, 1, 0, dev, "none")
    r.cfg = FLConfig(aggregator=args.aggregator, byzantine_f=N // 8, trim_ratio=0.1)
    r.local = list(range(N))
    r.row_of = {c: c for c in range(N)}
    r.owner = np.zeros(N, dtype=np.int64)
    r.stat_info = StatInfo(lambda: None)
    g = torch.Generator(device=dev).manual_seed(0)
    r.w_global = torch.randn(P, device=dev, generator=g) * 0.05
    r.b_global = torch.zeros(Q, device=dev)
    r.theta, r.bufs = padded_rows(N, P, dev), padded_rows(N, Q, dev)
    for c in range(N):  # one row at a time: no [N, P] temporary
        r.theta[c, :P] = r.w_global + 1e-3 * torch.randn(P, device=dev, generator=g)
        r.bufs[c, :Q] = torch.rand(Q, device=dev, generator=g)
    sampled = list(range(N))
    r.aggregate_robust(sampled)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
    ev[0].record()
    for i in range(args.reps):
        r.aggregate_robust(sampled)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps))
    print(json.dumps({"aggregator": args.aggregator, "clients": N, "params": P, "buffers": Q,
                      "ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
                      "rows_gib": round(base / 2 ** 30, 3),
                      "peak_transient_gib": round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 30, 3),
                      "checksum": float(r.w_global.double().sum())}), flush=True)


if __name__ == "__main__":
    main()
