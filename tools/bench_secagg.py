"""Timing of the aggregate phase of a round under ``--aggregator secure`` (``secagg.hip``) against the plain FedAvg
aggregate, on one GPU at the AlexNet3D round shape: 64 client rows x (P parameters + Q buffers) fp32.

A bare runner (no engine, no data) holds the rows; every variant goes through ``FLRunner.aggregate`` /
``aggregate_fedavg``, host work included (peer lists, key reconstruction, pinned uploads), so it measures whichever
implementation the tree has.  The variants alternate inside every repetition; a window is one call between a host clock
start and a device synchronise, and the median over ``--reps`` windows is reported.

A second table gives the kernel cost with remote peers: ``secagg_masked_sum`` over the ``clients / shards`` rows one
rank of an emulated ``--shards``-way sharding holds (every other participant is a remote peer whose mask has to be
generated), plus ``secagg_finish``, between device events.

Usage: python tools/bench_secagg.py [--clients 64] [--shards 8] [--reps 9] [--dropout 0.25] [--out FILE]"""
from __future__ import annotations

import argparse
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bare_runner(N, P, Q, dev, rows=None, **cfg_kw):
    """An ``FLRunner`` with rows but no engine or data; ``rows``: another bare runner whose row matrices it shares."""
    from neuroimagedisttraining_amd.engine.executor import FLConfig, FLRunner, padded_rows
    from neuroimagedisttraining_amd.engine.runner import StatInfo
    from neuroimagedisttraining_amd.parallel import runtime as rt
    r = FLRunner.__new__(FLRunner)
    r.device, r.N, r.P, r.Q, r.alg, r.mask, r.log = dev, N, P, Q, "fedavg", None, None
    r.info = rt.DistInfo(0, 1, 0, dev, "none")
    r.cfg = FLConfig(seed=1, **cfg_kw)
    r.local = list(range(N))
    r.row_of = {c: c for c in range(N)}
    r.owner = np.zeros(N, dtype=np.int64)
    r.sizes = np.array([150 + 7 * (c % 9) for c in range(N)], dtype=np.int64)
    r._pending_metrics, r._pinned_free = [], []
    r.stat_info = StatInfo(r._flush_metrics)
    r.w_global = torch.zeros(P, device=dev)
    r.b_global = torch.zeros(Q, device=dev)
    r.theta, r.bufs = (rows.theta, rows.bufs) if rows is not None else (padded_rows(N, P, dev), padded_rows(N, Q, dev))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--params", type=int, default=0)
    ap.add_argument("--buffers", type=int, default=0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dropout", type=float, default=0.25)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_secagg.py measures on a GPU; none is available")
    from neuroimagedisttraining_amd.algorithms.turboaggregate import saturation_bound
    from neuroimagedisttraining_amd.engine import secagg as SA
    if not a.params:
        from neuroimagedisttraining_amd.models.alexnet3d import AlexNet3D_Dropout
        with torch.device("meta"):
            m = AlexNet3D_Dropout(num_classes=1)
        a.params = sum(p.numel() for p in m.parameters())
        a.buffers = sum(b.numel() for b in m.buffers())
    dev = torch.device("cuda:0")
    N, P, Q = a.clients, a.params, a.buffers
    kinds = [("fedavg (weighted_rows_sum)", dict()),
             ("secure, fused", dict(aggregator="secure")),
             ("secure, fused, dropout %.2f" % a.dropout, dict(aggregator="secure", secagg_dropout=a.dropout)),
             ("secure, secagg_fuse=0", dict(aggregator="secure", secagg_fuse=False)),
             ("secure, secagg_fuse=0, dropout %.2f" % a.dropout,
              dict(aggregator="secure", secagg_fuse=False, secagg_dropout=a.dropout))]
    base = bare_runner(N, P, Q, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    w = torch.randn(P, device=dev, generator=g) * 0.05
    for c in range(N):  # one row at a time: no [N, P] temporary
        base.theta[c, :P] = w + 1e-3 * torch.randn(P, device=dev, generator=g)
        base.bufs[c, :Q] = torch.rand(Q, device=dev, generator=g)
    runners = [(name, bare_runner(N, P, Q, dev, rows=base, **kw)) for name, kw in kinds]
    sampled = list(range(N))
    times = {name: [] for name, _ in kinds}
    for rep in range(a.reps + 1):  # repetition 0 warms up: code objects, allocator, the key setup
        for name, r in runners:
            r._round_idx = rep
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.aggregate(sampled)
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) * 1e3)
            r._flush_metrics()
    ref = runners[0][1].w_global.double()
    prop = torch.cuda.get_device_properties(0)
    lines = ["aggregate phase of one round, %d clients x (P = %d + Q = %d) fp32 rows (%.0f MB), one process, %s"
             % (N, P, Q, N * (P + Q) * 4 / 1e6, torch.cuda.get_device_name(0)),
             "box: host %s, %s, %d CUs, torch %s, HIP %s"
             % (platform.node(), prop.gcnArchName, prop.multi_processor_count, torch.__version__, torch.version.hip),
             "host clock around FLRunner.aggregate ending in a device synchronise; median of %d alternating windows, "
             "min .. max in brackets" % a.reps]
    t_base = None
    for name, r in runners:
        ts = sorted(times[name])
        med = ts[len(ts) // 2]
        t_base = med if t_base is None else t_base
        lines.append("%-38s %9.3f ms [%.3f .. %.3f]  %6.2fx fedavg   max |w - fedavg w| %.3g   saturated %s dropped %s"
                     % (name, med, ts[0], ts[-1], med / t_base, float((r.w_global.double() - ref).abs().max()),
                        r.stat_info.get("secagg_saturated", "-"), r.stat_info.get("secagg_dropped", "-")))
    same = all(torch.equal(runners[i][1].w_global, runners[i + 2][1].w_global)
               and torch.equal(runners[i][1].b_global, runners[i + 2][1].b_global) for i in (1, 2))
    lines.append("fused and secagg_fuse=0 results bit-identical: %s" % same)

    # ---- kernel cost with remote peers: one rank of an emulated sharding
    keys = runners[1][1]._secagg_keys
    C = max(1, N // a.shards)
    B = saturation_bound(N)
    n_tot = float(base.sizes.sum())
    mine = list(range(C))
    wts = [int(base.sizes[c]) / n_tot for c in mine]
    out = torch.zeros(P, dtype=torch.int64, device=dev)
    res = torch.zeros(P, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines.append("")
    lines.append("kernels alone (device events, parameters segment): %d local rows of %d participants" % (C, N))
    dropped = list(range(N - int(a.dropout * N), N))
    alive = [c for c in range(N) if c not in dropped]
    cases = [("masked_sum, no remote peers", [[] for _ in mine]),
             ("masked_sum, %d remote peers per row" % (N - C),
              [[(j, int(keys.key[c, j])) for j in range(N) if j >= C] for c in mine])]
    for name, peers in cases:
        ts = []
        for rep in range(a.reps + 1):
            e0.record()
            SA.masked_sum(base.theta, mine, P, mine, peers, wts, rep, 0, 2 ** 16, B, out, hip=True)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = sorted(ts[1:])
        npeer = sum(len(p) for p in peers)
        lines.append("%-38s %9.3f ms [%.3f .. %.3f]  %.2f TB/s of row bytes, %.1f G masks/s"
                     % (name, ts[len(ts) // 2], ts[0], ts[-1], C * P * 4 / ts[len(ts) // 2] / 1e9,
                        npeer * P / ts[len(ts) // 2] / 1e6))
    for name, pairs in (("finish, no dropped clients", []),
                        ("finish, %d survivors x %d dropped" % (len(alive), len(dropped)),
                         keys.removal_pairs(dropped, alive))):
        ts = []
        for rep in range(a.reps + 1):
            e0.record()
            SA.finish(out, P, pairs, rep, 0, 2 ** 16, 1.0, res, hip=True)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = sorted(ts[1:])
        lines.append("%-38s %9.3f ms [%.3f .. %.3f]  %.1f G masks/s"
                     % (name, ts[len(ts) // 2], ts[0], ts[-1], len(pairs) * P / ts[len(ts) // 2] / 1e6))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
