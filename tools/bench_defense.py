"""Timing of the defended aggregation partial (``defense.hip``: ``rows_diff_norm`` + ``clipped_rows_sum``, clipping only
and weak-DP) against the plain FedAvg partial (``optim.hip`` ``weighted_rows_sum``) on one GPU, at the AlexNet3D row
shape: 64 client rows x P = 2,570,241 fp32 (658 MB, more than the 256 MiB Infinity Cache, so every pass streams from
HBM).  Half of the rows are clipped.  The three variants alternate inside every repetition; each timed window is
``--inner`` back-to-back calls between two device events; the median over ``--reps`` windows is reported together with
the effective rate over the bytes the variant has to read (one pass over the rows for FedAvg, two for the defence).

Usage: python tools/bench_defense.py [--rows 64] [--P 2570241] [--reps 15] [--inner 10] [--out FILE]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--P", type=int, default=2570241)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_defense.py measures on a GPU; none is available")
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine import defense as DF
    from neuroimagedisttraining_amd.engine.executor import padded_rows
    dev = torch.device("cuda")
    m = ops.ext()
    C, P = a.rows, a.P
    g = torch.Generator(device=dev).manual_seed(0)
    ref = torch.randn(P, device=dev, generator=g)
    rows = padded_rows(C, P, dev)
    scale = torch.where(torch.arange(C, device=dev) % 2 == 0, 1e-4, 1e-2).view(-1, 1)
    rows.copy_(ref + scale * torch.randn(C, P, device=dev, generator=g))
    wts = torch.full((C,), 1.0 / C, device=dev)
    cids = torch.arange(C, dtype=torch.int32, device=dev)
    Pp = (P + 63) // 64 * 64
    out = torch.zeros(Pp, device=dev)
    bound = 1.0  # norms: 1e-4 * sqrt(P) = 0.16 (kept) and 16 (clipped)

    def fedavg():
        m.weighted_rows_sum(rows.data_ptr(), wts.data_ptr(), C, P, rows.stride(0), 0.0, out.data_ptr(), ops.stream())

    def defended(stddev):
        def f():
            norm = DF.rows_diff_norm(rows, ref, hip=True)
            DF.clipped_rows_sum(rows, ref, wts, norm, cids, bound, stddev, 12345, out, hip=True)
        return f

    def norm_only():
        DF.rows_diff_norm(rows, ref, hip=True)

    variants = [("fedavg weighted_rows_sum", fedavg, 1), ("rows_diff_norm alone", norm_only, 1),
                ("norm_diff_clipping (norm + clipped sum)", defended(0.0), 2),
                ("weak_dp (norm + clipped sum + noise)", defended(0.025), 2)]
    for _, fn, _ in variants:  # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    norm = DF.rows_diff_norm(rows, ref, hip=True)
    clipped = int((norm > bound).sum())
    times = {name: [] for name, _, _ in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.reps):
        for name, fn, _ in variants:
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.inner)
    lines = ["defended aggregation partial, %d rows x P = %d fp32 (%.0f MB), %d rows clipped, %s"
             % (C, P, C * P * 4 / 1e6, clipped, torch.cuda.get_device_name(0)),
             "median of %d windows of %d calls (device events); min .. max in brackets" % (a.reps, a.inner)]
    base = None
    for name, _, passes in variants:
        ts = sorted(times[name])
        med = ts[len(ts) // 2]
        base = med if base is None else base
        lines.append("%-42s %8.3f ms [%.3f .. %.3f]  %5.2fx fedavg  %5.2f TB/s over %d pass(es) of the rows"
                     % (name, med, ts[0], ts[-1], med / base, passes * C * P * 4 / med / 1e9, passes))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
