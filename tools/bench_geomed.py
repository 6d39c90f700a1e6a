"""Timing of one Weiszfeld pass of ``--aggregator geomed`` on the fused kernel (``rows_geomed_step`` +
``geomed_weights``, ``robust.hip``) against the same pass composed from the kernels the tree had before it:
``weighted_rows_sum`` (``optim.hip``) for ``z``, then ``rows_diff_norm`` (``defense.hip``) for the K distances to it -
two reads of the K x P row matrix instead of one.  One GPU, one process, at 64 rows of AlexNet3D's parameter count
and 100 rows of vgg11's.

The two variants alternate inside every repetition; a window is one pass between two device events, and the median
over ``--reps`` windows is reported with [min .. max].  The fused pass's bytes are K * P * 4 (every element once).

Usage: python tools/bench_geomed.py [--reps 15] [--out FILE]"""
from __future__ import annotations

import argparse
import os
import platform
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TBS = 8.0  # MI355X HBM3E peak bandwidth, TB/s (vendor figure)


def param_count(name):
    with torch.device("meta"):
        if name == "AlexNet3D":
            from neuroimagedisttraining_amd.models.alexnet3d import AlexNet3D_Dropout
            m = AlexNet3D_Dropout(num_classes=1)
        else:
            from neuroimagedisttraining_amd.models.zoo2d import vgg11
            m = vgg11(10)
    return sum(p.numel() for p in m.parameters())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geomed.py measures on a GPU; none is available")
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine import robust as RB
    from neuroimagedisttraining_amd.engine.executor import padded_rows
    dev = torch.device("cuda:0")
    m, st = ops.ext(), ops.stream()
    prop = torch.cuda.get_device_properties(0)
    lines = ["one Weiszfeld pass (z = sum beta_i x_i and the K distances |x_i - z|), fp32 rows, one process, %s"
             % torch.cuda.get_device_name(0),
             "box: host %s, %s, %d CUs, torch %s, HIP %s"
             % (platform.node(), prop.gcnArchName, prop.multi_processor_count, torch.__version__, torch.version.hip),
             "fused: rows_geomed_step + geomed_weights.  composed: weighted_rows_sum + rows_diff_norm (both from the "
             "tree before this kernel; the composed z is an FMA chain, so its bits differ from the fused z)",
             "device events around one pass; median of %d alternating windows, min .. max in brackets; "
             "HBM peak %.1f TB/s" % (a.reps, PEAK_TBS)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, K in (("AlexNet3D", 64), ("vgg11", 100)):
        P = param_count(name)
        rows = padded_rows(K, P, dev)
        g = torch.Generator(device=dev).manual_seed(0)
        w = torch.randn(P, device=dev, generator=g) * 0.05
        for c in range(K):  # one row at a time: no [K, P] temporary
            rows[c, :P] = w + 1e-3 * torch.randn(P, device=dev, generator=g)
        ridx = torch.arange(K, dtype=torch.int32, device=dev)
        beta = torch.rand(K, device=dev, generator=g)
        beta = (beta / beta.sum()).contiguous()
        alpha = torch.full((K,), 1.0 / K, dtype=torch.float64, device=dev)
        z, dsq = torch.zeros(P, device=dev), torch.zeros(K, dtype=torch.float64, device=dev)
        zc, norm = torch.zeros(P, device=dev), torch.zeros(K, device=dev)
        part = torch.empty(K * m.rows_diff_norm_blocks(P), dtype=torch.float64, device=dev)

        def fused():
            RB.geomed_step(rows, ridx, P, beta, z, dsq, hip=True)
            RB.geomed_weights(dsq, alpha, 1e-6, hip=True)

        def composed():
            m.weighted_rows_sum(rows.data_ptr(), beta.data_ptr(), K, P, rows.stride(0), 0.0, zc.data_ptr(), st)
            m.rows_diff_norm(rows.data_ptr(), zc.data_ptr(), K, P, rows.stride(0), part.data_ptr(), norm.data_ptr(),
                             st)

        times = {"fused": [], "composed": []}
        for rep in range(a.reps + 2):  # the first two repetitions warm up: code objects, allocator
            for key, fn in (("fused", fused), ("composed", composed)):
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep >= 2:
                    times[key].append(e0.elapsed_time(e1))
        dz = float((z - zc).abs().max())
        dd = float((dsq.sqrt() - norm.double()).abs().max() / norm.double().max())
        lines.append("")
        lines.append("%s: K = %d rows x P = %d (%.0f MB); max |z fused - z composed| %.3g, distances agree to %.3g"
                     % (name, K, P, K * P * 4 / 1e6, dz, dd))
        med = {}
        for key in ("fused", "composed"):
            ts = sorted(times[key])
            med[key] = ts[len(ts) // 2]
            lines.append("  %-9s %9.3f ms [%.3f .. %.3f]  %.2f TB/s of K*P*4 bytes (%.0f %% of peak)"
                         % (key, med[key], ts[0], ts[-1], K * P * 4 / med[key] / 1e9,
                            100 * K * P * 4 / med[key] / 1e9 / PEAK_TBS))
        lo_c, hi_c = min(times["composed"]), max(times["composed"])
        where = "below (faster)" if med["fused"] < lo_c else "above (SLOWER)" if med["fused"] > hi_c else "INSIDE"
        lines.append("  fused / composed = %.2f; the fused median lies %s the composed [min .. max]"
                     % (med["fused"] / med["composed"], where))
        del rows
    lines += ["", "Not measured: several ranks (the per-pass re-gather of every chunk), the whole rule inside a round, "
              "other K or row lengths, kernel times from a profiler (these are event windows that include the "
              "launches and the small finish kernels), and whether the fused pass is bound by HBM or by its LDS "
              "phases."]
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
