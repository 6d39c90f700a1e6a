"""Timing of the client-grouped Linear layers of the 2-D model zoo: linear_g.hip (forward, data gradient, weight
gradient on the fp32 rows in place) against the batched library GEMM the engine ran before (autocast ``baddbmm`` over
the strided weight views plus ``torch.autograd.grad``), alternating inside every repetition; then one
``BatchedModuleEngine.train_step`` of cnn_cifar10 with NIDT_B2D_LINEAR = 1 and 0.
Usage: python tools/bench_linear.py [--out FILE] [--reps N]"""
import argparse
import os
import socket
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ZOO = [("cnn_cifar10", 1600, 384), ("cnn_cifar10", 384, 192), ("cnn_cifar10", 192, 10), ("lenet5", 800, 500),
       ("lenet5", 500, 10), ("LeNet5_cifar", 400, 120), ("LeNet5_cifar", 120, 84), ("LeNet5_cifar", 84, 10),
       ("vgg11", 512, 10)]
INNER = 20  # calls per timed window


def window(fn):
    """Device time of one call, from events around INNER back-to-back calls (ms)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


def alternate(fns, reps):
    """{name: median ms} of the variants, every repetition running each of them once in turn."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(window(fn))
    return {k: statistics.median(v) for k, v in ts.items()}


def bench_layer(G, B, K, N, reps):
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine.conv2d_hip import HipLinearFn
    m, s, dev = ops.ext(), ops.stream(), "cuda"
    ld = 3 + N * K + N + 7  # the blocks at 4-byte-aligned offsets inside a row, as in theta
    theta = torch.randn(G, ld, device=dev) * K ** -0.5
    w = theta[:, 3:3 + N * K].view(G, N, K).requires_grad_(True)
    b = theta[:, 3 + N * K:3 + N * K + N].requires_grad_(True)
    x = torch.randn(G * B, K, device=dev).to(torch.bfloat16).requires_grad_(True)
    dy = torch.randn(G * B, N, device=dev).to(torch.bfloat16)
    y = torch.empty(G * B, N, device=dev, dtype=torch.bfloat16)
    dx = torch.empty(G * B, K, device=dev, dtype=torch.bfloat16)
    dw = torch.empty(G, N, K, device=dev)
    db = torch.empty(G, N, device=dev)

    def lib_fwd():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return torch.baddbmm(b.unsqueeze(1), x.view(G, B, K), w.transpose(1, 2))

    def lib_step():
        return torch.autograd.grad(lib_fwd(), [x, w, b], dy.view(G, B, N))

    def hip_step():
        return torch.autograd.grad(HipLinearFn.apply(x, w, b, G), [x, w, b], dy)

    ref, got = lib_step(), hip_step()
    assert all(g.data_ptr() != r.data_ptr() for g, r in zip(got, ref))  # two results, not one tensor twice
    ndiff = int((got[0].view(ref[0].shape) != ref[0]).sum())
    rel = [float((g.float() - r.float()).norm() / r.float().norm()) for g, r in zip(got, ref)]
    t = alternate({
        "lib_fwd": lib_fwd, "hip_fwd": lambda: HipLinearFn.apply(x, w, b, G), "lib_step": lib_step,
        "hip_step": hip_step,
        "k_fwd": lambda: m.linear_g_fwd(x.data_ptr(), w.data_ptr(), ld, b.data_ptr(), ld, y.data_ptr(), G, B, K, N, s),
        "k_dgrad": lambda: m.linear_g_dgrad(dy.data_ptr(), w.data_ptr(), ld, dx.data_ptr(), G, B, K, N, s),
        "k_wgrad": lambda: m.linear_g_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), N * K, db.data_ptr(), N, G, B,
                                            K, N, s)}, reps)
    wbytes = 4.0 * G * N * K
    return ("%4d->%-4d G=%3d B=%2d | library fwd %.3f fwd+bwd %.3f | HipLinearFn fwd %.3f fwd+bwd %.3f (%.2fx) | "
            "kernels fwd %.3f dgrad %.3f wgrad %.3f ms = %.2f %.2f %.2f TB/s of fp32 weight bytes | "
            "rel dx %.1e (%d of %d elements differ) dw %.1e db %.1e"
            % (K, N, G, B, t["lib_fwd"], t["lib_step"], t["hip_fwd"], t["hip_step"], t["lib_step"] / t["hip_step"],
               t["k_fwd"], t["k_dgrad"], t["k_wgrad"], wbytes / t["k_fwd"] / 1e9, wbytes / t["k_dgrad"] / 1e9,
               wbytes / t["k_wgrad"] / 1e9, rel[0], ndiff, G * B * K, rel[1], rel[2]))


def bench_step(G, B, reps):
    """Host clock around train_step ending in a device synchronise, the two settings alternating."""
    from neuroimagedisttraining_amd.engine.batched2d import BatchedModuleEngine
    from neuroimagedisttraining_amd.engine.executor import padded_rows
    from neuroimagedisttraining_amd.engine.resnet2d_hip import CIFAR_MEAN, CIFAR_STD, synthetic_cifar
    from neuroimagedisttraining_amd.models import create_model
    torch.manual_seed(0)
    model = create_model("cnn_cifar10", dataset="cifar10", class_num=10)
    x8, y = synthetic_cifar(G * B, seed=1)
    eng = BatchedModuleEngine(model, x8, y, "cuda", CIFAR_MEAN, CIFAR_STD)
    theta = padded_rows(G, eng.players.total, "cuda")
    theta.copy_(torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cuda().expand(G, -1))
    grads = padded_rows(G, eng.players.total, "cuda")
    idx = torch.arange(G * B, dtype=torch.int32, device="cuda")
    ts = {"1": [], "0": []}
    before = os.environ.get("NIDT_B2D_LINEAR")
    for rep in range(reps + 2):  # two warm-up rounds
        for v in ts:
            os.environ["NIDT_B2D_LINEAR"] = v
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                eng.train_step(theta, None, grads, idx, G, B, 1.0, 7)
            torch.cuda.synchronize()
            if rep >= 2:
                ts[v].append((time.perf_counter() - t0) / 5 * 1e3)
    if before is None:
        del os.environ["NIDT_B2D_LINEAR"]
    else:
        os.environ["NIDT_B2D_LINEAR"] = before
    med = {v: statistics.median(t) for v, t in ts.items()}
    return ("cnn_cifar10 train_step G=%d B=%d: NIDT_B2D_LINEAR=1 %.3f ms [%.3f .. %.3f]   =0 %.3f ms [%.3f .. %.3f]   "
            "kernels / library = %.3f" % (G, B, med["1"], min(ts["1"]), max(ts["1"]), med["0"], min(ts["0"]),
                                          max(ts["0"]), med["1"] / med["0"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear: needs the GPU")
    p = torch.cuda.get_device_properties(0)
    lines = ["box: host %s, %s, %d CUs, torch %s, HIP %s, %s" % (socket.gethostname(), p.gcnArchName,
                                                                 p.multi_processor_count, torch.__version__,
                                                                 torch.version.hip, time.strftime("%Y-%m-%d")),
             "median of %d alternating windows of %d calls, device events, ms per call" % (args.reps, INNER)]
    print("\n".join(lines), flush=True)
    for G, B in ((100, 16), (8, 64)):
        for model, K, N in ZOO:
            lines.append("%-12s " % model + bench_layer(G, B, K, N, args.reps))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    lines.append(bench_step(100, 16, args.reps))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
