"""Timing of the conv weight / bias gradient of the batched 2-D engine: conv2d_wg.hip (one MFMA launch writing fp32 dW
and dB in the parameter layout) against the path it replaces (conv2d_any_wgrad + ``part.sum(0)`` + permute copy +
framework bias sum), and ``HipConv2dFn`` forward + backward with NIDT_B2D_WGRAD = 0 and 1, for every conv layer of
lenet5, LeNet5_cifar, cnn_cifar10 and vgg11; the variants alternate inside every repetition.  Then one
``BatchedModuleEngine.train_step`` of cnn_cifar10 and vgg11 under both settings.
Usage: python tools/bench_conv2d_wgrad.py [--out FILE] [--reps N]"""
import argparse
import os
import socket
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ZOO = [  # model, cin, cout, k, pad, H
    ("lenet5", 1, 20, 5, 0, 28), ("lenet5", 20, 50, 5, 0, 12), ("LeNet5_cifar", 3, 6, 5, 0, 32),
    ("LeNet5_cifar", 6, 16, 5, 0, 14), ("cnn_cifar10", 3, 64, 5, 0, 32), ("cnn_cifar10", 64, 64, 5, 0, 14),
    ("vgg11", 3, 64, 3, 1, 32), ("vgg11", 64, 128, 3, 1, 16), ("vgg11", 128, 256, 3, 1, 8),
    ("vgg11", 256, 256, 3, 1, 8), ("vgg11", 256, 512, 3, 1, 4), ("vgg11", 512, 512, 3, 1, 4),
    ("vgg11", 512, 512, 3, 1, 2)]
INNER = 5  # calls per timed window


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
    """{name: (median, min, max) ms} of the variants, every repetition running each of them once in turn."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(window(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def bench_layer(G, B, cin, cout, k, pad, H, reps):
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine.conv2d_hip import HipConv2dFn
    m, s, dev = ops.ext(), ops.stream(), "cuda"
    Ho = H + 2 * pad - k + 1
    nw = cout * cin * k * k
    ld = 3 + nw + cout + 7  # the blocks at 4-byte-aligned offsets inside a row, as in theta
    theta = torch.randn(G, ld, device=dev) * (cin * k * k) ** -0.5
    w = theta[:, 3:3 + nw].view(G, cout, cin, k, k).requires_grad_(True)
    b = theta[:, 3 + nw:3 + nw + cout].requires_grad_(True)
    x = torch.randn(G * B, H, H, cin, device=dev).to(torch.bfloat16)
    dy = torch.randn(G * B, Ho, Ho, cout, device=dev).to(torch.bfloat16)
    xn = x.permute(0, 3, 1, 2).requires_grad_(cin > 3)  # the first layers have no data gradient
    dyn = dy.permute(0, 3, 1, 2)
    dw, db = torch.empty(G, cout, cin, k, k, device=dev), torch.empty(G, cout, device=dev)
    part = torch.empty(m.conv2d_any_wgrad_chunks(B, Ho, Ho), G, cout, k * k, cin, device=dev)

    def parent():
        m.conv2d_any_wgrad(x.data_ptr(), dy.data_ptr(), part.data_ptr(), G, B, H, H, cin, cin, cout, k, pad, s)
        return (part.sum(0).view(G, cout, k, k, cin).permute(0, 1, 4, 2, 3).contiguous(),
                dy.float().view(G, B * Ho * Ho, cout).sum(1))

    def kernel():
        m.conv2d_wg(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), nw, db.data_ptr(), cout, G, B, H, H, cin, cin, cout, k,
                    pad, s)

    def fn(v):
        def run():
            os.environ["NIDT_B2D_WGRAD"] = v
            ins = [xn, w, b] if xn.requires_grad else [w, b]
            return torch.autograd.grad(HipConv2dFn.apply(xn, w, b, G, pad), ins, dyn)
        return run

    before = os.environ.get("NIDT_B2D_WGRAD")
    pw, pb = parent()
    kernel()
    rel = [float((a - r).norm() / r.norm()) for a, r in ((dw, pw), (db, pb))]
    t = alternate({"parent": parent, "kernel": kernel, "kernel'": kernel, "fn0": fn("0"), "fn1": fn("1")}, reps)
    if before is None:
        os.environ.pop("NIDT_B2D_WGRAD", None)
    else:
        os.environ["NIDT_B2D_WGRAD"] = before
    flop = 2.0 * G * B * Ho * Ho * nw
    f = lambda n: "%.3f [%.3f .. %.3f]" % t[n]  # noqa: E731
    return ("%3d->%-3d k%d H%-2d G=%3d B=%2d | wgrad+bias: parent path %s  conv2d_wg %s (again %s) = %.2fx, "
            "%.1f -> %.1f bf16 TF/s | HipConv2dFn fwd+bwd: WGRAD=0 %s  =1 %s = %.2fx | rel diff dw %.1e db %.1e"
            % (cin, cout, k, H, G, B, f("parent"), f("kernel"), f("kernel'"), t["parent"][0] / t["kernel"][0],
               flop / t["parent"][0] / 1e9, flop / t["kernel"][0] / 1e9, f("fn0"), f("fn1"), t["fn0"][0] / t["fn1"][0],
               rel[0], rel[1]))


def bench_step(name, G, B, reps):
    """Host clock around train_step ending in a device synchronise, the two settings alternating."""
    from neuroimagedisttraining_amd.engine.batched2d import BatchedModuleEngine
    from neuroimagedisttraining_amd.engine.executor import padded_rows
    from neuroimagedisttraining_amd.engine.resnet2d_hip import CIFAR_MEAN, CIFAR_STD, synthetic_cifar
    from neuroimagedisttraining_amd.models import create_model
    torch.manual_seed(0)
    model = create_model(name, dataset="cifar10", class_num=10)
    x8, y = synthetic_cifar(G * B, seed=1)
    eng = BatchedModuleEngine(model, x8, y, "cuda", CIFAR_MEAN, CIFAR_STD)
    theta = padded_rows(G, eng.players.total, "cuda")
    theta.copy_(torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cuda().expand(G, -1))
    grads = padded_rows(G, eng.players.total, "cuda")
    idx = torch.arange(G * B, dtype=torch.int32, device="cuda")
    ts = {"1": [], "0": []}
    before = os.environ.get("NIDT_B2D_WGRAD")
    for rep in range(reps + 2):  # two warm-up rounds
        for v in ts:
            os.environ["NIDT_B2D_WGRAD"] = v
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                eng.train_step(theta, None, grads, idx, G, B, 1.0, 7)
            torch.cuda.synchronize()
            if rep >= 2:
                ts[v].append((time.perf_counter() - t0) / 3 * 1e3)
    if before is None:
        del os.environ["NIDT_B2D_WGRAD"]
    else:
        os.environ["NIDT_B2D_WGRAD"] = before
    med = {v: statistics.median(t) for v, t in ts.items()}
    return ("%s train_step G=%d B=%d: NIDT_B2D_WGRAD=1 %.3f ms [%.3f .. %.3f]   =0 %.3f ms [%.3f .. %.3f]   "
            "new / parent = %.3f" % (name, G, B, med["1"], min(ts["1"]), max(ts["1"]), med["0"], min(ts["0"]),
                                     max(ts["0"]), med["1"] / med["0"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv2d_wgrad: needs the GPU")
    p = torch.cuda.get_device_properties(0)
    lines = ["box: host %s, %s, %d CUs, torch %s, HIP %s, %s" % (socket.gethostname(), p.gcnArchName,
                                                                 p.multi_processor_count, torch.__version__,
                                                                 torch.version.hip, time.strftime("%Y-%m-%d")),
             "median [min .. max] of %d alternating windows of %d calls, device events, ms per call; the spread of a "
             "path is its [min .. max] and the second conv2d_wg column (the same call again)" % (args.reps, INNER)]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for G, B in ((100, 16), (8, 64)):
        for model, cin, cout, k, pad, H in ZOO:
            emit("%-12s " % model + bench_layer(G, B, cin, cout, k, pad, H, args.reps))
            torch.cuda.empty_cache()
    for name in ("cnn_cifar10", "vgg11"):
        emit(bench_step(name, 100, 16, args.reps))


if __name__ == "__main__":
    main()
