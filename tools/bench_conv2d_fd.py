"""Timing of the conv forward and stride-1 data gradient of the batched 2-D engine: conv2d_fd.hip (LDS-staged MFMA
kernel, both directions on the forward weight image) against the path it replaces (conv2d_any_fwd, the data gradient
on a second, flipped-transposed image), and ``HipConv2dFn`` forward + backward with NIDT_B2D_FD = 0 and 1, for every
conv layer of lenet5, LeNet5_cifar, cnn_cifar10, vgg11 and the two EMNIST CNNs that the launcher serves (whether
or not ``conv2d_fd_ok`` routes it there); the variants alternate inside every repetition.  Each data-gradient side includes the ``conv2d_pack_w`` launch it needs (both images for the old kernel,
the forward image alone for the new one).  Then one ``BatchedModuleEngine.train_step`` of cnn_cifar10 and vgg11 under
both settings.
Usage: python tools/bench_conv2d_fd.py [--out FILE] [--reps N]"""
import argparse
import os
import socket
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_conv2d_wgrad import ZOO, INNER, alternate  # noqa: E402  (the same layer table, windows and alternation)

SW = "NIDT_B2D_FD"
# the EMNIST CNNs' second layers: the zoo's only 32-channel contractions (conv2d_fd_ok's channel threshold)
EXTRA = [("CNN_OriginalFedAvg", 32, 64, 5, 2, 14), ("CNN_DropOut", 32, 64, 3, 0, 26)]


def bench_layer(G, B, cin, cout, k, pad, H, reps):
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine.conv2d_hip import HipConv2dFn, conv2d_fd_ok, conv2d_fd_served
    m, s, dev = ops.ext(), ops.stream(), "cuda"
    head = "%3d->%-3d k%d H%-2d G=%3d B=%2d | " % (cin, cout, k, H, G, B)
    ok_f = conv2d_fd_served(k, pad, H, cin, cout, False)
    ok_d = cin > 3 and conv2d_fd_served(k, pad, H, cin, cout, True)
    if not (ok_f or ok_d):
        return head + "not served (stays on conv2d_any_fwd in both settings)"
    Ho = H + 2 * pad - k + 1
    nw = cout * cin * k * k
    ld = 3 + nw + cout + 7  # the blocks at 4-byte-aligned offsets inside a row, as in theta
    theta = torch.randn(G, ld, device=dev) * (cin * k * k) ** -0.5
    w = theta[:, 3:3 + nw].view(G, cout, cin, k, k).requires_grad_(True)
    b = theta[:, 3 + nw:3 + nw + cout].requires_grad_(True)
    bias = b.detach().contiguous()
    x = torch.randn(G * B, H, H, cin, device=dev).to(torch.bfloat16)
    dy = torch.randn(G * B, Ho, Ho, cout, device=dev).to(torch.bfloat16)
    xn = x.permute(0, 3, 1, 2).requires_grad_(cin > 3)  # the first layers have no data gradient
    dyn = dy.permute(0, 3, 1, 2)
    img = torch.empty(G, (cout + 63) // 64 * 64, k * k, (cin + 7) // 8 * 8, device=dev, dtype=torch.bfloat16)
    imgt = torch.empty(G, (cin + 63) // 64 * 64, k * k, (cout + 7) // 8 * 8, device=dev, dtype=torch.bfloat16)
    y = [torch.empty_like(dy) for _ in range(2)]
    dx = [torch.empty_like(x) for _ in range(2)]

    def pack(t):
        m.conv2d_pack_w(w.data_ptr(), ld, img.data_ptr(), imgt.data_ptr() if t else 0, G, cout, cin, k, s)

    def fwd_old():
        m.conv2d_any_fwd(x.data_ptr(), img.data_ptr(), bias.data_ptr(), y[0].data_ptr(), G, B, H, H, cin, cin, cout, k,
                         pad, s)

    def fwd_new():
        m.conv2d_fd(x.data_ptr(), img.data_ptr(), bias.data_ptr(), y[1].data_ptr(), G, B, H, H, cin, cin, cout, k, pad,
                    0, s)

    def dg_old():
        pack(True)
        m.conv2d_any_fwd(dy.data_ptr(), imgt.data_ptr(), 0, dx[0].data_ptr(), G, B, Ho, Ho, cout, cout, cin, k,
                         k - 1 - pad, s)

    def dg_new():
        pack(False)
        m.conv2d_fd(dy.data_ptr(), img.data_ptr(), 0, dx[1].data_ptr(), G, B, H, H, cin, cout, cout, k, pad, 1, s)

    def fn(v):
        def run():
            os.environ[SW] = v
            ins = [xn, w, b] if xn.requires_grad else [w, b]
            return torch.autograd.grad(HipConv2dFn.apply(xn, w, b, G, pad), ins, dyn)
        return run

    before = os.environ.get(SW)
    pack(True)
    fns = {"fn0": fn("0"), "fn1": fn("1")}
    if ok_f:
        fns.update({"f0": fwd_old, "f1": fwd_new, "f1'": fwd_new})
    if ok_d:
        fns.update({"d0": dg_old, "d1": dg_new})
    t = alternate(fns, reps)
    if before is None:
        os.environ.pop(SW, None)
    else:
        os.environ[SW] = before
    rel = lambda a, r: float((a.float() - r.float()).norm() / r.float().norm())  # noqa: E731
    flop = 2.0 * G * B * Ho * Ho * nw
    f = lambda n: "%.3f [%.3f .. %.3f]" % t[n]  # noqa: E731
    out = head
    if ok_f:
        out += ("fwd: conv2d_any %s  conv2d_fd %s (again %s) = %.2fx, %.1f -> %.1f bf16 TF/s, rel diff %.1e | "
                % (f("f0"), f("f1"), f("f1'"), t["f0"][0] / t["f1"][0], flop / t["f0"][0] / 1e9,
                   flop / t["f1"][0] / 1e9, rel(y[1], y[0])))
    else:
        out += "fwd: not served | "
    if ok_d:
        out += ("dgrad + pack: conv2d_any %s  conv2d_fd %s = %.2fx, rel diff %.1e | "
                % (f("d0"), f("d1"), t["d0"][0] / t["d1"][0], rel(dx[1], dx[0])))
    else:
        out += "dgrad: none or not served | "
    routed = "/".join("fd" if conv2d_fd_ok(k, pad, H, cin, cout, d) else "any" for d in (False, True))
    return out + ("HipConv2dFn fwd+bwd (=1 routes fwd/dgrad to %s): FD=0 %s  =1 %s = %.2fx"
                  % (routed, f("fn0"), f("fn1"), t["fn0"][0] / t["fn1"][0]))


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
    before = os.environ.get(SW)
    for rep in range(reps + 2):  # two warm-up rounds
        for v in ts:
            os.environ[SW] = v
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                eng.train_step(theta, None, grads, idx, G, B, 1.0, 7)
            torch.cuda.synchronize()
            if rep >= 2:
                ts[v].append((time.perf_counter() - t0) / 3 * 1e3)
    if before is None:
        del os.environ[SW]
    else:
        os.environ[SW] = before
    med = {v: statistics.median(t) for v, t in ts.items()}
    return ("%s train_step G=%d B=%d: %s=1 %.3f ms [%.3f .. %.3f]   =0 %.3f ms [%.3f .. %.3f]   new / parent = %.3f"
            % (name, G, B, SW, med["1"], min(ts["1"]), max(ts["1"]), med["0"], min(ts["0"]), max(ts["0"]),
               med["1"] / med["0"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv2d_fd: needs the GPU")
    p = torch.cuda.get_device_properties(0)
    lines = ["box: host %s, %s, %d CUs, torch %s, HIP %s, %s" % (socket.gethostname(), p.gcnArchName,
                                                                 p.multi_processor_count, torch.__version__,
                                                                 torch.version.hip, time.strftime("%Y-%m-%d")),
             "median [min .. max] of %d alternating windows of %d calls, device events, ms per call; the spread of a "
             "path is its [min .. max] and the second conv2d_fd forward column (the same call again)"
             % (args.reps, INNER)]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for G, B in ((100, 16), (8, 64)):
        for model, cin, cout, k, pad, H in ZOO + EXTRA:
            emit("%-12s " % model + bench_layer(G, B, cin, cout, k, pad, H, args.reps))
            torch.cuda.empty_cache()
    for name in ("cnn_cifar10", "vgg11"):
        emit(bench_step(name, 100, 16, args.reps))


if __name__ == "__main__":
    main()
