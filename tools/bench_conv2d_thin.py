"""Timing of the thin first conv layers of the batched 2-D engine on conv2d_thin.hip against the parent's routed paths:
forward against ``conv2d_pack_w`` + ``conv2d_any_fwd``; weight + bias gradient against ``conv2d_wg`` where
``conv2d_wg_ok`` routes to it, else ``conv2d_any_wgrad`` + partial sum + permute copy + framework bias sum;
``HipConv2dFn`` forward + backward and one ``train_step`` of cnn_cifar10 and vgg11 with NIDT_B2D_THIN = 0 / 1.  The
variants alternate inside every repetition (``bench_conv2d_wgrad.alternate``: device events, median [min .. max]).
Usage: python tools/bench_conv2d_thin.py [--out FILE] [--reps N]"""
import argparse
import os
import socket
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_conv2d_wgrad import INNER, alternate  # noqa: E402

THIN = [  # model, cin, cout, k, pad, H
    ("lenet5", 1, 20, 5, 0, 28), ("LeNet5_cifar", 3, 6, 5, 0, 32), ("cnn_cifar10", 3, 64, 5, 0, 32),
    ("vgg11", 3, 64, 3, 1, 32), ("emnist_cnn_k5", 1, 32, 5, 2, 28), ("emnist_cnn_k3", 1, 32, 3, 0, 28)]


def _env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def bench_layer(G, B, cin, cout, k, pad, H, reps):
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine import conv2d_hip as C
    m, s, dev = ops.ext(), ops.stream(), "cuda"
    Ho = H + 2 * pad - k + 1
    nw = cout * cin * k * k
    ld = 3 + nw + cout + 7  # the blocks at 4-byte-aligned offsets inside a row, as in theta
    theta = torch.randn(G, ld, device=dev) * (cin * k * k) ** -0.5
    w = theta[:, 3:3 + nw].view(G, cout, cin, k, k).requires_grad_(True)
    b = theta[:, 3 + nw:3 + nw + cout].requires_grad_(True)
    wd, bd = w.detach(), b.detach()
    x = torch.randn(G * B, H, H, cin, device=dev).to(torch.bfloat16)
    dy = torch.randn(G * B, Ho, Ho, cout, device=dev).to(torch.bfloat16)
    xn, dyn = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)  # a first layer has no data gradient
    y0, y1 = torch.empty_like(dy), torch.empty_like(dy)
    dw, db = torch.empty(G, cout, cin, k, k, device=dev), torch.empty(G, cout, device=dev)
    dw1, db1 = torch.empty_like(dw), torch.empty_like(db)
    part = torch.empty(m.conv2d_any_wgrad_chunks(B, Ho, Ho), G, cout, k * k, cin, device=dev)
    scratch = C.conv2d_thin_scratch(G, B, Ho, Ho, cout, k, cin, dev)
    on_wg = C.conv2d_wg_ok(k, Ho, G, cin, cout)

    def fwd_parent():
        wp, _ = C.pack_conv_images(wd, False)
        bc = bd.float().contiguous()  # HipConv2dFn's bias copy
        m.conv2d_any_fwd(x.data_ptr(), wp.data_ptr(), bc.data_ptr(), y0.data_ptr(), G, B, H, H, cin, cin, cout, k,
                         pad, s)

    def fwd_thin():
        m.conv2d_thin_fwd(x.data_ptr(), wd.data_ptr(), ld, bd.data_ptr(), ld, y1.data_ptr(), G, B, H, H, cin, cin,
                          cout, k, pad, s)

    def wg_parent():
        if on_wg:
            m.conv2d_wg(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), nw, db.data_ptr(), cout, G, B, H, H, cin, cin,
                        cout, k, pad, s)
            return dw, db
        m.conv2d_any_wgrad(x.data_ptr(), dy.data_ptr(), part.data_ptr(), G, B, H, H, cin, cin, cout, k, pad, s)
        return (part.sum(0).view(G, cout, k, k, cin).permute(0, 1, 4, 2, 3).contiguous(),
                dy.float().view(G, B * Ho * Ho, cout).sum(1))

    def wg_thin():
        m.conv2d_thin_wgrad(x.data_ptr(), dy.data_ptr(), dw1.data_ptr(), nw, db1.data_ptr(), cout, scratch.data_ptr(),
                            scratch.numel(), 0, G, B, H, H, cin, cin, cout, k, pad, s)

    def fn(v):
        def run():
            os.environ["NIDT_B2D_THIN"] = v
            return torch.autograd.grad(C.HipConv2dFn.apply(xn, w, b, G, pad), [w, b], dyn)
        return run

    before = os.environ.get("NIDT_B2D_THIN")
    fwd_parent(), fwd_thin(), wg_thin()
    pw, pb = wg_parent()
    rel = [float((a.float() - r.float()).norm() / r.float().norm()) for a, r in ((y1, y0), (dw1, pw), (db1, pb))]
    t = alternate({"f0": fwd_parent, "f1": fwd_thin, "f1'": fwd_thin, "w0": wg_parent, "w1": wg_thin, "w1'": wg_thin,
                   "fn0": fn("0"), "fn1": fn("1")}, reps)
    _env("NIDT_B2D_THIN", before)
    f = lambda n: "%.3f [%.3f .. %.3f]" % t[n]  # noqa: E731
    return ("%d->%-2d k%d H%-2d G=%3d B=%2d S=%-2d | fwd: pack + conv2d_any_fwd %s  thin %s (again %s) = %.2fx | "
            "wgrad+bias: parent (%s) %s  thin %s (again %s) = %.2fx | HipConv2dFn fwd+bwd: THIN=0 %s  =1 %s = %.2fx | "
            "rel diff y %.1e dw %.1e db %.1e"
            % (cin, cout, k, H, G, B, m.conv2d_thin_splits(G, B, Ho, Ho, cout, 0), f("f0"), f("f1"), f("f1'"),
               t["f0"][0] / t["f1"][0], "conv2d_wg" if on_wg else "staged fp32", f("w0"), f("w1"), f("w1'"),
               t["w0"][0] / t["w1"][0], f("fn0"), f("fn1"), t["fn0"][0] / t["fn1"][0], rel[0], rel[1], rel[2]))


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
    before = os.environ.get("NIDT_B2D_THIN")
    for rep in range(reps + 2):  # two warm-up rounds
        for v in ts:
            os.environ["NIDT_B2D_THIN"] = v
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                eng.train_step(theta, None, grads, idx, G, B, 1.0, 7)
            torch.cuda.synchronize()
            if rep >= 2:
                ts[v].append((time.perf_counter() - t0) / 3 * 1e3)
    _env("NIDT_B2D_THIN", before)
    med = {v: statistics.median(t) for v, t in ts.items()}
    return ("%s train_step G=%d B=%d: NIDT_B2D_THIN=1 %.3f ms [%.3f .. %.3f]   =0 %.3f ms [%.3f .. %.3f]   "
            "new / parent = %.3f" % (name, G, B, med["1"], min(ts["1"]), max(ts["1"]), med["0"], min(ts["0"]),
                                     max(ts["0"]), med["1"] / med["0"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv2d_thin: needs the GPU")
    p = torch.cuda.get_device_properties(0)
    lines = ["box: host %s, %s, %d CUs, torch %s, HIP %s, %s" % (socket.gethostname(), p.gcnArchName,
                                                                 p.multi_processor_count, torch.__version__,
                                                                 torch.version.hip, time.strftime("%Y-%m-%d")),
             "median [min .. max] of %d alternating windows of %d calls, device events, ms per call; the spread of a "
             "path is its [min .. max] and the 'again' column (the same call again); S: position splits by rule"
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
        for model, cin, cout, k, pad, H in THIN:
            emit("%-13s " % model + bench_layer(G, B, cin, cout, k, pad, H, args.reps))
            torch.cuda.empty_cache()
    for G, B in ((100, 16), (8, 64)):
        for name in ("cnn_cifar10", "vgg11"):
            emit(bench_step(name, G, B, args.reps))


if __name__ == "__main__":
    main()
