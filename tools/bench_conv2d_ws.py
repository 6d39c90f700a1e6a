"""Timing of conv2d_ws.hip (conv forward and stride-1 data gradient on the clients' fp32 weight blocks read in place)
against the path it replaces, for every 3 x 3 layer of vgg11 / vgg16 that its launcher serves: ``conv2d_pack_w`` alone
(forward image), ``conv2d_pack_w`` + ``conv2d_fd`` forward against ``conv2d_ws`` forward, ``conv2d_fd`` data gradient
(on the image the forward saved: no pack) against ``conv2d_ws`` data gradient, and ``HipConv2dFn`` forward + backward
with NIDT_B2D_WS = 0 and 2; the variants alternate inside every repetition.  Then ``BatchedModuleEngine.train_step``
and ``eval_logits`` of vgg11 and vgg16 with NIDT_B2D_WS = 0 and 1.  Both parts at 100 clients x 16 images and 8 x 64.
Usage: python tools/bench_conv2d_ws.py [--out FILE] [--reps N] [--no-steps]"""
import argparse
import os
import socket
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_conv2d_wgrad import INNER, alternate  # noqa: E402  (the same windows and alternation)

SW = "NIDT_B2D_WS"
LAYERS = [  # cin, cout, H of the 3 x 3, pad 1 layers of vgg11 / vgg16 (3->64 is thin; 64->64 on 32 x 32 is listed to
    # show that it is not served)
    (64, 64, 32), (64, 128, 16), (128, 128, 16), (128, 256, 8), (256, 256, 8), (256, 512, 4), (512, 512, 4),
    (512, 512, 2)]


def _restore(before):
    if before is None:
        os.environ.pop(SW, None)
    else:
        os.environ[SW] = before


def bench_layer(G, B, cin, cout, H, reps):
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine.conv2d_hip import HipConv2dFn, conv2d_ws_ok, conv2d_ws_served, conv2d_ws_tile
    m, s, dev, k, pad = ops.ext(), ops.stream(), "cuda", 3, 1
    head = "%3d->%-3d k3 H%-2d G=%3d B=%2d | " % (cin, cout, H, G, B)
    if not all(conv2d_ws_served(k, pad, B, H, H, cin, cout, d) for d in (False, True)):
        return head + "not served (the padded samples of a tile do not fit the slab)"
    nw = cout * cin * k * k
    ld = 3 + nw + cout + 7  # the blocks at 4-byte-aligned offsets inside a row, as in theta
    theta = torch.randn(G, ld, device=dev) * (cin * k * k) ** -0.5
    w = theta[:, 3:3 + nw].view(G, cout, cin, k, k).requires_grad_(True)
    b = theta[:, 3 + nw:3 + nw + cout].requires_grad_(True)
    bias = b.detach().contiguous()
    x = torch.randn(G * B, H, H, cin, device=dev).to(torch.bfloat16)
    dy = torch.randn(G * B, H, H, cout, device=dev).to(torch.bfloat16)
    xn, dyn = x.permute(0, 3, 1, 2).requires_grad_(True), dy.permute(0, 3, 1, 2)
    img = torch.empty(G, (cout + 63) // 64 * 64, k * k, cin, device=dev, dtype=torch.bfloat16)
    y = [torch.empty_like(dy) for _ in range(2)]
    dx = [torch.empty_like(x) for _ in range(2)]

    def pack():
        m.conv2d_pack_w(w.data_ptr(), ld, img.data_ptr(), 0, G, cout, cin, k, s)

    def fwd_old():
        pack()
        m.conv2d_fd(x.data_ptr(), img.data_ptr(), bias.data_ptr(), y[0].data_ptr(), G, B, H, H, cin, cin, cout, k, pad,
                    0, s)

    def fwd_new():
        m.conv2d_ws(x.data_ptr(), w.data_ptr(), ld, b.data_ptr(), ld, y[1].data_ptr(), G, B, H, H, cin, cin, cout, k,
                    pad, 0, s)

    def dg_old():
        m.conv2d_fd(dy.data_ptr(), img.data_ptr(), 0, dx[0].data_ptr(), G, B, H, H, cin, cout, cout, k, pad, 1, s)

    def dg_new():
        m.conv2d_ws(dy.data_ptr(), w.data_ptr(), ld, 0, 0, dx[1].data_ptr(), G, B, H, H, cin, cout, cout, k, pad, 1, s)

    def fn(v):
        def run():
            os.environ[SW] = v
            return torch.autograd.grad(HipConv2dFn.apply(xn, w, b, G, pad), [xn, w, b], dyn)
        return run

    before = os.environ.get(SW)
    t = alternate({"pk": pack, "f0": fwd_old, "f1": fwd_new, "f1'": fwd_new, "d0": dg_old, "d1": dg_new,
                   "d1'": dg_new, "fn0": fn("0"), "fn2": fn("2")}, reps)
    _restore(before)
    rel = lambda a, r: float((a.float() - r.float()).norm() / r.float().norm())  # noqa: E731
    f = lambda n: "%.3f [%.3f .. %.3f]" % t[n]  # noqa: E731
    gb = 4.0 * G * nw / 1e6  # fp32 weight bytes of the layer, MB
    routed = "/".join("ws" if conv2d_ws_ok(k, pad, B, H, H, cin, cout, d) else "fd" for d in (False, True))
    return head + (
        "tile %d/%d, %.0f MB of fp32 weights | pack %s | fwd: pack + conv2d_fd %s  conv2d_ws %s (again %s) = %.2fx, "
        "rel diff %.1e | dgrad: conv2d_fd %s  conv2d_ws %s (again %s) = %.2fx, rel diff %.1e | HipConv2dFn fwd+bwd "
        "(=1 routes fwd/dgrad to %s): WS=0 %s  =2 %s = %.2fx"
        % (conv2d_ws_tile(k, pad, B, H, H, False)[0], conv2d_ws_tile(k, pad, B, H, H, True)[0], gb, f("pk"), f("f0"),
           f("f1"), f("f1'"), t["f0"][0] / t["f1"][0], rel(y[1], y[0]), f("d0"), f("d1"), f("d1'"),
           t["d0"][0] / t["d1"][0], rel(dx[1], dx[0]), routed, f("fn0"), f("fn2"), t["fn0"][0] / t["fn2"][0]))


def bench_step(name, G, B, reps):
    """Host clock around train_step / eval_logits ending in a device synchronise, the two settings alternating."""
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
    calls = {"train_step": lambda: eng.train_step(theta, None, grads, idx, G, B, 1.0, 7),
             "eval_logits": lambda: eng.eval_logits(theta, None, idx, G, B)}
    before = os.environ.get(SW)
    out = []
    for what, call in calls.items():
        ts = {"1": [], "0": [], "0'": []}  # 0': the parent path again, its window-to-window spread
        for rep in range(reps + 2):  # two warm-up rounds
            for v in ts:
                os.environ[SW] = v[0]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    call()
                torch.cuda.synchronize()
                if rep >= 2:
                    ts[v].append((time.perf_counter() - t0) / 3 * 1e3)
        f = lambda v: "%.3f ms [%.3f .. %.3f]" % (statistics.median(ts[v]), min(ts[v]), max(ts[v]))  # noqa: E731
        out.append("%s %s G=%d B=%d: %s=1 %s   =0 %s (again %s)   new / parent = %.3f"
                   % (name, what, G, B, SW, f("1"), f("0"), f("0'"),
                      statistics.median(ts["1"]) / statistics.median(ts["0"])))
    _restore(before)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true", help="the layer table alone")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv2d_ws: needs the GPU")
    p = torch.cuda.get_device_properties(0)
    lines = ["box: host %s, %s, %d CUs, torch %s, HIP %s, %s" % (socket.gethostname(), p.gcnArchName,
                                                                 p.multi_processor_count, torch.__version__,
                                                                 torch.version.hip, time.strftime("%Y-%m-%d")),
             "median [min .. max] of %d alternating windows of %d calls, device events, ms per call; the spread of a "
             "path is its [min .. max] and its `again` column (the same call again in the same repetitions); steps: "
             "host clock around 3 calls ending in a synchronise" % (args.reps, INNER)]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for G, B in ((100, 16), (8, 64)):
        for cin, cout, H in LAYERS:
            emit(bench_layer(G, B, cin, cout, H, args.reps))
            torch.cuda.empty_cache()
    if not args.no_steps:
        for G, B in ((100, 16), (8, 64)):
            for name in ("vgg11", "vgg16"):
                for line in bench_step(name, G, B, args.reps):
                    emit(line)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
