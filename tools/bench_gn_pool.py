"""Timing of the norm blocks and pools of the batched 2-D engine: gn_pool.hip (GroupNorm + ReLU + 2x2 max-pool as one
forward and one backward kernel; the plain pool) against the framework expression it replaces (``group_norm`` in fp32,
the per-client affine, ``relu``, ``max_pool2d``), through the grouped twins of ``conv2d_hip`` with NIDT_B2D_GN = 0 and 1,
for vgg11's eight norm blocks and cnn_cifar10's two pools; the variants alternate inside every repetition.  A block is
timed as the next conv sees it: its input is the previous conv's channels-last bf16 output and its output is brought
to channels-last bf16 (free for the kernels, a cast for the framework path, which is what the engine does there).
Then ``BatchedModuleEngine.train_step`` of vgg11, vgg16 and cnn_cifar10 under both settings.
Usage: python tools/bench_gn_pool.py [--out FILE] [--reps N]"""
import argparse
import os
import socket
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_conv2d_wgrad import INNER, alternate  # noqa: E402  (the same windows and alternation)

SW = "NIDT_B2D_GN"
NORMS = [(64, 32, 1), (128, 16, 1), (256, 8, 0), (256, 8, 1), (512, 4, 0), (512, 4, 1), (512, 2, 0), (512, 2, 1)]
POOLS = [(64, 28), (64, 10)]  # cnn_cifar10: C, H of the pooled ReLU(conv) outputs


def _restore(before):
    if before is None:
        os.environ.pop(SW, None)
    else:
        os.environ[SW] = before


def bench_block(G, B, C, H, pool, norm, reps):
    """One norm block (GroupNorm(32, C), ReLU[, MaxPool2d(2, 2)]) or one lone pool: forward, and forward + backward."""
    import torch.nn as nn
    from neuroimagedisttraining_amd.engine.conv2d_hip import GGroupNorm, GMaxPool2d, _Group, _nhwc_bf16, gn2d_ok, \
        pool2d_ok
    dev = "cuda"
    grp = _Group()
    grp.G = G
    theta = torch.randn(G, 2 * C + 11, device=dev)
    theta[:, 3:3 + C] += 1.0
    grp.params = {"n.weight": theta[:, 3:3 + C].requires_grad_(True),  # views of the rows, as in the engine
                  "n.bias": theta[:, 3 + C:3 + 2 * C].requires_grad_(True)}
    mod = GGroupNorm(nn.GroupNorm(32, C), "n", grp, nn.ReLU(inplace=True), pool) if norm else GMaxPool2d()
    x = torch.randn(G * B, H, H, C, device=dev).to(torch.bfloat16).permute(0, 3, 1, 2).requires_grad_(True)
    Ho = H // 2 if pool else H
    dy = torch.randn(G * B, Ho, Ho, C, device=dev).to(torch.bfloat16)
    ins = [x] + (list(grp.params.values()) if norm else [])

    def fn(v, bwd):
        def run():
            os.environ[SW] = v
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = _nhwc_bf16(mod(x))
            return torch.autograd.grad(y, ins, dy) if bwd else y
        return run

    before = os.environ.get(SW)
    y1, y0 = fn("1", False)().float(), fn("0", False)().float()
    g1, g0 = fn("1", True)()[0].float(), fn("0", True)()[0].float()
    rel = lambda a, r: float((a - r).norm() / r.norm())  # noqa: E731
    t = alternate({"f0": fn("0", False), "f1": fn("1", False), "f1'": fn("1", False), "fb0": fn("0", True),
                   "fb1": fn("1", True)}, reps)
    _restore(before)
    f = lambda n: "%.3f [%.3f .. %.3f]" % t[n]  # noqa: E731
    served = gn2d_ok(H, H, C, 32, pool) if norm else pool2d_ok(H, H, C)
    return ("%s C%-3d H%-2d pool%d G=%3d B=%2d served %d | fwd: GN=0 %s  =1 %s (again %s) = %.2fx | fwd+bwd: GN=0 %s  "
            "=1 %s = %.2fx | rel diff y %.1e dx %.1e"
            % ("norm" if norm else "pool", C, H, pool, G, B, served, f("f0"), f("f1"), f("f1'"),
               t["f0"][0] / t["f1"][0], f("fb0"), f("fb1"), t["fb0"][0] / t["fb1"][0], rel(y1, y0), rel(g1, g0)))


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
    ts, loss = {"1": [], "0": []}, {}
    before = os.environ.get(SW)
    for rep in range(reps + 2):  # two warm-up rounds
        for v in ts:
            os.environ[SW] = v
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                loss[v] = eng.train_step(theta, None, grads, idx, G, B, 1.0, 7)
            torch.cuda.synchronize()
            if rep >= 2:
                ts[v].append((time.perf_counter() - t0) / 3 * 1e3)
    _restore(before)
    med = {v: statistics.median(t) for v, t in ts.items()}
    return ("%s train_step G=%d B=%d: %s=1 %.3f ms [%.3f .. %.3f]   =0 %.3f ms [%.3f .. %.3f]   new / parent = %.3f   "
            "max |loss diff| %.1e" % (name, G, B, SW, med["1"], min(ts["1"]), max(ts["1"]), med["0"], min(ts["0"]),
                                      max(ts["0"]), med["1"] / med["0"],
                                      float((loss["1"].float() - loss["0"].float()).abs().max())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gn_pool: needs the GPU")
    p = torch.cuda.get_device_properties(0)
    lines = ["box: host %s, %s, %d CUs, torch %s, HIP %s, %s" % (socket.gethostname(), p.gcnArchName,
                                                                 p.multi_processor_count, torch.__version__,
                                                                 torch.version.hip, time.strftime("%Y-%m-%d")),
             "median [min .. max] of %d alternating windows of %d calls, device events, ms per call; the spread of a "
             "path is its [min .. max] and the second =1 forward column (the same call again)" % (args.reps, INNER)]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for G, B in ((100, 16), (8, 64)):
        for C, H, pool in NORMS:
            emit(bench_block(G, B, C, H, pool, True, args.reps))
            torch.cuda.empty_cache()
        for C, H in POOLS:
            emit(bench_block(G, B, C, H, 1, False, args.reps))
            torch.cuda.empty_cache()
    for G, B in ((100, 16), (8, 64)):
        for name in ("vgg11", "vgg16", "cnn_cifar10"):
            emit(bench_step(name, G, B, args.reps))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
