"""conv2d_thin.hip (dense-K forward and position-split weight / bias gradient of the thin first layers): every element
of the raw bindings against fp64 with bounds from the arithmetic, bit-exact on the integer lattice for every split
count, and the first layer of cnn_cifar10 / vgg11 inside a train step of the batched 2-D engine."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _lattice as L

pytestmark = pytest.mark.gpu

G = 3
CASES = [  # cin, cout, k, pad, H, W, B
    (1, 20, 5, 0, 12, 12, 3), (3, 6, 5, 0, 9, 9, 4), (3, 64, 3, 1, 6, 6, 2),
    (3, 70, 5, 2, 7, 7, 3),   # two Cout tiles, ragged Cout
    (1, 8, 7, 3, 5, 9, 2),    # k = 7, H != W, rows shorter than a tile
    (4, 8, 3, 1, 2, 2, 5)]    # tiles straddle samples
SPLITS = (0, 1, 3, 5)
SENT = -7.25e11


def _ref64(x, dy, w, b, k, pad, groups):
    """fp64 (y, dw, db) per client of channels-last x [groups B, H, W, cin], dy [groups B, Ho, Wo, cout], w [groups,
    cout, cin, k, k], b [groups, cout]."""
    B, nc = x.shape[0] // groups, lambda t: t.double().permute(0, 3, 1, 2).contiguous()  # noqa: E731
    ys, dws = [], []
    for g in range(groups):
        xg, dg = nc(x[g * B:(g + 1) * B]), nc(dy[g * B:(g + 1) * B])
        ys.append(F.conv2d(xg, w[g].double(), b[g].double(), padding=pad).permute(0, 2, 3, 1))
        dws.append(torch.nn.grad.conv2d_weight(xg, w[g].shape, dg, padding=pad))
    return torch.cat(ys), torch.stack(dws), dy.double().view(groups, -1, dy.shape[-1]).sum(1)


@functools.lru_cache(maxsize=None)
def _case(case, lattice):
    """CPU operands (x, dy bf16; w, b fp32), the fp64 references (y, dw, db) with w rounded to bf16, and the same
    sums over absolute values; shared, never modified."""
    cin, cout, k, pad, H, W, B = case
    g = L.gen("conv2d_thin", case, lattice)
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    if lattice:
        x, dy = L.int_acts((G * B, H, W, cin), g), L.int_acts((G * B, Ho, Wo, cout), g)
        w, b = L.int_weights(G, cout, cin, k * k, g).view(G, cout, cin, k, k), L.int_bias(G, cout, g)
    else:
        x = torch.randn(G * B, H, W, cin, generator=g).to(torch.bfloat16)
        dy = torch.randn(G * B, Ho, Wo, cout, generator=g).to(torch.bfloat16)
        w = torch.randn(G, cout, cin, k, k, generator=g) * (cin * k * k) ** -0.5
        b = 0.1 * torch.randn(G, cout, generator=g)
    wr = w.to(torch.bfloat16).float()
    return x, dy, w, b, _ref64(x, dy, wr, b, k, pad, G), _ref64(x.abs(), dy.abs(), wr.abs(), b.abs(), k, pad, G)


def _rows(case, w=None, b=None):
    """Sentinel-filled client rows with the weight block at offset 3 and the bias block at an odd offset after it:
    (rows, weight view, bias view, mask of the elements outside both)."""
    cin, cout, k = case[:3]
    nw = cout * cin * k * k
    off_b = 3 + nw + 5 + (nw + 1) % 2
    Q = torch.full((G, off_b + cout + 13), SENT, device="cuda")
    keep = torch.ones_like(Q, dtype=torch.bool)
    keep[:, 3:3 + nw] = False
    keep[:, off_b:off_b + cout] = False
    wv, bv = Q[:, 3:3 + nw].view(G, cout, cin, k, k), Q[:, off_b:off_b + cout]
    if w is not None:
        wv.copy_(w)
        bv.copy_(b)
    return Q, wv, bv, keep


def _fwd(case, x, w, b):
    """conv2d_thin_fwd reading the client rows in place, y between two NaN guard rows: (y, guards untouched)."""
    from neuroimagedisttraining_amd import ops
    cin, cout, k, pad, H, W, B = case
    Q, wv, bv, _ = _rows(case, w, b)
    M = G * B * (H + 2 * pad - k + 1) * (W + 2 * pad - k + 1)
    xd, out = x.cuda(), torch.full((M + 2, cout), float("nan"), device="cuda", dtype=torch.bfloat16)
    ops.ext().conv2d_thin_fwd(xd.data_ptr(), wv.data_ptr(), Q.stride(0), bv.data_ptr(), Q.stride(0),
                              out[1:].data_ptr(), G, B, H, W, cin, cin, cout, k, pad, ops.stream())
    torch.cuda.synchronize()
    return out[1:-1], bool(torch.isnan(out[0]).all() and torch.isnan(out[-1]).all())


def _wgrad(case, x, dy, splits):
    """conv2d_thin_wgrad into sentinel rows: (rows, dw view, db view, mask of the elements outside both)."""
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine.conv2d_hip import conv2d_thin_scratch
    cin, cout, k, pad, H, W, B = case
    Q, dw, db, keep = _rows(case)
    xd, dyd = x.cuda(), dy.cuda()
    part = conv2d_thin_scratch(G, B, H + 2 * pad - k + 1, W + 2 * pad - k + 1, cout, k, cin, "cuda", splits)
    ops.ext().conv2d_thin_wgrad(xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), Q.stride(0), db.data_ptr(),
                                Q.stride(0), part.data_ptr(), part.numel(), splits, G, B, H, W, cin, cin, cout, k,
                                pad, ops.stream())
    torch.cuda.synchronize()
    return Q, dw, db, keep


def _within(name, got, ref, bound):
    err = (got.double().cpu().reshape(ref.shape) - ref).abs()
    bad = ~(err <= bound)
    print(name, "max err", float(err.max()), "max bound", float(bound.max()))
    assert not bad.any(), (name, int(bad.sum()), float(err.max()))


def _fwd_bound(case, ref, S):
    kp = (case[2] ** 2 * case[0] + 31) // 32 * 32
    return 2.0 ** -8 * ref.abs() + (kp + 8) * 2.0 ** -24 * S


@pytest.mark.parametrize("case", CASES)
def test_conv2d_thin_fwd_every_element_against_fp64_with_guard_rows(case):
    """|got - ref| <= 2^-8 |ref| + (Kp + 8) 2^-24 S, Kp = k k cin rounded up to 32, S the convolution of the absolute
    values (plus |bias|), w rounded to bf16: the bound of test_gpu_conv2d_fd.py.  The guard rows stay NaN."""
    x, _, w, b, (ry, _, _), (sy, _, _) = _case(case, False)
    y, guards = _fwd(case, x, w, b)
    _within("y", y, ry, _fwd_bound(case, ry, sy))
    assert guards, "guard row written"


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("case", CASES)
def test_conv2d_thin_wgrad_every_element_against_fp64_with_guards(case, splits):
    """|got - ref| <= M 2^-24 sum |dy||x| for dW and M 2^-24 sum |dy| for dB, M = B Ho Wo: an element passes through
    at most L + S <= M additions.  Every sentinel outside the written blocks stays."""
    cin, cout, k, pad, H, W, B = case
    x, dy, _, _, (_, rdw, rdb), (_, sdw, sdb) = _case(case, False)
    Q, dw, db, keep = _wgrad(case, x, dy, splits)
    M = B * (H + 2 * pad - k + 1) * (W + 2 * pad - k + 1)
    _within("dw", dw, rdw, M * 2.0 ** -24 * sdw)
    _within("db", db, rdb, M * 2.0 ** -24 * sdb)
    bits = torch.tensor(SENT, device="cuda").view(torch.int32)
    assert bool((Q.view(torch.int32)[keep] == bits).all()), "conv2d_thin_wgrad wrote outside the dw / db blocks"


@pytest.mark.parametrize("case", CASES)
def test_conv2d_thin_exact_on_integer_lattice_and_reproducible(case, monkeypatch):
    """Operands in {-2..2}, weights in {-1, 0, 1}: every partial sum is an integer below 2^24 and y a bf16 value, so
    y, dW and dB through HipConv2dFn, and dW / dB for every split count, equal fp64 bit for bit; two calls on the same
    random operands give the same bits."""
    from neuroimagedisttraining_amd.engine.conv2d_hip import HipConv2dFn, conv2d_thin_ok
    cin, cout, k, pad, H, W, B = case
    x, dy, w, b, (ry, rdw, rdb), _ = _case(case, True)
    L.require_bf16_exact(ry, "conv2d_thin lattice forward")
    L.require_fp32_exact(4.0 * dy.numel() / (G * cout), "conv2d_thin lattice")
    monkeypatch.setenv("NIDT_B2D_THIN", "1")
    assert conv2d_thin_ok(k, cin, cout)
    wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = HipConv2dFn.apply(x.cuda().permute(0, 3, 1, 2), wd, bd, G, pad)
    y.backward(dy.cuda().permute(0, 3, 1, 2))
    L.assert_exact(y.detach().permute(0, 2, 3, 1), ry, ("sample", "oh", "ow", "co"))
    L.assert_exact(wd.grad, rdw, ("client", "co", "ci", "kh", "kw"))
    L.assert_exact(bd.grad, rdb, ("client", "co"))
    for splits in SPLITS:
        _, dw, db, _ = _wgrad(case, x, dy, splits)
        L.assert_exact(dw, rdw, ("client", "co", "ci", "kh", "kw"))
        L.assert_exact(db, rdb, ("client", "co"))
    x, dy, w, b = _case(case, False)[:4]
    assert torch.equal(_wgrad(case, x, dy, 0)[0].view(torch.int32), _wgrad(case, x, dy, 0)[0].view(torch.int32))
    assert torch.equal(_fwd(case, x, w, b)[0].view(torch.int16), _fwd(case, x, w, b)[0].view(torch.int16))


@pytest.mark.parametrize("name", ["cnn_cifar10", "vgg11"])
def test_batched2d_first_layer_on_conv2d_thin_against_fp64(name, monkeypatch):
    """One train step with NIDT_B2D_THIN = 1: the first conv's output and its rows of ``grads`` within the two bounds
    above of fp64 computed from the layer's recorded bf16 input, output gradient and the clients' rows."""
    from neuroimagedisttraining_amd.engine.batched2d import BatchedModuleEngine
    from neuroimagedisttraining_amd.engine import conv2d_hip
    from neuroimagedisttraining_amd.engine.executor import padded_rows
    from neuroimagedisttraining_amd.engine.resnet2d_hip import CIFAR_MEAN, CIFAR_STD
    from neuroimagedisttraining_amd.models import create_model
    Gc, B = 4, 8
    torch.manual_seed(1)
    monkeypatch.setenv("NIDT_B2D_THIN", "1")
    model = create_model(name, dataset="cifar10", class_num=10)
    x8 = torch.randint(0, 256, (Gc * B, 32, 32, 3), dtype=torch.uint8)
    eng = BatchedModuleEngine(model, x8, torch.randint(0, 10, (Gc * B,)), "cuda", CIFAR_MEAN, CIFAR_STD)
    assert eng.uses_hip_layers
    seen = []

    def record(mod, inp, outp):
        seen.extend([inp[0].detach(), outp.detach()])
        outp.register_hook(seen.append)

    first = next(m for m in eng._grouped[0].modules() if isinstance(m, conv2d_hip.GConv2d))
    first.register_forward_hook(record)
    theta = padded_rows(Gc, eng.players.total, "cuda")
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cuda()
    theta.copy_(flat.expand(Gc, -1) + torch.randn(Gc, flat.numel(), device="cuda") * 0.01)
    grads = padded_rows(Gc, eng.players.total, "cuda")
    eng.train_step(theta, None, grads, torch.arange(Gc * B, dtype=torch.int32, device="cuda"), Gc, B, 1.0, 7)
    torch.cuda.synchronize()
    P = eng.players
    iw, ib = P.names.index(first.name + ".weight"), P.names.index(first.name + ".bias")
    (cout, cin, k, _), ow, ob = tuple(P.shapes[iw]), P.offsets[iw], P.offsets[ib]
    assert conv2d_hip.conv2d_thin_ok(k, cin, cout)
    x, y, gy = (t.to(torch.bfloat16).permute(0, 2, 3, 1).cpu() for t in seen)
    w = theta[:Gc, ow:ow + P.numel(iw)].view(Gc, cout, cin, k, k).to(torch.bfloat16).float().cpu()
    b = theta[:Gc, ob:ob + cout].cpu()
    ry, rdw, rdb = _ref64(x, gy, w, b, k, first.pad, Gc)
    sy, sdw, sdb = _ref64(x.abs(), gy.abs(), w.abs(), b.abs(), k, first.pad, Gc)
    M = B * gy.shape[1] * gy.shape[2]
    _within("y", y, ry, _fwd_bound((cin, cout, k), ry, sy))
    _within("dw", grads[:Gc, ow:ow + P.numel(iw)], rdw, M * 2.0 ** -24 * sdw)
    _within("db", grads[:Gc, ob:ob + cout], rdb, M * 2.0 ** -24 * sdb)
