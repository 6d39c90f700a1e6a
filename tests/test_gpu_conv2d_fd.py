"""conv2d_fd.hip (LDS-staged MFMA conv forward and stride-1 data gradient, both on the forward weight image): every
element of the raw binding against fp64 with a bound from the arithmetic, HipConv2dFn bit-exact on an integer lattice,
and the batched 2-D engine with the kernel against the path it replaces."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = [  # G, B, cin, cout, k, pad, H, W
    (2, 2, 64, 64, 3, 1, 4, 4),      # tile spans samples
    (2, 3, 72, 80, 3, 1, 8, 8),      # ragged channel chunk and ragged co tile, M = 192
    (2, 3, 64, 64, 5, 0, 14, 14),    # M = 300, ragged last tile, runs of 10
    (1, 5, 16, 24, 5, 2, 6, 6),      # pad 2
    (2, 16, 128, 64, 3, 1, 2, 2),    # 32 runs per tile, taps mostly padding
    (1, 2, 8, 20, 1, 0, 5, 5),       # k = 1, cout not a multiple of 8: its data gradient is not served
    (1, 2, 64, 64, 3, 1, 5, 7),      # non-square
    (1, 1, 64, 136, 7, 3, 3, 3)]     # kernel larger than the map, three co tiles


def _ref(x, w, b, dy, G, pad):
    """fp64 (y without bias, y, dx, dw, db) per client of channels-last x [G B, H, W, cin], dy [G B, Ho, Wo, cout],
    w [G, cout, cin, k, k], b [G, cout]."""
    B, out = x.shape[0] // G, [[] for _ in range(5)]
    for g in range(G):
        xi = x[g * B:(g + 1) * B].double().permute(0, 3, 1, 2).requires_grad_(True)
        wi, bi = w[g].double().requires_grad_(True), b[g].double().requires_grad_(True)
        y = F.conv2d(xi, wi, bi, padding=pad)
        y.backward(dy[g * B:(g + 1) * B].double().permute(0, 3, 1, 2))
        cl = lambda t: t.detach().permute(0, 2, 3, 1)  # noqa: E731
        for o, t in zip(out, (cl(y) - bi.detach(), cl(y), cl(xi.grad), wi.grad[None], bi.grad[None])):
            o.append(t)
    return [torch.cat(o) for o in out]


@functools.lru_cache(maxsize=None)
def _case(case, lattice):
    """CPU operands (x, dy bf16; w, b fp32) and their fp64 references; shared, never modified."""
    G, B, cin, cout, k, pad, H, W = case
    g = torch.Generator().manual_seed(hash(case) % 2 ** 31 + lattice)
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    if lattice:  # |x|, |dy| <= 4, w in {-1, 0, 1} with at most 16 non-zeros per output and per input channel
        draw = lambda s, a: torch.randint(-a, a + 1, s, generator=g).float()  # noqa: E731
        x, dy, b = draw((G * B, H, W, cin), 4), draw((G * B, Ho, Wo, cout), 4), draw((G, cout), 8)
        w = draw((G, cout, cin, k, k), 1)
        for perm in ((0, 1, 2, 3, 4), (0, 2, 1, 3, 4)):  # keep the 16 best random scores of every row / column
            s = (torch.rand(w.shape, generator=g) * (w != 0)).permute(perm).flatten(2)
            w = w * (s >= s.topk(min(16, s.shape[2])).values[..., -1:]).view(w.permute(perm).shape).permute(perm)
        assert int((w != 0).sum((2, 3, 4)).max()) <= 16 and int((w != 0).sum((1, 3, 4)).max()) <= 16
    else:
        x, dy = torch.randn(G * B, H, W, cin, generator=g), torch.randn(G * B, Ho, Wo, cout, generator=g)
        w = torch.randn(G, cout, cin, k, k, generator=g) * (cin * k * k) ** -0.5
        b = 0.1 * torch.randn(G, cout, generator=g)
    x, dy = x.to(torch.bfloat16), dy.to(torch.bfloat16)
    wr = w.to(torch.bfloat16).float()  # the values of the weight image
    return x, dy, w, b, _ref(x, wr, b, dy, G, pad), _ref(x.abs(), wr.abs(), b.abs(), dy.abs(), G, pad)


@pytest.mark.parametrize("case", CASES)
def test_conv2d_fd_every_element_against_fp64_with_guard_rows(case):
    """|got - ref| <= 2^-8 |ref| + (Kp + 8) 2^-24 S, Kp = k k ceil8(c) rounded up to 32 for c contraction channels, S
    the same convolution of the absolute values (plus |bias|): bf16 x bf16 products are exact in fp32, each fp32
    addition errs by at most 2^-24 of a partial sum <= S, the bf16 store by at most 2^-8 of the value.  Outputs are
    NaN-filled and one row longer: every element is written, the guard row is not.  A data gradient outside the
    launcher's rule (contraction cout not a multiple of 8) must raise."""
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine.conv2d_hip import conv2d_fd_served, pack_conv_w
    G, B, cin, cout, k, pad, H, W = case
    x, dy, w, b, (ry0, ry, rdx, _, _), (sy0, sy, sdx, _, _) = _case(case, False)
    m, s = ops.ext(), ops.stream()
    xd, dyd, bd, img = x.cuda(), dy.cuda(), b.cuda(), pack_conv_w(w.cuda())
    runs = [("y+b", xd, bd.data_ptr(), 0, ry, sy, cin), ("y", xd, 0, 0, ry0, sy0, cin), ("dx", dyd, 0, 1, rdx, sdx, cout)]
    for name, inp, bias, dgrad, ref, S, c in runs:
        out = torch.full((ref.numel() // ref.shape[-1] + 1, ref.shape[-1]), float("nan"), device="cuda",
                         dtype=torch.bfloat16)
        launch = lambda: m.conv2d_fd(inp.data_ptr(), img.data_ptr(), bias, out.data_ptr(), G, B, H, W, cin,  # noqa: E731
                                     c, cout, k, pad, dgrad, s)
        assert conv2d_fd_served(k, pad, W, cin, cout, bool(dgrad)) == (c % 8 == 0)
        if c % 8:
            with pytest.raises(ValueError):
                launch()
            continue
        launch()
        torch.cuda.synchronize()
        got = out[:-1].double().cpu().view(ref.shape)
        kp = (k * k * ((c + 7) // 8 * 8) + 31) // 32 * 32
        err = (got - ref).abs()
        bad = ~(err <= 2.0 ** -8 * ref.abs() + (kp + 8) * 2.0 ** -24 * S)
        print(name, "max err", float(err.max()), "non-finite", int((~torch.isfinite(got)).sum()))
        assert not bad.any(), (name, int(bad.sum()), float(err[bad].max()))
        assert bool(torch.isnan(out[-1]).all()), name + ": guard row written"


@pytest.mark.parametrize("case", CASES)
def test_hipconv2dfn_exact_on_integer_lattice(case):
    """Every sum is an integer of magnitude <= 16 * 4 + 8 = 72: exact in fp32 in any order and a bf16 value, so y and
    x.grad (conv2d_fd where served) and w.grad / b.grad (the existing kernels, behind the saved-tensor change) equal
    the fp64 reference bit for bit."""
    from neuroimagedisttraining_amd.engine.conv2d_hip import HipConv2dFn
    G, B, cin, cout, k, pad, H, W = case
    x, dy, w, b, (_, ry, rdx, rdw, rdb), _ = _case(case, True)
    xn = x.cuda().permute(0, 3, 1, 2).requires_grad_(True)
    wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = HipConv2dFn.apply(xn, wd, bd, G, pad)
    y.backward(dy.cuda().permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    for name, got, ref in (("y", y.detach().permute(0, 2, 3, 1), ry), ("dx", xn.grad.permute(0, 2, 3, 1), rdx),
                           ("dw", wd.grad, rdw), ("db", bd.grad, rdb)):
        assert torch.equal(got.double().cpu(), ref), (name, int((got.double().cpu() != ref).sum()))


def test_batched2d_convs_run_on_conv2d_fd_and_match_conv2d_any(monkeypatch):
    """A train step and an evaluation of cnn_cifar10 with NIDT_B2D_FD = 1 and 0 on the same rows; with 1 no transposed
    weight image is packed (conv2's data gradient reads the forward image), with 0 conv2 packs one."""
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine.batched2d import BatchedModuleEngine
    from neuroimagedisttraining_amd.engine.executor import padded_rows
    from neuroimagedisttraining_amd.engine.resnet2d_hip import CIFAR_MEAN, CIFAR_STD
    from neuroimagedisttraining_amd.models import create_model
    Gc, B = 4, 8
    torch.manual_seed(1)
    model = create_model("cnn_cifar10", dataset="cifar10", class_num=10)
    x8 = torch.randint(0, 256, (Gc * B, 32, 32, 3), dtype=torch.uint8)
    y = torch.randint(0, 10, (Gc * B,))
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cuda()
    rows = flat.expand(Gc, -1) + torch.randn(Gc, flat.numel(), device="cuda") * 0.01
    real, packs_t = ops.ext(), []

    class Ext:  # the extension with conv2d_pack_w's transposed-image argument recorded
        def __getattr__(self, name):
            return getattr(real, name)

        def conv2d_pack_w(self, w, ldw, img, imgt, *rest):
            packs_t.append(imgt != 0)
            return real.conv2d_pack_w(w, ldw, img, imgt, *rest)

    monkeypatch.setattr(ops, "ext", Ext)
    out, npack = {}, {}
    for fd in ("1", "0"):
        monkeypatch.setenv("NIDT_B2D_FD", fd)
        eng = BatchedModuleEngine(create_model("cnn_cifar10", dataset="cifar10", class_num=10), x8, y, "cuda",
                                  CIFAR_MEAN, CIFAR_STD)
        assert eng.uses_hip_layers
        theta = padded_rows(Gc, eng.players.total, "cuda")
        theta.copy_(rows)
        grads = padded_rows(Gc, eng.players.total, "cuda")
        idx = torch.arange(Gc * B, dtype=torch.int32, device="cuda")
        del packs_t[:]
        loss = eng.train_step(theta, None, grads, idx, Gc, B, 1.0, 7)
        logits = eng.eval_logits(theta, None, idx, Gc, B)
        torch.cuda.synchronize()
        npack[fd] = (len(packs_t), sum(packs_t))
        out[fd] = (loss.float().cpu(), grads.float().cpu(), logits.float().cpu())
    assert npack["1"][0] == npack["0"][0] > 0 and npack["1"][1] == 0 and npack["0"][1] >= 1, npack
    assert torch.allclose(out["1"][0], out["0"][0], rtol=2e-2, atol=2e-2), (out["1"][0], out["0"][0])
    assert float((out["1"][2] - out["0"][2]).norm() / out["0"][2].norm()) < 3e-2
    for g in range(Gc):
        a, b = out["1"][1][g], out["0"][1][g]
        assert float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.99, g
