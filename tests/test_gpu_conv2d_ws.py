"""conv2d_ws.hip (conv forward and stride-1 data gradient on the clients' fp32 weight blocks read in place): every
element of the raw binding against fp64 with a bound from the arithmetic, HipConv2dFn bit-exact on an integer lattice
with no weight image packed, and the batched 2-D engine with the kernel against the path it replaces."""
import pytest
import torch

from test_gpu_conv2d_fd import _case  # the shared operands and fp64 references (cached, never modified)

pytestmark = pytest.mark.gpu

CASES = [  # G, B, cin, cout, k, pad, H, W
    (2, 2, 64, 64, 3, 1, 4, 4),      # tile spans samples
    (2, 3, 72, 80, 3, 1, 8, 8),      # ragged chunk, ragged channel tile, M = 192
    (2, 16, 128, 64, 3, 1, 2, 2),    # 16 samples per tile, taps mostly padding
    (1, 5, 16, 24, 3, 0, 6, 6),      # pad 0, tile starts mid-sample
    (1, 2, 8, 20, 1, 0, 5, 5),       # k = 1; its data gradient has a contraction of 20: not served
    (1, 2, 64, 64, 3, 1, 5, 7),      # non-square
    (1, 1, 64, 136, 2, 1, 3, 3),     # even kernel, three channel tiles
    (1, 1, 32, 64, 3, 2, 3, 3),      # pad above (k - 1) / 2
    (1, 5, 24, 64, 3, 1, 8, 8),      # M = 320: 256-position tiles of four whole samples, ragged second tile
    (1, 3, 16, 72, 3, 1, 10, 10)]    # M = 300: 256-position tiles that straddle samples
UNSERVED = [(1, 1, 8, 8, 5, 2, 6, 6), (1, 1, 8, 8, 3, 1, 32, 32)]  # k = 5; a 32 x 32 map (1156 slab rows)


def _in_nan_rows(t, G):
    """t [G, n] fp32 -> the same values as client blocks at stride n + 37, the first 3 floats into a NaN-filled
    buffer (4-byte but not 16-byte aligned): (buffer, view of client 0's block, stride)."""
    n = t[0].numel()
    buf = torch.full((3 + G * (n + 37),), float("nan"), device="cuda")
    buf[3:].view(G, n + 37)[:, :n] = t.reshape(G, n).cuda()
    return buf, buf[3:], n + 37


@pytest.mark.parametrize("case", CASES + UNSERVED)
def test_conv2d_ws_every_element_against_fp64_with_guard_rows(case):
    """|got - ref| <= 2^-8 |ref| + (N + 8) 2^-24 S, N = 32 ceil(2 k k / 4) ceil(c / 16) for c contraction channels (the
    kernel walks 16-channel chunks and adds ceil(2 k k / 4) 32-deep MFMAs of (tap, octet) k-groups per chunk into one
    accumulator, zero padding included), S the same convolution of the absolute values (plus |bias|): bf16 x bf16
    products are exact in fp32, each fp32 addition errs by at most 2^-24 of a partial sum <= S, the bf16 store by at
    most 2^-8 of the value.  The fp32 weights and bias lie in NaN-filled buffers at a ragged client stride: nothing
    outside a client's block reaches the result.  Outputs are NaN-filled and one row longer: every element is written,
    the guard row is not.  A direction outside the launcher's rule must raise, and conv2d_ws_served says which."""
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine.conv2d_hip import conv2d_ws_served
    G, B, cin, cout, k, pad, H, W = case
    x, dy, w, b, (ry0, ry, rdx, _, _), (sy0, sy, sdx, _, _) = _case(case, False)
    m, s = ops.ext(), ops.stream()
    xd, dyd = x.cuda(), dy.cuda()
    (wbuf, w0, ldw), (bbuf, b0, ldb) = _in_nan_rows(w, G), _in_nan_rows(b, G)
    runs = [("y+b", xd, b0.data_ptr(), 0, ry, sy, cin), ("y", xd, 0, 0, ry0, sy0, cin), ("dx", dyd, 0, 1, rdx, sdx, cout)]
    for name, inp, bias, dgrad, ref, S, c in runs:
        out = torch.full((ref.numel() // ref.shape[-1] + 1, ref.shape[-1]), float("nan"), device="cuda",
                         dtype=torch.bfloat16)
        launch = lambda: m.conv2d_ws(inp.data_ptr(), w0.data_ptr(), ldw, bias, ldb, out.data_ptr(), G, B, H, W,  # noqa: E731
                                     cin, c, cout, k, pad, dgrad, s)
        served = case not in UNSERVED and c % 8 == 0
        assert conv2d_ws_served(k, pad, B, H, W, cin, cout, bool(dgrad)) == served
        if not served:
            with pytest.raises(ValueError):
                launch()
            continue
        launch()
        torch.cuda.synchronize()
        got = out[:-1].double().cpu().view(ref.shape)
        n = 32 * ((2 * k * k + 3) // 4) * ((c + 15) // 16)
        err = (got - ref).abs()
        bad = ~(err <= 2.0 ** -8 * ref.abs() + (n + 8) * 2.0 ** -24 * S)
        print(name, "max err", float(err.max()), "non-finite", int((~torch.isfinite(got)).sum()))
        assert not bad.any(), (name, int(bad.sum()), float(err[bad].max()))
        assert bool(torch.isnan(out[-1]).all()), name + ": guard row written"


class _CountPacks:
    """The extension with its conv2d_pack_w launches counted."""

    def __init__(self, real):
        self.real, self.packs = real, 0

    def __call__(self):
        return self

    def __getattr__(self, name):
        return getattr(self.real, name)

    def conv2d_pack_w(self, *args):
        self.packs += 1
        return self.real.conv2d_pack_w(*args)


@pytest.mark.parametrize("case", CASES)
def test_hipconv2dfn_on_conv2d_ws_exact_on_integer_lattice_without_pack(case, monkeypatch):
    """Every sum is an integer of magnitude <= 16 * 4 + 8 = 72: exact in fp32 in any order and a bf16 value, so with
    NIDT_B2D_WS=2 y and x.grad (conv2d_ws where served) and w.grad / b.grad (the existing kernels) equal the fp64
    reference bit for bit; a layer whose two directions are both served launches no conv2d_pack_w."""
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine.conv2d_hip import HipConv2dFn, conv2d_ws_served
    G, B, cin, cout, k, pad, H, W = case
    x, dy, w, b, (_, ry, rdx, rdw, rdb), _ = _case(case, True)
    ext = _CountPacks(ops.ext())
    monkeypatch.setattr(ops, "ext", ext)
    monkeypatch.setenv("NIDT_B2D_WS", "2")
    xn = x.cuda().permute(0, 3, 1, 2).requires_grad_(True)
    wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = HipConv2dFn.apply(xn, wd, bd, G, pad)
    y.backward(dy.cuda().permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    for name, got, ref in (("y", y.detach().permute(0, 2, 3, 1), ry), ("dx", xn.grad.permute(0, 2, 3, 1), rdx),
                           ("dw", wd.grad, rdw), ("db", bd.grad, rdb)):
        assert torch.equal(got.double().cpu(), ref), (name, int((got.double().cpu() != ref).sum()))
    both = all(conv2d_ws_served(k, pad, B, H, W, cin, cout, d) for d in (False, True))
    assert both == (cout % 8 == 0) and (ext.packs == 0) == both, (both, ext.packs)


def test_batched2d_vgg11_runs_on_conv2d_ws_and_matches_the_packed_path(monkeypatch):
    """A train step and an evaluation of vgg11 with NIDT_B2D_WS = 2 and 0 on the same rows (the tolerances of the
    conv2d_fd engine test, which makes the same kind of comparison); with 2 fewer conv2d_pack_w launches."""
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine.batched2d import BatchedModuleEngine
    from neuroimagedisttraining_amd.engine.executor import padded_rows
    from neuroimagedisttraining_amd.engine.resnet2d_hip import CIFAR_MEAN, CIFAR_STD
    from neuroimagedisttraining_amd.models import create_model
    Gc, B = 4, 8
    torch.manual_seed(1)
    model = create_model("vgg11", dataset="cifar10", class_num=10)
    x8 = torch.randint(0, 256, (Gc * B, 32, 32, 3), dtype=torch.uint8)
    y = torch.randint(0, 10, (Gc * B,))
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cuda()
    rows = flat.expand(Gc, -1) + torch.randn(Gc, flat.numel(), device="cuda") * 0.01
    ext = _CountPacks(ops.ext())
    monkeypatch.setattr(ops, "ext", ext)
    out, npack = {}, {}
    for ws in ("2", "0"):
        monkeypatch.setenv("NIDT_B2D_WS", ws)
        eng = BatchedModuleEngine(create_model("vgg11", dataset="cifar10", class_num=10), x8, y, "cuda", CIFAR_MEAN,
                                  CIFAR_STD)
        assert eng.uses_hip_layers
        theta = padded_rows(Gc, eng.players.total, "cuda")
        theta.copy_(rows)
        grads = padded_rows(Gc, eng.players.total, "cuda")
        idx = torch.arange(Gc * B, dtype=torch.int32, device="cuda")
        ext.packs = 0
        loss = eng.train_step(theta, None, grads, idx, Gc, B, 1.0, 7)
        logits = eng.eval_logits(theta, None, idx, Gc, B)
        torch.cuda.synchronize()
        npack[ws] = ext.packs
        out[ws] = (loss.float().cpu(), grads.float().cpu(), logits.float().cpu())
    assert 0 <= npack["2"] < npack["0"], npack
    assert torch.allclose(out["2"][0], out["0"][0], rtol=2e-2, atol=2e-2), (out["2"][0], out["0"][0])
    assert float((out["2"][2] - out["0"][2]).norm() / out["0"][2].norm()) < 3e-2
    for g in range(Gc):
        a, b = out["2"][1][g], out["0"][1][g]
        assert float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.99, g
