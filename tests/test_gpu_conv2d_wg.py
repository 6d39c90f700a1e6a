"""conv2d_wg.hip (MFMA conv weight / bias gradient in the parameter layout, and the weight-image pack): every element
against fp64 with bounds from the arithmetic, bit-exact on the integer lattice, the pack against the framework
packing byte for byte, and the batched 2-D engine with the kernel against the staged fp32 path it replaces."""
import functools

import pytest
import torch

import _lattice as L

pytestmark = pytest.mark.gpu

G = 3
CASES = [  # cin, cout, k, pad, H, B
    (1, 20, 5, 0, 12, 3), (3, 6, 5, 0, 9, 4), (6, 16, 5, 0, 7, 4), (20, 50, 5, 0, 8, 2), (32, 64, 5, 2, 7, 3),
    (72, 72, 3, 1, 6, 2), (16, 8, 3, 1, 2, 5), (8, 8, 1, 0, 5, 1)]
SENT = -7.25e11


def _wgrad64(x, dy, k, pad, groups):
    """fp64 CPU weight gradient per client of channels-last x [groups B, H, W, cin], dy [groups B, Ho, Wo, cout]."""
    B, cin, cout = x.shape[0] // groups, x.shape[-1], dy.shape[-1]
    return torch.stack([torch.nn.grad.conv2d_weight(
        x[g * B:(g + 1) * B].double().permute(0, 3, 1, 2).contiguous(), (cout, cin, k, k),
        dy[g * B:(g + 1) * B].double().permute(0, 3, 1, 2).contiguous(), padding=pad) for g in range(groups)])


@functools.lru_cache(maxsize=None)
def _case(cin, cout, k, pad, H, B, lattice):
    """(x, dy, dw, sum |dy||x|, db, sum |dy|): CPU operands (bf16) and fp64 references; shared, never modified."""
    g = L.gen("conv2d_wg", cin, cout, k, pad, H, B, lattice)
    draw = (lambda s: L.int_acts(s, g)) if lattice else (lambda s: torch.randn(s, generator=g).to(torch.bfloat16))
    Ho = H + 2 * pad - k + 1
    x, dy = draw((G * B, H, H, cin)), draw((G * B, Ho, Ho, cout))
    dd = dy.double().view(G, -1, cout)
    return x, dy, _wgrad64(x, dy, k, pad, G), _wgrad64(x.abs(), dy.abs(), k, pad, G), dd.sum(1), dd.abs().sum(1)


def _run(case, x, dy, has_b=True):
    """conv2d_wg into sentinel rows at odd offsets: (rows, dw view, db view, mask of the elements outside both)."""
    from neuroimagedisttraining_amd import ops
    cin, cout, k, pad, H, B = case
    nw = cout * cin * k * k
    off_w, off_b = 3, 3 + nw + 5
    ld = off_b + cout + 13
    Q = torch.full((G, ld), SENT, device="cuda")
    xd, dyd = x.cuda(), dy.cuda()
    ops.ext().conv2d_wg(xd.data_ptr(), dyd.data_ptr(), Q[:, off_w:].data_ptr(), ld,
                        Q[:, off_b:].data_ptr() if has_b else 0, ld, G, B, H, H, cin, cin, cout, k, pad, ops.stream())
    torch.cuda.synchronize()
    keep = torch.ones(G, ld, dtype=torch.bool, device="cuda")
    keep[:, off_w:off_w + nw] = False
    if has_b:
        keep[:, off_b:off_b + cout] = False
    return Q, Q[:, off_w:off_w + nw].view(G, cout, cin, k, k), Q[:, off_b:off_b + cout], keep


@pytest.mark.parametrize("case,has_b", [(c, i != 4) for i, c in enumerate(CASES)])
def test_conv2d_wg_every_element_against_fp64_with_guards(case, has_b):
    """|got - ref| <= M 2^-24 sum_m |dy||x| for dW and M 2^-24 sum_m |dy| for dB (M = B Ho Wo): products of two bf16
    values are exact in fp32, so only the M fp32 additions err, each by at most 2^-24 of a partial sum that the sum of
    absolute values bounds.  Every sentinel outside the written blocks stays."""
    cin, cout, k, pad, H, B = case
    x, dy, rdw, sdw, rdb, sdb = _case(*case, False)
    Q, dw, db, keep = _run(case, x, dy, has_b)
    M = B * (H + 2 * pad - k + 1) ** 2
    for name, got, ref, s in [("dw", dw, rdw, sdw)] + ([("db", db, rdb, sdb)] if has_b else []):
        err = (got.double().cpu() - ref).abs()
        bad = ~(err <= M * 2.0 ** -24 * s)
        print(name, "max err", float(err.max()), "max bound", float(M * 2.0 ** -24 * s.max()))
        assert not bad.any(), (name, int(bad.sum()), float(err.max()))
    bits = torch.tensor(SENT, device="cuda").view(torch.int32)
    assert bool((Q.view(torch.int32)[keep] == bits).all()), "conv2d_wg wrote outside the dw / db blocks"


@pytest.mark.parametrize("case", CASES)
def test_conv2d_wg_exact_on_integer_lattice_and_reproducible(case):
    """Operands in {-2..2}: every partial sum is an integer below 2^24 in any order, so dW and dB equal fp64 bit for
    bit; and two calls on the same random operands give the same bits."""
    x, dy, rdw, _, rdb, _ = _case(*case, True)
    L.require_fp32_exact(4.0 * dy.numel() / (G * dy.shape[-1]), "conv2d_wg lattice")
    _, dw, db, _ = _run(case, x, dy)
    L.assert_exact(dw, rdw, ("client", "co", "ci", "kh", "kw"))
    L.assert_exact(db, rdb, ("client", "co"))
    x, dy = _case(*case, False)[:2]
    assert torch.equal(_run(case, x, dy)[0].view(torch.int32), _run(case, x, dy)[0].view(torch.int32))


@pytest.mark.parametrize("cin,cout,k", sorted({c[:3] for c in CASES}))
def test_conv2d_pack_w_bytes_equal_framework_packing(cin, cout, k):
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine.conv2d_hip import pack_conv_w, pack_conv_wt
    torch.manual_seed(cin + cout + k)
    nw = cout * cin * k * k
    rows = torch.randn(G, nw + 11, device="cuda")
    w = rows[:, 3:3 + nw].view(G, cout, cin, k, k)
    ref = [pack_conv_w(w).view(torch.int16), pack_conv_wt(w).view(torch.int16)]
    for both in (True, False):
        img = [torch.full_like(r, 0x7f7f) for r in ref]
        ops.ext().conv2d_pack_w(w.data_ptr(), rows.stride(0), img[0].data_ptr(), img[1].data_ptr() if both else 0, G,
                                cout, cin, k, ops.stream())
        torch.cuda.synchronize()
        assert torch.equal(img[0], ref[0])
        assert torch.equal(img[1], ref[1] if both else torch.full_like(ref[1], 0x7f7f))


@pytest.mark.parametrize("name", ["cnn_cifar10", "vgg11"])
def test_batched2d_step_on_conv2d_wg_matches_staged_wgrad(name, monkeypatch):
    """One train step with NIDT_B2D_WGRAD = 1 and 0 on the same rows: equal losses (same packed bytes, same forward),
    and conv weight gradients within the sum of the two paths' summation bounds, 2 M 2^-24 sum |dy||x| per element,
    from the layers' own bf16 inputs and output gradients (recorded by module hooks in the first run).  The
    block-count rule of conv2d_wg_ok would keep the staged kernel for most layers at 4 clients, so it is switched off:
    every conv layer of both models (5 x 5 and 3 x 3, narrow and 64-wide tiles) goes through HipConv2dFn to
    conv2d_wg in the first run, which is asserted per layer."""
    from neuroimagedisttraining_amd.engine.batched2d import BatchedModuleEngine
    from neuroimagedisttraining_amd.engine import conv2d_hip
    from neuroimagedisttraining_amd.engine.executor import padded_rows
    from neuroimagedisttraining_amd.engine.resnet2d_hip import CIFAR_MEAN, CIFAR_STD
    from neuroimagedisttraining_amd.models import create_model
    Gc, B = 4, 8
    torch.manual_seed(1)
    model = create_model(name, dataset="cifar10", class_num=10)
    x8 = torch.randint(0, 256, (Gc * B, 32, 32, 3), dtype=torch.uint8)
    y = torch.randint(0, 10, (Gc * B,))
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cuda()
    rows = flat.expand(Gc, -1) + torch.randn(Gc, flat.numel(), device="cuda") * 0.01
    out, seen = {}, {}
    monkeypatch.setattr(conv2d_hip, "WG_MIN_BLOCKS", 0)
    for new in ("1", "0"):
        monkeypatch.setenv("NIDT_B2D_WGRAD", new)
        eng = BatchedModuleEngine(create_model(name, dataset="cifar10", class_num=10), x8, y, "cuda", CIFAR_MEAN,
                                  CIFAR_STD)
        assert eng.uses_hip_layers

        def record(mod, inp, outp):
            seen[mod.name] = [mod.pad, inp[0].detach()]
            outp.register_hook(lambda g: seen[mod.name].append(g))

        if new == "1":
            for mod in eng._grouped[0].modules():
                if isinstance(mod, conv2d_hip.GConv2d):
                    mod.register_forward_hook(record)
        theta = padded_rows(Gc, eng.players.total, "cuda")
        theta.copy_(rows)
        grads = padded_rows(Gc, eng.players.total, "cuda")
        loss = eng.train_step(theta, None, grads, torch.arange(Gc * B, dtype=torch.int32, device="cuda"), Gc, B, 1.0, 7)
        torch.cuda.synchronize()
        out[new] = (loss.float().cpu(), grads.float().cpu())
    assert torch.equal(out["1"][0], out["0"][0])
    P = eng.players
    assert seen
    for lname, (pad, x, gy) in seen.items():
        i = P.names.index(lname + ".weight")
        shp, o = tuple(P.shapes[i]), P.offsets[i]
        cl = lambda t: t.to(torch.bfloat16).permute(0, 2, 3, 1).cpu().abs()  # noqa: E731
        s = _wgrad64(cl(x), cl(gy), shp[-1], pad, Gc)
        M = B * gy.shape[2] * gy.shape[3]
        assert conv2d_hip.conv2d_wg_ok(shp[-1], gy.shape[3], Gc, shp[1], shp[0]), lname
        a, b = (out[v][1][:Gc, o:o + s[0].numel()].view((Gc,) + shp).double() for v in "10")
        err, bound = (a - b).abs(), 2 * M * 2.0 ** -24 * s
        print(lname, "rel", float(err.norm() / b.norm()), "max err / bound", float((err / (bound + 1e-300)).max()))
        assert bool((err <= bound).all()), (lname, float(err.max()))
