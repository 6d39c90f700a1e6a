"""linear_g.hip (client-grouped Linear forward, data gradient, weight / bias gradient on the fp32 rows in place):
every element against fp64 with bounds from the arithmetic, bit-exact on an integer lattice, and reached from the
batched 2-D engine."""
import pytest
import torch

pytestmark = pytest.mark.gpu

G = 3
SHAPES = [(1, 8, 1), (5, 33, 10), (16, 84, 10), (33, 120, 84), (65, 400, 120), (128, 512, 10), (8, 1600, 384)]
U = 2.0 ** -23


def _ref(x, dy, w, bias):
    """fp64 results and the fp64 sums of |products| (S) for y, dx, dw, db from [G, B, *] / [G, N, K] operands."""
    xd, dd, wd = x.double(), dy.double(), w.to(torch.bfloat16).double()
    e = torch.einsum
    y = e("gbk,gnk->gbn", xd, wd) + (bias.double().unsqueeze(1) if bias is not None else 0)
    sy = e("gbk,gnk->gbn", xd.abs(), wd.abs()) + (bias.double().abs().unsqueeze(1) if bias is not None else 0)
    return ((y, sy), (e("gbn,gnk->gbk", dd, wd), e("gbn,gnk->gbk", dd.abs(), wd.abs())),
            (e("gbn,gbk->gnk", dd, xd), e("gbn,gbk->gnk", dd.abs(), xd.abs())), (dd.sum(1), dd.abs().sum(1)))


@pytest.mark.parametrize("has_b", [True, False])
@pytest.mark.parametrize("B,K,N", SHAPES)
def test_linear_g_every_element_against_fp64_with_guards(B, K, N, has_b):
    """|err| <= 2^-8 |ref| + (Lp + 8) 2^-23 S for the bf16 outputs (y, dx) and (Lp + 8) 2^-23 S for the fp32 ones
    (dw; db with B + 8), Lp the contraction length rounded up to 32: bf16 x bf16 products are exact in fp32, each
    fp32 addition errs by at most 2^-23 of a partial sum <= S, a bf16 store by at most 2^-8 of the value.  The weights sit
    4-byte aligned in NaN-filled rows; the gradients land in sentinel-filled rows that must stay untouched elsewhere."""
    from neuroimagedisttraining_amd import ops
    m, dev = ops.ext(), "cuda"
    torch.manual_seed(B * 131 + K * 7 + N)
    off_w = 3
    off_b = off_w + N * K + 5
    ld = off_b + N + 13
    P = torch.full((G, ld), float("nan"), device=dev)
    w, bias = P[:, off_w:off_w + N * K].view(G, N, K), P[:, off_b:off_b + N]
    w.copy_(torch.randn(G, N, K, device=dev) * K ** -0.5)
    bias.copy_(0.1 * torch.randn(G, N, device=dev))
    x = torch.randn(G * B, K, device=dev).to(torch.bfloat16)
    dy = torch.randn(G * B, N, device=dev).to(torch.bfloat16)
    sent = -7.25e11
    Q = torch.full((G, ld), sent, device=dev)
    dw, db = Q[:, off_w:off_w + N * K].view(G, N, K), Q[:, off_b:off_b + N]
    y = torch.empty(G * B, N, device=dev, dtype=torch.bfloat16)
    dx = torch.empty(G * B, K, device=dev, dtype=torch.bfloat16)
    s = ops.stream()
    m.linear_g_fwd(x.data_ptr(), w.data_ptr(), ld, bias.data_ptr() if has_b else 0, ld, y.data_ptr(), G, B, K, N, s)
    m.linear_g_dgrad(dy.data_ptr(), w.data_ptr(), ld, dx.data_ptr(), G, B, K, N, s)
    m.linear_g_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ld, db.data_ptr() if has_b else 0, ld, G, B, K, N, s)
    torch.cuda.synchronize()
    (ry, sy), (rdx, sdx), (rdw, sdw), (rdb, sdb) = _ref(x.view(G, B, K), dy.view(G, B, N), w, bias if has_b else None)
    lp = lambda n: (n + 31) // 32 * 32 + 8  # noqa: E731
    checks = [("y", y.view(G, B, N), ry, 2.0 ** -8, lp(K) * U * sy),
              ("dx", dx.view(G, B, K), rdx, 2.0 ** -8, lp(N) * U * sdx), ("dw", dw, rdw, 0.0, lp(B) * U * sdw)]
    if has_b:
        checks.append(("db", db, rdb, 0.0, (B + 8) * U * sdb))
    for name, got, ref, rel, ab in checks:
        err = (got.double() - ref).abs()
        bad = ~(err <= rel * ref.abs() + ab)
        assert not bad.any(), (name, int(bad.sum()), float(err.max()))
    keep = torch.ones(G, ld, dtype=torch.bool, device=dev)
    keep[:, off_w:off_w + N * K] = False
    if has_b:
        keep[:, off_b:off_b + N] = False
    bits = torch.tensor(sent, device=dev).view(torch.int32)
    assert bool((Q.view(torch.int32)[keep] == bits).all()), "linear_g_wgrad wrote outside the dw / db blocks"


@pytest.mark.parametrize("B,K,N", [(5, 33, 10), (33, 120, 84), (65, 200, 65)])
def test_linear_g_exact_on_integer_lattice(B, K, N):
    """Operands in {-1, 0, 1} (bias in {-2..2}): every sum is an integer of magnitude <= 202 < 256, exact in fp32 in
    any order and representable in bf16, so HipLinearFn must equal the fp64 reference bit for bit."""
    from neuroimagedisttraining_amd.engine.conv2d_hip import HipLinearFn
    dev = "cuda"
    torch.manual_seed(B + K + N)
    P = torch.zeros(G, N * K + N, device=dev)
    P[:, :N * K] = torch.randint(-1, 2, (G, N * K), device=dev).float()
    P[:, N * K:] = torch.randint(-2, 3, (G, N), device=dev).float()
    w = P[:, :N * K].view(G, N, K).requires_grad_(True)
    bias = P[:, N * K:].requires_grad_(True)
    x = torch.randint(-1, 2, (G * B, K), device=dev).to(torch.bfloat16).requires_grad_(True)
    dy = torch.randint(-1, 2, (G * B, N), device=dev).to(torch.bfloat16)
    y = HipLinearFn.apply(x, w, bias, G)
    y.backward(dy)
    torch.cuda.synchronize()
    (ry, _), (rdx, _), (rdw, _), (rdb, _) = _ref(x.detach().view(G, B, K), dy.view(G, B, N), w.detach(), bias.detach())
    assert y.dtype == torch.bfloat16 and x.grad.dtype == torch.bfloat16 and w.grad.dtype == torch.float32
    assert torch.equal(y.detach().double().view(G, B, N), ry)
    assert torch.equal(x.grad.double().view(G, B, K), rdx)
    assert torch.equal(w.grad.double(), rdw)
    assert torch.equal(bias.grad.double(), rdb)


@pytest.mark.parametrize("name,ds", [("lenet5", "mnist"), ("cnn_cifar10", "cifar10")])
def test_batched2d_linears_run_on_linear_g_and_match_library_gemm(name, ds, monkeypatch):
    """A train step and an evaluation of the batched 2-D engine with the linear layers on linear_g.hip against the
    batched library GEMM (NIDT_B2D_LINEAR=0) on the same rows; the kernel run issues no aten matrix product."""
    from neuroimagedisttraining_amd.engine.batched2d import BatchedModuleEngine
    from neuroimagedisttraining_amd.engine.executor import padded_rows
    from neuroimagedisttraining_amd.engine.resnet2d_hip import CIFAR_MEAN, CIFAR_STD
    from neuroimagedisttraining_amd.models import create_model
    Gc, B = 4, 8
    torch.manual_seed(1)
    model = create_model(name, dataset=ds, class_num=10)
    c, S = (1, 28) if ds == "mnist" else (3, 32)
    x8 = torch.randint(0, 256, (Gc * B, S, S, c), dtype=torch.uint8)
    y = torch.randint(0, 10, (Gc * B,))
    mean, std = ((0.1307,), (0.3081,)) if c == 1 else (CIFAR_MEAN, CIFAR_STD)
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cuda()
    rows = flat.expand(Gc, -1) + torch.randn(Gc, flat.numel(), device="cuda") * 0.01
    out = {}
    for hip in ("1", "0"):
        monkeypatch.setenv("NIDT_B2D_LINEAR", hip)
        eng = BatchedModuleEngine(create_model(name, dataset=ds, class_num=10), x8, y, "cuda", mean, std)
        assert eng.uses_hip_layers
        theta = padded_rows(Gc, eng.players.total, "cuda")
        theta.copy_(rows)
        grads = padded_rows(Gc, eng.players.total, "cuda")
        idx = torch.arange(Gc * B, dtype=torch.int32, device="cuda")
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            loss = eng.train_step(theta, None, grads, idx, Gc, B, 1.0, 7)
            logits = eng.eval_logits(theta, None, idx, Gc, B)
            torch.cuda.synchronize()
        gemms = {e.name for e in prof.events()} & {"aten::bmm", "aten::baddbmm", "aten::addmm", "aten::mm"}
        assert bool(gemms) == (hip == "0"), gemms
        out[hip] = (loss.float().cpu(), grads.float().cpu(), logits.float().cpu())
    assert torch.allclose(out["1"][0], out["0"][0], rtol=2e-2, atol=2e-2), (out["1"][0], out["0"][0])
    assert float((out["1"][2] - out["0"][2]).norm() / out["0"][2].norm()) < 3e-2
    for g in range(Gc):
        a, b = out["1"][1][g], out["0"][1][g]
        assert float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.99, g
