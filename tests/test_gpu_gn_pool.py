"""gn_pool.hip (GroupNorm + ReLU + 2x2 max-pool of the batched 2-D zoo, and the plain pool): the forward against fp64
per element, the backward bit-exact on an integer lattice with supplied dyadic statistics, the pool against torch's fp64
CPU max_pool2d, and the batched 2-D engine with the kernels against the framework path they replace."""
import functools

import pytest
import torch
import torch.nn.functional as F

from _normlattice import (GN_EPS, K_GN_BWD, K_GN_FWD, U32, assert_within, bf16_bound, dyadic_stats, ints, rstd_error,
                          theta_rows)

pytestmark = pytest.mark.gpu

CASES = [  # G, B, H, W, C, groups, relu, pool
    (2, 3, 2, 2, 512, 32, 1, 1),    # several samples per block, ragged at the client boundary, 1x1 pooled map
    (2, 3, 4, 4, 64, 32, 1, 1),     # four groups inside one chunk
    (1, 2, 8, 8, 256, 32, 1, 0),    # no pool, cg = 8
    (2, 1, 6, 10, 128, 32, 1, 1),   # non-square map, divisor not a power of two
    (1, 1, 32, 32, 64, 32, 1, 1),   # the largest register-resident sample
    (1, 2, 4, 4, 32, 32, 0, 1),     # cg = 1, pool without ReLU
    (1, 2, 2, 2, 16, 2, 1, 0)]      # the narrowest chunk column count


def _pool(v, pool):
    """[N, H, W, C] -> the 2x2 window maximum (or v itself)."""
    return F.max_pool2d(v.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1) if pool else v


def _per_channel(s, B, cg):
    """per-(sample, group) [N, groups] or per-(client, channel) [G, C] -> [N, 1, 1, C]."""
    s = s.repeat_interleave(cg, 1) if cg else s.repeat_interleave(B, 0)
    return s[:, None, None, :]


@functools.lru_cache(maxsize=None)
def _fwd_case(case):
    """Random operands and the fp64 reference group_norm -> affine -> relu -> max_pool2d on the bf16 values of t, with
    the bound E = K_GN_FWD 2^-24 sum |terms| + the propagated error of the two-pass statistics (gn_stats_error's
    count, for any group count); a window's bound is the largest of its four (max and ReLU are 1-Lipschitz)."""
    G, B, H, W, C, groups, relu, pool = case
    g = torch.Generator().manual_seed(hash(case) % 2 ** 31)
    N, cg, n = G * B, C // groups, H * W * (C // groups)
    t = (torch.randn(N, H, W, C, generator=g) + 1.0).to(torch.bfloat16)
    theta = torch.randn(G, 2 * C + 24, generator=g)
    x = t.double()
    xg = x.view(N, H * W, groups, cg)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    rstd = 1.0 / torch.sqrt(var + GN_EPS)
    dmean = (n - 1) * U32 * xg.abs().sum((1, 3)) / n + U32 * mean.abs()
    dvar = (n + 3) * U32 * ((xg - mean[:, None, :, None]).abs() + dmean[:, None, :, None]).pow(2).mean((1, 3)) \
        + dmean ** 2 + 2 * U32 * GN_EPS
    drs = rstd_error(var, dvar, GN_EPS)
    mu, rs, dmu, drs_c = (_per_channel(v, B, cg) for v in (mean, rstd, dmean, drs))
    gam, bet = (_per_channel(theta[:, o:o + C].double(), B, 0) for o in (8, C + 16))
    pre = (x - mu) * rs * gam + bet
    E = K_GN_FWD * U32 * ((x * gam * rs).abs() + (mu * gam * rs).abs() + bet.abs()) \
        + gam.abs() * ((x - mu).abs() * drs_c + (rs + drs_c) * dmu)
    y = _pool(torch.relu(pre) if relu else pre, pool)
    return t, theta, y, bf16_bound(y, _pool(E, pool)), (mean, dmean, rstd, drs)


@pytest.mark.parametrize("case", CASES)
def test_gn2d_fwd_every_element_against_fp64_with_guard_row(case):
    """Outputs are NaN-filled and one row longer: every element is written, the guard row is not.  The saved statistics
    are within the two-pass bounds, and a null stats pointer (evaluation) gives the same y."""
    from neuroimagedisttraining_amd import ops
    G, B, H, W, C, groups, relu, pool = case
    t, theta, ref, bound, (mean, dmean, rstd, drs) = _fwd_case(case)
    m, s = ops.ext(), ops.stream()
    td, th = t.cuda(), theta.cuda()
    rows = ref.numel() // C
    outs = []
    for with_stats in (True, False):
        y = torch.full((rows + 1, C), float("nan"), device="cuda", dtype=torch.bfloat16)
        stats = torch.full((G * B + 1, groups, 2), float("nan"), device="cuda")
        m.gn2d_fwd(td.data_ptr(), th[:, 8:].data_ptr(), th[:, C + 16:].data_ptr(), th.stride(0), y.data_ptr(),
                   stats.data_ptr() if with_stats else 0, G * B, B, H, W, C, groups, 1e-5, relu, pool, s)
        torch.cuda.synchronize()
        print("y: worst err / bound", assert_within(y[:-1].view(ref.shape), ref, bound, "nhwc"))
        assert bool(torch.isnan(y[-1]).all()) and bool(torch.isnan(stats[-1]).all()), "guard row written"
        outs.append(y)
        if with_stats:
            print("mean", assert_within(stats[:-1, :, 0], mean, dmean, "ng"),
                  "rstd", assert_within(stats[:-1, :, 1], rstd, drs, "ng"))
        else:
            assert bool(torch.isnan(stats).all())
    assert torch.equal(outs[0][:-1], outs[1][:-1])


@pytest.mark.parametrize("shape", [(4, 4, 24, 8, 0), (3, 4, 64, 32, 1), (4, 4, 64, 3, 0), (64, 64, 32, 32, 0)])
def test_gn2d_rejects_shapes_outside_the_rule(shape):
    from neuroimagedisttraining_amd import ops
    from neuroimagedisttraining_amd.engine.conv2d_hip import gn2d_ok
    H, W, C, groups, pool = shape
    assert not gn2d_ok(H, W, C, groups, pool)
    assert all(gn2d_ok(c[2], c[3], c[4], c[5], c[7]) for c in CASES)
    buf = torch.zeros(1 << 18, device="cuda")
    p = buf.data_ptr()
    with pytest.raises(ValueError):
        ops.ext().gn2d_fwd(p, p, p, C, p, 0, 1, 1, H, W, C, groups, 1e-5, 1, pool, ops.stream())
    with pytest.raises(ValueError):
        ops.ext().gn2d_bwd(p, p, p, p, p, C, p, p, 1, 1, H, W, C, groups, 1, pool, ops.stream())


@pytest.mark.parametrize("case", CASES)
def test_gn2d_bwd_bit_exact_on_integer_lattice(case):
    """t in [-3, 3], dy in [-2, 2], mean in {-1, 0, 1}, rstd in {1/4, 1/2, 1}, gamma in {+-1, +-2}, integer beta: z is a
    multiple of 1/4, every sum is a short dyadic rational (exact in fp32 in any order), ties between positive window
    entries are frequent.  Reference: dy routed through the first maximum of each window of z, masked by z > 0, then
    dt = rstd (d gamma - m1 - xhat m2) in fp64.  dt equals ref.to(bfloat16) bit for bit where H W cg is a power of two
    (else within K_GN_BWD roundings: the expression is k_gn_bwd's), the summed partials equal the fp64 sums."""
    from neuroimagedisttraining_amd import ops
    G, B, H, W, C, groups, relu, pool = case
    g = torch.Generator().manual_seed(hash(case) % 2 ** 31 + 1)
    N, cg = G * B, C // groups
    t = ints((N, H, W, C), -3, 3, g)
    dy = ints((N, H // 2, W // 2, C) if pool else (N, H, W, C), -2, 2, g)
    stats = dyadic_stats((N, groups), g)
    theta, off_w, off_b = theta_rows(G, C, g)
    mu, rs = (_per_channel(stats[:, :, i].double(), B, cg) for i in (0, 1))
    gam, bet = (_per_channel(theta[:, o:o + C].double(), B, 0) for o in (off_w, off_b))
    xhat = (t.double() - mu) * rs
    z = (xhat * gam + bet).permute(0, 3, 1, 2)
    d = dy.double().permute(0, 3, 1, 2)
    if pool:  # torch's CPU max_pool2d keeps the first maximum in (row, column) order
        d = F.max_unpool2d(d, F.max_pool2d(z, 2, 2, return_indices=True)[1], 2, 2)
        ties = (z == F.interpolate(F.max_pool2d(z, 2, 2), scale_factor=2)) & (z > 0)
        assert int(F.avg_pool2d(ties.double(), 2, 2).gt(0.25).sum()) > 0, "no tie between positive entries"
    d = (d * (z > 0) if relu else d).permute(0, 2, 3, 1)
    pa, pb = d.sum((1, 2)), (d * xhat).sum((1, 2))                                         # [N, C]
    grp = lambda p: _per_channel((gam[:, 0, 0] * p).view(N, groups, cg).sum(2) / (H * W * cg), B, cg)  # noqa: E731
    m1, m2 = grp(pa), grp(pb)
    ref = rs * (d * gam - m1 - xhat * m2)
    terms = (rs * d * gam).abs() + (rs * m1).abs() + (rs * xhat * m2).abs()
    m, s = ops.ext(), ops.stream()
    th, td, dyd, st = theta.cuda(), t.cuda(), dy.cuda(), stats.cuda()
    dt = torch.full((N * H * W + 1, C), float("nan"), device="cuda", dtype=torch.bfloat16)
    part = torch.empty(N, C, 2, device="cuda")
    m.gn2d_bwd(dyd.data_ptr(), td.data_ptr(), st.data_ptr(), th[:, off_w:].data_ptr(),
               th[:, off_b:].data_ptr(), th.stride(0), dt.data_ptr(), part.data_ptr(), N, B, H, W, C, groups, relu,
               pool, s)
    gr = torch.empty(G, 2, C, device="cuda")
    m.gn_param_grads(part.data_ptr(), G, B, C, gr.data_ptr(), 2 * C, 0, C, s)
    torch.cuda.synchronize()
    got = dt[:-1].view(ref.shape)
    if (H * W * cg) & (H * W * cg - 1) == 0:
        bad = got.double().cpu() != ref.to(torch.bfloat16).double()
        assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[0].tolist())
    else:
        print("dt: worst err / bound", assert_within(got, ref, bf16_bound(ref, K_GN_BWD * U32 * terms), "nhwc"))
    assert bool(torch.isnan(dt[-1]).all()), "guard row written"
    assert torch.equal(gr[:, 0].double().cpu(), pb.view(G, B, C).sum(1)), "dgamma"
    assert torch.equal(gr[:, 1].double().cpu(), pa.view(G, B, C).sum(1)), "dbeta"


@pytest.mark.parametrize("shape", [(3, 2, 2, 8), (2, 10, 10, 64), (1, 4, 6, 16)])
def test_pool2d_equals_cpu_max_pool2d_and_its_autograd(shape):
    """Integers in [-2, 2], so ties occur in most windows: forward and backward equal torch's fp64 CPU max_pool2d (the
    first maximum of a window takes the gradient) bit for bit."""
    from neuroimagedisttraining_amd import ops
    N, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, dy = ints((N, H, W, C), -2, 2, g), ints((N, H // 2, W // 2, C), -3, 3, g)
    xr = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    ry = F.max_pool2d(xr, 2, 2)
    ry.backward(dy.double().permute(0, 3, 1, 2))
    m, s = ops.ext(), ops.stream()
    xd, dyd = x.cuda(), dy.cuda()
    y = torch.full((dy.numel() // C + 1, C), float("nan"), device="cuda", dtype=torch.bfloat16)
    dx = torch.full((x.numel() // C + 1, C), float("nan"), device="cuda", dtype=torch.bfloat16)
    m.pool2d_fwd(xd.data_ptr(), y.data_ptr(), N, H, W, C, s)
    m.pool2d_bwd(dyd.data_ptr(), xd.data_ptr(), dx.data_ptr(), N, H, W, C, s)
    torch.cuda.synchronize()
    assert torch.equal(y[:-1].view(dy.shape).double().cpu(), ry.detach().permute(0, 2, 3, 1))
    assert torch.equal(dx[:-1].view(x.shape).double().cpu(), xr.grad.permute(0, 2, 3, 1))
    assert bool(torch.isnan(y[-1]).all()) and bool(torch.isnan(dx[-1]).all()), "guard row written"
    with pytest.raises(ValueError):
        m.pool2d_fwd(xd.data_ptr(), y.data_ptr(), N, H, W + 1, C, s)


@pytest.mark.parametrize("name", ["vgg11", "cnn_cifar10"])
def test_batched2d_norm_and_pool_run_on_gn_pool_and_match_the_framework_path(name, monkeypatch):
    """A train step and an evaluation with NIDT_B2D_GN = 1 and 0 on the same rows: the same step within the engine
    tests' criteria; with 1 the profiler sees no aten group_norm (vgg11) and no aten max_pool2d op, with 0 it does."""
    from neuroimagedisttraining_amd.engine.batched2d import BatchedModuleEngine
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
    watched = ("aten::max_pool2d",) + (("aten::native_group_norm",) if name == "vgg11" else ())
    out = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("NIDT_B2D_GN", sw)
        eng = BatchedModuleEngine(create_model(name, dataset="cifar10", class_num=10), x8, y, "cuda", CIFAR_MEAN,
                                  CIFAR_STD)
        assert eng.uses_hip_layers
        theta = padded_rows(Gc, eng.players.total, "cuda")
        theta.copy_(rows)
        grads = padded_rows(Gc, eng.players.total, "cuda")
        idx = torch.arange(Gc * B, dtype=torch.int32, device="cuda")
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            loss = eng.train_step(theta, None, grads, idx, Gc, B, 1.0, 7)
            logits = eng.eval_logits(theta, None, idx, Gc, B)
            torch.cuda.synchronize()
        seen = {e.name for e in prof.events()}
        for w in watched:
            assert bool([o for o in seen if o.startswith(w)]) == (sw == "0"), (sw, w, sorted(seen))
        out[sw] = (loss.float().cpu(), grads.float().cpu(), logits.float().cpu())
    assert torch.allclose(out["1"][0], out["0"][0], rtol=2e-2, atol=2e-2), (out["1"][0], out["0"][0])
    assert float((out["1"][2] - out["0"][2]).norm() / out["0"][2].norm()) < 3e-2
    for c in range(Gc):
        a, b = out["1"][1][c], out["0"][1][c]
        assert float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.99, c
