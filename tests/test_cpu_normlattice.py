"""The helpers of tests/_normlattice.py without a GPU: the fp64 references agree with fp64 autograd of F.group_norm /
F.batch_norm; every lattice case of tests/test_gpu_exact_norm.py meets its exactness preconditions, and with
power-of-two divisors the reference formulas (and the kernels' own grouping of the same terms) evaluate identically in
fp32 and fp64; three corruptions of a correct fp32 emulation pass the older relative-norm thresholds and fail the new
assertions with the right index; and no per-element bound is loose enough to admit an error of one bf16 ulp on an
element of typical magnitude."""
import pytest
import torch
import torch.nn.functional as F

import _lattice as L
import _normlattice as NL

AXG = ("client", "sample", "position", "channel")
AXB = ("client", "position", "channel")


def _close(a, b, what):
    err = float((a.double() - b.double()).abs().max())
    assert err <= 1e-10 * max(1.0, float(b.double().abs().max())), (what, err)


# ========================================================================================= references vs autograd
@pytest.mark.parametrize("hw,C", [(6, 64), (4, 512)])
@pytest.mark.parametrize("res,relu", [(False, False), (True, True), (False, True)])
def test_gn_references_match_autograd(hw, C, res, relu):
    g = L.gen("gn_autograd", hw, C, res, relu)
    G, B, S = 3, 2, hw * hw
    N = G * B
    t = torch.randn(N, S, C, generator=g, dtype=torch.float64) * 2 + 1
    r = torch.randn(N, S, C, generator=g, dtype=torch.float64) if res else None
    dy = torch.randn(N, S, C, generator=g, dtype=torch.float64)
    gamma = torch.randn(G, C, generator=g, dtype=torch.float64).requires_grad_(True)
    beta = torch.randn(G, C, generator=g, dtype=torch.float64).requires_grad_(True)
    ta = t.clone().requires_grad_(True)
    ys = []
    for k in range(G):
        x = ta[k * B:(k + 1) * B].transpose(1, 2)            # [B, C, S]
        y = F.group_norm(x, NL.GN_GROUPS, gamma[k], beta[k], NL.GN_EPS).transpose(1, 2)
        ys.append(y)
    pre = torch.cat(ys)
    if res:
        pre = pre + r
    y = torch.relu(pre) if relu else pre
    (y * dy).sum().backward()
    gam = gamma.detach().repeat_interleave(B, 0)[:, None, :]
    bet = beta.detach().repeat_interleave(B, 0)[:, None, :]
    st, y_ref, pre_ref, _ = NL.gn_fwd_ref(t, r, gam, bet, relu)
    _close(y_ref, y.detach(), "y")
    xg = t.view(N, S, NL.GN_GROUPS, C // NL.GN_GROUPS)
    _close(st[..., 0], xg.mean((1, 3)), "mean")
    _close(st[..., 1], 1 / torch.sqrt(xg.var((1, 3), unbiased=False) + NL.GN_EPS), "rstd")
    dt, part, _, _ = NL.gn_bwd_ref(t, dy, (y.detach() > 0) if relu else None, st, gam)
    _close(dt, ta.grad, "dt")
    dg, db = NL.gn_param_grads_ref(part, G, B)
    _close(dg, gamma.grad, "dgamma")
    _close(db, beta.grad, "dbeta")


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("res,relu", [(False, False), (True, True), (False, True)])
def test_bn_references_match_autograd(train, res, relu):
    g = L.gen("bn_autograd", train, res, relu)
    G, M, C = 3, 37, 64
    t = torch.randn(G, M, C, generator=g, dtype=torch.float64) * 2 + 1
    r = torch.randn(G, M, C, generator=g, dtype=torch.float64) if res else None
    dy = torch.randn(G, M, C, generator=g, dtype=torch.float64)
    gamma = torch.randn(G, 1, C, generator=g, dtype=torch.float64).requires_grad_(True)
    beta = torch.randn(G, 1, C, generator=g, dtype=torch.float64).requires_grad_(True)
    rm0 = torch.randn(G, C, generator=g, dtype=torch.float64)
    rv0 = torch.rand(G, C, generator=g, dtype=torch.float64) + 0.5
    nbt0 = torch.full((G,), 5.0, dtype=torch.float64)
    rm, rv = rm0.clone(), rv0.clone()
    ta = t.clone().requires_grad_(True)
    pre = torch.stack([F.batch_norm(ta[k], rm[k], rv[k], gamma[k, 0], beta[k, 0], train, NL.BN_MOM, NL.BN_EPS)
                       for k in range(G)])
    if res:
        pre = pre + r
    y = torch.relu(pre) if relu else pre
    (y * dy).sum().backward()
    if train:
        stats, rm_ref, rv_ref, nbt_ref = NL.bn_stats_ref(t, rm0, rv0, nbt0)
        _close(rm_ref, rm, "running mean")
        _close(rv_ref, rv, "running var")
        assert torch.equal(nbt_ref, nbt0 + 1)
    else:
        stats = torch.stack([rm0, 1 / torch.sqrt(rv0 + NL.BN_EPS)], -1)
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    _close(NL.bn_apply_ref(t, r, stats, gamma.detach(), beta.detach(), relu), y.detach(), "y")
    mask = (y.detach() > 0) if relu else None
    dt, dg, db, coef, part, _ = NL.bn_bwd_ref(t, dy, mask, stats, gamma.detach(), not train)
    _close(dt, ta.grad, "dt")
    _close(dg, gamma.grad[:, 0], "dgamma")
    _close(db, beta.grad[:, 0], "dbeta")
    _close(coef[..., 0] * M, db, "coef")
    _close(part.sum(0)[..., 1], dg, "partials")


def test_bn_single_position_keeps_the_biased_variance():
    t = torch.tensor([[[3.0, -1.0]]], dtype=torch.float64)                         # G = 1, M = 1, C = 2
    stats, rm, rv, nbt = NL.bn_stats_ref(t, torch.zeros(1, 2), torch.ones(1, 2), torch.zeros(1))
    assert torch.equal(stats[..., 0], t[:, 0])
    _close(stats[..., 1], torch.full((1, 2), NL.BN_EPS, dtype=torch.float64) ** -0.5, "rstd of a zero variance")
    _close(rv, torch.full((1, 2), 1.0 - NL.BN_MOM, dtype=torch.float64), "running var")
    _close(rm, NL.BN_MOM * t[:, 0], "running mean")
    assert float(nbt) == 1.0


def test_res_reference_is_the_masked_sum():
    c = NL.bn_res_case(64, 70)
    out, p3, pd = NL.bn_res_ref(c.dx1, None, c.da, c.mask, c.omask, c.t3, c.s3, c.td, c.sd)
    exp = torch.where(c.omask > 0, c.dx1.double() + torch.where(c.mask > 0, c.da.double(), 0.0), 0.0)
    assert torch.equal(out, exp)
    out2, _, none = NL.bn_res_ref(c.dx1, c.dx2, None, None, c.omask, c.t3, c.s3, None, None)
    assert none is None and torch.equal(out2, torch.where(c.omask > 0, (c.dx1 + c.dx2).double(), 0.0))
    xh = (c.td.double() - c.sd[:, None, :, 0]) * c.sd[:, None, :, 1]
    assert p3.shape == (1, c.G, c.C, 2) and torch.equal(pd[0, ..., 1], (out * xh).sum(1))
    assert torch.equal(p3[0, ..., 0], out.sum(1)) and torch.equal(pd[0, ..., 0], out.sum(1))


# ================================================================================================ preconditions
@pytest.mark.parametrize("hw,C", NL.GN_SHAPES)
def test_gn_lattice_cases_meet_their_preconditions(hw, C):
    """The generators raise when a sum could round; with a power-of-two divisor the backward formula is the same in fp32
    and fp64, element for element, and the forward's ReLU input (gn_bwd_rm's mask) is exact in the kernel's grouping."""
    c = NL.gn_bwd_case(hw, C)
    assert c.pow2 == ((hw, C) not in ((6, 64), (7, 128)))
    for masked in (True, False):
        dt, part, _ = c.ref[masked]
        p32 = NL.gn_bwd_ref(c.t, c.dy, c.mask if masked else None, c.stats, c.gamma, torch.float32)
        assert torch.equal(p32[1].double(), part)
        assert float(part[..., 0].abs().max()) < L.FP32_EXACT
        if c.pow2:
            assert torch.equal(p32[0].double(), dt)
    sc = c.gamma * NL._gn_expand(c.stats[:, :, 1], c.cg)
    sh = c.beta - NL._gn_expand(c.stats[:, :, 0], c.cg) * sc
    assert torch.equal((c.t.float() * sc + sh).double(), c.pre)
    f = NL.gn_fwd_case(hw, C)
    assert float(f.stats[..., 0].abs().max()) == 0
    for key, (y, bound) in f.ref.items():
        assert bool(torch.isfinite(bound).all()) and float(bound.min()) > 0


@pytest.mark.parametrize("hw,C,nb", NL.GN_APPLY)
def test_gn_apply_partials_are_exact_and_combine_to_the_sample_statistics(hw, C, nb):
    c = NL.gn_fwd_case(hw, C)
    p = NL.gn_apply_part(c, nb).double()
    bp, k = c.S // nb, nb * c.cg
    assert nb * bp == c.S
    mean = p[..., 0].view(c.N, nb, NL.GN_GROUPS, c.cg)
    m2 = p[..., 1].view(c.N, nb, NL.GN_GROUPS, c.cg)
    m = mean.sum((1, 3)) / k
    var = (m2 + bp * (mean - m[:, None, :, None]) ** 2).sum((1, 3)) / (bp * k)
    assert float(m.abs().max()) == 0
    _close(1 / torch.sqrt(var + NL.GN_EPS), c.stats[..., 1], "Chan combine")
    if (hw, C, nb) == (4, 128, 4):
        assert (c.S * C // 8) % 1024 != 0


def _bn_kernel_form(c, mask, dtype):
    """dt as k_bnr_bwd_apply groups it: A dy' + (K2 t + K1), K2 = -A rstd m2, K1 = -A m1 - K2 mean."""
    st = c.stats.to(dtype)
    mu, rs = st[:, None, :, 0], st[:, None, :, 1]
    d = c.dy.to(dtype) * (mask.to(dtype) if mask is not None else 1)
    x = c.t.to(dtype)
    a, b = d.sum(1), (d * ((x - mu) * rs)).sum(1)
    m1, m2 = (a / c.M)[:, None], (b / c.M)[:, None]
    A = rs * c.gamma.to(dtype)
    K2 = -A * rs * m2
    K1 = -A * m1 - K2 * mu
    return A * d + (K2 * x + K1)


def _bn_cases():
    out = {(C, M, NL.BN_G) for C in NL.BN_C for M in NL.bn_stats_M(C) + NL.bn_bwd_M(C)}
    return sorted(out | set(NL.BN_STRIDE))


@pytest.mark.parametrize("C,M,G", _bn_cases())
def test_bn_lattice_cases_meet_their_preconditions(C, M, G):
    c = NL.bn_case(C, M, G)
    assert c.nchunk == (M + 2047) // 2048 and c.rows * (C // 8) == 256
    sc = c.gamma * c.stats[:, None, :, 1]
    sf = c.beta - c.stats[:, None, :, 0] * sc
    pre = NL.bn_apply_ref(c.t, None, c.stats, c.gamma, c.beta, False)
    y = NL.bn_apply_ref(c.t, c.res, c.stats, c.gamma, c.beta, True)
    assert torch.equal((c.t.float() * sc + sf).double(), pre)                       # the kernel's grouping, in fp32
    assert torch.equal(torch.relu(c.t.float() * sc + sf + c.res.float()).double(), y)
    if (C, M, G) in NL.BN_STRIDE or M not in NL.bn_bwd_M(C):
        return
    for mask in (c.mask, None):
        ref = NL.bn_bwd_ref(c.t, c.dy, mask, c.stats, c.gamma, 0)
        r32 = NL.bn_bwd_ref(c.t, c.dy, mask, c.stats, c.gamma, 0, torch.float32)
        assert torch.equal(r32[4].double(), ref[4]) and torch.equal(r32[1].double(), ref[1])
        ev = NL.bn_bwd_ref(c.t, c.dy, mask, c.stats, c.gamma, 1)
        assert torch.equal(NL.bn_bwd_ref(c.t, c.dy, mask, c.stats, c.gamma, 1, torch.float32)[0].double(), ev[0])
        if c.pow2:
            assert torch.equal(r32[0].double(), ref[0])
            assert torch.equal(_bn_kernel_form(c, mask, torch.float32).double(), ref[0])
        else:
            assert float((_bn_kernel_form(c, mask, torch.float64) - ref[0]).abs().max()) < 1e-12


def test_grid_stride_shapes_exceed_the_grid_cap():
    for C, M, G in NL.BN_STRIDE:
        assert M * C // 8 > (4096 // G + 1) * 256
        assert NL.bnr_grid_blocks(G, M, C) == 4096 // G + 1
        assert ((4096 // G + 1) * 256) % (C // 8) == 0     # the stride keeps a thread's channel chunk


@pytest.mark.parametrize("C,M", [(256, M) for M in NL.BN_RES_M] + [(64, 2049), (2048, 2049)])
def test_res_lattice_cases_meet_their_preconditions(C, M):
    c = NL.bn_res_case(C, M)
    out, p3, pd = NL.bn_res_ref(c.dx1, None, c.da, c.mask, c.omask, c.t3, c.s3, c.td, c.sd)
    assert float(out.abs().max()) <= 4 and p3.shape == pd.shape == (c.nchunk, c.G, C, 2)
    assert torch.equal(p3.float().double(), p3) and torch.equal(pd.float().double(), pd)


# ================================================================================================ comparisons
def test_assert_ulp_and_assert_within_report_named_indices():
    ref = torch.tensor([[1.0, 3.0], [0.75, -2.0]], dtype=torch.float64)
    got = ref.float()
    assert NL.assert_ulp(got, ref, 1, ("a", "b")) == 0
    up = torch.nextafter(got, torch.full_like(got, 10.0))
    assert NL.assert_ulp(up, ref, 1, ("a", "b")) == pytest.approx(1.0)
    two = torch.nextafter(up, torch.full_like(got, 10.0))
    with pytest.raises(AssertionError) as e:
        NL.assert_ulp(torch.where(ref == 0.75, two, got), ref, 1, ("a", "b"))
    assert "1 of 4" in str(e.value) and "first at (a=1, b=0)" in str(e.value)
    bad = got.clone()
    bad[0, 1] = float("nan")
    with pytest.raises(AssertionError) as e:
        NL.assert_within(bad, ref, torch.full_like(ref, 1.0), ("a", "b"))
    assert "(1 non-finite" in str(e.value) and "first at (a=0, b=1)" in str(e.value)
    assert float(NL.halfulp_bf16(torch.tensor(1.5))) == 2.0 ** -8
    assert float(NL.halfulp_bf16(torch.tensor(2.0))) == 2.0 ** -7
    assert float(NL.ulp32(torch.tensor(1.0))) == 2.0 ** -23


# ================================================================================================ corruptions
def test_norm_threshold_misses_an_unwritten_last_chunk_of_a_groupnorm_sample():
    """GroupNorm forward at hw 7, C 128 (784 chunks per sample, no multiple of 512): the last 8-channel chunk of one
    sample left unwritten stays under the forward threshold 1e-2 when the buffer is recycled from the same layer's
    previous call (the older test's parametrisations share t and theta, and differ in the residual); assert_within
    names the sample, position and channel.  (Over zeros the norm of this small tensor, 8 values of 37632, moves by
    about 1.5e-2: at the threshold's scale, caught or missed by the draw.)"""
    hw, C = 7, 128
    c = NL.gn_random_case(hw, C)
    assert (c.S * C // 8) % 512 != 0
    ref, _, bound = c.ref[True, True]
    y32 = NL.gn_fwd_ref(c.t, c.res, c.gamma, c.beta, True, torch.float32)[1]
    stale = NL.gn_fwd_ref(c.t, None, c.gamma, c.beta, True, torch.float32)[1].to(torch.bfloat16)
    good = y32.to(torch.bfloat16)                                                   # a correct fp32 kernel's output
    shape = (c.G, c.B, c.S, C)
    assert NL.assert_within(good, ref.view(shape), bound.view(shape), AXG) <= 1.0
    bad = good.clone()
    n = 1 * c.B + 1
    bad[n, c.S - 1, C - 8:] = stale[n, c.S - 1, C - 8:]
    assert NL.relnorm(bad.float(), y32) < 1e-2                                      # the old check passes
    last = (n, c.S - 1, slice(C - 8, C))
    out = ((stale[last].double() - ref[last]).abs() > bound[last]).nonzero().flatten()
    assert len(out) >= 3
    with pytest.raises(AssertionError) as e:
        NL.assert_within(bad, ref.view(shape), bound.view(shape), AXG)
    msg = str(e.value)
    assert msg.startswith("%d of " % len(out))
    assert "first at (client=1, sample=1, position=%d, channel=%d)" % (c.S - 1, C - 8 + int(out[0])) in msg
    nan = good.clone()
    nan[n, c.S - 1, C - 8:] = float("nan")                                          # the GPU test's sentinel
    with pytest.raises(AssertionError) as e:
        NL.assert_within(nan, ref.view(shape), bound.view(shape), AXG)
    assert str(e.value).startswith("8 of ") and "(8 non-finite" in str(e.value)


DROP_G, DROP_J = 1, 5       # the client and the 8-channel chunk of the thread whose tail position is dropped


def _bn_bwd_f32(t, dy, mask, stats, gamma, drop=None):
    """A correct fp32 BatchNorm backward (train mode); ``drop``: a position that the thread of client DROP_G and channel
    chunk DROP_J leaves out of its two sums."""
    d = dy.float() * mask.float()
    mu, rs = stats[:, None, :, 0].float(), stats[:, None, :, 1].float()
    xhat = (t.float() - mu) * rs
    keep = torch.ones(t.shape)
    if drop is not None:
        keep[DROP_G, drop, 8 * DROP_J:8 * DROP_J + 8] = 0
    a, b = (d * keep).sum(1), (d * xhat * keep).sum(1)
    M = t.shape[1]
    dt = rs * gamma.float() * (d - (a / M)[:, None] - xhat * (b / M)[:, None])
    return dt.to(torch.bfloat16), b, a, NL.bn_chunk_sums(d * keep, d * xhat * keep)


def test_norm_threshold_misses_a_position_dropped_at_a_chunk_boundary_of_a_batchnorm_backward():
    """M = 2049: position 2048, the only one of the second chunk, left out of (sum dy', sum dy' xhat) by one thread (one
    client, eight channels) stays under the thresholds 2e-2 (dt) and 1e-2 (dgamma / dbeta); on the lattice the partial
    tensor names chunk 1, the client and the channel.  (Left out for every channel of every client, dt still stays
    under 2e-2; the parameter rows, sums of about sqrt(M) zero-mean terms, move by 1 / sqrt(M) = 2.2e-2.)"""
    C, M, G = 64, 2049, NL.BN_G
    g = L.gen("bn_drop")
    t = (torch.randn(G, M, C, generator=g) * 3 + 1).to(torch.bfloat16)
    dy = torch.randn(G, M, C, generator=g).to(torch.bfloat16)
    mask = (torch.rand(G, M, C, generator=g) < 0.5).to(torch.bfloat16)
    gamma = torch.randn(G, 1, C, generator=g)
    stats = NL.bn_stats_ref(t, torch.zeros(G, C), torch.ones(G, C), torch.zeros(G))[0]
    ref = NL.bn_bwd_ref(t, dy, mask, stats, gamma, 0)
    good, bad = (_bn_bwd_f32(t, dy, mask, stats, gamma, drop) for drop in (None, M - 1))
    assert NL.relnorm(good[0].float(), ref[0]) < 5e-3
    assert NL.relnorm(bad[0].float(), ref[0]) < 2e-2                                 # the old checks pass
    assert NL.relnorm(torch.stack(bad[1:3]), torch.stack(ref[1:3])) < 1e-2
    assert not torch.equal(bad[1], good[1])
    c = NL.bn_case(C, M)
    ref = NL.bn_bwd_ref(c.t, c.dy, c.mask, c.stats, c.gamma, 0)
    good, bad = (_bn_bwd_f32(c.t, c.dy, c.mask, c.stats, c.gamma, drop) for drop in (None, M - 1))
    ax = ("chunk", "client", "channel", "sum")
    L.assert_exact(good[3], ref[4], ax)
    L.assert_exact(good[1], ref[1], ax[1:3])
    assert NL.assert_within(good[0], ref[0], NL.bn_bwd_bound(ref[0], ref[5]), AXB) <= 1.0
    nz = torch.nonzero(ref[4][1, DROP_G, 8 * DROP_J:8 * DROP_J + 8])
    assert len(nz) >= 1
    with pytest.raises(AssertionError) as e:
        L.assert_exact(bad[3], ref[4], ax)
    msg = str(e.value)
    assert msg.startswith("%d of " % len(nz))
    first = (DROP_G, 8 * DROP_J + int(nz[0, 0]), int(nz[0, 1]))
    assert "first at (chunk=1, client=%d, channel=%d, sum=%d)" % first in msg
    with pytest.raises(AssertionError):
        L.assert_exact(bad[1], ref[1], ax[1:3])


SWAP_G = 5                  # the client whose thread takes its neighbour's coefficients


def _apply_f32(t, stats, gamma, beta, swap=None):
    """A correct fp32 bnr_apply (no residual, no ReLU); ``swap``: the flat index q = position * (C / 8) + chunk of the
    one 16-byte chunk of client SWAP_G that is scaled with the coefficients of the next channel chunk."""
    sc = gamma.float() * stats[:, None, :, 1].float()
    sf = beta.float() - stats[:, None, :, 0].float() * sc
    y = t.float() * sc + sf
    if swap is not None:
        nch = t.shape[2] // 8
        p, lo = swap // nch, 8 * (swap % nch)
        nb = slice(lo + 8, lo + 16)
        y[SWAP_G, p, lo:lo + 8] = t[SWAP_G, p, lo:lo + 8].float() * sc[SWAP_G, 0, nb] + sf[SWAP_G, 0, nb]
    return y.to(torch.bfloat16)


def test_norm_threshold_misses_a_neighbours_coefficients_on_the_second_grid_stride_trip():
    """bnr_apply at C = 64, M = 8300, G = 16: one thread's chunk of the second trip of the grid-stride loop (chunks from
    257 * 256 on) scaled with its neighbour's sc / sh stays under 1e-2; on the lattice assert_exact names the client,
    the position and the channel."""
    C, M, G = NL.BN_STRIDE[1]
    trip = NL.bnr_grid_blocks(G, M, C) * 256
    assert trip < M * C // 8 and trip % (C // 8) == 0
    p0 = trip // (C // 8)
    g = L.gen("bn_stride")
    t = (torch.randn(G, M, C, generator=g) * 3 + 1).to(torch.bfloat16)
    gamma, beta = torch.randn(G, 1, C, generator=g), torch.randn(G, 1, C, generator=g)
    stats = NL.bn_stats_ref(t, torch.zeros(G, C), torch.ones(G, C), torch.zeros(G))[0]
    ref = NL.bn_apply_ref(t, None, stats, gamma, beta, False)
    bad = _apply_f32(t, stats, gamma, beta, trip + 3)
    assert not torch.equal(bad, _apply_f32(t, stats, gamma, beta))
    assert NL.relnorm(bad.float(), ref) < 1e-2                                       # the old check passes
    c = NL.bn_case(C, M, G)
    ref = NL.bn_apply_ref(c.t, None, c.stats, c.gamma, c.beta, False)
    exp = ref.to(torch.bfloat16).double()
    L.assert_exact(_apply_f32(c.t, c.stats, c.gamma, c.beta), exp, AXB)
    bad = _apply_f32(c.t, c.stats, c.gamma, c.beta, trip + 3)
    diff = torch.nonzero(bad.double() != exp)
    assert len(diff) > 0 and set(diff[:, 0].tolist()) == {SWAP_G} and set(diff[:, 1].tolist()) == {p0}
    assert set(diff[:, 2].tolist()) <= set(range(24, 32))
    with pytest.raises(AssertionError) as e:
        L.assert_exact(bad, exp, AXB)
    msg = str(e.value)
    assert msg.startswith("%d of " % len(diff))
    assert "first at (client=%d, position=%d, channel=%d)" % (SWAP_G, p0, int(diff[0, 2])) in msg


# ================================================================================================ bounds mean something
def _one_ulp_fails(ref, bound, what):
    """An error of one bf16 ulp on the element of median magnitude, and on most non-zero elements (elements that are
    small by cancellation have bounds above their own ulp), exceeds its bound."""
    ref, bound = ref.flatten(), bound.flatten()
    nz = torch.nonzero(ref.abs() > 0).flatten()
    ulp = 2 * NL.halfulp_bf16(ref[nz])
    i = ref[nz].abs().argsort()[len(nz) // 2]
    assert float(bound[nz][i]) < float(ulp[i]), what
    assert float((bound[nz] < ulp).double().mean()) > 0.6, what


@pytest.mark.parametrize("hw,C", NL.GN_RANDOM + [(7, 128)])
def test_random_groupnorm_bounds_fail_a_one_ulp_error(hw, C):
    c = NL.gn_random_case(hw, C)
    for key, (y, pre, bound) in c.ref.items():
        _one_ulp_fails(y, bound, ("gn_fwd random", hw, C, key))
    # the backward given the reference's own mask and statistics (rounded to fp32 as the kernel saves them)
    y, pre, _ = c.ref[False, True]
    dt, part, terms, aux = NL.gn_bwd_ref(c.t, c.dy, y > 0, c.stats.float(), c.gamma)
    _, ddt = NL.gn_bwd_sum_error(aux, c.S, c.cg)
    _one_ulp_fails(dt, NL.bf16_bound(dt, NL.K_GN_BWD_RANDOM * NL.U32 * terms + ddt), ("gn_bwd random", hw, C))


def test_lattice_bounds_of_the_non_dyadic_cases_fail_a_one_ulp_error():
    for hw, C in NL.GN_SHAPES:
        c = NL.gn_bwd_case(hw, C)
        for masked in (True, False):
            _one_ulp_fails(c.ref[masked][0], NL.gn_bwd_bound(c, masked), ("gn_bwd", hw, C))
        for key, (y, bound) in NL.gn_fwd_case(hw, C).ref.items():
            _one_ulp_fails(y, bound, ("gn_fwd", hw, C, key))
    for C in (64, 256):
        c = NL.bn_case(C, 2049)
        ref = NL.bn_bwd_ref(c.t, c.dy, c.mask, c.stats, c.gamma, 0)
        _one_ulp_fails(ref[0], NL.bn_bwd_bound(ref[0], ref[5]), ("bn_bwd", C))


def test_random_batchnorm_statistics_bound_is_far_below_the_statistics():
    t = NL.bn_random_t(256, 2049)
    dmean, dvar = NL.bn_stats_error(t)
    x = t.double()
    var = x.var(1, unbiased=False)
    assert float(dmean.max()) < 1e-2 and float((dvar / var).max()) < 0.25
    assert float(NL.rstd_error(var, dvar, NL.BN_EPS).max()) < 0.2
