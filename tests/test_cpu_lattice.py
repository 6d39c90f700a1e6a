"""CPU checks of the integer-lattice helper (tests/_lattice.py) behind tests/test_gpu_exact_conv.py: the generators meet
the exactness preconditions for every shape of the shared tables, ``assert_exact`` localises a wrong value, and — the
reason the exact tests exist — single-tap and single-position corruptions that the relative-norm thresholds of the
older conv tests (1e-2 forward, 2e-2 gradients) do not see are caught on lattice operands with their coordinates."""
import pytest
import torch
import torch.nn.functional as F

import _lattice as L


# ------------------------------------------------------------------------------------------------ generators
def _check_conv_case(c):
    assert set(c.x.float().unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    if c.dy is not None:
        assert set(c.dy.float().unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert set(c.w.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert bool((c.w.reshape(c.G, c.cout, c.cin, c.taps) != 0).any(1).any(1).all())  # every tap is live
    assert torch.equal(c.w.to(torch.bfloat16).float(), c.w)
    if c.bias is not None:
        assert float(c.bias.abs().max()) <= 4 and torch.equal(c.bias, c.bias.round())
    if c.xs is not None:
        assert set(c.xs.unique().tolist()) <= {1.0, 2.0} and set(c.xt.unique().tolist()) <= {-1.0, 0.0, 1.0}
    # the preconditions were asserted by the builder; the references are integers that bf16 / fp32 hold exactly
    assert float(c.y.abs().max()) > 0
    for ref in (c.y, c.dx) if c.dx is not None else (c.y,):
        assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= L.BF16_EXACT
        assert torch.equal(ref.to(torch.bfloat16).double(), ref)
    if c.dx is None:  # forward-only case
        return
    assert torch.equal(c.dw.float().double(), c.dw) and c.dw_bound < L.FP32_EXACT
    assert float(c.dx.abs().max()) > 0 and float(c.dw.abs().max()) > 0


@pytest.mark.parametrize("name,G,B,grads", L.conv3_cases())
def test_conv3_cases_meet_preconditions(name, G, B, grads):
    _check_conv_case(L.conv3(name, G, B, grads))


@pytest.mark.parametrize("name", list(L.GEN3) + [L.GEN3_SPLITK[0]])
def test_generic_3d_cases_meet_preconditions(name):
    _check_conv_case(L.gen3(name))


@pytest.mark.parametrize("name", list(L.GEN2))
def test_generic_2d_cases_meet_preconditions(name):
    c = L.gen2(name)
    _check_conv_case(c)
    assert c.cin_p % 64 == 0 and float(c.x[..., c.cin:].abs().sum()) == 0


@pytest.mark.parametrize("B,hw,cin,cout", L.SLAB2_BD + L.SLAB2)
def test_slab_2d_cases_meet_preconditions(B, hw, cin, cout):
    _check_conv_case(L.slab2(B, hw, cin, cout))


@pytest.mark.parametrize("cin,cout,k,pad,H", L.C2_SHAPES)
def test_conv2d_any_cases_meet_preconditions(cin, cout, k, pad, H):
    c = L.c2(cin, cout, k, pad, H)
    _check_conv_case(c)
    assert c.cin_p == cin


def test_gemm_cases_meet_preconditions():
    for K, N in L.G1_SHAPES:
        c = L.gemm_case("g1", L.GEMM_G, L.G1_MG, K, N)
        assert torch.equal(c.y.to(torch.bfloat16).double(), c.y)
        assert c.stats_exact  # sum |y| and sum y^2 per channel stay below 2^24 at this row count
    for N, K in L.W1_SHAPES:
        c = L.gemm_case("w1", L.GEMM_G, L.W1_MG, K, N)
        assert torch.equal((c.dw * 0.5).float().double(), c.dw * 0.5)


def test_gemm_shape_lists_match_the_norm_tests():
    import test_gpu_resnet3d as T
    assert L.G1_SHAPES == T.G1_SHAPES
    assert L.W1_SHAPES == [s for s in T.W1_SHAPES if s != (1024, 2048)]


def test_generators_refuse_what_they_cannot_meet():
    g = L.gen("refuse")
    with pytest.raises(ValueError, match="zero density"):
        L.int_weights(1, 4, 8, 9, g, nnz_per_row=0)
    with pytest.raises(ValueError, match="without a non-zero weight"):
        L.int_weights(1, 1, 1, 27, g, nnz_per_row=1)
    with pytest.raises(ValueError, match="exceeds 256"):
        L.conv_case("too_dense", 1, 2, 512, 64, 3, 1, 1, (4, 4, 4), nnz=27 * 512)
    with pytest.raises(ValueError, match="2\\^24"):
        L.require_fp32_exact(1 << 24, "bound")


def test_kernel_eligibility_of_the_table_shapes():
    """The host-side *_ok rules accept the shapes the GPU file sends to each union kernel (no GPU needed)."""
    from neuroimagedisttraining_amd import ops
    m = ops.ext()
    for name, (cin, cout, pad, sp, _) in L.CONV3.items():
        do = [s + 2 * pad - 2 for s in sp]
        for B in sorted({B for _, B in L.CONV3_GB[name]}):
            assert m.conv3d_fwd_tri_ok(B, *sp, cin, cout, pad)
        for _, B in L.CONV3_BWD_GB:
            assert m.conv3d_wgrad_tri_ok(B, *sp, cin, cout, pad) and m.conv3d_wgrad_slab_ok(B, *sp, cin, cout, pad)
            assert m.conv3d_fwd_tri_ok(B, *do, cout, cin, 2 - pad)
    B = L.SLAB3_GB[1]
    for name, (cin, cout, pad, sp) in L.SLAB3.items():
        do = [s + 2 * pad - 2 for s in sp]
        assert m.conv3d_fwd_slab_ok(B, *sp, cin, cout, pad) and m.conv3d_fwd_tri_ok(B, *sp, cin, cout, pad)
        assert m.conv3d_wgrad_slab_ok(B, *sp, cin, cout, pad)
        assert m.conv3d_fwd_slab_ok(B, *do, cout, cin, 2 - pad)
        assert B * do[0] * do[1] * do[2] > 2 * 256  # three or more 256-position bands
    for B, hw, cin, cout in L.SLAB2_BD:
        assert m.conv2d_fwd_slab_bd_ok(B, hw, hw, cin, cout) and not m.conv2d_fwd_slab_ok(B, hw, hw, cin, cout)
    for B, hw, cin, cout in L.SLAB2:
        assert m.conv2d_fwd_slab_ok(B, hw, hw, cin, cout)
    for K, N in L.G1_SHAPES:
        assert m.gemm1x1_ok(K, N)
    for N, K in L.W1_SHAPES:
        assert m.wgrad1x1_ok(N, K)


# ------------------------------------------------------------------------------------------------ assert_exact
def test_assert_exact_reports_first_and_worst_index():
    ref = torch.arange(2 * 3 * 4, dtype=torch.float64).view(2, 3, 4)
    L.assert_exact(ref.to(torch.bfloat16), ref, ("client", "row", "channel"))
    got = ref.clone()
    got[0, 2, 1] += 1
    got[1, 1, 3] -= 5
    with pytest.raises(AssertionError) as e:
        L.assert_exact(got, ref, ("client", "row", "channel"))
    msg = str(e.value)
    assert "2 of 24 values differ" in msg
    assert "first at (client=0, row=2, channel=1): got 10.0, reference 9.0" in msg
    assert "worst at (client=1, row=1, channel=3): got 14.0, reference 19.0" in msg
    got = ref.clone()
    got[1, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"\(1 non-finite\); first at \(client=1, row=0, channel=0\)"):
        L.assert_exact(got, ref, ("client", "row", "channel"))
    with pytest.raises(AssertionError, match="shape"):
        L.assert_exact(ref[:1], ref, ("client", "row", "channel"))


# ------------------------------------------------------------------------------------------------ the blind spot
def _random_case(G, B, cin, cout, stride, pad, dims, seed):
    """The older tests' recipe: randn inputs and gradients, 0.05 randn weights, all rounded to bf16; fp64 references."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((G * B,) + dims + (cin,), generator=g).to(torch.bfloat16)
    w = (torch.randn(G, cout, cin, 3, 3, 3, generator=g) * 0.05).to(torch.bfloat16).float()
    y, dy, dx, dw = L.conv_reference(x, w, lambda s: torch.randn(s, generator=g).to(torch.bfloat16), G, stride, pad)
    return x, w, y, dy, dx, dw


def _as_kernel_output(ref):
    return ref.to(torch.bfloat16)  # what a correct kernel stores


def test_norm_threshold_misses_a_dropped_tap_at_a_corner_voxel():
    """128 -> 192, 5x7x5, pad 1, B = 16: the centre tap missing at the corner voxel (0, 0, 0) of one sample, in all 192
    channels, stays under the forward threshold 1e-2; on lattice operands assert_exact names the voxel."""
    G, B, cin, cout, pad, dims = 2, 16, 128, 192, 1, (5, 7, 5)
    g_, n_ = 1, 5  # client 1, sample 5
    x, w, y, _, _, _ = _random_case(G, B, cin, cout, 1, pad, dims, 1)
    assert L.relerr(_as_kernel_output(y).float(), y) < 5e-3  # storage noise alone
    bad = y.clone()
    bad[g_ * B + n_, 0, 0, 0] -= w[g_, :, :, 1, 1, 1].double() @ x[g_ * B + n_, 0, 0, 0].double()
    assert not torch.equal(_as_kernel_output(bad), _as_kernel_output(y))
    assert L.relerr(_as_kernel_output(bad).float(), y) < 1e-2  # the old check passes
    c = L.conv3("pad1", *L.CONV3_BWD_GB[0])
    assert (c.G, c.B, c.cin, c.cout, c.dims) == (G, B, cin, cout, dims)
    drop = c.w[g_, :, :, 1, 1, 1].double() @ c.x[g_ * B + n_, 0, 0, 0].double()
    ch = torch.nonzero(drop)
    assert len(ch) > cout // 2
    bad = c.y.clone()
    bad[g_ * B + n_, 0, 0, 0] -= drop
    names = ("client", "sample", "d", "h", "w", "channel")
    L.assert_exact(_as_kernel_output(c.y), c.y.view(G, B, *c.out, cout), names)
    with pytest.raises(AssertionError) as e:
        L.assert_exact(_as_kernel_output(bad), c.y.view(G, B, *c.out, cout), names)
    msg = str(e.value)
    assert msg.startswith("%d of " % len(ch))
    assert "first at (client=1, sample=5, d=0, h=0, w=0, channel=%d)" % int(ch[0]) in msg
    assert "worst at (client=1, sample=5, d=0, h=0, w=0, channel=%d)" % int(drop.abs().argmax()) in msg


def test_norm_threshold_misses_a_dropped_tap_on_the_last_odd_phase_plane_of_a_stride2_dgrad():
    """64 -> 128, 3x3x3 stride 2, 5x7x5: one tap missing at one voxel of the last odd-phase depth plane of dX stays
    under the gradient threshold 2e-2; on lattice operands assert_exact names the voxel."""
    name = "k3s2_odd"
    cin, cout, k, stride, dims = L.GEN3[name]
    G, B = L.GEN_GB
    g_, n_ = 2, 1
    d, h, w_ = dims[0] - 2, 1, 1           # d = 3: the last odd plane; reached by tap kd = 0 from the dy plane 2
    tap, src = (0, 0, 0), ((d + 1) // 2, 1, 1)  # x index = 2 o - 1 + k per axis

    def dropped(w, dy):
        return w[g_, :, :, tap[0], tap[1], tap[2]].double().t() @ dy[g_ * B + n_, src[0], src[1], src[2]].double()
    x, w, _, dy, dx, _ = _random_case(G, B, cin, cout, stride, 1, dims, 2)
    bad = dx.clone()
    bad[g_ * B + n_, d, h, w_] -= dropped(w, dy)
    assert not torch.equal(_as_kernel_output(bad), _as_kernel_output(dx))
    assert L.relerr(_as_kernel_output(bad).float(), dx) < 2e-2  # the old check passes
    c = L.gen3(name)
    drop = dropped(c.w, c.dy)
    ch = torch.nonzero(drop)
    assert len(ch) > 0
    bad = c.dx.clone()
    bad[g_ * B + n_, d, h, w_] -= drop
    names = ("client", "sample", "d", "h", "w", "channel")
    with pytest.raises(AssertionError) as e:
        L.assert_exact(_as_kernel_output(bad), c.dx.view(G, B, *dims, cin), names)
    msg = str(e.value)
    assert msg.startswith("%d of " % len(ch))
    assert "first at (client=2, sample=1, d=%d, h=1, w=1, channel=%d)" % (d, int(ch[0])) in msg
    # the dropped term is a real term of that voxel: removing it from the conv's definition reproduces the corruption
    xg = torch.zeros(1, cin, *dims, dtype=torch.float64, requires_grad=True)
    wz = c.w[g_].double().clone()
    wz[:, :, tap[0], tap[1], tap[2]] = 0
    only = torch.zeros_like(c.dy[g_ * B + n_].double())
    only[src] = c.dy[g_ * B + n_][src].double()
    full = torch.autograd.grad(F.conv3d(xg, c.w[g_].double(), None, stride, 1), xg, only.movedim(-1, 0)[None])[0]
    part = torch.autograd.grad(F.conv3d(xg, wz, None, stride, 1), xg, only.movedim(-1, 0)[None])[0]
    assert torch.equal((full - part)[0, :, d, h, w_], drop)


def test_norm_threshold_misses_a_position_dropped_from_a_weight_gradient():
    """128 -> 192, 5x7x5, pad 1, B = 16: one output position (all its taps) missing from a client's weight gradient
    stays under the gradient threshold 2e-2 (and under 1e-2); on lattice operands assert_exact names client and tap."""
    G, B, cin, cout, pad, dims = 2, 16, 128, 192, 1, (5, 7, 5)
    g_, n_, pos = 1, 15, (4, 6, 4)  # the last position of the last sample: the tail of the last position block

    def dropped(x, dy):
        """dW contribution of that position: dy[pos] (outer) the 3x3x3 input patch around it."""
        xp = F.pad(x[g_ * B + n_].double().movedim(-1, 0), (pad,) * 6)
        patch = xp[:, pos[0]:pos[0] + 3, pos[1]:pos[1] + 3, pos[2]:pos[2] + 3]
        return torch.einsum("o,cdhw->ocdhw", dy[g_ * B + n_][pos].double(), patch)
    x, w, _, dy, _, dw = _random_case(G, B, cin, cout, 1, pad, dims, 3)
    bad = dw.clone()
    bad[g_] -= dropped(x, dy)
    assert not torch.equal(bad.float(), dw.float())
    assert L.relerr(bad.float(), dw) < 1e-2  # the old checks (1e-2 and 2e-2) pass
    c = L.conv3("pad1", *L.CONV3_BWD_GB[0])
    drop = dropped(c.x, c.dy)
    nz = torch.nonzero(drop.reshape(cout, cin, 27))
    assert len(nz) > 0
    # interior taps only: the position sits in a corner, so the taps reaching into the padding contribute nothing
    assert float(drop[:, :, 2].abs().sum()) == 0 and float(drop[:, :, :, 2].abs().sum()) == 0
    bad = c.dw.clone()
    bad[g_] -= drop
    names = ("client", "cout", "cin", "tap")
    L.assert_exact(c.dw.float(), c.dw.reshape(G, cout, cin, 27), names)
    with pytest.raises(AssertionError) as e:
        L.assert_exact(bad.float(), c.dw.reshape(G, cout, cin, 27), names)
    msg = str(e.value)
    assert msg.startswith("%d of " % len(nz))
    assert "first at (client=1, cout=%d, cin=%d, tap=%d)" % tuple(int(v) for v in nz[0]) in msg
