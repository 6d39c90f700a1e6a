"""Bit-exact tests of the bf16 implicit-GEMM conv kernels (conv3d.hip, conv2d_any.hip) and the 1x1 GEMMs (gemm1x1.hip,
wgrad1x1.hip) on integer-lattice operands (tests/_lattice.py): every product and partial sum is an exactly
representable integer, so a correct kernel equals the fp64 CPU reference bit for bit whatever its accumulation order,
and one dropped, doubled or misplaced tap or position anywhere fails with its coordinates.  The relative-norm tests of
the same kernels (test_gpu_kernels.py, test_gpu_resnet2d.py, test_gpu_resnet3d.py, test_gpu_batched2d.py) keep the
random-data coverage and the statistics epilogues, whose results are not integers.

The bindings are called directly, so the kernel under test is the one named; output, partial and gradient buffers start
as NaN, and gradient slices sit between sentinel columns that must stay untouched.
"""
import pytest
import torch

import _lattice as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
AX3 = ("client", "sample", "d", "h", "w", "channel")
AX2 = ("client", "sample", "h", "w", "channel")
AXW = ("client", "cout", "cin", "tap")
SENT = -3.0


def _m():
    from neuroimagedisttraining_amd import ops
    return ops.ext()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _nan_bf16(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.bfloat16)


def _nan_f32(*shape):
    return torch.full(shape, NAN, device=DEV)


def _cs(ref, c):
    """[G B, ...] reference -> [G, B, ...] (client and sample axes)."""
    return ref.view((c.G, c.B) + tuple(ref.shape[1:]))


def _image(c):
    """Forward weight image [G, cout, taps, cin_p] bf16 of a case (taps major, channels zero-padded)."""
    w = c.w.reshape(c.G, c.cout, c.cin, c.taps).permute(0, 1, 3, 2)
    if c.cin_p != c.cin:
        w = torch.nn.functional.pad(w, (0, c.cin_p - c.cin))
    return w.contiguous().to(torch.bfloat16).to(DEV)


def _rows(c, off, tail, ncol=None):
    """Gradient rows [G, off + n + tail]: sentinel columns around a NaN slice of n = cout cin_p taps."""
    n = c.cout * c.cin_p * c.taps if ncol is None else ncol
    rows = torch.full((c.G, off + n + tail), SENT, device=DEV)
    rows[:, off:off + n] = NAN
    return rows, n


def _check_rows(c, rows, off, n, scale, what):
    torch.cuda.synchronize()
    assert float(rows[:, :off].sub(SENT).abs().max()) == 0 and float(rows[:, off + n:].sub(SENT).abs().max()) == 0, what
    got = rows[:, off:off + n].view(c.G, c.cout, c.cin_p, c.taps)
    L.assert_exact(got[:, :, :c.cin], (c.dw * scale).reshape(c.G, c.cout, c.cin, c.taps), AXW)
    if c.cin_p != c.cin:  # zero input channels: their gradient is exactly 0
        assert float(got[:, :, c.cin:].abs().max()) == 0, what


def _stats_buf(c):
    """NaN statistics buffer large enough for every block size (>= 64 positions per block)."""
    mg = c.B
    for o in c.out:
        mg *= o
    return _nan_f32(c.G * ((mg + 63) // 64 + c.B) * c.cout * 2)


def _mg(c):
    mg = c.B
    for o in c.out:
        mg *= o
    return mg


# ================================================================================================ 3x3x3 stride 1
def _x_eff(c):
    """The conv's bf16 input on the device; a fused-transform case pre-transformed (integers in [0, 5])."""
    x = c.x
    if c.xs is not None:
        B = c.B
        x = torch.cat([torch.relu(x[g * B:(g + 1) * B].float() * c.xs[g] + c.xt[g]) for g in range(c.G)])
        x = x.to(torch.bfloat16)
    return x.to(DEV)


def _fwd3_params():
    out = []
    for name in L.CONV3:
        for G, B in L.CONV3_GB[name]:
            kernels = ["fwd", "bld", "tri"] + ["splitk%d" % k for k in L.SPLITK3]
            out += [(name, G, B, k) for k in kernels]
    for name in L.SLAB3:
        out += [(name,) + L.SLAB3_GB + (k,) for k in ("fwd", "tri", "slab")]
    return out


@pytest.mark.parametrize("name,G,B,kernel", _fwd3_params())
def test_conv3_forward_exact(name, G, B, kernel):
    """conv3d_fwd (LDS-DMA per-tap kernel at its 64-, 128- and 256-position blocks; the register-staged kernel with the
    fused input transform), conv3d_fwd_bld, conv3d_fwd_splitk, conv3d_fwd_tri and conv3d_fwd_slab, with
    and without bias, against one fp64 reference per case."""
    m = _m()
    c = L.conv3(name, G, B, grads=name in L.SLAB3)  # the slab cases are the backward tests' cases too
    sp, cin, cout, pad = c.dims, c.cin, c.cout, c.pad
    w = _image(c)
    bias = c.bias.to(DEV)
    fused = kernel == "fwd" and c.xs is not None
    x = c.x.to(DEV) if fused else _x_eff(c)
    xs, xt = (c.xs.to(DEV), c.xt.to(DEV)) if fused else (None, None)
    y = _nan_bf16(G * B, *c.out, cout)
    y0 = _nan_bf16(G * B, *c.out, cout)
    stats = _stats_buf(c)
    Mg = _mg(c)
    if kernel == "fwd":
        bp = m.conv3d_fwd_bp(cin, cout, 1 if fused else 0, G, Mg)
        if name == "pad1":
            assert bp == {2: 64, 8: 128, 16: 256}[G]
        m.conv3d_fwd(x.data_ptr(), w.data_ptr(), bias.data_ptr(), xs.data_ptr() if fused else 0,
                     xt.data_ptr() if fused else 0, y.data_ptr(), stats.data_ptr(), G, B, *sp, cin, cout, pad, _st())
        m.conv3d_fwd(x.data_ptr(), w.data_ptr(), 0, xs.data_ptr() if fused else 0, xt.data_ptr() if fused else 0,
                     y0.data_ptr(), 0, G, B, *sp, cin, cout, pad, _st())
    elif kernel == "bld":  # bias rows at a stride, as read from the flat parameter rows
        theta = torch.full((G, cout + 37), SENT, device=DEV)
        theta[:, 5:5 + cout] = bias
        m.conv3d_fwd_bld(x.data_ptr(), w.data_ptr(), theta.data_ptr() + 4 * 5, theta.stride(0), y.data_ptr(),
                         stats.data_ptr(), G, B, *sp, cin, cout, pad, _st())
        m.conv3d_fwd_bld(x.data_ptr(), w.data_ptr(), 0, 0, y0.data_ptr(), 0, G, B, *sp, cin, cout, pad, _st())
    elif kernel.startswith("splitk"):
        ks = int(kernel[6:])
        if G <= 2:
            assert m.conv3d_fwd_ksplit(cin, cout, G, Mg) > 1
        part = _nan_f32(ks * G * Mg * cout)
        m.conv3d_fwd_splitk(x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), stats.data_ptr(),
                            part.data_ptr(), ks, G, B, *sp, cin, cout, pad, _st())
        part0 = _nan_f32(ks * G * Mg * cout)
        m.conv3d_fwd_splitk(x.data_ptr(), w.data_ptr(), 0, y0.data_ptr(), 0, part0.data_ptr(), ks, G, B, *sp, cin, cout,
                            pad, _st())
    elif kernel == "tri":
        assert m.conv3d_fwd_tri_ok(B, *sp, cin, cout, pad)
        tab = torch.empty(m.conv3d_fwd_tri_table_size(B, *sp, pad), device=DEV, dtype=torch.int32)
        m.conv3d_fwd_tri_table(tab.data_ptr(), B, *sp, pad, _st())
        m.conv3d_fwd_tri(x.data_ptr(), w.data_ptr(), bias.data_ptr(), 0, y.data_ptr(), stats.data_ptr(), G, B, *sp, cin,
                         cout, pad, tab.data_ptr(), _st())
        m.conv3d_fwd_tri(x.data_ptr(), w.data_ptr(), 0, 0, y0.data_ptr(), 0, G, B, *sp, cin, cout, pad, tab.data_ptr(),
                         _st())
    else:
        assert kernel == "slab" and m.conv3d_fwd_slab_ok(B, *sp, cin, cout, pad)
        tab = torch.empty(m.conv3d_fwd_slab_table_size(B, *sp, pad), device=DEV, dtype=torch.int32)
        m.conv3d_fwd_slab_table(tab.data_ptr(), B, *sp, pad, _st())
        m.conv3d_fwd_slab(x.data_ptr(), w.data_ptr(), bias.data_ptr(), 0, y.data_ptr(), stats.data_ptr(), G, B, *sp,
                          cin, cout, pad, tab.data_ptr(), _st())
        m.conv3d_fwd_slab(x.data_ptr(), w.data_ptr(), 0, 0, y0.data_ptr(), 0, G, B, *sp, cin, cout, pad,
                          tab.data_ptr(), _st())
    torch.cuda.synchronize()
    L.assert_exact(y0, _cs(c.y, c), AX3)
    L.assert_exact(y, _cs(L.y_with_bias(c), c), AX3)


def _wgrad3_params():
    out = []
    for name in L.CONV3:
        out += [(name, G, B, k, ns) for G, B in L.CONV3_BWD_GB for k in ("dma", "reg", "tri", "slab")
                for ns in (1, 3, 0)]
    for name in L.SLAB3:
        out += [(name,) + L.SLAB3_GB + (k, ns) for k in ("dma", "slab") for ns in (1, 3, 0)]
    return out


@pytest.mark.parametrize("name,G,B,kernel,ns", _wgrad3_params())
def test_conv3_wgrad_exact(name, G, B, kernel, ns):
    """conv3d_wgrad (LDS-DMA form with a position table, register-staged form without — the latter also with the fused
    input transform), conv3d_wgrad_tri and conv3d_wgrad_slab at split counts 1, 3 and the cost model's, scale 1 and
    0.5, straight into sentinel-guarded gradient rows: exact in fp32."""
    m = _m()
    c = L.conv3(name, G, B)
    sp, cin, cout, pad = c.dims, c.cin, c.cout, c.pad
    fused = kernel == "reg" and c.xs is not None
    x = c.x.to(DEV) if fused else _x_eff(c)
    xs, xt = (c.xs.to(DEV), c.xt.to(DEV)) if fused else (None, None)
    dy = c.dy.to(DEV)
    if kernel in ("dma", "reg"):
        ns = ns or m.conv3d_wgrad_nsplit(G, B, *sp, cin, cout, pad)
        ptab = None
        if kernel == "dma":
            ptab = torch.empty(_mg(c), 2, device=DEV, dtype=torch.int32)
            m.conv3d_pos_table(ptab.data_ptr(), B, *sp, pad, _st())

        def run(part, rows, ld, off, scale):
            m.conv3d_wgrad(x.data_ptr(), xs.data_ptr() if fused else 0, xt.data_ptr() if fused else 0, dy.data_ptr(),
                           part.data_ptr(), rows.data_ptr(), ld, off, G, B, *sp, cin, cout, pad, ns, scale,
                           ptab.data_ptr() if ptab is not None else 0, _st())
    elif kernel == "tri":
        assert m.conv3d_wgrad_tri_ok(B, *sp, cin, cout, pad)
        ns = ns or m.conv3d_wgrad_tri_nsplit(G, B, *sp, cin, cout, pad)
        stab = torch.empty(m.conv3d_wgrad_tri_table_size(B, *sp, pad), device=DEV, dtype=torch.int32)
        m.conv3d_wgrad_tri_table(stab.data_ptr(), B, *sp, pad, _st())

        def run(part, rows, ld, off, scale):
            m.conv3d_wgrad_tri(x.data_ptr(), dy.data_ptr(), part.data_ptr(), rows.data_ptr(), ld, off, G, B, *sp, cin,
                               cout, pad, ns, scale, stab.data_ptr(), _st())
    else:
        assert m.conv3d_wgrad_slab_ok(B, *sp, cin, cout, pad)
        ns = ns or m.conv3d_wgrad_slab_nsplit(G, B, *sp, cin, cout, pad)
        stab = torch.empty(m.conv3d_wgrad_slab_table_size(B, *sp, pad), device=DEV, dtype=torch.int32)
        m.conv3d_wgrad_slab_table(stab.data_ptr(), B, *sp, pad, _st())

        def run(part, rows, ld, off, scale):
            m.conv3d_wgrad_slab(x.data_ptr(), dy.data_ptr(), part.data_ptr(), rows.data_ptr(), ld, off, G, B, *sp, cin,
                                cout, pad, ns, scale, stab.data_ptr(), _st())
    assert ns >= 1
    for scale, off in ((1.0, 3), (0.5, 5)):
        rows, n = _rows(c, off, 7)
        part = _nan_f32(ns * G * cout * 27 * cin)
        run(part, rows, rows.stride(0), off, scale)
        _check_rows(c, rows, off, n, scale, (kernel, ns, scale))


def _dgrad3_params():
    out = []
    for name in L.CONV3:
        out += [(name, G, B, k) for G, B in L.CONV3_BWD_GB for k in ("fwd", "tri")]
    for name in L.SLAB3:
        out += [(name,) + L.SLAB3_GB + (k,) for k in ("fwd", "slab")]
    return out


@pytest.mark.parametrize("name,G,B,kernel", _dgrad3_params())
def test_conv3_dgrad_through_forward_exact(name, G, B, kernel):
    """Data gradient = the forward kernels on pack_conv_w's flipped, transposed image of the fp32 weights, at padding
    2 - pad (pad 0, 1 and 2); the packed images themselves bit for bit."""
    m = _m()
    c = L.conv3(name, G, B)
    sp, cin, cout, pad = c.dims, c.cin, c.cout, c.pad
    theta = torch.full((G, cout * cin * 27 + 64), SENT, device=DEV)
    theta[:, :cout * cin * 27] = c.w.view(G, -1).to(DEV)
    wp = _nan_bf16(G, cout, 27, cin)
    wt = _nan_bf16(G, cin, 27, cout)
    m.pack_conv_w(theta.data_ptr(), theta.stride(0), 0, G, cout, cin, 1.0, wp.data_ptr(), wt.data_ptr(), _st())
    dy = c.dy.to(DEV)
    dx = _nan_bf16(G * B, *sp, cin)
    do, p2 = c.out, 2 - pad
    if kernel == "fwd":
        m.conv3d_fwd(dy.data_ptr(), wt.data_ptr(), 0, 0, 0, dx.data_ptr(), 0, G, B, *do, cout, cin, p2, _st())
    elif kernel == "tri":
        assert m.conv3d_fwd_tri_ok(B, *do, cout, cin, p2)
        tab = torch.empty(m.conv3d_fwd_tri_table_size(B, *do, p2), device=DEV, dtype=torch.int32)
        m.conv3d_fwd_tri_table(tab.data_ptr(), B, *do, p2, _st())
        m.conv3d_fwd_tri(dy.data_ptr(), wt.data_ptr(), 0, 0, dx.data_ptr(), 0, G, B, *do, cout, cin, p2, tab.data_ptr(),
                         _st())
    else:
        assert kernel == "slab" and m.conv3d_fwd_slab_ok(B, *do, cout, cin, p2)
        tab = torch.empty(m.conv3d_fwd_slab_table_size(B, *do, p2), device=DEV, dtype=torch.int32)
        m.conv3d_fwd_slab_table(tab.data_ptr(), B, *do, p2, _st())
        m.conv3d_fwd_slab(dy.data_ptr(), wt.data_ptr(), 0, 0, dx.data_ptr(), 0, G, B, *do, cout, cin, p2,
                          tab.data_ptr(), _st())
    torch.cuda.synchronize()
    L.assert_exact(wp, c.w.view(G, cout, cin, 27).permute(0, 1, 3, 2), ("client", "cout", "tap", "cin"))
    L.assert_exact(wt, c.w.view(G, cout, cin, 27).flip(3).permute(0, 2, 3, 1), ("client", "cin", "tap", "cout"))
    L.assert_exact(dx, _cs(c.dx, c), AX3)


# ================================================================================================ generic grouped path
def _layer(c, three_d):
    """The engine's layer object for a case (tap-slot order, channel padding) and its images from the WeightPacker."""
    if three_d:
        from neuroimagedisttraining_amd.engine.resnet3d_hip import GConv3
        conv = GConv3(0, c.cout, c.cin, c.k, c.stride, c.pad)
    else:
        from neuroimagedisttraining_amd.engine.resnet2d_hip import GroupedConv
        conv = GroupedConv(0, c.cout, c.cin, c.k, c.stride, c.pad, hip=True)
    P = conv.numel
    theta = torch.zeros(c.G, (P + 63) // 64 * 64, device=DEV)[:, :P]
    theta.copy_(c.w.view(c.G, -1).to(DEV))
    wp, wt = conv._wp(theta, c.G, conv.need_dgrad)
    torch.cuda.synchronize()
    assert conv.cin_p == c.cin_p
    L.assert_exact(wp, _image(c), ("client", "cout", "tap", "cin"))
    return conv, wp, wt


def _generic(c, three_d):
    """Forward, weight gradient (splits 1, 3, the cost model's) and data gradient of one generic-path case."""
    m = _m()
    conv, wp, wt = _layer(c, three_d)
    G, B, cin, cout, kt, st, pad = c.G, c.B, c.cin_p, c.cout, c.taps, c.stride, c.pad
    D, H, W = c.dims if three_d else (1,) + c.dims
    Do, Ho, Wo = c.out if three_d else (1,) + c.out
    padd = pad if kt == 27 else 0
    ax = AX3 if three_d else AX2
    x, dy = c.x.to(DEV), c.dy.to(DEV)
    y = _nan_bf16(G * B, *c.out, cout)
    m.conv_fwd_g(x.data_ptr(), wp.data_ptr(), y.data_ptr(), G, B, D, H, W, cin, cout, kt, st, pad, padd, _st())
    torch.cuda.synchronize()
    L.assert_exact(y, _cs(c.y, c), ax)
    # weight gradient
    ptab = torch.empty(B * Do * Ho * Wo, 2, device=DEV, dtype=torch.int32)
    m.conv_pos_table_g(ptab.data_ptr(), B, D, H, W, kt, st, pad, padd, _st())
    ns_model = m.conv_wgrad_nsplit_g(G, B, D, H, W, cin, cout, kt, st, pad, padd)
    assert ns_model >= 1
    for ns in sorted({1, 3, ns_model}):
        for scale, off in ((1.0, 3), (0.5, 5)):
            rows, n = _rows(c, off, 7)
            part = _nan_f32(ns * G * cout * kt * cin)
            m.conv_wgrad_g(x.data_ptr(), dy.data_ptr(), part.data_ptr(), rows.data_ptr(), rows.stride(0), off, G, B, D,
                           H, W, cin, cout, kt, st, pad, padd, ns, scale, ptab.data_ptr(), _st())
            _check_rows(c, rows, off, n, scale, (ns, scale))
    if wt is None:  # the channel-padded stem needs no input gradient
        return
    # data gradient
    slots = list(conv.slots)
    wt_ref = torch.empty(G, c.cin, kt, cout, dtype=torch.float64)
    wflat = c.w.reshape(G, cout, c.cin, kt).double()
    for t in range(kt):
        wt_ref[:, :, slots[t], :] = wflat[:, :, :, t].transpose(1, 2)
    L.assert_exact(wt, wt_ref, ("client", "cin", "slot", "cout"))
    if st == 1:
        p2 = c.k - 1 - pad
        dx = _nan_bf16(G * B, *c.dims, cin)
        m.conv_fwd_g(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), G, B, Do, Ho, Wo, cout, cin, kt, 1, p2,
                     p2 if kt == 27 else 0, _st())
        ref = c.dx
    elif c.k == 3:  # sub-pixel phases over the dy grid, written straight into dx
        dx = _nan_bf16(G * B, *c.dims, cin)
        m.conv_dgrad_s2_g(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), G, B, Do, Ho, Wo, cout, cin, kt, D, H, W, _st())
        ref = c.dx
    else:  # 1x1 stride 2: the half-resolution gradient of the even positions (the odd ones are exactly 0)
        ref = c.dx[:, ::2, ::2, ::2] if three_d else c.dx[:, ::2, ::2]
        assert float(c.dx.abs().sum()) == float(ref.abs().sum()) and tuple(ref.shape[1:-1]) == c.out
        dx = _nan_bf16(G * B, *c.out, cin)
        m.conv_fwd_g(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), G, B, Do, Ho, Wo, cout, cin, 1, 1, 0, 0, _st())
    torch.cuda.synchronize()
    L.assert_exact(dx, _cs(ref.contiguous(), c), ax)


@pytest.mark.parametrize("name", list(L.GEN3))
def test_generic_conv3d_exact(name):
    """conv_fwd_g / conv_wgrad_g with conv_pos_table_g / conv_dgrad_s2_g at 3-D shapes (3x3x3 at stride 1 and 2 on odd
    and even extents, 1x1x1 at stride 1 and 2), the weight images through the WeightPacker."""
    _generic(L.gen3(name), True)


@pytest.mark.parametrize("name", list(L.GEN2))
def test_generic_conv2d_exact(name):
    """The same kernels at 2-D shapes (9 taps, D = 1): 3x3 stride 1, the channel-padded 3 -> 64 stem, stride 2 on odd
    and even maps, the 1x1 stride-2 projection."""
    _generic(L.gen2(name), False)


@pytest.mark.parametrize("ks", L.GEN_KS)
def test_generic_conv_splitk_exact(ks):
    """conv_fwd_gk (fp32 partials + k_fwd_splitk_sum) on a 512 -> 512 3x3x3 layer at a 2x3x2 map, which picks a split
    by itself, at forced split factors."""
    m = _m()
    c = L.gen3(L.GEN3_SPLITK[0])
    conv, wp, _ = _layer(c, True)
    G, B, cin, cout = c.G, c.B, c.cin, c.cout
    assert m.conv_fwd_g_ksplit(G, B, *c.dims, cin, cout, 27, 1, 1, 1) > 1
    x = c.x.to(DEV)
    part = _nan_f32(ks * G * _mg(c) * cout)
    y = _nan_bf16(G * B, *c.out, cout)
    m.conv_fwd_gk(x.data_ptr(), wp.data_ptr(), y.data_ptr(), part.data_ptr(), ks, G, B, *c.dims, cin, cout, 27, 1, 1, 1,
                  _st())
    torch.cuda.synchronize()
    L.assert_exact(y, _cs(c.y, c), AX3)


# ================================================================================================ 2-D slab kernels
@pytest.mark.parametrize("B,hw,cin,cout", L.SLAB2_BD)
def test_conv2d_slab_batched_depth_exact(B, hw, cin, cout):
    """conv2d_fwd_slab_bd: 8x8 maps whose 256-position blocks span several samples."""
    m = _m()
    c = L.slab2(B, hw, cin, cout)
    G = c.G
    assert m.conv2d_fwd_slab_bd_ok(B, hw, hw, cin, cout)
    x, w = c.x.to(DEV), _image(c)
    tab = torch.empty(m.conv2d_fwd_slab_bd_table_size(B, hw, hw, cin, cout), device=DEV, dtype=torch.int32)
    m.conv2d_fwd_slab_bd_table(tab.data_ptr(), B, hw, hw, cin, cout, _st())
    y = _nan_bf16(G * B, hw, hw, cout)
    m.conv2d_fwd_slab_bd(x.data_ptr(), w.data_ptr(), y.data_ptr(), G, B, hw, hw, cin, cout, tab.data_ptr(), _st())
    torch.cuda.synchronize()
    L.assert_exact(y, _cs(c.y, c), AX2)


@pytest.mark.parametrize("B,hw,cin,cout", L.SLAB2)
def test_conv2d_slab_exact(B, hw, cin, cout):
    """conv2d_fwd_slab and the output of conv2d_fwd_slab_stats (its statistics stay with the GroupNorm tests)."""
    m = _m()
    c = L.slab2(B, hw, cin, cout)
    G = c.G
    assert m.conv2d_fwd_slab_ok(B, hw, hw, cin, cout)
    x, w = c.x.to(DEV), _image(c)
    tab = torch.empty(m.conv3d_fwd_slab_table_size(B, 1, hw, hw, 1), device=DEV, dtype=torch.int32)
    m.conv3d_fwd_slab_table(tab.data_ptr(), B, 1, hw, hw, 1, _st())
    y = _nan_bf16(G * B, hw, hw, cout)
    m.conv2d_fwd_slab(x.data_ptr(), w.data_ptr(), y.data_ptr(), G, B, hw, hw, cin, cout, tab.data_ptr(), _st())
    ys = _nan_bf16(G * B, hw, hw, cout)
    zb = torch.zeros(G, cout, device=DEV)
    stats = _stats_buf(c)
    m.conv2d_fwd_slab_stats(x.data_ptr(), w.data_ptr(), zb.data_ptr(), ys.data_ptr(), stats.data_ptr(), G, B, hw, hw,
                            cin, cout, tab.data_ptr(), _st())
    torch.cuda.synchronize()
    L.assert_exact(y, _cs(c.y, c), AX2)
    L.assert_exact(ys, _cs(c.y, c), AX2)


# ================================================================================================ 1x1 GEMMs
@pytest.mark.parametrize("K,N", L.G1_SHAPES)
def test_gemm1x1_exact(K, N):
    """gemm1x1_g (every tile configuration, a partial last m-tile): the bf16 output, and the [STATS] channel sums of y
    and y^2, which are exact too when their bounds stay below 2^24."""
    m = _m()
    assert m.gemm1x1_ok(K, N)
    c = L.gemm_case("g1", L.GEMM_G, L.G1_MG, K, N)
    G, Mg = c.G, c.Mg
    x, w = c.x.to(DEV), c.w.to(torch.bfloat16).to(DEV)
    y = _nan_bf16(G, Mg, N)
    nch = m.gemm1x1_chunks(G, Mg, K, N)
    part = _nan_f32(nch, G, N, 2)
    m.gemm1x1_g(x.data_ptr(), w.data_ptr(), y.data_ptr(), G, Mg, K, N, part.data_ptr(), _st())
    y2 = _nan_bf16(G, Mg, N)
    m.gemm1x1_g(x.data_ptr(), w.data_ptr(), y2.data_ptr(), G, Mg, K, N, 0, _st())
    torch.cuda.synchronize()
    ax = ("client", "row", "channel")
    L.assert_exact(y, c.y, ax)
    L.assert_exact(y2, c.y, ax)
    ps = part.double().sum(0).cpu()
    if c.stats_exact:
        L.assert_exact(ps[..., 0], c.ysum, ("client", "channel"))
        L.assert_exact(ps[..., 1], c.ysq, ("client", "channel"))
    else:
        assert L.relerr(ps[..., 0], c.ysum) < 1e-5 and L.relerr(ps[..., 1], c.ysq) < 1e-5


@pytest.mark.parametrize("N,K", L.W1_SHAPES)
def test_wgrad1x1_exact(N, K):
    """wgrad1x1_g (every tile configuration; one chunk written by the kernel, several through k_wgrad_reduce), scale 1
    and 0.5, into sentinel-guarded rows: exact in fp32."""
    m = _m()
    assert m.wgrad1x1_ok(N, K)
    c = L.gemm_case("w1", L.GEMM_G, L.W1_MG, K, N)
    G, Mg = c.G, c.Mg
    x, dy = c.x.to(DEV), c.dy.to(DEV)
    for nmb in sorted({1, 3, m.wgrad1x1_chunks(G, Mg, N, K)}):
        for scale, off in ((1.0, 7), (0.5, 2)):
            rows = torch.full((G, off + N * K + 19), SENT, device=DEV)
            rows[:, off:off + N * K] = NAN
            part = _nan_f32(max(nmb, 1) * G * N * K)
            m.wgrad1x1_g(x.data_ptr(), dy.data_ptr(), part.data_ptr(), rows.data_ptr(), rows.stride(0), off, G, Mg, N,
                         K, nmb, scale, _st())
            torch.cuda.synchronize()
            assert float(rows[:, :off].sub(SENT).abs().max()) == 0
            assert float(rows[:, off + N * K:].sub(SENT).abs().max()) == 0
            L.assert_exact(rows[:, off:off + N * K], c.dw * scale, ("client", "cout", "cin"))


# ================================================================================================ conv2d_any
@pytest.mark.parametrize("cin,cout,k,pad,H", L.C2_SHAPES)
def test_conv2d_any_exact(cin, cout, k, pad, H):
    """conv2d_any.hip through HipConv2dFn at channel counts that are no multiple of its tiles: forward with bias, data
    gradient through the flipped image, weight gradient (chunk partials) and bias gradient."""
    from neuroimagedisttraining_amd.engine.conv2d_hip import HipConv2dFn
    c = L.c2(cin, cout, k, pad, H)
    G = c.G
    x = c.x.to(DEV).permute(0, 3, 1, 2).requires_grad_(True)  # channels-last bf16
    w = c.w.to(DEV).requires_grad_(True)
    b = c.bias.to(DEV).requires_grad_(True)
    y = HipConv2dFn.apply(x, w, b, G, pad)
    dy = c.dy.to(DEV).permute(0, 3, 1, 2)
    y.backward(dy)
    torch.cuda.synchronize()
    L.assert_exact(y.permute(0, 2, 3, 1), _cs(L.y_with_bias(c), c), AX2)
    L.assert_exact(x.grad.permute(0, 2, 3, 1), _cs(c.dx, c), AX2)
    L.assert_exact(w.grad.reshape(G, cout, cin, k * k), c.dw.reshape(G, cout, cin, k * k), AXW)
    db = c.dy.double().view(G, -1, cout).sum(1)
    L.assert_exact(b.grad, db, ("client", "channel"))
