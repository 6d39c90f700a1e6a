"""Host-side rules of the union-staged conv kernels (``csrc/kernels/conv3d.hip``: ``k_conv_wgrad_tri``,
``k_conv_fwd_tri``, ``k_conv_fwd_slab``): the union size of a band of output positions (which decides eligibility and the kernel's U) against
an independent Python model of the padded-input rows the three kw taps read, and the launch-choice rules measured in
``profiles/r2_ab_wgrad_tri.txt`` / ``profiles/r2_ab_fwd_tri.txt``.  Runs on the CPU (host functions of the built
extension; skipped when it is not built)."""
import pytest


def _ext():
    from neuroimagedisttraining_amd import ops
    try:
        return ops.ext()
    except Exception as e:  # noqa: BLE001 - extension not built in this environment
        pytest.skip("HIP extension not built: %s" % e)


def _union_rows(B, D, H, W, pad, P, slab=False):
    """Largest number of distinct padded-input rows {b(p) + kw} (``slab``: the whole window b(p) .. b(p) + 2 Wp + 2)
    over the bands of P consecutive output positions."""
    Dp, Hp, Wp = D + 2 * pad, H + 2 * pad, W + 2 * pad
    Do, Ho, Wo = Dp - 2, Hp - 2, Wp - 2
    S, vol = Do * Ho * Wo, Dp * Hp * Wp
    mg = B * S
    best = 0
    for m0 in range(0, mg, P):
        rows = set()
        for m in range(m0, min(m0 + P, mg)):
            n, r = divmod(m, S)
            od, r = divmod(r, Ho * Wo)
            oh, ow = divmod(r, Wo)
            base = n * vol + (od * Hp + oh) * Wp + ow
            rows.update(range(base, base + (2 * Wp + 3 if slab else 3)))
        best = max(best, len(rows))
    return best


@pytest.mark.parametrize("shape", [(16, 19, 23, 19, 0), (3, 19, 23, 19, 0), (16, 17, 21, 17, 2), (16, 5, 7, 5, 1),
                                   (2, 5, 7, 5, 2), (1, 9, 6, 11, 1)])
@pytest.mark.parametrize("P", [64, 256])
def test_union_size_matches_python_model(shape, P):
    m = _ext()
    assert m.conv3d_union_umax(*shape, P) == _union_rows(*shape, P)


def test_union_kernel_choices():
    m = _ext()
    conv2 = (16, 19, 23, 19, 64, 128, 0)        # AlexNet3D conv2 forward / wgrad geometry (B=16)
    conv2_dgrad = (16, 17, 21, 17, 128, 64, 2)  # its data gradient: a pad-2 forward
    conv4 = (16, 5, 7, 5, 192, 192, 1)
    for G in (64, 8, 1):
        assert m.conv3d_wgrad_tri_pick(G, *conv2) == 1          # unpadded wgrad: always
        assert m.conv3d_fwd_tri_ok(*conv2_dgrad) == 1           # supported ...
        assert m.conv3d_fwd_tri_pick(G, *conv2_dgrad) == 0      # ... but not chosen (no consistent gain)
    assert m.conv3d_fwd_tri_pick(64, *conv2) == 1
    # padded wgrad: only with >= 8 K output positions per launch (64 K before the overlapped stage DMA, [ADMA])
    assert m.conv3d_wgrad_tri_pick(64, *conv4) == 1
    assert m.conv3d_wgrad_tri_pick(8, *conv4) == 1              # 22 K positions
    assert m.conv3d_wgrad_tri_pick(1, *conv4) == 0              # 2.8 K positions
    assert m.conv3d_fwd_tri_pick(64, *conv4) == 0               # padded forwards stay on the per-tap kernel
    # split factors stay within the model's bounds and keep >= 8 steps per block
    for G in (64, 8, 1):
        ns = m.conv3d_wgrad_tri_nsplit(G, *conv2)
        assert 1 <= ns <= 64 and 16 * 17 * 21 * 17 // ns >= 512
    # table sizes: one entry per band, 2U + P ints with U a multiple of 8 covering the largest union
    n_bands = -(-16 * 17 * 21 * 17 // 64)
    per = m.conv3d_wgrad_tri_table_size(16, 19, 23, 19, 0) // n_bands
    assert per * n_bands == m.conv3d_wgrad_tri_table_size(16, 19, 23, 19, 0)
    assert (per - 64) % 16 == 0 and (per - 64) // 2 >= m.conv3d_union_umax(16, 19, 23, 19, 0, 64)


@pytest.mark.parametrize("shape", [(16, 19, 23, 19, 0), (16, 17, 21, 17, 2), (5, 10, 12, 11, 1), (16, 8, 14, 20, 1),
                                   (3, 19, 23, 19, 0), (16, 5, 7, 5, 1), (4, 31, 37, 31, 1), (4, 16, 19, 16, 1)])
def test_slab_union_matches_python_model(shape):
    """kd-slab unions: size vs the Python model, and the addressing invariant the kernel relies on — every tap
    (kh, kw) of a position reads union row idx(p) + kh Wp + kw (whole windows make the union contiguous there)."""
    m = _ext()
    B, D, H, W, pad = shape
    um = _union_rows(*shape, 256, slab=True)
    assert m.conv3d_slab_umax(*shape) == um
    assert m.conv3d_fwd_slab_ok(B, D, H, W, 64, 64, pad) == (1 if um <= 416 else 0)      # 64-channel blocks
    assert m.conv3d_fwd_slab_ok(B, D, H, W, 64, 128, pad) == (1 if um <= 384 else 0)     # 128-channel blocks
    Dp, Hp, Wp = D + 2 * pad, H + 2 * pad, W + 2 * pad
    Do, Ho, Wo = Dp - 2, Hp - 2, Wp - 2
    S, vol = Do * Ho * Wo, Dp * Hp * Wp
    for m0 in range(0, B * S, 256):
        bases = []
        for q in range(m0, min(m0 + 256, B * S)):
            n, r = divmod(q, S)
            od, r = divmod(r, Ho * Wo)
            oh, ow = divmod(r, Wo)
            bases.append(n * vol + (od * Hp + oh) * Wp + ow)
        union = sorted({b + e for b in bases for e in range(2 * Wp + 3)})
        pos = {r: i for i, r in enumerate(union)}
        for b in bases:
            for kh in range(3):
                for kw in range(3):
                    assert pos[b + kh * Wp + kw] == pos[b] + kh * Wp + kw


def test_slab_kernel_choice():
    m = _ext()
    conv2 = (16, 19, 23, 19, 64, 128, 0)
    conv2_dgrad = (16, 17, 21, 17, 128, 64, 2)
    for G in (64, 8):
        assert m.conv3d_fwd_slab_ok(*conv2) == 1 and m.conv3d_fwd_slab_ok(*conv2_dgrad) == 1
        assert m.conv3d_fwd_slab_pick(G, *conv2_dgrad) == 1      # padded data gradient: the slab kernel
    assert m.conv3d_fwd_slab_ok(16, 5, 7, 5, 192, 192, 1) == 0   # 5x7x5 bands: unions of ~470 rows
    n_bands = -(-16 * 19 * 23 * 19 // 256)
    assert m.conv3d_fwd_slab_table_size(16, 17, 21, 17, 2) == n_bands * (2 * 384 + 256)


def test_conv2d_slab_choice():
    """2-D 3x3 convs on the slab kernel (D = 1 volumes, pad 1): eligible when every 256-position block lies in one
    sample and the band union fits; picked for 64-channel blocks always and 128-channel blocks from 160 blocks up."""
    m = _ext()
    assert m.conv3d_slab_umax(16, 1, 32, 32, 1) == _union_rows(16, 1, 32, 32, 1, 256, slab=True) == 340
    assert m.conv3d_slab_umax(16, 1, 64, 64, 1) == 396                      # Tiny layer 1: the 416-row variant
    assert m.conv2d_fwd_slab_ok(16, 32, 32, 64, 64) == 1
    assert m.conv2d_fwd_slab_ok(16, 64, 64, 64, 64) == 1
    assert m.conv2d_fwd_slab_ok(16, 64, 64, 128, 128) == 0                  # 416-row unions only for 64-ch blocks
    assert m.conv2d_fwd_slab_ok(16, 8, 8, 256, 256) == 0                    # 64-position samples: blocks straddle
    assert m.conv2d_fwd_slab_ok(16, 16, 16, 256, 256) == 1
    assert m.conv2d_fwd_slab_pick(1, 16, 32, 32, 64, 64) == 1              # 64-channel blocks: any grid
    assert m.conv2d_fwd_slab_pick(4, 16, 16, 16, 128, 128) == 0            # 64 blocks of 128 channels
    assert m.conv2d_fwd_slab_pick(10, 16, 16, 16, 128, 128) == 1           # 160 blocks
    assert m.conv2d_fwd_slab_pick(2, 16, 16, 16, 256, 256) == 0            # 64 blocks
    assert m.conv2d_fwd_slab_pick(10, 16, 16, 16, 256, 256) == 1
    n_bands = 16 * 32 * 32 // 256
    assert m.conv3d_fwd_slab_table_size(16, 1, 32, 32, 1) == n_bands * (2 * 384 + 256)


# Host decisions of the conv launchers, recorded from the build before the launch dispatch was rewritten (default
# environment: no NIDT_* switch set): function -> (arguments, result; a string = the call raises ValueError with that
# text).  Shapes: the AlexNet3D conv2 / conv2 data gradient / conv3 / conv4 / conv5 geometries above at 1, 8 and 64
# clients, the 31x37x31 layer-1 conv of the 3D ResNet at 1 and 8, and the ResNet-18-GN maps 32x32 (64 channels), 16x16
# (128), 8x8 (256), 4x4 (512) and the Tiny 64x64 (64) at B = 16 and 10 / 100 clients.
_PINNED = {
    "conv3d_fwd_tri_ok": [
        ((16, 19, 23, 19, 64, 128, 0), 1), ((16, 17, 21, 17, 128, 64, 2), 1), ((16, 5, 7, 5, 128, 192, 1), 1),
        ((16, 5, 7, 5, 192, 192, 1), 1), ((16, 5, 7, 5, 192, 128, 1), 1), ((4, 31, 37, 31, 64, 64, 1), 1),
    ],
    "conv3d_fwd_slab_ok": [
        ((16, 19, 23, 19, 64, 128, 0), 1), ((16, 17, 21, 17, 128, 64, 2), 1), ((16, 5, 7, 5, 128, 192, 1), 0),
        ((16, 5, 7, 5, 192, 192, 1), 0), ((16, 5, 7, 5, 192, 128, 1), 0), ((4, 31, 37, 31, 64, 64, 1), 1),
    ],
    "conv3d_wgrad_tri_ok": [
        ((16, 19, 23, 19, 64, 128, 0), 1), ((16, 17, 21, 17, 128, 64, 2), 1), ((16, 5, 7, 5, 128, 192, 1), 1),
        ((16, 5, 7, 5, 192, 192, 1), 1), ((16, 5, 7, 5, 192, 128, 1), 1), ((4, 31, 37, 31, 64, 64, 1), 1),
    ],
    "conv3d_wgrad_slab_ok": [
        ((16, 19, 23, 19, 64, 128, 0), 1), ((16, 17, 21, 17, 128, 64, 2), 0), ((16, 5, 7, 5, 128, 192, 1), 1),
        ((16, 5, 7, 5, 192, 192, 1), 1), ((16, 5, 7, 5, 192, 128, 1), 1), ((4, 31, 37, 31, 64, 64, 1), 0),
    ],
    "conv3d_fwd_tri_table_size": [
        ((16, 19, 23, 19, 0), 340480), ((16, 17, 21, 17, 2), 465024), ((16, 5, 7, 5, 1), 11264),
        ((4, 31, 37, 31, 1), 498176),
    ],
    "conv3d_fwd_slab_table_size": [
        ((16, 19, 23, 19, 0), 389120), ((16, 17, 21, 17, 2), 531456),
        ((16, 5, 7, 5, 1), 'nidt: conv3d_fwd_slab_table_size: shape not eligible'), ((4, 31, 37, 31, 1), 604928),
        ((16, 1, 32, 32, 1), 65536), ((1, 16, 32, 32, 1), 65536), ((16, 1, 16, 16, 1), 16384),
        ((1, 16, 16, 16, 1), 16384), ((16, 1, 8, 8, 1), 4352), ((1, 16, 8, 8, 1), 4352),
        ((16, 1, 4, 4, 1), 'nidt: conv3d_fwd_slab_table_size: shape not eligible'),
        ((1, 16, 4, 4, 1), 'nidt: conv3d_fwd_slab_table_size: shape not eligible'), ((16, 1, 64, 64, 1), 278528),
        ((1, 16, 64, 64, 1), 278528),
    ],
    "conv3d_wgrad_tri_table_size": [
        ((16, 19, 23, 19, 0), 340032), ((16, 17, 21, 17, 2), 465024), ((16, 5, 7, 5, 1), 11264),
        ((4, 31, 37, 31, 1), 497952),
    ],
    "conv3d_wgrad_slab_table_size": [
        ((16, 19, 23, 19, 0), 558624), ((16, 17, 21, 17, 2), 'nidt: conv3d_wgrad_slab_table_size: shape not eligible'),
        ((16, 5, 7, 5, 1), 16192), ((4, 31, 37, 31, 1), 'nidt: conv3d_wgrad_slab_table_size: shape not eligible'),
    ],
    "conv3d_fwd_bp": [
        ((64, 128, 0, 1, 97104), 256), ((64, 128, 0, 8, 97104), 256), ((64, 128, 0, 64, 97104), 256),
        ((128, 64, 0, 1, 132848), 256), ((128, 64, 0, 8, 132848), 256), ((128, 64, 0, 64, 132848), 256),
        ((128, 192, 0, 1, 2800), 64), ((128, 192, 0, 8, 2800), 128), ((128, 192, 0, 64, 2800), 256),
        ((192, 192, 0, 1, 2800), 64), ((192, 192, 0, 8, 2800), 128), ((192, 192, 0, 64, 2800), 256),
        ((192, 128, 0, 1, 2800), 64), ((192, 128, 0, 8, 2800), 64), ((192, 128, 0, 64, 2800), 256),
        ((64, 64, 0, 1, 142228), 256), ((64, 64, 0, 8, 142228), 256), ((64, 64, 0, 10, 16384), 256),
        ((64, 64, 0, 100, 16384), 256), ((128, 128, 0, 10, 4096), 64), ((128, 128, 0, 100, 4096), 256),
        ((256, 256, 0, 10, 1024), 64), ((256, 256, 0, 100, 1024), 256), ((512, 512, 0, 10, 256), 64),
        ((512, 512, 0, 100, 256), 256), ((64, 64, 0, 10, 65536), 256), ((64, 64, 0, 100, 65536), 256),
    ],
    "conv3d_fwd_ksplit": [
        ((64, 128, 1, 97104), 1), ((64, 128, 8, 97104), 1), ((64, 128, 64, 97104), 1), ((128, 64, 1, 132848), 1),
        ((128, 64, 8, 132848), 1), ((128, 64, 64, 132848), 1), ((128, 192, 1, 2800), 4), ((128, 192, 8, 2800), 1),
        ((128, 192, 64, 2800), 1), ((192, 192, 1, 2800), 4), ((192, 192, 8, 2800), 1), ((192, 192, 64, 2800), 1),
        ((192, 128, 1, 2800), 6), ((192, 128, 8, 2800), 1), ((192, 128, 64, 2800), 1), ((64, 64, 1, 142228), 1),
        ((64, 64, 8, 142228), 1), ((64, 64, 10, 16384), 1), ((64, 64, 100, 16384), 1), ((128, 128, 10, 4096), 1),
        ((128, 128, 100, 4096), 1), ((256, 256, 10, 1024), 1), ((256, 256, 100, 1024), 1), ((512, 512, 10, 256), 1),
        ((512, 512, 100, 256), 1), ((64, 64, 10, 65536), 1), ((64, 64, 100, 65536), 1),
    ],
    "conv3d_fwd_tri_pick": [
        ((1, 16, 19, 23, 19, 64, 128, 0), 1), ((8, 16, 19, 23, 19, 64, 128, 0), 1),
        ((64, 16, 19, 23, 19, 64, 128, 0), 1), ((1, 16, 17, 21, 17, 128, 64, 2), 0),
        ((8, 16, 17, 21, 17, 128, 64, 2), 0), ((64, 16, 17, 21, 17, 128, 64, 2), 0),
        ((1, 16, 5, 7, 5, 128, 192, 1), 0), ((8, 16, 5, 7, 5, 128, 192, 1), 0), ((64, 16, 5, 7, 5, 128, 192, 1), 0),
        ((1, 16, 5, 7, 5, 192, 192, 1), 0), ((8, 16, 5, 7, 5, 192, 192, 1), 0), ((64, 16, 5, 7, 5, 192, 192, 1), 0),
        ((1, 16, 5, 7, 5, 192, 128, 1), 0), ((8, 16, 5, 7, 5, 192, 128, 1), 0), ((64, 16, 5, 7, 5, 192, 128, 1), 0),
        ((1, 4, 31, 37, 31, 64, 64, 1), 0), ((8, 4, 31, 37, 31, 64, 64, 1), 0),
    ],
    "conv3d_fwd_slab_pick": [
        ((1, 16, 19, 23, 19, 64, 128, 0), 1), ((8, 16, 19, 23, 19, 64, 128, 0), 1),
        ((64, 16, 19, 23, 19, 64, 128, 0), 1), ((1, 16, 17, 21, 17, 128, 64, 2), 1),
        ((8, 16, 17, 21, 17, 128, 64, 2), 1), ((64, 16, 17, 21, 17, 128, 64, 2), 1),
        ((1, 16, 5, 7, 5, 128, 192, 1), 0), ((8, 16, 5, 7, 5, 128, 192, 1), 0), ((64, 16, 5, 7, 5, 128, 192, 1), 0),
        ((1, 16, 5, 7, 5, 192, 192, 1), 0), ((8, 16, 5, 7, 5, 192, 192, 1), 0), ((64, 16, 5, 7, 5, 192, 192, 1), 0),
        ((1, 16, 5, 7, 5, 192, 128, 1), 0), ((8, 16, 5, 7, 5, 192, 128, 1), 0), ((64, 16, 5, 7, 5, 192, 128, 1), 0),
        ((1, 4, 31, 37, 31, 64, 64, 1), 1), ((8, 4, 31, 37, 31, 64, 64, 1), 1),
    ],
    "conv3d_wgrad_tri_pick": [
        ((1, 16, 19, 23, 19, 64, 128, 0), 1), ((8, 16, 19, 23, 19, 64, 128, 0), 1),
        ((64, 16, 19, 23, 19, 64, 128, 0), 1), ((1, 16, 17, 21, 17, 128, 64, 2), 1),
        ((8, 16, 17, 21, 17, 128, 64, 2), 1), ((64, 16, 17, 21, 17, 128, 64, 2), 1),
        ((1, 16, 5, 7, 5, 128, 192, 1), 0), ((8, 16, 5, 7, 5, 128, 192, 1), 1), ((64, 16, 5, 7, 5, 128, 192, 1), 1),
        ((1, 16, 5, 7, 5, 192, 192, 1), 0), ((8, 16, 5, 7, 5, 192, 192, 1), 1), ((64, 16, 5, 7, 5, 192, 192, 1), 1),
        ((1, 16, 5, 7, 5, 192, 128, 1), 0), ((8, 16, 5, 7, 5, 192, 128, 1), 1), ((64, 16, 5, 7, 5, 192, 128, 1), 1),
        ((1, 4, 31, 37, 31, 64, 64, 1), 1), ((8, 4, 31, 37, 31, 64, 64, 1), 1),
    ],
    "conv3d_wgrad_tri_nsplit": [
        ((1, 16, 19, 23, 19, 64, 128, 0), 64), ((8, 16, 19, 23, 19, 64, 128, 0), 22),
        ((64, 16, 19, 23, 19, 64, 128, 0), 7), ((1, 16, 17, 21, 17, 128, 64, 2), 55),
        ((8, 16, 17, 21, 17, 128, 64, 2), 7), ((64, 16, 17, 21, 17, 128, 64, 2), 8),
        ((1, 16, 5, 7, 5, 128, 192, 1), 5), ((8, 16, 5, 7, 5, 128, 192, 1), 2), ((64, 16, 5, 7, 5, 128, 192, 1), 1),
        ((1, 16, 5, 7, 5, 192, 192, 1), 5), ((8, 16, 5, 7, 5, 192, 192, 1), 1), ((64, 16, 5, 7, 5, 192, 192, 1), 1),
        ((1, 16, 5, 7, 5, 192, 128, 1), 5), ((8, 16, 5, 7, 5, 192, 128, 1), 2), ((64, 16, 5, 7, 5, 192, 128, 1), 1),
        ((1, 4, 31, 37, 31, 64, 64, 1), 64), ((8, 4, 31, 37, 31, 64, 64, 1), 14),
    ],
    "conv3d_wgrad_slab_nsplit": [
        ((1, 16, 19, 23, 19, 64, 128, 0), 42), ((8, 16, 19, 23, 19, 64, 128, 0), 5),
        ((64, 16, 19, 23, 19, 64, 128, 0), 2), ((1, 16, 17, 21, 17, 128, 64, 2), 42),
        ((8, 16, 17, 21, 17, 128, 64, 2), 16), ((64, 16, 17, 21, 17, 128, 64, 2), 2),
        ((1, 16, 5, 7, 5, 128, 192, 1), 5), ((8, 16, 5, 7, 5, 128, 192, 1), 3), ((64, 16, 5, 7, 5, 128, 192, 1), 1),
        ((1, 16, 5, 7, 5, 192, 192, 1), 5), ((8, 16, 5, 7, 5, 192, 192, 1), 1), ((64, 16, 5, 7, 5, 192, 192, 1), 1),
        ((1, 16, 5, 7, 5, 192, 128, 1), 5), ((8, 16, 5, 7, 5, 192, 128, 1), 3), ((64, 16, 5, 7, 5, 192, 128, 1), 1),
        ((1, 4, 31, 37, 31, 64, 64, 1), 64), ((8, 4, 31, 37, 31, 64, 64, 1), 10),
    ],
    "conv3d_wgrad_nsplit": [
        ((1, 16, 19, 23, 19, 64, 128, 0), 36), ((8, 16, 19, 23, 19, 64, 128, 0), 9),
        ((64, 16, 19, 23, 19, 64, 128, 0), 4), ((1, 16, 17, 21, 17, 128, 64, 2), 36),
        ((8, 16, 17, 21, 17, 128, 64, 2), 9), ((64, 16, 17, 21, 17, 128, 64, 2), 4),
        ((1, 16, 5, 7, 5, 128, 192, 1), 5), ((8, 16, 5, 7, 5, 128, 192, 1), 1), ((64, 16, 5, 7, 5, 128, 192, 1), 1),
        ((1, 16, 5, 7, 5, 192, 192, 1), 5), ((8, 16, 5, 7, 5, 192, 192, 1), 1), ((64, 16, 5, 7, 5, 192, 192, 1), 1),
        ((1, 16, 5, 7, 5, 192, 128, 1), 5), ((8, 16, 5, 7, 5, 192, 128, 1), 1), ((64, 16, 5, 7, 5, 192, 128, 1), 1),
        ((1, 4, 31, 37, 31, 64, 64, 1), 64), ((8, 4, 31, 37, 31, 64, 64, 1), 9),
    ],
    "conv_wgrad_nsplit_g": [
        ((1, 16, 19, 23, 19, 64, 128, 27, 1, 0, 0), 36), ((8, 16, 19, 23, 19, 64, 128, 27, 1, 0, 0), 9),
        ((64, 16, 19, 23, 19, 64, 128, 27, 1, 0, 0), 4), ((1, 16, 17, 21, 17, 128, 64, 27, 1, 2, 2), 36),
        ((8, 16, 17, 21, 17, 128, 64, 27, 1, 2, 2), 9), ((64, 16, 17, 21, 17, 128, 64, 27, 1, 2, 2), 4),
        ((1, 16, 5, 7, 5, 128, 192, 27, 1, 1, 1), 5), ((8, 16, 5, 7, 5, 128, 192, 27, 1, 1, 1), 1),
        ((64, 16, 5, 7, 5, 128, 192, 27, 1, 1, 1), 1), ((1, 16, 5, 7, 5, 192, 192, 27, 1, 1, 1), 5),
        ((8, 16, 5, 7, 5, 192, 192, 27, 1, 1, 1), 1), ((64, 16, 5, 7, 5, 192, 192, 27, 1, 1, 1), 1),
        ((1, 16, 5, 7, 5, 192, 128, 27, 1, 1, 1), 5), ((8, 16, 5, 7, 5, 192, 128, 27, 1, 1, 1), 1),
        ((64, 16, 5, 7, 5, 192, 128, 27, 1, 1, 1), 1), ((1, 4, 31, 37, 31, 64, 64, 27, 1, 1, 1), 64),
        ((8, 4, 31, 37, 31, 64, 64, 27, 1, 1, 1), 9), ((10, 16, 1, 32, 32, 64, 64, 9, 1, 1, 0), 16),
        ((100, 16, 1, 32, 32, 64, 64, 9, 1, 1, 0), 3), ((10, 16, 1, 16, 16, 128, 128, 9, 1, 1, 0), 5),
        ((100, 16, 1, 16, 16, 128, 128, 9, 1, 1, 0), 1), ((10, 16, 1, 8, 8, 256, 256, 9, 1, 1, 0), 1),
        ((100, 16, 1, 8, 8, 256, 256, 9, 1, 1, 0), 1), ((10, 16, 1, 4, 4, 512, 512, 9, 1, 1, 0), 1),
        ((100, 16, 1, 4, 4, 512, 512, 9, 1, 1, 0), 1), ((10, 16, 1, 64, 64, 64, 64, 9, 1, 1, 0), 17),
        ((100, 16, 1, 64, 64, 64, 64, 9, 1, 1, 0), 5),
    ],
    "conv2d_fwd_slab_ok": [
        ((16, 32, 32, 64, 64), 1), ((16, 16, 16, 128, 128), 1), ((16, 8, 8, 256, 256), 0), ((16, 4, 4, 512, 512), 0),
        ((16, 64, 64, 64, 64), 1),
    ],
    "conv2d_fwd_slab_bd_ok": [
        ((16, 32, 32, 64, 64), 0), ((16, 16, 16, 128, 128), 0), ((16, 8, 8, 256, 256), 1), ((16, 4, 4, 512, 512), 1),
        ((16, 64, 64, 64, 64), 0),
    ],
    "conv2d_fwd_slab_bd_table_size": [
        ((16, 32, 32, 64, 64), 'nidt: conv2d_fwd_slab_bd_table_size: shape not eligible'),
        ((16, 16, 16, 128, 128), 'nidt: conv2d_fwd_slab_bd_table_size: shape not eligible'),
        ((16, 8, 8, 256, 256), 4352), ((16, 4, 4, 512, 512), 1792),
        ((16, 64, 64, 64, 64), 'nidt: conv2d_fwd_slab_bd_table_size: shape not eligible'),
    ],
    "conv2d_fwd_slab_pick": [
        ((10, 16, 32, 32, 64, 64), 1), ((100, 16, 32, 32, 64, 64), 1), ((10, 16, 16, 16, 128, 128), 1),
        ((100, 16, 16, 16, 128, 128), 1), ((10, 16, 8, 8, 256, 256), 0), ((100, 16, 8, 8, 256, 256), 0),
        ((10, 16, 4, 4, 512, 512), 0), ((100, 16, 4, 4, 512, 512), 0), ((10, 16, 64, 64, 64, 64), 1),
        ((100, 16, 64, 64, 64, 64), 1),
    ],
    "conv2d_fwd_slab_bd_pick": [
        ((10, 16, 32, 32, 64, 64), 0), ((100, 16, 32, 32, 64, 64), 0), ((10, 16, 16, 16, 128, 128), 0),
        ((100, 16, 16, 16, 128, 128), 0), ((10, 16, 8, 8, 256, 256), 1), ((100, 16, 8, 8, 256, 256), 1),
        ((10, 16, 4, 4, 512, 512), 0), ((100, 16, 4, 4, 512, 512), 1), ((10, 16, 64, 64, 64, 64), 0),
        ((100, 16, 64, 64, 64, 64), 0),
    ],
}


def test_host_decisions_pinned():
    m = _ext()
    assert sum(len(v) for v in _PINNED.values()) == 268
    for fn, cases in _PINNED.items():
        for args, want in cases:
            if isinstance(want, str):
                with pytest.raises(ValueError) as err:
                    getattr(m, fn)(*args)
                assert str(err.value) == want, (fn, args)
            else:
                assert getattr(m, fn)(*args) == want, (fn, args)
