"""Integer-lattice operands, fp64 CPU references and a bit-exact comparison for the bf16 conv / GEMM kernels.

Operands are small integers (activations and output gradients in {-2..2}, weights in {-1, 0, 1}, bias in [-4, 4]), so
every product and every partial sum of a convolution is an integer far below 2^24: the fp32 accumulation order of a
kernel does not matter, a bf16 store of a result of magnitude <= 256 is exact, and a correct kernel equals the fp64
reference bit for bit.  One wrong, missing or repeated term anywhere changes an integer and fails ``assert_exact``,
which reports where.

The preconditions that make this true are asserted here on the reference alone, before any comparison:

* bf16 outputs: ``max |ref| <= 256`` (bf16 holds every integer up to 256);
* fp32 outputs: the bound ``sum |a| |b|`` per output is below 2^24 (the bound, not the realised value: partial sums
  occur in any order).  For weight gradients the bound used is ``positions * max|x| * max|dy|``, which dominates it.

This is a plain helper module (no fixtures): ``tests/test_cpu_lattice.py`` checks the generators and the comparison
without a GPU, ``tests/test_gpu_exact_conv.py`` runs the kernels.  Both take their shapes from the tables below.
"""
import functools
import types
import zlib

import torch
import torch.nn.functional as F

BF16_EXACT = 256          # every integer of magnitude <= 256 is a bf16 value
FP32_EXACT = 1 << 24      # every integer of magnitude <= 2^24 is an fp32 value
NNZ_PER_ROW = 256         # default non-zero weights per output row

# ------------------------------------------------------------------------------------------------ shape tables
# 3x3x3 stride-1 family (conv3d_fwd, _splitk, _tri, _bld; conv3d_wgrad, _tri, _slab; dgrad through conv3d_fwd)
#   name: (cin, cout, pad, (D, H, W), fused input transform)
CONV3 = {
    "pad1": (128, 192, 1, (5, 7, 5), False),
    "pad0": (64, 128, 0, (7, 9, 7), False),
    "pad2": (128, 64, 2, (5, 7, 5), False),
    "xf": (192, 192, 1, (5, 7, 5), True),
}
# (G, B) per case: pad1 takes the 64-, 128- and 256-position blocks of the forward
CONV3_GB = {"pad1": [(2, 3), (8, 16), (16, 16)], "pad0": [(2, 3), (8, 16)], "pad2": [(2, 3), (8, 16)],
            "xf": [(2, 3), (16, 16)]}
# weight / data gradients: B = 16 has steps crossing depth slices and samples, B = 3 a short last position block
CONV3_BWD_GB = [(2, 16), (2, 3)]
SPLITK3 = (2, 3, 4)       # split factors of conv3d_fwd_splitk
# kd-slab union kernels (conv3d_fwd_slab, conv3d_wgrad_slab): the 5x7x5 maps above do not fit their unions at B >= 2,
# so they get the smallest maps with three or more 256-position bands that conv3d_fwd_slab_ok accepts
#   name: (cin, cout, pad, (D, H, W)), at (G, B) = SLAB3_GB
SLAB3 = {
    "slab_pad1": (128, 128, 1, (3, 11, 10)),
    "slab_pad0": (64, 64, 0, (4, 15, 10)),
    "slab_pad2": (64, 128, 2, (3, 9, 9)),
}
SLAB3_GB = (2, 3)

# generic grouped path (conv_fwd_g, conv_fwd_gk, conv_wgrad_g, conv_dgrad_s2_g), 3-D: (cin, cout, k, stride, (D, H, W))
GEN3 = {
    "k3s1": (64, 64, 3, 1, (5, 6, 5)),
    "k3s2_odd": (64, 128, 3, 2, (5, 7, 5)),
    "k3s2_even": (64, 128, 3, 2, (4, 6, 4)),
    "k1s1": (128, 64, 1, 1, (4, 5, 4)),
    "k1s2": (128, 256, 1, 2, (4, 5, 4)),
}
GEN3_SPLITK = ("k3s1_512", (512, 512, 3, 1, (2, 3, 2)))
GEN_KS = (2, 5, 8)
# 2-D (kt 9 / 1, D = 1): (cin, cout, k, stride, pad, hw)
GEN2 = {
    "c64_hw8": (64, 64, 3, 1, 1, 8),
    "stem3": (3, 64, 3, 1, 1, 8),
    "s2_hw7": (64, 128, 3, 2, 1, 7),
    "s2_hw8": (64, 128, 3, 2, 1, 8),
    "k1s2": (64, 128, 1, 2, 0, 8),
}
GEN_GB = (3, 2)
# 2-D slab kernels: (B, hw, cin, cout).  8x8 maps run on the depth-batched form (conv2d_fwd_slab_bd); the plain and
# statistics forms need whole 256-position blocks per sample, i.e. 16x16 maps at the least
SLAB2_BD = [(6, 8, 64, 64), (3, 8, 128, 256)]
SLAB2 = [(3, 16, 64, 64), (2, 16, 128, 256)]
SLAB2_G = 2

# 1x1 GEMMs: the lists of tests/test_gpu_resnet3d.py (the GPU file asserts they have not drifted)
G1_SHAPES = [(64, 256), (64, 128), (64, 64), (128, 256), (128, 128), (128, 64), (256, 128), (256, 64), (512, 64),
             (512, 128), (256, 1024)]
G1_MG = 2 * 64 * 9 + 37
W1_SHAPES = [(64, 64), (256, 64), (64, 256), (128, 128), (128, 256), (256, 128), (512, 128), (128, 512)]
W1_MG = 64 * 5 + 21
GEMM_G = 3

# conv2d_any: (cin, cout, k, pad, H) at (G, B) = C2_GB
C2_SHAPES = [(1, 20, 5, 0, 12), (3, 6, 5, 0, 9), (32, 64, 5, 2, 7), (64, 128, 3, 1, 6)]
C2_GB = (3, 4)


# ------------------------------------------------------------------------------------------------ generators
def gen(*key):
    """A CPU generator seeded by the case key (the same operands in every process)."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def int_acts(shape, g):
    """Integer activations / output gradients, uniform in {-2..2}, bf16."""
    return torch.randint(-2, 3, tuple(shape), generator=g).to(torch.bfloat16)


def int_weights(G, cout, cin, taps, g, nnz_per_row=NNZ_PER_ROW):
    """fp32 weights [G, cout, cin, taps] in {-1, 0, 1}: each entry non-zero with probability nnz_per_row / (taps cin)
    (at most 1), so an output row has about nnz_per_row terms.  Every (client, tap) keeps a non-zero weight."""
    density = min(1.0, nnz_per_row / float(taps * cin))
    if not density > 0:
        raise ValueError("int_weights: zero density")
    keep = torch.rand(G, cout, cin, taps, generator=g) < density
    sign = torch.randint(0, 2, (G, cout, cin, taps), generator=g) * 2 - 1
    w = (keep * sign).float()
    if not bool((w != 0).any(1).any(1).all()):
        raise ValueError("int_weights: a tap was left without a non-zero weight (cout %d cin %d taps %d)"
                         % (cout, cin, taps))
    return w


def int_bias(G, cout, g):
    return torch.randint(-4, 5, (G, cout), generator=g).float()


def int_transform(G, cin, g):
    """Fused input transform relu(x * xs + xt): xs in {1, 2}, xt in {-1, 0, 1} (results are integers in [0, 5])."""
    return (torch.randint(1, 3, (G, cin), generator=g).float(), torch.randint(-1, 2, (G, cin), generator=g).float())


# ------------------------------------------------------------------------------------------------ preconditions
def require_bf16_exact(ref, what):
    m = float(ref.abs().max())
    if not m <= BF16_EXACT:
        raise ValueError("%s: max |ref| = %g exceeds %d, a bf16 store would round" % (what, m, BF16_EXACT))
    return m


def require_fp32_exact(bound, what):
    if not float(bound) < FP32_EXACT:
        raise ValueError("%s: sum |a||b| bound %g reaches 2^24, fp32 partial sums could round" % (what, float(bound)))
    return float(bound)


# ------------------------------------------------------------------------------------------------ comparison
def assert_exact(got, ref, names):
    """``got`` (any dtype / device) equals the fp64 reference bit for bit.  ``ref`` carries one axis per name (e.g.
    client, sample, d, h, w, channel); ``got`` is viewed in that shape.  A failure reports the mismatch count and the
    first and the worst index with the values there; a non-finite output fails too."""
    ref = ref.detach().double().cpu()
    assert len(names) == ref.dim(), (names, tuple(ref.shape))
    got = got.detach().double().cpu()
    assert got.numel() == ref.numel(), "shape: got %s, reference %s" % (tuple(got.shape), tuple(ref.shape))
    got = got.reshape(ref.shape)
    if torch.equal(got, ref):
        return
    bad = got != ref  # NaN != x holds, so non-finite outputs count
    err = (got - ref).abs()
    err[~torch.isfinite(got)] = float("inf")
    flat = bad.flatten()

    def at(i):
        idx = []
        for s in reversed(ref.shape):
            idx.append(i % s)
            i //= s
        idx = tuple(reversed(idx))
        return "(%s): got %r, reference %r" % (", ".join("%s=%d" % (n, v) for n, v in zip(names, idx)),
                                               float(got[idx]), float(ref[idx]))
    first = int(torch.nonzero(flat)[0])
    worst = int(err.flatten().argmax())
    raise AssertionError("%d of %d values differ (%d non-finite); first at %s; worst at %s"
                         % (int(flat.sum()), flat.numel(), int((~torch.isfinite(got)).sum()), at(first), at(worst)))


def relerr(a, b):
    """The whole-tensor relative norm of the older conv tests."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------ references
def _nc(x):  # channels-last [N, *sp, C] -> [N, C, *sp]
    return x.movedim(-1, 1)


def _cl(x):  # [N, C, *sp] -> channels-last, contiguous
    return x.movedim(1, -1).contiguous()


def conv_reference(x, w, dy_of, G, stride, pad, xs=None, xt=None, grads=True):
    """fp64 CPU reference of a client-grouped conv, by autograd per client.  x: [G B, *sp, cin] (channels last), w:
    [G, cout, cin, *k]; ``dy_of(shape)`` draws the output gradient [G B, *out, cout].  Returns (y, dy, dx, dw), y / dx
    channels-last fp64, dw [G, cout, cin, *k] fp64.  With an input transform (xs, xt: [G, cin]) the conv reads
    relu(x xs + xt) and dx is the gradient with respect to that transformed input.  Without ``grads`` only y is
    computed (dy, dx, dw are None)."""
    nd = x.dim() - 2
    conv = F.conv3d if nd == 3 else F.conv2d
    B = x.shape[0] // G
    ys, dxs, dws = [], [], []
    dy = None
    for g in range(G):
        xin = x[g * B:(g + 1) * B].double()
        if xs is not None:
            xin = torch.relu(xin * xs[g].double() + xt[g].double())
        xin = _nc(xin).contiguous().requires_grad_(grads)
        wg = w[g].double().requires_grad_(grads)
        y = conv(xin, wg, None, stride, pad)
        if not grads:
            ys.append(_cl(y))
            continue
        if dy is None:
            dy = dy_of((x.shape[0],) + tuple(y.shape[2:]) + (y.shape[1],))
        y.backward(_nc(dy[g * B:(g + 1) * B].double()))
        ys.append(_cl(y.detach()))
        dxs.append(_cl(xin.grad))
        dws.append(wg.grad)
    if not grads:
        return torch.cat(ys), None, None, None
    return torch.cat(ys), dy, torch.cat(dxs), torch.stack(dws)


@functools.lru_cache(maxsize=4)
def conv_case(name, G, B, cin, cout, k, stride, pad, dims, bias=False, xf=False, nnz=NNZ_PER_ROW, pad_cin=True,
              grads=True):
    """One lattice case of a client-grouped conv (2-D or 3-D by len(dims)) with its fp64 references and the
    preconditions asserted.  Fields (CPU tensors): x [G B, *dims, cin_p] bf16 (cin zero-padded to a multiple of 64
    unless ``pad_cin`` is off, as the channel-padded stem), w [G, cout, cin, *k] fp32, bias / xs / xt [G, c] fp32 or
    None, dy [G B, *out, cout] bf16, y (no bias) / dx fp64 channels-last, dw fp64 [G, cout, cin, *k] (dy, dx, dw None
    without ``grads``: forward-only cases).  Cached: the tests of a kernel family share one case and must not modify
    it."""
    g = gen(name, G, B, cin, cout, k, stride, pad, dims, bias, xf, grads)
    nd = len(dims)
    taps = k ** nd
    c = types.SimpleNamespace(name=name, G=G, B=B, cin=cin, cout=cout, k=k, stride=stride, pad=pad, dims=tuple(dims),
                              taps=taps)
    x = int_acts((G * B,) + tuple(dims) + (cin,), g)
    c.w = int_weights(G, cout, cin, taps, g, nnz).view((G, cout, cin) + (k,) * nd)
    c.bias = int_bias(G, cout, g) if bias else None
    c.xs, c.xt = int_transform(G, cin, g) if xf else (None, None)
    c.y, c.dy, c.dx, c.dw = conv_reference(x, c.w, lambda s: int_acts(s, g), G, stride, pad, c.xs, c.xt, grads)
    c.out = tuple(c.y.shape[1:-1])
    c.cin_p = (cin + 63) // 64 * 64 if pad_cin else cin
    c.x = x if c.cin_p == cin else F.pad(x, (0, c.cin_p - cin))
    c.y_max = require_bf16_exact(c.y if c.bias is None else c.y + _bias_rows(c), name + " forward")
    require_bf16_exact(c.y, name + " forward without bias")
    if not grads:
        return c
    c.dx_max = require_bf16_exact(c.dx, name + " data gradient")
    npos = B
    for o in c.out:
        npos *= o
    xmax = 5.0 if xf else 2.0
    c.dw_bound = require_fp32_exact(npos * xmax * 2.0, name + " weight gradient")
    assert float(c.dw.abs().max()) <= c.dw_bound
    return c


def _bias_rows(c):
    return c.bias.double().repeat_interleave(c.B, 0).view((c.G * c.B,) + (1,) * len(c.out) + (c.cout,))


def y_with_bias(c):
    return c.y + _bias_rows(c)


@functools.lru_cache(maxsize=2)
def gemm_case(name, G, Mg, K, N):
    """Per-client GEMM lattice case: x [G, Mg, K] bf16, w [G, N, K] fp32 (y = x w^T, exact in bf16), dy [G, Mg, N]
    bf16 and dw = dy^T x [G, N, K] (exact in fp32); ysum / ysq: the per-channel sums of y and y^2 with their bounds."""
    g = gen(name, G, Mg, K, N)
    c = types.SimpleNamespace(name=name, G=G, Mg=Mg, K=K, N=N)
    c.x = int_acts((G, Mg, K), g)
    c.w = int_weights(G, N, K, 1, g).view(G, N, K)
    c.dy = int_acts((G, Mg, N), g)
    c.y = torch.bmm(c.x.double(), c.w.double().transpose(1, 2))
    c.dw = torch.bmm(c.dy.double().transpose(1, 2), c.x.double())
    require_bf16_exact(c.y, name + " output")
    require_fp32_exact(Mg * 4.0, name + " weight gradient")
    c.ysum, c.ysq = c.y.sum(1), (c.y * c.y).sum(1)
    # sum |y| and sum y^2 are the bounds of the two statistics sums (every term of the second is non-negative)
    c.stats_exact = float(c.y.abs().sum(1).max()) < FP32_EXACT and float(c.ysq.max()) < FP32_EXACT
    return c


# ------------------------------------------------------------------------------------------------ case lists
def conv3_cases():
    """(name, G, B, grads) of every 3x3x3 stride-1 case the GPU file builds, forward and backward."""
    out = [(n, G, B, False) for n in CONV3 for G, B in CONV3_GB[n]]
    out += [(n, G, B, True) for n in CONV3 for G, B in CONV3_BWD_GB]
    out += [(n,) + SLAB3_GB + (True,) for n in SLAB3]
    return out


def conv3(name, G, B, grads=True):
    if name in SLAB3:
        cin, cout, pad, sp = SLAB3[name]
        xf = False
    else:
        cin, cout, pad, sp, xf = CONV3[name]
    return conv_case(name, G, B, cin, cout, 3, 1, pad, sp, bias=True, xf=xf, grads=grads)


def gen3(name):
    cin, cout, k, stride, dims = GEN3[name] if name in GEN3 else GEN3_SPLITK[1]
    G, B = GEN_GB if name in GEN3 else (2, 2)
    return conv_case(name, G, B, cin, cout, k, stride, (k - 1) // 2, dims)


def gen2(name):
    cin, cout, k, stride, pad, hw = GEN2[name]
    return conv_case("2d_" + name, GEN_GB[0], GEN_GB[1], cin, cout, k, stride, pad, (hw, hw))


def slab2(B, hw, cin, cout):
    return conv_case("slab2d", SLAB2_G, B, cin, cout, 3, 1, 1, (hw, hw))


def c2(cin, cout, k, pad, H):
    return conv_case("c2", C2_GB[0], C2_GB[1], cin, cout, k, 1, pad, (H, H), bias=True, pad_cin=False)
