"""Lattice operands, fp64 references, per-element bounds and comparisons for the GroupNorm (gn.hip) and BatchNorm
(bnr.hip) kernels.

The apply and backward kernels take their statistics as an input tensor, so a test supplies dyadic ones: mean in
{-1, 0, 1}, rstd in {1/4, 1/2, 1}; activations, gradients and residuals are small integers, gamma is in {+-1, +-2} and
beta a small integer.  Every scale factor is then a power of two and every intermediate a short dyadic rational: fp32
arithmetic is exact in any summation order, with or without fma, and a correct kernel stores ``ref.to(bfloat16)`` (round
to nearest even) of the fp64 reference bit for bit.  This needs every divisor (S * cg of a GroupNorm group, M of a
BatchNorm) to be a power of two; the generators check the sums actually formed (``require_dyadic``) and the CPU test
evaluates every reference formula in fp32 and in fp64 and asserts they are equal.

Where a divisor is no power of two, or the kernel computes rsqrt(var + eps) itself, the result is not dyadic and the
comparison is a per-element a-priori bound (``assert_within``):

    |got - ref| <= halfulp_bf16(|ref| + E) + E,    E = K 2^-24 sum |terms| (+ propagated statistics error)

with K twice the number of fp32 roundings of the kernel's expression (counted next to each constant below) and the
terms those of the expression, so cancellation does not hide an error.  The bf16 store is round to nearest even of 8
significant bits: its error is at most half a bf16 ulp of the rounded value, 2^(floor(log2 |v|) - 8), which lies between
2^-9 |v| and 2^-8 |v|.  (A flat 2^-9 |ref| is below that half ulp for every value that is no power of two, so a
correctly rounded store would fail it; the half ulp itself is the tightest term that holds.)  A ReLU is 1-Lipschitz
and adds nothing.  Nothing here is tuned to what a kernel returns.

Plain helper module (no fixtures): tests/test_cpu_normlattice.py checks it without a GPU, tests/test_gpu_exact_norm.py
runs the kernels.  Both take their cases from the tables below.
"""
import functools
import types

import torch

from _lattice import FP32_EXACT, gen, require_fp32_exact

U32 = 2.0 ** -24                       # unit roundoff of fp32
GN_GROUPS = 32
GN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))   # the kernels' float constants, as doubles
BN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))
BN_MOM = float(torch.tensor(0.1, dtype=torch.float32))
BNR_CHUNK = 2048                       # positions per partial block (kBnrChunk)
FILL = 64.0                            # filler of the unused theta / grads / bufs columns: a wrong offset shows

# ------------------------------------------------------------------------------------------------ case tables
GN_G, GN_B = 3, 2
# (hw, C): NV1, NV2 with a ragged last row, NV2, NV4, NV8, NV16, and the two streaming shapes
GN_SHAPES = [(6, 64), (7, 128), (4, 512), (8, 256), (16, 128), (32, 64), (64, 64), (32, 128)]
# gn_apply: (hw, C, nb); nb * bp == S with bp a power of two.  4/128 has S C / 8 = 256 chunks, no multiple of 1024
GN_APPLY = [(4, 128, 4), (8, 256, 1), (16, 128, 4), (32, 64, 4), (32, 64, 1)]
GN_RANDOM = [(16, 128), (32, 128)]     # one register-resident and one streaming shape for the random-input cases

BN_G = 3
BN_C = (64, 256, 2048)


def gn_streaming(hw, C):
    return hw * hw * C > 65536


def gn_pow2(hw, C):
    n = hw * hw * (C // GN_GROUPS)
    return n & (n - 1) == 0


def bn_rows(C):
    return 256 // (C // 8)


def bn_stats_M(C):
    r = bn_rows(C)
    return [1, 4 * r - 1, 2048, 2049, 2 * 2048 + r + 1]


def bn_bwd_M(C):
    return [64, 2048, 4096, 2049, 2 * 2048 + bn_rows(C) + 1]


def bn_pow2(M):
    return M & (M - 1) == 0


BN_STRIDE = [(2048, 2049, 3), (64, 8300, 16)]      # (C, M, G) whose apply grids take a second grid-stride trip
BN_RES_M = (2048, 2049, 4099)


def bnr_grid_blocks(G, M, C):
    """bnr_grid's formula: blocks of 256 threads, one 8-channel chunk per thread and trip."""
    per = M * (C // 8)
    return max(1, min(4096 // max(1, G) + 1, (per + 255) // 256))


def nchunk(M):
    return (M + BNR_CHUNK - 1) // BNR_CHUNK


# ------------------------------------------------------------------------------------------------ generators
def ints(shape, lo, hi, g, dtype=torch.bfloat16):
    """Integers uniform in {lo..hi}."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(dtype)


def dyadic_stats(rows, g):
    """[*rows, 2] fp32: mean in {-1, 0, 1}, rstd in {1/4, 1/2, 1}."""
    mean = torch.randint(-1, 2, tuple(rows), generator=g).float()
    rstd = 2.0 ** -torch.randint(0, 3, tuple(rows), generator=g).float()
    return torch.stack([mean, rstd], -1).contiguous()


def theta_rows(G, C, g):
    """(theta [G, ldt] fp32, off_w, off_b): gamma in {+-1, +-2} and integer beta in [-2, 2] at non-zero offsets inside
    rows wider than 2 C; every other column holds FILL."""
    off_w, off_b = 24, 24 + C + 8
    theta = torch.full((G, off_b + C + 16), FILL)
    sign = torch.randint(0, 2, (G, C), generator=g) * 2 - 1
    theta[:, off_w:off_w + C] = (sign * torch.randint(1, 3, (G, C), generator=g)).float()
    theta[:, off_b:off_b + C] = torch.randint(-2, 3, (G, C), generator=g).float()
    return theta, off_w, off_b


def zero_sum_acts(N, S, C, g, amp=2):
    """Integer t [N, S, C] in [-amp, amp] whose sum over every (sample, group) is zero: half of a group's entries are
    drawn, the other half are their negatives in a shuffled order."""
    cg = C // GN_GROUPS
    n = S * cg
    if n % 2:
        raise ValueError("zero_sum_acts: odd group size %d" % n)
    h = torch.randint(-amp, amp + 1, (N, GN_GROUPS, n // 2), generator=g)
    v = torch.cat([h, -h], 2)
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(N * GN_GROUPS)]).view(N, GN_GROUPS, n)
    v = torch.gather(v, 2, perm)
    t = v.view(N, GN_GROUPS, S, cg).permute(0, 2, 1, 3).reshape(N, S, C)
    if int(t.view(N, S, GN_GROUPS, cg).sum((1, 3)).abs().max()) != 0:
        raise ValueError("zero_sum_acts: a group sum is not zero")
    return t.to(torch.bfloat16)


def require_dyadic(abs_bound, frac_bits, what):
    """A sum of multiples of 2^-frac_bits whose absolute terms add up to abs_bound is exact in fp32 in any order."""
    return require_fp32_exact(float(abs_bound) * 2.0 ** frac_bits, what)


# ------------------------------------------------------------------------------------------------ comparisons
def _at(i, shape, names, got, ref):
    idx = []
    for s in reversed(shape):
        idx.append(i % s)
        i //= s
    idx = tuple(reversed(idx))
    return "(%s): got %r, reference %r" % (", ".join("%s=%d" % (n, v) for n, v in zip(names, idx)),
                                           float(got[idx]), float(ref[idx]))


def _prep(got, ref, names):
    ref = ref.detach().double().cpu()
    assert len(names) == ref.dim(), (names, tuple(ref.shape))
    got = got.detach().double().cpu()
    assert got.numel() == ref.numel(), "shape: got %s, reference %s" % (tuple(got.shape), tuple(ref.shape))
    return got.reshape(ref.shape), ref


def assert_within(got, ref, bound, names):
    """Per element |got - ref| <= bound (a tensor of ref's shape, or broadcastable to it).  A failure reports the count
    and the first and the worst index (largest err / bound) by named axes; non-finite values fail.  Returns the
    largest err / bound."""
    got, ref = _prep(got, ref, names)
    bound = torch.as_tensor(bound, dtype=torch.float64).cpu().expand(ref.shape)
    assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), "assert_within: bad bound"
    err = (got - ref).abs()
    err[~torch.isfinite(got)] = float("inf")
    bad = ~(err <= bound)
    ratio = err / bound.clamp_min(1e-300)
    ratio[err == 0] = 0.0
    if not bool(bad.any()):
        return float(ratio.max()) if ratio.numel() else 0.0
    flat = bad.flatten()
    first = int(torch.nonzero(flat)[0])
    worst = int(ratio.flatten().argmax())
    raise AssertionError("%d of %d values outside their bound (%d non-finite, worst err / bound %.3g); first at %s; "
                         "worst at %s" % (int(flat.sum()), flat.numel(), int((~torch.isfinite(got)).sum()),
                                          float(ratio.flatten()[worst]), _at(first, ref.shape, names, got, ref),
                                          _at(worst, ref.shape, names, got, ref)))


def ulp32(x):
    """The spacing of fp32 at |x| (fp64 tensor)."""
    e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))[1] - 1          # floor(log2 |x|)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 23)


def assert_ulp(got, ref64, n, names):
    """fp32 ``got`` within n fp32 ulps (of the reference's binade) of the fp64 reference; reports like assert_within
    and returns the largest error in ulps."""
    return assert_within(got, ref64, n * ulp32(ref64.detach().double().cpu()), names) * n


def halfulp_bf16(v):
    """Half a bf16 ulp at magnitude |v|: the largest error of a round-to-nearest store of a value of that size."""
    e = torch.frexp(v.double().abs().clamp_min(2.0 ** -126))[1] - 1
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8)


def bf16_bound(ref, e32):
    """The bound of a bf16 store of an fp32 value that is within e32 of ref."""
    return halfulp_bf16(ref.abs() + e32) + e32


def relnorm(a, b):
    """The whole-tensor relative norm of the older normalisation tests."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-12))


# ------------------------------------------------------------------------------------------------ GroupNorm references
def _gn_rows(theta, off, C, B):
    """theta [G, ldt] -> the [G B, 1, C] rows at column off."""
    return theta[:, off:off + C].repeat_interleave(B, 0)[:, None, :]


def _gn_expand(s, cg):
    """per-group [N, 32] -> per-channel [N, 1, C]."""
    return s.repeat_interleave(cg, 1)[:, None, :]


# fp32 roundings of y = fma(t, sc, sh) (+ res): var division 1, + eps 1, rsqrtf 2 (1 ulp), sc = gamma rstd 1,
# mu sc 1, beta - mu sc 1, fma 1, + res 1  ->  9, K = 18
K_GN_FWD = 18


def gn_fwd_ref(t, res, gamma, beta, relu, dtype=torch.float64):
    """GroupNorm(32) over [N, S, C] channels-last samples with per-sample affine rows gamma / beta [N, 1, C], optional
    residual and ReLU.  Returns (y, pre, stats [N, 32, 2] = (mean, rstd), terms) with pre the ReLU input and terms
    |t gamma rstd| + |mu gamma rstd| + |beta| + |res| of every element."""
    N, S, C = t.shape
    cg = C // GN_GROUPS
    x = t.to(dtype)
    xg = x.view(N, S, GN_GROUPS, cg)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    rstd = 1.0 / torch.sqrt(var + GN_EPS)
    return (torch.stack([mean, rstd], -1),) + gn_affine_ref(x, res, mean, rstd, gamma, beta, relu)


def gn_affine_ref(x, res, mean, rstd, gamma, beta, relu):
    """(y, pre, terms) of the normalisation + affine (+ residual) (+ ReLU) given per-group mean / rstd [N, 32]."""
    cg = x.shape[2] // GN_GROUPS
    dtype = x.dtype
    mu, rs = _gn_expand(mean, cg), _gn_expand(rstd, cg)
    gam, bet = gamma.to(dtype), beta.to(dtype)
    pre = (x - mu) * rs * gam + bet
    terms = (x * gam * rs).abs() + (mu * gam * rs).abs() + bet.abs()
    if res is not None:
        pre = pre + res.to(dtype)
        terms = terms + res.to(dtype).abs()
    return (torch.relu(pre) if relu else pre), pre, terms


def gn_stats_error(t, n_terms):
    """Worst-case fp32 error of the two-pass statistics k_gn_fwd forms over the n_terms = S cg values of a group:
    (dmean, dvar) [N, 32] in fp64.  Sum of t: (n - 1) u sum |t|, one more rounding for the division.  Squared
    deviations d = fl(t - mean'): each d^2 carries 2 u (the subtraction) and the fma-accumulated sum (n - 1) u more, the
    division and the eps add one each; around the wrong mean the sum grows by n dmean^2."""
    N, S, C = t.shape
    cg = C // GN_GROUPS
    xg = t.double().view(N, S, GN_GROUPS, cg)
    mean = xg.mean((1, 3))
    dmean = (n_terms - 1) * U32 * xg.abs().sum((1, 3)) / n_terms + U32 * mean.abs()
    dev = (xg - mean[:, None, :, None]).abs() + dmean[:, None, :, None]
    var_hi = (dev ** 2).mean((1, 3))
    dvar = (n_terms + 3) * U32 * var_hi + dmean ** 2 + 2 * U32 * GN_EPS
    return dmean, dvar


def rstd_error(var, dvar, eps):
    """|d rstd| for |d var| <= dvar (rsqrt is monotone and convex: the low side is the larger) plus the 1-ulp rsqrtf."""
    lo = (var - dvar).clamp_min(0.0)
    rs = 1.0 / torch.sqrt(var + eps)
    return 1.0 / torch.sqrt(lo + eps) - rs + 2 * U32 * rs


# fp32 roundings of dt = rstd (dy gamma - m1 - xhat m2) on dyadic operands (dy gamma, xhat and the group sums are
# exact): the division of m1 or m2 1, xhat m2 1, two subtractions 2, the product with rstd 1  ->  5, K = 10
K_GN_BWD = 10
# with kernel-made (non-dyadic) statistics xhat = (t - mu) rstd rounds twice more and dy gamma once  ->  8, K = 16
K_GN_BWD_RANDOM = 16


def gn_bwd_ref(t, dy, mask, stats, gamma, dtype=torch.float64):
    """GroupNorm backward from the saved stats [N, 32, 2]: dy' = dy [mask], xhat = (t - mean) rstd,
    part [N, C, 2] = (sum_s dy', sum_s dy' xhat), m1 / m2 the group means of gamma part over S cg, and
    dt = rstd (dy' gamma - m1 - xhat m2).  gamma: [N, 1, C]; mask: bool or None.  Returns (dt, part, terms, aux) with
    terms = |rstd dy' gamma| + |rstd m1| + |rstd xhat m2| and aux the pieces the random-input bound needs."""
    N, S, C = t.shape
    cg = C // GN_GROUPS
    st = stats.to(dtype)
    mu, rs = _gn_expand(st[:, :, 0], cg), _gn_expand(st[:, :, 1], cg)
    gam = gamma.to(dtype)
    d = dy.to(dtype)
    if mask is not None:
        d = d * mask.to(dtype)
    xhat = (t.to(dtype) - mu) * rs
    pa, pb = d.sum(1), (d * xhat).sum(1)
    m1 = _gn_expand((gam[:, 0] * pa).view(N, GN_GROUPS, cg).sum(2) / (S * cg), cg)
    m2 = _gn_expand((gam[:, 0] * pb).view(N, GN_GROUPS, cg).sum(2) / (S * cg), cg)
    dt = rs * (d * gam - m1 - xhat * m2)
    terms = (rs * d * gam).abs() + (rs * m1).abs() + (rs * xhat * m2).abs()
    aux = types.SimpleNamespace(d=d, xhat=xhat, rs=rs, gam=gam, m1=m1, m2=m2, pa=pa, pb=pb)
    return dt, torch.stack([pa, pb], -1), terms, aux


def gn_bwd_sum_error(aux, S, cg):
    """Worst-case fp32 error of dt from the sums k_gn_bwd forms on non-lattice operands: (dpart [N, C, 2], ddt).  Per
    channel sum_s dy' carries (S - 1) u sum |dy'| and sum_s dy' xhat (S + 2) u sum |dy' xhat| (xhat rounds twice, the
    fma once per term); the gamma-weighted group sum adds cg u sum |gamma part| and the division u |m|."""
    N = aux.d.shape[0]
    dpa = (S - 1) * U32 * aux.d.abs().sum(1)
    dpb = (S + 2) * U32 * (aux.d * aux.xhat).abs().sum(1)
    g = aux.gam[:, 0].abs()

    def grp(dp, p, m):
        s = (g * dp).view(N, GN_GROUPS, cg).sum(2) + cg * U32 * (g * p.abs()).view(N, GN_GROUPS, cg).sum(2)
        return _gn_expand(s / (S * cg), cg) + U32 * m.abs()
    dm1, dm2 = grp(dpa, aux.pa, aux.m1), grp(dpb, aux.pb, aux.m2)
    return torch.stack([dpa, dpb], -1), aux.rs * (dm1 + aux.xhat.abs() * dm2)


def gn_param_grads_ref(part, G, B):
    """(dgamma, dbeta) [G, C] from the per-sample partials [G B, C, 2]."""
    p = part.view(G, B, part.shape[1], 2).sum(1)
    return p[..., 1], p[..., 0]


def gn_block_partials(t, nb):
    """The producing conv's epilogue statistics of t [N, S, C]: [N nb, C, 2] = (mean, M2) of each channel over each of
    the sample's nb blocks of S / nb positions, in fp64."""
    N, S, C = t.shape
    x = t.double().view(N, nb, S // nb, C)
    mean = x.mean(2)
    m2 = ((x - mean[:, :, None]) ** 2).sum(2)
    return torch.stack([mean, m2], -1).view(N * nb, C, 2)


# ------------------------------------------------------------------------------------------------ BatchNorm references
def bn_chunk_sums(a, b):
    """[nchunk, G, C, 2] sums of (a, b) [G, M, C] over chunks of BNR_CHUNK positions: the partial layout of bnr.hip."""
    out = []
    for p0 in range(0, a.shape[1], BNR_CHUNK):
        out.append(torch.stack([a[:, p0:p0 + BNR_CHUNK].sum(1), b[:, p0:p0 + BNR_CHUNK].sum(1)], -1))
    return torch.stack(out)


def bn_stats_ref(t, rm, rv, nbt, eps=BN_EPS, mom=BN_MOM):
    """Training statistics of t [G, M, C] (fp64): stats [G, C, 2] = (mean, rstd) with the biased variance, and the
    running mean / unbiased running variance / num_batches_tracked after one update (momentum mom); a single position
    (M == 1) has no unbiased variance and k_bnr_finalize keeps the biased one (0)."""
    x = t.double()
    M = x.shape[1]
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    unb = var * M / (M - 1) if M > 1 else var
    return (torch.stack([mean, rstd], -1), (1.0 - mom) * rm.double() + mom * mean,
            (1.0 - mom) * rv.double() + mom * unb, nbt.double() + 1.0)


def bn_stats_error(t):
    """Worst-case fp32 error of the one-pass sums k_bnr_partial forms over a chunk (sum t: (n - 1) u sum |t|; sum t^2 by
    fma: (n - 1) u sum t^2, n <= BNR_CHUNK; the chunks are combined in fp64), propagated to (dmean, dvar) [G, C]:
    var = q / M - mean^2."""
    x = t.double()
    M = x.shape[1]
    n = min(M, BNR_CHUNK)
    mean = x.mean(1)
    dmean = (n - 1) * U32 * x.abs().sum(1) / M
    dvar = (n - 1) * U32 * (x * x).sum(1) / M + 2 * mean.abs() * dmean + dmean ** 2
    return dmean, dvar


def _bn_rows(theta, off, C):
    return theta[:, off:off + C][:, None, :]


def bn_apply_ref(t, res, stats, gamma, beta, relu, dtype=torch.float64):
    """y = (t - mean) rstd gamma + beta (+ res) (ReLU); t [G, M, C], stats [G, C, 2], gamma / beta [G, 1, C]."""
    st = stats.to(dtype)
    y = (t.to(dtype) - st[:, None, :, 0]) * st[:, None, :, 1] * gamma.to(dtype) + beta.to(dtype)
    if res is not None:
        y = y + res.to(dtype)
    return torch.relu(y) if relu else y


# fp32 roundings of dt = fma(A, dy', fma(K2, t, K1)) on dyadic operands (A = rstd gamma and the products with it are
# powers-of-two scalings): the fp32 casts of m1 and m2 2, the subtraction in K1 1, the two fmas 2  ->  5, K = 10
K_BN_BWD = 10


def bn_bwd_ref(t, dy, mask, stats, gamma, eval_mode, dtype=torch.float64, terms=True):
    """BatchNorm backward: dy' = dy [mask], xhat = (t - mean) rstd, a = sum_M dy' (dbeta), b = sum_M dy' xhat (dgamma),
    coef = (a, b) / M, A = rstd gamma and dt = A (dy' - m1 - xhat m2) in train mode, A dy' in eval mode (the running
    statistics carry no gradient).  Returns (dt, dgamma, dbeta, coef [G, C, 2], part [nchunk, G, C, 2], terms) with
    terms = |A dy'| + |A m1| + |K2 mean| + |K2 t|, K2 = -A rstd m2 (None unless asked for: the bound's input).
    eval_mode "both": the pair (train, eval) of such tuples from one pass."""
    st = stats.to(dtype)
    mu, rs = st[:, None, :, 0], st[:, None, :, 1]
    x = t.to(dtype)
    M = x.shape[1]
    d = dy.to(dtype)
    if mask is not None:
        d = d * mask.to(dtype)
    xhat = (x - mu) * rs
    dx = d * xhat
    a, b = d.sum(1), dx.sum(1)
    coef = torch.stack([a, b], -1) / M
    part = bn_chunk_sums(d, dx)
    del dx
    A = rs * gamma.to(dtype)
    Ad = A * d
    out = []
    for ev in ((False, True) if eval_mode == "both" else (bool(eval_mode),)):
        if ev:
            out.append((Ad, b, a, coef, part, Ad.abs() if terms else None))
            continue
        m1, m2 = coef[:, None, :, 0], coef[:, None, :, 1]
        dt = Ad - A * (m1 + xhat * m2)
        tm = None
        if terms:
            K2 = A * rs * m2
            tm = Ad.abs() + (A * m1).abs() + (K2 * mu).abs() + (K2 * x).abs()
        out.append((dt, b, a, coef, part, tm))
    return tuple(out) if eval_mode == "both" else out[0]


def bn_res_ref(dx1, dx2, da, mask, omask, t3, s3, td, sd):
    """[RESBN]: out = (dx1 + (dx2 | da [mask > 0])) [omask > 0] with the backward partials of the two BatchNorms that
    consume it: (out, part3, partd) with part = chunk sums of (out, out xhat); partd is None without td."""
    second = dx2.double() if dx2 is not None else da.double() * ((mask.double() > 0) if mask is not None else 1.0)
    out = (dx1.double() + second) * (omask.double() > 0)

    def part(t, s):
        s = s.double()
        return bn_chunk_sums(out, out * (t.double() - s[:, None, :, 0]) * s[:, None, :, 1])
    return out, part(t3, s3), part(td, sd) if td is not None else None


# ------------------------------------------------------------------------------------------------ lattice cases
@functools.lru_cache(maxsize=2)
def gn_bwd_case(hw, C, G=GN_G, B=GN_B):
    """GroupNorm backward on the lattice: t in [-3, 3], dy in [-2, 2], a 0/1 mask, dyadic stats.  The references for
    mask {tensor, none} are c.ref[True / False] = (dt, part, terms); shared by the tests of a shape, not to be
    modified."""
    g = gen("gn_bwd", hw, C, G, B)
    N, S, cg = G * B, hw * hw, C // GN_GROUPS
    c = types.SimpleNamespace(hw=hw, C=C, G=G, B=B, N=N, S=S, cg=cg, pow2=gn_pow2(hw, C))
    c.t = ints((N, S, C), -3, 3, g)
    c.dy = ints((N, S, C), -2, 2, g)
    c.mask = ints((N, S, C), 0, 1, g)
    c.stats = dyadic_stats((N, GN_GROUPS), g)
    c.theta, c.off_w, c.off_b = theta_rows(G, C, g)
    c.gamma, c.beta = _gn_rows(c.theta, c.off_w, C, B), _gn_rows(c.theta, c.off_b, C, B)
    # the sums formed: per channel sum |dy| (integers) and sum |dy xhat| (multiples of 1/4, |xhat| <= 4); per group the
    # gamma-weighted sums of cg of them (|gamma| <= 2)
    require_dyadic(S * 2.0 * cg * 2.0, 0, "gn_bwd %d/%d: sum dy gamma" % (hw, C))
    require_dyadic(S * 2.0 * 4.0 * cg * 2.0, 2, "gn_bwd %d/%d: sum dy xhat gamma" % (hw, C))
    c.ref = {m: gn_bwd_ref(c.t, c.dy, c.mask if m else None, c.stats, c.gamma)[:3] for m in (True, False)}
    # the ReLU input of the forward that gn_bwd_rm recomputes: exact on the lattice, zero at some elements
    c.pre = gn_affine_ref(c.t.double(), None, c.stats[:, :, 0].double(), c.stats[:, :, 1].double(), c.gamma, c.beta,
                          False)[1]
    if not bool((c.pre == 0).any()):
        raise ValueError("gn_bwd %d/%d: no element with a ReLU input of exactly 0" % (hw, C))
    return c


def gn_bwd_bound(c, masked):
    dt, _, terms = c.ref[masked]
    return bf16_bound(dt, K_GN_BWD * U32 * terms)


@functools.lru_cache(maxsize=2)
def gn_fwd_case(hw, C, G=GN_G, B=GN_B):
    """GroupNorm forward on zero-sum integer t in [-2, 2] (mean 0 and sum t^2 exact), integer residual."""
    g = gen("gn_fwd", hw, C, G, B)
    N, S, cg = G * B, hw * hw, C // GN_GROUPS
    c = types.SimpleNamespace(hw=hw, C=C, G=G, B=B, N=N, S=S, cg=cg, pow2=gn_pow2(hw, C))
    c.t = zero_sum_acts(N, S, C, g)
    c.res = ints((N, S, C), -2, 2, g)
    c.theta, c.off_w, c.off_b = theta_rows(G, C, g)
    c.gamma, c.beta = _gn_rows(c.theta, c.off_w, C, B), _gn_rows(c.theta, c.off_b, C, B)
    require_dyadic(S * cg * 2.0, 0, "gn_fwd %d/%d: sum t" % (hw, C))
    require_dyadic(S * cg * 4.0, 0, "gn_fwd %d/%d: sum t^2" % (hw, C))
    c.ref = {}
    for res in (False, True):
        for relu in (False, True):
            st, y, pre, terms = gn_fwd_ref(c.t, c.res if res else None, c.gamma, c.beta, relu)
            c.ref[res, relu] = (y, bf16_bound(y, K_GN_FWD * U32 * terms))
    c.stats = st
    if float(st[:, :, 0].abs().max()) != 0:
        raise ValueError("gn_fwd %d/%d: a group mean is not zero" % (hw, C))
    return c


def gn_apply_part(c, nb):
    """The (mean, M2) block partials of a forward case as the fp32 tensor gn_apply reads; they must be exact in fp32,
    and so must the sums k_gn_apply forms from them (multiples of 1 / bp)."""
    p64 = gn_block_partials(c.t, nb)
    p = p64.float()
    if not torch.equal(p.double(), p64):
        raise ValueError("gn_apply %d/%d nb %d: a block partial is not an fp32 value" % (c.hw, c.C, nb))
    bp = c.S // nb
    if bp & (bp - 1):
        raise ValueError("gn_apply: bp %d is no power of two" % bp)
    fb = bp.bit_length() - 1
    mean, m2 = p64[..., 0].view(c.N, nb, GN_GROUPS, c.cg), p64[..., 1].view(c.N, nb, GN_GROUPS, c.cg)
    require_dyadic(mean.abs().sum((1, 3)).max(), fb, "gn_apply: sum of block means")
    require_dyadic((mean * mean).max(), 2 * fb, "gn_apply: squared block mean")
    require_dyadic((m2 + bp * mean * mean).sum((1, 3)).max(), fb, "gn_apply: M2 combine")
    return p


@functools.lru_cache(maxsize=2)
def gn_random_case(hw, C, G=GN_G, B=GN_B):
    """Random bf16 t with mean / std = 4, random gamma / beta / residual: the forward under the summation-error bound.
    c.ref[res, relu] = (y, pre, bound)."""
    g = gen("gn_random", hw, C, G, B)
    N, S, cg = G * B, hw * hw, C // GN_GROUPS
    c = types.SimpleNamespace(hw=hw, C=C, G=G, B=B, N=N, S=S, cg=cg)
    c.t = (torch.randn(N, S, C, generator=g) + 4.0).to(torch.bfloat16)
    c.res = torch.randn(N, S, C, generator=g).to(torch.bfloat16)
    c.dy = torch.randn(N, S, C, generator=g).to(torch.bfloat16)
    c.off_w, c.off_b = 24, 24 + C + 8
    c.theta = torch.full((G, c.off_b + C + 16), FILL)
    c.theta[:, c.off_w:c.off_w + C] = torch.randn(G, C, generator=g)
    c.theta[:, c.off_b:c.off_b + C] = torch.randn(G, C, generator=g)
    c.gamma, c.beta = _gn_rows(c.theta, c.off_w, C, B), _gn_rows(c.theta, c.off_b, C, B)
    dmean, dvar = gn_stats_error(c.t, S * cg)
    c.ref = {}
    for res, relu in ((False, False), (False, True), (True, False), (True, True)):
        st, y, pre, terms = gn_fwd_ref(c.t, c.res if res else None, c.gamma, c.beta, relu)
        drs = rstd_error(1.0 / st[:, :, 1] ** 2 - GN_EPS, dvar, GN_EPS)
        mu, dmu, rs, drs_c = (_gn_expand(v, cg) for v in (st[:, :, 0], dmean, st[:, :, 1], drs))
        gam = c.gamma.double().abs()
        e_stats = gam * ((c.t.double() - mu).abs() * drs_c + (rs + drs_c) * dmu)
        c.ref[res, relu] = (y, pre, bf16_bound(y, K_GN_FWD * U32 * terms + e_stats))
    c.stats, c.dmean, c.drstd = st, dmean, drs
    return c


@functools.lru_cache(maxsize=2)
def bn_case(C, M, G=BN_G):
    """BatchNorm lattice operands [G, M, C]: t in [-3, 3], dy / res in [-2, 2], a 0/1 mask, dyadic stats, lattice
    affine rows; the preconditions of the sums over M are asserted."""
    g = gen("bn", C, M, G)
    c = types.SimpleNamespace(C=C, M=M, G=G, rows=bn_rows(C), nchunk=nchunk(M), pow2=bn_pow2(M))
    c.t = ints((G, M, C), -3, 3, g)
    c.dy = ints((G, M, C), -2, 2, g)
    c.res = ints((G, M, C), -2, 2, g)
    c.mask = ints((G, M, C), 0, 1, g)
    c.stats = dyadic_stats((G, C), g)
    c.theta, c.off_w, c.off_b = theta_rows(G, C, g)
    c.gamma, c.beta = _bn_rows(c.theta, c.off_w, C), _bn_rows(c.theta, c.off_b, C)
    require_dyadic(M * 3.0, 0, "bn C %d M %d: sum t" % (C, M))
    require_dyadic(M * 9.0, 0, "bn C %d M %d: sum t^2" % (C, M))
    require_dyadic(M * 2.0, 0, "bn C %d M %d: sum dy" % (C, M))
    require_dyadic(M * 2.0 * 4.0, 2, "bn C %d M %d: sum dy xhat" % (C, M))
    return c


def bn_bwd_bound(dt, terms):
    return bf16_bound(dt, K_BN_BWD * U32 * terms)


def bn_tmask(c):
    """The ReLU mask bnr_bwd_tm recomputes: bf16(relu(fma(t, sc, sf))) > 0.  On the lattice the ReLU input is exact and
    a positive one is at least 1/4, so the bf16 store cannot round it to zero."""
    pre = bn_apply_ref(c.t, None, c.stats, c.gamma, c.beta, False)
    return (pre.to(torch.bfloat16).double() > 0), pre


@functools.lru_cache(maxsize=2)
def bn_res_case(C, M, G=BN_G):
    """[RESBN] lattice operands: dx1 / dx2 / da in [-2, 2], 0/1 masks, t3 / td in [-3, 3] with dyadic stats."""
    g = gen("bn_res", C, M, G)
    c = types.SimpleNamespace(C=C, M=M, G=G, nchunk=nchunk(M))
    for n in ("dx1", "dx2", "da"):
        setattr(c, n, ints((G, M, C), -2, 2, g))
    c.mask, c.omask = ints((G, M, C), 0, 1, g), ints((G, M, C), 0, 1, g)
    c.t3, c.td = ints((G, M, C), -3, 3, g), ints((G, M, C), -3, 3, g)
    c.s3, c.sd = dyadic_stats((G, C), g), dyadic_stats((G, C), g)
    c.theta, c.off_w, c.off_b = theta_rows(G, C, g)
    c.gamma = _bn_rows(c.theta, c.off_w, C)
    require_dyadic(min(M, BNR_CHUNK) * 4.0, 0, "bn_res: sum out")
    require_dyadic(min(M, BNR_CHUNK) * 4.0 * 4.0, 2, "bn_res: sum out xhat")
    return c


def bn_random_t(C, M, G=BN_G):
    """Random bf16 t with mean / std = 16: the one-pass sum of squares at its worst."""
    g = gen("bn_random", C, M, G)
    return (torch.randn(G, M, C, generator=g) + 16.0).to(torch.bfloat16)


assert FP32_EXACT == 1 << 24
