"""Per-element and bit-exact tests of the GroupNorm (gn.hip) and BatchNorm (bnr.hip) kernels against the fp64 references
of tests/_normlattice.py.  With dyadic statistics supplied by the test and integer operands every intermediate of the
apply and backward kernels is a short dyadic rational, so a correct kernel stores ``ref.to(bfloat16)`` bit for bit
(power-of-two divisors); where a divisor is no power of two, or the kernel computes rsqrt(var + eps) itself, each
element is held to an a-priori bound (half a bf16 ulp plus the counted fp32 roundings, _normlattice.py).  One unwritten,
doubled or misplaced 16-byte chunk fails with its coordinates; the relative-norm tests of the same kernels
(test_gpu_resnet2d.py, test_gpu_resnet3d.py) stay as they are.

The raw bindings are called, so the kernel under test is the one named.  Output buffers start as NaN and carry one
guard row after the last sample / client that must stay untouched; gradient and buffer rows sit between filler columns.

Largest measured err / bound per kernel family on an MI355X (every ratio above 1 is a failure; each test prints its
own).  Where the result is stored in bf16 the ratio sits just below 1 by construction: among 10^5 to 10^7 elements some
land on (lattice: exactly on) a rounding tie, where a correct store is off by the full half ulp of the bound.
    gn_fwd 0.9992, gn_apply 0.9992 (and bit-identical to gn_fwd on the same t), gn_bwd 0.9998, gn_bwd_rm 0.9998
    gn_fwd random inputs: y 0.9987, saved mean 0.0010, saved rstd 0.0033; gn_bwd on them: dt 0.9988, partials 0.0060
    bnr_bwd 0.9996, bnr_bwd_tm 0.9994, bnr_bwd_part 0.9996
    bnr_stats / bnr_finalize_part (1 ulp) 0.50 ulp, bnr_eval_stats (2 ulp) 0.91 ulp
    bnr_stats random inputs (mean / std = 16, M = 2049): mean 0.0005, rstd 0.0005 (|rstd error| 2.3e-5, bound 5.9e-2)
"""
import types

import pytest
import torch

import _lattice as L
import _normlattice as NL

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENT = -96.0
AXG = ("client", "sample", "position", "channel")
AXB = ("client", "position", "channel")


def _m():
    from neuroimagedisttraining_amd import ops
    return ops.ext()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _d(x):
    return None if x is None else x.contiguous().to(DEV)


def _p(x):
    return 0 if x is None else x.data_ptr()


def _out(n, *shape, dtype=torch.bfloat16):
    """[n + 1, *shape]: n NaN rows for the kernel and one guard row."""
    buf = torch.full((n + 1,) + shape, NAN, device=DEV, dtype=dtype)
    buf[n] = SENT
    return buf


def _guard_ok(*bufs):
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[-1] == SENT).all()), "the guard row after the last sample was written"


def _rec(family, ratio):
    print("normlattice err/bound %s %.4f" % (family, ratio))
    assert ratio <= 1.0


def _exact_bf16(got, ref64, shape, names, family):
    """got equals the bf16 rounding (nearest even) of the fp64 reference bit for bit."""
    print("normlattice exact %s" % family)
    exp = ref64.to(torch.bfloat16)
    if torch.equal(got.cpu().view(exp.shape), exp):
        return
    L.assert_exact(got, exp.double().view(shape), names)


def _rows_ok(rows, spans, what):
    """Every column of rows [G, ld] outside the (offset, length) spans still holds the filler."""
    keep = torch.ones(rows.shape[1], dtype=torch.bool)
    for off, n in spans:
        keep[off:off + n] = False
    assert bool((rows.cpu()[:, keep] == NL.FILL).all()), what + ": a neighbouring column changed"


# ================================================================================================ GroupNorm
def _gn_bwd_run(c, dy_bf16, mask, rm=False):
    m = _m()
    dy = _d(c.dy if dy_bf16 else c.dy.float())
    t, stats, theta, mk = _d(c.t), _d(c.stats), _d(c.theta), _d(mask)
    dt, part = _out(c.N, c.S, c.C), _out(c.N, c.C, 2, dtype=torch.float32)
    if rm:
        m.gn_bwd_rm(dy.data_ptr(), int(dy_bf16), t.data_ptr(), stats.data_ptr(), theta.data_ptr(), theta.stride(0),
                    c.off_w, c.off_b, dt.data_ptr(), part.data_ptr(), c.N, c.B, c.S, c.C, _st())
    else:
        m.gn_bwd(dy.data_ptr(), int(dy_bf16), _p(mk), t.data_ptr(), stats.data_ptr(), theta.data_ptr(),
                 theta.stride(0), c.off_w, dt.data_ptr(), part.data_ptr(), c.N, c.B, c.S, c.C, _st())
    _guard_ok(dt, part)
    return dt, part


def _gn_bwd_check(c, dt, part, ref, family):
    dt_ref, part_ref, terms = ref
    shape = (c.G, c.B, c.S, c.C)
    L.assert_exact(part[:c.N], part_ref.view(c.G, c.B, c.C, 2), ("client", "sample", "channel", "sum"))
    if c.pow2:
        _exact_bf16(dt[:c.N], dt_ref, shape, AXG, family)
    else:
        bound = NL.bf16_bound(dt_ref, NL.K_GN_BWD * NL.U32 * terms)
        _rec(family, NL.assert_within(dt[:c.N], dt_ref.view(shape), bound.view(shape), AXG))


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("dy_bf16", [True, False])
@pytest.mark.parametrize("hw,C", NL.GN_SHAPES)
def test_gn_bwd_lattice(hw, C, dy_bf16, masked):
    """gn_bwd with dyadic statistics: bf16 dy (the HOLD kernels) and fp32 dy, with and without a mask tensor, at every
    kernel instantiation; then gn_param_grads on the exact partials, between filler columns."""
    m = _m()
    c = NL.gn_bwd_case(hw, C)
    dt, part = _gn_bwd_run(c, dy_bf16, c.mask if masked else None)
    _gn_bwd_check(c, dt, part, c.ref[masked], "gn_bwd")
    grads = torch.full_like(c.theta, NL.FILL).to(DEV)
    m.gn_param_grads(part.data_ptr(), c.G, c.B, C, grads.data_ptr(), grads.stride(0), c.off_w, c.off_b, _st())
    torch.cuda.synchronize()
    dg, db = NL.gn_param_grads_ref(c.ref[masked][1], c.G, c.B)
    L.assert_exact(grads[:, c.off_w:c.off_w + C], dg, ("client", "channel"))
    L.assert_exact(grads[:, c.off_b:c.off_b + C], db, ("client", "channel"))
    _rows_ok(grads, [(c.off_w, C), (c.off_b, C)], "gn_param_grads")


@pytest.mark.parametrize("dy_bf16", [True, False])
@pytest.mark.parametrize("hw,C", [s for s in NL.GN_SHAPES if not NL.gn_streaming(*s)])
def test_gn_bwd_rm_lattice(hw, C, dy_bf16):
    """gn_bwd_rm == gn_bwd given the mask fma(t, sc, sh) > 0; the ReLU input is exact on the lattice (and exactly 0 at
    some elements, which are masked out)."""
    assert _m().gn_rm_ok(hw * hw, C) == 1
    c = NL.gn_bwd_case(hw, C)
    live = c.pre > 0
    ref = NL.gn_bwd_ref(c.t, c.dy, live, c.stats, c.gamma)[:3]
    dt, part = _gn_bwd_run(c, dy_bf16, None, rm=True)
    _gn_bwd_check(c, dt, part, ref, "gn_bwd_rm")
    dt2, part2 = _gn_bwd_run(c, dy_bf16, live.to(torch.bfloat16))
    assert torch.equal(dt[:c.N].view(torch.int16), dt2[:c.N].view(torch.int16)) and torch.equal(part, part2)


def test_gn_rm_ok_rejects_streaming_shapes():
    for hw, C in NL.GN_SHAPES:
        assert _m().gn_rm_ok(hw * hw, C) == (0 if NL.gn_streaming(hw, C) else 1)


def _gn_stats_check(c, stats):
    ref = c.stats.view(c.G, c.B, NL.GN_GROUPS, 2)
    got = stats[:c.N].cpu().view(ref.shape)
    assert bool((got[..., 0] == 0).all()), "a saved mean is not exactly 0"
    return NL.assert_ulp(got[..., 1], ref[..., 1], 2, ("client", "sample", "group"))


def _gn_fwd_run(c, res, relu):
    m = _m()
    t, r, theta = _d(c.t), _d(c.res if res else None), _d(c.theta)
    y, stats = _out(c.N, c.S, c.C), _out(c.N, NL.GN_GROUPS, 2, dtype=torch.float32)
    m.gn_fwd(t.data_ptr(), _p(r), theta.data_ptr(), theta.stride(0), c.off_w, c.off_b, y.data_ptr(),
             stats.data_ptr(), c.N, c.B, c.S, c.C, int(relu), _st())
    _guard_ok(y, stats)
    return y, stats


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("hw,C", NL.GN_SHAPES)
def test_gn_fwd_lattice(hw, C, res, relu):
    """gn_fwd on zero-sum integer t: the saved mean is exactly 0, rstd within 2 ulp, y within its bound per element."""
    c = NL.gn_fwd_case(hw, C)
    y, stats = _gn_fwd_run(c, res, relu)
    _gn_stats_check(c, stats)
    ref, bound = c.ref[res, relu]
    shape = (c.G, c.B, c.S, C)
    _rec("gn_fwd", NL.assert_within(y[:c.N], ref.view(shape), bound.view(shape), AXG))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("hw,C,nb", NL.GN_APPLY)
def test_gn_apply_lattice(hw, C, nb, res, relu):
    """gn_apply from exact per-block (mean, M2) partials of lattice t: saved stats and y as gn_fwd, and against
    gn_fwd's own output on the same t."""
    m = _m()
    c = NL.gn_fwd_case(hw, C)
    part = _d(NL.gn_apply_part(c, nb))
    t, r, theta = _d(c.t), _d(c.res if res else None), _d(c.theta)
    y, stats = _out(c.N, c.S, C), _out(c.N, NL.GN_GROUPS, 2, dtype=torch.float32)
    m.gn_apply(t.data_ptr(), _p(r), part.data_ptr(), nb, c.S // nb, theta.data_ptr(), theta.stride(0), c.off_w,
               c.off_b, y.data_ptr(), stats.data_ptr(), c.N, c.B, c.S, C, int(relu), _st())
    _guard_ok(y, stats)
    _gn_stats_check(c, stats)
    ref, bound = c.ref[res, relu]
    shape = (c.G, c.B, c.S, C)
    _rec("gn_apply", NL.assert_within(y[:c.N], ref.view(shape), bound.view(shape), AXG))
    y2, _ = _gn_fwd_run(c, res, relu)
    _rec("gn_apply_vs_gn_fwd", NL.assert_within(y[:c.N], y2[:c.N].double().view(shape), bound.view(shape), AXG))


@pytest.mark.parametrize("hw,C", NL.GN_RANDOM)
def test_gn_random_inputs_and_mask_consistency(hw, C):
    """Random t with mean / std = 4 (one register-resident, one streaming shape): stats and y under the worst-case
    summation bound; the ReLU mask of the stored y differs from the reference's only where the ReLU input is within
    its bound of 0; and the backward given that y as its mask, against the reference with the same mask."""
    m = _m()
    c = NL.gn_random_case(hw, C)
    shape = (c.G, c.B, c.S, C)
    for res, relu in ((True, False), (False, True)):
        y, stats = _gn_fwd_run(c, res, relu)
        ref, pre, bound = c.ref[res, relu]
        _rec("gn_fwd_random", NL.assert_within(y[:c.N], ref.view(shape), bound.view(shape), AXG))
    sref = c.stats.view(c.G, c.B, NL.GN_GROUPS, 2)
    got = stats[:c.N].cpu().view(sref.shape)
    ax = ("client", "sample", "group")
    _rec("gn_fwd_random_mean", NL.assert_within(got[..., 0], sref[..., 0],
                                                 c.dmean.view(sref.shape[:3]) + NL.ulp32(sref[..., 0]), ax))
    _rec("gn_fwd_random_rstd", NL.assert_within(got[..., 1], sref[..., 1], c.drstd.view(sref.shape[:3]), ax))
    # (res False, relu True) is the last forward: y is the mask tensor of the backward
    live = y[:c.N].cpu().double() > 0
    differ = live != (pre > 0)
    assert bool((pre.abs()[differ] <= bound[differ]).all()), "a ReLU decision differs away from 0"
    dy, t, theta = _d(c.dy), _d(c.t), _d(c.theta)
    dt, part = _out(c.N, c.S, C), _out(c.N, C, 2, dtype=torch.float32)
    m.gn_bwd(dy.data_ptr(), 1, y.data_ptr(), t.data_ptr(), stats.data_ptr(), theta.data_ptr(), theta.stride(0),
             c.off_w, dt.data_ptr(), part.data_ptr(), c.N, c.B, c.S, C, _st())
    _guard_ok(dt, part)
    dt_ref, part_ref, terms, aux = NL.gn_bwd_ref(c.t, c.dy, live, stats[:c.N].cpu(), c.gamma)
    dpart, ddt = NL.gn_bwd_sum_error(aux, c.S, c.cg)
    _rec("gn_bwd_random_part", NL.assert_within(part[:c.N], part_ref.view(c.G, c.B, C, 2),
                                                 (dpart + 2 * NL.U32 * part_ref.abs()).view(c.G, c.B, C, 2),
                                                 ("client", "sample", "channel", "sum")))
    bound = NL.bf16_bound(dt_ref, NL.K_GN_BWD_RANDOM * NL.U32 * terms + ddt)
    _rec("gn_bwd_random", NL.assert_within(dt[:c.N], dt_ref.view(shape), bound.view(shape), AXG))


# ================================================================================================ BatchNorm
def _bufs(G, C, seed):
    """(bufs [G, ldb] fp32 on the CPU, off_rm, off_rv, off_nbt): random running rows and a step count of 5 between
    filler columns."""
    g = L.gen("bufs", G, C, seed)
    off_rm, off_rv = 8, 8 + C + 8
    off_nbt = off_rv + C + 4
    bufs = torch.full((G, off_nbt + 5), NL.FILL)
    bufs[:, off_rm:off_rm + C] = torch.randn(G, C, generator=g)
    bufs[:, off_rv:off_rv + C] = torch.rand(G, C, generator=g) + 0.5
    bufs[:, off_nbt] = 5.0
    return bufs, off_rm, off_rv, off_nbt


def _bn_stats_check(t, bufs0, offs, stats, bufs, family):
    G, M, C = t.shape
    off_rm, off_rv, off_nbt = offs
    sref, rm, rv, nbt = NL.bn_stats_ref(t, bufs0[:, off_rm:off_rm + C], bufs0[:, off_rv:off_rv + C], bufs0[:, off_nbt])
    ax = ("client", "channel")
    r = [NL.assert_ulp(stats[:G], sref, 1, ax + ("stat",)),
         NL.assert_ulp(bufs[:, off_rm:off_rm + C], rm, 1, ax), NL.assert_ulp(bufs[:, off_rv:off_rv + C], rv, 1, ax)]
    L.assert_exact(bufs[:, off_nbt], nbt, ("client",))
    _rows_ok(bufs, [(off_rm, C), (off_rv, C), (off_nbt, 1)], family)
    _rec(family + "_ulp", max(r))


def _bn_stats_params():
    return [(C, M) for C in NL.BN_C for M in NL.bn_stats_M(C)]


@pytest.mark.parametrize("C,M", _bn_stats_params())
def test_bnr_stats_lattice(C, M):
    """bnr_stats on integer t: the chunk partials are exact in their [nchunk][G][C][2] layout; stats, the running rows
    (momentum 0.1, unbiased variance, the M == 1 rule) and num_batches_tracked within 1 ulp of the fp64 formulas."""
    m = _m()
    c = NL.bn_case(C, M)
    G = c.G
    assert m.bnr_workspace(G, M, C) == c.nchunk * G * C * 2
    bufs0, off_rm, off_rv, off_nbt = _bufs(G, C, M)
    t, bufs = _d(c.t), _d(bufs0)
    ws, stats = _out(c.nchunk, G, C, 2, dtype=torch.float32), _out(G, C, 2, dtype=torch.float32)
    m.bnr_stats(t.data_ptr(), G, M, C, NL.BN_EPS, NL.BN_MOM, ws.data_ptr(), stats.data_ptr(), bufs.data_ptr(),
                bufs.stride(0), off_rm, off_rv, off_nbt, _st())
    _guard_ok(ws, stats)
    x = c.t.double()
    L.assert_exact(ws[:c.nchunk], NL.bn_chunk_sums(x, x * x), ("chunk", "client", "channel", "sum"))
    _bn_stats_check(c.t, bufs0, (off_rm, off_rv, off_nbt), stats, bufs, "bnr_stats")


def test_bnr_stats_random_inputs():
    """Random t with mean / std = 16 at M = 2049: the one-pass sum of squares in fp32 under its worst-case bound."""
    m = _m()
    C, M, G = 256, 2049, NL.BN_G
    tc = NL.bn_random_t(C, M)
    t = _d(tc)
    ws, stats = _out(NL.nchunk(M), G, C, 2, dtype=torch.float32), _out(G, C, 2, dtype=torch.float32)
    m.bnr_stats(t.data_ptr(), G, M, C, NL.BN_EPS, NL.BN_MOM, ws.data_ptr(), stats.data_ptr(), 0, 0, 0, 0, -1, _st())
    _guard_ok(ws, stats)
    sref = NL.bn_stats_ref(tc, torch.zeros(G, C), torch.ones(G, C), torch.zeros(G))[0]
    dmean, dvar = NL.bn_stats_error(tc)
    var = 1.0 / sref[..., 1] ** 2 - NL.BN_EPS
    assert float((dvar / var).max()) < 0.5
    ax = ("client", "channel")
    _rec("bnr_stats_random_mean", NL.assert_within(stats[:G, :, 0], sref[..., 0], dmean + NL.ulp32(sref[..., 0]), ax))
    drs = NL.rstd_error(var, dvar, NL.BN_EPS)
    _rec("bnr_stats_random_rstd", NL.assert_within(stats[:G, :, 1], sref[..., 1], drs, ax))
    print("bnr_stats random: largest |rstd error| %.3g (bound %.3g)"
          % (float((stats[:G, :, 1].cpu().double() - sref[..., 1]).abs().max()), float(drs.max())))


def test_bnr_finalize_part_matches_bnr_stats():
    """bnr_finalize_part from test-built partials of three uneven position ranges == bnr_stats on the same t."""
    m = _m()
    C, M = 256, 2049
    c = NL.bn_case(C, M)
    G = c.G
    x = c.t.double()
    cuts = [0, 700, 1500, M]
    part = torch.stack([torch.stack([x[:, a:b].sum(1), (x[:, a:b] ** 2).sum(1)], -1) for a, b in zip(cuts, cuts[1:])])
    bufs0, off_rm, off_rv, off_nbt = _bufs(G, C, M)
    outs = []
    for from_part in (True, False):
        bufs, stats = _d(bufs0), _out(G, C, 2, dtype=torch.float32)
        if from_part:
            p = _d(part.float())
            m.bnr_finalize_part(p.data_ptr(), 3, G, M, C, NL.BN_EPS, NL.BN_MOM, stats.data_ptr(), bufs.data_ptr(),
                                bufs.stride(0), off_rm, off_rv, off_nbt, _st())
        else:
            t, ws = _d(c.t), _out(c.nchunk, G, C, 2, dtype=torch.float32)
            m.bnr_stats(t.data_ptr(), G, M, C, NL.BN_EPS, NL.BN_MOM, ws.data_ptr(), stats.data_ptr(),
                        bufs.data_ptr(), bufs.stride(0), off_rm, off_rv, off_nbt, _st())
        _guard_ok(stats)
        _bn_stats_check(c.t, bufs0, (off_rm, off_rv, off_nbt), stats, bufs, "bnr_finalize_part")
        outs.append((stats, bufs))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("C", NL.BN_C)
def test_bnr_eval_stats(C):
    """bnr_eval_stats: the running mean copied exactly, rstd = rsqrtf(running var + eps) within 2 ulp."""
    m = _m()
    G = NL.BN_G
    bufs0, off_rm, off_rv, _ = _bufs(G, C, 0)
    bufs, stats = _d(bufs0), _out(G, C, 2, dtype=torch.float32)
    m.bnr_eval_stats(G, C, NL.BN_EPS, bufs.data_ptr(), bufs.stride(0), off_rm, off_rv, stats.data_ptr(), _st())
    _guard_ok(stats)
    assert torch.equal(bufs.cpu(), bufs0)
    L.assert_exact(stats[:G, :, 0], bufs0[:, off_rm:off_rm + C], ("client", "channel"))
    ref = 1.0 / torch.sqrt(bufs0[:, off_rv:off_rv + C].double() + NL.BN_EPS)
    _rec("bnr_eval_stats_2ulp", NL.assert_ulp(stats[:G, :, 1], ref, 2, ("client", "channel")) / 2)


def _bn_apply_params():
    out = [(C, M, NL.BN_G) for C, M in _bn_stats_params()]
    return out + [s for s in NL.BN_STRIDE if s not in out]


@pytest.mark.parametrize("C,M,G", _bn_apply_params())
def test_bnr_apply_lattice(C, M, G):
    """bnr_apply with dyadic statistics, residual {no, yes} x ReLU {no, yes}, bit-exact; the last two shapes exceed the
    grid cap, so every thread takes a second grid-stride trip with its channel chunk unchanged."""
    m = _m()
    if (C, M, G) in NL.BN_STRIDE:
        assert M * C // 8 > (4096 // G + 1) * 256
        assert NL.bnr_grid_blocks(G, M, C) == 4096 // G + 1
    c = NL.bn_case(C, M, G)
    t, r, stats, theta = _d(c.t), _d(c.res), _d(c.stats), _d(c.theta)
    for res in (False, True):
        for relu in (False, True):
            y = _out(G, M, C)
            m.bnr_apply(t.data_ptr(), r.data_ptr() if res else 0, stats.data_ptr(), theta.data_ptr(), theta.stride(0),
                        c.off_w, c.off_b, y.data_ptr(), G, M, C, int(relu), _st())
            _guard_ok(y)
            ref = NL.bn_apply_ref(c.t, c.res if res else None, c.stats, c.gamma, c.beta, relu)
            _exact_bf16(y[:G], ref, (G, M, C), AXB, "bnr_apply")


def _bn_bwd_run(c, dy_bf16, mask, eval_mode, tmask=None, t=None, dy=None, part=None):
    """bnr_bwd / bnr_bwd_tm (tmask given) / bnr_bwd_part (part given); returns (dt, grads, coef, ws)."""
    m = _m()
    G, M, C = c.G, c.M, c.C
    t = _d(c.t if t is None else t)
    dy = _d(c.dy if dy is None else dy)
    dy = dy if dy_bf16 else dy.float()
    mk, stats, theta = _d(mask), _d(c.stats), _d(c.theta)
    grads = torch.full_like(c.theta, NL.FILL).to(DEV)
    coef, dt = _out(G, C, 2, dtype=torch.float32), _out(G, M, C)
    ws = _out(c.nchunk, G, C, 2, dtype=torch.float32) if part is None else part
    args = (stats.data_ptr(), theta.data_ptr(), theta.stride(0), c.off_w, c.off_b, grads.data_ptr(), grads.stride(0),
            ws.data_ptr(), coef.data_ptr(), dt.data_ptr(), G, M, C)
    if part is not None:
        m.bnr_bwd_part(t.data_ptr(), dy.data_ptr(), *args, _st())
    elif tmask is not None:
        m.bnr_bwd_tm(t.data_ptr(), dy.data_ptr(), int(dy_bf16), _p(mk), *args, int(eval_mode), int(tmask), _st())
    else:
        m.bnr_bwd(t.data_ptr(), dy.data_ptr(), int(dy_bf16), _p(mk), *args, int(eval_mode), _st())
    _guard_ok(coef, dt, ws)
    return dt, grads, coef, ws


def _bn_bwd_check(c, out, ref, exact, family):
    dt, grads, coef, ws = out
    dt_ref, dg, db, coef_ref, part_ref, terms = ref
    G, M, C = c.G, c.M, c.C
    L.assert_exact(ws[:c.nchunk], part_ref, ("chunk", "client", "channel", "sum"))
    L.assert_exact(grads[:, c.off_w:c.off_w + C], dg, ("client", "channel"))
    L.assert_exact(grads[:, c.off_b:c.off_b + C], db, ("client", "channel"))
    _rows_ok(grads, [(c.off_w, C), (c.off_b, C)], family)
    NL.assert_ulp(coef[:G], coef_ref, 1, ("client", "channel", "coef"))
    if exact:
        _exact_bf16(dt[:G], dt_ref, (G, M, C), AXB, family)
    else:
        _rec(family, NL.assert_within(dt[:G], dt_ref, NL.bn_bwd_bound(dt_ref, terms), AXB))


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("C,M", [(C, M) for C in NL.BN_C for M in NL.bn_bwd_M(C)])
def test_bnr_bwd_lattice(C, M, masked):
    """bnr_bwd over dy {bf16, fp32} x mask {tensor, none} x eval_mode {0, 1}: the chunk partials, the dgamma / dbeta
    rows (between filler columns) and eval-mode dt are bit-exact at every M, coef within 1 ulp, train-mode dt bit-exact
    where M is a power of two and within its bound elsewhere."""
    c = NL.bn_case(C, M)
    refs = NL.bn_bwd_ref(c.t, c.dy, c.mask if masked else None, c.stats, c.gamma, "both", terms=not c.pow2)
    for eval_mode in (0, 1):
        for dy_bf16 in (True, False):
            out = _bn_bwd_run(c, dy_bf16, c.mask if masked else None, eval_mode)
            _bn_bwd_check(c, out, refs[eval_mode], eval_mode or c.pow2, "bnr_bwd")


@pytest.mark.parametrize("C,M", [(C, M) for C in NL.BN_C for M in (64, 2049)])
def test_bnr_bwd_tm_lattice(C, M):
    """bnr_bwd_tm(tmask=1) == bnr_bwd given the mask bf16(relu(fma(t, sc, sf))) > 0, train and eval mode."""
    c = NL.bn_case(C, M)
    live, pre = NL.bn_tmask(c)
    assert bool((pre == 0).any()) and bool(live.any())
    for eval_mode in (0, 1):
        ref = NL.bn_bwd_ref(c.t, c.dy, live, c.stats, c.gamma, eval_mode)
        out = _bn_bwd_run(c, True, None, eval_mode, tmask=1)
        _bn_bwd_check(c, out, ref, eval_mode or c.pow2, "bnr_bwd_tm")
        out2 = _bn_bwd_run(c, True, live.to(torch.bfloat16), eval_mode)
        for a, b in zip(out, out2):
            assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16)
                               if b.dtype == torch.bfloat16 else b)


@pytest.mark.parametrize("second", ["dx2", "da_mask"])
@pytest.mark.parametrize("has_d", [False, True])
@pytest.mark.parametrize("C,M", [(256, M) for M in NL.BN_RES_M] + [(64, 2049), (2048, 2049)])
def test_bnr_res_partial_and_bwd_part_lattice(C, M, has_d, second):
    """bnr_res_partial: out and both partial tensors bit-exact, with and without the downsample operand, dx2 versus
    da + mask; bnr_bwd_part fed from its bn3 partials == the backward of bn3 on the reference out."""
    m = _m()
    c = NL.bn_res_case(C, M)
    G = c.G
    dx2 = c.dx2 if second == "dx2" else None
    da, mask = (None, None) if second == "dx2" else (c.da, c.mask)
    td, sd = (c.td, c.sd) if has_d else (None, None)
    out_ref, p3_ref, pd_ref = NL.bn_res_ref(c.dx1, dx2, da, mask, c.omask, c.t3, c.s3, td, sd)
    ops = [_d(v) for v in (c.dx1, dx2, da, mask, c.omask, c.t3, c.s3, td, sd)]
    out = _out(G, M, C)
    ws3, wsd = (_out(c.nchunk, G, C, 2, dtype=torch.float32) for _ in range(2))
    m.bnr_res_partial(out.data_ptr(), _p(ops[0]), _p(ops[1]), _p(ops[2]), _p(ops[3]), _p(ops[4]), _p(ops[5]),
                      _p(ops[6]), ws3.data_ptr(), _p(ops[7]), _p(ops[8]), wsd.data_ptr() if has_d else 0, G, M, C,
                      _st())
    _guard_ok(out, ws3, wsd)
    ax = ("chunk", "client", "channel", "sum")
    _exact_bf16(out[:G], out_ref, (G, M, C), AXB, "bnr_res_partial")
    L.assert_exact(ws3[:c.nchunk], p3_ref, ax)
    if has_d:
        L.assert_exact(wsd[:c.nchunk], pd_ref, ax)
    else:
        assert bool(torch.isnan(wsd[:c.nchunk]).all())
    # the backward of bn3 from those partials: t3 / s3 with the case's gamma row, dy = out, no mask
    b = types.SimpleNamespace(G=G, M=M, C=C, nchunk=c.nchunk, pow2=NL.bn_pow2(M), t=c.t3, stats=c.s3, theta=c.theta,
                              off_w=c.off_w, off_b=c.off_b)
    ref = NL.bn_bwd_ref(c.t3, out_ref, None, c.s3, c.gamma, 0)
    res = _bn_bwd_run(b, True, None, 0, dy=out[:G], part=ws3)
    _bn_bwd_check(b, res, ref, b.pow2, "bnr_bwd_part")
