"""CPU checks of tests/_stemlattice.py: the slot map, the references against PyTorch in fp64, every exactness precondition
of the lattice cases, the coverage of the shape table, and mutations showing that each listed corruption of a reference
changes the expected tensors in at least one element (the whole-tensor norms of the older stem test do not see them)."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import _alexlattice as A
import _lattice as L
import _normlattice as NL
import _stemlattice as S


def _cf(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def _relerr(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ================================================================================================ slots, polyphase
def test_slot_map_holds_every_tap_once():
    live = [k for k in S.SLOT_TAP if k >= 0]
    assert len(S.SLOT_TAP) == 512 and sorted(live) == list(range(343)) and S.SLOT_TAP.count(-1) == 169
    # the header's example: k = 2 j + r - 1 per dimension
    assert S.stem_tap(0) == -1 and S.stem_tap(7) == 0 and S.stem_tap(511) == 342
    s = ((1 * 16 + 2 * 4 + 3) << 3) | 0b101                        # (jd, jh, jw) = (1, 2, 3), (rd, rh, rw) = (1, 0, 1)
    assert S.stem_tap(s) == ((2 * 1 + 1 - 1) * 7 + (2 * 2 + 0 - 1)) * 7 + (2 * 3 + 1 - 1)


@pytest.mark.parametrize("name", ["pow2", "lane33"])        # odd extents (7, 15, 31) and even ones (6, ., 66)
def test_polyphase_conv_equals_strided_conv(name):
    c = S.fwd_case(name)
    xp, xq = S.polyphase_ref(c.vols[list(S.IDX)], c.d)
    assert torch.equal(xq.permute(0, 2, 3, 4, 1), xp)
    for n in (0, 3):
        got = S.phase_conv(xp[n], c.w[n // S.B]).permute(1, 2, 3, 0)
        x = c.vols[S.IDX[n]].double().view(1, 1, *c.vols.shape[1:])
        ref = F.conv3d(x, c.w[n // S.B].double().view(64, 1, 7, 7, 7), stride=2, padding=3)[0].permute(1, 2, 3, 0)
        assert torch.equal(got, ref) and torch.equal(got, c.acc[n])
    # the gather itself, element by element on a few coordinates
    d, v = c.d, c.vols[S.IDX[1]]
    for z, y, x, r in [(0, 0, 0, 7), (2, 2, 2, 0), (d.PZ - 1, d.PY - 1, d.PX - 1, 0), (3, 4, 5, 5), (2, 3, 9, 2)]:
        sz, sy, sx = 2 * z - 4 + (r >> 2), 2 * y - 4 + ((r >> 1) & 1), 2 * x - 4 + (r & 1)
        inside = 0 <= sz < d.D and 0 <= sy < d.H and 0 <= sx < d.W
        assert int(xp[1, z, y, x, r]) == (int(v[sz, sy, sx]) if inside else 0)


def test_volumes_encode_their_coordinates():
    v = S.volumes("pow2")
    assert v.dtype == torch.uint8 and int(v.max()) == 255 and int(v.min()) == 0
    for a, b in itertools.combinations(range(1, 4), 2):
        assert not torch.equal(v.transpose(a, b)[:, :7, :7, :7], v[:, :7, :7, :7])
    assert len({bytes(v[i].numpy().tobytes()) for i in range(S.NVOL)}) == S.NVOL
    b = S.volumes("pow2", "bin")
    assert set(b.unique().tolist()) == {0, 255}


# ================================================================================================ shape table
def test_shape_table_covers_the_classes():
    for name, (shape, classes) in S.SHAPES.items():
        assert S.shape_classes(name) == set(classes), name
        d = S.shape_dims(name)
        assert 2 <= d.OW <= 64 and d.OD >= 2 and d.OH >= 2
        assert shape != (121, 145, 121)
    union = set().union(*(set(c) for _, c in S.SHAPES.values()))
    assert union == {"ow61", "px8", "wgrad4", "wgrad", "ow33", "ow64", "ring", "od9", "pow2"}
    ds = [S.shape_dims(n) for n in S.SHAPES]
    for k in ("OD", "OH", "OW"):
        assert {getattr(d, k) % 2 for d in ds} == {0, 1}, k
    assert sum("ring" in c for _, c in S.SHAPES.values()) >= 3
    d = S.shape_dims("full")
    assert d.OD == 9 and d.nchunk == 2 and d.OD % S.WG_OD != 0 and d.PX == 64
    assert S.shape_dims("lane33").OW - 32 == 1                      # the position half ph = 1 has a single valid lane
    assert S.G >= 2 and S.B >= 2
    assert list(S.IDX) != list(range(S.N)) and len(set(S.IDX)) < len(S.IDX) and max(S.IDX) < S.NVOL > len(set(S.IDX))
    assert S.CHAIN_SHAPE == min((n for n in S.SHAPES if n != "pow2"), key=lambda n: S.shape_dims(n).M)
    assert S.LD > 64 * 343 + 128 and S.OFF_W > 0
    assert {n for n, m in S.bn_cases() if m == 1} == {"pow2", "short8"}
    assert {("wgrad4" in S.SHAPES[n][1]) for n, m in S.bn_cases() if m == 1} == {True, False}


# ================================================================================================ forward
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_fwd_case_preconditions(name):
    c = S.fwd_case(name)
    assert c.acc_bound < 2 ** 24 and float(c.acc.abs().max()) <= c.acc_bound
    assert torch.equal(c.acc, c.acc.round())
    # the stored value through plain fp32 arithmetic: one rounded product, one RNE to bf16
    y32 = (c.acc.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32)).to(torch.bfloat16)
    assert torch.equal(y32.view(torch.int16), c.y.view(torch.int16))
    assert bool((c.w[0] != c.w[1]).any()) and float(c.w.abs().max()) == 8
    # every channel has taps of different weight (an exchange of two of them moves the result), dense and sparse rows
    assert bool(((c.w.amax(2) - c.w.amin(2)) > 0).all())
    assert bool((c.w[:, 0::2] != 0).float().mean() > 0.9) and bool((c.w[:, 1::2] != 0).float().mean() < 0.3)
    # the last valid column and the first row after the 5-row ring wraps carry non-zero values in every channel
    assert bool((c.y[:, :, :, c.d.OW - 1].float().abs().amax((0, 1, 2)) > 0).all())
    if c.d.OH >= 6:
        assert bool((c.y[:, :, 5].float().abs().amax((0, 1, 2)) > 0).all())


def test_scale_fold_is_not_always_the_identity():
    """fl32(255 m fl32(1 / 255)) != m for some integers m, so the integer-y case is proven by enumeration, not assumed."""
    m = torch.arange(-256, 257, dtype=torch.float32)
    p = (255.0 * m) * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    assert bool((p != m).any())
    assert torch.equal(p.to(torch.bfloat16).float(), m)             # the bf16 store restores every |m| <= 256


def test_stat_case_is_exact():
    c = S.stat_case()
    d = c.d
    assert torch.equal(c.m, c.m.round()) and float(c.m.abs().max()) <= 8
    assert torch.equal(c.y.double(), c.m), "a stored value is not the intended integer"
    assert len(c.m.unique()) >= 9 and bool((c.m.view(-1, 64).amax(0) > c.m.view(-1, 64).amin(0)).all())
    # blocks of OH x OW = 8 x 16 positions, one valid position per lane of the first position half: every lane count and
    # every merged count is a power of two
    assert (d.OH, d.OW) == (8, 16) and d.M == 1024
    Y = 8.0
    # shifted sums: |dv| <= 2 Y integers; s1^2 < 2^24; merged means are multiples of 2^-7, their differences squared
    # multiples of 2^-12 below 4 Y^2; M2 a multiple of 2^-7 below 128 * 4 Y^2
    L.require_fp32_exact((16 * 2 * Y) ** 2, "s1^2")
    L.require_fp32_exact(16 * 4 * Y * Y, "s2")
    NL.require_dyadic(4 * Y * Y, 12, "dm^2")
    NL.require_dyadic(128 * 4 * Y * Y, 7, "M2")
    for v, bits in ((c.mean, 7), (c.m2, 7)):
        assert torch.equal(v * 2 ** bits, (v * 2 ** bits).round()) and torch.equal(v.float().double(), v)
    yc = c.y.double().view(S.G, -1, 64)
    assert torch.equal(yc.mean(1) * 1024, (yc.mean(1) * 1024).round())
    assert float(c.m2.min()) > 0


@pytest.mark.parametrize("name", list(S.SHAPES))
def test_stats_bound_is_far_below_a_dropped_position(name):
    c = S.fwd_case(name)
    e_mean, e_m2 = S.stats_bound(c.y)
    assert bool(torch.isfinite(e_m2).all()) and float(e_mean.min()) > 0
    # leaving out the last valid column moves block means by orders of magnitude more than the bound
    y = c.y.double().clone()
    cut = y[:, :, :, :-1]
    mean_cut = cut.reshape(S.G, S.B * c.d.OD, -1, 64).mean(2)
    moved = (mean_cut - c.mean).abs()
    assert float((moved > 100 * e_mean).float().mean()) > 0.9
    assert S.k_mean(c.d.OH) == 4 * c.d.OH + 42 and S.k_m2(c.d.OH) == 6 * c.d.OH + 45


# ================================================================================================ pool
@pytest.mark.parametrize("name", ["pow2", "lane33", "short8"])
def test_pool_reference_matches_max_pool3d_without_ties(name):
    d = S.shape_dims(name)
    z = torch.randn(2, d.OD, d.OH, d.OW, 8, generator=L.gen("stem", "notie", name), dtype=torch.float64) + 0.5
    out, am = S.pool_ref(z, d)
    p, i = F.max_pool3d(_cf(torch.relu(z) + 1e-9 * (z > 0)), 3, 2, 1, return_indices=True)
    live = out > 0                                                   # among several zeros PyTorch also takes the first
    od, r = i // (d.OH * d.OW), i % (d.OH * d.OW)
    oh, ow = r // d.OW, r % d.OW
    qd = torch.arange(d.QD).view(1, 1, -1, 1, 1)
    qh = torch.arange(d.QH).view(1, 1, 1, -1, 1)
    qw = torch.arange(d.QW).view(1, 1, 1, 1, -1)
    li = (od - (2 * qd - 1)) * 9 + (oh - (2 * qh - 1)) * 3 + (ow - (2 * qw - 1))
    assert torch.equal(li.permute(0, 2, 3, 4, 1).to(torch.uint8), am)
    assert float((p.permute(0, 2, 3, 4, 1) - out).abs().max()) < 1e-8 and bool(live.any())


def _brute_first_max(z, d, n, ch):
    zr = torch.relu(z[n, ..., ch])
    am = torch.zeros(d.QD, d.QH, d.QW, dtype=torch.uint8)
    for qd, qh, qw in itertools.product(range(d.QD), range(d.QH), range(d.QW)):
        best, arg = -float("inf"), 0
        for k in range(27):
            a, b, e = 2 * qd - 1 + k // 9, 2 * qh - 1 + (k // 3) % 3, 2 * qw - 1 + k % 3
            if 0 <= a < d.OD and 0 <= b < d.OH and 0 <= e < d.OW and float(zr[a, b, e]) > best:
                best, arg = float(zr[a, b, e]), k
        am[qd, qh, qw] = arg
    return am


@pytest.mark.parametrize("name", ["short8", "pow2"])
def test_pool_reference_on_ties_equals_a_first_maximum_scan(name):
    c = S.bn_case(name, 0)
    for n, ch in [(0, 0), (2, 1), (1, S.CH_DEAD), (3, S.CH_ZERO), (2, 7)]:
        assert torch.equal(_brute_first_max(c.z, c.d, n, ch), c.amax[n, ..., ch])


@pytest.mark.parametrize("name", list(S.SHAPES))
def test_pool_lattice_contents(name):
    c = S.bn_case(name, 0)
    d = c.d
    win = S.pool_windows(c.z, d)
    mx = win.amax(-1, keepdim=True)
    ismax = win == mx
    tied = (ismax.sum(-1) > 1) & (mx.squeeze(-1) > 0)
    assert float(tied.float().mean()) > 0.3
    for k in (0, 13, 26):                                            # positive ties with a maximum at the first, the
        assert bool((tied & ismax[..., k]).any()), k                 # middle and the last voxel of the window
    assert bool((c.scale < 0).any()) and bool((c.scale[:, S.CH_ZERO] == 0).all())
    assert float(c.z[..., S.CH_DEAD].max()) < 0 and float(c.out[..., S.CH_DEAD].float().abs().max()) == 0
    # windows that are all <= 0: the argmax is the first VALID voxel, index 13 / 12 / 10 / 9 / 4 / 3 / 1 / 0 by border
    first = torch.zeros(d.QD, d.QH, d.QW, dtype=torch.uint8)
    for qd, qh, qw in itertools.product(range(d.QD), range(d.QH), range(d.QW)):
        first[qd, qh, qw] = (qd == 0) * 9 + (qh == 0) * 3 + (qw == 0)
    assert set(first.unique().tolist()) == {0, 1, 3, 4, 9, 10, 12, 13}
    dead = mx.squeeze(-1) <= 0
    assert bool(dead[..., S.CH_DEAD].all()) and float(dead.float().mean()) > 0.02
    assert torch.equal(c.amax[dead], first.view(1, d.QD, d.QH, d.QW, 1).expand_as(c.amax)[dead])
    # the last window is cut at the far border exactly where the extent is odd (both occur for every axis over the table)
    for o, q in ((d.OD, d.QD), (d.OH, d.QH), (d.OW, d.QW)):
        assert (2 * (q - 1) + 1 >= o) == (o % 2 == 1)
    assert torch.equal(c.out.double(), torch.relu(mx.squeeze(-1)))


# ================================================================================================ backward
@pytest.mark.parametrize("name,mode", S.bn_cases(), ids=str)
def test_bwd_case_preconditions(name, mode):
    c = S.bn_case(name, mode)
    d = c.d
    assert torch.equal(c.y[0], c.y[1]) and not torch.equal(c.y[0], c.y[2])
    assert bool((c.gamma[0] != c.gamma[1]).any()) and bool((c.shift[0] != c.shift[1]).any())
    # voxels that collect the gradient of 0, 1, 2, 4 and 8 windows
    cnt = S.unpool_ref(torch.ones_like(c.dpool, dtype=torch.float64), c.amax, torch.ones_like(c.z), d)
    assert {0.0, 1.0, 2.0, 4.0, 8.0} <= set(cnt.unique().tolist())
    assert float(cnt[0, 1, 1, 1].min()) == 8 or float(cnt[0, 1, 1, 1, S.CH_ZERO]) < 8
    assert bool(((c.z <= 0) & (cnt > 0)).any()), "no voxel is masked by the ReLU"
    assert torch.equal(c.dz.float().double(), c.dz)
    if mode == 0:
        L.require_bf16_exact(c.dz, "dz")
        assert float(c.s1.abs().max()) == 0 and float(c.s2.abs().max()) == 0
        assert float(c.coef[:, :, 1:].abs().max()) == 0
        assert bool((c.part.abs().amax((1, 3)) > 0)[:, [0, 1, 2, 4, 6]].all())
    xhat = (c.y.double() - S.rep(c.mean)) * S.rep(c.invstd)
    assert torch.equal(xhat, xhat.round())
    L.require_fp32_exact((c.dz.abs() * xhat.abs()).view(S.G, S.B * d.OD, -1, 64).sum(2).max(), "block sum of dz xhat")
    L.require_fp32_exact(c.dz.abs().view(S.G, S.B * d.OD, -1, 64).sum(2).max(), "block sum of dz")
    assert torch.equal(c.part.float().double(), c.part)
    M = float(d.M)
    if mode == 1:
        pl = c.planted
        assert int(pl.sum()) > 64
        assert torch.equal(c.s1[pl], torch.full_like(c.s1[pl], c.delta))
        assert torch.equal(c.s1 / M * M, c.s1) and torch.equal(c.s2 / M * M, c.s2)
        q = (c.s2 / M).abs()[pl]
        assert bool((torch.frexp(q)[0] == 0.5).all())                # s2 / M is a power of two
        live = pl & (c.gamma != 0)
        assert bool((c.coef[:, :, 1][live] != 0).all()) and int((c.coef[:, :, 2][live] != 0).sum()) > 32
        b = c.coef[:, :, 1][live].abs()
        assert bool((torch.frexp(b)[0] == 0.5).all())                # b is a power of two
        assert bool((~pl & (c.s1 != 0)).sum() == 0)
    if mode == 2:
        assert not torch.equal(c.coef.float().double(), c.coef)      # inexact quotients: the 1-ulp check applies
        return
    assert torch.equal(c.coef.float().double(), c.coef)
    assert torch.equal(c.dy64.float().double(), c.dy64), "dy is not exact in fp32 before its bf16 store"
    if mode == 0:                                                    # mode 1: one RNE of the exact fp32 value
        assert torch.equal(c.dy.double(), c.dy64), "dy is no bf16 number"
    dyb = c.dy.double()
    frac = 3 if (name, mode) == ("pow2", 1) else 0                   # dy is an integer but for delta = M / 8
    assert torch.equal(dyb * 2 ** frac, (dyb * 2 ** frac).round())
    per_block = torch.stack([dyb[:, o:o + S.WG_OD].abs().reshape(S.N, -1, 64).sum(1) for o in range(0, d.OD, S.WG_OD)])
    NL.require_dyadic(255.0 * float(per_block.max()), frac, "slab entry")
    assert torch.equal(c.slab.float().double(), c.slab)
    assert bool((c.slab.abs().amax((2, 3, 4)) > 0).all())            # every (sample, chunk) contributes
    # the 169 non-tap slots of the row hold ordinary correlations in the slabs
    empty = torch.tensor([k < 0 for k in S.SLOT_TAP]).view(4, 128)
    assert bool((c.slab.abs().amax((0, 1, 3))[empty] > 0).any())


@pytest.mark.parametrize("name,mode", [("pow2", 0), ("short8", 1)])
def test_backward_references_match_fp64_autograd(name, mode):
    """Unpool, ReLU mask, dgamma / dbeta against autograd through the module chain with the case's (given) statistics; the
    BN coefficients against autograd through batch_norm on real batch statistics; the weight gradient against autograd
    through conv3d of x / 255 (the bf16 store of y is straight-through: dy is the gradient at the stored value)."""
    c = S.bn_case(name, mode)
    d = c.d
    for g in range(S.G):
        sl = slice(g * S.B, (g + 1) * S.B)
        y = c.y[sl].double().requires_grad_(True)
        gm = c.gamma[g].double().clone().requires_grad_(True)
        bt = c.beta[g].double().clone().requires_grad_(True)
        z = (y - c.mean[g].double()) * c.invstd[g].double() * gm + bt
        assert torch.equal(z.detach(), c.z[sl])
        o = S.pool_windows(z, d).gather(-1, c.amax[sl].long().unsqueeze(-1)).squeeze(-1)
        o.backward(c.dpool[sl].double())
        assert torch.equal(gm.grad, c.s2[g]) and torch.equal(bt.grad, c.s1[g])
        assert torch.equal(y.grad, c.dz[sl] * (c.gamma[g] * c.invstd[g]).double())
        # weight gradient
        w = torch.zeros(64, 1, 7, 7, 7, dtype=torch.float64, requires_grad=True)
        x = torch.stack([c.vols[i] for i in S.IDX[g * S.B:(g + 1) * S.B]]).double().unsqueeze(1) / 255.0
        F.conv3d(x, w, stride=2, padding=3).backward(_cf(c.dy[sl].double()))
        assert _relerr(S.row_ref64(c.slab)[g], w.grad.view(64, 343)) < 1e-13
        assert _relerr(c.row[g], w.grad.view(64, 343)) < 2 ** -23
    # BN training backward on real batch statistics
    yi = _cf(c.y[:S.B].double()).requires_grad_(True)
    gm = torch.rand(64, dtype=torch.float64, generator=L.gen("stem", "bnauto")) + 0.5
    F.batch_norm(yi, None, None, gm, torch.zeros(64, dtype=torch.float64), True, 0.1, 1e-300).backward(_cf(c.dz[:S.B]))
    yf = c.y[:S.B].double().view(-1, 64)
    mu = yf.mean(0)
    iv = 1.0 / yf.var(0, unbiased=False).sqrt()
    dzf = c.dz[:S.B].reshape(-1, 64)
    s1, s2 = dzf.sum(0), (dzf * (yf - mu) * iv).sum(0)
    co = S.coef_ref(s1.view(1, 64), s2.view(1, 64), gm.view(1, 64), iv.view(1, 64), mu.view(1, 64), float(yf.shape[0]))[0]
    dy = co[:, 0] * c.dz[:S.B] + co[:, 1] * c.y[:S.B].double() + co[:, 2]
    assert _relerr(dy, yi.grad.permute(0, 2, 3, 4, 1)) < 1e-12


def test_chain_reference_skips_under_one_percent():
    """The chained case on the CPU (fp64 conv, bf16 store, fp64 statistics): the share of windows within one bf16 ulp of
    a tie and of voxels within one bf16 ulp of the ReLU threshold stays below SKIP_MAX for the chosen seed."""
    c = S.chain_case()
    d = c.d
    yref, ybound = S.chain_fwd_ref(c)
    # half a bf16 ulp plus the counted fp32 roundings of the sum: below one bf16 ulp except where the sum cancels
    assert float((ybound / S.ulp_bf16(yref)).median()) < 1.0
    y = yref.float().to(torch.bfloat16)
    mean, m2 = S.stats_ref(y)
    nb = torch.full((S.B * d.OD,), float(d.OH * d.OW), dtype=torch.float64)
    mg, vg, n = A.chan_merge(torch.stack([mean, m2], 3), nb)
    r = A.bn_fin_ref(c.bn, mg, vg, n, S.EPS)
    z, zmag, _, _, _, skip = S.chain_pool_ref(y, r.scale.float(), r.shift.float(), d)
    print("stemlattice chain (CPU) windows skipped %.4f, voxels near the threshold %.4f"
          % (float(skip.float().mean()), float(S.near_threshold(z, zmag).float().mean())))
    assert float(skip.float().mean()) < S.SKIP_MAX and float(S.near_threshold(z, zmag).float().mean()) < S.SKIP_MAX
    assert float((z > 0).float().mean()) > 0.2 and float((z <= 0).float().mean()) > 0.2


# ================================================================================================ mutations
def test_mutation_two_taps_of_one_channel_exchanged():
    c = S.fwd_case("pow2")
    g, ch, k1, k2 = 1, 9, 171, 172                                   # a sparse channel, the centre tap and its neighbour
    w = c.w.clone()
    if w[g, ch, k1] == w[g, ch, k2]:
        k2 = int(torch.nonzero(w[g, ch] != w[g, ch, k1])[0])
    w[g, ch, [k1, k2]] = w[g, ch, [k2, k1]]
    y = S.y_store(S.conv_acc(c.vols, w, S.IDX))
    old = _relerr(y.float(), c.y.float())
    print("stemlattice mutation exchanged taps: relative norm %.3g (old threshold 1e-2)" % old)
    assert 0 < old < 1e-2
    e = A.first_mismatch(y.view(torch.int16), c.y.view(torch.int16), S.AX_Y)
    assert e is not None and "channel=%d)" % ch in e and "sample=%d," % (g * S.B) in e
    assert torch.equal(y[:g * S.B], c.y[:g * S.B])


def test_mutation_two_phase_bits_exchanged():
    c = S.fwd_case("pow2")
    v = c.vols[list(S.IDX)]
    xp, xq = S.polyphase_ref(v, c.d)
    bp, bq = S.polyphase_ref(v, c.d, bits=(1, 0, 2))
    assert A.first_mismatch(bp, xp, ("sample", "z", "y", "x", "phase")) is not None
    assert A.first_mismatch(bq, xq, ("sample", "phase", "z", "y", "x")) is not None
    assert torch.equal(bp[..., [0, 1, 6, 7]], xp[..., [0, 1, 6, 7]])     # phases with rd == rh stay
    assert not torch.equal(S.phase_conv(bp[0], c.w[0]).permute(1, 2, 3, 0), c.acc[0])


def test_mutation_last_column_and_wrapped_row_dropped():
    c = S.bn_case("full", 0)
    d = c.d
    for what, mask in (("ow = OW - 1", (slice(None), slice(None), d.OW - 1)), ("oh = 4 (4-row ring)", (slice(None), 4)),
                       ("oh = 5 (5-row ring)", (slice(None), 5))):
        keep = torch.ones(d.OD, d.OH, d.OW, dtype=torch.bool)
        keep[mask] = False
        slab = S.wgrad_ref(c.dy, c.xq, d, pos_mask=keep)
        old = _relerr(S.row_ref(slab), c.row)
        print("stemlattice mutation dropped %s: relative norm of the row %.3g (old threshold 2e-2)" % (what, old))
        with pytest.raises(AssertionError, match="sample=0, chunk=0, jd=0"):
            L.assert_exact(slab, c.slab, S.AX_SLAB)
        assert not torch.equal(S.row_ref(slab), c.row)
    f = S.fwd_case("full")
    y = f.y.clone()
    y[:, :, :, d.OW - 1] = 0
    assert 0 < _relerr(y.float(), f.y.float()) and A.first_mismatch(y.view(torch.int16), f.y.view(torch.int16), S.AX_Y)


def test_mutation_od_tail_chunk_dropped():
    c = S.bn_case("full", 0)
    d = c.d
    keep = torch.ones(d.OD, d.OH, d.OW, dtype=torch.bool)
    keep[S.WG_OD:] = False
    slab = S.wgrad_ref(c.dy, c.xq, d, pos_mask=keep)
    assert torch.equal(slab[:, 0], c.slab[:, 0]) and float(slab[:, 1].abs().max()) == 0
    old = _relerr(S.row_ref(slab), c.row)
    print("stemlattice mutation dropped od tail chunk: relative norm of the row %.3g" % old)
    with pytest.raises(AssertionError, match="chunk=1"):
        L.assert_exact(slab, c.slab, S.AX_SLAB)
    e = A.first_mismatch(S.row_ref(slab), c.row, ("client", "channel", "tap"))
    assert e is not None


def test_mutation_argmax_takes_the_last_maximum():
    c = S.bn_case("short8", 0)
    out, am = S.pool_ref(c.z, c.d, last=True)
    assert torch.equal(out.to(torch.bfloat16).view(torch.int16), c.out.view(torch.int16))    # the values do not move
    e = A.first_mismatch(am, c.amax, S.AX_Q)
    assert e is not None
    dz = S.unpool_ref(c.dpool.double(), am, c.z, c.d)
    assert A.first_mismatch(dz, c.dz, S.AX_Y) is not None


def test_mutation_one_window_of_eight_dropped():
    c = S.bn_case("short8", 0)
    dz = S.unpool_ref(c.dpool.double(), c.amax, c.z, c.d, drop_k=26)     # the window a voxel closes as its last voxel
    bad = dz != c.dz
    print("stemlattice mutation dropped window: %d of %d dz values move" % (int(bad.sum()), bad.numel()))
    assert 0 < int(bad.sum()) < bad.numel() // 20
    assert bool(bad[0, 1, 1, 1].any())                                   # the planted 8-window voxel among them
    part, _, _ = S.block_sums(dz, c.y, c.mean, c.invstd)
    assert not torch.equal(part, c.part)


def test_mutation_one_block_partial_dropped():
    c = S.bn_case("short8", 1)
    ch = int(torch.nonzero(c.planted[0])[0])
    blocks = torch.nonzero(c.part[0, :, ch, 0] != 0)
    _, s1, s2 = S.block_sums(c.dz, c.y, c.mean, c.invstd, skip=(0, int(blocks[-1])))
    assert float(s1[0, ch]) != float(c.s1[0, ch])
    coef = S.coef_ref(s1, s2, c.gamma, c.invstd, c.mean, float(c.d.M))
    with pytest.raises(AssertionError, match="client=0, channel="):
        L.assert_exact(coef, c.coef, S.AX_GC + ("coef",))
    with pytest.raises(AssertionError):
        L.assert_exact(s1, c.s1, S.AX_GC)


def test_mutation_sample_index_used_as_volume_index():
    c = S.fwd_case("short8")
    y = S.y_store(S.conv_acc(c.vols, c.w, list(range(S.N))))
    e = A.first_mismatch(y.view(torch.int16), c.y.view(torch.int16), S.AX_Y)
    assert e is not None and "sample=0," in e
    xp, _ = S.polyphase_ref(c.vols[list(S.IDX)], c.d)
    bp, _ = S.polyphase_ref(c.vols[:S.N], c.d)
    assert not torch.equal(xp[0], bp[0]) and torch.equal(xp[1], bp[0]) and torch.equal(xp[2], bp[1])
