"""CPU checks of tests/_alexlattice.py: every precondition the bit-exact GPU comparisons of tests/test_gpu_exact_alexnet.py
rest on holds for every table entry, the references agree with fp64 autograd on one real instance each, and each of five
single-element corruptions passes the older relative-norm thresholds (computed as the older tests compute them) while the
new assertion fails at the corrupted index."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _alexlattice as A
import _lattice as L
import _normlattice as NL


def _relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _cf(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def _pool_at(h, amax):
    """max_pool3d(3, 3) whose window choices are given argmax bytes (tests/test_gpu_kernels.py routes the same way)."""
    Bn, C, D, H, W = h.shape
    Dp, Hp, Wp = D // 3, H // 3, W // 3
    a = amax.long().permute(0, 4, 1, 2, 3)
    pd = torch.arange(Dp).view(1, 1, Dp, 1, 1)
    ph = torch.arange(Hp).view(1, 1, 1, Hp, 1)
    pw = torch.arange(Wp).view(1, 1, 1, 1, Wp)
    flat = ((3 * pd + a // 9) * H + 3 * ph + (a // 3) % 3) * W + 3 * pw + a % 3
    return torch.gather(h.reshape(Bn, C, -1), 2, flat.reshape(Bn, C, -1)).view(Bn, C, Dp, Hp, Wp)


# ================================================================================================ conv1 layout
@pytest.mark.parametrize("ro,ks", [(0, 128), (1, 128), (2, 128), (0, 224)])
def test_slot_layout_covers_125_taps_once(ro, ks):
    slots = A.c1_slots(ro, ks)
    assert len(slots) == ks
    assert sorted(A.slot_taps(slots)) == list(range(125))
    assert slots.count(None) == ks - 125
    assert all(A.tp_valid(*s) for s in slots if s is not None)


def test_slot_layout_structure():
    """The layout as the comment above c1_slot128 states it: 8 F groups of 8 phases in k-steps 0-1, D + H groups in k-step
    2, W + the 2-phase groups in k-step 3, 3 empty slots at the end of the last lane group."""
    s = A.c1_slots(0)
    g = A._groups()
    assert [len(g[k]) for k in ("F", "D", "H", "W", "DH", "DW", "HW", "DHW")] == [8, 4, 4, 4, 2, 2, 2, 1]
    assert [s[8 * i][0] for i in range(8)] == g["F"]
    assert [s[64 + 8 * i][0] for i in range(4)] == g["D"] and [s[68 + 8 * i][0] for i in range(4)] == g["H"]
    assert [s[96 + 8 * i][0] for i in range(4)] == g["W"]
    assert s[125:] == [None, None, None] and s[124] == (26, 0)
    # the paired orders keep the same groups per k-step and pair equal jw within (fq 0, fq 1) and (fq 2, fq 3)
    for ro in (1, 2):
        p = A.c1_slots(ro)
        for st in range(3):
            assert sorted(x[0] for x in p[32 * st:32 * st + 32]) == sorted(x[0] for x in s[32 * st:32 * st + 32])
            for e in (0, 4):
                t = [p[32 * st + 8 * fq + e][0] for fq in range(4)]
                assert t[0] % 3 == t[1] % 3 and t[2] % 3 == t[3] % 3


# ================================================================================================ conv1 forward
def test_conv1_operands_and_bounds():
    v, c = A.volumes(), A.conv1_case()
    assert int(v.min()) == 0 and int(v.max()) == 255
    assert not torch.equal(v[0], v[1]) and not torch.equal(v[0], v[2]) and not torch.equal(v[1], v[2])
    b = A.C1_BORDER
    assert b >= 9 and int(v[1, :b].max()) == 0 and int(v[1, :, :, -b:].max()) == 0 and int(v[1, b:-b, b:-b, b:-b].max()) == 255
    idx = c.idx.tolist()
    assert idx != sorted(idx) and len(set(idx)) == 3 and max(idx.count(i) for i in idx) == 2
    assert float(c.w.abs().max()) <= A.C1_WMAX and torch.equal(c.w.half().float(), c.w)
    sw = c.w.abs().sum(2)
    assert float(255 * sw.max()) < A.ACC_LIMIT                      # masking the 5 tag bits removes nothing
    assert float((1024 + 255) * sw.max()) < L.FP32_EXACT            # the running magnitude of the offset accumulation
    assert float(c.acc.abs().max()) < A.ACC_LIMIT and torch.equal(c.acc, c.acc.round())
    assert bool((c.scale < 0).any()) and bool((c.scale > 0).any()) and bool((c.scale[:, A.C1_ZERO_SCALE_CH] == 0).all())
    live = (c.out.float() > 0).view(-1, A.C1).any(0)
    assert not bool(live[c.dead].any()) and bool(live[~c.dead].all())       # dead channels are dead, the others are not
    assert bool((c.shift[:, ~c.dead] > 0).any()) and bool((c.shift[:, ~c.dead] < 0).any())


@pytest.mark.parametrize("k", sorted(set(A.C1_KEXP)))
def test_scale_fold_is_a_power_of_two(k):
    """fl(255 2^-k * fl(1 / 255)) = 2^-k in fp32: the forward's |scale| / 255 is exact for these scales."""
    s = torch.tensor(255.0 * 2.0 ** -k, dtype=torch.float32)
    r = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(255.0, dtype=torch.float32)
    assert float(s * r) == 2.0 ** -k


def test_conv1_tie_rule_in_the_zero_border():
    """Windows inside the zero border tie at all 27 candidates with acc = 0: the largest index wins."""
    c = A.conv1_case()
    n = c.idx.tolist().index(1)
    for cell in ((0, 0, 0), (18, 22, 18)):
        assert float(c.macc[(n,) + cell].abs().max()) == 0.0
        assert bool((c.amax[(n,) + cell] == 26).all())
    k = A.window_keys(torch.tensor([[-3, 5, 5, -3] + [-7] * 23, [-3, -9, -3, -9] + [-9] * 23]))
    assert k.argmax(-1).tolist() == [2, 0]                          # acc >= 0: largest index; acc < 0: smallest
    assert bool((c.out[n, 0, 0, 0].float() > 0).any())              # some of these tied cells are checked (shift > 0)


def test_conv1_forward_reference_matches_fp64_pipeline():
    """conv3d -> affine -> relu -> max_pool3d in fp64 on one real sample equals the lattice reference (the tie rule does
    not affect values); the argmax gathers the maximum."""
    c, v = A.conv1_case(), A.volumes()
    n, g = 1, 0
    x = v[int(c.idx[n])].double().view(1, 1, *A.VOL)
    w = (c.w[g] * c.sign[g].unsqueeze(1)).double().view(A.C1, 1, 5, 5, 5)
    y = F.conv3d(x, w, stride=2)
    z = y * c.mult[g].view(1, -1, 1, 1, 1) + c.shift[g].double().view(1, -1, 1, 1, 1)
    p = F.max_pool3d(torch.relu(z), 3, 3)
    assert torch.equal(p.permute(0, 2, 3, 4, 1)[0].to(torch.bfloat16), c.out[n])
    routed = torch.relu(_pool_at(z, c.amax[n:n + 1]))
    assert torch.equal(routed, p)


def test_pack_reference():
    c = A.conv1_case()
    w8, w125 = A.pack_ref(c, 1.0)
    assert torch.equal(w125, c.w)
    back = w8.view(torch.float16).float()
    slots = A.c1_slots(0)
    for kk in (0, 37, 70, 100, 124):
        assert torch.equal(back[:, :, kk], c.w[:, :, A.tp_to_k(*slots[kk])] * c.sign)
    assert bool((w8[:, :, 125:] == 0).all())
    w8b, _ = A.pack_ref(c, 1.0, ro=2)
    assert not torch.equal(w8, w8b) and torch.equal(w8.sort(2)[0], w8b.sort(2)[0])


# ================================================================================================ conv1 statistics
def test_moments_reference_matches_package_reference():
    from neuroimagedisttraining_amd.data.synthetic_fl import conv1_moments_reference
    m = A.moments_ref()
    assert torch.equal(m[:1], conv1_moments_reference(A.volumes()[:1]))
    assert float(m.max()) < 2.0 ** 53 and torch.equal(m, m.round())


def test_bnstats_conditioning_and_bounds():
    """The two fp64 references (direct, moment form) agree to the measured conditioning; no bound admits 2 ulp."""
    c = A.conv1_case()
    cond = A.bnstats_cond()
    print("alexlattice measured conditioning of var (direct vs moment form): %.3g" % cond)
    assert cond < 2.0 ** -40
    md, vd = A.bnstats_direct(c)
    mm, vm, mu, covw = A.bnstats_moment_form(c.w, c.idx.tolist(), c.B)
    assert float(((md - mm).abs() / md.abs().clamp_min(1.0)).max()) < 2.0 ** -40
    g = L.gen("alex", "bnstats", "g2")
    theta, off = A.bnstats_theta(c.G, g)
    bufs, boff = A.bnstats_bufs(c.G, g)
    r = A.bnstats_from(md, vd, mu, covw, theta, off, bufs, boff, float(c.B * A.NPOS))
    b = A.bnstats_bounds(r, 4 * cond)
    assert bool((b.invstd < 2 * NL.ulp32(r.invstd)).all()) and bool((b.scale < 2 * NL.ulp32(r.scale)).all())
    # the running variance is the unbiased one: the biased one misses the bound
    biased = (1.0 - A.MOM) * bufs[:, boff.rv:boff.rv + 64].double() + A.MOM * vd
    assert bool(((biased - r.rv).abs() > b.rv).all())
    G, idx, w = A.bnstats_g32()
    assert G >= 32 and set(idx) == {0, 1, 2} and float(w.abs().max()) <= A.C1_WMAX


# ================================================================================================ conv1 weight gradient
def test_wgrad_inputs_cover_every_offset():
    w = A.wgrad_case()
    assert set(w.dp.float().unique().tolist()) == {0.0, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0}
    assert 0.45 < float((w.dp.float() == 0).float().mean()) < 0.55
    assert 0.45 < float((w.pout.float() > 0).float().mean()) < 0.55
    a = w.amax
    for pd in range(2):
        for ph in range(2):
            for pw in range(2):
                assert len(a[:, pd::2, ph::2, pw::2].unique()) == 27
    for sl in (a[:, 0], a[:, -1], a[:, :, 0], a[:, :, -1], a[:, :, :, 0], a[:, :, :, -1]):
        assert len(sl.unique()) == 27
    # integer sums below 2^24 per sample, with the largest per-sample scale of the NB = 256 case
    dz = A.wgrad_dz(w.dp, w.pout)
    L.require_fp32_exact(float(dz.abs().view(4, -1, A.C1).sum(1).max()) * 255 * max(A.big_scales()), "conv1 wgrad sums")
    assert torch.equal(w.S, w.S.round()) and float(w.S.abs().max()) < L.FP32_EXACT


def test_wgrad_big_case_mixes_samples_aperiodically():
    NB, B = A.C1_BIG
    s = A.big_scales(NB)
    assert set(s) == {1, 2, 4}
    coef = torch.tensor(s, dtype=torch.float64).view(NB // B, B // 4, 4).sum(1)         # weight of base sample j per client
    assert len({tuple(r) for r in coef.tolist()}) >= NB // B // 2
    assert any(s[n] != s[n + 4] for n in range(NB - 4)) and any(s[n] != s[n + B] for n in range(NB - B))
    w = A.wgrad_case()
    S, D = A.wgrad_client(w.S, w.D, B, s)
    assert S.shape == (NB // B, A.C1, 125) and float(S.abs().max()) * 1 < 2.0 ** 53


def test_wgrad_and_closed_form_match_fp64_autograd():
    """S, D against autograd of conv -> argmax-routed pool on one sample; the train and eval closed forms against autograd
    through BatchNorm on client 0 (two samples) with real gamma and the fp64 moment statistics."""
    c, w, v = A.conv1_case(), A.wgrad_case(), A.volumes()
    B = w.B
    wt = c.w[0].double().view(A.C1, 1, 5, 5, 5).requires_grad_(True)
    bias = torch.zeros(A.C1, dtype=torch.float64, requires_grad=True)
    x = torch.stack([v[int(i)].double() for i in w.idx[:B]]).unsqueeze(1)
    y = F.conv3d(x, wt, bias, stride=2)
    live = _cf(w.pout[:B].double()) > 0
    dpo = _cf(w.dp[:B].double())
    (_pool_at(y, w.amax[:B]) * live)[0].backward(dpo[0], retain_graph=True)
    assert torch.equal(wt.grad.view(A.C1, 125), w.S[0]) and torch.equal(bias.grad, w.D[0])
    # train-mode closed form
    g = L.gen("alex", "autograd")
    gm = (torch.rand(A.C1, generator=g).double() + 0.5) * (torch.randint(0, 2, (A.C1,), generator=g) * 2 - 1)
    gm.requires_grad_(True)
    bt = torch.zeros(A.C1, dtype=torch.float64, requires_grad=True)
    wt.grad = None
    z = F.batch_norm(y, None, None, gm, bt, True, 0.1, A.EPS)
    (_pool_at(z, w.amax[:B]) * live).backward(dpo)
    _, var, mu, covw = A.bnstats_moment_form(c.w[:1], w.idx[:B].tolist(), B)
    f = A.fin_case(1, False)
    f.mu, f.covw, f.w125, f.wscale = mu, covw, c.w[:1], 1.0
    f.invstd, f.gamma = 1.0 / torch.sqrt(var + A.EPS), gm.detach().view(1, -1)
    S, D = A.wgrad_client(w.S[:B], w.D[:B], B)
    r = A.fin_ref(f, S, D, exact=False)
    assert _relerr(r["dW"][0], wt.grad.view(A.C1, 125)) < 1e-7      # limited by the cancellation in M / N - mu mu^T
    assert _relerr(r["dgamma"][0], gm.grad) < 1e-9 and _relerr(r["dbeta"][0], bt.grad) < 1e-12
    # eval-mode closed form: running statistics are constants
    wt2 = c.w[0].double().view(A.C1, 1, 5, 5, 5).requires_grad_(True)
    b2 = torch.randint(-2, 3, (A.C1,), generator=g).double().requires_grad_(True)
    rm, rv = torch.randn(A.C1, generator=g).double() * 100, torch.rand(A.C1, generator=g).double() * 1e4 + 1
    gm2 = gm.detach().clone().requires_grad_(True)
    z = F.batch_norm(F.conv3d(x, wt2, b2, stride=2), rm, rv, gm2, bt, False, 0.1, A.EPS)
    (_pool_at(z, w.amax[:B]) * live).backward(dpo)
    f.invstd, f.emean = (1.0 / torch.sqrt(rv + A.EPS)).view(1, -1), (rm - b2.detach()).view(1, -1)
    r = A.fin_ref(f, S, D, exact=False)
    assert _relerr(r["dW"][0], wt2.grad.view(A.C1, 125)) < 1e-12 and _relerr(r["dbias"][0], b2.grad) < 1e-12
    assert _relerr(r["dgamma"][0], gm2.grad) < 1e-9


@pytest.mark.parametrize("eval_mode", [False, True])
def test_closed_form_case_is_exact_in_fp32(eval_mode):
    w = A.wgrad_case()
    f = A.fin_case(w.G, eval_mode)
    r = A.fin_ref(f, *A.wgrad_client(w.S, w.D, w.B))           # asserts every result is an fp32 number
    assert float(r["dW"].abs().max()) > 0 and float(r["dgamma"].abs().max()) > 0
    assert (f.emean is not None) == eval_mode and bool((r["dbias"] != 0).any()) == eval_mode
    keep = torch.ones(f.ldg, dtype=torch.bool)
    for o, n in f.spans:
        assert bool(keep[o:o + n].all())
        keep[o:o + n] = False
    assert int(keep.sum()) == 8 * 5                             # filler columns around every slice


# ================================================================================================ bn.hip
@pytest.mark.parametrize("G,B", A.BN_GB)
@pytest.mark.parametrize("shape", A.BN_SHAPES, ids=str)
def test_bn_pool_case_preconditions(shape, G, B):
    c = A.bn_pool_case(*shape, G, B)
    D, H, W, C = shape
    assert C % 8 == 0 and bool((c.scale == 0).any()) and bool((c.scale < 0).any())
    win = A.pool_windows(c.z)
    tied = (win == win.amax(-1, keepdim=True)).sum(-1) > 1
    assert float(tied.float().mean()) > 0.5                      # deliberately tied windows
    assert bool((c.amax[(c.scale == 0).repeat_interleave(B, 0).view(c.NB, 1, 1, 1, C).expand_as(c.amax)] == 0).all())
    # PyTorch's rule: max_pool3d returns the first maximum in scan order
    p, i = F.max_pool3d(_cf(c.z), 3, 3, return_indices=True)
    d, r = i // (H * W), i % (H * W)
    li = (d % 3) * 9 + ((r // W) % 3) * 3 + (r % W) % 3
    assert torch.equal(li.permute(0, 2, 3, 4, 1).to(torch.uint8), c.amax)
    assert torch.equal(torch.relu(p).permute(0, 2, 3, 4, 1).to(torch.bfloat16), c.out)


def test_bn_shape_tables():
    assert {(D % 3, H % 3, W % 3) for D, H, W, _ in A.BN_SHAPES} >= {(2, 0, 2), (2, 1, 2), (0, 0, 0), (1, 2, 1)}
    assert (5 // 3, 7 // 3, 5 // 3) == (1, 2, 1) and 256 % (24 // 8) != 0
    cases = A.bn_bwd_cases()
    assert len(cases) == len(A.BN_SHAPES) * len(A.BN_GB) * 4
    for pool in (0, 1):
        for ev in (0, 1):
            sub = [c for c in cases if c[2] == pool and c[3] == ev]
            assert {c[4] for c in sub} == set(A.BN_NCHUNK) and {c[5] for c in sub} == {True, False}
    # one nchunk exceeds the number of positions of its case: some chunks are empty
    assert any(c[4] > c[1][1] * np.prod(c[0][:3]) for c in cases)


@pytest.mark.parametrize("pool", [0, 1])
def test_bn_bwd_reference_matches_fp64_autograd(pool):
    """Train and eval references against autograd through batch_norm with the case's own (dyadic) statistics replaced by
    the batch statistics of a real instance."""
    shape, gb = (5, 7, 5, 128), (2, 3)
    c = copy.copy(A.bn_bwd_case(shape, gb, pool, 0))
    D, H, W, C = shape
    G, B = gb
    for g in range(G):
        sl = slice(g * B, (g + 1) * B)
        yi = _cf(c.y[sl].double()).requires_grad_(True)
        gm = c.gamma[g].double().clone().requires_grad_(True)
        bt = (c.shift[g] + c.mean[g] * c.scale[g]).double().clone().requires_grad_(True)
        # the case's mean / invstd are given numbers, not the batch statistics: build the same function by hand
        z = (yi - c.mean[g].double().view(1, C, 1, 1, 1)) * c.invstd[g].double().view(1, C, 1, 1, 1)
        z = z * gm.view(1, C, 1, 1, 1) + bt.view(1, C, 1, 1, 1)
        if pool:
            o = _pool_at(z, c.amax[sl]) * (_cf(c.pout[sl].double()) > 0)
        else:
            o = torch.relu(z)
        o.backward(_cf(c.dsrc[sl].double()))
        assert torch.equal(gm.grad, c.sdx[g]) and torch.equal(bt.grad, c.sdz[g])
        # eval mode: statistics are constants, dy = gamma invstd dz
        e = A.bn_bwd_case(shape, gb, pool, 1)
    # train mode on batch statistics: autograd through batch_norm itself against the header's coefficients
    yi = _cf(c.y[:B].double()).requires_grad_(True)
    gm = c.gamma[0].double()
    z = F.batch_norm(yi, None, None, gm, torch.zeros(C, dtype=torch.float64), True, 0.1, 1e-300)
    dz = _cf(c.dz[:B])
    z.backward(dz)
    yf = c.y[:B].double().view(-1, C)
    mu, iv = yf.mean(0), 1.0 / yf.var(0, unbiased=False).sqrt()
    N = float(yf.shape[0])
    sdz, sdx = c.dz[:B].reshape(-1, C).sum(0), (c.dz[:B].reshape(-1, C) * (yf - mu) * iv).sum(0)
    dy = gm * iv * c.dz[:B] + (-gm * iv * sdz / N + gm * iv * iv * mu * sdx / N) + (-gm * iv * iv * sdx / N) * c.y[:B].double()
    assert _relerr(dy, yi.grad.permute(0, 2, 3, 4, 1)) < 1e-12
    assert e.ev == 1 and torch.equal(e.dy, e.coef[:, :, 0].repeat_interleave(B, 0).view(-1, 1, 1, 1, C) * e.dz)


def test_bn_bwd_pool_remainder_gets_only_the_affine_term():
    c = A.bn_bwd_case((5, 7, 5, 128), (2, 3), 1, 0)
    assert not bool(c.inside.all())
    out = ~c.inside
    assert float(c.dz[:, out].abs().max()) == 0.0 and float(c.dz.abs().max()) > 0
    rep = lambda v: v.repeat_interleave(c.B, 0).view(c.NB, 1, 1, 1, c.C)  # noqa: E731
    want = rep(c.coef[:, :, 1]) + rep(c.coef[:, :, 2]) * c.y.double()
    assert torch.equal(c.dy[:, out], want.expand_as(c.dy)[:, out])


@pytest.mark.parametrize("case", A.BN_FIN, ids=str)
def test_bn_finalize_partials_merge_to_the_closed_form(case):
    c = A.bn_fin_case(*case)
    nPB, BP, ragged, C, G = case
    assert (c.Mg % BP != 0) == ragged
    mean, var, n = A.chan_merge(c.stats, c.nb)
    assert float(n[0, 0]) == c.Mg
    # fp64 Chan merge: equal to the closed form up to fp64 rounding, hence equal after the kernel's fp32 casts
    assert torch.equal(mean.float().double(), c.mean)
    assert torch.equal((1.0 / var.sqrt()).float().double(), torch.ldexp(torch.ones_like(var), c.m))
    if nPB > 1:
        assert bool((c.stats[:, :, :, 0] != c.mean.unsqueeze(1)).any())      # the d^2 term of the merge is exercised
    r = A.bn_fin_ref(c, c.mean, c.var, float(c.Mg), 0.0)
    for k in ("invstd", "scale", "shift"):
        v = getattr(r, k)
        assert torch.equal(v.float().double(), v)
    # the unbiased running variance: the biased one misses the bound
    biased = (1.0 - A.MOM) * c.bufs[:, c.off_rv:c.off_rv + C].double() + A.MOM * c.var
    assert bool(((biased - r.rv).abs() > r.rv_bound).all())


def test_bn_finalize_table_covers_the_issue():
    t = A.BN_FIN
    assert {c[0] for c in t} == {1, 3, 64, 65, 130} and {c[1] for c in t} == {64, 128, 256}
    assert {c[2] for c in t} == {True, False} and {c[3] for c in t} >= {8, 192} and {c[4] for c in t} == {1, 3}
    assert any((c[3] * c[4]) % 4 != 0 for c in t)               # G C no multiple of the four pairs of a block


def test_bn_eval_and_apply_cases():
    for exact in (True, False):
        c = A.bn_eval_case(3, 8, exact)
        assert (c.eps == 0.0) == exact
        if exact:
            for v in (c.invstd, c.scale, c.shift):
                assert torch.equal(v.float().double(), v)
    for a in A.BN_APPLY:
        c = A.bn_apply_case(*a)
        assert c.npos % c.S == 0 and bool((c.h.float() > 0).any()) and bool((c.h.float() == 0).any())
    assert (A.BN_APPLY[1][0] * (A.BN_APPLY[1][1] // 8)) % 256 != 0


# ================================================================================================ heads
def test_hash4_matches_the_package_twin():
    from neuroimagedisttraining_amd.ops.reference import dropout_keep, hash4_np
    a, b, c = np.arange(7), np.arange(7) * 3, np.arange(7) * 11
    assert np.array_equal(A.hash4(99, a, b, c), hash4_np(99, a, b, c))
    m = A.head_masks(1234, [5, 2], 8, 0.5)
    assert np.array_equal(m[0].numpy(), dropout_keep(1234, 2, 8, 256, 0.5, 0, [5, 2]))
    assert np.array_equal(m[1].numpy(), dropout_keep(1234, 2, 8, 64, 0.5, 1, [5, 2]))
    assert 0.4 < float(m[0].float().mean()) < 0.6


@pytest.mark.parametrize("kind,keep", [("int", 1.0), ("zero", 1.0), ("int", 0.5)])
def test_head_reference_matches_fp64_autograd(kind, keep):
    c = A.head_case(kind, A.HEAD_G, 8)
    masks = A.head_masks(1234, [5, 2], c.B, keep) if keep < 1 else None
    r = A.head_ref(c, True, keep, masks)
    if kind == "zero":
        assert float(r.logits.abs().max()) == 0.0 and float(r.dp5.abs().max()) > 0
        for k in ("w1", "b1", "w2"):
            assert float(r.g[k].abs().max()) > 0
            assert torch.equal(r.g[k].float().double(), r.g[k])              # exact in fp32
    else:
        assert float(r.logits.abs().max()) > 0 and float(r.logits.abs().max()) < 40
        assert torch.equal(r.logits, r.logits.round())
    for g in range(c.G):
        sl = slice(g * c.B, (g + 1) * c.B)
        p5 = c.p5[sl].double().requires_grad_(True)
        w1, b1 = c.w1[g].clone().requires_grad_(True), c.b1[g].clone().requires_grad_(True)
        w2, b2 = c.w2[g].clone().requires_grad_(True), c.b2[g:g + 1].clone().requires_grad_(True)
        f = p5.permute(0, 2, 1).reshape(c.B, A.HF)
        if masks is not None:
            f = f * masks[0][g].double() / keep
        h = torch.relu(F.linear(f, w1, b1))
        if masks is not None:
            h = h * masks[1][g].double() / keep
        z = F.linear(h, w2.view(1, -1), b2).view(-1)
        loss = F.binary_cross_entropy_with_logits(z, c.y[sl].double())
        loss.backward()
        assert torch.equal(z.detach(), r.logits[g]) and abs(float(loss.detach()) - float(r.loss[g])) < 1e-14
        for k, v in (("w1", w1.grad.view(-1)), ("b1", b1.grad), ("w2", w2.grad), ("b2", b2.grad)):
            assert float((v - r.g[k][g]).abs().max()) < 1e-14, k
        assert float((p5.grad - r.dp5[sl]).abs().max()) < 1e-14
    assert A.DEV_REL < 2.0 ** -20


@pytest.mark.parametrize("case", A.CLS_CASES, ids=str)
def test_cls_reference_matches_fp64_autograd(case):
    HW, C, K, B, exact = case
    c = A.cls_case(*case)
    assert C % 2 == 0 and c.off_w % 2 == 0 and c.ld % 2 == 0
    if exact:
        assert K & (K - 1) == 0 and B & (B - 1) == 0 and float(c.z.abs().max()) == 0.0
        assert torch.equal(c.dlog.float().double(), c.dlog) and torch.equal(c.dW.float().double(), c.dW)
        assert K == 1 or float(c.dW.abs().max()) > 0
    else:
        assert torch.equal(c.z, c.z.round()) and len(c.z.unique()) > 3
    for g in range(c.G):
        sl = slice(g * B, (g + 1) * B)
        a = c.a[sl].double().requires_grad_(True)
        W, b = c.W[g].clone().requires_grad_(True), c.bias[g].clone().requires_grad_(True)
        z = F.linear(a.mean(1), W, b)
        loss = F.cross_entropy(z, c.y[sl])
        loss.backward()
        assert abs(float(loss.detach()) - float(c.losses[g])) < 1e-12
        assert float((W.grad.view(-1) - c.dW[g]).abs().max()) < 1e-12 and float((b.grad - c.db[g]).abs().max()) < 1e-12
        assert float((a.grad - c.da[sl]).abs().max()) < 1e-12


# ================================================================================================ mutations
def test_mutation_swapped_taps_in_one_channel():
    """Two taps of one tap group swapped in one channel of the packed weights: the pooled output stays inside the old
    relative-norm threshold (1e-2 per client against fp64), the bit comparison names the channel."""
    c = A.conv1_case()
    g, ch = 0, 4                                   # a live channel of small scale (k = 10): the norm hardly sees it
    assert int(c.kexp[g, ch]) == 10 and not bool(c.dead[ch])
    s = A.c1_slots(0)
    k1, k2 = A.tp_to_k(*s[8]), A.tp_to_k(*s[9])                    # tap group 1, phases 0 and 1
    w = c.w.clone()
    assert w[g, ch, k1] != w[g, ch, k2]
    w[g, ch, [k1, k2]] = w[g, ch, [k2, k1]]
    acc = c.acc.clone()
    acc[:c.B, ch] = A.conv1_acc(A.volumes(), (w * c.sign.unsqueeze(2))[:, ch:ch + 1].expand(-1, A.C1, -1).contiguous(),
                                c.idx[:c.B], c.B)[:, 0]
    out, amax, _ = A.conv1_pool_ref(acc, c.mult, c.shift, c.B)
    old = _relerr(out[:c.B].float(), c.out[:c.B].float())
    print("alexlattice mutation swapped taps: old relative norm %.3g (threshold 1e-2)" % old)
    assert 0 < old < 1e-2
    with pytest.raises(AssertionError, match=r"output bits.*channel=%d\)" % ch):
        A.check_conv1_fwd(out, amax, c)


def test_mutation_argmax_flipped_to_a_tied_neighbour():
    c = A.conv1_case()
    n = c.idx.tolist().index(1)
    ch = int(torch.nonzero(c.out[n, 0, 0, 0].float() > 0)[0])
    amax = c.amax.clone()
    assert int(amax[n, 0, 0, 0, ch]) == 26
    amax[n, 0, 0, 0, ch] = 25                                      # a tied candidate of the all-zero window
    assert float((amax != c.amax).float().mean()) < 1e-3           # the older mode-comparison threshold
    with pytest.raises(AssertionError, match=r"argmax.*sample=%d, pd=0, ph=0, pw=0, channel=%d\)" % (n, ch)):
        A.check_conv1_fwd(c.out, amax, c)


def test_mutation_dropped_cell_in_the_weight_gradient():
    w = A.wgrad_case()
    dz = A.wgrad_dz(w.dp, w.pout)
    cell = tuple(int(v) for v in torch.nonzero(dz[1] != 0)[1000])
    S1, D1 = A.wgrad_sums(w.dp[1:2], w.pout[1:2], w.amax[1:2], w.idx[1:2], drop=(0,) + cell)
    S = w.S.clone()
    S[1] = S1[0]
    Sc, _ = A.wgrad_client(S, w.D, w.B)
    Sr, _ = A.wgrad_client(w.S, w.D, w.B)
    old = _relerr(Sc[0], Sr[0])
    print("alexlattice mutation dropped cell: old relative norm %.3g (threshold 2e-2)" % old)
    assert 0 < old < 2e-2
    e = A.first_mismatch(Sc, Sr, ("client", "channel", "tap"))
    assert e is not None and "client=0, channel=%d," % cell[3] in e
    assert float(D1[0, cell[3]]) != float(w.D[1, cell[3]])


def test_mutation_dropped_block_partial_in_bn_finalize():
    c = A.bn_fin_case(130, 64, True, 192, 1)
    mean, var, n = A.chan_merge(c.stats, c.nb, skip=17)
    good = A.bn_fin_ref(c, c.mean, c.var, float(c.Mg), 0.0)
    bad = A.bn_fin_ref(c, mean, var, n, 0.0)
    for k in ("scale", "shift"):
        old = NL.relnorm(getattr(bad, k), getattr(good, k))
        print("alexlattice mutation dropped block: old relative norm of %s %.3g (threshold 3e-2)" % (k, old))
        assert old < 3e-2
    with pytest.raises(AssertionError, match="client=0, channel="):
        L.assert_exact(bad.invstd.float(), good.invstd, ("client", "channel"))
    with pytest.raises(AssertionError):
        NL.assert_ulp(bad.invstd.float(), good.invstd, 2, ("client", "channel"))


def test_mutation_wrong_dropout_stream_for_layer_2():
    """Layer 2 hashed with layer 1's stream: the logits move at the first sample whose hidden mask differs.  (The logits
    move by O(1), so this corruption is caught by the older whole-step threshold too; only the index is new.)"""
    c = A.head_case("int", A.HEAD_G, 8)
    good = A.head_ref(c, True, 0.5, A.head_masks(1234, [5, 2], c.B, 0.5))
    bad = A.head_ref(c, True, 0.5, A.head_masks(1234, [5, 2], c.B, 0.5, layer2_seed=1234))
    first = int(torch.nonzero((good.logits != bad.logits).view(-1))[0])
    with pytest.raises(AssertionError, match=r"first at \(sample=%d\)" % first):
        L.assert_exact(bad.logits.view(-1), good.logits.view(-1), ("sample",))
