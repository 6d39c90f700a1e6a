"""Bit-exact tests of the optimizer kernels (``optim.hip``: ``clip_sgd_mask``, ``local_opt``, ``local_opt_pack``,
``local_opt_pack_wt``), the SNIP selection kernels (``select.hip``) and the row aggregation kernels
(``weighted_rows_sum``, ``broadcast_row``, ``masked_rows_sum``, ``masked_mean_rows``, ``mix_rows``, ``pair_sqdist``)
against the fp64 references of ``tests/_rowlattice.py``.

On the dyadic lattice every comparison is on bit patterns: fp32 results against the reference's fp32 bit patterns
(the sign of a zero included), the bf16 images against the reference rounded to bf16.  Every row buffer comes from
``padded_rows`` with NaN in the columns [P, ld), compared bitwise after the call: a pad column read into a norm
poisons the row, a write shows.  The only tolerance is the counted bound of
the non-dyadic coefficient case (``K_COEF`` / ``K_GRAD`` in the helper).

Selection domain: finite non-negative fp32 including +0.0 and denormals, and +inf; negative values and NaN are out
of scope (the radix select orders the bit patterns as unsigned integers)."""
import numpy as np
import pytest
import torch

import _lattice as L
import _normlattice as NL
import _rowlattice as RL

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
AX = ("client", "element")


def _m():
    from neuroimagedisttraining_amd import ops
    return ops.ext()


def _st():
    from neuroimagedisttraining_amd import ops
    return ops.stream()


def _engine():
    from neuroimagedisttraining_amd.engine.executor import HipEngine
    eng = HipEngine.__new__(HipEngine)
    eng.m = _m()
    return eng


class Rows:
    """``padded_rows`` filled with ``vals`` [C, P] (numpy fp64, or None: NaN everywhere) and NaN in the pad columns."""

    def __init__(self, vals, C=None, P=None):
        from neuroimagedisttraining_amd.engine.executor import padded_rows
        if vals is not None:
            C, P = vals.shape
        self.t = padded_rows(C, P, DEV)
        self.full = self.t._base
        assert self.full is not None and self.full.shape[1] % 64 == 0 and self.t.data_ptr() % 16 == 0
        self.full.fill_(NAN)
        if vals is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(vals)).float())
        self.P = P
        self.before = self.full.clone()

    def pad_untouched(self):
        return torch.equal(self.full[:, self.P:].view(torch.int32), self.before[:, self.P:].view(torch.int32))

    def unchanged(self):
        return torch.equal(self.full.view(torch.int32), self.before.view(torch.int32))


def _exact(got, ref, names=AX, what=""):
    """Device fp32 ``got`` equals the fp64 numpy reference bit for bit (the reference holds fp32 values only, so its
    cast to fp32 is exact; the sign of a zero counts).  ``what`` names the configuration in a failure."""
    r = torch.from_numpy(np.ascontiguousarray(ref))
    r32 = r.float().to(got.device).reshape(got.shape)
    if torch.equal(got.contiguous().view(torch.int32), r32.contiguous().view(torch.int32)):
        return
    try:
        L.assert_exact(got, r, names)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None
    try:  # equal values, other bits: the sign of a zero
        RL.assert_bits(got.contiguous().view(torch.int32), r32.contiguous().view(torch.int32), names)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None


def _spec(c, dev_ref, dev_pref, bits):
    from neuroimagedisttraining_amd.engine.runner import StepSpec
    cfg = c.cfg

    def row(r):
        return r.t[0] if r.t.shape[0] == 1 else r.t
    return StepSpec(mask_mode=cfg.mode, bits=bits, shared=cfg.shared, prox_mu=RL.MU if cfg.mu else 0.0,
                    ref=row(dev_ref) if cfg.mu else None, lamda=RL.LAMDA if cfg.lamda else 0.0,
                    pref=row(dev_pref) if cfg.lamda else None)


def _run_local_opt(c, call):
    """Upload the case, run ``call(theta, grads, mom_buf, spec, momentum, lr, lr_dev)``, compare w, g, buf and every
    pad column with the reference."""
    cfg = c.cfg
    w, g, buf, ref, pref = Rows(c.w), Rows(c.g), Rows(c.buf), Rows(c.ref), Rows(c.pref)
    bits = c.bits.to(DEV) if c.bits is not None else None
    bits0 = bits.clone() if bits is not None else None
    spec = _spec(c, ref, pref, bits)
    lr_dev = torch.tensor([RL.LR], dtype=torch.float32, device=DEV) if cfg.lr_dev else None
    call(w.t, g.t, buf.t, spec, RL.MOM if cfg.mom else 0.0, 0.8125 if cfg.lr_dev else RL.LR, lr_dev)
    torch.cuda.synchronize()
    _exact(w.t, c.w1, what="w of %r" % (cfg,))
    if cfg.keep_grad:
        _exact(g.t, c.g1, what="g of %r" % (cfg,))
    else:
        assert g.unchanged(), "keep_grad = 0: the gradient rows changed: %r" % (cfg,)
    if cfg.mom:
        _exact(buf.t, c.buf1, what="buf of %r" % (cfg,))
    else:
        assert buf.unchanged(), "momentum 0: the momentum rows changed: %r" % (cfg,)
    for name, r in (("w", w), ("g", g), ("buf", buf)):
        assert r.pad_untouched(), "a pad column [P, ld) of %s was written: %r" % (name, cfg)
    assert ref.unchanged() and pref.unchanged() and (bits is None or torch.equal(bits, bits0)), \
        "an input (ref, pref or the mask bits) was written: %r" % (cfg,)
    return w


# ------------------------------------------------------------------------------------------------ local_opt
@pytest.mark.parametrize("P,i", [(P, i) for P in RL.OPT_P for i in range(len(RL.opt_cfgs(P)))])
def test_local_opt_exact(P, i):
    """mask_mode 0/1/2 x shared / per-row bits x momentum x FedProx x Ditto x shared / per-row references x clipped /
    unclipped x keep_grad x lr_dev (pairwise-covering; the full flag product at P = 8197), rows with different clip
    coefficients, bit for bit on w, g and buf."""
    eng = _engine()
    cfg = RL.opt_cfgs(P)[i]
    c = RL.opt_case(cfg)
    _run_local_opt(c, lambda th, gr, mb, spec, mom, lr, lr_dev: eng.local_opt(
        th, gr, mb, spec, lr, RL.WD, mom, c.max_norm, lr_dev=lr_dev, keep_grad=cfg.keep_grad))


@pytest.mark.parametrize("P,i", [(P, i) for P in RL.OPT_P_BIG for i in range(2)])
def test_local_opt_exact_large(P, i):
    """nblk = 258 (second trip of the partial re-reduction loop) and the rescaled chunk of opt_chunk (8196 x 1024)."""
    eng = _engine()
    cfg = RL.opt_cfgs(P)[i]
    c = RL.opt_case(cfg)
    assert RL.opt_chunk(P)[1] > RL.OPT_THREADS
    _run_local_opt(c, lambda th, gr, mb, spec, mom, lr, lr_dev: eng.local_opt(
        th, gr, mb, spec, lr, RL.WD, mom, c.max_norm, lr_dev=lr_dev, keep_grad=cfg.keep_grad))


def test_local_opt_without_rows_launches_nothing():
    m = _m()
    c = RL.opt_case(RL.opt_cfgs(1027)[0])
    w, g, buf = Rows(c.w), Rows(c.g), Rows(c.buf)
    m.local_opt(w.t.data_ptr(), g.t.data_ptr(), buf.t.data_ptr(), w.t.stride(0), 0, 0, 0, 0, 0, 0.0, 0, 0, 0.0, 0, 0,
                c.P, RL.LR, RL.WD, RL.MOM, 1.0, 0, 1, _st())
    torch.cuda.synchronize()
    assert w.unchanged() and g.unchanged() and buf.unchanged()


# ------------------------------------------------------------------------------------------------ clip_sgd_mask
@pytest.mark.parametrize("P,i", [(P, i) for P in RL.CSM_P for i in range(len(RL.csm_cfgs(P)))])
def test_clip_sgd_mask_exact(P, i):
    """All eight instantiations (float mask, momentum, bf16 emission) x first 0 / 1 (first: NaN in buf is ignored) at
    every P of the optimizer table, coef_out equal to the row's power of two, wbf equal to the reference rounded to
    bf16 bit for bit."""
    m = _m()
    cfg = RL.csm_cfgs(P)[i]
    c = RL.csm_case(cfg)
    w, g = Rows(c.w), Rows(c.g)
    buf = Rows(None if (cfg.first and cfg.mom) else c.buf, c.C, P)
    ld = w.t.stride(0)
    mask = torch.from_numpy(c.mask).float().to(DEV) if cfg.mask else None
    ws = torch.full((m.clip_sgd_mask_workspace(c.C, P),), NAN, device=DEV)
    coef = torch.full((c.C,), NAN, device=DEV)
    wbf = torch.full((c.C, ld), 0x7fc1, dtype=torch.int16, device=DEV)
    lr_dev = torch.tensor([RL.LR], dtype=torch.float32, device=DEV) if cfg.lr_dev else None
    # without momentum: either no buffer, or a buffer with momentum 0 (both take the kernel without momentum)
    buf_ptr = buf.t.data_ptr() if (cfg.mom or cfg.first) else 0
    mom = RL.MOM if (cfg.mom or not cfg.first) else 0.0
    m.clip_sgd_mask(w.t.data_ptr(), g.t.data_ptr(), buf_ptr, mask.data_ptr() if cfg.mask else 0, ws.data_ptr(),
                    coef.data_ptr(), wbf.data_ptr() if cfg.wbf else 0, c.C, P, ld, 0.8125 if cfg.lr_dev else RL.LR,
                    RL.WD, mom, int(cfg.first), c.max_norm, lr_dev.data_ptr() if cfg.lr_dev else 0,
                    int(cfg.keep_grad), _st())
    torch.cuda.synchronize()
    _exact(coef, c.coef, ("client",), "coef_out of %r" % (cfg,))
    _exact(w.t, c.w1, what="w of %r" % (cfg,))
    if cfg.keep_grad:
        _exact(g.t, c.g1, what="g of %r" % (cfg,))
    else:
        assert g.unchanged(), "keep_grad = 0: the gradient rows changed: %r" % (cfg,)
    if cfg.mom:
        _exact(buf.t, c.buf1, what="buf of %r" % (cfg,))
    else:
        assert buf.unchanged(), "no momentum: the momentum rows changed: %r" % (cfg,)
    for name, r in (("w", w), ("g", g), ("buf", buf)):
        assert r.pad_untouched(), "a pad column [P, ld) of %s was written: %r" % (name, cfg)
    if cfg.wbf:
        RL.assert_bits(wbf[:, :P], c.wbf, AX)
        assert bool((wbf[:, P:] == 0x7fc1).all()), "a pad column of wbf was written: %r" % (cfg,)
    else:
        assert bool((wbf == 0x7fc1).all()), "wbf = 0: the bf16 rows were written: %r" % (cfg,)


# ------------------------------------------------------------------------------------------------ fused pack
def _packer(G):
    from neuroimagedisttraining_amd.engine.resnet2d_hip import GroupedConv, WeightPacker
    layers, P = RL.pack_layout()
    convs = [GroupedConv(off, cout, cin, k, 1, (k - 1) // 2, True) for off, cout, cin, k in layers]
    pk = WeightPacker(convs, DEV)
    pk._plan(G, True)
    return pk, convs, layers, P


@pytest.mark.parametrize("i,wt", [(i, wt) for i in range(len(RL.PACK_MODES)) for wt in (False, True)])
def test_local_opt_pack_exact(i, wt):
    """k_local_step_pack / k_local_step_pack_wt on a synthetic layout (stem 3 -> 64 k3, 64 -> 64 k3, 64 -> 128 k1, 128
    -> 64 k3 at unaligned offsets, other parameter ranges of 5, 1, 3, 67 and 4099 floats) under weight / gradient masks,
    FedProx and Ditto, clipped: w, g, buf equal the fp64 reference of the plain step, the forward images equal the
    reference rounded to bf16 in [G, Cout, kt, Cin_p] (zero in the padded channels), and with wt the data-gradient
    images in [G, Cin_p, slot(t), Cout] too.  Both image sets come from the reference, not from pack.hip."""
    eng = _engine()
    c = RL.pack_case(RL.PACK_MODES[i])
    cfg = c.cfg
    pk, convs, layers, P = _packer(c.C)
    assert P == c.P
    plan = pk.fused_plan((c.C, True), P, wt)
    img = plan[6]
    img.view(torch.int16).fill_(0x7fc1)
    _run_local_opt(c, lambda th, gr, mb, spec, mom, lr, lr_dev: eng.local_opt_pack(
        th, gr, mb, spec, lr, RL.WD, mom, c.max_norm, plan, lr_dev=lr_dev, keep_grad=cfg.keep_grad, wt=wt))
    exp = RL.pack_images(c.w1, layers, lambda li: convs[li].slots)
    views = pk._plans[(c.C, True)][5]
    for li, ((vp, vt), (fwd, tr)) in enumerate(zip(views, exp)):
        got = img[vp[0]:vp[0] + fwd.numel()].view(torch.int16)
        RL.assert_bits(got, fwd.view(torch.int16), ("client", "cout", "tap", "cin"))
        if vt is None:
            assert li == 0                       # the channel-padded stem has no data-gradient image
            continue
        got = img[vt[0]:vt[0] + tr.numel()].view(torch.int16)
        if wt:
            RL.assert_bits(got, tr.view(torch.int16), ("client", "cin", "slot", "cout"))
        else:
            assert bool((got == 0x7fc1).all()), "the plain fused step wrote a data-gradient image"


# ------------------------------------------------------------------------------------------------ non-dyadic coefficient
@pytest.mark.parametrize("P", RL.COEF_P)
def test_clip_coefficient_within_counted_bound(P):
    """Random normal gradients: coef_out of clip_sgd_mask and the clipped gradient written back by clip_sgd_mask and by
    local_opt against fp64, per element, within K 2^-24 |ref| (K counted in the helper, not measured)."""
    m = _m()
    c = RL.coef_case(P)
    w, g = Rows(c.w.double().numpy()), Rows(c.g.double().numpy())
    ws = torch.full((m.clip_sgd_mask_workspace(c.C, P),), NAN, device=DEV)
    coef = torch.full((c.C,), NAN, device=DEV)
    m.clip_sgd_mask(w.t.data_ptr(), g.t.data_ptr(), 0, 0, ws.data_ptr(), coef.data_ptr(), 0, c.C, P, w.t.stride(0),
                    RL.LR, RL.WD, 0.0, 1, RL.COEF_MAX_NORM, 0, 1, _st())
    torch.cuda.synchronize()
    r1 = NL.assert_within(coef, c.coef, c.coef_bound, ("client",))
    r2 = NL.assert_within(g.t, c.g1, c.g1_bound, AX)
    assert g.pad_untouched() and w.pad_untouched()
    from neuroimagedisttraining_amd.engine.runner import StepSpec
    w2, g2 = Rows(c.w.double().numpy()), Rows(c.g.double().numpy())
    _engine().local_opt(w2.t, g2.t, None, StepSpec(), RL.LR, RL.WD, 0.0, RL.COEF_MAX_NORM, keep_grad=True)
    torch.cuda.synchronize()
    r3 = NL.assert_within(g2.t, c.g1, c.g1_bound, AX)
    print("P %d: err / bound coef %.3f, gradient %.3f (clip_sgd_mask), %.3f (local_opt)" % (P, r1, r2, r3))


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("n", RL.SELECT_N)
@pytest.mark.parametrize("name", RL.SELECT_SETS)
def test_radix_select_and_threshold_mask_exact(name, n):
    """The threshold bits equal the k-th largest bit pattern and mask == (v >= thr), for k in {1, 2, n/2, n - 1, n} and
    every rank at which a tie group starts or ends.  Both references are formed on the host from the uint32 bit
    patterns (for non-negative floats the unsigned order is the float order), so no device comparison, and no
    denormal handling of one, enters them."""
    m = _m()
    bits = RL.select_data(name, n)
    v = torch.from_numpy(bits.view(np.float32).copy()).to(DEV)
    st = torch.empty(4, dtype=torch.int32, device=DEV)
    hist = torch.empty(256, dtype=torch.int32, device=DEV)
    mask = torch.empty(n + 64, device=DEV)
    ks = RL.select_ranks(bits)
    got = []
    for k in ks:
        ref = RL.kth_largest_bits(bits, k)
        m.radix_select_kth(v.data_ptr(), n, k, st.data_ptr(), hist.data_ptr(), _st())
        got.append(st[3:4].clone())
        mask.fill_(NAN)
        m.threshold_mask(v.data_ptr(), n, st.data_ptr(), mask.data_ptr(), _st())
        exp = torch.from_numpy((bits >= np.uint32(ref)).astype(np.float32)).to(DEV)   # uint32 order, on the host
        assert torch.equal(mask[:n].view(torch.int32), exp.view(torch.int32)), (k, hex(ref))
        assert bool(torch.isnan(mask[n:]).all())
    got = torch.cat(got).cpu().numpy().view(np.uint32)
    exp = np.array([RL.kth_largest_bits(bits, k) for k in ks], dtype=np.uint32)
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, "k = %d: threshold 0x%08x, k-th largest 0x%08x" % (ks[bad[0]], got[bad[0]], exp[bad[0]])


@pytest.mark.parametrize("name,n", [("five_ties", 4099), ("denormals", 257)])
def test_topk_wrappers_exact(name, n):
    from neuroimagedisttraining_amd.ops import library, topk  # noqa: F401  (registers torch.ops.nidt.*)
    bits = RL.select_data(name, n)
    v = torch.from_numpy(bits.view(np.float32).copy()).to(DEV)
    for k in RL.select_ranks(bits):
        ref = RL.kth_largest_bits(bits, k)
        assert int(topk.kth_largest(v, k).view(torch.int32)) == ref
        assert int(torch.ops.nidt.kth_largest(v, k).view(torch.int32)) == ref
        exp = torch.from_numpy((bits >= np.uint32(ref)).astype(np.float32)).to(DEV)
        assert torch.equal(topk.threshold_mask(v, k).view(torch.int32), exp.view(torch.int32)), k
    for k in (0, n + 1):
        with pytest.raises(ValueError, match="k out of range"):           # the wrapper's own check
            topk.kth_largest(v, k)
        with pytest.raises(ValueError, match="k out of range"):           # the same check through the custom op
            torch.ops.nidt.kth_largest(v, k)
        st = torch.zeros(4, dtype=torch.int32, device=DEV)
        hist = torch.zeros(256, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError, match="1 <= k <= n"):               # NIDT_REQUIRE: std::invalid_argument
            _m().radix_select_kth(v.data_ptr(), n, k, st.data_ptr(), hist.data_ptr(), _st())


@pytest.mark.parametrize("n", RL.SELECT_N)
def test_mask_stats_exact(n):
    """Non-zero count and Hamming distance with != 0 semantics: -0.0 counts as zero, NaN as non-zero; b = 0: no second
    mask."""
    m = _m()
    rng = RL.rng_of("mask_stats", n)
    vals = np.array([0.0, -0.0, 1.0, NAN, 0.5, 1.0, 0.0], dtype=np.float32)
    a, b = rng.choice(vals, size=n), rng.choice(vals, size=n)
    out = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    da, db = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    with np.errstate(invalid="ignore"):
        nz, hd = int((a != 0).sum()), int(((a != 0) != (b != 0)).sum())
    m.mask_stats(da.data_ptr(), db.data_ptr(), n, out.data_ptr(), _st())
    assert out.tolist() == [nz, hd]
    m.mask_stats(da.data_ptr(), 0, n, out.data_ptr(), _st())
    assert out.tolist() == [nz, 0]
    m.mask_stats(db.data_ptr(), da.data_ptr(), n, out.data_ptr(), _st())
    with np.errstate(invalid="ignore"):
        assert out.tolist() == [int((b != 0).sum()), hd]


@pytest.mark.parametrize("P", (1, 255, 257, 8197))
def test_saliency_acc_exact(P):
    """score += |theta grad| alpha on the lattice (alpha = 2^-1, a non-zero starting score, a score row stride that
    differs from the rows'), pad columns of every buffer untouched."""
    from neuroimagedisttraining_amd.engine.executor import padded_rows
    G = 3
    theta, grad = RL.int_rows(G, P, -8, 8, "sal theta"), RL.int_rows(G, P, -2, 2, "sal grad")
    s0 = RL.int_rows(G, P, 0, 9, "sal score") / 2
    th, gr = Rows(theta), Rows(grad)
    full = padded_rows(G, P + 70, DEV)._base
    full.fill_(NAN)
    score = full[:, :P]
    score.copy_(torch.from_numpy(s0).float())
    assert score.stride(0) != th.t.stride(0)
    before = full.clone()
    _engine().saliency_acc(th.t, gr.t, score, 0.5)
    torch.cuda.synchronize()
    _exact(score, s0 + np.abs(theta * grad) * 0.5)
    assert torch.equal(full[:, P:].view(torch.int32), before[:, P:].view(torch.int32))
    assert th.unchanged() and gr.unchanged()


# ------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("n", RL.ROW_N)
@pytest.mark.parametrize("C", (1, 5))
def test_weighted_rows_sum_exact(C, n):
    """beta = 0 ignores a NaN-filled output; beta = 2^-1 accumulates; nothing is written past n."""
    m = _m()
    rows = RL.int_rows(C, n, -8, 8, "wrs")
    wts = np.array(RL.ROW_WEIGHTS[:C])
    r = Rows(rows)
    w = torch.tensor(wts, dtype=torch.float32, device=DEV)
    out = torch.full((n + 8,), NAN, device=DEV)
    m.weighted_rows_sum(r.t.data_ptr(), w.data_ptr(), C, n, r.t.stride(0), 0.0, out.data_ptr(), _st())
    ref = (wts[:, None] * rows).sum(0)
    _exact(out[:n], ref, ("element",))
    assert bool(torch.isnan(out[n:]).all())
    acc0 = RL.int_rows(1, n, -8, 8, "wrs acc")[0]
    out[:n].copy_(torch.from_numpy(acc0).float())
    m.weighted_rows_sum(r.t.data_ptr(), w.data_ptr(), C, n, r.t.stride(0), 0.5, out.data_ptr(), _st())
    _exact(out[:n], 0.5 * acc0 + ref, ("element",))
    assert bool(torch.isnan(out[n:]).all()) and r.unchanged()


@pytest.mark.parametrize("n", RL.ROW_N)
def test_broadcast_row_exact(n):
    m = _m()
    src = RL.int_rows(1, n, -8, 8, "bcast")
    s = Rows(src)
    d = Rows(None, 4, n)
    m.broadcast_row(s.t.data_ptr(), n, d.t.stride(0), 4, d.t.data_ptr(), _st())
    torch.cuda.synchronize()
    _exact(d.t, np.repeat(src, 4, 0))
    assert d.pad_untouched() and s.unchanged()


@pytest.mark.parametrize("n", RL.ROW_N)
def test_masked_rows_sum_exact(n):
    """Accumulates into non-zero sum / cnt, with per-row bits and with bits = None (every row counts)."""
    from neuroimagedisttraining_amd.engine import masks as MK
    R = 5
    rows = RL.int_rows(R, n, -8, 8, "mrs")
    mk = RL.mask_rows(R, n, RL.rng_of("mrs bits", n))
    s0, c0 = RL.int_rows(1, n, -8, 8, "mrs s")[0], RL.int_rows(1, n, 0, 3, "mrs c")[0]
    r = Rows(rows)
    for bits, cnt in ((RL.pack_bits_high(mk).to(DEV), mk.sum(0)), (None, np.full(n, R))):
        s, c = (torch.cat([torch.from_numpy(x).float(), torch.full((8,), NAN)]).to(DEV) for x in (s0, c0))
        MK.masked_rows_sum(r.t, n, bits, s, c)
        torch.cuda.synchronize()
        _exact(s[:n], s0 + rows.sum(0), ("element",))
        _exact(c[:n], c0 + cnt, ("element",))
        assert bool(torch.isnan(s[n:]).all()) and bool(torch.isnan(c[n:]).all())
    assert r.unchanged()


@pytest.mark.parametrize("n", RL.ROW_N)
def test_masked_mean_rows_exact(n):
    """Values are multiples of 60, so num / cnt is an integer for up to 6 neighbours; positions kept by no neighbour
    and positions whose own bit is off give 0."""
    from neuroimagedisttraining_amd.engine import masks as MK
    nei = (6, 1, 3)
    S = sum(nei)
    src = RL.int_rows(S, n, -8, 8, "mmr") * 60
    rng = RL.rng_of("mmr bits", n)
    sm, own = RL.mask_rows(S, n, rng), RL.mask_rows(len(nei), n, rng)
    s, d = Rows(src), Rows(None, len(nei), n)
    sb, ob = RL.pack_bits_high(sm).to(DEV), RL.pack_bits_high(own).to(DEV)
    plan, exp, k = [], [], 0
    for r, cnt in enumerate(nei):
        plan.append((d.t[r], ob[r], [(s.t[j], sb[j]) for j in range(k, k + cnt)]))
        num, den = (src[k:k + cnt] * sm[k:k + cnt]).sum(0), sm[k:k + cnt].sum(0)
        exp.append(np.where((den > 0) & own[r], num / np.maximum(den, 1), 0.0))
        k += cnt
    exp = np.stack(exp)
    assert np.array_equal(exp, np.round(exp))
    if n >= 1023:
        assert bool(((sm[6:7].sum(0) == 0) & own[1]).any()) and bool((~own[0] & (sm[:6].sum(0) > 0)).any())
    MK.masked_mean_rows(plan, n)
    torch.cuda.synchronize()
    _exact(d.t, exp)
    assert d.pad_untouched() and s.unchanged()


@pytest.mark.parametrize("n", RL.ROW_N)
def test_mix_rows_exact(n):
    """Uneven rowptr, an output row with no source (written as zeros) and negative weights."""
    from neuroimagedisttraining_amd.engine import masks as MK
    rows = RL.int_rows(5, n, -8, 8, "mix")
    r, out = Rows(rows), Rows(None, 3, n)
    w = RL.ROW_WEIGHTS
    terms = ([(0, w[0]), (3, w[1])], [], [(1, w[2]), (2, w[4]), (4, w[3]), (0, w[1])])
    MK.mix_rows([(out.t[i], [(r.t[j], x) for j, x in t]) for i, t in enumerate(terms)], n)
    torch.cuda.synchronize()
    exp = np.stack([sum((x * rows[j] for j, x in t), np.zeros(n)) for t in terms])
    _exact(out.t, exp)
    assert out.pad_untouched() and r.unchanged()


@pytest.mark.parametrize("n", RL.SQDIST_N)
def test_pair_sqdist_exact(n):
    """The fp64 sum of the fp32 block partials equals the exact integer (a pair of identical rows: 0), up to one past
    the 256-block cap."""
    from neuroimagedisttraining_amd.engine import masks as MK
    rows = RL.int_rows(5, n, -8, 8, "sqd")
    r = Rows(rows)
    pairs = [(0, 1), (2, 2), (4, 0)]
    L.require_fp32_exact(RL.pair_sqdist_chunks(n)[1] * 256.0, "pair_sqdist partial")
    d = MK.pair_sqdist([(r.t[a], r.t[b]) for a, b in pairs], n)
    exp = [float(((rows[a] - rows[b]) ** 2).sum()) for a, b in pairs]
    assert d.dtype == torch.float64 and d.cpu().tolist() == exp
    assert exp[1] == 0.0 and r.unchanged()
