"""Bit-exact and counted-bound tests of the AlexNet3D kernels against the fp64 references of tests/_alexlattice.py: the
fused conv1 forward, its BN statistics and weight gradient (conv1.hip), the BatchNorm-pool kernels (bn.hip,
bn_relu_apply) and the heads (head.hip).  The raw bindings are called, so the kernel under test is the one named.  Output,
partial and gradient buffers start as NaN (uint8 buffers as 255); gradient slices sit between filler columns that must
stay untouched.

Argmax rules.  The fused conv1 forward carries the window index in the 5 low mantissa bits of the accumulator: among
equal accumulators the LARGEST index dd 9 + dh 3 + dw wins when acc >= 0, the smallest when acc < 0.  bn_relu_pool
takes the FIRST maximum in (d, h, w) scan order (PyTorch's rule).  The two rules differ on ties; each is pinned here.

Exact (bit for bit, or equal as fp64 values): polyphase, patch moments, pack_conv1_w (w8 per slot, w125), conv1_fwd_pool in
both modes (and the two modes against each other, ties included), the part-slab sums S / D of conv1_wgrad in modes 0, 1, 2
at NB = 4 and NB = 256, the closed form of k_conv1_wgrad_fin (train and eval), every NIDT_C1* variant in a child process,
bn_relu_pool (values and argmax), bn_relu_apply, bn_bwd sums / eval-mode dy, bn_finalize and bn_eval with eps = 0, head
logits (eval, train, dropout), the zero-logit head gradients, cls_head_train with softmax 1 / K.
Bounded (counted fp32 roundings, _alexlattice.py): conv1_bnstats, the running statistics, train-mode bn_bwd dy (N = B D H W
is no power of two for the issue's shapes), bn_finalize / bn_eval with the real eps, head and cls gradients on non-zero
integer logits, the dropout backward (exact zeros where a mask drops).

Measured on an MI355X (largest err / bound per kernel; each test prints its own, every ratio above 1 fails).  Where the
result is stored in bf16, or the bound is one fp32 rounding, the ratio sits just below 1 by construction.
    conditioning of var in M / N - mu mu^T (direct vs moment form, fp64, CPU): 9.2e-16 relative; bound uses 4 x that
    conv1_bnstats: invstd 0.976, scale 0.488, shift 0.547, mean 0.985, mu 0.687, covw 0.999, running mean 0.429, var 0.409
    bn_bwd (train): dy 0.9999, Bc / Cc 0.50 ulp (bound 1 ulp)
    bn_finalize (real eps): invstd 0.47 ulp, scale 0.47 ulp (bound 2 ulp), shift 0.241, running mean 0.339, var 0.368
    bn_eval (real eps): invstd 1.24 ulp (bound 2), scale 1.24 ulp (bound 3), shift 0.295
    head: device term of sigma(z) - y through db2 (at B = 1 it is dz2 itself): 0.217 x 2^-24 of its terms at B = 1, 0.271
          at worst over the cases (DEV_REL = 4 x 0.271); with K_HEAD = 8: dw1 0.165, db1 0.076, dw2 0.097, db2 0.030,
          dp5 0.968 (bf16), loss 0.078; under dropout dw1 0.082, dw2 0.080, dp5 0.302, loss 0.057
    cls_head_train (K = 10): dlog 0.077, dW 0.138, db 0.098, da 0.903 (bf16), lossn 0.044, losses 0.028
Wall time of this file on an MI355X: 151 tests in 20.9 s (slowest: a variant child, 2.5 s; slowest in-process case 0.9 s);
tests/test_gpu_kernels.py on the same machine: 122 tests in 22.1 s.
No kernel bug found: every kernel and every variant met its exact or counted check on the first run.
"""
import os
import subprocess
import sys

import pytest
import torch

import _alexlattice as A
import _alexlattice_child as R
import _lattice as L
import _normlattice as NL

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
_m = R.ext
_st = R._st


def _rec(family, ratio):
    print("alexlattice err/bound %s %.4f" % (family, ratio))
    assert ratio <= 1.0


def _rows_ok(rows, spans, what):
    keep = torch.ones(rows.shape[1], dtype=torch.bool)
    for off, n in spans:
        keep[off:off + n] = False
    assert bool((rows.cpu()[:, keep] == A.FILL).all()), what + ": a neighbouring column changed"


# ================================================================================================ conv1 operands
@pytest.fixture(scope="module")
def dev():
    """The three volumes in polyphase layout (polyphase binding, checked against the Python polyphase) and their moments."""
    from neuroimagedisttraining_amd.ops.reference import polyphase
    m = _m()
    vol = A.volumes().to(DEV)
    x8 = torch.full((3, 61, 73, 61, 8), 255, dtype=torch.uint8, device=DEV)
    mom = torch.full((3, 125 + 125 * 125), NAN, dtype=torch.float64, device=DEV)
    m.polyphase(vol.data_ptr(), x8.data_ptr(), 3, _st())
    m.conv1_sample_moments(x8.data_ptr(), 3, mom.data_ptr(), _st())
    torch.cuda.synchronize()
    assert torch.equal(x8, polyphase(vol))
    assert torch.equal(x8.cpu(), A.polyphase_ref(A.volumes()))
    return dict(x8=x8, mom=mom)


def test_conv1_sample_moments_exact(dev):
    e = A.first_mismatch(dev["mom"], A.moments_ref(), ("volume", "moment"))
    assert e is None, "patch moments must be exact integers: " + e


@pytest.mark.parametrize("scale_arg", [1.0 / 255.0, 1.0])
def test_pack_conv1_w_slots(scale_arg):
    """w8 slot by slot against the layout's definition (default process: 128 slots, original tap order), w125 exactly."""
    m, c = _m(), A.conv1_case()
    assert m.conv1_kslots() == 128
    w8, w125 = R.run_pack(m, c.theta.to(DEV), c.P, c.off_w, c.off_sign, c.G, scale_arg)
    torch.cuda.synchronize()
    r8, r125 = A.pack_ref(c, scale_arg)
    e = A.first_mismatch(w8, r8, ("client", "channel", "slot"))
    assert e is None, "packed f16 weights: " + e
    e = A.first_mismatch(w125.view(torch.int32), r125.view(torch.int32), ("client", "channel", "tap"))
    assert e is None, "w125 bits: " + e
    # without the sign row the same slots hold the unflipped weights
    w8n, _ = R.run_pack(m, c.theta.to(DEV), c.P, c.off_w, -1, c.G, scale_arg)
    e = A.first_mismatch(w8n, A.pack_ref(c, scale_arg, signed=False)[0], ("client", "channel", "slot"))
    assert e is None, "packed f16 weights, off_sign = -1: " + e


def _fwd(dev, mode):
    m, c = _m(), A.conv1_case()
    m.conv1_fwd_mode(mode)
    try:
        w8, _ = R.run_pack(m, c.theta.to(DEV), c.P, c.off_w, c.off_sign, c.G, 1.0 / 255.0)
        return R.run_fwd(m, dev["x8"], c.idx.to(DEV), w8, c.scale.to(DEV), c.shift.to(DEV), c.NB, c.B)
    finally:
        m.conv1_fwd_mode(-1)


@pytest.mark.parametrize("mode", [0, 1])
def test_conv1_fwd_pool_exact(dev, mode):
    """Output bits of the whole [4, 19, 23, 19, 64] tensor and the argmax bytes wherever the pooled value is > 0."""
    out, amax = _fwd(dev, mode)
    A.check_conv1_fwd(out, amax, A.conv1_case())


def test_conv1_fwd_modes_identical(dev):
    (o0, a0), (o1, a1) = _fwd(dev, 0), _fwd(dev, 1)
    e = A.first_mismatch(o0.view(torch.int16), o1.view(torch.int16), A.FWD_AXES)
    assert e is None, "pipe vs wave-tile output bits: " + e
    e = A.first_mismatch(a0, a1, A.FWD_AXES)
    assert e is None, "pipe vs wave-tile argmax bytes: " + e


# ================================================================================================ conv1 BN statistics
def _bnstats(dev, G, B, idx, w, upd, seed):
    m = _m()
    g = L.gen("alex", "bnstats", seed)
    theta_w = w.view(G, 8000).contiguous().to(DEV)
    _, w125 = R.run_pack(m, theta_w, 8000, 0, -1, G, 1.0)
    theta, off = A.bnstats_theta(G, g)
    bufs, boff = A.bnstats_bufs(G, g)
    th, bf = theta.to(DEV), bufs.to(DEV)
    o = {k: torch.full(s, NAN, device=DEV) for k, s in
         dict(scale=(G, 64), shift=(G, 64), mean=(G, 64), invstd=(G, 64), mu=(G, 125), covw=(G, 64, 125)).items()}
    Mb = torch.full((G, 125 + 125 * 125), NAN, dtype=torch.float64, device=DEV)
    idd = torch.as_tensor(idx, dtype=torch.int32).to(DEV)
    m.conv1_bnstats(dev["mom"].data_ptr(), idd.data_ptr(), B, G, Mb.data_ptr(), w125.data_ptr(), th.data_ptr(), off.P,
                    off.bias, off.g, off.b, bf.data_ptr(), boff.Q, boff.rm, boff.rv, boff.nbt, A.MOM, A.EPS, upd,
                    o["scale"].data_ptr(), o["shift"].data_ptr(), o["mean"].data_ptr(), o["invstd"].data_ptr(),
                    o["mu"].data_ptr(), o["covw"].data_ptr(), _st())
    torch.cuda.synchronize()
    return o, bf.cpu(), theta, off, bufs, boff


def _bnstats_check(o, bf, r, bufs, boff, upd, cond, tag):
    b = A.bnstats_bounds(r, cond)
    ax = ("client", "channel")
    for k in ("invstd", "scale", "shift", "mean"):
        _rec("conv1_bnstats %s %s" % (tag, k), NL.assert_within(o[k], getattr(r, k), getattr(b, k), ax))
    _rec("conv1_bnstats %s mu" % tag, NL.assert_within(o["mu"], r.mu, A.U32 * r.mu.abs() + 2.0 ** -40, ("client", "tap")))
    cb = A.U32 * r.covw.abs() + cond * r.covw.abs().amax(2, keepdim=True)
    _rec("conv1_bnstats %s covw" % tag, NL.assert_within(o["covw"], r.covw, cb, ("client", "channel", "tap")))
    if not upd:
        assert torch.equal(bf, bufs), "update_running = 0 changed the buffer row"
        return
    _rec("conv1_bnstats %s running mean" % tag, NL.assert_within(bf[:, boff.rm:boff.rm + 64], r.rm, b.rm, ax))
    _rec("conv1_bnstats %s running var" % tag, NL.assert_within(bf[:, boff.rv:boff.rv + 64], r.rv, b.rv, ax))
    assert torch.equal(bf[:, boff.nbt].double(), r.nbt)
    _rows_ok(bf, [(boff.rm, 64), (boff.rv, 64), (boff.nbt, 1)], "conv1_bnstats buffers")


@pytest.mark.parametrize("upd", [0, 1])
def test_conv1_bnstats_g2_direct(dev, upd):
    """G = 2 (one channel per block) against the mean / biased variance of the integer conv output itself."""
    c = A.conv1_case()
    o, bf, theta, off, bufs, boff = _bnstats(dev, c.G, c.B, c.idx, c.w, upd, "g2")
    mean, var = A.bnstats_direct(c)
    _, _, mu, covw = A.bnstats_moment_form(c.w, c.idx.tolist(), c.B)
    r = A.bnstats_from(mean, var, mu, covw, theta, off, bufs, boff, float(c.B * A.NPOS))
    _bnstats_check(o, bf, r, bufs, boff, upd, 4 * A.bnstats_cond(), "G=2")


@pytest.mark.parametrize("upd", [0, 1])
def test_conv1_bnstats_g32_moment_form(dev, upd):
    """G = 32, B = 1 (eight channels per block) against the moment form evaluated in fp64 from the exact moments."""
    G, idx, w = A.bnstats_g32()
    o, bf, theta, off, bufs, boff = _bnstats(dev, G, 1, idx, w, upd, "g32")
    mean, var, mu, covw = A.bnstats_moment_form(w, idx, 1)
    r = A.bnstats_from(mean, var, mu, covw, theta, off, bufs, boff, float(A.NPOS))
    _bnstats_check(o, bf, r, bufs, boff, upd, 4 * A.bnstats_cond(), "G=32")


# ================================================================================================ conv1 weight gradient
def _wg_dev(NB):
    """Device inputs of conv1_wgrad at NB samples: the NB = 4 case, or its period-4 extension with per-sample scales."""
    w = A.wgrad_case()
    if NB == 4:
        return w.idx.to(DEV), w.dp.to(DEV), w.pout.to(DEV), w.amax.to(DEV), None
    s = A.big_scales(NB)
    sel = (torch.arange(NB) % 4).to(DEV)
    sc = torch.tensor(s, dtype=torch.float32, device=DEV).view(NB, 1, 1, 1, 1)
    dp = (w.dp.to(DEV)[sel].float() * sc).bfloat16()
    return w.idx.to(DEV)[sel].contiguous(), dp, w.pout.to(DEV)[sel].contiguous(), w.amax.to(DEV)[sel].contiguous(), s


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("NB,B", [(A.C1_NB, A.C1_B), A.C1_BIG])
def test_conv1_wgrad_slab_sums_exact(dev, NB, B, mode):
    """The per-client fp64 sum of the part slabs equals the integer reference exactly: S (125 taps) and D."""
    m, w = _m(), A.wgrad_case()
    idx, dp, pout, amax, s = _wg_dev(NB)
    if NB == 4:
        assert m.conv1_wgrad_nq(NB) == 2 and m.conv1_wgrad_mx_npb(NB) == 1
    else:
        npb = m.conv1_wgrad_mx_npb(NB)
        assert m.conv1_wgrad_nq(NB) == 1 and npb > 1 and 19 % npb != 0
    S, D = A.wgrad_client(w.S, w.D, B, s)
    m.conv1_wgrad_mode(mode)
    try:
        part, _ = R.run_wgrad(m, dev["x8"], idx, dp, pout, amax, NB, B, A.fin_case(NB // B, False))
    finally:
        m.conv1_wgrad_mode(-1)
    R.check_slabs(part, NB // B, R.nslab(m, NB, B, mode), S, D, "mode %d NB %d" % (mode, NB))


@pytest.mark.parametrize("eval_mode", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_conv1_wgrad_closed_form_exact(dev, mode, eval_mode):
    """k_conv1_wgrad_fin on dyadic statistics: dW, dgamma, dbeta = D and dbias bit for bit, train and eval form."""
    m, w = _m(), A.wgrad_case()
    idx, dp, pout, amax, _ = _wg_dev(4)
    f = A.fin_case(w.G, eval_mode)
    ref = A.fin_ref(f, *A.wgrad_client(w.S, w.D, w.B))
    m.conv1_wgrad_mode(mode)
    try:
        _, grad = R.run_wgrad(m, dev["x8"], idx, dp, pout, amax, w.NB, w.B, f)
    finally:
        m.conv1_wgrad_mode(-1)
    grad = grad.cpu()
    _rows_ok(grad, f.spans, "conv1_wgrad gradient row")
    L.assert_exact(grad[:, f.goff_w:f.goff_w + 8000], ref["dW"].view(w.G, 8000), ("client", "weight"))
    for k, o in (("dbias", f.goff_bias), ("dgamma", f.goff_g), ("dbeta", f.goff_b)):
        L.assert_exact(grad[:, o:o + 64], ref[k], ("client", "channel"))


# ================================================================================================ environment variants
VARIANTS = [{"NIDT_C1_TAPORD": "1"}, {"NIDT_C1_TAPORD": "2"}, {"NIDT_C1_K224": "1"}, {"NIDT_C1_FWD": "0"},
            {"NIDT_C1WG_DOT": "1", "NIDT_C1WG_MX": "0"}, {"NIDT_C1WG_UNROLL": "4", "NIDT_C1WG_MX": "0"}]
CHILD_TIMEOUT = 10      # seconds: one measured child run takes 2.3 s (interpreter start, extension load, two checks);
                        # 3 x that is 7 s, rounded up
_child_fault = []       # a child that ended by signal or timeout: no further child is started


@pytest.fixture(scope="module")
def child_case(dev, tmp_path_factory):
    c, w = A.conv1_case(), A.wgrad_case()
    S, D = A.wgrad_client(w.S, w.D, w.B)
    path = tmp_path_factory.mktemp("alexlattice") / "case.pt"
    torch.save(dict(x8=dev["x8"].cpu(),
                    c=dict(G=c.G, B=c.B, NB=c.NB, P=c.P, off_w=c.off_w, off_sign=c.off_sign, idx=c.idx, theta=c.theta,
                           scale=c.scale, shift=c.shift, out=c.out, amax=c.amax),
                    w=dict(dp=w.dp, pout=w.pout, amax=w.amax, S=S, D=D)), path)
    return str(path)


@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_conv1_env_variant_in_child(child_case, env):
    """Each opt-in variant, selected by its environment variable in a fresh child process, passes the NB = 4 forward and
    slab checks."""
    assert not _child_fault, "an earlier variant child ended by signal or timeout (%s): not launching" % _child_fault[0]
    e = dict(os.environ)
    e.update(env)
    try:
        p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                         "_alexlattice_child.py"), child_case],
                           env=e, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _child_fault.append("%s: timeout" % env)
        raise AssertionError("variant child %s did not finish in %d s" % (env, CHILD_TIMEOUT))
    print(p.stdout[-2000:])
    if p.returncode < 0:
        _child_fault.append("%s: signal %d" % (env, -p.returncode))
    assert p.returncode == 0, "variant %s: exit %d\n%s\n%s" % (env, p.returncode, p.stdout[-2000:], p.stderr[-2000:])


# ================================================================================================ bn.hip
def _nan(*shape, dtype=torch.float32, guard=0):
    """NaN buffer; with guard > 0 its first axis gets that many extra sentinel rows (checked by _guard)."""
    b = torch.full((shape[0] + guard,) + tuple(shape[1:]), NAN, device=DEV, dtype=dtype)
    if guard:
        b[shape[0]:] = R.SENT
    return b


def _guard(n, *bufs):
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[n:].float() == R.SENT).all()), "rows behind the last sample / pair were written"


def _bits_equal(got, ref_bf16, names, what):
    e = A.first_mismatch(got.cpu().view(torch.int16), ref_bf16.contiguous().view(torch.int16), names)
    assert e is None, what + ": " + e


@pytest.mark.parametrize("G,B", A.BN_GB)
@pytest.mark.parametrize("shape", A.BN_SHAPES, ids=str)
def test_bn_relu_pool_exact(shape, G, B):
    """Value bits exact; the argmax is the first maximum in (d, h, w) scan order, ties and negative scales included."""
    m = _m()
    c = A.bn_pool_case(*shape, G, B)
    D, H, W, C = shape
    out = _nan(c.NB, D // 3, H // 3, W // 3, C, dtype=torch.bfloat16, guard=1)
    am = torch.full((c.NB + 1, D // 3, H // 3, W // 3, C), 255, dtype=torch.uint8, device=DEV)
    y, sc, sh = c.y.to(DEV), c.scale.to(DEV), c.shift.to(DEV)
    m.bn_relu_pool(y.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr(), am.data_ptr(), c.NB, B, D, H, W, C, _st())
    _guard(c.NB, out)
    assert bool((am[c.NB] == 255).all())
    _bits_equal(out[:c.NB], c.out, A.POOL_AXES, "bn_relu_pool output bits")
    e = A.first_mismatch(am[:c.NB], c.amax, A.POOL_AXES)
    assert e is None, "bn_relu_pool argmax (first maximum in scan order): " + e


@pytest.mark.parametrize("shape,gb,pool,ev,nchunk,convb", A.bn_bwd_cases(),
                         ids=lambda v: str(v).replace(" ", ""))
def test_bn_bwd_lattice(shape, gb, pool, ev, nchunk, convb):
    """sum dz, sum dz xhat and the conv-bias gradient exact; eval-mode dy exact in bf16; train-mode coefficients within 1
    ulp of their fp64 values and dy within half a bf16 ulp plus K_BN_BWD fp32 roundings (N is no power of two)."""
    m = _m()
    c = A.bn_bwd_case(shape, gb, pool, ev)
    D, H, W, C = shape
    G, B = gb
    ldg = 32 + 3 * C
    og, ob, oc = 8, 16 + C, 24 + 2 * C
    grad = torch.full((G, ldg), A.FILL, device=DEV)
    theta = torch.full((G, 16 + C), A.FILL, device=DEV)
    theta[:, 8:8 + C] = c.gamma.to(DEV)
    part = _nan(G * nchunk * C * 2)
    coef = _nan(G, C, 3)
    dy = _nan(c.NB, D, H, W, C, dtype=torch.bfloat16, guard=1)
    t = {k: getattr(c, k).contiguous().to(DEV) for k in ("y", "dsrc", "scale", "shift", "mean", "invstd")}
    pout = c.pout.to(DEV) if pool else None
    am = c.amax.to(DEV) if pool else None
    m.bn_bwd(pool, t["y"].data_ptr(), t["dsrc"].data_ptr(), pout.data_ptr() if pool else 0, am.data_ptr() if pool else 0,
             t["scale"].data_ptr(), t["shift"].data_ptr(), t["mean"].data_ptr(), t["invstd"].data_ptr(), c.NB, B, D, H, W,
             C, part.data_ptr(), nchunk, theta.data_ptr(), 16 + C, 8, grad.data_ptr(), ldg, og, ob, oc if convb else -1,
             coef.data_ptr(), dy.data_ptr(), ev, _st())
    _guard(c.NB, dy)
    grad = grad.cpu()
    _rows_ok(grad, [(og, C), (ob, C)] + ([(oc, C)] if convb else []), "bn_bwd gradient row")
    ax = ("client", "channel")
    L.assert_exact(grad[:, og:og + C], c.sdx, ax)
    L.assert_exact(grad[:, ob:ob + C], c.sdz, ax)
    if convb:
        L.assert_exact(grad[:, oc:oc + C], c.convb, ax)
    L.assert_exact(coef[:, :, 0], c.coef[:, :, 0], ax)
    tag = "bn_bwd pool=%d eval=%d" % (pool, ev)
    if ev:
        L.assert_exact(coef[:, :, 1:], c.coef[:, :, 1:], ax + ("coef",))
        _bits_equal(dy[:c.NB], c.dy.to(torch.bfloat16), A.DENSE_AXES, tag + " dy bits")
        return
    _rec(tag + " coef (ulp)", NL.assert_ulp(coef[:, :, 1:], c.coef[:, :, 1:], 1, ax + ("coef",)))
    bound = NL.bf16_bound(c.dy, A.K_BN_BWD * A.U32 * c.dy_terms)
    _rec(tag + " dy", NL.assert_within(dy[:c.NB], c.dy, bound, A.DENSE_AXES))


def _fin_run(c, eps, upd):
    m = _m()
    n = c.G * c.C
    o = {k: _nan(n, guard=8) for k in ("scale", "shift", "mean", "invstd")}
    st, th, bf = c.stats.float().contiguous().to(DEV), c.theta.to(DEV), c.bufs.to(DEV)
    m.bn_finalize(st.data_ptr(), c.nPB, c.BP, c.Mg, c.G, c.C, th.data_ptr(), c.ldt, c.off_g, c.off_b, bf.data_ptr(), c.ldb,
                  c.off_rm, c.off_rv, c.off_nbt, A.MOM, eps, o["scale"].data_ptr(), o["shift"].data_ptr(),
                  o["mean"].data_ptr(), o["invstd"].data_ptr(), upd, _st())
    _guard(n, *o.values())
    return {k: v[:n].view(c.G, c.C) for k, v in o.items()}, bf.cpu()


def _running_ok(c, bf, r, upd, tag):
    if not upd:
        assert torch.equal(bf, c.bufs), tag + ": update_running = 0 changed the buffer row"
        return
    ax = ("client", "channel")
    _rec(tag + " running mean", NL.assert_within(bf[:, c.off_rm:c.off_rm + c.C], r.rm, r.rm_bound, ax))
    _rec(tag + " running var", NL.assert_within(bf[:, c.off_rv:c.off_rv + c.C], r.rv, r.rv_bound, ax))
    assert torch.equal(bf[:, c.off_nbt].double(), r.nbt)
    _rows_ok(bf, [(c.off_rm, c.C), (c.off_rv, c.C), (c.off_nbt, 1)], tag + " buffers")


@pytest.mark.parametrize("upd", [0, 1])
@pytest.mark.parametrize("exact", [True, False], ids=["eps0", "eps"])
@pytest.mark.parametrize("case", A.BN_FIN, ids=str)
def test_bn_finalize_lattice(case, exact, upd):
    """Chan merge of dyadic partials whose total mean is an integer and total variance 4^-m.  eps0: eps = 0, so invstd =
    2^m and scale, shift, mean are exact.  eps: the real eps, invstd and scale within 2 ulp, shift within 4 roundings."""
    c = A.bn_fin_case(*case)
    eps = 0.0 if exact else A.EPS
    o, bf = _fin_run(c, eps, upd)
    r = A.bn_fin_ref(c, c.mean, c.var, float(c.Mg), eps)
    ax = ("client", "channel")
    L.assert_exact(o["mean"], r.mean, ax)
    if exact:
        for k in ("invstd", "scale", "shift"):
            L.assert_exact(o[k], getattr(r, k), ax)
    else:
        _rec("bn_finalize invstd (2 ulp)", NL.assert_ulp(o["invstd"], r.invstd, 2, ax) / 2)
        _rec("bn_finalize scale (2 ulp)", NL.assert_ulp(o["scale"], r.scale, 2, ax) / 2)
        _rec("bn_finalize shift", NL.assert_within(o["shift"], r.shift, 4 * A.U32 * r.shift_terms, ax))
    _running_ok(c, bf, r, upd, "bn_finalize")


@pytest.mark.parametrize("null_out", [False, True])
@pytest.mark.parametrize("exact", [True, False], ids=["eps0", "eps"])
@pytest.mark.parametrize("G,C", [(3, 8), (1, 192)])
def test_bn_eval_lattice(G, C, exact, null_out):
    m = _m()
    c = A.bn_eval_case(G, C, exact)
    n = G * C
    o = {k: _nan(n, guard=8) for k in ("scale", "shift", "mean", "invstd")}
    th, bf = c.theta.to(DEV), c.bufs.to(DEV)
    m.bn_eval(G, C, th.data_ptr(), c.ldt, c.off_g, c.off_b, bf.data_ptr(), c.ldb, c.off_rm, c.off_rv, c.eps,
              o["scale"].data_ptr(), o["shift"].data_ptr(), 0 if null_out else o["mean"].data_ptr(),
              0 if null_out else o["invstd"].data_ptr(), _st())
    _guard(n, *o.values())
    assert torch.equal(bf.cpu(), c.bufs), "bn_eval changed the buffers"
    ax = ("client", "channel")
    v = {k: b[:n].view(G, C) for k, b in o.items()}
    if null_out:
        assert bool(torch.isnan(v["mean"]).all()) and bool(torch.isnan(v["invstd"]).all())
    else:
        L.assert_exact(v["mean"], c.rm, ax)
    if exact:
        L.assert_exact(v["scale"], c.scale, ax)
        L.assert_exact(v["shift"], c.shift, ax)
        if not null_out:
            L.assert_exact(v["invstd"], c.invstd, ax)
        return
    if not null_out:
        _rec("bn_eval invstd (2 ulp)", NL.assert_ulp(v["invstd"], c.invstd, 2, ax) / 2)
    _rec("bn_eval scale (3 ulp)", NL.assert_ulp(v["scale"], c.scale, 3, ax) / 3)
    _rec("bn_eval shift", NL.assert_within(v["shift"], c.shift, 6 * A.U32 * c.shift_terms, ax))


@pytest.mark.parametrize("npos,C,S", A.BN_APPLY)
def test_bn_relu_apply_exact(npos, C, S):
    m = _m()
    c = A.bn_apply_case(npos, C, S)
    h = _nan(npos, C, dtype=torch.bfloat16, guard=1)
    y, sc, sh = c.y.to(DEV), c.scale.to(DEV), c.shift.to(DEV)
    m.bn_relu_apply(y.data_ptr(), sc.data_ptr(), sh.data_ptr(), h.data_ptr(), npos, C, S, _st())
    _guard(npos, h)
    _bits_equal(h[:npos], c.h, ("position", "channel"), "bn_relu_apply bits")


# ================================================================================================ head.hip
def _head_run(c, train, keep=1.0, seed=0, cids=None, seed_dev=None):
    m = _m()
    o = c.o
    logits, loss = _nan(c.NB, guard=1), _nan(c.G, guard=1)
    dp5 = _nan(c.NB, 2, 128, dtype=torch.bfloat16, guard=1)
    grad = torch.full((c.G, o.ld), A.FILL, device=DEV)
    p5, th, y = c.p5.to(DEV), c.theta.to(DEV), c.y.to(DEV)
    ci = None if cids is None else torch.tensor(cids, dtype=torch.int32, device=DEV)
    sd = None if seed_dev is None else torch.tensor([seed_dev], dtype=torch.int64, device=DEV)
    m.head(p5.data_ptr(), th.data_ptr(), o.ld, o.w1, o.b1, o.w2, o.b2, y.data_ptr(), logits.data_ptr(), loss.data_ptr(),
           grad.data_ptr(), o.ld, dp5.data_ptr(), c.G, c.B, int(train), keep, seed, 0 if ci is None else ci.data_ptr(),
           0 if sd is None else sd.data_ptr(), _st())
    _guard(c.NB, logits, dp5)
    _guard(c.G, loss)
    return logits[:c.NB].cpu(), loss[:c.G].cpu(), grad.cpu(), dp5[:c.NB].cpu()


def _head_grads(c, grad):
    o = c.o
    return dict(w1=grad[:, o.w1:o.w1 + A.HH * A.HF], b1=grad[:, o.b1:o.b1 + A.HH], w2=grad[:, o.w2:o.w2 + A.HH],
                b2=grad[:, o.b2:o.b2 + 1])


@pytest.mark.parametrize("B", A.HEAD_EVAL_B)
def test_head_eval_logits_exact(B):
    """Integer logits bit for bit, through the 32-sample chunk loop (B = 33, 70); eval mode writes nothing else."""
    c = A.head_case("int", A.HEAD_G, B)
    logits, loss, grad, dp5 = _head_run(c, False)
    L.assert_exact(logits, A.head_ref(c, False).logits.view(-1), ("sample",))
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dp5.float()).all()) and bool((grad == A.FILL).all())


@pytest.mark.parametrize("B", A.HEAD_TRAIN_B)
def test_head_train_zero_logits_exact(B):
    """All logits exactly 0: sigma = 1/2, dz2 = +-1/(2B), every gradient exact; loss = log1pf(1) within 1 ulp of log 2."""
    c = A.head_case("zero", A.HEAD_G, B)
    r = A.head_ref(c, True)
    assert float(r.logits.abs().max()) == 0.0
    logits, loss, grad, dp5 = _head_run(c, True)
    L.assert_exact(logits, r.logits.view(-1), ("sample",))
    _rows_ok(grad, c.o.spans, "head gradient row")
    for k, v in _head_grads(c, grad).items():
        assert float(r.g[k].abs().max()) > 0 or k == "b2"
        L.assert_exact(v, r.g[k], ("client", k))
    assert float(r.dp5.abs().max()) > 0
    _bits_equal(dp5, r.dp5.to(torch.bfloat16), ("sample", "h", "channel"), "head dp5 bits")
    NL.assert_ulp(loss, r.loss, 1, ("client",))


def _head_bounded(c, r, logits, loss, grad, dp5, tag):
    e = A.K_HEAD * A.U32 + A.DEV_REL
    L.assert_exact(logits, r.logits.view(-1), ("sample",))
    _rows_ok(grad, c.o.spans, "head gradient row")
    for k, v in _head_grads(c, grad).items():
        _rec("%s d%s" % (tag, k), NL.assert_within(v, r.g[k], e * r.t[k] + 2.0 ** -60, ("client", k)))
    _rec(tag + " dp5", NL.assert_within(dp5, r.dp5, NL.bf16_bound(r.dp5, e * r.dp5_t), ("sample", "h", "channel")))
    z, y = r.logits, c.y.double().view(c.G, c.B)
    lt = (torch.relu(z) + (z * y).abs() + torch.log1p(torch.exp(-z.abs()))).mean(1)
    _rec(tag + " loss", NL.assert_within(loss, r.loss, e * lt, ("client",)))
    # the device term alone (B = 1: db2 is dz2 = sigma(z) - y): error in units of 2^-24 |sigma| + |sigma - y|
    d = ((_head_grads(c, grad)["b2"].double() - r.g["b2"]).abs() / (A.U32 * r.t["b2"])).max()
    print("alexlattice head device term %s: db2 error %.3f x 2^-24 of its terms" % (tag, float(d)))


@pytest.mark.parametrize("B", A.HEAD_TRAIN_B)
def test_head_train_integer_logits_bounded(B):
    c = A.head_case("int", A.HEAD_G, B)
    r = A.head_ref(c, True)
    assert float(r.logits.abs().max()) > 0
    _head_bounded(c, r, *_head_run(c, True), "head B=%d" % B)


HEAD_SEED, HEAD_CIDS = 1234, [5, 2]


def test_head_dropout_masks_exact():
    """keep = 0.5 (inv_keep = 2 exact): forward logits exact under the masks regenerated from hash4; backward within the
    counted bound, and exactly 0 wherever a mask drops."""
    c = A.head_case("int", A.HEAD_G, 8)
    masks = A.head_masks(HEAD_SEED, HEAD_CIDS, c.B, 0.5)
    r = A.head_ref(c, True, 0.5, masks)
    logits, loss, grad, dp5 = _head_run(c, True, 0.5, HEAD_SEED, HEAD_CIDS)
    _head_bounded(c, r, logits, loss, grad, dp5, "head dropout")
    drop = ~masks[0].view(c.NB, 128, 2).permute(0, 2, 1)
    assert float(dp5.float()[drop].abs().max()) == 0.0, "dp5 is non-zero at a dropped feature"
    assert float(dp5.float().abs().max()) > 0


def _head_slice(c, g):
    import copy
    s = copy.copy(c)
    s.G, s.NB = 1, c.B
    s.p5, s.y, s.theta = c.p5[g * c.B:(g + 1) * c.B], c.y[g * c.B:(g + 1) * c.B], c.theta[g:g + 1]
    return s


def test_head_dropout_sharding_and_device_seed():
    """cids = [5, 2] gives each client the rows of running that id alone; seed_dev = k equals seed + k."""
    c = A.head_case("int", A.HEAD_G, 8)
    both = _head_run(c, True, 0.5, HEAD_SEED, HEAD_CIDS)
    for g, cid in enumerate(HEAD_CIDS):
        one = _head_run(_head_slice(c, g), True, 0.5, HEAD_SEED, [cid])
        B = c.B
        for a, b, what in ((both[0][g * B:(g + 1) * B], one[0], "logits"), (both[1][g:g + 1], one[1], "loss"),
                           (both[2][g:g + 1], one[2], "gradient row"), (both[3][g * B:(g + 1) * B], one[3], "dp5")):
            assert torch.equal(a, b), "client id %d alone differs from its row of the pair: %s" % (cid, what)
    dev = _head_run(c, True, 0.5, HEAD_SEED, HEAD_CIDS, seed_dev=7)
    host = _head_run(c, True, 0.5, HEAD_SEED + 7, HEAD_CIDS)
    assert not torch.equal(dev[0], both[0]), "seed_dev = 7 left the masks unchanged"
    for a, b in zip(dev, host):
        assert torch.equal(a, b), "seed_dev = 7 differs from seed + 7"


@pytest.mark.parametrize("HW,C,K,B,exact", A.CLS_CASES)
def test_cls_head_train_lattice(HW, C, K, B, exact):
    """exact: softmax exactly 1 / K, so dlog, dW, db, da and pooled are exact and the loss is logf(K) within 1 ulp.
    Otherwise distinct integer logits under the counted bound K_CLS."""
    m = _m()
    c = A.cls_case(HW, C, K, B, exact)
    N, G = c.N, c.G
    pooled, dlog, lossn = _nan(N, C, guard=1), _nan(N, K, guard=1), _nan(N, guard=1)
    losses = _nan(G, guard=1)
    da = _nan(N, HW, C, dtype=torch.bfloat16, guard=1)
    grad = torch.full((G, c.ld), A.FILL, device=DEV)
    a, th, y = c.a.to(DEV), c.theta.to(DEV), c.y.to(DEV)
    m.cls_head_train(a.data_ptr(), th.data_ptr(), c.ld, c.off_w, c.off_b, y.data_ptr(), G, B, HW, C, K, pooled.data_ptr(),
                     dlog.data_ptr(), lossn.data_ptr(), losses.data_ptr(), grad.data_ptr(), c.ld, da.data_ptr(), _st())
    _guard(N, pooled, dlog, lossn, da)
    _guard(G, losses)
    grad = grad.cpu()
    _rows_ok(grad, c.spans, "cls_head_train gradient row")
    gW, gb = grad[:, c.off_w:c.off_w + K * C], grad[:, c.off_b:c.off_b + K]
    L.assert_exact(pooled[:N], c.pooled, ("sample", "channel"))
    if exact:
        assert float(c.z.abs().max()) == 0.0
        L.assert_exact(dlog[:N], c.dlog, ("sample", "class"))
        L.assert_exact(gW, c.dW, ("client", "weight"))
        L.assert_exact(gb, c.db, ("client", "class"))
        # by value: the exact input gradient is zero (the softmax gradients sum to 0), of either sign
        L.assert_exact(da[:N], c.da.to(torch.bfloat16).double(), ("sample", "hw", "channel"))
        NL.assert_ulp(lossn[:N], c.lossn, 1, ("sample",))
        NL.assert_ulp(losses[:G], c.losses, 1, ("client",))
        return
    e = A.K_CLS * A.U32 + A.DEV_REL
    tag = "cls_head K=%d C=%d" % (K, C)
    _rec(tag + " dlog", NL.assert_within(dlog[:N], c.dlog, e * c.dlog_t, ("sample", "class")))
    _rec(tag + " dW", NL.assert_within(gW, c.dW, e * c.dW_t + 2.0 ** -60, ("client", "weight")))
    _rec(tag + " db", NL.assert_within(gb, c.db, e * c.db_t, ("client", "class")))
    _rec(tag + " da", NL.assert_within(da[:N], c.da, NL.bf16_bound(c.da, e * c.da_t), ("sample", "hw", "channel")))
    lt = torch.logsumexp(c.z, 1).abs() + c.z.gather(1, c.y.view(-1, 1)).squeeze(1).abs()
    _rec(tag + " lossn", NL.assert_within(lossn[:N], c.lossn, e * lt, ("sample",)))
    _rec(tag + " losses", NL.assert_within(losses[:G], c.losses, e * lt.view(G, B).mean(1), ("client",)))
