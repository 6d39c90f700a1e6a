"""Integer-lattice operands and fp64 CPU references for the AlexNet3D kernels: the fused conv1 forward, its BN statistics
and weight gradient (conv1.hip), the BatchNorm-pool kernels (bn.hip, bn_relu_apply) and the heads (head.hip).

The references are written from the formulas in the kernel headers, not from the kernels' loops:

* conv1 forward: ``acc = conv3d(volume, sign w)`` (stride 2) with integer weights |w| <= 8 against raw uint8 voxels is an
  exact integer below 2^19 in any summation order; ``z = acc 2^-k + shift`` is exact in fp32 for scales ``+-255 2^-k``
  (``fl(255 2^-k fl(1/255)) = 2^-k``), so the pooled output is one round-to-nearest-even to bf16 of an exact value.  The
  argmax tag rides in the 5 low mantissa bits of the accumulator: among equal ``acc`` the largest window index
  ``dd 9 + dh 3 + dw`` wins when ``acc >= 0`` and the smallest when ``acc < 0``.
* conv1 weight gradient: ``S[c][k] = sum_cells dz patch(argmax voxel)[k]``, ``D[c] = sum dz`` with
  ``dz = pooled > 0 ? dL/dpooled : 0``: integer sums below 2^24 per sample for bf16-integer ``dp``.
* BatchNorm-pool (bn.hip): ``z = y s + t`` on bf16 integers with ``s = +-2^k``; the argmax is the FIRST maximum in
  (d, h, w) scan order (PyTorch's rule) - unlike the fused conv1 forward above.

This is a plain helper module (CPU only, no fixtures): tests/test_cpu_alexlattice.py proves the preconditions,
tests/test_gpu_exact_alexnet.py runs the kernels.
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

import _lattice as L
import _normlattice as NL

U32 = NL.U32
FILL = NL.FILL
VOL = (121, 145, 121)
PPH = (61, 73, 61)
OD = (59, 71, 59)
PD = (19, 23, 19)
C1 = 64
NPOS = OD[0] * OD[1] * OD[2]
NCELL = PD[0] * PD[1] * PD[2]
EPS = NL.BN_EPS
MOM = NL.BN_MOM

# ------------------------------------------------------------------------------------------------ conv1 case tables
C1_G, C1_B = 2, 2
C1_NB = C1_G * C1_B
C1_IDX = (2, 0, 1, 0)                  # non-identity map into the three volumes, volume 0 used twice
C1_WMAX = 8                            # |w| <= 8: f16(w) = w
C1_KEXP = (0, 3, 8, 5, 10, 1)          # scale = +-255 2^-k, k = C1_KEXP[c % 6]
C1_ZERO_SCALE_CH = 7                   # scale exactly 0
C1_DEAD_SHIFT = -float(2 ** 19)        # channels c % 8 == 5: z < 0 everywhere (|acc| 2^-k < 2^19)
C1_BORDER = 16                         # zero border of volume 1: the first and last pooled cells tie at all 27 taps
ACC_LIMIT = 1 << 19                    # |acc| below this: the 5 tag bits hold no accumulator bit
C1_BIG = (256, 16)                     # (NB, B) of the large weight-gradient case
FWD_AXES = ("sample", "pd", "ph", "pw", "channel")


def tp_valid(t, r):
    jd, jh, jw = t // 9, (t // 3) % 3, t % 3
    return 2 * jd + (r >> 2) < 5 and 2 * jh + ((r >> 1) & 1) < 5 and 2 * jw + (r & 1) < 5


def tp_to_k(t, r):
    jd, jh, jw = t // 9, (t // 3) % 3, t % 3
    return (2 * jd + (r >> 2)) * 25 + (2 * jh + ((r >> 1) & 1)) * 5 + (2 * jw + (r & 1))


def _groups():
    """Tap groups t = 9 jd + 3 jh + jw by which of their j are 2: F (none), D, H, W, DH, DW, HW, DHW, ascending t."""
    cls = {}
    for t in range(27):
        jd, jh, jw = t // 9, (t // 3) % 3, t % 3
        key = ("D" if jd == 2 else "") + ("H" if jh == 2 else "") + ("W" if jw == 2 else "")
        cls.setdefault(key or "F", []).append(t)
    return cls


def _phases(t):
    return [r for r in range(8) if tp_valid(t, r)]


def c1_slots(ro=0, ks=128):
    """(tap group, phase) of every K slot of a packed conv1 weight row, None for an empty slot: the layout described
    above c1_slot128 in conv1.hip.  ks = 224: the legacy 27 x 8 layout.  ro: the tap-group order (0 ascending, 1 and 2
    with the two lane quarters of a read paired by jw; 2 also regroups the 2-phase groups of k-step 3)."""
    if ks == 224:
        return [(kk >> 3, kk & 7) if (kk >> 3) < 27 and tp_valid(kk >> 3, kk & 7) else None for kk in range(224)]
    assert ks == 128
    g = _groups()
    pair = (lambda q: [q[0], q[2], q[1], q[3]]) if ro else (lambda q: list(q))
    Fg = pair(g["F"][:4]) + pair(g["F"][4:])
    Dg, Hg, Wg = pair(g["D"]), pair(g["H"]), g["W"]
    if ro == 2:
        x1 = [g["DW"][0], g["DW"][1], g["DHW"][0], None]
        x2 = [g["DH"][0], g["DH"][1], g["HW"][0], g["HW"][1]]
    else:
        x1 = [g["DH"][0], g["DW"][0], g["HW"][0], g["DHW"][0]]
        x2 = [g["DH"][1], g["DW"][1], g["HW"][1], None]
    out = []
    for kk in range(128):
        st, fq, e = kk >> 5, (kk >> 3) & 3, kk & 7
        if st < 2:
            t, ph = Fg[4 * st + fq], list(range(8))
            out.append((t, ph[e]))
            continue
        if st == 2:
            t = Dg[fq] if e < 4 else Hg[fq]
            out.append((t, _phases(t)[e & 3]))
            continue
        if e < 4:
            out.append((Wg[fq], _phases(Wg[fq])[e]))
            continue
        t = (x1 if e < 6 else x2)[fq]
        if t is None:
            out.append(None)
            continue
        if ro == 2 and e < 6:
            r = (0, 2)[e & 1]             # the X1 quarter reads phases 0, 2 of its group (DHW has no phase 2)
            out.append((t, r) if tp_valid(t, r) else None)
            continue
        ph = _phases(t)
        out.append((t, ph[e & 1]) if (e & 1) < len(ph) else None)
    return out


def slot_taps(slots):
    """The original tap k = kd 25 + kh 5 + kw of every non-empty slot."""
    return [tp_to_k(*s) for s in slots if s is not None]


# ------------------------------------------------------------------------------------------------ conv1 operands
@functools.lru_cache(maxsize=1)
def volumes():
    """Three distinct uint8 volumes with the full 0..255 range; volume 1 has a constant-zero border C1_BORDER thick."""
    g = L.gen("alex", "volumes")
    v = torch.randint(0, 256, (3,) + VOL, generator=g, dtype=torch.uint8)
    v[:, 60, 70, :2] = torch.tensor([0, 255], dtype=torch.uint8)
    b = C1_BORDER
    inner = v[1, b:-b, b:-b, b:-b].clone()
    v[1] = 0
    v[1, b:-b, b:-b, b:-b] = inner
    return v


def polyphase_ref(vol):
    """[N, 121, 145, 121] -> [N, 61, 73, 61, 8]: voxel (d, h, w) at (d>>1, h>>1, w>>1), phase (d&1)<<2 | (h&1)<<1 | w&1."""
    N = vol.shape[0]
    pad = torch.zeros((N, 122, 146, 122), dtype=vol.dtype)
    pad[:, :121, :145, :121] = vol
    return pad.view(N, 61, 2, 73, 2, 61, 2).permute(0, 1, 3, 5, 2, 4, 6).reshape(N, 61, 73, 61, 8).contiguous()


@functools.lru_cache(maxsize=1)
def conv1_case():
    """Weights, scales, shifts and the exact reference of the fused forward at (G, B) = (2, 2)."""
    g = L.gen("alex", "conv1")
    c = types.SimpleNamespace(G=C1_G, B=C1_B, NB=C1_NB)
    c.idx = torch.tensor(C1_IDX, dtype=torch.int32)
    c.w = torch.randint(-C1_WMAX, C1_WMAX + 1, (c.G, C1, 125), generator=g).float()
    ch = torch.arange(C1)
    c.kexp = torch.tensor(C1_KEXP)[ch % len(C1_KEXP)].view(1, C1).expand(c.G, C1).contiguous()
    sgn = torch.where((ch.view(1, C1) + torch.arange(c.G).view(c.G, 1)) % 3 == 1, -1.0, 1.0)
    c.scale = (sgn * 255.0 * torch.ldexp(torch.ones(c.G, C1), -c.kexp)).float()
    c.scale[:, C1_ZERO_SCALE_CH] = 0.0
    c.shift = torch.randint(-4, 5, (c.G, C1), generator=g).float()
    c.shift[:, ch % 8 == 5] = C1_DEAD_SHIFT
    c.shift[:, C1_ZERO_SCALE_CH] = torch.tensor([3.0, -3.0])         # z = shift: a constant live / dead channel
    c.dead = (ch % 8 == 5)
    c.sign = torch.where(c.scale < 0, -1.0, 1.0)                     # what off_sign folds into the packed weights
    # z = acc * mult + shift, mult = fl(|scale| * fl(1/255)) = 2^-k (0 for the zero-scale channel)
    c.mult = torch.ldexp(torch.ones(c.G, C1), -c.kexp).double()
    c.mult[:, C1_ZERO_SCALE_CH] = 0.0
    # theta row: [w 8000 | FILL 8 | scale 64 (off_sign) | FILL 8]
    c.P = 8000 + 8 + 64 + 8
    c.off_w, c.off_sign = 0, 8008
    c.theta = torch.full((c.G, c.P), FILL)
    c.theta[:, :8000] = c.w.view(c.G, 8000)
    c.theta[:, 8008:8072] = c.scale
    c.acc = conv1_acc(volumes(), c.w * c.sign.unsqueeze(2), c.idx, c.B)
    c.out, c.amax, c.macc = conv1_pool_ref(c.acc, c.mult, c.shift, c.B)
    return c


def conv1_acc(vols, w, idx, B):
    """Integer-valued fp32 stride-2 convolution of sample n = volume idx[n] with its client's filters:
    [NB, 64, 59, 71, 59].  Exact: every partial sum is an integer below 255 sum|w| < 2^24."""
    out = []
    for n, i in enumerate(idx.tolist()):
        x = vols[i].float().view(1, 1, *VOL)
        out.append(F.conv3d(x, w[n // B].view(C1, 1, 5, 5, 5), stride=2)[0])
    return torch.stack(out)


def window_keys(win):
    """Tagged-accumulator order of the 27 candidates of a pooling window (last axis, index dd 9 + dh 3 + dw): the tag is
    OR-ed into the magnitude, so a larger index is larger for acc >= 0 and smaller for acc < 0."""
    i = torch.arange(27, dtype=torch.int64)
    return win * 64 + torch.where(win >= 0, i, -i)


def _windows(a):
    """[C, 59, 71, 59] -> [C, 19, 23, 19, 27] pooling windows (3, 3, floor mode)."""
    a = a[:, :57, :69, :57]
    w = a.unfold(1, 3, 3).unfold(2, 3, 3).unfold(3, 3, 3)
    return w.reshape(a.shape[0], PD[0], PD[1], PD[2], 27)


def conv1_pool_ref(acc, mult, shift, B):
    """Pooled bf16 output [NB, 19, 23, 19, 64], argmax bytes and the winning accumulator of the fused forward."""
    outs, ams, mx = [], [], []
    for n in range(acc.shape[0]):
        g = n // B
        win = _windows(acc[n]).to(torch.int64)
        am = window_keys(win).argmax(-1)
        m = win.gather(-1, am.unsqueeze(-1)).squeeze(-1).double()
        z = m * mult[g].view(C1, 1, 1, 1) + shift[g].double().view(C1, 1, 1, 1)
        outs.append(torch.relu(z).permute(1, 2, 3, 0))
        ams.append(am.permute(1, 2, 3, 0).to(torch.uint8))
        mx.append(m.permute(1, 2, 3, 0))
    z = torch.stack(outs)
    assert torch.equal(z.float().double(), z), "conv1 reference: z is not exact in fp32"
    return z.to(torch.bfloat16), torch.stack(ams), torch.stack(mx)


def pack_ref(c, scale_arg, ro=0, ks=128, signed=True):
    """(w8 [G, 64, ks] int16 bit patterns of f16(sign w) per slot, w125 [G, 64, 125] = f16(w) * scale_arg in fp32)."""
    slots = c1_slots(ro, ks)
    bits = c.w.to(torch.float16).view(torch.int16).to(torch.int32) & 0xffff
    if signed:
        bits = torch.where(c.sign.unsqueeze(2) < 0, bits ^ 0x8000, bits)
    w8 = torch.zeros(c.G, C1, ks, dtype=torch.int32)
    for kk, s in enumerate(slots):
        if s is not None:
            w8[:, :, kk] = bits[:, :, tp_to_k(*s)]
    w8 = torch.where(w8 >= 0x8000, w8 - 0x10000, w8).to(torch.int16)
    w125 = c.w.to(torch.float16).float() * torch.tensor(scale_arg, dtype=torch.float32)
    return w8, w125


def first_mismatch(got, ref, names):
    """None, or the coordinates and values of the first differing element of two equal-shaped tensors."""
    got, ref = got.cpu(), ref.cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    bad = got != ref
    if not bool(bad.any()):
        return None
    i = int(torch.nonzero(bad.flatten())[0])
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))
    return "%d of %d differ; first at (%s): got %r, reference %r" % (
        int(bad.sum()), bad.numel(), ", ".join("%s=%d" % p for p in zip(names, idx)), got[idx].item(), ref[idx].item())


def check_conv1_fwd(out, amax, c):
    """Bit equality of the pooled bf16 output; argmax bytes wherever the pooled value is > 0; every byte < 27."""
    e = first_mismatch(out.cpu().view(torch.int16), c.out.view(torch.int16), FWD_AXES)
    assert e is None, "conv1 forward output bits: " + e
    amax = amax.cpu()
    assert int(amax.max()) < 27, "argmax byte out of range: %d" % int(amax.max())
    live = c.out.float() > 0
    e = first_mismatch(torch.where(live, amax, torch.zeros_like(amax)),
                       torch.where(live, c.amax, torch.zeros_like(c.amax)), FWD_AXES)
    assert e is None, "conv1 forward argmax: " + e


# ------------------------------------------------------------------------------------------------ conv1 BN statistics
@functools.lru_cache(maxsize=1)
def moments_ref():
    """Exact per-volume patch moments [3, 125 + 125^2] (integer-valued fp64): sum p and sum p p^T over all positions."""
    out = torch.zeros(3, 125 + 125 * 125, dtype=torch.float64)
    for n in range(3):
        p = patches(n).double()
        out[n, :125] = p.sum(0)
        out[n, 125:] = (p.t() @ p).reshape(-1)
    return out


@functools.lru_cache(maxsize=3)
def patches(v):
    """[59 71 59, 125] fp32 patches of volume v (tap k = kd 25 + kh 5 + kw)."""
    x = volumes()[v].float()
    return x.unfold(0, 5, 2).unfold(1, 5, 2).unfold(2, 5, 2).reshape(-1, 125).contiguous()


def bnstats_theta(G, g):
    """theta [G, 3*64 + fillers]: integer conv bias, dyadic gamma of both signs, integer beta."""
    P = 8 + 64 + 8 + 64 + 8 + 64 + 8
    th = torch.full((G, P), FILL)
    off = types.SimpleNamespace(bias=8, g=80, b=152, P=P)
    th[:, 8:72] = torch.randint(-3, 4, (G, 64), generator=g).float()
    k = torch.randint(-2, 3, (G, 64), generator=g)
    th[:, 80:144] = torch.ldexp(torch.ones(G, 64), k) * (torch.randint(0, 2, (G, 64), generator=g) * 2 - 1).float()
    th[:, 152:216] = torch.randint(-4, 5, (G, 64), generator=g).float()
    return th, off


def bnstats_bufs(G, g):
    Q = 8 + 64 + 8 + 64 + 8 + 1 + 7
    bufs = torch.full((G, Q), FILL)
    off = types.SimpleNamespace(rm=8, rv=80, nbt=152, Q=Q)
    bufs[:, 8:72] = torch.randint(-8, 9, (G, 64), generator=g).float()
    bufs[:, 80:144] = torch.randint(1, 9, (G, 64), generator=g).float()
    bufs[:, 152] = torch.arange(G).float() + 3
    return bufs, off


def bnstats_from(mean_nb, var, mu, covw, theta, off, bufs, boff, npos):
    """The outputs of conv1_bnstats from the fp64 batch mean (no bias) / biased variance per (g, c), as fp64 values, with
    the magnitudes each counted bound needs."""
    r = types.SimpleNamespace()
    bias = theta[:, off.bias:off.bias + 64].double()
    gm = theta[:, off.g:off.g + 64].double()
    bt = theta[:, off.b:off.b + 64].double()
    r.var = var
    r.invstd = 1.0 / torch.sqrt(var + EPS)
    r.scale = gm * r.invstd
    r.shift = bt - mean_nb * r.scale
    r.shift_terms = bt.abs() + (mean_nb * r.scale).abs()
    r.mean = mean_nb + bias
    r.mu, r.covw = mu, covw
    rm = bufs[:, boff.rm:boff.rm + 64].double()
    rv = bufs[:, boff.rv:boff.rv + 64].double()
    unb = var * npos / (npos - 1.0)
    r.rm = (1.0 - MOM) * rm + MOM * r.mean
    r.rm_terms = ((1.0 - MOM) * rm).abs() + (MOM * r.mean).abs()
    r.rv = (1.0 - MOM) * rv + MOM * unb
    r.rv_terms = ((1.0 - MOM) * rv).abs() + (MOM * unb).abs()
    r.nbt = bufs[:, boff.nbt].double() + 1
    return r


def bnstats_moment_form(w, idx, B):
    """mean_c = w_c . mu, var_c = w_c^T (M / N - mu mu^T) w_c per client from the exact moments, in fp64; also mu [G, 125]
    and covw [G, 64, 125] = Cov w_c."""
    mom = moments_ref()
    G = len(idx) // B
    Mb = mom[torch.as_tensor(idx).long()].view(G, B, -1).sum(1)
    N = float(B * NPOS)
    mu = Mb[:, :125] / N
    cov = Mb[:, 125:].view(G, 125, 125) / N - mu.unsqueeze(2) * mu.unsqueeze(1)
    wd = w.double()
    covw = torch.einsum("gkl,gcl->gck", cov, wd)
    return (wd * mu.unsqueeze(1)).sum(2), (wd * covw).sum(2), mu, covw


def bnstats_direct(c):
    """Mean and biased variance of the integer conv output of the forward case, per (g, c), in fp64."""
    y = (c.acc.double() * c.sign.repeat_interleave(c.B, 0).double().view(c.NB, C1, 1, 1, 1))
    y = y.view(c.G, c.B, C1, -1).permute(0, 2, 1, 3).reshape(c.G, C1, -1)
    mean = y.mean(2)
    return mean, ((y - mean.unsqueeze(2)) ** 2).mean(2)


def bnstats_bounds(r, cond_rel):
    """Counted fp32 roundings of the kernel's last block (|error| <= count * 2^-24 * |term|) plus the conditioning of the
    fp64 variance (relative error cond_rel of var, i.e. cond_rel / 2 of invstd)."""
    civ = r.invstd * 0.5 * cond_rel * r.var / (r.var + EPS)
    b = types.SimpleNamespace()
    b.invstd = 1 * U32 * r.invstd + civ                                   # (float)(1 / sqrt)
    b.scale = 2 * U32 * r.scale.abs() + civ * (r.scale / r.invstd).abs()  # + one product
    # shift = bt - (float)mnb * gm * inv: (float)mnb, two products, one subtraction
    b.shift = 4 * U32 * r.shift_terms + civ * (r.shift_terms / r.invstd)
    b.mean = 1 * U32 * r.mean.abs() + 2.0 ** -40 * r.mean.abs().clamp_min(1.0)
    b.rm = 4 * U32 * r.rm_terms                                           # 1 - m, (float) mean, two products, one sum
    b.rv = 4 * U32 * r.rv_terms + cond_rel * r.rv_terms
    return b


# ------------------------------------------------------------------------------------------------ conv1 weight gradient
@functools.lru_cache(maxsize=1)
def wgrad_case():
    """Given (not forward-derived) inputs of conv1_wgrad at NB = 4 and the exact per-sample S [4, 64, 125] / D [4, 64]."""
    g = L.gen("alex", "wgrad")
    c = types.SimpleNamespace(G=C1_G, B=C1_B, NB=C1_NB)
    c.idx = torch.tensor(C1_IDX, dtype=torch.int32)
    shp = (c.NB,) + PD + (C1,)
    mag = torch.tensor([1.0, 2.0, 4.0])[torch.randint(0, 3, shp, generator=g)]
    sgn = (torch.randint(0, 2, shp, generator=g) * 2 - 1).float()
    c.dp = (mag * sgn * (torch.rand(shp, generator=g) < 0.5)).to(torch.bfloat16)
    c.pout = (torch.randint(0, 2, shp, generator=g) * 2 - 1).to(torch.bfloat16)
    c.amax = torch.randint(0, 27, shp, generator=g, dtype=torch.uint8)
    c.S, c.D = wgrad_sums(c.dp, c.pout, c.amax, c.idx)
    return c


def wgrad_dz(dp, pout):
    return torch.where(pout.float() > 0, dp.float(), torch.zeros(())).double()


def wgrad_sums(dp, pout, amax, idx, drop=None):
    """Per sample: scatter dz to the argmax voxels of the conv output grid and correlate with the volume.  ``drop``: a
    (sample, pd, ph, pw, channel) cell left out (mutation checks)."""
    dz = wgrad_dz(dp, pout)
    if drop is not None:
        dz = dz.clone()
        dz[drop] = 0
    NB = dp.shape[0]
    pd = torch.arange(PD[0]).view(-1, 1, 1, 1)
    ph = torch.arange(PD[1]).view(1, -1, 1, 1)
    pw = torch.arange(PD[2]).view(1, 1, -1, 1)
    S = torch.zeros(NB, C1, 125, dtype=torch.float64)
    for n in range(NB):
        a = amax[n].long()
        pos = ((3 * pd + a // 9) * OD[1] + 3 * ph + (a // 3) % 3) * OD[2] + 3 * pw + a % 3      # [19, 23, 19, 64]
        Z = torch.zeros(C1, NPOS, dtype=torch.float64)
        Z.scatter_(1, pos.view(-1, C1).t().contiguous(), dz[n].view(-1, C1).t().contiguous())
        S[n] = Z @ patches(int(idx[n])).double()
    return S, dz.view(NB, -1, C1).sum(1)


def wgrad_client(S, D, B, s=None):
    """Per-client sums of per-sample S / D (optionally sample n weighted by s[n], base sample n mod 4)."""
    NB = S.shape[0] if s is None else len(s)
    sel = torch.arange(NB) % S.shape[0]
    wt = torch.ones(NB, dtype=torch.float64) if s is None else torch.as_tensor(s, dtype=torch.float64)
    return ((S[sel] * wt.view(-1, 1, 1)).view(NB // B, B, C1, 125).sum(1),
            (D[sel] * wt.view(-1, 1)).view(NB // B, B, C1).sum(1))


def big_scales(NB=C1_BIG[0]):
    """Per-sample powers of two in {1, 2, 4}, assigned aperiodically (a quadratic residue sequence)."""
    return [(1, 2, 4)[(n * n + n // 7) % 3] for n in range(NB)]


def part_sum(part, G, nsl):
    """Per-client sum of the part slabs, in fp64."""
    p = part[:G * nsl].double().view(G, nsl, C1, 126).sum(1)
    return p[:, :, :125], p[:, :, 125]


def fin_case(G, eval_mode):
    """Dyadic mu / covw / invstd / gamma / w125 / wscale for the closed form of k_conv1_wgrad_fin, chosen so every product of
    the header's formulas is exact in fp64 and each result is an fp32 number (asserted by fin_ref)."""
    g = L.gen("alex", "fin", eval_mode)
    f = types.SimpleNamespace(G=G)
    f.mu = torch.randint(0, 8, (G, 125), generator=g).float()
    f.covw = torch.randint(-1, 2, (G, C1, 125), generator=g).float()
    f.invstd = torch.full((G, C1), 0.5)
    f.invstd[:, ::3] = 0.25
    f.gamma = torch.ldexp(torch.ones(G, C1), torch.randint(-1, 2, (G, C1), generator=g)) * \
        (torch.randint(0, 2, (G, C1), generator=g) * 2 - 1).float()
    f.w125 = torch.zeros(G, C1, 125)
    for gi in range(G):
        for ch in range(C1):
            ks = torch.randperm(125, generator=g)[:2]
            f.w125[gi, ch, ks] = torch.tensor([1.0, -1.0])
    f.wscale = 2.0 ** -8
    f.emean = torch.randint(-4, 5, (G, C1), generator=g).float() if eval_mode else None
    # grads row: [FILL 8 | dW 8000 | FILL 8 | dbias 64 | FILL 8 | dgamma 64 | FILL 8 | dbeta 64 | FILL 8]
    f.goff_w, f.goff_bias, f.goff_g, f.goff_b = 8, 8016, 8088, 8160
    f.ldg = 8232
    f.spans = [(8, 8000), (8016, 64), (8088, 64), (8160, 64)]
    return f


def fin_ref(f, S, D, exact=True):
    """dW, dbias, dgamma, dbeta of the header's closed form from per-client S [G, 64, 125], D [G, 64] (fp64).  exact:
    require every result to be an fp32 number (the lattice cases)."""
    iv, gm = f.invstd.double().unsqueeze(2), f.gamma.double().unsqueeze(2)
    w, Dd = f.w125.double(), D.unsqueeze(2)
    if f.emean is not None:
        dW = gm * iv * S
        dbias = (gm * iv * Dd).squeeze(2)
        dg = (iv * ((w * S).sum(2, keepdim=True) - Dd * f.emean.double().unsqueeze(2))).squeeze(2)
    else:
        r = S - Dd * f.mu.double().unsqueeze(1)
        dgk = iv * (w * r).sum(2, keepdim=True)
        dW = gm * iv * (r - dgk * iv * f.covw.double())
        dbias = torch.zeros_like(D)
        dg = dgk.squeeze(2)
    out = dict(dW=dW * f.wscale, dbias=dbias, dgamma=dg, dbeta=D.clone())
    for k, v in out.items():
        assert not exact or torch.equal(v.float().double(), v), "closed form: %s is not exact in fp32" % k
    return out


@functools.lru_cache(maxsize=1)
def bnstats_cond():
    """Measured conditioning of the fp64 cancellation in M / N - mu mu^T: the largest relative difference of the variance
    between the two fp64 references (direct over the conv output, and the moment form) at G = 2."""
    c = conv1_case()
    _, vd = bnstats_direct(c)
    _, vm, _, _ = bnstats_moment_form(c.w, c.idx.tolist(), c.B)
    return float(((vd - vm).abs() / vd).max())


@functools.lru_cache(maxsize=1)
def bnstats_g32():
    """(G, idx, w) of the eight-channels-per-block path: 32 clients of one sample each over the three volumes."""
    G = 32
    idx = [(n * n + n // 3) % 3 for n in range(G)]
    w = torch.randint(-C1_WMAX, C1_WMAX + 1, (G, C1, 125), generator=L.gen("alex", "g32")).float()
    return G, idx, w


# ================================================================================================ bn.hip
BN_SHAPES = [(17, 21, 17, 128), (5, 7, 5, 128), (3, 3, 3, 8), (4, 5, 7, 256), (6, 3, 4, 24)]
BN_GB = [(2, 1), (2, 3)]
BN_NCHUNK = (1, 7, 64, 4096)           # 4096: more chunks than positions for every shape but the first
K_BN_BWD = 4                           # fp32 roundings of dy: (float) Bc, (float) Cc, the inner and the outer fma
POOL_AXES = ("sample", "pd", "ph", "pw", "channel")
DENSE_AXES = ("sample", "d", "h", "w", "channel")


def pow2(shape, lo, hi, g, signed=True):
    """+-2^k, k uniform in [lo, hi]."""
    v = torch.ldexp(torch.ones(shape), torch.randint(lo, hi + 1, shape, generator=g))
    return v * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() if signed else v


def pool_windows(z):
    """[N, D, H, W, C] -> [N, D/3, H/3, W/3, C, 27] (floor mode), window index dd 9 + dh 3 + dw."""
    N, D, H, W, C = z.shape
    Dp, Hp, Wp = D // 3, H // 3, W // 3
    w = z[:, :3 * Dp, :3 * Hp, :3 * Wp].unfold(1, 3, 3).unfold(2, 3, 3).unfold(3, 3, 3)
    return w.reshape(N, Dp, Hp, Wp, C, 27)


@functools.lru_cache(maxsize=4)
def bn_pool_case(D, H, W, C, G, B):
    """bn_relu_pool on the lattice: bf16 integers y in {-2..2} (every window has ties), scales +-2^k and 0, integer
    shifts; z is exact, the output one RNE, the argmax the first maximum in scan order."""
    g = L.gen("alex", "bnpool", D, H, W, C, G, B)
    c = types.SimpleNamespace(D=D, H=H, W=W, C=C, G=G, B=B, NB=G * B)
    c.y = torch.randint(-2, 3, (c.NB, D, H, W, C), generator=g).to(torch.bfloat16)
    c.scale = pow2((G, C), -2, 2, g)
    c.scale[:, 3::8] = 0.0
    c.shift = torch.randint(-4, 5, (G, C), generator=g).float()
    c.z = bn_affine(c.y, c.scale, c.shift, B)
    assert torch.equal(c.z.float().double(), c.z)
    win = pool_windows(c.z)
    c.amax = win.argmax(-1).to(torch.uint8)           # torch.argmax: the first of several maxima
    c.out = torch.relu(win.amax(-1)).to(torch.bfloat16)
    return c


def bn_affine(y, scale, shift, B):
    s = scale.double().repeat_interleave(B, 0).view(-1, 1, 1, 1, y.shape[-1])
    t = shift.double().repeat_interleave(B, 0).view(-1, 1, 1, 1, y.shape[-1])
    return y.double() * s + t


def bn_bwd_cases():
    """(shape, (G, B), pool, eval_mode, nchunk, with conv-bias slice): the full cross, nchunk and the bias slice cycled."""
    out, i = [], 0
    for sh in BN_SHAPES:
        for gb in BN_GB:
            for pool in (0, 1):
                for ev in (0, 1):
                    out.append((sh, gb, pool, ev, BN_NCHUNK[(i + i // 4) % 4], (i // 8 + i) % 2 == 0))
                    i += 1
    return out


@functools.lru_cache(maxsize=2)
def bn_bwd_case(shape, gb, pool, ev):
    """bn_bwd on the lattice: integer y / dsrc, dyadic mean, invstd and gamma.  sum dz and sum dz xhat are exact; in eval
    mode dy = gamma invstd dz is exact in bf16, in train mode (N = B D H W is no power of two for these shapes) the three
    coefficients are fp64 values rounded once and dy is held to the counted bound K_BN_BWD."""
    D, H, W, C = shape
    G, B = gb
    g = L.gen("alex", "bnbwd", shape, gb, pool, ev)
    c = types.SimpleNamespace(D=D, H=H, W=W, C=C, G=G, B=B, NB=G * B, pool=pool, ev=ev)
    c.y = torch.randint(-4, 5, (c.NB, D, H, W, C), generator=g).to(torch.bfloat16)
    c.mean = torch.randint(-2, 3, (G, C), generator=g).float()
    c.invstd = pow2((G, C), -1, 1, g, signed=False)
    c.gamma = pow2((G, C), -1, 1, g)
    beta = torch.randint(-2, 3, (G, C), generator=g).float()
    c.scale = c.gamma * c.invstd
    c.shift = beta - c.mean * c.scale
    z = bn_affine(c.y, c.scale, c.shift, B)
    rep = lambda v: v.double().repeat_interleave(B, 0).view(c.NB, 1, 1, 1, C)  # noqa: E731
    if pool:
        win = pool_windows(z)
        c.amax = win.argmax(-1).to(torch.uint8)
        c.pout = torch.relu(win.amax(-1)).to(torch.bfloat16)
        c.dsrc = torch.randint(-2, 3, c.pout.shape, generator=g).to(torch.bfloat16)
        dzp = torch.where(c.pout.float() > 0, c.dsrc.float(), torch.zeros(())).double()
        Dp, Hp, Wp = D // 3, H // 3, W // 3
        full = torch.zeros(c.NB, Dp, Hp, Wp, C, 27, dtype=torch.float64)
        full.scatter_(-1, c.amax.long().unsqueeze(-1), dzp.unsqueeze(-1))
        dz = torch.zeros(c.NB, D, H, W, C, dtype=torch.float64)
        dz[:, :3 * Dp, :3 * Hp, :3 * Wp] = full.view(c.NB, Dp, Hp, Wp, C, 3, 3, 3).permute(
            0, 1, 5, 2, 6, 3, 7, 4).reshape(c.NB, 3 * Dp, 3 * Hp, 3 * Wp, C)
        c.inside = torch.zeros(D, H, W, dtype=torch.bool)
        c.inside[:3 * Dp, :3 * Hp, :3 * Wp] = True
    else:
        c.amax = c.pout = None
        c.dsrc = torch.randint(-2, 3, c.y.shape, generator=g).to(torch.bfloat16)
        dz = torch.where(z > 0, c.dsrc.double(), torch.zeros((), dtype=torch.float64))
    yd = c.y.double()
    xhat = (yd - rep(c.mean)) * rep(c.invstd)
    c.sdz = dz.view(G, -1, C).sum(1)
    c.sdx = (dz * xhat).view(G, -1, C).sum(1)
    # fp32 partial sums of the reduce kernel are exact: multiples of 1/2 (invstd >= 1/2) below 2^24 in units of 1/2
    c.sum_bound = L.require_fp32_exact(2.0 * float((dz.abs() * xhat.abs()).view(G, -1, C).sum(1).max()) + 1, "bn_bwd sums")
    gm, iv, mu = c.gamma.double(), c.invstd.double(), c.mean.double()
    N = float(B * D * H * W)
    if ev:
        c.coef = torch.stack([gm * iv, torch.zeros_like(gm), torch.zeros_like(gm)], 2)
        c.convb = gm * iv * c.sdz
    else:
        c.coef = torch.stack([gm * iv, -gm * iv * c.sdz / N + gm * iv * iv * mu * c.sdx / N,
                              -gm * iv * iv * c.sdx / N], 2)
        c.convb = torch.zeros_like(gm)
    A_, Bc, Cc = (rep(c.coef[:, :, i]) for i in range(3))
    c.dy = A_ * dz + Bc + Cc * yd
    c.dy_terms = (A_ * dz).abs() + Bc.abs() + (Cc * yd).abs()
    c.dz = dz
    return c


# (nPB, BP, ragged last block, C, G)
BN_FIN = [(1, 64, False, 8, 3), (1, 128, True, 192, 1), (3, 256, True, 8, 3), (3, 64, False, 192, 1),
          (64, 128, False, 8, 3), (64, 256, True, 192, 1), (65, 64, True, 8, 3), (65, 128, False, 192, 1),
          (130, 256, False, 8, 3), (130, 64, True, 192, 1),
          (3, 128, True, 6, 3)]      # G C = 18 pairs: the last block of four (g, c) waves is ragged
K_RUN = 5      # running statistic: 1 - momentum, the (float) cast, two products, one sum


def bn_fin_case(nPB, BP, ragged, C, G):
    """Per-block (mean, M2) partials whose merge is known in closed form: block means m0 + s_b delta with s_b in
    {-1, 0, 1} summing to zero over the equal-sized full blocks, M2_b = n_b (4^-m - delta^2 s_b^2), delta = 2^-(m+2).
    The total mean is m0 and the total biased variance 4^-m exactly; every partial is an fp32 number."""
    g = L.gen("alex", "bnfin", nPB, BP, ragged, C, G)
    c = types.SimpleNamespace(nPB=nPB, BP=BP, C=C, G=G)
    last = BP // 2 + 3 if ragged else BP
    c.Mg = (nPB - 1) * BP + last
    nb = torch.full((nPB,), float(BP), dtype=torch.float64)
    nb[-1] = last
    nfull = nPB - 1 if ragged else nPB
    # a non-zero integer: the merged mean is m0 (1 + O(2^-52)), which rounds to m0 in fp32 only if m0 != 0
    m0 = (torch.randint(1, 4, (G, C), generator=g) * (torch.randint(0, 2, (G, C), generator=g) * 2 - 1)).double()
    c.m = torch.randint(0, 3, (G, C), generator=g)
    tv = torch.ldexp(torch.ones(G, C, dtype=torch.float64), -2 * c.m)
    delta = torch.ldexp(torch.ones(G, C, dtype=torch.float64), -(c.m + 2))
    s = torch.zeros(G, C, nPB, dtype=torch.float64)
    half = nfull // 2
    for gi in range(G):
        for ch in range(C):
            p = torch.randperm(nfull, generator=g)
            s[gi, ch, p[:half]] = 1.0
            s[gi, ch, p[half:2 * half]] = -1.0
    mean_b = m0.unsqueeze(2) + delta.unsqueeze(2) * s
    m2_b = nb.view(1, 1, -1) * (tv.unsqueeze(2) - (delta.unsqueeze(2) * s) ** 2)
    c.stats = torch.stack([mean_b, m2_b], 3).permute(0, 2, 1, 3).contiguous()        # [G, nPB, C, 2]
    assert torch.equal(c.stats.float().double(), c.stats), "bn_finalize partials are not fp32 numbers"
    c.nb, c.mean, c.var = nb, m0, tv
    # theta: [8 | gamma C | 8 | beta C | 8]; bufs: [8 | rm C | 8 | rv C | 8 | nbt | 7]
    c.ldt, c.off_g, c.off_b = 24 + 2 * C, 8, 16 + C
    c.theta = torch.full((G, c.ldt), FILL)
    c.theta[:, 8:8 + C] = pow2((G, C), -2, 2, g)
    c.theta[:, 16 + C:16 + 2 * C] = torch.randint(-4, 5, (G, C), generator=g).float()
    c.ldb, c.off_rm, c.off_rv, c.off_nbt = 32 + 2 * C, 8, 16 + C, 24 + 2 * C
    c.bufs = torch.full((G, c.ldb), FILL)
    c.bufs[:, 8:8 + C] = torch.randint(-8, 9, (G, C), generator=g).float()
    c.bufs[:, 16 + C:16 + 2 * C] = torch.randint(1, 9, (G, C), generator=g).float() / 64
    c.bufs[:, c.off_nbt] = torch.arange(G).float() + 2
    return c


def chan_merge(stats, nb, skip=None):
    """Chan's parallel merge of [G, nPB, C, 2] partials in fp64 (sequential over blocks); ``skip``: a block left out."""
    G, nPB, C, _ = stats.shape
    n = torch.zeros(G, C, dtype=torch.float64)
    mean, m2 = torch.zeros_like(n), torch.zeros_like(n)
    for b in range(nPB):
        if b == skip:
            continue
        mb, qb = stats[:, b, :, 0].double(), stats[:, b, :, 1].double()
        nn = n + nb[b]
        d = mb - mean
        mean = mean + d * nb[b] / nn
        m2 = m2 + qb + d * d * n * nb[b] / nn
        n = nn
    return mean, m2 / n, n


def bn_fin_ref(c, mean, var, n, eps):
    r = types.SimpleNamespace()
    gm = c.theta[:, c.off_g:c.off_g + c.C].double()
    bt = c.theta[:, c.off_b:c.off_b + c.C].double()
    r.invstd = 1.0 / torch.sqrt(var + eps)
    r.scale = gm * r.invstd
    r.shift = bt - mean * r.scale
    r.shift_terms = bt.abs() + (mean * r.scale).abs()
    r.mean = mean
    rm = c.bufs[:, c.off_rm:c.off_rm + c.C].double()
    rv = c.bufs[:, c.off_rv:c.off_rv + c.C].double()
    unb = var * n / (n - 1.0)
    r.rm = (1.0 - MOM) * rm + MOM * mean
    r.rm_bound = K_RUN * U32 * (((1.0 - MOM) * rm).abs() + (MOM * mean).abs())
    r.rv = (1.0 - MOM) * rv + MOM * unb
    r.rv_bound = K_RUN * U32 * (((1.0 - MOM) * rv).abs() + (MOM * unb).abs())
    r.nbt = c.bufs[:, c.off_nbt].double() + 1
    return r


def bn_eval_case(G, C, exact):
    """bn_eval operands: running variance 4^j (with eps = 0 the square root and the quotient are exact), integer running
    mean and beta, gamma +-2^k."""
    g = L.gen("alex", "bneval", G, C, exact)
    c = bn_fin_case(1, 64, False, C, G)
    j = torch.randint(-2, 3, (G, C), generator=g)
    c.bufs[:, c.off_rv:c.off_rv + C] = torch.ldexp(torch.ones(G, C), 2 * j)
    c.eps = 0.0 if exact else EPS
    rm = c.bufs[:, c.off_rm:c.off_rm + C].double()
    rv = c.bufs[:, c.off_rv:c.off_rv + C].double()
    gm = c.theta[:, c.off_g:c.off_g + C].double()
    bt = c.theta[:, c.off_b:c.off_b + C].double()
    c.invstd = 1.0 / torch.sqrt(rv + c.eps)
    c.scale = gm * c.invstd
    c.shift = bt - rm * c.scale
    c.shift_terms = bt.abs() + (rm * c.scale).abs()
    c.rm = rm
    return c


BN_APPLY = [(2 * 175, 192, 175), (3 * 37, 24, 37)]      # (npos, C, S): the second is no multiple of the block's rows


def bn_apply_case(npos, C, S):
    g = L.gen("alex", "bnapply", npos, C, S)
    c = types.SimpleNamespace(npos=npos, C=C, S=S, G=npos // S)
    c.y = torch.randint(-4, 5, (npos, C), generator=g).to(torch.bfloat16)
    c.scale = pow2((c.G, C), -2, 2, g)
    c.scale[:, 5::8] = 0.0
    c.shift = torch.randint(-4, 5, (c.G, C), generator=g).float()
    z = c.y.double().view(c.G, S, C) * c.scale.double().unsqueeze(1) + c.shift.double().unsqueeze(1)
    assert torch.equal(z.float().double(), z)
    c.h = torch.relu(z).view(npos, C).to(torch.bfloat16)
    return c


# ================================================================================================ head.hip
HF, HH = 256, 64
HEAD_EVAL_B = (1, 32, 33, 70)
HEAD_TRAIN_B = (1, 8, 32)
HEAD_G = 2
# device expf / log1pf / logf / division: relative error allowed on top of the counted roundings.  Measured against fp64
# on an MI355X through db2 (at B = 1 it is dz2 = sigma(z) - y itself): at most 0.271 x 2^-24 of its terms; 4 x that, far
# below the 2^-20 above which the case would be mis-designed
DEV_REL = 1.1 * U32
K_HEAD = 8      # fp32 roundings from the logit to a gradient term: 1 + e, the quotient, - y, / B, the product, the sum
M64 = (1 << 64) - 1


def hash4(seed, a, b, c):
    """numpy uint64 transcription of hash4 in head.hip: a SplitMix64 finaliser of seed ^ golden * (a << 40 ^ b << 20 ^ c),
    high 32 bits."""
    a, b, c = (np.asarray(v, dtype=np.uint64) for v in (a, b, c))
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) ^ (np.uint64(0x9e3779b97f4a7c15) * ((a << np.uint64(40)) ^ (b << np.uint64(20)) ^ c))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def head_masks(seed, cids, B, keep, layer2_seed=None):
    """Keep masks [G, B, 256] and [G, B, 64] of the two dropout layers (layer 2 hashes seed ^ 0x5bd1e995)."""
    thr = np.uint64(int(keep * 4294967296.0))
    out = []
    for nf, s in ((HF, seed), (HH, (seed ^ 0x5bd1e995) if layer2_seed is None else layer2_seed)):
        g, b, f = np.meshgrid(np.asarray(cids), np.arange(B), np.arange(nf), indexing="ij")
        out.append(torch.from_numpy(hash4(s, g, b, f).astype(np.uint64) < thr))
    return out


def head_layout():
    """theta / grads row: [8 | w1 64x256 | 8 | b1 64 | 8 | w2 64 | 8 | b2 | 7]."""
    o = types.SimpleNamespace(w1=8, b1=8 + HH * HF + 8)
    o.w2 = o.b1 + HH + 8
    o.b2 = o.w2 + HH + 8
    o.ld = o.b2 + 8
    o.spans = [(o.w1, HH * HF), (o.b1, HH), (o.w2, HH), (o.b2, 1)]
    return o


def head_case(kind, G, B):
    """Head operands on the lattice.  kind "int": sparse integer weights (integer logits); kind "zero": the channel pairs
    (c, c + 64) of p5 are equal and hidden unit o + 32 mirrors unit o on the swapped feature halves with w2 negated, so
    every logit is exactly 0 while no gradient but db-free sums vanishes."""
    g = L.gen("alex", "head", kind, G, B)
    c = types.SimpleNamespace(G=G, B=B, NB=G * B, o=head_layout())
    p5 = torch.randint(-2, 3, (c.NB, 2, 128), generator=g)
    w1 = torch.randint(-1, 2, (G, HH, HF), generator=g) * (torch.rand(G, HH, HF, generator=g) < 0.125)
    b1 = torch.randint(-2, 3, (G, HH), generator=g)
    # about four non-zero output weights: integer logits of a few units, where the sigmoid is not saturated
    w2 = (torch.randint(0, 2, (G, HH), generator=g) * 2 - 1) * (torch.rand(G, HH, generator=g) < 1.0 / 16)
    b2 = torch.randint(-1, 2, (G,), generator=g)
    if kind == "zero":
        p5[:, :, 64:] = p5[:, :, :64]
        w1[:, 32:] = torch.roll(w1[:, :32], 128, 2)
        b1[:, 32:] = b1[:, :32]
        w2[:, :32] = torch.randint(0, 2, (G, 32), generator=g) * 2 - 1
        w2[:, 32:] = -w2[:, :32]
        b2[:] = 0
    c.p5 = p5.to(torch.bfloat16)
    c.w1, c.b1, c.w2, c.b2 = w1.double(), b1.double(), w2.double(), b2.double()
    c.theta = torch.full((G, c.o.ld), FILL)
    c.theta[:, c.o.w1:c.o.w1 + HH * HF] = w1.float().view(G, -1)
    c.theta[:, c.o.b1:c.o.b1 + HH] = b1.float()
    c.theta[:, c.o.w2:c.o.w2 + HH] = w2.float()
    c.theta[:, c.o.b2] = b2.float()
    c.y = torch.randint(0, 2, (c.NB,), generator=g).float()
    return c


def head_ref(c, train, keep=1.0, masks=None):
    """fp64 forward / backward of the head from the header: flattened feature f = c 2 + h of the [2, 128] map, dropout by
    keep masks scaled 1 / keep, BCE-with-logits mean over the client's batch."""
    G, B = c.G, c.B
    F0 = c.p5.double().permute(0, 2, 1).reshape(G, B, HF)                # f = c * 2 + h
    r = types.SimpleNamespace()
    m1 = masks[0].double() / keep if masks is not None else torch.ones_like(F0)
    Ff = F0 * m1
    z1 = torch.einsum("gof,gbf->gbo", c.w1, Ff) + c.b1.unsqueeze(1)
    m2 = masks[1].double() / keep if masks is not None else torch.ones_like(z1)
    Hd = torch.relu(z1) * m2
    r.logits = (Hd * c.w2.unsqueeze(1)).sum(2) + c.b2.view(G, 1)
    if not train:
        return r
    y = c.y.double().view(G, B)
    z = r.logits
    r.lossn = torch.relu(z) - z * y + torch.log1p(torch.exp(-z.abs()))
    r.loss = r.lossn.mean(1)
    sig = torch.sigmoid(z)
    dz2 = (sig - y) / B
    e2 = (sig.abs() + (sig - y).abs()) / B                               # magnitude the device error of dz2 scales with
    dz1 = dz2.unsqueeze(2) * c.w2.unsqueeze(1) * m2 * (z1 > 0)
    a1 = e2.unsqueeze(2) * c.w2.abs().unsqueeze(1) * m2 * (z1 > 0)
    r.g = dict(b2=dz2.sum(1, keepdim=True), w2=torch.einsum("gb,gbo->go", dz2, Hd), b1=dz1.sum(1),
               w1=torch.einsum("gbo,gbf->gof", dz1, Ff).reshape(G, -1))
    r.t = dict(b2=e2.sum(1, keepdim=True), w2=torch.einsum("gb,gbo->go", e2, Hd.abs()), b1=a1.sum(1),
               w1=torch.einsum("gbo,gbf->gof", a1, Ff.abs()).reshape(G, -1))
    dF = torch.einsum("gbo,gof->gbf", dz1, c.w1) * m1
    tF = torch.einsum("gbo,gof->gbf", a1, c.w1.abs()) * m1
    r.dp5 = dF.view(c.NB, 128, 2).permute(0, 2, 1).contiguous()
    r.dp5_t = tF.view(c.NB, 128, 2).permute(0, 2, 1).contiguous()
    return r


# (HW, C, K, B, exact): exact = equal class rows on pairwise-equal channels, K a power of two
CLS_G = 2
CLS_CASES = [(1, 2, 1, 1, True), (16, 64, 256, 4, True), (16, 512, 256, 1, True), (1, 512, 16, 4, True),
             (16, 64, 10, 4, False), (1, 2, 10, 1, False), (16, 512, 10, 4, False)]
K_CLS = 24     # exp, the K = 10 term sum (10), quotient, - onehot, / B, product and sum of a gradient entry, + margin


def cls_case(HW, C, K, B, exact):
    """cls_head_train operands: integer activations (their mean over HW = 1 or 16 positions is dyadic).  exact: channel
    c + C/2 repeats channel c and every class row is w with w[c + C/2] = -w[c], bias 0, so every logit is exactly 0 and
    the softmax exactly 1 / K.  Otherwise the K = 10 class rows give distinct small integer logits."""
    g = L.gen("alex", "cls", HW, C, K, B, exact)
    G = CLS_G
    c = types.SimpleNamespace(HW=HW, C=C, K=K, B=B, G=G, N=G * B, exact=exact)
    a = torch.randint(-2, 3, (c.N, HW, C), generator=g) * 16
    if exact:
        a[:, :, C // 2:] = a[:, :, :C // 2]
        row = torch.randint(-1, 2, (G, 1, C // 2), generator=g)
        W = torch.cat([row, -row], 2).expand(G, K, C).contiguous()
        bias = torch.zeros(G, K)
    else:
        a = a // 16
        a[:, 0, 0] = torch.randint(-2, 3, (c.N,), generator=g) * HW      # channel 0 pools to an integer in {-2..2};
        a[:, 1:, 0] = 0                                                   # it alone feeds the logits: small integers
        W = torch.zeros(G, K, C, dtype=torch.int64)
        W[:, :, 0] = torch.arange(K).view(1, K) % 4
        bias = (torch.arange(K).view(1, K).expand(G, K) % 3).float()
    c.a = a.to(torch.bfloat16)
    c.W, c.bias = W.double(), bias.double()
    c.off_w, c.off_b = 8, 8 + K * C + 8
    c.ld = c.off_b + K + 8
    c.ld += c.ld % 2
    c.spans = [(c.off_w, K * C), (c.off_b, K)]
    c.theta = torch.full((G, c.ld), FILL)
    c.theta[:, c.off_w:c.off_w + K * C] = W.float().view(G, -1)
    c.theta[:, c.off_b:c.off_b + K] = bias.float()
    c.y = torch.randint(0, K, (c.N,), generator=g)
    # reference
    c.pooled = c.a.double().mean(1)
    z = torch.einsum("gkc,gbc->gbk", c.W, c.pooled.view(G, B, C)) + c.bias.unsqueeze(1)
    c.z = z.view(c.N, K)
    lse = torch.logsumexp(c.z, 1)
    c.lossn = lse - c.z.gather(1, c.y.view(-1, 1)).squeeze(1)
    c.losses = c.lossn.view(G, B).mean(1)
    p = torch.softmax(c.z, 1)
    oh = F.one_hot(c.y, K).double()
    c.dlog = (p - oh) / B
    c.dlog_t = (p + oh) / B
    dl = c.dlog.view(G, B, K)
    c.dW = torch.einsum("gbk,gbc->gkc", dl, c.pooled.view(G, B, C)).reshape(G, -1)
    c.dW_t = torch.einsum("gbk,gbc->gkc", c.dlog_t.view(G, B, K), c.pooled.abs().view(G, B, C)).reshape(G, -1)
    c.db = dl.sum(1)
    c.db_t = c.dlog_t.view(G, B, K).sum(1)
    c.da = (torch.einsum("gbk,gkc->gbc", dl, c.W) / HW).view(c.N, 1, C).expand(c.N, HW, C)
    c.da_t = (torch.einsum("gbk,gkc->gbc", c.dlog_t.view(G, B, K), c.W.abs()) / HW).view(c.N, 1, C).expand(c.N, HW, C)
    return c
