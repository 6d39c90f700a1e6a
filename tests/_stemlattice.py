"""Integer-lattice operands, case tables and fp64 CPU references for the ten kernels of the 3D ResNet stem (stem.hip):
Conv3d(1, 64, 7, stride 2, pad 3) on raw uint8 volumes -> BatchNorm3d -> ReLU -> MaxPool3d(3, 2, 1), client-grouped,
forward and backward.

The references follow the header comment of stem.hip and the PyTorch modules, not the kernels' loops:

* polyphase: ``Xp[z'][y'][x'][r] = X[2z' - 4 + rd][2y' - 4 + rh][2x' - 4 + rw]`` (zero outside), r = 4 rd + 2 rh + rw, and
  the phase-major copy ``Xq[r][z'][y'][x']``.  The voxels are a hash of (volume, z, y, x), so no two axes or phase bits can
  be exchanged without changing bytes.
* slots: slot s = 8 t + r, t = 16 jd + 4 jh + jw, holds tap (kd, kh, kw) = (2 jd + rd - 1, 2 jh + rh - 1, 2 jw + rw - 1) when
  all three lie in [0, 7) and is empty otherwise (343 live, 169 empty).
* conv forward: integer weights |w| <= 8 against raw uint8 voxels give an integer accumulator below 343 * 255 * 8 < 2^24 in
  any summation order; the stored value is ``bf16_rne(fp32(acc * fl32(1 / 255)))`` - the product is exact in fp64.
* block statistics: mean and M2 = sum (y - mean)^2 of the stored bf16 values per (client, sample-in-client, od) block.
* pool: ``z = relu(y scale + shift)``, windows 3^3 / stride 2 / pad 1, the FIRST maximum in (d, h, w) scan order over the
  valid voxels, index kd 9 + kh 3 + kw of the full window.
* unpool: ``dz[v] = [y scale + shift > 0] * sum over the (<= 8) windows whose argmax is v of dpool``; block sums of dz and
  dz xhat, xhat = (y - mean) invstd.
* BN backward: dbeta = s1 = sum dz, dgamma = s2 = sum dz xhat, ``dy = gamma invstd (dz - s1 / M - xhat s2 / M)`` written as
  a dz + b y + d.  The sums take dz before its bf16 store, dy the stored dz (they differ only in mode 1 at the short
  shape, where a voxel collects 500 + a few units).
* weight gradient: ``slab[n][chunk][jd][c][(4 jh + jw) 8 + r] = sum over the chunk's positions of dy[pos][c]
  Xq[r][od + jd][oh + jh][ow + jw]`` for ALL 128 slots of a jd block (the kernels compute the 169 empty slots of the row as
  ordinary correlations too; only k_stem_wgrad_fin leaves them out), and the row ``dW[c][tap] = fp32(sum of the client's
  slabs / 255)``.

Counted bound of the block statistics at ragged shapes (``stats_bound``).  k_stem_fwd keeps, per (channel, position lane),
the shifted sums s1 = sum dv, s2 = sum dv^2, dv = y - sh with sh one stored value of the block, over n_l <= 2 OH terms,
converts them to (n_l, sh + s1 / n_l, s2 - s1^2 / n_l) and merges lanes with Chan's formula in 5 steps (4 shuffles, one LDS
step).  With u = 2^-24, per (block, channel) A = max |y|, R = max y - min y (so |dv|, |mean differences| <= R <= 2 A) and
N_b = OH OW:
  mean:  the n_l additions of s1 and the subtraction dv err by <= n_l u sum |dv|, i.e. 2 OH u R after the division; the
         division and the addition of sh add 2 u A; a merge step rounds the difference, the product, the quotient and the
         sum: <= 4 u 2 A.  With R <= 2 A:  E_mean = (4 OH + 2 + 40) u A = K_MEAN(OH) u A.
  M2:    s2 takes n_l fused multiply-adds of a dv with 1 rounding each (relative error (n_l + 2) u of sum dv^2); s1^2 / n_l
         errs by <= 2 n_l u (sum |dv|)^2 / n_l + 2 u s1^2 / n_l <= (2 n_l + 2) u sum dv^2 (Cauchy-Schwarz), the subtraction
         adds one rounding: (3 n_l + 5) u sum dv^2 in all.  A merge step adds <= 8 u of its terms.  Every term is bounded
         by Q = N_b R^2 (the conditioning of the shifted sums: a sum of squared deviations from any point of the block's
         range), and the error of the lane means enters each merge step through 2 |dm| E_mean n1 n2 / nn <= R E_mean N_b / 2:
         E_M2 = (6 OH + 5 + 40) u Q + 5 N_b R E_mean / 2 = K_M2(OH) u Q + 2.5 N_b R E_mean.
Both bounds come from the operation count alone; a dropped or doubled position moves the mean by about |y| / N_b, five
orders of magnitude above E_mean.

This is a plain helper module (CPU only, no fixtures): tests/test_cpu_stemlattice.py proves the preconditions and the
discriminating power, tests/test_gpu_exact_stem.py runs the kernels.
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

import _alexlattice as A
import _lattice as L
import _normlattice as NL

U32 = NL.U32
FILL = NL.FILL
EPS = NL.BN_EPS
MOM = NL.BN_MOM
SC = 64                                # stem channels
SK = 512                               # k-slots
TAPS = 343
WG_OD = 8                              # od planes per weight-gradient chunk (kWgOD)
INV255 = float(torch.tensor(1.0 / 255.0, dtype=torch.float32))      # fl32(1 / 255) as a double

G, B = 2, 2
N = G * B
IDX = (2, 0, 1, 0)                     # non-identity map into the store, volume 0 used twice
NVOL = 4                               # volumes in the store: volume 3 is never used

# name: ((D, H, W), classes it serves)
SHAPES = {
    "full": ((17, 13, 121), ("ow61", "wgrad4", "ring", "od9")),
    "short8": ((9, 20, 10), ("px8", "wgrad4", "ring")),
    "pow2": ((7, 15, 31), ("wgrad", "ring", "pow2")),
    "lane33": ((6, 9, 66), ("ow33", "wgrad")),
    "wide": ((5, 5, 128), ("ow64", "wgrad")),
}
CHAIN_SHAPE = "short8"                 # the smallest ragged shape: the chained random-operand case
AX_Y = ("sample", "od", "oh", "ow", "channel")
AX_Q = ("sample", "qd", "qh", "qw", "channel")
AX_STAT = ("client", "block", "channel")
AX_GC = ("client", "channel")
AX_SLAB = ("sample", "chunk", "jd", "channel", "slot")

# theta / gradient row: [8 | conv1.weight 64 x 343 | 8 | bn1.weight 64 | 8 | bn1.bias 64 | 8], fillers = FILL
OFF_W = 8
OFF_G = OFF_W + SC * TAPS + 8
OFF_B = OFF_G + SC + 8
LD = OFF_B + SC + 8
SPANS = [(OFF_W, SC * TAPS), (OFF_G, SC), (OFF_B, SC)]


def dims(shape):
    D, H, W = shape
    d = types.SimpleNamespace(D=D, H=H, W=W)
    d.OD, d.OH, d.OW = ((n - 1) // 2 + 1 for n in shape)
    d.PZ, d.PY, d.PX = d.OD + 3, d.OH + 3, d.OW + 3
    d.QD, d.QH, d.QW = ((o - 1) // 2 + 1 for o in (d.OD, d.OH, d.OW))
    d.nchunk = (d.OD + WG_OD - 1) // WG_OD
    d.M = B * d.OD * d.OH * d.OW
    return d


def shape_dims(name):
    return dims(SHAPES[name][0])


def shape_classes(name):
    """The classes of the issue's table a shape serves, derived from its extents (the table's labels are checked
    against these)."""
    d = shape_dims(name)
    out = set()
    if d.OW == 61 and d.PX == 64:
        out.add("ow61")
    if d.PX == 8 and d.OW == 5:
        out.add("px8")
    out.add("wgrad4" if d.PX % 8 == 0 else "wgrad")
    if d.OW == 33:
        out.add("ow33")
    if d.OW == 64 and d.W == 128:
        out.add("ow64")
    if d.OH >= 6:
        out.add("ring")
    if d.OD == 9:
        out.add("od9")
    if all(o & (o - 1) == 0 for o in (d.OH, d.OW)) and d.OH >= 8 and d.OW >= 8:
        out.add("pow2")
    return out


# ------------------------------------------------------------------------------------------------ slots
def stem_tap(s):
    """Tap index (kd 7 + kh) 7 + kw of slot s, or -1 for an empty slot (header of stem.hip)."""
    t, r = s >> 3, s & 7
    jd, jh, jw = t >> 4, (t >> 2) & 3, t & 3
    rd, rh, rw = r >> 2, (r >> 1) & 1, r & 1
    k = (2 * jd + rd - 1, 2 * jh + rh - 1, 2 * jw + rw - 1)
    if min(k) < 0 or max(k) > 6:
        return -1
    return (k[0] * 7 + k[1]) * 7 + k[2]


SLOT_TAP = [stem_tap(s) for s in range(SK)]


# ------------------------------------------------------------------------------------------------ volumes, polyphase
@functools.lru_cache(maxsize=None)
def volumes(name, kind="hash"):
    """[NVOL, D, H, W] uint8: a 32-bit integer hash of (volume, z, y, x), low byte ("hash") or one bit x 255 ("bin")."""
    D, H, W = SHAPES[name][0]
    v, z, y, x = np.meshgrid(np.arange(NVOL, dtype=np.uint64), np.arange(D, dtype=np.uint64),
                             np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64), indexing="ij")
    m = np.uint64(0xffffffff)
    h = ((v + np.uint64(1)) * np.uint64(0x9e3779b1) ^ (z + np.uint64(1)) * np.uint64(0x85ebca77)
         ^ (y + np.uint64(1)) * np.uint64(0xc2b2ae3d) ^ (x + np.uint64(1)) * np.uint64(0x27d4eb2f)) & m
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(0x2c1b3c6d)) & m
    h = ((h ^ (h >> np.uint64(12))) * np.uint64(0x297a2d39)) & m
    h = h ^ (h >> np.uint64(15))
    if kind == "bin":
        return torch.from_numpy((((h >> np.uint64(9)) & np.uint64(1)) * np.uint64(255)).astype(np.uint8))
    return torch.from_numpy((h & np.uint64(0xff)).astype(np.uint8))


def polyphase_ref(vols, d, bits=(0, 1, 2)):
    """(xp [n, PZ, PY, PX, 8], xq [n, 8, PZ, PY, PX]) of the given volumes [n, D, H, W].  ``bits``: which of (rd, rh, rw)
    forms bit 2, 1, 0 of the phase; (1, 0, 2) exchanges two phase bits (mutation checks)."""
    n = vols.shape[0]
    pad = torch.zeros((n, 2 * d.PZ, 2 * d.PY, 2 * d.PX), dtype=vols.dtype)
    pad[:, 4:4 + d.D, 4:4 + d.H, 4:4 + d.W] = vols
    v = pad.view(n, d.PZ, 2, d.PY, 2, d.PX, 2)                       # padded index 2 z' + rd = source index + 4
    ax = (2, 4, 6)
    xp = v.permute(0, 1, 3, 5, ax[bits[0]], ax[bits[1]], ax[bits[2]]).reshape(n, d.PZ, d.PY, d.PX, 8).contiguous()
    return xp, xp.permute(0, 4, 1, 2, 3).contiguous()


def phase_conv(xp, w):
    """The stride-1 4^3 convolution over the 8 phase channels of one polyphase image [PZ, PY, PX, 8] with the slot-ordered
    weights of w [64, 343] (fp64): the polyphase form of the header."""
    ws = torch.zeros(SC, SK, dtype=torch.float64)
    for s, k in enumerate(SLOT_TAP):
        if k >= 0:
            ws[:, s] = w[:, k].double()
    k5 = ws.view(SC, 4, 4, 4, 8).permute(0, 4, 1, 2, 3).contiguous()       # [c, r, jd, jh, jw]
    return F.conv3d(xp.double().permute(3, 0, 1, 2).unsqueeze(0), k5)[0]


# ------------------------------------------------------------------------------------------------ parameter rows
def theta_rows(w, gamma=None, beta=None):
    th = torch.full((w.shape[0], LD), FILL)
    th[:, OFF_W:OFF_W + SC * TAPS] = w.reshape(w.shape[0], -1)
    if gamma is not None:
        th[:, OFF_G:OFF_G + SC] = gamma
    if beta is not None:
        th[:, OFF_B:OFF_B + SC] = beta
    return th


def bn_rows(gen, gamma=None, beta=None):
    """A namespace in the format A.bn_fin_ref reads: gamma +-2^k / integer beta rows and running-statistics rows."""
    c = types.SimpleNamespace(G=G, C=SC)
    c.ldt, c.off_g, c.off_b = 24 + 2 * SC, 8, 16 + SC
    c.theta = torch.full((G, c.ldt), FILL)
    c.theta[:, 8:8 + SC] = A.pow2((G, SC), -2, 2, gen) if gamma is None else gamma
    c.theta[:, 16 + SC:16 + 2 * SC] = torch.randint(-4, 5, (G, SC), generator=gen).float() if beta is None else beta
    c.ldb, c.off_rm, c.off_rv, c.off_nbt = 32 + 2 * SC, 8, 16 + SC, 24 + 2 * SC
    c.bufs = torch.full((G, c.ldb), FILL)
    c.bufs[:, 8:8 + SC] = torch.randint(-8, 9, (G, SC), generator=gen).float()
    c.bufs[:, 16 + SC:16 + 2 * SC] = torch.randint(1, 9, (G, SC), generator=gen).float() / 64
    c.bufs[:, c.off_nbt] = torch.arange(G).float() + 2
    return c


# ------------------------------------------------------------------------------------------------ conv forward
def int_weights(gen):
    """[G, 64, 343] integers |w| <= 8: even channels dense, odd channels sparse (about 1 tap in 4)."""
    w = torch.randint(-8, 9, (G, SC, TAPS), generator=gen).float()
    keep = torch.rand(G, SC, TAPS, generator=gen) < 0.25
    keep[:, 0::2] = True
    return w * keep


def unit_weights(gen):
    """[G, 64, 343] with exactly 8 taps of +-1 per channel: |sum over any voxel subset| <= 8."""
    w = torch.zeros(G, SC, TAPS)
    for g in range(G):
        for c in range(SC):
            k = torch.randperm(TAPS, generator=gen)[:8]
            w[g, c, k] = (torch.randint(0, 2, (8,), generator=gen) * 2 - 1).float()
    return w


def conv_acc(vols, w, idx):
    """fp64 accumulators [n, OD, OH, OW, 64] of Conv3d(1, 64, 7, 2, 3) of sample n = stored volume idx[n] with its
    client's filters, on the raw byte values (no 1 / 255)."""
    out = []
    for n, i in enumerate(idx):
        x = vols[i].double().view(1, 1, *vols.shape[1:])
        out.append(F.conv3d(x, w[n // B].double().view(SC, 1, 7, 7, 7), stride=2, padding=3)[0].permute(1, 2, 3, 0))
    return torch.stack(out).contiguous()


def y_store(acc):
    """The stored value: one fp32 rounding of acc * fl32(1 / 255) (exact in fp64), one RNE to bf16."""
    return (acc * INV255).float().to(torch.bfloat16)


def stats_ref(y):
    """fp64 (mean, M2) [G, B OD, 64] of the stored values per block b = (sample in client) OD + od."""
    n, OD, OH, OW, C = y.shape
    yb = y.double().view(G, B * OD, OH * OW, C)
    mean = yb.mean(2)
    return mean, ((yb - mean.unsqueeze(2)) ** 2).sum(2)


def k_mean(OH):
    return 4 * OH + 2 + 40


def k_m2(OH):
    return 6 * OH + 5 + 40


def stats_bound(y):
    """(E_mean, E_M2) [G, B OD, 64] of the module docstring."""
    n, OD, OH, OW, C = y.shape
    yb = y.double().view(G, B * OD, OH * OW, C)
    Amax = yb.abs().amax(2)
    R = yb.amax(2) - yb.amin(2)
    nb = float(OH * OW)
    e_mean = k_mean(OH) * U32 * Amax
    return e_mean, k_m2(OH) * U32 * nb * R * R + 2.5 * nb * R * e_mean


@functools.lru_cache(maxsize=None)
def fwd_case(name):
    """Integer weights against the hashed volumes: accumulators, stored values and block statistics."""
    g = L.gen("stem", "fwd", name)
    c = types.SimpleNamespace(name=name, d=shape_dims(name))
    c.vols = volumes(name)
    c.idx = torch.tensor(IDX, dtype=torch.int32)
    c.w = int_weights(g)
    c.theta = theta_rows(c.w)
    c.acc_bound = L.require_fp32_exact(255.0 * float(c.w.abs().sum(2).max()), name + " conv accumulator")
    c.acc = conv_acc(c.vols, c.w, IDX)
    c.y = y_store(c.acc)
    c.mean, c.m2 = stats_ref(c.y)
    return c


@functools.lru_cache(maxsize=None)
def stat_case():
    """The power-of-two shape with 0 / 255 volumes and 8 unit taps per channel: every stored value is the integer
    acc / 255 in [-8, 8], every block has 8 x 16 positions, so every shifted sum and Chan merge of the kernel is exact
    (test_cpu_stemlattice proves both) and mean, M2 are compared bit for bit."""
    name = "pow2"
    g = L.gen("stem", "stat", name)
    c = types.SimpleNamespace(name=name, d=shape_dims(name))
    c.vols = volumes(name, "bin")
    c.idx = torch.tensor(IDX, dtype=torch.int32)
    c.w = unit_weights(g)
    c.bn = bn_rows(g)
    c.theta = theta_rows(c.w)
    c.acc = conv_acc(c.vols, c.w, IDX)
    c.m = c.acc / 255.0
    c.y = y_store(c.acc)
    c.mean, c.m2 = stats_ref(c.y)
    return c


@functools.lru_cache(maxsize=None)
def pack_case():
    g = L.gen("stem", "pack")
    w = torch.randn(G, SC, TAPS, generator=g) * 0.05
    bits = w.to(torch.bfloat16).view(torch.int16)
    ref = torch.zeros(G, SC, SK, dtype=torch.int16)
    for s, k in enumerate(SLOT_TAP):
        if k >= 0:
            ref[:, :, s] = bits[:, :, k]
    return types.SimpleNamespace(w=w, theta=theta_rows(w), wk=ref)


# ------------------------------------------------------------------------------------------------ pool
def rep(v):
    """[G, 64] -> per-sample rows broadcastable against [N, *, *, *, 64]."""
    return v.double().repeat_interleave(B, 0).view(-1, 1, 1, 1, v.shape[-1])


def affine(y, scale, shift):
    return y.double() * rep(scale) + rep(shift)


def pool_windows(z, d):
    """relu(z) [n, OD, OH, OW, C] -> [n, QD, QH, QW, C, 27] windows (3, stride 2, pad 1), -inf outside the map."""
    n, C = z.shape[0], z.shape[-1]
    zp = torch.full((n, 2 * d.QD + 1, 2 * d.QH + 1, 2 * d.QW + 1, C), -float("inf"), dtype=torch.float64)
    zp[:, 1:1 + d.OD, 1:1 + d.OH, 1:1 + d.OW] = torch.relu(z)
    w = zp.unfold(1, 3, 2).unfold(2, 3, 2).unfold(3, 3, 2)
    return w.reshape(n, d.QD, d.QH, d.QW, C, 27)


def pool_ref(z, d, last=False):
    """(pooled value fp64, argmax uint8): the first maximum of relu(z) in scan order over the valid voxels (``last``: the
    last one - mutation checks)."""
    win = pool_windows(z, d)
    am = 26 - win.flip(-1).argmax(-1) if last else win.argmax(-1)        # torch.argmax: the first of several maxima
    return win.amax(-1), am.to(torch.uint8)


def unpool_ref(dpool, amax, z, d, drop_k=None):
    """dz [n, OD, OH, OW, C] fp64: every window's gradient lands on its argmax voxel, masked by z > 0.  ``drop_k``: window
    offset kd 9 + kh 3 + kw whose contributions are left out (mutation checks)."""
    n, C = dpool.shape[0], dpool.shape[-1]
    full = torch.zeros(n, d.QD, d.QH, d.QW, C, 27, dtype=torch.float64)
    full.scatter_(-1, amax.long().unsqueeze(-1), dpool.double().unsqueeze(-1))
    if drop_k is not None:
        full[..., drop_k] = 0
    dzp = torch.zeros(n, 2 * d.QD + 1, 2 * d.QH + 1, 2 * d.QW + 1, C, dtype=torch.float64)
    for k in range(27):
        kd, kh, kw = k // 9, (k // 3) % 3, k % 3
        dzp[:, kd:kd + 2 * d.QD:2, kh:kh + 2 * d.QH:2, kw:kw + 2 * d.QW:2] += full[..., k]
    return torch.where(z > 0, dzp[:, 1:1 + d.OD, 1:1 + d.OH, 1:1 + d.OW], torch.zeros((), dtype=torch.float64))


def block_sums(dz, y, mean, invstd, skip=None):
    """(part [G, B OD, 64, 2], s1 [G, 64], s2 [G, 64]): per-block and per-client sums of dz and dz xhat.  ``skip``: a
    (client, block) left out of the client sums (mutation checks)."""
    n, OD, OH, OW, C = dz.shape
    xhat = (y.double() - rep(mean)) * rep(invstd)
    p1 = dz.view(G, B * OD, OH * OW, C).sum(2)
    p2 = (dz * xhat).view(G, B * OD, OH * OW, C).sum(2)
    part = torch.stack([p1, p2], 3)
    tot = part.clone()
    if skip is not None:
        tot[skip[0], skip[1]] = 0
    return part, tot[..., 0].sum(1), tot[..., 1].sum(1)


def coef_ref(s1, s2, gamma, invstd, mean, M):
    """(a, b, d) [G, 64, 3] fp64 of dy = gamma invstd (dz - s1 / M - xhat s2 / M) = a dz + b y + d."""
    gm, iv, mu = gamma.double(), invstd.double(), mean.double()
    return torch.stack([gm * iv, -gm * iv * iv * (s2 / M), -gm * iv * (s1 / M) + gm * iv * iv * mu * (s2 / M)], 2)


def dy_exact(coef, dz, y):
    a, b, dd = (rep(coef[:, :, i]) for i in range(3))
    return a * dz + (b * y.double() + dd)


def wgrad_ref(dy, xq, d, pos_mask=None):
    """Slabs [n, nchunk, 4 jd, 64, 128] fp64: sum over the chunk's output positions of dy[pos][c] Xq[r][pos + (jd, jh,
    jw)], slot (4 jh + jw) 8 + r.  ``pos_mask`` [OD, OH, OW]: positions left out (mutation checks)."""
    n = dy.shape[0]
    dy = dy.double()
    if pos_mask is not None:
        dy = dy * pos_mask.double().view(1, d.OD, d.OH, d.OW, 1)
    x = xq.double()
    slab = torch.zeros(n, d.nchunk, 4, SC, 128, dtype=torch.float64)
    for oc in range(d.nchunk):
        o0, o1 = oc * WG_OD, min(d.OD, (oc + 1) * WG_OD)
        for jd in range(4):
            for jh in range(4):
                for jw in range(4):
                    xs = x[:, :, o0 + jd:o1 + jd, jh:jh + d.OH, jw:jw + d.OW]
                    s0 = (jh * 4 + jw) * 8
                    slab[:, oc, jd, :, s0:s0 + 8] = torch.einsum("ndhwc,nrdhw->ncr", dy[:, o0:o1], xs)
    return slab


def row_ref64(slab):
    """[G, 64, 343] fp64: the sum of the client's slabs at the tap's slot / 255."""
    nchunk = slab.shape[1]
    tot = slab.double().view(G, B * nchunk, 4, SC, 128).sum(1)
    row = torch.zeros(G, SC, TAPS, dtype=torch.float64)
    for s, k in enumerate(SLOT_TAP):
        if k >= 0:
            row[:, :, k] = tot[:, s >> 7, :, s & 127]
    return row / 255.0


def row_ref(slab):
    """The gradient row: fp32(fp64(S) / 255)."""
    return row_ref64(slab).float()


PEAK = 8                               # planted strict maxima: |y| = 8 against |y| <= 2 elsewhere
DEAD_SHIFT = -64.0
CH_ZERO, CH_DEAD = 3, 5                # channels with scale 0 / with a shift below every y scale


@functools.lru_cache(maxsize=None)
def bn_case(name, mode=0):
    """Constructed inputs of stem_pool and stem_bwd with every intermediate of the backward as an exact fp64 tensor.

    y: bf16 integers in {-2..2} (ties in every window), the two samples of a client equal; gamma in +-{1, 2} (0 in channel
    CH_ZERO), invstd in {1, 2}, integer mean in [-1, 1] and beta in [-2, 2] (DEAD_SHIFT in channel CH_DEAD), so
    scale = gamma invstd, shift = beta - mean scale and z = y scale + shift are exact.  Client 0 carries a strict maximum
    at the odd voxel (1, 1, 1) (argmax of all 8 windows around it), client 1 at (0, 1, 1) (4 windows).
    dpool: bf16 integers in {-2..2}, sample 1 of a client the negative of sample 0, hence s1 = s2 = 0 per (client,
    channel): b = d = 0, a = gamma invstd, dy = a dz an exact bf16 integer (mode 0).
    mode 1: one pooled cell of sample 0 per (client, channel) - where a live argmax voxel with |y - mean| in {1, 2}
    exists - is set to ``delta`` (and to 0 in sample 1), with delta = M (M 2^-3 at the power-of-two shape) a bf16 number: s1 = delta and
    s2 = delta xhat0 with a power of two xhat0, so s1 / M and s2 / M are exact and b, d non-zero dyadic numbers.
    mode 2: delta = 128 where M is no power of two: inexact quotients (coefficients within one ulp; no slab check)."""
    g = L.gen("stem", "bn", name)
    c = types.SimpleNamespace(name=name, mode=mode, d=shape_dims(name))
    d = c.d
    c.idx = torch.tensor(IDX, dtype=torch.int32)
    y = torch.randint(-2, 3, (G, 1, d.OD, d.OH, d.OW, SC), generator=g)
    c.gamma = (torch.randint(1, 3, (G, SC), generator=g) * (torch.randint(0, 2, (G, SC), generator=g) * 2 - 1)).float()
    c.gamma[:, CH_ZERO] = 0.0
    c.invstd = torch.randint(1, 3, (G, SC), generator=g).float()
    c.mean = torch.randint(-1, 2, (G, SC), generator=g).float()
    c.beta = torch.randint(-2, 3, (G, SC), generator=g).float()
    c.beta[:, CH_DEAD] = DEAD_SHIFT
    c.beta[:, CH_ZERO] = torch.tensor([3.0, -3.0])                  # z = shift: a constant live / dead channel
    c.scale = c.gamma * c.invstd
    c.shift = c.beta - c.mean * c.scale
    sgn = torch.where(c.scale < 0, -1, 1)
    y[0, 0, 1, 1, 1] = PEAK * sgn[0]
    y[1, 0, 0, 1, 1] = PEAK * sgn[1]
    c.y = y.expand(G, B, d.OD, d.OH, d.OW, SC).reshape(N, d.OD, d.OH, d.OW, SC).to(torch.bfloat16).contiguous()
    c.z = affine(c.y, c.scale, c.shift)
    assert torch.equal(c.z.float().double(), c.z)
    out, c.amax = pool_ref(c.z, d)
    assert torch.equal(out.to(torch.bfloat16).double(), out), "pooled lattice value is no bf16 number"
    c.out = out.to(torch.bfloat16)
    dp = torch.randint(-2, 3, (G, 1, d.QD, d.QH, d.QW, SC), generator=g).double()
    dp = torch.cat([dp, -dp], 1).reshape(N, d.QD, d.QH, d.QW, SC).contiguous()
    c.delta = 0.0
    c.planted = torch.zeros(G, SC, dtype=torch.bool)
    if mode:
        pw2 = d.M & (d.M - 1) == 0
        c.delta = float(d.M) / 8 if (mode == 1 and pw2) else float(d.M) if mode == 1 else 128.0
        assert float(torch.tensor(c.delta).to(torch.bfloat16)) == c.delta, "delta is no bf16 number"
        win = pool_windows(c.z, d)
        for gi in range(G):
            n0 = gi * B
            ywin = pool_windows(c.y[n0:n0 + 1].double() + 100.0, d) - 100.0        # y of every window candidate
            ya = ywin[0].gather(-1, c.amax[n0].long().unsqueeze(-1)).squeeze(-1)   # y at the argmax voxel
            live = win[n0].amax(-1) > 0
            dev = (ya - c.mean[gi].double()).abs()
            ok = live & ((dev == 1) | (dev == 2))
            for ch in range(SC):
                cells = torch.nonzero(ok[..., ch])
                if len(cells):
                    qd, qh, qw = (int(v) for v in cells[len(cells) // 2])
                    dp[n0, qd, qh, qw, ch] = c.delta
                    dp[n0 + 1, qd, qh, qw, ch] = 0.0
                    c.planted[gi, ch] = True
    c.dpool = dp.to(torch.bfloat16)
    assert torch.equal(c.dpool.double(), dp)
    c.dz = unpool_ref(dp, c.amax, c.z, d)
    c.part, c.s1, c.s2 = block_sums(c.dz, c.y, c.mean, c.invstd)
    c.coef = coef_ref(c.s1, c.s2, c.gamma, c.invstd, c.mean, float(d.M))
    c.theta = theta_rows(torch.full((G, SC, TAPS), FILL), c.gamma, c.beta)
    c.exact = mode != 2
    if not c.exact:
        return c
    c.dy64 = dy_exact(c.coef, c.dz.float().to(torch.bfloat16).double(), c.y)     # the weight gradient reads the STORED dz
    c.dy = c.dy64.float().to(torch.bfloat16)            # one RNE of an exact fp32 value (asserted on the CPU)
    c.vols = volumes(name)
    _, c.xq = polyphase_ref(c.vols[list(IDX)], d)
    c.slab = wgrad_ref(c.dy, c.xq, d)
    c.row = row_ref(c.slab)
    return c


def bn_cases():
    """(shape, mode) of every backward case: mode 0 everywhere, mode 1 where delta = M (or M / 8) is a bf16 number - one
    k_stem_wgrad and one k_stem_wgrad4 shape -, mode 2 at a ragged shape."""
    return [(n, 0) for n in SHAPES] + [("pow2", 1), ("short8", 1), ("lane33", 2)]


# ------------------------------------------------------------------------------------------------ chained random case
K_CONV = TAPS + 2                      # fp32 roundings of a stored conv value before the bf16 store: the sum, x 1/255
K_POOL = 1                             # the fma of z
K_DY = 3                               # two fmas and the bf16-boundary margin
SKIP_MAX = 0.01                        # largest share of near-tie / near-threshold elements left out per tensor


@functools.lru_cache(maxsize=None)
def chain_case():
    """Random (non-lattice) operands of the chained test at CHAIN_SHAPE."""
    name = CHAIN_SHAPE
    g = L.gen("stem", "chain", name)
    c = types.SimpleNamespace(name=name, d=shape_dims(name))
    c.vols = volumes(name)
    c.idx = torch.tensor(IDX, dtype=torch.int32)
    c.w = torch.randn(G, SC, TAPS, generator=g) * 0.05
    c.bn = bn_rows(g, gamma=torch.rand(G, SC, generator=g) + 0.5, beta=torch.randn(G, SC, generator=g) * 0.2)
    c.theta = theta_rows(c.w, c.bn.theta[:, c.bn.off_g:c.bn.off_g + SC], c.bn.theta[:, c.bn.off_b:c.bn.off_b + SC])
    c.dpool = torch.randn(N, c.d.QD, c.d.QH, c.d.QW, SC, generator=g).to(torch.bfloat16)
    return c


def ulp_bf16(v):
    return 2.0 * NL.halfulp_bf16(v)


def chain_fwd_ref(c):
    """fp64 conv of the bf16-rounded weights, x / 255, and the bound of the stored value."""
    wb = c.w.to(torch.bfloat16).double()
    y = conv_acc(c.vols, wb, IDX) / 255.0
    mag = conv_acc(c.vols, wb.abs(), IDX) / 255.0
    return y, NL.bf16_bound(y, K_CONV * U32 * mag)


def chain_pool_ref(y, scale, shift, d):
    """From the device's y, scale, shift: (z, pooled value, bound, argmax, windows to skip).  A window is skipped when its
    two largest DISTINCT candidates lie within one bf16 ulp of each other, or its maximum within one bf16 ulp of 0."""
    z = affine(y, scale, shift)
    zmag = (y.double() * rep(scale)).abs() + rep(shift).abs()
    win = pool_windows(z, d)
    out, am = pool_ref(z, d)
    u = ulp_bf16(out.abs().clamp_min(2.0 ** -20))
    second = torch.where(win < out.unsqueeze(-1), win, torch.full_like(win, -float("inf"))).amax(-1)
    skip = ((out - second) <= u) | ((out > 0) & (out <= u))
    mwin = pool_windows(zmag, d).clamp_min(0).amax(-1)
    return z, zmag, out, NL.bf16_bound(out, K_POOL * U32 * mwin), am, skip


def near_threshold(z, zmag):
    """Voxels whose z lies within one bf16 ulp (at the size of its terms) of the ReLU threshold."""
    return z.abs() <= ulp_bf16(zmag.clamp_min(2.0 ** -20))


def chain_slab_bound(coef, dz, y, xq, d):
    """(reference slabs, bound): dy = bf16(a dz + b y + d) is internal to the kernel; its fp32 value is within K_DY u of
    the terms of the fp64 value, so the store can differ by one bf16 ulp only where the fp64 value lies that close to a
    rounding boundary.  The bound sums x * that ulp over such positions, plus the fp32 accumulation of the slab (one
    rounding per position of the chunk on the running sum of |dy| x)."""
    a, b, dd = (rep(coef[:, :, i]) for i in range(3))
    v = a * dz.double() + (b * y.double() + dd)
    terms = (a * dz.double()).abs() + (b * y.double()).abs() + dd.abs()
    e32 = K_DY * U32 * terms
    dyb = v.float().to(torch.bfloat16).double()
    u = ulp_bf16(v.abs().clamp_min(2.0 ** -100))
    flip = ((v - dyb).abs() >= 0.5 * u - e32 - 2.0 ** -60 * terms)
    npos = min(d.OD, WG_OD) * d.OH * d.OW
    slab = wgrad_ref(dyb, xq, d)
    bound = wgrad_ref(u * flip + npos * U32 * dyb.abs(), xq, d)
    return slab, bound
