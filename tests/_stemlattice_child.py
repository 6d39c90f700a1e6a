"""Runners of the stem lattice checks on the GPU (raw bindings of stem.hip), shared by tests/test_gpu_exact_stem.py and
by the child process it starts for the environment-selected weight-gradient kernel (NIDT_STEM_WG4 is read once per
process).  As a program: ``python _stemlattice_child.py SHAPE MODE`` rebuilds the backward case ``bn_case(SHAPE, MODE)`` of
tests/_stemlattice.py, runs stem_bwd with whatever kernel the environment selects and checks every slab entry and the
gradient row; it prints the coordinates of the first mismatch and exits non-zero.

Every output buffer starts as NaN (uint8 buffers as 255) and carries guard rows of the sentinel behind its end; the
parameter and gradient rows sit between filler columns that must stay untouched."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import _lattice as L  # noqa: E402
import _stemlattice as S  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SENT = -96.0
SENT8 = 0xA5


def ext():
    from neuroimagedisttraining_amd import ops
    return ops.ext()


def _st():
    return torch.cuda.current_stream().cuda_stream


def nan(*shape, dtype=torch.float32, guard=1):
    """NaN buffer whose first axis gets ``guard`` extra sentinel rows (checked by ``guard_ok``)."""
    b = torch.full((shape[0] + guard,) + tuple(shape[1:]), NAN, device=DEV, dtype=dtype)
    b[shape[0]:] = SENT
    return b


def u8(*shape, guard=1):
    b = torch.full((shape[0] + guard,) + tuple(shape[1:]), 255, device=DEV, dtype=torch.uint8)
    b[shape[0]:] = SENT8
    return b


def guard_ok(n, *bufs):
    torch.cuda.synchronize()
    for b in bufs:
        want = SENT8 if b.dtype == torch.uint8 else SENT
        assert bool((b[n:].float() == want).all()), "rows behind the end of an output buffer were written"


def untouched(*pairs):
    """No element of the (rows, buffer) pairs was written: NaN / 255 bodies, sentinel guards."""
    torch.cuda.synchronize()
    for n, b in pairs:
        ok = bool((b[:n] == 255).all()) if b.dtype == torch.uint8 else bool(torch.isnan(b[:n].float()).all())
        assert ok, "a kernel ran: an output buffer lost its initial fill"
        guard_ok(n, b)


def rows_ok(rows, spans, what):
    keep = torch.ones(rows.shape[1], dtype=torch.bool)
    for off, n in spans:
        keep[off:off + n] = False
    assert bool((rows.cpu()[:, keep] == S.FILL).all()), what + ": a filler column changed"


def bits_equal(got, ref, names, what):
    """Bit equality of two 16-bit (bf16 / int16) tensors."""
    e = S.A.first_mismatch(got.cpu().contiguous().view(torch.int16), ref.contiguous().view(torch.int16), names)
    assert e is None, what + ": " + e


def run_polyphase(m, vols, idx, d, train=True):
    """stem_polyphase of the whole store: xp [N, PZ, PY, PX, 8], xq [N, 8, PZ, PY, PX] (None in the eval form)."""
    n = idx.numel()
    xp = u8(n, d.PZ, d.PY, d.PX, 8)
    xq = u8(n, 8, d.PZ, d.PY, d.PX)
    m.stem_polyphase(vols.data_ptr(), idx.data_ptr(), n, d.D, d.H, d.W, xp.data_ptr(), xq.data_ptr() if train else 0, _st())
    guard_ok(n, xp, xq)
    return xp, xq


def run_fwd(m, xp, theta, d, n=S.N, b=S.B):
    """stem_fwd: (wk [G, 64, 512] int16 bits, y [n, OD, OH, OW, 64] bf16, stats [G, B OD, 64, 2])."""
    g = n // b
    wk = torch.full((g + 1, S.SC, S.SK), -1, dtype=torch.int16, device=DEV)
    y = nan(n, d.OD, d.OH, d.OW, S.SC, dtype=torch.bfloat16)
    stats = nan(n * d.OD, S.SC, 2, guard=4)
    m.stem_fwd(xp.data_ptr(), theta.data_ptr(), theta.stride(0), S.OFF_W, n, b, d.D, d.H, d.W, wk.data_ptr(),
               y.data_ptr(), stats.data_ptr(), _st())
    guard_ok(n, y)
    guard_ok(n * d.OD, stats)
    assert bool((wk[g] == -1).all()), "packed weights of a client that does not exist were written"
    return wk[:g], y[:n], stats[:n * d.OD].view(g, b * d.OD, S.SC, 2)


def run_finalize(m, stats, bn, d, upd, eps=S.EPS):
    """bn_finalize with the stem's arguments: B OD blocks of OH OW positions per client."""
    n = S.G * S.SC
    o = {k: nan(n, guard=8) for k in ("scale", "shift", "mean", "invstd")}
    th, bf = bn.theta.to(DEV), bn.bufs.to(DEV)
    m.bn_finalize(stats.data_ptr(), S.B * d.OD, d.OH * d.OW, S.B * d.OD * d.OH * d.OW, S.G, S.SC, th.data_ptr(), bn.ldt,
                  bn.off_g, bn.off_b, bf.data_ptr(), bn.ldb, bn.off_rm, bn.off_rv, bn.off_nbt, S.MOM, eps,
                  o["scale"].data_ptr(), o["shift"].data_ptr(), o["mean"].data_ptr(), o["invstd"].data_ptr(), upd, _st())
    guard_ok(n, *o.values())
    return {k: v[:n].view(S.G, S.SC) for k, v in o.items()}, bf.cpu()


def run_pool(m, y, scale, shift, d):
    out = nan(S.N, d.QD, d.QH, d.QW, S.SC, dtype=torch.bfloat16)
    amax = u8(S.N, d.QD, d.QH, d.QW, S.SC)
    m.stem_pool(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), S.N, S.B, d.D, d.H, d.W, out.data_ptr(), amax.data_ptr(),
                _st())
    guard_ok(S.N, out, amax)
    return out[:S.N], amax[:S.N]


def bwd_bufs(d, n=S.N):
    g = n // S.B
    return dict(dz=nan(n, d.OD, d.OH, d.OW, S.SC, dtype=torch.bfloat16), part=nan(n * d.OD, S.SC, 2, guard=4),
                coef=nan(g * S.SC, 3, guard=8), slab=nan(n * d.nchunk * 4, S.SC, 128),
                grad=torch.full((g, S.LD), S.FILL, device=DEV))


def run_bwd(m, t, d, theta, bufs=None, n=S.N, b=S.B):
    """stem_bwd on device tensors t = dict(dpool, amax, y, xq, scale, shift, mean, invstd): dz, part, coef, slab, grad."""
    o = bufs or bwd_bufs(d, n)
    m.stem_bwd(t["dpool"].data_ptr(), t["amax"].data_ptr(), t["y"].data_ptr(), t["xq"].data_ptr(), t["scale"].data_ptr(),
               t["shift"].data_ptr(), t["mean"].data_ptr(), t["invstd"].data_ptr(), n, b, d.D, d.H, d.W, theta.data_ptr(),
               theta.stride(0), S.OFF_G, o["grad"].data_ptr(), S.LD, S.OFF_W, S.OFF_G, S.OFF_B, o["dz"].data_ptr(),
               o["part"].data_ptr(), o["coef"].data_ptr(), o["slab"].data_ptr(), _st())
    guard_ok(n, o["dz"])
    guard_ok(n * d.OD, o["part"])
    guard_ok(n // b * S.SC, o["coef"])
    guard_ok(n * d.nchunk * 4, o["slab"])
    g = n // b
    return dict(dz=o["dz"][:n], part=o["part"][:n * d.OD].view(g, b * d.OD, S.SC, 2),
                coef=o["coef"][:g * S.SC].view(g, S.SC, 3), grad=o["grad"].cpu(),
                slab=o["slab"][:n * d.nchunk * 4].view(n, d.nchunk, 4, S.SC, 128))


def bwd_inputs(c):
    t = {k: getattr(c, k).contiguous().to(DEV) for k in ("dpool", "amax", "y", "scale", "shift", "mean", "invstd")}
    t["xq"] = c.xq.to(DEV) if hasattr(c, "xq") else S.polyphase_ref(S.volumes(c.name)[list(S.IDX)], c.d)[1].to(DEV)
    return t


def check_wgrad(o, c, what):
    """Every slab entry of every block and the [64][343] gradient row, bit for bit."""
    assert bool(torch.isfinite(o["slab"]).all()), what + ": a slab entry was not written"
    L.assert_exact(o["slab"], c.slab, S.AX_SLAB)
    L.assert_exact(o["grad"][:, S.OFF_W:S.OFF_W + S.SC * S.TAPS].reshape(S.G, S.SC, S.TAPS), c.row,
                   ("client", "channel", "tap"))
    rows_ok(o["grad"], S.SPANS, what + " gradient row")


def main(name, mode):
    c = S.bn_case(name, int(mode))
    o = run_bwd(ext(), bwd_inputs(c), c.d, c.theta.to(DEV))
    check_wgrad(o, c, "stem_bwd %s mode %s" % (name, mode))
    print("slabs and gradient row ok (NIDT_STEM_WG4=%s, PX %d)" % (os.environ.get("NIDT_STEM_WG4", "1"), c.d.PX))


if __name__ == "__main__":
    try:
        main(sys.argv[1], sys.argv[2])
    except AssertionError as e:
        print("MISMATCH:", e)
        sys.exit(1)
