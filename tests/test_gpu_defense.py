"""GPU tests of ``csrc/kernels/defense.hip`` (``rows_diff_norm``, ``clipped_rows_sum``) and of
``FLRunner.aggregate_defended`` on the device.

Shapes: P = 3 (the scalar tail only), 4099 (several threads and a tail, one block per row in the norm kernel) and
262147 (33 norm blocks per row — ``rows_diff_norm_blocks`` is asserted below — and 257 blocks in the sum kernel)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from neuroimagedisttraining_amd.engine import defense as DF
from neuroimagedisttraining_amd.engine import masks as MK

pytestmark = pytest.mark.gpu

DEV = "cuda"
P_BIG = 262147  # 32 * 8192 + 3: the norm kernel's block chunk is 8192 columns


def _m():
    from neuroimagedisttraining_amd import ops
    return ops.ext()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _backing(C, P, fill=0.0):
    """``[C + 2, ld]`` backing store (``ld`` = P rounded up to 64) and its ``[C, ld]`` middle rows."""
    ld = (P + 63) // 64 * 64
    back = torch.full((C + 2, ld), fill, dtype=torch.float32, device=DEV)
    return back, back[1:1 + C]


def _launch(rows, ref, wts, C, P, bound, stddev=0.0, seed=0, cids=None, mbits=None, out=None):
    """Both kernels on ``rows`` (a ``[C, ld]`` view); returns (norm [C], out [Pp])."""
    m = _m()
    nblk = m.rows_diff_norm_blocks(P)
    part = torch.full((C, nblk), float("nan"), dtype=torch.float64, device=DEV)
    norm = torch.full((C,), float("nan"), dtype=torch.float32, device=DEV)
    m.rows_diff_norm(rows.data_ptr(), ref.data_ptr(), C, P, rows.stride(0), part.data_ptr(), norm.data_ptr(), _st())
    if out is None:
        out = torch.zeros((P + 63) // 64 * 64, dtype=torch.float32, device=DEV)
    if cids is None:
        cids = torch.arange(C, dtype=torch.int32, device=DEV)
    m.clipped_rows_sum(rows.data_ptr(), ref.data_ptr(), wts.data_ptr(), norm.data_ptr(), cids.data_ptr(), C, P,
                       rows.stride(0), float(bound), float(stddev), int(seed),
                       mbits.data_ptr() if mbits is not None else 0, out.data_ptr(), _st())
    torch.cuda.synchronize()
    return norm, out


def _oracle(rows, ref, wts, norm, P, bound):
    """fp64 evaluation of sum_c w_c ((rows_c - ref) / max(1, norm_c / bound) + ref) with the given norms."""
    d = rows[:, :P].double() - ref.double()
    mc = torch.clamp_min(norm.double() / bound, 1.0).view(-1, 1)
    return (wts.double().view(-1, 1) * (d / mc + ref.double())).sum(0)


# ---------------------------------------------------------------------------------------------- 1. lattice
# (norm k, planted value v): (k / v)^2 entries of +-v, every other difference 0, so the squared norm is k^2 exactly
LATTICE_BOUND = 8.0
LATTICE_ROWS = [(16, 4), (7, None), (32, 4), (8, 4), (3, None)]    # m_c = 2, 1, 4, 1 (at the bound), 1
LATTICE_WTS = [0.5, 2.0, 0.25, 1.0, 0.125]


def _plant(P, k, v):
    """(positions, integer differences) with sum of squares k^2."""
    if v is None:
        vals = {7: [2, -3, 6], 3: [-1, 2, 2]}[k]
        pos = [0, P // 2, P - 1] if P > 3 else [0, 1, 2]
        return pos, vals
    if P == 3:  # one entry carries the whole norm
        return [k % 3], [-k]
    n = (k // v) ** 2
    pos = np.unique(np.linspace(0, P - 1, n).astype(np.int64))
    assert len(pos) == n and pos[0] == 0 and pos[-1] == P - 1
    return pos.tolist(), [v if i % 2 == 0 else -v for i in range(n)]


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("P", [3, 4099, P_BIG])
def test_integer_lattice_is_bit_exact(P, C):
    """Small-integer rows and ref, squared norms that are perfect squares (< 2^24), power-of-two bound and weights,
    m_c in {1, 2, 4}: every intermediate of both kernels is exact in fp32, so ``norm`` is the planted integer and
    ``out`` equals the fp64 evaluation of the formula bit for bit."""
    nblk = _m().rows_diff_norm_blocks(P)
    assert nblk == {3: 1, 4099: 1, P_BIG: 33}[P]  # the largest shape reduces several blocks per row
    g = torch.Generator().manual_seed(P + C)
    ref = torch.randint(-8, 9, (P,), generator=g).float().to(DEV)
    back, rows = _backing(C, P)
    rows[:, :P] = ref
    for c in range(C):
        pos, vals = _plant(P, *LATTICE_ROWS[c])
        rows[c, torch.tensor(pos, device=DEV)] += torch.tensor(vals, dtype=torch.float32, device=DEV)
    wts = torch.tensor(LATTICE_WTS[:C], device=DEV)
    norm, out = _launch(rows, ref, wts, C, P, LATTICE_BOUND)
    want_norm = torch.tensor([float(k) for k, _ in LATTICE_ROWS[:C]], device=DEV)
    assert torch.equal(norm, want_norm), (norm, want_norm)
    mc = torch.clamp_min(want_norm / LATTICE_BOUND, 1.0)
    assert set(mc.tolist()) <= {1.0, 2.0, 4.0} and (C == 1 or set(mc.tolist()) == {1.0, 2.0, 4.0})
    want = _oracle(rows, ref, wts, want_norm, P, LATTICE_BOUND)
    assert torch.equal(want.float().double(), want)  # the oracle itself is exactly representable
    assert torch.equal(out[:P], want.float())
    assert float(out[P:].abs().max() if out.numel() > P else 0.0) == 0.0


# ---------------------------------------------------------------------------------------------- 2. guards
def test_padding_and_neighbour_rows_are_never_read_and_out_tail_is_untouched():
    C, P = 3, 4099
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(P, generator=g).to(DEV)
    data = ref + 0.1 * torch.randn(C, P, generator=g).to(DEV)
    wts = torch.tensor([0.5, 0.3, 0.2], device=DEV)
    back, rows = _backing(C, P)
    rows[:, :P] = data
    norm0, out0 = _launch(rows, ref, wts, C, P, 4.0)
    assert bool(torch.isfinite(norm0).all()) and bool(torch.isfinite(out0).all())

    back, rows = _backing(C, P, fill=float("nan"))  # NaN padding columns, NaN rows above and below
    rows[:, :P] = data
    assert bool(torch.isnan(back[0]).all()) and bool(torch.isnan(back[C + 1]).all())
    assert bool(torch.isnan(rows[:, P:]).all()) and rows.shape[1] > P
    Pp = rows.shape[1]
    out = torch.full((Pp,), 777.0, dtype=torch.float32, device=DEV)  # poisoned, [P, Pp) must survive
    norm1, out1 = _launch(rows, ref, wts, C, P, 4.0, out=out)
    assert torch.equal(norm1, norm0)
    assert torch.equal(out1[:P], out0[:P])
    assert bool((out1[P:] == 777.0).all())


# ---------------------------------------------------------------------------------------------- 3. random data
def test_random_rows_against_fp64_oracle():
    C, P = 5, P_BIG
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(P, generator=g).to(DEV)
    scale = torch.tensor([0.02, 0.05, 0.1, 0.2, 0.3]).view(-1, 1)
    back, rows = _backing(C, P)
    rows[:, :P] = ref + (scale * torch.randn(C, P, generator=g)).to(DEV)
    wts = torch.rand(C, generator=g).to(DEV)
    bound = 30.0  # norms ~ scale * sqrt(P) = 10 .. 154: rows 0, 1 pass, rows 2 - 4 are clipped
    norm, out = _launch(rows, ref, wts, C, P, bound)
    want_norm = (rows[:, :P].double() - ref.double()).norm(dim=1)
    rel = float(((norm.double() - want_norm).abs() / want_norm).max())
    print("norm: largest relative error", rel)
    assert rel <= 1e-6
    assert int((norm > bound).sum()) == 3
    err = _relerr(out[:P], _oracle(rows, ref, wts, norm, P, bound))
    print("out: relative error", err)
    assert err < 1e-6


# ---------------------------------------------------------------------------------------------- 4. noise
def test_device_noise_matches_the_fp64_twin():
    """rows = ref = 0, one row of weight 1, stddev 1: ``out`` is ``z`` itself (0 + 1 * z and fma(1, z, 0) are exact).

    Bound on |z_device - z_twin|, from the accuracy the HIP math API documents for the device functions without fast
    math (logf 1 ulp, sqrtf 1 ulp, cospif at most 2 ulp) and not from a measurement: u1 >= 2^-24 gives
    |z| <= sqrt(2 * 24 * ln 2) = 5.77; u1, u2, -2 * log and 2 * u2 are exact scalings, the square root halves logf's
    relative error and adds its own ulp, cospif adds at most 2 ulp and the product rounds once: under 4 ulp relative,
    i.e. 5.77 * 4 * 2^-23 = 2.8e-6 absolute.  1e-5 leaves more than 3x headroom (the fp64 twin's own error is
    ~1e-15)."""
    P = 1 << 18
    seed, cid = DF.round_seed(7, 3), 11
    ref = torch.zeros(P, device=DEV)
    back, rows = _backing(1, P)
    wts = torch.ones(1, device=DEV)
    cids = torch.tensor([cid], dtype=torch.int32, device=DEV)
    _, out = _launch(rows, ref, wts, 1, P, 1.0, stddev=1.0, seed=seed, cids=cids)
    z = DF.noise_z_np(seed, cid, np.arange(P))
    err = float(np.abs(out[:P].double().cpu().numpy() - z).max())
    print("device noise: largest absolute error vs the fp64 twin", err)
    assert err <= 1e-5
    _, again = _launch(rows, ref, wts, 1, P, 1.0, stddev=1.0, seed=seed, cids=cids)
    assert torch.equal(out, again)
    # another client id or seed is another stream
    _, other = _launch(rows, ref, wts, 1, P, 1.0, stddev=1.0, seed=seed, cids=cids + 1)
    assert not torch.equal(out, other)

    # shared mask bits: unset coordinates come out as ref bit for bit, set ones as in the unmasked launch
    g = torch.Generator().manual_seed(4)
    P2 = 4099
    ref2 = torch.randn(P2, generator=g).to(DEV)
    back, rows2 = _backing(1, P2)
    rows2[:, :P2] = ref2
    keep = (torch.rand(P2, generator=g) < 0.5).to(DEV)
    bits = MK.pack_bits(keep.view(1, -1).float())
    _, full = _launch(rows2, ref2, wts, 1, P2, 1.0, stddev=1.0, seed=seed, cids=cids)
    _, masked = _launch(rows2, ref2, wts, 1, P2, 1.0, stddev=1.0, seed=seed, cids=cids, mbits=bits)
    assert torch.equal(masked[:P2][~keep], ref2[~keep])
    assert torch.equal(masked[:P2][keep], full[:P2][keep])
    assert not bool((full[:P2] == ref2).any())


# ---------------------------------------------------------------------------------------------- 5. runner
class SmallNet(nn.Module):
    """~21 k parameters (three norm-kernel blocks per row) with BatchNorm buffers."""

    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(nn.Conv3d(1, 4, 3, 2), nn.BatchNorm3d(4), nn.ReLU())
        self.classifier = nn.Sequential(nn.Linear(4, 160), nn.ReLU(), nn.Linear(160, 128), nn.ReLU(), nn.Linear(128, 1))

    def forward(self, x):
        return self.classifier(self.features(x).amax((2, 3, 4)))


SIZES = (10, 6, 12, 8, 4)


def _runner(device, **cfg_kw):
    from neuroimagedisttraining_amd.engine.executor import ClientSplit, FLConfig, FLRunner, TorchEngine
    from neuroimagedisttraining_amd.parallel import runtime as rt
    torch.manual_seed(0)
    splits, off = [], 0
    for n in SIZES:
        splits.append(ClientSplit(np.arange(off, off + n), np.arange(off + n, off + n + 2)))
        off += n + 2
    vols = torch.zeros((off, 9, 9, 9), dtype=torch.uint8)
    model = SmallNet()
    eng = TorchEngine(model, vols, torch.zeros(off), device)
    info = rt.DistInfo(0, 1, 0, torch.device(device), "none")
    cfg = FLConfig(comm_round=1, epochs=1, batch_size=4, seed=7, **cfg_kw)
    return FLRunner(eng, splits, cfg, info, model, algorithm="salientgrads")


def _set_rows(r):
    g = torch.Generator().manual_seed(9)
    mask = (torch.rand(r.P, generator=g) < 0.6).float()
    w = torch.randn(r.P, generator=g) * 0.5 * mask
    upd = torch.randn(r.N, r.P, generator=g) * torch.tensor([0.002, 0.02, 0.004, 0.03, 0.01]).view(-1, 1) * mask
    bufs = torch.rand(r.N, r.Q, generator=g)
    r.set_mask(mask.to(r.device))
    r.w_global.copy_(w)
    for c in range(r.N):
        r.theta[r.row_of[c], :r.P] = (w + upd[c]).to(r.device)
        r.bufs[r.row_of[c], :r.Q] = bufs[c].to(r.device)


@pytest.mark.parametrize("sampled", [[0, 1, 2, 3, 4], [2, 3, 4]], ids=["contiguous-kernels", "gathered-fallback"])
def test_runner_weak_dp_on_device_matches_its_cpu_fallback(sampled):
    """``FLRunner.aggregate`` with ``weak_dp`` on CUDA rows set by hand (SalientGrads mask active) against the same
    runner on the CPU (torch twin + numpy noise).  1e-5: the clipped sum alone agrees to ~1e-6 (the random-data test),
    the noise term adds the device functions' error (<= 2.8e-6, the noise test) times stddev <= 1."""
    from neuroimagedisttraining_amd.engine.runner import _contiguous
    kw = dict(defense_type="weak_dp", norm_bound=1.0, stddev=0.5)
    dev, cpu = _runner(DEV, **kw), _runner("cpu", **kw)
    assert _m().rows_diff_norm_blocks(dev.P) >= 3
    for r in (dev, cpu):
        _set_rows(r)
        r._round_idx = 2
    rows, _ = dev._local_rows(sampled)
    assert _contiguous(rows) == (len(sampled) == 5)  # the second case takes the torch fallback on the device
    g0 = dev.w_global.clone()
    dev.aggregate(sampled)
    cpu.aggregate(sampled)
    torch.cuda.synchronize()
    diff = float((dev.w_global.cpu() - cpu.w_global).abs().max())
    print("device vs CPU fallback: largest absolute difference", diff)
    assert torch.allclose(dev.w_global.cpu(), cpu.w_global, atol=1e-5)
    assert torch.allclose(dev.b_global.cpu(), cpu.b_global, atol=1e-6)
    assert not torch.equal(dev.w_global, g0)
    assert float(dev.w_global[dev.mask == 0].abs().max()) == 0.0  # pruned and 0 everywhere: no noise lands there
    assert dev.stat_info["defense_clipped"] == cpu.stat_info["defense_clipped"] > 0
    assert dev.stat_info["defense_max_ratio"] == pytest.approx(cpu.stat_info["defense_max_ratio"], rel=1e-5)
