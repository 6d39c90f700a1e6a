"""GPU tests of ``csrc/kernels/secagg.hip`` (``secagg_upload``, ``secagg_masked_sum``, ``secagg_finish``) and of
``FLRunner.aggregate_secure`` on the device.

The rows of every kernel test are the middle of a ``[C + 2, ld]`` backing store whose guard rows and pad columns
``[P, ld)`` hold NaN, so a read outside them is counted as a non-finite value; every output carries a sentinel past its
last element.  P = 3: one thread's scalar tail; 4099: five blocks, the last with a three-column tail; 262147: 257
blocks.  All comparisons but the random-data bound are bit for bit: the protocol is integer arithmetic."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from neuroimagedisttraining_amd.algorithms import turboaggregate as TA
from neuroimagedisttraining_amd.engine import secagg as SA

pytestmark = pytest.mark.gpu

DEV = "cuda"
P = TA.P_DEFAULT
S = 2 ** 16
ROUND = 5
SENT_I32, SENT_I64, SENT_F32 = -7, -7, -7.0


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(n, K):
    """Rows, client ids (every third id of a federation of 3 K), keys, weights and the numpy uploads of all K rows
    with every peer listed: computed once per shape and shared (never modified)."""
    g = torch.Generator().manual_seed(1000 * K + n % 997)
    M = (torch.randn(K, n, generator=g) * 2.0).numpy()
    ids = [3 * k + 1 for k in range(K)]
    keys = SA.SecAggKeys(3 * K, SA.default_threshold(K), seed=K)
    sizes = [4 + 3 * ((5 * k) % 7) for k in range(K)]
    n_tot = float(sum(sizes))
    wts = [s / n_tot for s in sizes]
    full = [[(j, int(keys.key[c, j])) for j in ids if j != c] for c in ids]
    B = TA.saturation_bound(K)
    up = {seg: SA.upload_twin(M, ids, full, wts, ROUND, seg, S, B)[0] for seg in (0, 1)}
    for a in (M, up[0], up[1]):
        a.setflags(write=False)
    return M, ids, keys, sizes, wts, full, B, up


def _backing(M):
    """``M`` ``[C, n]`` as rows 1 .. C of a NaN ``[C + 2, ld]`` device store; returns (store, row list)."""
    C, n = M.shape
    ld = (n + 63) // 64 * 64
    back = torch.full((C + 2, ld), float("nan"), dtype=torch.float32, device=DEV)
    back[1:C + 1, :n] = torch.tensor(M).to(DEV)
    return back, list(range(1, C + 1))


SHAPES = [(n, K) for n in (3, 4099, 262147) for K in (2, 5, 8)]


# ------------------------------------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("n,K", SHAPES)
def test_upload_equals_the_numpy_twin(n, K):
    M, ids, keys, sizes, wts, full, B, up = _case(n, K)
    back, ridx = _backing(M)
    for seg in (0, 1):
        out = torch.full((K * n + 5,), SENT_I32, dtype=torch.int32, device=DEV)
        got, ev = SA.upload(back, ridx, n, ids, full, wts, ROUND, seg, S, B, out=out, hip=True)
        torch.cuda.synchronize()
        assert int(ev) == 0  # a read of a guard row or a pad column would have counted a NaN
        assert np.array_equal(got.cpu().numpy().astype(np.int64), up[seg])
        assert bool((out[K * n:] == SENT_I32).all())
    assert not np.array_equal(up[0], up[1])


def _masked_sum(back, rows, n, cids, peers, wts, seg, B):
    out = torch.full((n + 4,), SENT_I64, dtype=torch.int64, device=DEV)
    ev = SA.masked_sum(back, rows, n, cids, peers, wts, ROUND, seg, S, B, out, hip=True)
    assert bool((out[n:] == SENT_I64).all()) and int(out[:n].min()) >= 0 and int(out[:n].max()) < P
    return out[:n], int(ev)


def _finish(total, n, pairs, seg, a, scale=S):
    out = torch.full((n + 3,), SENT_F32, dtype=torch.float32, device=DEV)
    SA.finish(total.contiguous(), n, pairs, ROUND, seg, scale, a, out, hip=True)
    assert bool((out[n:] == SENT_F32).all())
    return out[:n]


@pytest.mark.parametrize("n,K", SHAPES)
def test_masked_sum_equals_the_summed_uploads_for_any_sharding_and_dropout(n, K):
    """One launch over the survivors (masks towards the dropped clients only), and the survivors split into 2 and 3
    groups, each launched with the other groups as remote peers and the partials added in int64: the column sum of
    the survivors' uploads mod p every time, and the same fp32 bits after ``secagg_finish`` (= the numpy twin's)."""
    M, ids, keys, sizes, wts, full, B, up = _case(n, K)
    back, ridx = _backing(M)
    seg = K % 2
    for ndrop in range(0, min(2, K - keys.T - 1) + 1):
        dropped = [ids[1], ids[K - 1]][:ndrop]
        al = [k for k in range(K) if ids[k] not in dropped]
        alive = [ids[k] for k in al]
        want = up[seg][al].sum(0) % P
        pairs = keys.removal_pairs(dropped, alive)
        a = float(sum(sizes[k] for k in al)) / float(sum(sizes))
        ref = SA.finish_twin(want, pairs, ROUND, seg, S, a)
        results = []
        for ngroups in (1, 2, 3):
            total = torch.zeros(n, dtype=torch.int64, device=DEV)
            for grp in [al[i::ngroups] for i in range(ngroups)]:
                if not grp:
                    continue
                here = set(ids[k] for k in grp)
                peers = [[(j, key) for j, key in full[k] if j not in here] for k in grp]
                part, ev = _masked_sum(back, [ridx[k] for k in grp], n, [ids[k] for k in grp], peers,
                                       [wts[k] for k in grp], seg, B)
                assert ev == 0
                total += part
            torch.cuda.synchronize()
            assert np.array_equal(total.cpu().numpy() % P, want), (ndrop, ngroups)
            results.append(_finish(total, n, pairs, seg, a))
        torch.cuda.synchronize()
        assert np.array_equal(results[0].cpu().numpy().view(np.int32), ref.view(np.int32)), ndrop
        for r in results[1:]:
            assert torch.equal(_bits(r), _bits(results[0])), ndrop
    if K > 2:
        assert ndrop >= 1


def test_device_mersenne_fold_is_exact():
    """``sec_modp`` on chosen z, through ``secagg_finish`` with no pairs, S = 1 and a = 1: the output is the centred
    residue of ``sum`` read as an unsigned 64-bit value.  The edge values (the three partial terms of 2^64 - 1,
    2^64 - 2 and 0xBFFF...F add up to 2^32 or more) and z = q p + r with random q < 2^33 and |r| < 2^22 have small
    centred residues, which fp32 holds exactly."""
    edge = [0, 1, P - 1, P, P + 1, 2 * P, 2 * P + 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 62 - 1, 2 ** 62, 2 ** 62 + 1,
            2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 0xBFFFFFFFFFFFFFFF, 0xBFFFFFFFFFFFFFFE, 0xC000000000000000,
            0x7FFFFFFFFFFFFFFF, 0x3FFFFFFFFFFFFFFF, 2 ** 64 - 3, 2 ** 64 - 2, 2 ** 64 - 1, (2 ** 64 - 1) // P * P]
    rng = np.random.RandomState(3)
    q = rng.randint(1, 2 ** 33, 5000, dtype=np.int64)
    r = rng.randint(-2 ** 22, 2 ** 22, 5000, dtype=np.int64)
    z = edge + [int(a) * P + int(b) for a, b in zip(q, r)]
    assert all(0 <= v < 2 ** 64 for v in z)
    want = [v % P - (P if v % P > P // 2 else 0) for v in z]
    assert want[-5000:] == [int(b) for b in r] and want[len(edge) - 4:len(edge) - 1] == [1, 2, 3]
    host = np.array(z, dtype=np.uint64).view(np.int64)
    assert [int(v) for v in SA.finish_twin(host, [], 0, 0, 1, 1.0)] == want
    got = _finish(torch.from_numpy(host).to(DEV), len(z), [], 0, 1.0, scale=1)
    torch.cuda.synchronize()
    assert [int(v) for v in got.cpu().numpy()] == want


# ------------------------------------------------------------------------------------------------ 2. random data
@pytest.mark.parametrize("ndrop", [0, 2])
def test_random_data_within_the_quantisation_bound(ndrop):
    """``|secure - fp64 weighted mean| <= K_alive / (2 S a) + ulp32(result) / 2`` per coordinate.

    Client i sends ``q_i = rint(x_i S)`` with ``x_i = theta_i w_i``, so ``|q_i - x_i S| <= 1/2``; the masks cancel
    exactly and no value saturates, so the server decodes ``c = sum_alive q_i`` with ``|c - S sum_alive x_i| <=
    K_alive / 2``.  Dividing by ``S a`` gives ``|c / (S a) - mean| <= K_alive / (2 S a)`` for the survivors' weighted
    mean ``sum_alive x_i / a``, and the one rounding to fp32 adds at most half an ulp of the result.  (The fp64
    roundings of the products and divisions are 2^-53 relative: 1e-11 of the first term.)"""
    n, K = 4099, 8
    M, ids, keys, sizes, wts, full, B, up = _case(n, K)
    back, ridx = _backing(M)
    dropped = [ids[0], ids[5]][:ndrop]
    al = [k for k in range(K) if ids[k] not in dropped]
    alive = [ids[k] for k in al]
    peers = [[(j, key) for j, key in full[k] if j in dropped] for k in al]
    total, ev = _masked_sum(back, [ridx[k] for k in al], n, alive, peers, [wts[k] for k in al], 0, B)
    a = float(sum(sizes[k] for k in al)) / float(sum(sizes))
    got = _finish(total, n, keys.removal_pairs(dropped, alive), 0, a).cpu().numpy()
    mean = sum(M[k].astype(np.float64) * wts[k] for k in al) / a
    err = np.abs(got.astype(np.float64) - mean)
    bound = len(al) / (2.0 * S * a) + np.spacing(np.abs(got)).astype(np.float64) / 2
    print("largest error / bound", float((err / bound).max()), "largest error", float(err.max()))
    assert ev == 0 and bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------ 3. saturation
def test_saturated_and_non_finite_values_are_counted_and_stay_local():
    n, K = 4099, 5
    M, ids, keys, sizes, wts, full, B, up = _case(n, K)
    none = [[] for _ in range(K)]
    clean, ev0 = _masked_sum(*_backing(M), n, ids, none, wts, 0, B)
    bad = M.copy()
    bad[1, 7] = (B / S) / wts[1] * 1.01  # above B / S after weighting
    bad[2, 4098] = float("nan")
    bad[4, 2048] = float("inf")
    back, ridx = _backing(bad)
    dirty, ev = _masked_sum(back, ridx, n, ids, none, wts, 0, B)
    assert (ev0, ev) == (0, 3)
    got, ref = _finish(dirty, n, [], 0, 1.0), _finish(clean, n, [], 0, 1.0)
    same = torch.ones(n, dtype=torch.bool, device=DEV)
    same[[7, 2048, 4098]] = False
    assert torch.equal(_bits(got[same]), _bits(ref[same])) and bool(torch.isfinite(got).all())
    up_bad, ev_up = SA.upload(back, ridx, n, ids, full, wts, ROUND, 0, S, B, hip=True)
    assert int(ev_up) == 3  # the same rows one by one: the count does not depend on which rows share a launch
    assert np.array_equal(up_bad.sum(0, dtype=torch.int64).cpu().numpy() % P, dirty.cpu().numpy())
    one, ev1 = _masked_sum(back, ridx[1:2], n, ids[1:2], none[:1], wts[1:2], 0, B)
    q, evq = TA.quantize_bounded(bad[1], wts[1], S, B)
    assert (ev1, evq) == (1, 1) and np.array_equal(one.cpu().numpy(), q)
    assert int(TA.dequantize(q, 1, P)[7]) == B


# ------------------------------------------------------------------------------------------------ 4. runner
class SmallNet(nn.Module):
    """~21 k parameters (six blocks of the kernels' 4 x 256 columns) with BatchNorm buffers."""

    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(nn.Conv3d(1, 4, 3, 2), nn.BatchNorm3d(4), nn.ReLU())
        self.classifier = nn.Sequential(nn.Linear(4, 160), nn.ReLU(), nn.Linear(160, 128), nn.ReLU(), nn.Linear(128, 1))

    def forward(self, x):
        return self.classifier(self.features(x).amax((2, 3, 4)))


def _runner(device, sizes, **cfg_kw):
    from neuroimagedisttraining_amd.engine.executor import ClientSplit, FLConfig, FLRunner, TorchEngine
    from neuroimagedisttraining_amd.parallel import runtime as rt
    torch.manual_seed(0)
    splits, off = [], 0
    for n in sizes:
        splits.append(ClientSplit(np.arange(off, off + n), np.arange(off + n, off + n + 2)))
        off += n + 2
    vols = torch.zeros((off, 9, 9, 9), dtype=torch.uint8)
    model = SmallNet()
    eng = TorchEngine(model, vols, torch.zeros(off), device)
    info = rt.DistInfo(0, 1, 0, torch.device(device), "none")
    cfg = FLConfig(comm_round=1, epochs=1, batch_size=4, seed=7, **cfg_kw)
    return FLRunner(eng, splits, cfg, info, model, algorithm="fedavg")


def _set_rows(r, lattice=False):
    g = torch.Generator().manual_seed(9)
    if lattice:
        rows = torch.randint(-2 ** 12, 2 ** 12, (r.N, r.P), generator=g).float() / 256
        bufs = torch.randint(0, 2 ** 12, (r.N, r.Q), generator=g).float() / 256
    else:
        w = torch.randn(r.P, generator=g) * 0.5
        rows = w + torch.randn(r.N, r.P, generator=g) * 0.01
        bufs = torch.rand(r.N, r.Q, generator=g) * 5
    for c in range(r.N):
        r.theta[r.row_of[c], :r.P] = rows[c].to(r.device)
        r.bufs[r.row_of[c], :r.Q] = bufs[c].to(r.device)
    return rows, bufs


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("sampled,dropout", [([0, 1, 2, 3, 4, 5], 0.0), ([0, 1, 2, 3, 4, 5], 0.34), ([0, 2, 3, 5], 0.25)])
def test_runner_on_device_matches_the_cpu_path(sampled, dropout, fuse):
    kw = dict(aggregator="secure", secagg_dropout=dropout, secagg_fuse=fuse)
    sizes = (10, 6, 12, 8, 4, 6)
    dev, cpu = _runner(DEV, sizes, **kw), _runner("cpu", sizes, **kw)
    for r in (dev, cpu):
        _set_rows(r)
        r._round_idx = 3
        r.aggregate(sampled)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dev.w_global.cpu()), _bits(cpu.w_global))
    assert torch.equal(_bits(dev.b_global.cpu()), _bits(cpu.b_global))
    want = min(int(dropout * len(sampled)), len(sampled) - len(sampled) // 2 - 1)
    assert dev.stat_info["secagg_dropped"] == cpu.stat_info["secagg_dropped"] == want
    assert dev.stat_info["secagg_saturated"] == cpu.stat_info["secagg_saturated"] == 0
    assert dev.stat_info["aggregate_elems"] == dev.P + dev.Q
    assert (want > 0) == (dropout > 0)


def test_lattice_rows_give_the_fp64_mean_and_fedavg_bits():
    """theta on multiples of 2^-8 below 16 and 8 clients of equal size: ``theta / 8 * 2^16`` is an integer, so the
    quantisation is exact and the secure aggregate is the fp64 mean bit for bit - which the fp32 FedAvg row sum also
    is on this lattice (every partial sum has fewer than 24 significant bits)."""
    dev = _runner(DEV, (6,) * 8, aggregator="secure")
    rows, bufs = _set_rows(dev, lattice=True)
    sampled = list(range(8))
    dev._round_idx = 0
    dev.aggregate(sampled)
    sw, sb = dev.w_global.clone(), dev.b_global.clone()
    dev.aggregate_fedavg(sampled)
    torch.cuda.synchronize()
    assert torch.equal(sw.cpu().double(), rows.double().mean(0)) and torch.equal(sb.cpu().double(), bufs.double().mean(0))
    assert torch.equal(_bits(sw), _bits(dev.w_global)) and torch.equal(_bits(sb), _bits(dev.b_global))
    assert dev.stat_info["secagg_saturated"] == 0


def test_one_round_with_dropout_on_the_hip_engine():
    """A full round (local training on the AlexNet3D kernels, then the secure aggregation with one of three clients
    dropped) leaves the global model the numpy twins compute from the trained rows."""
    from neuroimagedisttraining_amd.data.synthetic_fl import build_fl_volumes, to_hip_store
    from neuroimagedisttraining_amd.engine.executor import FLConfig, FLRunner, HipEngine
    from neuroimagedisttraining_amd.models.alexnet3d import AlexNet3D_Dropout
    from neuroimagedisttraining_amd.parallel import runtime as rt
    C = 3
    vol, labels, sp = build_fl_volumes(list(range(C)), C, 6, 2, torch.device(DEV), seed=3)
    x8, mom = to_hip_store(vol)
    del vol
    torch.manual_seed(0)
    model = AlexNet3D_Dropout(num_classes=1)
    eng = HipEngine(model, x8, mom, labels, torch.device(DEV))
    cfg = FLConfig(comm_round=1, epochs=1, batch_size=4, seed=3, frequency_of_the_test=0, aggregator="secure",
                   secagg_dropout=0.34)
    r = FLRunner(eng, [sp[c] for c in range(C)], cfg, rt.DistInfo(0, 1, 0, torch.device(DEV), "none"), model,
                 algorithm="fedavg")
    w0 = r.w_global.clone()
    r.run_round(0)
    torch.cuda.synchronize()
    assert r.stat_info["secagg_dropped"] == 1 and r.stat_info["secagg_saturated"] == 0
    assert bool(torch.isfinite(r.w_global).all()) and not torch.equal(r.w_global, w0)
    ow, ob = torch.empty(r.P), torch.empty(r.Q)
    rows, loc = r._local_rows(range(C))
    SA.aggregate(r.theta.cpu(), r.bufs.cpu(), r.P, r.Q, rows, loc, list(range(C)), r.sizes, r.info, r._secagg_keys, 0,
                 ow, ob, dropped=SA.draw_dropped(3, 0, range(C), 0.34, 1), hip=False)
    assert torch.equal(_bits(r.w_global.cpu()), _bits(ow)) and torch.equal(_bits(r.b_global.cpu()), _bits(ob))
