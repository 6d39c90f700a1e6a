"""CPU tests of the secure aggregation (``--aggregator secure``): the counter-based mask PRG and its Mersenne fold, the
saturating quantisation, the numpy twins of ``csrc/kernels/secagg.hip`` against the host protocol
(``TurboAggregateTrainer(prg="counter")``) bit for bit with and without dropouts, the runner on one rank against two
gloo ranks and against the eager oracle, and the public surface (flags, rejected combinations)."""
import argparse
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from neuroimagedisttraining_amd.algorithms import turboaggregate as TA
from neuroimagedisttraining_amd.engine import masks as MK
from neuroimagedisttraining_amd.engine import secagg as SA

P = TA.P_DEFAULT
S = 2 ** 16


# ------------------------------------------------------------------------------------------------ 1. PRG
def test_mersenne_fold_equals_python_modulo():
    rng = np.random.RandomState(0)
    z = [int(a) << 32 | int(b) for a, b in zip(rng.randint(0, 2 ** 32, 4096, dtype=np.uint64),
                                               rng.randint(0, 2 ** 32, 4096, dtype=np.uint64))]
    z += [0, 1, P - 1, P, P + 1, 2 * P, 2 * P + 1, 2 ** 31, 2 ** 62 - 1, 2 ** 62, 2 ** 62 + 1, 2 ** 63, 2 ** 64 - 1,
          2 ** 64 - 2, 0xBFFFFFFFFFFFFFFF, 0xBFFFFFFFFFFFFFFE,  # partial terms that add up to 2^32 or more
          (2 ** 64 - 1) // P * P, (2 ** 64 - 1) // P * P - 1]
    got = TA.mod_mersenne31(np.array(z, dtype=np.uint64))
    assert [int(v) for v in got] == [v % P for v in z]


def test_mix_hash64_extends_mix_hash_and_masks_change_with_round_segment_and_key():
    j = np.arange(1000, dtype=np.uint64)
    seed = (5 << 32) | 123456789
    z = MK._mix_hash64_np(seed, 1, j)
    assert z.dtype == np.uint64 and np.array_equal(z >> np.uint64(32), MK._mix_hash_np(seed, 1, j))
    m = TA.counter_mask(123456789, 5, 1, j)
    assert m.dtype == np.int64 and int(m.min()) >= 0 and int(m.max()) < P
    assert np.array_equal(m, np.array([int(v) % P for v in z], dtype=np.int64))
    for other in (TA.counter_mask(123456789, 6, 1, j), TA.counter_mask(123456789, 5, 0, j),
                  TA.counter_mask(123456788, 5, 1, j)):
        assert int((other == m).sum()) <= 2  # 1000 draws from Z_p: a collision is a 1e-6 event
    assert 0.45 * P < float(m.mean()) < 0.55 * P


# ------------------------------------------------------------------------------------------------ 2. quantisation
def test_quantisation_equals_quantize_and_counts_saturation():
    g = torch.Generator().manual_seed(1)
    v = (torch.randn(5000, generator=g) * 3).numpy()
    v[:8] = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 2 ** -17, -2 ** -17, 0.0], dtype=np.float32) / np.float32(S)  # ties
    w = 12 / 41
    K = 5
    q, ev = TA.quantize_saturated(v, w, S, K)
    assert ev == 0 and np.array_equal(q, TA.quantize(v.astype(np.float64) * w, S, P))
    q1, _ = TA.quantize_saturated(v[:8], 1.0, S, K)
    assert [int(x) for x in TA.dequantize(q1, 1, P)] == [0, 2, 2, 0, -2, 0, 0, 0]  # half to even
    B = TA.saturation_bound(K)
    assert B == (P - 1) // 2 // K and K * B <= (P - 1) // 2
    bad = np.array([B / S + 1.0, -(B / S) - 1.0, np.nan, np.inf, -np.inf, (B - 1000) / S, 1.0], dtype=np.float32)
    q, ev = TA.quantize_saturated(bad, 1.0, S, K)
    assert ev == 5
    inside = int(np.round(float(np.float32((B - 1000) / S)) * S))
    assert [int(x) for x in TA.dequantize(q, 1, P)] == [B, -B, 0, 0, 0, inside, S]


# ------------------------------------------------------------------------------------------------ 3. twins == trainer
IDS = [0, 2, 3, 4, 5]  # five participants of a federation of six
SIZES = {0: 10, 2: 6, 3: 12, 4: 8, 5: 4}


def _protocol_case(n=257, seed=2):
    g = torch.Generator().manual_seed(seed)
    M = (torch.randn(len(IDS), n, generator=g) * 0.7).numpy()
    keys = SA.SecAggKeys(6, 2, seed=11)
    n_tot = float(sum(SIZES.values()))
    wts = [SIZES[c] / n_tot for c in IDS]
    return M, keys, wts, n_tot


@pytest.mark.parametrize("dropped", [(), (3,), (0, 4)])
@pytest.mark.parametrize("seg", [0, 1])
def test_twins_equal_the_counter_trainer_bit_for_bit(dropped, seg):
    M, keys, wts, n_tot = _protocol_case()
    t = keys.trainer
    rnd = 3
    B = TA.saturation_bound(len(IDS))
    alive = [c for c in IDS if c not in dropped]
    rows = [IDS.index(c) for c in alive]
    full = [[(j, int(keys.key[c, j])) for j in IDS if j != c] for c in alive]
    up, ev = SA.upload_twin(M[rows], alive, full, [wts[r] for r in rows], rnd, seg, S, B)
    want = {c: t.client_upload(c, M[IDS.index(c)], wts[IDS.index(c)], round=rnd, seg=seg, peers=IDS) for c in alive}
    assert ev == 0
    for k, c in enumerate(alive):
        assert np.array_equal(up[k], want[c]), c
        assert int(up[k].min()) >= 0 and int(up[k].max()) < P
    # the masked sum generates only the masks that do not cancel among the summed rows: those towards dropped clients
    rest = [[(j, int(keys.key[c, j])) for j in dropped] for c in alive]
    ms, _ = SA.masked_sum_twin(M[rows], alive, rest, [wts[r] for r in rows], rnd, seg, S, B)
    assert np.array_equal(ms, up.sum(0) % P)
    a = float(sum(SIZES[c] for c in alive)) / n_tot
    got = SA.finish_twin(ms, keys.removal_pairs(dropped, alive), rnd, seg, S, a)
    ref = t.server_aggregate(want, dropped=list(dropped), round=rnd, seg=seg, alive_weight=a)
    assert got.dtype == ref.dtype == np.float32 and np.array_equal(got.view(np.int32), ref.view(np.int32))
    exact = sum(wts[IDS.index(c)] * M[IDS.index(c)].astype(np.float64) for c in alive) / a
    err = np.abs(got.astype(np.float64) - exact)
    assert float(err.max()) <= len(alive) / (2 * S * a) + 2.0 ** -24 * float(np.abs(exact).max())
    assert (a == 1.0) == (not dropped)


def test_reconstruction_needs_more_than_threshold_survivors_and_the_draw_leaves_them():
    keys = SA.SecAggKeys(6, 2, seed=11)
    assert keys.reconstruct([1], [0, 2, 3]) == {1: int(keys.trainer.sk[1])}
    with pytest.raises(ValueError, match="survivors"):
        keys.reconstruct([1], [0, 2])
    with pytest.raises(ValueError, match="threshold"):
        SA.SecAggKeys(4, 4)
    for rnd in range(20):
        for frac, T in ((0.25, 4), (0.5, 4), (0.9, 4), (0.9, 1)):
            d = SA.draw_dropped(7, rnd, range(8), frac, T)
            assert d == SA.draw_dropped(7, rnd, list(range(8))[::-1], frac, T) and set(d) <= set(range(8))
            assert len(d) == min(int(frac * 8), 8 - T - 1) and 8 - len(d) > T
    assert SA.draw_dropped(7, 0, range(8), 0.0, 4) == []
    assert len({tuple(SA.draw_dropped(7, r, range(8), 0.25, 4)) for r in range(20)}) > 1


def test_default_mt_trainer_is_unchanged():
    rng = np.random.RandomState(0)
    v = rng.randn(50)
    a, b = TA.TurboAggregateTrainer(3, seed=4), TA.TurboAggregateTrainer(3, seed=4, prg="mt")
    assert a.prg == "mt" and np.array_equal(a.client_upload(1, v, 0.5), b.client_upload(1, v, 0.5))
    key = a.pair_key(1, 2)
    r = np.random.RandomState(key % (2 ** 32)).randint(P, size=50).astype(np.int64)
    assert np.array_equal(a._mask(1, 2, 50), r) and np.array_equal(a._mask(2, 1, 50), (-r) % P)
    with pytest.raises(ValueError, match="prg"):
        TA.TurboAggregateTrainer(3, prg="philox")


# ------------------------------------------------------------------------------------------------ 4. runner
class Tiny3D(nn.Module):
    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(nn.Conv3d(1, 4, 3, 2), nn.BatchNorm3d(4), nn.ReLU(), nn.MaxPool3d(2, 2),
                                      nn.Conv3d(4, 8, 3), nn.BatchNorm3d(8), nn.ReLU())
        self.classifier = nn.Sequential(nn.Dropout(), nn.Linear(8, 1))

    def forward(self, x):
        return self.classifier(self.features(x).amax((2, 3, 4)))


SIZES5 = (10, 6, 12, 8, 4)


def _runner(rank=0, world=1, sizes=SIZES5, rounds=2, algorithm="fedavg", **cfg_kw):
    from neuroimagedisttraining_amd.engine.executor import ClientSplit, FLConfig, FLRunner, TorchEngine
    from neuroimagedisttraining_amd.parallel import runtime as rt
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(5)
    n_te = 4
    N = sum(sizes) + n_te * len(sizes)
    vols = torch.randint(0, 256, (N, 15, 15, 15), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 2, (N,), generator=g).float()
    splits, off = [], 0
    for n in sizes:
        splits.append(ClientSplit(np.arange(off, off + n), np.arange(off + n, off + n + n_te)))
        off += n + n_te
    model = Tiny3D()
    eng = TorchEngine(model, vols, labels, "cpu")
    info = rt.DistInfo(rank, world, rank, torch.device("cpu"), "gloo" if world > 1 else "none")
    cfg = FLConfig(comm_round=rounds, epochs=2, batch_size=4, lr=0.05, dense_ratio=0.5, seed=7, **cfg_kw)
    return FLRunner(eng, splits, cfg, info, model, algorithm=algorithm)


def _hand_rows(r, seed=3):
    g = torch.Generator().manual_seed(seed)
    r.w_global.copy_(torch.randn(r.P, generator=g) * 0.5)
    for c in range(r.N):
        row = r.row_of[c]
        r.theta[row, :r.P] = r.w_global + torch.randn(r.P, generator=g) * 0.01
        r.bufs[row, :r.Q] = torch.rand(r.Q, generator=g) * 3


def _bits(t):
    return t.contiguous().view(torch.int32)


SECURE = dict(aggregator="secure", secagg_dropout=0.25)


def _dist_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    r = _runner(rank, world, **SECURE)
    for k in range(2):
        r.run_round(k)
    if rank == 0:
        torch.save({"w": r.w_global, "b": r.b_global, "sat": r.stat_info["secagg_saturated"],
                    "dropped": r.stat_info["secagg_dropped"], "elems": r.stat_info["aggregate_elems"]}, out)
    dist.destroy_process_group()


def test_two_rank_gloo_is_bit_identical_to_one_process(tmp_path):
    """Integer arithmetic: two rounds of local training and secure aggregation with one dropped client on 2 gloo ranks
    leave the very bits one process leaves (no tolerance), global parameters and BN buffers."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "w.pt")
    mp.start_processes(_dist_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    got = torch.load(out, weights_only=True)
    r = _runner(**SECURE)
    for k in range(2):
        r.run_round(k)
    assert torch.equal(_bits(got["w"]), _bits(r.w_global)) and torch.equal(_bits(got["b"]), _bits(r.b_global))
    assert got["dropped"] == r.stat_info["secagg_dropped"] == 1
    assert got["sat"] == r.stat_info["secagg_saturated"] == 0
    assert got["elems"] == r.stat_info["aggregate_elems"] == r.P + r.Q


def _float_state(r, vec_p, vec_b):
    sd = {}
    for name, t in r.template.state_dict().items():
        lay, vec = (r.e.players, vec_p) if name in r.e.players.names else (r.e.blayers, vec_b)
        i = lay.index(name)
        sd[name] = vec[lay.offsets[i]:lay.offsets[i] + lay.numel(i)].view(lay.shapes[i]).clone()
    return sd


@pytest.mark.parametrize("frac", [1.0, 0.6])
@pytest.mark.parametrize("dropout", [0.0, 0.4])
def test_runner_equals_the_eager_oracle_and_the_unfused_path(dropout, frac):
    """The runner's aggregate (masked sum of the rows in place), its ``secagg_fuse=False`` form (every client's upload
    materialised) and the eager ``FedAvgAPI._aggregate`` (host protocol over state dicts) give the same bits; with
    ``frac < 1`` the sampled rows are not contiguous."""
    from neuroimagedisttraining_amd.algorithms.fedavg import FedAvgAPI
    kw = dict(aggregator="secure", secagg_dropout=dropout, frac=frac)
    r, u = _runner(**kw), _runner(secagg_fuse=False, **kw)
    rnd = 1
    sampled = r.sample_clients(rnd)
    assert len(sampled) == (5 if frac == 1.0 else 3)
    for x in (r, u):
        _hand_rows(x)
        x._round_start(rnd)
        x.aggregate(sampled)
    assert torch.equal(_bits(r.w_global), _bits(u.w_global)) and torch.equal(_bits(r.b_global), _bits(u.b_global))
    n_drop = min(int(dropout * len(sampled)), len(sampled) - len(sampled) // 2 - 1)
    assert r.stat_info["secagg_dropped"] == u.stat_info["secagg_dropped"] == n_drop
    api = FedAvgAPI.__new__(FedAvgAPI)
    api.args = types.SimpleNamespace(aggregator="secure", seed=7, client_num_in_total=5, secagg_dropout=dropout)
    api.stat_info = {}
    w_locals = [(int(r.sizes[c]), _float_state(r, r.theta[r.row_of[c], :r.P], r.bufs[r.row_of[c], :r.Q]))
                for c in sampled]
    want = api._aggregate(w_locals, None, round_idx=rnd, client_ids=sampled)
    got = _float_state(r, r.w_global, r.b_global)
    assert list(want) == list(got)
    for k in want:
        assert torch.equal(_bits(want[k]), _bits(got[k])), k
    assert api.stat_info["secagg_dropped"] == n_drop and api.stat_info["secagg_saturated"] == 0
    # and it is FedAvg's mean of the survivors up to the quantisation step
    dropped = SA.draw_dropped(7, rnd, sampled, dropout, len(sampled) // 2)
    alive = [c for c in sampled if c not in dropped]
    n_al = float(sum(r.sizes[c] for c in alive))
    mean = sum(r.theta[r.row_of[c], :r.P].double() * (float(r.sizes[c]) / n_al) for c in alive)
    assert float((r.w_global.double() - mean).abs().max()) <= len(sampled) / S


def test_lattice_rows_give_the_exact_mean_and_saturation_is_counted():
    r = _runner(sizes=(6,) * 8, aggregator="secure")
    g = torch.Generator().manual_seed(4)
    for c in range(8):
        r.theta[r.row_of[c], :r.P] = torch.randint(-2 ** 12, 2 ** 12, (r.P,), generator=g).float() / 256
        r.bufs[r.row_of[c], :r.Q] = torch.randint(0, 2 ** 12, (r.Q,), generator=g).float() / 256
    r._round_start(0)
    r.aggregate(list(range(8)))
    assert torch.equal(r.w_global.double(), r.theta[:, :r.P].double().mean(0))
    assert torch.equal(r.b_global.double(), r.bufs[:, :r.Q].double().mean(0))
    assert r.stat_info["secagg_saturated"] == 0
    keep = r.w_global.clone()
    B = TA.saturation_bound(8)
    r.theta[r.row_of[2], 5] = 8 * (B / S) + 1000.0  # weight 1/8: above B / S after weighting
    r.theta[r.row_of[3], 17] = float("nan")
    r.bufs[r.row_of[4], 1] = float("inf")
    r._round_start(1)
    r.aggregate(list(range(8)))
    assert r.stat_info["secagg_saturated"] == 3
    same = torch.ones(r.P, dtype=torch.bool)
    same[[5, 17]] = False
    assert torch.equal(r.w_global[same], keep[same]) and bool(torch.isfinite(r.w_global).all())
    assert bool(torch.isfinite(r.b_global).all())


# ------------------------------------------------------------------------------------------------ 5. surface
def _parse(algo, argv=()):
    from neuroimagedisttraining_amd import cli
    return cli.add_args(argparse.ArgumentParser(), algo).parse_args(list(argv))


def test_flags_reach_flconfig():
    from neuroimagedisttraining_amd import cli
    from neuroimagedisttraining_amd.algorithms.hip_dispatch import _full_args
    args = _parse("fedavg", ["--aggregator", "secure", "--secagg_scale", "4096", "--secagg_dropout", "0.25",
                             "--secagg_threshold", "3", "--secagg_fuse", "0"])
    cfg = cli.fl_config(args, "fedavg")
    assert (cfg.aggregator, cfg.secagg_scale, cfg.secagg_dropout, cfg.secagg_threshold, cfg.secagg_fuse) == \
        ("secure", 4096, 0.25, 3, False)
    d = cli.fl_config(_parse("sailentgrads"), "sailentgrads")
    assert (d.aggregator, d.secagg_scale, d.secagg_dropout, d.secagg_threshold, d.secagg_fuse) == \
        ("fedavg", 2 ** 16, 0.0, 0, True)
    full = _full_args(types.SimpleNamespace(comm_round=3), "fedprox")  # a reference script's args lack the flags
    assert (full.secagg_scale, full.secagg_dropout, full.secagg_threshold, full.secagg_fuse) == (2 ** 16, 0.0, 0, 1)
    assert cli.identity(_parse("fedavg"), "fedavg") == \
        "fedavg-dir0.3-mdl3DCNN-batchsize16-cm200-total_clnt4-neighbor3-seed0-lr0.001"


def test_rejected_combinations_raise_when_the_config_is_built():
    from neuroimagedisttraining_amd import cli
    from neuroimagedisttraining_amd.engine.executor import FLConfig
    from neuroimagedisttraining_amd.engine.personalized import make_runner
    with pytest.raises(ValueError, match=r"weak_dp.*secure"):
        FLConfig(aggregator="secure", defense_type="weak_dp")
    with pytest.raises(ValueError, match=r"secure.*update_topk=0\.1"):
        FLConfig(aggregator="secure", update_topk=0.1)
    with pytest.raises(ValueError, match="secagg_dropout"):
        FLConfig(aggregator="secure", secagg_dropout=1.0)
    with pytest.raises(ValueError, match=r"secure.*ditto"):
        cli.fl_config(_parse("ditto", ["--aggregator", "secure"]), "ditto")
    with pytest.raises(ValueError, match=r"norm_diff_clipping.*secure"):
        cli.fl_config(_parse("fedprox", ["--aggregator", "secure", "--defense_type", "norm_diff_clipping"]), "fedprox")
    base = _runner(sizes=(6, 6))
    cfg = FLConfig(aggregator="secure")
    for algo in ("ditto", "local", "dpsgd", "fedfomo", "subavg", "dispfl"):
        with pytest.raises(ValueError, match=r"secure.*" + algo):
            make_runner(algo, base.e, base.splits, cfg, base.info, Tiny3D())
    FLConfig(aggregator="secure", secagg_dropout=0.5, secagg_threshold=2)
