"""CPU tests of norm-difference clipping and weak-DP aggregation on the client-batched executor: agreement with the
reference-semantics ``RobustAggregator``, the no-op bound, the counter-based noise twin, sharding invariance over two
gloo ranks, and the public surface (flags, config validation, the eager oracle)."""
import argparse
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from neuroimagedisttraining_amd.core import robustness as R
from neuroimagedisttraining_amd.engine import defense as DF
from neuroimagedisttraining_amd.engine import masks as MK


class Tiny3D(nn.Module):
    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(nn.Conv3d(1, 4, 3, 2), nn.BatchNorm3d(4), nn.ReLU(), nn.MaxPool3d(2, 2),
                                      nn.Conv3d(4, 8, 3), nn.BatchNorm3d(8), nn.ReLU())
        self.classifier = nn.Sequential(nn.Dropout(), nn.Linear(8, 1))

    def forward(self, x):
        return self.classifier(self.features(x).amax((2, 3, 4)))


def _runner(rank=0, world=1, sizes=(10, 10, 10, 10), rounds=2, algorithm="salientgrads", **cfg_kw):
    """A TorchEngine runner over ``len(sizes)`` clients with ``sizes[c]`` train samples each (4 test samples)."""
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


SIZES5 = (10, 6, 12, 8, 4)


def _hand_rows(r, shift=100.0, seed=3):
    """Random w_global and per-client BN buffers, rows = w_global + small updates, client 3 shifted by ``shift``."""
    g = torch.Generator().manual_seed(seed)
    r.w_global.copy_(torch.randn(r.P, generator=g) * 0.5)
    for c in range(r.N):
        row = r.row_of[c]
        r.theta[row, :r.P] = r.w_global + torch.randn(r.P, generator=g) * 0.01
        r.bufs[row, :r.Q] = torch.rand(r.Q, generator=g)
    r.theta[r.row_of[3], :r.P] += shift
    return r.w_global.clone()


def _float_state(r, vec_p, vec_b):
    """One model's state dict (all fp32, the keys and shapes of the template) from flat params / buffers."""
    sd = {}
    for lay, vec in ((r.e.players, vec_p), (r.e.blayers, vec_b)):
        for i, n in enumerate(lay.names):
            sd[n] = vec[lay.offsets[i]:lay.offsets[i] + lay.numel(i)].view(lay.shapes[i]).clone()
    return sd


# ------------------------------------------------------------------------------------------------ 1. oracle
def test_clipping_matches_robust_aggregator_oracle():
    from neuroimagedisttraining_amd.algorithms.common import weighted_average
    bound = 1.0
    r = _runner(sizes=SIZES5, defense_type="norm_diff_clipping", norm_bound=bound)
    g0 = _hand_rows(r)
    b0 = r.b_global.clone()
    sampled = list(range(5))
    n_tot = float(sum(SIZES5))
    ra = R.RobustAggregator(types.SimpleNamespace(defense_type="norm_diff_clipping", norm_bound=bound, stddev=0.0))
    gsd = _float_state(r, g0, b0)
    w_locals = []
    for c in sampled:
        row = r.row_of[c]
        w_locals.append((SIZES5[c], ra.norm_diff_clipping(_float_state(r, r.theta[row, :r.P], r.bufs[row, :r.Q]), gsd)))
    want = weighted_average(w_locals)
    want_p = r.e.players.flatten_state(want)
    want_b = r.e.blayers.flatten_state(want)

    r.aggregate(sampled)
    got = r.w_global.clone()
    assert torch.allclose(got, want_p, atol=1e-6), float((got - want_p).abs().max())
    # BN buffers: the plain weighted mean (never clipped)
    plain_b = sum(SIZES5[c] / n_tot * r.bufs[r.row_of[c], :r.Q] for c in sampled)
    assert torch.allclose(r.b_global, want_b, atol=1e-6)
    assert torch.allclose(r.b_global, plain_b, atol=1e-6)
    assert r.stat_info["defense_clipped"] == 1
    assert r.stat_info["defense_max_ratio"] > 100.0

    # the outlier moves w_global by at most w_3 * norm_bound: against the same round with client 3 sending no update
    r.w_global.copy_(g0)
    r.theta[r.row_of[3], :r.P] = g0
    r.aggregate(sampled)
    moved = float((got - r.w_global).double().norm())
    w3 = SIZES5[3] / n_tot
    print("outlier moved w_global by", moved, "bound", w3 * bound)
    assert moved <= w3 * bound * (1 + 1e-5)
    assert moved > 0.5 * w3 * bound  # and it was clipped to the ball's surface, not dropped


def test_theta_bufs_split_is_is_weight_param():
    """``ParamLayout``'s params / buffers split of the engines' models is the reference's ``is_weight_param``."""
    from neuroimagedisttraining_amd.models import customized_resnet18
    from neuroimagedisttraining_amd.models.alexnet3d import AlexNet3D_Dropout
    from neuroimagedisttraining_amd.models.resnet3d import resnet3d_50
    with torch.device("meta"):
        models = [AlexNet3D_Dropout(num_classes=1), resnet3d_50(num_classes=1), customized_resnet18(class_num=10),
                  Tiny3D()]
    for m in models:
        params = [n for n, _ in m.named_parameters()]
        bufs = [n for n, _ in m.named_buffers()]
        assert params and all(R.is_weight_param(n) for n in params), type(m).__name__
        assert not any(R.is_weight_param(n) for n in bufs), type(m).__name__
        assert set(params) | set(bufs) == set(m.state_dict().keys())


# ------------------------------------------------------------------------------------------------ 2. no-op bound
def test_huge_bound_is_plain_fedavg():
    a = _runner(sizes=SIZES5, defense_type="norm_diff_clipping", norm_bound=1e30)
    b = _runner(sizes=SIZES5)
    for r in (a, b):
        _hand_rows(r)
        r.aggregate(list(range(5)))
    assert torch.allclose(a.w_global, b.w_global, atol=1e-6)
    assert torch.allclose(a.b_global, b.b_global, atol=1e-6)
    assert a.stat_info["defense_clipped"] == 0
    assert "defense_clipped" not in b.stat_info


# ------------------------------------------------------------------------------------------------ 3. noise twin
NOISE_SEED = 20240611


def test_noise_twin_is_standard_normal():
    N = 1 << 20
    z = DF.noise_z_np(NOISE_SEED, 3, np.arange(N))
    mean, var = float(z.mean()), float(z.var())
    print("noise twin: mean %.3e var-1 %.3e" % (mean, var - 1.0))
    assert abs(mean) < 5 * 2.0 ** -10            # 5 standard errors: 1 / sqrt(2^20) = 2^-10
    assert abs(var - 1.0) < 5 * np.sqrt(2.0 / N)  # 5 standard errors of a unit normal's sample variance
    assert np.abs(z).max() <= np.sqrt(2 * 24 * np.log(2.0)) + 1e-12  # u1 >= 2^-24
    # keyed by client and seed: other streams are other numbers
    assert not np.array_equal(z[:64], DF.noise_z_np(NOISE_SEED, 4, np.arange(64)))
    assert not np.array_equal(z[:64], DF.noise_z_np(NOISE_SEED + 1, 3, np.arange(64)))
    assert DF.round_seed(7, 0) != DF.round_seed(7, 1)


def _expected_noise(r, sampled, round_idx, stddev):
    n_tot = float(sum(r.sizes[c] for c in sampled))
    seed = DF.round_seed(r.cfg.seed, round_idx)
    idx = np.arange(r.P)
    return stddev * sum(float(r.sizes[c]) / n_tot * DF.noise_z_np(seed, c, idx) for c in sampled)


def test_weak_dp_zero_updates_gives_the_twin_noise():
    stddev = 0.5
    r = _runner(sizes=SIZES5, algorithm="fedavg", defense_type="weak_dp", norm_bound=1.0, stddev=stddev)
    sampled = [0, 1, 3, 4]
    g0 = r.w_global.clone()
    outs = []
    for round_idx in (0, 1):
        r.w_global.copy_(g0)
        r.theta[:, :r.P] = g0
        r._round_idx = round_idx
        r.aggregate(sampled)
        want = _expected_noise(r, sampled, round_idx, stddev)
        err = float(np.abs((r.w_global - g0).double().numpy() - want).max())
        print("round", round_idx, "noise error", err)
        assert err < 1e-6
        assert r.stat_info["defense_clipped"] == 0 and r.stat_info["defense_max_ratio"] == 0.0
        outs.append(r.w_global.clone())
    assert not torch.equal(outs[0], outs[1])  # the round index keys the noise


def test_weak_dp_under_salientgrads_mask_keeps_pruned_zero():
    stddev = 0.5
    r = _runner(sizes=SIZES5, algorithm="salientgrads", defense_type="weak_dp", norm_bound=1.0, stddev=stddev)
    g = torch.Generator().manual_seed(1)
    mask = (torch.rand(r.P, generator=g) < 0.5).float()
    r.mask, r.mask_bits = mask, MK.pack_bits(mask.view(1, -1))
    g0 = r.w_global * mask
    r.w_global.copy_(g0)
    r.theta[:, :r.P] = g0
    sampled = list(range(5))
    r._round_idx = 0
    r.aggregate(sampled)
    assert float(r.w_global[mask == 0].abs().max()) == 0.0  # pruned coordinates stay exactly 0
    want = _expected_noise(r, sampled, 0, stddev) * mask.numpy()
    assert float(np.abs((r.w_global - g0).double().numpy() - want).max()) < 1e-6
    assert float((r.w_global - g0)[mask > 0].abs().min()) > 0.0


# ------------------------------------------------------------------------------------------------ 4. sharding
WEAK_DP = dict(defense_type="weak_dp", norm_bound=0.05, stddev=0.01)


def _dist_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    r = _runner(rank, world, **WEAK_DP)
    r.generate_global_mask_snip()
    for k in range(2):
        r.run_round(k)
    if rank == 0:
        torch.save({"w": r.w_global, "acc": r.stat_info["global_test_acc"],
                    "clipped": r.stat_info["defense_clipped"], "ratio": r.stat_info["defense_max_ratio"]}, out)
    dist.destroy_process_group()


def test_two_rank_gloo_weak_dp_matches_single_process(tmp_path):
    """Clipping norms and the noise are functions of the client, not of the rank that holds it: 2 gloo ranks
    reproduce one process over two rounds (SalientGrads mask active: the defended all-reduce is dense, because the
    clipped sum is not 0 at pruned coordinates while the global model still is dense there)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "w.pt")
    mp.start_processes(_dist_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    got = torch.load(out, weights_only=True)
    r = _runner(**WEAK_DP)
    r.generate_global_mask_snip()
    for k in range(2):
        r.run_round(k)
    assert torch.allclose(got["w"], r.w_global, atol=1e-5), float((got["w"] - r.w_global).abs().max())
    assert np.allclose(got["acc"], r.stat_info["global_test_acc"])
    assert got["clipped"] == r.stat_info["defense_clipped"]
    assert got["ratio"] == pytest.approx(r.stat_info["defense_max_ratio"], rel=1e-5)
    assert got["clipped"] > 0  # the bound is small enough that the clipping path ran


# ------------------------------------------------------------------------------------------------ 5. surface
def _parse(algo, argv=()):
    from neuroimagedisttraining_amd import cli
    return cli.add_args(argparse.ArgumentParser(), algo).parse_args(list(argv))


def test_flags_reach_flconfig_and_identity_is_unchanged():
    from neuroimagedisttraining_amd import cli
    from neuroimagedisttraining_amd.algorithms.hip_dispatch import _full_args
    args = _parse("fedavg", ["--defense_type", "weak_dp", "--norm_bound", "2.5", "--stddev", "0.125"])
    cfg = cli.fl_config(args, "fedavg")
    assert (cfg.defense_type, cfg.norm_bound, cfg.stddev) == ("weak_dp", 2.5, 0.125)
    ra = R.RobustAggregator(args)  # the names RobustAggregator reads
    assert (ra.defense_type, ra.norm_bound, ra.stddev) == ("weak_dp", 2.5, 0.125)
    d = cli.fl_config(_parse("fedavg"), "fedavg")
    assert (d.defense_type, d.norm_bound, d.stddev) == ("none", 5.0, 0.025)
    full = _full_args(types.SimpleNamespace(comm_round=3), "fedavg")  # a reference script's args lack the flags
    assert (full.defense_type, full.norm_bound, full.stddev) == ("none", 5.0, 0.025)
    # identity strings (log file names) of the default flags: exactly what they were before the flags existed
    assert cli.identity(_parse("fedavg"), "fedavg") == \
        "fedavg-dir0.3-mdl3DCNN-batchsize16-cm200-total_clnt4-neighbor3-seed0-lr0.001"
    assert cli.identity(_parse("fedprox"), "fedprox") == \
        "fedprox-dir0.3-mdl3DCNN-batchsize16-cm200-total_clnt128-neighbor128-seed0-lr0.001-mu0.01-aggfedavg"
    assert cli.identity(_parse("sailentgrads"), "sailentgrads") == (
        "SailentGrads-ABCD-dir0.3-mdl3DCNNcustomizedlowbatch-csv0-ERK_init-same_init-DST-cm200-total_clnt4"
        "-neighbor4-dr0.5-active1.0-seed1024-lr0.01-batchsize16-iteration1-stratifiedFalse")


def test_rejected_combinations_raise_when_the_config_is_built():
    from neuroimagedisttraining_amd import cli
    from neuroimagedisttraining_amd.engine.executor import FLConfig
    from neuroimagedisttraining_amd.engine.personalized import make_runner
    with pytest.raises(ValueError, match=r"weak_dp.*median"):
        FLConfig(defense_type="weak_dp", aggregator="median")
    with pytest.raises(ValueError, match=r"norm_diff_clipping.*update_topk=0\.1"):
        FLConfig(defense_type="norm_diff_clipping", update_topk=0.1)
    with pytest.raises(ValueError, match="defense_type"):
        FLConfig(defense_type="clip")
    with pytest.raises(ValueError, match=r"weak_dp.*krum"):
        cli.fl_config(_parse("fedprox", ["--defense_type", "weak_dp", "--aggregator", "krum"]), "fedprox")
    with pytest.raises(ValueError, match=r"weak_dp.*ditto"):
        cli.fl_config(_parse("ditto", ["--defense_type", "weak_dp"]), "ditto")
    base = _runner(sizes=(6, 6))
    cfg = FLConfig(defense_type="norm_diff_clipping")
    for algo in ("ditto", "local", "dpsgd", "fedfomo", "subavg", "dispfl"):
        with pytest.raises(ValueError, match=r"norm_diff_clipping.*" + algo):
            make_runner(algo, base.e, base.splits, cfg, base.info, Tiny3D())
    FLConfig(aggregator="median", update_topk=0.0)  # without a defence nothing changes


def test_eager_fedavg_aggregate_clips_like_the_manual_computation():
    from neuroimagedisttraining_amd.algorithms.common import weighted_average
    from neuroimagedisttraining_amd.algorithms.fedavg import FedAvgAPI
    torch.manual_seed(2)
    w_global = {k: v.detach().clone().float() for k, v in Tiny3D().state_dict().items()}
    w_locals = []
    for i, n in enumerate((10, 30, 20)):
        sd = {k: v + (5.0 if i == 1 else 0.01) * torch.randn_like(v) for k, v in w_global.items()}
        w_locals.append((n, sd))
    bound = 0.5
    api = FedAvgAPI.__new__(FedAvgAPI)
    api.args = types.SimpleNamespace(defense_type="norm_diff_clipping", norm_bound=bound, stddev=0.0,
                                     aggregator="fedavg")
    got = api._aggregate(w_locals, w_global)
    manual = []
    for n, sd in w_locals:
        keys = [k for k in sd if R.is_weight_param(k)]
        nrm = float(torch.cat([(sd[k] - w_global[k]).reshape(-1) for k in keys]).norm())
        scale = max(1.0, nrm / bound)
        manual.append((n, {k: (w_global[k] + (sd[k] - w_global[k]) / scale) if k in keys else sd[k] for k in sd}))
    want = weighted_average(manual)
    assert set(got) == set(want)
    for k in want:
        assert torch.allclose(got[k].float(), want[k].float(), atol=1e-6), k
    # callers that pass no global state, or set no defence, get the plain weighted mean
    plain = weighted_average(w_locals)
    for k, v in api._aggregate(w_locals).items():
        assert torch.equal(v, plain[k])
    api.args.defense_type = "none"
    for k, v in api._aggregate(w_locals, w_global).items():
        assert torch.equal(v, plain[k])
    # weak_dp: noise on the weight parameters only (torch.randn: not the executor's counter-based bits)
    api.args = types.SimpleNamespace(defense_type="weak_dp", norm_bound=1e30, stddev=0.1, aggregator="fedavg")
    noisy = api._aggregate(w_locals, w_global)
    for k in plain:
        if R.is_weight_param(k):
            assert not torch.equal(noisy[k].float(), plain[k].float()), k
        else:
            assert torch.allclose(noisy[k].float(), plain[k].float(), atol=1e-6), k
