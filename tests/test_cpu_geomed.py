"""CPU tests of the geometric-median (RFA) rule: the twins of ``rows_geomed_step`` / ``geomed_weights`` against fp64,
``core/robustness.geometric_median`` against a numpy Weiszfeld loop, the flags, the chunk driver on 1 and 2 ranks."""
import argparse
import os
import socket

import numpy as np
import pytest
import torch

from neuroimagedisttraining_amd.core import robustness as R
from neuroimagedisttraining_amd.engine import robust as RB

NAN, INF = float("nan"), float("inf")


def _rows(K, n, seed, outliers=0):
    """K rows near one another, the last ``outliers`` of them far away."""
    g = torch.Generator().manual_seed(seed)
    M = torch.randn(1, n, generator=g) * 0.5 + 0.05 * torch.randn(K, n, generator=g)
    M[K - outliers:] += 30.0
    return M


@pytest.mark.parametrize("K,n", [(1, 5), (3, 67), (8, 1031), (65, 259)])
def test_step_twin_against_fp64(K, n):
    """z within the a-priori bound of a sequential fp32 sum of K rounded products, (K + 1) 2^-24 sum_i beta_i |x_ij|;
    dsq, taken from the same fp32 z, within n 2^-53 relative of numpy's fp64 sum (n non-negative terms)."""
    M = _rows(K, n, 7 * K + n)
    beta = torch.rand(K, generator=torch.Generator().manual_seed(K)).float()
    if K >= 3:
        beta[[0, K - 1]] = 0.0
    z, dsq = RB.geomed_step_twin(M, beta)
    A, b = M.numpy().astype(np.float64), beta.numpy().astype(np.float64)
    assert bool((np.abs(z.numpy() - b @ A) <= (K + 1) * 2.0 ** -24 * (b @ np.abs(A))).all())
    d = (M.numpy() - z.numpy()).astype(np.float64)
    ref = (d * d).sum(1)
    assert bool((np.abs(dsq.numpy() - ref) <= n * 2.0 ** -53 * ref).all())


def test_weights_twin_edge_cases():
    alpha = torch.full((4,), 0.25, dtype=torch.float64)
    beta, obj = RB.geomed_weights_twin(torch.tensor([4.0, NAN, 1e-20, INF], dtype=torch.float64), alpha, 1e-6)
    w = np.array([0.25 / 2.0, 0.0, 0.25 / 1e-6, 0.0])  # d < nu is floored at nu; NaN and Inf rows get no weight
    assert beta.tolist() == (w / (w[0] + w[1] + w[2] + w[3])).astype(np.float32).tolist()
    assert float(obj) == 0.25 * 2.0 + 0.25 * np.sqrt(1e-20)
    beta, obj = RB.geomed_weights_twin(torch.tensor([NAN, INF], dtype=torch.float64), alpha[:2], 1e-6)
    assert beta.tolist() == [0.0, 0.0] and bool(torch.isnan(obj))
    beta, _ = RB.geomed_weights_twin(torch.tensor([1.0, 1.0, 1.0]), torch.tensor([0.5, 0.0, 0.5]), 1e-6)
    assert beta.tolist() == [0.5, 0.0, 0.5]  # alpha = 0: no weight


@pytest.mark.parametrize("K,bad", [(5, 1), (9, 3), (4, 0)])
def test_core_geometric_median_against_numpy_weiszfeld(K, bad):
    M = _rows(K, 300, K, outliers=bad)
    X = M.numpy().astype(np.float64)
    z = X.mean(0)
    for _ in range(5):
        w = 1.0 / np.maximum(1e-6, np.linalg.norm(X - z, axis=1))
        z = (w / w.sum()) @ X
    got = R.geometric_median(M, iters=6, nu=1e-6)
    assert got.dtype == torch.float32 and np.allclose(got.numpy(), z, rtol=1e-6, atol=1e-6)
    if bad:  # closer to the honest rows than the mean is, and a NaN / Inf row changes nothing
        honest = X[:K - bad].mean(0)
        assert np.linalg.norm(z - honest) < 0.2 * np.linalg.norm(X.mean(0) - honest)
        P = torch.cat([M, torch.full((1, 300), NAN), torch.full((1, 300), INF)])
        assert torch.allclose(R.geometric_median(P, 6, 1e-6), got, rtol=1e-6, atol=1e-6)


def test_flags_reach_the_config_and_bad_combinations_raise():
    from neuroimagedisttraining_amd import cli
    from neuroimagedisttraining_amd.engine.executor import FLConfig
    parser = argparse.ArgumentParser()
    cli.add_args(parser, "fedavg")
    args = parser.parse_args(["--aggregator", "geomed", "--geomed_iters", "7", "--geomed_nu", "1e-4"])
    cfg = cli.fl_config(args, "fedavg")
    assert (cfg.aggregator, cfg.geomed_iters, cfg.geomed_nu) == ("geomed", 7, 1e-4)
    assert (FLConfig().geomed_iters, FLConfig().geomed_nu) == (4, 1e-6)
    for kw in (dict(geomed_iters=0), dict(geomed_nu=0.0), dict(aggregator="geomed", defense_type="weak_dp")):
        with pytest.raises(ValueError):
            FLConfig(**kw)


N_ROWS, P, Q = 8, 1200, 70
SAMPLED = [7, 1, 2, 4, 5, 0]
BUDGETS = {1: 4 * 6 * 1216, 2: 4 * 6 * 640, 7: 4 * 6 * 192}
OWNER = [0, 1, 0, 0, 1, 1, 1, 0]
RANK_CLIENTS = {0: [3, 7, 0, 2], 1: [5, 6, 1, 4]}


def _run(clients, owner, rank, world, budget):
    """Rows of ``clients`` in that order; client 4 is far away, client 5 not finite, unsampled rows and pads NaN."""
    from neuroimagedisttraining_amd.parallel import runtime as rt
    info = rt.DistInfo(rank, world, rank, torch.device("cpu"), "gloo" if world > 1 else "none")
    th, bu = _rows(N_ROWS, P, 21), _rows(N_ROWS, Q, 22)
    th[4] += 50.0
    th[5, 17] = INF
    theta = torch.full((len(clients), (P + 63) // 64 * 64), NAN)
    bufs = torch.full((len(clients), (Q + 63) // 64 * 64), NAN)
    rows = [r for r, c in enumerate(clients) if c in SAMPLED]
    for r in rows:
        theta[r, :P], bufs[r, :Q] = th[clients[r]], bu[clients[r]]
    out_w, out_b = torch.full((P,), NAN), torch.full((Q,), NAN)
    res = RB.aggregate("geomed", theta, bufs, P, Q, rows, [clients[r] for r in rows], SAMPLED, owner, info, out_w,
                       out_b, budget=budget, hip=False, iters=3, nu=1e-6)
    return torch.cat([out_w, out_b]), res["objective"], torch.cat([th, bu], 1)


def _single(budget):
    return _run([3, 6, 7, 0, 2, 5, 1, 4], [0] * N_ROWS, 0, 1, budget)


def test_driver_follows_the_schedule_for_any_chunking():
    assert {k: len(RB.column_chunks(6, P, b)) for k, b in BUDGETS.items()} == {1: 1, 2: 2, 7: 7}
    got, obj, full = _single(BUDGETS[1])
    # z is per column and the fp64 distances only steer the weights.  Another chunking moves a weight by an fp32 ulp
    # at most: |dz| <= (K + 1) 2^-23 sum_i beta_i |x_ij| < 7 * 1.2e-7 * 4 here
    for k in (2, 7):
        other, oobj, _ = _single(BUDGETS[k])
        assert torch.allclose(other, got, rtol=0, atol=4e-6) and abs(float(oobj) - float(obj)) <= 1e-5 * float(obj)
    assert bool(torch.isfinite(got).all())  # client 5 (one Inf) is screened out
    assert torch.allclose(got, R.geometric_median(full[sorted(SAMPLED)], 3, 1e-6), rtol=1e-5, atol=1e-5)


def _dist_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.save(_run(RANK_CLIENTS[rank], OWNER, rank, world, BUDGETS[2])[:2], "%s.%d" % (out, rank))
    dist.destroy_process_group()


def test_two_rank_gloo_driver_matches_single_process(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "r.pt")
    mp.start_processes(_dist_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    ref = _single(BUDGETS[2])
    for rank in (0, 1):
        got = torch.load("%s.%d" % (out, rank), weights_only=True)
        assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)) and float(got[1]) == float(ref[1]), rank
