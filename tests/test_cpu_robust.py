"""CPU tests of ``engine/robust.py``: the torch / numpy twins of the kernels in ``robust.hip`` (order statistics under
the NaN-last, ties-by-client order; fp64 sums of squared fp32 differences; Krum scoring and selection) and the
column-chunk driver, in one process and over two gloo ranks."""
import os

import numpy as np
import pytest
import torch

from neuroimagedisttraining_amd.core import robustness as R
from neuroimagedisttraining_amd.engine import robust as RB

NAN, INF = float("nan"), float("inf")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. order twins
@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_median_twin_equals_coordinate_median_bit_for_bit(K):
    g = torch.Generator().manual_seed(K)
    M = torch.randn(K, 1031, generator=g)
    lo, hi = RB.median_range(K)
    got = RB.order_mean_twin(M, lo, hi)
    assert torch.equal(_bits(got), _bits(R.coordinate_median(M)))


@pytest.mark.parametrize("K,ratio", [(5, 0.2), (8, 0.1), (8, 0.25), (20, 0.1), (3, 0.4)])
def test_trimmed_mean_twin_within_the_sequential_sum_bound(K, ratio):
    """|twin - trimmed_mean| <= (hi - lo - 1) * 2^-24 * sum |s_r| per coordinate: the bound of a sequential fp32 sum
    of hi - lo terms (torch's own summation order obeys it too)."""
    g = torch.Generator().manual_seed(10 * K)
    M = torch.randn(K, 2053, generator=g) * 3
    lo, hi = RB.trim_range(K, ratio)
    got = RB.order_mean_twin(M, lo, hi)
    want = R.trimmed_mean(M, ratio)
    S = M.sort(dim=0).values[lo:hi].double()
    bound = (hi - lo - 1) * 2.0 ** -24 * S.abs().sum(0)
    err = (got.double() - want.double()).abs()
    print("trimmed mean: largest error / bound", float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())


def test_order_rules_nan_inf_zero_and_ties():
    for K in (5, 6, 7, 8):
        lo, hi = RB.median_range(K)
        n_ok = (K - 1) // 2  # this many NaNs leave a finite median, one more does not
        for n_nan, finite in ((n_ok, True), (n_ok + 1, False)):
            col = torch.arange(1, K + 1, dtype=torch.float32)
            pos = torch.randperm(K, generator=torch.Generator().manual_seed(K + n_nan))[:n_nan]
            col[pos] = NAN
            got = RB.order_mean_twin(col.view(K, 1), lo, hi)
            assert bool(torch.isfinite(got).all()) == finite, (K, n_nan, got)
            if finite:
                left = col[~torch.isnan(col)].sort().values
                full = torch.cat([left, torch.full((n_nan,), NAN)])
                assert float(got) == float((full[lo:hi].sum() / (hi - lo)))
    col = torch.tensor([INF, 1.0, -INF, NAN]).view(4, 1)
    assert [float(RB.order_mean_twin(col, r, r + 1)) for r in range(3)] == [-INF, 1.0, INF]
    assert bool(torch.isnan(RB.order_mean_twin(col, 3, 4)).all())
    # -0 == +0: the client order decides, and the value that is written keeps its own sign bit
    for first, second in ((0.0, -0.0), (-0.0, 0.0)):
        col = torch.tensor([first, second, 5.0, -5.0]).view(4, 1)
        s1, s2 = RB.order_mean_twin(col, 1, 2), RB.order_mean_twin(col, 2, 3)
        assert torch.equal(_bits(s1), _bits(torch.tensor([first])))
        assert torch.equal(_bits(s2), _bits(torch.tensor([second])))
    # duplicates: every rank slot of a run of equal values holds that value
    col = torch.tensor([2.0, 1.0, 2.0, 2.0, 1.0, 3.0]).view(6, 1)
    assert [float(RB.order_mean_twin(col, r, r + 1)) for r in range(6)] == [1.0, 1.0, 2.0, 2.0, 2.0, 3.0]


# ------------------------------------------------------------------------------------------------ 2. Krum twins
def _clusters(K, f, n, seed):
    """Honest rows within 0.01 of each other, ``f`` rows at +100.  The honest cluster sits at the origin: core.krum's
    fp32 Gram form resolves distances of 1e-3 only while the rows' own norms are that small too."""
    g = torch.Generator().manual_seed(seed)
    M = 0.01 * torch.rand(K, n, generator=g)
    byz = torch.randperm(K, generator=g)[:f]
    M[byz] += 100.0
    return M, set(byz.tolist())


@pytest.mark.parametrize("K,f", [(6, 1), (10, 2), (16, 3)])
def test_krum_twin_selects_what_core_krum_selects(K, f):
    M, byz = _clusters(K, f, 200, K)
    D = RB.pair_sqdist_twin(M)
    assert torch.equal(D, D.t()) and float(D.diag().abs().max()) == 0.0
    for multi in (1, K - f):
        sel, _ = RB.krum_select_twin(D, f, multi)
        _, want = R.krum(M, f=f, multi=multi)
        assert set(sel.tolist()) == set(want.tolist())
        assert not (set(sel.tolist()) & byz)


def test_krum_twin_ties_go_to_the_lower_index():
    M = torch.tensor([[0.0], [1.0], [2.0], [10.0]])  # K = 4, f = 0: m = 2; scores 5, 2, 5, 145
    D = RB.pair_sqdist_twin(M)
    sel, score = RB.krum_select_twin(D, 0, 3)
    assert score.tolist() == [5.0, 2.0, 5.0, 145.0]
    assert sel.tolist() == [1, 0, 2]
    M = 3.0 * torch.eye(5)  # every pair at squared distance 18: all scores equal
    sel, score = RB.krum_select_twin(RB.pair_sqdist_twin(M), 1, 5)
    assert set(score.tolist()) == {36.0} and sel.tolist() == [0, 1, 2, 3, 4]


def test_krum_twin_never_selects_a_nan_or_inf_row():
    g = torch.Generator().manual_seed(3)
    H = torch.randint(-8, 9, (5, 40), generator=g).float()
    M = torch.cat([H[:2], torch.full((1, 40), NAN), H[2:], torch.full((1, 40), INF)])  # rows 2 and 6 are bad
    D = RB.pair_sqdist_twin(M)
    sel, score = RB.krum_select_twin(D, 2, 5)  # K = 7, f = 2: m = 3 <= the 4 finite distances of an honest row
    assert set(sel.tolist()) == {0, 1, 3, 4, 5}
    assert not np.isfinite(score[[2, 6]]).any()
    _, score_h = RB.krum_select_twin(RB.pair_sqdist_twin(H), 0, 5)  # K = 5, f = 0: m = 3 as well
    assert score[[0, 1, 3, 4, 5]].tolist() == score_h.tolist()


# ------------------------------------------------------------------------------------------------ 3. driver
N_ROWS, P, Q = 8, 1200, 70
SAMPLED = [7, 1, 2, 4, 5, 0]
KINDS = ("krum", "multikrum", "median", "trimmed_mean")
KW = dict(f=1, multi=4, trim_ratio=0.2)


def _client_rows():
    """Client c's (params, buffers) on the 2^-6 lattice in [-4, 4] (squared distances, and the mean of four rows, are
    exact), client 4 shifted by +100."""
    g = torch.Generator().manual_seed(21)
    th = torch.randint(-256, 257, (N_ROWS, P), generator=g).float() / 64
    bu = torch.randint(-256, 257, (N_ROWS, Q), generator=g).float() / 64
    th[:, :] = th[:1] + (th - th[:1]) / 64  # clients near one another
    th[4] += 100.0
    return th, bu


def _store(clients):
    """Row matrices holding ``clients`` in that row order (padded rows; padding columns NaN)."""
    th, bu = _client_rows()
    theta = torch.full((len(clients), (P + 63) // 64 * 64), NAN)
    bufs = torch.full((len(clients), (Q + 63) // 64 * 64), NAN)
    for r, c in enumerate(clients):
        theta[r, :P], bufs[r, :Q] = th[c], bu[c]
    return theta, bufs


def _run(kind, clients, owner, info, budget):
    theta, bufs = _store(clients)
    for r, c in enumerate(clients):  # rows of clients that were not sampled must not be read
        if c not in SAMPLED:
            theta[r], bufs[r] = NAN, NAN
    rows = [r for r, c in enumerate(clients) if c in SAMPLED]
    loc = [clients[r] for r in rows]
    out_w, out_b = torch.full((P,), NAN), torch.full((Q,), NAN)
    res = RB.aggregate(kind, theta, bufs, P, Q, rows, loc, SAMPLED, owner, info, out_w, out_b, budget=budget,
                       hip=False, **KW)
    return out_w, out_b, res["sel"]


def _single(kind, budget):
    from neuroimagedisttraining_amd.parallel import runtime as rt
    info = rt.DistInfo(0, 1, 0, torch.device("cpu"), "none")
    return _run(kind, [3, 6, 7, 0, 2, 5, 1, 4], [0] * N_ROWS, info, budget)


BUDGETS = {1: 4 * 6 * 1216, 2: 4 * 6 * 640, 7: 4 * 6 * 192}


@pytest.mark.parametrize("kind", KINDS)
def test_driver_is_bit_identical_for_any_chunking(kind):
    assert {k: len(RB.column_chunks(6, P, b)) for k, b in BUDGETS.items()} == {1: 1, 2: 2, 7: 7}
    ref = _single(kind, BUDGETS[1])
    assert bool(torch.isfinite(ref[0]).all()) and bool(torch.isfinite(ref[1]).all())
    for k in (2, 7):
        got = _single(kind, BUDGETS[k])
        assert torch.equal(_bits(got[0]), _bits(ref[0])) and torch.equal(_bits(got[1]), _bits(ref[1]))
        assert got[2] == ref[2]
    # against the whole-matrix library path on the same rows
    th, bu = _client_rows()
    order = sorted(SAMPLED)
    M = torch.cat([th[order], bu[order]], 1)
    if kind == "median":
        assert torch.equal(torch.cat([ref[0], ref[1]]), R.coordinate_median(M))
    elif kind == "trimmed_mean":
        assert torch.allclose(torch.cat([ref[0], ref[1]]), R.trimmed_mean(M, KW["trim_ratio"]), atol=1e-5)
    else:
        multi = 1 if kind == "krum" else KW["multi"]
        _, want = R.krum(M, f=KW["f"], multi=multi)
        assert ref[2] == sorted(order[i] for i in want.tolist()) and 4 not in ref[2]
        assert torch.equal(torch.cat([ref[0], ref[1]]), M[[order.index(c) for c in ref[2]]].mean(0))


OWNER = [0, 1, 0, 0, 1, 1, 1, 0]
RANK_CLIENTS = {0: [3, 7, 0, 2], 1: [5, 6, 1, 4]}  # rank 0's sampled rows are consecutive, rank 1's are not


def _dist_worker(rank, world, port, out):
    import torch.distributed as dist
    from neuroimagedisttraining_amd.parallel import runtime as rt
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    info = rt.DistInfo(rank, world, rank, torch.device("cpu"), "gloo")
    res = {kind: _run(kind, RANK_CLIENTS[rank], OWNER, info, BUDGETS[2]) for kind in KINDS}
    torch.save(res, "%s.%d" % (out, rank))
    dist.destroy_process_group()


def test_two_rank_gloo_driver_matches_single_process(tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "r.pt")
    mp.start_processes(_dist_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    for rank in (0, 1):
        got = torch.load("%s.%d" % (out, rank), weights_only=True)
        for kind in KINDS:
            ref = _single(kind, BUDGETS[2])
            assert torch.equal(_bits(got[kind][0]), _bits(ref[0])), (rank, kind)
            assert torch.equal(_bits(got[kind][1]), _bits(ref[1])), (rank, kind)
            assert got[kind][2] == ref[2]
