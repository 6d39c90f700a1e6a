"""CPU proof of ``tests/_rowlattice.py``: every table entry meets its preconditions, the fp32 chain evaluated step by
step equals the fp64 reference, the reference formula reproduces ``TorchEngine.local_opt`` run in fp64 (an independence
check of the formula, not the oracle), the counted bound of the non-dyadic coefficient case holds for three summation
orders, the radix reference agrees with ``torch.topk``, and four mutations of a correct fp32 twin show what the older
relative-norm checks of the optimizer miss."""
import itertools

import numpy as np
import pytest
import torch

import _lattice as L
import _rowlattice as RL

AX = ("client", "element")


# ------------------------------------------------------------------------------------------------ tables
def test_tables_reach_every_path():
    assert RL.opt_chunk(RL.OPT_P_BIG[0]) == (8192, 258)            # second trip of the 256-thread partial loop
    assert RL.opt_chunk(RL.OPT_P_BIG[1]) == (8196, 1024)           # the rescaled chunk
    assert RL.opt_chunk(8192 * 1024) == (8192, 1024) and RL.opt_chunk(8192 * 1024 + 1)[0] > 8192
    assert {P % 4 for P in RL.OPT_P} == {0, 1, 2, 3} and min(RL.OPT_P) < 4
    flags = RL.pairwise_flags()
    vals = [(0, 1, 2)] + [(False, True)] * 8
    for i, j in itertools.combinations(range(9), 2):
        assert {(r[i], r[j]) for r in flags} == set(itertools.product(vals[i], vals[j])), (i, j)
    full = {(c.mode, c.shared, c.mom, c.mu, c.lamda) for c in RL.opt_cfgs(RL.OPT_P_FULL)}
    assert full == {RL._norm_cfg(RL.OptCfg(RL.OPT_P_FULL, 3, *r, False, False, False, False))[2:7]
                    for r in itertools.product((0, 1, 2), *[(False, True)] * 4)} and len(full) == 40
    # the other four flags of the product entries do not follow the product's flags: FedProx entries clipped and
    # unclipped, Ditto with shared and per-row references, momentum with and without keep_grad, both lr forms
    prod = RL.opt_cfgs(RL.OPT_P_FULL)[len(flags):]
    for a, b in (("mu", "clipped"), ("lamda", "ref_shared"), ("mom", "keep_grad"), ("mu", "lr_dev"), ("mode", "clipped")):
        va = {getattr(c, a) for c in prod}
        assert {(getattr(c, a), getattr(c, b)) for c in prod} == set(itertools.product(va, (False, True))), (a, b)
    for P in RL.OPT_P:
        cf = RL.opt_cfgs(P)
        assert {c.keep_grad for c in cf} == {c.lr_dev for c in cf} == {False, True}
        assert {c.clipped for c in cf} == ({False} if P in RL.OPT_P_NOCLIP else {False, True})
        assert {(c.mu, c.ref_shared) for c in cf} >= {(True, False), (True, True)}
    for P in RL.CSM_P:
        cf = RL.csm_cfgs(P)
        assert {(c.mask, c.mom, c.wbf, c.first) for c in cf} == set(itertools.product((False, True), repeat=4))
        assert {c.lr_dev for c in cf} == {c.keep_grad for c in cf} == {False, True}
        if P not in RL.OPT_P_NOCLIP:
            assert {(c.wbf, c.clipped) for c in cf} == set(itertools.product((False, True), repeat=2))
            assert {(c.mask, c.clipped) for c in cf} == {(c.mom, c.clipped) for c in cf} == {(c.wbf, c.clipped) for c in cf}
    pm = RL.PACK_MODES
    for i, j in itertools.combinations((2, 4, 5, 6), 2):            # mode, mom, mu, lamda
        assert {(c[i], c[j]) for c in pm} == set(itertools.product({c[i] for c in pm}, (False, True))), (i, j)
    assert {c.mode for c in pm} == {0, 1, 2} and all(c.clipped for c in pm)


def test_pack_layout_offsets():
    layers, P = RL.pack_layout()
    assert layers[0][0] == 5 and 1.2e5 < P < 1.4e5
    ends = [o + co * ci * k * k for o, co, ci, k in layers]
    assert [b[0] - e for b, e in zip(layers[1:], ends)] == [1, 3, 67] and P - ends[-1] == 4099
    starts = [0] + ends
    assert {s % 4 for s in starts} == {0, 1, 2}
    assert {(layers[0][0] + 27 * co) % 4 for co in range(64)} == {0, 1, 2, 3}   # the stem's chunk starts
    assert P - ends[-1] > 4096                                                   # one range split at 4096


def test_mask_bits_set_past_P_and_forced_bits():
    rng = RL.rng_of("bits")
    for P in (1, 5, 33, 1027):
        m = RL.mask_rows(3, P, rng)
        bits = RL.pack_bits_high(m)
        assert bits.shape == (3, RL.mask_words(P)) and bits.dtype == torch.int32
        w = bits.numpy().view(np.uint32)
        allb = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(3, -1)
        assert np.array_equal(allb[:, :P].astype(bool), m) and bool(allb[:, P:].all())
        for q, p in enumerate(RL.forced_positions(P)):
            assert [bool(m[r, p]) for r in range(3)] == [bool((q + r) & 1) for r in range(3)]


# ------------------------------------------------------------------------------------------------ optimizer chain
def _check_fp32(c, chain):
    """The fp32 evaluation (sum of squares, coefficient, chain: one rounding per operation) equals the fp64 reference."""
    w1, g1, b1 = chain(np.float32)
    L.assert_exact(torch.from_numpy(w1), torch.from_numpy(c.w1), AX)
    L.assert_exact(torch.from_numpy(g1), torch.from_numpy(c.g1), AX)
    if c.buf1 is not None:
        L.assert_exact(torch.from_numpy(b1), torch.from_numpy(c.buf1), AX)


def _opt_fp32(c):
    cfg, C, P = c.cfg, c.C, c.P
    refb, prefb = np.broadcast_to(c.ref, (C, P)), np.broadcast_to(c.pref, (C, P))
    t32 = np.stack([RL.sqnorm_terms(c.w[r], c.g[r], refb[r], c.m[r], cfg.mode, cfg.mu, np.float32).sum(dtype=np.float32)
                    for r in range(C)])
    assert t32.dtype == np.float32 and np.array_equal(t32.astype(np.float64), c.t)
    coef32 = RL.clip_coef(t32, c.max_norm, np.float32)
    assert np.array_equal(coef32.astype(np.float64), c.coef)
    _check_fp32(c, lambda f: RL.opt_chain(c.w, c.g, c.buf, refb, prefb, c.m, coef32[:, None], cfg.mode, cfg.mom, cfg.mu,
                                          cfg.lamda, f))
    if cfg.clipped:
        assert len(set(c.m_exp)) == C and all(c.t[r] == 4.0 ** c.m_exp[r] for r in range(C))
        assert c.max_norm < np.sqrt(c.t.min()) and np.log2(c.max_norm) == int(np.log2(c.max_norm))
    assert float(np.abs(c.w).max()) <= 8 and float(np.abs(c.ref).max()) <= 8 and float(np.abs(c.pref).max()) <= 8
    assert np.array_equal(c.buf * 4, np.round(c.buf * 4))
    big = np.abs(c.g) > 2                                           # the spikes: powers of two, few
    assert int(big.sum()) <= RL.N_SPIKES * C
    assert np.array_equal(np.log2(np.abs(c.g[big])), np.round(np.log2(np.abs(c.g[big]))))


@pytest.mark.parametrize("P", RL.OPT_P)
def test_local_opt_cases_are_exact_in_fp32(P):
    for cfg in RL.opt_cfgs(P):
        _opt_fp32(RL.opt_case(cfg))


@pytest.mark.parametrize("P,i", [(P, i) for P in RL.OPT_P_BIG for i in range(2)])
def test_local_opt_large_cases_are_exact_in_fp32(P, i):
    """Both configurations at nblk = 258 and both at the rescaled chunk."""
    assert len(RL.opt_cfgs(P)) == 2
    cfg = RL.opt_cfgs(P)[i]
    c = RL.opt_case(cfg)
    assert float(np.abs(c.g).max()) <= 2.0 ** (c.m_exp[-1] - 1) and not cfg.mu
    _opt_fp32(c)


def test_pack_cases_are_exact_in_fp32():
    for cfg in RL.PACK_MODES:
        c = RL.pack_case(cfg)
        assert c.P == RL.pack_layout()[1]
        _opt_fp32(c)


@pytest.mark.parametrize("P", RL.CSM_P)
def test_clip_sgd_mask_cases_are_exact_in_fp32_and_round_in_bf16(P):
    ties = inexact = 0
    for cfg in RL.csm_cfgs(P):
        c = RL.csm_case(cfg)
        t32 = (c.g.astype(np.float32) ** 2).sum(1, dtype=np.float32)
        assert np.array_equal(t32.astype(np.float64), c.t)
        coef32 = RL.clip_coef(t32, c.max_norm, np.float32)
        assert np.array_equal(coef32.astype(np.float64), c.coef)
        _check_fp32(c, lambda f: RL.csm_chain(c.w, c.g, c.buf, c.mask, coef32[:, None], cfg.mom, cfg.first, f))
        if cfg.wbf:
            assert torch.equal(c.wbf, torch.from_numpy(c.w1.astype(np.float32)).to(torch.bfloat16).view(torch.int16))
            if cfg.clipped:
                assert RL.bf16_ties(c.w1) > 0 and RL.bf16_inexact(c.w1) > RL.bf16_ties(c.w1)
            ties += RL.bf16_ties(c.w1)
            inexact += RL.bf16_inexact(c.w1)
    if P not in RL.OPT_P_NOCLIP:  # the tables that can clip contain values that round in bf16, exact ties among them
        assert ties > 100 and inexact > 2 * ties


def test_pack_table_contains_bf16_ties():
    c = RL.pack_case(RL.PACK_MODES[0])
    assert RL.bf16_ties(c.w1) > 1000 and RL.bf16_inexact(c.w1) > RL.bf16_ties(c.w1)


# ------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("P", (5, 1027, RL.OPT_P_FULL))
def test_reference_reproduces_torch_engine_in_fp64(P):
    """``TorchEngine.local_opt`` on fp64 rows, one row per call (it takes one shared reference row).  Unclipped cases
    agree exactly.  Clipped ones agree to 1e-7 max|g|: the twin adds a double 1e-6 to the norm, which a norm of 32 or
    more absorbs in fp32 but not in fp64 (relative 1e-6 / 32 on the coefficient)."""
    from neuroimagedisttraining_amd.engine.executor import TorchEngine
    from neuroimagedisttraining_amd.engine.runner import StepSpec
    for cfg in RL.opt_cfgs(P):
        c = RL.opt_case(cfg)
        th, gr, bu = (torch.from_numpy(x.copy()) for x in (c.w, c.g, c.buf))
        for r in range(c.C):
            rr = 0 if cfg.ref_shared else r
            br = None if c.bits is None else c.bits[(0 if cfg.shared else r):(0 if cfg.shared else r) + 1]
            spec = StepSpec(mask_mode=cfg.mode, bits=br, shared=True, prox_mu=RL.MU if cfg.mu else 0.0,
                            ref=torch.from_numpy(c.ref[rr]) if cfg.mu else None, lamda=RL.LAMDA if cfg.lamda else 0.0,
                            pref=torch.from_numpy(c.pref[rr]) if cfg.lamda else None)
            TorchEngine.local_opt(None, th[r:r + 1], gr[r:r + 1], bu[r:r + 1] if cfg.mom else None, spec, RL.LR, RL.WD,
                                  RL.MOM if cfg.mom else 0.0, c.max_norm, keep_grad=True)
        tol = 1e-7 * float(np.abs(c.g).max()) if cfg.clipped else 0.0
        for got, ref in ((th, c.w1), (gr, c.g1)) + (((bu, c.buf1),) if cfg.mom else ()):
            assert float((got - torch.from_numpy(ref)).abs().max()) <= tol, cfg


# ------------------------------------------------------------------------------------------------ mutations
OLD_G, OLD_P, OLD_LR, OLD_WD, OLD_MAX = 4, 2570241, 0.01, 5e-4, 10.0


def _old_operands():
    """The operands of test_local_opt_matches_reference_order / test_clip_sgd_mask_matches_reference (scales and shape)."""
    g_ = L.gen("old optimizer test")
    theta = torch.randn(OLD_G, OLD_P, generator=g_)
    grad = torch.randn(OLD_G, OLD_P, generator=g_) * 0.01
    grad[1] *= 1000
    mask = torch.rand(OLD_P, generator=g_) > 0.5
    coef = torch.clamp(OLD_MAX / (grad.double().norm(dim=1) + 1e-6), max=1.0).float()
    # every row is clipped there (0.01 sqrt(P) = 16 > 10): rows 0, 2, 3 to about 0.62, row 1 to about 6e-4
    assert coef[1] < 1e-3 and bool(((coef[[0, 2, 3]] > 0.6) & (coef[[0, 2, 3]] < 0.65)).all())
    assert len(set(coef.tolist())) == OLD_G
    return theta, grad, mask, coef


def _step32(theta, grad, mask, coef, wd=None):
    """A correct fp32 twin of the masked clip + SGD step (no momentum); ``wd``: per-element weight decay."""
    wd = OLD_WD if wd is None else wd
    return torch.where(mask, theta - OLD_LR * (grad * coef.view(-1, 1) + wd * theta), torch.zeros(()))


def _lattice_mode1():
    cfg = next(c for c in RL.opt_cfgs(RL.OPT_P_FULL) if c.mode == 1 and c.clipped and not c.mu and not c.lamda
               and not c.mom and not c.shared)
    return RL.opt_case(cfg)


def _fails_at(bad, c, row, col):
    with pytest.raises(AssertionError) as e:
        L.assert_exact(torch.from_numpy(bad), torch.from_numpy(c.w1), AX)
    assert "first at (client=%d, element=%d)" % (row, col) in str(e.value), str(e.value)


def test_norm_threshold_misses_an_unupdated_tail_element():
    """P % 4 == 1: the scalar tail element of every row left at its old value moves the old quotient by about 1e-7;
    on the lattice assert_exact names it."""
    theta, grad, mask, coef = _old_operands()
    good = _step32(theta, grad, mask, coef)
    bad = good.clone()
    bad[:, -1] = theta[:, -1]
    assert not torch.equal(bad, good) and RL.relerr(bad, good) < 1e-6
    c = _lattice_mode1()
    r = int(np.flatnonzero(c.w1[:, -1] != c.w[:, -1])[0])
    bad = c.w1.copy()
    bad[r, -1] = c.w[r, -1]
    _fails_at(bad, c, r, c.P - 1)


def test_norm_threshold_misses_weight_decay_dropped_at_a_chunk_end():
    """Weight decay left out on the last element of the first chunk (element 8191) of every row."""
    theta, grad, mask, coef = _old_operands()
    good = _step32(theta, grad, mask, coef)
    wd = torch.full((1, OLD_P), OLD_WD)
    wd[0, RL.OPT_CHUNK - 1] = 0.0
    bad = _step32(theta, grad, mask | True, coef, wd)
    bad = torch.where(mask, bad, torch.zeros(()))
    if not bool(mask[RL.OPT_CHUNK - 1]):
        pytest.fail("the draw masks element 8191: choose another seed")
    assert not torch.equal(bad, good) and RL.relerr(bad, good) < 1e-6
    c = _lattice_mode1()
    i = RL.OPT_CHUNK - 1
    r = int(np.flatnonzero(c.m[:, i] & (c.w[:, i] != 0))[0])
    bad = c.w1.copy()
    bad[r, i] = c.w[r, i] - RL.LR * c.g1[r, i]
    _fails_at(bad, c, r, i)


def test_norm_threshold_misses_a_mask_bit_from_the_neighbouring_nibble():
    """One small kept weight zeroed because its bit was read four elements further on."""
    theta, grad, mask, coef = _old_operands()
    good = _step32(theta, grad, mask, coef)
    cand = torch.nonzero(mask[:-4] & ~mask[4:] & (good[0, :-4].abs() < 1e-3) & (good[0, :-4] != 0)).flatten()
    i = int(cand[0])
    bad = good.clone()
    bad[0, i] = 0.0
    assert RL.relerr(bad, good) < 1e-6
    c = _lattice_mode1()
    i = int(np.flatnonzero(c.m[0, :-4] & ~c.m[0, 4:] & (c.w1[0, :-4] != 0))[0])
    bad = c.w1.copy()
    bad[0, i] = 0.0
    _fails_at(bad, c, 0, i)


def test_norm_threshold_misses_a_neighbouring_rows_coefficient():
    """The first row's coefficient (0.62) used for the second row, the one the older test scales up (6e-4): this the old
    quotient does see, the row's step grows a thousandfold and the quotient moves by about 3e-2.  It does not see the
    same fault between the other rows, which that test also clips (0.01 sqrt(P) = 16 > 10) to coefficients within
    0.1 % of each other: row 2 stepped with row 3's coefficient moves the quotient by about 1e-8.  On the lattice the
    rows' coefficients differ by powers of two and every element with a non-zero gradient fails."""
    theta, grad, mask, coef = _old_operands()
    good = _step32(theta, grad, mask, coef)
    wrong = coef.clone()
    wrong[1] = coef[0]
    assert RL.relerr(_step32(theta, grad, mask, wrong), good) > 1e-6        # caught by the old check
    near = coef.clone()
    near[2] = coef[3]
    bad = _step32(theta, grad, mask, near)
    assert not torch.equal(bad, good) and RL.relerr(bad, good) < 1e-6       # missed
    c = _lattice_mode1()
    cfg = c.cfg
    wrong = c.coef.copy()
    wrong[1] = c.coef[0]
    bad = RL.opt_chain(c.w, c.g, c.buf, np.broadcast_to(c.ref, c.w.shape), np.broadcast_to(c.pref, c.w.shape), c.m,
                       wrong[:, None], cfg.mode, cfg.mom, cfg.mu, cfg.lamda)[0]
    n = int((bad != c.w1).sum())
    assert n == int((c.m[1] & (c.g[1] != 0)).sum()) > c.P // 4
    with pytest.raises(AssertionError) as e:
        L.assert_exact(torch.from_numpy(bad), torch.from_numpy(c.w1), AX)
    assert str(e.value).startswith("%d of " % n) and "client=1" in str(e.value)


# ------------------------------------------------------------------------------------------------ coefficient bound
@pytest.mark.parametrize("P", RL.COEF_P)
def test_coefficient_bound_holds_for_three_summation_orders(P):
    """The fp32 sum of squares in the kernels' order, in that order over the reversed row and as one pairwise tree
    (every term passes through fewer fp32 roundings than K_COEF counts) gives a coefficient inside the bound; the
    neighbouring row's coefficient is outside."""
    c = RL.coef_case(P)
    for r in range(c.C):
        sq = (c.g[r].numpy() * c.g[r].numpy()).astype(np.float32)
        for t in (RL.sum_order_kernel(sq), RL.sum_order_kernel(sq, True), RL.sum_order_pairwise(sq)):
            coef = np.float32(RL.COEF_MAX_NORM) / (np.sqrt(np.float32(t)) + np.float32(1e-6))
            assert abs(float(coef) - float(c.coef[r])) <= float(c.coef_bound[r]), (r, t)
            # one more ulp on the square root and on the quotient (not assumed correctly rounded) still fits
            worst = float(coef) * (1 + 4 * 2.0 ** -24)
            assert abs(worst - float(c.coef[r])) <= float(c.coef_bound[r])
        other = float(c.coef[(r + 1) % c.C])
        assert abs(other - float(c.coef[r])) > 1000 * float(c.coef_bound[r])
    assert RL.K_COEF == 26 and RL.K_GRAD == 27


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("name", RL.SELECT_SETS)
def test_radix_reference_agrees_with_topk(name):
    for n in RL.SELECT_N:
        bits = RL.select_data(name, n)
        assert bits.dtype == np.uint32 and int(bits.max()) <= RL.INF_BITS          # non-negative, no NaN
        v = torch.from_numpy(bits.view(np.float32).copy())
        ks = RL.select_ranks(bits)
        assert {1, n}.issubset(ks) and all(1 <= k <= n for k in ks)
        if n > 5000:
            ks = ks[:6] + ks[-6:]
        srt = torch.sort(v, descending=True).values
        for k in ks:
            thr = RL.kth_largest_bits(bits, k)
            assert thr == int(srt[k - 1].view(torch.int32)) & 0xffffffff
            assert thr == int(torch.topk(v, k).values[-1].view(torch.int32)) & 0xffffffff, (n, k)
    big = RL.select_data(name, 4099)
    vals = set(RL.select_values(name))
    assert set(big.tolist()) == vals                                                # every value of the set occurs
    if name.startswith("zero_digit_"):
        j = int(name[-1])
        zero = [b for b in vals if (b >> (8 * j)) & 0xff == 0]
        thr = {RL.kth_largest_bits(big, k) for k in RL.select_ranks(big)}
        # a threshold with digit 0 at byte j, and larger values that share its higher bytes (so the scan passes them)
        assert any(b in thr and any(o > b and o >> (8 * (j + 1)) == b >> (8 * (j + 1)) for o in vals) for b in zero)
    if name == "denormals":
        assert 0 in vals and any(0 < b < 0x00800000 for b in vals)
    if name == "with_inf":
        assert 0 < int((big == RL.INF_BITS).sum()) < 20


# ------------------------------------------------------------------------------------------------ row kernels
def test_row_kernel_lattices_are_exact():
    for n in RL.SQDIST_N:
        nblk, chunk = RL.pair_sqdist_chunks(n)
        L.require_fp32_exact(chunk * 16.0 ** 2, "pair_sqdist partial at n = %d" % n)   # |a - b| <= 16 per element
        assert nblk * chunk >= n and (nblk - 1) * chunk < n
    assert RL.pair_sqdist_chunks(RL.SQDIST_N[-1])[0] == 256 and RL.pair_sqdist_chunks(16385)[0] == 2
    assert all(60 % k == 0 for k in range(1, 7))                                       # masked_mean_rows: num / cnt
    L.require_fp32_exact(6 * 60 * 8, "masked_mean_rows numerator")
    L.require_fp32_exact(5 * 8 * 2.0 * 4 + 8 * 2, "weighted_rows_sum in quarters")
    assert all(w * 4 == int(w * 4) for w in RL.ROW_WEIGHTS)
