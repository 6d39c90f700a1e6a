"""Dyadic-lattice operands, fp64 references, case tables and comparisons for the optimizer kernels (``optim.hip``:
``clip_sgd_mask``, ``local_opt``, ``local_opt_pack``, ``local_opt_pack_wt``), the SNIP selection kernels (``select.hip``)
and the row aggregation kernels (``weighted_rows_sum`` / ``broadcast_row`` of ``optim.hip``, ``masked_rows_sum``,
``masked_mean_rows``, ``mix_rows``, ``pair_sqdist`` of ``sparse.hip``).

These kernels are elementwise chains and order-free sums.  On operands that are small multiples of a power of two,
every product, every sum and every partial sum is an fp32 value, with or without fused multiply-adds and in any order,
so a correct kernel equals the fp64 reference bit for bit and one wrong, skipped or doubled element fails
``assert_exact``.

The optimizer lattice: ``w``, ``ref``, ``pref`` integers in [-8, 8] with ``w - ref`` in [-2, 2], ``buf`` an integer / 4,
``g`` an integer in [-2, 2] (in {-1, 0, 1} at the two large P), ``lr = 2^-2``, ``wd = 2^-3``, ``mom = mu = lamda = 2^-1``.
The clip coefficient ``min(1, max_norm / (sqrtf(t) + 1e-6f))`` is made a power of two either by ``max_norm = 2^20``
(coefficient 1) or by a row norm ``t = 4^m`` with ``sqrt(t) >= 32`` (in fp32 ``32 + 1e-6f == 32`` while ``16 + 1e-6f !=
16``) and ``max_norm`` a power of two below it.  ``t`` is the masked, prox-adjusted squared norm; the generator reaches
``4^m`` exactly by clearing up to 36 *spike* elements of the row and writing the base-4 digits of the remainder there:
an entry ``g = +-2^j`` (with ``w = ref``) adds ``4^j``, an entry ``w - ref = +-1``, ``g = 0`` adds ``mu^2 = 1/4``.  The
spikes are the only entries of ``g`` beyond [-2, 2] (powers of two up to ``2^(m-1)``).  Rows of one call get different
``m``, so a kernel that takes another row's coefficient fails.  For large P the density of non-zero ``g`` (and of
``w != ref``) is lowered so that ``t`` stays below ``4^m``.

The preconditions are asserted here on the reference alone: the partial-sum bound of ``t`` in units of its lattice
spacing is below 2^24, ``t = 4^m``, and every intermediate of the chain survives a cast to fp32 and back.

This is a plain helper module (no fixtures): ``tests/test_cpu_rowlattice.py`` proves it without a GPU,
``tests/test_gpu_exact_rows.py`` runs the kernels.
"""
import collections
import functools
import itertools
import types
import zlib

import numpy as np
import torch

from _lattice import FP32_EXACT, assert_exact, require_fp32_exact  # noqa: F401  (re-exported)

LR, WD, MOM, MU, LAMDA = 2.0 ** -2, 2.0 ** -3, 2.0 ** -1, 2.0 ** -1, 2.0 ** -1
MAX_NORM_OFF = 2.0 ** 20               # unclipped form: the coefficient is 1
EPS32 = float(np.float32(1e-6))        # the kernels' 1e-6f as a double
OPT_THREADS, OPT_CHUNK = 256, 8192     # kOptThreads, opt_chunk's default chunk
N_SPIKES = 36                          # a remainder below 4^11 has 12 base-4 digits in quarters, each at most 3
FORCED = (0, 3, 4, 31, 32)             # and P - 1: elements whose mask bit is forced (single set / cleared bits)

# smallest P that reach each path of opt_chunk / opt_range / the sqnorm kernels (chunk 8192, 256 threads x 4 floats)
OPT_P = (1, 3, 4, 5, 1023, 1024, 1027, 8191, 8192, 8193, 8197, 3 * 8192 + 2)
OPT_P_FULL = 8197                      # the full flag product runs here
OPT_P_NOCLIP = (1, 3, 4, 5)            # too few elements for the spikes: unclipped form only
OPT_P_BIG = (2105345, 8388609)         # nblk = 258 (second trip of the partial loop); opt_chunk rescales (8196 x 1024)
OPT_C, OPT_C_BIG = 3, 2

OptCfg = collections.namedtuple("OptCfg", "P C mode shared mom mu lamda ref_shared clipped keep_grad lr_dev")
CsmCfg = collections.namedtuple("CsmCfg", "P C mask mom wbf first clipped keep_grad lr_dev")


def opt_chunk(P):
    """Python twin of ``opt_chunk`` (optim.hip): (chunk, blocks per row)."""
    chunk = OPT_CHUNK
    nb = (P + chunk - 1) // chunk
    if nb > 1024:
        chunk = ((P + 1023) // 1024 + 3) & ~3
        nb = (P + chunk - 1) // chunk
    return chunk, nb


def mask_words(P):
    return ((P + 31) // 32 + 3) // 4 * 4


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------ case tables
@functools.lru_cache(maxsize=None)
def pairwise_flags():
    """A pairwise-covering subset of (mode, shared, mom, mu, lamda, ref_shared, clipped, keep_grad, lr_dev): every
    pair of values of two flags occurs in some row (greedy, deterministic)."""
    vals = [(0, 1, 2)] + [(False, True)] * 8
    full = list(itertools.product(*vals))
    todo = {((i, a), (j, b)) for i in range(9) for j in range(i + 1, 9) for a in vals[i] for b in vals[j]}
    rows = []
    while todo:
        best = max(full, key=lambda r: sum(1 for (i, a), (j, b) in todo if r[i] == a and r[j] == b))
        rows.append(best)
        todo = {p for p in todo if not (best[p[0][0]] == p[0][1] and best[p[1][0]] == p[1][1])}
    return tuple(rows)


def _norm_cfg(c):
    """Flags without effect set to one value (so equal cases are listed once)."""
    if c.mode == 0:
        c = c._replace(shared=False)
    if not (c.mu or c.lamda):
        c = c._replace(ref_shared=False)
    if c.P in OPT_P_NOCLIP:
        c = c._replace(clipped=False)
    return c


@functools.lru_cache(maxsize=None)
def opt_cfgs(P):
    """The ``local_opt`` configurations at P: pairwise-covering, the full product of (mode, shared, mom, mu, lamda) at
    ``OPT_P_FULL`` (the other four flags from a hash of the entry's index, so independent of the product's flags), two
    at the large P (g in {-1, 0, 1}, no prox)."""
    if P in OPT_P_BIG:
        return (OptCfg(P, OPT_C_BIG, 1, True, True, False, False, False, True, True, False),
                OptCfg(P, OPT_C_BIG, 2, False, False, False, False, False, True, False, True))
    out = [OptCfg(P, OPT_C, *r) for r in pairwise_flags()]
    if P == OPT_P_FULL:
        for i, (mode, shared, mom, mu, lamda) in enumerate(itertools.product((0, 1, 2), (False, True), (False, True),
                                                                              (False, True), (False, True))):
            h = zlib.crc32(b"full product %d" % i)
            out.append(OptCfg(P, OPT_C, mode, shared, mom, mu, lamda, bool(h & 1), bool(h & 2), bool(h & 4), bool(h & 8)))
    seen, res = set(), []
    for c in map(_norm_cfg, out):
        if c not in seen:
            seen.add(c)
            res.append(c)
    return tuple(res)


@functools.lru_cache(maxsize=None)
def csm_cfgs(P):
    """``clip_sgd_mask``: the eight instantiations (float mask, momentum, bf16 emission), ``first`` 0 / 1, clipped or
    not, keep_grad, lr_dev (the last three from a hash of the entry's index, the same at every P)."""
    out = []
    for i, (mask, mom, wbf) in enumerate(itertools.product((False, True), repeat=3)):
        for first in (False, True):
            h = zlib.crc32(b"clip_sgd_mask %d" % (2 * i + first))
            clipped = P not in OPT_P_NOCLIP and bool(h & 3)
            out.append(CsmCfg(P, OPT_C, mask, mom, wbf, first, clipped, bool(h & 4), bool(h & 8)))
    return tuple(out)


CSM_P = OPT_P
CSM_SHIFT = 5
PACK_MODES = tuple(OptCfg(0, OPT_C, *r) for r in (
    # (mode, shared, mom, mu, lamda, ref_shared, clipped, keep_grad, lr_dev): pairwise over mode x mom x mu x lamda
    (0, False, True, True, True, True, True, True, False),
    (0, False, False, False, False, False, True, False, True),
    (1, True, True, False, True, False, True, False, False),
    (1, False, False, True, False, True, True, True, True),
    (2, False, True, True, False, False, True, True, False),
    (2, True, False, False, True, True, True, False, False),
    (1, False, True, False, False, False, True, True, False),
    (2, False, False, True, True, False, True, False, True),
    (0, False, True, False, False, False, True, True, False),
    (0, False, False, True, False, True, True, False, False),
    (1, False, False, False, True, True, True, True, False),
    (2, False, True, False, True, True, True, True, False)))

# synthetic pack layout: (cout, cin, k) of the conv layers, the first offset, and the gaps after each layer
PACK_LAYERS = ((64, 3, 3), (64, 64, 3), (128, 64, 1), (64, 128, 3))
PACK_FIRST, PACK_GAPS = 5, (1, 3, 67, 4099)


def pack_layout():
    """[(offset, cout, cin, k)], P of the synthetic layout: layer starts at residues 1, 2, 1, 0 mod 4 (the stem's
    per-output-channel chunks, 27 floats apart, at every residue), the other parameter ranges start at residues 0, 1, 2,
    1, 0 and the last one (4099 floats) is split at 4096."""
    out, off = [], PACK_FIRST
    for (cout, cin, k), gap in zip(PACK_LAYERS, PACK_GAPS):
        out.append((off, cout, cin, k))
        off += cout * cin * k * k + gap
    return out, off


# ------------------------------------------------------------------------------------------------ mask bits
def forced_positions(P):
    return sorted({p for p in FORCED + (P - 1,) if 0 <= p < P})


def mask_rows(R, P, rng):
    """Random bool [R, P] with single set and cleared bits forced: at each forced element the bit alternates with the
    element's rank and the row, and the following element (where it is free) gets the opposite bit."""
    m = rng.random((R, P)) < 0.5
    fp = forced_positions(P)
    for r in range(R):
        for q, p in enumerate(fp):
            b = bool((q + r) & 1)
            m[r, p] = b
            if p + 1 < P and p + 1 not in fp:
                m[r, p + 1] = not b
    return m


def pack_bits_high(m):
    """bool [R, P] -> int32 bit rows [R, W] (bit i of word i >> 5) with every unused bit (from P to 32 W) SET: a kernel
    that reads a bit past P sees a kept element."""
    R, P = m.shape
    W = mask_words(P)
    full = np.ones((R, W * 32), dtype=bool)
    full[:, :P] = m
    words = (full.reshape(R, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy())


def unpack_bits_np(bits, P):
    w = bits.numpy().view(np.uint32)
    return (((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w.shape[0], -1)[:, :P]).astype(bool)


# ------------------------------------------------------------------------------------------------ the chain
def roundtrips(x):
    return bool(np.array_equal(x.astype(np.float32).astype(np.float64), x))


def opt_chain(w, g, buf, ref, pref, m, coef, mode, mom, mu, lamda, dtype=np.float64, trace=None, lr=LR):
    """The element step of ``LocalOpt`` (header comment of optim.hip), one operation per line, in ``dtype``:
       g' = g m (mode 2);  g' += mu (w - ref);  g' *= coef;  d = wd w + g';  buf = mom buf + d, d = buf;
       w -= lr d;  w -= lr lamda (w - pref);  w = 0 where m is off (mode 1).
    Returns (w, g', buf).  ``trace``: a list that receives every intermediate."""
    f = dtype
    keep = (lambda x: (trace.append(x), x)[1]) if trace is not None else (lambda x: x)
    w, g = w.astype(f), g.astype(f)
    gj = np.where(m, g, f(0)) if mode == 2 else g
    if mu:
        dr = keep(w - ref.astype(f))
        gj = keep(keep(f(MU) * dr) + gj)
    gj = keep(gj * coef.astype(f))
    d = keep(keep(f(WD) * w) + gj)
    b = None
    if mom:
        b = keep(keep(f(MOM) * buf.astype(f)) + d)
        d = b
    w1 = keep(w - keep(f(lr) * d))
    if lamda:
        pull = f(f(lr) * f(LAMDA))
        w1 = keep(w1 - keep(pull * keep(w1 - pref.astype(f))))
    if mode == 1:
        w1 = np.where(m, w1, f(0))
    return w1, gj, b


def csm_chain(w, g, buf, mask, coef, mom, first, dtype=np.float64, trace=None, lr=LR):
    """The element step of ``clip_sgd_mask`` (header comment of optim.hip): g *= coef; d = g + wd w;
    buf = first ? d : mom buf + d, d = buf; w -= lr d; w *= mask."""
    f = dtype
    keep = (lambda x: (trace.append(x), x)[1]) if trace is not None else (lambda x: x)
    w, g = w.astype(f), g.astype(f)
    gj = keep(g * coef.astype(f))
    d = keep(keep(f(WD) * w) + gj)
    b = None
    if mom:
        b = d if first else keep(keep(f(MOM) * buf.astype(f)) + d)
        d = b
    w1 = keep(w - keep(f(lr) * d))
    if mask is not None:
        w1 = keep(w1 * mask.astype(f))
    return w1, gj, b


def clip_coef(t, max_norm, dtype=np.float64):
    """min(1, max_norm / (sqrtf(t) + 1e-6f)) per row.  The sum ``sqrtf(t) + 1e-6f`` is an fp32 sum by definition of the
    step (on the lattice sqrt(t) is a power of two >= 32, which absorbs the 1e-6f; in fp64 it would not); the square
    root and the division are taken in ``dtype`` and are exact on the lattice."""
    f = dtype
    den = (np.sqrt(t.astype(f)).astype(np.float32) + np.float32(EPS32)).astype(f)
    c = f(max_norm) / den
    return np.minimum(c, f(1)).astype(f)


def sqnorm_terms(w, g, ref, m, mode, mu, dtype=np.float64):
    """The terms of the masked, prox-adjusted squared norm (before the sum)."""
    f = dtype
    gj = np.where(m, g.astype(f), f(0)) if mode == 2 else g.astype(f)
    if mu:
        gj = f(MU) * (w.astype(f) - ref.astype(f)) + gj
    return gj * gj


# ------------------------------------------------------------------------------------------------ generator
def _m_rows(C, mu):
    """Exponents m of the rows (t = 4^m): the largest keeps 4^m in lattice units (quarters with prox) below 2^24."""
    top = 10 if mu else 11
    return [top - (C - 1) + c for c in range(C)]


def _place_norm(w, g, ref, m, mode, mu, target, rng, what):
    """Make sum g'^2 of one row exactly ``target`` (a power of 4) by rewriting up to N_SPIKES elements; in place."""
    P = w.shape[0]
    ctrl = np.flatnonzero(m) if mode == 2 else np.arange(P)
    if len(ctrl) == 0:
        raise ValueError("%s: no element whose gradient reaches the norm" % what)
    idx = np.unique(ctrl[np.linspace(0, len(ctrl) - 1, min(N_SPIKES, len(ctrl))).astype(np.int64)])
    w[idx] = ref[idx]
    g[idx] = 0
    t0 = float(sqnorm_terms(w, g, ref, m, mode, mu).sum())
    q = (target - t0) * 4
    if q < 0 or q != int(q):
        raise ValueError("%s: base norm %g above the target %g" % (what, t0, target))
    q, j, spikes = int(q), 0, []
    while q:
        spikes += [j] * (q % 4)
        q //= 4
        j += 1
    if len(spikes) > len(idx):
        raise ValueError("%s: %d spikes needed, %d elements free" % (what, len(spikes), len(idx)))
    order = rng.permutation(len(idx))
    for k, j in enumerate(spikes):
        i = idx[order[k]]
        s = 1 if rng.random() < 0.5 else -1
        if j == 0:
            assert mu, what
            w[i] = ref[i] + s            # g' = mu (w - ref) = +-1/2
        else:
            g[i] = s * 2.0 ** (j - 1)    # g' = g = +-2^(j-1)
    return len(spikes)


def _rows(P, C, mu, big, rng):
    """g, w - ref and buf of C rows.  Non-zero g (and, with prox, w != ref) have density min(1, 4^m0 / (5 P)), m0 the
    smallest exponent of the rows: E[g^2] <= 2 and E[(mu (w - ref))^2] = 1/2 per element, so the expected squared norm
    before the spikes is at most half of the smallest target 4^m0."""
    top0 = _m_rows(C, mu)[0]
    dens = min(1.0, 4.0 ** top0 / (5.0 * P))
    lo = 1 if big else 2
    g = rng.integers(-lo, lo + 1, (C, P)).astype(np.float64) * (rng.random((C, P)) < dens)
    d = rng.integers(-2, 3, (C, P)).astype(np.float64)
    if mu:
        d *= rng.random((C, P)) < dens
    buf = rng.integers(-16, 17, (C, P)).astype(np.float64) / 4
    return g, d, buf


def _finish_norm(c, terms_of, what, shift=1):
    """Shared tail of the generators: assert the sum preconditions, set max_norm = 2^(m_0 - shift) and coef."""
    C = c.w.shape[0]
    units = 4.0 if c.mu else 1.0
    if c.clipped:
        c.m_exp = _m_rows(C, c.mu)
        c.max_norm = 2.0 ** (c.m_exp[0] - shift)
    else:
        c.m_exp, c.max_norm = None, MAX_NORM_OFF
    c.t = np.stack([terms_of(r).sum() for r in range(C)])
    for r in range(C):
        # every term is >= 0 and a multiple of 1 / units, so every partial sum in any order is at most t
        require_fp32_exact(c.t[r] * units, "%s row %d squared norm" % (what, r))
        if c.clipped:
            assert c.t[r] == 4.0 ** c.m_exp[r] and np.sqrt(c.t[r]) >= 32, (what, r, c.t[r])
    c.coef = clip_coef(c.t, c.max_norm)
    c.coef32 = clip_coef(c.t.astype(np.float32), c.max_norm, np.float32)
    if c.clipped:
        assert np.array_equal(c.coef, [c.max_norm / 2.0 ** e for e in c.m_exp]), (what, c.coef)
        assert len(set(c.coef.tolist())) == C
    else:
        assert np.array_equal(c.coef, np.ones(C)), (what, c.coef)
    assert np.array_equal(c.coef32.astype(np.float64), c.coef), what


def _opt_case(cfg, key):
    rng = rng_of("opt", key, cfg)
    P, C = cfg.P, cfg.C
    c = types.SimpleNamespace(cfg=cfg, P=P, C=C, mu=cfg.mu, clipped=cfg.clipped)
    big = P in OPT_P_BIG
    R = 1 if cfg.ref_shared else C
    c.ref = rng.integers(-6, 7, (R, P)).astype(np.float64)
    c.pref = rng.integers(-8, 9, (R, P)).astype(np.float64)
    c.g, d, c.buf = _rows(P, C, cfg.mu, big, rng)
    c.w = np.broadcast_to(c.ref, (C, P)) + d
    if cfg.mode:
        mrows = mask_rows(1 if cfg.shared else C, P, rng)
        c.bits = pack_bits_high(mrows)
        assert np.array_equal(unpack_bits_np(c.bits, P), mrows)
        c.m = np.broadcast_to(mrows, (C, P))
    else:
        c.bits, c.m = None, np.ones((C, P), dtype=bool)
    refb = np.broadcast_to(c.ref, (C, P))
    what = "local_opt %r" % (cfg,)
    if cfg.clipped:
        for r, e in enumerate(_m_rows(C, cfg.mu)):
            _place_norm(c.w[r], c.g[r], refb[r], c.m[r], cfg.mode, cfg.mu, 4.0 ** e, rng, what)
    _finish_norm(c, lambda r: sqnorm_terms(c.w[r], c.g[r], refb[r], c.m[r], cfg.mode, cfg.mu), what)
    assert float(np.abs(c.w).max()) <= 8 and float(np.abs(c.w - refb).max()) <= 2
    trace = []
    c.w1, c.g1, c.buf1 = opt_chain(c.w, c.g, c.buf, refb, np.broadcast_to(c.pref, (C, P)), c.m, c.coef[:, None],
                                   cfg.mode, cfg.mom, cfg.mu, cfg.lamda, trace=trace)
    for i, x in enumerate(trace):
        assert roundtrips(x), "%s: intermediate %d of the chain is not an fp32 value" % (what, i)
    return c


@functools.lru_cache(maxsize=4)
def opt_case(cfg):
    """One lattice case of ``local_opt`` with its fp64 reference (numpy, [C, P]; ref / pref [1 or C, P]; bits int32
    [1 or C, W] torch or None; m bool [C, P]; coef [C]; w1, g1, buf1 the expected rows, buf1 None without momentum).
    Cached: do not modify."""
    return _opt_case(cfg, "flat")


@functools.lru_cache(maxsize=2)
def pack_case(cfg):
    """``opt_case`` on the synthetic pack layout (P of ``pack_layout``)."""
    return _opt_case(cfg._replace(P=pack_layout()[1]), "pack")


@functools.lru_cache(maxsize=4)
def csm_case(cfg):
    """One lattice case of ``clip_sgd_mask``: w, g, buf [C, P], float mask [P] or None, w1 / g1 / buf1 expected, wbf
    the expected bf16 bit patterns (int16 torch [C, P])."""
    rng = rng_of("csm", cfg)
    P, C = cfg.P, cfg.C
    c = types.SimpleNamespace(cfg=cfg, P=P, C=C, mu=False, clipped=cfg.clipped)
    c.g, d, c.buf = _rows(P, C, False, False, rng)
    ref = rng.integers(-6, 7, (C, P)).astype(np.float64)
    c.w = ref + d
    ones = np.ones(P, dtype=bool)
    what = "clip_sgd_mask %r" % (cfg,)
    if cfg.clipped:
        for r, e in enumerate(_m_rows(C, False)):
            _place_norm(c.w[r], c.g[r], ref[r], ones, 0, False, 4.0 ** e, rng, what)
    # the norm of the unmasked gradient; coefficients 2^-5, 2^-6, 2^-7, so the updated weights carry up to 9 fraction
    # bits and 12 significant ones: the bf16 store rounds, ties included
    _finish_norm(c, lambda r: c.g[r] * c.g[r], what, shift=CSM_SHIFT)
    c.mask = mask_rows(1, P, rng)[0].astype(np.float64) if cfg.mask else None
    trace = []
    c.w1, c.g1, c.buf1 = csm_chain(c.w, c.g, c.buf, c.mask, c.coef[:, None], cfg.mom, cfg.first, trace=trace)
    for i, x in enumerate(trace):
        assert roundtrips(x), "%s: intermediate %d of the chain is not an fp32 value" % (what, i)
    c.wbf = torch.from_numpy(c.w1).to(torch.bfloat16).view(torch.int16)
    return c


def bf16_ties(x):
    """Number of entries of an fp64 array of fp32 values that lie exactly half-way between two bf16 values."""
    b = x.astype(np.float32).view(np.uint32)
    return int(((b & 0xffff) == 0x8000).sum())


def bf16_inexact(x):
    return int(((x.astype(np.float32).view(np.uint32) & 0xffff) != 0).sum())


# ------------------------------------------------------------------------------------------------ pack images
def pack_images(w1, layers, slots_of):
    """Expected bf16 images of the updated rows w1 [G, P] (fp64): per layer the forward image [G, Cout, kt, Cin_p] (zero
    in the padded channels) and the data-gradient image [G, Cin_p, slot(t), Cout], from the reference alone."""
    G = w1.shape[0]
    out = []
    for li, (off, cout, cin, k) in enumerate(layers):
        kt, cin_p = k * k, (cin + 63) // 64 * 64
        w = torch.from_numpy(np.ascontiguousarray(w1[:, off:off + cout * cin * kt])).view(G, cout, cin, kt)
        fwd = torch.zeros(G, cout, kt, cin_p, dtype=torch.float64)
        fwd[..., :cin] = w.permute(0, 1, 3, 2)
        fwd = fwd.to(torch.bfloat16)
        slots = list(slots_of(li))
        tr = torch.empty(G, cin_p, kt, cout, dtype=torch.bfloat16)
        for t in range(kt):
            tr[:, :, slots[t], :] = fwd[:, :, t, :].transpose(1, 2)
        out.append((fwd, tr))
    return out


# ------------------------------------------------------------------------------------------------ non-dyadic coefficient
# Roundings of t = sum g^2 as the kernels form it, counted as the largest number of fp32 roundings any one term passes
# through (all terms are >= 0, so the relative error of the sum is at most that count times u = 2^-24, to first order):
#   the square 1, the 4-term expression 3, the thread's accumulator 9 (chunk / 1024 = 8 trips, 9 with the rescaled
#   chunk 8196), block_sum 6 (wave shuffles) + 4 (waves) = 10, the partial re-reduction loop 4 (nblk <= 1024 over 256
#   threads), its block_sum 10                                                                       -> 37 u on t
# sqrtf halves it (18.5 u) and adds 1 u if correctly rounded, plus one extra ulp (2 u) as that is not assumed: 21.5 u;
# + 1e-6f: 1 u; the division 1 u plus one extra ulp (2 u): 25.5 u; the minimum is exact.
K_COEF = 26
K_GRAD = K_COEF + 1                    # g * coef: one more rounding
COEF_P = (8197, 2105345)
COEF_SCALES = (0.5, 3.0, 1.25)
COEF_MAX_NORM = 10.0


@functools.lru_cache(maxsize=2)
def coef_case(P):
    """Random normal gradients (rows at different scales, all clipped at max_norm 10): fp32 operands w, g [C, P] (torch)
    and the fp64 coefficient / clipped gradient with their a-priori bounds K 2^-24 |ref|."""
    g_ = torch.Generator().manual_seed(zlib.crc32(repr(("coef", P)).encode()))
    C = len(COEF_SCALES)
    c = types.SimpleNamespace(P=P, C=C)
    c.g = torch.randn(C, P, generator=g_) * torch.tensor(COEF_SCALES).view(C, 1)
    c.w = torch.randn(C, P, generator=g_)
    t = (c.g.double() ** 2).sum(1)
    c.coef = COEF_MAX_NORM / (t.sqrt() + EPS32)
    assert bool((c.coef < 0.5).all())
    c.g1 = c.g.double() * c.coef.view(C, 1)
    c.coef_bound = K_COEF * 2.0 ** -24 * c.coef.abs()
    c.g1_bound = K_GRAD * 2.0 ** -24 * c.g1.abs()
    return c


def sum_order_kernel(sq, reverse=False):
    """fp32 sum of the squares sq [P] (fp32 numpy) in the kernels' order: per block a thread-strided accumulation of
    4-element groups, a tree over the threads, then a strided sum of the block partials and a tree."""
    P = sq.shape[0]
    if reverse:
        sq = sq[::-1]
    chunk, nb = opt_chunk(P)
    x = np.zeros(nb * chunk, dtype=np.float32)
    x[:P] = sq
    trips = -(-chunk // (4 * OPT_THREADS))
    blk = np.zeros((nb, trips * 4 * OPT_THREADS), dtype=np.float32)
    blk[:, :chunk] = x.reshape(nb, chunk)
    q = blk.reshape(nb, trips, OPT_THREADS, 4)
    acc = np.zeros((nb, OPT_THREADS), dtype=np.float32)
    for t in range(trips):
        acc = acc + (((q[:, t, :, 0] + q[:, t, :, 1]) + q[:, t, :, 2]) + q[:, t, :, 3])
    part = _tree32(acc)
    lanes = np.zeros(-(-nb // OPT_THREADS) * OPT_THREADS, dtype=np.float32)
    lanes[:nb] = part
    lanes = lanes.reshape(-1, OPT_THREADS)
    acc = np.zeros(OPT_THREADS, dtype=np.float32)
    for t in range(lanes.shape[0]):
        acc = acc + lanes[t]
    return float(_tree32(acc[None])[0])


def _tree32(x):
    """Pairwise fp32 tree over the last axis (a power of two long)."""
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def sum_order_pairwise(sq):
    n = 1 << int(np.ceil(np.log2(max(2, sq.shape[0]))))
    x = np.zeros(n, dtype=np.float32)
    x[:sq.shape[0]] = sq
    return float(_tree32(x[None])[0])


# ------------------------------------------------------------------------------------------------ selection
# Domain: finite non-negative fp32 including +0.0 and denormals, and +inf (what saliency_acc and the score
# normalisation can produce).  Negative values and NaN are out of scope: the radix select orders bit patterns as
# unsigned integers, which is the float order only for non-negative values.
SELECT_N = (1, 2, 255, 256, 257, 4099, 524289)       # the last: one past 2048 blocks x 256 (the grid-stride loop)
SELECT_SETS = ("all_equal", "five_ties", "low_byte", "top_byte", "zero_digit_0", "zero_digit_1", "zero_digit_2",
               "zero_digit_3", "denormals", "with_inf")
INF_BITS = 0x7f800000


def _zero_digit_values(j):
    """Bit patterns around a value whose byte j is zero: the same prefix with digit 0, 1, 2 at byte j, each with two
    settings of the byte below (bit 1 of it clear or set; none below byte 0), and one more digit-0 value just under
    the base, so the pass over byte j ends its scan at digit 0 when the threshold is one of the digit-0 values."""
    base = 0x3f810101 & ~(0xff << (8 * j))
    low = [0] if j == 0 else [0, 2 << (8 * (j - 1))]
    return [base | (dgt << (8 * j)) | lo for dgt in (0, 1, 2) for lo in low] + [base - 1 if j == 0 else base ^ 0x1]


def select_values(name):
    if name == "all_equal":
        return [0x3f800000]
    if name == "five_ties":
        return [0x00000000, 0x3a83126f, 0x3f000000, 0x3f800000, 0x41200000]
    if name == "low_byte":
        return [0x3f800000 | b for b in range(256)]
    if name == "top_byte":
        return [b << 24 for b in range(0x80)]             # 0x00000000 (+0.0) ... 0x7f000000
    if name.startswith("zero_digit_"):
        return _zero_digit_values(int(name[-1]))
    if name == "denormals":
        return [0x00000000, 0x00000001, 0x00000002, 0x00000100, 0x00010000, 0x007fffff, 0x00800000]
    if name == "with_inf":
        return [0x00000000, 0x3f800000, 0x7f7fffff, INF_BITS]
    raise KeyError(name)


@functools.lru_cache(maxsize=8)
def select_data(name, n):
    """uint32 bit patterns [n] (numpy) of the data set: every value of the set occurs when n allows, in random order
    with random multiplicities (long ties for the small sets)."""
    vals = np.array(sorted(set(select_values(name))), dtype=np.uint32)
    assert int(vals.max()) <= INF_BITS
    rng = rng_of("select", name, n)
    if name == "with_inf" and n > 4:       # a few +inf, not a quarter of the data
        p = np.array([0.3, 0.4, 0.3 - 3.0 / n, 3.0 / n])
        out = rng.choice(vals, size=n, p=p)
    else:
        out = rng.choice(vals, size=n)
    k = min(n, len(vals))
    out[rng.permutation(n)[:k]] = rng.permutation(vals)[:k]
    return out


def select_ranks(bits):
    """k in {1, 2, n/2, n - 1, n} and every rank (1-based, counted from the largest) at which a tie group starts or
    ends."""
    n = bits.shape[0]
    ks = {1, 2, n // 2, n - 1, n}
    _, counts = np.unique(bits, return_counts=True)
    end = np.cumsum(counts[::-1])                         # last rank of each group, from the largest value
    ks |= set(end.tolist()) | set((end - counts[::-1] + 1).tolist())
    return sorted(k for k in ks if 1 <= k <= n)


def kth_largest_bits(bits, k):
    return int(np.sort(bits)[bits.shape[0] - k])


# ------------------------------------------------------------------------------------------------ row kernels
ROW_N = (1, 3, 4, 5, 1023, 1024, 1027, 4099)              # one block covers 1024 elements
SQDIST_N = ROW_N + (16384, 16385, 32773, 4194309)         # the last: one past the 256-block cap
ROW_WEIGHTS = (0.5, -0.25, 1.5, 2.0, -1.0)                # dyadic


def int_rows(R, n, lo, hi, *key):
    """Integers in [lo, hi] as fp64 numpy [R, n]."""
    return rng_of("rows", R, n, lo, hi, key).integers(lo, hi + 1, (R, n)).astype(np.float64)


def pair_sqdist_chunks(n):
    """(blocks, chunk) of ``pair_sqdist`` (sparse.hip)."""
    nblk = min(256, max(1, (n + 16383) // 16384))
    return nblk, (((n + nblk - 1) // nblk) + 3) & ~3


# ------------------------------------------------------------------------------------------------ comparisons
def assert_bits(got, ref, names):
    """Integer tensors (bit patterns) equal; a failure names the first index by axes."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.numel() == ref.numel(), "shape: got %s, reference %s" % (tuple(got.shape), tuple(ref.shape))
    got = got.reshape(ref.shape)
    if torch.equal(got, ref):
        return
    bad = torch.nonzero(got != ref)
    i = tuple(int(v) for v in bad[0])
    raise AssertionError("%d of %d bit patterns differ; first at (%s): got 0x%x, reference 0x%x"
                         % (len(bad), ref.numel(), ", ".join("%s=%d" % p for p in zip(names, i)),
                            int(got[i]) & 0xffffffff, int(ref[i]) & 0xffffffff))


def relerr(a, b):
    """The whole-tensor relative norm of the older optimizer tests."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-30))
