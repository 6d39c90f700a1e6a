"""Krum, Multi-Krum, coordinate median and trimmed mean over the client rows (``csrc/kernels/robust.hip``).

Three primitives read an fp32 row matrix in place through a list ``ridx`` of row numbers (the list is the client
order; rows that are not listed and columns past ``n`` are never touched):

* :func:`order_mean` — per column, the mean of the order statistics ``lo .. hi-1`` of the listed rows (median:
  ``lo = (K-1)//2, hi = K//2 + 1``; trimmed mean: ``lo = b, hi = K - b``): a sequential fp32 sum in ascending rank and
  one fp32 division;
* :func:`pair_sqdist` — ``D[i][k] (+)= sum_j ((double)(a_i[j] - a_k[j]))^2``: an fp32 difference, an exact fp64 square
  and fp64 sums (the Gram form ``d_i + d_k - 2 g_ik`` cancels once the clients differ by less than their norm);
* :func:`krum_select` — Krum scores (the ``m = max(1, K - f - 2)`` smallest distances of a row, added ascending in
  fp64) and the ``multi`` clients with the smallest scores.

One total order serves all of them, "a before b": ``a < b``; or b is NaN and a is not; or neither (equal values,
``-0 == +0``, both NaN) and a comes first in the client order.  So a column that holds fewer than half NaNs still has
a finite median, an Inf or NaN row is never selected by Krum while enough finite rows exist, and ties break the same
way on every rank.  (``core/robustness.py``, the eager CPU path, keeps torch's behaviour: ``torch.median`` returns NaN
for a column with one NaN, ``topk`` ties are unspecified.)

:func:`aggregate` drives them over column chunks, so no ``K x (P + Q)`` matrix is ever gathered.  CUDA rows take the
HIP kernels; the torch / numpy twins here follow the kernels' operation order.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..parallel import runtime as rt

KINDS = ("krum", "multikrum", "median", "trimmed_mean")
MAX_K = 256


def _use_hip(mat, hip):
    """Whether the HIP kernels run: ``hip`` None = whenever the operand allows it; True = they must (a layout the
    kernels cannot take is an error, never a silent torch run); False = the twins."""
    ok = (mat.device.type == "cuda" and mat.dtype == torch.float32 and mat.dim() == 2 and mat.stride(1) == 1
          and mat.stride(0) % 4 == 0 and mat.data_ptr() % 16 == 0)
    if hip and not ok:
        raise ValueError("robust kernels need 16-byte aligned fp32 CUDA rows (unit column stride, row stride % 4 == 0)")
    return ok if hip is None else bool(hip)


def _to_dev(values, dtype, device):
    """Small host list -> device tensor through pinned memory: the host does not wait for the queued GPU work."""
    t = torch.tensor([int(v) for v in values], dtype=dtype)
    return t.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else t


def _ridx(ridx, device):
    if torch.is_tensor(ridx):
        assert ridx.dtype == torch.int32 and ridx.is_contiguous() and ridx.device == device
        return ridx
    return _to_dev(ridx, torch.int32, device)


def median_range(K):
    return (K - 1) // 2, K // 2 + 1


def trim_range(K, trim_ratio):
    b = int(K * trim_ratio)
    return b, K - b


# ------------------------------------------------------------------------------------------------ order statistics
def order_mean_twin(M, lo, hi):
    """``[n]`` fp32 from ``M`` ``[K, n]`` (rows in client order): stable sort (NaN last, ties by row), sequential
    fp32 sum of the sorted rows ``lo .. hi-1``, one fp32 division."""
    S = torch.sort(M.float(), dim=0, stable=True).values
    acc = S[lo].clone()
    for r in range(lo + 1, hi):
        acc = acc + S[r]
    return acc / torch.full((1,), float(hi - lo), dtype=torch.float32, device=M.device)


def order_mean(mat, ridx, n, lo, hi, out, hip=None):
    """``out[:n]`` = mean of the order statistics ``lo .. hi-1`` of ``mat[ridx, :n]`` per column.  Nothing past
    ``out[n]`` is written."""
    ridx = _ridx(ridx, mat.device)
    K = ridx.numel()
    if not (1 <= K <= MAX_K and 0 <= lo < hi <= K):
        raise ValueError("order_mean: 1 <= K <= %d and 0 <= lo < hi <= K (K=%d lo=%d hi=%d)" % (MAX_K, K, lo, hi))
    if n == 0:
        return out
    if _use_hip(mat, hip):
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n and out.device == mat.device
        ops.ext().rows_order_mean(mat.data_ptr(), mat.stride(0), ridx.data_ptr(), K, n, lo, hi, out.data_ptr(),
                                  ops.stream())
        return out
    out[:n] = order_mean_twin(mat.index_select(0, ridx.long())[:, :n], lo, hi)
    return out


# ------------------------------------------------------------------------------------------------ Krum
def pair_sqdist_twin(M):
    """``[K, K]`` fp64: sums of the squared fp32 differences of the rows of ``M`` ``[K, n]``; the diagonal is 0."""
    M = M.float()
    K = M.shape[0]
    D = torch.zeros((K, K), dtype=torch.float64, device=M.device)
    for i in range(K):  # one row against all: [K, n] temporaries only
        d = (M[i:i + 1] - M).double()
        D[i] = (d * d).sum(1)
        D[i, i] = 0.0
    return D


def pair_sqdist(mat, ridx, n, D=None, accumulate=False, hip=None):
    """``D`` ``[K, K]`` fp64 (+)= the pairwise squared distances of ``mat[ridx, :n]``."""
    ridx = _ridx(ridx, mat.device)
    K = ridx.numel()
    if not 1 <= K <= MAX_K:
        raise ValueError("pair_sqdist: 1 <= K <= %d (K=%d)" % (MAX_K, K))
    if D is None:
        assert not accumulate
        D = torch.empty((K, K), dtype=torch.float64, device=mat.device)
    assert D.dtype == torch.float64 and D.is_contiguous() and D.shape == (K, K) and D.device == mat.device
    if _use_hip(mat, hip):
        m = ops.ext()
        part = torch.empty(m.rows_pair_sqdist_workspace(K, n), dtype=torch.float64, device=mat.device)
        m.rows_pair_sqdist(mat.data_ptr(), mat.stride(0), ridx.data_ptr(), K, n, part.data_ptr(), D.data_ptr(),
                           1 if accumulate else 0, ops.stream())
        return D
    T = pair_sqdist_twin(mat.index_select(0, ridx.long())[:, :n])
    if accumulate:
        D += T
    else:
        D.copy_(T)
    return D


def krum_select_twin(D, f, multi):
    """(sel ``[multi]`` int64, score ``[K]`` fp64) from ``D`` ``[K, K]``: numpy, in the kernel's order (stable sorts
    put NaN last and break ties by index; sequential fp64 sums)."""
    Dn = np.asarray(D.detach().cpu().numpy() if torch.is_tensor(D) else D, dtype=np.float64)
    K = Dn.shape[0]
    m = min(max(1, K - f - 2), K - 1)
    score = np.zeros(K, dtype=np.float64)
    for i in range(K):
        v = np.delete(Dn[i], i)
        v = v[np.argsort(v, kind="stable")]
        t = np.float64(0.0)
        for r in range(m):
            t = t + v[r]
        score[i] = t
    sel = np.argsort(score, kind="stable")[:multi]
    return sel.astype(np.int64), score


def krum_select(D, f, multi, hip=None):
    """(sel ``[multi]`` int32, score ``[K]`` fp64) on ``D``'s device."""
    K = D.shape[0]
    if not (1 <= K <= MAX_K and f >= 0 and 1 <= multi <= K):
        raise ValueError("krum_select: 1 <= K <= %d, f >= 0, 1 <= multi <= K (K=%d f=%d multi=%d)"
                         % (MAX_K, K, f, multi))
    use = D.device.type == "cuda" if hip is None else bool(hip)
    if use:
        if not (D.device.type == "cuda" and D.dtype == torch.float64 and D.is_contiguous()):
            raise ValueError("krum_select kernel needs a contiguous fp64 CUDA matrix")
        sel = torch.empty(multi, dtype=torch.int32, device=D.device)
        score = torch.empty(K, dtype=torch.float64, device=D.device)
        ops.ext().krum_select(D.data_ptr(), K, int(f), int(multi), sel.data_ptr(), score.data_ptr(), ops.stream())
        return sel, score
    sel, score = krum_select_twin(D, f, multi)
    return torch.from_numpy(sel).to(torch.int32).to(D.device), torch.from_numpy(score).to(D.device)


# ------------------------------------------------------------------------------------------------ driver
def column_chunks(K, ncols, budget=2e9):
    """[(first column, width)]: chunks of a ``K``-row section whose gathered copy stays under ``budget`` bytes.  A
    function of (K, ncols, budget) only - never of the world size - so results do not depend on the sharding.  Widths
    are multiples of 64 columns (16-B aligned chunk starts) but for the last."""
    w = max(64, int(budget // (4 * max(1, K))) // 64 * 64)
    return [(c0, min(w, ncols - c0)) for c0 in range(0, ncols, w)]


def _runs(rows):
    """Maximal runs of consecutive integers of the ascending list ``rows``: [(first, length)]."""
    runs = []
    for r in rows:
        if runs and runs[-1][0] + runs[-1][1] == r:
            runs[-1][1] += 1
        else:
            runs.append([r, 1])
    return [(a, b) for a, b in runs]


def aggregate(kind, theta, bufs, P, Q, local_rows, local_clients, sampled, owner, info, out_w, out_b, f=0, multi=1,
              trim_ratio=0.1, budget=2e9, hip=None):
    """Robust aggregate of the sampled clients' (params, buffers) into ``out_w`` ``[P]`` / ``out_b`` ``[Q]``.

    ``theta`` / ``bufs``: this rank's row matrices; ``local_rows`` / ``local_clients``: the rows of the sampled
    clients that live here and their global ids; ``owner[c]``: the rank that holds client c.  The client order is the
    ascending client id on every rank.

    One process reads the rows in place (``ridx`` = the rows in client order; no gather, no copy).  Several ranks
    gather, per column chunk, that chunk of their sampled rows (sizes known on every rank: no size exchange) and run
    the same kernel with ``ridx`` = the client-id permutation of the gathered rows.  Median / trimmed mean write each
    result chunk; Krum accumulates ``D`` over the parameter and buffer chunks in chunk order, selects, and forms the
    mean of the selected rows as a weighted row sum of the local rows (weight ``1 / multi``, in row order) plus one
    all-reduce: plain Krum is an exact copy of the selected row.  Returns ``{"sel": selected client ids or None}``."""
    if kind not in KINDS:
        raise ValueError("unknown aggregator %r" % (kind,))
    order = sorted(int(c) for c in sampled)
    K = len(order)
    if not 1 <= K <= MAX_K:
        raise ValueError("robust aggregation takes 1 .. %d sampled clients (got %d)" % (MAX_K, K))
    dev = theta.device
    world = info.world if info.enabled else 1
    row_of = {int(c): int(r) for r, c in zip(local_rows, local_clients)}
    rows = sorted(row_of.values())
    if world == 1:
        ridx = _ridx([row_of[c] for c in order], dev)
        rows_t = None
    else:
        cnt = [sum(1 for c in order if int(owner[c]) == r) for r in range(world)]
        by_row = sorted(row_of, key=lambda c: row_of[c])  # this rank's clients in the order its rows are gathered
        ids = rt.all_gather_sized(_to_dev(by_row, torch.int32, dev), cnt, info)
        ridx = torch.argsort(ids).to(torch.int32).contiguous()
        rows_t = None if (not rows or rows[-1] - rows[0] + 1 == len(rows)) else _to_dev(rows, torch.int64, dev)

    def chunk_of(src, c0, w):
        """(matrix, ridx rows are numbers of) for the columns [c0, c0 + w) of a section."""
        if world == 1:
            return src[:, c0:]
        w4 = (w + 3) // 4 * 4
        piece = torch.zeros((len(rows), w4), dtype=torch.float32, device=dev)
        if rows:
            piece[:, :w] = (src[rows[0]:rows[-1] + 1, c0:c0 + w] if rows_t is None
                            else src[:, c0:c0 + w].index_select(0, rows_t))
        return rt.all_gather_sized(piece.view(-1), [n * w4 for n in cnt], info).view(K, w4)

    krum = kind in ("krum", "multikrum")
    if krum:
        D = torch.zeros((K, K), dtype=torch.float64, device=dev)
        first = True
    else:
        lo, hi = median_range(K) if kind == "median" else trim_range(K, trim_ratio)
    for src, ncols, out in ((theta, P, out_w), (bufs, Q, out_b)):
        for c0, w in column_chunks(K, ncols, budget):
            mat = chunk_of(src, c0, w)
            if krum:
                pair_sqdist(mat, ridx, w, D, accumulate=not first, hip=hip)
                first = False
            else:
                order_mean(mat, ridx, w, lo, hi, out[c0:c0 + w], hip=hip)
    if not krum:
        return {"sel": None}
    multi = 1 if kind == "krum" else max(1, min(int(multi), K))
    sel, _ = krum_select(D, f, multi, hip=None if hip is None else bool(hip) and dev.type == "cuda")
    chosen = sorted(order[i] for i in sel.tolist())  # K small integers: the round's one read-back
    mine = sorted(row_of[c] for c in chosen if c in row_of)
    Pp = (P + 63) // 64 * 64  # keeps the buffer section 16-B aligned
    buf = torch.zeros(Pp + Q, dtype=torch.float32, device=dev)
    wt = torch.full((max(1, len(mine)),), 1.0 / multi, dtype=torch.float32, device=dev)
    if mine and _use_hip(theta, hip) and (not Q or _use_hip(bufs, hip)):
        m, st = ops.ext(), ops.stream()
        for j, (r0, cnt_r) in enumerate(_runs(mine)):  # skipped rows are never read: a NaN row cannot leak in
            beta = 0.0 if j == 0 else 1.0
            m.weighted_rows_sum(theta[r0].data_ptr(), wt.data_ptr(), cnt_r, P, theta.stride(0), beta, buf.data_ptr(),
                                st)
            if Q:
                m.weighted_rows_sum(bufs[r0].data_ptr(), wt.data_ptr(), cnt_r, Q, bufs.stride(0), beta,
                                    buf[Pp:].data_ptr(), st)
    else:
        for r in mine:
            buf[:P] = buf[:P] + wt[:1] * theta[r, :P]
            buf[Pp:] = buf[Pp:] + wt[:1] * bufs[r, :Q]
    rt.all_reduce_buckets(buf, info)
    out_w.copy_(buf[:P])
    out_b.copy_(buf[Pp:])
    return {"sel": chosen}
