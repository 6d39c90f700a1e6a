"""Secure aggregation of the client rows: masked FedAvg over Z_p, p = 2^31 - 1 (``csrc/kernels/secagg.hip``).

The protocol (one definition for the kernels, the numpy twins here and the host trainer
``algorithms/turboaggregate.py`` ``TurboAggregateTrainer(prg="counter")``):

* client i of the round's K participants quantises its weighted row, ``q = rint((double(theta) * w_i) * S)`` with
  ``w_i = n_i / n_tot``, ``|q|`` saturated at ``B = ((p - 1) / 2) // K`` and non-finite values sent as 0 (both
  counted), and adds one mask per peer: ``+m`` towards a higher client id, ``p - m`` towards a lower one, with
  ``m = counter_mask(key_ij, round, segment, coordinate)`` and ``key_ij`` the pair's agreed key;
* the server sums the uploads mod p - the masks of two survivors cancel - reconstructs the secret key of every client
  that dropped after the key setup from the survivors' BGW shares (host scalars), removes the survivors' masks towards
  it, centres the residues and returns ``float32(double(c) / S / a)``, ``a`` = the survivors' share of the weights.

Three primitives read an fp32 row matrix in place through a list ``ridx`` of row numbers (rows that are not listed and
columns past ``n`` are never touched): :func:`upload` (the masked rows, what each client would send),
:func:`masked_sum` (their column sum mod p without materialising them: only the masks that do not cancel inside the
call are generated) and :func:`finish`.  Everything is integer arithmetic, so the aggregate is the same bits for any
sharding of the clients.  Masked rows are int32 tensors holding the residues in [0, p) (p < 2^31).

This simulates the protocol's data flow and cost with a statistical PRG, as the reference does; it makes no
cryptographic strength claim.  CUDA rows take the HIP kernels; the numpy twins follow the kernels' arithmetic.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..algorithms.turboaggregate import (P_DEFAULT, TurboAggregateTrainer, my_key_agreement, quantize_bounded,
                                         saturation_bound)
from ..parallel import runtime as rt
from .masks import _mix_hash_np, counter_mask, mod_mersenne31

SEG_PARAMS, SEG_BUFS = 0, 1
P_FIELD = P_DEFAULT


def _use_hip(mat, hip):
    """Whether the HIP kernels run: ``hip`` None = whenever the operand allows it; True = they must (a layout the
    kernels cannot take is an error, never a silent numpy run); False = the twins."""
    ok = (mat.device.type == "cuda" and mat.dtype == torch.float32 and mat.dim() == 2 and mat.stride(1) == 1
          and mat.stride(0) % 4 == 0 and mat.data_ptr() % 16 == 0)
    if hip and not ok:
        raise ValueError("secagg kernels need 16-byte aligned fp32 CUDA rows (unit column stride, row stride % 4 == 0)")
    return ok if hip is None else bool(hip)


def _to_dev(values, dtype, device):
    """Small host array -> device tensor through pinned memory: the host does not wait for the queued GPU work."""
    t = torch.as_tensor(np.asarray(values), dtype=dtype)
    return t.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else t


def pack_peers(peers):
    """Per-row peer lists ``[[(client id, key), ...], ...]`` -> (offsets ``[C + 1]``, ids, keys) int32 arrays."""
    off = np.zeros(len(peers) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(p) for p in peers])
    flat = [e for p in peers for e in p]
    ids = np.array([int(e[0]) for e in flat], dtype=np.int32)
    keys = np.array([int(e[1]) for e in flat], dtype=np.int32)
    assert all(0 <= int(e[1]) < P_FIELD for e in flat)
    return off, ids, keys


def _check(round_idx, seg, scale, B):
    if not (0 <= int(round_idx) < 2 ** 32 and seg in (SEG_PARAMS, SEG_BUFS) and scale >= 1 and 1 <= B < 2 ** 30):
        raise ValueError("secagg: 0 <= round < 2^32, seg 0 | 1, scale >= 1, 1 <= B < 2^30 (round=%s seg=%s scale=%s "
                         "B=%s)" % (round_idx, seg, scale, B))


def _check_rows(mat, ridx, n):
    if not (1 <= n <= mat.shape[1] and len(ridx) >= 1 and all(0 <= int(r) < mat.shape[0] for r in ridx)):
        raise ValueError("secagg: rows %s / %d columns outside the %s matrix" % (list(ridx), n, tuple(mat.shape)))


# ------------------------------------------------------------------------------------------------ numpy twins
def upload_twin(M, cids, peers, wts, round_idx, seg, scale, B):
    """(masked rows int64 ``[C, n]`` in [0, p), events) from the rows ``M`` ``[C, n]`` fp32."""
    M = np.asarray(M, dtype=np.float32)
    C, n = M.shape
    j = np.arange(n, dtype=np.uint64)
    out = np.zeros((C, n), dtype=np.int64)
    events = 0
    for c in range(C):
        y, ev = quantize_bounded(M[c], wts[c], scale, B, P_FIELD)
        events += ev
        for pid, key in peers[c]:
            m = counter_mask(key, round_idx, seg, j)
            y = (y + (m if int(pid) > int(cids[c]) else P_FIELD - m)) % P_FIELD
        out[c] = y
    return out, events


def masked_sum_twin(M, cids, peers, wts, round_idx, seg, scale, B):
    """(column sum of :func:`upload_twin` mod p, int64 ``[n]``; events), one row at a time."""
    M = np.asarray(M, dtype=np.float32)
    acc = np.zeros(M.shape[1], dtype=np.int64)
    events = 0
    for c in range(M.shape[0]):
        y, ev = upload_twin(M[c:c + 1], cids[c:c + 1], peers[c:c + 1], wts[c:c + 1], round_idx, seg, scale, B)
        acc = (acc + y[0]) % P_FIELD
        events += ev
    return acc, events


def finish_twin(total, pairs, round_idx, seg, scale, a):
    """fp32 ``[n]`` from the reduced sums ``total`` (int64, read as unsigned 64-bit values as the kernel does) and the
    ``(survivor, dropped, key)`` pairs."""
    s = mod_mersenne31(np.ascontiguousarray(total, dtype=np.int64).view(np.uint64)).astype(np.int64)
    j = np.arange(s.size, dtype=np.uint64)
    for sid, did, key in pairs:
        m = counter_mask(key, round_idx, seg, j)
        added = m if int(sid) < int(did) else P_FIELD - m
        s = (s - added) % P_FIELD
    c = np.where(s > P_FIELD // 2, s - P_FIELD, s)
    return ((c.astype(np.float64) / float(scale)) / float(a)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ primitives
def _row_args(mat, ridx, cids, peers, wts):
    dev = mat.device
    off, ids, keys = pack_peers(peers)
    pad = (lambda x: x if x.size else np.zeros(1, dtype=np.int32))  # an empty list still gets a valid pointer
    return (_to_dev(ridx, torch.int32, dev), _to_dev(cids, torch.int32, dev), _to_dev(wts, torch.float64, dev),
            _to_dev(off, torch.int32, dev), _to_dev(pad(ids), torch.int32, dev), _to_dev(pad(keys), torch.int32, dev))


def _gather_np(mat, ridx, n):
    return mat.index_select(0, torch.as_tensor(list(ridx), dtype=torch.long, device=mat.device))[:, :n].cpu().numpy()


def upload(mat, ridx, n, cids, peers, wts, round_idx, seg, scale, B, out=None, hip=None):
    """(masked rows int32 ``[C, n]``, events int64 scalar tensor) of ``mat[ridx, :n]``: ``cids`` the rows' client
    ids, ``peers[c]`` = ``[(client id, key), ...]`` and ``wts`` the fp64 weights.  ``out``: a contiguous int32 tensor
    of at least ``C * n`` words to write the rows to (nothing past them is written)."""
    _check(round_idx, seg, scale, B)
    _check_rows(mat, ridx, n)
    C = len(ridx)
    assert C >= 1 and n >= 1 and len(cids) == C and len(peers) == C and len(wts) == C
    if out is not None:
        assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= C * n and out.device == mat.device
        out = out.view(-1)[:C * n].view(C, n)
    if _use_hip(mat, hip):
        m = ops.ext()
        a = _row_args(mat, ridx, cids, peers, wts)
        out = torch.empty((C, n), dtype=torch.int32, device=mat.device) if out is None else out
        cnt = torch.empty(C * m.secagg_blocks(n), dtype=torch.int32, device=mat.device)
        m.secagg_upload(mat.data_ptr(), mat.stride(0), *[t.data_ptr() for t in a], C, n, int(round_idx), int(seg),
                        float(scale), float(B), out.data_ptr(), cnt.data_ptr(), ops.stream())
        return out, cnt.sum(dtype=torch.int64)
    y, ev = upload_twin(_gather_np(mat, ridx, n), list(cids), peers, list(wts), round_idx, seg, scale, B)
    y = torch.from_numpy(y.astype(np.int32)).to(mat.device)
    if out is not None:
        out.copy_(y)
    return (y if out is None else out), torch.tensor(ev, dtype=torch.int64, device=mat.device)


def masked_sum(mat, ridx, n, cids, peers, wts, round_idx, seg, scale, B, out, hip=None):
    """``out[:n]`` (int64) = the column sum mod p of :func:`upload`'s rows; returns the events (int64 scalar tensor).
    Nothing past ``out[n]`` is written."""
    _check(round_idx, seg, scale, B)
    _check_rows(mat, ridx, n)
    C = len(ridx)
    assert C >= 1 and n >= 1 and len(cids) == C and len(peers) == C and len(wts) == C
    assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() >= n and out.device == mat.device
    if _use_hip(mat, hip):
        m = ops.ext()
        if out.data_ptr() % 16:
            raise ValueError("secagg_masked_sum needs a 16-byte aligned int64 output")
        a = _row_args(mat, ridx, cids, peers, wts)
        cnt = torch.empty(m.secagg_blocks(n), dtype=torch.int32, device=mat.device)
        m.secagg_masked_sum(mat.data_ptr(), mat.stride(0), *[t.data_ptr() for t in a], C, n, int(round_idx), int(seg),
                            float(scale), float(B), out.data_ptr(), cnt.data_ptr(), ops.stream())
        return cnt.sum(dtype=torch.int64)
    y, ev = masked_sum_twin(_gather_np(mat, ridx, n), list(cids), peers, list(wts), round_idx, seg, scale, B)
    out[:n] = torch.from_numpy(y).to(out.device)
    return torch.tensor(ev, dtype=torch.int64, device=mat.device)


def finish(total, n, pairs, round_idx, seg, scale, a, out, hip=None):
    """``out[:n]`` (fp32) from the reduced int64 sums ``total[:n]`` and the ``(survivor id, dropped id, key)`` pairs;
    ``a`` = the survivors' share of the weights.  Nothing past ``out[n]`` is written."""
    _check(round_idx, seg, scale, 1)
    assert total.dtype == torch.int64 and total.is_contiguous() and total.numel() >= n and n >= 1
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n and out.device == total.device
    if not 0.0 < a <= 1.0:
        raise ValueError("secagg finish: the survivors' weight share must lie in (0, 1] (got %r)" % (a,))
    use = total.device.type == "cuda" if hip is None else bool(hip)
    if use:
        if total.device.type != "cuda":
            raise ValueError("secagg_finish kernel needs CUDA tensors")
        dev = total.device
        z = np.zeros(1, dtype=np.int32)
        cols = [np.array([int(p[k]) for p in pairs], dtype=np.int32) if pairs else z for k in range(3)]
        sid, did, key = (_to_dev(c, torch.int32, dev) for c in cols)
        ops.ext().secagg_finish(total.data_ptr(), n, sid.data_ptr(), did.data_ptr(), key.data_ptr(), len(pairs),
                                int(round_idx), int(seg), float(scale), float(a), out.data_ptr(), ops.stream())
        return out
    out[:n] = torch.from_numpy(finish_twin(total[:n].cpu().numpy(), pairs, round_idx, seg, scale, a)).to(out.device)
    return out


# ------------------------------------------------------------------------------------------------ keys and dropouts
class SecAggKeys:
    """Key setup of a federation of ``n`` clients: secret / public keys, every pair's agreed key and the BGW shares
    of the secret keys (threshold ``T``) - the state of a ``TurboAggregateTrainer(prg="counter")``, so the eager
    path and the executor agree on every key for the same (n, T, seed)."""

    def __init__(self, n, threshold, seed=0, scale=2 ** 16):
        if not 1 <= int(threshold) < n:
            raise ValueError("secure aggregation needs 1 <= threshold < clients (threshold=%s, clients=%s)"
                             % (threshold, n))
        self.trainer = TurboAggregateTrainer(n, scale=scale, threshold=int(threshold), seed=int(seed) % (2 ** 32),
                                             prg="counter")
        self.n, self.T = n, int(threshold)
        t = self.trainer
        self.key = np.array([[t.pair_key(i, j) if i != j else 0 for j in range(n)] for i in range(n)], dtype=np.int64)

    def reconstruct(self, dropped, alive):
        """{dropped client: its secret key} from the shares of the first T + 1 ``alive`` clients (more than T must
        have survived)."""
        alive = sorted(int(c) for c in alive)
        if len(alive) <= self.T:
            raise ValueError("secure aggregation: %d survivors cannot reconstruct keys shared with threshold %d"
                             % (len(alive), self.T))
        return self.trainer.reconstruct_sks(dropped, alive)

    def removal_pairs(self, dropped, alive):
        """``[(survivor, dropped, key)]``: the masks the server has to take out, keys from the reconstructed secrets."""
        t = self.trainer
        sk = self.reconstruct(dropped, alive) if len(dropped) else {}
        return [(int(i), int(k), my_key_agreement(sk[int(k)], t.pk[int(i)], t.p, t.g))
                for k in sorted(int(d) for d in dropped) for i in sorted(int(c) for c in alive)]


def default_threshold(K):
    return max(1, int(K) // 2)


def draw_dropped(seed, round_idx, sampled, frac, threshold):
    """The sampled clients that drop after the key setup of round ``round_idx``: ``int(frac * K)`` of them, fewer
    where more than ``threshold`` must survive; a deterministic function of (seed, round), the same on every rank."""
    order = sorted(int(c) for c in sampled)
    K = len(order)
    n = max(0, min(int(float(frac) * K), K - int(threshold) - 1))
    if n == 0:
        return []
    s = int(_mix_hash_np(int(seed) & 0xffffffffffffffff, 0x73656361, int(round_idx) & 0xffffffff))
    return sorted(int(c) for c in np.random.RandomState(s).choice(order, n, replace=False))


# ------------------------------------------------------------------------------------------------ driver
def aggregate(theta, bufs, P, Q, local_rows, local_clients, sampled, sizes, info, keys, round_idx, out_w, out_b,
              scale=2 ** 16, dropped=(), fuse=True, budget=2e9, hip=None):
    """Secure FedAvg of the sampled clients' (params, buffers) into ``out_w`` ``[P]`` / ``out_b`` ``[Q]``.

    ``theta`` / ``bufs``: this rank's row matrices; ``local_rows`` / ``local_clients``: the rows of the sampled
    clients that live here and their global ids; ``sizes[c]``: client c's sample count; ``keys``: the
    :class:`SecAggKeys` of the federation; ``dropped``: sampled clients that never upload.

    ``fuse``: :func:`masked_sum` over the local survivors (masks only towards participants on other ranks and dropped
    clients); else :func:`upload` in row chunks of at most ``budget`` bytes, summed - the protocol's real cost, the
    same bits.  Then one int64 SUM all-reduce of the ``[P + Q]`` partials (with the event count in their last word)
    and :func:`finish` on every rank.  Returns a device int64 ``[2]``: saturated / non-finite values, dropped clients."""
    order = sorted(int(c) for c in sampled)
    K = len(order)
    gone = set(int(c) for c in dropped)
    alive = [c for c in order if c not in gone]
    if not gone <= set(order) or len(alive) <= keys.T:
        raise ValueError("secure aggregation: dropped clients must be sampled and more than T = %d of %d must survive"
                         % (keys.T, K))
    B = saturation_bound(K, P_FIELD)
    n_tot = float(sum(int(sizes[c]) for c in order))
    a = float(sum(int(sizes[c]) for c in alive)) / n_tot
    dev = theta.device
    mine = [(int(r), int(c)) for r, c in zip(local_rows, local_clients) if int(c) not in gone]
    here = set(c for _, c in mine)
    Pp, Qp = (P + 1) // 2 * 2, (Q + 1) // 2 * 2  # 16-byte aligned sections of the int64 partial
    acc = torch.zeros(Pp + Qp + 2, dtype=torch.int64, device=dev)
    if mine:
        ridx = [r for r, _ in mine]
        cids = [c for _, c in mine]
        wts = [int(sizes[c]) / n_tot for c in cids]
        peers = [[(j, int(keys.key[c, j])) for j in order if j != c and not (fuse and j in here)] for c in cids]
        for seg, src, n, off in ((SEG_PARAMS, theta, P, 0), (SEG_BUFS, bufs, Q, Pp)):
            if not n:
                continue
            part = acc[off:off + n]
            if fuse:
                ev = masked_sum(src, ridx, n, cids, peers, wts, round_idx, seg, scale, B, part, hip=hip)
            else:
                ev = torch.zeros((), dtype=torch.int64, device=dev)
                step = max(1, int(budget // (4 * n)))
                for c0 in range(0, len(ridx), step):
                    sl = slice(c0, c0 + step)
                    up, e = upload(src, ridx[sl], n, cids[sl], peers[sl], wts[sl], round_idx, seg, scale, B, hip=hip)
                    part += up.sum(0, dtype=torch.int64)
                    ev = ev + e
                part.remainder_(P_FIELD)
            acc[Pp + Qp] += ev
    rt.all_reduce_buckets(acc, info)
    pairs = keys.removal_pairs(sorted(gone), alive)
    fin_hip = None if hip is None else bool(hip) and dev.type == "cuda"
    for seg, n, off, out in ((SEG_PARAMS, P, 0, out_w), (SEG_BUFS, Q, Pp, out_b)):
        if n:
            finish(acc[off:off + n], n, pairs, round_idx, seg, scale, a, out, hip=fin_hip)
    return torch.cat([acc[Pp + Qp:Pp + Qp + 1], _to_dev([len(gone)], torch.int64, dev)])
