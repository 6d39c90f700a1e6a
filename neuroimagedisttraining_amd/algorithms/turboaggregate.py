"""Secure-aggregation building blocks (reference ``fedml_api/standalone/turboaggregate/{mpc_function,TA_trainer,
TA_client}.py``) and a working secure FedAvg.

Finite-field helpers over a prime ``p`` (int64 numpy; p < 2**31 so products fit): modular inverse, Lagrange
coefficients, BGW (Shamir) encoding/decoding, Lagrange Coded Computing (LCC) encoding/decoding, additive secret
sharing and a toy Diffie-Hellman key agreement.  The reference's trainer hook is a ``pass`` stub; here
:class:`TurboAggregateTrainer` runs an actual secure aggregation round: every client quantises its weighted
update to fixed point in Z_p, adds pairwise masks derived from agreed keys (they cancel in the sum), the server
sums the masked vectors and de-quantises — the result equals plain FedAvg up to the quantisation step, and the
server never sees an individual client's vector.  Dropped clients' masks are recovered from BGW shares of their
secret keys held by the survivors.
"""
from __future__ import annotations

import numpy as np

from ..engine.masks import counter_mask, mod_mersenne31  # noqa: F401 (the prg="counter" mask PRG)

P_DEFAULT = 2 ** 31 - 1  # Mersenne prime


def modular_inv(a, p):
    """a^-1 mod p (p prime) by Fermat."""
    return pow(int(a) % p, p - 2, p)


def divmod(_num, _den, _p):  # noqa: A001 (reference name)
    return (int(_num) % _p) * modular_inv(_den, _p) % _p


def PI(vals, p):  # noqa: N802
    acc = 1
    for v in vals:
        acc = acc * (int(v) % p) % p
    return acc


def gen_Lagrange_coeffs(alpha_s, beta_s, p, is_K1=0):  # noqa: N802
    """U[i][j] = prod_{o != beta_j} (alpha_i - o) / (beta_j - o)  (mod p)."""
    alphas = [alpha_s[0]] if is_K1 == 1 else list(alpha_s)
    U = np.zeros((len(alphas), len(beta_s)), dtype=np.int64)
    for i, a in enumerate(alphas):
        for j, b in enumerate(beta_s):
            others = [o for o in beta_s if o != b]
            U[i, j] = divmod(PI([a - o for o in others], p), PI([b - o for o in others], p), p)
    return U


# model-sized encodings (U [N x K] @ X [K x d], d in the millions) go to the gfx950 kernel when a GPU is present
DEVICE_MIN_ELEMS = 1 << 16


def matmul_mod_device(A, B, p, device="cuda"):
    """(A @ B) mod p on the GPU (``mpc.hip`` ``modp_matmul``): int64 operands reduced to [0, p), p < 2^32."""
    import torch
    from .. import ops
    A = torch.as_tensor(np.asarray(A, dtype=np.int64) % p).to(device).contiguous()
    B = torch.as_tensor(np.asarray(B, dtype=np.int64) % p).to(device).contiguous()
    C = torch.empty((A.shape[0], B.shape[1]), dtype=torch.int64, device=device)
    ops.ext().modp_matmul(A.data_ptr(), B.data_ptr(), C.data_ptr(), A.shape[0], A.shape[1], B.shape[1], int(p),
                          ops.stream())
    return C.cpu().numpy()


def _matmul_mod(A, B, p):
    """(A @ B) mod p without int64 overflow (row-by-row accumulation of reduced products); large products on the
    GPU kernel."""
    A = np.asarray(A, dtype=np.int64) % p
    B = np.asarray(B, dtype=np.int64) % p
    if B.size >= DEVICE_MIN_ELEMS and p < (1 << 32):
        import torch
        if torch.cuda.is_available():
            return matmul_mod_device(A, B, p)
    out = np.zeros((A.shape[0], B.shape[1]), dtype=np.int64)
    for k in range(A.shape[1]):
        out = (out + (A[:, k:k + 1] * B[k:k + 1, :]) % p) % p
    return out


def BGW_encoding(X, N, T, p, rng=None):  # noqa: N802
    """Shamir shares of X (shape [m, d]) for N workers, threshold T: f(a) = X + sum_t R_t a^t at a = 1..N."""
    rng = np.random if rng is None else rng
    X = np.asarray(X, dtype=np.int64) % p
    R = rng.randint(p, size=(T,) + X.shape).astype(np.int64)
    out = np.zeros((N,) + X.shape, dtype=np.int64)
    for n in range(N):
        a = n + 1
        acc = X.copy()
        ap = 1
        for t in range(T):
            ap = ap * a % p
            acc = (acc + R[t] * ap) % p
        out[n] = acc
    return out


def gen_BGW_lambda_s(alpha_s, p):  # noqa: N802
    """Lagrange coefficients that interpolate f(0) from evaluations at alpha_s."""
    return gen_Lagrange_coeffs([0], list(alpha_s), p)[0]


def BGW_decoding(f_eval, worker_idx, p):  # noqa: N802
    """Recover f(0) from >= T+1 shares; ``worker_idx`` are 0-based worker ids (evaluation points idx+1)."""
    lam = gen_BGW_lambda_s([int(i) + 1 for i in worker_idx], p)
    f = np.asarray(f_eval, dtype=np.int64) % p
    acc = np.zeros(f.shape[1:], dtype=np.int64)
    for k, l in enumerate(lam):
        acc = (acc + f[k] * int(l)) % p
    return acc


def LCC_encoding_with_points(X, alpha_s, beta_s, p):  # noqa: N802
    """Encode the rows X[j] (placed at beta_j) and evaluate the interpolant at alpha_s."""
    U = gen_Lagrange_coeffs(alpha_s, beta_s, p)
    X = np.asarray(X, dtype=np.int64)
    flat = X.reshape(X.shape[0], -1)
    return _matmul_mod(U, flat, p).reshape((len(alpha_s),) + X.shape[1:])


def LCC_decoding_with_points(f_eval, eval_points, target_points, p):  # noqa: N802
    return LCC_encoding_with_points(f_eval, target_points, eval_points, p)


def lcc_points(n, p):
    """The reference's evaluation points: n consecutive integers centred on 0, mod p
    (``stt = -floor(n/2)``, ``mpc_function.py:121-125``)."""
    s = -int(np.floor(n / 2))
    return [int(v) % p for v in range(s, s + n)]


def LCC_encoding(X, N, K, T, p, rng=None):  # noqa: N802
    """Split X [m, d] into K row blocks, append T random blocks, LCC-encode for N workers.  Data blocks sit at the
    reference's centred points beta (K + T of them) and worker j evaluates at the centred point alpha_j (N of
    them), so the shares equal the reference's (``mpc_function.py:111-135``)."""
    rng = np.random if rng is None else rng
    X = np.asarray(X, dtype=np.int64) % p
    m = X.shape[0] // K
    blocks = [X[i * m:(i + 1) * m] for i in range(K)] + [rng.randint(p, size=(m,) + X.shape[1:]) for _ in range(T)]
    return LCC_encoding_with_points(np.stack(blocks), lcc_points(N, p), lcc_points(K + T, p), p)


def LCC_encoding_w_Random(X, R_, N, K, T, p):  # noqa: N802
    X = np.asarray(X, dtype=np.int64) % p
    m = X.shape[0] // K
    blocks = [X[i * m:(i + 1) * m] for i in range(K)] + [np.asarray(R_[t], dtype=np.int64) for t in range(T)]
    return LCC_encoding_with_points(np.stack(blocks), lcc_points(N, p), lcc_points(K + T, p), p)


def LCC_encoding_w_Random_partial(X, R_, N, K, T, p, worker_idx):  # noqa: N802
    return LCC_encoding_w_Random(X, R_, N, K, T, p)[list(worker_idx)]


def LCC_decoding(f_eval, f_deg, N, K, T, worker_idx, p):  # noqa: N802
    """Interpolate the K data blocks from the evaluations of workers ``worker_idx`` (reference
    ``mpc_function.py:195-212``: targets are the K centred points, sources the workers' centred points).  As in
    the reference, the targets coincide with the encoder's first K points only when floor(K/2) ==
    floor((K+T)/2) (e.g. T = 1 with even K); :func:`LCC_decoding_with_points` takes explicit points."""
    if (K // 2) != ((K + T) // 2):
        import warnings
        warnings.warn("LCC_decoding(K=%d, T=%d): the reference's targets lcc_points(K) differ from the encoder's data "
                      "points; use LCC_decode_blocks to recover the encoded blocks" % (K, T), stacklevel=2)
    alpha = lcc_points(N, p)
    ev = [alpha[int(i)] for i in worker_idx]
    need = (K + T - 1) * f_deg + 1
    return LCC_decoding_with_points(np.asarray(f_eval)[:need], ev[:need], lcc_points(K, p), p)


def LCC_decode_blocks(f_eval, f_deg, N, K, T, worker_idx, p):  # noqa: N802
    """Recover the K data blocks that :func:`LCC_encoding` placed at its first K points beta (of K + T) from the
    evaluations of workers ``worker_idx`` — the decoder that matches the encoder for every K, T (the
    reference-compatible :func:`LCC_decoding` does only when floor(K/2) == floor((K+T)/2))."""
    alpha = lcc_points(N, p)
    ev = [alpha[int(i)] for i in worker_idx]
    need = (K + T - 1) * f_deg + 1
    return LCC_decoding_with_points(np.asarray(f_eval)[:need], ev[:need], lcc_points(K + T, p)[:K], p)


def Gen_Additive_SS(d, n_out, p, rng=None):  # noqa: N802
    """n_out additive shares of zero-sum over Z_p (rows sum to 0 mod p)."""
    rng = np.random if rng is None else rng
    s = rng.randint(p, size=(n_out - 1, d)).astype(np.int64)
    last = (-s.sum(0)) % p
    return np.concatenate([s, last[None]], 0)


def my_pk_gen(my_sk, p, g):
    return my_sk if g == 0 else pow(int(g), int(my_sk), p)


def my_key_agreement(my_sk, u_pk, p, g):
    return int(my_sk) * int(u_pk) % p if g == 0 else pow(int(u_pk), int(my_sk), p)


# ------------------------------------------------------------------------------------------------ secure FedAvg
def quantize(v, scale, p):
    q = np.round(np.asarray(v, dtype=np.float64) * scale).astype(np.int64)
    return q % p


def dequantize(q, scale, p):
    q = np.asarray(q, dtype=np.int64) % p
    q = np.where(q > p // 2, q - p, q)
    return q.astype(np.float64) / scale


def saturation_bound(K, p=P_DEFAULT):
    """Largest ``|q|`` one of ``K`` participants may send so that the sum of K values stays decodable."""
    return ((p - 1) // 2) // max(1, int(K))


def quantize_saturated(vec, weight, scale, K, p=P_DEFAULT):
    """(residues int64 in [0, p), events): ``q = rint((double(vec) * weight) * scale)`` (round half to even, the bits
    of :func:`quantize` on fp64 input), ``|q|`` saturated at :func:`saturation_bound` of ``K`` participants, a
    non-finite value -> 0; ``events`` counts both."""
    return quantize_bounded(vec, weight, scale, saturation_bound(K, p), p)


def quantize_bounded(vec, weight, scale, B, p=P_DEFAULT):
    """:func:`quantize_saturated` with the bound given."""
    B = float(B)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (np.asarray(vec).astype(np.float64) * float(weight)) * float(scale)
        fin = np.isfinite(x)
        r = np.round(np.where(fin, x, 0.0))
    events = int((~fin).sum() + (np.abs(r) > B).sum())
    return np.clip(r, -B, B).astype(np.int64) % p, events


class TurboAggregateTrainer:
    """Secure FedAvg over flat parameter vectors with pairwise masking and BGW-protected secret keys.

    ``prg="mt"`` (default): a pair's mask is a Mersenne-Twister stream seeded by its key, the same in every round.
    ``prg="counter"``: :func:`counter_mask` keyed by (key, round, segment, coordinate) and saturating quantisation
    (:func:`quantize_saturated`) - the protocol of ``csrc/kernels/secagg.hip``, whose rows :meth:`client_upload`
    then reproduces bit for bit."""

    def __init__(self, n_clients, p=P_DEFAULT, g=7, scale=2 ** 16, threshold=None, seed=0, prg="mt"):
        if prg not in ("mt", "counter"):
            raise ValueError("prg %r: one of mt | counter" % (prg,))
        if prg == "counter" and p != P_DEFAULT:
            raise ValueError("prg=counter is defined over p = 2^31 - 1 only")
        self.n, self.p, self.g, self.scale, self.prg = n_clients, p, g, scale, prg
        self.T = threshold if threshold is not None else max(1, n_clients // 2)
        self.rng = np.random.RandomState(seed)
        self.sk = self.rng.randint(1, p - 1, size=n_clients)
        self.pk = [my_pk_gen(s, p, g) for s in self.sk]
        # each client's secret key is Shamir-shared with everyone (for dropout recovery)
        self.sk_shares = [BGW_encoding(np.array([[s]]), n_clients, self.T, p, self.rng) for s in self.sk]
        self.saturated = 0  # prg="counter": saturated + non-finite values over all uploads so far

    def pair_key(self, i, j):
        return my_key_agreement(self.sk[i], self.pk[j], self.p, self.g)

    def _stream(self, key, d, round, seg):  # noqa: A002
        if self.prg == "counter":
            return counter_mask(key, round, seg, np.arange(d, dtype=np.uint64))
        return np.random.RandomState(key % (2 ** 32)).randint(self.p, size=d).astype(np.int64)

    def _mask(self, i, j, d, round=0, seg=0):  # noqa: A002
        r = self._stream(self.pair_key(i, j), d, round, seg)
        return r if i < j else (-r) % self.p

    def client_upload(self, i, vec, weight, round=0, seg=0, peers=None):  # noqa: A002
        """Client i's masked vector.  ``prg="counter"``: ``round`` / ``seg`` key the masks and ``peers`` (default:
        every other client) are the round's other participants; K = len(peers) + 1 sets the saturation bound."""
        d = vec.size
        peers = [j for j in range(self.n) if j != i] if peers is None else [int(j) for j in peers if int(j) != i]
        if self.prg == "counter":
            y, ev = quantize_saturated(vec, weight, self.scale, len(peers) + 1, self.p)
            self.saturated += ev
        else:
            y = quantize(vec * weight, self.scale, self.p)
        for j in peers:
            y = (y + self._mask(i, j, d, round, seg)) % self.p
        return y

    def reconstruct_sks(self, dropped, alive):
        """{k: client k's secret key} for the ``dropped`` clients, from the BGW shares the first T + 1 of the ``alive``
        clients hold."""
        hold = sorted(int(c) for c in alive)[:self.T + 1]
        lam = [int(v) for v in gen_BGW_lambda_s([i + 1 for i in hold], self.p)]
        out = {}
        for k in dropped:
            sk_k = sum(int(self.sk_shares[int(k)][i][0, 0]) * l for i, l in zip(hold, lam)) % self.p
            assert sk_k == int(self.sk[int(k)])
            out[int(k)] = sk_k
        return out

    def server_sum(self, uploads, dropped=(), round=0, seg=0):  # noqa: A002
        """Sum of the uploads mod p with the survivors' masks towards the ``dropped`` clients removed: residues."""
        alive = sorted(uploads)
        d = next(iter(uploads.values())).size
        s = np.zeros(d, dtype=np.int64)
        for i in alive:
            s = (s + uploads[i]) % self.p
        sks = self.reconstruct_sks(dropped, alive)
        for k in dropped:
            sk_k = sks[int(k)]
            for i in alive:  # the survivors' masks with k did not cancel: remove them
                r = self._stream(my_key_agreement(sk_k, self.pk[i], self.p, self.g), d, round, seg)
                m_ik = r if i < k else (-r) % self.p  # mask client i added for pair (i, k)
                s = (s - m_ik) % self.p
        return s

    def server_aggregate(self, uploads, dropped=(), round=0, seg=0, alive_weight=1.0):  # noqa: A002
        """``uploads``: dict client -> masked vector.  Masks of dropped clients are removed by reconstructing
        their secret keys from BGW shares held by the survivors.  ``prg="counter"``: the result is
        ``float32(double(c) / scale / alive_weight)`` (``alive_weight`` = the survivors' share of the weights)."""
        s = self.server_sum(uploads, dropped, round, seg)
        if self.prg == "counter":
            return ((dequantize(s, 1, self.p) / float(self.scale)) / float(alive_weight)).astype(np.float32)
        return dequantize(s, self.scale, self.p)


def secure_state_average(trainer, w_locals, client_ids, round_idx=0, dropped=(), is_param=None):
    """Sample-weighted mean of ``w_locals`` (``[(n_samples, state_dict)]`` of the participants ``client_ids``) through
    a ``prg="counter"`` trainer: the entries ``is_param`` keeps travel as segment 0 and the others (BN statistics) as
    segment 1, each flattened in state order; the ``dropped`` participants never upload and their masks are recovered.
    The client-batched executor's ``--aggregator secure`` computes the same bits.  Every entry comes back as float32,
    the format the server decodes to (``weighted_average`` likewise returns integer entries such as
    ``num_batches_tracked`` as floats)."""
    import torch
    ids = [int(c) for c in client_ids]
    keys = list(w_locals[0][1].keys())
    is_param = is_param or (lambda k: True)
    gone = set(int(c) for c in dropped)
    n_tot = float(sum(n for n, _ in w_locals))
    a = float(sum(n for (n, _), c in zip(w_locals, ids) if c not in gone)) / n_tot
    out = {}
    for seg, ks in enumerate(([k for k in keys if is_param(k)], [k for k in keys if not is_param(k)])):
        if not ks:
            continue
        uploads = {}
        for (n, sd), c in zip(w_locals, ids):
            if c not in gone:
                vec = np.concatenate([sd[k].detach().reshape(-1).float().cpu().numpy() for k in ks])
                uploads[c] = trainer.client_upload(c, vec, n / n_tot, round=round_idx, seg=seg, peers=ids)
        agg = trainer.server_aggregate(uploads, dropped=sorted(gone), round=round_idx, seg=seg, alive_weight=a)
        o = 0
        for k in ks:
            t = w_locals[0][1][k]
            out[k] = torch.from_numpy(agg[o:o + t.numel()].copy()).view(t.shape).to(t.device)
            o += t.numel()
    return {k: out[k] for k in keys}


class TA_Client:  # noqa: N801 (reference name)
    """Turbo-Aggregate participant (reference ``turboaggregate/TA_client.py:8-26``): local data handles plus the
    ``isdrop`` flag the protocol uses to simulate a client that drops out after uploading nothing; the
    server side recovers the masks of dropped clients in :meth:`TurboAggregateTrainer.server_aggregate`."""

    def __init__(self, local_training_data, local_test_data, local_sample_number, args, device, client_idx=0):
        self.local_training_data = local_training_data
        self.local_test_data = local_test_data
        self.local_sample_number = local_sample_number
        self.args, self.device, self.client_idx = args, device, client_idx
        import torch.nn as nn
        self.criterion = nn.CrossEntropyLoss()
        self.isdrop = False

    def set_dropout(self, isdrop):
        self.isdrop = bool(isdrop)

    def get_sample_number(self):
        return self.local_sample_number


def secure_round(trainer, clients, vectors, weights):
    """One Turbo-Aggregate round over ``TA_Client`` objects: every client that is not marked dropped uploads its
    masked, weighted update; the server removes the dropped clients' masks and returns the weighted sum."""
    uploads = {i: trainer.client_upload(i, vectors[i], weights[i]) for i, c in enumerate(clients) if not c.isdrop}
    dropped = [i for i, c in enumerate(clients) if c.isdrop]
    return trainer.server_aggregate(uploads, dropped=dropped)
