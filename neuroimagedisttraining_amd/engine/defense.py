"""Norm-difference clipping and weak-DP noise fused into the FedAvg row sum (``csrc/kernels/defense.hip``).

The reference's only defence (``fedml_core/robustness/robust_aggregation.py:32-55``): each client's update
``w_i - w_g`` over the weight parameters is scaled into an L2 ball of radius ``norm_bound``; "weak DP" then adds
``N(0, stddev^2)`` to every client's weights.  Here both run on the client rows in place:

* :func:`rows_diff_norm` — ``||rows[c, :P] - ref||_2`` per row (fp32 difference, fp64 accumulation);
* :func:`clipped_rows_sum` — ``sum_c w_c * ((rows[c] - ref) / max(1, norm_c / bound) + ref + stddev * z_c)``.

The noise ``z(seed, client, coordinate)`` is counter based (:func:`noise_z_np` is the fp64 twin of the kernel's
fp32 Box-Muller), so a client draws the same noise on whichever rank and in whichever row it lives — results do not
depend on the sharding, which ``torch.randn`` cannot give.  Deviation from the reference: with a SalientGrads mask the
noise is confined to the coordinates the mask keeps (a pruned weight that is 0 everywhere stays exactly 0); the
reference would add noise to pruned coordinates too.

Contiguous CUDA rows take the HIP kernels; anything else (CPU, gathered rows) takes the torch twin, which follows the
kernel's operation order.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .masks import _mix_hash_np, unpack_bits

DEFENSES = ("none", "norm_diff_clipping", "weak_dp")
_SEED2 = 0x5bd1e995


def round_seed(seed, round_idx):
    """Noise seed of one round: a hash of (cfg.seed, round), the same on every rank."""
    return int(_mix_hash_np(int(seed) & 0xffffffffffffffff, 0x64656665, int(round_idx) & 0xffffffff))


def noise_z_np(seed, cid, j):
    """fp64 twin of ``noise_z`` in defense.hip: unit normals keyed by (seed, client id, coordinates ``j``)."""
    j = np.asarray(j, dtype=np.uint64)
    h1 = _mix_hash_np(seed, cid, j)
    h2 = _mix_hash_np(int(seed) ^ _SEED2, cid, j)
    u1 = ((h1 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24   # (0, 1]
    u2 = (h2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24                    # [0, 1)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(np.pi * (2.0 * u2))


def _use_hip(rows, ref, hip):
    """Whether the HIP kernels run: ``hip`` None = whenever the operands allow it; True = they must (a layout the
    kernels cannot take is an error, never a silent torch run); False = the torch twin."""
    ok = (rows.device.type == "cuda" and rows.dtype == torch.float32 and rows.stride(1) == 1
          and rows.stride(0) % 4 == 0 and rows.data_ptr() % 16 == 0 and ref.dtype == torch.float32
          and ref.is_contiguous() and ref.data_ptr() % 16 == 0 and rows.shape[1] >= ref.numel())
    if hip and not ok:
        raise ValueError("defense kernels need contiguous 16-byte aligned fp32 CUDA rows and ref")
    return ok if hip is None else bool(hip)


def rows_diff_norm(rows, ref, hip=None):
    """``[C]`` fp32 norms of ``rows[c, :P] - ref`` (``rows`` ``[C, >= P]`` fp32, ``ref`` ``[P]``)."""
    C, P = rows.shape[0], ref.numel()
    norm = torch.empty(C, dtype=torch.float32, device=rows.device)
    if C == 0:
        return norm
    if _use_hip(rows, ref, hip):
        m = ops.ext()
        part = torch.empty((C, m.rows_diff_norm_blocks(P)), dtype=torch.float64, device=rows.device)
        m.rows_diff_norm(rows.data_ptr(), ref.data_ptr(), C, P, rows.stride(0), part.data_ptr(), norm.data_ptr(),
                         ops.stream())
        return norm
    for c in range(C):  # one row at a time: [P] temporaries only
        d = (rows[c, :P] - ref).double()
        norm[c] = (d * d).sum().sqrt().float()
    return norm


def clipped_rows_sum(rows, ref, wts, norm, cids, norm_bound, stddev, seed, out, mbits=None, hip=None):
    """``out[:P] = sum_c wts[c] * ((rows[c, :P] - ref) / max(1, norm[c] / norm_bound) + ref + stddev * z_c)``.

    ``cids``: global client id of every row (the noise key; a list on the torch path, any int32 tensor on the HIP
    path); ``mbits``: optional shared ``[1, W]`` bit row — noise only where the bit is set.  Nothing past ``P`` is
    written."""
    C, P = rows.shape[0], ref.numel()
    if _use_hip(rows, ref, hip):
        assert out.dtype == torch.float32 and out.is_contiguous() and out.data_ptr() % 16 == 0 and out.numel() >= P
        ct = cids if torch.is_tensor(cids) else torch.tensor(list(cids), dtype=torch.int32).to(rows.device)
        assert ct.dtype == torch.int32 and ct.numel() == C and wts.dtype == torch.float32 and wts.numel() == C
        if mbits is not None:
            assert mbits.dtype == torch.int32 and mbits.is_contiguous() and mbits.numel() * 32 >= P
        ops.ext().clipped_rows_sum(rows.data_ptr(), ref.data_ptr(), wts.data_ptr(), norm.data_ptr(), ct.data_ptr(), C,
                                   P, rows.stride(0), float(norm_bound), float(stddev), int(seed),
                                   mbits.data_ptr() if (mbits is not None and stddev > 0) else 0, out.data_ptr(),
                                   ops.stream())
        return out
    dev = rows.device
    bound = torch.full((1,), float(norm_bound), dtype=torch.float32, device=dev)
    m = torch.clamp_min(norm / bound, 1.0)
    keep = unpack_bits(mbits.view(1, -1), P)[0] if (mbits is not None and stddev > 0) else None
    sd = torch.full((1,), float(stddev), dtype=torch.float32, device=dev)
    acc = torch.zeros(P, dtype=torch.float32, device=dev)
    cl = [int(c) for c in (cids.tolist() if torch.is_tensor(cids) else cids)] if stddev > 0 else None
    idx = np.arange(P, dtype=np.uint64)
    for c in range(C):  # rows in ascending order, one at a time: [P] temporaries only
        r = (rows[c, :P] - ref) / m[c:c + 1] + ref
        if stddev > 0:
            z = torch.from_numpy(noise_z_np(seed, cl[c], idx).astype(np.float32)).to(dev)
            nz = sd * z
            r = r + (nz * keep if keep is not None else nz)
        acc = acc + wts[c:c + 1] * r
    out[:P] = acc
    return out
