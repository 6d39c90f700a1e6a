"""FedAvg and FedProx (reference ``fedml_api/standalone/fedavg/fedavg_api.py:40-173``).

Per round: sample clients, each trains from ``w_global``, sample-weighted average of all keys,
evaluate the global model and each client's personal (last local) model.  After the last round
every client runs one extra local "fine-tune" pass from ``w_global`` and a final evaluation
(``fedavg_api.py:78-88``).

FedProx (new; BASELINE.json config 4) is FedAvg with the proximal term ``mu/2 ||w - w_g||^2``
added to each local loss (``args.fedprox_mu``) and an optional robust aggregator
(``args.aggregator`` in {``fedavg``, ``krum``, ``multikrum``, ``median``, ``trimmed_mean``}).
"""
from __future__ import annotations

import time

import numpy as np

from .common import APIBase
from ..core import robustness as R


def secure_aggregate(args, stat_info, w_locals, round_idx=0, client_ids=None, keys=None):
    """``--aggregator secure`` on the eager path: the host protocol (``TurboAggregateTrainer(prg="counter")``) over the
    participants' states, with the key setup and the dropout draw of ``engine/secagg.py`` - the oracle of the
    client-batched executor's secure aggregation, equal to it bit for bit.  ``keys``: the key setup of an earlier
    round (reused while the federation and the threshold stay the same).  Returns (global state, key setup) and records
    ``secagg_saturated`` / ``secagg_dropped`` in ``stat_info``."""
    from ..engine import secagg as SA
    from .turboaggregate import secure_state_average
    if (getattr(args, "defense_type", None) or "none") != "none" or float(getattr(args, "update_topk", 0.0) or 0) > 0:
        raise ValueError("aggregator=secure cannot be combined with defense_type or update_topk")
    ids = list(range(len(w_locals))) if client_ids is None else [int(c) for c in client_ids]
    T = int(getattr(args, "secagg_threshold", 0) or 0) or SA.default_threshold(len(ids))
    N = int(getattr(args, "client_num_in_total", 0) or 0) or (max(ids) + 1)
    seed = int(getattr(args, "seed", 0) or 0)
    if keys is None or keys.T != T or keys.n != N:
        keys = SA.SecAggKeys(N, T, seed=seed, scale=int(getattr(args, "secagg_scale", 2 ** 16) or 2 ** 16))
    dropped = SA.draw_dropped(seed, round_idx, ids, float(getattr(args, "secagg_dropout", 0.0) or 0.0), T)
    keys.trainer.saturated = 0
    out = secure_state_average(keys.trainer, w_locals, ids, round_idx, dropped, is_param=R.is_weight_param)
    stat_info["secagg_saturated"] = int(keys.trainer.saturated)
    stat_info["secagg_dropped"] = len(dropped)
    return out, keys


class FedAvgAPI(APIBase):

    def _aggregate(self, w_locals, w_global=None, round_idx=0, client_ids=None):
        """Sample-weighted mean (or ``args.aggregator``; ``secure``: :meth:`_aggregate_secure` over the participants
        ``client_ids`` of round ``round_idx``).  With ``args.defense_type`` in {``norm_diff_clipping``,
        ``weak_dp``} and the current global state ``w_global``, every client first goes through the reference's
        ``RobustAggregator`` (``robust_aggregation.py:32-55``): its update over the weight parameters is clipped to
        ``args.norm_bound``; ``weak_dp`` then adds ``torch.randn * args.stddev`` to those entries.  This is the
        reference-semantics oracle for the executor's clipping (``engine/defense.py``), not for its noise bits."""
        kind = getattr(self.args, "aggregator", "fedavg") or "fedavg"
        defense = getattr(self.args, "defense_type", None) or "none"
        if kind == "secure":
            return self._aggregate_secure(w_locals, round_idx, client_ids)
        if defense != "none" and kind == "fedavg" and w_global is not None:
            ra = R.RobustAggregator(self.args)
            clipped = []
            for n, w in w_locals:
                w = ra.norm_diff_clipping(w, w_global)
                if defense == "weak_dp":
                    w = {k: ra.add_noise(v) if R.is_weight_param(k) else v for k, v in w.items()}
                clipped.append((n, w))
            w_locals = clipped
        if kind == "fedavg":
            return super()._aggregate(w_locals)
        return R.robust_aggregate(kind, w_locals, f=int(getattr(self.args, "byzantine_f", 0) or 0),
                                  trim_ratio=float(getattr(self.args, "trim_ratio", 0.1) or 0.1))

    def _aggregate_secure(self, w_locals, round_idx=0, client_ids=None):
        out, self._secagg_keys = secure_aggregate(self.args, self.stat_info, w_locals, round_idx, client_ids,
                                                  getattr(self, "_secagg_keys", None))
        return out

    def _local_kwargs(self, w_global):
        if float(getattr(self.args, "fedprox_mu", 0.0) or 0.0) > 0:
            return {"prox_ref": w_global}
        return {}

    def train(self):
        w_global = self.model_trainer.get_model_params()
        w_per_mdls = [dict(w_global) for _ in range(self.args.client_num_in_total)]
        for round_idx in range(self.args.comm_round):
            t0 = time.perf_counter()
            self.logger.info("################Communication round : %d", round_idx)
            idx = np.sort(self._client_sampling(round_idx, self.args.client_num_in_total,
                                                self.args.client_num_per_round))
            w_locals = []
            for c in idx:
                client = self.client_list[c]
                w, flops, comm = client.train(w_global, round_idx, None, **self._local_kwargs(w_global))
                w_per_mdls[c] = w
                w_locals.append((client.get_sample_number(), w))
                self.stat_info["sum_training_flops"] += flops
                self.stat_info["sum_comm_params"] += comm
            w_global = self._aggregate(w_locals, w_global, round_idx=round_idx, client_ids=idx)
            freq = max(1, int(getattr(self.args, "frequency_of_the_test", 1) or 1))
            if round_idx % freq == 0 or round_idx == self.args.comm_round - 1:
                self._test_on_all_clients(w_global, w_per_mdls, round_idx)
            self.stat_info["round_time_s"].append(time.perf_counter() - t0)
        if getattr(self.args, "final_finetune", True):
            for c in range(self.args.client_num_in_total):
                w, _, _ = self.client_list[c].train(w_global, self.args.comm_round, None)
                w_per_mdls[c] = w
            self._test_on_all_clients(w_global, w_per_mdls, -1)
        self.w_global = w_global
        return w_global


class FedProxAPI(FedAvgAPI):
    """FedAvg with a proximal local objective; ``args.fedprox_mu`` defaults to 0.01."""

    def __init__(self, dataset, device, args, model_trainer, logger=None):
        if not getattr(args, "fedprox_mu", 0):
            args.fedprox_mu = 0.01
        super().__init__(dataset, device, args, model_trainer, logger)
