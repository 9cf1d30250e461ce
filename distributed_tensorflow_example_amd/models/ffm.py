"""Field-aware factorization machine (Juan et al. 2016) on CTR batches.

P fields, K factors per (feature, field): a linear table w [F], a factor table
V [F, P * K] whose columns q K .. (q + 1) K of row j are feature j's vector aimed
at field q, and a bias b.  For batch row r, entry i has field p_i, id j_i, value x_i:

    A_r[p][q, :] = sum_{i in field p} x_i V[j_i, q K : (q + 1) K]
    z_r  = b + sum_i x_i w[j_i] + sum_{p < q} < A_r[p][q, :], A_r[q][p, :] >
    loss = mean_r sigmoid_xent(z_r, y_r)

Entries of one field are sum-pooled, as embedding_lookup_sparse(combiner="sum")
pools a multivalent column, and only different fields interact.  With at most one
entry per field this is exactly Juan et al.'s model,
sum_{i < i'} x_i x_i' < V[j_i, field(i')], V[j_i', field(i)] >.  A repeated id counts
once per occurrence; ids outside [0, F) are skipped.  With dz_r = (sigmoid(z_r) - y_r) / B
and the bag gradient G_r[p][q, :] = dz_r A_r[q][p, :] (0 for q == p: same-field pairs
are excluded, so there is no self term to correct for)

    dL/dV[j, :] = sum_{occ of j} x G_r[p_occ][:]    dL/dw[j] = sum_{occ of j} x dz_r    dL/db = sum_r dz_r

and every touched row takes one update of a row-local rule of optim/rules.py (sgd,
momentum, adagrad, rmsprop, ftrl) with its duplicate-summed gradient; b takes the
dense form of the rule.

A batch is a CSR over (row, field) bags, (labels [B], offsets [B * P + 1], ids, vals):
bag r * P + p holds row r's entries of field p, empty bags allowed; `ffm_batch` makes
it from a per-entry field array.

One GPU: the step is ffm_rows (csrc/kernels/ffm.hip), the fixed-order sums and the
one-writer table update over the B * P bags (FFMPlan.rows, .sums, .update) plus the
bias rule, and evaluation is ffm_rows plus the evaluation record's reduce.  On the
CPU, or with DTF_FFM_FUSED=0, a torch fp32 path computes the same thing from
index_add_ into [B * P, P * K].  Tables are not sharded: world_size > 1 is refused.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from .. import ops, optim
from ..optim.rules import RULES
from ..parallel.world import World, get_world
from .eval_record import StreamingEvalMixin, _dev


def ffm_batch(labels, offsets, ids, vals, fields, num_fields: int):
    """The bag form (labels, offsets [B * P + 1], ids, vals) of a CSR batch over rows (offsets [B + 1]) with a field
    per entry: each row's entries grouped by field with a stable sort, so equal fields keep their order.  Torch
    ops on the tensors' device."""
    offsets, ids, fields = torch.as_tensor(offsets), torch.as_tensor(ids), torch.as_tensor(fields).to(torch.int64)
    P, B = int(num_fields), offsets.numel() - 1
    if fields.numel() != ids.numel() or bool(((fields < 0) | (fields >= P)).any()):
        raise ValueError(f"ffm_batch: one field in [0, {P}) per entry")
    row = torch.repeat_interleave(torch.arange(B, device=offsets.device), torch.diff(offsets))
    key, perm = torch.sort(row * P + fields.to(offsets.device), stable=True)
    bags = torch.zeros(B * P + 1, dtype=torch.int64, device=offsets.device)
    bags[1:] = torch.cumsum(torch.bincount(key, minlength=B * P), 0)
    perm = perm.to(ids.device)
    return labels, bags, ids[perm], None if vals is None else torch.as_tensor(vals)[perm]


class FFMTrainer(StreamingEvalMixin):
    _stream_reports_bad_ids = True

    def __init__(self, num_features: int, num_fields: int, factors: int = 4, lr: float = 0.01,
                 world: Optional[World] = None, seed: int = 1, device=None, init_std: float = 0.01,
                 optimizer: str = "sgd", optimizer_hp: Optional[dict] = None, auc_bins: int = 200):
        rule = RULES.get(optimizer)
        if rule is None or not rule.row_local:
            raise ValueError(f"FFMTrainer: optimizer must be one of {[n for n, r in RULES.items() if r.row_local]}, "
                             f"not '{optimizer}'")
        self.world = world or get_world()
        if self.world.world_size > 1:
            raise ValueError("FFMTrainer: sharded FFM tables are not built; train on one worker (world_size == 1)")
        if num_fields < 2 or factors < 1:
            raise ValueError("FFMTrainer: at least two fields and one factor")
        self.device = torch.device(device) if device is not None else self.world.device
        self.num_features, self.num_fields, self.factors = int(num_features), int(num_fields), int(factors)
        self.lr = float(lr)
        self.optimizer, self.optimizer_hp, self.rule = optimizer, dict(optimizer_hp or {}), rule
        rule.hp(self.optimizer_hp)                     # checked as TF's constructor checks them
        f32 = dict(dtype=torch.float32, device=self.device)
        self.w = torch.zeros(self.num_features, **f32)
        self.V = torch.empty(self.num_features, self.num_fields * self.factors, **f32)
        ops.philox_normal_(self.V, 1, 0, seed, 0.0, init_std)      # over the global element index
        self.b = torch.zeros(1, **f32)
        init = rule.slot_init(self.optimizer_hp)
        self.w_slots = {n: torch.full_like(self.w, v0) for n, v0 in zip(rule.slots, init)}
        self.V_slots = {n: torch.full_like(self.V, v0) for n, v0 in zip(rule.slots, init)}
        self._bopt = optim.fused(optimizer, [self.b], self.lr, **self.optimizer_hp)
        self.global_step = 0
        self._plan = self._graphed = self._fused = None
        self._init_eval_records(auc_bins)

    # ----------------------------------------------------------------- plumbing
    def sync_exchange(self):
        """Nothing is routed: every batch seen so far is applied."""

    def _route_table(self):
        return self

    @property
    def num_rows(self) -> int:
        return self.num_features

    def _fused_ok(self) -> bool:
        """One worker on a GPU and a shape the kernel takes: the step and the evaluation run on
        csrc/kernels/ffm.hip.  DTF_FFM_FUSED=0 keeps the torch path."""
        ok = self._fused
        if ok is None:
            ok = self.device.type == "cuda" and os.environ.get("DTF_FFM_FUSED", "1") != "0"
            if ok:
                from .. import _native
                if not _native.load().FFMPlan.supported(self.num_fields, self.factors):
                    raise ValueError(f"FFMTrainer: the fused step takes factors a multiple of 4, 2 .. 32 fields and "
                                     f"fields * factors <= 128, not {self.num_fields} x {self.factors} "
                                     f"(DTF_FFM_FUSED=0 runs the torch path)")
            self._fused = ok
        return ok

    _eval_fused_ok = _fused_ok

    def _native_plan(self):
        if self._plan is None:
            from .. import _native
            self._plan = _native.load().FFMPlan(self.w, self.V, self.b, self.num_fields)   # the tensors themselves
        return self._plan

    def _parts(self, batch):
        labels, offsets, ids, vals = batch
        dev = self.device
        labels, offsets = _dev(labels, dev, torch.float32).reshape(-1), _dev(offsets, dev, torch.int64)
        if offsets.numel() != labels.numel() * self.num_fields + 1:
            raise ValueError("FFMTrainer: offsets must hold B * num_fields + 1 entries, one bag per (row, field); "
                             "ffm_batch makes them from a field per entry")
        return labels, offsets, _dev(ids, dev, torch.int64), None if vals is None else _dev(vals, dev, torch.float32)

    # ----------------------------------------------------------------- the torch path
    def _forward_general(self, offsets, ids, vals):
        """(z [B], A [B, P, P, K], bag of each kept entry, its id, its value): fp32 torch."""
        P, K = self.num_fields, self.factors
        nb = offsets.numel() - 1
        bag = torch.repeat_interleave(torch.arange(nb, device=ids.device), torch.diff(offsets))
        ok = (ids >= 0) & (ids < self.num_features)
        bag, idk = bag[ok], ids[ok]
        x = torch.ones(idk.numel(), dtype=torch.float32, device=ids.device) if vals is None else vals[ok]
        A = torch.zeros(nb, P * K, dtype=torch.float32, device=ids.device).index_add_(0, bag, self.V[idk] * x[:, None])
        A = A.view(nb // P, P, P, K)
        T = (A * A.transpose(1, 2)).sum(-1)                          # T[r, p, q] = < A_r[p][q], A_r[q][p] >
        pair = 0.5 * (T.sum((1, 2)) - T.diagonal(dim1=1, dim2=2).sum(1))
        lin = torch.zeros(nb // P, dtype=torch.float32, device=ids.device).index_add_(
            0, torch.div(bag, P, rounding_mode="floor"), self.w[idk] * x)
        return self.b + lin + pair, A, bag, idk, x

    @torch.no_grad()
    def _train_step_general(self, labels, offsets, ids, vals) -> torch.Tensor:
        P, K = self.num_fields, self.factors
        z, A, bag, idk, x = self._forward_general(offsets, ids, vals)
        loss = ops.sigmoid_xent(z, labels)
        dz = (torch.sigmoid(z) - labels) / labels.numel()
        G = dz[:, None, None, None] * A.transpose(1, 2)              # G[r, p, q] = dz_r A_r[q][p]
        G = (G * (1 - torch.eye(P, dtype=torch.float32, device=z.device))[None, :, :, None]).reshape(-1, P * K)
        touched, inv = torch.unique(idk, return_inverse=True)
        gw = torch.zeros(touched.numel(), dtype=torch.float32, device=z.device)
        gw.index_add_(0, inv, x * dz[torch.div(bag, P, rounding_mode="floor")])
        gV = torch.zeros(touched.numel(), P * K, dtype=torch.float32, device=z.device)
        gV.index_add_(0, inv, x[:, None] * G[bag])
        for table, slots, g in ((self.w, self.w_slots, gw), (self.V, self.V_slots, gV)):
            rows = [table[touched]] + [s[touched] for s in slots.values()]
            self.rule.update_(*(rows + [None] * (3 - len(rows))), g, self.lr, self.optimizer_hp, True)
            for t, r in zip([table] + list(slots.values()), rows):
                t[touched] = r
        self._bopt.step([dz.sum().reshape(1)])
        return loss

    # ----------------------------------------------------------------- steps
    @torch.no_grad()
    def _train_step_fused(self, labels, offsets, ids, vals) -> torch.Tensor:
        """ffm_rows, the fixed-order sums, the one-writer table update over the bags and b's dense rule.  The
        returned loss is a copy: the plan's own is overwritten by the next step."""
        plan = self._native_plan()
        plan.rows(labels, offsets, ids, vals, 1.0 / labels.numel())
        loss, db = plan.sums()
        plan.update(offsets, ids, vals, self.rule.kind, self.lr, list(self.w_slots.values()),
                    list(self.V_slots.values()), **self.rule.native_kwargs(self.optimizer_hp))
        self._bopt.step([db])
        return loss.clone()

    def train_step(self, batch) -> torch.Tensor:
        labels, offsets, ids, vals = self._parts(batch)
        if not self._fused_ok():
            loss = self._train_step_general(labels, offsets, ids, vals)
        elif self._graphed is not None:
            if vals is None:
                vals = torch.ones(ids.numel(), dtype=torch.float32, device=self.device)
            self._native_plan().reserve(labels.numel(), ids.numel())       # the scratch never grows inside a capture
            loss = self._graphed(labels, offsets, ids, vals)
        else:
            loss = self._train_step_fused(labels, offsets, ids, vals)
        self.global_step += 1
        return loss

    def enable_graph(self, on: bool = True):
        """Replay each fused step as one captured hipGraph, captured per batch shape at its first use."""
        from ..utils.graphs import GraphedStep

        if not on:
            self._graphed = None
            return
        if not self._fused_ok():
            raise RuntimeError("graph capture needs the fused GPU step")
        self._graphed = GraphedStep(self._train_step_fused, self._state_tensors)

    def _state_tensors(self):
        """Everything a step mutates (restored after a capture's warmup)."""
        slots = list(self.w_slots.values()) + list(self.V_slots.values())
        bopt = [t for t in self._bopt.m + self._bopt.v if t is not None] + [self._bopt.step_t]
        return [self.w, self.V, self.b] + slots + bopt

    # ------------------------------------------------------------- evaluation
    # (evaluate / auc_update / evaluate_stream / auc / reset_auc: StreamingEvalMixin's, over the hooks below)
    def _eval_into(self, batch, record, reset: bool, want_pred: bool):
        labels, offsets, ids, vals = self._parts(batch)
        return self._native_plan().evaluate(labels, offsets, ids, vals, record, reset, want_pred,
                                            self._auc_rec.auc_bins)

    def _eval_general(self, batch):
        labels, offsets, ids, vals = self._parts(batch)
        return self._forward_general(offsets, ids, vals)[0], labels, ids

    @torch.no_grad()
    def predict(self, batch) -> torch.Tensor:
        return self.evaluate(batch)[1]

    def checkpoint_tensors(self):
        """(sharded, replicated) tensors under TF-style names; nothing is sharded here."""
        repl = {"ffm/linear": self.w, "ffm/factors": self.V, "ffm/bias": self.b,
                "global_step": torch.tensor(float(self.global_step))}
        for name, slots in (("ffm/linear", self.w_slots), ("ffm/factors", self.V_slots)):
            for sname, t in slots.items():
                repl[f"{name}/{sname}"] = t
        for sname, t in zip(self.rule.slots, (self._bopt.m[0], self._bopt.v[0])):
            repl[f"ffm/bias/{sname}"] = t
        return {}, repl
