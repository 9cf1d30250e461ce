"""Second-order factorization machine (Rendle 2010) on libsvm / CTR batches.

    S_r[f] = sum_i x_i V[id_i, f]          Q_r[f] = sum_i x_i^2 V[id_i, f]^2
    z_r    = b + sum_i x_i w[id_i] + 0.5 * sum_f (S_r[f]^2 - Q_r[f])
    loss   = mean_r sigmoid_xent(z_r, y_r)

Sums over i run over row r's entries; a repeated id counts once per occurrence;
ids outside [0, F) are skipped.  With dz_r = (sigmoid(z_r) - y_r) / B the
gradient of a table row j is

    dL/dw[j]   = sum_{occ of j} x dz_r
    dL/dV[j,f] = sum_{occ of j} x dz_r S_r[f]  -  V[j,f] q_j,      q_j = sum_{occ of j} x^2 dz_r
    dL/db      = sum_r dz_r

and every touched row takes one update of a row-local rule of optim/rules.py
(sgd, momentum, adagrad, rmsprop, ftrl) with its duplicate-summed gradient, as
TensorFlow applies an IndexedSlices gradient; b takes the dense form of the rule.

One GPU: the step is three launches of csrc/kernels/fm.hip around one sort
(FMPlan.rows, .sums, .update) plus the bias rule, and evaluation is fm_rows plus
the evaluation record's reduce.  On the CPU, or with DTF_FM_FUSED=0, a short
torch fp32 path computes the same thing (index_add_ for the bags, the closed
form above, the rules' torch form).  Tables are not sharded: world_size > 1 is
refused.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from .. import ops, optim
from ..optim.rules import RULES
from ..parallel.world import World, get_world
from .eval_record import StreamingEvalMixin, _dev


class FMTrainer(StreamingEvalMixin):
    _stream_reports_bad_ids = True

    def __init__(self, num_features: int, factors: int = 8, lr: float = 0.01, world: Optional[World] = None,
                 seed: int = 1, device=None, init_std: float = 0.01, optimizer: str = "sgd",
                 optimizer_hp: Optional[dict] = None, auc_bins: int = 200):
        rule = RULES.get(optimizer)
        if rule is None or not rule.row_local:
            raise ValueError(f"FMTrainer: optimizer must be one of {[n for n, r in RULES.items() if r.row_local]}, "
                             f"not '{optimizer}'")
        self.world = world or get_world()
        if self.world.world_size > 1:
            raise ValueError("FMTrainer: sharded FM tables are not built; train on one worker (world_size == 1)")
        self.device = torch.device(device) if device is not None else self.world.device
        self.num_features, self.factors, self.lr = int(num_features), int(factors), float(lr)
        self.optimizer, self.optimizer_hp, self.rule = optimizer, dict(optimizer_hp or {}), rule
        rule.hp(self.optimizer_hp)                     # checked as TF's constructor checks them
        f32 = dict(dtype=torch.float32, device=self.device)
        self.w = torch.zeros(self.num_features, **f32)
        self.V = torch.empty(self.num_features, self.factors, **f32)
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
        """One worker on a GPU and factors the kernels take: the step and the evaluation run on
        csrc/kernels/fm.hip.  DTF_FM_FUSED=0 keeps the torch path."""
        ok = self._fused
        if ok is None:
            ok = self.device.type == "cuda" and os.environ.get("DTF_FM_FUSED", "1") != "0"
            if ok:
                from .. import _native
                if not _native.load().FMPlan.supported(self.factors):
                    raise ValueError(f"FMTrainer: the fused step takes factors a multiple of 4 in 4 .. 128, not "
                                     f"{self.factors} (DTF_FM_FUSED=0 runs the torch path)")
            self._fused = ok
        return ok

    _eval_fused_ok = _fused_ok

    def _native_plan(self):
        if self._plan is None:
            from .. import _native
            self._plan = _native.load().FMPlan(self.w, self.V, self.b)     # the tensors themselves, not copies
        return self._plan

    def _parts(self, batch):
        labels, offsets, ids, vals = batch.to(self.device) if hasattr(batch, "to") else batch
        dev = self.device
        return (_dev(labels, dev, torch.float32).reshape(-1), _dev(offsets, dev, torch.int64),
                _dev(ids, dev, torch.int64), None if vals is None else _dev(vals, dev, torch.float32))

    # ----------------------------------------------------------------- the torch path
    def _forward_general(self, offsets, ids, vals):
        """(z [B], S [B, K], row of each kept entry, its id, its value): fp32 torch."""
        B = offsets.numel() - 1
        row = torch.repeat_interleave(torch.arange(B, device=ids.device), torch.diff(offsets))
        ok = (ids >= 0) & (ids < self.num_features)
        row, idk = row[ok], ids[ok]
        x = torch.ones(idk.numel(), dtype=torch.float32, device=ids.device) if vals is None else vals[ok]
        xv = self.V[idk] * x[:, None]
        S = torch.zeros(B, self.factors, dtype=torch.float32, device=ids.device).index_add_(0, row, xv)
        Q = torch.zeros_like(S).index_add_(0, row, xv * xv)
        lin = torch.zeros(B, dtype=torch.float32, device=ids.device).index_add_(0, row, self.w[idk] * x)
        return self.b + lin + 0.5 * (S * S - Q).sum(1), S, row, idk, x

    @torch.no_grad()
    def _train_step_general(self, labels, offsets, ids, vals) -> torch.Tensor:
        z, S, row, idk, x = self._forward_general(offsets, ids, vals)
        loss = ops.sigmoid_xent(z, labels)
        dz = (torch.sigmoid(z) - labels) / labels.numel()
        touched, inv = torch.unique(idk, return_inverse=True)
        xdz = x * dz[row]
        gw = torch.zeros(touched.numel(), dtype=torch.float32, device=z.device).index_add_(0, inv, xdz)
        q = torch.zeros_like(gw).index_add_(0, inv, x * xdz)
        gV = torch.zeros(touched.numel(), self.factors, dtype=torch.float32, device=z.device)
        gV.index_add_(0, inv, xdz[:, None] * S[row])
        gV -= self.V[touched] * q[:, None]
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
        """fm_rows, the fixed-order sums, the one-writer table update and b's dense rule: no router, dedup or
        autograd.  The returned loss is a copy: the plan's own is overwritten by the next step."""
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
        repl = {"fm/linear": self.w, "fm/factors": self.V, "fm/bias": self.b,
                "global_step": torch.tensor(float(self.global_step))}
        for name, slots in (("fm/linear", self.w_slots), ("fm/factors", self.V_slots)):
            for sname, t in slots.items():
                repl[f"{name}/{sname}"] = t
        for sname, t in zip(self.rule.slots, (self._bopt.m[0], self._bopt.v[0])):
            repl[f"fm/bias/{sname}"] = t
        return {}, repl
