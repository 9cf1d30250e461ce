"""DeepFM (Guo et al. 2017) on libsvm / CTR batches: a factorization machine and an MLP tower
that read the same factor table.

Two forms.  Without fields (num_fields None) the batches are CSR rows, and the tower reads the
pooled factors S_r (as models/wide_deep.py's tower reads its sum-combined bag).  With
num_fields = P the batches are models/ffm.py's bag form (labels [B], offsets [B * P + 1], ids,
vals; `ffm_batch` makes it from a field per entry), entries of one bag are sum-pooled, and the
tower reads the concatenation of the P per-field embeddings, as the paper's does:

    A_r[p] = sum_{i in bag (r, p)} x_i V[id_i, :]       a_0 = [A_r[0] | ... | A_r[P-1]]   (P * K wide)
    demb[r P + p, :] = dz_r S_r + da_0,r[p K : (p + 1) K]     dL/dV[j,f] = sum_occ x demb[bag_occ, f] - V[j,f] q_j

with S, Q and the FM term over all of the row's entries, as without fields:

    S_r[f] = sum_i x_i V[id_i, f]        Q_r[f] = sum_i x_i^2 V[id_i, f]^2
    fm_r   = sum_i x_i w[id_i] + 0.5 sum_f (S_r[f]^2 - Q_r[f])
    a_0    = S_r;   a_l = relu(a_{l-1} W_{l-1} + b_{l-1}), l = 1 .. nh;   t_r = a_nh . w_last + b_last
    z_r    = (fm_r + t_r) + b           loss = mean_r sigmoid_xent(z_r, y_r)

With dz_r = (sigmoid(z_r) - y_r) / B:

    da_nh = dz w_last^T;   dzl[l] = da_l * (a_l > 0);   da_{l-1} = dzl[l] W_{l-1}^T
    demb_r = dz_r S_r + da_0,r
    dL/dw[j]   = sum_occ x dz_r
    dL/dV[j,f] = sum_occ x demb_r[f] - V[j,f] q_j,   q_j = sum_occ x^2 dz_r
    dW_l = a_l^T dzl[l+1];  db_l = sum_r dzl[l+1];  dw_last = a_nh^T dz;  db_last = db = sum_r dz

The tables take FMTrainer's row-local rule, the tower `dense_optimizer` (a fused optimizer of
optim/), b the dense form of the tables' rule as in FMTrainer.

One GPU: the step is dfm_rows (csrc/kernels/deepfm.hip; with fields dfmf_rows,
csrc/kernels/deepfm_fields.hip: bags, tower, head and the backward through
the tower in one launch), a gemm and a col_sum per layer for the weight gradients, the fixed-order
sums, fm.hip's one-writer table update and the two dense optimizer launches; evaluation is dfm_rows
plus the evaluation record's reduce.  On the CPU, or with DTF_DFM_FUSED=0, a short torch fp32 path
computes the same closed form without autograd.  Tables are not sharded: world_size > 1 is refused.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch

from .. import ops, optim
from .fm import FMTrainer


class DeepFMTrainer(FMTrainer):
    def __init__(self, num_features: int, factors: int = 8, hidden: Sequence[int] = (256, 128),
                 dense_optimizer: str = "adam", dense_lr: Optional[float] = None, dense_hp: Optional[dict] = None,
                 num_fields: Optional[int] = None, **fm):
        """fm: FMTrainer's keyword arguments (lr, world, seed, device, init_std, optimizer, optimizer_hp,
        auc_bins); dense_lr None: lr.  num_fields P: the tower reads P concatenated per-field embeddings and the
        batches are in the bag form (offsets [B * P + 1]); None: the pooled factors, CSR rows."""
        super().__init__(num_features, factors, **fm)
        self.hidden = tuple(int(h) for h in hidden)
        if not self.hidden or min(self.hidden) < 1:
            raise ValueError("DeepFMTrainer: hidden must name at least one positive width")
        if num_fields is not None and int(num_fields) < 1:
            raise ValueError("DeepFMTrainer: num_fields must be at least 1 (None: no fields)")
        self.num_fields = None if num_fields is None else int(num_fields)
        g = torch.Generator().manual_seed(int(fm.get("seed", 1)) + 2)       # the tower as WideDeep initialises its own
        dims = [self.factors * (self.num_fields or 1)] + list(self.hidden) + [1]
        self.layers = []
        for i in range(len(dims) - 1):
            w = torch.randn(dims[i], dims[i + 1], generator=g) * (2.0 / dims[i]) ** 0.5
            self.layers += [w.to(self.device), torch.zeros(dims[i + 1], dtype=torch.float32, device=self.device)]
        # the tower's gradients are views of one bucket (written with beta = 0 every step), then b's
        flat = torch.zeros(sum(p.numel() for p in self.layers) + 1, dtype=torch.float32, device=self.device)
        self.layer_grads, off = [], 0
        for p in self.layers:
            self.layer_grads.append(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        self._db = flat[off:off + 1]
        self.dense_optimizer, self.dense_hp = dense_optimizer, dict(dense_hp or {})
        self.dense_lr = self.lr if dense_lr is None else float(dense_lr)
        self._dopt = optim.fused(dense_optimizer, self.layers, self.dense_lr, **self.dense_hp)

    # ----------------------------------------------------------------- plumbing
    def _fused_ok(self) -> bool:
        """One worker on a GPU and a shape dfm_rows takes: the step and the evaluation run on
        csrc/kernels/deepfm.hip.  DTF_DFM_FUSED=0 keeps the torch path."""
        ok = self._fused
        if ok is None:
            ok = self.device.type == "cuda" and os.environ.get("DTF_DFM_FUSED", "1") != "0"
            if ok:
                from .. import _native
                if not _native.load().DeepFMPlan.supported(self.factors, list(self.hidden), self.num_fields or 0):
                    raise ValueError(f"DeepFMTrainer: the fused step takes factors a multiple of 4 in 4 .. 128, 1 to "
                                     f"3 hidden widths, multiples of 16 up to 512, and at most 64 fields with fields * "
                                     f"factors <= 512, not {self.factors} / {self.hidden} / {self.num_fields} "
                                     f"(DTF_DFM_FUSED=0 runs the torch path)")
            self._fused = ok
        return ok

    _eval_fused_ok = _fused_ok

    def _native_plan(self):
        if self._plan is None:
            from .. import _native
            self._plan = _native.load().DeepFMPlan(self.w, self.V, self.layers, self.b,     # the tensors themselves
                                                   num_fields=self.num_fields or 0)
        return self._plan

    def _parts(self, batch):
        labels, offsets, ids, vals = super()._parts(batch)
        if self.num_fields is not None and offsets.numel() != labels.numel() * self.num_fields + 1:
            raise ValueError("DeepFMTrainer: with num_fields, offsets must hold B * num_fields + 1 entries, one bag per "
                             "(row, field); ffm_batch makes them from a field per entry")
        return labels, offsets, ids, vals

    # ----------------------------------------------------------------- the torch path
    def _forward_general(self, offsets, ids, vals):
        """FMTrainer's tuple with the tower's score added to z, then the activations [a_0, ..., a_nh] and the bag of
        each kept entry: a_0 = S and the entry's row, or with fields the [B, P * K] concatenation and bag r * P + p."""
        P = self.num_fields
        z, S, row, idk, x = super()._forward_general(offsets if P is None else offsets[::P], ids, vals)
        a0, bag = S, row
        if P is not None:
            nb = offsets.numel() - 1
            bag = torch.repeat_interleave(torch.arange(nb, device=ids.device), torch.diff(offsets))
            bag = bag[(ids >= 0) & (ids < self.num_features)]
            a0 = torch.zeros(nb, self.factors, dtype=torch.float32, device=ids.device)
            a0 = a0.index_add_(0, bag, self.V[idk] * x[:, None]).view(nb // P, P * self.factors)
        acts = [a0]
        for l in range(len(self.hidden)):
            acts.append(torch.relu(acts[-1] @ self.layers[2 * l] + self.layers[2 * l + 1]))
        t = acts[-1] @ self.layers[-2] + self.layers[-1]
        return z + t.reshape(-1), S, row, idk, x, acts, bag

    @torch.no_grad()
    def _train_step_general(self, labels, offsets, ids, vals) -> torch.Tensor:
        z, S, row, idk, x, acts, bag = self._forward_general(offsets, ids, vals)
        loss = ops.sigmoid_xent(z, labels)
        dz = (torch.sigmoid(z) - labels) / labels.numel()
        # the tower's backward: the gradient at each pre-activation, the weight gradients, da_0
        nl = len(self.layers) // 2
        g = dz[:, None]
        grads = [None] * (2 * nl)
        for l in range(nl - 1, -1, -1):
            grads[2 * l], grads[2 * l + 1] = acts[l].t() @ g, g.sum(0)
            g = g @ self.layers[2 * l].t()
            if l > 0:
                g = g * (acts[l] > 0)
        if self.num_fields is None:
            demb = dz[:, None] * S + g
        else:                                                       # [B * P, K]: dz S on every block of da_0
            demb = ((dz[:, None] * S)[:, None, :] + g.view(-1, self.num_fields, self.factors)).reshape(-1, self.factors)
        touched, inv = torch.unique(idk, return_inverse=True)
        xdz = x * dz[row]
        gw = torch.zeros(touched.numel(), dtype=torch.float32, device=z.device).index_add_(0, inv, xdz)
        q = torch.zeros_like(gw).index_add_(0, inv, x * xdz)
        gV = torch.zeros(touched.numel(), self.factors, dtype=torch.float32, device=z.device)
        gV.index_add_(0, inv, x[:, None] * demb[bag])
        gV -= self.V[touched] * q[:, None]
        for table, slots, gt in ((self.w, self.w_slots, gw), (self.V, self.V_slots, gV)):
            rows = [table[touched]] + [s[touched] for s in slots.values()]
            self.rule.update_(*(rows + [None] * (3 - len(rows))), gt, self.lr, self.optimizer_hp, True)
            for t, r in zip([table] + list(slots.values()), rows):
                t[touched] = r
        self._bopt.step([dz.sum().reshape(1)])
        self._dopt.step(grads)
        return loss

    # ----------------------------------------------------------------- the fused step
    @torch.no_grad()
    def _train_step_fused(self, labels, offsets, ids, vals) -> torch.Tensor:
        """dfm_rows (with fields: dfmf_rows), the weight gradients (beta = 0) by the general path's gemm / col_sum launches, the fixed-order
        sums, the one-writer table update and the dense rules: no router, dedup or autograd.  The returned loss
        is a copy: the plan's own is overwritten by the next step."""
        from .. import _native
        C = _native.load()
        plan = self._native_plan()
        plan.rows(labels, offsets, ids, vals, 1.0 / labels.numel())
        nl = len(self.layers) // 2
        for l in range(nl - 1):
            dzl = plan.dzl(l + 1)
            C.gemm(plan.act(l), True, dzl, False, self.layer_grads[2 * l], None, 0, 1.0, 0.0, None)
            C.col_sum(dzl, self.layer_grads[2 * l + 1])
        C.gemm(plan.act(nl - 1), True, plan.dz(), False, self.layer_grads[-2], None, 0, 1.0, 0.0, None)
        loss = plan.sums(self.layer_grads[-1], self._db)            # mean loss; sum(dz) -> both biases' gradients
        plan.update(offsets, ids, vals, self.rule.kind, self.lr, list(self.w_slots.values()),
                    list(self.V_slots.values()), **self.rule.native_kwargs(self.optimizer_hp))
        self._bopt.step([self._db])
        self._dopt.step(self.layer_grads)
        return loss.clone()

    def _state_tensors(self):
        """Everything a step mutates (restored after a capture's warmup)."""
        dopt = [t for t in self._dopt.m + self._dopt.v if t is not None] + [self._dopt.step_t]
        return super()._state_tensors() + self.layers + dopt

    def checkpoint_tensors(self):
        """FMTrainer's names, and the tower under deepfm/."""
        local, repl = super().checkpoint_tensors()
        nl = len(self.layers) // 2
        names = [f"deepfm/{'logits' if l == nl - 1 else f'hidden_{l}'}/{k}" for l in range(nl) for k in ("kernel", "bias")]
        for i, (name, p) in enumerate(zip(names, self.layers)):
            repl[name] = p
            for sname, t in zip(self._dopt.rule.slots, (self._dopt.m[i], self._dopt.v[i])):
                repl[f"{name}/{sname}"] = t
        return local, repl
