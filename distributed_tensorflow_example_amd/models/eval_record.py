"""The evaluation record and the evaluation methods every model shares.

`EvalRecord` owns the int64 device record the forward-only evaluation kernels
add their batches to (csrc/kernels/eval_record.h is the same layout on the
native side):

    {loss sum (fp64 bits), rows, bad ids, pos[T + 1], neg[T + 1]}

with T = streaming_auc's num_thresholds.  No other module indexes a record by
number.

`StreamingEvalMixin` is evaluate / auc_update / evaluate_stream / auc /
reset_auc over three hooks of the model:

    _eval_fused_ok()                               one GPU, every table row local: the native kernels apply
    _eval_into(batch, record_tensor, reset, want_pred)   the native call; returns the probabilities [B] or None
    _eval_general(batch) -> (logits [B], labels [B], ids)   the routed forward (exact exchange), on self.device;
                                                   ids are read only where bad ids are reported
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops

_HEAD = 3      # loss sum, rows, bad ids; then the two histograms


class EvalRecord:
    def __init__(self, auc_bins: int, device):
        """streaming_auc's num_thresholds = auc_bins -> auc_bins + 1 histogram bins."""
        self.auc_bins = int(auc_bins)
        nb = self.auc_bins + 1
        self.tensor = torch.zeros(_HEAD + 2 * nb, dtype=torch.int64, device=device)
        self.pos, self.neg = self._histograms(self.tensor)      # views: the kernels add to them in place

    def _histograms(self, t):
        nb = self.auc_bins + 1
        return t[_HEAD:_HEAD + nb], t[_HEAD + nb:]

    def mean_loss(self, rows: int) -> torch.Tensor:
        """The loss sum over `rows` as a 0-d fp32 device value (no host read-back)."""
        return (self.tensor[:1].view(torch.float64) / rows).float()[0]

    def read(self):
        """(loss sum, rows, bad ids, pos, neg) on the host: one copy."""
        host = self.tensor.cpu()
        return (float(host[:1].view(torch.float64)[0]), int(host[1]), int(host[2])) + self._histograms(host)

    def zero_(self):
        self.tensor.zero_()

    def clone(self) -> torch.Tensor:
        """A snapshot of the record's int64 values (a tensor: comparable with torch.equal)."""
        return self.tensor.clone()


class StreamingEvalMixin:
    _eval_plan_attr = "_plan"          # where the model keeps its native plan once built
    _stream_reports_bad_ids = False    # evaluate_stream also returns "bad_ids"

    def _init_eval_records(self, auc_bins: int):
        # auc_pos / auc_neg are views of the model's own record: the fused evaluation adds to them in place
        self._auc_rec = EvalRecord(auc_bins, self.device)
        self.auc_pos, self.auc_neg = self._auc_rec.pos, self._auc_rec.neg
        self._eval_rec = self._stream_rec = None

    def fused_eval_runs(self) -> int:
        """Evaluations that ran on the one-GPU plan's forward-only kernels so far."""
        plan = getattr(self, self._eval_plan_attr, None)
        return int(plan.eval_runs()) if plan is not None else 0

    @torch.no_grad()
    def evaluate(self, batch):
        """(mean loss, probabilities [B]) of a batch without updating anything.
        Lookups use the exact exchange: evaluation batches need no fixed shapes.
        Collective: first applies any voided steps of the current window.  One
        worker on a GPU: the plan's two evaluation kernels, no routing."""
        self.sync_exchange()
        if self._eval_fused_ok() and _rows(batch) > 0:
            rec = self._eval_rec
            if rec is None:
                rec = self._eval_rec = EvalRecord(self._auc_rec.auc_bins, self.device)
            pred = self._eval_into(batch, rec.tensor, True, True)
            return rec.mean_loss(pred.numel()), pred
        logits, labels, _ = self._eval_general(batch)
        return ops.sigmoid_xent(logits, labels).detach(), torch.sigmoid(logits)

    @torch.no_grad()
    def auc_update(self, batch):
        """Add the batch's predictions to the streaming-AUC histograms."""
        self.sync_exchange()
        if _rows(batch) == 0:
            return
        if self._eval_fused_ok():
            # the record's loss sum / rows / bad ids ride along
            self._eval_into(batch, self._auc_rec.tensor, False, False)
            return
        logits, labels, _ = self._eval_general(batch)
        ops.auc_histogram_(torch.sigmoid(logits), labels, self.auc_pos, self.auc_neg)

    @torch.no_grad()
    def evaluate_stream(self, batches) -> dict:
        """{"loss", "auc", "rows"} (Wide&Deep: and "bad_ids") of an iterable of
        batches (this worker's): the mean loss over all rows and streaming_auc's
        value.  On one GPU every batch is added to one device record, read back
        once at the end; the model's own AUC histograms (auc_update / auc) are
        left alone.  Batches of no rows are skipped."""
        self.sync_exchange()
        if self._eval_fused_ok():
            rec = self._stream_rec
            if rec is None:
                rec = self._stream_rec = EvalRecord(self._auc_rec.auc_bins, self.device)
            first = True
            for batch in batches:
                if _rows(batch) > 0:
                    self._eval_into(batch, rec.tensor, first, False)
                    first = False
            if first:
                rec.zero_()
            loss_sum, rows, bad, pos, neg = rec.read()
        else:
            acc = EvalRecord(self._auc_rec.auc_bins, self.device)
            pos, neg = acc.pos, acc.neg
            rows, bad, total = 0, 0, torch.zeros((), dtype=torch.float64, device=self.device)
            for batch in batches:
                if _rows(batch) == 0:
                    continue
                logits, labels, ids = self._eval_general(batch)
                total += ops.sigmoid_xent(logits, labels, reduction="none").double().sum()
                ops.auc_histogram_(torch.sigmoid(logits), labels, pos, neg)
                if self._stream_reports_bad_ids:
                    bad += int(((ids < 0) | (ids >= self._route_table().num_rows)).sum())
                rows += labels.numel()
            loss_sum = float(total)
        out = {"loss": loss_sum / rows if rows else float("nan"), "auc": ops.auc_from_histograms(pos, neg),
               "rows": rows}
        if self._stream_reports_bad_ids:
            out["bad_ids"] = bad
        return out

    def auc(self, all_workers: bool = True) -> float:
        pos, neg = self.auc_pos.clone(), self.auc_neg.clone()
        if all_workers and self.world.world_size > 1:
            self.world.all_reduce(pos)
            self.world.all_reduce(neg)
        return ops.auc_from_histograms(pos, neg)

    def reset_auc(self):
        self.auc_pos.zero_()
        self.auc_neg.zero_()


def _rows(batch) -> int:
    labels = batch.labels if hasattr(batch, "labels") else batch[0]
    return int(labels.numel() if torch.is_tensor(labels) else np.asarray(labels).size)


def _dev(t, dev, dtype):
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    return t.to(dev, dtype).contiguous()
