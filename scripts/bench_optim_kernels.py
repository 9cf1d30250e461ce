#!/usr/bin/env python
"""Time the two optimizer kernels alone, one JSON line per case.

  dense: FusedAdamW.step over BERT-base's parameter set, bf16 gradients and bf16
         shadows (multi_tensor_apply; the step also bumps the device step count,
         a one-element kernel)
  rows:  sparse_rows_apply, Adagrad, a [1e6, 64] table, 163,840 touched rows
         (Wide&Deep's B = 4096 x 40 ids)

Device events around `--launches` back-to-back launches after a warm-up; only
calls that both sides of a refactor share, so the same file times either build."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_tensorflow_example_amd import _native, optim  # noqa: E402


def bert_base_shapes(vocab=30522, hidden=768, layers=12, inter=3072, pos=512):
    ln = [(hidden,), (hidden,)]
    emb = [(vocab, hidden), (pos, hidden), (2, hidden)] + ln
    layer = [(hidden, hidden), (hidden,)] * 4 + ln + [(hidden, inter), (inter,), (inter, hidden), (hidden,)] + ln
    return emb + layer * layers + [(hidden, hidden), (hidden,)]


def timed(fn, launches, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches       # us per launch


def dense(launches):
    g = torch.Generator(device="cuda").manual_seed(0)
    ps = [torch.randn(s, device="cuda", generator=g) * 0.02 for s in bert_base_shapes()]
    grads = [(torch.randn(p.shape, device="cuda", generator=g) * 1e-3).bfloat16() for p in ps]
    opt = optim.FusedAdamW(ps, 1e-4)
    for p in ps:
        opt.attach_shadow(p, torch.empty_like(p, dtype=torch.bfloat16))
    us = timed(lambda: opt.step(grads), launches)
    return {"case": "dense_adamw_bert_base_bf16grad_shadow", "elements": sum(p.numel() for p in ps), "us": us}


def rows(launches, R=1_000_000, D=64, n=163_840):
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn(R, D, device="cuda", generator=g)
    acc = torch.full_like(table, 0.1)
    idx = torch.randperm(R, device="cuda", generator=g)[:n].contiguous()
    grad = torch.randn(n, D, device="cuda", generator=g)
    C = _native.load()
    us = timed(lambda: C.sparse_rows_apply(table, acc, None, idx, grad, 4, 0.05), launches)
    return {"case": "rows_adagrad_1e6x64_163840", "touched_rows": n, "us": us}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    for case in (dense, rows):
        print(json.dumps({"tag": a.tag, **case(a.launches), "launches": a.launches}), flush=True)
