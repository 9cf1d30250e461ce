#!/usr/bin/env python3
"""Forward and backward time of one layer's self-attention: ops.transformer.fused_attention
against the composed path of models/bert.py BertLayer.forward (bias add, two batched
GEMMs, the softmax kernel, permute copies), each in a fresh process.

    python scripts/bench_attention.py --S 512 --batch 32 [--heads 12] [--p 0.1] [--path both]

Event-timed over --iters launches after --warmup; one JSON line per run with the
forward / backward microseconds, the bf16 MFMA FLOP rate of each (forward
4 B NH S^2 64, backward 10 B NH S^2 64) and the peak memory above the inputs.
"""
import argparse
import json
import math
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def composed(T, torch, qkv, bias, mask, nh, scale, p):
    B, S, H3 = qkv.shape
    d = H3 // (3 * nh)
    x = (qkv + bias.to(qkv.dtype)).view(B, S, 3, nh, d)
    q, k, v = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 3, 1), x[:, :, 2].permute(0, 2, 1, 3)
    probs = T.attention_softmax(torch.matmul(q, k), mask, scale, p, True)
    return torch.matmul(probs.to(v.dtype), v).permute(0, 2, 1, 3).reshape(B, S, nh * d)


def run(a):
    import torch
    from distributed_tensorflow_example_amd.ops import transformer as T

    B, S, nh = a.batch, a.S, a.heads
    scale = 1.0 / math.sqrt(64)
    torch.manual_seed(0)
    qkv = torch.randn(B, S, 3 * nh * 64, device="cuda").bfloat16().requires_grad_()
    bias = (torch.randn(3 * nh * 64, device="cuda") * 0.3).requires_grad_()
    mask = torch.zeros(B, S, device="cuda")
    mask[:, S - S // 8:] = -10000.0
    dy = torch.randn(B, S, nh * 64, device="cuda").bfloat16()
    if a.path == "fused":
        if not T.attention_supported(S, 64):
            raise SystemExit("fused attention does not support S=%d in this process" % S)
        fn = lambda: T.fused_attention(qkv, bias, mask, nh, scale, a.p)
    else:
        fn = lambda: composed(T, torch, qkv, bias, mask, nh, scale, a.p)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fwd = bwd = 0.0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for it in range(a.warmup + a.iters):
        qkv.grad = bias.grad = None
        ev[0].record()
        out = fn()
        ev[1].record()
        out.backward(dy)
        ev[2].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            fwd += ev[0].elapsed_time(ev[1])
            bwd += ev[1].elapsed_time(ev[2])
    fwd_us, bwd_us = 1e3 * fwd / a.iters, 1e3 * bwd / a.iters
    flop = B * nh * S * S * 64.0
    print(json.dumps(dict(bench="attention", path=a.path, S=S, batch=B, heads=nh, p=a.p, iters=a.iters,
                          fwd_us=round(fwd_us, 1), bwd_us=round(bwd_us, 1),
                          fwd_tflops=round(4 * flop / fwd_us / 1e6, 1), bwd_tflops=round(10 * flop / bwd_us / 1e6, 1),
                          peak_extra_mb=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--S", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--path", choices=["fused", "composed", "both"], default="both")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.path != "both":
        return run(a)
    for path in ("fused", "composed"):          # a fresh process each
        argv = [sys.executable, os.path.abspath(__file__), "--path", path] + [
            "--%s=%s" % (k, getattr(a, k)) for k in ("S", "batch", "heads", "p", "iters", "warmup")]
        r = subprocess.run(argv, cwd=REPO)
        if r.returncode != 0:
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
