"""Cost of evaluating the Wide&Deep model on one GPU, through WideDeep's public
interface only:

    python scripts/bench_wide_deep_eval.py [--features 100000000] [--rounds 3] [--out FILE]

The README's Wide&Deep configuration: F = 1e8 features, D = 64, tower
512-256-1, about 40 ids per row (Zipf), device-resident batches of 4096 and 500
rows.  Two variants, measured in alternating fresh child processes, `--rounds`
each: this tree (the fused forward-only kernel, csrc/kernels/wide_deep_eval.hip)
and this tree with DTF_WD_EVAL_FUSED=0 (the general path: the training router,
two bag kernels through a remap, one gemm per tower layer, head, sigmoid, loss
and histogram kernels).  The general path is the baseline: before the fused
kernel there was no evaluation to time.

Per variant, device time (events) of `evaluate` and `auc_update` per batch, and
of one `evaluate_stream` over 16 batches (wall clock: it ends in its read-back).
Medians over the rounds with min / max; one JSON document.

Sanity floor for the fused path: the tower is 2 B (64 * 512 + 512 * 256 + 256)
= 1.34 GFLOP at B = 4096; at the exact-fp32 matrix rate of an MI355X (155 TF)
that is about 9 us.  The floor does not count the bag reads (4096 rows x 40
ids x 256 B = 42 MB of random rows).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np


def _batch(rng, B, F, per=40):
    k = rng.integers(per // 2, per * 3 // 2 + 1, B)
    off = np.zeros(B + 1, np.int64)
    np.cumsum(k, out=off[1:])
    n = int(off[-1])
    ids = np.minimum(rng.zipf(1.2, n) - 1, F - 1).astype(np.int64)
    return ((rng.random((B, 1)) < 0.3).astype(np.float32), off, ids, rng.random(n).astype(np.float32))


def _device_ms(torch, fn, reps=20, warmup=5, inner=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return float(np.median(out))


def _wall_ms(torch, fn, reps=10, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def worker(tree, F):
    sys.path.insert(0, tree)
    import torch

    from distributed_tensorflow_example_amd.models.wide_deep import WideDeep
    from distributed_tensorflow_example_amd.parallel.world import World

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    m = WideDeep(F, emb_dim=64, hidden=(512, 256), lr=0.05, dense_opt="adam", dense_lr=1e-3, world=World(device=dev))
    res = {"fused": bool(m._eval_fused_ok())}
    stream = [tuple(torch.from_numpy(a).to(dev) for a in _batch(rng, 4096, F)) for _ in range(16)]
    d500 = tuple(torch.from_numpy(a).to(dev) for a in _batch(rng, 500, F))
    for name, b in (("4096", stream[0]), ("500", d500)):
        res[f"evaluate_dev_{name}_device_ms"] = _device_ms(torch, lambda b=b: m.evaluate(b))
        res[f"auc_update_dev_{name}_device_ms"] = _device_ms(torch, lambda b=b: m.auc_update(b))
    res["evaluate_stream_16x4096_wall_ms"] = _wall_ms(torch, lambda: m.evaluate_stream(stream))
    st = m.evaluate_stream(stream)
    res["stream_loss"], res["stream_auc"], res["stream_rows"] = st["loss"], st["auc"], st["rows"]
    res["fused_eval_runs"] = int(m.fused_eval_runs())
    props = torch.cuda.get_device_properties(0)
    res["box"] = f"{socket.gethostname()}: {props.name}, {props.gcnArchName}, {props.multi_processor_count} CUs"
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.features)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    variants = [("fused", here, {"DTF_WD_EVAL_FUSED": "1"}), ("general_path", here, {"DTF_WD_EVAL_FUSED": "0"})]
    runs = {name: [] for name, _, _ in variants}
    for r in range(a.rounds):
        # alternating: one process per variant per round, the order reversed every other round
        for name, tree, env in (variants if r % 2 == 0 else variants[::-1]):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, "--features",
                                str(a.features)], capture_output=True, text=True, env=dict(os.environ, **env),
                               timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                raise SystemExit(f"{name} round {r} failed:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            runs[name].append(json.loads(line[-1][7:]))
            print(name, r, line[-1][7:], flush=True)
    out = {"features": a.features, "emb_dim": 64, "tower": "512-256-1", "rounds": a.rounds, "ids_per_row": 40,
           "tower_gflop_at_4096": round(2 * 4096 * (64 * 512 + 512 * 256 + 256) / 1e9, 3),
           "fp32_mfma_floor_us_at_4096": round(2 * 4096 * (64 * 512 + 512 * 256 + 256) / 155e12 * 1e6, 2),
           "variants": {}}
    for name, rs in runs.items():
        v = {}
        for k in rs[0]:
            xs = [x[k] for x in rs]
            if k.endswith("_ms"):
                v[k] = {"median": round(float(np.median(xs)), 5), "min": round(min(xs), 5), "max": round(max(xs), 5)}
            else:
                v[k] = xs[-1]
        out["variants"][name] = v
    f, g = out["variants"]["fused"], out["variants"]["general_path"]
    out["box"] = f["box"]
    out["general_over_fused"] = {k: round(g[k]["median"] / f[k]["median"], 2) for k in f if k.endswith("_ms")}
    # faster by more than the spread: the fused path's slowest run under the general path's fastest
    out["fused_faster_beyond_spread"] = {k: bool(f[k]["max"] < g[k]["min"]) for k in f if k.endswith("_ms")}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
