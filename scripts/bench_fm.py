"""Cost of a factorization-machine training step and evaluation on one GPU, through FMTrainer's public interface:

    python scripts/bench_fm.py [--features 100000000] [--rounds 3] [--out FILE] [--hidden 512,256] [--fields 22]
                               [--tower-fields 39]

F = 1e8 features, K = 64 factors, about 40 ids per row (Zipf-hot), SGD, device-resident batches of 500 and 4096
rows.  Two variants, measured in alternating fresh child processes, `--rounds` each: the fused path
(csrc/kernels/fm.hip) and the same build with DTF_FM_FUSED=0 (the torch path: gathers, index_add_, unique and
indexed writes).  The torch path is the baseline: before the kernels there was no factorization machine to time.

Per variant and batch size, the time between two events on the stream around 10 host-issued calls, per call, of
`train_step` eager, of `train_step` replayed as a captured graph (fused only) and of `evaluate`.  That is wall time on
the stream: gaps in which the device waits for the host's next launch are inside it, so an eager figure is an upper
bound on the kernels' time; no kernel trace is taken here.  The fused worker also times `evaluate` at each forced
rows-per-wave of fm_rows (FMPlan.set_rpw) next to the automatic pick.  Medians over the rounds with min / max; one
JSON document.

--hidden W1,W2,..: the same for DeepFM (models/deepfm.py DeepFMTrainer with that tower, csrc/kernels/deepfm.hip):
its fused path against its torch path (DTF_DFM_FUSED=0, the baseline: there was no DeepFM before), and the plain
fused FM step next to both; no rows-per-wave sweep.  The record then also lists every run of every variant.

--fields P: the same for the field-aware FM (models/ffm.py FFMTrainer with P fields of K = 4 factors,
csrc/kernels/ffm.hip): one entry per field and row (Zipf-hot ids), the batch in the (row, field) bag form; its fused
path against its torch path (DTF_FFM_FUSED=0, the baseline: there was no FFM before); no rows-per-wave sweep, and the
record lists every run.

--tower-fields P (with --hidden): DeepFM with fields (DeepFMTrainer(num_fields=P) with K = 8 factors,
csrc/kernels/deepfm_fields.hip): one entry per field and row, the batch in the bag form; its fused path against its
torch path (DTF_DFM_FUSED=0, the baseline: there was no field form before) and, for context, the pooled DeepFM at
K = 64 of the same build and tower (its own batches of about 40 ids per row).  The record lists every run.

What a step must move at B = 4096: 4096 x 40 table rows x 256 B = 42 MB of random 256-byte reads in fm_rows, and
per distinct id one 256-byte read and write in the update.
"""
import argparse
import json
import os
import socket
import subprocess
import sys

import numpy as np

RPWS = (1, 2, 4, 8)


def _batch(rng, B, F, per=40):
    k = rng.integers(per // 2, per * 3 // 2 + 1, B)
    off = np.zeros(B + 1, np.int64)
    np.cumsum(k, out=off[1:])
    n = int(off[-1])
    ids = np.minimum(rng.zipf(1.2, n) - 1, F - 1).astype(np.int64)
    return ((rng.random(B) < 0.3).astype(np.float32), off, ids, rng.uniform(0.5, 1.5, n).astype(np.float32))


def _ffm_batch(rng, B, F, P):
    """One entry per (row, field) bag."""
    n = B * P
    ids = np.minimum(rng.zipf(1.2, n) - 1, F - 1).astype(np.int64)
    return ((rng.random(B) < 0.3).astype(np.float32), np.arange(n + 1, dtype=np.int64), ids,
            rng.uniform(0.5, 1.5, n).astype(np.float32))


def _stream_ms(torch, fn, reps=20, warmup=5, inner=10):
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


def worker(tree, F, hidden=(), fields=0, tower_fields=0):
    sys.path.insert(0, tree)
    import torch

    from distributed_tensorflow_example_amd.models import DeepFMTrainer, FFMTrainer, FMTrainer
    from distributed_tensorflow_example_amd.parallel.world import World

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    if fields:
        m = FFMTrainer(F, num_fields=fields, factors=4, lr=0.05, world=World(device=dev))
    elif tower_fields:
        m = DeepFMTrainer(F, factors=8, hidden=hidden, num_fields=tower_fields, lr=0.05, world=World(device=dev))
        fields = tower_fields                      # the batches: one entry per (row, field) bag
    elif hidden:
        m = DeepFMTrainer(F, factors=64, hidden=hidden, lr=0.05, world=World(device=dev))
    else:
        m = FMTrainer(F, factors=64, lr=0.05, world=World(device=dev))
    res = {"fused": bool(m._fused_ok())}
    batches = {B: tuple(torch.from_numpy(a).to(dev) for a in (_ffm_batch(rng, B, F, fields) if fields else _batch(rng, B, F)))
               for B in (500, 4096)}
    for B, b in batches.items():
        res[f"train_step_eager_{B}_event_ms"] = _stream_ms(torch, lambda b=b: m.train_step(b))
        res[f"evaluate_{B}_event_ms"] = _stream_ms(torch, lambda b=b: m.evaluate(b))
    if res["fused"]:
        plan = m._native_plan()
        for B, b in ({} if hidden or fields else batches).items():     # (the plain FM only)
            res[f"rpw_auto_{B}"] = int(plan.rpw_for(B))
            for r in RPWS:
                plan.set_rpw(r)
                res[f"evaluate_{B}_rpw{r}_event_ms"] = _stream_ms(torch, lambda b=b: m.evaluate(b))
            plan.set_rpw(0)
        m.enable_graph()
        for B, b in batches.items():
            res[f"train_step_graph_{B}_event_ms"] = _stream_ms(torch, lambda b=b: m.train_step(b))
    props = torch.cuda.get_device_properties(0)
    res["box"] = f"{socket.gethostname()}: {props.name}, {props.gcnArchName}, {props.multi_processor_count} CUs"
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="")
    ap.add_argument("--hidden", default="", help="DeepFM's hidden widths, e.g. 512,256 (default: the plain FM)")
    ap.add_argument("--fields", type=int, default=0, help="the field-aware FM with this many fields of 4 factors")
    ap.add_argument("--tower-fields", type=int, default=0,
                    help="with --hidden: DeepFM whose tower reads this many concatenated fields of 8 factors")
    a = ap.parse_args()
    if a.tower_fields and (not a.hidden or a.fields):
        raise SystemExit("--tower-fields goes with --hidden and without --fields")
    if a.worker:
        return worker(a.worker, a.features, tuple(int(h) for h in a.hidden.split(",") if h), a.fields, a.tower_fields)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    variants = [("fused", {"DTF_FM_FUSED": "1"}, ""), ("general_path", {"DTF_FM_FUSED": "0"}, "")]
    if a.hidden:
        variants = [("fused", {"DTF_DFM_FUSED": "1"}, a.hidden), ("general_path", {"DTF_DFM_FUSED": "0"}, a.hidden),
                    ("fm_fused", {"DTF_FM_FUSED": "1"}, "")]
    if a.fields:
        variants = [("fused", {"DTF_FFM_FUSED": "1"}, ""), ("general_path", {"DTF_FFM_FUSED": "0"}, "")]
    variants = [v + (0,) for v in variants]
    if a.tower_fields:
        variants = [("fused", {"DTF_DFM_FUSED": "1"}, a.hidden, a.tower_fields),
                    ("general_path", {"DTF_DFM_FUSED": "0"}, a.hidden, a.tower_fields),
                    ("pooled_fused", {"DTF_DFM_FUSED": "1"}, a.hidden, 0)]
    runs = {name: [] for name, _, _, _ in variants}
    for r in range(a.rounds):
        # alternating: one process per variant per round, the order reversed every other round
        for name, env, hidden, tf in (variants if r % 2 == 0 else variants[::-1]):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", here, "--features",
                                str(a.features), "--hidden", hidden, "--fields", str(a.fields), "--tower-fields", str(tf)],
                               capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                raise SystemExit(f"{name} round {r} failed:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            runs[name].append(json.loads(line[-1][7:]))
            print(name, r, line[-1][7:], flush=True)
    out = {"features": a.features, "factors": 64, "optimizer": "sgd", "rounds": a.rounds, "ids_per_row": 40,
           "table_row_bytes_read_by_fm_rows_at_4096": 4096 * 40 * 256, "variants": {}}
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
    out["general_over_fused"] = {k: round(g[k]["median"] / f[k]["median"], 2) for k in g if k.endswith("_ms")}
    # faster by more than the spread: the fused path's slowest run under the general path's fastest
    out["fused_faster_beyond_spread"] = {k: bool(f[k]["max"] < g[k]["min"]) for k in g if k.endswith("_ms")}
    if a.fields:
        out.update(fields=a.fields, factors=4, ids_per_row=a.fields, table_row_bytes_read_by_fm_rows_at_4096=4096 * a.fields ** 2 * 16)
        out["runs"] = {name: {k: [x[k] for x in rs] for k in rs[0] if k.endswith("_ms")} for name, rs in runs.items()}
    elif a.tower_fields:
        out.update(hidden=[int(h) for h in a.hidden.split(",")], tower_fields=a.tower_fields, factors=8,
                   ids_per_row=a.tower_fields, pooled_factors=64, pooled_ids_per_row=40,
                   table_row_bytes_read_by_fm_rows_at_4096=4096 * a.tower_fields * 32)
        out["runs"] = {name: {k: [x[k] for x in rs] for k in rs[0] if k.endswith("_ms")} for name, rs in runs.items()}
    elif a.hidden:
        out["hidden"] = [int(h) for h in a.hidden.split(",")]
        fm = out["variants"]["fm_fused"]
        out["fused_over_fm_fused"] = {k: round(f[k]["median"] / fm[k]["median"], 2) for k in f if k.endswith("_ms") and k in fm}
        out["runs"] = {name: {k: [x[k] for x in rs] for k in rs[0] if k.endswith("_ms")} for name, rs in runs.items()}
    else:
        out["rpw"] = {str(B): {"auto": f[f"rpw_auto_{B}"],
                               **{f"rpw{r}_evaluate_ms": f[f"evaluate_{B}_rpw{r}_event_ms"] for r in RPWS}} for B in (500, 4096)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
