"""Cost of evaluating the sparse-LR model (lr2.py Test() and its closing
streaming_auc loop) on one GPU, through the public trainer / Session
interface only -- so the same script measures any checkout of this repository:

    python scripts/bench_sparse_lr_eval.py [--features 1000000000] [--rounds 3] [--out FILE]
                                           [--other [LABEL=]TREE[,[LABEL=]TREE...]]

Variants, measured in alternating child processes, `--rounds` each: this tree,
this tree with DTF_SLR_FUSED=0 (the general sharded path), and every `--other`
tree (another built checkout, e.g. `parent_commit=../parent`).  Per variant:

1. device time (events) of SparseLRTrainer.evaluate and auc_update on
   device-resident batches of 1,000 rows (Test()'s sample) and 500 rows,
   about 40 ids per row, run_lr2.sh's feature count;
2. host-fed: evaluate from a loader batch of host CSR arrays (CSRBatch), `sess.run([global_step,
   cross_entropy])` and `sess.run(auc_op)` of examples/lr2_compat.py's graph
   (wall clock per call, every call synchronised by its fetch);
3. the training step, SGD and FTRL, device-resident (device events) and
   host-fed (wall clock per call over a queue of calls).

Medians over the rounds with min / max; one JSON document.
"""
import argparse
import json
import os
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


def _device_ms(torch, fn, reps=30, warmup=5, inner=10):
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


def _wall_ms(torch, fn, reps=30, warmup=5, inner=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / inner)
    return float(np.median(out))


def worker(tree, F):
    sys.path.insert(0, tree)
    os.environ.setdefault("DTF_SHARD_MIN_ROWS", "1000")
    import torch

    import distributed_tensorflow_example_amd.compat as tf
    from distributed_tensorflow_example_amd.data.libsvm import CSRBatch
    from distributed_tensorflow_example_amd.models import sparse_lr
    from distributed_tensorflow_example_amd.parallel.world import World

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    h1000, h500 = _batch(rng, 1000, F), _batch(rng, 500, F)
    d1000, d500 = (tuple(torch.from_numpy(a).to(dev) for a in b) for b in (h1000, h500))
    c1000 = CSRBatch(*h1000)              # the loader's host batch type: every path takes it
    res = {}
    for opt in ("sgd", "ftrl"):
        tr = sparse_lr.SparseLRTrainer(F, 0.001, World(device=dev), seed=1, optimizer=opt)
        # the training step first, on a fresh trainer: every tree is in the same state here
        res[f"train_{opt}_dev_500_device_ms"] = _device_ms(torch, lambda: tr.train_step(d500))
        if tr._fused_ok():                # NumPy tuples go through the packed feed (the fused step only)
            res[f"train_{opt}_host_500_wall_ms"] = _wall_ms(torch, lambda: tr.train_step(h500))
        if opt == "sgd":
            res["fused"] = bool(tr._fused_ok())
            for name, b in (("1000", d1000), ("500", d500)):
                res[f"evaluate_dev_{name}_device_ms"] = _device_ms(torch, lambda b=b: tr.evaluate(b))
                res[f"auc_update_dev_{name}_device_ms"] = _device_ms(torch, lambda b=b: tr.auc_update(b))
            res["evaluate_host_1000_wall_ms"] = _wall_ms(torch, lambda: float(tr.evaluate(c1000)[0]), inner=1)
            res["evaluate_host_1000_queued_wall_ms"] = _wall_ms(torch, lambda: tr.evaluate(c1000))
            res["auc"] = float(tr.auc())
        if opt == "sgd":                  # (a tree from before the fused evaluation has no such counter)
            res["fused_eval_runs"] = int(getattr(tr, "fused_eval_runs", lambda: 0)())
        del tr
        torch.cuda.empty_cache()
    # examples/lr2_compat.py's graph and feeds
    tf.reset_default_graph()
    with tf.device(tf.train.replica_device_setter(ps_tasks=1)):
        gs = tf.get_variable("global_step", [], initializer=tf.constant_initializer(0), trainable=False)
        shp, idx, fid, fv = (tf.placeholder(tf.int64), tf.placeholder(tf.int64), tf.placeholder(tf.int64),
                             tf.placeholder(tf.float32))
        y = tf.placeholder(tf.float32, [None, 1])
        with tf.name_scope("weights"):
            W = tf.Variable(tf.random_normal([F, 1]))
        with tf.name_scope("bias"):
            b = tf.Variable(tf.zeros([1]))
        py_x = tf.add(tf.nn.embedding_lookup_sparse(W, tf.SparseTensor(shape=shp, indices=idx, values=fid),
                                                    tf.SparseTensor(shape=shp, indices=idx, values=fv),
                                                    combiner="sum"), b)
        ce = tf.reduce_mean(tf.nn.sigmoid_cross_entropy_with_logits(py_x, y))
        train = tf.train.GradientDescentOptimizer(0.001).minimize(ce, global_step=gs)
        auc_op = tf.contrib.metrics.streaming_auc(tf.nn.sigmoid(py_x), y)

    def feed(hb):
        lab, off, ids, vals = hb
        rows = np.repeat(np.arange(len(lab), dtype=np.int64), np.diff(off))
        return {y: lab, shp: [F, len(lab)], idx: np.stack([rows, ids], 1), fid: ids, fv: vals}
    f1000, f500 = feed(h1000), feed(h500)
    with tf.Session() as sess:
        sess.run([tf.global_variables_initializer(), tf.local_variables_initializer()])
        for _ in range(3):
            sess.run([train], feed_dict=f500)
        res["session_gs_ce_1000_wall_ms"] = _wall_ms(torch, lambda: sess.run([gs, ce], feed_dict=f1000), inner=1)
        res["session_auc_op_500_wall_ms"] = _wall_ms(torch, lambda: sess.run(auc_op, feed_dict=f500), inner=1)
        res["session_train_500_wall_ms"] = _wall_ms(torch, lambda: sess.run([train], feed_dict=f500))
        from distributed_tensorflow_example_amd.compat import lowering
        plan = lowering.plan_for(train)
        res["session_eval_runs"] = int(getattr(plan, "eval_runs", 0)) if plan is not None else 0
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=1_000_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--other", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.features)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    variants = [("this", here, {}), ("this_general_path", here, {"DTF_SLR_FUSED": "0"})]
    for i, t in enumerate(x for x in a.other.split(",") if x):
        label, _, path = t.rpartition("=")
        variants.append((label or f"other{i}:{os.path.basename(os.path.normpath(path))}", os.path.abspath(path), {}))
    runs = {name: [] for name, _, _ in variants}
    for r in range(a.rounds):
        # alternating: one process per variant per round, the order reversed every other round
        for name, tree, env in (variants if r % 2 == 0 else variants[::-1]):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, "--features",
                                str(a.features)], capture_output=True, text=True, env=dict(os.environ, **env),
                               timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                raise SystemExit(f"{name} round {r} failed:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            runs[name].append(json.loads(line[-1][7:]))
            print(name, r, line[-1][7:], flush=True)
    out = {"features": a.features, "rounds": a.rounds, "ids_per_row": 40, "variants": {}}
    for name, rs in runs.items():
        v = {}
        for k in rs[0]:
            xs = [x[k] for x in rs]
            if k.endswith("_ms"):
                v[k] = {"median": round(float(np.median(xs)), 5), "min": round(min(xs), 5), "max": round(max(xs), 5)}
            else:
                v[k] = xs[-1]
        out["variants"][name] = v
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
