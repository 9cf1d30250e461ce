"""Cost of evaluating the reference's test set (10,000 x 784, example.py:187)
on the forward-only kernel (csrc/kernels/mlp_eval.hip, models/mlp.py evaluate):

1. device time of one evaluation of device-resident rows, uint8 and float32
   (device events, median of `--reps`), as bytes of x read per second;
2. end to end, alternating new and old, `--runs` each:
   `sess.run(accuracy, test feed)` with the float feed, lowered against the
   eager op-by-op path (a Session with DTF_GRAPH_LOWERING=0: for this fetch
   the code the Session ran before the evaluation lowering existed), and
   `tr.evaluate(images_u8, labels_u8)` against the CPU `reference_forward` it
   replaces in examples/mnist_example.py; plus the bare 31 MB host-to-device
   copy both Session paths pay.

    python scripts/bench_eval.py [--reps 30] [--runs 5] [--out FILE] [--kernel-only]

`--kernel-only` runs part 1 alone (for a profiler run of its own).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

N, K = 10000, 784


def _median_ms(fn, reps, warmup=5, inner=1):
    """Median device time (ms) of `inner` back-to-back calls of fn, per call."""
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
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def _wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_part(C, mlp, imgs, labels, reps):
    dev = torch.device("cuda", torch.cuda.current_device())
    flat = mlp.init_params(1).to(dev)
    p = mlp.unflatten(flat)
    four = (p["weights/Variable"], p["biases/Variable"], p["weights/Variable_1"], p["biases/Variable_1"])
    rec = torch.zeros(3, dtype=torch.int64, device=dev)
    xu = torch.from_numpy(imgs).to(dev)
    xf = (xu.float() / 255.0).contiguous()
    lab = torch.from_numpy(labels).to(dev)
    res = {}
    for name, x in (("uint8", xu), ("float32", xf)):
        nbytes = x.numel() * x.element_size()

        def run(x=x):
            C.mlp_eval(x, lab, *four, 0, False, rec, True)
        med1, lo1, hi1 = _median_ms(run, reps)
        med20, lo20, hi20 = _median_ms(run, reps, inner=20)
        res[name] = {"x_bytes": nbytes,
                     "device_ms_one_call_median": round(med1, 5), "device_ms_one_call_min_max": [round(lo1, 5), round(hi1, 5)],
                     "device_ms_per_call_20_back_to_back_median": round(med20, 5),
                     "device_ms_per_call_20_back_to_back_min_max": [round(lo20, 5), round(hi20, 5)],
                     "x_TB_per_s_one_call": round(nbytes / (med1 * 1e-3) / 1e12, 4),
                     "x_TB_per_s_back_to_back": round(nbytes / (med20 * 1e-3) / 1e12, 4)}
    # the arithmetic floor of the pass: exact-fp32 MFMA at 64 FLOP / clk / SIMD
    res["mfma_flop"] = 2 * N * K * 112 + 2 * N * 112 * 16            # hidden tiles padded to 7 x 16, classes to 16
    return res


def end_to_end_part(mlp, imgs, labels, runs):
    import distributed_tensorflow_example_amd.compat as tf
    from distributed_tensorflow_example_amd.compat import lowering as L
    from test_lowering_cpu import _graph

    dev = torch.device("cuda", torch.cuda.current_device())
    x32 = imgs.astype(np.float32) / np.float32(255.0)
    onehot = np.eye(10, dtype=np.float32)[labels]
    res = {}
    g = _graph(tf)
    rng = np.random.default_rng(0)
    os.environ["DTF_GRAPH_LOWERING"] = "1"
    with tf.Session() as sess:
        sess.run(tf.global_variables_initializer())
        for _ in range(3):
            bx = (rng.integers(0, 256, (100, 784)) / 255.0).astype(np.float32)
            by = np.eye(10, dtype=np.float32)[rng.integers(0, 10, 100)]
            sess.run([g["train"], g["ce"]], feed_dict={g["x"]: bx, g["y_"]: by})
        plan = L.plan_for(g["train"])
        os.environ["DTF_GRAPH_LOWERING"] = "0"
        eager = tf.Session()
        os.environ["DTF_GRAPH_LOWERING"] = "1"
        feed = {g["x"]: x32, g["y_"]: onehot}
        vals = {}

        def lowered():
            vals["lowered"] = sess.run(g["acc"], feed_dict=feed)

        def old():
            vals["eager"] = eager.run(g["acc"], feed_dict=feed)
        for _ in range(2):
            lowered(), old()
        n0 = plan.eval_runs
        t_new, t_old = [], []
        for _ in range(runs):
            t_new.append(_wall_ms(lowered))
            t_old.append(_wall_ms(old))
        res["session_accuracy_float_feed"] = {
            "lowered_ms": [round(t, 3) for t in t_new], "eager_ms": [round(t, 3) for t in t_old],
            "lowered_ms_median": round(float(np.median(t_new)), 3), "eager_ms_median": round(float(np.median(t_old)), 3),
            "eager_ms_spread": round(max(t_old) - min(t_old), 3),
            "eval_runs_counted": plan.eval_runs - n0, "accuracy_lowered": float(vals["lowered"]),
            "accuracy_eager": float(vals["eager"])}
    tf.reset_default_graph()
    # the 31 MB copy both paths pay, from the caller's pageable array; from pinned memory for comparison
    pinned = torch.from_numpy(x32).pin_memory()
    dst = torch.empty(x32.shape, dtype=torch.float32, device=dev)
    med, lo, hi = _median_ms(lambda: dst.copy_(pinned, non_blocking=True), 10, warmup=2)
    pageable = sorted(_wall_ms(lambda: torch.from_numpy(x32).to(dev)) for _ in range(5))[2]
    s = res["session_accuracy_float_feed"]
    s["h2d_copy_31MB_pinned_ms"] = round(med, 3)
    s["h2d_copy_31MB_pageable_ms"] = round(pageable, 3)
    s["copy_share_of_lowered"] = round(pageable / s["lowered_ms_median"], 3)    # both paths copy from pageable memory
    s["copy_share_of_eager"] = round(pageable / s["eager_ms_median"], 3)
    # the trainer's evaluation against the CPU forward it replaces in the example
    tr = mlp.FusedMLPTrainer(batch_size=100, lr=0.0005)
    vals = {}

    def new():
        vals["new"] = tr.evaluate(imgs, labels)[1]

    def cpu():
        z = mlp.reference_forward(tr.get_params().cpu(), torch.from_numpy(x32), "sigmoid")
        vals["cpu"] = float((z.argmax(1).numpy() == labels).mean())
    for _ in range(2):
        new(), cpu()
    t_new, t_old = [], []
    for _ in range(runs):
        t_new.append(_wall_ms(new))
        t_old.append(_wall_ms(cpu))
    res["trainer_evaluate_uint8"] = {
        "evaluate_ms": [round(t, 3) for t in t_new], "cpu_reference_forward_ms": [round(t, 3) for t in t_old],
        "evaluate_ms_median": round(float(np.median(t_new)), 3),
        "cpu_reference_forward_ms_median": round(float(np.median(t_old)), 3),
        "accuracy_evaluate": vals["new"], "accuracy_cpu": vals["cpu"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on the GPU: none visible")
    from distributed_tensorflow_example_amd import _native
    from distributed_tensorflow_example_amd.data.mnist import synthetic_mnist
    from distributed_tensorflow_example_amd.models import mlp

    imgs, labels = synthetic_mnist(N, seed=1)
    imgs = np.ascontiguousarray(imgs.reshape(N, K))
    out = {"rows": N, "features": K, "device": torch.cuda.get_device_name(0), "reps": a.reps, "runs": a.runs,
           "kernel": kernel_part(_native.load(), mlp, imgs, labels, a.reps)}
    if not a.kernel_only:
        out.update(end_to_end_part(mlp, imgs, labels, a.runs))
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
