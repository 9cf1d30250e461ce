"""libsvm text -> CSR batches: the C++ thread stream against the GPU parser.

    python scripts/bench_libsvm_parse.py --out profiles/libsvm_gpu_parse_ab.json [--mb 256] [--runs 3]

Synthetic shards (about 40 ids per row) are written once, then every
configuration runs in a fresh process, the configurations alternating, `--runs`
times each:

* cpuN        `LibsvmStream` (the C++ parser) with N threads, batches of 500 rows drained
              as fast as they come;
* gpu         `GpuBatchStream`: file -> pinned buffer -> device -> kernels -> device batches
              (everything the queue mode does);
* gpu_device  the kernels alone on a chunk already in device memory (HIP events).

Reported per configuration: rows/s and text GB/s, median and [min, max].
`--example` adds examples/sparse_lr.py --mode=queue steps/s with --parser=cpu
against --parser=gpu (one ps, one worker).  A measurement, not a gate.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
BATCH = 500


def make_shards(d: str, mb: int):
    from distributed_tensorflow_example_amd.data import libsvm

    first = libsvm.write_synthetic(os.path.join(d, "seed"), 1, 16000, 4762348, nnz_per_row=40, seed=1)[0]
    size = os.path.getsize(first)
    files = []
    for k in range(max(1, (mb << 20) // size)):      # copies: the parsers do not care, the disk cache does not either
        f = os.path.join(d, f"part-{k:05d}")
        shutil.copyfile(first, f)
        files.append(f)
    os.remove(first)
    return files


def run_cpu(files, threads):
    from distributed_tensorflow_example_amd import _native

    C = _native.load()
    t0 = time.perf_counter()
    st = C.LibsvmStream(files, BATCH, threads, 1.0, False, 64, 0)
    rows = 0
    while True:
        b = st.next(120.0)
        if b is None:
            break
        rows += len(b[0])
    return rows, time.perf_counter() - t0


def run_gpu(files, chunk_bytes):
    import torch

    from distributed_tensorflow_example_amd.data import libsvm

    gp = libsvm.GpuLibsvmParser(torch.device("cuda", 0), chunk_bytes, BATCH)
    gp.parse_bytes(b"1 3:1\n")                       # first-launch costs stay out of the timing
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = libsvm.GpuBatchStream(gp, files, loop=False)
    rows = 0
    while True:
        b = st.next()
        if b is None:
            break
        rows += int(b[0].shape[0])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st.stop()
    assert gp.fallback_chunks == 0, "the synthetic shards are regular text"
    return rows, dt


def run_gpu_device(files, chunk_bytes, reps=10):
    """The kernels alone: one chunk resident on the device, parsed `reps` times."""
    import numpy as np
    import torch

    from distributed_tensorflow_example_amd import _native

    C = _native.load()
    dev = torch.device("cuda", 0)
    with open(files[0], "rb") as fh:
        data = fh.read(chunk_bytes)
    data = data[:data.rfind(b"\n") + 1]
    n = len(data)
    plan = C.libsvm_gpu_plan(n, BATCH, 0)
    text = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
    ws = torch.empty(plan["workspace_bytes"], dtype=torch.uint8, device=dev)
    labels = torch.empty(plan["rows"], dtype=torch.float32, device=dev)
    ids = torch.empty(plan["nnz"], dtype=torch.int64, device=dev)
    vals = torch.empty(plan["nnz"], dtype=torch.float32, device=dev)
    offs = torch.empty(plan["batches"] * (BATCH + 1), dtype=torch.int64, device=dev)
    meta = torch.empty(plan["meta"], dtype=torch.int64, device=dev)
    call = lambda: C.libsvm_gpu_parse_into(text, n, 0, 0, 1.0, BATCH, 0, 0, ws, labels, ids, vals, offs, meta)  # noqa: E731
    call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    m = meta[:8].cpu().numpy()
    assert m[2] == 0
    return int(m[0]) * reps, e0.elapsed_time(e1) / 1e3, n * reps


def worker(a):
    files = sorted(os.path.join(a.dir, f) for f in os.listdir(a.dir) if f.startswith("part-"))
    total = sum(os.path.getsize(f) for f in files)
    if a.run.startswith("cpu"):
        rows, dt = run_cpu(files, int(a.run[3:]))
    elif a.run == "gpu":
        rows, dt = run_gpu(files, a.chunk_bytes)
    else:
        rows, dt, total = run_gpu_device(files, a.chunk_bytes)
    print(json.dumps({"config": a.run, "rows": rows, "seconds": dt, "rows_per_s": rows / dt,
                      "text_gb_per_s": total / dt / 1e9}))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_example(d, files, parser, steps):
    conf = os.path.join(d, f"cluster_{parser}.json")
    with open(conf, "w") as f:
        json.dump({"ps": [f"127.0.0.1:{_free_port()}"], "worker": [f"127.0.0.1:{_free_port()}"]}, f)
    out = os.path.join(d, f"result_{parser}.json")
    common = [f"--cluster_conf={conf}", f"--train={','.join(files)}", f"--test={files[0]}", "--mode=queue",
              "--num_epochs=1", f"--steps_per_epoch={steps}", "--batch_size=500", "--thread_num=16",
              "--trace_step_interval=1000000", f"--parser={parser}"]
    script = os.path.join(REPO, "examples", "sparse_lr.py")
    env = dict(os.environ, PYTHONPATH=REPO)
    ps = subprocess.Popen([sys.executable, script, "--job_name=ps", "--task_index=0"] + common, env=env,
                          stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT)
    try:
        w = subprocess.run([sys.executable, script, "--job_name=worker", "--task_index=0", f"--result_json={out}"]
                           + common, env=env, capture_output=True, text=True, timeout=600)
        if w.returncode != 0:
            raise RuntimeError(w.stdout[-3000:] + w.stderr[-3000:])
        ps.wait(timeout=60)
    finally:
        if ps.poll() is None:
            ps.kill()
    with open(out) as f:
        r = json.load(f)
    return {"parser": parser, "steps": r["steps"], "train_s": r["train_s"], "steps_per_s": r["steps"] / r["train_s"],
            "auc": r["auc"], "gpu_chunks": r["gpu_chunks"], "fallback_chunks": r["fallback_chunks"]}


def _spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk_bytes", type=int, default=16 << 20)
    ap.add_argument("--configs", default="cpu2,cpu8,cpu16,gpu,gpu_device")
    ap.add_argument("--example", action="store_true")
    ap.add_argument("--example_steps", type=int, default=2000)
    ap.add_argument("--run", default="")          # (internal) one configuration in this process
    ap.add_argument("--dir", default="")
    a = ap.parse_args()
    if a.run:
        return worker(a)
    d = tempfile.mkdtemp(prefix="libsvm_bench_")
    try:
        files = make_shards(d, a.mb)
        total = sum(os.path.getsize(f) for f in files)
        configs = a.configs.split(",")
        got = {c: [] for c in configs}
        for _ in range(a.runs):                   # alternating: cpu2, cpu8, ..., gpu, cpu2, ...
            for c in configs:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--run", c, "--dir", d,
                                    "--chunk_bytes", str(a.chunk_bytes)], capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise RuntimeError(f"{c}: {r.stdout[-2000:]}{r.stderr[-2000:]}")
                got[c].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(got[c][-1], flush=True)
        res = {"text_bytes": total, "files": len(files), "batch_size": BATCH, "chunk_bytes": a.chunk_bytes,
               "runs": a.runs, "configs": {}}
        for c, rs in got.items():
            res["configs"][c] = {"rows_per_s": _spread([r["rows_per_s"] for r in rs]),
                                 "text_gb_per_s": _spread([r["text_gb_per_s"] for r in rs]), "rows": rs[0]["rows"]}
        if a.example:
            ex = {"cpu": [], "gpu": []}
            for _ in range(a.runs):
                for p in ("cpu", "gpu"):
                    ex[p].append(run_example(d, files, p, a.example_steps))
                    print(ex[p][-1], flush=True)
            res["sparse_lr_queue"] = {p: {"steps_per_s": _spread([r["steps_per_s"] for r in rs]),
                                          "auc": rs[0]["auc"], "gpu_chunks": rs[0]["gpu_chunks"],
                                          "fallback_chunks": rs[0]["fallback_chunks"]} for p, rs in ex.items()}
        print(json.dumps(res))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
