#!/usr/bin/env python3
"""Is the device code of every csrc/kernels/*.hip the same as at another commit?

For a refactor that only moves declarations and helpers between files: each .hip
is compiled to gfx950 assembly (the build's own hip flags plus
`--cuda-device-only -S`) at the base revision and in the working tree, the lines
holding `__hip_cuid_` are dropped (that symbol is random per compile) and the two
texts are compared.  Needs hipcc only, no GPU.

    python scripts/device_asm_diff.py --base HEAD~1 [-j 8] [--keep DIR] [--json profiles/x.json]

--keep DIR keeps the assembly (DIR/base, DIR/tree) and reuses a base already
there; --json writes the per-file result under the key "device_asm" of that
file, leaving its other keys alone.  Exit status 1 when any file differs.
"""
import argparse
import concurrent.futures as cf
import glob
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ARCH = os.environ.get("DTF_OFFLOAD_ARCH", "gfx950")
# _build.py's hip_flags; paths relative to the tree's root, so that both trees compile the same command
FLAGS = [f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17", "-fno-gpu-rdc", "-munsafe-fp-atomics",
         "-Wno-unused-result", "-Icsrc", "-Icsrc/kernels", "-Icsrc/runtime", "--cuda-device-only", "-S"]


def emit(root, rel, out):
    """Assembly of root/rel without the per-compile symbol, written to out; returns its lines."""
    if not os.path.exists(out):
        r = subprocess.run([os.path.join(ROCM, "bin", "hipcc")] + FLAGS + [rel, "-o", out + ".tmp"], cwd=root,
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{rel} in {root}:\n{r.stderr[-4000:]}")
        os.replace(out + ".tmp", out)
    with open(out) as f:
        return [ln for ln in f if "__hip_cuid_" not in ln]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", required=True, help="git revision to compare the working tree against")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 4))
    ap.add_argument("--keep", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)

    tmp = None
    work = a.keep
    if work is None:
        tmp = tempfile.TemporaryDirectory(prefix="device_asm_")
        work = tmp.name
    work = os.path.abspath(work)
    base_src = os.path.join(work, "base_src")
    for d in ("base", "tree", "base_src"):
        os.makedirs(os.path.join(work, d), exist_ok=True)
    rev = subprocess.check_output(["git", "rev-parse", a.base], cwd=REPO, text=True).strip()
    ar = subprocess.run(["git", "archive", rev, "csrc"], cwd=REPO, capture_output=True, check=True)
    subprocess.run(["tar", "-x", "-C", base_src], input=ar.stdout, check=True)

    rels = sorted(os.path.relpath(p, REPO) for p in glob.glob(os.path.join(REPO, "csrc", "kernels", "*.hip")))
    # the tree's assembly is never reused: it is what is being checked
    for rel in rels:
        p = os.path.join(work, "tree", os.path.basename(rel) + ".s")
        if os.path.exists(p):
            os.remove(p)
    jobs = {}
    with cf.ThreadPoolExecutor(max_workers=a.j) as ex:
        for rel in rels:
            name = os.path.basename(rel) + ".s"
            if os.path.exists(os.path.join(base_src, rel)):
                jobs[(rel, "base")] = ex.submit(emit, base_src, rel, os.path.join(work, "base", name))
            jobs[(rel, "tree")] = ex.submit(emit, REPO, rel, os.path.join(work, "tree", name))
    rows, bad = [], 0
    for rel in rels:
        tree = jobs[(rel, "tree")].result()
        base = jobs[(rel, "base")].result() if (rel, "base") in jobs else None
        same = base == tree
        bad += not same
        rows.append({"file": rel, "lines": len(tree), "base_lines": None if base is None else len(base),
                     "identical": same})
        print(f"{'identical' if same else 'DIFFERENT':9s} {len(tree):8d} lines  {rel}")
    print(f"{len(rows) - bad} of {len(rows)} files identical to {rev[:12]}")
    if a.json:
        path = os.path.join(REPO, a.json) if not os.path.isabs(a.json) else a.json
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc["device_asm"] = {
            "how": "scripts/device_asm_diff.py: hipcc " + " ".join(FLAGS) + " of every csrc/kernels/*.hip at the "
                   "base revision and in this tree, lines with __hip_cuid_ dropped, texts compared",
            "base": rev, "files": rows, "identical": len(rows) - bad, "different": bad}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if tmp is not None:
        tmp.cleanup()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
