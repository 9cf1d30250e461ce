#!/usr/bin/env python3
"""What one granule-gather pass of the persistent MLP kernel issues, read from
the generated gfx950 code (needs hipcc, no GPU).

Compiles csrc/kernels/mlp_persist_f32.hip device-only to assembly with the
build's flags and, per kernel, finds the loops that hold granule loads
(`buffer_load_dwordx4 ... sc1`, not the system-scope `sc0 sc1` peer loads):
the E1 and the E2 gather loop, in program order.  Per loop it reports

  loads             granule loads in the loop body
  loads_before_wait granule loads issued before the first `s_waitcnt vmcnt`
                    that follows a load: what is in flight when the wave
                    first waits for data
  insts             instructions in the loop body

Usage: python scripts/probes/gather_pass_shape.py [--kernel SUBSTR] [--asm FILE] [--json]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRC = os.path.join(REPO, "csrc", "kernels", "mlp_persist_f32.hip")
# <ACT 0, NW 1, SPLIT, !RES, !INS>: what bench.py runs
FLAGSHIP = "mlp_persist_f32ILi0ELi1ELb1ELb0ELb0E"

GRAN_LOAD = re.compile(r"^buffer_load_dwordx4\b(?!.*\bsc0\b).*\bsc1\b")
VM_WAIT = re.compile(r"^s_waitcnt\b.*\bvmcnt\(")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)")


def hipcc() -> str | None:
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cand = os.path.join(rocm, "bin", "hipcc")
    return cand if os.path.exists(cand) else shutil.which("hipcc")


def compile_asm(src: str = SRC, arch: str = "gfx950") -> str:
    cc = hipcc()
    if cc is None:
        raise RuntimeError("hipcc not found")
    csrc = os.path.join(REPO, "csrc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [cc, f"--offload-arch={arch}", "-O3", "-std=c++17", "-fno-gpu-rdc", "-munsafe-fp-atomics",
               f"-I{csrc}", f"-I{os.path.join(csrc, 'kernels')}", f"-I{os.path.join(csrc, 'runtime')}",
               "--cuda-device-only", "-S", src, "-o", out]
        subprocess.run(cmd, check=True, capture_output=True, text=True)
        with open(out) as f:
            return f.read()


def kernels(asm: str) -> dict[str, list[str]]:
    """kernel name -> its lines (labels and instructions, comments stripped)"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    lines = asm.splitlines()
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\w+):", ln)
        if m and m.group(1) in names:
            start[m.group(1)] = i
    out = {}
    for n, s in start.items():
        body = []
        for ln in lines[s + 1:]:
            t = ln.split(";", 1)[0].strip()
            if t.startswith(".Lfunc_end"):
                break
            if not t or (t.startswith(".") and not LABEL.match(t)):
                continue
            body.append(t)
        out[n] = body
    return out


def gather_loops(body: list[str]) -> list[dict]:
    """the innermost loops (label .. backward branch) that hold granule loads"""
    insts, label_at = [], {}
    for t in body:
        m = LABEL.match(t)
        if m:
            label_at[m.group(1)] = len(insts)
        else:
            insts.append(t)
    loops = []
    for i, t in enumerate(insts):
        m = BRANCH.match(t)
        if m and m.group(1) in label_at and label_at[m.group(1)] <= i:
            loops.append((label_at[m.group(1)], i))
    # not a waterfall loop (a non-uniform resource read lane by lane around one load)
    loops = [(lo, hi) for lo, hi in loops
             if not (hi - lo < 24 and any(t.startswith("v_readfirstlane_b32") for t in insts[lo:hi + 1]))]
    loads = [i for i, t in enumerate(insts) if GRAN_LOAD.match(t)]
    owner: dict[tuple[int, int], list[int]] = {}
    for ld in loads:
        inside = [lp for lp in loops if lp[0] <= ld <= lp[1]]
        if inside:
            owner.setdefault(min(inside, key=lambda lp: lp[1] - lp[0]), []).append(ld)
    res = []
    for (lo, hi), lds in sorted(owner.items()):
        before = 0
        for t in insts[lo:hi + 1]:
            if GRAN_LOAD.match(t):
                before += 1
            elif before and VM_WAIT.match(t):
                break
        res.append({"loads": len(lds), "loads_before_wait": before, "insts": hi - lo + 1})
    return res


def report(asm: str, kernel: str | None = None) -> dict[str, list[dict]]:
    return {n: gather_loops(b) for n, b in kernels(asm).items()
            if "mlp_persist_f32" in n and (kernel is None or kernel in n)}


def registers(asm: str) -> dict[str, dict]:
    """kernel name -> vgpr count, spill count, scratch bytes from the code object's metadata"""
    out = {}
    for blk in asm.split("- .agpr_count:")[1:]:
        g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "mlp_persist_f32" in name:
            out[name] = {"vgpr": g("vgpr_count"), "spill": g("vgpr_spill_count"),
                         "scratch": g("private_segment_fixed_size")}
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--kernel", default=None, help="only kernels whose mangled name holds this (default: all)")
    ap.add_argument("--flagship", action="store_true", help="only bench.py's instantiation")
    ap.add_argument("--asm", default=None, help="read this assembly file, do not compile")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args(argv)
    asm = open(a.asm).read() if a.asm else compile_asm()
    rep = report(asm, FLAGSHIP if a.flagship else a.kernel)
    regs = registers(asm)
    if a.json:
        print(json.dumps({"loops": rep, "registers": {k: regs.get(k) for k in rep}}))
        return 0
    for n, loops in rep.items():
        r = regs.get(n, {})
        print(f"{n}: vgpr {r.get('vgpr')} spill {r.get('spill')} scratch {r.get('scratch')}")
        for i, lp in enumerate(loops):
            print(f"  gather loop {i}: {lp['loads']} loads, {lp['loads_before_wait']} before the first wait, "
                  f"{lp['insts']} instructions")
    return 0


if __name__ == "__main__":
    sys.exit(main())
