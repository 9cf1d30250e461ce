#!/usr/bin/env python3
"""Record tests/golden/mlp_persist_gather_parent.json: the sha256 of the parameter
and metric bytes of every one-GPU case of tests/test_mlp_persist_gather_gpu.py.

Run it on an MI355X from the root of a built tree of the commit to compare with
(the parent of the gather rewrite), with that test file copied into its tests/:

    PYTHONPATH=. python scripts/record_mlp_persist_gather_golden.py OUT.json
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main(out):
    import numpy as np
    import test_mlp_persist_gather_gpu as t
    from distributed_tensorflow_example_amd import _native

    cases = {}
    for c in t.CASES + [t.SPREAD]:
        p, m = t.run_case(*c)
        t._check_reference(c[0], c[1], False, p, m)
        cases[t.case_id(*c)] = t.digests(p, m)
    for B, act, prec in ((100, "sigmoid", "fp32"), (17, "relu", "fp32"), (100, "relu", "fp32-mfma")):
        for cuts in t.PARTITIONS:
            assert t.digests(*t.run_case(B, act, prec, "packed", cuts)) == cases[t.case_id(B, act, prec, "packed")], cuts
    a, b = t.run_case(*t.SPREAD), t.run_case(100, "sigmoid", "fp32", "packed")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with open(out, "w") as f:
        json.dump({"native_src_hash": _native.src_hash(), "steps": t.STEPS, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(cases), "cases from build", _native.src_hash())


if __name__ == "__main__":
    main(sys.argv[1])
