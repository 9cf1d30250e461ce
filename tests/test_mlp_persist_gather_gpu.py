"""The granule gathers of the persistent fp32 MLP step
(csrc/kernels/mlp_persist_f32.hip, gather_gran): a pass issues the loads of
every outstanding slot of a group before it compares a tag, slots the whole wave
holds are skipped by a scalar branch, and lanes that take no data load past the
region's range.  The acceptance rule and the part[] slots are those of the
per-lane loop it replaced, so every sum keeps its operands and its order:

* 7 steps (both step parities, each parity slot reused three times, sequence
  tags carried across launches) at B = 1, 16, 17, 100, 112, sigmoid and relu,
  both engines: metrics of every step and the final parameters against the
  fp32 reference, at the tolerances of tests/test_mlp_persist_operand_prep_gpu.py;
* the bytes of the parameters and the metrics of every one-GPU case hash to
  what the parent build (per-lane slot loop) gave on an MI355X
  (tests/golden/mlp_persist_gather_parent.json, written by
  scripts/record_mlp_persist_gather_golden.py);
* launch partitions 7 / 3 + 4 / 1 x 7 are array_equal;
* the spread placement (write-through stores), two ranks on one GPU (NW = 2)
  and the resident engine (RES) run the same function."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from distributed_tensorflow_example_amd.data.mnist import PinnedEpoch
from distributed_tensorflow_example_amd.models import mlp

from test_mlp_persist_operand_prep_gpu import LR, _data
from test_mlp_persist_head_gpu import STEPS, _check_reference

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_persist_gather_parent.json")

BATCHES = (1, 16, 17, 100, 112)   # one row, a tile edge, one row past it, the workload's batch, all 7 tiles
CASES = [(B, act, prec, "packed") for B in BATCHES for act in ("sigmoid", "relu") for prec in ("fp32", "fp32-mfma")]
SPREAD = (100, "sigmoid", "fp32", "spread")
PARTITIONS = ((7,), (3, 4), (1,) * 7)


def case_id(B, act, prec, placement):
    return f"B{B}-{act}-{prec}-{placement}"


def run_case(B, act, prec, placement, cuts=(STEPS,)):
    """STEPS steps, one launch per entry of `cuts`: (params, metrics of every step)."""
    assert sum(cuts) == STEPS
    imgs, labels = _data(B)
    tr = mlp.FusedMLPTrainer(batch_size=B, lr=LR, act=act, device=torch.device("cuda"))
    run = mlp.PersistentMLPRunner(tr, PinnedEpoch(imgs, labels, B), steps_per_launch=STEPS, precision=prec,
                                  placement=placement)
    for n in cuts:
        run.run(n)
    torch.cuda.synchronize()
    assert run.error() == 0
    assert tr.global_step == STEPS
    return tr.get_params().cpu().numpy().copy(), np.asarray(tr.read_metrics(0, STEPS)).copy()


def digests(params, metrics):
    return {"params": hashlib.sha256(np.ascontiguousarray(params).tobytes()).hexdigest(),
            "metrics": hashlib.sha256(np.ascontiguousarray(metrics).tobytes()).hexdigest()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("B,act,prec,placement", CASES + [SPREAD], ids=lambda v: str(v))
def test_gather_reference_and_parent_bits(native, golden, B, act, prec, placement):
    p, m = run_case(B, act, prec, placement)
    _check_reference(B, act, False, p, m)
    assert digests(p, m) == golden[case_id(B, act, prec, placement)]


@pytest.mark.parametrize("B,act,prec", [(100, "sigmoid", "fp32"), (17, "relu", "fp32"), (100, "relu", "fp32-mfma")])
def test_gather_launch_partitions_bit_equal(native, golden, B, act, prec):
    """One launch, 3 + 4 and 7 launches of one step: the tags of the hand-offs
    run on across launches, and every partition gives the parent's bits."""
    for cuts in PARTITIONS:
        p, m = run_case(B, act, prec, "packed", cuts)
        assert digests(p, m) == golden[case_id(B, act, prec, "packed")], cuts


def test_gather_spread_equals_packed(native):
    """Write-through stores and other XCDs' loads carry the same granules."""
    a, b = run_case(*SPREAD), run_case(100, "sigmoid", "fp32", "packed")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_gather_two_ranks_same_gpu(native):
    """The NW = 2 instantiation: two ranks sharing cuda:0, bit-identical replicas."""
    from test_mlp_persist_gpu import _persist_selftest

    _persist_selftest(2, "fp32", "bf16", "one-shot")


def test_gather_resident_engine(monkeypatch):
    """The resident instantiation: six Session.run steps against the fp64 graph."""
    from test_lowering_cpu import _graph
    from test_resident_gpu import _batches, _check_steps

    monkeypatch.setenv("DTF_RESIDENT_IDLE_S", "2.0")
    import distributed_tensorflow_example_amd.compat as tf

    g = _graph(tf, False, "sigmoid")
    with tf.Session() as sess:
        sess.run(tf.global_variables_initializer())
        params = [v.numpy().astype(np.float64) for v in g["W"]]
        _check_steps(tf, sess, g, params, _batches(6, 100, 11), 0.5, "sigmoid", False)
    tf.reset_default_graph()
