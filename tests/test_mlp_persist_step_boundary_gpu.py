"""The step boundary of the one-GPU split engine (csrc/kernels/mlp_persist_f32.hip).
Workgroup 0's wave 7 reduces the per-row loss / accuracy of a step in front of
barrier A with VALU lane permutes in the order of wave_sum's butterfly, and
takes the metric ring slot from a 32-bit modulo of the launch's first slot
(MET_FAST): every loss, accuracy and ring slot must be what it was, however the
steps are cut into launches and wherever the ring wraps.

The head waves keep preparing the next step's operands after P2, wave 7 behind
its DMA (DTF_PERSIST_DBG bit 2: wave 7 late too, on the instrumented
instantiation); both must give the same bits, for every cut.

Helpers, data and reference bounds are those of
test_mlp_persist_operand_prep_gpu.py (parameter-delta relative error < 2e-5,
loss rtol / atol 1e-5)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_example_amd.data.mnist import PinnedEpoch
from distributed_tensorflow_example_amd.models import mlp
from test_mlp_persist_operand_prep_gpu import LR, _check_reference, _data, _reference, _run

pytestmark = pytest.mark.gpu

CASES = ((100, "sigmoid"), (37, "relu"))
CUTS = (7, 3, 1)            # 7 steps as one launch, as 3 + 3 + 1, as 7 launches of 1
EDGES = (1, 16, 17, 112)    # one row, a full first tile, one row into the second, no padding

_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import test_mlp_persist_operand_prep_gpu as t
out = {}
for B, act in ((100, "sigmoid"), (37, "relu")):
    for spl in (7, 3, 1):
        p, m = t._run(B, act, 7, spl)
        out[f"p_{B}_{act}_{spl}"] = p
        out[f"m_{B}_{act}_{spl}"] = m
np.savez(sys.argv[3], **out)
print("step-boundary child done")
"""


@pytest.fixture(scope="module")
def forced_late(native, tmp_path_factory):
    """The same runs with every wave on the late path (bit 2, read once per
    process: a fresh child), on the instrumented instantiation of the kernel."""
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    dump = str(tmp_path_factory.mktemp("step_boundary") / "late.npz")
    env = dict(os.environ, PYTHONPATH=repo, DTF_PERSIST_DBG="4")
    r = subprocess.run([sys.executable, "-c", _CHILD, repo, here, dump], capture_output=True, text=True, timeout=100,
                       env=env, cwd=repo)
    assert r.returncode == 0 and "step-boundary child done" in r.stdout, (r.stdout + r.stderr)[-3000:]
    return dict(np.load(dump))


@pytest.mark.parametrize("B,act", CASES)
def test_step_boundary_cuts_and_paths_bit_equal(native, forced_late, B, act):
    """Default and forced-late, each cut three ways: a launch's first ring slot
    comes from its global step, a step's operands from the prologue or the
    previous step -- always the one-launch run's bits."""
    p0, m0 = _run(B, act, 7, CUTS[0])
    _check_reference(B, act, 7, p0, m0)
    for spl in CUTS[1:]:
        p, m = _run(B, act, 7, spl)
        assert np.array_equal(p, p0) and np.array_equal(m, m0), ("default", spl)
    for spl in CUTS:
        assert np.array_equal(forced_late[f"p_{B}_{act}_{spl}"], p0), ("late", spl)
        assert np.array_equal(forced_late[f"m_{B}_{act}_{spl}"], m0), ("late", spl)


@pytest.mark.parametrize("B", EDGES)
def test_step_boundary_edge_batches(native, B):
    """3 steps in launches of 2 and 1: rows of padding contribute zeros to both
    sums, and the mean is over B."""
    p, m = _run(B, "sigmoid", 3, 2)
    _check_reference(B, "sigmoid", 3, p, m)


def test_step_boundary_metric_ring_wraps(native):
    """A ring of 5 slots under 7 steps in launches of 3, 3, 1: the slot of a step
    is (global step) mod ring whichever launch runs it and wherever inside a
    launch the ring wraps, so the ring ends with steps 5, 6, 2, 3, 4."""
    B, act, steps = 100, "sigmoid", 7
    imgs, labels = _data(B)
    tr = mlp.FusedMLPTrainer(batch_size=B, lr=LR, act=act, metrics_ring=5, device=torch.device("cuda"))
    run = mlp.PersistentMLPRunner(tr, PinnedEpoch(imgs, labels, B), steps_per_launch=3, precision="fp32")
    run.run(steps)
    torch.cuda.synchronize()
    assert run.error() == 0 and tr.global_step == steps
    got = np.asarray(tr.read_metrics(2, 7))
    _, m_full = _run(B, act, steps, 3)
    assert np.array_equal(got, m_full[2:7])
    _, _, losses, accs = _reference(B, act, steps)
    assert np.allclose(got[:, 0], losses[2:7], rtol=1e-5, atol=1e-5)
    assert np.allclose(got[:, 1], accs[2:7], atol=1e-6)


def test_step_boundary_leaves_f32_mfma_engine_alone(native):
    """The f32-input MFMA engine (neither change) still matches the reference
    and is bit-equal across launch cuts."""
    a = _run(100, "sigmoid", 7, 7, precision="fp32-mfma")
    b = _run(100, "sigmoid", 7, 3, precision="fp32-mfma")
    _check_reference(100, "sigmoid", 7, *a)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
