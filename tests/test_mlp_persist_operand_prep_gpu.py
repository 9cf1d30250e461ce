"""Operand preparation inside the hand-off waits of the one-GPU split engine
(csrc/kernels/mlp_persist_f32.hip, PREP): a step's weight-gradient operands
are converted in its E1 window and the next step's forward operands in its E2
window (early path) or after P2 (late path).  Which steps take the prologue,
the in-loop and the no-next-step path depends only on how the steps are cut
into launches, and every path must give the same bits.

Checked on the parent build (operands converted in front of the MFMAs): it is
bit-equal across the launch partitions below, so the partitions are compared
with array_equal here."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_example_amd.data.mnist import PinnedEpoch, synthetic_mnist
from distributed_tensorflow_example_amd.models import mlp

pytestmark = pytest.mark.gpu

LR = 0.05
NB = 8          # distinct batches per data set: no step sees another step's batch


def _seed(B):
    return 100 + B


@functools.lru_cache(maxsize=None)
def _data(B):
    return synthetic_mnist(B * NB, seed=_seed(B))


@functools.lru_cache(maxsize=None)
def _reference(B, act, steps):
    """fp32 SGD (models/mlp.reference_step) from the trainer's initial
    parameters: (p0, final params, losses, accuracies); computed once per case."""
    imgs, labels = _data(B)
    p0 = mlp.FusedMLPTrainer(batch_size=B, lr=LR, act=act, device=torch.device("cuda")).get_params().cpu().clone()
    p = p0.clone()
    losses, accs = [], []
    for b in range(steps):
        x = torch.from_numpy(imgs[b * B:(b + 1) * B]).float() / 255.0
        y = torch.from_numpy(labels[b * B:(b + 1) * B])
        loss, acc = mlp.reference_step(p, x, y, LR, act)
        losses.append(loss.item())
        accs.append(acc.item())
    return p0, p, np.array(losses), np.array(accs)


def _run(B, act, steps, per_launch, precision="fp32"):
    imgs, labels = _data(B)
    dev = torch.device("cuda")
    tr = mlp.FusedMLPTrainer(batch_size=B, lr=LR, act=act, device=dev)
    run = mlp.PersistentMLPRunner(tr, PinnedEpoch(imgs, labels, B), steps_per_launch=per_launch, precision=precision)
    run.run(steps)
    torch.cuda.synchronize()
    assert run.error() == 0
    assert tr.global_step == steps
    return tr.get_params().cpu().numpy().copy(), np.asarray(tr.read_metrics(0, steps)).copy()


def _check_reference(B, act, steps, params, metrics):
    p0, p_ref, losses, accs = _reference(B, act, steps)
    d_k = torch.from_numpy(params).double() - p0.double()
    d_r = p_ref.double() - p0.double()
    rel = ((d_k - d_r).norm() / d_r.norm()).item()
    print(f"B={B} act={act} steps={steps}: param delta rel {rel:.3e}, "
          f"max loss diff {np.abs(metrics[:, 0] - losses).max():.3e}")
    assert rel < 2e-5, rel
    assert np.allclose(metrics[:, 0], losses, rtol=1e-5, atol=1e-5), (metrics[:, 0], losses)
    assert np.allclose(metrics[:, 1], accs, atol=1e-6)


@pytest.mark.parametrize("act", ["sigmoid", "relu"])
@pytest.mark.parametrize("B", [100, 37])
def test_operand_prep_launch_partition_bit_equal(native, B, act):
    """7 steps as one launch, as launches of 3, 3, 1 and as 7 launches of 1: the
    first step of a launch is prepared in the prologue, a later one in the
    previous step's windows, and a launch's last step prepares nothing."""
    outs = [_run(B, act, 7, spl) for spl in (7, 3, 1)]
    _check_reference(B, act, 7, *outs[0])
    for p, m in outs[1:]:
        assert np.array_equal(p, outs[0][0])
        assert np.array_equal(m, outs[0][1])


@pytest.mark.parametrize("B", [1, 17, 112])
def test_operand_prep_edge_batches(native, B):
    """A single row, one row into the second batch tile, and no padding at all:
    3 steps in launches of 2 and 1."""
    p, m = _run(B, "sigmoid", 3, 2)
    _check_reference(B, "sigmoid", 3, p, m)


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import test_mlp_persist_operand_prep_gpu as t
out = {}
for B, act in ((100, "sigmoid"), (37, "relu")):
    p, m = t._run(B, act, 7, 3)
    out[f"p_{B}_{act}"] = p
    out[f"m_{B}_{act}"] = m
np.savez(sys.argv[3], **out)
print("late-path child done")
"""


def test_operand_prep_late_path_same_bits(native, tmp_path):
    """DTF_PERSIST_DBG bit 2 (read once per process: a fresh child) makes every
    wave prepare the next step's operands after P2 instead of in the E2 window;
    parameters and metrics are array_equal to the default (early-path) run."""
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    dump = str(tmp_path / "late.npz")
    env = dict(os.environ, PYTHONPATH=repo, DTF_PERSIST_DBG="4")
    r = subprocess.run([sys.executable, "-c", _CHILD, repo, here, dump], capture_output=True, text=True, timeout=100,
                       env=env, cwd=repo)
    assert r.returncode == 0 and "late-path child done" in r.stdout, (r.stdout + r.stderr)[-3000:]
    late = np.load(dump)
    for B, act in ((100, "sigmoid"), (37, "relu")):
        p, m = _run(B, act, 7, 3)
        assert np.array_equal(late[f"p_{B}_{act}"], p), (B, act)
        assert np.array_equal(late[f"m_{B}_{act}"], m), (B, act)


def test_operand_prep_leaves_f32_mfma_engine_alone(native):
    """The f32-input MFMA engine (no PREP) still matches the reference and is
    bit-equal across launch partitions."""
    a = _run(100, "sigmoid", 7, 7, precision="fp32-mfma")
    b = _run(100, "sigmoid", 7, 3, precision="fp32-mfma")
    _check_reference(100, "sigmoid", 7, *a)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
