"""The head of the persistent fp32 MLP step (csrc/kernels/mlp_persist_f32.hip):
the per-row loss / hit run after the dz2 / dz3 / a2 stores and in workgroup 0
alone, the label's probability is reduced only for the naive loss, and a head
wave sets two flags -- the first (all a weight-gradient chunk waits for) behind
the dz2 pieces, the second behind the tile's dW2 / db2 partial and, in
workgroup 0, its loss / hit rows; wave 7 waits for the seven second flags before
its fold and its metric reduction.

Every sum keeps its operands and its order, so the launch partitions and the
forced one-flag order (DTF_PERSIST_DBG bit 4: the chunks wait for the second
flag) are compared with array_equal; the metrics of every step are compared
with the fp32 reference at the tolerances of
tests/test_mlp_persist_operand_prep_gpu.py.

The naive loss -sum(y log softmax) of the reference must be finite for a case
to say anything (asserted).  With the trainer's N(0, 1) initial weights it is
for sigmoid (the smallest label probability of a row is ~4e-11) and is not for
relu: the logits reach hundreds, a softmax probability underflows to 0 in fp32
and the reference's 0 * log(0) is NaN at every B.  The relu naive cases
therefore start from the same weights scaled by W_SMALL, where it is finite."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_example_amd.data.mnist import PinnedEpoch
from distributed_tensorflow_example_amd.models import mlp

from test_mlp_persist_operand_prep_gpu import LR, _data

pytestmark = pytest.mark.gpu

STEPS = 7
W_SMALL = 0.05


def _scale(act, naive):
    """Initial-weight scale of a case (see the module doc)."""
    return W_SMALL if (naive and act == "relu") else 1.0


@functools.lru_cache(maxsize=None)
def _reference(B, act, scale=1.0):
    """fp32 SGD from the trainer's initial parameters (mlp.init_params, seed 1):
    (p0, final params, [STEPS] stable losses, naive losses, accuracies).  The
    gradient does not depend on the form of the loss.  Computed once per case."""
    imgs, labels = _data(B)
    p0 = mlp.init_params(1) * scale
    p = p0.clone()
    stable, naive, accs = [], [], []
    for b in range(STEPS):
        x = torch.from_numpy(imgs[b * B:(b + 1) * B]).float() / 255.0
        y = torch.from_numpy(labels[b * B:(b + 1) * B])
        ln, _, _ = mlp.reference_loss_and_grad(p, x, y, act, naive=True)
        ls, acc, g = mlp.reference_loss_and_grad(p, x, y, act, naive=False)
        p.sub_(LR * g)
        stable.append(ls.item())
        naive.append(ln.item())
        accs.append(acc.item())
    return p0, p, np.array(stable), np.array(naive), np.array(accs)


def _run(B, act, per_launch, naive=False, ring=8192, precision="fp32"):
    """STEPS steps in launches of `per_launch`: (params, metrics of steps 0..STEPS-1
    as the ring holds them -- with ring < STEPS a wrapped slot shows a later step)."""
    imgs, labels = _data(B)
    dev = torch.device("cuda")
    tr = mlp.FusedMLPTrainer(batch_size=B, lr=LR, act=act, device=dev, naive_loss=naive, metrics_ring=ring)
    if _scale(act, naive) != 1.0:
        tr.set_params(mlp.init_params(1) * _scale(act, naive))
    run = mlp.PersistentMLPRunner(tr, PinnedEpoch(imgs, labels, B), steps_per_launch=per_launch, precision=precision)
    run.run(STEPS)
    torch.cuda.synchronize()
    assert run.error() == 0
    assert tr.global_step == STEPS
    return tr.get_params().cpu().numpy().copy(), np.asarray(tr.read_metrics(0, STEPS)).copy()


def _check_reference(B, act, naive, params, metrics, steps=None):
    """Parameters and the metric rows `metrics[i]` of reference steps `steps[i]`."""
    p0, p_ref, stable, nv, accs = _reference(B, act, _scale(act, naive))
    steps = np.arange(STEPS) if steps is None else np.asarray(steps)
    losses = (nv if naive else stable)[steps]
    assert np.isfinite(losses).all(), losses
    d_k = torch.from_numpy(params).double() - p0.double()
    d_r = p_ref.double() - p0.double()
    rel = ((d_k - d_r).norm() / d_r.norm()).item()
    print(f"B={B} act={act} naive={naive}: param delta rel {rel:.3e}, "
          f"max loss diff {np.abs(metrics[:, 0] - losses).max():.3e}, "
          f"max acc diff {np.abs(metrics[:, 1] - accs[steps]).max():.3e}")
    assert rel < 2e-5, rel
    assert np.allclose(metrics[:, 0], losses, rtol=1e-5, atol=1e-5), (metrics[:, 0], losses)
    assert np.allclose(metrics[:, 1], accs[steps], atol=1e-6), (metrics[:, 1], accs[steps])


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("act", ["sigmoid", "relu"])
@pytest.mark.parametrize("B", [1, 16, 17, 100, 112])
def test_head_metrics_of_every_step(native, B, act, naive):
    """One row; a full tile; a tile plus one row; the benchmark's batch (4 valid
    rows in tile 6); all tiles full -- loss and accuracy of all 7 ring slots."""
    p, m = _run(B, act, STEPS, naive=naive)
    _check_reference(B, act, naive, p, m)


CUTS = (7, 3, 1)
CUT_CASES = ((100, "sigmoid"), (37, "relu"))
NAIVE_CASES = ((100, "sigmoid"), (17, "relu"))   # the naive loss's branch of the row metrics, in 3 + 3 + 1


@pytest.mark.parametrize("B,act", CUT_CASES)
def test_head_launch_partition_bit_equal(native, B, act):
    """7 steps as one launch, as 3 + 3 + 1 and as 7 launches of 1."""
    outs = [_run(B, act, spl) for spl in CUTS]
    _check_reference(B, act, False, *outs[0])
    for p, m in outs[1:]:
        assert np.array_equal(p, outs[0][0])
        assert np.array_equal(m, outs[0][1])


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import test_mlp_persist_head_gpu as t
out = {}
for B, act in t.CUT_CASES:
    for spl in t.CUTS:
        p, m = t._run(B, act, spl)
        out[f"p_{B}_{act}_{spl}"] = p
        out[f"m_{B}_{act}_{spl}"] = m
for B, act in t.NAIVE_CASES:
    p, m = t._run(B, act, 3, naive=True)
    out[f"p_{B}_{act}_naive"] = p
    out[f"m_{B}_{act}_naive"] = m
np.savez(sys.argv[3], **out)
print("one-flag child done")
"""


def test_head_flag_order_same_bits(native, tmp_path):
    """DTF_PERSIST_DBG bit 4 (read once per process: a fresh child) makes the
    chunks wait for the second head flag -- one flag behind the dW2 / db2 partial
    and the metric rows.  Same cuts, and two naive-loss runs for that branch of
    the row metrics; parameters and metrics are array_equal to the default
    two-flag run."""
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    dump = str(tmp_path / "oneflag.npz")
    env = dict(os.environ, PYTHONPATH=repo, DTF_PERSIST_DBG="16")
    r = subprocess.run([sys.executable, "-c", _CHILD, repo, here, dump], capture_output=True, text=True, timeout=100,
                       env=env, cwd=repo)
    assert r.returncode == 0 and "one-flag child done" in r.stdout, (r.stdout + r.stderr)[-3000:]
    forced = np.load(dump)
    for B, act in CUT_CASES:
        for spl in CUTS:
            p, m = _run(B, act, spl)
            assert np.array_equal(forced[f"p_{B}_{act}_{spl}"], p), (B, act, spl)
            assert np.array_equal(forced[f"m_{B}_{act}_{spl}"], m), (B, act, spl)
    for B, act in NAIVE_CASES:
        p, m = _run(B, act, 3, naive=True)
        assert np.isfinite(m).all(), m
        assert np.array_equal(forced[f"p_{B}_{act}_naive"], p), (B, act)
        assert np.array_equal(forced[f"m_{B}_{act}_naive"], m), (B, act)


@pytest.mark.parametrize("per_launch", [7, 3])
def test_head_wrapped_ring_holds_the_right_steps(native, per_launch):
    """A 5-slot ring wrapped by 7 steps: slots 0, 1 hold steps 5, 6 and slots
    2..4 steps 2..4 -- a stale or missing second flag in wave 7's reduction would
    leave another step's rows in a slot."""
    p, m = _run(100, "sigmoid", per_launch, ring=5)
    _check_reference(100, "sigmoid", False, p, m, steps=[5, 6, 2, 3, 4, 5, 6])
    # the rows are distinguishable: no two steps share a loss
    assert len(set(np.round(_reference(100, "sigmoid")[2], 4))) == STEPS


def test_head_f32_mfma_engine(native):
    """The f32-input MFMA engine shares the head."""
    p, m = _run(100, "sigmoid", STEPS, precision="fp32-mfma")
    _check_reference(100, "sigmoid", False, p, m)
