"""Fewer bytes through the hand-off memory path of the persistent fp32 MLP
engine (csrc/kernels/mlp_persist_f32.hip): the weight-gradient x^T operands
come from the row-major LDS image through transposing LDS reads
(ds_read_b64_tr_b8); the stage record carries no x^T copy and the image's rows
112..127 are zeroed once per launch.

Every case is compared with fp32 SGD (models/mlp.reference_step) at the
tolerances of test_mlp_persist_operand_prep_gpu.py: the batch sizes walk the
padding patterns of the 7 batch tiles (what a hand-off may and may not skip),
and the all-255 images make any leak from the zero rows or any permuted byte
of a transposing read a gradient error of order one."""
import functools

import numpy as np
import pytest
import torch

from distributed_tensorflow_example_amd.data.mnist import PinnedEpoch, synthetic_mnist
from distributed_tensorflow_example_amd.models import mlp

pytestmark = pytest.mark.gpu

LR = 0.05
NB = 4          # distinct batches per data set: no step sees another step's batch
STEPS = 3


@functools.lru_cache(maxsize=None)
def _data(B, kind):
    imgs, labels = synthetic_mnist(B * NB, seed=300 + B)
    if kind == "saturated":   # every pixel 255, random labels
        imgs = np.full_like(imgs, 255)
    return imgs, labels


@functools.lru_cache(maxsize=None)
def _reference(B, act, kind):
    """fp32 SGD from the trainer's initial parameters: (p0, final params, losses,
    accuracies); computed once per case."""
    imgs, labels = _data(B, kind)
    p0 = mlp.FusedMLPTrainer(batch_size=B, lr=LR, act=act, device=torch.device("cuda")).get_params().cpu().clone()
    p = p0.clone()
    losses, accs = [], []
    for b in range(STEPS):
        x = torch.from_numpy(imgs[b * B:(b + 1) * B]).float() / 255.0
        y = torch.from_numpy(labels[b * B:(b + 1) * B])
        loss, acc = mlp.reference_step(p, x, y, LR, act)
        losses.append(loss.item())
        accs.append(acc.item())
    return p0, p, np.array(losses), np.array(accs)


def _run(B, act, kind, precision="fp32"):
    """3 steps in launches of 2 and 1."""
    imgs, labels = _data(B, kind)
    dev = torch.device("cuda")
    tr = mlp.FusedMLPTrainer(batch_size=B, lr=LR, act=act, device=dev)
    run = mlp.PersistentMLPRunner(tr, PinnedEpoch(imgs, labels, B), steps_per_launch=2, precision=precision)
    run.run(STEPS)
    torch.cuda.synchronize()
    assert run.error() == 0
    assert tr.global_step == STEPS
    return tr.get_params().cpu().numpy().copy(), np.asarray(tr.read_metrics(0, STEPS)).copy()


def _check(B, act, kind, precision="fp32"):
    params, metrics = _run(B, act, kind, precision)
    p0, p_ref, losses, accs = _reference(B, act, kind)
    d_k = torch.from_numpy(params).double() - p0.double()
    d_r = p_ref.double() - p0.double()
    rel = ((d_k - d_r).norm() / d_r.norm()).item()
    print(f"B={B} act={act} {kind} {precision}: param delta rel {rel:.3e}, "
          f"max loss diff {np.abs(metrics[:, 0] - losses).max():.3e}, "
          f"max accuracy diff {np.abs(metrics[:, 1] - accs).max():.3e}")
    assert np.isfinite(params).all()
    assert rel < 2e-5, rel
    assert np.allclose(metrics[:, 0], losses, rtol=1e-5, atol=1e-5), (metrics[:, 0], losses)
    assert np.allclose(metrics[:, 1], accs, atol=1e-6), (metrics[:, 1], accs)


@pytest.mark.parametrize("B", [1, 16, 17, 100, 112])
def test_handoff_padding_patterns(native, B):
    """B = 1: one real row, six batch tiles all padding; 16: a tile boundary
    exactly, tile 1 all padding; 17: one row into tile 1; 100: the workload's
    pattern, tile 6 with 4 rows; 112: no padding row, only the class padding."""
    _check(B, "sigmoid", "synthetic")


@pytest.mark.parametrize("B", [112, 100])
def test_handoff_saturated_pixels(native, B):
    """Every pixel 255: the zero rows 112..127 of the LDS image (B = 112: all 16
    of them behind real rows; B = 100: behind the record's own zero rows) and the
    byte order of the transposing reads."""
    _check(B, "sigmoid", "saturated")


def test_handoff_f32_mfma_engine_transposing_reads(native):
    """The engine without the bf16 split takes its 4-row x^T dwords from
    transposing reads of two batch tiles' rows at once (its own row pattern)."""
    _check(37, "relu", "synthetic", precision="fp32-mfma")
