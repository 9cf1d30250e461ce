"""DeepFMTrainer's torch path (models/deepfm.py), the float64 reference itself (tests/deepfm_reference.py) and the
reference's preconditions for every case of tests/test_deepfm_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deepfm_reference as D  # noqa: E402
from distributed_tensorflow_example_amd.models import DeepFMTrainer  # noqa: E402
from test_fm_cpu import HP, ROW_TOL, STEPS, train_batch  # noqa: E402
from test_fm_gpu import F, _rows_batch  # noqa: E402

# (K, hidden, tile, B) of the rows kernel's test: K % 16 != 0 and LPR padding; a ragged second tile; eight column
# chunks; three hidden layers (layer 1's mask and S read from global memory)
ROWS_CASES = [(4, (16,), 16, 1), (20, (48, 16), 16, 17), (64, (64,), 32, 33), (128, (512, 256), 16, 37),
              (128, (64, 32, 16), 32, 37)]


def tower(rng, K, hidden, bias_std=0.1):
    dims = [K] + list(hidden) + [1]
    return [t for i in range(len(dims) - 1) for t in
            ((rng.standard_normal((dims[i], dims[i + 1])) * (2.0 / dims[i]) ** 0.5).astype(np.float32),
             (rng.standard_normal(dims[i + 1]) * bias_std).astype(np.float32))]


def rows_case(K, hidden, B):
    """test_fm_gpu._rows_batch cut to B rows, its tables, and a tower whose hidden biases D.settle_relu moved off 0."""
    labels, off, ids, vals = _rows_batch()
    batch = (labels[:B], off[:B + 1], ids[:off[B]], vals[:off[B]])
    rng = np.random.default_rng(K + len(hidden))
    w, V = (rng.standard_normal(F) * 0.3).astype(np.float32), (rng.standard_normal((F, K)) * 0.05).astype(np.float32)
    layers = tower(rng, K, hidden)
    D.settle_relu(batch, w, V, 0.25, layers)
    return batch, w, V, 0.25, layers


@pytest.mark.parametrize("K,hidden,tile,B", ROWS_CASES)
def test_preconditions_of_the_gpu_cases(K, hidden, tile, B):
    o, _ = D.check_preconditions(*rows_case(K, hidden, B))
    assert all((a > 0).any() and (a == 0).any() for a in o["act"][1:]), "both sides of every ReLU"


def check_steps(tr, kind, seed):
    """Three train_steps of `tr` against the float64 steps from the same start: w, V, b, the tower and every slot."""
    rng = np.random.default_rng(seed)
    tr.V.copy_(torch.from_numpy(rng.standard_normal(tuple(tr.V.shape)).astype(np.float32) * 0.3))
    tr.w.copy_(torch.from_numpy(rng.standard_normal(tr.w.numel()).astype(np.float32) * 0.3))
    for t in tr.layers[1::2]:
        t.copy_(torch.from_numpy(rng.standard_normal(t.numel()).astype(np.float32) * 0.1))
    dense = (tr.dense_optimizer, tr.dense_hp)
    ref, r32 = (D.init_state(kind, HP[kind], *dense, tr.w.cpu().numpy(), tr.V.cpu().numpy(), 0.0,
                             [t.cpu().numpy() for t in tr.layers]) for _ in range(2))
    tol = lambda x: ROW_TOL["atol"] + ROW_TOL["rtol"] * x.abs()    # noqa: E731
    tables = [tr.w, tr.V] + list(tr.w_slots.values()) + list(tr.V_slots.values())
    for step, layout in enumerate(STEPS):
        batch = train_batch(rng, **layout)
        untouched = np.setdiff1d(np.arange(tr.w.numel()), batch[2])
        before = [t[untouched].clone() for t in tables]
        for n in r32:                                   # the precondition's step starts from the reference's state
            r32[n] = [None if t is None else t.clone() for t in ref[n]]
        want, bound = D.step(kind, HP[kind], tr.lr, *dense, tr.dense_lr, ref, batch, step + 1)
        D.step(kind, HP[kind], tr.lr, *dense, tr.dense_lr, r32, batch, step + 1, np.float32)
        loss = tr.train_step(tuple(torch.from_numpy(x) for x in batch))
        assert abs(float(loss) - want) <= bound
        got = {"w": [tr.w] + list(tr.w_slots.values()), "V": [tr.V] + list(tr.V_slots.values()),
               "b": [tr.b] + [t for t in (tr._bopt.m[0], tr._bopt.v[0]) if t is not None]}
        for i, t in enumerate(tr.layers):
            got[f"L{i}"] = [t] + [s for s in (tr._dopt.m[i], tr._dopt.v[i]) if s is not None]
        for n in got:
            for g, w64, w32 in zip(got[n], ref[n], r32[n]):
                assert bool(((w32 - w64).abs() < 0.25 * tol(w64)).all()), "precondition: an fp32 gradient moves the reference"
                assert bool(((g.double().cpu().reshape(w64.shape) - w64).abs() <= tol(w64)).all()), f"{n} step {step}"
        assert all(torch.equal(t[untouched], t0) for t, t0 in zip(tables, before)), "an untouched row changed"


def trainer(kind, device, **kw):
    return DeepFMTrainer(300, factors=20, hidden=(32, 16), lr=0.1, dense_lr=0.01, device=device, optimizer=kind,
                         optimizer_hp=HP[kind], **kw)


@pytest.mark.parametrize("kind", ["sgd", "ftrl"])
def test_cpu_steps_against_float64(kind):
    tr = trainer(kind, "cpu")
    check_steps(tr, kind, seed=3)
    local, repl = tr.checkpoint_tensors()
    assert local == {} and {"fm/linear", "fm/factors", "fm/bias", "deepfm/hidden_0/kernel", "deepfm/hidden_1/bias",
                            "deepfm/logits/kernel", "deepfm/logits/kernel/Adam_1"} <= set(repl)
    with pytest.raises(ValueError):
        DeepFMTrainer(10, optimizer="adam", device="cpu")


def test_reference_gradient_against_central_differences():
    """w, V, every W_l and b_l and the bias; id 2 repeats inside row 0 and across rows: the shared-table term dz S + da_0."""
    rng = np.random.default_rng(0)
    Fs, K = 6, 4
    off, ids = np.array([0, 3, 4, 4, 7, 9]), np.array([2, 2, 5, 0, 1, 2, 6, 3, -1])
    batch = ((rng.random(5) < 0.5).astype(np.float64), off, ids, rng.uniform(0.5, 1.5, ids.size))
    w, V, b = rng.standard_normal(Fs), rng.standard_normal((Fs, K)) * 0.5, 0.3
    layers = [t.astype(np.float64) for t in tower(rng, K, (16,), 0.3)]
    gw, gV, gb, _, gl = D.grads(batch, w, V, b, layers)
    params, h = [w, V] + layers, 1e-6
    loss = lambda p, b=b: D.forward(batch, p[0], p[1], b, p[2:])["loss"].mean()    # noqa: E731
    for k, g in enumerate([gw, gV] + gl):
        for i in np.ndindex(params[k].shape):
            hi, lo = [t.copy() for t in params], [t.copy() for t in params]
            hi[k][i] += h
            lo[k][i] -= h
            assert abs((loss(hi) - loss(lo)) / (2 * h) - g.reshape(params[k].shape)[i]) <= 1e-8 + 1e-6 * abs(g.reshape(params[k].shape)[i])
    assert abs((loss(params, b + h) - loss(params, b - h)) / (2 * h) - gb) <= 1e-8
