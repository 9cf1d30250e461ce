"""FFMTrainer's torch path and ffm_batch (models/ffm.py) against the float64 reference of tests/ffm_reference.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ffm_reference as R  # noqa: E402
from distributed_tensorflow_example_amd.models import FFMTrainer, ffm_batch  # noqa: E402
from distributed_tensorflow_example_amd.optim.rules import RULES  # noqa: E402
from test_fm_cpu import HP, ROW_TOL, STEPS, train_batch  # noqa: E402

ROW_LOCAL = [n for n, r in RULES.items() if r.row_local]


def bag_batch(rng, P, **layout):
    """test_fm_cpu.train_batch (a hot id over the update's chunk edges, a repeated id, ids outside the table) with a
    random field per entry, in the bag form, as NumPy arrays."""
    labels, off, ids, vals = train_batch(rng, **layout)
    out = ffm_batch(labels, off, ids, vals, rng.integers(0, P, ids.size), P)
    return tuple(t.numpy() if torch.is_tensor(t) else t for t in out)


def check_steps(tr, kind, seed):
    """Three train_steps of `tr` against the float64 steps from the same start: w, V, b and every slot, within
    test_optim_rules_gpu.py's row tolerance; an fp32 autograd gradient moves the reference by under a quarter of it."""
    rng, P = np.random.default_rng(seed), tr.num_fields
    tr.V.copy_(torch.from_numpy(rng.standard_normal(tuple(tr.V.shape)).astype(np.float32) * 0.2))
    tr.w.copy_(torch.from_numpy(rng.standard_normal(tr.w.numel()).astype(np.float32) * 0.3))
    ref, r32 = (R.init_state(kind, HP[kind], tr.w.cpu().numpy(), tr.V.cpu().numpy(), 0.0) for _ in range(2))
    tol = lambda x: ROW_TOL["atol"] + ROW_TOL["rtol"] * x.abs()    # noqa: E731
    tables = [tr.w, tr.V] + list(tr.w_slots.values()) + list(tr.V_slots.values())
    for step, layout in enumerate(STEPS):
        batch = bag_batch(rng, P, **layout)
        untouched = np.setdiff1d(np.arange(tr.w.numel()), batch[2])
        before = [t[untouched].clone() for t in tables]
        for n in r32:                                   # the precondition's step starts from the reference's state
            r32[n] = [None if t is None else t.clone() for t in ref[n]]
        want, bound = R.step(kind, HP[kind], tr.lr, ref, batch, P)
        R.step(kind, HP[kind], tr.lr, r32, batch, P, torch.float32)
        loss = tr.train_step(tuple(torch.from_numpy(x) for x in batch))
        assert abs(float(loss) - want) <= bound
        got = {"w": [tr.w] + list(tr.w_slots.values()), "V": [tr.V] + list(tr.V_slots.values()),
               "b": [tr.b] + [t for t in (tr._bopt.m[0], tr._bopt.v[0]) if t is not None]}
        for n in got:
            for g, w64, w32 in zip(got[n], ref[n], r32[n]):
                assert bool(((w32 - w64).abs() < 0.25 * tol(w64)).all()), "precondition: an fp32 gradient moves the reference"
                assert bool(((g.double().cpu().reshape(w64.shape) - w64).abs() <= tol(w64)).all()), f"{n} step {step}"
        assert all(torch.equal(t[untouched], t0) for t, t0 in zip(tables, before)), "an untouched row changed"


@pytest.mark.parametrize("kind", ROW_LOCAL)
def test_cpu_steps_against_float64(kind):
    tr = FFMTrainer(300, num_fields=5, factors=4, lr=0.1, device="cpu", optimizer=kind, optimizer_hp=HP[kind])
    check_steps(tr, kind, seed=3)
    repl = tr.checkpoint_tensors()[1]
    assert all(f"ffm/{t}/{s}" in repl for t in ("linear", "factors", "bias") for s in tr.rule.slots) and "ffm/bias" in repl


def test_ffm_batch_groups_each_row_by_field():
    """Rows of fields (2, 0, 2, 1) and (1, 1), P = 3: equal fields keep their order, empty bags are kept."""
    labels, vals = np.array([1.0, 0.0], np.float32), np.arange(6, dtype=np.float32)
    got = ffm_batch(labels, np.array([0, 4, 6]), np.arange(10, 16), vals, np.array([2, 0, 2, 1, 1, 1]), 3)
    assert got[0] is labels and got[1].tolist() == [0, 1, 2, 4, 4, 6, 6]
    assert got[2].tolist() == [11, 13, 10, 12, 14, 15] and got[3].tolist() == [1, 3, 0, 2, 4, 5]
    with pytest.raises(ValueError):
        ffm_batch(labels, np.array([0, 4, 6]), np.arange(10, 16), None, np.array([3, 0, 2, 1, 1, 1]), 3)
    with pytest.raises(ValueError):
        FFMTrainer(10, num_fields=3, optimizer="adam", device="cpu")
