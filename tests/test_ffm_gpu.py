"""The one-GPU field-aware factorization machine (csrc/kernels/ffm.hip, FFMPlan, models/ffm.py FFMTrainer) against
the float64 reference of tests/ffm_reference.py, within R.bounds (derived there; t = R.chain(P, K))."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ffm_reference as R  # noqa: E402
import sparse_lr_eval_reference as E  # noqa: E402
from distributed_tensorflow_example_amd.models import FFMTrainer  # noqa: E402
from test_ffm_cpu import HP, ROW_LOCAL, bag_batch, check_steps  # noqa: E402

pytestmark = pytest.mark.gpu
F, B = 50, 37
KEYS = ("z", "loss", "dz", "dz_bag", "G")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows_batch(P):
    """37 rows of P bags.  Row 0: all bags empty; 1: one entry (no pair); 2: one entry per field; 3: only the first and
    the last field; 4: bags of 64 and 65 entries (the chunk edges); 5: 50 + 40 entries, the chunk edge inside the
    second bag; 6: id 9 twice in one bag and once in another field; then 0 .. 2 entries per bag.  Values in
    +-[0.5, 1.5] and one exact 0; ids -1 and F once each."""
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 3, (B, P))
    lens[:7] = 0
    lens[1, 1], lens[2], lens[3, 0], lens[3, P - 1] = 1, 1, 2, 3
    lens[4, :2], lens[5, :2], lens[6, :2] = (64, 65), (50, 40), (2, 1)
    off = np.concatenate([[0], np.cumsum(lens.ravel())]).astype(np.int64)
    ids = rng.integers(0, F, off[-1]).astype(np.int64)
    vals = (rng.uniform(0.5, 1.5, ids.size) * rng.choice([-1.0, 1.0], ids.size)).astype(np.float32)
    ids[off[6 * P]:off[6 * P + 2]] = 9
    ids[off[4 * P] + 2], ids[off[5 * P] + 70], vals[off[4 * P] + 3] = -1, F, 0.0
    return (rng.random(B) < 0.5).astype(np.float32), off, ids, vals


@pytest.mark.parametrize("P,K", [(2, 4), (3, 4), (5, 8), (16, 8), (32, 4)])
def test_rows_against_float64(native, P, K):
    rng = np.random.default_rng(P * K)
    batch = _rows_batch(P)
    w, V, b = (rng.standard_normal(F) * 0.3).astype(np.float32), (rng.standard_normal((F, P * K)) * 0.05).astype(np.float32), 0.25
    f, f32 = R.forward(batch, w, V, b, P), R.forward(batch, w, V, b, P, np.float32)
    bd = R.bounds(f, P, K)
    for k in KEYS:
        assert (np.abs(f32[k] - f[k]) <= 0.25 * bd[k]).all(), f"precondition: fp32 NumPy {k} outside a quarter of the bound"
    plan = native.FFMPlan(_cuda(w), _cuda(V), torch.tensor([b], device="cuda"), P)
    runs = []
    for _ in range(2):                                  # the same batch twice: the same bits
        plan.rows(*(_cuda(x) for x in batch), 1.0 / B)
        got = dict(z=plan.z(), loss=plan.lrow(), dz=plan.dz(), dz_bag=plan.dz_bag(), G=plan.demb())
        runs.append([t.clone() for t in got.values()] + [plan.brow().clone()])
    for k, t in got.items():
        err = np.abs(t.double().cpu().numpy() - f[k])
        print(f"P={P} K={K} {k}: max err / bound = {(err / np.maximum(bd[k], 1e-300)).max():.3g}")
        assert (err <= bd[k]).all(), k
    diag = got["G"].view(B, P, P, K)[:, torch.arange(P), torch.arange(P)]
    assert bool((diag == 0).all()) and bool((got["G"] != 0).any())
    assert np.array_equal(plan.brow().cpu().numpy(), f["brow"]) and f["brow"].sum() == 2
    assert all(torch.equal(x, y) for x, y in zip(*runs))


@pytest.mark.parametrize("kind", ROW_LOCAL)
def test_train_steps_against_float64(kind):
    runs = []
    for _ in range(2):                                  # the same start twice: the same bits (one writer per element)
        tr = FFMTrainer(300, num_fields=5, factors=4, lr=0.1, device="cuda", optimizer=kind, optimizer_hp=HP[kind])
        check_steps(tr, kind, seed=4)
        assert tr._native_plan().updates() == 3
        runs.append([t.clone() for t in tr._state_tensors()])
    assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_evaluation(monkeypatch):
    rng, P, K = np.random.default_rng(8), 5, 4
    tr = FFMTrainer(300, num_fields=P, factors=K, lr=0.1, device="cuda", init_std=0.2, auc_bins=50)
    tr.w.copy_(_cuda((rng.standard_normal(300) * 0.5).astype(np.float32)))
    assert tr._fused_ok()                               # (decided once, at the first question)
    monkeypatch.setenv("DTF_FFM_FUSED", "0")
    gen = FFMTrainer(300, num_fields=P, factors=K, lr=0.1, device="cuda", auc_bins=50)
    for d, s in zip(gen._state_tensors(), tr._state_tensors()):
        d.copy_(s)
    assert not gen._fused_ok()
    batches = [bag_batch(rng, P, B=n_rows, n=n) for n_rows, n in ((5, 30), (48, 200), (17, 90))]
    fs = [R.forward(bt, tr.w.cpu().numpy(), tr.V.cpu().numpy(), 0.0, P) for bt in batches]
    bds = [R.bounds(f, P, K) for f in fs]
    pos, neg = np.zeros(51, np.int64), np.zeros(51, np.int64)
    for bt, f, bd in zip(batches, fs, bds):
        tb = tuple(torch.from_numpy(x) for x in bt)
        for m in (tr, gen):
            loss, pred = m.evaluate(tb)
            assert abs(float(loss) - f["loss"].mean()) <= bd["loss"].mean()
            assert (np.abs(pred.double().cpu().numpy() - f["p"]) <= bd["p"]).all()
        tr.auc_update(tb)
        k = E.bins_of(tr.predict(tb).cpu().numpy(), 50)              # the kernel's own p: exact bins
        pos += np.bincount(k[bt[0] != 0], minlength=51)
        neg += np.bincount(k[bt[0] == 0], minlength=51)
    assert np.array_equal(tr.auc_pos.cpu().numpy(), pos) and np.array_equal(tr.auc_neg.cpu().numpy(), neg)
    out = tr.evaluate_stream(tuple(torch.from_numpy(x) for x in bt) for bt in batches)
    assert out["rows"] == 70 and out["bad_ids"] == 6 and abs(out["auc"] - E.compute_auc(pos, neg)) <= 1e-6
    assert abs(out["loss"] * 70 - sum(f["loss"].sum() for f in fs)) <= sum(bd["loss"].sum() for bd in bds)
    assert tr.fused_eval_runs() == 3 * 4 and gen.fused_eval_runs() == 0


def test_refusals_and_graph(native):
    assert not any(native.FFMPlan.supported(P, K) for P, K in ((33, 4), (2, 6), (17, 8), (1, 4)))
    assert native.FFMPlan.supported(22, 4)
    with pytest.raises(ValueError):
        FFMTrainer(300, num_fields=5, device="cuda", optimizer="adam")
    plan = native.FFMPlan(torch.zeros(F, device="cuda"), torch.zeros(F, 12, device="cuda"), torch.zeros(1, device="cuda"), 3)
    with pytest.raises(RuntimeError):                   # the row form's B + 1 offsets, refused before any launch
        plan.rows(torch.zeros(4, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda"),
                  torch.zeros(0, dtype=torch.int64, device="cuda"), None, 1.0)
    assert plan.runs() == 0
    eager, graphed = (FFMTrainer(300, num_fields=5, factors=4, lr=0.1, device="cuda", init_std=0.3, optimizer="ftrl",
                                 optimizer_hp=HP["ftrl"]) for _ in range(2))
    graphed.enable_graph()
    rng = np.random.default_rng(2)
    for _ in range(3):                                  # three replays of one capture against three eager steps
        bt = tuple(torch.from_numpy(x) for x in bag_batch(rng, 5, n=400))
        le, lg = eager.train_step(bt), graphed.train_step(bt)
        assert torch.equal(le, lg) and all(torch.equal(x, y) for x, y in zip(eager._state_tensors(), graphed._state_tensors()))
    assert graphed._graphed.captures == 1 and graphed._graphed.replays == 3
