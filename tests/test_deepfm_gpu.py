"""One-GPU DeepFM (csrc/kernels/deepfm.hip, DeepFMPlan, models/deepfm.py DeepFMTrainer) against the float64 reference
of tests/deepfm_reference.py, whose docstring derives every bound used here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deepfm_reference as D  # noqa: E402
import sparse_lr_eval_reference as E  # noqa: E402
from distributed_tensorflow_example_amd.models import DeepFMTrainer  # noqa: E402
from distributed_tensorflow_example_amd.optim.rules import RULES  # noqa: E402
from test_deepfm_cpu import ROWS_CASES, check_steps, rows_case, trainer  # noqa: E402
from test_fm_cpu import HP, train_batch  # noqa: E402

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("K,hidden,tile,B", ROWS_CASES)
def test_rows_against_float64(native, K, hidden, tile, B):
    batch, w, V, b, layers = rows_case(K, hidden, B)
    o, bd = D.check_preconditions(batch, w, V, b, layers)
    plan = native.DeepFMPlan(_cuda(w), _cuda(V), [_cuda(t) for t in layers], torch.tensor([b], device="cuda"))
    plan.set_tile(tile)
    plan.reserve(B, 0)
    print(f"K={K} hidden={hidden} tile={tile}: {plan.lds_bytes(tile)} B of LDS")
    nl, runs = len(hidden) + 1, []
    for _ in range(2):                                  # the second run: the same bits
        plan.scratch().fill_(float("nan"))
        plan.rows(*(_cuda(x) for x in batch), 1.0 / B)
        assert int((~torch.isnan(plan.scratch())).sum()) == B * plan.row_floats(), "written outside the batch's rows"
        runs.append(plan.scratch().clone())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    got = [("z", plan.z(), o["z"], bd["z"]), ("loss", plan.lrow(), o["loss"], bd["loss"]),
           ("dz", plan.dz().reshape(-1), o["dz"], bd["dz"]), ("demb", plan.demb(), o["demb"], bd["demb"])]
    got += [(f"act{l}", plan.act(l), o["act"][l], bd["act"][l]) for l in range(nl)]
    got += [(f"dzl{l}", plan.dzl(l), o["dzl"][l], bd["dzl"][l]) for l in range(1, nl)]
    for name, t, want, bound in got:
        err = np.abs(t.double().cpu().numpy() - want)
        print(f"  {name}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
        assert (err <= bound).all(), name
    assert np.array_equal(plan.brow().cpu().numpy(), o["brow"]) and o["brow"].sum() == (2 if B > 4 else 0)


@pytest.mark.parametrize("kind", [n for n, r in RULES.items() if r.row_local])
def test_train_steps_against_float64(kind):
    runs = []
    for _ in range(2):                                  # the same start twice: the same bits (one writer per element)
        tr = trainer(kind, "cuda")
        check_steps(tr, kind, seed=4)
        assert tr._native_plan().updates() == 3 and tr._native_plan().runs() == 3
        runs.append([t.clone() for t in tr._state_tensors()])
    assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_evaluation(monkeypatch):
    rng = np.random.default_rng(8)
    tr = trainer("sgd", "cuda", init_std=0.1, auc_bins=50)
    tr.w.copy_(_cuda((rng.standard_normal(300) * 0.5).astype(np.float32)))
    for t in tr.layers[1::2]:
        t.copy_(_cuda((rng.standard_normal(t.numel()) * 0.1).astype(np.float32)))
    assert tr._fused_ok()                               # (decided once, at the first question)
    monkeypatch.setenv("DTF_DFM_FUSED", "0")
    gen = trainer("sgd", "cuda", auc_bins=50)
    for d, s in zip(gen._state_tensors(), tr._state_tensors()):
        d.copy_(s)
    assert not gen._fused_ok()
    batches = [train_batch(rng, B, n) for B, n in ((5, 30), (48, 200), (17, 90))]
    layers = [t.cpu().numpy() for t in tr.layers]
    fs = [D.forward(bt, tr.w.cpu().numpy(), tr.V.cpu().numpy(), 0.0, layers) for bt in batches]
    bds = [D.bounds(f, layers) for f in fs]
    pos, neg = np.zeros(51, np.int64), np.zeros(51, np.int64)
    for bt, f, bd in zip(batches, fs, bds):
        for m in (tr, gen):
            loss, pred = m.evaluate(tuple(torch.from_numpy(x) for x in bt))
            assert abs(float(loss) - f["loss"].mean()) <= bd["loss"].mean()
            assert (np.abs(pred.double().cpu().numpy() - f["p"]) <= bd["p"]).all()
        tr.auc_update(tuple(torch.from_numpy(x) for x in bt))
        k = E.bins_of(tr.predict(tuple(torch.from_numpy(x) for x in bt)).cpu().numpy(), 50)      # the kernel's own p: exact bins
        pos += np.bincount(k[bt[0] != 0], minlength=51)
        neg += np.bincount(k[bt[0] == 0], minlength=51)
    assert np.array_equal(tr.auc_pos.cpu().numpy(), pos) and np.array_equal(tr.auc_neg.cpu().numpy(), neg)
    assert abs(tr.auc() - E.compute_auc(pos, neg)) <= 1e-6
    out = tr.evaluate_stream(tuple(torch.from_numpy(x) for x in bt) for bt in batches)
    assert out["rows"] == 70 and out["bad_ids"] == 6 and abs(out["auc"] - E.compute_auc(pos, neg)) <= 1e-6
    assert abs(out["loss"] * 70 - sum(f["loss"].sum() for f in fs)) <= sum(bd["loss"].sum() for bd in bds)
    assert tr.fused_eval_runs() == 3 * 4 and gen.fused_eval_runs() == 0


def test_refusals_and_graph(native):
    ok = native.DeepFMPlan.supported
    assert ok(20, [48, 16]) and not any((ok(6, [16]), ok(20, [24]), ok(20, [16, 16, 16, 16])))
    with pytest.raises(ValueError):
        DeepFMTrainer(300, factors=20, device="cuda", optimizer="adam")
    with pytest.raises(ValueError):
        DeepFMTrainer(300, factors=6, hidden=(16,), device="cuda")._fused_ok()
    eager, graphed = (trainer("ftrl", "cuda", init_std=0.3) for _ in range(2))
    graphed.enable_graph()
    rng = np.random.default_rng(2)
    for _ in range(3):                                  # three replays of one capture against three eager steps
        bt = tuple(torch.from_numpy(x) for x in train_batch(rng, n=400))
        le, lg = eager.train_step(bt), graphed.train_step(bt)
        assert torch.equal(le, lg) and all(torch.equal(x, y) for x, y in zip(eager._state_tensors(), graphed._state_tensors()))
    assert graphed._graphed.captures == 1 and graphed._graphed.replays == 3
