"""One-GPU DeepFM with fields (csrc/kernels/deepfm_fields.hip, DeepFMPlan(num_fields), DeepFMTrainer(num_fields))
against the float64 reference of tests/deepfm_fields_reference.py, whose docstring states every bound used here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deepfm_fields_reference as RF  # noqa: E402
import test_deepfm_gpu as TG  # noqa: E402
from test_deepfm_fields_cpu import ROWS_CASES, check_steps, rows_case, trainer  # noqa: E402
from test_ffm_cpu import ROW_LOCAL, bag_batch  # noqa: E402

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("P,K,hidden,tile,B", ROWS_CASES)
def test_rows_against_float64(native, P, K, hidden, tile, B):
    batch, w, V, b, layers = rows_case(P, K, hidden, B)
    o, bd = RF.check_preconditions(batch, w, V, b, layers)
    plan = native.DeepFMPlan(_cuda(w), _cuda(V), [_cuda(t) for t in layers], torch.tensor([b], device="cuda"), num_fields=P)
    plan.set_tile(tile)
    plan.reserve(B, 0)
    print(f"P={P} K={K} hidden={hidden} tile={tile}: {plan.lds_bytes(tile)} B of LDS")
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


# test_deepfm_gpu's training and evaluation tests as they stand (their tolerances, bit-equal second run, update and
# run counts, loss / predictions / AUC bins against the reference and the DTF_DFM_FUSED=0 path), on bag batches of
# three fields, this module's trainer and the field reference
test_train_steps_against_float64 = pytest.mark.parametrize("kind", ROW_LOCAL)(
    RF.rebind(TG.test_train_steps_against_float64, trainer=trainer, check_steps=check_steps))
test_evaluation = RF.rebind(TG.test_evaluation, D=RF, trainer=trainer,
                            train_batch=lambda rng, B, n: bag_batch(rng, 3, B=B, n=n))


def test_refusals_and_graph(native):
    ok = native.DeepFMPlan.supported
    assert ok(8, [512, 256], 39) and not any((ok(8, [16], 65), ok(128, [16], 5), ok(6, [16], 2)))
    tr = trainer("sgd", "cuda")
    rng = np.random.default_rng(2)
    labels, off, ids, vals = (_cuda(x) for x in bag_batch(rng, 3, n=400))
    with pytest.raises(RuntimeError):                   # B + 1 offsets: rows, not bags
        tr._native_plan().rows(labels, off[::3].contiguous(), ids, vals, 1.0)
    eager, graphed = (trainer("ftrl", "cuda", init_std=0.3) for _ in range(2))
    graphed.enable_graph()
    for _ in range(3):                                  # three replays of one capture against three eager steps
        bt = tuple(torch.from_numpy(x) for x in bag_batch(rng, 3, n=400))
        le, lg = eager.train_step(bt), graphed.train_step(bt)
        assert torch.equal(le, lg) and all(torch.equal(x, y) for x, y in zip(eager._state_tensors(), graphed._state_tensors()))
    assert graphed._graphed.captures == 1 and graphed._graphed.replays == 3
