"""The fused one-GPU Wide&Deep training step (csrc/kernels/wide_deep_train.hip
wd_train_rows, csrc/bind_wide_deep.cpp WideDeepTrainPlan, models/wide_deep.py
WideDeep(fused_step=True)) against the float64 model and the derived bounds of
tests/wide_deep_train_reference.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_deep_eval_reference as R  # noqa: E402
import wide_deep_train_reference as T  # noqa: E402
from test_wide_deep_eval_gpu import _cuda, _dev, _distinct_batch, _wd  # noqa: E402

pytestmark = pytest.mark.gpu


def _plan(native, fx, combiner="sum", tile=0):
    wide, emb = _cuda(fx[4]).reshape(-1, 1).contiguous(), _cuda(fx[5])
    plan = native.WideDeepTrainPlan(wide, emb, [_cuda(a) for a in fx[6]],
                                    torch.tensor([fx[7]], dtype=torch.float32, device="cuda"), combiner)
    plan.set_tile(tile)
    return plan


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _within(name, got, want, bound):
    """Every element within its bound; returns the largest error / bound ratio."""
    err = np.abs(_np(got).reshape(want.shape) - want)
    assert (err <= bound).all(), f"{name}: error {err.max():.3g} at bound {bound.reshape(-1)[err.argmax()]:.3g}"
    return float((err / np.maximum(bound, 1e-300)).max())


def _check_backward(plan, r, nh):
    ratios = [_within("dz", plan.dz(), r["dz"], r["dzb"]), _within("demb", plan.demb(), r["demb"], r["dembb"])]
    ratios += [_within(f"dzl[{l}]", plan.dzl(l), r["dzl"][l], r["dzlb"][l]) for l in range(1, nh + 1)]
    return max(ratios)


@pytest.mark.parametrize("D,hidden,tile,B", T.EXACT_CASES)
def test_exact_fixture(native, D, hidden, tile, B):
    fx = R.exact_fixture(B, D, hidden, R.exact_seed(D, B))
    r = T.backward(*fx[:8], exact_sum=True)
    plan = _plan(native, fx, tile=tile)
    assert plan.tile_for(B) == tile and plan.lds_bytes(tile) <= 160 * 1024
    plan.reserve(B)
    plan.scratch().fill_(float("nan"))
    plan.rows(*_dev(fx), 1.0 / B)
    for l in range(len(hidden) + 1):                                   # the forward is exact: bit for bit
        assert np.array_equal(_np(plan.act(l)), r["act"][l]), f"act[{l}]"
    assert np.array_equal(_np(plan.z()), r["m"]["z"])
    _check_backward(plan, r, len(hidden))
    R.check_rows(r["m"], loss32=_np(plan.lrow()))
    # every element of rows < B was written (the views above hold no NaN) and nothing else was
    assert int((~torch.isnan(plan.scratch())).sum()) == B * plan.row_floats()
    bad = plan.brow().cpu().numpy()
    assert bad.sum() == fx[8] == r["m"]["bad"]
    if B >= 12:        # row 7's out-of-range id is counted; the model skips it, so the bounds above hold as if it were absent
        assert bad[7] == 1 and fx[2][int(fx[1][7]) + 1] >= fx[5].shape[0]


@pytest.mark.parametrize("D,hidden,combiner,seed", T.RANDOM_CASES)
def test_random_fixture_inside_bounds(native, D, hidden, combiner, seed):
    fx = R.random_fixture(33, D, hidden, seed)
    r = T.backward(*fx[:8], combiner)
    for tile in (16, 32):
        plan = _plan(native, fx, combiner, tile)
        plan.rows(*_dev(fx), 1.0 / 33)
        R.check_rows(r["m"], z32=plan.z().cpu().numpy(), loss32=_np(plan.lrow()))
        ratio = _check_backward(plan, r, len(hidden))
        print(f"tile {tile}: largest backward error / bound {ratio:.3g}; mask margin {r['margin']:.3g}")
        again = [t.clone() for t in (plan.demb(), plan.dz(), plan.dzl(1))]
        plan.rows(*_dev(fx), 1.0 / 33)
        assert all(torch.equal(a, b) for a, b in zip(again, (plan.demb(), plan.dz(), plan.dzl(1))))   # the same bits


def _tensors(wd):
    return [wd.wide.local, wd.emb.local] + [p.data for p in wd.dense_params]


def test_widedeep_fused_step(native):
    D, hidden, lr = 16, (32, 16), 0.1
    fx = R.random_fixture(33, D, hidden, seed=1)
    batch = _distinct_batch(11)
    lab, off, ids, vals = (t.cpu().numpy() for t in batch)
    wd = _wd(fx, D, hidden, fused_step=True)
    assert wd._train_fused_ok()
    before = [_np(t) for t in _tensors(wd)]
    layers = [t.cpu().numpy() for t in _tensors(wd)[2:-1]]
    r = T.backward(lab, off, ids, vals, fx[4], fx[5], layers, fx[7])
    loss = wd.train_step(batch)
    assert wd.global_step == 1 and wd._native_train_plan().runs() == 1
    assert abs(float(loss) - r["m"]["mean"]) <= r["m"]["mean_bound"]
    lr32 = float(np.float32(lr))
    rows = np.repeat(np.arange(lab.size), np.diff(off))
    v = vals.astype(np.float64)[:, None]
    # the tables' gradients (no id repeats): v_j demb[row] and v_j dz[row]; three more roundings in v * g
    g = [np.zeros_like(before[0]), np.zeros_like(before[1])] + [x.reshape(b.shape) for x, b in zip(r["grads"], before[2:])]
    gb = [np.zeros_like(x) for x in g[:2]] + [x.reshape(b.shape) for x, b in zip(r["gradb"], before[2:])]
    g[0][ids], gb[0][ids] = v * r["dz"][rows, None], v * r["dzb"][rows, None]
    g[1][ids], gb[1][ids] = v * r["demb"][rows], v * r["dembb"][rows]
    for name, t, th, gi, gbi in zip(["wide", "emb", "W0", "b0", "W1", "b1", "w_last", "b_last", "bias"], _tensors(wd),
                                    before, g, gb):
        new = th - lr32 * gi
        ratio = _within(name, t, new, T.step_bound(new, gi, gbi, lr32))
        print(f"{name}: largest update error / bound {ratio:.3g}")
        assert not np.array_equal(_np(t), th)
    # a graphed model with static capacity: the eager fused model's bits over two steps, one capture
    a, b = _wd(fx, D, hidden, fused_step=True), _wd(fx, D, hidden, fused_step=True, ids_capacity=64 * 5 + 7, rows=64)
    b.enable_graph()
    for seed in (11, 12):
        la, lb = a.train_step(_distinct_batch(seed)), b.train_step(_distinct_batch(seed))
        assert torch.equal(la, lb)
    assert b._graphed.captures == 1 and b._graphed.replays == 2 and b.global_step == 2
    assert all(torch.equal(x, y) for x, y in zip(_tensors(a), _tensors(b)))
    loss, _ = b.evaluate(tuple(torch.from_numpy(x).cuda() for x in fx[:4]))   # the fused evaluation sees the trained tensors
    m = R.model(*fx[:4], *(x.cpu().numpy() for x in _tensors(b)[:2]), [x.cpu().numpy() for x in _tensors(b)[2:-1]],
                float(b.bias.detach()), 200)
    assert abs(float(loss) - m["mean"]) <= m["mean_bound"] + R.U * abs(m["mean"])


@pytest.mark.parametrize("kw,hidden", [(dict(sparse_opt="adagrad"), (32, 16)), (dict(), (8,))])
def test_other_configurations_train_as_today(native, kw, hidden):
    fx = R.random_fixture(33, 16, hidden, seed=3)
    a, b = _wd(fx, 16, hidden, fused_step=True, **kw), _wd(fx, 16, hidden, **kw)
    assert not a._train_fused_ok() and not b._train_fused_ok()
    assert torch.equal(a.train_step(_distinct_batch(11)), b.train_step(_distinct_batch(11)))
    assert all(torch.equal(x, y) for x, y in zip(_tensors(a), _tensors(b))) and a._train_plan is None


def test_refusals_launch_nothing(native):
    fx = R.exact_fixture(16, seed=2)
    plan = _plan(native, fx)
    lab, off, ids, vals = _dev(fx)
    plan.reserve(16)
    plan.scratch().fill_(-7.0)
    for args in [(lab.double(), off, ids, vals), (lab, off.int(), ids, vals), (lab, off, ids.int(), vals),
                 (lab, off, ids, vals.double()), (lab.cpu(), off, ids, vals), (lab, off, ids.cpu(), vals),
                 (lab, off[:-1].contiguous(), ids, vals), (lab, off, ids, vals[:-1].contiguous())]:
        with pytest.raises(RuntimeError):
            plan.rows(*args, 1.0 / 16)
    torch.cuda.synchronize()
    assert plan.runs() == 0 and bool((plan.scratch() == -7.0).all())
    assert not native.WideDeepTrainPlan.supported(16, [8]) and native.WideDeepTrainPlan.supported(128, [512, 512, 512])
    wide, emb = _cuda(fx[4]).reshape(-1, 1).contiguous(), _cuda(fx[5])
    with pytest.raises(RuntimeError, match="unsupported shape"):                # a hidden width of 8
        native.WideDeepTrainPlan(wide, emb, [torch.zeros(16, 8, device="cuda"), torch.zeros(8, device="cuda"),
                                             torch.zeros(8, 1, device="cuda"), torch.zeros(1, device="cuda")],
                                 torch.zeros(1, device="cuda"), "sum")
