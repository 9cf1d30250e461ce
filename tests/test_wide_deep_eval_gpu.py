"""The forward-only Wide&Deep evaluation on the GPU (csrc/kernels/wide_deep_eval.hip
wd_eval_rows + the shared record reduce, csrc/bind_wide_deep.cpp
WideDeepEvalPlan, models/wide_deep.py) against the float64 model and derived
bounds of tests/wide_deep_eval_reference.py.

Exact fixture: z bit for bit, every bin and both histograms exactly.  Random
fixtures: z, p and the loss per row inside their bounds; a bin differs from the
model's only next to a threshold within the row's own bound."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_deep_eval_reference as R  # noqa: E402
from eval_record_util import SENT, _check_sentinels, _outs, _read, _record  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 5000


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _plan(native, fx, combiner="sum", tile=0):
    """(plan, the tensors it holds): wide [F, 1], emb [F, D], layers, bias."""
    wide = _cuda(fx[4]).reshape(-1, 1).contiguous()
    emb = _cuda(fx[5])
    layers = [_cuda(a) for a in fx[6]]
    bias = torch.tensor([fx[7]], dtype=torch.float32, device="cuda")
    plan = native.WideDeepEvalPlan(wide, emb, layers, bias, combiner)
    plan.set_tile(tile)
    return plan, (wide, emb, layers, bias)


def _dev(fx):
    lab, off, ids, vals = fx[:4]
    return (_cuda(lab).reshape(-1), _cuda(off), _cuda(ids), None if vals is None else _cuda(vals))


def _row_losses(plan, B):
    """The fp32 row losses, probabilities and bad counts the rows kernel left in
    the plan's scratch (lrow | prow | brow, one third each)."""
    sc = plan.scratch()
    cap = sc.numel() // 3
    return (sc[:B].cpu().numpy().astype(np.float64), sc[cap:cap + B].cpu().numpy(),
            sc[2 * cap:2 * cap + B].view(torch.int32).cpu().numpy())


def _exact_checks(plan, fx, B, Ts):
    """Evaluate the exact fixture once per T and compare everything exactly."""
    for T in Ts:
        m = R.model(*fx[:8], T, exact_sum=True)
        big_rec, rec = _record(T)
        big_out, pred, logits = _outs(B)
        plan.evaluate(*_dev(fx), rec, True, pred, logits)
        ls, rows, bad, pos, neg = _read(rec, T)
        _check_sentinels(big_rec, big_out, B)
        z = logits.cpu().numpy()
        assert np.array_equal(z.astype(np.float64), m["z"])                     # bit for bit
        rl, rp, rb = _row_losses(plan, B)
        k = R.check_rows(m, z32=z, p32=pred.cpu().numpy(), loss32=rl)
        assert np.array_equal(rp, pred.cpu().numpy())
        assert np.array_equal(k, m["bins"])                                      # every bin
        assert np.array_equal(pos, m["pos"]) and np.array_equal(neg, m["neg"])   # both histograms
        assert rows == B and bad == fx[8] == m["bad"] and rb.sum() == bad
        assert abs(ls - m["loss_sum"]) <= B * m["mean_bound"]
        assert abs(ls - float(rl.sum())) <= 4 * B * 2.0 ** -53 * abs(ls)          # the record summed these very values
    return m, z, rb


# ------------------------------------------------------------------ kernel: exact
@pytest.mark.parametrize("D,hidden,tile,B", R.EXACT_CASES)
def test_exact_fixture_bit_for_bit(native, D, hidden, tile, B):
    fx = R.exact_fixture(B, D, hidden, R.exact_seed(D, B))
    plan, _ = _plan(native, fx, tile=tile)
    assert plan.tile_for(B) == tile
    m, z, rb = _exact_checks(plan, fx, B, R.EXACT_T)
    if B >= 12:
        assert rb[7] == 1 and rb.sum() == 1 and fx[0][10, 0] == 0.5        # the out-of-range id, the float label
        assert {0, 1, 64, 65, 130} <= set(np.diff(fx[1]).tolist())
    assert plan.eval_runs() == len(R.EXACT_T)


def test_exact_fixture_large_tower(native):
    """The widest supported tower and D (two columns per lane, eight column
    chunks, 32 K blocks), every sum exact: bit for bit at both tiles."""
    fx = R.exact_fixture(33, 128, (512, 256), seed=31)
    for tile in (16, 32):
        plan, _ = _plan(native, fx, tile=tile)
        _exact_checks(plan, fx, 33, (200,))
    plan.set_tile(0)                    # the automatic rule: 32 rows only for narrow towers from 16384 rows
    assert plan.tile_for(33) == 16 and plan.tile_for(1 << 20) == 16
    narrow, _ = _plan(native, R.exact_fixture(1, 16, (32, 16), seed=1))
    assert narrow.tile_for(16383) == 16 and narrow.tile_for(16384) == 32
    fx = R.exact_fixture(17, 128, (512, 512, 512), seed=32)
    plan, _ = _plan(native, fx, tile=32)
    assert plan.lds_bytes(32) == 4 * 32 * 1032 + 8 * 32 <= 160 * 1024
    _exact_checks(plan, fx, 17, (200,))


@pytest.mark.parametrize("tile", [16, 32])
def test_no_values_means_one(native, tile):
    fx = R.exact_fixture(33, seed=21, with_vals=False)
    assert fx[3] is None
    plan, _ = _plan(native, fx, tile=tile)
    _exact_checks(plan, fx, 33, (200,))


@pytest.mark.parametrize("target", [40.0, -40.0])
def test_logit_of_plus_minus_40_through_the_shared_bias(native, target):
    fx = R.exact_fixture(33, seed=21)
    z0 = R.model(*fx[:8], 200, exact_sum=True)["z"][2]
    fx = fx[:7] + (target - float(z0),) + fx[8:]
    plan, _ = _plan(native, fx)
    for T in R.EXACT_T:
        m, z, _ = _exact_checks(plan, fx, 33, (T,))
        assert z[2] == target
        assert m["bins"][2] == (T - 1 if target > 0 else 1)                      # the edge bins


# ------------------------------------------------------------------ kernel: random
@pytest.mark.parametrize("D,hidden,combiner,seed", R.RANDOM_CASES)
def test_random_fixture_inside_bounds(native, D, hidden, combiner, seed):
    B = 33
    fx = R.random_fixture(B, D, hidden, seed)
    m = R.model(*fx[:8], 200, combiner)
    for tile in (16, 32):
        plan, _ = _plan(native, fx, combiner, tile)
        big_rec, rec = _record(200)
        big_out, pred, logits = _outs(B)
        plan.evaluate(*_dev(fx), rec, True, pred, logits)
        ls, rows, bad, pos, neg = _read(rec, 200)
        _check_sentinels(big_rec, big_out, B)
        z, p = logits.cpu().numpy(), pred.cpu().numpy()
        rl, _, rb = _row_losses(plan, B)
        err = abs(ls / B - m["mean"])
        print(f"tile {tile}: max z error / bound {np.max(np.abs(z - m['z']) / m['zb']):.3g}; max row loss error / "
              f"bound {np.max(np.abs(rl - m['loss']) / m['lb']):.3g}; mean loss error {err:.3g} (bound "
              f"{m['mean_bound']:.3g})")
        k = R.check_rows(m, z32=z, p32=p, loss32=rl)
        # the reduce bins the kernel's own fp32 p exactly as the shared threshold function does
        assert np.array_equal(pos, np.bincount(k[m["positive"]], minlength=201))
        assert np.array_equal(neg, np.bincount(k[~m["positive"]], minlength=201))
        R.check_histograms(pos, neg, m)
        assert rows == B and bad == 0 and not rb.any() and err <= m["mean_bound"]


# ------------------------------------------------------------------ record handling
def test_record_accumulates_resets_and_repeats(native):
    fx = R.random_fixture(65, 20, (48, 16), seed=2)
    lab, off, ids, vals = fx[:4]
    plan, _ = _plan(native, fx, "mean")
    _, whole = _record(200)
    plan.evaluate(*_dev(fx), whole, True)
    _, again = _record(200)
    plan.evaluate(*_dev(fx), again, True)
    assert torch.equal(whole, again)                                             # two runs, the same bits
    _, parts = _record(200)
    cuts = [0, 1, 33, 65]
    for c, (r0, r1) in enumerate(zip(cuts[:-1], cuts[1:])):
        s, e = int(off[r0]), int(off[r1])
        part = (lab[r0:r1], off[r0:r1 + 1] - off[r0], ids[s:e], vals[s:e])
        plan.evaluate(*_dev(part), parts, c == 0)
    a, b = _read(whole, 200), _read(parts, 200)
    assert a[1:3] == b[1:3] == (65, 0) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    assert abs(a[0] - b[0]) <= 4 * 2.0 ** -53 * abs(a[0])
    plan.evaluate(*_dev(fx), parts, False)                                       # accumulates on
    c = _read(parts, 200)
    assert c[1] == 130 and np.array_equal(c[3], 2 * a[3]) and abs(c[0] - 2 * a[0]) <= 8 * 2.0 ** -53 * c[0]
    plan.evaluate(*_dev(fx), parts, True)                                        # reset restarts
    assert torch.equal(parts, whole)
    assert plan.eval_runs() == 7


def test_nan_prefill_scratch_and_outputs(native):
    """Everything the kernels write is written for every row, and nothing else:
    NaN-filled outputs and scratch, sentinels around record and outputs."""
    fx = R.exact_fixture(33, seed=21)
    m = R.model(*fx[:8], 200, exact_sum=True)
    plan, _ = _plan(native, fx)
    _, rec = _record(200)
    plan.evaluate(*_dev(fx), rec, True)                   # allocates the scratch
    sc = plan.scratch()
    cap = sc.numel() // 3
    sc.fill_(float("nan"))
    nanbits = int(sc[:1].view(torch.int32))
    big_rec, rec2 = _record(200)
    big_out, pred, logits = _outs(33)
    plan.evaluate(*_dev(fx), rec2, True, pred, logits)
    _check_sentinels(big_rec, big_out, 33)
    assert torch.equal(rec, rec2) and plan.scratch().data_ptr() == sc.data_ptr()
    h = sc.cpu()
    for part in range(3):
        rows = h[part * cap:part * cap + 33]
        rest = h[part * cap + 33:(part + 1) * cap]
        assert (rest.view(torch.int32) == nanbits).all()                         # nothing past row B - 1
        assert not torch.isnan(rows).any() if part < 2 else (rows.view(torch.int32) != nanbits).all()
    assert np.array_equal(logits.cpu().numpy().astype(np.float64), m["z"])


def test_evaluation_replays_in_a_graph(native):
    from distributed_tensorflow_example_amd.utils.graphs import GraphedStep

    fx = R.random_fixture(33, 64, (64, 32), seed=13)
    plan, _ = _plan(native, fx, "sqrtn")
    _, once = _record(200)
    plan.evaluate(*_dev(fx), once, True)
    rec = torch.zeros_like(once)
    g = GraphedStep(lambda lab, off, ids, vals: plan.evaluate(lab, off, ids, vals, rec, False), lambda: [rec])
    for _ in range(3):
        g(*_dev(fx))
    assert g.captures == 1 and g.replays == 3
    a, b = _read(once, 200), _read(rec, 200)
    assert b[1] == 3 * a[1] and np.array_equal(b[3], 3 * a[3]) and np.array_equal(b[4], 3 * a[4])
    assert abs(b[0] - 3 * a[0]) <= 8 * 2.0 ** -53 * abs(b[0])
    # a larger eager batch outgrows the plan's scratch; the captured graph's stays alive
    big = R.random_fixture(1100, 64, (64, 32), seed=13)
    _, other = _record(200)
    plan.evaluate(*_dev(big), other, True)
    assert _read(other, 200)[1] == 1100
    g(*_dev(fx))
    c = _read(rec, 200)
    assert g.captures == 1 and c[1] == 4 * a[1] and np.array_equal(c[3], 4 * a[3]) and np.array_equal(c[4], 4 * a[4])


def test_refusals_launch_nothing(native):
    fx = R.exact_fixture(16, seed=2)
    plan, (wide, emb, layers, bias) = _plan(native, fx)
    lab, off, ids, vals = _dev(fx)
    big, rec = _record(200)
    bad_calls = [
        (lab.double(), off, ids, vals, rec, True),                               # labels not fp32
        (lab, off.int(), ids, vals, rec, True),                                  # offsets not int64
        (lab, off[:-1].contiguous(), ids, vals, rec, True),                      # not B + 1 offsets
        (lab, off, ids.int(), vals, rec, True),                                  # ids not int64
        (lab, off, ids, vals[:-1].contiguous(), rec, True),                      # one value per id
        (lab.cpu(), off, ids, vals, rec, True),                                  # a host tensor
        (lab, off, ids, vals, rec[:-1], True),                                   # a record of the wrong length
        (lab, off, ids, vals, torch.zeros(8, dtype=torch.int64, device="cuda"), True),   # T < 2
        (lab, off, ids, vals, rec.int(), True),
        (lab, off, ids, vals, rec, True, torch.zeros(15, device="cuda"), None),  # pred != B
        (lab, off, ids, vals, rec, True, None, torch.zeros(17, device="cuda")),  # logits != B
    ]
    for args in bad_calls:
        with pytest.raises(RuntimeError):
            plan.evaluate(*args)
    torch.cuda.synchronize()
    assert plan.eval_runs() == 0 and (big == SENT).all()
    # unsupported shapes are refused when the plan is built
    assert not native.WideDeepEvalPlan.supported(6, [16]) and not native.WideDeepEvalPlan.supported(16, [8])
    assert not native.WideDeepEvalPlan.supported(16, [16, 16, 16, 16]) and not native.WideDeepEvalPlan.supported(132, [16])
    assert not native.WideDeepEvalPlan.supported(16, [528]) and native.WideDeepEvalPlan.supported(128, [512, 512, 512])
    with pytest.raises(RuntimeError, match="unsupported shape"):
        native.WideDeepEvalPlan(wide, emb[:, :6].contiguous(), [torch.zeros(6, 16, device="cuda"), layers[1][:16].contiguous(),
                                                               torch.zeros(16, 1, device="cuda"), layers[-1]], bias, "sum")
    with pytest.raises(RuntimeError):
        native.WideDeepEvalPlan(wide, emb, layers, bias, "max")
    plan.evaluate(lab, off, ids, vals, rec, True)
    assert plan.eval_runs() == 1 and _read(rec, 200)[1] == 16


# ------------------------------------------------------------------ WideDeep
def _wd(fx, D, hidden, combiner="sum", **kw):
    from distributed_tensorflow_example_amd.models.wide_deep import WideDeep
    from distributed_tensorflow_example_amd.parallel.world import World

    m = WideDeep(F, emb_dim=D, hidden=hidden, lr=0.1, world=World(device=torch.device("cuda", 0)), combiner=combiner,
                 **kw)
    with torch.no_grad():
        m.wide.local.copy_(torch.from_numpy(fx[4]).reshape(-1, 1))
        m.emb.local.copy_(torch.from_numpy(fx[5]))
        for p, a in zip(m.layers, fx[6]):
            p.data.copy_(torch.from_numpy(a).reshape(p.shape))
        m.bias.data.fill_(float(fx[7]))
    return m


_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import wide_deep_eval_reference as R
from test_wide_deep_eval_gpu import _wd
fx = R.random_fixture(33, 20, (48, 16), seed=2)
wd = _wd(fx, 20, (48, 16), "mean")
assert not wd._eval_fused_ok()
batch = tuple(torch.from_numpy(a).cuda() for a in fx[:4])
loss, p = wd.evaluate(batch)
wd.auc_update(batch)
st = wd.evaluate_stream([batch, batch])
assert wd.fused_eval_runs() == 0
np.savez(sys.argv[2], loss=float(loss), p=p.cpu().numpy(), pos=wd.auc_pos.cpu().numpy(), neg=wd.auc_neg.cpu().numpy(),
         auc=wd.auc(), sloss=st["loss"], sauc=st["auc"], srows=st["rows"], sbad=st["bad_ids"])
"""


def test_widedeep_against_model_and_general_path(native, tmp_path):
    fx = R.random_fixture(33, 20, (48, 16), seed=2)
    m = R.model(*fx[:8], 200, "mean")
    wd = _wd(fx, 20, (48, 16), "mean")
    assert wd._eval_fused_ok() and wd.fused_eval_runs() == 0
    dev_batch = tuple(torch.from_numpy(a).cuda() for a in fx[:4])
    host_batch = tuple(fx[:4])
    recs = []
    for batch in (dev_batch, host_batch, tuple(torch.from_numpy(a) for a in fx[:4])):
        loss, p = wd.evaluate(batch)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and p.shape == (33,)
        assert abs(float(loss) - m["mean"]) <= m["mean_bound"] + R.U * abs(m["mean"])
        R.check_rows(m, p32=p.cpu().numpy())
        recs.append((wd._eval_rec.clone(), p.clone()))
    for rec, p in recs[1:]:                                                      # device and host batches: one record
        assert torch.equal(rec, recs[0][0]) and torch.equal(p, recs[0][1])
    assert wd.fused_eval_runs() == 3
    wd.auc_update(dev_batch)
    wd.auc_update(host_batch)
    R.check_histograms(wd.auc_pos.cpu().numpy(), wd.auc_neg.cpu().numpy(), [m, m])
    auc2 = wd.auc()
    wd.reset_auc()
    assert int(wd.auc_pos.sum()) == 0 and int(wd.auc_neg.sum()) == 0
    wd.auc_update(host_batch)
    pos, neg = wd.auc_pos.cpu().numpy(), wd.auc_neg.cpu().numpy()
    assert abs(wd.auc() - R.compute_auc(pos, neg)) <= 1e-6 and abs(wd.auc() - auc2) <= 1e-6
    st = wd.evaluate_stream([dev_batch, host_batch])
    assert st["rows"] == 66 and st["bad_ids"] == 0 and abs(st["loss"] - m["mean"]) <= m["mean_bound"]
    assert abs(st["auc"] - wd.auc()) <= 1e-6
    assert np.array_equal(wd.auc_pos.cpu().numpy(), pos)                         # the stream has its own record
    empty = wd.evaluate_stream([])
    assert empty["rows"] == 0 and np.isnan(empty["loss"])
    assert wd.fused_eval_runs() == 8
    # the same build's general path (router, bag kernels, gemms, torch sigmoid, xent op, auc_hist)
    out = str(tmp_path / "general.npz")
    env = dict(os.environ, DTF_WD_EVAL_FUSED="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, REPO, out], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    gen = np.load(out)
    fused = float(wd.evaluate(dev_batch)[0])
    gbound = m["mean_bound"] + m["fp32_sum_extra"] + R.U * abs(m["mean"])        # its mean is an fp32 reduction
    fbound = m["mean_bound"] + R.U * abs(m["mean"])
    print(f"fused {fused:.9g} general {float(gen['loss']):.9g} model {m['mean']:.9g} bounds {fbound:.3g} {gbound:.3g}")
    assert abs(float(gen["loss"]) - m["mean"]) <= gbound and abs(float(gen["sloss"]) - m["mean"]) <= gbound
    assert abs(float(gen["loss"]) - fused) <= gbound + fbound                    # the two paths' summed bounds
    R.check_rows(m, p32=gen["p"])
    R.check_histograms(gen["pos"], gen["neg"], m)
    assert int(gen["srows"]) == 66 and int(gen["sbad"]) == 0
    for key, cls in (("pos", True), ("neg", False)):                             # fused vs general: the near rows
        a = np.cumsum({"pos": pos, "neg": neg}[key][::-1])[::-1][1:]
        b = np.cumsum(gen[key][::-1])[::-1][1:]
        assert (np.abs(a - b) <= (m["near"] & (m["positive"] == cls)[:, None]).sum(0)).all()


@pytest.mark.parametrize("D,hidden", [(16, (8,)), (6, (16,))])
def test_unsupported_shapes_take_the_general_path(native, D, hidden):
    fx = R.random_fixture(33, D, hidden, seed=3)
    m = R.model(*fx[:8], 200)
    wd = _wd(fx, D, hidden)
    assert not wd._eval_fused_ok()
    batch = tuple(torch.from_numpy(a).cuda() for a in fx[:4])
    loss, p = wd.evaluate(batch)
    assert abs(float(loss) - m["mean"]) <= m["mean_bound"] + m["fp32_sum_extra"] + R.U * abs(m["mean"])
    R.check_rows(m, p32=p.cpu().numpy())
    wd.auc_update(batch)
    R.check_histograms(wd.auc_pos.cpu().numpy(), wd.auc_neg.cpu().numpy(), m)
    st = wd.evaluate_stream([batch])
    assert st["rows"] == 33 and abs(st["loss"] - m["mean"]) <= m["mean_bound"]
    assert wd.fused_eval_runs() == 0


def _distinct_batch(seed, B=64, per=5):
    """A training batch in which no id repeats: every scatter update adds once
    per id, so a step is deterministic (no order of float atomics to differ in)."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(F)[:B * per].astype(np.int64)
    return tuple(torch.from_numpy(a).cuda() for a in (
        (rng.random((B, 1)) < 0.4).astype(np.float32), np.arange(0, B * per + 1, per, dtype=np.int64), ids,
        rng.random(B * per).astype(np.float32)))


def _state(wd, auc=True):
    """Tables and their sparse slots, the tower, Adam's slots and step, flat_grad (and the AUC histograms)."""
    st = list(wd.wide.state_tensors()) + list(wd.emb.state_tensors()) + [p.data for p in wd.dense_params]
    st += [wd.opt.step_t, wd.flat_grad] + ([wd.auc_pos, wd.auc_neg] if auc else [])
    return st + [t for t in list(wd.opt.m) + list(wd.opt.v) if t is not None]


@pytest.mark.parametrize("graphed", [False, True])
def test_training_state_is_untouched(native, graphed):
    fx = R.random_fixture(33, 16, (32, 16), seed=1)
    t1, t2 = _distinct_batch(11), _distinct_batch(12)
    ev = tuple(torch.from_numpy(a).cuda() for a in fx[:4])

    def mk():
        wd = _wd(fx, 16, (32, 16), dense_opt="adam", dense_lr=0.01, sparse_opt="sgd" if graphed else "adagrad",
                 ids_capacity=64 * 5 if graphed else None, rows=64)
        if graphed:
            wd.enable_graph()
        return wd
    a, b = mk(), mk()
    a.train_step(t1)
    b.train_step(t1)
    a.auc_update(ev)
    before = [t.clone() for t in _state(a)]
    step = a.global_step
    loss, p = a.evaluate(ev)
    st = a.evaluate_stream([ev, ev])
    torch.cuda.synchronize()
    for x, y in zip(before, _state(a)):
        assert torch.equal(x, y)                                                 # tables, slots, tower, Adam, flat_grad, AUC
    assert a.global_step == step == 1 and a.fused_eval_runs() == 4 and st["rows"] == 66
    # the evaluation saw the trained weights
    layers = [q.detach().cpu().numpy() for q in a.layers]
    m = R.model(*fx[:4], a.wide.local.cpu().numpy(), a.emb.local.cpu().numpy(), layers, float(a.bias.detach()), 200)
    assert not np.array_equal(layers[0], fx[6][0])
    R.check_rows(m, p32=p.cpu().numpy())
    assert abs(float(loss) - m["mean"]) <= m["mean_bound"] + R.U * abs(m["mean"])
    # train -> evaluate -> train equals train -> train, bit for bit
    la, lb = a.train_step(t2), b.train_step(t2)
    assert torch.equal(la, lb)
    for x, y in zip(_state(a, auc=False), _state(b, auc=False)):
        assert torch.equal(x, y)
    if graphed:
        assert a._graphed.replays == 2 and b._graphed.replays == 2
