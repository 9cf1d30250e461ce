"""The one-GPU factorization machine (csrc/kernels/fm.hip, FMPlan, models/fm.py FMTrainer) against the float64
reference of tests/fm_reference.py.

Bounds (R.bounds; U = 2^-24): |z err| <= zb = 8 (n_r + K) U M_r and |loss err| <= lb.  sigmoid' <= 1/4 and the
kernel's exp / divide add a few roundings of a value <= 1, so |p err| <= pb = zb / 4 + 8 U and |dz err| <= pb / B.
demb = dz S: |err| <= |dz| 8 (n_r + K) U A_r[f] + (pb / B) |S_r[f]| + 4 U |demb|, A_r[f] = sum |x v|."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fm_reference as R  # noqa: E402
import sparse_lr_eval_reference as E  # noqa: E402
from distributed_tensorflow_example_amd.models import FMTrainer  # noqa: E402
from distributed_tensorflow_example_amd.optim.rules import RULES  # noqa: E402
from test_fm_cpu import HP, check_steps, train_batch  # noqa: E402
from test_wide_deep_update_gpu import LAYOUTS  # noqa: E402

pytestmark = pytest.mark.gpu
U, F = R.U, 50


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows_batch():
    """37 rows: empty, 1, 64, 65 and 130 entries (chunk edges), one id three times, then short rows; values in
    +-[0.5, 1.5] and one exact 0; ids -1 and F once each."""
    rng = np.random.default_rng(5)
    lens = np.array([0, 1, 64, 65, 130, 3] + list(rng.integers(1, 9, 31)))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = rng.integers(0, F, off[-1]).astype(np.int64)
    vals = (rng.uniform(0.5, 1.5, ids.size) * rng.choice([-1.0, 1.0], ids.size)).astype(np.float32)
    ids[off[5]:off[6]] = 9
    ids[off[3] + 2], ids[off[4] + 70], vals[off[4] + 3] = -1, F, 0.0
    return (rng.random(37) < 0.5).astype(np.float32), off, ids, vals


def _row_bounds(f, B):
    zb, lb = R.bounds(f)
    pb = zb / 4 + 8 * U
    scale = 8 * (f["n"] + f["S"].shape[1]) * U
    db = np.abs(f["dz"])[:, None] * scale[:, None] * f["A"] + (pb / B)[:, None] * np.abs(f["S"]) + 4 * U * np.abs(f["demb"])
    return dict(z=zb, loss=lb, p=pb, dz=pb / B, demb=db)


@pytest.mark.parametrize("rpw", [0, 3])
@pytest.mark.parametrize("K", [4, 20, 64, 128])
def test_rows_against_float64(native, K, rpw):
    rng = np.random.default_rng(K)
    batch = _rows_batch()
    w, V, b = (rng.standard_normal(F) * 0.3).astype(np.float32), (rng.standard_normal((F, K)) * 0.05).astype(np.float32), 0.25
    f, f32 = R.forward(*batch, w, V, b), R.forward(*batch, w, V, b, np.float32)
    bd = _row_bounds(f, 37)
    for k in ("z", "loss", "dz", "demb"):
        assert (np.abs(f32[k] - f[k]) <= 0.25 * bd[k]).all(), f"precondition: fp32 NumPy {k} outside a quarter of the bound"
    plan = native.FMPlan(_cuda(w), _cuda(V), torch.tensor([b], device="cuda"))
    plan.set_rpw(rpw)
    plan.rows(*(_cuda(x) for x in batch), 1.0 / 37)
    got = dict(z=plan.z(), loss=plan.lrow(), dz=plan.dz(), demb=plan.demb())
    for k, t in got.items():
        err = np.abs(t.double().cpu().numpy() - f[k])
        print(f"K={K} rpw={rpw} {k}: max err / bound = {(err / np.maximum(bd[k], 1e-300)).max():.3g}")
        assert (err <= bd[k]).all(), k
    assert np.array_equal(plan.brow().cpu().numpy(), f["brow"]) and f["brow"].sum() == 2


@pytest.mark.parametrize("kind", [n for n, r in RULES.items() if r.row_local])
def test_train_steps_against_float64(kind):
    runs = []
    for _ in range(2):                                  # the same start twice: the same bits (one writer per element)
        tr = FMTrainer(300, factors=20, lr=0.1, device="cuda", optimizer=kind, optimizer_hp=HP[kind])
        check_steps(tr, kind, seed=4)
        assert tr._native_plan().updates() == 3
        runs.append([t.clone() for t in tr._state_tensors()])
    assert all(torch.equal(x, y) for x, y in zip(*runs))


@pytest.mark.parametrize("K", [4, 12, 64, 128])                  # 12: K / 4 lanes per row do not divide the wave
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_run_boundaries_exact(native, name, K):
    """The FM form of the one-writer update (a run also carries q = sum x^2 dz, the writer subtracts V_old q) at the
    chunk edges of test_wide_deep_update_gpu.py's layouts, bit for bit on integer data: with <= 200 occurrences per
    id every intermediate is an integer or a half-integer below 2^23 (asserted), so fp32 is exact in any order."""
    rng = np.random.default_rng(len(name) + K)
    ids = rng.permutation(np.concatenate([np.full(c, i, np.int64) for i, c in LAYOUTS[name]]))
    off = np.sort(np.concatenate([[0, ids.size], rng.integers(0, ids.size + 1, 6)])).astype(np.int64)
    nb = off.size - 1
    vals = rng.integers(0, 4, ids.size).astype(np.float32)
    dz, demb = rng.integers(-3, 4, nb).astype(np.float64), rng.integers(-3, 4, (nb, K)).astype(np.float64)
    w0, V0 = rng.integers(-8, 9, F).astype(np.float32), rng.integers(-8, 9, (F, K)).astype(np.float32)
    bag, ok, x = np.repeat(np.arange(nb), np.diff(off)), (ids >= 0) & (ids < F), vals.astype(np.float64)
    gw, q, ge = np.zeros(F), np.zeros(F), np.zeros((F, K))
    np.add.at(gw, ids[ok], (x * dz[bag])[ok])
    np.add.at(q, ids[ok], (x * x * dz[bag])[ok])
    np.add.at(ge, ids[ok], (x[:, None] * demb[bag])[ok])
    gV = ge - V0 * q[:, None]
    want_w, want_V = w0 - 0.5 * gw, V0 - 0.5 * gV
    # the same sums over absolute values bound every partial sum of any order
    aw, aq, ae = np.zeros(F), np.zeros(F), np.zeros((F, K))
    np.add.at(aw, ids[ok], np.abs(x * dz[bag])[ok])
    np.add.at(aq, ids[ok], np.abs(x * x * dz[bag])[ok])
    np.add.at(ae, ids[ok], np.abs(x[:, None] * demb[bag])[ok])
    top = max(aw.max(), aq.max(), ae.max(), (ae + np.abs(V0) * aq[:, None]).max(), np.abs(want_w).max(), np.abs(want_V).max())
    assert top < 2.0 ** 23 and np.bincount(ids[ok]).max() <= 200, "precondition: fp32 is exact on this data"
    results = []
    for _ in range(2):                                  # the same start state twice: the same bits
        w, V = _cuda(w0), _cuda(V0)
        plan = native.FMPlan(w, V, torch.zeros(1, device="cuda"))
        dev = (_cuda(off), _cuda(ids), _cuda(vals))
        plan.rows(torch.zeros(nb, device="cuda"), *dev, 1.0)        # sizes the scratch; the given gradients in its place
        plan.dz().copy_(_cuda(dz.astype(np.float32)))
        plan.demb().copy_(_cuda(demb.astype(np.float32)))
        plan.update(*dev, RULES["sgd"].kind, 0.5, [], [])
        results.append((w.cpu().numpy(), V.cpu().numpy()))
    assert np.array_equal(results[0][0].astype(np.float64), want_w)
    assert np.array_equal(results[0][1].astype(np.float64), want_V)
    rest = np.setdiff1d(np.arange(F), np.unique(ids[ok]))
    assert np.array_equal(results[0][0][rest].view(np.int32), w0[rest].view(np.int32))
    assert np.array_equal(results[0][1][rest].view(np.int32), V0[rest].view(np.int32))
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(*results))


def _copy_tables(dst, src):
    for d, s in zip(dst._state_tensors(), src._state_tensors()):
        d.copy_(s)


def test_evaluation(monkeypatch):
    rng = np.random.default_rng(8)
    tr = FMTrainer(300, factors=20, lr=0.1, device="cuda", init_std=0.1, auc_bins=50)
    tr.w.copy_(_cuda((rng.standard_normal(300) * 0.5).astype(np.float32)))
    assert tr._fused_ok()                               # (decided once, at the first question)
    monkeypatch.setenv("DTF_FM_FUSED", "0")
    gen = FMTrainer(300, factors=20, lr=0.1, device="cuda", auc_bins=50)
    _copy_tables(gen, tr)
    assert not gen._fused_ok()
    batches = [train_batch(rng, B, n) for B, n in ((5, 30), (48, 200), (17, 90))]
    fs = [R.forward(*bt, tr.w.cpu().numpy(), tr.V.cpu().numpy(), 0.0) for bt in batches]
    pos, neg = np.zeros(51, np.int64), np.zeros(51, np.int64)
    for bt, f in zip(batches, fs):
        bd = _row_bounds(f, bt[0].size)
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
    want = sum(f["loss"].sum() for f in fs)
    assert out["rows"] == 70 and out["bad_ids"] == 6 and abs(out["auc"] - E.compute_auc(pos, neg)) <= 1e-6
    assert abs(out["loss"] * 70 - want) <= sum(R.bounds(f)[1].sum() for f in fs)
    assert tr.fused_eval_runs() == 3 * 4 and gen.fused_eval_runs() == 0


def test_refusals_and_graph(native):
    assert not any(native.FMPlan.supported(K) for K in (6, 132, 0)) and native.FMPlan.supported(20)
    with pytest.raises(ValueError):
        FMTrainer(300, factors=20, device="cuda", optimizer="adam")
    with pytest.raises(ValueError):
        FMTrainer(300, factors=6, device="cuda")._fused_ok()
    eager, graphed = (FMTrainer(300, factors=20, lr=0.1, device="cuda", init_std=0.3, optimizer="ftrl",
                                optimizer_hp=HP["ftrl"]) for _ in range(2))
    graphed.enable_graph()
    rng = np.random.default_rng(2)
    for _ in range(3):                                  # three replays of one capture against three eager steps
        bt = tuple(torch.from_numpy(x) for x in train_batch(rng, n=400))
        le, lg = eager.train_step(bt), graphed.train_step(bt)
        assert torch.equal(le, lg) and all(torch.equal(x, y) for x, y in zip(eager._state_tensors(), graphed._state_tensors()))
    assert graphed._graphed.captures == 1 and graphed._graphed.replays == 3
