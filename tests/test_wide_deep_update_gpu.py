"""The one-writer table update of the fused Wide&Deep step (csrc/kernels/wide_deep_update.hip, WideDeepTrainPlan.update,
WideDeep(fused_step="combined")) against float64 models: bit-exact on integer data at the chunk edges, ROW_TOL for the rules."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_deep_eval_reference as R  # noqa: E402
import wide_deep_train_reference as T  # noqa: E402
from distributed_tensorflow_example_amd.optim.rules import RULES  # noqa: E402
from test_wide_deep_eval_gpu import _cuda, _wd  # noqa: E402

pytestmark = pytest.mark.gpu
ROW_TOL = dict(rtol=1e-4, atol=1e-5)        # test_optim_rules_gpu.py
V = 50
HP = {"sgd": {}, "momentum": {"momentum": 0.9, "use_nesterov": True}, "adagrad": {}, "rmsprop": {"momentum": 0.5, "epsilon": 1e-6},
      "ftrl": {"l1_regularization_strength": 0.001, "l2_regularization_strength": 0.1}}
# sorted-order layouts as (id, count) runs; a chunk is 64 sorted positions
LAYOUTS = {
    "n63": [(1, 3), (2, 60)], "n64": [(3, 30), (4, 34)], "n65": [(3, 30), (4, 35)], "n257": [(0, 100), (5, 1), (6, 156)],
    "fills_chunk": [(0, 64), (1, 64), (2, 10)], "ends_at_chunk_end": [(1, 20), (2, 108), (3, 5)],
    "starts_at_63": [(1, 63), (2, 10)], "four_chunks": [(1, 40), (2, 182), (3, 98)],
    "outside": [(-3, 5), (0, 2), (7, 70), (V + 2, 4)], "single_run": [(9, 200)]}


def _gsum(off, ids, vals, dz, demb, combiner):
    """float64 duplicate-summed gradients of the wide [V] and embedding [V, D] tables, and the touched rows."""
    bag = np.repeat(np.arange(off.size - 1), np.diff(off))
    v = np.ones(ids.size) if vals is None else vals.astype(np.float64)
    ws = np.bincount(bag, v * v if combiner == "sqrtn" else v, off.size - 1)
    sc = {"sum": np.ones_like(ws), "mean": 1 / np.maximum(ws, 1e-30), "sqrtn": 1 / np.sqrt(np.maximum(ws, 1e-30))}[combiner]
    ok = (ids >= 0) & (ids < V)
    w, gw, ge = (v * sc[bag])[ok], np.zeros(V), np.zeros((V, demb.shape[1]))
    np.add.at(gw, ids[ok], w * dz[bag[ok]])
    np.add.at(ge, ids[ok], w[:, None] * demb[bag[ok]])
    return gw, ge, np.unique(ids[ok])


def _plan(native, D, combiner, wide, emb):
    dev = dict(device="cuda")
    return native.WideDeepTrainPlan(wide, emb, [torch.zeros(D, 16, **dev), torch.zeros(16, **dev), torch.zeros(16, 1, **dev),
                                                torch.zeros(1, **dev)], torch.zeros(1, **dev), combiner)


def _load(plan, off, ids, vals, dz, demb):
    """rows() on the batch (sizes the scratch), then the given bag gradients in its place."""
    dev = (_cuda(off), _cuda(ids), None if vals is None else _cuda(vals))
    plan.rows(torch.zeros(off.size - 1, device="cuda"), *dev, 1.0)
    plan.dz().copy_(_cuda(dz.astype(np.float32)).reshape(-1, 1))
    plan.demb().copy_(_cuda(demb.astype(np.float32)))
    return dev


@pytest.mark.parametrize("D", [4, 12, 16, 64, 96, 128])          # 12, 96: D / 4 lanes per row do not divide the wave
@pytest.mark.parametrize("name,novals,combiner", [(n, False, "sum") for n in LAYOUTS] + [("four_chunks", True, "sum"),
                                                                                        ("outside", True, "mean")])
def test_run_boundaries_exact(native, name, novals, combiner, D):
    rng = np.random.default_rng(len(name) + D)
    ids = rng.permutation(np.concatenate([np.full(c, i, np.int64) for i, c in LAYOUTS[name]]))
    if combiner == "mean":                          # bags of 2^k ids, no values: every scale is exact
        off = np.concatenate([[0], np.cumsum([1, 2, 4, 8, 16, 32, 16, 2])]).astype(np.int64)      # 81 ids
    else:
        off = np.sort(np.concatenate([[0, ids.size], rng.integers(0, ids.size + 1, 6)])).astype(np.int64)
    nb = off.size - 1
    vals = None if novals else rng.integers(0, 4, ids.size).astype(np.float32)
    dz, demb = rng.integers(-3, 4, nb).astype(np.float64), rng.integers(-3, 4, (nb, D)).astype(np.float64)
    w0, e0 = rng.integers(-8, 9, (V, 1)).astype(np.float32), rng.integers(-8, 9, (V, D)).astype(np.float32)
    gw, ge, touched = _gsum(off, ids, vals, dz, demb, combiner)
    results = []
    for _ in range(2):                              # the same start state twice: the same bits
        wide, emb = _cuda(w0), _cuda(e0)
        plan = _plan(native, D, combiner, wide, emb)
        dev = _load(plan, off, ids, vals, dz, demb)
        plan.update(*dev, RULES["sgd"].kind, 0.5, [], [])
        results.append((wide.cpu().numpy(), emb.cpu().numpy()))
    assert np.array_equal(results[0][0].astype(np.float64), w0 - 0.5 * gw[:, None])
    assert np.array_equal(results[0][1].astype(np.float64), e0 - 0.5 * ge)
    rest = np.setdiff1d(np.arange(V), touched)
    assert np.array_equal(results[0][1][rest].view(np.int32), e0[rest].view(np.int32))
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(*results))


def _batch(rng, B, n, lo, hi):
    """(labels, offsets, ids, vals): ids repeat within and across bags, id 7 about every second time (a run over chunks)."""
    ids = np.where(rng.random(n) < 0.5, 7, rng.integers(lo, hi, n)).astype(np.int64)
    off = np.sort(np.concatenate([[0, n], rng.integers(0, n + 1, B - 1)])).astype(np.int64)
    return (rng.random((B, 1)) < 0.4).astype(np.float32), off, ids, rng.uniform(0.5, 1.5, n).astype(np.float32)


def _rule64(kind, state, g, touched, lr, round_g=False):
    """RULES[kind].update_ in float64 on the touched rows of (var, slot a, slot b); returns the new state."""
    new = [None if s is None else s.clone() for s in state]
    g = torch.from_numpy(g.astype(np.float32).astype(np.float64) if round_g else g)[touched]
    rows = [None if s is None else s[touched] for s in new]
    RULES[kind].update_(*rows, g, lr, HP[kind], False)
    for s, r in zip(new, rows):
        if s is not None:
            s[touched] = r
    return new


@pytest.mark.parametrize("D,combiner", [(4, "sum"), (64, "sqrtn")])
@pytest.mark.parametrize("kind", list(HP))
def test_rules(native, kind, D, combiner):
    rule, lr = RULES[kind], 0.1
    rng = np.random.default_rng(100 + D)
    tabs = [[_cuda((rng.standard_normal((V, d)) * 0.3).astype(np.float32))] +
            [torch.full((V, d), v0, device="cuda") for v0 in rule.slot_init(HP[kind])] for d in (1, D)]
    plan = _plan(native, D, combiner, tabs[0][0], tabs[1][0])
    ref = [[t.double().cpu() for t in tab] + [None] * (3 - len(tab)) for tab in tabs]
    tol = lambda x: ROW_TOL["atol"] + ROW_TOL["rtol"] * x.abs()    # noqa: E731
    for step in range(2):
        _, off, ids, vals = _batch(rng, 9, 330, -1, V + 1)           # both sorted ends out of range
        dz, demb = (rng.uniform(-1, 1, sh).astype(np.float32).astype(np.float64) for sh in (9, (9, D)))
        gw, ge, touched = _gsum(off, ids, vals, dz, demb, combiner)
        before = [[t.clone() for t in tab] for tab in tabs]
        dev = _load(plan, off, ids, vals, dz, demb)
        args = (*dev, rule.kind, lr, tabs[0][1:], tabs[1][1:])
        plan.update(*args, torch.ones(1, dtype=torch.int32, device="cuda"), **rule.native_kwargs(HP[kind]))
        assert all(torch.equal(x, y) for a, b in zip(tabs, before) for x, y in zip(a, b)), "skip = 1 changed something"
        plan.update(*args, None, **rule.native_kwargs(HP[kind]))
        rest = torch.from_numpy(np.setdiff1d(np.arange(V), touched)).cuda()
        for tab, bef, g, r in zip(tabs, before, (gw[:, None], ge), ref):
            new, r32 = _rule64(kind, r, g, touched, lr), _rule64(kind, r, g, touched, lr, round_g=True)
            for name, got, b0, want, w32 in zip(("var", "slot a", "slot b"), tab, bef, new, r32):
                assert bool(((w32 - want).abs() < 0.25 * tol(want)).all()), "precondition: fp32 gsum moves the reference"
                err = (got.double().cpu() - want).abs()
                assert bool((err <= tol(want)).all()), f"{name} step {step}"
                assert torch.equal(got[rest], b0[rest]), f"{name}: an untouched row changed"
            r[:] = new
    # the refusals: Adam, a missing slot, an FTRL hyper-parameter out of range; nothing is launched
    n, state = plan.updates(), [t.clone() for tab in tabs for t in tab]
    slots = [torch.zeros(V, 1, device="cuda")] * 2, [torch.zeros(V, D, device="cuda")] * 2
    for k, ws, es, kw in [(RULES["adam"].kind, *slots, {}), (RULES["adagrad"].kind, [], [], {}),
                          (RULES["rmsprop"].kind, slots[0][:1], slots[1][:1], {}), (RULES["ftrl"].kind, *slots, {"l1": -1.0})]:
        with pytest.raises(RuntimeError):
            plan.update(*dev, k, lr, ws, es, None, **kw)
    assert plan.updates() == n and all(torch.equal(x, y) for x, y in zip(state, (t for tab in tabs for t in tab)))


@pytest.mark.parametrize("kind", list(HP))
def test_model_combined_matches_general_path(native, kind):
    """Tables and slots of both paths within ROW_TOL after each of two steps; at each step the loss and tower of each
    path inside test_widedeep_fused_step's bounds around the float64 step from that path's own state before it."""
    D, hidden, kw = 16, (32, 16), dict(sparse_opt=kind, sparse_hp=HP[kind])
    fx = R.random_fixture(33, D, hidden, seed=1)
    a, b = _wd(fx, D, hidden, fused_step="combined", **kw), _wd(fx, D, hidden, **kw)
    g = _wd(fx, D, hidden, fused_step="combined", ids_capacity=64 * 5, rows=64, **kw)
    g.enable_graph()
    assert a._train_fused_ok() and g._train_fused_ok() and not b._train_fused_ok()
    assert not _wd(fx, D, hidden, fused_step="combined", sparse_opt="adam")._train_fused_ok()
    _tables = lambda wd: wd.wide.state_tensors() + wd.emb.state_tensors()    # noqa: E731
    batches = [_batch(np.random.default_rng(seed), 64, 320, 0, 40) for seed in (21, 22)]
    lr32 = float(np.float32(0.1))
    for nb in batches:
        bt = tuple(_cuda(x) for x in nb)
        olds = [[p.data.cpu().numpy() for p in m.dense_params] for m in (a, b)]
        refs = [T.backward(*nb, m.wide.local.cpu().numpy().reshape(-1), m.emb.local.cpu().numpy(), old[:-1], float(old[-1][0]))
                for m, old in zip((a, b), olds)]
        la, lb, lg = a.train_step(bt), b.train_step(bt), g.train_step(bt)
        assert torch.equal(la, lg) and all(torch.equal(x, y) for x, y in zip(_tables(a) + a.dense_params, _tables(g) + g.dense_params))
        for x, y in zip(_tables(a), _tables(b)):
            np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), **ROW_TOL)
        for m, l, r, old in zip((a, b), (la, lb), refs, olds):
            assert abs(float(l) - r["m"]["mean"]) <= r["m"]["mean_bound"]
            for p, th, gi, gb in zip(m.dense_params, old, r["grads"], r["gradb"]):
                new = th.astype(np.float64) - lr32 * gi.reshape(th.shape)
                assert (np.abs(p.data.double().cpu().numpy() - new) <= T.step_bound(new, gi.reshape(th.shape), gb.reshape(th.shape), lr32)).all()
    assert g._graphed.captures == 1 and g._graphed.replays == 2 and a._native_train_plan().updates() == 2
    state = [t.clone() for t in _tables(g)]
    g.train_step((torch.zeros(64, 1), torch.zeros(65, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0)))
    assert all(torch.equal(x, y) for x, y in zip(state, _tables(g)))
