"""The float64 model of the sparse-LR evaluation (tests/sparse_lr_eval_reference.py)
checked on the CPU: against torch's float64 loss and the package's own AUC
histograms, an fp32 emulation of the kernel's arithmetic inside the derived
bounds (and mutants of it outside them), the conditions the GPU fixtures must
meet, and the Session's evaluation lowering with the plan's run_eval stubbed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sparse_lr_eval_reference as R  # noqa: E402

EXACT_T = (200, 1000, 2)


@pytest.fixture(scope="module")
def exact():
    fx = R.exact_fixture(257, seed=0)
    return fx, {T: R.model(*fx[:6], T, exact_sum=True) for T in EXACT_T}


@pytest.fixture(scope="module")
def rand():
    fx = R.random_fixture()
    return fx, R.model(*fx[:6], 200)


def test_model_matches_torch_and_ops(rand):
    from distributed_tensorflow_example_amd import ops

    (lab, off, ids, vals, W, b, _), m = rand
    seg = torch.repeat_interleave(torch.arange(len(off) - 1), torch.diff(torch.from_numpy(off)))
    z = torch.zeros(len(off) - 1, dtype=torch.float64).index_add(
        0, seg, torch.from_numpy(W).double()[torch.from_numpy(ids)] * torch.from_numpy(vals).double()) + float(np.float32(b))
    y = torch.from_numpy(lab).double().reshape(-1)
    per = torch.nn.functional.binary_cross_entropy_with_logits(z, y, reduction="none").numpy()
    np.testing.assert_allclose(m["z"], z.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(m["loss"], per, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(m["mean"], per.mean(), rtol=1e-12)
    # the package's CPU histogram bins fp32 predictions at the same thresholds
    p32 = torch.from_numpy(m["p"].astype(np.float32))
    pos, neg = torch.zeros(201, dtype=torch.int64), torch.zeros(201, dtype=torch.int64)
    ops.auc_histogram_(p32, torch.from_numpy(lab).reshape(-1), pos, neg)
    k32 = R.bins_of(p32.numpy(), 200)
    assert np.array_equal(pos.numpy(), np.bincount(k32[m["positive"]], minlength=201))
    assert np.array_equal(neg.numpy(), np.bincount(k32[~m["positive"]], minlength=201))
    R.check_histograms(pos.numpy(), neg.numpy(), m)
    assert abs(ops.auc_from_histograms(pos, neg) - R.compute_auc(pos.numpy(), neg.numpy())) <= 1e-6
    assert 0.0 < m["auc"] < 1.0
    assert np.array_equal(R.thresholds(200).astype(np.float32), ops.auc_thresholds(200).numpy())


def test_emulation_inside_bounds(exact, rand):
    (fx, ms), (rfx, rm) = exact, rand
    z, loss, p, k, pos, neg = R.emulate(*rfx[:6], 200)
    kk = R.check_rows(rm, z, p, loss)
    assert np.array_equal(kk, k)
    R.check_histograms(pos, neg, rm)
    assert abs(float(loss.astype(np.float64).mean()) - rm["mean"]) <= rm["mean_bound"]
    for T in EXACT_T:
        z, loss, p, k, pos, neg = R.emulate(*fx[:6], T)
        assert np.array_equal(z.astype(np.float64), ms[T]["z"])          # exact, bit for bit
        assert np.array_equal(k, ms[T]["bins"]) and np.array_equal(pos, ms[T]["pos"]) and np.array_equal(neg, ms[T]["neg"])
        R.check_rows(ms[T], z, p, loss)


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_mutants_are_caught(exact):
    fx, ms = exact
    m = ms[200]
    caught = 0
    z, loss, p, k, pos, neg = R.emulate(*fx[:6], 200, mutant="no_bias")
    caught += _fails(lambda: R.check_rows(m, z, p, loss))
    z, loss, p, k, pos, neg = R.emulate(*fx[:6], 200, mutant="bool_label")
    caught += _fails(lambda: R.check_rows(m, z, p, loss))
    z, loss, p, k, pos, neg = R.emulate(*fx[:6], 200, mutant="bin_shift")
    caught += not np.array_equal(k, m["bins"]) and _fails(lambda: R.check_histograms(pos, neg, m))
    # p >= t instead of p > t shows where a p sits on a threshold: z = 0, T = 3
    lab, off, ids, vals = np.ones((1, 1), np.float32), np.array([0, 0]), np.zeros(0, np.int64), np.zeros(0, np.float32)
    W0 = np.zeros(8, np.float32)
    good = R.emulate(lab, off, ids, vals, W0, 0.0, 3)
    ge = R.emulate(lab, off, ids, vals, W0, 0.0, 3, mutant="ge")
    caught += int(good[3][0] == R.model(lab, off, ids, vals, W0, 0.0, 3)["bins"][0] and ge[3][0] != good[3][0])
    assert caught >= 3, caught
    assert caught == 4


def test_gpu_fixtures_meet_their_conditions(exact, rand):
    fx, ms = exact
    for T, want_margin, want_bins in ((200, 1.28e-4, 67), (1000, 1.4e-5, 93)):
        # the whole grid k / 8, |k| <= 64 (what any exact-fixture row can give), and +-40
        grid = np.arange(-64, 65) / 8.0
        p = 1.0 / (1.0 + np.exp(-grid))
        d = np.abs(p[:, None] - R.thresholds(T)[None, :]).min()
        assert d >= want_margin * 0.99, (T, d)
        assert len(np.unique(R.bins_of(p, T))) == want_bins
        m = ms[T]
        # the margin exceeds the derived bound on p: no row near a threshold (z = +-40 included)
        assert R.margin(m) >= d and R.margin(m) > 10 * m["pb"].max()
        assert not m["near"].any()
    assert (ms[2]["bins"] == 1).all()
    m = ms[200]
    assert np.all(np.abs(m["z"] * 8 - np.round(m["z"] * 8)) == 0)
    zs = set(m["z"].tolist())
    assert 40.0 in zs and -40.0 in zs and m["bad"] == 1
    assert fx[0][10, 0] == 0.5 and m["z"][10] != 0.0          # the label-0.5 row's loss depends on the float label
    assert np.abs(np.delete(m["z"], [8, 9])).max() <= 8.0
    lens = set(np.diff(fx[1]).tolist())
    assert {0, 1, 64, 65, 130} <= lens
    # random fixture: the near-threshold share is a condition of the fixture (<= 1 %)
    rfx, rm = rand
    assert R.near_share(rm, guard=1e-5) <= 0.01
    assert rm["near"].any(1).mean() <= 0.01
    assert rm["pb"].max() < 1e-5 and rm["zb"].max() < 1e-4


# ------------------------------------------------------------------ SparseLRTrainer on the CPU: the general path
def _trainer(fx, auc_bins=200):
    from distributed_tensorflow_example_amd.models.sparse_lr import SparseLRTrainer
    from distributed_tensorflow_example_amd.parallel.world import World

    tr = SparseLRTrainer(fx[4].size, 0.1, World(device="cpu"), seed=2, device="cpu", auc_bins=auc_bins)
    with torch.no_grad():
        tr.W.local.copy_(torch.from_numpy(fx[4]).reshape(-1, 1))
        tr.b.data.fill_(float(fx[5]))
    return tr


def _batch(fx):
    return tuple(None if a is None else torch.from_numpy(a) for a in fx[:4])


def test_trainer_cpu_auc_and_stream():
    fx, fx2 = R.random_fixture(B=257, seed=5), R.random_fixture(B=64, seed=5)      # (the same W and b)
    assert np.array_equal(fx[4], fx2[4]) and fx[5] == fx2[5]
    m, m2 = R.model(*fx[:6], 50), R.model(*fx2[:6], 50)
    tr = _trainer(fx, auc_bins=50)
    assert not tr._fused_ok() and tr.auc_pos.numel() == 51 and tr.auc_neg.numel() == 51
    tr.auc_update(_batch(fx))
    tr.auc_update(_batch(fx2))
    pos, neg = tr.auc_pos.numpy().copy(), tr.auc_neg.numpy().copy()
    R.check_histograms(pos, neg, [m, m2])
    assert abs(tr.auc() - R.compute_auc(pos, neg)) <= 1e-6
    st = tr.evaluate_stream([_batch(fx), _batch(fx2)])
    assert set(st) == {"loss", "auc", "rows"} and st["rows"] == 321
    want = (m["loss_sum"] + m2["loss_sum"]) / 321
    assert abs(st["loss"] - want) <= (257 * m["mean_bound"] + 64 * m2["mean_bound"]) / 321
    assert abs(st["auc"] - tr.auc()) <= 1e-6
    assert np.array_equal(tr.auc_pos.numpy(), pos) and np.array_equal(tr.auc_neg.numpy(), neg)   # its own record
    tr.reset_auc()
    assert int(tr.auc_pos.sum()) == 0 and int(tr.auc_neg.sum()) == 0
    tr.auc_update(_batch(fx))
    R.check_histograms(tr.auc_pos.numpy(), tr.auc_neg.numpy(), m)
    assert tr.fused_eval_runs() == 0


def test_trainer_cpu_empty_stream_and_no_values():
    fx = R.random_fixture(B=9, seed=1)
    tr = _trainer(fx)
    st = tr.evaluate_stream([])
    assert st["rows"] == 0 and np.isnan(st["loss"]) and set(st) == {"loss", "auc", "rows"}
    lab, off, ids, _ = _batch(fx)
    assert tr.evaluate_stream([(lab[:0], off[:1], ids[:0], None)])["rows"] == 0                  # no rows: skipped
    m = R.model(fx[0], fx[1], fx[2], None, fx[4], fx[5], 200)
    loss, p = tr.evaluate((lab, off, ids, None))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and p.shape == (9,)
    assert abs(float(loss) - m["mean"]) <= m["mean_bound"] + m["fp32_sum_extra"] + R.U * abs(m["mean"])
    R.check_rows(m, p32=p.numpy())
    assert tr.global_step == 0


# ------------------------------------------------------------------ Session wiring
def _lr2_graph(tf, F, scope):
    with tf.name_scope(scope):
        shp, ind, fid, fvl = (tf.placeholder(tf.int64), tf.placeholder(tf.int64), tf.placeholder(tf.int64),
                              tf.placeholder(tf.float32))
        y = tf.placeholder(tf.float32, [None, 1])
        W = tf.Variable(tf.random_normal([F, 1]))
        b = tf.Variable(tf.zeros([1]))
        logits = tf.add(tf.nn.embedding_lookup_sparse(W, tf.SparseTensor(shape=shp, indices=ind, values=fid),
                                                      tf.SparseTensor(shape=shp, indices=ind, values=fvl),
                                                      combiner="sum"), b)
        loss = tf.reduce_mean(tf.nn.sigmoid_cross_entropy_with_logits(logits, y))
        prob = tf.nn.sigmoid(logits)
    return dict(shp=shp, ind=ind, fid=fid, fvl=fvl, y=y, W=W, b=b, logits=logits, loss=loss, prob=prob)


def test_try_lower_eval_accepts_global_step_and_refuses_mixed_plans(monkeypatch):
    monkeypatch.setenv("DTF_SHARD_MIN_ROWS", "1000")
    import distributed_tensorflow_example_amd.compat as tf
    from distributed_tensorflow_example_amd.compat import lowering

    F, B = 5000, 8
    tf.reset_default_graph()
    with tf.device(tf.train.replica_device_setter(ps_tasks=1)):
        gs = tf.get_variable("global_step", [], initializer=tf.constant_initializer(0), trainable=False)
        g1, g2 = _lr2_graph(tf, F, "a"), _lr2_graph(tf, F, "b")
        t1 = tf.train.GradientDescentOptimizer(0.5).minimize(g1["loss"], global_step=gs, var_list=[g1["W"], g1["b"]])
        t2 = tf.train.GradientDescentOptimizer(0.5).minimize(g2["loss"], var_list=[g2["W"], g2["b"]])
        auc = tf.contrib.metrics.streaming_auc(g1["prob"], g1["y"])
    rng = np.random.default_rng(0)
    rows = np.repeat(np.arange(B), 3)
    ids = rng.integers(0, F, rows.size).astype(np.int64)

    def feed(g):
        return {g["y"]: np.zeros((B, 1), np.float32), g["shp"]: [F, B], g["ind"]: np.stack([rows, ids], 1),
                g["fid"]: ids, g["fvl"]: np.ones(ids.size, np.float32)}
    both = dict(feed(g1))
    both.update(feed(g2))
    sess = tf.Session()
    sess.run([tf.global_variables_initializer(), tf.local_variables_initializer()])
    # an evaluation before any train run finds the graph's plans
    eager = float(sess.run([gs, g1["loss"]], feed_dict=both)[1])           # CPU tables: run_eval declines
    p1, p2 = lowering.plan_for(t1), lowering.plan_for(t2)
    assert p1 is not None and p2 is not None and p1.eval_runs == 0
    calls = []

    def stub(plan):
        def run_eval(ctx, needs):
            calls.append((plan, sorted(t.name for t in needs.values())))
            for k, t in needs.items():
                if t is plan.pat.loss:
                    ctx.memo[k] = torch.tensor(0.25)
                else:
                    ctx.memo[k] = torch.full((B, 1), 0.75)
            plan.eval_runs += 1
            return True
        monkeypatch.setattr(plan, "run_eval", run_eval)
    stub(p1)
    stub(p2)
    out = sess.run([gs, g1["loss"]], feed_dict=both)                       # lr2.py's own fetch list
    assert float(out[1]) == 0.25 and float(out[0]) == 0.0 and len(calls) == 1 and calls[0][0] is p1
    assert calls[0][1] == [g1["loss"].name]
    assert float(sess.run(g1["loss"], feed_dict=both)) == 0.25 and len(calls) == 2
    sess.run(auc, feed_dict=both)                                          # through streaming_auc's update op
    assert len(calls) == 3 and calls[2][1] == [g1["prob"].name]
    sess.run([g1["logits"], g1["prob"], g1["loss"]], feed_dict=both)
    assert len(calls) == 4 and len(calls[3][1]) == 3
    # two plans in one run, a matched variable, an interior node: op by op
    n = len(calls)
    mixed = sess.run([g1["loss"], g2["loss"]], feed_dict=both)
    sess.run([g1["loss"], g1["b"]], feed_dict=both)
    sess.run([g1["loss"], g1["W"]], feed_dict=both)
    assert len(calls) == n and abs(float(mixed[0]) - eager) < 1e-6
    assert p1.eval_runs == 4 and p2.eval_runs == 0 and p1.steps == 0
    sess.close()
    tf.reset_default_graph()
