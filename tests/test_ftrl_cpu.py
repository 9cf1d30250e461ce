"""FTRL-Proximal (tf.train.FtrlOptimizer) on the CPU: the float64 model's own
sanity, the row-sparse rule of a sharded table, the dense fused optimizer, the
compat front end with its TF-named checkpoint slots, and 2 gloo ranks == 1 for
the sparse-LR trainer.  The GPU twin is tests/test_ftrl_gpu.py."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from ftrl_reference import SLOT_TOL, VAR_TOL, LRModel, ftrl_dense, ftrl_rows, hp_of, sigma
from test_sparse_optim_cpu import make_steps

from distributed_tensorflow_example_amd.parallel.sharded_embedding import ShardedEmbedding
from distributed_tensorflow_example_amd.parallel.world import World

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LR = 0.05          # the learning rate of tests/test_sparse_optim_*.py
HP = {"ftrl": hp_of(-0.5, 0.05, 0.01, 0.02)}
POWERS = [-0.5, -0.3, 0.0]
REGS = [(0.0, 0.0, 0.0), (0.05, 0.01, 0.0), (0.05, 0.01, 0.02)]     # (l1, l2, l2_shrinkage)


def run_ftrl_table(rows, D, steps, lr, hp, device="cpu", void_step=None):
    """make_steps' updates through ShardedEmbedding._apply_local (run_table of
    tests/test_sparse_optim_cpu.py with the FTRL hyper-parameters)."""
    t = ShardedEmbedding(rows, D, World(device=device), init_std=0.5, seed=3, device=device)
    t0 = t.local.detach().cpu().numpy().copy()
    t.set_optimizer("ftrl", **hp)
    for k, (idx, g) in enumerate(steps):
        void = None
        if void_step is not None:
            void = torch.tensor([1 if k == void_step else 0], dtype=torch.int32, device=device)
        t._apply_local(torch.as_tensor(idx, device=device), torch.as_tensor(g, device=device), lr, 1.0, void)
        assert float(t._gacc.abs().max()) == 0.0        # the step accumulator is clean between steps
    return t, t0


def check_table(t, model, lin_atol=None):
    var, acc, lin = model
    np.testing.assert_allclose(t.local.cpu().numpy(), var, **VAR_TOL)
    np.testing.assert_allclose(t.slots["Ftrl"].cpu().numpy(), acc, **SLOT_TOL)
    lin_tol = SLOT_TOL if lin_atol is None else dict(SLOT_TOL, atol=lin_atol)
    np.testing.assert_allclose(t.slots["Ftrl_1"].cpu().numpy(), lin, **lin_tol)


def within(a, b, tol):
    return bool(np.all(np.abs(a - b) <= tol["atol"] + tol["rtol"] * np.abs(b)))


# ---------------------------------------------------------------- the model itself
def test_model_is_adagrad_from_zero():
    """l1 = l2 = 0, learning_rate_power = -0.5, var = 0: one step is Adagrad's
    step from the same accumulator."""
    rng = np.random.default_rng(0)
    g, acc = rng.standard_normal(100), rng.random(100) + 0.1
    var, acc_new, lin = ftrl_dense(np.zeros(100), acc, np.zeros(100), g, 0.3)
    np.testing.assert_allclose(acc_new, acc + g * g, rtol=1e-15)
    np.testing.assert_allclose(var, -0.3 * g / np.sqrt(acc + g * g), rtol=1e-12)
    np.testing.assert_allclose(lin, g, rtol=1e-15)


def test_model_power_zero_has_no_sigma():
    rng = np.random.default_rng(1)
    acc = rng.random(50) + 0.1
    assert np.all(sigma(acc, acc + rng.random(50), 0.1, 0.0) == 0.0)
    var = rng.standard_normal(50)
    _, _, lin = ftrl_dense(var, acc, np.zeros(50), np.ones(50), 0.1, lr_power=0.0)
    assert np.array_equal(lin, np.ones(50))             # linear += g, nothing of var


@pytest.mark.parametrize("mutant", ["l2", "shrunk_acc", "ge"])
def test_model_mutants_fall_outside_the_tolerance(mutant):
    """Each wrong reading of the rule is told apart by the row test's inputs at
    the tolerance used throughout.  `ge`: |linear| == l1 gives 0 either way
    unless the division is 0 / 0 (acc == 0, g == 0, l2 == 0), so that row is
    planted -- the case where the threshold must be a select."""
    rows, D = 300, 4
    steps = make_steps(rows, D, 128, 4, seed=D)
    rng = np.random.default_rng(3)
    table = 0.5 * rng.standard_normal((rows, D))
    hp, acc, lin = HP["ftrl"], None, None
    if mutant == "ge":
        hp = hp_of(-0.5, 0.05, 0.0, 0.0)
        acc, lin = np.full((rows, D), 0.1), np.zeros((rows, D))
        r = int(steps[0][0][steps[0][0] >= 0][0])
        steps = [(np.array([r], np.int64), np.zeros((1, D), np.float32))]
        acc[r], lin[r] = 0.0, hp["l1_regularization_strength"]
    good = ftrl_rows(table, steps, LR, hp, acc, lin)
    bad = ftrl_rows(table, steps, LR, hp, acc, lin, mutant=mutant)
    assert np.isfinite(good[0]).all()
    assert not (within(bad[0], good[0], VAR_TOL) and within(bad[1], good[1], SLOT_TOL)
                and within(bad[2], good[2], SLOT_TOL))


# ---------------------------------------------------------------- row-sparse rule
@pytest.mark.parametrize("reg", REGS)
@pytest.mark.parametrize("lr_power", POWERS)
@pytest.mark.parametrize("D", [1, 4, 6])
def test_row_rule_matches_model(D, lr_power, reg):
    rows = 300
    hp = hp_of(lr_power, *reg)
    steps = make_steps(rows, D, 128, 4, seed=D)
    t, t0 = run_ftrl_table(rows, D, steps, LR, hp)
    check_table(t, ftrl_rows(t0, steps, LR, hp))


def test_voided_step_changes_nothing():
    rows, D = 200, 4
    steps = make_steps(rows, D, 64, 3, seed=11)
    t, t0 = run_ftrl_table(rows, D, steps, LR, HP["ftrl"], void_step=1)
    check_table(t, ftrl_rows(t0, [steps[0], steps[2]], LR, HP["ftrl"]))


def test_untouched_rows_keep_value_and_slots():
    t = ShardedEmbedding(50, 2, World(device="cpu"), seed=1)
    before = t.local.clone()
    t.set_optimizer("ftrl", **HP["ftrl"])
    t._apply_local(torch.tensor([3, 3, -1, 7]), torch.tensor([[1.0, 1.0], [-1.0, -1.0], [5.0, 5.0], [1.0, 2.0]]),
                   0.1, 1.0, None)
    changed = (t.local != before).any(1).nonzero().reshape(-1).tolist()
    assert changed == [3, 7]                 # row 3: summed gradient exactly 0, still recomputed from linear
    acc, lin = t.slots["Ftrl"], t.slots["Ftrl_1"]
    keep = torch.ones(50, dtype=torch.bool)
    keep[[3, 7]] = False
    assert torch.equal(acc[keep], torch.full((48, 2), 0.1)) and torch.equal(lin[keep], torch.zeros(48, 2))
    assert torch.equal(acc[3], torch.full((2,), 0.1))           # g == 0: accum unchanged
    model = ftrl_rows(before.numpy(), [(np.array([3, 3, -1, 7]), np.array([[1, 1], [-1, -1], [5, 5], [1, 2.0]]))],
                      0.1, HP["ftrl"])
    check_table(t, model)


def test_zero_branch_is_a_select():
    """acc == 0, g == 0, l2 == 0: the untaken division is 0 / 0; var must be 0.0."""
    t = ShardedEmbedding(10, 1, World(device="cpu"), seed=1)
    t.set_optimizer("ftrl", **hp_of(-0.5, 0.0, 0.0, 0.0, acc0=0.0))
    t._apply_local(torch.tensor([2, 5]), torch.zeros(2, 1), 0.1, 1.0, None)
    assert t.local[2, 0] == 0.0 and t.local[5, 0] == 0.0 and torch.isfinite(t.local).all()


def exact_zero_case(seed, rows=300, D=4, n=128):
    """Inputs, hyper-parameters and the model's result of the exact-zero test,
    with the mask of elements far enough from the threshold to compare:
    | |linear| - l1 | > 1e-4 max(1, |linear|)."""
    hp = hp_of(-0.5, 1.0, 0.01, 0.0)          # l1 = 1: about half of the touched weights end at 0
    steps = make_steps(rows, D, n, 4, seed=seed)
    return hp, steps


def compare_zero_sets(local, model, l1):
    var, _, lin = model
    far = np.abs(np.abs(lin) - l1) > 1e-4 * np.maximum(1.0, np.abs(lin))
    assert 1.0 - far.mean() <= 0.02, 1.0 - far.mean()           # the excluded share
    zm, zt = var == 0.0, local == 0.0                           # float 0.0, not a small number
    assert zm[far].sum() > 0.05 * far.sum()                     # the test has zeros to compare
    assert np.array_equal(zm[far], zt[far])


@pytest.mark.parametrize("seed", [21, 22])
def test_exact_zeros_match_model(seed):
    hp, steps = exact_zero_case(seed)
    t, t0 = run_ftrl_table(300, 4, steps, LR, hp)
    compare_zero_sets(t.local.numpy(), ftrl_rows(t0, steps, LR, hp), hp["l1_regularization_strength"])


# ---------------------------------------------------------------- dense fused optimizer
def test_fused_ftrl_cpu_matches_model():
    from distributed_tensorflow_example_amd import optim

    assert optim.KINDS["ftrl"] == 6
    rng = np.random.default_rng(5)
    shapes = [(7,), (33, 5)]
    ps = [torch.tensor(rng.standard_normal(s), dtype=torch.float32) for s in shapes]
    model = [(p.numpy().astype(np.float64), np.full(p.shape, 0.2), np.zeros(p.shape)) for p in ps]
    opt = optim.FusedFtrl(ps, 0.1, learning_rate_power=-0.4, initial_accumulator_value=0.2, l1=0.02, l2=0.01,
                          l2_shrinkage=0.03)
    for k in range(5):
        gs = [rng.standard_normal(s).astype(np.float32) for s in shapes]
        scale = 0.5 if k % 2 else 1.0
        opt.step([torch.from_numpy(g) for g in gs], grad_scale=scale)
        model = [ftrl_dense(v, a, l, g.astype(np.float64) * scale, 0.1, -0.4, 0.02, 0.01, 0.03)
                 for (v, a, l), g in zip(model, gs)]
    for i, p in enumerate(ps):
        np.testing.assert_allclose(p.numpy(), model[i][0], **VAR_TOL)
        np.testing.assert_allclose(opt.m[i].numpy(), model[i][1], **SLOT_TOL)
        np.testing.assert_allclose(opt.v[i].numpy(), model[i][2], **SLOT_TOL)
    with pytest.raises(ValueError):
        optim.FusedFtrl(ps, 0.1, learning_rate_power=0.5)


# ---------------------------------------------------------------- compat front end
F = 4000


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _lr2_graph(tf, **kw):
    """lr2.py's graph (examples/lr2_compat.py) with FtrlOptimizer: W is ps-placed
    and big enough to be a PartitionedVariable, b is a dense variable."""
    with tf.device(tf.train.replica_device_setter(ps_tasks=1)):
        gs = tf.get_variable("global_step", [], initializer=tf.constant_initializer(0), trainable=False)
        with tf.name_scope("input"):
            shp, idx = tf.placeholder(tf.int64), tf.placeholder(tf.int64)
            fid, fv = tf.placeholder(tf.int64), tf.placeholder(tf.float32)
            y = tf.placeholder(tf.float32, [None, 1])
            sp_f = tf.SparseTensor(shape=shp, indices=idx, values=fid)
            sp_v = tf.SparseTensor(shape=shp, indices=idx, values=fv)
        with tf.name_scope("weights"):
            W = tf.Variable(tf.random_normal([F, 1]))
        with tf.name_scope("bias"):
            b = tf.Variable(tf.zeros([1]))
        with tf.name_scope("loss"):
            py_x = tf.add(tf.nn.embedding_lookup_sparse(W, sp_f, sp_v, combiner="sum"), b)
            ce = tf.reduce_mean(tf.nn.sigmoid_cross_entropy_with_logits(py_x, y))
        opt = tf.train.FtrlOptimizer(0.3, l1_regularization_strength=0.01, l2_regularization_strength=0.02, **kw)
        train = opt.minimize(ce, global_step=gs)
    return dict(gs=gs, shp=shp, idx=idx, fid=fid, fv=fv, y=y, W=W, b=b, train=train, ce=ce, opt=opt)


def _csr_batches(n, B=40, seed=0):
    """CSR batches with duplicates inside and across rows, no zero values."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = rng.integers(1, 9, B)
        offs = np.zeros(B + 1, np.int64)
        np.cumsum(k, out=offs[1:])
        ids = rng.integers(0, 300, int(offs[-1])).astype(np.int64) * 13 % F
        vals = (rng.random(int(offs[-1])) * 0.9 + 0.1).astype(np.float32)
        out.append(((rng.random((B, 1)) < 0.4).astype(np.float32), offs, ids, vals))
    return out


def _feed(g, batch):
    y, offs, ids, vals = batch
    row = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    col = np.concatenate([np.arange(k) for k in np.diff(offs)])
    return {g["y"]: y, g["shp"]: np.array([len(offs) - 1, 16]), g["idx"]: np.stack([row, col], 1).astype(np.int64),
            g["fid"]: ids, g["fv"]: vals}


@pytest.fixture
def compat(monkeypatch):
    sys.path.insert(0, REPO)
    monkeypatch.setenv("DTF_SHARD_MIN_ROWS", "1000")
    import distributed_tensorflow_example_amd.compat as tf
    from distributed_tensorflow_example_amd.parallel import world as Wm

    Wm.reset()
    tf.reset_default_graph()
    tf.set_random_seed(7)
    yield tf
    tf.reset_default_graph()
    Wm.reset()


def test_compat_ftrl_constructor_checks(compat):
    tf = compat
    assert "FtrlOptimizer" in tf.train.__all__
    for kw in ({"initial_accumulator_value": -0.1}, {"learning_rate_power": 0.5},
               {"l1_regularization_strength": -1.0}, {"l2_regularization_strength": -1.0},
               {"l2_shrinkage_regularization_strength": -1.0}):
        with pytest.raises(ValueError):
            tf.train.FtrlOptimizer(0.1, **kw)
    o = tf.train.FtrlOptimizer(0.1)
    assert o.name == "Ftrl" and o.get_slot_names() == ["Ftrl", "Ftrl_1"]


@pytest.mark.parametrize("names", [{}, {"accum_name": "acc", "linear_name": "lin"}])
def test_compat_ftrl_slot_names(compat, names):
    tf = compat
    g = _lr2_graph(tf, **names)
    assert type(g["W"]).__name__ == "PartitionedVariable"
    have = {v.name for v in tf.global_variables()}
    a, l = names.get("accum_name", "Ftrl"), names.get("linear_name", "Ftrl_1")
    assert {f"weights/Variable/{a}:0", f"weights/Variable/{l}:0", f"bias/Variable/{a}:0",
            f"bias/Variable/{l}:0"} <= have
    assert g["W"].table.opt_kind == "ftrl" and set(g["W"].table.slots) == {"Ftrl", "Ftrl_1"}


def test_compat_lr2_graph_runs_unlowered_and_matches_model(compat):
    """A dense variable (b) and a partitioned one (W) under FtrlOptimizer.minimize
    on the lr2-shaped graph: only GradientDescentOptimizer is lowered to the fused
    step, so this one runs op by op -- and trains like the float64 model."""
    tf = compat
    from distributed_tensorflow_example_amd.compat import lowering

    g = _lr2_graph(tf)
    batches = _csr_batches(4)
    with tf.Session() as sess:
        sess.run(tf.global_variables_initializer())
        m = LRModel(g["W"].numpy(), 0.3, hp_of(-0.5, 0.01, 0.02, 0.0))
        for bt in batches:
            _, loss = sess.run([g["train"], g["ce"]], feed_dict=_feed(g, bt))
            assert abs(float(loss) - m.step(*bt)) < 1e-5
        plan = lowering.plan_for(g["train"])
        assert plan is None or (plan.trainer is None and plan._nplan is None and plan.steps == 0)
        np.testing.assert_allclose(g["W"].numpy().reshape(-1), m.W, **VAR_TOL)
        np.testing.assert_allclose(g["W"].table.slots["Ftrl"].numpy().reshape(-1), m.acc, **SLOT_TOL)
        np.testing.assert_allclose(g["W"].table.slots["Ftrl_1"].numpy().reshape(-1), m.lin, **SLOT_TOL)
        np.testing.assert_allclose(np.asarray(sess.run(g["b"])).reshape(-1), m.b, **VAR_TOL)
        assert float(sess.run(g["gs"])) == 4.0


def test_compat_ftrl_checkpoint_resumes_bit_equal(compat, tmp_path):
    tf = compat
    from distributed_tensorflow_example_amd.compat import saver as S

    batches = _csr_batches(6, seed=2)

    def state(g, sess):
        t = g["W"].table
        slots = {v.name: v.value.detach().clone() for v in tf.global_variables() if v.name.startswith("bias/Variable/")}
        return [g["W"].numpy().copy(), t.slots["Ftrl"].clone(), t.slots["Ftrl_1"].clone(),
                np.asarray(sess.run(g["b"])).copy(), slots]

    g = _lr2_graph(tf)
    with tf.Session() as sess:
        sess.run(tf.global_variables_initializer())
        w0 = g["W"].numpy().copy()
        for bt in batches:
            sess.run(g["train"], feed_dict=_feed(g, bt))
        full = state(g, sess)
    tf.reset_default_graph()
    tf.set_random_seed(7)
    g = _lr2_graph(tf)
    with tf.Session() as sess:
        sess.run(tf.global_variables_initializer())
        assert np.array_equal(g["W"].numpy(), w0)
        for bt in batches[:3]:
            sess.run(g["train"], feed_dict=_feed(g, bt))
        path = tf.train.Saver().save(sess, str(tmp_path / "m"), global_step=g["gs"])
    idx = S.read_bundle_index(path)
    for name in ("weights/Variable", "weights/Variable/Ftrl", "weights/Variable/Ftrl_1"):
        assert idx[name]["slices"] == [[(0, F), (0, 1)]], (name, idx[name])     # one worker: one partition
    assert {"bias/Variable/Ftrl", "bias/Variable/Ftrl_1"} <= set(idx)
    tf.reset_default_graph()
    tf.set_random_seed(99)                    # a fresh graph with other initial values
    g = _lr2_graph(tf)
    with tf.Session() as sess:
        sess.run(tf.global_variables_initializer())
        tf.train.Saver().restore(sess, path)
        for bt in batches[3:]:
            sess.run(g["train"], feed_dict=_feed(g, bt))
        assert float(sess.run(g["gs"])) == 6.0
        got = state(g, sess)
    assert np.array_equal(got[0], full[0]) and torch.equal(got[1], full[1]) and torch.equal(got[2], full[2])
    assert np.array_equal(got[3], full[3])
    assert got[4].keys() == full[4].keys() and all(torch.equal(got[4][k], full[4][k]) for k in full[4])


# ---------------------------------------------------------------- the trainer, 1 and 2 ranks
def _trainer_worker(rank, ws, port, q, files, steps):
    try:
        sys.path.insert(0, REPO)
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port))
        from distributed_tensorflow_example_amd import ckpt
        from distributed_tensorflow_example_amd.data import libsvm
        from distributed_tensorflow_example_amd.models import sparse_lr
        from distributed_tensorflow_example_amd.parallel import world as W

        w = W.init(backend="gloo")
        data = libsvm.load_files(files, 2)
        tr = sparse_lr.SparseLRTrainer(3000, 0.5, w, seed=5, rows=200 // ws, optimizer="ftrl",
                                       optimizer_hp=hp_of(-0.5, 0.002, 0.01, 0.0))
        B = 200
        for s in range(steps):
            rows = np.arange(s * B, (s + 1) * B)
            tr.train_step(data.take(rows[rank * B // ws:(rank + 1) * B // ws]))
        out = [tr.W.full_table().numpy().copy(), tr.W.slot_view("Ftrl").full_table().numpy().copy(),
               tr.W.slot_view("Ftrl_1").full_table().numpy().copy(), tr.b.detach().numpy().copy(),
               tr.b_slots.numpy().copy()]
        local, repl = tr.checkpoint_tensors()
        prefix = ckpt.save_sharded(os.path.join(os.path.dirname(files[0]), f"ck{ws}", "lr"), local, repl, w,
                                   global_step=tr.global_step)
        q.put((rank, out, prefix))
    except Exception:
        import traceback

        q.put((rank, traceback.format_exc(), None))


def _run_trainer(ws, files, steps):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_trainer_worker, args=(r, ws, port, q, files, steps)) for r in range(ws)]
    [p.start() for p in ps]
    out = sorted([q.get(timeout=240) for _ in range(ws)], key=lambda r: r[0])
    [p.join(60) for p in ps]
    for r in out:
        assert not isinstance(r[1], str), r[1]
    return out


def test_trainer_ftrl_two_ranks_equal_one(tmp_path):
    """SparseLRTrainer(optimizer="ftrl") on the sharded path: 2 x 100 rows == 1 x
    200 (the 1/W average travels as grad_scale), at the tolerance of the SGD
    2-rank tests (tests/test_sparse_cpu.py); the checkpoint holds TF's slots."""
    from distributed_tensorflow_example_amd.compat import saver
    from distributed_tensorflow_example_amd.data import libsvm

    files = libsvm.write_synthetic(str(tmp_path / "train" / "part"), 2, 700, 3000, 12, seed=0)
    one = _run_trainer(1, files, 6)
    two = _run_trainer(2, files, 6)
    for a, b in zip(two[0][1], two[1][1]):
        assert np.array_equal(a, b)
    for a, b in zip(one[0][1], two[0][1]):
        assert np.allclose(a, b, atol=1e-6), np.abs(a - b).max()
    assert (one[0][1][0] == 0.0).sum() > 0               # l1 > 0: exact zeros among the touched rows
    idx = saver.read_bundle_index(two[0][2])
    assert {"weights/Variable/Ftrl", "weights/Variable/Ftrl_1", "bias/Variable/Ftrl", "bias/Variable/Ftrl_1"} <= set(idx)
    assert idx["weights/Variable/Ftrl"]["slices"] == [[(0, 1500), (0, 1)], [(1500, 1500), (0, 1)]]
    assert np.array_equal(saver.read_tensor(two[0][2], "weights/Variable/Ftrl_1").numpy(), two[0][1][2])


def test_trainer_default_is_sgd_without_slots():
    from distributed_tensorflow_example_amd.models.sparse_lr import SparseLRTrainer

    tr = SparseLRTrainer(100, 0.1, World(device="cpu"), device="cpu")
    assert tr.optimizer == "sgd" and tr.W.slots == {} and tr.b_slots is None and tr._bopt is None
    assert set(tr.checkpoint_tensors()[0]) == {"weights/Variable"}
    with pytest.raises(ValueError):
        SparseLRTrainer(100, 0.1, World(device="cpu"), device="cpu", optimizer="adagrad")
    with pytest.raises(ValueError):
        ShardedEmbedding(10, 1, World(device="cpu")).set_optimizer("ftrl", learning_rate_power=0.5)


def test_example_trains_with_ftrl(tmp_path):
    """examples/sparse_lr.py --optimizer=ftrl (one ps, one worker) on synthetic
    libsvm shards: the loss falls, the AUC is above chance, and the result JSON
    reports the share of exactly-zero weights among the rows seen."""
    import json
    import re
    import subprocess

    from distributed_tensorflow_example_amd.data import libsvm

    tr = libsvm.write_synthetic(str(tmp_path / "train" / "part"), 2, 1000, 3000, 12, seed=0)
    te = libsvm.write_synthetic(str(tmp_path / "test" / "part"), 1, 400, 3000, 12, seed=1)
    conf = tmp_path / "cluster_conf.json"
    conf.write_text(json.dumps({"ps": [f"127.0.0.1:{_free_port()}"], "worker": [f"127.0.0.1:{_free_port()}"]}))
    common = [f"--cluster_conf={conf}", f"--train={','.join(tr)}", f"--test={','.join(te)}", "--features=3000",
              "--num_epochs=3", "--learning_rate=0.5", "--batch_size=100", "--trace_step_interval=5",
              "--optimizer=ftrl", "--l1=0.01", "--l2=0.001", "--learning_rate_power=-0.5"]
    env = dict(os.environ, PYTHONPATH=REPO, DTF_RENDEZVOUS_TIMEOUT="120", CUDA_VISIBLE_DEVICES="")
    script = os.path.join(REPO, "examples", "sparse_lr.py")
    procs = [subprocess.Popen([sys.executable, script, "--job_name=ps", "--task_index=0"] + common, env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True),
             subprocess.Popen([sys.executable, script, "--job_name=worker", "--task_index=0",
                               f"--result_json={tmp_path}/w0.json"] + common, env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True)]
    try:
        outs = [p.communicate(timeout=240)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), outs
    res = json.loads((tmp_path / "w0.json").read_text())
    losses = [float(x) for x in re.findall(r"loss: ([0-9.eE+-]+)", outs[1])]
    assert res["loss"] == losses[-1] < losses[0]
    assert res["auc"] > 0.5 and res["optimizer"] == "ftrl" and res["global_step"] == 60
    assert res["rows_seen"] > 0 and 0.0 < res["zero_share"] < 1.0
