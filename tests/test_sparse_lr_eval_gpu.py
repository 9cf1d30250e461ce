"""The forward-only sparse-LR evaluation on the GPU (csrc/kernels/sparse_lr.hip
slr_eval_rows + slr_eval_reduce, csrc/bind_sparse.cpp SparseLRPlan.evaluate /
eval_csr / eval_coo, models/sparse_lr.py, compat/lowering.py) against the
float64 model and derived bounds of tests/sparse_lr_eval_reference.py.

Exact fixture: z bit for bit, every bin and the histograms exactly.  Random
fixture: z, p and the loss per row inside their bounds; a bin differs from the
model's only next to a threshold within the row's own bound."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sparse_lr_eval_reference as R  # noqa: E402
from eval_record_util import SENT, _check_sentinels, _outs, _read, _record  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 5000


def _plan(native, W, b, ftrl=False, gs=None):
    Wd = torch.from_numpy(np.asarray(W, np.float32)).reshape(-1, 1).cuda().contiguous()
    bd = torch.tensor([b], dtype=torch.float32, device="cuda")
    plan = native.SparseLRPlan(Wd, bd, gs)
    slots = None
    if ftrl:
        slots = (torch.full_like(Wd, 0.1), torch.zeros_like(Wd), torch.tensor([0.1, 0.0], device="cuda"))
        plan.set_ftrl(*slots, l1=0.002, l2=0.01)
    return plan, Wd, bd, slots


def _dev(fx):
    lab, off, ids, vals = fx[:4]
    return (torch.from_numpy(lab).reshape(-1).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(ids).cuda(),
            None if vals is None else torch.from_numpy(vals).cuda())


def _row_losses(plan, dev_batch, T=2):
    """The kernel's loss of every row on its own: one one-row evaluation per row
    on slices of the device batch (the offsets index the whole id array), each
    into a record of its own; one read-back.  A one-row record's loss sum is
    the fp32 row loss exactly.  Also each row's out-of-range count."""
    lab, off, ids, vals = dev_batch
    B, n = lab.numel(), 3 + 2 * (T + 1)
    recs = torch.full((B, n), SENT, dtype=torch.int64, device="cuda")
    runs = plan.eval_runs()
    for r in range(B):
        plan.evaluate(lab[r:r + 1], off[r:r + 2], ids, vals, recs[r], True)
    assert plan.eval_runs() == runs + B
    h = recs.cpu()
    assert (h[:, 1] == 1).all() and (h[:, 3:].sum(1) == 1).all()
    return h[:, 0].contiguous().view(torch.float64).numpy().copy(), h[:, 2].numpy().copy()


@pytest.fixture(scope="module")
def rand():
    fx = R.random_fixture()
    return fx, R.model(*fx[:6], 200)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("B,T", [(1, 200), (5, 200), (255, 200), (256, 1000), (257, 200), (257, 1000), (257, 2)])
def test_exact_fixture_bit_for_bit(native, B, T):
    fx = R.exact_fixture(B, seed=B)
    m = R.model(*fx[:6], T, exact_sum=True)
    plan, Wd, bd, _ = _plan(native, fx[4], fx[5])
    big_rec, rec = _record(T)
    big_out, pred, logits = _outs(B)
    plan.evaluate(*_dev(fx), rec, True, pred, logits)
    ls, rows, bad, pos, neg = _read(rec, T)
    _check_sentinels(big_rec, big_out, B)
    z = logits.cpu().numpy()
    assert np.array_equal(z.astype(np.float64), m["z"])                     # bit for bit
    k = R.check_rows(m, z32=z, p32=pred.cpu().numpy())
    assert np.array_equal(k, m["bins"])
    assert np.array_equal(pos, m["pos"]) and np.array_equal(neg, m["neg"])
    assert rows == B and bad == fx[6] == m["bad"] and plan.bad_ids() == fx[6]
    assert abs(ls - m["loss_sum"]) <= B * m["mean_bound"]
    # every row's own loss (the label 0.5, z = +-40 and out-of-range rows among them) and bad count
    rl, rb = _row_losses(plan, _dev(fx))
    R.check_rows(m, loss32=rl)
    assert rb.sum() == fx[6] and plan.bad_ids() == 2 * fx[6]
    if B >= 12:
        assert rb[7] == 1 and fx[0][10, 0] == 0.5 and m["loss"][10] != R.model(
            (fx[0] != 0).astype(np.float32), *fx[1:6], T, exact_sum=True)["loss"][10]   # the float label matters there
        p = pred.cpu().numpy()
        assert z[8] == 40.0 and z[9] == -40.0 and p[8] == 1.0 and 0.0 <= p[9] < 1e-17     # edge bins T - 1 and 1
        assert k[8] == T - 1 and k[9] == 1
    assert plan.eval_runs() == 1 + B and plan.runs() == 0


@pytest.mark.parametrize("entry", ["evaluate", "eval_csr"])
def test_vals_none_means_one(native, entry):
    lab, off, ids, _, W, b, _ = R.exact_fixture(64, seed=3, edge_rows=False)
    m = R.model(lab, off, ids, None, W, b, 200, exact_sum=True)
    plan, *_ = _plan(native, W, b)
    _, rec = _record(200)
    _, pred, logits = _outs(64)
    if entry == "evaluate":
        plan.evaluate(*_dev((lab, off, ids, None)), rec, True, pred, logits)
    else:
        assert plan.eval_csr(lab, off, ids, None, rec, True, pred, logits)
    z = logits.cpu().numpy()
    assert np.array_equal(z.astype(np.float64), m["z"])
    k = R.check_rows(m, z32=z, p32=pred.cpu().numpy())
    _, rows, bad, pos, neg = _read(rec, 200)
    assert rows == 64 and bad == 0
    assert np.array_equal(pos, np.bincount(k[m["positive"]], minlength=201))
    assert np.array_equal(neg, np.bincount(k[~m["positive"]], minlength=201))
    R.check_histograms(pos, neg, m)


def test_random_fixture_inside_bounds(native, rand):
    fx, m = rand
    B = m["rows"]
    plan, *_ = _plan(native, fx[4], fx[5])
    big_rec, rec = _record(200)
    big_out, pred, logits = _outs(B)
    plan.evaluate(*_dev(fx), rec, True, pred, logits)
    ls, rows, bad, pos, neg = _read(rec, 200)
    _check_sentinels(big_rec, big_out, B)
    z, p = logits.cpu().numpy(), pred.cpu().numpy()
    k = R.check_rows(m, z32=z, p32=p)
    # the kernel bins its own fp32 p exactly as the shared threshold function does
    assert np.array_equal(pos, np.bincount(k[m["positive"]], minlength=201))
    assert np.array_equal(neg, np.bincount(k[~m["positive"]], minlength=201))
    R.check_histograms(pos, neg, m)
    err = abs(ls / B - m["mean"])
    print(f"mean loss error {err:.3g} (bound {m['mean_bound']:.3g}); max z error "
          f"{np.abs(z - m['z']).max():.3g} (bound {m['zb'].max():.3g}); bins moved {(k != m['bins']).sum()}")
    assert rows == B and bad == 0 and err <= m["mean_bound"]
    # every row's own loss inside its own bound
    rl, _ = _row_losses(plan, _dev(fx))
    R.check_rows(m, loss32=rl)
    print(f"max row loss error / bound {np.max(np.abs(rl - m['loss']) / m['lb']):.3g}")
    assert abs(float(rl.sum()) - ls) <= 4 * B * 2.0 ** -53 * abs(ls)            # the record summed these very values


def test_entry_points_give_identical_records(native):
    fx = R.exact_fixture(257, seed=1)
    lab, off, ids, vals, W, b, nbad = fx
    plan, *_ = _plan(native, W, b)
    recs = []
    for entry in ("evaluate", "eval_csr", "eval_coo", "eval_coo_unsorted", "eval_csr_strided"):
        _, rec = _record(200)
        _, pred, logits = _outs(257)
        coo = R.coo_of(off, ids)
        if entry == "evaluate":
            plan.evaluate(*_dev(fx), rec, True, pred, logits)
        elif entry == "eval_csr":
            assert plan.eval_csr(lab, off, ids, vals, rec, True, pred, logits)
        elif entry == "eval_csr_strided":
            assert plan.eval_csr(lab.reshape(-1), off, np.repeat(ids, 2)[::2], np.repeat(vals, 2)[::2], rec, True,
                                 pred, logits)
        elif entry == "eval_coo":
            assert plan.eval_coo(lab, coo, ids, vals, rec, True, pred, logits)
        else:
            perm = np.random.default_rng(0).permutation(ids.size)           # rows out of order: the counting sort
            assert plan.eval_coo(lab, coo[perm], ids[perm], vals[perm], rec, True, pred, logits)
        recs.append((rec.clone(), pred.clone(), logits.clone()))
    for rec, pred, logits in recs[1:]:
        assert torch.equal(rec, recs[0][0]) and torch.equal(pred, recs[0][1]) and torch.equal(logits, recs[0][2])
    assert plan.eval_runs() == 5 and plan.bad_ids() == 5 * nbad


def test_refused_feeds_launch_nothing(native):
    lab, off, ids, vals, W, b, _ = R.exact_fixture(16, seed=2)
    plan, *_ = _plan(native, W, b)
    big, rec = _record(200)
    coo = R.coo_of(off, ids)
    assert not plan.eval_csr(lab.astype(np.float64), off, ids, vals, rec, True)          # labels not fp32
    assert not plan.eval_csr(lab, off.astype(np.int32), ids, vals, rec, True)
    assert not plan.eval_csr(lab, off[:-1], ids, vals, rec, True)                        # not B + 1 offsets
    bad_off = off.copy()
    bad_off[3] = off[-1] + 5
    assert not plan.eval_csr(lab, bad_off, ids, vals, rec, True)                         # not a CSR of nnz
    assert not plan.eval_coo(lab, coo, ids.astype(np.int32), vals, rec, True)
    bad_coo = coo.copy()
    bad_coo[5, 0] = 16
    assert not plan.eval_coo(lab, bad_coo, ids, vals, rec, True)                         # a row outside the batch
    torch.cuda.synchronize()
    assert plan.eval_runs() == 0 and (big == SENT).all() and plan.bad_ids() == 0
    with pytest.raises(RuntimeError):
        plan.eval_csr(lab, off, ids, vals, torch.zeros(8, dtype=torch.int64, device="cuda"), True)    # T < 2
    with pytest.raises(RuntimeError):
        plan.evaluate(*_dev((lab, off, ids, vals)), rec, True, torch.zeros(15, device="cuda"), None)  # pred != B


def test_record_accumulates_resets_and_repeats(native, rand):
    fx, m = rand
    lab, off, ids, vals = fx[:4]
    plan, *_ = _plan(native, fx[4], fx[5])
    _, whole = _record(200)
    plan.evaluate(*_dev(fx), whole, True)
    _, again = _record(200)
    plan.evaluate(*_dev(fx), again, True)
    assert torch.equal(whole, again)                                                     # two runs, the same bits
    _, parts = _record(200)
    cuts = [0, 1, 257, 500]                                                              # 1 + 256 + 243 rows
    for c, (r0, r1) in enumerate(zip(cuts[:-1], cuts[1:])):
        s, e = int(off[r0]), int(off[r1])
        part = (lab[r0:r1], off[r0:r1 + 1] - off[r0], ids[s:e], vals[s:e])
        if c == 1:
            assert plan.eval_csr(*part, parts, False)                                    # host and device calls mix
        else:
            plan.evaluate(*_dev(part), parts, c == 0)
    a, b = _read(whole, 200), _read(parts, 200)
    assert a[1:3] == b[1:3] == (500, 0) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    assert abs(a[0] - b[0]) <= 4 * 2.0 ** -53 * abs(a[0])
    plan.evaluate(*_dev(fx), parts, False)                                               # accumulates on
    c = _read(parts, 200)
    assert c[1] == 1000 and np.array_equal(c[3], 2 * a[3]) and abs(c[0] - 2 * a[0]) <= 8 * 2.0 ** -53 * c[0]
    plan.evaluate(*_dev(fx), parts, True)                                                # reset restarts
    assert torch.equal(parts, whole)


def test_evaluation_replays_in_a_graph(native, rand):
    from distributed_tensorflow_example_amd.utils.graphs import GraphedStep

    fx, m = rand
    plan, *_ = _plan(native, fx[4], fx[5])
    _, once = _record(200)
    plan.evaluate(*_dev(fx), once, True)
    rec = torch.zeros_like(once)
    g = GraphedStep(lambda lab, off, ids, vals: plan.evaluate(lab, off, ids, vals, rec, False), lambda: [rec])
    for _ in range(3):
        g(*_dev(fx))
    assert g.captures == 1 and g.replays == 3
    a, b = _read(once, 200), _read(rec, 200)
    assert b[1] == 3 * a[1] and np.array_equal(b[3], 3 * a[3]) and np.array_equal(b[4], 3 * a[4])
    assert abs(b[0] - 3 * a[0]) <= 8 * 2.0 ** -53 * b[0]
    # a larger eager batch outgrows the plan's scratch; the captured graph's stays alive
    big = R.random_fixture(B=1100, seed=9)
    _, other = _record(200)
    plan.evaluate(*_dev(big), other, True)
    assert _read(other, 200)[1] == 1100
    g(*_dev(fx))
    c = _read(rec, 200)
    assert g.captures == 1 and c[1] == 4 * a[1] and np.array_equal(c[3], 4 * a[3]) and np.array_equal(c[4], 4 * a[4])
    assert abs(c[0] - 4 * a[0]) <= 8 * 2.0 ** -53 * c[0]


@pytest.mark.parametrize("ftrl", [False, True])
def test_training_state_is_untouched(native, rand, ftrl):
    fx, m = rand
    gs = torch.zeros((), dtype=torch.int64, device="cuda")
    plan, Wd, bd, slots = _plan(native, fx[4], fx[5], ftrl=ftrl, gs=gs)
    plan.step(*_dev(fx), 0.1)
    state = [Wd, bd, gs, plan.loss()] + (list(slots) + [plan.grad_accumulator()] if ftrl else [])
    before = [t.clone() for t in state]
    _, rec = _record(200)
    plan.evaluate(*_dev(fx), rec, True)
    assert plan.eval_csr(*fx[:4], rec, False)
    assert plan.eval_coo(fx[0], R.coo_of(fx[1], fx[2]), fx[2], fx[3], rec, False)
    torch.cuda.synchronize()
    for a, b in zip(before, state):
        assert torch.equal(a, b)
    assert plan.runs() == 1 and plan.eval_runs() == 3 and int(gs) == 1 and plan.timing()["runs"] == 1


def _distinct_batch(seed, B=64, per=5):
    """A training batch in which no id repeats: its scatter update adds once per
    id, so the step is deterministic (no order of float atomics to differ in)."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(F)[:B * per].astype(np.int64)
    return ((rng.random((B, 1)) < 0.4).astype(np.float32), np.arange(0, B * per + 1, per, dtype=np.int64), ids,
            rng.random(B * per).astype(np.float32))


def test_host_fed_train_eval_train_share_the_slots(native, rand):
    """run_csr / eval_csr / eval_csr / run_csr back to back on one stream with no
    host synchronisation: training and evaluation share the two staging slots,
    and every call must see the feed it packed.  The same calls on device
    tensors (no staging) give the same bits, and the model's sequence holds."""
    fx, _ = rand
    t1, t2 = _distinct_batch(11), _distinct_batch(12)
    half = (fx[0][:250], fx[1][:251], fx[2][:int(fx[1][250])], fx[3][:int(fx[1][250])])
    host, W1, b1, _ = _plan(native, fx[4], fx[5])
    dev, W2, b2, _ = _plan(native, fx[4], fx[5])
    _, rh = _record(200)
    _, rd = _record(200)
    assert host.run_csr(*t1, 0.25) and host.eval_csr(*half, rh, True) and host.eval_csr(*fx[:4], rh, False)
    assert host.run_csr(*t2, 0.25)
    dev.step(*_dev(t1), 0.25)
    Ws, bs = W2.cpu().numpy().reshape(-1), float(b2)            # the weights the evaluations must have seen
    dev.evaluate(*_dev(half), rd, True)
    dev.evaluate(*_dev(fx), rd, False)
    dev.step(*_dev(t2), 0.25)
    torch.cuda.synchronize()
    assert torch.equal(rh, rd) and torch.equal(W1, W2) and torch.equal(b1, b2)
    assert not np.array_equal(Ws, fx[4]) and host.eval_runs() == 2 and host.runs() == 2
    ms = [R.model(*half, Ws, bs, 200), R.model(*fx[:4], Ws, bs, 200)]
    ls, rows, bad, pos, neg = _read(rh, 200)
    R.check_histograms(pos, neg, ms)
    assert rows == 750 and bad == 0
    assert abs(ls - ms[0]["loss_sum"] - ms[1]["loss_sum"]) <= 250 * ms[0]["mean_bound"] + 500 * ms[1]["mean_bound"]


# ------------------------------------------------------------------ trainer
def _trainer(fx, optimizer="sgd"):
    from distributed_tensorflow_example_amd.models import sparse_lr
    from distributed_tensorflow_example_amd.parallel.world import World

    tr = sparse_lr.SparseLRTrainer(F, 0.1, World(device=torch.device("cuda", 0)), seed=2, optimizer=optimizer)
    with torch.no_grad():
        tr.W.local.copy_(torch.from_numpy(fx[4]).reshape(-1, 1))
        tr.b.data.fill_(float(fx[5]))
    return tr


_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import sparse_lr_eval_reference as R
from distributed_tensorflow_example_amd.models import sparse_lr
from distributed_tensorflow_example_amd.parallel.world import World
fx = R.random_fixture()
tr = sparse_lr.SparseLRTrainer(5000, 0.1, World(device=torch.device("cuda", 0)), seed=2)
assert not tr._fused_ok()
with torch.no_grad():
    tr.W.local.copy_(torch.from_numpy(fx[4]).reshape(-1, 1)); tr.b.data.fill_(float(fx[5]))
batch = tuple(torch.from_numpy(a).cuda() for a in fx[:4])
loss, p = tr.evaluate(batch)
tr.auc_update(batch)
st = tr.evaluate_stream([batch, batch])
np.savez(sys.argv[2], loss=float(loss), p=p.cpu().numpy(), pos=tr.auc_pos.cpu().numpy(), neg=tr.auc_neg.cpu().numpy(),
         auc=tr.auc(), sloss=st["loss"], sauc=st["auc"], srows=st["rows"])
"""


def test_trainer_against_model_and_general_path(native, rand, tmp_path):
    fx, m = rand
    tr = _trainer(fx)
    assert tr._fused_ok()
    dev_batch = tuple(torch.from_numpy(a).cuda() for a in fx[:4])
    host_batch = tuple(fx[:4])
    for batch in (dev_batch, host_batch):
        loss, p = tr.evaluate(batch)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and p.shape == (500,)
        assert abs(float(loss) - m["mean"]) <= m["mean_bound"] + R.U * abs(m["mean"])
        R.check_rows(m, p32=p.cpu().numpy())
    assert tr._plan.eval_runs() == 2 and tr._plan.runs() == 0
    tr.reset_auc()
    tr.auc_update(dev_batch)
    tr.auc_update(host_batch)
    R.check_histograms(tr.auc_pos.cpu().numpy(), tr.auc_neg.cpu().numpy(), [m, m])
    auc2 = tr.auc()
    tr.reset_auc()
    assert int(tr.auc_pos.sum()) == 0
    tr.auc_update(host_batch)
    pos, neg = tr.auc_pos.cpu().numpy(), tr.auc_neg.cpu().numpy()
    assert abs(tr.auc() - R.compute_auc(pos, neg)) <= 1e-6 and abs(tr.auc() - auc2) <= 1e-6
    st = tr.evaluate_stream([dev_batch, host_batch])
    assert st["rows"] == 1000 and abs(st["loss"] - m["mean"]) <= m["mean_bound"]
    assert abs(st["auc"] - tr.auc()) <= 1e-6
    assert np.array_equal(tr.auc_pos.cpu().numpy(), pos)                                 # the stream has its own record
    # the same build's general path (sharded lookup, bag kernel, torch sigmoid, xent op, auc_hist)
    out = str(tmp_path / "general.npz")
    env = dict(os.environ, DTF_SLR_FUSED="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, REPO, out], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    gen = np.load(out)
    bound = m["mean_bound"] + m["fp32_sum_extra"] + R.U * abs(m["mean"])                 # its mean is an fp32 reduction
    print(f"fused {float(tr.evaluate(dev_batch)[0]):.9g} general {float(gen['loss']):.9g} model {m['mean']:.9g} "
          f"bound {bound:.3g}")
    assert abs(float(gen["loss"]) - m["mean"]) <= bound and abs(float(gen["sloss"]) - m["mean"]) <= bound
    R.check_rows(m, p32=gen["p"])
    R.check_histograms(gen["pos"], gen["neg"], m)
    assert int(gen["srows"]) == 1000
    assert abs(float(gen["auc"]) - R.compute_auc(gen["pos"], gen["neg"])) <= 1e-6
    # fused vs general: rows above a threshold differ by at most the near rows there
    for key, cls in (("pos", True), ("neg", False)):
        a = np.cumsum({"pos": pos, "neg": neg}[key][::-1])[::-1][1:]
        b = np.cumsum(gen[key][::-1])[::-1][1:]
        assert (np.abs(a - b) <= (m["near"] & (m["positive"] == cls)[:, None]).sum(0)).all()


def test_trainer_ftrl_plan_evaluates(native, rand):
    fx, m = rand
    tr = _trainer(fx, optimizer="ftrl")
    loss, p = tr.evaluate(tuple(fx[:4]))
    assert tr._plan.ftrl() and tr._plan.eval_runs() == 1
    assert abs(float(loss) - m["mean"]) <= m["mean_bound"] + R.U * abs(m["mean"])
    R.check_rows(m, p32=p.cpu().numpy())


# ------------------------------------------------------------------ Session
def _lr2(tf):
    with tf.device(tf.train.replica_device_setter(ps_tasks=1)):
        gs = tf.get_variable("global_step", [], initializer=tf.constant_initializer(0), trainable=False)
        shp, idx, fid, fv = (tf.placeholder(tf.int64), tf.placeholder(tf.int64), tf.placeholder(tf.int64),
                             tf.placeholder(tf.float32))
        y = tf.placeholder(tf.float32, [None, 1])
        with tf.name_scope("weights"):
            W = tf.Variable(tf.random_normal([F, 1]))
        with tf.name_scope("bias"):
            b = tf.Variable(tf.zeros([1]))
        py_x = tf.add(tf.nn.embedding_lookup_sparse(W, tf.SparseTensor(shape=shp, indices=idx, values=fid),
                                                    tf.SparseTensor(shape=shp, indices=idx, values=fv),
                                                    combiner="sum"), b)
        ce = tf.reduce_mean(tf.nn.sigmoid_cross_entropy_with_logits(py_x, y))
        train = tf.train.GradientDescentOptimizer(0.1).minimize(ce, global_step=gs)
        auc = tf.contrib.metrics.streaming_auc(tf.nn.sigmoid(py_x), y)
    return dict(gs=gs, shp=shp, idx=idx, fid=fid, fv=fv, y=y, W=W, b=b, ce=ce, train=train, auc=auc)


def _feed(g, fx, tensors=False):
    lab, off, ids, vals = fx[:4]
    d = {g["y"]: lab, g["idx"]: R.coo_of(off, ids), g["fid"]: ids, g["fv"]: vals}
    if tensors:
        d = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}
    d[g["shp"]] = [F, len(lab)]
    return d


def _confusion(tf, sess):
    v = {t.name.split("/")[-1].split(":")[0]: np.asarray(sess.run(t)) for t in tf.local_variables()}
    return v["true_positives"], v["false_negatives"], v["true_negatives"], v["false_positives"]


def test_session_eval_lowered_matches_op_by_op(native, rand, monkeypatch):
    monkeypatch.setenv("DTF_SHARD_MIN_ROWS", "1000")
    import distributed_tensorflow_example_amd.compat as tf
    from distributed_tensorflow_example_amd.compat import lowering

    fx, _ = rand
    fxs = [fx, R.random_fixture(B=257, seed=7), R.random_fixture(B=64, seed=8)]
    tf.reset_default_graph()
    g = _lr2(tf)
    with tf.Session() as sess:
        sess.run([tf.global_variables_initializer(), tf.local_variables_initializer()])
        with torch.no_grad():
            g["W"].table.local.copy_(torch.from_numpy(fx[4]).reshape(-1, 1))
            g["b"].value.data.fill_(float(fx[5]))
        # an evaluation before the first train run: the plan is built on demand
        gs0, ce0 = sess.run([g["gs"], g["ce"]], feed_dict=_feed(g, fx))
        plan = lowering.plan_for(g["train"])
        m0 = R.model(*fx[:6], 200)
        assert plan is not None and plan.eval_runs == 1 and plan.steps == 0 and float(gs0) == 0.0
        assert abs(float(ce0) - m0["mean"]) <= m0["mean_bound"] + R.U * abs(m0["mean"])
        for _ in range(2):
            sess.run([g["train"]], feed_dict=_feed(g, fx))
        assert plan.steps == 2 and plan._nplan.runs() == 2
        Wn, bn = g["W"].numpy().reshape(-1), float(np.asarray(sess.run(g["b"])).reshape(-1)[0])
        ms = [R.model(*f[:4], Wn, bn, 200) for f in fxs]
        evals = plan.eval_runs
        gsv, ce = sess.run([g["gs"], g["ce"]], feed_dict=_feed(g, fx))          # lr2.py's Test() fetch
        assert float(gsv) == 2.0 and type(ce) is np.float32
        for f in fxs:
            val = sess.run(g["auc"], feed_dict=_feed(g, f))                      # lr2.py's closing loop
        conf = _confusion(tf, sess)
        assert plan.eval_runs == evals + 4 and plan._nplan.eval_runs() == evals + 4
        assert plan.steps == 2 and plan._nplan.runs() == 2 and float(sess.run(g["gs"])) == 2.0
        # a tensor feed: op by op, the same value
        ce_t = sess.run(g["ce"], feed_dict=_feed(g, fx, tensors=True))
        assert plan.eval_runs == evals + 4
        # the same runs op by op
        monkeypatch.setenv("DTF_GRAPH_LOWERING", "0")
        eager = tf.Session()
        eager.run(tf.local_variables_initializer())
        gse, cee = eager.run([g["gs"], g["ce"]], feed_dict=_feed(g, fx))
        for f in fxs:
            vale = eager.run(g["auc"], feed_dict=_feed(g, f))
        confe = _confusion(tf, eager)
        assert plan.eval_runs == evals + 4 and float(gse) == 2.0 and type(cee) is type(ce)
    bound = ms[0]["mean_bound"] + R.U * abs(ms[0]["mean"])
    print(f"lowered ce {ce:.9g} op-by-op {cee:.9g} tensor-fed {float(ce_t):.9g} model {ms[0]['mean']:.9g}")
    assert abs(float(ce) - ms[0]["mean"]) <= bound
    assert abs(float(cee) - ms[0]["mean"]) <= bound + ms[0]["fp32_sum_extra"]
    assert abs(float(ce_t) - ms[0]["mean"]) <= bound + ms[0]["fp32_sum_extra"]
    # the four confusion variables: fp32 counts (exact below 2^24); rows above a
    # threshold within the near rows of the model, and of each other
    npos = sum(int(m["positive"].sum()) for m in ms)
    nneg = sum(m["rows"] for m in ms) - npos
    for (tp, fn, tn, fp), name in ((conf, "lowered"), (confe, "op by op")):
        assert tp.dtype == np.float32 and tp.shape == (200,)
        assert np.array_equal(tp + fn, np.full(200, npos, np.float32)), name
        assert np.array_equal(fp + tn, np.full(200, nneg, np.float32)), name
    for i, cls in ((0, True), (3, False)):
        want = sum(np.cumsum(m["pos" if cls else "neg"][::-1])[::-1][1:] for m in ms)
        slack = sum((m["near"] & (m["positive"] == cls)[:, None]).sum(0) for m in ms)
        assert (np.abs(conf[i] - want) <= slack).all() and (np.abs(confe[i] - want) <= slack).all()
        assert (np.abs(conf[i] - confe[i]) <= slack).all()
    assert np.allclose(np.asarray(val[1]), np.asarray(vale[1]), atol=1e-4)
    tf.reset_default_graph()


@pytest.mark.parametrize("fused", ["1", "0"])
def test_session_out_of_range_id_raises_at_the_check(native, monkeypatch, fused):
    monkeypatch.setenv("DTF_SHARD_MIN_ROWS", "1000")
    monkeypatch.setenv("DTF_SPARSE_ID_CHECK", "2")
    monkeypatch.setenv("DTF_SLR_FUSED", fused)
    import distributed_tensorflow_example_amd.compat as tf
    from distributed_tensorflow_example_amd.compat import lowering

    fx = R.exact_fixture(16, seed=4)                 # one id outside [0, F)
    ok = R.exact_fixture(16, seed=4, edge_rows=False)
    tf.reset_default_graph()
    g = _lr2(tf)
    with tf.Session() as sess:
        sess.run([tf.global_variables_initializer(), tf.local_variables_initializer()])
        a = sess.run([g["gs"], g["ce"]], feed_dict=_feed(g, ok))
        plan = lowering.plan_for(g["train"])
        assert plan is not None and plan.eval_runs == (1 if fused == "1" else 0)
        if fused == "1":
            with pytest.raises(ValueError, match="outside"):
                sess.run([g["gs"], g["ce"]], feed_dict=_feed(g, fx))            # the second evaluation: the check's turn
            assert plan.eval_runs == 2
        else:
            b = sess.run([g["gs"], g["ce"]], feed_dict=_feed(g, ok))             # DTF_SLR_FUSED=0: op by op
            assert plan._nplan is None and float(a[1]) == float(b[1])
    tf.reset_default_graph()
