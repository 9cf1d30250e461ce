"""models/mlp.py `evaluate` without a GPU: CPU parameters take the PyTorch
path with the same interface, an empty set is an error, and a CPU Session's
accuracy fetch stays eager.  Also the inputs and the fp64 reference that
tests/test_mlp_eval_gpu.py shares."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from test_lowering_cpu import _graph  # noqa: E402

MARGIN = 1e-4      # counts are compared on rows whose fp64 top-2 logit margin is at least this


def ref64(W1, b1, W2, b2, x32, ids, act="sigmoid", naive=False):
    """fp64 evaluation of the same formulas on the float32 inputs:
    (mean loss, correct count, predictions, logits, minimum top-2 margin)."""
    W1, b1, W2, b2, x = (np.asarray(a, dtype=np.float64) for a in (W1, b1, W2, b2, x32))
    z2 = x @ W1 + b1
    a2 = 1.0 / (1.0 + np.exp(-z2)) if act == "sigmoid" else np.maximum(z2, 0.0)
    z3 = a2 @ W2 + b2
    zs = z3 - z3.max(1, keepdims=True)
    lse = np.log(np.exp(zs).sum(1))
    rows = np.arange(len(ids))
    if naive:
        y = np.exp(zs) / np.exp(zs).sum(1, keepdims=True)
        loss = -np.log(y[rows, ids])
    else:
        loss = lse - zs[rows, ids]
    pred = z3.argmax(1)
    top = np.sort(z3, 1)
    margin = float((top[:, -1] - top[:, -2]).min()) if z3.shape[1] > 1 else np.inf
    return float(loss.mean()), int((pred == ids).sum()), pred, z3, margin


def labels_for(W1, b1, W2, b2, x32, rng, act="sigmoid"):
    """The fp64 argmax on even rows, random classes on odd rows: accuracy near 0.55."""
    _, _, pred, z3, _ = ref64(W1, b1, W2, b2, x32, np.zeros(len(x32), dtype=np.int64), act)
    ids = rng.integers(0, z3.shape[1], len(x32))
    ids[::2] = pred[::2]
    return ids.astype(np.int64)


def pixels(rng, N, K):
    """uint8 pixels with 80 % of them zeroed."""
    u8 = rng.integers(0, 256, (N, K), dtype=np.uint8)
    u8[rng.random((N, K)) < 0.8] = 0
    return u8


@functools.lru_cache(maxsize=None)
def case(N, seed, act="sigmoid", naive=False, scale=1.0):
    """784-100-10 inputs of the issue: uint8 pixels from default_rng(100 + seed),
    `init_params(seed)` with the biases set, labels by `labels_for`, and the
    fp64 reference.  Computed once per (N, seed, act, naive) and shared; do not modify."""
    from distributed_tensorflow_example_amd.models import mlp

    rng = np.random.default_rng(100 + seed)
    u8 = pixels(rng, N, mlp.D_IN)
    x32 = u8.astype(np.float32) / np.float32(255.0)
    flat = mlp.init_params(seed) * scale
    flat[mlp.OFF_B1:mlp.OFF_B2] = 0.1 * torch.linspace(-1, 1, mlp.HIDDEN)
    flat[mlp.OFF_B2:] = 0.1 * torch.linspace(-1, 1, mlp.N_CLS)
    p = mlp.unflatten(flat)
    four = [p[k].numpy() for k in ("weights/Variable", "biases/Variable", "weights/Variable_1", "biases/Variable_1")]
    ids = labels_for(*four, x32, rng, act)
    loss, correct, pred, z3, margin = ref64(*four, x32, ids, act, naive)
    return dict(u8=u8, x32=x32, flat=flat, four=four, ids=ids, onehot=np.eye(mlp.N_CLS, dtype=np.float32)[ids],
                loss=loss, correct=correct, pred=pred, z3=z3, margin=margin)


@pytest.mark.parametrize("x_kind,label_kind,naive", [("u8", "ids", False), ("f32", "onehot", True),
                                                     ("f32", "ids", False)])
def test_evaluate_cpu_matches_fp64(x_kind, label_kind, naive):
    from distributed_tensorflow_example_amd.models import mlp

    c = case(333, 1, "sigmoid", naive)
    assert c["margin"] >= MARGIN                       # no row is excluded from the count
    x = c["u8"] if x_kind == "u8" else c["x32"]
    labels = c["ids"] if label_kind == "ids" else c["onehot"]
    loss, acc, pred = mlp.evaluate(c["flat"], x, labels, naive=naive, return_predictions=True)
    assert isinstance(loss, float) and isinstance(acc, float)
    assert abs(loss - c["loss"]) <= 1e-5 * abs(c["loss"]), (loss, c["loss"])
    assert round(acc * 333) == c["correct"]
    assert pred.dtype == torch.int32 and np.array_equal(pred.numpy(), c["pred"])
    # the four tensors instead of the flat master, no predictions: the same numbers
    four = [torch.from_numpy(a) for a in c["four"]]
    assert mlp.evaluate(four, x, labels, naive=naive) == (loss, acc)


def test_evaluate_empty_set_raises():
    from distributed_tensorflow_example_amd.models import mlp

    flat = mlp.init_params(1)
    with pytest.raises(ValueError):
        mlp.evaluate(flat, np.zeros((0, 784), np.uint8), np.zeros((0,), np.uint8))
    with pytest.raises(ValueError):
        mlp.evaluate(flat, torch.zeros(0, 784), torch.zeros(0, dtype=torch.int64))


def test_cpu_session_accuracy_fetch_stays_eager(monkeypatch):
    """A CPU Session trains and evaluates op by op: no plan, no evaluation run."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)    # the graph's device: the CPU, on any machine
    import distributed_tensorflow_example_amd.compat as tf
    from distributed_tensorflow_example_amd.compat import lowering as L

    g = _graph(tf)
    c = case(333, 1)
    rng = np.random.default_rng(0)
    bx = rng.random((20, 784), dtype=np.float32)
    by = np.eye(10, dtype=np.float32)[rng.integers(0, 10, 20)]
    with tf.Session() as sess:
        sess.run(tf.global_variables_initializer())
        assert not g["W"][0].value.is_cuda
        sess.run([g["train"], g["ce"]], feed_dict={g["x"]: bx, g["y_"]: by})
        acc, ce = sess.run([g["acc"], g["ce"]], feed_dict={g["x"]: c["x32"], g["y_"]: c["onehot"]})
        W1, W2, b1, b2 = [v.numpy() for v in g["W"]]
        ref_loss, ref_correct, _, _, margin = ref64(W1, b1, W2, b2, c["x32"], c["ids"], naive=True)
        assert type(acc) is np.float32 and type(ce) is np.float32
        assert abs(ce - ref_loss) <= 1e-5 * abs(ref_loss)
        assert margin >= MARGIN and round(float(acc) * 333) == ref_correct
        assert L.plan_for(g["train"]) is None               # CPU sessions never lower ...
        assert not any(r() is not None and r().op is g["train"] for r in L._EVAL.values())   # ... nor evaluate
    tf.reset_default_graph()
