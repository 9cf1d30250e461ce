"""Float64 model of the Wide&Deep forward-only evaluation, with derived error
bounds for the fp32 kernel (csrc/kernels/wide_deep_eval.hip wd_eval_rows +
eval_record.hip eval_record_reduce).  Not a test module: tests/test_wide_deep_eval_*.py
import it.  The p / loss / bin bounds, the thresholds and the histogram rule
are tests/sparse_lr_eval_reference.py's, applied as they are once z and its
bound zb are known; that module is imported, not changed.

The model, per batch row r with entries (id_j, v_j), n of them inside [0, F):

    wide = sum_j Wt[id_j] v_j                    ids outside [0, F) skipped for both tables, counted
    a_c  = sum_j v_j E[id_j, c]
    emb  = a * scale;  scale = 1 (sum) | 1 / max(sum_j v_j, 1e-30) (mean) | 1 / sqrt(max(sum_j v_j^2, 1e-30)) (sqrtn)
           (the scale of an empty row is 1; the floor is fp32(1e-30), as in embedding_bag_fwd)
    h_0  = emb;  h_{l+1} = relu(h_l W_l + b_l) over the hidden layers;  t = h w_last + b_last
    z    = wide + t + bias;  loss, p, bins, histograms, AUC: sparse_lr_eval_reference

all in float64 from the fp32 inputs' exact values.

Bound zb on the kernel's z (u = 2^-24, gamma(k) = k u / (1 - k u); Higham,
Accuracy and Stability, 3.1 and 4.2).  Nothing below comes from running the
kernel.

Bag column.  The kernel adds n products in some order (per lane in sequence,
then a butterfly over the lanes that share a column; additions of an idle
lane's zero are exact, a fused multiply-add only removes roundings): a term
passes through its product's rounding and at most n - 1 inexact additions, so
|a~_c - a_c| <= gamma(n) A_c,  A_c = sum_j |v_j E[id_j, c]|.

Scale (mean / sqrtn).  The sum s of n terms (v_j, or the rounded products
v_j^2), in any order, has |s~ - s| <= gamma(n) S, S = sum_j |term|; the floor
max(., 1e-30) is 1-Lipschitz, so with m = max(s, 1e-30) (the model asserts
s >= 0) the relative error of the floored sum is at most theta = gamma(n) S / m.
1 / x and rsqrt(x) turn a relative error theta of x into at most
theta / (1 - theta), and round themselves within 2.5 ulp / 2 ulp (<= 4 u
relative; the HIP single-precision limits); the product a~ * scale~ rounds once:

    ds  = theta / (1 - theta) (1 + 4 u) + 4 u,   f = (1 + ds)(1 + u) - 1
    e_c = scale (gamma(n) A_c (1 + f) + |a_c| f)               (sum: scale = 1, f = 0: e_c = gamma(n) A_c)

Layer with fan-in K, input h with per-column absolute error e.  The matrix
cores accumulate exact fp32 products in a fused multiply-add chain over k
(K roundings; zero padding adds exact zeros) and the bias addition rounds once:

    e'_j = sum_k |W_kj| e_k + gamma(K + 1) (sum_k |W_kj| (|h_k| + e_k) + |b_j|)

ReLU is 1-Lipschitz: the error passes through it unchanged.  The width-1 last
layer is a per-lane sequence plus a butterfly (at most K / 64 + 6 <= K additions
for K >= 16) and the bias: the same formula, giving e_t.

Head.  The wide sum is one product rounding, the lane's additions and the
butterfly per term: e_w = gamma(n + 1) sum_j |Wt v|.  z = fl(fl(wide + t) + bias)
rounds twice on magnitudes within |wide| + e_w + |t| + e_t + |bias|:

    zb = e_w + e_t + gamma(2) (|wide| + e_w + |t| + e_t + |bias|)

Exact fixture (combiner sum).  Table entries and every tower weight and bias
are multiples of 1/4, values are in {1/2, 1, 2}: bag terms are multiples of
1/8, and the terms of layer l (1-based) multiples of g_l = 2^-(3 + 2 l).  Where
the absolute sum of every such sum (bias included) stays below 2^24 granules,
every partial sum in any order is a multiple of the granule below 2^24 of them,
hence an fp32 number: nothing rounds, zb = 0 and z is compared bit for bit.  The
shared bias only has to be a multiple of the last granule.  `model(...,
exact_sum=True)` asserts these conditions itself.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sparse_lr_eval_reference import (LN2, TINY, U, bins_of, check_histograms, check_rows, compute_auc,  # noqa: E402,F401
                                      gamma, margin, near_share, rel_exp, thresholds)

FLOOR = float(np.float32(1e-30))
COMBINERS = ("sum", "mean", "sqrtn")


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _is_multiple(a, g):
    a = np.asarray(a, np.float64) / g
    return bool(np.all(a == np.round(a)))


def logits(labels, offsets, ids, vals, Wt, E, layers, bias, combiner="sum", exact_sum=False):
    """(z, zb, bad) in float64: the model's logit per row, the kernel's bound on
    it and the number of ids outside [0, F).  layers: [W_0, b_0, ..., w_last, b_last]."""
    assert combiner in COMBINERS
    off = np.asarray(offsets, np.int64)
    ids = np.asarray(ids, np.int64)
    B, nnz = off.size - 1, ids.size
    v = np.ones(nnz, np.float64) if vals is None else _f64(vals)
    Wt = _f64(Wt).reshape(-1)
    E = _f64(E)
    F, D = E.shape
    assert Wt.size == F
    bias = float(np.float32(bias))
    Ws = [_f64(layers[2 * i]) for i in range(len(layers) // 2)]
    bs = [_f64(layers[2 * i + 1]).reshape(-1) for i in range(len(layers) // 2)]
    ok = (ids >= 0) & (ids < F)
    row = np.repeat(np.arange(B), np.diff(off))
    bad = int((~ok).sum())
    ro, io, vo = row[ok], ids[ok], v[ok]
    n = np.bincount(ro, minlength=B).astype(np.float64)
    wide = np.bincount(ro, weights=Wt[io] * vo, minlength=B)
    wmag = np.bincount(ro, weights=np.abs(Wt[io] * vo), minlength=B)
    a = np.zeros((B, D))
    A = np.zeros((B, D))
    np.add.at(a, ro, vo[:, None] * E[io])
    np.add.at(A, ro, np.abs(vo[:, None] * E[io]))
    nonempty = np.diff(off) > 0
    scale = np.ones(B)
    f = np.zeros(B)
    if combiner != "sum":
        term = vo if combiner == "mean" else vo * vo
        s = np.bincount(ro, weights=term, minlength=B)
        S = np.bincount(ro, weights=np.abs(term), minlength=B)
        assert (s >= 0).all(), "the scale's bound is derived for non-negative weight sums"
        m = np.maximum(s, FLOOR)
        sc = 1.0 / m if combiner == "mean" else 1.0 / np.sqrt(m)
        scale = np.where(nonempty, sc, 1.0)
        theta = gamma(n + (combiner == "sqrtn")) * S / m
        assert (theta < 0.5).all()
        ds = theta / (1.0 - theta) * (1.0 + 4.0 * U) + 4.0 * U
        f = np.where(nonempty, (1.0 + ds) * (1.0 + U) - 1.0, 0.0)
    h = a * scale[:, None]
    e = scale[:, None] * (gamma(n)[:, None] * A * (1.0 + f[:, None]) + np.abs(a) * f[:, None])
    if exact_sum:
        assert combiner == "sum" and _is_multiple(E, 0.25) and _is_multiple(Wt, 0.25)
        assert np.isin(v, (0.5, 1.0, 2.0)).all()
        assert A.max(initial=0.0) * 8 < 2.0 ** 24 and wmag.max(initial=0.0) * 8 < 2.0 ** 24
    g = 0.125
    for l, (W, b) in enumerate(zip(Ws, bs)):
        K = W.shape[0]
        assert h.shape[1] == K and b.size == W.shape[1]
        y = h @ W + b
        mag = np.abs(h) @ np.abs(W) + np.abs(b)
        e = e @ np.abs(W) + gamma(K + 1.0) * ((np.abs(h) + e) @ np.abs(W) + np.abs(b))
        if exact_sum:
            g /= 4.0
            assert _is_multiple(W, 0.25) and _is_multiple(b, 0.25) and mag.max() / g < 2.0 ** 24
        h = np.maximum(y, 0.0) if l < len(Ws) - 1 else y
    assert h.shape[1] == 1
    t, et = h[:, 0], e[:, 0]
    ew = gamma(n + 1.0) * wmag
    z = wide + t + bias
    zb = ew + et + gamma(2.0) * (np.abs(wide) + ew + np.abs(t) + et + abs(bias))
    if exact_sum:
        assert _is_multiple(bias, g) and (wmag + np.abs(t) + abs(bias)).max() / g < 2.0 ** 24
        zb = np.zeros(B)
    return z, zb, bad


def model(labels, offsets, ids, vals, Wt, E, layers, bias, T, combiner="sum", exact_sum=False):
    """The float64 model and the fp32 kernel's per-row bounds: the dict of
    sparse_lr_eval_reference.model (same keys, same p / loss / bin bounds)."""
    y = _f64(labels).reshape(-1)
    B = y.size
    z, zb, bad = logits(labels, offsets, ids, vals, Wt, E, layers, bias, combiner, exact_sum)
    p = 1.0 / (1.0 + np.exp(-z))
    l1p = np.log1p(np.exp(-np.abs(z)))
    loss = np.maximum(z, 0.0) - z * y + l1p
    q = 1.0 / (1.0 + np.exp(np.maximum(np.abs(z) - zb, 0.0)))
    re = rel_exp(np.abs(z) + zb)
    pb = zb * np.minimum(q, 0.25) + q * re + 4.0 * U * p + TINY
    lb = zb * (1.0 + np.abs(y)) + q * re + 4.0 * U * l1p + 3.0 * U * (np.abs(z) * (1.0 + np.abs(y)) + LN2) + TINY
    k = bins_of(p, T)
    isp = y != 0.0
    pos = np.bincount(k[isp], minlength=T + 1).astype(np.int64)
    neg = np.bincount(k[~isp], minlength=T + 1).astype(np.int64)
    thr = thresholds(T)
    near = np.abs(p[:, None] - thr[None, :]) <= pb[:, None]
    near[:, 0] = near[:, -1] = False
    mean = float(loss.sum() / B)
    mb = float(lb.sum() / B + (B + 2) * 2.0 ** -53 * np.abs(loss).mean())
    return dict(z=z, p=p, loss=loss, zb=zb, pb=pb, lb=lb, bins=k, pos=pos, neg=neg, near=near, positive=isp,
                mean=mean, mean_bound=mb, fp32_sum_extra=float((B - 1) * U * np.abs(loss).mean()),
                loss_sum=float(loss.sum()), rows=B, bad=bad, auc=compute_auc(pos, neg), T=T)


# ------------------------------------------------------------------ fixtures
def _quarters(rng, shape, nonzero):
    """Multiples of 1/4 in {-1/2, -1/4, 1/4, 1/2}, each entry nonzero with probability `nonzero`."""
    val = rng.choice(np.array([-0.5, -0.25, 0.25, 0.5], np.float32), shape)
    return np.where(rng.random(shape) < nonzero, val, np.float32(0)).astype(np.float32)


def exact_fixture(B, D=16, hidden=(32, 16), seed=0, F=5000, with_vals=True, edge_rows=True, bias=0.0):
    """Every sum exact in fp32 in any order (the module docstring's conditions;
    model(..., exact_sum=True) asserts them).  Row lengths cycle through 0, 1,
    64, 65, 130 (and small ones); with edge_rows and B >= 12: row 5 repeats an
    id, row 7 holds one out-of-range id (bad = 1), row 10 has the label 0.5.
    Returns (labels [B, 1], offsets, ids, vals | None, Wt, E, layers, bias, bad)."""
    rng = np.random.default_rng(seed)
    Wt = _quarters(rng, F, 0.5)
    E = _quarters(rng, (F, D), 0.5)
    dims = [D] + list(hidden) + [1]
    layers = []
    for i in range(len(dims) - 1):
        layers += [_quarters(rng, (dims[i], dims[i + 1]), min(1.0, 6.0 / dims[i])),
                   _quarters(rng, dims[i + 1], 0.75)]
    lens = [0, 1, 64, 65, 130, 3, 7, 20]
    rows_ids = [rng.integers(0, F, lens[r % len(lens)]).astype(np.int64) for r in range(B)]
    labels = (rng.random(B) < 0.4).astype(np.float32)
    bad = 0
    if edge_rows and B >= 12:
        rows_ids[5] = np.array([7, 7, 7], np.int64)
        rows_ids[7] = np.array([12, F + 3, 13, 14, 15, 16, 17], np.int64)
        bad = 1
        labels[10] = 0.5
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum([len(i) for i in rows_ids], out=offsets[1:])
    ids = np.concatenate(rows_ids)
    vals = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), ids.size) if with_vals else None
    return labels.reshape(B, 1), offsets, ids, vals, Wt, E, layers, float(bias), bad


def random_fixture(B=33, D=16, hidden=(32, 16), seed=1, F=5000, per_row=20):
    """Normal tables, positive uniform values, Zipf ids, about per_row ids per
    row; row 0 is empty when B > 1.  The tower's weights are normal and sparse,
    about 8 per column (variance preserving: std 1/2), and the last layer is
    scaled by 0.1.  A dense layer would do for the kernel but not for the bound:
    the layer rule propagates absolute values, so a dense fan-in of K loosens it
    by about sqrt(K) per layer (0.04 on p at 128-512-256-1, eight bins wide),
    and the near-threshold rule would then decide nothing.  With 8 terms per
    column the bound on p stays near 1e-5, well inside a bin at T = 200."""
    rng = np.random.default_rng(seed)
    Wt = (rng.standard_normal(F) * 0.3).astype(np.float32)
    E = (rng.standard_normal((F, D)) * 0.3).astype(np.float32)
    dims = [D] + list(hidden) + [1]
    layers = []
    for i in range(len(dims) - 1):
        K, N = dims[i], dims[i + 1]
        W = rng.standard_normal((K, N)) * 0.5 * (rng.random((K, N)) < min(1.0, 8.0 / K))
        layers += [(W * (0.1 if N == 1 else 1.0)).astype(np.float32),
                   (rng.standard_normal(N) * 0.1).astype(np.float32)]
    k = rng.integers(per_row // 2, per_row * 3 // 2 + 1, B)
    if B > 1:
        k[0] = 0
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum(k, out=offsets[1:])
    n = int(offsets[-1])
    ids = np.minimum(rng.zipf(1.3, n) - 1, F - 1).astype(np.int64)
    vals = (0.1 + 0.9 * rng.random(n)).astype(np.float32)
    labels = (rng.random((B, 1)) < 0.4).astype(np.float32)
    return labels, offsets, ids, vals, Wt, E, layers, -0.3, 0


# The cases both test modules run (the CPU module asserts the conditions on them
# that the GPU module relies on).  Exact: (D, hidden, row tile, B) with B at one
# below, at and one above the tile, two tiles + 1, and 1.
EXACT_SHAPES = ((16, (32, 16)), (64, (64,)))
EXACT_CASES = [(D, hid, tile, B) for D, hid in EXACT_SHAPES for tile in (16, 32)
               for B in (tile - 1, tile, tile + 1, 2 * tile + 1)] + [(D, hid, 16, 1) for D, hid in EXACT_SHAPES]
EXACT_T = (2, 200, 1000)
# Random: (D, hidden, combiner, seed) at B = 33; every D, every tower and every combiner appears.
RANDOM_CASES = [(4, (16,), "sum", 1), (20, (48, 16), "mean", 2), (64, (64, 32), "sqrtn", 13),
                (128, (512, 256), "sum", 14), (64, (512, 256), "mean", 5), (20, (16,), "sqrtn", 6),
                (128, (64, 32, 16), "sum", 17)]


def exact_seed(D, B):
    return 100 * D + B


# ------------------------------------------------------------------ fp32 emulation
MUTANTS =("no_relu", "no_layer_bias", "no_wide", "mean_for_sum", "transposed", "no_shared_bias")


def emulate(labels, offsets, ids, vals, Wt, E, layers, bias, T, combiner="sum", mutant=None):
    """The kernel's arithmetic in NumPy float32 (bags in sequence, fp32 matrix
    products, expf / log1pf from libm in fp32) -> (z, loss, p, bins, pos, neg).
    mutant: 'no_relu' (the first hidden ReLU missing), 'no_layer_bias' (layer
    0's bias dropped), 'no_wide' (the wide part dropped), 'mean_for_sum' (mean
    where sum was asked), 'transposed' (the first square layer's weight
    transposed), 'no_shared_bias'."""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    y = np.asarray(labels, f).reshape(-1)
    B = y.size
    Wt = np.asarray(Wt, f).reshape(-1)
    E = np.asarray(E, f)
    F, D = E.shape
    if mutant == "mean_for_sum":
        assert combiner == "sum"
        combiner = "mean"
    h = np.zeros((B, D), f)
    wide = np.zeros(B, f)
    for r in range(B):
        ws = f(0)
        for j in range(int(offsets[r]), int(offsets[r + 1])):
            i = int(ids[j])
            if i < 0 or i >= F:
                continue
            v = f(1.0) if vals is None else f(vals[j])
            h[r] = (h[r] + (E[i] * v).astype(f)).astype(f)
            wide[r] = f(wide[r] + f(Wt[i] * v))
            ws = f(ws + (f(v * v) if combiner == "sqrtn" else v))
        if offsets[r + 1] > offsets[r] and combiner != "sum":
            m = max(ws, f(1e-30))
            h[r] = (h[r] * (f(1) / m if combiner == "mean" else f(1) / np.sqrt(m, dtype=f))).astype(f)
    nl = len(layers) // 2
    done_t = False
    for l in range(nl):
        W, b = np.asarray(layers[2 * l], f), np.asarray(layers[2 * l + 1], f).reshape(-1)
        if mutant == "transposed" and not done_t and W.shape[0] == W.shape[1]:
            W, done_t = np.ascontiguousarray(W.T), True
        y2 = (h @ W).astype(f)
        if not (mutant == "no_layer_bias" and l == 0):
            y2 = (y2 + b).astype(f)
        h = y2 if (l == nl - 1 or (mutant == "no_relu" and l == 0)) else np.maximum(y2, f(0))
    assert mutant != "transposed" or done_t, "the 'transposed' mutant needs a square layer"
    t = h[:, 0]
    z = t.copy() if mutant == "no_wide" else (wide + t).astype(f)
    if mutant != "no_shared_bias":
        z = (z + f(bias)).astype(f)
    e = np.exp(-np.abs(z), dtype=f)
    loss = ((np.maximum(z, f(0)) - z * y).astype(f) + np.log1p(e, dtype=f)).astype(f)
    p = (f(1) / (f(1) + np.exp(-z, dtype=f))).astype(f)
    k = bins_of(p, T)
    isp = y != 0
    return (z, loss, p, k, np.bincount(k[isp], minlength=T + 1).astype(np.int64),
            np.bincount(k[~isp], minlength=T + 1).astype(np.int64))
