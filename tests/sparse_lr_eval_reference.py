"""Float64 model of the sparse-LR forward-only evaluation, with derived error
bounds for the fp32 kernels (csrc/kernels/sparse_lr.hip slr_eval_rows +
eval_record.hip eval_record_reduce).  Not a test module:
tests/test_sparse_lr_eval_*.py and test_eval_record_gpu.py import it.

The model (lr2.py:383-400), per batch row r with entries (id_j, v_j):

    z_r    = b + sum_j W[id_j] v_j          ids outside [0, F) skipped and counted
    loss_r = max(z, 0) - z y + log1p(exp(-|z|))
    p_r    = 1 / (1 + exp(-z))
    bin_r  = #{i : t_i < p_r},  t = fp32(-1e-7), fp32(j / (T - 1)) (0 < j < T - 1), fp32(1 + 1e-7)
    pos / neg [T + 1]: rows per bin with label != 0 / == 0;  AUC: TF's compute_auc

all in float64 from the fp32 inputs' exact values.

Bounds for the kernel (u = 2^-24, the fp32 unit roundoff).  None of them comes
from running the kernel.

z.  The kernel forms n products fl(W v) (n: the row's in-range entries), adds
them in some order (per lane in sequence, then a butterfly over the wave; adds
of the idle lanes' zeros are exact) and adds the bias.  A term passes through
one product rounding, at most n - 1 inexact additions and the bias addition,
so with the standard summation bound (Higham, Accuracy and Stability, 4.2)

    zb = gamma(n + 1) (sum_j |W v| + |b|),   gamma(k) = k u / (1 - k u).

A fused multiply-add only removes roundings.  Where every product is a
multiple of 1/8 and sum |W v| + |b| < 2^20 (the exact fixture), every partial
sum in any order is a multiple of 1/8 below 2^20, hence an fp32 number: no
addition rounds and zb = 0 (`exact_sum`, which checks the condition).

exp.  The kernel's __expf(x) is exp2(fl(x * fl(log2 e))) on the hardware's
exp2 (1 ulp <= 2 u relative).  The argument carries the constant's rounding,
the product's rounding (u each) and here the error of x itself; an argument
error d scales the result by 2^d, i.e. relatively by |x log2 e| ln 2 (2 u) =
2 u |x| at first order.  With a third u |x| and 2 u more for the second order
terms and a possible range-scaling multiply:

    re(x) = u (3 |x| + 4),  plus 2^-126 absolute where the result is flushed.

p = 1 / (1 + e), e = __expf(-z~), z~ within zb of z.  sigmoid' = p (1 - p) <=
min(p, 1 - p) = sigmoid(-|z|), which falls with |z|: over the interval of z~ it
is at most q = sigmoid(-max(|z| - zb, 0)), and at most 1/4 anywhere, so z's
error moves p by at most zb min(q, 1/4); dp/de = -1 / (1 + e)^2 gives
e re / (1 + e)^2 = p (1 - p) re <= q re; the addition 1 + e rounds once (u) and
the division is within 2.5 ulp (<= 3 u, the OpenCL / HIP single-precision
limit; correctly rounded it is u):

    pb = zb min(q, 1/4) + q re(|z| + zb) + 4 u p + 2^-126.

Whatever the roundings, e >= 0 gives fl(1 + e) >= 1 and 0 <= fl(1 / fl(1 + e))
<= 1 (rounding is monotone): the kernel's p never crosses the two outer
thresholds -1e-7 and 1 + 1e-7, which therefore never count as near.

loss = fmax(z, 0) - z y + log1pf(e), e = __expf(-|z~|).  d loss / dz = p - y,
|p - y| <= 1 + |y|; d log1p(e) / de * e = e / (1 + e) = q; log1pf is within
2 ulp (<= 4 u relative, of a value <= ln 2); the product z y and the two
additions round once each on magnitudes <= |z| (1 + |y|) + ln 2:

    lb = zb (1 + |y|) + q re(|z| + zb) + 4 u log1p(exp(-|z|))
         + 3 u (|z| (1 + |y|) + ln 2) + 2^-126.

Mean loss.  eval_record_reduce adds the fp32 row losses in fp64 (B additions,
each 2^-53 relative) and the host divides by the row count:

    mb = sum_r lb_r / B + (B + 2) 2^-53 mean |loss|      (+ u |mean| once the mean is stored as fp32).

A path that adds the row losses in fp32 instead (the general path's mean
reduction) adds (B - 1) u mean |loss| for its own summation.

Bins.  A row's fp32 p is within pb of the model's, so its bin can differ from
the model's only if a threshold lies within pb of the model's p, and then it
moves across that threshold alone (pb is far below the threshold spacing):
`near[r, i] = |p_r - t_i| <= pb_r`.  On histograms this reads: the count of
rows above threshold i (the suffix sum of the bins > i, TF's true / false
positives) differs from the model's by at most the number of near rows of that
class at threshold i (`check_histograms`).
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
LN2 = float(np.log(2.0))


def thresholds(T):
    """streaming_auc's fp32 thresholds as float64 values (exact)."""
    t = [0.0 - 1e-7] + [(i + 1) * 1.0 / (T - 1) for i in range(T - 2)] + [1.0 + 1e-7]
    return np.asarray(t, np.float32).astype(np.float64)


def bins_of(p, T):
    """#{i : t_i < p}; NaN -> 0 (as the kernel).  Exact for fp32 and float64 p alike."""
    p = np.asarray(p, np.float64)
    k = np.searchsorted(thresholds(T), p, side="left")
    return np.where(np.isnan(p), 0, k).astype(np.int64)


def gamma(k):
    return k * U / (1.0 - k * U)


def rel_exp(x):
    return U * (3.0 * np.abs(x) + 4.0)


def compute_auc(pos, neg):
    """TF contrib.metrics compute_auc (ROC, trapezoid, epsilon 1e-6, fp32) from T + 1-bin histograms."""
    pos, neg = np.asarray(pos, np.float64), np.asarray(neg, np.float64)
    tp = np.cumsum(pos[::-1])[::-1][1:]
    fp = np.cumsum(neg[::-1])[::-1][1:]
    tp, fn = tp.astype(np.float32), (pos.sum() - tp).astype(np.float32)
    fp, tn = fp.astype(np.float32), (neg.sum() - fp).astype(np.float32)
    eps = np.float32(1e-6)
    rec = (tp + eps) / (tp + fn + eps)
    x = fp / (fp + tn + eps)
    return float(np.sum(((x[:-1] - x[1:]) * (rec[:-1] + rec[1:]) / np.float32(2.0)).astype(np.float32),
                        dtype=np.float32))


def model(labels, offsets, ids, vals, W, b, T, exact_sum=False):
    """The float64 model and the fp32 kernel's per-row bounds; a dict of arrays."""
    y = np.asarray(labels, np.float32).reshape(-1).astype(np.float64)
    off = np.asarray(offsets, np.int64)
    ids = np.asarray(ids, np.int64)
    B, n = y.size, ids.size
    v = np.ones(n, np.float64) if vals is None else np.asarray(vals, np.float32).astype(np.float64)
    W = np.asarray(W, np.float32).reshape(-1).astype(np.float64)
    b = float(np.float32(b))
    F = W.size
    ok = (ids >= 0) & (ids < F)
    row = np.repeat(np.arange(B), np.diff(off))
    prod = np.where(ok, W[np.where(ok, ids, 0)] * v, 0.0)
    z = b + np.bincount(row, weights=prod, minlength=B)
    mag = abs(b) + np.bincount(row, weights=np.abs(prod), minlength=B)
    cnt = np.bincount(row, weights=ok.astype(np.float64), minlength=B)
    bad = int((~ok).sum())
    p = 1.0 / (1.0 + np.exp(-z))
    l1p = np.log1p(np.exp(-np.abs(z)))
    loss = np.maximum(z, 0.0) - z * y + l1p
    zb = gamma(cnt + 1.0) * mag
    if exact_sum:
        assert np.all(prod * 8 == np.round(prod * 8)) and b * 8 == round(b * 8) and mag.max() < 2.0 ** 20
        zb = np.zeros(B)
    q = 1.0 / (1.0 + np.exp(np.maximum(np.abs(z) - zb, 0.0)))
    re = rel_exp(np.abs(z) + zb)
    pb = zb * np.minimum(q, 0.25) + q * re + 4.0 * U * p + TINY
    lb = zb * (1.0 + np.abs(y)) + q * re + 4.0 * U * l1p + 3.0 * U * (np.abs(z) * (1.0 + np.abs(y)) + LN2) + TINY
    k = bins_of(p, T)
    isp = y != 0.0
    pos = np.bincount(k[isp], minlength=T + 1).astype(np.int64)
    neg = np.bincount(k[~isp], minlength=T + 1).astype(np.int64)
    thr = thresholds(T)
    near = np.abs(p[:, None] - thr[None, :]) <= pb[:, None]                 # [B, T]
    near[:, 0] = near[:, -1] = False                                        # 0 <= fp32 p <= 1 always
    mean = float(loss.sum() / B)
    mb = float(lb.sum() / B + (B + 2) * 2.0 ** -53 * np.abs(loss).mean())
    return dict(z=z, p=p, loss=loss, zb=zb, pb=pb, lb=lb, bins=k, pos=pos, neg=neg, near=near, positive=isp,
                mean=mean, mean_bound=mb, fp32_sum_extra=float((B - 1) * U * np.abs(loss).mean()),
                loss_sum=float(loss.sum()), rows=B, bad=bad, auc=compute_auc(pos, neg), T=T)


def _interior_distance(p, T):
    """Distance of each p to the nearest interior threshold (the outer two are
    never crossed); inf for T = 2."""
    thr = thresholds(T)[1:-1]
    if thr.size == 0:
        return np.full(np.shape(p), np.inf)
    return np.abs(np.asarray(p, np.float64)[:, None] - thr[None, :]).min(1)


def near_share(m, guard=1e-5):
    """Share of rows within max(own bound, guard) of a threshold."""
    return float((_interior_distance(m["p"], m["T"]) <= np.maximum(m["pb"], guard)).mean())


def margin(m):
    """Smallest distance of any row's p to a threshold it could cross."""
    return float(_interior_distance(m["p"], m["T"]).min())


def check_rows(m, z32=None, p32=None, loss32=None):
    """Per-row fp32 results against the model: inside the bounds; a bin (of the
    fp32 p) differs only next to a threshold within the row's bound, by one."""
    if z32 is not None:
        assert (np.abs(np.asarray(z32, np.float64) - m["z"]) <= m["zb"]).all(), "z outside its bound"
    if loss32 is not None:
        assert (np.abs(np.asarray(loss32, np.float64) - m["loss"]) <= m["lb"]).all(), "row loss outside its bound"
    if p32 is not None:
        p32 = np.asarray(p32, np.float64)
        assert (np.abs(p32 - m["p"]) <= m["pb"]).all(), "p outside its bound"
        k = bins_of(p32, m["T"])
        d = k - m["bins"]
        assert (np.abs(d) <= 1).all(), "a bin moved by more than one"
        moved = np.nonzero(d)[0]
        for r in moved:            # the threshold crossed: index min(k, model bin)
            assert m["near"][r, min(k[r], m["bins"][r])], f"row {r}: bin moved away from any threshold"
        return k
    return None


def check_histograms(pos, neg, ms):
    """Histograms against the model(s) of the scored batches (a list: one stream)
    under the near-threshold rule: totals equal; rows above threshold i differ
    by at most the class's near rows at i."""
    ms = ms if isinstance(ms, (list, tuple)) else [ms]
    pos, neg = np.asarray(pos, np.int64).reshape(-1), np.asarray(neg, np.int64).reshape(-1)
    for h, key, cls in ((pos, "pos", True), (neg, "neg", False)):
        want = sum(m[key] for m in ms)
        assert h.shape == want.shape and h.sum() == want.sum(), f"{key}: row total"
        slack = sum((m["near"] & (m["positive"] == cls)[:, None]).sum(0) for m in ms)     # [T]
        got_above = np.cumsum(h[::-1])[::-1][1:]
        want_above = np.cumsum(want[::-1])[::-1][1:]
        assert (np.abs(got_above - want_above) <= slack).all(), f"{key}: counts above a threshold"


# ------------------------------------------------------------------ fixtures
def exact_fixture(B, seed=0, F=5000, edge_rows=True):
    """W multiples of 1/8, values +-1 / +-2: every partial sum is exact in fp32 in
    any order, z lands on k / 8 with |k| <= 64.  Row lengths cycle through 0, 1,
    64, 65, 130 (and small ones); with edge_rows and B >= 12 the first rows hold:
    a repeated id, a zero-valued padding entry, one out-of-range id (bad = 1),
    z = +40 and z = -40, a label of 0.5 (on a row with z != 0).  Returns (labels [B, 1], offsets, ids,
    vals, W, b, bad)."""
    rng = np.random.default_rng(seed)
    W = (rng.integers(-4, 5, F) / 8.0).astype(np.float32)
    W[:4] = [5.0, -5.0, 0.125, 0.25]             # ids 0 / 1 build z = +-40 (8 entries of value 1 or 2 ...)
    b = 0.125
    lens = [0, 1, 64, 65, 130, 3, 7, 20]
    rows_ids, rows_vals = [], []
    for r in range(B):
        n = lens[r % len(lens)]
        for _ in range(200):
            i = rng.integers(4, F, n)
            v = rng.choice(np.array([1.0, -1.0, 2.0, -2.0], np.float32), n)
            k = 8.0 * (b + float((W[i].astype(np.float64) * v).sum()))
            if abs(k) <= 64 and (k != 0 or r != 10):     # row 10 (label 0.5): z != 0, so the float label shows
                break
        else:
            i, v = i[:0], v[:0]
        rows_ids.append(i.astype(np.int64))
        rows_vals.append(v.astype(np.float32))
    labels = (rng.random(B) < 0.4).astype(np.float32)
    bad = 0
    if edge_rows and B >= 12:
        rows_ids[5], rows_vals[5] = np.array([7, 7, 7], np.int64), np.array([1, 2, -1], np.float32)   # repeated id
        rows_ids[6], rows_vals[6] = np.array([9, 10, 11], np.int64), np.array([1, 0, 2], np.float32)  # padding entry
        rows_ids[7], rows_vals[7] = np.array([12, F + 3, 13], np.int64), np.array([1, 1, -1], np.float32)
        bad = 1
        rows_ids[8], rows_vals[8] = np.array([0, 0, 0, 0, 2], np.int64), np.array([2, 2, 2, 2, -1], np.float32)  # +40
        rows_ids[9], rows_vals[9] = np.array([1, 1, 1, 1, 2], np.int64), np.array([2, 2, 2, 2, -1], np.float32)  # -40
        labels[8], labels[9] = 0.0, 1.0
        labels[10] = 0.5
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum([len(i) for i in rows_ids], out=offsets[1:])
    ids = np.concatenate(rows_ids) if B else np.zeros(0, np.int64)
    vals = np.concatenate(rows_vals) if B else np.zeros(0, np.float32)
    return labels.reshape(B, 1), offsets, ids, vals, W, b, bad


def random_fixture(B=500, seed=1, F=5000, per_row=20):
    """Normal W, uniform values, Zipf ids, about per_row ids per row."""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal(F) * 0.5).astype(np.float32)
    b = np.float32(-0.3)
    k = rng.integers(per_row // 2, per_row * 3 // 2 + 1, B)
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum(k, out=offsets[1:])
    n = int(offsets[-1])
    ids = np.minimum(rng.zipf(1.3, n) - 1, F - 1).astype(np.int64)
    vals = rng.random(n).astype(np.float32)
    labels = (rng.random((B, 1)) < 0.4).astype(np.float32)
    return labels, offsets, ids, vals, W, float(b), 0


def coo_of(offsets, ids):
    rows = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))
    return np.stack([rows, ids], 1)


# ------------------------------------------------------------------ fp32 emulation
def emulate(labels, offsets, ids, vals, W, b, T, mutant=None):
    """The kernel's arithmetic in NumPy float32 (lanes stride the row, a butterfly
    over 64 lanes, expf / log1pf from libm in fp32) -> (z, loss, p, bins, pos, neg).
    mutant: 'no_bias', 'bool_label' (label read as bool in the loss),
    'bin_shift' (bins shifted by one), 'ge' (p >= t instead of p > t)."""
    f = np.float32
    y = np.asarray(labels, f).reshape(-1)
    B = y.size
    W = np.asarray(W, f).reshape(-1)
    F = W.size
    z = np.zeros(B, f)
    for r in range(B):
        lanes = np.zeros(64, f)
        for j in range(int(offsets[r]), int(offsets[r + 1])):
            i = int(ids[j])
            if i < 0 or i >= F:
                continue
            v = f(1.0) if vals is None else f(vals[j])
            lane = (j - int(offsets[r])) % 64
            lanes[lane] = f(lanes[lane] + f(W[i] * v))
        off = 32
        while off:
            lanes = (lanes + lanes[np.arange(64) ^ off]).astype(f)
            off >>= 1
        z[r] = lanes[0] if mutant == "no_bias" else f(lanes[0] + f(b))
    yl = (y != 0).astype(f) if mutant == "bool_label" else y
    e = np.exp(-np.abs(z), dtype=f)
    loss = (np.maximum(z, f(0)) - z * yl).astype(f) + np.log1p(e, dtype=f)
    p = (f(1) / (f(1) + np.exp(-z, dtype=f))).astype(f)
    thr = thresholds(T)
    k = np.searchsorted(thr, p.astype(np.float64), side="right" if mutant == "ge" else "left").astype(np.int64)
    if mutant == "bin_shift":
        k = np.minimum(k + 1, T)
    isp = y != 0
    return (z, loss.astype(f), p, k, np.bincount(k[isp], minlength=T + 1).astype(np.int64),
            np.bincount(k[~isp], minlength=T + 1).astype(np.int64))
