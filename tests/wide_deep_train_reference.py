"""Float64 model of the fused Wide&Deep training step's per-row half
(csrc/kernels/wide_deep_train.hip wd_train_rows) and of the dense gradients, with
derived bounds for the fp32 kernel.  Not a test module.  The forward model, its
bounds and the fixtures are tests/wide_deep_eval_reference.py's (imported, not
changed); the forward is repeated here only to keep every layer's activation,
pre-activation and bound, and its z is asserted equal to that module's.

Backward of the model, gs = the loss's scale per row (the fp32 value of 1 / B):

    dz      = (p - y) gs
    da_nh   = dz w_last^T;  dzl[l] = da_l * (act[l] > 0);  da_{l-1} = dzl[l] W_{l-1}^T;  demb = da_0
    dW_l    = act[l]^T dzl[l+1];  db_l = sum_r dzl[l+1];  dw_last = act[nh]^T dz;  db_last = dbias = sum_r dz

Bounds (u = 2^-24, gamma(k) as in the forward's; nothing comes from running the kernel):

dz.  The kernel's p is within the forward model's pb; the subtraction and the
product with gs round once each:  e1 = pb + u (|p - y| + pb),  dzb = gs e1 + u gs (|p - y| + e1).
da_nh = dz w_k rounds once:  e = |w_k| dzb + u |w_k| (|dz| + dzb).
A backward layer is linear in its input g with error e; the matrix cores add N
exact products in a chain of N roundings:
    e'_k = sum_j |W_kj| e_j + gamma(N) sum_j |W_kj| (|g_j| + e_j).
The mask multiplies by 0 or 1 -- the same one on both sides only where model and
kernel agree on act[l] > 0.  backward() asserts that: every hidden pre-activation
is either exact (the exact fixture: 0 masks to 0 on both sides) or farther from 0
than the forward bound on it.  No row and no element is left out.
Dense gradients: a product of two bounded factors summed over B rows, by a kernel
that may split the rows (at most B + 8 roundings per term):
    bound(act^T g) = eact^T |g| + (|act| + eact)^T eg + gamma(B + 8) (|act| + eact)^T (|g| + eg)
    bound(sum_r g) = sum_r eg + gamma(B + 8) sum_r (|g| + eg)       (db_last / dbias: float64 sums, rounded once: within it)
Updates.  theta' = theta - lr g in fp32 rounds the step's products (at most 3)
and the final addition:  |theta'~ - theta'| <= lr (bound(g) + 3 u |g|) + u |theta'| (step_bound).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_deep_eval_reference as R  # noqa: E402

U, gamma, _f64 = R.U, R.gamma, R._f64


def backward(labels, offsets, ids, vals, Wt, E, layers, bias, combiner="sum", exact_sum=False, gscale=None):
    """dict: m (the forward model's dict, T = 200), act / acte (lists, act[0] = the
    scaled bag output), margin (min |pre-activation| / bound over the hidden layers,
    inf where exact), dz, dzb, dzl / dzlb (index l = 1 .. nh, [0] unused), demb,
    dembb, grads / gradb (dense gradients and bounds in [W_0, b_0, ..., w_last, b_last, bias] order)."""
    m = R.model(labels, offsets, ids, vals, Wt, E, layers, bias, 200, combiner, exact_sum)
    y = _f64(labels).reshape(-1)
    B = y.size
    gs = float(np.float32(1.0 / B)) if gscale is None else float(np.float32(gscale))
    # ---- forward again, keeping the layers (wide_deep_eval_reference.logits's rules)
    off, ids = np.asarray(offsets, np.int64), np.asarray(ids, np.int64)
    v = np.ones(ids.size) if vals is None else _f64(vals)
    E64 = _f64(E)
    F, D = E64.shape
    ok = (ids >= 0) & (ids < F)
    ro, io, vo = np.repeat(np.arange(B), np.diff(off))[ok], ids[ok], v[ok]
    n = np.bincount(ro, minlength=B).astype(np.float64)
    a, A = np.zeros((B, D)), np.zeros((B, D))
    np.add.at(a, ro, vo[:, None] * E64[io])
    np.add.at(A, ro, np.abs(vo[:, None] * E64[io]))
    scale, f = np.ones(B), np.zeros(B)
    if combiner != "sum":
        term = vo if combiner == "mean" else vo * vo
        s = np.bincount(ro, weights=term, minlength=B)
        mx = np.maximum(s, R.FLOOR)
        nonempty = np.diff(off) > 0
        scale = np.where(nonempty, 1.0 / mx if combiner == "mean" else 1.0 / np.sqrt(mx), 1.0)
        theta = gamma(n + (combiner == "sqrtn")) * np.bincount(ro, weights=np.abs(term), minlength=B) / mx
        ds = theta / (1.0 - theta) * (1.0 + 4.0 * U) + 4.0 * U
        f = np.where(nonempty, (1.0 + ds) * (1.0 + U) - 1.0, 0.0)
    h = a * scale[:, None]
    e = np.zeros_like(h) if exact_sum else scale[:, None] * (gamma(n)[:, None] * A * (1.0 + f[:, None]) + np.abs(a) * f[:, None])
    Ws = [_f64(w) for w in layers[0::2]]
    bs = [_f64(b).reshape(-1) for b in layers[1::2]]
    nh = len(Ws) - 1
    act, acte, margin = [h], [e], np.inf
    for W, b in zip(Ws[:-1], bs[:-1]):
        K = W.shape[0]
        pre = h @ W + b
        e = np.zeros_like(pre) if exact_sum else e @ np.abs(W) + gamma(K + 1.0) * ((np.abs(h) + e) @ np.abs(W) + np.abs(b))
        if not exact_sum:                       # the masks agree: no pre-activation within its bound of 0
            assert (np.abs(pre) > e).all(), "a hidden pre-activation lies within its bound of 0: choose another seed"
            margin = min(margin, float((np.abs(pre) / e).min()))
        h = np.maximum(pre, 0.0)
        act.append(h)
        acte.append(e)
    t = h @ Ws[-1][:, 0] + bs[-1][0]
    wide = np.bincount(ro, weights=_f64(Wt).reshape(-1)[io] * vo, minlength=B)
    assert np.array_equal(wide + t + float(np.float32(bias)), m["z"])      # this forward is that module's
    # ---- backward
    d = m["p"] - y
    e1 = m["pb"] + U * (np.abs(d) + m["pb"])
    dz, dzb = d * gs, gs * e1 + U * gs * (np.abs(d) + e1)
    w = Ws[-1][:, 0]
    g = (dz[:, None] * w[None, :]) * (act[nh] > 0)
    eg = (np.abs(w)[None, :] * dzb[:, None] + U * np.abs(w)[None, :] * (np.abs(dz) + dzb)[:, None]) * (act[nh] > 0)
    dzl, dzlb = [None] * (nh + 1), [None] * (nh + 1)
    dzl[nh], dzlb[nh] = g, eg
    for l in range(nh - 1, -1, -1):
        W, N = Ws[l], Ws[l].shape[1]
        eg = eg @ np.abs(W).T + gamma(float(N)) * ((np.abs(g) + eg) @ np.abs(W).T)
        g = g @ W.T
        if l >= 1:
            g, eg = g * (act[l] > 0), eg * (act[l] > 0)
            dzl[l], dzlb[l] = g, eg
    # ---- dense gradients
    gB = gamma(B + 8.0)
    grads, gradb = [], []
    for l in range(nh + 1):
        gl, el = (dzl[l + 1], dzlb[l + 1]) if l < nh else (dz[:, None], dzb[:, None])
        x, ex = act[l], acte[l]
        grads += [x.T @ gl, gl.sum(0)]
        gradb += [ex.T @ np.abs(gl) + (np.abs(x) + ex).T @ el + gB * ((np.abs(x) + ex).T @ (np.abs(gl) + el)),
                  el.sum(0) + gB * (np.abs(gl) + el).sum(0)]
    grads.append(grads[-1].copy())
    gradb.append(gradb[-1].copy())
    return dict(m=m, act=act, acte=acte, margin=margin, dz=dz, dzb=dzb, dzl=dzl, dzlb=dzlb, demb=g, dembb=eg,
                grads=grads, gradb=gradb, gscale=gs)


def step_bound(theta_new, g, gb, lr):
    """The bound on an fp32 SGD update theta - lr g (module docstring)."""
    return lr * (gb + 3.0 * U * np.abs(g)) + U * np.abs(theta_new)


# (D, hidden, tile, B): one row; a ragged last tile at both tile sizes; one column
# chunk against eight; three hidden layers at the largest LDS footprint
EXACT_CASES = [(16, (32, 16), 16, 1), (16, (32, 16), 16, 17), (16, (32, 16), 32, 33), (64, (64,), 32, 65),
               (128, (512, 256), 16, 33), (128, (512, 512, 512), 32, 17)]
# (D, hidden, combiner, seed) at B = 33: backward() asserts the mask condition for each (the CPU test runs them)
RANDOM_CASES = [(4, (16,), "sum", 1), (128, (512, 256), "sum", 14), (128, (64, 32, 16), "sum", 17),
                (20, (48, 16), "mean", 2), (64, (64, 32), "sqrtn", 13)]
