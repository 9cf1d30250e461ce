"""float64 NumPy model of DeepFM with fields (models/deepfm.py num_fields, csrc/kernels/deepfm_fields.hip) on a bag
batch (labels [B], offsets [B P + 1], ids, vals; P read off it): fm_reference.forward once over rows (offsets[::P]: S,
Q, fm, n, M) and once over bags (A_r[p], its magnitude), then deepfm_reference's tower on the concatenation.  Bounds:
deepfm_reference's `8 terms U magnitude`; terms[0] is the bag's entry count per K-wide block, behind the first layer
n_r + P K; the demb bound's S part (|dz| 8 (n_r + K) U A_r + dzb |S_r| + 4 U |dz S|) repeats per block.  settle_relu,
check_preconditions and step are deepfm_reference's own code run on this module's forward / bounds / grads (`rebind`)."""
import types

import numpy as np

import deepfm_reference as D
import fm_reference as R

U = D.U
init_state = D.init_state


def rebind(fn, **names):
    """`fn` with these module-level names replaced: its code as it stands, looked up in other globals."""
    return types.FunctionType(fn.__code__, dict(fn.__globals__, **names), fn.__name__, fn.__defaults__)


def forward(batch, w, V, b, layers, dtype=np.float64):
    labels, off, ids, vals = batch
    B, K = labels.size, V.shape[1]
    P = (off.size - 1) // B
    f = R.forward(labels, off[::P], ids, vals, w, V, b, dtype)
    g = R.forward(np.zeros(B * P), off, ids, vals, w, V, b, dtype)
    L = [np.asarray(t).astype(dtype) for t in layers]
    A = [np.abs(np.asarray(t, np.float64)) for t in layers]
    nh = len(L) // 2 - 1
    act, mag, pre = [g["S"].reshape(B, P * K)], [g["A"].reshape(B, P * K)], []
    terms = [np.repeat(g["n"].reshape(B, P), K, 1)]                 # [B, P K]; behind it [B, 1]
    for l in range(nh):
        pre.append(act[l] @ L[2 * l] + L[2 * l + 1])
        act.append(np.maximum(pre[l], 0))
        mag.append(mag[l] @ A[2 * l] + A[2 * l + 1])
        terms.append((terms[l] if l else f["n"][:, None]) + L[2 * l].shape[0])
    z = f["z"] + (act[nh] @ L[-2].reshape(-1) + L[-1][0])
    y = labels.reshape(-1).astype(dtype)
    p = 1 / (1 + np.exp(-z))
    dz = (p - y) / dtype(B)
    da = dz[:, None] * L[-2].reshape(1, -1)
    o = dict(f, z=z, p=p, dz=dz, loss=np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z))), act=act, pre=pre,
             mag=mag, terms=terms, da_nh=da, Mz=f["M"] + mag[nh] @ A[-2].reshape(-1) + A[-1][0],
             tz=terms[nh][:, 0] + L[-2].shape[0], dzl=[None] * (nh + 1))
    for l in range(nh, 0, -1):
        o["dzl"][l] = da * (act[l] > 0)
        da = o["dzl"][l] @ L[2 * l - 2].T
    o["demb"] = dz[:, None] * np.tile(f["S"], (1, P)) + da           # [B, P K] = [B P, K]
    return o


def bounds(o, layers):
    A = [np.abs(np.asarray(t, np.float64)) for t in layers]
    nh, (B, K) = len(A) // 2 - 1, o["S"].shape
    P = o["act"][0].shape[1] // K
    zb = 8 * o["tz"] * U * o["Mz"]
    pb = zb / 4 + 8 * U
    bd = dict(z=zb, loss=zb + 16 * U * (np.abs(o["z"]) + 1), p=pb, dz=pb / B,
              act=[8 * t * U * m for t, m in zip(o["terms"], o["mag"])], dzl=[None] * (nh + 1))
    E = bd["dz"][:, None] * A[-2].reshape(1, -1) + 4 * U * np.abs(o["da_nh"])
    for l in range(nh, 0, -1):
        bd["dzl"][l] = E * (o["act"][l] > 0)
        E = bd["dzl"][l] @ A[2 * l - 2].T + 8 * A[2 * l - 2].shape[1] * U * (np.abs(o["dzl"][l]) @ A[2 * l - 2].T)
    adz, aS = np.abs(o["dz"])[:, None], np.abs(o["S"])
    spart = adz * (8 * (o["n"] + K) * U)[:, None] * o["A"] + bd["dz"][:, None] * aS + 4 * U * adz * aS
    bd["demb"] = E + np.tile(spart, (1, P)) + 4 * U * np.abs(o["demb"])
    return bd


def grads(batch, w, V, b, layers, dtype=np.float64):
    """deepfm_reference.grads over bags: gw [F], gV [F, K], gb, the touched rows, and the tower's list."""
    o = forward(batch, w, V, b, layers, dtype)
    labels, off, ids, vals = batch
    K, P = V.shape[1], (off.size - 1) // labels.size
    bag = np.repeat(np.arange(off.size - 1), np.diff(off))
    ok = (ids >= 0) & (ids < w.size)
    r, j = bag[ok], ids[ok]
    x = (np.ones(ids.size) if vals is None else vals)[ok].astype(dtype)
    dzb, demb = np.repeat(o["dz"], P), o["demb"].reshape(-1, K)
    gw, q, gV = np.zeros(w.size, dtype), np.zeros(w.size, dtype), np.zeros(V.shape, dtype)
    np.add.at(gw, j, x * dzb[r])
    np.add.at(q, j, x * x * dzb[r])
    np.add.at(gV, j, x[:, None] * demb[r])
    nh, gl = len(layers) // 2 - 1, []
    for l in range(nh):
        gl += [o["act"][l].T @ o["dzl"][l + 1], o["dzl"][l + 1].sum(0)]
    gl += [o["act"][nh].T @ o["dz"][:, None], o["dz"].sum().reshape(1)]
    return gw, gV - V.astype(dtype) * q[:, None], o["dz"].sum(), np.unique(j), gl


_own = dict(forward=forward, bounds=bounds, grads=grads)
settle_relu = rebind(D.settle_relu, **_own)
check_preconditions = rebind(D.check_preconditions, **_own)
step = rebind(D.step, **_own)
