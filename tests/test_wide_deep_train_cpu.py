"""tests/wide_deep_train_reference.py on the CPU: the mask condition its bounds rest
on, for every fixture the GPU tests use, and its gradients against central
differences of the forward model's mean loss."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import wide_deep_eval_reference as R  # noqa: E402
import wide_deep_train_reference as T  # noqa: E402


@pytest.mark.parametrize("D,hidden,combiner,seed", T.RANDOM_CASES)
def test_masks_agree_on_the_random_fixtures(D, hidden, combiner, seed):
    r = T.backward(*R.random_fixture(33, D, hidden, seed)[:8], combiner)     # asserts |pre-activation| > bound itself
    print(f"mask margin {r['margin']:.3g}")
    assert r["margin"] > (4.3 if combiner == "sum" else 1.0)


@pytest.mark.parametrize("combiner", R.COMBINERS)
def test_gradients_against_central_differences(combiner):
    fx = R.random_fixture(9, 8, (16, 16), seed=5, F=50, per_row=4)
    lab, off, ids, vals, Wt, E, layers, bias = fx[:8]
    r = T.backward(*fx[:8], combiner)
    h = np.float32(2.0 ** -10)                      # an exactly representable step on fp32 inputs

    def slope(i, idx):                              # of the mean loss along element idx of tensor i (6: the table E)
        up, dn = [[a.copy() for a in layers] + [E.copy()] for _ in range(2)]
        up[i][idx] += h
        dn[i][idx] -= h
        lo, hi = (R.model(lab, off, ids, vals, Wt, t[6], t[:6], bias, 200, combiner)["mean"] for t in (dn, up))
        return (hi - lo) / (float(up[i][idx]) - float(dn[i][idx]))
    for i, idx in [(0, (3, 5)), (1, (7,)), (2, (4, 9)), (3, (2,)), (4, (6, 0)), (5, (0,))]:
        assert abs(slope(i, idx) - r["grads"][i][idx]) <= 1e-5 * (abs(r["grads"][i][idx]) + 1e-3), (i, idx)
    # demb through the table: entry j of row r moves E[id_j] by v_j scale_r demb[r] (a repeated id: summed)
    j = int(off[3])
    rows, v = np.repeat(np.arange(9), np.diff(off)), vals.astype(np.float64)
    s = np.maximum(np.bincount(rows, weights=v if combiner == "mean" else v * v, minlength=9), 1e-30)
    scale = {"sum": np.ones(9), "mean": 1 / s, "sqrtn": 1 / np.sqrt(s)}[combiner]
    sel = ids == ids[j]
    want = float((v[sel] * scale[rows[sel]] * r["demb"][rows[sel], 2]).sum())
    assert abs(slope(6, (ids[j], 2)) - want) <= 1e-5 * (abs(want) + 1e-3)
