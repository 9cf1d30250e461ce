"""float64 NumPy model of FTRL-Proximal as TensorFlow applies it (ApplyFtrl /
SparseApplyFtrl with the V2 shrinkage term): the reference of every FTRL test
(tests/test_ftrl_cpu.py, tests/test_ftrl_gpu.py).

Per element, g the gradient after duplicate summation, p = -learning_rate_power:

    g_s     = g + 2 * l2_shrinkage * var
    acc_new = acc + g * g                       (the unshrunk g)
    sigma   = (acc_new^p - acc^p) / lr
    linear += g_s - sigma * var
    quad    = acc_new^p / lr + 2 * l2
    var     = |linear| > l1 ? (sign(linear) * l1 - linear) / quad : 0
    acc     = acc_new

`mutant` swaps in one of three known wrong readings of the rule, so a test can
show that its inputs and tolerance tell them apart from the right one:
"l2" (l2 instead of 2 * l2), "shrunk_acc" (the shrunk gradient squared into
the accumulator), "ge" (>= instead of > in the threshold).
"""
import numpy as np

# the project's tolerance for the sparse rules (tests/test_sparse_optim_*.py)
VAR_TOL = dict(rtol=1e-4, atol=1e-5)
SLOT_TOL = dict(rtol=1e-4, atol=1e-6)


def hp_of(lr_power=-0.5, l1=0.0, l2=0.0, shrink=0.0, acc0=0.1):
    """TF's hyper-parameter names (what set_optimizer / optimizer_hp take)."""
    return {"learning_rate_power": lr_power, "initial_accumulator_value": acc0, "l1_regularization_strength": l1,
            "l2_regularization_strength": l2, "l2_shrinkage_regularization_strength": shrink}


def _pow(a, p):
    if p == 0.0:
        return np.ones_like(a)
    return np.sqrt(a) if p == 0.5 else np.power(a, p)


def sigma(acc, acc_new, lr, lr_power):
    p = -float(lr_power)
    return (_pow(acc_new, p) - _pow(acc, p)) / lr


def ftrl_dense(var, acc, lin, g, lr, lr_power=-0.5, l1=0.0, l2=0.0, shrink=0.0, mutant=None):
    """One step on float64 arrays; returns (var, acc, lin), the inputs are not changed."""
    var, acc, lin, g = (np.asarray(a, np.float64) for a in (var, acc, lin, g))
    p = -float(lr_power)
    gs = g + 2.0 * shrink * var
    acc_new = acc + (gs * gs if mutant == "shrunk_acc" else g * g)
    lin_new = lin + gs - sigma(acc, acc_new, lr, lr_power) * var
    quad = _pow(acc_new, p) / lr + (l2 if mutant == "l2" else 2.0 * l2)
    take = np.abs(lin_new) >= l1 if mutant == "ge" else np.abs(lin_new) > l1
    with np.errstate(divide="ignore", invalid="ignore"):
        step = (np.sign(lin_new) * l1 - lin_new) / quad
    return np.where(take, step, 0.0), acc_new, lin_new


def ftrl_rows(table, steps, lr, hp, acc=None, lin=None, mutant=None):
    """The row-sparse rule over steps = [(idx, g)]: idx [n] (-1: padding), g [n, D].
    Duplicates are summed first, every touched row is then updated once (also with
    a summed gradient of exactly 0), untouched rows keep value and slots.
    Returns (var, accum, linear)."""
    var = np.asarray(table, np.float64).copy()
    acc = np.full_like(var, hp["initial_accumulator_value"]) if acc is None else np.asarray(acc, np.float64).copy()
    lin = np.zeros_like(var) if lin is None else np.asarray(lin, np.float64).copy()
    for idx, g in steps:
        gs = np.zeros_like(var)
        keep = idx >= 0
        np.add.at(gs, idx[keep], np.asarray(g, np.float64)[keep])
        r = np.zeros(var.shape[0], bool)
        r[idx[keep]] = True
        var[r], acc[r], lin[r] = ftrl_dense(var[r], acc[r], lin[r], gs[r], lr, hp["learning_rate_power"],
                                            hp["l1_regularization_strength"], hp["l2_regularization_strength"],
                                            hp["l2_shrinkage_regularization_strength"], mutant)
    return var, acc, lin


class LRModel:
    """lr2.py's sparse logistic regression trained by FTRL, in float64: W [F] and
    the bias are FTRL variables.  An entry with value 0 or an id outside [0, F) is
    padding: it neither contributes nor marks its id as touched (the fused
    one-GPU step's contract)."""

    def __init__(self, W, lr, hp, b=0.0):
        self.W = np.asarray(W, np.float64).reshape(-1).copy()
        self.acc = np.full_like(self.W, hp["initial_accumulator_value"])
        self.lin = np.zeros_like(self.W)
        self.b = np.array([b], np.float64)
        self.bacc = np.array([hp["initial_accumulator_value"]], np.float64)
        self.blin = np.zeros(1)
        self.lr, self.hp, self.global_step = lr, hp, 0

    def step(self, labels, offsets, ids, vals=None):
        hp = self.hp
        args = (self.lr, hp["learning_rate_power"], hp["l1_regularization_strength"],
                hp["l2_regularization_strength"], hp["l2_shrinkage_regularization_strength"])
        F, B = self.W.shape[0], len(offsets) - 1
        ids = np.asarray(ids, np.int64)
        vals = np.ones(len(ids)) if vals is None else np.asarray(vals, np.float64)
        row = np.repeat(np.arange(B), np.diff(offsets))
        n = int(offsets[-1])
        ids, vals = ids[:n], vals[:n]
        live = (ids >= 0) & (ids < F) & (vals != 0.0)
        z = np.zeros(B)
        np.add.at(z, row[live], self.W[ids[live]] * vals[live])
        z += self.b[0]
        y = np.asarray(labels, np.float64).reshape(-1)
        loss = float(np.mean(np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))))
        dz = (1.0 / (1.0 + np.exp(-z)) - y) / B
        g = np.zeros(F)
        np.add.at(g, ids[live], dz[row[live]] * vals[live])
        t = np.zeros(F, bool)
        t[ids[live]] = True
        self.W[t], self.acc[t], self.lin[t] = ftrl_dense(self.W[t], self.acc[t], self.lin[t], g[t], *args)
        self.b, self.bacc, self.blin = ftrl_dense(self.b, self.bacc, self.blin, np.array([dz.sum()]), *args)
        self.global_step += 1
        return loss
