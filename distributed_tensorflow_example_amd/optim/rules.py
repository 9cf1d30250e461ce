"""The optimizer rules, once, for every Python consumer (the C++ twin is
csrc/kernels/optim_rules.h): RULES[name] holds a kind's number, its TF slot
names and their initial values, its hyper-parameters under TF's names with TF's
defaults, the keyword arguments the kernels take, and the in-place float32
torch rule that the CPU paths run.

The formulas are TensorFlow's (GradientDescent, Momentum, Adam with epsilon
outside the sqrt, Adagrad, RMSProp, ApplyFtrlV2) and are written out once, next
to their kernel form, in the header; adamw shares adam's rule, its decoupled
decay is the caller's.

`fast_rsqrt` is the one difference between the dense path (False: x / sqrt(a))
and the row path of a sharded table (True: x * rsqrt(a)), as in the header."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, Tuple, Union

import torch

# TF's hyper-parameter name -> the kernels' keyword (csrc/bind_ops.cpp: optim_hyper)
_NATIVE = {"momentum": "momentum", "use_nesterov": "nesterov", "beta1": "beta1", "beta2": "beta2", "decay": "decay",
           "epsilon": "eps", "learning_rate_power": "lr_power", "l1_regularization_strength": "l1",
           "l2_regularization_strength": "l2", "l2_shrinkage_regularization_strength": "l2_shrinkage"}


def _over_sqrt(x, a, fast_rsqrt):
    return x * torch.rsqrt(a) if fast_rsqrt else x / a.sqrt()


def _sgd(var, a, b, g, lr, h, fast_rsqrt, t):
    var.sub_(lr * g)


def _momentum(var, a, b, g, lr, h, fast_rsqrt, t):
    mu = h["momentum"]
    a.mul_(mu).add_(g)
    var.sub_(lr * (g + mu * a if h["use_nesterov"] else a))


def _adam(var, a, b, g, lr, h, fast_rsqrt, t):
    b1, b2 = h["beta1"], h["beta2"]
    a.mul_(b1).add_((1 - b1) * g)
    b.mul_(b2).add_((1 - b2) * g * g)
    lr_t = lr * (1 - b2 ** t) ** 0.5 / (1 - b1 ** t)
    var.sub_(lr_t * a / (b.sqrt() + h["epsilon"]))


def _adagrad(var, a, b, g, lr, h, fast_rsqrt, t):
    a.add_(g * g)
    var.sub_(_over_sqrt(lr * g, a, fast_rsqrt))


def _rmsprop(var, a, b, g, lr, h, fast_rsqrt, t):
    rho = h["decay"]
    a.mul_(rho).add_((1 - rho) * g * g)
    b.mul_(h["momentum"]).add_(_over_sqrt(lr * g, a + h["epsilon"], fast_rsqrt))
    var.sub_(b)


def _ftrl(var, acc, lin, g, lr, h, fast_rsqrt, t):
    """Same operation order as ftrl_update in the header; g: the duplicate-summed, unshrunk gradient."""
    p, l1 = -h["learning_rate_power"], h["l1_regularization_strength"]
    l2, shrink = h["l2_regularization_strength"], h["l2_shrinkage_regularization_strength"]
    pw = (lambda x: x.sqrt()) if p == 0.5 else ((lambda x: torch.ones_like(x)) if p == 0.0 else (lambda x: x.pow(p)))
    gs = g + 2.0 * shrink * var if shrink != 0.0 else g
    an = acc + g * g
    pn = pw(an)
    sigma = (pn - pw(acc)) / lr
    l = lin + gs - sigma * var
    quad = pn / lr + 2.0 * l2
    step = (torch.sign(l) * l1 - l) / quad
    var.copy_(torch.where(l.abs() > l1, step, torch.zeros_like(step)))   # a select: the untaken 0 / 0 never lands
    acc.copy_(an)
    lin.copy_(l)


@dataclass(frozen=True)
class Rule:
    name: str
    kind: int                                   # the kernels' number (optim_rules.h: OptimKind)
    slots: Tuple[str, ...]                      # TF's slot names: slot a, slot b
    init: Tuple[Union[float, str], ...]         # each slot's initial value: a number, or the hyper-parameter holding it
    defaults: Dict[str, float]                  # hyper-parameters, TF's names and defaults
    update: Callable
    row_local: bool = True                      # updates only the rows a gradient touches (all but Adam)
    sparse: bool = True                         # TF has a sparse apply for it: a sharded table can use it
    nonneg: Tuple[str, ...] = ()                # the constructor checks TF makes
    nonpos: Tuple[str, ...] = ()

    def hp(self, given: dict) -> dict:
        """`given` over the defaults, as floats (use_nesterov: bool), checked as TF's constructor checks them."""
        h = {k: type(d)(given.get(k, d)) for k, d in self.defaults.items()}
        for k in self.nonneg:
            if h[k] < 0.0:
                raise ValueError(f"{k} {h[k]} needs to be positive or zero")
        for k in self.nonpos:
            if h[k] > 0.0:
                raise ValueError(f"{k} {h[k]} needs to be negative or zero")
        return h

    def slot_init(self, given: dict) -> Tuple[float, ...]:
        h = self.hp(given)
        return tuple(h[v] if isinstance(v, str) else v for v in self.init)

    def native_kwargs(self, given: dict) -> dict:
        """The hyper-parameter keywords of multi_tensor_apply / sparse_rows_apply (and SparseLRPlan.set_ftrl)."""
        return {_NATIVE[k]: v for k, v in self.hp(given).items() if k in _NATIVE}

    def update_(self, var, a, b, g, lr, given, fast_rsqrt, t=None):
        """The rule in place on float32 tensors: a, b = the slots (None where the
        kind has none), g already scaled, t = Adam's step count."""
        self.update(var, a, b, g, lr, self.hp(given), fast_rsqrt, t)


_ADAM = {"beta1": 0.9, "beta2": 0.999, "epsilon": 1e-8}
_FTRL = {"learning_rate_power": -0.5, "initial_accumulator_value": 0.1, "l1_regularization_strength": 0.0,
         "l2_regularization_strength": 0.0, "l2_shrinkage_regularization_strength": 0.0}
RULES = {r.name: r for r in (
    Rule("sgd", 0, (), (), {}, _sgd),
    Rule("momentum", 1, ("Momentum",), (0.0,), {"momentum": 0.0, "use_nesterov": False}, _momentum),
    Rule("adam", 2, ("Adam", "Adam_1"), (0.0, 0.0), _ADAM, _adam, row_local=False),
    Rule("adamw", 3, ("Adam", "Adam_1"), (0.0, 0.0), _ADAM, _adam, row_local=False, sparse=False),
    Rule("adagrad", 4, ("Adagrad",), ("initial_accumulator_value",), {"initial_accumulator_value": 0.1}, _adagrad),
    Rule("rmsprop", 5, ("RMSProp", "Momentum"), (1.0, 0.0), {"decay": 0.9, "momentum": 0.0, "epsilon": 1e-10},
         _rmsprop),
    Rule("ftrl", 6, ("Ftrl", "Ftrl_1"), ("initial_accumulator_value", 0.0), _FTRL, _ftrl,
         nonneg=tuple(k for k in _FTRL if k != "learning_rate_power"), nonpos=("learning_rate_power",)),
)}
KINDS = {name: r.kind for name, r in RULES.items()}
