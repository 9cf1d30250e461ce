"""optim/rules.py is the one Python owner of the optimizer rules: every consumer
creates the slots the table names, with the values it gives, and both CPU
update paths (the dense fused step and the row step of a sharded table) keep
the bits they had before the rules were shared (tests/golden/optim_rules_cpu.npz,
written by scripts/dump_optim_states.py --golden at the commit before)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from distributed_tensorflow_example_amd import optim
from distributed_tensorflow_example_amd.compat import train
from distributed_tensorflow_example_amd.compat.partitioned import PartitionedSlot
from distributed_tensorflow_example_amd.optim.rules import KINDS, RULES
from distributed_tensorflow_example_amd.parallel.sharded_embedding import ShardedEmbedding
from distributed_tensorflow_example_amd.parallel.world import World

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_rules_cpu.npz")
ACC0 = 0.3      # not the default: the initial value must come from the hyper-parameter
SLOTS = {"sgd": (), "momentum": ("Momentum",), "adam": ("Adam", "Adam_1"), "adamw": ("Adam", "Adam_1"),
         "adagrad": ("Adagrad",), "rmsprop": ("RMSProp", "Momentum"), "ftrl": ("Ftrl", "Ftrl_1")}
INIT = {"sgd": (), "momentum": (0.0,), "adam": (0.0, 0.0), "adamw": (0.0, 0.0), "adagrad": (ACC0,),
        "rmsprop": (1.0, 0.0), "ftrl": (ACC0, 0.0)}
HP = {"adagrad": {"initial_accumulator_value": ACC0}, "ftrl": {"initial_accumulator_value": ACC0}}
FUSED = {"sgd": lambda p: optim.FusedSGD(p, 0.1), "momentum": lambda p: optim.FusedMomentum(p, 0.1),
         "adam": lambda p: optim.FusedAdam(p), "adamw": lambda p: optim.FusedAdamW(p),
         "adagrad": lambda p: optim.FusedAdagrad(p, 0.1, ACC0), "rmsprop": lambda p: optim.FusedRMSProp(p, 0.1),
         "ftrl": lambda p: optim.FusedFtrl(p, 0.1, initial_accumulator_value=ACC0)}
COMPAT = {"sgd": lambda: train.GradientDescentOptimizer(0.1), "momentum": lambda: train.MomentumOptimizer(0.1, 0.9),
          "adam": lambda: train.AdamOptimizer(), "adagrad": lambda: train.AdagradOptimizer(0.1, ACC0),
          "rmsprop": lambda: train.RMSPropOptimizer(0.1),
          "ftrl": lambda: train.FtrlOptimizer(0.1, initial_accumulator_value=ACC0)}


def test_table_numbers_slots_and_initial_values():
    assert KINDS == {"sgd": 0, "momentum": 1, "adam": 2, "adamw": 3, "adagrad": 4, "rmsprop": 5, "ftrl": 6}
    assert optim.KINDS is KINDS
    for kind, rule in RULES.items():
        assert rule.kind == KINDS[kind] and rule.slots == SLOTS[kind]
        assert rule.slot_init(HP.get(kind, {})) == INIT[kind]
        assert rule.row_local == (kind not in ("adam", "adamw"))


@pytest.mark.parametrize("kind", list(RULES))
def test_fused_optimizer_slots(kind):
    opt = FUSED[kind]([torch.zeros(5), torch.zeros(2, 3)])
    assert opt.rule is RULES[kind]
    for slot, v0 in zip((opt.m, opt.v), INIT[kind] + (None, None)):
        for p, t in zip(opt.params, slot):
            assert (t is None) if v0 is None else torch.equal(t, torch.full_like(p, v0))


@pytest.mark.parametrize("kind", [k for k, r in RULES.items() if r.sparse])
def test_sharded_table_compat_and_partitioned_slots(kind):
    t = ShardedEmbedding(12, 3, World(device="cpu"), seed=1)
    t.set_optimizer(kind, **HP.get(kind, {}))
    assert tuple(t.slots) == SLOTS[kind]
    pv = SimpleNamespace(name="w:0", shape=(12, 3), rows=12, dim=3, partitioner=None, world=None, placement=None,
                         table=t)
    for name, v0 in zip(SLOTS[kind], INIT[kind]):
        assert torch.equal(t.slots[name], torch.full_like(t.local, v0))
        assert PartitionedSlot(pv, name).init == v0
    o = COMPAT[kind]()
    assert tuple(o.get_slot_names()) == SLOTS[kind]
    assert tuple(o._slot_init(n) for n in o.get_slot_names()) == INIT[kind]


def test_adamw_has_no_sparse_rule():
    with pytest.raises(ValueError):
        ShardedEmbedding(12, 3, World(device="cpu"), seed=1).set_optimizer("adamw")


# ---------------------------------------------------------------- both CPU paths keep their bits
LR, MU = 0.05, 0.9
_FTRL_HP = dict(learning_rate_power=-0.4, initial_accumulator_value=0.2, l1_regularization_strength=0.02,
                l2_regularization_strength=0.01, l2_shrinkage_regularization_strength=0.03)
CASES = {   # fixture key -> (fused optimizer, set_optimizer kind, hyper-parameters)
    "momentum": (lambda p: optim.FusedMomentum(p, LR, MU, False), "momentum", {"momentum": MU}),
    "nesterov": (lambda p: optim.FusedMomentum(p, LR, MU, True), "momentum", {"momentum": MU, "use_nesterov": True}),
    "adagrad": (lambda p: optim.FusedAdagrad(p, LR, 0.1), "adagrad", {"initial_accumulator_value": 0.1}),
    "rmsprop": (lambda p: optim.FusedRMSProp(p, LR, 0.9, 0.5, 1e-10), "rmsprop",
                {"decay": 0.9, "momentum": 0.5, "epsilon": 1e-10}),
    "ftrl": (lambda p: optim.FusedFtrl(p, LR, -0.4, 0.2, 0.02, 0.01, 0.03), "ftrl", _FTRL_HP),
    "ftrl_sqrt": (lambda p: optim.FusedFtrl(p, LR), "ftrl", {}),
}


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_paths_keep_their_bits(golden, name):
    """Three steps on the same values: the dense step, and the row step with rows = arange(n)."""
    make, kind, hp = CASES[name]
    p0, gs = golden["p0"], golden["g"]
    n = p0.shape[0]
    p = torch.from_numpy(p0.copy())
    opt = make([p])
    t = ShardedEmbedding(n, p0.shape[1], World(device="cpu"), seed=1)
    t.local.copy_(torch.from_numpy(p0))
    t.set_optimizer(kind, **hp)
    for g in gs:
        opt.step([torch.from_numpy(g.copy())])
        t._apply_local(torch.arange(n), torch.from_numpy(g.copy()), LR, 1.0, None)
    dense = np.stack([x.numpy() for x in (p, opt.m[0], opt.v[0]) if x is not None])
    rows = np.stack([t.local.numpy()] + [s.numpy() for s in t.slots.values()])
    assert dense.tobytes() == golden[f"{name}_dense"].tobytes()
    assert rows.tobytes() == golden[f"{name}_rows"].tobytes()
    if kind in ("adagrad", "rmsprop"):      # x / sqrt(a) and x * rsqrt(a) are not the same float32 arithmetic
        assert dense.tobytes() != rows.tobytes()
