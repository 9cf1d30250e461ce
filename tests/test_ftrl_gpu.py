"""FTRL-Proximal on the GPU against the float64 model (tests/ftrl_reference.py):
the row-sparse kernel (csrc/kernels/sparse_optim.hip kind 6), the dense
multi-tensor kernel (csrc/kernels/ops.hip kind 6) and the fused one-GPU
sparse-LR step (csrc/kernels/sparse_lr.hip: slr_ftrl_gsum / _rule / _clear).
Tolerance: the project's own for the sparse rules (VAR_TOL / SLOT_TOL)."""
import numpy as np
import pytest
import torch

from ftrl_reference import SLOT_TOL, VAR_TOL, LRModel, ftrl_dense, ftrl_rows, hp_of
from test_ftrl_cpu import (HP, LR, POWERS, REGS, check_table, compare_zero_sets, exact_zero_case, run_ftrl_table)
from test_sparse_optim_cpu import make_steps

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- row-sparse kernel
# Two cases miss the stock atol of 1e-6 on `linear` on the GPU, by one element of
# 80,000 each (1.28e-6 off where |linear| = 1.4e-3): sigma = (acc'^0.3 - acc^0.3) /
# lr is a difference of two powf results times 1 / lr = 20.  Their bound follows
# the project's rule for such a case: the float32 CPU twin (_rows_apply_torch)
# against the float64 model on the same inputs needs the atol below (max of
# |twin - model| - rtol |model| at the stock rtol of 1e-4), and the GPU is
# allowed twice that -- float atomics' arrival order, powf versus NumPy's pow.
TWIN_LINEAR_ATOL = {(16, -0.3, (0.0, 0.0, 0.0)): 9.32e-7,       # measured; GPU bound 1.864e-6
                    (16, -0.3, (0.05, 0.01, 0.0)): 9.32e-7}     # measured; GPU bound 1.864e-6


@pytest.mark.parametrize("reg", REGS)
@pytest.mark.parametrize("lr_power", POWERS)
@pytest.mark.parametrize("D", [1, 6, 16])           # scalar and 4-wide column paths
def test_row_kernel_matches_model(native, D, lr_power, reg):
    rows = 5000
    hp = hp_of(lr_power, *reg)
    steps = make_steps(rows, D, 2048, 4, seed=D)
    t, t0 = run_ftrl_table(rows, D, steps, LR, hp, device="cuda")
    twin = TWIN_LINEAR_ATOL.get((D, lr_power, reg))
    check_table(t, ftrl_rows(t0, steps, LR, hp), lin_atol=None if twin is None else 2.0 * twin)


def test_row_kernel_voided_step(native):
    rows, D = 3000, 4
    steps = make_steps(rows, D, 512, 3, seed=5)
    t, t0 = run_ftrl_table(rows, D, steps, LR, HP["ftrl"], device="cuda", void_step=1)
    check_table(t, ftrl_rows(t0, [steps[0], steps[2]], LR, HP["ftrl"]))


def test_row_kernel_refusals(native):
    table, slot = torch.zeros(10, 4, device="cuda"), torch.full((10, 4), 0.1, device="cuda")
    rows = torch.zeros(3, dtype=torch.int64, device="cuda")
    g = torch.zeros(3, 4, device="cuda")
    for a, b in ((None, None), (slot, None), (None, slot)):      # FTRL needs accum and linear
        with pytest.raises(RuntimeError):
            native.sparse_rows_apply(table, a, b, rows, g, 6, 0.1)
    with pytest.raises(RuntimeError):                             # g's D != the table's
        native.sparse_rows_apply(table, slot, slot.clone(), rows, torch.zeros(3, 5, device="cuda"), 6, 0.1)
    with pytest.raises(RuntimeError):                             # learning_rate_power > 0
        native.sparse_rows_apply(table, slot, slot.clone(), rows, g, 6, 0.1, lr_power=0.5)
    assert float(table.abs().max()) == 0.0 and torch.equal(slot, torch.full((10, 4), 0.1, device="cuda"))


@pytest.mark.parametrize("seed", [21, 22])
def test_row_kernel_exact_zeros_match_model(native, seed):
    hp, steps = exact_zero_case(seed, rows=5000, D=4, n=2048)
    t, t0 = run_ftrl_table(5000, 4, steps, LR, hp, device="cuda")
    compare_zero_sets(t.local.cpu().numpy(), ftrl_rows(t0, steps, LR, hp), hp["l1_regularization_strength"])


def test_row_kernel_zero_branch_is_a_select(native):
    """acc == 0, g == 0, l2 == 0: the untaken division is 0 / 0; var must be 0.0."""
    from distributed_tensorflow_example_amd.parallel.sharded_embedding import ShardedEmbedding
    from distributed_tensorflow_example_amd.parallel.world import World

    for D in (1, 4):
        t = ShardedEmbedding(10, D, World(device="cuda"), seed=1, device="cuda")
        t.set_optimizer("ftrl", **hp_of(-0.5, 0.0, 0.0, 0.0, acc0=0.0))
        t._apply_local(torch.tensor([2, 5], device="cuda"), torch.zeros(2, D, device="cuda"), 0.1, 1.0, None)
        loc = t.local.cpu()
        assert torch.isfinite(loc).all() and float(loc[2].abs().max()) == 0.0 and float(loc[5].abs().max()) == 0.0


# ---------------------------------------------------------------- dense multi-tensor kernel
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_dense_kernel_matches_model(native, gdt):
    """Three tensors of 1, 4097 and 10,000 elements: the 4096-element chunk edge."""
    from distributed_tensorflow_example_amd import optim

    rng = np.random.default_rng(8)
    sizes = [1, 4097, 10_000]
    p0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    ps = [torch.from_numpy(p).cuda() for p in p0]
    hp = dict(learning_rate_power=-0.4, initial_accumulator_value=0.2, l1=0.02, l2=0.01, l2_shrinkage=0.03)
    opt = optim.FusedFtrl(ps, 0.1, **hp)
    model = [(p.astype(np.float64), np.full(p.shape, 0.2), np.zeros(p.shape)) for p in p0]
    skip = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k in range(5):
        gs = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(gdt) for n in sizes]
        scale = 0.5 if k % 2 else 1.0
        skip.fill_(1 if k == 2 else 0)                    # a voided step: nothing changes
        opt.step([g.cuda() for g in gs], grad_scale=scale, skip=skip)
        if k != 2:
            model = [ftrl_dense(v, a, l, g.double().numpy() * scale, 0.1, -0.4, 0.02, 0.01, 0.03)
                     for (v, a, l), g in zip(model, gs)]
    assert int(opt.step_t.item()) == 4
    for i, p in enumerate(ps):
        np.testing.assert_allclose(p.cpu().numpy(), model[i][0], **VAR_TOL)
        np.testing.assert_allclose(opt.m[i].cpu().numpy(), model[i][1], **SLOT_TOL)
        np.testing.assert_allclose(opt.v[i].cpu().numpy(), model[i][2], **SLOT_TOL)


# ---------------------------------------------------------------- fused one-GPU sparse-LR step
F = 10_007
LR_HP = hp_of(-0.5, 0.002, 0.01, 0.0)


def _world():
    from distributed_tensorflow_example_amd.parallel import world as W

    return W.get_world() if W._WORLD is not None else W.init()


def _edge_batches(nsteps, with_vals, seed=0, bad_in_step=0):
    """B = 33: the second 32-row workgroup holds one row.  Id 77 twice inside
    row 3 and again in row 32 (both workgroups), id 500 in rows 0 and 32, row 5
    empty, one id outside [0, F) in row 7 of one step."""
    rng = np.random.default_rng(seed)
    B = 33
    out = []
    for s in range(nsteps):
        rows = []
        for r in range(B):
            ids = list(rng.integers(0, F, int(rng.integers(1, 12))))
            if r == 3:
                ids += [77, 77]
            if r == 0:
                ids += [500]
            if r == 32:
                ids += [77, 500]
            if r == 5:
                ids = []
            if r == 7 and s == bad_in_step:
                ids += [F + 5]
            rows.append(ids)
        offs = np.zeros(B + 1, np.int64)
        np.cumsum([len(i) for i in rows], out=offs[1:])
        ids = np.array([i for r in rows for i in r], np.int64)
        vals = (rng.random(len(ids)) * 0.9 + 0.1).astype(np.float32) if with_vals else None
        out.append(((rng.random((B, 1)) < 0.4).astype(np.float32), offs, ids, vals))
    return out


def _overflow_batches(nsteps, seed=1):
    """B = 32, 200 distinct ids per row, neighbouring rows share 50: 4850
    distinct ids in one workgroup, more than its 4096-slot LDS table, so the
    straight-to-memory path runs (and ids from it meet in the election)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nsteps):
        perm = rng.permutation(F)
        ids = np.concatenate([perm[(r * 150 + np.arange(200)) % 7000] for r in range(32)]).astype(np.int64)
        offs = np.arange(0, 32 * 200 + 1, 200, dtype=np.int64)
        out.append(((rng.random((32, 1)) < 0.4).astype(np.float32), offs, ids,
                    (rng.random(len(ids)) * 0.9 + 0.1).astype(np.float32)))
    return out


def _to_dev(batch):
    return tuple(None if a is None else torch.from_numpy(a).cuda() for a in batch)


def _trainer(lr=0.3, **kw):
    from distributed_tensorflow_example_amd.models.sparse_lr import SparseLRTrainer

    return SparseLRTrainer(F, lr, _world(), seed=3, optimizer="ftrl", optimizer_hp=LR_HP, **kw)


def _check_against_model(tr, m):
    np.testing.assert_allclose(tr.W.local.cpu().numpy().reshape(-1), m.W, **VAR_TOL)
    np.testing.assert_allclose(tr.W.slots["Ftrl"].cpu().numpy().reshape(-1), m.acc, **SLOT_TOL)
    np.testing.assert_allclose(tr.W.slots["Ftrl_1"].cpu().numpy().reshape(-1), m.lin, **SLOT_TOL)
    np.testing.assert_allclose(tr.b.detach().cpu().numpy(), m.b, **VAR_TOL)
    np.testing.assert_allclose(tr.b_slots.cpu().numpy(), [m.bacc[0], m.blin[0]], **SLOT_TOL)


def _accumulator_clean(tr):
    """All 0.0 bits: no gradient and no NaN claim left behind."""
    g = tr._plan.grad_accumulator()
    return int(g.view(torch.int32).ne(0).sum().item()) == 0


@pytest.mark.parametrize("with_vals", [True, False])
@pytest.mark.parametrize("entry", ["step", "run_csr"])      # device int64 ids | host feed, int32 ids (F < 2^31)
def test_fused_step_matches_model(native, entry, with_vals):
    tr = _trainer()
    assert tr._fused_ok()
    m = LRModel(tr.W.local.cpu().numpy(), 0.3, LR_HP)
    for k, bt in enumerate(_edge_batches(5, with_vals)):
        loss = float(tr.train_step(_to_dev(bt) if entry == "step" else bt))
        assert abs(loss - m.step(*bt)) < 1e-5, k
        assert _accumulator_clean(tr), k
    assert tr._plan.ftrl() and tr._plan.runs() == 5
    assert tr._plan.bad_ids() == 1                          # the one id outside [0, F): counted, nothing touched
    assert tr.global_step == m.global_step == 5
    _check_against_model(tr, m)
    if with_vals:
        assert int((tr.W.local == 0.0).sum()) > 0           # l1 > 0: exact zeros among the touched rows


@pytest.mark.parametrize("entry", ["step", "run_csr"])
def test_fused_step_lds_table_overflow(native, entry):
    tr = _trainer()
    m = LRModel(tr.W.local.cpu().numpy(), 0.3, LR_HP)
    for k, bt in enumerate(_overflow_batches(3)):
        loss = float(tr.train_step(_to_dev(bt) if entry == "step" else bt))
        assert abs(loss - m.step(*bt)) < 1e-5, k
        assert _accumulator_clean(tr), k
    assert tr._plan.bad_ids() == 0
    _check_against_model(tr, m)


def test_fused_step_counts_the_graph_global_step(native):
    """The plan's own global_step variable (the lowered Session's) is counted by
    the workgroup that updates the bias, as in the SGD step."""
    W = torch.randn(F, 1, device="cuda")
    b = torch.zeros(1, device="cuda")
    gs = torch.zeros((), dtype=torch.int64, device="cuda")
    plan = native.SparseLRPlan(W, b, gs)
    acc, lin = torch.full_like(W, 0.1), torch.zeros_like(W)
    plan.set_ftrl(acc, lin, torch.tensor([0.1, 0.0], device="cuda"), l1=0.002, l2=0.01)
    lab, offs, ids, vals = _to_dev(_edge_batches(1, True, bad_in_step=-1)[0])
    for _ in range(3):
        plan.step(lab.reshape(-1), offs, ids, vals, 0.3)
    assert int(gs.item()) == 3


def test_fused_step_replays_in_a_graph(native):
    """The four kernels captured in one hipGraph (utils/graphs.GraphedStep, what
    enable_graph uses): two replays train like two eager steps, and the
    accumulator's clear is replayed with them."""
    from distributed_tensorflow_example_amd.utils.graphs import GraphedStep

    bt = _to_dev(_edge_batches(1, True, bad_in_step=-1)[0])
    eager, graphed = _trainer(), _trainer()
    graphed.enable_graph()
    assert graphed._fused_ok()
    graphed.train_step(bt)                                   # builds the plan (same first step on both)
    eager.train_step(bt)
    g = GraphedStep(lambda *b: graphed._train_step_fused(b),
                    lambda: graphed.W.state_tensors() + [graphed.b.data, graphed.b_slots])
    for k in range(2):
        le, lg = float(eager.train_step(bt)), float(g(*bt))
        assert abs(le - lg) < 1e-5, k
        assert _accumulator_clean(graphed), k
    assert g.captures == 1 and g.replays == 2
    for a, b, tol in ((eager.W.local, graphed.W.local, VAR_TOL), (eager.b.data, graphed.b.data, VAR_TOL),
                      (eager.W.slots["Ftrl"], graphed.W.slots["Ftrl"], SLOT_TOL),
                      (eager.W.slots["Ftrl_1"], graphed.W.slots["Ftrl_1"], SLOT_TOL),
                      (eager.b_slots, graphed.b_slots, SLOT_TOL)):
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), **tol)


def test_fused_step_matches_general_path(native, monkeypatch):
    """DTF_SLR_FUSED=0 in the same process: the sharded path (dedup, bag backward,
    rows_apply kind 6, the dense kernel on the bias) trains like the fused step."""
    batches = [_to_dev(b) for b in _edge_batches(5, True, seed=4, bad_in_step=-1)]
    monkeypatch.setenv("DTF_SLR_FUSED", "0")
    general = _trainer()
    assert not general._fused_ok()
    monkeypatch.setenv("DTF_SLR_FUSED", "1")
    fused = _trainer()
    assert fused._fused_ok()
    for k, bt in enumerate(batches):
        lg, lf = float(general.train_step(bt)), float(fused.train_step(bt))
        assert abs(lg - lf) < 1e-5, k
    assert fused.global_step == general.global_step == 5
    for a, b, tol in ((general.W.local, fused.W.local, VAR_TOL), (general.b.data, fused.b.data, VAR_TOL),
                      (general.W.slots["Ftrl"], fused.W.slots["Ftrl"], SLOT_TOL),
                      (general.W.slots["Ftrl_1"], fused.W.slots["Ftrl_1"], SLOT_TOL),
                      (general.b_slots, fused.b_slots, SLOT_TOL)):
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), **tol)


def test_default_optimizer_keeps_the_sgd_plan(native):
    """optimizer="sgd" (the default): the plan is built and called as before,
    and no slot tensor exists anywhere."""
    from distributed_tensorflow_example_amd.models.sparse_lr import SparseLRTrainer

    tr = SparseLRTrainer(F, 0.3, _world(), seed=3)
    assert tr.optimizer == "sgd" and tr.W.slots == {} and tr.b_slots is None and tr._bopt is None
    assert tr.W._gacc is None
    w0 = tr.W.local.clone()
    tr.train_step(_to_dev(_edge_batches(1, True, bad_in_step=-1)[0]))
    assert type(tr._plan).__name__ == "SparseLRPlan" and not tr._plan.ftrl()
    with pytest.raises(RuntimeError):
        tr._plan.grad_accumulator()
    assert tr.W.slots == {} and not torch.equal(tr.W.local, w0)
