"""What the two optimizer kernels' indexing can get wrong, pinned against a
float64 evaluation of the rules (csrc/kernels/optim_rules.h):

dense kernel (ops.hip: multi_tensor_apply) -- sizes at the 4,096-element chunk
edge and the 4-element vector tail, each tensor once 16-byte aligned and once
one element into its buffer (the scalar path), fp32 and bf16 gradients, with
and without bf16 shadows, guard elements around every stream, a voided step,
the learning rate read from the device;
row kernel (sparse_optim.hip: rows_apply) -- D = 1, 4, 6, 64 (the V = 1 and
V = 4 instantiations, more than one 256-thread block), padding rows,
untouched rows, a voided step.

sgd / momentum / nesterov run on values whose every intermediate is exactly
representable in float32 (the reference checks that itself), so fused
multiply-adds cannot matter and the result is the float64 one bit for bit.
The other kinds use the tolerances the project already has for these kernels."""
import numpy as np
import pytest
import torch

from distributed_tensorflow_example_amd import optim
from distributed_tensorflow_example_amd.optim.rules import RULES
from ftrl_reference import ftrl_dense

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8193)
DIMS = (1, 4, 6, 64)
STEPS = 3
GUARD = 8             # elements: 32 B (fp32) / 16 B (bf16), so a guarded view stays 16-byte aligned
SENTINEL = 768.0      # exact in bf16 too
LR, MU, GSCALE, WD = 0.25, 0.5, 0.5, 0.125
DENSE_TOL = dict(atol=2e-5, rtol=1e-5)      # test_ops_gpu.py: the fused optimizers against their CPU math
ROW_TOL = dict(rtol=1e-4, atol=1e-5)        # test_sparse_optim_gpu.py
FTRL = dict(learning_rate_power=-0.4, initial_accumulator_value=0.2, l1_regularization_strength=0.02,
            l2_regularization_strength=0.01, l2_shrinkage_regularization_strength=0.03)
EXACT = {   # name -> (rule, hyper-parameters, weight decay)
    "sgd": ("sgd", {}, WD),
    "momentum": ("momentum", {"momentum": MU}, WD),
    "nesterov": ("momentum", {"momentum": MU, "use_nesterov": True}, WD),
}
TOLERANCE = {
    "adagrad": ("adagrad", {"initial_accumulator_value": 0.1}, 0.0),
    "rmsprop": ("rmsprop", {"decay": 0.9, "momentum": 0.5, "epsilon": 1e-10}, 0.0),
    "adam": ("adam", {"beta1": 0.9, "beta2": 0.999, "epsilon": 1e-8}, 0.01),
    "adamw": ("adamw", {"beta1": 0.9, "beta2": 0.999, "epsilon": 1e-6}, 0.01),
    "ftrl": ("ftrl", FTRL, 0.0),
}


def make_fused(kind, ps, lr, hp, wd):
    if kind == "sgd":
        return optim.FusedSGD(ps, lr, weight_decay=wd)
    if kind == "momentum":
        return optim.FusedMomentum(ps, lr, hp["momentum"], hp.get("use_nesterov", False), weight_decay=wd)
    if kind in ("adam", "adamw"):
        cls = optim.FusedAdam if kind == "adam" else optim.FusedAdamW
        return cls(ps, lr, hp["beta1"], hp["beta2"], hp["epsilon"], weight_decay=wd)
    if kind == "adagrad":
        return optim.FusedAdagrad(ps, lr, hp["initial_accumulator_value"])
    if kind == "rmsprop":
        return optim.FusedRMSProp(ps, lr, hp["decay"], hp["momentum"], hp["epsilon"])
    return optim.FusedFtrl(ps, lr, hp["learning_rate_power"], hp["initial_accumulator_value"],
                           hp["l1_regularization_strength"], hp["l2_regularization_strength"],
                           hp["l2_shrinkage_regularization_strength"])


def rule64(kind, p, a, b, g, lr, hp, t):
    """One step of the TF rule in float64 on the scaled gradient; returns (p, a, b)."""
    if kind == "sgd":
        return p - lr * g, a, b
    if kind == "momentum":
        a = hp["momentum"] * a + g
        return p - lr * (g + hp["momentum"] * a if hp.get("use_nesterov") else a), a, b
    if kind == "adagrad":
        a = a + g * g
        return p - lr * g / np.sqrt(a), a, b
    if kind == "rmsprop":
        a = hp["decay"] * a + (1 - hp["decay"]) * g * g
        b = hp["momentum"] * b + lr * g / np.sqrt(a + hp["epsilon"])
        return p - b, a, b
    if kind == "ftrl":
        return ftrl_dense(p, a, b, g, lr, hp["learning_rate_power"], hp["l1_regularization_strength"],
                          hp["l2_regularization_strength"], hp["l2_shrinkage_regularization_strength"])
    a = hp["beta1"] * a + (1 - hp["beta1"]) * g
    b = hp["beta2"] * b + (1 - hp["beta2"]) * g * g
    lr_t = lr * np.sqrt(1 - hp["beta2"] ** t) / (1 - hp["beta1"] ** t)
    return p - lr_t * a / (np.sqrt(b) + hp["epsilon"]), a, b


def dense64(kind, p, a, b, g, lr, hp, wd, t):
    """The dense kernel's step: gradient scale and weight decay around the rule."""
    g = g * GSCALE
    if kind in ("sgd", "momentum", "adam") and wd:
        g = g + wd * p
    q, a, b = rule64(kind, p, a, b, g, lr, hp, t)
    return (q - lr * wd * p if kind == "adamw" else q), a, b


def exactly_float32(x):
    return np.array_equal(x.astype(np.float32).astype(np.float64), x)


def guarded(values, dtype, off, device="cuda"):
    """[guard | off pad | values | guard]: returns (buffer, the view of `values`)."""
    n = values.shape[0]
    buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=dtype, device=device)
    view = buf[GUARD + off: GUARD + off + n]
    view.copy_(torch.from_numpy(values).to(dtype))
    return buf, view


def guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    rest = torch.cat([buf[:lo], buf[lo + view.shape[0]:]]).float()
    return bool((rest == SENTINEL).all())


def draw(rng, n, exact, bound):
    if exact:
        return rng.integers(-bound, bound + 1, size=n).astype(np.float32)
    return (rng.standard_normal(n) * (bound / 8.0)).astype(np.float32)


@pytest.mark.parametrize("shadow", [False, True], ids=["noshadow", "shadow"])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(EXACT) + list(TOLERANCE))
def test_dense_kernel(native, name, gdt, shadow):
    exact = name in EXACT
    kind, hp, wd = (EXACT if exact else TOLERANCE)[name]
    rule = RULES[kind]
    rng = np.random.default_rng(SIZES.index(4097) + len(name))
    init = rule.slot_init(hp) + (None, None)
    shapes = [(n, off) for n in SIZES for off in (0, 1)]
    P = [guarded(draw(rng, n, exact, 64), torch.float32, off) for n, off in shapes]
    opt = make_fused(kind, [v for _, v in P], 9.0, hp, wd)
    opt.set_lr(LR)                                          # the kernel reads the device tensor, not the 9.0
    slots = []
    for v0, dst in zip(init[:2], (opt.m, opt.v)):           # the optimizer's slots, re-homed between guards
        bufs = [guarded(np.full(n, v0, np.float32), torch.float32, off) if v0 is not None else None
                for n, off in shapes]
        slots.append(bufs)
        for i, bv in enumerate(bufs):
            dst[i] = bv[1] if bv is not None else None
    S = [guarded(np.zeros(n, np.float32), torch.bfloat16, off) for n, off in shapes] if shadow else []
    for (_, p), (_, sh) in zip(P, S):
        opt.attach_shadow(p, sh)
    ref = [(p.cpu().double().numpy(), *(np.full(p.shape[0], v0, np.float64) if v0 is not None else None
                                        for v0 in init[:2])) for _, p in P]
    skip = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t in range(1, STEPS + 2):
        voided = t == STEPS + 1
        G = [guarded(draw(rng, n, exact, 8), gdt, off) for n, off in shapes]
        before = [x.clone() for x in (b for b, _ in P + S + [s for sl in slots for s in sl if s is not None])]
        skip.fill_(1 if voided else 0)
        opt.step([g for _, g in G], grad_scale=GSCALE, skip=skip)
        now = [b for b, _ in P + S + [s for sl in slots for s in sl if s is not None]]
        if voided:      # nothing changes: no parameter, slot, shadow or step count
            assert all(torch.equal(x, y) for x, y in zip(before, now))
            assert int(opt.step_t.item()) == STEPS
            break
        ref = [dense64(kind, p, a, b, g.cpu().double().numpy(), LR, hp, wd, t)
               for (p, a, b), (_, g) in zip(ref, G)]
        assert all(guards_intact(b, v) for b, v in G)
    for i, ((n, off), (p64, a64, b64)) in enumerate(zip(shapes, ref)):
        got = [P[i][1]] + [sl[i][1] for sl in slots if sl[i] is not None]
        want = [x for x in (p64, a64, b64) if x is not None]
        for g_, w_ in zip(got, want):
            if exact:
                assert exactly_float32(w_), (name, n, off)
                assert np.array_equal(g_.cpu().numpy().view(np.int32), w_.astype(np.float32).view(np.int32)), (n, off)
            else:
                np.testing.assert_allclose(g_.cpu().numpy(), w_, err_msg=f"{name} n={n} off={off}", **DENSE_TOL)
        assert guards_intact(*P[i]) and all(guards_intact(*sl[i]) for sl in slots if sl[i] is not None)
        if shadow:
            assert torch.equal(S[i][1], P[i][1].bfloat16()) and guards_intact(*S[i])


ROW_EXACT = {k: v[:2] for k, v in EXACT.items()}
ROW_TOLERANCE = {k: v[:2] for k, v in TOLERANCE.items() if RULES[v[0]].row_local}


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("name", list(ROW_EXACT) + list(ROW_TOLERANCE))
def test_row_kernel(native, name, D):
    exact = name in ROW_EXACT
    kind, hp = (ROW_EXACT if exact else ROW_TOLERANCE)[name]
    rule = RULES[kind]
    R, n = 400, 300
    rng = np.random.default_rng(D + len(name))
    t0 = draw(rng, R * D, exact, 64).reshape(R, D)
    table = torch.from_numpy(t0).cuda()
    init = rule.slot_init(hp) + (None, None)
    sa, sb = (torch.full_like(table, v0) if v0 is not None else None for v0 in init[:2])
    ref = (t0.astype(np.float64), *(np.full((R, D), v0, np.float64) if v0 is not None else None for v0 in init[:2]))
    touched = np.zeros(R, bool)
    skip = torch.zeros(1, dtype=torch.int32, device="cuda")
    state = [x for x in (table, sa, sb) if x is not None]
    for t in range(1, STEPS + 2):
        voided = t == STEPS + 1
        rows = rng.permutation(R)[:n]                       # distinct, as the owner makes them
        rows[rng.random(n) < 0.15] = -1                     # exchange padding
        g = draw(rng, n * D, exact, 8).reshape(n, D)
        before = [x.clone() for x in state]
        skip.fill_(1 if voided else 0)
        native.sparse_rows_apply(table, sa, sb, torch.from_numpy(rows).cuda(), torch.from_numpy(g).cuda(),
                                 rule.kind, LR, skip=skip, **rule.native_kwargs(hp))
        if voided:
            assert all(torch.equal(x, y) for x, y in zip(before, state))
            break
        r = rows[rows >= 0]
        touched[r] = True
        new = rule64(kind, *(x[r] if x is not None else None for x in ref), g[rows >= 0].astype(np.float64), LR, hp, t)
        for x, y in zip(ref, new):
            if x is not None:
                x[r] = y
        quiet = torch.from_numpy(np.setdiff1d(np.arange(R), r)).cuda()     # rows this step left alone, slots too
        assert all(torch.equal(x[quiet], y[quiet]) for x, y in zip(before, state))
    assert touched.any() and not touched.all()
    for got, want in zip(state, (x for x in ref if x is not None)):
        if exact:
            assert exactly_float32(want)
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.astype(np.float32).view(np.int32))
        else:
            np.testing.assert_allclose(got.cpu().numpy(), want, err_msg=f"{name} D={D}", **ROW_TOL)
