"""tests/attention_reference.py on the CPU, before it judges a kernel
(tests/test_attention_edges_gpu.py): the float64 model against float64 autograd,
the dropout hash against a scalar transcription, the derived bounds against the
fp32 / bf16 emulation of the kernels for every GPU case (they hold, and the fp32
share stays below a quarter at the median element), mutants of the emulation
(they fall outside), and the conditions a case needs to say anything."""
import pytest
import torch

import attention_reference as R


def _case(name):
    return R.CASES[R.CASE_IDS.index(name)]


# ---- the model against autograd ---------------------------------------------------------------

def _close(a, b, what):
    err = float((a - b).abs().max())
    assert err <= 1e-10 * max(1e-30, float(b.abs().max())), (what, err)


@pytest.mark.parametrize("p,seed", [(0.0, 0), (0.3, R.SEEDS["h32"]), (0.3, R.SEEDS["h64"])])
@pytest.mark.parametrize("has_mask", [True, False])
@pytest.mark.parametrize("has_bias", [True, False])
def test_model_matches_float64_autograd(has_bias, has_mask, p, seed):
    B, NH, S, scale = 2, 2, 32, 0.125
    H3 = 3 * NH * R.HD
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(B, S, H3, generator=g) * 2).bfloat16()
    bias = torch.randn(H3, generator=g) * 0.5 if has_bias else None
    mask = R.graded_mask(B, S) if has_mask else None
    dO = torch.randn(B, S, NH * R.HD, generator=g).bfloat16()
    keep = R.keep_mask(seed, p, B, NH, S) if p > 0 else None
    m = R.model(qkv, bias, mask, dO, NH, scale, keep)

    x = R.operands(qkv, bias).double().requires_grad_()
    q, k, v = R.heads(x, NH, 3)
    z = scale * torch.matmul(q, k.transpose(-1, -2))
    if has_mask:
        z = z + mask.double()[:, None, None, :]
    pr = torch.softmax(z, -1)
    if keep is not None:
        pr = pr * keep
    out = torch.matmul(pr, v)                                   # [B, NH, S, 64]
    out.backward(R.heads(dO.double(), NH, 1)[0])
    dq, dk, dv = R.split_dqkv(x.grad, NH)
    _close(m["O"], out.detach(), "O")
    _close(m["lse"], torch.logsumexp(z.detach(), -1), "lse")
    _close(m["dQ"], dq, "dQ")
    _close(m["dK"], dk, "dK")
    _close(m["dV"], dv, "dV")
    _close(m["dbias"], x.grad.sum((0, 1)), "dbias")
    _close(m["D"], (R.heads(dO.double(), NH, 1)[0] * out.detach()).sum(-1), "D")
    if has_bias:
        # the operand is ONE bf16 rounding of the fp32 sum
        want = (qkv.float() + bias).bfloat16()
        assert torch.equal(R.operands(qkv, bias).bfloat16(), want)
        assert torch.equal(R.operands(qkv, bias), want.float())
    else:
        assert torch.equal(R.operands(qkv, None), qkv.float())


# ---- the dropout bits -------------------------------------------------------------------------

def _hash32_scalar(seed, i):
    """common.h hash32 on Python ints, masked by hand."""
    M32, M64 = (1 << 32) - 1, (1 << 64) - 1
    seed &= M64
    if seed >> 63:
        k = (seed & M32) ^ (((seed >> 32) * 0x85EBCA6B) & M32)
        x = (((i & M32) ^ k) + (i >> 32) * 0x9E3779B9) & M32
        x ^= x >> 16
        x = (x * 0x7FEB352D) & M32
        x ^= x >> 15
        x = (x * 0x846CA68B) & M32
        x ^= x >> 16
        return x
    x = seed ^ ((i * 0x9E3779B97F4A7C15) & M64)
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x & M32


@pytest.mark.parametrize("seed", list(R.SEEDS.values()) + [-1, 0, (1 << 63) - 1, -(1 << 63)])
def test_hash32_vectorised_equals_scalar(seed):
    import numpy as np
    idx = [0, 1, 2, 63, 64, 12345, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 7, (1 << 40) + 3]
    got = R.hash32(seed, np.array(idx, dtype=np.uint64))
    assert [int(v) for v in got] == [_hash32_scalar(seed, i) for i in idx]


def test_threshold_and_inv_keep_conventions():
    assert R.attn_thresh(0.0) == 0 and R.attn_thresh(-1.0) == 0
    assert R.attn_thresh(0.5) == 1 << 31
    assert R.attn_thresh(0.1) == 429496736           # float(0.1) = 0x3DCCCCCD: 13421773 * 2^-27, times 2^32
    assert R.attn_thresh(1.0) == 4294967295          # clamped
    assert R.inv_keep(0.5) == 2.0 and R.inv_keep(0.0) == 1.0
    assert R.inv_keep(0.1) == float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(0.1)))
    km = R.keep_mask(R.SEEDS["h32"], 0.1, 1, 2, 32)
    assert km.shape == (1, 2, 32, 32) and set(km.unique().tolist()) == {0.0, R.inv_keep(0.1)}
    # element index order ((b * NH + h) * S + q) * S + k: the flat order of [B, NH, S, S]
    import numpy as np
    flat = R.hash32(R.SEEDS["h32"], np.arange(2 * 32 * 32, dtype=np.uint64)) >= np.uint32(R.attn_thresh(0.1))
    assert torch.equal(km.reshape(-1) > 0, torch.from_numpy(flat))
    assert torch.equal(R.keep_mask(5, 0.0, 1, 1, 32), torch.ones(1, 1, 32, 32, dtype=torch.float64))


# ---- the bounds and the emulation, on every GPU case ------------------------------------------

@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_emulation_stays_inside_the_bounds(case):
    r = R.reference(case)
    for n in R.OUTPUTS:
        assert r["emu_elem"][n] <= 1.0, (n, r["emu_elem"][n])
        assert torch.isfinite(r["tol"][n]).all() and bool((r["tol"][n] >= 0).all()), n
    # a bf16-limited output sits near its bound: the bounds are attainable, not slack
    assert r["emu_elem"]["O"] >= 0.5 and r["emu_elem"]["dV"] >= 0.5, r["emu_elem"]
    # the fp32 allowance can never hide a bf16-sized error
    for n in ("O", "dQ", "dK", "dV", "dbias"):
        share = float((r["tol32"][n] / r["tol"][n].clamp_min(1e-300)).median())
        assert share < 0.25, (n, share)
    # lse and Dbuf (against the ctx it is handed) are fp32-sized
    assert float((r["tol"]["lse"] / r["ref"]["lse"].abs().clamp_min(1.0)).max()) < 2.0 ** -12
    assert torch.equal(r["tol"]["lse"], r["tol32"]["lse"])


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_case_conditions(case):
    c = R.reference(case)["cond"]
    if case.mask:
        assert c["open_keys_min"] >= case.S / 4, c
        assert c["graded_share"] >= 0.10, c
        m = R.inputs(case)[2]
        assert float(m[case.B - 1, case.S - 5:].max()) == -10000.0 and (case.S - 5) % 16 != 0
        assert set(m.unique().tolist()) == set(R.GRADES)
    if case.p > 0:
        assert abs(c["keep_sigma"]) <= 4.0, c
        assert c["kept_per_row_min"] >= 8, c


def test_case_list_covers_the_issue():
    cs = R.CASES
    assert len(set(R.CASE_IDS)) == len(cs)
    a = [c for c in cs if c.group == "A"]
    assert {(c.S, c.B, c.NH) for c in a} >= {(S, B, NH) for S in R.ALL_S for B, NH in ((1, 1), (2, 3))} | {(128, 2, 12)}
    assert {c.S for c in a if c.scale == 0.25} == {64, 192}
    for S in (64, 192):
        assert {(c.bias, c.mask) for c in a if c.S == S} == {(True, True), (False, True), (True, False), (False, False)}
    b = [c for c in cs if c.group == "B"]
    assert {(c.S, c.p, c.seed) for c in b} == {(S, p, s) for S in (64, 128, 192, 256) for p in (0.1, 0.5)
                                               for s in R.SEEDS.values()}
    assert (R.SEEDS["h32"] & R.M64) >> 63 == 1 and R.SEEDS["h64"] >> 63 == 0


def test_bias_partials_reference_layout():
    """Row b * S / 16 + r of the partials holds rows 16 r ... 16 r + 15 of batch element
    b; column part * NH * 64 + h * 64 + d.  Their column sums are dbias."""
    case = _case("A-S192-B2-NH3")
    r = R.reference(case)
    want, bound = R.bpart_reference(r["ref"], r["tol"])
    assert want.shape == bound.shape == (case.B * case.S // 16, 3 * case.NH * R.HD)
    _close(want.sum(0), r["ref"]["dbias"], "column sums")
    b, rr, h, d = 1, 5, 2, 17
    for part, n in enumerate(("dQ", "dK", "dV")):
        _close(want[b * (case.S // 16) + rr, (part * case.NH + h) * R.HD + d],
               r["ref"][n][b, h, 16 * rr:16 * rr + 16, d].sum(), n)
    # without the bf16 store term, and still above the fp32 sum alone
    assert bool((bound.sum(0) <= r["tol"]["dbias_stored"]).all()) and bool((bound > 0).all())


# ---- mutants of the emulation fall outside ----------------------------------------------------

MUTANT_CASES = [
    ("mask_neighbour", "A-S64-B2-NH3", ("O", "lse", "dQ", "dV")),
    ("mask_neighbour", "A-S192-B2-NH3", ("O", "lse", "dQ", "dV")),
    ("drop_tile", "A-S64-B2-NH3", ("O", "lse")),
    ("drop_tile", "A-S256-B2-NH3", ("O", "lse")),
    ("swap_dk_slabs", "A-S64-B2-NH3", ("dK",)),
    ("swap_dk_slabs", "A-S192-B2-NH3", ("dK",)),
    ("lse_off", "A-S128-B2-NH3", ("lse",)),
    ("dropout_fwd_only", "B-S64-B2-NH3-p0.1-h32", ("dV",)),
    ("dropout_fwd_only", "B-S256-B2-NH3-p0.5-h64", ("dV",)),
    ("D_no_dropout", "B-S64-B2-NH3-p0.1-h32", ("D", "dQ", "dK")),
    ("D_no_dropout", "B-S192-B2-NH3-p0.5-h64", ("D", "dQ", "dK")),
]


@pytest.mark.parametrize("mutant,name,outside", MUTANT_CASES)
def test_mutants_fall_outside_the_bounds(mutant, name, outside):
    case = _case(name)
    r = R.reference(case)
    qkv, bias, mask, dO = R.inputs(case)
    keep = R.keep_mask(case.seed, case.p, case.B, case.NH, case.S) if case.p > 0 else None
    mut = R.emulate(qkv, bias, mask, dO, case.NH, case.scale, keep, mutant=mutant)
    fig = {n: R.elem_ratio(mut[n], r["ref"][n], r["tol"][n]) for n in R.OUTPUTS}
    print(mutant, name, {n: float("%.3g" % v) for n, v in fig.items()})
    for n in outside:
        assert fig[n] > 1.0, (n, fig)
    # and the row yardstick (twice the emulation's own worst row) sees it as well
    rows = {n: R.row_ratio(mut[n], r["ref"][n], r["tol"][n]) for n in R.ROW_OUTPUTS}
    seen = [n for n in R.ROW_OUTPUTS if n in outside and rows[n] > 2 * r["emu_rows"][n]]
    assert seen or not set(outside) & set(R.ROW_OUTPUTS), (rows, r["emu_rows"])

