"""tests/transformer_reference.py on the CPU, before it judges a kernel
(tests/test_transformer_edges_gpu.py): the float64 models against float64 autograd
of the plain compositions (the hash bits as a fixed mask), the derived bounds against
the fp32 / bf16 emulation of the kernels for every case (they hold, the bf16-limited
outputs come near them, the fp32 share stays below a quarter at the median element,
mean / rstd / the softmax row sums are fp32-sized), mutants of the emulation (they
fall outside), and the conditions a case needs to say anything."""
import math
import os
import re

import numpy as np
import pytest
import torch

import attention_reference as A
import transformer_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(a, b, what):
    err = float((a - b).abs().max())
    assert err <= 1e-10 * max(1e-30, float(b.abs().max())), (what, err)


DROPS = [(0.0, 0), (0.3, R.SEEDS["h32"]), (0.3, R.SEEDS["h64"])]


# ---- the models against autograd --------------------------------------------------------------

@pytest.mark.parametrize("p,seed", DROPS)
@pytest.mark.parametrize("kind,with_res", [("bdrln", True), ("bdrln", False), ("f32in", False), ("emb", False)])
def test_layernorm_models_match_float64_autograd(kind, with_res, p, seed):
    g = torch.Generator().manual_seed(11)
    N, H, S = 10, 256, 5
    keep = R.keep_scale(R.keep_bits(seed, p, N, H), p)
    gam = (1 + 0.1 * torch.randn(H, generator=g)).double().requires_grad_()
    bet = (0.1 * torch.randn(H, generator=g)).double().requires_grad_()
    dy = torch.randn(N, H, generator=g).bfloat16()
    if kind == "bdrln":
        inp = dict(x=torch.randn(N, H, generator=g).bfloat16(), bias=torch.randn(H, generator=g) * 0.1,
                   res=torch.randn(N, H, generator=g).bfloat16() if with_res else None)
        t = (inp["x"].double() + inp["bias"].double()).requires_grad_()
        v = t * keep + (inp["res"].double() if with_res else 0)
    elif kind == "f32in":
        inp = dict(x=torch.randn(N, H, generator=g))
        t = inp["x"].double().requires_grad_()
        v = t
    else:
        inp = dict(word=torch.randn(7, H, generator=g), typ=torch.randn(2, H, generator=g),
                   pos=torch.randn(S + 2, H, generator=g), ids=torch.randint(0, 7, (N // S, S), generator=g),
                   tt=torch.randint(0, 2, (N // S, S), generator=g), S=S)
        t = (inp["word"].double()[inp["ids"].reshape(-1)] + inp["typ"].double()[inp["tt"].reshape(-1)]
             + inp["pos"].double()[torch.arange(N) % S]).requires_grad_()
        v = t
    inp.update(gamma=gam.detach().float(), beta=bet.detach().float())
    gam64, bet64 = inp["gamma"].double().requires_grad_(), inp["beta"].double().requires_grad_()
    v.retain_grad() if v is not t else None
    eps = R.f32(R.EPS)
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    y = (v - mean) / torch.sqrt(var + eps) * gam64 + bet64
    ykeep = keep if kind != "bdrln" else torch.ones_like(keep)
    yo = y * ykeep
    ref, tol = R.ln_fwd_model(kind, inp, keep)
    _close(ref["y"], yo.detach(), "y")
    _close(ref["s"], v.detach(), "s")
    _close(ref["mean"], mean.detach().squeeze(-1), "mean")
    _close(ref["rstd"], (var.detach() + eps).squeeze(-1) ** -0.5, "rstd")
    for n in ("y", "s", "mean", "rstd"):
        assert torch.isfinite(tol[n]).all() and bool((tol[n] > 0).all())
    # backward: ln_bwd sees the gradient of y (the wrappers apply dropout_bf16 to dy first for
    # the embedding forms), the stored s and the statistics -- here all exact
    y.backward(dy.double())
    bkeep = keep if kind == "bdrln" else torch.ones_like(keep)
    bref, _ = R.ln_bwd_model(dy, v.detach(), mean.detach().squeeze(-1), (var.detach() + eps).squeeze(-1) ** -0.5,
                             inp["gamma"], bkeep)
    ds = v.grad if v is not t else t.grad
    _close(bref["ds"], ds, "ds")
    _close(bref["dgamma"], gam64.grad, "dgamma")
    _close(bref["dbeta"], bet64.grad, "dbeta")
    if kind == "bdrln":
        _close(bref["dxb"], t.grad, "dxb")
        _close(bref["dbias"], t.grad.sum(0), "dbias")


def test_gelu_model_matches_float64_autograd():
    g = torch.Generator().manual_seed(12)
    x = R.gelu_x(33, 12, g)
    bias = torch.randn(12, generator=g) * 0.02
    dy = torch.randn(33, 12, generator=g).bfloat16()
    z = (x.double() + bias.double()).requires_grad_()
    y = z * 0.5 * (1 + torch.special.erf(z / math.sqrt(2.0)))
    y.backward(dy.double())
    ref, tol = R.gelu_model(x, bias, dy)
    _close(ref["y"], y.detach(), "y")
    _close(ref["dx"], z.grad, "dx")
    _close(ref["dbias"], z.grad.sum(0), "dbias")
    ygelu = torch.nn.functional.gelu(z.detach())
    _close(ref["y"], ygelu, "gelu")


def test_gelu_polynomial_error_is_absolute_not_relative():
    """Abramowitz-Stegun 7.1.26 in float64: the cdf error stays below 7.5e-8 (6.97e-8
    measured), and below z = -6 it exceeds one bf16 ulp of y = z cdf(z)."""
    z = torch.linspace(-9, 9, 180001, dtype=torch.float64)
    t = 1.0 / (1.0 + R.AS_P * z.abs() / math.sqrt(2.0))
    poly, _, _ = R._as_poly(t)
    tail = 0.5 * poly * torch.exp(-0.5 * z * z)
    cdf = torch.where(z >= 0, 1 - tail, tail)
    exact = 0.5 * torch.special.erfc(-z / math.sqrt(2.0))
    err = (cdf - exact).abs()
    assert 6.9e-8 < float(err.max()) <= R.AS_CDF
    far = z < -6.5
    assert bool((err[far] * z[far].abs() > R.U_BF * (z[far] * exact[far]).abs()).any())


@pytest.mark.parametrize("p,seed", DROPS)
@pytest.mark.parametrize("masked", [True, False])
def test_softmax_models_match_float64_autograd(masked, p, seed):
    g = torch.Generator().manual_seed(13)
    rows_per_batch, Sk = 3, 20
    rows = 2 * rows_per_batch
    S = (torch.randn(rows, Sk, generator=g) * 8).bfloat16()
    mask = R.graded_mask(2, Sk) if masked else None
    keep = R.keep_scale(R.keep_bits(seed, p, rows, Sk), p)
    dPd = torch.randn(rows, Sk, generator=g).bfloat16()
    s = S.double().requires_grad_()
    z = R.f32(0.125) * s
    if masked:
        z = z + mask.double().repeat_interleave(rows_per_batch, 0)
    P = torch.softmax(z, -1)
    (P * keep).backward(dPd.double())
    ref, tol = R.softmax_fwd_model(S, mask, rows_per_batch, 0.125, keep)
    _close(ref["P"], P.detach(), "P")
    _close(ref["Pd"], (P * keep).detach(), "Pd")
    bref, _ = R.softmax_bwd_model(dPd, P.detach(), 0.125, keep)
    _close(bref["dS"], s.grad, "dS")


# ---- the dropout bits -------------------------------------------------------------------------

def test_threshold_formula_is_the_attention_kernels():
    """thresh_of in transformer.hip is attn_thresh's formula: floor(double(float(p)) * 2^32),
    clamped to 2^32 - 1, 0 for p <= 0."""
    src = open(os.path.join(REPO, "csrc", "kernels", "transformer.hip")).read()
    body = re.search(r"static inline uint32_t thresh_of\(float p\) \{(.*?)\n\}", src, re.S).group(1)
    assert "if (p <= 0.f) return 0u;" in body
    assert "double t = (double)p * 4294967296.0;" in body
    assert "return t >= 4294967295.0 ? 4294967295u : (uint32_t)t;" in body
    assert R.attn_thresh is A.attn_thresh and R.hash32 is A.hash32 and R.inv_keep is A.inv_keep
    assert R.attn_thresh(0.1) == 429496736 and R.attn_thresh(0.5) == 1 << 31 and R.attn_thresh(0.0) == 0


def test_element_index_is_row_times_width_plus_column():
    for seed in R.SEEDS.values():
        b = R.keep_bits(seed, 0.3, 5, 12)
        flat = R.hash32(seed, np.arange(60, dtype=np.uint64)) >= np.uint32(R.attn_thresh(0.3))
        assert torch.equal(b.reshape(-1), torch.from_numpy(flat))
        assert torch.equal(R.keep_bits_rows(seed, 0.3, [4, 1], 12), b[[4, 1]])
    k = R.keep_scale(R.keep_bits(R.SEEDS["h32"], 0.1, 4, 64), 0.1)
    assert set(k.unique().tolist()) == {0.0, R.inv_keep(0.1)}
    assert torch.equal(R.keep_scale(R.keep_bits(5, 0.0, 3, 8), 0.0), torch.ones(3, 8, dtype=torch.float64))


# ---- the bounds and the emulation, on every case ----------------------------------------------

BF16_LIMITED = dict(bdrln=("y", "ds"), f32in=("y", "ds"), emb=("y", "ds"), gelu=("y", "dx"), softmax=("P",),
                    dropout=())
SHARE = dict(bdrln=("y", "s", "ds", "dxb"), f32in=("y", "ds"), emb=("y", "s", "ds"), gelu=("y", "dx"),
             softmax=("P", "Pd", "dS"), dropout=("y",))


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_emulation_stays_inside_the_bounds(case):
    r = R.reference(case)
    ref, tol, tol32 = r["ref"], r["tol"], r["tol32"]
    for n, v in r["emu_elem"].items():
        assert v <= 1.0, (n, v)
        assert torch.isfinite(tol[n]).all() and bool((tol[n] > 0).all()), n
    # a bf16-limited output sits near its bound somewhere: the bounds are attainable
    for n in BF16_LIMITED[case.kind]:
        assert r["emu_elem"][n] >= 0.5, (n, r["emu_elem"][n])
    # the fp32 allowance can never hide a bf16-sized error: its share at the median element
    # that is not exactly zero (a dropped element, a masked key).  In a fully masked softmax
    # row every z is about -10000 and W |z| = 6e-4 is the true size of the fp32 error of z:
    # those rows are left out of the median.
    for n in SHARE[case.kind]:
        live = ref[n] != 0
        if case.kind == "softmax":
            live = live & (ref["z"].max(-1, keepdim=True).values > -5000)
        if not bool(live.any()):
            continue
        share = float((tol32[n] / tol[n])[live].median())
        assert share < 0.25, (n, share)
    # fp32-sized outputs: relative to the scale of what they sum
    if case.kind in R.LN_KINDS:
        scale = ref["s"].abs().mean(-1)
        assert float((tol["mean"] / torch.maximum(ref["mean"].abs(), scale)).max()) <= 2.0 ** -12
        # rstd inherits the error of v - mean over the row's spread: the condition number
        # mean|v| * rstd of the row (1 for an ordinary row, 192 for the cancellation cases)
        cond = (scale * ref["rstd"]).clamp_min(1.0)
        assert float((tol["rstd"] / ref["rstd"] / cond).max()) <= 2.0 ** -12
        if "cancel" not in case.tags:
            assert float(cond.max()) < 2.0 and float((tol["rstd"] / ref["rstd"]).max()) <= 2.0 ** -12
        assert torch.equal(tol["mean"], tol32["mean"]) and torch.equal(tol["rstd"], tol32["rstd"])
    if case.kind == "softmax":
        live = ref["z"].max(-1).values > -5000          # a fully masked row: W |z| = 6e-4, see above
        assert float(tol["rowsum"][live].max()) <= 2.0 ** -12
        rs = torch.exp(ref["z"] - ref["z"].max(-1, keepdim=True).values).sum(-1)
        assert bool((((r["emu"]["rowsum"] - rs).abs() / rs)[live] <= tol["rowsum"][live]).all())


def test_emulation_worst_ratios_per_output():
    """The figures the pull request records: the worst error / bound of the emulation."""
    worst = {}
    for c in R.CASES:
        for n, v in R.reference(c)["emu_elem"].items():
            k = "%s.%s" % (c.kind, n)
            worst[k] = max(worst.get(k, 0.0), v)
    print({k: float("%.3g" % v) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0


# ---- mutants of the emulation fall outside ----------------------------------------------------

LN_FWD_MUTANT_CASES = [
    ("one_pass_var", "bdrln-N37-H256-cancel", ("rstd",)),
    ("one_pass_var", "f32in-N9-H768-cancel", ("rstd",)),
    ("tail_row_stats", "bdrln-N37-H768-res", ("y", "mean", "rstd")),
    ("tail_row_stats", "bdrln-N9-H256", ("y", "mean", "rstd")),
    ("tail_row_stats", "f32in-N3-H768", ("y", "mean", "rstd")),
    ("drop_after_residual", "bdrln-N37-H768-res-p0.1-h32", ("y", "s")),
    ("drop_after_residual", "bdrln-N37-H768-res-p0.5-h64", ("y", "s")),
    ("mask_no_row_base", "bdrln-N9-H256-p0.5-h64", ("y", "s")),
    ("mask_no_row_base", "f32in-N37-H768-p0.1-h32", ("y",)),
    ("mask_no_row_base", "emb-B5-S7-H256-mixed-p0.5-h32", ("y",)),
    ("pos_row_mod_off", "emb-B3-S7-H512-zeros", ("y", "s", "mean")),
    ("pos_row_mod_off", "emb-B5-S16-H512-mixed", ("y", "s", "mean")),
]


@pytest.mark.parametrize("mutant,name,outside", LN_FWD_MUTANT_CASES)
def test_layernorm_forward_mutants_fall_outside(mutant, name, outside):
    c = R.case(name)
    r = R.reference(c)
    mut = R.ln_fwd_emulate(c.kind, R.inputs(c), c.seed, c.p, mutant=mutant)
    fig = {n: R.elem_ratio(mut[n], r["ref"][n], r["tol"][n]) for n in ("y", "s", "mean", "rstd")}
    print(mutant, name, {n: float("%.3g" % v) for n, v in fig.items()})
    for n in outside:
        assert fig[n] > 1.0, (n, fig)


LN_BWD_MUTANT_CASES = [
    ("ds_no_s2", "bdrln-N37-H1024-res", ("ds", "dxb")),
    ("ds_no_s2", "bdrln-N1-H256", ("ds", "dxb")),
    ("colsum_skip_last_row", "bdrln-N37-H768-res", ("dgamma", "dbeta", "dbias")),
    ("colsum_skip_last_row", "bdrln-N9-H256-res", ("dgamma", "dbeta", "dbias")),
    ("dxb_unmasked", "bdrln-N37-H768-res-p0.1-h32", ("dxb", "dbias")),
    ("dxb_unmasked", "bdrln-N9-H256-p0.5-h64", ("dxb", "dbias")),
]


@pytest.mark.parametrize("mutant,name,outside", LN_BWD_MUTANT_CASES)
def test_layernorm_backward_mutants_fall_outside(mutant, name, outside):
    r = R.reference(R.case(name))
    mut = R.ln_bwd_emulate(*r["hand"], r["bkeep"], mutant=mutant)
    fig = {n: R.elem_ratio(mut[n], r["ref"][n], r["tol"][n]) for n in R.LN_BWD_OUTPUTS}
    print(mutant, name, {n: float("%.3g" % v) for n, v in fig.items()})
    for n in outside:
        assert fig[n] > 1.0, (n, fig)


@pytest.mark.parametrize("name", ["emb-B3-S7-H512-zeros", "emb-B5-S16-H512-mixed", "emb-B9-S7-H256-mixed"])
def test_embedding_type_swap_mutant_is_seen_exactly(name):
    c = R.case(name)
    inp = R.inputs(c)
    ds = integer_bf16(c.B * c.S, c.H, 5)
    pos, typ = R.emb_bwd_aux_model(ds, inp["tt"], c.S)
    mpos, mtyp = R.emb_bwd_aux_model(ds, inp["tt"], c.S, mutant="typ_swapped")
    assert torch.equal(pos, mpos) and not torch.equal(typ, mtyp)
    assert torch.equal(typ.sum(0), pos.sum(0)) and torch.equal(typ.sum(0), ds.double().sum(0))


GELU_MUTANT_CASES = [
    ("bias_col_shift", "gelu-N33-H1024", ("y", "dx")),
    ("bias_col_shift", "gelu-N5-H12", ("y", "dx")),
    ("grad_cdf_only", "gelu-N31-H3072", ("dx", "dbias")),
    ("grad_cdf_only", "gelu-N31-H516", ("dx", "dbias")),
    ("strip_tail_dropped", "gelu-N5-H1032", ("y", "dx", "dbias")),
    ("strip_tail_dropped", "gelu-N67-H1028", ("y", "dx", "dbias")),
]


@pytest.mark.parametrize("mutant,name,outside", GELU_MUTANT_CASES)
def test_gelu_mutants_fall_outside(mutant, name, outside):
    c = R.case(name)
    r, inp = R.reference(c), R.inputs(c)
    mut = R.gelu_emulate(inp["x"], inp["bias"], inp["dy"], mutant=mutant)
    fig = {n: R.elem_ratio(mut[n], r["ref"][n], r["tol"][n]) for n in ("y", "dx", "dbias")}
    print(mutant, name, {n: float("%.3g" % v) for n, v in fig.items()})
    for n in outside:
        assert fig[n] > 1.0, (n, fig)


SOFTMAX_MUTANT_CASES = [
    ("mask_other_batch", "softmax-Sk64-Sq5-graded", ("P", "Pd", "dS")),
    ("mask_other_batch", "softmax-Sk260-Sq1-graded", ("P", "Pd", "dS")),
    ("last_group_dropped", "softmax-Sk260-Sq5-none", ("P", "Pd")),
    ("last_group_dropped", "softmax-Sk1028-Sq5-none", ("P", "Pd")),
    ("bwd_dot_undropped", "softmax-Sk64-Sq5-graded-p0.1-h32", ("dS",)),
    ("bwd_dot_undropped", "softmax-Sk260-Sq5-graded-p0.5-h64", ("dS",)),
]


@pytest.mark.parametrize("mutant,name,outside", SOFTMAX_MUTANT_CASES)
def test_softmax_mutants_fall_outside(mutant, name, outside):
    c = R.case(name)
    r, inp = R.reference(c), R.inputs(c)
    mut = R.softmax_emulate(inp["S"], inp["mask"], inp["rows_per_batch"], inp["scale"], r["keep"], inp["dPd"],
                            mutant=mutant)
    # the backward is judged from the P it was handed, as on the GPU
    bref, btol = R.softmax_bwd_model(inp["dPd"], mut["P"].bfloat16(), inp["scale"], r["keep"])
    ref, tol = dict(r["ref"], **bref), dict(r["tol"], **btol)
    if mutant == "mask_other_batch":        # P itself is wrong; dS follows the wrong P, so judge it from the true one
        ref, tol = r["ref"], r["tol"]
    fig = {n: R.elem_ratio(mut[n], ref[n], tol[n]) for n in ("P", "Pd", "dS")}
    print(mutant, name, {n: float("%.3g" % v) for n, v in fig.items()})
    for n in outside:
        assert fig[n] > 1.0, (n, fig)


def test_every_mutant_has_two_cases_one_of_them_an_edge():
    tables = {R.LN_FWD_MUTANTS: LN_FWD_MUTANT_CASES, R.LN_BWD_MUTANTS: LN_BWD_MUTANT_CASES,
              R.GELU_MUTANTS: GELU_MUTANT_CASES, R.SOFTMAX_MUTANTS: SOFTMAX_MUTANT_CASES}

    def edge(c):
        d = dict(c.d)
        return (d.get("N", 0) % 2 == 1 or d.get("H", 0) % 8 == 4 or d.get("Sk", 0) % 256 not in (0, 64)
                or d.get("B", 4) % 4 != 0)

    for names, table in tables.items():
        for m in names:
            cs = [R.case(n) for mm, n, _ in table if mm == m]
            assert len(cs) >= 2 and any(edge(c) for c in cs), m


# ---- the conditions a case needs ---------------------------------------------------------------

def integer_bf16(N, H, seed):
    """Integer-valued bf16 in [-8, 8]: every partial sum of fewer than 2^20 of them is exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (N, H), generator=g).float().bfloat16()


@pytest.mark.parametrize("case", [c for c in R.CASES if c.p > 0], ids=[c.name for c in R.CASES if c.p > 0])
def test_dropout_case_conditions(case):
    bits = R.reference(case)["keep"] > 0
    n = bits.numel()
    p = float(np.float32(case.p))
    sigma = (float(bits.double().mean()) - (1 - p)) / math.sqrt(p * (1 - p) / n)
    assert abs(sigma) <= 4.0, sigma
    assert int(bits.sum(-1).min()) >= 8


@pytest.mark.parametrize("case", R.cases_of("softmax"), ids=[c.name for c in R.cases_of("softmax")])
def test_softmax_case_conditions(case):
    inp = R.inputs(case)
    z = R.reference(case)["ref"]["z"]
    span = R.f32(inp["scale"]) * inp["S"].double()
    assert float(span.max()) == 30.0 and float(span.min()) == -30.0
    assert inp["S"].shape[0] in (6, 30) and inp["S"].shape[0] % 4 != 0
    m = inp["mask"]
    if m is None:
        assert case.mask == "none"
        return
    assert not torch.equal(m[0], m[1])                                   # differs per batch row
    open_rows = [b for b in range(m.shape[0]) if float(m[b].max()) > -100]
    assert len(open_rows) == (1 if case.mask == "full" else 2)
    for b in open_rows:
        assert int((m[b] > -100).sum()) >= case.Sk / 4
    if case.Sk >= 64:
        assert set(m.unique().tolist()) == {0.0, -1.0, -2.5, -0.75, -10000.0}
    assert z.shape == inp["S"].shape


@pytest.mark.parametrize("case", R.cases_of("gelu"), ids=[c.name for c in R.cases_of("gelu")])
def test_gelu_inputs_cover_the_range(case):
    z = R.reference(case)["ref"]["z"].reshape(-1)
    assert float(z.abs().max()) < 9.5
    counts = torch.histc(z, bins=18, min=-9, max=9)
    assert int(counts.min()) >= 1, counts


def test_cancellation_cases():
    for c in R.CASES:
        if "cancel" in c.tags:
            s = R.reference(c)["ref"]["s"]
            assert float((s.mean(-1) - 3).abs().max()) < 0.01
            assert 0.5 < float(s.std(-1).mean()) * 64 < 1.5


def test_exact_cases_keep_every_partial_sum_below_2_to_24():
    """The integer-valued reducer inputs of the GPU file: |value| <= 8 and at most
    max(COLSUM_N) rows, 5 slabs or 16 batch rows, so every partial sum is far below 2^24."""
    assert 8 * max(max(R.COLSUM_N), max(R.SLAB_S), max(R.EMB_B), max(R.LN_N)) + 2 ** 10 < 2 ** 24
    x = integer_bf16(300, 130, 1)
    assert torch.equal(x.float(), x.float().round()) and float(x.float().abs().max()) == 8.0


def test_case_list_covers_the_issue():
    cs = R.CASES
    assert len(set(R.CASE_IDS)) == len(cs)
    for kind in ("bdrln", "f32in"):
        k = R.cases_of(kind)
        assert {c.H for c in k if c.N == 37} >= set(R.ALL_H)
        res = (True, False) if kind == "bdrln" else (False,)
        assert {(c.N, c.H, c.res) for c in k if c.p == 0 and not c.tags} >= {(N, H, r) for N in R.LN_N
                                                                             for H in (256, 768) for r in res}
        assert any("cancel" in c.tags for c in k)
        assert {(c.p, c.seed) for c in k if c.p > 0} == {(p, s) for p in R.DROP_P for s in R.SEEDS.values()}
    assert {c.res for c in R.cases_of("bdrln") if c.p > 0} == {True, False}
    e = R.cases_of("emb")
    assert {c.H for c in e if c.B * c.S == 37} >= set(R.ALL_H)
    assert {c.B for c in e} >= set(R.EMB_B) and {c.S for c in e} >= set(R.EMB_S) and {c.H for c in e} >= set(R.EMB_H)
    assert {c.tt for c in e} == {"zeros", "ones", "mixed"} and all(c.pos_rows > c.S for c in e)
    assert {(c.p, c.seed) for c in e if c.p > 0} == {(p, s) for p in R.DROP_P for s in R.SEEDS.values()}
    for c in e:
        ids = R.inputs(c)["ids"].reshape(-1)
        assert ids.numel() == 1 or (int(ids.min()) == 0 and int(ids.max()) == c.V - 1)
    assert any(R.inputs(c)["ids"].unique().numel() < c.B * c.S for c in e)
    g = R.cases_of("gelu")
    assert {c.H for c in g} == set(R.GELU_H4) | set(R.GELU_H8) and all(h % 8 == 4 for h in R.GELU_H4)
    assert {c.N for c in g if c.H % 8} == set(R.GELU_N) and {c.N for c in g if c.H % 8 == 0} == set(R.GELU_N)
    s = R.cases_of("softmax")
    assert {c.Sk for c in s} == set(R.SOFTMAX_SK)
    assert {(c.Sk, c.Sq) for c in s if c.mask == "graded" and c.p == 0} == {(k, q) for k in R.SOFTMAX_SK
                                                                            for q in R.SOFTMAX_SQ}
    assert {c.mask for c in s} == {"graded", "full", "none"}
    assert {R.softmax_nc(c.Sk) for c in s} == {1, 2, 4, 8, 16}
    assert {(c.p, c.seed) for c in s if c.p > 0} == {(p, sd) for p in R.DROP_P for sd in R.SEEDS.values()}
    assert {(c.p, c.seed) for c in R.cases_of("dropout")} == {(p, sd) for p in R.DROP_P for sd in R.SEEDS.values()}
    assert (R.SEEDS["h32"] & A.M64) >> 63 == 1 and R.SEEDS["h64"] >> 63 == 0
    # the grid caps of the launchers: row_grid 8192 blocks of 4 rows (bdrln_fwd16: of 8), 32768 and 65536 blocks
    assert R.WRAP["bdrln"][0] > 8192 * 8 and R.WRAP["f32in"][0] > 8192 * 4 and R.WRAP["softmax"][0] > 8192 * 4
    assert R.WRAP["gelu8"][0] * R.WRAP["gelu8"][1] > 32768 * 256 * 8
    assert R.WRAP["dropout"][0] * R.WRAP["dropout"][1] > 65536 * 256 * 4
    src = open(os.path.join(REPO, "csrc", "kernels", "transformer.hip")).read()
    assert "return g < 8192 ? (g > 0 ? g : 1) : 8192;" in src and "if (g8 > 32768) g8 = 32768;" in src
    assert src.count("if (g > 65536) g = 65536;") == 2
