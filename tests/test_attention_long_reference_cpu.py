"""tests/attention_long_reference.py on the CPU, before it judges a kernel
(tests/test_attention_long_gpu.py): the float64 model at S = 384 against float64
autograd, the streamed emulation at blocks of 32 / 64 / 128 keys inside the bounds for
every GPU case, every mutant of the emulation outside them at both positions and at
blocks of 64 and 128, and the fp32 share of the bounds below the bounds."""
import pytest
import torch

import attention_long_reference as L
import attention_reference as R


def _close(a, b, what):
    err = float((a - b).abs().max())
    assert err <= 1e-10 * max(1e-30, float(b.abs().max())), (what, err)


@pytest.mark.parametrize("p,seed", [(0.0, 0), (0.3, R.SEEDS["h32"]), (0.3, R.SEEDS["h64"])])
def test_model_matches_float64_autograd_at_384(p, seed):
    B, NH, S, scale = 2, 2, 384, 0.125
    H3 = 3 * NH * R.HD
    g = torch.Generator().manual_seed(11)
    qkv = (torch.randn(B, S, H3, generator=g) * 2).bfloat16()
    bias = torch.randn(H3, generator=g) * 0.5
    mask = L.long_mask(B, S, first_block=True)
    dO = torch.randn(B, S, NH * R.HD, generator=g).bfloat16()
    keep = R.keep_mask(seed, p, B, NH, S) if p > 0 else None
    m = R.model(qkv, bias, mask, dO, NH, scale, keep)
    x = R.operands(qkv, bias).double().requires_grad_()
    q, k, v = R.heads(x, NH, 3)
    z = scale * torch.matmul(q, k.transpose(-1, -2)) + mask.double()[:, None, None, :]
    pr = torch.softmax(z, -1)
    if keep is not None:
        pr = pr * keep
    out = torch.matmul(pr, v)
    out.backward(R.heads(dO.double(), NH, 1)[0])
    dq, dk, dv = R.split_dqkv(x.grad, NH)
    _close(m["O"], out.detach(), "O")
    _close(m["lse"], torch.logsumexp(z.detach(), -1), "lse")
    _close(m["dQ"], dq, "dQ")
    _close(m["dK"], dk, "dK")
    _close(m["dV"], dv, "dV")
    _close(m["dbias"], x.grad.sum((0, 1)), "dbias")


def test_bounds_without_the_streaming_terms_are_the_one_pass_bounds():
    """bounds(..., nblk=0) is R.bounds term for term; with the steps counted every bound
    is at least that, and by an fp32-sized amount only."""
    c = L.case("B-S384-B2-NH3-p0.1-h32")
    qkv, bias, mask, dO = L.inputs(c)
    m = R.model(qkv, bias, mask, dO, c.NH, c.scale, L.keep_of(c))
    one, zero, full = R.bounds(m, c.scale), L.bounds(m, c.scale, 0), L.reference(c)["tol"]
    assert set(one) == set(zero) == set(full)
    for n in one:
        assert torch.equal(one[n], zero[n]), n
        assert bool((full[n] >= one[n]).all()), n
        assert float(((full[n] - one[n]) / one[n].clamp_min(1e-300)).max()) < (0.05 if n in ("lse",) else 0.01), n


def test_masks_are_the_ones_the_cases_need():
    m = L.long_mask(2, 384, first_block=True)
    assert m[0].tolist() == [-0.25 * ((383 - k) // 32) for k in range(384)]
    assert float(m[0, -1]) == 0.0 and float(m[0, 0]) == -2.75          # first block: e^-2.75 ... of the weight
    assert bool((m[1, :128] == -10000.0).all()) and float(m[1, 128:379].max()) == 0.0
    assert float(m[1, 379:].max()) == -10000.0 and 379 % 16 != 0
    plain = L.long_mask(2, 384)
    assert torch.equal(plain[1], R.graded_mask(2, 384)[1]) and torch.equal(plain[0], m[0])


def test_case_list_covers_the_issue():
    cs = L.CASES
    assert len(set(L.CASE_IDS)) == len(cs)
    a = [c for c in cs if c.group == "A"]
    assert {(c.S, c.B, c.NH) for c in a} == {(384, 1, 1), (384, 2, 3), (512, 2, 3), (640, 2, 2), (1024, 1, 2)}
    s384 = [c for c in a if (c.S, c.B, c.NH) == (384, 2, 3)]
    assert {(c.bias, c.mask, c.scale, c.first_block) for c in s384} == {
        (True, True, 0.125, False), (False, True, 0.125, False), (True, False, 0.125, False),
        (True, True, 0.25, False), (True, True, 0.125, True)}
    b = [c for c in cs if c.group == "B"]
    assert {(c.S, c.p, c.seed) for c in b} == {(S, p, s) for S in (384, 512) for p in (0.1, 0.5)
                                               for s in R.SEEDS.values()}
    assert all(c.S % 128 == 0 for c in cs) and (640 // 128) % 2 == 1


@pytest.mark.parametrize("c", L.CASES, ids=L.CASE_IDS)
def test_emulation_stays_inside_the_bounds(c):
    r = L.reference(c)
    qkv, bias, mask, dO = L.inputs(c)
    for n in L.OUTPUTS:
        assert torch.isfinite(r["tol"][n]).all() and bool((r["tol"][n] >= 0).all()), n
        # bounds(..., u=0), the fp32 share, is below the bound everywhere
        assert bool((r["tol32"][n] <= r["tol"][n]).all()), n
    for n in ("O", "dQ", "dK", "dV", "dbias"):
        share = float((r["tol32"][n] / r["tol"][n].clamp_min(1e-300)).median())
        assert share < 0.25, (n, share)
    assert torch.equal(r["tol"]["lse"], r["tol32"]["lse"])
    for block in L.BLOCKS:
        fig = L.figures(L.emulate(qkv, bias, mask, dO, c.NH, c.scale, L.keep_of(c), block=block), r)
        print(c.name, block, {n: float("%.3g" % v) for n, v in fig.items()})
        for n in L.OUTPUTS:
            assert fig[n] <= 1.0, (block, n, fig[n])
        # a bf16-limited output sits near its bound: the bounds are attainable, not slack
        assert fig["O"] >= 0.5 and fig["dV"] >= 0.5, fig


# mutant -> (case, the outputs that must leave their bounds)
MUTANT_CASES = {
    "sum_after_dropout": ("B-S384-B2-NH3-p0.1-h32", ("O", "lse")),
    "no_rescale_acc": ("A-S384-B2-NH3", ("O",)),
    "stale_v": ("A-S384-B2-NH3", ("O",)),
    "lse_first_max": ("A-S384-B2-NH3", ("lse",)),
    "dq_skip_block": ("A-S384-B2-NH3", ("dQ",)),
    "dkv_skip_qblock": ("A-S384-B2-NH3", ("dK", "dV")),
    "D_no_dropout": ("B-S384-B2-NH3-p0.1-h32", ("D", "dQ", "dK")),
}


@pytest.mark.parametrize("block", [64, 128])
@pytest.mark.parametrize("pos", L.POSITIONS)
@pytest.mark.parametrize("mutant", L.MUTANTS)
def test_mutants_fall_outside_the_bounds(mutant, pos, block):
    name, outside = MUTANT_CASES[mutant]
    c = L.case(name)
    r = L.reference(c)
    qkv, bias, mask, dO = L.inputs(c)
    mut = L.emulate(qkv, bias, mask, dO, c.NH, c.scale, L.keep_of(c), block=block, mutant=mutant, pos=pos)
    fig = L.figures(mut, r)
    print(mutant, pos, block, {n: float("%.3g" % v) for n, v in fig.items()})
    for n in outside:
        assert fig[n] > 1.0, (n, fig)
