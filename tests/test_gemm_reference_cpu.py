"""tests/gemm_reference.py against itself, without a GPU: the exact tier's cases
really are exact (and really need rounding where they claim to), bf16_rne is
torch's rounding, the fp32 transcriptions agree with float64 to the measured
tables, and the bounds are tight enough that known-wrong variants of the
formulas fall outside them -- so the GPU tests that use them are not vacuous."""
import numpy as np
import pytest
import torch

import gemm_reference as R

ALL = [c for g in R.CASES.values() for c in g]
EXACT = [c for c in ALL if not c.gauss]
GRID = np.arange(-64 * 16, 64 * 16 + 1) / 16.0     # multiples of 2^-4: every z the activation cases reach


def test_case_names_unique_and_contract_shapes():
    names = [c.name for c in ALL]
    assert len(set(names)) == len(names)
    for c in ALL:
        assert c.K % 64 == 0 and (c.variant not in (8, 9) or c.K % 128 == 0), c.name
        assert not (c.tA and c.M % 8) and not (not c.tB and c.N % 8), c.name
        if c.split_k != 1:
            assert not c.obf and c.act == 0 and c.beta in (0.0, 1.0), c.name
        if c.kind in ("ga", "dg"):
            assert c.M % 256 == 0 and c.N % 256 == 0 and c.K % 128 == 0, c.name


@pytest.mark.parametrize("c", [c for c in EXACT if c.M * c.N * c.K <= 2 ** 27], ids=lambda c: c.name)
def test_every_partial_sum_is_exact(c):
    ex = R.exact(c)
    assert float((ex.magnitude / ex.unit).max()) < 2 ** 24
    assert np.array_equal(ex.z / ex.unit, np.round(ex.z / ex.unit))
    assert np.array_equal(ex.z.astype(np.float32).astype(np.float64), ex.z)


def test_large_cases_exact_by_their_worst_element():
    for c in EXACT:
        if c.M * c.N * c.K > 2 ** 27:
            worst = abs(c.alpha) * c.K * (c.rng * c.scale) ** 2 + 4 + 8 * abs(c.beta)
            assert worst / R.unit(c) < 2 ** 24, c.name


@pytest.mark.parametrize("c", [c for c in EXACT if c.obf and c.kind == "gemm" and c.act == 0 and c.rng == 11 and not c.bias and c.beta == 0.0
                               and c.K == 128 and c.alpha == 1.0 and c.M * c.N >= 4096], ids=lambda c: c.name)
def test_bf16_cases_need_rounding(c):
    z = R.exact(c).z
    frac = float(np.mean(R.bf16_val(R.bf16_rne(z)) != z))
    assert 0.2 <= frac <= 0.8, frac


@pytest.mark.parametrize("c", R.CASES["K"], ids=lambda c: c.name)
def test_stats_cases_are_exact_and_tell_stored_from_unrounded(c):
    z = R.exact(c).z
    stored = R.bf16_val(R.bf16_rne(z))
    ps, pu = R.bn_partials(stored, c.M), R.bn_partials(z, c.M)
    assert ps.shape == (2, (c.M + 127) // 128, c.N)
    assert float(np.abs(ps).max()) < 2 ** 24 and float(np.abs(pu).max()) < 2 ** 24
    if c.M * c.N >= 128 * 136:
        assert float(np.mean(stored != z)) >= 0.01
        assert np.any(ps[0] != pu[0]) and np.any(ps[1] != pu[1])


def test_bf16_rne_is_torch_rounding():
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    lows = np.array([0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)   # below / on / above every tie
    bits = (hi[:, None] | lows[None, :]).ravel()
    x = bits.view(np.float32)
    finite = np.isfinite(x)
    want = torch.from_numpy(x.copy()).bfloat16().view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_rne(x)
    assert np.array_equal(got[finite], want[finite])
    assert np.all(np.isnan(R.bf16_val(got[np.isnan(x)])))
    # exact ties go to the even neighbour, both ways
    assert R.bf16_rne(np.float32(257.0)) == R.bf16_rne(np.float32(256.0))
    assert R.bf16_rne(np.float32(259.0)) == R.bf16_rne(np.float32(260.0))
    assert R.bf16_trunc(np.float32(259.0)) == R.bf16_rne(np.float32(258.0))
    k = R.bf16_key(R.bf16_rne(np.array([-3.0, -0.0, 0.0, 1.0, 300.0])))
    assert np.all(np.diff(k) > 0)


@pytest.mark.parametrize("kind,act", [("act", R.ACT_SIGMOID), ("act", R.ACT_TANH), ("act", R.ACT_GELU),
                                      ("gelu_fwd", None), ("gelu_grad", None)])
def test_transcription_tables(kind, act):
    ref, A, H = R.err_table(kind, GRID, act)
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(A)) and np.all(np.isfinite(H))
    assert np.all(A >= 0) and A.max() > 0 and H.max() > 0
    print(f"{kind} act={act}: max A = {A.max():.3e} at z = {GRID[A.argmax()]}, max H = {H.max():.3e}, "
          f"max (A + H) / max(|z|, 1) = {((A + H) / np.maximum(np.abs(GRID), 1)).max():.3e}")
    assert ((A + H) / np.maximum(np.abs(GRID), 1.0)).max() < 2e-6     # a few fp32 roundings, nothing more


def test_polynomial_gelu_is_erf_gelu():
    assert np.abs(R.gelu_fwd64(GRID) - R.act64(GRID, R.ACT_GELU)).max() <= 0.5 * 64 * 1.5e-7
    assert np.all(np.abs(R.gelu_fwd64(GRID) - R.act64(GRID, R.ACT_GELU)) <= 0.5 * np.abs(GRID) * 1.5e-7 + 1e-12)
    d = 1e-6
    num = (R.gelu_fwd64(GRID + d) - R.gelu_fwd64(GRID - d)) / (2 * d)
    assert np.abs(R.gelu_grad64(GRID) - num).max() < 1e-6      # continuous at 0, the derivative of the same formula


def _zs(group, kind):
    out = []
    for c in R.CASES[group]:
        if c.kind == kind and not c.gauss and c.M * c.N <= 256 * 256:
            out.append(R.exact(c).z.ravel())
    return np.unique(np.concatenate(out))


def test_mutant_erf_coefficient_leaves_the_bounds():
    """gelu_fwd_f / gelu_grad2 with 0.254829592 -> 0.254829 on the z the cases produce."""
    z = _zs("L", "ga")
    ref, E = R.pointwise("gelu_fwd", z)
    for contract in (False, True):
        bad = R.gelu_fwd_f32(z, contract, a1=0.254829).astype(np.float64)
        lo, hi = R.bf16_bracket(ref, E)
        k = R.bf16_key(R.bf16_rne(bad))
        n_fp32, n_bf16 = int(np.sum(np.abs(bad - ref) > E)), int(np.sum((k < lo) | (k > hi)))
        print(f"gelu_fwd mutant (contract={contract}): {n_fp32} of {z.size} grid points outside E, {n_bf16} outside the bf16 bracket")
        assert n_fp32 > 0
    c = next(c for c in R.CASES["L"] if c.kind == "dg" and c.bias)
    dh = R.exact(c._replace(bias=False)).z
    aux, bias = R.dg_inputs(c)
    s = aux + bias
    ref, E, *_ = R.dgelu_bounds(dh, s, c.M)
    lo, hi = R.bf16_bracket(ref, E)
    for contract in (False, True):
        bad = (dh.astype(np.float32) * R.gelu_grad2_f32(s, contract, a1=0.254829)).astype(np.float32)
        k = R.bf16_key(R.bf16_rne(bad))
        n = int(np.sum((k < lo) | (k > hi)))
        print(f"gelu_grad2 mutant (contract={contract}): {n} of {dh.size} dU outside the bf16 bracket")
        assert n > 0
        good = (dh.astype(np.float32) * R.gelu_grad2_f32(s, contract)).astype(np.float32)
        k = R.bf16_key(R.bf16_rne(good))
        assert not np.any((k < lo) | (k > hi))


def test_mutant_pdf_constant_leaves_the_bounds():
    c = next(c for c in R.CASES["L"] if c.kind == "dg" and c.bias)
    dh = R.exact(c._replace(bias=False)).z
    aux, bias = R.dg_inputs(c)
    ref, E, *_ = R.dgelu_bounds(dh, aux + bias, c.M)
    bad = (dh.astype(np.float32) * R.gelu_grad2_f32(aux + bias, pdf0=0.3989)).astype(np.float64)
    loose = E + R.HB * np.abs(ref)
    assert np.sum(np.abs(R.bf16_val(R.bf16_rne(bad)) - ref) > loose) > 0 or \
        np.sum(np.abs(bad - ref) > E) > 0.1 * bad.size
    lo, hi = R.bf16_bracket(ref, E)
    k = R.bf16_key(R.bf16_rne(bad))
    assert np.sum((k < lo) | (k > hi)) > 100


def test_mutant_truncation_leaves_the_bounds():
    for c in R.CASES["E"]:
        if c.obf and c.act >= R.ACT_SIGMOID and c.M * c.N <= 256 * 256:
            z = R.exact(c).z
            ref, E = R.pointwise("act", z, c.act)
            y = R.apply_act_slow_f32(z, c.act)
            lo, hi = R.bf16_bracket(ref, E)
            good, bad = R.bf16_key(R.bf16_rne(y)), R.bf16_key(R.bf16_trunc(y))
            assert not np.any((good < lo) | (good > hi)), c.name
            assert np.all(np.abs(R.bf16_val(R.bf16_rne(y)) - ref) <= E + R.HB * np.abs(ref)), c.name
            assert np.sum((bad < lo) | (bad > hi)) > 0.1 * z.size, c.name
            assert np.any(np.abs(R.bf16_val(R.bf16_trunc(y)) - ref) > E + R.HB * np.abs(ref)), c.name
    c = next(c for c in R.CASES["A"] if c.obf)
    z = R.exact(c).z
    assert np.mean(R.bf16_trunc(z) != R.bf16_rne(z)) > 0.05


def test_mutant_gelu_of_rounded_aux_leaves_the_bounds():
    """gelu_fwd_f applied to bf16(z): visible only where z is no bf16 number and GELU is not saturated."""
    c = next(c for c in R.CASES["L"] if c.name.startswith("Lga16"))
    z = R.exact(c).z
    assert np.mean(R.bf16_val(R.bf16_rne(z)) != z) > 0.5 and np.mean(np.abs(z) < 4) > 0.5
    ref, E = R.pointwise("gelu_fwd", z)
    lo, hi = R.bf16_bracket(ref, E)
    good = R.bf16_key(R.bf16_rne(R.gelu_fwd_f32(z)))
    bad = R.bf16_key(R.bf16_rne(R.gelu_fwd_f32(R.bf16_val(R.bf16_rne(z)))))
    assert not np.any((good < lo) | (good > hi))
    assert np.mean((bad < lo) | (bad > hi)) > 0.05
    assert R.neighbourhood_max(np.array([0.1, 0.2, 0.6, 3.0]), np.array([1.0, 5.0, 2.0, 3.0])).tolist() == [5, 5, 5, 3]


def test_groups_identical():
    keys = np.array([3, 1, 3, 2, 1])
    assert R.groups_identical(keys, np.array([7, 5, 7, 9, 5]))
    assert not R.groups_identical(keys, np.array([7, 5, 8, 9, 5]))
    assert R.groups_identical((keys, np.array([0, 0, 1, 0, 0])), np.array([7, 5, 8, 9, 5]))


@pytest.mark.parametrize("c", [c for c in R.CASES["M"] if c.kind == "gemm"], ids=lambda c: c.name)
def test_gaussian_bound_holds_for_fp32_sums_in_two_orders(c):
    a, b = R._raw_operands(c)
    R0 = 48                                                              # the first rows are enough
    ex = R.exact(c)
    ex = ex._replace(z=ex.z[:R0], magnitude=ex.magnitude[:R0], c0=None if ex.c0 is None else ex.c0[:R0])
    bound = R.gauss_bound(c._replace(obf=False), ex)
    prod = (a[:R0, :, None] * b[None, :, :]).astype(np.float32)          # exact products [R0, K, N]
    seq = np.zeros((R0, c.N), np.float32)
    for k in range(c.K):
        seq = seq + prod[:, k, :]
    pair = prod
    while pair.shape[1] > 1:
        if pair.shape[1] % 2:
            pair = np.concatenate([pair, np.zeros_like(pair[:, :1])], 1)
        pair = pair[:, 0::2] + pair[:, 1::2]
    worst = 0.0
    for s in (seq, pair[:, 0]):
        y = np.float32(c.alpha) * s
        if ex.bias is not None:
            y = y + ex.bias.astype(np.float32)
        if ex.c0 is not None:
            y = y + np.float32(c.beta) * ex.c0.astype(np.float32)
        worst = max(worst, float((np.abs(y.astype(np.float64) - ex.z) / bound).max()))
    print(f"{c.name}: worst fp32 error / bound = {worst:.3f}")
    assert worst < 0.5
