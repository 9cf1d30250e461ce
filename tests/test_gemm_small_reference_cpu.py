"""tests/gemm_small_reference.py against itself, without a GPU: the exact tier's
cases really are exact, the case list reaches every path of dtfk_gemm's
dispatch, tiles and K chunks are told apart, and the comparison the GPU suite
makes would catch a subtly wrong kernel -- each mutant below is applied to the
*reference* output and must be detected on at least one case of the list."""
import numpy as np
import pytest
import torch

import gemm_reference as R
import gemm_small_reference as S

INT = [c for c in S.ALL if not c.gauss]


def test_case_names_unique_and_within_the_binding_contract():
    names = [c.name for c in S.ALL]
    assert len(set(names)) == len(names)
    for c in S.ALL:
        assert c.K >= 1 and c.M >= 1 and c.N >= 1, c.name
        assert not (c.has_Z and c.exc and c.M > 1), f"{c.name}: the binding rejects Z with a padded out"
        assert c.beta in (0.0, 1.0, 0.5, 2.0), c.name
        assert np.log2(abs(c.alpha)) == round(np.log2(abs(c.alpha))), c.name
        assert c.K <= 4096, c.name


@pytest.mark.parametrize("c", INT, ids=lambda c: c.name)
def test_every_partial_sum_is_exact(c):
    ex = S.exact(c)
    assert float((ex.magnitude / ex.unit).max()) < 2 ** 24
    assert np.array_equal(ex.z / ex.unit, np.round(ex.z / ex.unit))
    assert np.array_equal(ex.z.astype(np.float32).astype(np.float64), ex.z)
    a, b = S.stored_operands(c)
    assert np.array_equal(a, np.round(a)) and np.array_equal(b, np.round(b))
    assert c.K * np.abs(a).max() * np.abs(b).max() < 2 ** 24 or float(ex.magnitude.max()) < 2 ** 24
    if c.has_Z:
        assert np.array_equal(R.f32_bits(ex.z).view(np.float32).astype(np.float64), ex.z)


def test_operand_tensors_hold_the_stored_values_in_nan_parents():
    for c in (S.CASES["I"][1], S.CASES["I"][-1], S.CASES["A"][1], S.CASES["A"][3], S.CASES["V"][2], S.CASES["W"][5]):
        A, B = S.operands(c)
        a, b = S.stored_operands(c)
        assert A.dtype == (torch.bfloat16 if c.abf else torch.float32)
        assert np.array_equal(A.double().numpy(), a.T if c.tA else a), c.name
        assert np.array_equal(B.double().numpy(), b.T if c.tB else b), c.name
        for t, ex, off in ((A, c.exa, c.offa), (B, c.exb, c.offb)):
            assert t.stride() == (t.shape[1] + ex, 1) and t.storage_offset() == 8 + off
            assert int(torch.isnan(t._base).sum()) == t._base.numel() - t.numel()


def test_plan_reaches_every_path():
    got = {}
    for c in S.ALL:
        for label in S.paths(c):
            got.setdefault(label, []).append(c.name)
    missing = S.required_paths() - set(got)
    assert not missing, missing
    # exact-tier cases alone reach them too (the bounded tier adds no path)
    got_exact = {label for c in S.EXACT for label in S.paths(c)}
    assert not S.required_paths() - got_exact
    for label in sorted(got, key=str):
        print(label, len(got[label]))


def test_tile_and_tail_values_reach_each_mfma_kernel_in_each_layout():
    """Group T: for every (kernel that plan names, layout) the M, N and K seen
    cover the lists.  The one exception: fp32 x fp32 -> fp32 with N = 1 and no
    transA always goes to the row-form matrix-vector kernel, so N = 1 cannot
    reach the f32 MFMA kernel in those two layouts (group V covers the row form)."""
    seen = {}
    for c in S.CASES["T"]:
        s = seen.setdefault((S.plan_of(c).kernel, c.tA, c.tB), (set(), set(), set()))
        s[0].add(c.M), s[1].add(c.N), s[2].add(c.K)
    for kern, Ks in (("bf16", S.K_BF16), ("f32", S.K_F32)):
        for tA, tB in S.LAYOUTS:
            Ms, Ns, Kk = seen[(kern, tA, tB)]
            want_N = set(S.MN) - ({1} if kern == "f32" and not tA else set())
            assert set(S.MN) <= Ms, (kern, tA, tB, sorted(set(S.MN) - Ms))
            assert want_N <= Ns, (kern, tA, tB, sorted(want_N - Ns))
            assert set(Ks) <= Kk, (kern, tA, tB, sorted(set(Ks) - Kk))
            if kern == "f32" and not tA:
                assert 1 not in Ns
    # the diverted N = 1 cases do run, on the row form
    assert seen[("gemv_rows", False, True)][1] == {1} and seen[("gemv_rows", False, False)][1] == {1}


def test_plan_mirrors_the_dispatch_at_known_points():
    P = S.plan
    assert P(37, 53, 512, 1, 1, 0, 0, 1, 0, 0.0, False)[:5] == ("bf16", 1, 2, 2, 256)
    assert P(37, 53, 520, 1, 1, 0, 0, 1, 0, 1.0, False)[:5] == ("bf16", 1, 2, 2, 288)
    assert P(37, 53, 777, 0, 0, 0, 0, 1, 0, 0.0, False)[:5] == ("f32", 1, 3, 3, 288)
    assert P(37, 53, 1024, 0, 0, 0, 1, 0, 0, 0.0, False)[:5] == ("f32", 1, 4, 4, 256)
    assert P(37, 53, 3073, 1, 1, 0, 0, 1, 0, 0.0, False)[:5] == ("bf16", 1, 11, 12, 288)
    assert P(257, 257, 520, 1, 1, 0, 0, 1, 0, 0.0, False)[:5] == ("bf16", 25, 2, 2, 288)
    for kw in (dict(beta=0.5), dict(c_bf16=1), dict(act=1), dict(has_Z=True)):
        args = dict(M=37, N=53, K=520, a_bf16=1, b_bf16=1, c_bf16=0, tA=0, tB=1, act=0, beta=0.0, has_Z=False)
        args.update(kw)
        assert P(**args).split == 1, kw
    assert P(511, 1, 100, 0, 0, 0, 0, 1, 2, 0.5, True).kernel == "gemv_rows"
    assert P(130, 1, 1000, 0, 0, 0, 1, 0, 0, 1.0, False)[-2:] == (16, 63)
    assert P(64, 1, 64, 0, 0, 0, 1, 0, 0, 0.0, False)[-2:] == (1, 64)
    assert P(65, 1, 65, 0, 0, 0, 1, 0, 0, 0.0, False)[-2:] == (2, 33)
    assert P(1, 1, 130, 0, 0, 0, 1, 0, 0, 0.0, False)[-2:] == (3, 44)
    assert P(65, 1, 65, 0, 0, 0, 1, 0, 0, 0.5, False).kernel == "f32"
    assert P(65, 1, 65, 0, 0, 0, 1, 0, 3, 0.0, False).kernel == "f32"
    assert P(65, 1, 65, 0, 0, 0, 1, 0, 0, 0.0, True).kernel == "f32"
    assert P(65, 1, 65, 1, 0, 0, 1, 0, 0, 0.0, False).kernel == "bf16"
    assert P(0, 5, 7, 0, 0, 0, 0, 1, 0, 0.0, False).kernel == "none"
    # the list holds a split whose recomputed factor is below the first estimate, and split >= 4, and ragged last chunks
    pl = [S.plan_of(c) for c in S.CASES["S"]]
    assert any(p.split < p.split_est for p in pl) and any(p.split >= 4 for p in pl)
    for kern, step in (("bf16", 32), ("f32", 16)):
        assert any(p.kernel == kern and (c.K - (p.split - 1) * p.kchunk) % step for p, c in zip(pl, S.CASES["S"]))
    assert all(S.plan_of(c).split == 1 for c in S.CASES["U"])
    assert all(S.plan_of(c).kernel == "f32" for c in S.CASES["X"])
    assert {S.plan_of(c).tiles for c in S.CASES["R"]} == {1, 7, 8, 9, 15, 17, 25}
    assert {S.plan_of(c).tiles for c in S.CASES["R"] if S.plan_of(c).split > 1} == {1, 7, 8, 9, 15, 17, 25}


def test_tiles_and_k_chunks_are_told_apart():
    """No two 64x64 tiles of z agree on their common part, and no two K chunks
    have the same partial product: swapping or doubling one is visible."""
    for c in S.EXACT:
        p = S.plan_of(c)
        if p.tiles > 1 and p.kernel in ("bf16", "f32"):
            z = S.exact(c).z
            tiles = [z[i:i + 64, j:j + 64] for i in range(0, c.M, 64) for j in range(0, c.N, 64)]
            for i in range(len(tiles)):
                for j in range(i + 1, len(tiles)):
                    r, q = (min(a, b) for a, b in zip(tiles[i].shape, tiles[j].shape))
                    if r * q >= 4:
                        assert not np.array_equal(tiles[i][:r, :q], tiles[j][:r, :q]), (c.name, i, j)
        if max(p.split, p.gy) > 1 and c.M * c.N >= 4:
            part = S.chunk_partials(c)
            assert np.array_equal(part.sum(0) + (S.exact(c).z - c.alpha * np.matmul(*S.effective_operands(c))),
                                  S.exact(c).z), c.name
            for i in range(len(part)):
                assert np.any(part[i] != 0), (c.name, i)
                for j in range(i + 1, len(part)):
                    assert not np.array_equal(part[i], part[j]), (c.name, i, j)


def test_wide_family_needs_fp32_operands_and_bf16_cases_need_rounding():
    n = 0
    for c in S.EXACT:
        if c.fam == "wide" and c.K >= 4 and min(c.M, c.N) * c.K >= 60:     # enough entries for chance not to matter
            a, b = S._drawn(c)
            assert np.any(S._rb(a) != a) and np.any(S._rb(b) != b), c.name
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
            n += 1
    assert n > 50
    for c in S.CASES["I"]:
        if c.obf and c.fam == "int":
            z = S.exact(c).z
            assert 0.1 <= float(np.mean(R.bf16_val(R.bf16_rne(z)) != z)) <= 0.9, c.name
    for c in S.CASES["E"]:
        if c.obf and c.beta != 0.0:
            z = S.exact(c).z
            assert float(np.mean(R.bf16_val(R.bf16_rne(z)) != z)) >= 0.2, c.name


def test_reference_passes_its_own_checks():
    for c in S.EXACT[::7]:
        ex = S.exact(c)
        wc, wz = S.want_bits(c, ex)
        assert S.check_exact(c, ex, wc, wz) is None
    for c in S.BOUNDED[::5]:
        ex = S.exact(c)
        ref, E = R.pointwise("act", ex.z, c.act)
        y = R.apply_act_slow_f32(ex.z, c.act)
        bits = R.bf16_rne(y) if c.obf else R.f32_bits(y)
        msg, fig = S.check_bounded(c, bits, ref, E, S.keys_of(ex), trans=y)
        assert msg is None, msg
        assert all(v <= 1.0 for k, v in fig.items() if k != "differ")


# ---------------------------------------------------------------------- mutants

def _detected(mutant, cases):
    """The names of the cases on which check_exact sees the mutant.  mutant(c, ex)
    returns (C bits, Z bits) or None when it does not apply to c."""
    hit = []
    for c in cases:
        ex = S.exact(c)
        out = mutant(c, ex)
        if out is None:
            continue
        msg = S.check_exact(c, ex, *out)
        if msg is not None:
            assert c.name in msg and "first (m=" in msg
            hit.append(c.name)
    return hit


def _bits_of(c, z):
    return R.expected_bits(R.act64(z, c.act), c.obf), (R.f32_bits(z) if c.has_Z else None)


def test_mutant_last_k_dropped():
    def mutant(c, ex):
        return _bits_of(c, S.exact(c, None, True).z) if c.K > 1 else None
    cases = S.CASES["T"] + S.CASES["S"] + S.CASES["V"] + S.CASES["W"]
    cases = [c for c in cases if c.act <= 1 and c.M * c.N >= 16]
    hit = set(_detected(mutant, cases))
    for c in cases:                  # on every fp32 output (a bf16 C can round a small difference away)
        if c.K > 1 and not c.obf and min(c.M, c.N) >= 15:     # a single b[K - 1] can be 0 by chance
            assert c.name in hit, c.name
    assert len(hit) >= 0.9 * len([c for c in cases if c.K > 1])


def test_mutant_last_row_or_column_of_a_ragged_tile_zeroed():
    def row(c, ex):
        z = ex.z.copy()
        z[-1, :] = 0.0
        return _bits_of(c, z) if c.M % 64 else None

    def col(c, ex):
        z = ex.z.copy()
        z[:, -1] = 0.0
        return _bits_of(c, z) if c.N % 64 else None
    cases = [c for c in S.CASES["T"] if c.K >= 7 and min(c.M, c.N) >= 15]
    assert len(_detected(row, cases)) >= 0.9 * len([c for c in cases if c.M % 64])
    assert len(_detected(col, cases)) >= 0.9 * len([c for c in cases if c.N % 64])


def test_mutant_two_tiles_swapped():
    def mutant(c, ex):
        if S.plan_of(c).tiles < 2 or S.plan_of(c).kernel not in ("bf16", "f32"):
            return None
        z = ex.z.copy()
        i, j = (64, 0) if c.M > 64 else (0, 64)
        r, q = min(64, c.M - i), min(64, c.N - j)
        z[:r, :q], z[i:i + r, j:j + q] = ex.z[i:i + r, j:j + q], ex.z[:r, :q]
        return _bits_of(c, z)
    cases = S.CASES["R"] + [c for c in S.CASES["T"] if c.K >= 7]
    hit = _detected(mutant, cases)
    assert len(hit) == len([c for c in cases if mutant(c, S.exact(c)) is not None]) and len(hit) > 40


def test_mutant_bias_added_by_every_split_chunk():
    def mutant(c, ex):
        p = S.plan_of(c)
        n = max(p.split, p.gy)
        return _bits_of(c, ex.z + (n - 1) * ex.bias) if c.bias and n > 1 else None
    hit = _detected(mutant, S.CASES["S"] + S.CASES["R"] + S.CASES["W"])
    assert any(n.startswith("S-") and "-bbf" in n for n in hit) and any(n.startswith("S-") and "-fff" in n for n in hit)
    assert any(n.startswith("W-") for n in hit) and any(n.startswith("R-") for n in hit)


def test_mutant_beta_applied_when_zero():
    """With beta = 0 the C view is NaN before the call: a kernel that reads it returns NaN."""
    def mutant(c, ex):
        return _bits_of(c, ex.z + np.nan) if c.beta == 0.0 else None
    cases = [c for c in S.CASES["E"] + S.CASES["V"] + S.CASES["W"] + S.CASES["S"] if c.act <= 1]
    hit = _detected(mutant, cases)
    assert len(hit) == len([c for c in cases if c.beta == 0.0]) and len(hit) >= 60


def test_mutant_bf16_truncation_instead_of_rne():
    def mutant(c, ex):
        return (R.bf16_trunc(R.act64(ex.z, c.act)), R.f32_bits(ex.z) if c.has_Z else None) if c.obf else None
    cases = [c for c in S.CASES["I"] + S.CASES["E"] + S.CASES["T"] if c.obf and c.M * c.N >= 64 and c.K >= 7]
    assert len(_detected(mutant, cases)) >= 0.9 * len(cases)


def test_mutant_fp32_operand_rounded_to_bf16_on_the_f32_path():
    def mutant(c, ex):
        if S.rounds_operands(c) or c.fam != "wide" or c.K < 4:
            return None
        return _bits_of(c, S.exact(c, True).z)
    hit = _detected(mutant, S.EXACT)
    for group in "IESVWX":           # both MFMA layouts, split-K, and both matrix-vector kernels
        assert any(n.startswith(group + "-") for n in hit), group
    # and the reverse: on mixed / bf16-output paths the unrounded product is wrong

    def reverse(c, ex):
        if not S.rounds_operands(c) or c.fam != "wide" or (c.abf and c.bbf):
            return None
        return _bits_of(c, S.exact(c, False).z)
    assert len(_detected(reverse, S.CASES["I"])) == 4 * 5


def test_mutant_z_taken_after_the_activation():
    def mutant(c, ex):
        if not (c.has_Z and c.act == R.ACT_RELU):
            return None
        return R.expected_bits(R.act64(ex.z, c.act), c.obf), R.f32_bits(R.act64(ex.z, c.act))
    hit = _detected(mutant, S.EXACT)
    assert any(n.startswith("Z-") for n in hit) and any(n.startswith("V") for n in hit)
    # the bounded tier checks Z bit for bit too: act(z) is not z
    for c in S.BOUNDED:
        if c.has_Z and c.M * c.N >= 9:
            ex = S.exact(c)
            assert S.first_mismatch(c, R.f32_bits(R.apply_act_slow_f32(ex.z, c.act)), R.f32_bits(ex.z), "Z") is not None


def test_mutant_gemv_ldbk_taken_as_one():
    """b(k) read at B[k] instead of B[k * ldb]: the stride-3 view's parent is NaN between the elements."""
    def mutant(c, ex):
        if c.N != 1 or c.tB or c.exb == 0 or c.K < 2:
            return None
        _, B = S.operands(c)
        flat = B._base.double().numpy()[B.storage_offset():B.storage_offset() + c.K]
        a, _ = S.effective_operands(c)
        bias = 0.0 if ex.bias is None else ex.bias
        c0 = 0.0 if ex.c0 is None else c.beta * ex.c0
        return _bits_of(c, c.alpha * (a @ flat[:, None]) + bias + c0)
    for group in "VW":
        cases = [c for c in S.CASES[group] if c.act <= 1]
        hit = _detected(mutant, cases)
        assert len(hit) == len([c for c in cases if not c.tB and c.exb and c.K >= 2]) and len(hit) >= 10


def test_mutant_activation_formula_leaves_the_bound():
    """A sigmoid built on a wrong constant (log2 e to 4 digits) and a tanh-GELU
    in place of the erf-GELU fall outside E on the cases' own z."""
    for c in S.BOUNDED:
        if c.obf or c.M * c.N < 64:
            continue
        ex = S.exact(c)
        ref, E = R.pointwise("act", ex.z, c.act)
        z = ex.z.astype(np.float32)
        if c.act == R.ACT_SIGMOID:
            bad = (1.0 / (1.0 + np.exp2(-z.astype(np.float64) * 1.4427))).astype(np.float32)
        elif c.act == R.ACT_GELU:
            z64 = z.astype(np.float64)
            bad = (0.5 * z64 * (1.0 + np.tanh(0.7978845608 * (z64 + 0.044715 * z64 ** 3)))).astype(np.float32)
        else:
            continue
        msg, _ = S.check_bounded(c, R.f32_bits(bad), ref, E, S.keys_of(ex))
        assert msg is not None and "outside E" in msg, c.name


def test_locate_names_tile_wave_fragment_and_chunk():
    c = next(c for c in S.CASES["S"] if c.M == 70 and not c.abf)
    s = S.locate(c, 69, 129)
    assert "tile=(1,2) = #5 of 6" in s and "wave=(0,0)" in s and "fragment=(0,0)" in s and "lane=17 reg=1" in s
    assert "2 k-chunks of 288 (last 232)" in s
    s = S.locate(c, 47, 100)
    assert "tile=(0,1)" in s and "wave=(1,1)" in s and "fragment=(0,0)" in s and "lane=52 reg=3" in s
    ex = S.exact(c)
    wc, _ = S.want_bits(c, ex)
    part = S.chunk_partials(c)
    msg = S.first_mismatch(c, R.f32_bits(ex.z + part[1]), wc)
    assert "k-chunk 1's partial product (added twice)" in msg
    msg = S.first_mismatch(c, R.f32_bits(ex.z - part[0]), wc)
    assert "k-chunk 0's partial product (missing)" in msg
    assert "gemv_cols block.x=2 lane=1, 16 k-chunks of 63 (last 55)" in S.locate(
        next(c for c in S.CASES["W"] if c.M == 130 and c.K == 1000), 129, 0)
    assert "gemv_rows block=2 wave=0" in S.locate(next(c for c in S.CASES["V"] if c.M == 9), 8, 0)


@pytest.mark.parametrize("c", S.GAUSS, ids=lambda c: c.name)
def test_gaussian_bound_holds_for_fp32_sums_in_two_orders(c):
    """A sequential and a pairwise fp32 sum of rounded fp32 products stay well
    inside the bound; the reference really is the product of the rounded operands."""
    a, b = S.effective_operands(c)
    R0 = min(c.M, 24)
    ex = S.exact(c)
    ex = ex._replace(z=ex.z[:R0], magnitude=ex.magnitude[:R0], c0=None if ex.c0 is None else ex.c0[:R0])
    bound = S.gauss_bound(c._replace(obf=False), ex)
    prod = (a[:R0, :, None].astype(np.float32) * b[None, :, :].astype(np.float32))
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
    if S.rounds_operands(c) and not (c.abf and c.bbf):     # the unrounded product is outside the fp32-level bound
        a0, b0 = S.stored_operands(c)
        z0 = c.alpha * (a0 @ b0)[:R0] + (ex.z - c.alpha * (a @ b)[:R0])
        assert np.mean(np.abs(z0 - ex.z) > bound) > 0.5
