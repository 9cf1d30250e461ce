"""tests/conv_reference.py against itself and against torch: the float64 models
against float64 conv2d under autograd, the flip against the torch permutation,
the stride-2 class and row maps against a brute-force enumeration, bf16_rne
against torch's rounding, the weight-gradient plan mirror at the plans the GPU
tests claim, an fp32 / bf16 emulation of the kernels against both tiers, and
six mutants that the exact fixtures of tests/test_conv_igemm_edges_gpu.py must
tell apart from the model."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_reference as R


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


# ---- bf16 rounding

def test_bf16_rne_is_torchs_rounding():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-6, 6, 20000),
                        np.arange(-2100, 2100, dtype=np.float64),                    # integers: ties above 256
                        np.array([0.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, np.inf, -np.inf, 3.3895e38])])
    want = R.tensor_bits(torch.from_numpy(v.astype(np.float32)).bfloat16())
    assert np.array_equal(R.bf16_rne(v), want)
    assert list(R.bf16_round(np.array([257.0, 259.0, 261.0]))) == [256.0, 260.0, 260.0]   # ties to even


# ---- the models against float64 autograd

SHAPES = [(2, 5, 7, 8, 6, 1, 3), (3, 5, 4, 8, 6, 2, 3), (2, 4, 5, 8, 6, 2, 3), (1, 1, 1, 8, 6, 2, 3), (2, 2, 2, 8, 8, 2, 3),
          (2, 5, 7, 8, 6, 1, 1), (3, 5, 4, 8, 6, 2, 1), (1, 1, 9, 8, 8, 1, 3)]


@pytest.mark.parametrize("N,H,W,C,K,stride,ks", SHAPES)
def test_models_match_float64_autograd(N, H, W, C, K, stride, ks):
    rng = np.random.default_rng(N * 100 + H * 10 + W + stride)
    x = rng.standard_normal((N, H, W, C))
    w = rng.standard_normal((K, ks, ks, C))
    Ho, Wo = R.out_size(H, stride), R.out_size(W, stride)
    dy = rng.standard_normal((N, Ho, Wo, K))
    xt, wt = _nchw(x).requires_grad_(True), _nchw(w).requires_grad_(True)
    y = F.conv2d(xt, wt, None, stride, ks // 2)
    assert y.shape == (N, K, Ho, Wo)
    y.backward(_nchw(dy))
    np.testing.assert_allclose(R.fwd64(x, w, stride), _nhwc(y.detach()), rtol=0, atol=1e-12)
    np.testing.assert_allclose(R.wgrad64(dy, x, stride, ks), _nhwc(wt.grad), rtol=0, atol=1e-12)
    if stride == 1:
        np.testing.assert_allclose(R.dx1_64(dy, w), _nhwc(xt.grad), rtol=0, atol=1e-12)
    elif ks == 3:
        np.testing.assert_allclose(R.dx2_64(dy, w, H, W), _nhwc(xt.grad), rtol=0, atol=1e-12)


@pytest.mark.parametrize("K,C,ks", [(4, 6, 3), (6, 4, 1), (5, 5, 3)])
def test_flip_is_the_torch_permutation(K, C, ks):
    w = np.random.default_rng(K).standard_normal((K, ks, ks, C))
    want = _nchw(w).flip(2, 3).transpose(0, 1)                 # [C, K, ks, ks]
    got = R.flip(w)
    assert np.array_equal(got, _nhwc(want))
    for c in range(C):
        for r in range(ks):
            for s in range(ks):
                assert np.array_equal(got[c, ks - 1 - r, ks - 1 - s], w[:, r, s, c])


# ---- row maps

@pytest.mark.parametrize("N", [1, 2, 70])
def test_dx2_maps_match_enumeration(N):
    for H in range(1, 6):
        for W in range(1, 6):
            want_tiles, counts = [], []
            for ph, pw in ((1, 1), (1, 0), (0, 1), (0, 0)):
                rows = [(n * H + h) * W + w for n in range(N) for h in range(H) for w in range(W)
                        if h % 2 == ph and w % 2 == pw]
                counts.append((len(rows) + 127) // 128)
                want_tiles += [rows[i:i + 128] for i in range(0, len(rows), 128)]
            got = R.dx2_tiles(N, H, W)
            assert R.dx2_class_tiles(N, H, W) == counts and len(got) == sum(counts)
            assert [list(map(int, t)) for t in got] == want_tiles
            assert sorted(int(p) for t in got for p in t) == list(range(N * H * W))     # every pixel once


def test_forward_row_map():
    Ho, Wo = 3, 43
    for m in (0, 42, 43, 128, 257):
        n, ho, wo = R.fwd_row_pixel(m, Ho, Wo)
        assert (n * Ho + ho) * Wo + wo == m and ho < Ho and wo < Wo
    t = R.fwd_tiles(129)
    assert len(t) == 2 and len(t[0]) == 128 and list(t[1]) == [128]


# ---- the plan mirror at the plans the GPU cases claim

def test_plan_mirror_gives_the_claimed_plans():
    for c in R.WG_CASES:
        p = R.wgrad_plan(c.N, c.H, c.W, c.C, c.K, c.stride, c.ks)._asdict()
        assert {k: p[k] for k in c.claim} == c.claim, (c.name, p)
    p = R.wgrad_plan(4, 32, 32, 128, 128, 1, 3)
    assert p == R.Plan(8, 8, 128, 128, 1, 4, 8 * 9 * 128 * 128)
    p = R.wgrad_plan(4, 32, 36, 128, 128, 1, 3)
    assert p.splits == 16 and -(-72 // p.sps) == 15              # 72 steps in 16 splits of 5: the last is empty
    assert R.wgrad_plan(4, 32, 32, 128, 128, 1, 3, xcd_on=False).xcd == 0
    many = R.wgrad_plan(2, 6, 7, 64, 64, 1, 3, wgs=64, minsteps=1)
    assert many.splits == 2 and many.sps == 1                     # 84 pixels: two steps, one per split


# ---- the emulation meets both tiers

def _uniq(cases, key):
    seen = {}
    for c in cases:
        seen.setdefault(key(c), c)
    return list(seen.values())


FWD_SHAPES = _uniq(R.FWD_CASES, lambda c: (c.N, c.H, c.W, c.C, c.K, c.stride, c.ks, c.family))


@pytest.mark.parametrize("c", FWD_SHAPES, ids=lambda c: c.name)
def test_emulation_is_exact_forward(c):
    x, w, z, tiles, _ = R.fwd_fixture(c)
    acc = R.emu_fwd(x, w, c.stride)
    assert np.array_equal(acc.astype(np.float64), z)
    y, part = R.emu_store(acc, tiles, len(z), stats=True)
    want = R.epi_plain(z)
    assert np.array_equal(y, want)
    ws = R.epi_stats(want, tiles)
    assert np.array_equal(R.f32_bits(part[0]), R.f32_bits(ws[0]))
    if c.family == "narrow":
        assert np.array_equal(R.bf16_val(want), z)               # y = z: nothing is rounded
        assert np.array_equal(R.f32_bits(part[1]), R.f32_bits(ws[1]))
        assert ws[1].max() < 2 ** 24


@pytest.mark.parametrize("c", R.WG_CASES, ids=lambda c: c.name)
def test_emulation_is_exact_wgrad(c):
    dy, x, prior, dw = R.wg_fixture(c)
    plan = R.wgrad_plan(c.N, c.H, c.W, c.C, c.K, c.stride, c.ks)
    got = R.emu_wgrad(dy, x, c.stride, c.ks, plan, prior)
    assert np.array_equal(R.f32_bits(got), R.f32_bits(prior + dw))


def test_bnb_fixture_is_exact():
    c = next(c for c in R.FWD_CASES if c.mode == "epi3" and c.C == 192)
    x, w, z, tiles, rng = R.fwd_fixture(c)
    bnx, st, y_in, res = R.bnb_fixture(rng, len(z), c.K, True)
    R.bnb_magnitude(z, bnx, st, y_in, res)
    bits, part = R.epi_bnb(z, bnx, st, tiles, y_in, res)
    assert np.array_equal(part.astype(np.float32).astype(np.float64), part)
    # the same in fp32, fma or not: the mask argument and every product are exact
    arg32 = (bnx.astype(np.float32) * st[2].astype(np.float32) + st[3].astype(np.float32)) + res.astype(np.float32)
    assert np.array_equal(arg32.astype(np.float64), bnx * st[2] + st[3] + res)
    frac = (arg32 > 0).mean()
    assert 0.2 < frac < 0.8 and (arg32 == 0).any()                # both branches, and the borderline itself


def test_emulation_is_inside_the_bounded_tier():
    rng = np.random.default_rng(5)
    x = R.randn_bf16(rng, (1, 3, 43, 192))
    w = R.randn_bf16(rng, (128, 3, 3, 192), (2.0 / 1728) ** 0.5)
    ref = R.fwd64(x, w, 1).reshape(-1, 128)
    E = 1728 * R.U * R.fwd64(np.abs(x), np.abs(w), 1).reshape(-1, 128)
    acc = R.emu_fwd(x, w, 1)
    assert np.all(np.abs(acc - ref) <= E)
    bits = R.bf16_rne(acc)
    assert np.all(np.abs(R.bf16_val(bits) - ref) <= E + R.HB * np.abs(ref))
    lo, hi = R.bf16_bracket(ref, E)
    k = R.bf16_key(bits)
    assert np.all((k >= lo) & (k <= hi))
    dy = R.randn_bf16(rng, (1, 25, 44, 64))
    xx = R.randn_bf16(rng, (1, 25, 44, 64))
    plan = R.wgrad_plan(1, 25, 44, 64, 64, 1, 1)
    prior = rng.standard_normal((64, 1, 1, 64)).astype(np.float32).astype(np.float64)
    dref = R.wgrad64(dy, xx, 1, 1)
    E = (1100 + plan.splits) * R.U * R.wgrad64(np.abs(dy), np.abs(xx), 1, 1)
    got = R.emu_wgrad(dy, xx, 1, 1, plan, prior).astype(np.float64)
    assert np.all(np.abs(got - (prior + dref)) <= E + R.ULP * np.abs(prior + dref))


# ---- mutants: each defect is visible at the fixtures the GPU tests use

def _fails(flags, what):
    assert any(flags), f"mutant '{what}' passes every fixture"
    return sum(flags)


def test_mutant_flip_without_channel_transpose():
    flags = []
    for c in FWD_SHAPES:
        if c.ks == 3 and c.stride == 1 and c.C == c.K:
            rng = np.random.default_rng(c.N + c.W)
            dy = R.ints(rng, (c.N, c.H, c.W, c.K), c.family, "x")
            w = R.ints(rng, (c.K, 3, 3, c.C), c.family, "w")
            good = R.epi_plain(R.dx1_64(dy, w))
            bad = R.epi_plain(R.fwd64(dy, np.ascontiguousarray(w[:, ::-1, ::-1, :]), 1))
            flags.append(not np.array_equal(good, bad))
    assert len(flags) >= 6 and all(flags)


def test_mutant_tap_off_by_one():
    flags = []
    for c in FWD_SHAPES:
        if c.ks == 3:
            x, w, z, tiles, _ = R.fwd_fixture(c)
            y, _ = R.emu_store(R.emu_fwd(x, w, c.stride, mutant="tap"), tiles, len(z))
            flags.append(not np.array_equal(y, R.epi_plain(z)))
    assert all(flags) and len(flags) >= 20


def test_mutant_parity_classes_swapped():
    flags = []
    for c in R.DX2_CASES:
        dy, w, z, tiles, _ = R.dx2_fixture(c, "narrow")
        bad = R.dx2_64(dy, w, c.H, c.W, swap=True).reshape(z.shape)
        differs = not np.array_equal(R.epi_plain(bad), R.epi_plain(z))
        if c.H >= 2 or c.W >= 2:                                   # a (1,0) or (0,1) pixel exists
            assert differs, c.name
        flags.append(differs)
    _fails(flags, "swap")


def _partial(c):
    M = c.N * R.out_size(c.H, c.stride) * R.out_size(c.W, c.stride)
    return M % R.BM != 0


def test_mutant_last_valid_row_dropped():
    flags = []
    for c in FWD_SHAPES:
        x, w, z, tiles, _ = R.fwd_fixture(c)
        y, _ = R.emu_store(R.emu_fwd(x, w, c.stride), tiles, len(z), mutant="lastrow")
        differs = not np.array_equal(y, R.epi_plain(z))
        assert differs == _partial(c), c.name
        flags.append(differs)
    _fails(flags, "lastrow")


def test_mutant_invalid_rows_counted():
    flags = []
    for c in FWD_SHAPES:
        if c.family != "narrow":
            continue
        x, w, z, tiles, _ = R.fwd_fixture(c)
        _, part = R.emu_store(R.emu_fwd(x, w, c.stride), tiles, len(z), mutant="invalid", stats=True)
        want = R.epi_stats(R.epi_plain(z), tiles)
        differs = not np.array_equal(R.f32_bits(part), R.f32_bits(want))
        assert differs == (_partial(c) and bool(np.any(z[0] != 0))), c.name
        flags.append(differs)
    assert _fails(flags, "invalid") >= 10


def test_mutant_split_summed_twice():
    flags = []
    for c in R.WG_CASES:
        dy, x, prior, dw = R.wg_fixture(c)
        plan = R.wgrad_plan(c.N, c.H, c.W, c.C, c.K, c.stride, c.ks)
        got = R.emu_wgrad(dy, x, c.stride, c.ks, plan, prior, mutant="twice")
        flags.append(not np.array_equal(R.f32_bits(got), R.f32_bits(prior + dw)))
    assert all(flags)
