"""csrc/kernels/conv_igemm.hip per element, at the smallest shapes where each of its
paths exists: conv_fwd (3x3 / 1x1, stride 1 / 2, both channel-tile widths, the
single-step variant, plain / accumulate / statistics / BN-backward / residual
BN-backward epilogues), its stride-2 input-gradient form over the four parity
classes, conv_wgrad + wgrad_reduce over the tile pairs, step counts, splits,
reduce groups and the XCD dispatch, and the two filter flips.

Reference, fixtures and bounds: tests/conv_reference.py (float64 on the CPU; its
own checks, with the mutants these fixtures tell apart, are in
tests/test_conv_reference_cpu.py).  Two tiers:

* exact: integer-valued bf16 operands -- every partial sum is an integer below
  2^24, so y equals bf16_rne(z), dW equals the model added into an integer prior,
  and on the narrow family the statistics and BN-backward partials equal the
  model, all bit for bit.  No tolerance.
* bounded: randn operands against float64 within the derived bounds of
  conv_reference.py, and bit-identical repeats.

Every output is a view inside a larger sentinel-filled buffer and is NaN before
the call unless the kernel is to read it; afterwards every sentinel bit is
unchanged.  Every weight-gradient case asserts, through conv_wgrad_plan, the
plan it is there for.

Measured on an MI355X (the whole file: 13 s), worst |error| / bound of the bounded
tier; 1.0 would be a failure.  y: 0.80 (3x3), 0.77 (3x3 stride 2), 0.95 (1x1), dx
of the stride-2 gradient 0.96 -- that is the bf16 store reaching half an ulp,
the 2^-8 |ref| term; dW 0.001 - 0.015.  The exact tier has no figure: it is equal
or it fails.

The paths chosen by environment variables that are read once per process run in
a fresh child each: `python tests/test_conv_igemm_edges_gpu.py child NAME` is the
body of test_env_selected_path[NAME].
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_reference as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = {torch.float32: -7777.25, torch.bfloat16: -7744.0}
MARGIN = 256          # elements; a multiple of 8 bf16 / 4 fp32: the middle stays 16-byte aligned


def _sync():
    """A fault of an earlier launch surfaces here and is sticky: end the session
    rather than launch more work on a faulted device."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, stopping the session: {e}", returncode=3)


def _ibits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Guard:
    """numel elements between two sentinel margins: NaN, or `init` (flat, in memory order)."""

    def __init__(self, numel, dtype, init=None):
        self.n = numel
        self.pre = torch.full((numel + 2 * MARGIN,), SENT[dtype], dtype=dtype)
        mid = self.pre[MARGIN:MARGIN + numel]
        if init is None:
            mid.fill_(float("nan"))
        else:
            mid.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)).to(dtype))
        self.dev = self.pre.cuda()

    def flat(self):
        return self.dev[MARGIN:MARGIN + self.n]

    def cl(self, N, C, H, W):
        """channels_last [N, C, H, W] view of the middle."""
        return self.dev.as_strided((N, C, H, W), (H * W * C, 1, W * C, C), MARGIN)

    def nchw(self, N, C, H, W):
        return self.dev.as_strided((N, C, H, W), (C * H * W, H * W, W, 1), MARGIN)

    def finish(self, name):
        """Bits of the middle after the call; asserts that the margins kept theirs."""
        _sync()
        post = self.dev.cpu()
        for sl in (slice(0, MARGIN), slice(MARGIN + self.n, None)):
            bad = (_ibits(post[sl]) != _ibits(self.pre[sl])).nonzero()
            assert bad.numel() == 0, f"{name}: {bad.numel()} sentinel elements were overwritten; first at {int(bad[0])} of margin {sl}"
        return R.tensor_bits(post[MARGIN:MARGIN + self.n])

    def unchanged(self):
        _sync()
        return torch.equal(_ibits(self.dev.cpu()), _ibits(self.pre))


def _dev(a):
    return R.cl(a).cuda()


def _f32dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().cuda()


def _same(got, want, what):
    msg = R.first_mismatch(got, want, what)
    assert msg is None, msg


def _part_rows(got, want, name, exact=(True, True), scale=None):
    """[2, P, K] partials tile by tile; exact[t]: bit for bit, else within scale[t]."""
    for t, q in ((0, "first"), (1, "second")):
        for p in range(want.shape[1]):
            if exact[t]:
                _same(R.f32_bits(got[t, p]).reshape(1, -1), R.f32_bits(want[t, p]).reshape(1, -1),
                      f"{name}: {q} partial of tile {p}")
            else:
                err = np.abs(got[t, p].astype(np.float64) - want[t, p])
                assert np.all(err <= scale[t][p]), f"{name}: {q} partial of tile {p} off by {err.max()} (bound {scale[t][p].max()})"


# ---------------------------------------------------------------- forward

def run_fwd(native, c):
    x, w, z, tiles, rng = R.fwd_fixture(c)
    M, K = z.shape
    P = len(tiles)
    Ho, Wo = R.out_size(c.H, c.stride), R.out_size(c.W, c.stride)
    assert native.conv3x3_tiles(c.N, c.H, c.W, c.stride) == P
    bnx = st = y_in = res = None
    if c.mode in ("epi2", "epi3"):
        bnx, st, y_in, res = R.bnb_fixture(rng, M, K, c.mode == "epi3")
        R.bnb_magnitude(z, bnx, st, y_in, res)
    elif c.mode == "acc":
        y_in = rng.integers(-4, 5, (M, K)).astype(np.float64)
    yb = Guard(M * K, torch.bfloat16, init=y_in)
    pb = Guard(2 * P * K, torch.float32) if c.mode.startswith("epi") else None
    shp = (c.N, Ho, Wo, K)
    native.conv3x3_fwd(_dev(x), _dev(w), yb.cl(c.N, K, Ho, Wo), None if pb is None else pb.flat(), c.stride, c.bn,
                       c.mode in ("acc", "epi3"), None if bnx is None else _dev(bnx.reshape(shp)),
                       None if st is None else _f32dev(st), None if res is None else _dev(res.reshape(shp)))
    got = yb.finish(c.name + " y").reshape(M, K)
    if c.mode in ("epi2", "epi3"):
        want, wpart = R.epi_bnb(z, bnx, st, tiles, y_in, res)
    else:
        want = R.epi_plain(z, y_in)
        wpart = R.epi_stats(want, tiles) if c.mode == "epi1" else None
    _same(got, want, f"{c.name}: y (row = n, ho, wo of the output; column = channel)")
    if pb is not None:
        gp = pb.finish(c.name + " part").view(np.float32).reshape(2, P, K)
        if c.family == "narrow":
            assert np.abs(wpart).max() < 2 ** 24
            _part_rows(gp, wpart, c.name)
        else:       # sum y is an integer below 2^24; sum y^2 is not: 128 fp32 additions of exact squares
            _part_rows(gp, wpart, c.name, exact=(True, False), scale=(None, R.BM * R.U * wpart[1]))


@pytest.mark.parametrize("c", R.FWD_CASES, ids=lambda c: c.name)
def test_forward_exact(native, c):
    run_fwd(native, c)


# ------------------------------------------------- stride-2 input gradient

def run_dx2(native, c, family, modes=("plain", "acc", "epi2")):
    dy, w, z, tiles, rng = R.dx2_fixture(c, family)
    Mpix, C = z.shape
    P = len(tiles)
    assert native.conv3x3_dx2_tiles(c.N, c.H, c.W) == P == sum(R.dx2_class_tiles(c.N, c.H, c.W))
    d_dy, d_wt = _dev(dy), _dev(R.flip(w))
    assert native.conv3x3_dx2_supported(d_dy, _dev(w), c.H, c.W)
    for mode in modes:
        name = f"dx2 {c.name} {family} {mode}"
        y_in = rng.integers(-4, 5, (Mpix, C)).astype(np.float64) if mode == "acc" else None
        bnx = st = None
        if mode == "epi2":
            bnx, st, _, _ = R.bnb_fixture(rng, Mpix, C, False)
            R.bnb_magnitude(z, bnx, st, None, None)
        out = Guard(Mpix * C, torch.bfloat16, init=y_in)
        pb = Guard(2 * P * C, torch.float32) if mode == "epi2" else None
        native.conv3x3_dx2(d_dy, d_wt, out.cl(c.N, C, c.H, c.W), None if pb is None else pb.flat(), c.bn, mode == "acc",
                           None if bnx is None else _dev(bnx.reshape(c.N, c.H, c.W, C)),
                           None if st is None else _f32dev(st))
        got = out.finish(name).reshape(Mpix, C)
        if mode == "epi2":
            want, wpart = R.epi_bnb(z, bnx, st, tiles)
            _same(got, want, f"{name}: dx (row = pixel (n H + h) W + w)")
            _part_rows(pb.finish(name + " part").view(np.float32).reshape(2, P, C), wpart, name)
        else:
            _same(got, R.epi_plain(z, y_in), f"{name}: dx (row = pixel (n H + h) W + w)")


@pytest.mark.parametrize("c", R.DX2_CASES, ids=lambda c: c.name)
def test_dx2_exact(native, c):
    run_dx2(native, c, "narrow")
    run_dx2(native, c, "wide", modes=("plain",))


# ---------------------------------------------------------- weight gradient

def _plan(native, c):
    return R.Plan(*native.conv_wgrad_plan(c.N, c.H, c.W, c.C, c.K, c.stride, c.ks))


def _dw_guard(prior, kcrs):
    """prior [K, ks, ks, C] -> (guard, [K, C, ks, ks] view) in the contiguous (kcrs) or channels_last layout."""
    K, ks, _, C = prior.shape
    if kcrs:
        g = Guard(prior.size, torch.float32, init=prior.transpose(0, 3, 1, 2))
        return g, g.nchw(K, C, ks, ks)
    g = Guard(prior.size, torch.float32, init=prior)
    return g, g.cl(K, C, ks, ks)


def run_wg(native, c, mirror_kw=None):
    plan = _plan(native, c)
    assert plan == R.wgrad_plan(c.N, c.H, c.W, c.C, c.K, c.stride, c.ks, **(mirror_kw or {})), (c.name, plan)
    got = plan._asdict()
    assert {k: got[k] for k in c.claim} == c.claim, f"{c.name}: the plan is {plan}, the case is there for {c.claim}"
    dy, x, prior, dw = R.wg_fixture(c)
    d_dy, d_x = _dev(dy), _dev(x)
    want = prior + dw
    for kcrs in (0, 1):
        g, view = _dw_guard(prior, kcrs)
        native.conv3x3_wgrad(d_dy, d_x, view, c.stride)
        bits = g.finish(f"{c.name} kcrs={kcrs}")
        w = want.transpose(0, 3, 1, 2) if kcrs else want
        _same(bits.reshape(c.K, -1), R.f32_bits(w).reshape(c.K, -1),
              f"{c.name}: dW, {'KCRS' if kcrs else 'KRSC'} layout (row = output channel), plan {plan}")


@pytest.mark.parametrize("c", R.WG_CASES, ids=lambda c: c.name)
def test_wgrad_exact(native, c):
    run_wg(native, c)


def test_wgrad_plan_is_read_only_and_refuses(native):
    assert native.conv_wgrad_plan(4, 32, 32, 128, 128, 1, 3) == (8, 8, 128, 128, 1, 4, 8 * 9 * 128 * 128)
    assert native.conv_wgrad_plan(1, 1, 1, 64, 64, 1, 1) == (1, 1, 64, 64, 0, 1, 0)
    for bad in ((1, 4, 4, 64, 64, 0, 3), (1, 4, 4, 64, 64, 3, 3), (1, 4, 4, 96, 64, 1, 3), (1, 4, 4, 64, 64, 1, 2)):
        with pytest.raises(RuntimeError):
            native.conv_wgrad_plan(*bad)


# ------------------------------------------------------------ bounded tier

def _bounded_y(bits, ref, E, name):
    y = R.bf16_val(bits)
    assert np.all(np.isfinite(y)), f"{name}: non-finite output"
    bad = np.argwhere(np.abs(y - ref) > E + R.HB * np.abs(ref))
    assert bad.size == 0, f"{name}: {len(bad)} outside n 2^-24 sum|a||b| + 2^-8 |ref|; first {tuple(bad[0])}"
    lo, hi = R.bf16_bracket(ref, E)
    k = R.bf16_key(bits)
    bad = np.argwhere((k < lo) | (k > hi))
    assert bad.size == 0, f"{name}: {len(bad)} outside [bf16(ref - E), bf16(ref + E)]; first {tuple(bad[0])}"
    print(f"RATIO {name}: worst |y - ref| / bound = {(np.abs(y - ref) / (E + R.HB * np.abs(ref) + 1e-300)).max():.3f}")


@pytest.mark.parametrize("ks,stride,bn", [(3, 1, 0), (3, 2, 128), (1, 1, 64)])
def test_forward_random_bounded_and_repeatable(native, ks, stride, bn):
    N, H, W, C, K = 1, 3, 43, 192, 128
    rng = np.random.default_rng(ks * 10 + stride)
    x = R.randn_bf16(rng, (N, H, W, C))
    w = R.randn_bf16(rng, (K, ks, ks, C), (2.0 / (ks * ks * C)) ** 0.5)
    Ho, Wo = R.out_size(H, stride), R.out_size(W, stride)
    M = N * Ho * Wo
    ref = R.fwd64(x, w, stride).reshape(M, K)
    E = ks * ks * C * R.U * R.fwd64(np.abs(x), np.abs(w), stride).reshape(M, K)
    tiles = R.fwd_tiles(M)
    runs = []
    for rep in range(2):
        yb, pb = Guard(M * K, torch.bfloat16), Guard(2 * len(tiles) * K, torch.float32)
        native.conv3x3_fwd(_dev(x), _dev(w), yb.cl(N, K, Ho, Wo), pb.flat(), stride, bn)
        runs.append((yb.finish("y"), pb.finish("part")))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "two runs differ"
    bits = runs[0][0].reshape(M, K)
    _bounded_y(bits, ref, E, f"forward ks={ks} stride={stride}")
    gp = runs[0][1].view(np.float32).reshape(2, len(tiles), K).astype(np.float64)
    y = R.bf16_val(bits)
    want, mag = R.epi_stats(bits, tiles), R.tile_sums(np.abs(y), tiles)
    # of the values the kernel stored: at most 128 fp32 additions, each within U of the running sum of magnitudes
    assert np.all(np.abs(gp[0] - want[0]) <= R.BM * R.U * mag), "sum y partials"
    assert np.all(np.abs(gp[1] - want[1]) <= (R.BM + 1) * R.U * want[1]), "sum y^2 partials"


def test_dx2_random_bounded(native):
    N, H, W, C, K = 3, 15, 13, 64, 128
    rng = np.random.default_rng(3)
    dy = R.randn_bf16(rng, (N, R.out_size(H, 2), R.out_size(W, 2), K))
    w = R.randn_bf16(rng, (K, 3, 3, C), (2.0 / (9 * K)) ** 0.5)
    ref = R.dx2_64(dy, w, H, W).reshape(-1, C)
    E = 4 * K * R.U * R.dx2_64(np.abs(dy), np.abs(w), H, W).reshape(-1, C)       # at most 4 taps x K channels
    out = Guard(ref.size, torch.bfloat16)
    native.conv3x3_dx2(_dev(dy), _dev(R.flip(w)), out.cl(N, C, H, W))
    _bounded_y(out.finish("dx").reshape(-1, C), ref, E, "dx2")


@pytest.mark.parametrize("name", ["short-last-split", "xcd-16-splits-one-empty", "tile64x128-partial-column-tile"])
def test_wgrad_random_bounded_and_repeatable(native, name):
    c = next(c for c in R.WG_CASES if c.name == name)
    plan = _plan(native, c)
    assert {k: plan._asdict()[k] for k in c.claim} == c.claim
    rng = np.random.default_rng(len(name))
    Ho, Wo = R.out_size(c.H, c.stride), R.out_size(c.W, c.stride)
    dy = R.randn_bf16(rng, (c.N, Ho, Wo, c.K))
    x = R.randn_bf16(rng, (c.N, c.H, c.W, c.C))
    prior = rng.standard_normal((c.K, c.ks, c.ks, c.C)).astype(np.float32).astype(np.float64)
    ref = prior + R.wgrad64(dy, x, c.stride, c.ks)
    E = (c.N * Ho * Wo + plan.splits) * R.U * R.wgrad64(np.abs(dy), np.abs(x), c.stride, c.ks) + R.ULP * np.abs(ref)
    runs = []
    for rep in range(2):
        g, view = _dw_guard(prior, 0)
        native.conv3x3_wgrad(_dev(dy), _dev(x), view, c.stride)
        runs.append(g.finish(name))
    assert np.array_equal(runs[0], runs[1]), "two runs differ"
    got = runs[0].view(np.float32).reshape(ref.shape).astype(np.float64)
    assert np.all(np.isfinite(got))
    r = np.abs(got - ref) / (E + 1e-300)
    print(f"RATIO wgrad {name}: {r.max():.3f}")
    assert r.max() <= 1.0, f"{name}: dW off by {r.max():.3f} of its bound at {np.unravel_index(r.argmax(), r.shape)}"


# ------------------------------------------------------------ filter flips

def _rand_filter(K, C, ks, seed):
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(0, 2 ** 15, (K, ks, ks, C), generator=g).to(torch.int16)      # any bit pattern: the kernels copy
    return bits.view(torch.bfloat16).permute(0, 3, 1, 2)                                # channels_last [K, C, ks, ks]


def _flip_want(w):
    return _ibits(w.flip(2, 3).transpose(0, 1).contiguous())                            # [C, K, ks, ks]


FLIPS = [(K, C, ks) for ks in (1, 3) for K, C in ((64, 64), (64, 192), (192, 64), (128, 256))]


@pytest.mark.parametrize("K,C,ks", FLIPS)
def test_wflip_is_the_torch_permutation(native, K, C, ks):
    w = _rand_filter(K, C, ks, K + C + ks)
    out = Guard(w.numel(), torch.bfloat16)
    native.conv3x3_wflip(w.cuda(), out.cl(C, K, ks, ks))
    out.finish("wt")
    assert torch.equal(_ibits(out.cl(C, K, ks, ks).cpu().contiguous()), _flip_want(w))


def test_wflip_multi_is_the_torch_permutation(native):
    shapes = FLIPS + [(96, 64, 3), (64, 96, 1), (96, 160, 3)]       # 96, 160: partial 64 x 64 tiles
    ws, outs, rows, tiles = [], [], [], []
    for i, (K, C, ks) in enumerate(shapes):
        w = _rand_filter(K, C, ks, 100 + i).cuda()
        assert w.is_contiguous(memory_format=torch.channels_last)
        out = Guard(w.numel(), torch.bfloat16)
        ws.append(w)
        outs.append(out)
        rows.append([w.data_ptr(), out.flat().data_ptr(), K, C, ks])
        tiles += [[i, rs, k0, c0] for rs in range(ks * ks) for k0 in range(0, K, 64) for c0 in range(0, C, 64)]
    native.conv_wflip_multi(torch.tensor(rows, dtype=torch.int64).cuda(), torch.tensor(tiles, dtype=torch.int32).cuda())
    for (K, C, ks), w, out in zip(shapes, ws, outs):
        out.finish(f"wt {K}x{C}x{ks}")
        assert torch.equal(_ibits(out.cl(C, K, ks, ks).cpu().contiguous()), _flip_want(w.cpu())), (K, C, ks)


# -------------------------------------------------------------- refusals

def _fwd_args(N=1, C=64, H=4, W=4, K=64, ks=3, Ho=None, Wo=None):
    x = torch.ones((N, H, W, C), dtype=torch.bfloat16).permute(0, 3, 1, 2).cuda()
    w = torch.ones((K, ks, ks, C), dtype=torch.bfloat16).permute(0, 3, 1, 2).cuda()
    Ho, Wo = Ho or H, Wo or W
    y = Guard(N * Ho * Wo * K, torch.bfloat16)
    return x, w, y, y.cl(N, K, Ho, Wo)


@pytest.mark.parametrize("stride", [0, 3, -1])
def test_refuses_stride(native, stride):
    x, w, y, yv = _fwd_args()
    assert native.conv3x3_supported(x, w, stride) is False
    with pytest.raises(RuntimeError, match="stride"):
        native.conv3x3_fwd(x, w, yv, None, stride)
    dw = Guard(64 * 64 * 9, torch.float32)
    with pytest.raises(RuntimeError, match="stride"):
        native.conv3x3_wgrad(yv, x, dw.nchw(64, 64, 3, 3), stride)
    assert y.unchanged() and dw.unchanged()


@pytest.mark.parametrize("C,K,bn", [(96, 64, 0), (64, 96, 0), (32, 64, 0), (64, 192, 128)])
def test_refuses_channel_counts_and_tile_width(native, C, K, bn):
    x, w, y, yv = _fwd_args(C=C, K=K)
    with pytest.raises(RuntimeError):
        native.conv3x3_fwd(x, w, yv, None, 1, bn)
    if bn == 0:
        assert native.conv3x3_supported(x, w, 1) is False
        dw = Guard(K * C * 9, torch.float32)
        with pytest.raises(RuntimeError):
            native.conv3x3_wgrad(yv, x, dw.nchw(K, C, 3, 3), 1)
        assert dw.unchanged()
    assert y.unchanged()


def test_refuses_dx2_tile_width_and_part_without_bn_x(native):
    N, H, W, C, K = 1, 4, 4, 192, 64
    dy = torch.ones((N, 2, 2, K), dtype=torch.bfloat16).permute(0, 3, 1, 2).cuda()
    wt = torch.ones((C, 3, 3, K), dtype=torch.bfloat16).permute(0, 3, 1, 2).cuda()
    dx = Guard(N * H * W * C, torch.bfloat16)
    part = Guard(2 * native.conv3x3_dx2_tiles(N, H, W) * C, torch.float32)
    with pytest.raises(RuntimeError):
        native.conv3x3_dx2(dy, wt, dx.cl(N, C, H, W), None, 128)               # 128 does not divide 192
    with pytest.raises(RuntimeError, match="bn_x"):
        native.conv3x3_dx2(dy, wt, dx.cl(N, C, H, W), part.flat())
    assert dx.unchanged() and part.unchanged()


def test_refuses_residual_without_accumulate_and_statistics_with_accumulate(native):
    x, w, y, yv = _fwd_args()
    part = Guard(2 * 1 * 64, torch.float32)
    like = torch.ones((1, 4, 4, 64), dtype=torch.bfloat16).permute(0, 3, 1, 2).cuda()
    st = torch.ones(4 * 64).cuda()
    with pytest.raises(RuntimeError):
        native.conv3x3_fwd(x, w, yv, part.flat(), 1, 0, False, like, st, like)       # bn_res without accumulate
    with pytest.raises(RuntimeError):
        native.conv3x3_fwd(x, w, yv, part.flat(), 1, 0, True, like, st, None)        # accumulate without bn_res
    with pytest.raises(RuntimeError):
        native.conv3x3_fwd(x, w, yv, None, 1, 0, True, None, None, like)             # bn_res without bn_x
    # statistics of the convolution alone would be handed on as those of y + conv
    with pytest.raises(RuntimeError, match="accumulate"):
        native.conv3x3_fwd(x, w, yv, part.flat(), 1, 0, True)
    assert y.unchanged() and part.unchanged()


# ----------------------------------- the env-selected paths, one fresh child each

def _case(cases, name):
    return next(c for c in cases if c.name == name)


def _child_fwd_xcd(native):
    """DTF_CONV_FWD_XCD=1: one pixel tile (7 surplus workgroups per channel tile return
    early) and nine (the grid rounds up to 16), two channel tiles, every epilogue."""
    for N, H, W in ((1, 1, 127), (1, 9, 127)):
        for ks, C in ((3, 64), (1, 64), (1, 128)):
            for bn in (64, 128):
                for mode in R.MODES:
                    yield R.Fwd(f"xcd-n{N}h{H}w{W}c{C}f{ks}b{bn}-{mode}", N, H, W, C, 128, 1, ks, bn, mode, "narrow"), None


def _child_wgrad(names, **mirror_kw):
    def gen(native):
        for n in names:
            yield _case(R.WG_CASES, n), mirror_kw
    return gen


_STEPS = [c.name for c in R.WG_CASES if c.name.startswith("steps-")]
_MANY = [R.Wg("many-64x128", 2, 6, 7, 64, 64, 1, 3, R.claim(2, 1, 64, 128, 0, 2)),
         R.Wg("many-one-step", 5, 3, 3, 64, 64, 1, 3, R.claim(1, 1, 64, 128, 0, 1)),
         R.Wg("many-stride2", 3, 15, 13, 64, 128, 2, 3, R.claim(3, 1, 128, 128, 0, 2)),
         R.Wg("many-xcd", 2, 16, 16, 128, 128, 1, 3, R.claim(8, 1, 128, 128, 1, 4)),
         R.Wg("many-G16", 1, 32, 32, 64, 64, 1, 1, R.claim(16, 1, 64, 64, 0, 16))]
# the two XCD shapes in plain split-major order: 8 splits stay 8, 9 are not rounded up to 16
_NO_XCD = [R.Wg("no-xcd-8-splits", 4, 32, 32, 128, 128, 1, 3, R.claim(8, 8, 128, 128, 0, 4)),
           R.Wg("no-xcd-9-splits", 4, 32, 36, 128, 128, 1, 3, R.claim(9, 8, 128, 128, 0, 4))]

CHILDREN = {
    "fwd_xcd": ({"DTF_CONV_FWD_XCD": "1"}, _child_fwd_xcd),
    "wgrad_depth2": ({"DTF_CONV_WGRAD_DEPTH": "2"},
                     _child_wgrad(_STEPS + ["tile128x128", "tile128x64", "tile64x64", "xcd-8-splits", "stride2-odd"])),
    "wgrad_no_xcd": ({"DTF_CONV_XCD": "0"}, lambda native: ((c, dict(xcd_on=False)) for c in _NO_XCD)),
    "wgrad_many_splits": ({"DTF_CONV_WGRAD_MINSTEPS": "1", "DTF_CONV_WGRAD_WGS": "64"},
                          lambda native: ((c, dict(wgs=64, minsteps=1)) for c in _MANY)),
}


def _child(which):
    env, gen = CHILDREN[which]
    assert all(os.environ.get(k) == v for k, v in env.items())
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    from distributed_tensorflow_example_amd import _native
    native = _native.load()
    ran, failed = 0, []
    for c, kw in gen(native):
        try:
            if isinstance(c, R.Fwd):
                run_fwd(native, c)
            else:
                run_wg(native, c, kw)
        except AssertionError as e:
            failed.append([c.name, str(e)[:400]])
        ran += 1
    print(json.dumps({"ok": not failed, "ran": ran, "failed": failed}))
    return 0 if not failed else 1


@pytest.mark.parametrize("which", list(CHILDREN))
def test_env_selected_path(which):
    env = dict(os.environ, **CHILDREN[which][0])
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", which], env=env, cwd=REPO, timeout=300,
                       capture_output=True, text=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    out = json.loads(lines[-1])
    assert not out["failed"], out["failed"]
    assert p.returncode == 0 and out["ok"] and out["ran"] >= 2, (p.returncode, out, p.stderr[-2000:])


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "child":
        sys.exit(_child(sys.argv[2]))
    sys.exit("usage: test_conv_igemm_edges_gpu.py child NAME")
