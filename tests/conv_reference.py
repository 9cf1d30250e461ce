"""Float64 model of the implicit-GEMM convolutions (csrc/kernels/conv_igemm.hip),
the operands that make their results exactly computable, and the bounds the
random tier is held to.

A helper module, not a test file: `import conv_reference` (pytest puts tests/ on
sys.path).  NumPy and CPU torch only; tests/test_conv_reference_cpu.py checks
this file against torch and against mutants, tests/test_conv_igemm_edges_gpu.py
holds the kernels to it.

Layouts.  Everything here is pixel-major, as the kernels see it: activations
[N, H, W, C] (the memory of a channels_last [N, C, H, W] tensor), filters
[K, ks, ks, C] (KRSC, channels_last [K, C, ks, ks]), the flipped filter
[C, ks, ks, K], matrices of GEMM rows [M, K] with M = N Ho Wo.  ks 3 has pad 1,
ks 1 pad 0, so Ho = (H - 1) // stride + 1 for both.

The exact tier
--------------
Operands are integer-valued bf16 and the accumulators fp32.  Every product and
every partial sum is an integer no larger than sum |x||w| (`magnitude`), which the
fixture builder asserts to be below 2^24: the accumulators are exact in any
order, on any pixel split, through slabs.  y must equal bf16_rne(z) and dW the
model, bit for bit, also added into an integer-valued prior.  Two families:

  wide    entries uniform in [-3, 3]: |z| reaches several hundred, so the bf16
          rounding of y is exercised (integers above 256 are not all bf16).
  narrow  x in {-1, 0, 1} at density 1/4, w in {-1, 0, 1} at density 1/2; the
          builder asserts max |z| <= 256 (over 3x3 x 192 channels the standard
          deviation is about 15).  Then y = z exactly, y^2 <= 2^16, and every
          128-row sum of y and y^2 is an integer below 2^24: the statistics
          partials are exact too.

BN-backward epilogues (EPI 2 / 3) on the narrow family: bn_x is an integer in
[-4, 4], scale in {-0.5, 0.5, 1, 2}, shift and the residual on a 1/8 grid, mean
on a 1/4 grid, invstd in {0.5, 1, 2}, the folded gradient an integer in [-4, 4].
The mask argument x scale + shift (+ res) is a multiple of 1/8 below 2^5, exact
with or without an fma, so the mask has no borderline; x_hat is a multiple of
1/8, g an integer, g x_hat a multiple of 1/8, and a 128-row sum of it stays
below 2^24 eighths (`bnb_magnitude` asserts all of it).  The partials are exact.

The bounded tier
----------------
randn operands rounded to bf16.  An fp32 dot product of n terms summed in any
order differs from the exact one by at most n 2^-24 sum |a||b| (to first order;
n is at most 1728 here and the bound is never approached), and the store rounds
once more to bf16:

    |y - ref|  <= n 2^-24 sum|x||w| + 2^-8 |ref|
    y in [bf16(ref - E), bf16(ref + E)],  E = n 2^-24 sum|x||w|   (monotone form)
    |dW - ref| <= (P + splits) 2^-24 sum|dy||x|  (+ one ulp of the result when
                  it is added into a prior gradient)
"""
import collections

import numpy as np
import torch

U = 2.0 ** -24
ULP = 2.0 ** -23
HB = 2.0 ** -8
BM = 128                # GEMM rows per tile
PK = 64                 # pixels per weight-gradient step

DX2_CLASSES = ((1, 1), (1, 0), (0, 1), (0, 0))   # (h % 2, w % 2) in dispatch order


# ------------------------------------------------------------------ bf16 bits

def bf16_rne(x):
    """uint16 bf16 bits of x (through fp32, exact for the exact tier): round to
    nearest, ties to even, on the bits."""
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, np.uint16(0x7FC0), r)


def bf16_val(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_round(x):
    """float64 value of x rounded to bf16."""
    return bf16_val(bf16_rne(x))


def bf16_key(bits):
    b = np.asarray(bits, dtype=np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF) - 1, b)


def bf16_bracket(ref, err):
    """Keys (lo, hi) a bf16 output lies between when its value before rounding is
    within err of ref (U |ref| more for the float64 -> fp32 step of bf16_rne)."""
    e = err + U * np.abs(ref)
    return bf16_key(bf16_rne(ref - e)), bf16_key(bf16_rne(ref + e))


def f32_bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def tensor_bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.view(torch.int32).numpy().view(np.uint32)


# --------------------------------------------------------------- float64 models

def out_size(H, stride):
    return (H - 1) // stride + 1


def _taps(x, ks, stride, pad=None):
    """x [N, H, W, C] -> {(r, s): x[n, ho st + r - pad, wo st + s - pad, :]} as [N, Ho, Wo, C], zero outside."""
    N, H, W, C = x.shape
    pad = ks // 2 if pad is None else pad
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    big = ks + 1
    xp = np.zeros((N, H + 2 * big, W + 2 * big, C), x.dtype)
    xp[:, big:big + H, big:big + W] = x
    out = {}
    for r in range(ks):
        for s in range(ks):
            h0, w0 = big + r - pad, big + s - pad
            out[r, s] = xp[:, h0:h0 + (Ho - 1) * stride + 1:stride, w0:w0 + (Wo - 1) * stride + 1:stride]
    return out


def fwd64(x, w, stride, pad=None):
    """y[n, ho, wo, k] = sum_{r,s,c} x[n, ho st + r - pad, wo st + s - pad, c] w[k][r][s][c]."""
    ks = w.shape[1]
    t = _taps(np.asarray(x, np.float64), ks, stride, pad)
    w = np.asarray(w, np.float64)
    return sum(t[r, s] @ w[:, r, s, :].T for r in range(ks) for s in range(ks))


def flip(w):
    """wt[c][ks-1-r][ks-1-s][k] = w[k][r][s][c]."""
    return np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))


def dx1_64(dy, w):
    """Input gradient of a stride-1 conv: the same convolution of dy with the flipped filter."""
    return fwd64(dy, flip(w), 1)


def dx2_64(dy, w, H, W, swap=False):
    """Input gradient of a stride-2 3x3 conv, per parity class of the input pixel:
    dx[n, h, w, c] = sum over (r, s) with h+1-r, w+1-s even, and k, of
    dy[n, (h+1-r)/2, (w+1-s)/2, k] w[k][r][s][c].  swap: the mutant that takes
    class (1,0) for (0,1)."""
    dy = np.asarray(dy, np.float64)
    w = np.asarray(w, np.float64)
    N, Hy, Wy, K = dy.shape
    C = w.shape[3]
    assert Hy == out_size(H, 2) and Wy == out_size(W, 2) and w.shape[1] == 3
    dyp = np.zeros((N, Hy + 1, Wy + 1, K))
    dyp[:, :Hy, :Wy] = dy
    dx = np.zeros((N, H, W, C))
    for ph, pw in DX2_CLASSES:
        Hc, Wc = len(range(ph, H, 2)), len(range(pw, W, 2))
        if Hc == 0 or Wc == 0:
            continue
        qh, qw = (pw, ph) if swap and ph != pw else (ph, pw)
        acc = np.zeros((N, Hc, Wc, C))
        for r in ((0, 2) if qh else (1,)):
            for s in ((0, 2) if qw else (1,)):
                dh, dw = (qh + 1 - r) // 2, (qw + 1 - s) // 2
                acc += dyp[:, dh:dh + Hc, dw:dw + Wc] @ w[:, r, s, :]
        dx[:, ph::2, pw::2] = acc
    return dx


def wgrad64(dy, x, stride, ks):
    """dW[k][r][s][c] = sum_p dy[p][k] x[n, ho st + r - pad, wo st + s - pad, c]."""
    dy = np.asarray(dy, np.float64)
    t = _taps(np.asarray(x, np.float64), ks, stride)
    K, C = dy.shape[3], x.shape[3]
    dw = np.zeros((K, ks, ks, C))
    d2 = dy.reshape(-1, K)
    for (r, s), xs in t.items():
        dw[:, r, s, :] = d2.T @ xs.reshape(-1, C)
    return dw


# --------------------------------------------------------------------- row maps

def fwd_row_pixel(m, Ho, Wo):
    """GEMM row of the forward -> (n, ho, wo)."""
    return m // (Ho * Wo), (m // Wo) % Ho, m % Wo


def fwd_tiles(M):
    """Flat pixel indices of each 128-row tile of the forward."""
    return [np.arange(t, min(t + BM, M)) for t in range(0, M, BM)]


def dx2_class_tiles(N, H, W):
    return [-(-N * len(range(ph, H, 2)) * len(range(pw, W, 2)) // BM) for ph, pw in DX2_CLASSES]


def dx2_tiles(N, H, W):
    """Flat pixel indices (n H + h) W + w of each 128-row tile of the stride-2 input
    gradient: classes in dispatch order, rows (n, h / 2, w / 2) within a class,
    each class padded to whole tiles."""
    tiles = []
    for ph, pw in DX2_CLASSES:
        n, h, w = np.meshgrid(np.arange(N), np.arange(ph, H, 2), np.arange(pw, W, 2), indexing="ij")
        pix = ((n * H + h) * W + w).reshape(-1)
        tiles += [pix[t:t + BM] for t in range(0, len(pix), BM)]
    return tiles


# --------------------------------------------------------------- epilogue models

def tile_sums(v, tiles):
    """v [Mpix, K] -> [P, K] of sums over each tile's pixels."""
    return np.stack([v[t].sum(0) for t in tiles]) if tiles else np.zeros((0, v.shape[1]))


def epi_plain(z, y_in=None):
    """bf16 bits stored: bf16(z), or with accumulate bf16(bf16(z) + y_in)."""
    v = bf16_round(z)
    return bf16_rne(v if y_in is None else v + y_in)


def epi_stats(ybits, tiles):
    """EPI 1: [2, P, K] sums of the stored y and y^2 over each tile's valid rows."""
    y = bf16_val(ybits)
    return np.stack([tile_sums(y, tiles), tile_sums(y * y, tiles)])


def epi_bnb(z, bnx, st, tiles, y_in=None, res=None):
    """EPI 2 (y_in, res None) / EPI 3.  st = [mean, invstd, scale, shift] ([4, K]).
    Returns (bits of g, [2, P, K] sums of g and g x_hat)."""
    v = bf16_round(z)
    if y_in is not None:
        v = bf16_round(v + y_in)
    mean, invstd, scale, shift = st
    arg = bnx * scale + shift + (0.0 if res is None else res)
    g = np.where(arg > 0, v, 0.0)
    gx = g * (bnx - mean) * invstd
    return bf16_rne(g), np.stack([tile_sums(g, tiles), tile_sums(gx, tiles)])


# --------------------------------------------------------------------- fixtures

def _rng(*key):
    return np.random.default_rng([abs(hash_int(k)) for k in key])


def hash_int(k):
    if isinstance(k, str):
        return sum((i + 1) * ord(ch) for i, ch in enumerate(k))
    return int(k)


def ints(rng, shape, family, what):
    """Integer operand of a family; what: 'x' (activation / gradient) or 'w'."""
    if family == "wide":
        return rng.integers(-3, 4, shape).astype(np.float64)
    assert family == "narrow"
    dens = 0.25 if what == "x" else 0.5
    return (rng.integers(0, 2, shape) * 2 - 1) * (rng.random(shape) < dens).astype(np.float64)


def magnitude(a, b, fn):
    """max over outputs of sum |a||b| through the model fn: every partial sum the
    kernel can form is an integer no larger than this."""
    return float(fn(np.abs(a), np.abs(b)).max())


def check_exact(z, mag, family):
    assert mag < 2 ** 24, mag
    assert np.array_equal(z, np.round(z))
    if family == "narrow":
        assert np.abs(z).max() <= 256, np.abs(z).max()


def bnb_fixture(rng, M, K, with_res):
    """bn_x, stats [4, K], and (EPI 3) the folded gradient and the residual, all [M, K]."""
    bnx = rng.integers(-4, 5, (M, K)).astype(np.float64)
    mean = rng.integers(-8, 9, K) / 4.0
    invstd = rng.choice([0.5, 1.0, 2.0], K)
    scale = rng.choice([-0.5, 0.5, 1.0, 2.0], K)
    shift = rng.integers(-16, 17, K) / 8.0
    st = np.stack([mean, invstd, scale, shift])
    y_in = rng.integers(-4, 5, (M, K)).astype(np.float64) if with_res else None
    res = rng.integers(-16, 17, (M, K)) / 8.0 if with_res else None
    return bnx, st, y_in, res


def bnb_magnitude(z, bnx, st, y_in, res):
    """Asserts the exactness conditions of the EPI 2 / 3 fixture."""
    mean, invstd, scale, shift = st
    arg = np.abs(bnx * scale) + np.abs(shift) + (0 if res is None else np.abs(res))
    assert np.array_equal(arg * 8, np.round(arg * 8)) and arg.max() < 32         # 8 bits below 2^5: exact in fp32 and bf16
    xh = (bnx - mean) * invstd
    assert np.array_equal(xh * 8, np.round(xh * 8))
    v = np.abs(z) + (0 if y_in is None else np.abs(y_in))
    assert np.array_equal(v, np.round(v))
    assert BM * v.max() * np.abs(xh).max() * 8 < 2 ** 24
    for a in (bnx, y_in, res):
        if a is not None:
            assert np.array_equal(bf16_round(a), a)


# ------------------------------------------------- weight-gradient plan (mirror)

Plan = collections.namedtuple("Plan", "splits sps bm bnw xcd G ws")


def wgrad_plan(N, H, W, C, K, stride, ks, wgs=0, minsteps=8, xcd_on=True):
    """Mirror of dtfk_conv_wgrad_launch_plan; the GPU tests assert the binding agrees."""
    P = N * out_size(H, stride) * out_size(W, stride)
    NC = ks * ks * C
    bm = 128 if K % 128 == 0 else 64
    if NC % 128 == 0:
        bnw = 128
    else:
        bnw = 128 if NC >= 512 and -(-NC // 128) * 128 - NC <= NC // 8 else 64
    tiles = (K // bm) * -(-NC // bnw)
    steps = -(-P // PK)
    if wgs > 0:
        target = wgs
    elif ks == 1:
        target = 256 if tiles <= 4 else 512
    else:
        target = 1024 if tiles >= 32 else 512
    splits = max(1, min(-(-target // tiles), steps // minsteps))
    sps = -(-steps // splits)
    splits = -(-steps // sps)
    use_xcd = xcd_on and 8 <= tiles <= 16
    if use_xcd and splits >= 8:
        splits = -(-splits // 8) * 8
        sps = -(-steps // splits)
    ws = splits * tiles * bm * bnw if splits > 1 else 0
    slab = ws // splits if ws else 0
    xcd = int(use_xcd and splits >= 8 and splits % 8 == 0)
    G = 1
    while G < 16 and 2 * G <= splits and (slab // 4) * G < 131072:
        G *= 2
    return Plan(splits, sps, bm, bnw, xcd, G, ws)


# ------------------------------------------------------------------- emulation
# The kernels' arithmetic in NumPy fp32, in the kernels' step order; `mutant`
# switches in one defect.  What the exact tier must tell apart from the model.

def emu_fwd(x, w, stride, mutant=None):
    """conv_fwd's accumulator: fp32, one (tap, 64-channel chunk) step after the other. -> [M, K] fp32"""
    ks = w.shape[1]
    t = _taps(np.asarray(x, np.float32), ks, stride, pad=0 if mutant == "tap" else None)
    w = np.asarray(w, np.float32)
    C = w.shape[3]
    acc = None
    for r in range(ks):
        for s in range(ks):
            for c0 in range(0, C, 64):
                step = t[r, s][..., c0:c0 + 64].reshape(-1, 64) @ w[:, r, s, c0:c0 + 64].T
                acc = step if acc is None else acc + step
    return acc


def emu_store(acc, tiles, npix, mutant=None, stats=False):
    """The epilogue: bf16 y over each tile's valid rows (NaN bits where nothing is
    stored) and, with stats, the [2, P, K] fp32 partials.  Mutants: 'lastrow'
    (the last valid row of a partial tile is not stored), 'invalid' (the rows
    past the end of a partial tile hold pixel 0's values and are summed)."""
    K = acc.shape[1]
    y = np.full((npix, K), 0x7FC0, np.uint16)
    part = np.zeros((2, len(tiles), K), np.float32)
    for i, t in enumerate(tiles):
        rows = t[:-1] if mutant == "lastrow" and len(t) < BM else t
        y[rows] = bf16_rne(acc[rows])
        if stats:
            v = bf16_val(bf16_rne(acc[t])).astype(np.float32)
            if mutant == "invalid" and len(t) < BM:
                v = np.concatenate([v, np.repeat(bf16_val(bf16_rne(acc[:1])).astype(np.float32), BM - len(t), 0)])
            part[0, i] = v.sum(0, dtype=np.float32)
            part[1, i] = (v * v).sum(0, dtype=np.float32)
    return y, part


def emu_wgrad(dy, x, stride, ks, plan, prior=None, mutant=None):
    """conv_wgrad + wgrad_reduce: per split, fp32 steps of 64 pixels; slabs summed
    by G threads (thread g: slabs g, g + G, ...) combined in g order, added into
    prior.  Mutant 'twice': the second-last slab is summed twice."""
    t = _taps(np.asarray(x, np.float32), ks, stride)
    K, C = dy.shape[3], x.shape[3]
    d2 = np.asarray(dy, np.float32).reshape(-1, K)
    xs = np.stack([t[r, s].reshape(-1, C) for r in range(ks) for s in range(ks)], 1).reshape(len(d2), -1)   # [P, ks ks C]
    P = len(d2)
    slabs = []
    for z in range(plan.splits):
        acc = np.zeros((K, xs.shape[1]), np.float32)
        for p0 in range(z * plan.sps * PK, min((z + 1) * plan.sps * PK, P), PK):
            p1 = min(p0 + PK, (z + 1) * plan.sps * PK, P)
            acc = acc + d2[p0:p1].T @ xs[p0:p1]
        slabs.append(acc)
    if mutant == "twice":
        slabs.append(slabs[max(len(slabs) - 2, 0)])
    G = plan.G if plan.splits > 1 else 1
    tot = None
    for g in range(G):
        zg = np.zeros_like(slabs[0])
        for s_ in slabs[g::G]:
            zg = zg + s_
        tot = zg if tot is None else tot + zg
    tot = tot.reshape(K, ks, ks, C)
    return tot if prior is None else (np.asarray(prior, np.float32) + tot)


# ------------------------------------------------------------------------ cases

Fwd = collections.namedtuple("Fwd", "name N H W C K stride ks bn mode family")
MODES = ("plain", "acc", "epi1", "epi2", "epi3")


def _fwd_cases():
    out = []

    def add(tag, N, H, W, C, K, stride, ks, bn, modes, families):
        for mode in modes:
            for fam in families:
                if mode in ("epi2", "epi3") and fam == "wide":     # their fixture is exact on the narrow family
                    continue
                out.append(Fwd(f"{tag}-n{N}h{H}w{W}c{C}k{K}s{stride}f{ks}b{bn}-{mode}-{fam}", N, H, W, C, K, stride, ks,
                               bn, mode, fam))

    both = ("narrow", "wide")
    # M = 1, 127, 128, 129 (a tile crossing images, and crossing rows), 257
    for N, H, W in ((1, 1, 1), (1, 1, 127), (1, 8, 16), (3, 1, 43), (1, 3, 43), (1, 1, 257)):
        add("M", N, H, W, 64, 64, 1, 3, 64, MODES, both)
    # 9, 18, 27 K steps
    for C in (128, 192):
        for N, H, W in ((3, 1, 43), (1, 3, 43)):
            add("C", N, H, W, C, 64, 1, 3, 64, MODES, both)
    # channel tiles: blockIdx.y > 0 at both widths
    for K, bn in ((128, 64), (128, 128), (192, 64), (256, 128)):
        add("K", 1, 3, 43, 64, K, 1, 3, bn, MODES, both)
    for H, W in ((1, 1), (2, 2), (5, 4), (4, 5)):
        add("S2", 2, H, W, 64, 64, 2, 3, 64, MODES, both)
    # 1x1: ONE (C = 64), two steps with the early prefetch (C = 128), three steps
    for C in (64, 128, 192):
        for stride in (1, 2):
            for bn in (64, 128):
                add("1x1", 3, 5, 9, C, 128, stride, 1, bn, MODES, both if C == 64 else ("narrow",))
    return out


FWD_CASES = _fwd_cases()

Dx2 = collections.namedtuple("Dx2", "name N H W C K bn")


def _dx2_cases():
    out = [Dx2(f"n{N}h{H}w{W}", N, H, W, 64, 64, 64) for N in (1, 2) for H in range(1, 6) for W in range(1, 6)]
    out.append(Dx2("n3h15w13", 3, 15, 13, 64, 64, 64))
    out += [Dx2(f"n2h5w4-k{K}", 2, 5, 4, 64, K, 64) for K in (128, 192)]
    out += [Dx2(f"n3h15w13-c128-bn{bn}", 3, 15, 13, 128, 64, bn) for bn in (64, 128)]
    out.append(Dx2("n2h5w4-c192", 2, 5, 4, 192, 64, 64))
    return out


DX2_CASES = _dx2_cases()

Wg = collections.namedtuple("Wg", "name N H W C K stride ks claim")   # claim: the plan fields the case is there for


def claim(splits, sps, bm, bnw, xcd, G):
    """The plan a weight-gradient case is there for, written out (not computed)."""
    return dict(splits=splits, sps=sps, bm=bm, bnw=bnw, xcd=xcd, G=G)


def _wg_cases():
    out = [
        Wg("tile128x128", 2, 6, 7, 128, 128, 1, 3, claim(1, 2, 128, 128, 0, 1)),
        Wg("tile128x64", 2, 6, 7, 64, 128, 1, 1, claim(1, 2, 128, 64, 0, 1)),
        Wg("tile64x128-partial-column-tile", 2, 6, 7, 64, 64, 1, 3, claim(1, 2, 64, 128, 0, 1)),
        Wg("tile64x64", 2, 6, 7, 64, 64, 1, 1, claim(1, 2, 64, 64, 0, 1)),
        Wg("images-per-step", 5, 3, 3, 64, 64, 1, 3, claim(1, 1, 64, 128, 0, 1)),
        Wg("wo-above-64", 1, 2, 70, 64, 64, 1, 3, claim(1, 3, 64, 128, 0, 1)),
        Wg("stride2-odd", 3, 15, 13, 64, 128, 2, 3, claim(1, 3, 128, 128, 0, 1)),
        Wg("stride2-odd-1x1", 3, 15, 13, 128, 64, 2, 1, claim(1, 3, 64, 128, 0, 1)),
        Wg("two-splits-G2", 1, 32, 32, 64, 64, 1, 1, claim(2, 8, 64, 64, 0, 2)),
        Wg("short-last-split", 1, 25, 44, 64, 64, 1, 1, claim(2, 9, 64, 64, 0, 2)),        # 1100 pixels: 18 steps, the last short
        Wg("two-splits-G1", 1, 32, 32, 256, 256, 1, 3, claim(2, 8, 128, 128, 0, 1)),
        Wg("eight-splits-G8", 1, 64, 64, 64, 64, 1, 1, claim(8, 8, 64, 64, 0, 8)),
        Wg("sixteen-splits-G16", 2, 64, 64, 64, 64, 1, 1, claim(16, 8, 64, 64, 0, 16)),
        Wg("xcd-8-splits", 4, 32, 32, 128, 128, 1, 3, claim(8, 8, 128, 128, 1, 4)),          # 9 tiles
        Wg("xcd-16-splits-one-empty", 4, 32, 36, 128, 128, 1, 3, claim(16, 5, 128, 128, 1, 4)),   # 72 steps: 9 splits -> 16
    ]
    for Wd in (1, 63, 64, 65, 129, 193, 257, 321, 385, 449):
        out.append(Wg(f"steps-w{Wd}", 1, 1, Wd, 64, 64, 1, 1, claim(1, -(-Wd // 64), 64, 64, 0, 1)))
    return out


WG_CASES = _wg_cases()


def fwd_fixture(c):
    """Operands and float64 result of a forward case: x [N,H,W,C], w [K,ks,ks,C], z [M,K], tiles."""
    rng = _rng("fwd", c.N, c.H, c.W, c.C, c.K, c.stride, c.ks, c.family)
    x = ints(rng, (c.N, c.H, c.W, c.C), c.family, "x")
    w = ints(rng, (c.K, c.ks, c.ks, c.C), c.family, "w")
    z = fwd64(x, w, c.stride)
    check_exact(z, magnitude(x, w, lambda a, b: fwd64(a, b, c.stride)), c.family)
    M = z.shape[0] * z.shape[1] * z.shape[2]
    return x, w, z.reshape(M, c.K), fwd_tiles(M), rng


def dx2_fixture(c, family):
    rng = _rng("dx2", c.N, c.H, c.W, c.C, c.K, family)
    Hy, Wy = out_size(c.H, 2), out_size(c.W, 2)
    dy = ints(rng, (c.N, Hy, Wy, c.K), family, "x")
    w = ints(rng, (c.K, 3, 3, c.C), family, "w")
    z = dx2_64(dy, w, c.H, c.W)
    check_exact(z, magnitude(dy, w, lambda a, b: dx2_64(a, b, c.H, c.W)), family)
    return dy, w, z.reshape(-1, c.C), dx2_tiles(c.N, c.H, c.W), rng


def wg_fixture(c):
    rng = _rng("wg", c.N, c.H, c.W, c.C, c.K, c.stride, c.ks)
    Ho, Wo = out_size(c.H, c.stride), out_size(c.W, c.stride)
    dy = ints(rng, (c.N, Ho, Wo, c.K), "wide", "x")
    x = ints(rng, (c.N, c.H, c.W, c.C), "wide", "x")
    prior = rng.integers(-1000, 1001, (c.K, c.ks, c.ks, c.C)).astype(np.float64)
    dw = wgrad64(dy, x, c.stride, c.ks)
    mag = magnitude(dy, x, lambda a, b: wgrad64(a, b, c.stride, c.ks))
    assert mag + 1000 < 2 ** 24 and np.array_equal(dw, np.round(dw))
    return dy, x, prior, dw


def randn_bf16(rng, shape, scale=1.0):
    """randn rounded to bf16, as float64."""
    return bf16_round(rng.standard_normal(shape) * scale)


# ------------------------------------------------------------------ torch views

def cl(a, dtype=torch.bfloat16):
    """Pixel-major [N, H, W, C] array -> the channels_last [N, C, H, W] torch tensor of that memory."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).permute(0, 3, 1, 2)


def first_mismatch(got, want, what):
    """None, or where two bit arrays [M, K] first differ."""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    if bad.size == 0:
        return None
    i = tuple(bad[0])
    return f"{what}: {len(bad)} of {np.asarray(want).size} differ; first at {i}: got 0x{int(got[i]):x}, want 0x{int(want[i]):x}"
