"""Float64 model of the generic GEMM (csrc/kernels/gemm.hip: the 64x64-tile bf16
and exact-f32 MFMA kernels and the two N = 1 matrix-vector kernels behind
dtfk_gemm), the operands that make its result exactly computable, the bounds its
inexact epilogues are held to, and the list of cases.

A helper module, not a test file: `import gemm_small_reference`.  It builds on
tests/gemm_reference.py (bf16 bit helpers, embed / on, act64, the error tables,
groups_identical) and adds what this kernel family needs.  NumPy and CPU torch
only; tests/test_gemm_small_reference_cpu.py checks this file against itself,
tests/test_gemm_edges_gpu.py holds the kernels to it.

The exact tier
--------------
As in gemm_reference.py: integer-valued operands with K max|a| max|b| < 2^24,
alpha a power of two, bias and C0 on a power-of-two grid, beta in {0, 1, 0.5, 2},
and (|alpha| sum|a||b| + |bias| + |beta C0|) / unit < 2^24 per element (asserted
per case on the CPU).  Every partial sum is then an integer multiple of `unit`
below 2^24 units, exact in fp32 in any order: on the 16x16x32 bf16 and the
16x16x4 f32 MFMA, over any K split, through atomics, and in the matrix-vector
kernels' two-accumulators-plus-wave_sum and four-groups-plus-atomics orders.
An fp32 C, and Z, equal z bit for bit; a bf16 C equals bf16_rne(act(z)).

Two operand families:
  int   integers in [-rng, rng]: exact in bf16, valid for every instantiation.
  wide  the same, with a sparse set of entries replaced by +-{257, 259, 514, 518,
        1023}: exact in fp32, not bf16 numbers (three of them exact ties).  A
        carries them at k % 4 == 1 and B at k % 4 == 3, so no product has two
        of them and the magnitude condition holds.  dtfk_gemm's rule is: fp32 x
        fp32 into an fp32 C never rounds an operand (exact-f32 MFMA, or a
        matrix-vector kernel); every other combination converts both operands
        to bf16, round to nearest even.  `exact` applies that rule from the
        dtypes alone, so the wide family proves which path ran.

Operands are drawn from a seeded generator, independently per element, so every
64x64 tile of z and every K chunk's partial product differs from every other
(asserted on the CPU): a mis-mapped, swapped or doubled tile or chunk cannot
cancel.

The bounded tier
----------------
gemm.hip's apply_act is, formula for formula, gemm_big.hip's apply_act_slow:
    relu     fmaxf(z, 0.f)                                   (exact)
    sigmoid  1.f / (1.f + __expf(-z))
    tanh     tanhf(z)
    gelu     0.5f * z * (1.f + erff(z * 0.70710678118654752f))
so gemm_reference.apply_act_slow_f32 is its transcription and
gemm_reference.pointwise("act", z, act) gives (act64(z), E = A + H + FLOOR)
unchanged; nothing here is fitted.  A bf16 C is also held to the monotone
bracket [bf16(ref - E), bf16(ref + E)], and outputs with the same exact z must
have the same bits.

Gaussian operands (`gauss_bound`): with t = sum_k a_k b_k computed in fp32 in
any order, every product is rounded at most once (relative U; exact for bf16
operands, and an fma only removes roundings) and every partial sum once, so by
the standard dot-product bound |t_fp32 - t| <= gamma_K sum|a||b| with gamma_K =
K U / (1 - K U); alpha t, + bias and + beta C0 are three more roundings of
values bounded by `magnitude`.  Hence |z_fp32 - z| <= (K + 3) U magnitude to
first order.  gemm_reference.gauss_bound is 2 (K + 2) U magnitude (+ 2^-8 |z|
for a bf16 C), which is larger for every K >= 1 and also covers the second-order
terms and the MFMA's internal accumulation order; it is used as it is.  Where
the kernel rounds operands to bf16, the reference is the product of the
*rounded* operands.

`plan` mirrors dtfk_gemm's dispatch on the host.  It labels cases and lets the
CPU test assert that the list reaches every path; it never takes part in an
expected value.
"""
import collections
import functools
import zlib

import numpy as np
import torch

import gemm_reference as R

ACT_NAMES = {R.ACT_NONE: "none", R.ACT_RELU: "relu", R.ACT_SIGMOID: "sigmoid", R.ACT_TANH: "tanh", R.ACT_GELU: "gelu"}
ACTS = tuple(ACT_NAMES)
BM = BN = 64
WIDE = np.array([257.0, 259.0, 514.0, 518.0, 1023.0])

_FIELDS = ("name group fam M N K tA tB abf bbf obf alpha beta bias act has_Z exa offa exb offb exc coff rng seed gauss "
           "kind scale")
Case = collections.namedtuple("Case", _FIELDS)


def case(group, M, N, K, tA=False, tB=True, abf=True, bbf=True, obf=False, alpha=1.0, beta=0.0, bias=False, act=0,
         has_Z=False, exa=0, offa=0, exb=0, offb=0, exc=0, coff=0, rng=None, fam="int", seed=None):
    """exa / exb / exc: elements added to the leading dimension of A / B / C
    (ld = cols + ex).  offa / offb / coff: elements the view starts after a
    16-byte aligned address.  rng: operand integers are uniform in [-rng, rng]:
    11 for a linear bf16 C at short K (most z then need rounding), else 3.
    seed: cases that must see the same operands pass the same seed."""
    if rng is None:
        rng = 11 if (obf and act <= R.ACT_RELU and K <= 129) else 3
    dt = "".join("b" if x else "f" for x in (abf, bbf, obf))
    full = f"{group}-{M}x{N}x{K}-{'T' if tA else 'N'}{'T' if tB else 'N'}-{dt}"
    if fam != "int":
        full += "-" + fam
    for tag, val, default in (("alpha", alpha, 1.0), ("beta", beta, 0.0), ("bias", int(bias), 0),
                              ("exa", exa, 0), ("offa", offa, 0), ("exb", exb, 0), ("offb", offb, 0), ("exc", exc, 0),
                              ("coff", coff, 0)):
        if val != default:
            full += f"-{tag}{val:g}"
    if act:
        full += "-" + ACT_NAMES[act]
    if has_Z:
        full += "-Z"
    if seed is None:
        seed = zlib.crc32(full.encode())
    return Case(full, group, fam, M, N, K, tA, tB, abf, bbf, obf, float(alpha), float(beta), bool(bias), act, has_Z,
                exa, offa, exb, offb, exc, coff, rng, seed, fam == "gauss", "gemm", 1.0)


# ------------------------------------------------------------------- dispatch

Plan = collections.namedtuple("Plan", "kernel tiles split split_est kchunk gy kc")


def plan(M, N, K, a_bf16, b_bf16, c_bf16, tA, tB, act, beta, has_Z):
    """dtfk_gemm's dispatch: the kernel ('none' | 'gemv_rows' | 'gemv_cols' |
    'f32' | 'bf16'), the split-K factor (split_est: before it is recomputed from
    the rounded chunk), the chunk, and the column form's grid.y / chunk."""
    tiles = ((M + BM - 1) // BM) * ((N + BN - 1) // BN)
    if tiles == 0:
        return Plan("none", 0, 1, 1, K, 0, 0)
    f32 = not (a_bf16 or b_bf16 or c_bf16)
    if f32 and N == 1:
        if not tA:
            return Plan("gemv_rows", tiles, 1, 1, K, 0, 0)
        if act == R.ACT_NONE and not has_Z and beta in (0.0, 1.0):
            bx = (M + 63) // 64
            gy = max(1, min((K + 63) // 64, 512 // bx))
            kc = (K + gy - 1) // gy
            gy = (K + kc - 1) // kc
            return Plan("gemv_cols", tiles, 1, 1, K, gy, kc)
    split, est, kchunk = 1, 1, K
    if act == R.ACT_NONE and not has_Z and not c_bf16 and beta in (0.0, 1.0) and tiles < 256 and K >= 512:
        split = (512 + tiles - 1) // tiles
        if split > K // 256:
            split = K // 256
        est = split
        if split > 1:
            kchunk = ((K + split - 1) // split + 31) // 32 * 32
            split = (K + kchunk - 1) // kchunk
        if split <= 1:
            split, kchunk = 1, K
    if f32 and split > 1:
        kchunk = (kchunk + 15) // 16 * 16
    return Plan("f32" if f32 else "bf16", tiles, split, est, kchunk, 0, 0)


def plan_of(c):
    return plan(c.M, c.N, c.K, c.abf, c.bbf, c.obf, c.tA, c.tB, c.act, c.beta, c.has_Z)


def paths(c):
    """The labels of the paths case c takes, for the coverage accounting: the
    kernel instantiation, and split / unsplit per MFMA kernel and layout."""
    p = plan_of(c)
    if p.kernel == "gemv_rows":
        return [("gemv_rows",)]
    if p.kernel == "gemv_cols":
        return [("gemv_cols", min(p.gy, 4))]          # gy classes 1, 2, 3, 4 and more
    how = "split" if p.split > 1 else "unsplit"
    if p.kernel == "f32":
        return [("f32", c.tA, c.tB), ("f32", how, c.tA, c.tB)]
    return [("bf16", c.abf, c.bbf, c.tA, c.tB, c.obf), ("bf16", how, c.tA, c.tB)]


def rounds_operands(c):
    """dtfk_gemm's documented rule, from the dtypes alone: only fp32 x fp32 into
    an fp32 C keeps fp32 operands; everything else multiplies bf16 values."""
    return c.abf or c.bbf or c.obf


# ------------------------------------------------------------------- operands

def _rb(x):
    return R.bf16_val(R.bf16_rne(x))


@functools.lru_cache(maxsize=16)
def _drawn(c):
    """float64 A' [M, K] and B' [K, N] as drawn, before any storage rounding."""
    g = np.random.default_rng(c.seed)
    if c.gauss:
        a = g.standard_normal((c.M, c.K)) * c.K ** -0.5
        b = g.standard_normal((c.K, c.N)) * c.K ** -0.5
        return a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    a = g.integers(-c.rng, c.rng + 1, (c.M, c.K)).astype(np.float64)
    b = g.integers(-c.rng, c.rng + 1, (c.K, c.N)).astype(np.float64)
    if c.fam == "wide":
        k = np.arange(c.K)
        wa = (k % 4 == 1)[None, :] & (g.random((c.M, c.K)) < 0.5)
        wb = (k % 4 == 3)[:, None] & (g.random((c.K, c.N)) < 0.5)
        a = np.where(wa, g.choice(WIDE, (c.M, c.K)) * g.choice([-1.0, 1.0], (c.M, c.K)), a)
        b = np.where(wb, g.choice(WIDE, (c.K, c.N)) * g.choice([-1.0, 1.0], (c.K, c.N)), b)
    return a, b


def stored_operands(c):
    """float64 A' and B' as the device tensors hold them: a bf16 tensor holds the
    rounded value, an fp32 tensor the drawn one."""
    a, b = _drawn(c)
    return (_rb(a) if c.abf else a), (_rb(b) if c.bbf else b)


def effective_operands(c, force_round=None):
    """What the kernel multiplies.  force_round: the mutant's switch."""
    a, b = stored_operands(c)
    if rounds_operands(c) if force_round is None else force_round:
        return _rb(a), _rb(b)
    return a, b


def operands(c):
    """A and B as CPU tensors in the storage layout transA / transB require (A
    stored [K, M] when transA, B stored [N, K] when transB), each a view 8 + off
    elements into a NaN-filled parent with row stride cols + ex."""
    a, b = stored_operands(c)
    sa = torch.from_numpy(np.ascontiguousarray(a.T if c.tA else a))
    sb = torch.from_numpy(np.ascontiguousarray(b.T if c.tB else b))
    sa = sa.bfloat16() if c.abf else sa.float()
    sb = sb.bfloat16() if c.bbf else sb.float()
    return (R.embed(sa, 0, off=8 + c.offa, ld=sa.shape[1] + c.exa),
            R.embed(sb, 0, off=8 + c.offb, ld=sb.shape[1] + c.exb))


@functools.lru_cache(maxsize=8)
def exact(c, force_round=None, drop_last_k=False):
    """gemm_reference.Exact of case c: z = alpha A'B' + bias + beta C0 in float64
    and the per-element magnitude.  The two switches are the CPU test's mutants."""
    a, b = effective_operands(c, force_round)
    if drop_last_k:
        a, b = a[:, :-1], b[:-1]
    bias, c0 = R.epilogue_inputs(c)
    z = c.alpha * (a @ b)
    mag = abs(c.alpha) * (np.abs(a) @ np.abs(b))
    if bias is not None:
        z = z + bias
        mag = mag + np.abs(bias)
    if c0 is not None:
        z = z + c.beta * c0
        mag = mag + np.abs(c.beta * c0)
    return R.Exact(z + 0.0, bias, c0, mag, R.unit(c))


def chunk_partials(c):
    """[split, M, N]: alpha A'B' restricted to each K chunk of plan_of(c)."""
    p = plan_of(c)
    a, b = effective_operands(c)
    if p.kernel == "gemv_cols":
        n, kc = p.gy, p.kc
    else:
        n, kc = p.split, p.kchunk
    return np.stack([c.alpha * (a[:, i * kc:(i + 1) * kc] @ b[i * kc:(i + 1) * kc]) for i in range(n)])


def want_bits(c, ex):
    """(C bits, Z bits or None) of the exact tier: act in {none, relu}."""
    assert c.act <= R.ACT_RELU
    return R.expected_bits(R.act64(ex.z, c.act), c.obf), (R.f32_bits(ex.z) if c.has_Z else None)


gauss_bound = R.gauss_bound      # derivation: module docstring


# ------------------------------------------------------------ failure messages

def locate(c, m, n):
    """Where element (m, n) of C lives in the kernel that plan_of(c) names."""
    p = plan_of(c)
    if p.kernel == "gemv_rows":
        return f"(m={m}) gemv_rows block={m // 4} wave={m % 4}, lanes over k = 0..{c.K - 1}"
    if p.kernel == "gemv_cols":
        return (f"(m={m}) gemv_cols block.x={m // 64} lane={m % 64}, {p.gy} k-chunks of {p.kc} "
                f"(last {c.K - (p.gy - 1) * p.kc})")
    nt_n = (c.N + BN - 1) // BN
    mi, ni = m % BM, n % BN
    s = (f"(m={m}, n={n}) kernel={p.kernel} tile=({m // BM},{n // BN}) = #{(m // BM) * nt_n + n // BN} of {p.tiles} "
         f"wave=({mi // 32},{ni // 32}) fragment=({(mi % 32) // 16},{(ni % 32) // 16}) "
         f"lane={16 * ((mi % 16) // 4) + ni % 16} reg={mi % 4}")
    if p.split > 1:
        s += f", {p.split} k-chunks of {p.kchunk} (last {c.K - (p.split - 1) * p.kchunk})"
    else:
        s += f", one k-chunk of {c.K}"
    return s


def _blame_chunk(c, m, n, diff):
    """Names the K chunk whose partial product, missing or doubled, explains diff."""
    p = plan_of(c)
    if max(p.split, p.gy) <= 1 or not np.isfinite(diff):
        return ""
    part = chunk_partials(c)[:, m, n]
    for i, v in enumerate(part):
        if v != 0.0 and diff in (v, -v):
            return f"; the difference is k-chunk {i}'s partial product ({'added twice' if diff == v else 'missing'})"
    return ""


def first_mismatch(c, got_bits, want, what="C"):
    """None, or a message naming the first differing element."""
    got_bits = np.asarray(got_bits).reshape(want.shape)
    bad = np.argwhere(got_bits != want)
    if bad.size == 0:
        return None
    m, n = (int(v) for v in bad[0])
    val = (lambda b: R.bf16_val(b) if b.dtype == np.uint16 else b.view(np.float32).astype(np.float64))
    g, w = float(val(got_bits[m:m + 1, n:n + 1])[0, 0]), float(val(want[m:m + 1, n:n + 1])[0, 0])
    return (f"{c.name}: {what} differs at {len(bad)} of {want.size} elements; first {locate(c, m, n)}: "
            f"got {g!r} (0x{int(got_bits[m, n]):x}), expected {w!r} (0x{int(want[m, n]):x})"
            + _blame_chunk(c, m, n, g - w))


def check_exact(c, ex, c_bits, z_bits):
    """None, or the first failure of the exact tier."""
    wc, wz = want_bits(c, ex)
    msg = first_mismatch(c, c_bits, wc, "C")
    if msg is None and c.has_Z:
        msg = first_mismatch(c, z_bits, wz, "Z")
    return msg


BRACKET_STEPS = (0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0)


def check_bounded(c, bits, ref, E, keys, trans=None):
    """An activated C against float64 ref within E (fp32 level) -- for a bf16 C
    within E + 2^-8 |ref| and inside the monotone bracket -- plus bit-identity of
    outputs with the same exact argument.  Returns (message or None, figures):
    figures maps a label to the measured |error| / allowance (fp32) or to the
    smallest multiple of E, in steps of 1/8, whose bracket holds every output;
    "differ" is (how many fp32 outputs differ from the transcription `trans`, of how many)."""
    fig = {}
    bits = np.asarray(bits).reshape(ref.shape)
    y = R.bf16_val(bits) if c.obf else bits.view(np.float32).astype(np.float64)
    if not np.all(np.isfinite(y)):
        m, n = map(int, np.argwhere(~np.isfinite(y))[0])
        return f"{c.name}: C is not finite at {locate(c, m, n)}", fig
    if c.obf:
        bad = np.argwhere(np.abs(y - ref) > E + R.HB * np.abs(ref))
        if bad.size:
            m, n = map(int, bad[0])
            return (f"{c.name}: C: {len(bad)} outside E + 2^-8 |ref|; first {locate(c, m, n)}: got {y[m, n]!r}, "
                    f"ref {ref[m, n]!r}"), fig
        k = R.bf16_key(bits)
        lo, hi = R.bf16_bracket(ref, E)
        bad = np.argwhere((k < lo) | (k > hi))
        if bad.size:
            m, n = map(int, bad[0])
            return (f"{c.name}: C: {len(bad)} outside [bf16(ref - E), bf16(ref + E)]; first {locate(c, m, n)}: "
                    f"got {y[m, n]!r}, ref {ref[m, n]!r}"), fig
        for f in BRACKET_STEPS:
            lo, hi = R.bf16_bracket(ref, f * E)
            if not np.any((k < lo) | (k > hi)):
                break
        fig["bf16 bracket factor"] = f
    else:
        r = np.abs(y - ref) / E
        fig["fp32"] = float(r.max())
        if trans is not None:
            off = bits != R.f32_bits(trans)
            fig["differ"] = (int(off.sum()), off.size)
            fig["fp32, over the outputs that differ from the transcription"] = float(r[off].max()) if off.any() else 0.0
        bad = np.argwhere(r > 1.0)
        if bad.size:
            m, n = map(int, bad[0])
            return (f"{c.name}: C: {len(bad)} outside E, worst ratio {r.max():.3f}; first {locate(c, m, n)}: "
                    f"got {y[m, n]!r}, ref {ref[m, n]!r}"), fig
    if not R.groups_identical(keys, bits):
        return f"{c.name}: C: outputs with the same exact argument differ in their bits", fig
    return None, fig


def keys_of(ex):
    return np.round(ex.z / ex.unit).astype(np.int64)


# ------------------------------------------------------------------ the case list

LAYOUTS = R.LAYOUTS
MN = (1, 15, 16, 17, 31, 33, 63, 64, 65, 129)
K_BF16 = (1, 7, 8, 9, 31, 32, 33, 65)
K_F32 = (1, 3, 4, 5, 15, 16, 17, 33)
# every dtype combination that reaches the bf16 kernel: (fp32, fp32, fp32) goes to the exact-f32 kernel, so 4 of the
# bf16 kernel's 32 compiled instantiations cannot be reached through dtfk_gemm; 28 + 4 can
DT_BF16 = [(a, b, o) for a in (True, False) for b in (True, False) for o in (False, True) if a or b or o]
DT_F32 = (False, False, False)
# split-K lengths: two even chunks; a ragged last chunk that is no multiple of the K step (twice); split 4; and
# 3073, where tiles = 1 estimates 12 chunks, rounds the chunk up to 288 and recomputes 11
K_SPLIT = (512, 520, 777, 1024, 3073)
GEMV_B = ((True, 0), (False, 0), (False, 2))          # (transB, exb): [1, K]; contiguous [K, 1]; [K, 1] with row stride 3
ACT_ALPHA = lambda K: 2.0 ** -3 if K <= 64 else (2.0 ** -4 if K <= 256 else 2.0 ** -6)   # keeps z where act is not saturated


def _cases():
    G = collections.OrderedDict((k, []) for k in ("T", "A", "R", "I", "E", "Z", "S", "U", "V", "W", "X", "G"))
    # T: tile, tail, grid: per layout and MFMA kernel every M, N and K of the lists at least once (asserted on the CPU
    # against plan()), all dtypes in turn.  fp32 x fp32 -> fp32 with N = 1 leaves the MFMA kernel: with transA a
    # beta of 0.5 keeps it there (the column form is linear, beta 0 or 1); without transA the row form takes every
    # N = 1, so that case runs on the row form and a second one carries its M and K to the MFMA kernel at N = 15
    for li, (tA, tB) in enumerate(LAYOUTS):
        for kern, Ks in (("bf16", K_BF16), ("f32", K_F32)):
            for i in range(10):
                for M, N, K in ((MN[i], MN[(3 * i + 1 + li) % 10], Ks[(i + li) % 8]),
                                (MN[(7 * i + 2) % 10], MN[i], Ks[(i + 3 + li) % 8])):
                    a, b, o = DT_BF16[(i + 2 * li) % 7] if kern == "bf16" else DT_F32
                    kw = dict(bias=bool(i & 1), exc=(0, 1, 8, 3)[i % 4], coff=i % 2, exa=(0, 3)[(i // 2) % 2],
                              exb=(0, 5)[(i // 3) % 2])
                    if kern == "f32" and N == 1 and tA:
                        kw["beta"] = 0.5
                    G["T"].append(case("T", M, N, K, tA, tB, a, b, o, **kw))
                    if kern == "f32" and N == 1 and not tA:
                        G["T"].append(case("T", M, 15, K, tA, tB, a, b, o, **kw))
    # the whole M x N cross at one ragged K, forward layout, both kernels
    for M in MN:
        for N in MN:
            G["T"].append(case("Tx", M, N, 33, False, True, True, True, False))
            G["T"].append(case("Tx", M, N, 17, False, True, *DT_F32))
    # A: alignment: full tiles, (a) aligned, (b) A / B one element off, (c) ld = cols + 1, (d) ld = cols + 8
    for li, (tA, tB) in enumerate(LAYOUTS):
        for a, b, o in ((True, True, False), (False, False, True), DT_F32):
            seed = 1000 + 10 * li + 4 * a + 2 * b + o
            for kw in (dict(), dict(offa=1), dict(offb=1), dict(exa=1, exb=1), dict(exa=8, exb=8)):
                G["A"].append(case("A", 64, 64, 64, tA, tB, a, b, o, seed=seed, **kw))
    # R: tile remap at 1, 7, 8, 9, 15, 17, 25 tiles; with K = 520 the same grids under split-K (gridDim.y = 2)
    for M, N in ((64, 64), (40, 418), (100, 250), (129, 129), (130, 300), (1030, 50), (257, 257)):
        for tA, tB in ((False, True), (True, False)):
            for a, b, o in ((True, True, False), DT_F32):
                G["R"].append(case("R", M, N, 17 if not a else 33, tA, tB, a, b, o, bias=True))
                G["R"].append(case("R", M, N, 520, tA, tB, a, b, o, bias=True, beta=1.0))
    # I: all 32 + 4 instantiations at one ragged shape, both operand families
    for tA, tB in LAYOUTS:
        for a, b, o in DT_BF16 + [DT_F32]:
            for fam in ("int", "wide"):
                G["I"].append(case("I", 37, 53, 41, tA, tB, a, b, o, fam=fam, rng=3 if fam == "wide" else None,
                                   bias=fam == "wide", exc=3))
    # E: the linear epilogue: bias, alpha, beta, through an fp32 and a bf16 C; N = 53 is no multiple of 16
    i = 0
    for bias in (False, True):
        for alpha in (1.0, 0.5, -2.0):
            for beta in (0.0, 1.0, 0.5, 2.0):
                for a, b, o in ((True, True, False), (True, True, True), DT_F32):
                    tA, tB = LAYOUTS[i % 4]
                    i += 1
                    G["E"].append(case("E", 70, 53, 41, tA, tB, a, b, o, alpha=alpha, beta=beta, bias=bias,
                                       exc=(0, 3)[i % 2], coff=(i // 2) % 2, fam=("int", "wide")[(i // 4) % 2],
                                       rng=3 if (i // 4) % 2 else None))
    # Z: every activation, with and without Z, on both MFMA kernels (two tiles, ragged)
    i = 0
    for act in ACTS:
        for a, b, o in ((True, True, False), (False, True, True), DT_F32):
            for has_Z in (False, True):
                for beta in (0.0, 0.5):
                    tA, tB = LAYOUTS[i % 4]
                    i += 1
                    G["Z"].append(case("Z", 70, 45, 41, tA, tB, a, b, o, alpha=ACT_ALPHA(41), beta=beta, bias=True,
                                       act=act, has_Z=has_Z, exc=0 if has_Z else 3, rng=3))
    # S: automatic split-K on both MFMA kernels and all layouts
    for tA, tB in LAYOUTS:
        for a, b, o in ((True, True, False), (False, True, False), (True, False, False), DT_F32):
            for K in K_SPLIT:
                if a != b and K not in (520, 1024):
                    continue
                for beta, bias in ((0.0, False), (1.0, True)):
                    G["S"].append(case("S", 37, 53, K, tA, tB, a, b, o, beta=beta, bias=bias, exc=3,
                                       fam="wide" if K == 777 else "int"))
            if a == b:
                G["S"].append(case("S", 70, 130, 520, tA, tB, a, b, o, beta=1.0, bias=True, alpha=-2.0))
    # U: the same K with an epilogue that must not split
    for li, (tA, tB) in enumerate(LAYOUTS):
        for a, b in ((True, True), (False, False)):
            K = (520, 777)[li % 2]
            G["U"].append(case("U", 37, 53, K, tA, tB, a, b, False, beta=0.5, bias=True))
            G["U"].append(case("U", 37, 53, K, tA, tB, a, b, False, act=R.ACT_RELU, bias=True))
            G["U"].append(case("U", 37, 53, K, tA, tB, a, b, False, has_Z=True, bias=True))
            G["U"].append(case("U", 37, 53, K, tA, tB, a, b, False, alpha=ACT_ALPHA(K), act=R.ACT_SIGMOID, bias=True))
            if a:
                G["U"].append(case("U", 37, 53, K, tA, tB, a, b, True, bias=True))
    # V: matrix-vector, row form
    i = 0
    for M in (1, 3, 4, 5, 9):
        for K in (1, 63, 64, 65, 127, 128, 129, 193):
            for tB, exb in GEMV_B:
                i += 1
                act = ACTS[i % 5]
                has_Z = i % 3 == 0
                G["V"].append(case("V", M, 1, K, False, tB, *DT_F32, alpha=ACT_ALPHA(K) if act > 1 else (1.0, -2.0)[i % 2],
                                   beta=(0.0, 0.5, 1.0)[(i // 2) % 3], bias=bool((i // 3) % 2), act=act, has_Z=has_Z,
                                   exb=exb, offb=i % 2, exa=(0, 3)[(i // 5) % 2], exc=0 if (has_Z and M > 1) else (2, 0, 7)[i % 3],
                                   fam="int" if act > 1 else ("int", "wide")[(i // 7) % 2], rng=3))   # wide values would saturate
    for act in ACTS:                                   # every activation with Z at one shape
        for beta in (0.0, 0.5, 1.0):
            G["V"].append(case("Vz", 9, 1, 193, False, False, *DT_F32, alpha=ACT_ALPHA(193), beta=beta, bias=True,
                               act=act, has_Z=True, exb=2))
    # W: matrix-vector, column form (linear, beta in {0, 1})
    i = 0
    for M in (1, 63, 64, 65, 130):
        for K in (1, 3, 4, 5, 63, 64, 65, 130, 1000):
            for tB, exb in GEMV_B:
                i += 1
                G["W"].append(case("W", M, 1, K, True, tB, *DT_F32, alpha=(1.0, 0.5, -2.0)[i % 3], beta=float(i % 2),
                                   bias=bool((i // 2) % 2), exb=exb, offb=(i // 3) % 2, exa=(0, 1, 8)[i % 3],
                                   exc=(0, 2, 7)[(i // 2) % 3], fam=("int", "wide")[(i // 5) % 2], rng=3))
    # X: transA with N = 1 and an epilogue the column form does not have: falls through to the f32 MFMA kernel
    for M, K in ((65, 65), (130, 5), (1, 130)):
        for tB, exb in GEMV_B:
            G["X"].append(case("X", M, 1, K, True, tB, *DT_F32, beta=0.5, bias=True, exb=exb, fam="wide", rng=3))
            G["X"].append(case("X", M, 1, K, True, tB, *DT_F32, has_Z=True, bias=True, exb=exb))
            G["X"].append(case("X", M, 1, K, True, tB, *DT_F32, act=R.ACT_RELU, beta=1.0, exb=exb, exc=2))
            G["X"].append(case("X", M, 1, K, True, tB, *DT_F32, alpha=ACT_ALPHA(K), act=R.ACT_TANH, bias=True, exb=exb))
    # G: Gaussian operands, one or two runs per kernel
    G["G"].append(case("G", 70, 45, 100, False, True, False, True, False, alpha=0.5, beta=1.0, bias=True, fam="gauss", exc=3))
    G["G"].append(case("G", 70, 45, 100, True, False, True, False, True, beta=1.0, bias=True, fam="gauss"))
    G["G"].append(case("G", 70, 45, 777, True, False, True, True, False, bias=True, fam="gauss"))
    G["G"].append(case("G", 70, 45, 100, False, True, *DT_F32, alpha=0.5, beta=1.0, bias=True, fam="gauss", exc=3))
    G["G"].append(case("G", 70, 45, 777, True, False, *DT_F32, bias=True, fam="gauss"))
    G["G"].append(case("G", 9, 1, 193, False, False, *DT_F32, beta=0.5, bias=True, fam="gauss", exb=2))
    G["G"].append(case("G", 130, 1, 1000, True, False, *DT_F32, beta=1.0, bias=True, fam="gauss", exb=2))
    return G


CASES = _cases()
ALL = [c for g in CASES.values() for c in g]
EXACT = [c for c in ALL if not c.gauss and c.act <= R.ACT_RELU]
BOUNDED = [c for c in ALL if not c.gauss and c.act >= R.ACT_SIGMOID]
GAUSS = CASES["G"]


def required_paths():
    """Every path the list must reach: 32 + 4 MFMA instantiations, split and
    unsplit per kernel, both matrix-vector kernels, each gy class."""
    need = {("gemv_rows",)} | {("gemv_cols", g) for g in (1, 2, 3, 4)}
    for tA, tB in LAYOUTS:
        need.add(("f32", tA, tB))
        for kern in ("f32", "bf16"):
            need.add((kern, "split", tA, tB))
            need.add((kern, "unsplit", tA, tB))
        for a, b, o in DT_BF16:
            need.add(("bf16", a, b, tA, tB, o))
    return need
