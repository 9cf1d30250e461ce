"""Float64 model of the large-tile bf16 GEMM (csrc/kernels/gemm_big.hip), the
operands that make its result exactly computable, and the error bounds its
inexact epilogues are held to.

A helper module, not a test file: `import gemm_reference` (pytest puts tests/ on
sys.path).  NumPy and CPU torch only; tests/test_gemm_reference_cpu.py checks
this file against itself, tests/test_gemm_big_edges_gpu.py holds the kernels to it.

The exact tier
--------------
Operands are bf16 and the accumulator is fp32.  With integer-valued A and B and
K * max|a| * max|b| < 2^24 every product and every partial sum is an integer
below 2^24 in magnitude, hence exactly representable in fp32, in any summation
order, on any K split, through atomics or slabs.  With alpha a power of two and
bias and C0 on a power-of-two grid, z = alpha A'B' + bias + beta C0 is exact as
long as (|alpha| sum|a||b| + |bias| + |beta C0|) / unit < 2^24 (`magnitude`):
every intermediate the kernel can form is a multiple of `unit` below 2^24 units.
An fp32 output must then equal z bit for bit and a bf16 output must equal
bf16_rne(z) bit for bit.

The bounded tier
----------------
An activation of an exact z, y = act(z), is held to

    |y - act64(z)| <= A(z) + H(z) + FLOOR  (+ 2^-8 |act64(z)| for a bf16 output)

(bf16 keeps 8 significant bits: half an ulp is 2^-8 of the binade's lower end,
so 2^-8 |v| is the smallest relative bound a correctly rounded store can meet --
1 + 2^-8 rounds to 1.  The bracket below is the sharp form.)

A(z): the worst measured error against float64 of the NumPy fp32 transcription
    of the kernel's formula over the case's own z within about 1 of z (the
    cases' z are a finite set of grid points, so the table is enumerated, not
    sampled; buckets of width 0.5, each with its two neighbours).  Not the error
    at z alone: rounding errors at neighbouring arguments have the same scale
    and unrelated signs, so at one point the transcription can be exact by luck
    while the kernel, whose approximate instructions may differ from the
    correctly rounded value in the last bit, rounds its later operations the
    other way (measured on the GPU with the pointwise table: up to 0.9 of the
    allowance at the outputs that differ from the transcription).  Where hipcc
    may or may not contract a multiply and an add into an fma, the larger error
    of the two transcriptions is taken.
H(z): one term per hardware-approximate instruction the formula uses, each at
    its documented accuracy and propagated through the float64 formula:
      v_exp_f32 (inside __expf = v_exp_f32(x * log2e); the multiply is part of
                 the transcription)                 1 ulp  = relative 2^-23
      v_rcp_f32 (__builtin_amdgcn_rcpf)             1 ulp  = relative 2^-23
      erff, tanhf (OCML)                            4 ulp  = relative 2^-21
    No OCML accuracy table ships with the toolchain this was written against, so
    erff / tanhf take the 4 ulp fallback.  `1.f / x` compiles to the correctly
    rounded division sequence (v_div_scale / v_div_fmas / v_div_fixup) and needs
    no term.
FLOOR = 2^-118: v_exp_f32 flushes a denormal result to zero, which moves a
    result by less than 2^-126 * max|z|.
For the tanh-free GELU of common.h (gelu_cdf_pdf, Abramowitz-Stegun 7.1.26) the
float64 reference is the same formula in float64: the polynomial is the
kernel's definition of GELU (|formula64 - erf-GELU| <= 0.5 |z| 1.5e-7, checked on
the CPU).

Because rounding to bf16 is monotone, a bf16 output whose fp32 value lies in
[ref - E, ref + E] must lie in [bf16_rne(ref - E), bf16_rne(ref + E)]
(`bf16_bracket`); that is checked next to the looser 2^-8 form.
"""
import collections
import functools
import zlib

import numpy as np
import torch

U = 2.0 ** -24        # fp32 unit roundoff
ULP = 2.0 ** -23      # one fp32 ulp, relative (upper bound)
HB = 2.0 ** -8        # bf16 unit roundoff (8 significant bits, round to nearest)
FLOOR = 2.0 ** -118
OCML_ULP = 4.0        # erff / tanhf: fallback, see the module docstring

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_GELU = 0, 1, 2, 3, 4
LAYOUTS = [(False, True), (False, False), (True, False), (True, True)]   # (transA, transB)
F = np.float32


# ------------------------------------------------------------------ bf16 bits

def bf16_rne(x):
    """uint16 bf16 bits of x (any float array; values are first taken to fp32,
    which is exact for everything the exact tier produces), round to nearest,
    ties to even, done on the bits."""
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, np.uint16(0x7FC0), r)


def bf16_trunc(x):
    """The mutant: the upper half of the fp32 bits."""
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
    return (b >> 16).astype(np.uint16)


def bf16_val(bits):
    """float64 value of bf16 bits."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_key(bits):
    """Monotone integer key of bf16 bits (orders like the values; -0 < +0)."""
    b = np.asarray(bits, dtype=np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF) - 1, b)


def bf16_bracket(ref, err):
    """Keys (lo, hi) between which a bf16 output must lie when its value before
    rounding is within err of ref.  The float64 -> fp32 step of bf16_rne can move
    a bound by U |ref| at most, which is added to err first."""
    e = err + U * np.abs(ref)
    return bf16_key(bf16_rne(ref - e)), bf16_key(bf16_rne(ref + e))


def tensor_bits(t):
    """CPU torch tensor (bf16 or fp32) -> numpy array of its bits."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.view(torch.int32).numpy().view(np.uint32)


def f32_bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


# ---------------------------------------------------------------------- cases

_FIELDS = ("name kind M N K tA tB variant obf alpha beta bias act split_k pa pb pc coff rng seed gauss accumulate scale")
Case = collections.namedtuple("Case", _FIELDS)


def case(name, M, N, K, tA=False, tB=True, variant=8, obf=False, alpha=1.0, beta=0.0, bias=False, act=0, split_k=1,
         pa=0, pb=0, pc=0, coff=0, rng=None, kind="gemm", gauss=False, accumulate=False, scale=1.0):
    """kind: gemm | stats | ga (gemm_gelu_aux) | dg (gemm_dgelu).  pa / pb / pc:
    leading-dimension padding of A / B / C in units of 8 elements.  coff: extra
    element offset of the C view.  rng: operand integers are uniform in
    [-rng, rng]: 3; 11 for a bf16 output, so that at K = 128 (std of z ~500) about
    40 % of the outputs are not bf16 numbers and genuinely need rounding (+-7
    gives 11 %); 5 for the statistics, whose sums of squares over 128 rows must
    stay below 2^24 while a few percent of the stored values are still rounded.
    scale: a power of two both operands are multiplied by (still exact in bf16);
    A'B' then lies on the grid scale^2."""
    if rng is None:
        rng = 5 if kind == "stats" else (11 if obf else 3)
    full = f"{name}-{M}x{N}x{K}-{'T' if tA else 'N'}{'T' if tB else 'N'}-v{variant}-{'bf16' if obf else 'fp32'}"
    for tag, val, default in (("alpha", alpha, 1.0), ("beta", beta, 0.0), ("bias", int(bias), 0), ("act", act, 0),
                              ("split", split_k, 1), ("pa", pa, 0), ("pb", pb, 0), ("pc", pc, 0), ("coff", coff, 0),
                              ("acc", int(accumulate), 0), ("scale", scale, 1.0)):
        if val != default:
            full += f"-{tag}{val:g}"
    return Case(full, kind, M, N, K, tA, tB, variant, obf, float(alpha), float(beta), bool(bias), act, split_k, pa, pb,
                pc, coff, rng, zlib.crc32(full.encode()), gauss, accumulate, float(scale))


def embed(t, p, off=8, fill=float("nan")):
    """A copy of the 2-D tensor t as a view inside a wider flat parent: the view
    starts `off` elements in, its row stride is cols + 8 p, and everything
    outside it is `fill`.  view._base is the parent."""
    rows, cols = t.shape
    ld = cols + 8 * p
    parent = torch.full((off + rows * ld + 8,), fill, dtype=t.dtype)
    view = parent.as_strided((rows, cols), (ld, 1), off)
    view.copy_(t)
    return view


def on(view, device):
    """The same view of a copy of its parent on `device`."""
    return view._base.to(device).as_strided(view.size(), view.stride(), view.storage_offset())


def _gen(c):
    return np.random.default_rng(c.seed)


def _raw_operands(c):
    """float64 A' [M, K] and B' [K, N]."""
    g = _gen(c)
    if c.gauss:
        a = g.standard_normal((c.M, c.K)) * c.K ** -0.5
        b = g.standard_normal((c.K, c.N)) * c.K ** -0.5
        rb = lambda x: bf16_val(bf16_rne(x))
        return rb(a), rb(b)
    a = g.integers(-c.rng, c.rng + 1, (c.M, c.K)).astype(np.float64) * c.scale
    b = g.integers(-c.rng, c.rng + 1, (c.K, c.N)).astype(np.float64) * c.scale
    return a, b


def operands(c):
    """bf16 A and B in the storage layout transA / transB require (A stored
    [K, M] when transA, B stored [N, K] when transB), each a view 8 elements
    into a NaN-filled parent with row stride cols + 8 p."""
    a, b = _raw_operands(c)
    sa = torch.from_numpy(np.ascontiguousarray(a.T if c.tA else a)).bfloat16()
    sb = torch.from_numpy(np.ascontiguousarray(b.T if c.tB else b)).bfloat16()
    return embed(sa, c.pa), embed(sb, c.pb)


def epilogue_inputs(c):
    """bias [N] (fp32 values, multiples of 2^-3 in [-4, 4]; neighbouring columns,
    and columns 4, 8, 16, 64, 192 or 256 apart, differ) or None; C0 [M, N]
    (multiples of 2^-3 with at most 7 significant bits: exact in bf16) or None
    when beta == 0."""
    n = np.arange(c.N)
    bias = (((n * 37 + (n // 64) * 11) % 65) - 32) / 8.0 if c.bias else None
    c0 = None
    if c.beta != 0.0:
        c0 = np.random.default_rng(c.seed ^ 0x5EED).integers(-64, 65, (c.M, c.N)) / 8.0
    if c.gauss:
        g = np.random.default_rng(c.seed ^ 0xB1A5)
        bias = g.standard_normal(c.N).astype(np.float32).astype(np.float64) if c.bias else None
        if c0 is not None:
            c0 = g.standard_normal((c.M, c.N))
            c0 = bf16_val(bf16_rne(c0)) if c.obf else c0.astype(np.float32).astype(np.float64)
    return bias, c0


Exact = collections.namedtuple("Exact", "z bias c0 magnitude unit")


def unit(c):
    """The power-of-two grid every intermediate of case c lies on."""
    u = min(1.0, abs(c.alpha)) * c.scale ** 2
    if c.bias or c.kind in ("ga", "dg"):
        u = min(u, 2.0 ** -3)
    if c.beta != 0.0:
        u = min(u, abs(c.beta) * 2.0 ** -3)
    return u


@functools.lru_cache(maxsize=8)
def exact(c):
    """z = alpha A'B' + bias + beta C0 in float64, and `magnitude` =
    |alpha| sum_k |a||b| + |bias| + |beta C0| per element (the largest value any
    partial result of the kernel can reach)."""
    a, b = _raw_operands(c)
    bias, c0 = epilogue_inputs(c)
    z = c.alpha * (a @ b)
    mag = abs(c.alpha) * (np.abs(a) @ np.abs(b))
    if bias is not None:
        z = z + bias
        mag = mag + np.abs(bias)
    if c0 is not None:
        z = z + c.beta * c0
        mag = mag + np.abs(c.beta * c0)
    return Exact(z + 0.0, bias, c0, mag, unit(c))      # + 0.0: no negative zero (the kernel adds bias or +0)


def expected_bits(z, obf):
    return bf16_rne(z) if obf else f32_bits(z)


def bn_partials(y_stored, M):
    """[2, ceil(M / 128), N] float64: per 128-row block, the column sums and
    sums of squares of the stored values."""
    y = np.asarray(y_stored, dtype=np.float64)
    P = (M + 127) // 128
    out = np.zeros((2, P, y.shape[1]))
    for p in range(P):
        blk = y[p * 128:min(M, (p + 1) * 128)]
        out[0, p] = blk.sum(0)
        out[1, p] = (blk * blk).sum(0)
    return out


def locate(c, m, n, w192=None):
    """Where element (m, n) lives in the 8-wave tile: for failure messages."""
    w192 = c.variant == 9 if w192 is None else w192
    bnt = 192 if w192 else 256
    wn = bnt // 4
    mi, ni = m % 256, n % bnt
    return (f"(m={m}, n={n}) tile=({m // 256},{n // bnt}) wave=({mi // 128},{ni // wn}) "
            f"quadrant=({(mi % 128) // 64},{0 if ni % wn < 32 else 1}) in-wave=({mi % 128},{ni % wn})")


def first_mismatch(c, got_bits, want_bits, what="C", w192=None):
    """None, or a message naming the first differing element."""
    bad = np.argwhere(got_bits != want_bits)
    if bad.size == 0:
        return None
    m, n = (int(v) for v in bad[0])
    return (f"{c.name}: {what} differs at {len(bad)} of {got_bits.size} elements; first {locate(c, m, n, w192)}: "
            f"got 0x{int(got_bits[m, n]):x}, expected 0x{int(want_bits[m, n]):x}")


# ------------------------------------------- fp32 transcriptions of the kernels

def _f(x):
    return np.asarray(x, dtype=np.float32)


def _fma(a, b, c):
    # a * b is exact in float64 (24 + 24 bits); one rounding to float64 and one to
    # fp32 differ from a single rounding only on a 2^-29 fraction of inputs
    return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, np.float64)).astype(F)


def expf_hw(x):
    """__expf(x): v_exp_f32(x * log2e) -- one fp32 multiply, then the exp2
    instruction (here: correctly rounded; its 1 ulp is a term of H)."""
    a = (_f(x) * F(1.4426950408889634)).astype(F)
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(a.astype(np.float64)).astype(F)


def _erf64(x):
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64)))).numpy()


def apply_act_slow_f32(z, act):
    """gemm_big.hip apply_act_slow, line by line."""
    z = _f(z)
    with np.errstate(over="ignore", under="ignore"):
        if act == ACT_RELU:
            return np.maximum(z, F(0))
        if act == ACT_SIGMOID:                       # 1.f / (1.f + __expf(-z))
            return (F(1) / (F(1) + expf_hw(-z))).astype(F)
        if act == ACT_TANH:                          # tanhf(z)
            return np.tanh(z.astype(np.float64)).astype(F)
        if act == ACT_GELU:                          # 0.5f * z * (1.f + erff(z * 0.70710678118654752f))
            e = _erf64((z * F(0.70710678118654752)).astype(F)).astype(F)
            return ((F(0.5) * z) * (F(1) + e)).astype(F)
    return z


def act64(z, act):
    z = np.asarray(z, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        if act == ACT_RELU:
            return np.maximum(z, 0.0)
        if act == ACT_SIGMOID:
            return 1.0 / (1.0 + np.exp(-z))
        if act == ACT_TANH:
            return np.tanh(z)
        if act == ACT_GELU:
            return 0.5 * z * (1.0 + _erf64(z * 0.7071067811865476))
    return z


# Abramowitz-Stegun 7.1.26 as common.h / gemm_big.hip write it
AS_P, AS_A = 0.3275911, (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
PDF0 = 0.3989422804014327
RSQRT2 = 0.70710678118654752


def gelu_cdf_pdf_f32(z, contract=False, a1=AS_A[0], pdf0=PDF0):
    """common.h gelu_cdf_pdf.  contract: `1.f - tail` with tail = (0.5f * poly) * e
    fused into one fma, as -ffp-contract=fast allows."""
    z = _f(z)
    x = (np.abs(z) * F(RSQRT2)).astype(F)
    t = (F(1) / _fma(np.full_like(x, F(AS_P)), x, F(1))).astype(F)               # rcpf(fmaf(p, x, 1))
    p = _fma(t, np.full_like(t, F(AS_A[4])), F(AS_A[3]))
    p = _fma(t, p, F(AS_A[2]))
    p = _fma(t, p, F(AS_A[1]))
    p = _fma(t, p, F(a1))
    poly = (t * p).astype(F)
    e = expf_hw(((F(-0.5) * z).astype(F) * z).astype(F))
    hp = (F(0.5) * poly).astype(F)
    tail = (hp * e).astype(F)
    one_minus = _fma(-hp, e, F(1)) if contract else (F(1) - tail).astype(F)
    cdf = np.where(z >= 0, one_minus, tail)
    pdf = (F(pdf0) * e).astype(F)
    return cdf, pdf


def gelu_fwd_f32(z, contract=False, **kw):
    """gemm_big.hip gelu_fwd_f: z * cdf."""
    cdf, _ = gelu_cdf_pdf_f32(z, contract, **kw)
    return (_f(z) * cdf).astype(F)


def gelu_grad2_f32(z, contract=False, a1=AS_A[0], pdf0=PDF0):
    """gemm_big.hip gelu_grad2 (per lane).  contract: every `a * b + c` of the
    source as one fma (v_pk_fma_f32), and `1.f - tail` fused with its product."""
    z = _f(z)
    mad = (lambda a, b, c: _fma(a, np.broadcast_to(_f(b), a.shape), c)) if contract else \
        (lambda a, b, c: ((a * _f(b)).astype(F) + _f(c)).astype(F))
    x = (np.abs(z) * F(RSQRT2)).astype(F)
    d = mad(x, F(AS_P), F(1))
    t = (F(1) / d).astype(F)
    half = lambda v: (F(0.5) * F(v)).astype(F)         # the constants fold at compile time
    poly = mad((t * F(0.5)).astype(F), F(AS_A[4]), half(AS_A[3]))
    poly = mad(t, poly, half(AS_A[2]))
    poly = mad(t, poly, half(AS_A[1]))
    poly = mad(t, poly, half(a1))
    poly = (t * poly).astype(F)
    a = ((z * z).astype(F) * F(-0.5)).astype(F)
    e = expf_hw(a)
    tail = (poly * e).astype(F)
    one_minus = _fma(-poly, e, F(1)) if contract else (F(1) - tail).astype(F)
    cdf = np.where(z >= 0, one_minus, tail)
    ep = (e * F(pdf0)).astype(F)
    return _fma(z, ep, cdf) if contract else ((z * ep).astype(F) + cdf).astype(F)


def _as64(z, dt=0.0, de=0.0):
    """cdf, pdf of the same formula in float64; t and e optionally off by the
    relative amounts dt, de (the hardware terms)."""
    z = np.asarray(z, np.float64)
    x = np.abs(z) * RSQRT2
    t = (1.0 / (AS_P * x + 1.0)) * (1.0 + dt)
    poly = t * (AS_A[0] + t * (AS_A[1] + t * (AS_A[2] + t * (AS_A[3] + t * AS_A[4]))))
    e = np.exp(-0.5 * z * z) * (1.0 + de)
    tail = 0.5 * poly * e
    return np.where(z >= 0, 1.0 - tail, tail), PDF0 * e


def gelu_fwd64(z, dt=0.0, de=0.0):
    cdf, _ = _as64(z, dt, de)
    return np.asarray(z, np.float64) * cdf


def gelu_grad64(z, dt=0.0, de=0.0):
    cdf, pdf = _as64(z, dt, de)
    return np.asarray(z, np.float64) * pdf + cdf


# ----------------------------------------------------- bounds of the inexact parts

def _hw_two(f64, z):
    """H for a formula with one rcp and one exp: the largest move of the float64
    formula when t and e are each off by one ulp either way."""
    base = f64(z)
    return np.max([np.abs(f64(z, st * ULP, se * ULP) - base) for st in (-1, 1) for se in (-1, 1)], axis=0)


def err_table(kind, zs, act=None):
    """(ref64, A, H) at the points zs (float64, exactly representable in fp32).
    kind: 'act' (apply_act_slow, needs act), 'gelu_fwd' (gelu_fwd_f), 'gelu_grad' (gelu_grad2)."""
    zs = np.asarray(zs, np.float64)
    if kind == "gelu_fwd":
        ref = gelu_fwd64(zs)
        A = np.maximum(np.abs(gelu_fwd_f32(zs, False) - ref), np.abs(gelu_fwd_f32(zs, True) - ref))
        return ref, A, _hw_two(gelu_fwd64, zs)
    if kind == "gelu_grad":
        ref = gelu_grad64(zs)
        A = np.maximum(np.abs(gelu_grad2_f32(zs, False) - ref), np.abs(gelu_grad2_f32(zs, True) - ref))
        return ref, A, _hw_two(gelu_grad64, zs)
    ref = act64(zs, act)
    A = np.abs(apply_act_slow_f32(zs, act).astype(np.float64) - ref)
    with np.errstate(over="ignore", under="ignore"):
        if act == ACT_SIGMOID:      # y = 1 / (1 + e): dy = e / (1 + e)^2 de, de = ULP e
            e = np.exp(-zs)
            H = np.where(np.isfinite(e), ULP * e / (1.0 + e) ** 2, 0.0)
            H = np.nan_to_num(H, nan=0.0)
        elif act == ACT_TANH:
            H = OCML_ULP * ULP * np.abs(ref)
        elif act == ACT_GELU:       # y = 0.5 z (1 + erf): dy = 0.5 |z| d erf
            H = 0.5 * np.abs(zs) * OCML_ULP * ULP * np.abs(_erf64(zs * 0.7071067811865476))
        else:
            H = np.zeros_like(zs)
    return ref, A, H


def neighbourhood_max(zs, A, width=0.5):
    """max of A over the bucket floor(z / width) of each z and the two buckets next to it."""
    b = np.floor(np.asarray(zs) / width).astype(np.int64)
    b -= b.min() - 1
    top = np.zeros(b.max() + 2)
    np.maximum.at(top, b, A)
    return np.maximum(np.maximum(top[b - 1], top[b]), top[b + 1])


def pointwise(kind, z, act=None):
    """(ref64, E) per element of z, E = A + H + FLOOR, through the table of the
    distinct values of z."""
    z = np.asarray(z, np.float64)
    uz, inv = np.unique(z, return_inverse=True)
    ref, A, H = err_table(kind, uz, act)
    inv = inv.reshape(z.shape)
    return ref[inv], (neighbourhood_max(uz, A) + H + FLOOR)[inv]


def groups_identical(keys, bits):
    """True when all outputs with the same key (the exact argument of the
    function) have the same bits.  keys: integer array(s) of bits' shape."""
    if not isinstance(keys, (tuple, list)):
        keys = (keys,)
    flat = [np.asarray(k).ravel() for k in keys]
    order = np.lexsort(flat)
    same = np.ones(order.size - 1, bool)
    for k in flat:
        ks = k[order]
        same &= ks[1:] == ks[:-1]
    b = np.asarray(bits).ravel()[order]
    return bool(np.all(b[1:][same] == b[:-1][same]))


def dgelu_bounds(dh, s, M):
    """gemm_dgelu at exact dh = A'B' [M, N] and exact s = aux + bias.  Returns
    ref_dU, E_dU (fp32 level: |dh| (A_g + H_g) + U |dh g|), ref_colpart [M/128, N],
    E_colpart, ref_db [N], E_db (accumulate=False; the caller adds U |db0 + ref_db|
    + U-level slop for the extra add of accumulate=True).

    dU = fl(dh * g_hw): one rounding, U |dh g| to first order (the second-order
    part is below U E and is covered by doubling that term's U to ULP).
    colpart sums 128 fp32 products in some order: each partial sum is rounded
    once, 127 additions, each partial sum at most sum |dh g| + E.
    db sums P = M/128 partials the same way."""
    g, Eg = pointwise("gelu_grad", s)
    ref = dh * g
    E = np.abs(dh) * Eg + ULP * np.abs(ref) + FLOOR
    P = M // 128
    blk = lambda x: x.reshape(P, 128, -1).sum(1)
    ref_cp = blk(ref)
    E_cp = blk(E) + 127 * U * (blk(np.abs(ref)) + blk(E))
    ref_db = ref_cp.sum(0)
    E_db = E_cp.sum(0) + max(P - 1, 0) * U * (np.abs(ref_cp).sum(0) + E_cp.sum(0))
    return ref, E, ref_cp, E_cp, ref_db, E_db


def gauss_bound(c, ex):
    """|C - ref64| <= 2 (K + 2) U magnitude: K products (exact) and K + 2
    additions / scalings in fp32, each rounding at most U times the running
    magnitude; the factor 2 covers the MFMA's undocumented internal accumulation
    rounding.  A bf16 output adds 2^-8 |ref64|."""
    b = 2.0 * (c.K + 2) * U * ex.magnitude
    return b + (HB * np.abs(ex.z) if c.obf else 0.0)


# ------------------------------------------------------------------ the case list

def _cases():
    G = collections.OrderedDict((k, []) for k in "ABCDEFGHIJKLMN")
    both = (False, True)
    # A: one interior tile, every layout, variant and K-loop length
    for tA, tB in LAYOUTS:
        for v, Ks in ((4, (64, 128, 256, 384)), (8, (128, 256, 384)), (9, (128, 256, 384)), (0, (128, 256, 384))):
            for K in Ks:
                for obf in both:
                    G["A"].append(case("A", 256, 192 if v == 9 else 256, K, tA, tB, v, obf))
    # B: tails.  K-contiguous operands take any row count, M/N-contiguous ones multiples of 8
    for tA, tB in LAYOUTS:
        Ms = (8, 136, 264) if tA else (1, 15, 17, 255, 257)
        Ns = (1, 255, 257) if tB else (8, 136, 264)
        for M in Ms:
            for N in Ns:
                for v in (4, 8, 9):
                    for obf in both:
                        G["B"].append(case("B", M, N, 128, tA, tB, v, obf))
        for N in (200, 224, 232, 392):
            for obf in both:
                G["B"].append(case("B192", 256, N, 128, tA, tB, 9, obf))
    # C: non-vector stores on a tile that is otherwise interior
    for tA, tB in ((False, True), (True, True)):
        for v in (4, 8, 9):
            for obf in both:
                for beta in (0.0, 1.0 if tA else -0.5):
                    for N in (257, 260):
                        G["C"].append(case("Cld", 256, N, 128, tA, tB, v, obf, beta=beta, bias=True))
    for tA, tB in LAYOUTS:
        for v in (8, 9):
            for obf in both:
                for beta in (0.0, -0.5):
                    G["C"].append(case("Coff", 256, 192 if v == 9 else 256, 128, tA, tB, v, obf, beta=beta, bias=True,
                                       pc=1, coff=4 if obf else 2))
    # D: leading dimensions of A, B, C independently
    pads = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 0, 0), (0, 3, 0), (0, 0, 3), (3, 1, 3))
    i = 0
    for tA, tB in LAYOUTS:
        for v in (4, 8):
            for pa, pb, pc in pads:
                for M, N in ((256, 256), (264, 136)):
                    i += 1
                    G["D"].append(case("D", M, N, 128, tA, tB, v, bool(i & 1), alpha=-2.0, beta=1.0 if i & 2 else 0.0,
                                       bias=True, pa=pa, pb=pb, pc=pc))
    for tA, tB in ((False, True), (True, False)):
        for M, N in ((256, 192), (264, 200)):
            for obf in both:
                G["D"].append(case("D192", M, N, 128, tA, tB, 9, obf, alpha=-2.0, beta=1.0, bias=True, pa=3, pb=1, pc=3))
    # E: epilogue order on the LDS-staged interior (both widths), an edge tile, a non-vector tile, the one-barrier loop
    for M, N, v in ((256, 256, 8), (256, 192, 9), (136, 264, 8), (256, 257, 8), (256, 256, 4)):
        for act in (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_GELU):
            for beta in (1.0, -0.5):
                for obf in both:
                    # bounded activations: +-3 keeps z (std ~6) where they are not saturated
                    G["E"].append(case("E", M, N, 128, False, True, v, obf, alpha=2.0 ** -3, beta=beta, bias=True,
                                       act=act, pc=0 if N == 257 else 1, rng=3 if act >= ACT_SIGMOID else None))
    # F: tile order (XCD remap) at grids of 1, 3, 7, 8, 9, 11, 17 tiles
    for M, N in ((256, 256), (768, 256), (1792, 256), (1024, 512), (768, 768), (2816, 256), (4352, 256)):
        for v in (4, 8, 9):
            for obf in both:
                G["F"].append(case("F", M, N * 3 // 4 if v == 9 else N, 128, False, True, v, obf, bias=True))
    # G: explicit split-K (fp32, linear): atomics on both loops, slabs
    for v, K, sk, N0 in ((4, 1024, 2, 256), (4, 1600, 3, 256), (8, 512, 2, 256), (8, 896, 3, 256), (8, 1024, 2, 258)):
        for tA, tB in (((False, True), (True, True)) if N0 == 258 else ((True, False), (False, True))):
            for M, N in ((256, N0), (264, 264 if N0 == 256 else 258)):
                for beta in (0.0, 1.0):
                    G["G"].append(case("G", M, N, K, tA, tB, v, False, beta=beta, bias=True, split_k=sk, pc=1))
    # H: automatic split-K: 8 slabs; one-barrier atomics with a short last chunk
    for K in (2048, 2112):
        for beta in (0.0, 1.0):
            G["H"].append(case("H", 256, 256, K, True, False, 0, False, beta=beta, bias=True, split_k=0, pc=1))
    # I: long K without a split
    for v in (4, 8):
        for obf in both:
            G["I"].append(case("I", 256, 256, 4096, False, True, v, obf, rng=3))
    # J: automatic 192-wide dispatch
    G["J"].append(case("J", 6656, 768, 128, False, True, 0, True, bias=True))
    # K: gemm_bn_stats
    for tA, tB in ((False, True), (False, False)):
        for M in (8, 136, 256, 384, 520):
            for N in (8, 136, 256, 264):
                for K in (128, 256):
                    G["K"].append(case("K", M, N, K, tA, tB, 8, True, kind="stats", pc=1))
    # L: fused GELU epilogues
    for M, N, K in ((256, 256, 128), (512, 768, 256), (768, 256, 384)):
        for tA, tB in LAYOUTS:
            G["L"].append(case("Lga", M, N, K, tA, tB, 8, True, kind="ga", bias=True, pc=1))
            if M == 256:   # operands on the grid 2^-4: z (std ~2, grid 2^-8) where GELU is not saturated and z is
                # no bf16 number, so gelu(z) and gelu(bf16(z)) differ
                G["L"].append(case("Lga16", M, N, K, tA, tB, 8, True, kind="ga", bias=True, pc=1, scale=2.0 ** -4))
            for bias in both:
                for acc in both:
                    G["L"].append(case("Ldg", M, N, K, tA, tB, 8, True, kind="dg", bias=bias, pc=1, accumulate=acc))
    # M: Gaussian operands, one run per kernel path
    for tA, tB in LAYOUTS:
        G["M"].append(case("M", 264, 264, 256, tA, tB, 8, tA, alpha=0.5, beta=1.0, bias=True, gauss=True, pc=1))
    G["M"].append(case("M192", 264, 200, 256, False, True, 9, True, bias=True, gauss=True))
    G["M"].append(case("Mv4", 264, 264, 192, False, True, 4, False, bias=True, gauss=True))
    G["M"].append(case("Mslab", 264, 264, 512, True, False, 8, False, beta=1.0, bias=True, split_k=2, gauss=True))
    G["M"].append(case("Matom", 264, 264, 1024, True, False, 4, False, beta=1.0, bias=True, split_k=2, gauss=True))
    G["M"].append(case("Matom8", 264, 258, 1024, False, True, 8, False, bias=True, split_k=2, gauss=True))
    G["M"].append(case("Mstats", 384, 264, 256, False, True, 8, True, kind="stats", gauss=True, pc=1))
    G["M"].append(case("Mga", 256, 256, 256, False, True, 8, True, kind="ga", bias=True, gauss=True, pc=1))
    G["M"].append(case("Mdg", 256, 256, 256, False, False, 8, True, kind="dg", bias=True, gauss=True, pc=1))
    return G


CASES = _cases()
EXACT_GROUPS = "ABCDFGHIJ"


def dg_inputs(c):
    """gemm_dgelu's saved pre-activation aux [M, N] (bf16-exact multiples of
    2^-3 in [-6, 6]) and bias [N] (multiples of 2^-3 in [-2, 2]) or None, as float64."""
    g = np.random.default_rng(c.seed ^ 0xA0C5)
    if c.gauss:
        aux = bf16_val(bf16_rne(g.standard_normal((c.M, c.N)) * 2.0))
        bias = g.standard_normal(c.N).astype(np.float32).astype(np.float64) if c.bias else None
        return aux, bias
    aux = g.integers(-48, 49, (c.M, c.N)) / 8.0
    n = np.arange(c.N)
    bias = (((n * 37) % 33) - 16) / 8.0 if c.bias else None
    return aux, bias
