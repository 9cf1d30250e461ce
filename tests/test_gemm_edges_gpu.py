"""csrc/kernels/gemm.hip per element through native.gemm, at the smallest shapes
where each of its paths exists: the 28 + 4 reachable MFMA instantiations (bf16
kernel: A fp32/bf16 x B fp32/bf16 x four layouts x fp32/bf16 C, without fp32 x
fp32 -> fp32, which is the exact-f32 kernel's), tile / tail / grid edges, vector
and masked scalar loads, the XCD tile remap, automatic split-K on both kernels,
every epilogue (alpha, beta through an fp32 and a bf16 C, bias, activation, Z),
both matrix-vector kernels, and the binding's rejections.

Reference, bounds and the case list: tests/gemm_small_reference.py (float64 on
the CPU; its own checks are in tests/test_gemm_small_reference_cpu.py).

* exact tier: integer-valued operands, power-of-two alpha, bias / C0 on a
  power-of-two grid: C (fp32) and Z equal the reference bit for bit, a bf16 C
  equals its round-to-nearest-even bf16 bit for bit.  No tolerance.
* bounded tier: sigmoid / tanh / erf-GELU of an exact z against float64 within
  E = A + H + FLOOR of gemm_reference.py, the monotone bf16 bracket, and
  bit-identity of outputs with the same z (Z itself stays exact); Gaussian
  operands against the float64 product within gauss_bound.

Every output (C, Z) is a view inside a sentinel-filled parent with guard rows
above and below, NaN before the call unless the kernel is to read it;
afterwards every sentinel bit is unchanged and every element of the view is
finite.  Operands are views inside NaN-filled parents.

A few remap cases exceed M, N = 200 because their tile counts (15, 17, 25) need it.

Measured on an MI355X (1204 tests, 11 s; the slowest 0.16 s), worst |error| /
allowance per quantity, always against the float64 reference; 1.0 would be a
failure.  The allowance of an fp32 quantity is E = A + H + FLOOR of
gemm_reference.py.  A bf16 output hides its fp32 value, so there the figure is
the smallest multiple of E whose bf16 bracket [bf16(ref - f E), bf16(ref + f E)]
still holds every output (steps of 1/8; 0 means every output is the rounded
reference itself).

    sigmoid   fp32 1.000 -- reached only where the kernel returns the
              transcription's own bits (99.3 % of the outputs) at the point whose
              transcription error is the largest of its neighbourhood, which is
              A by definition; over the 0.7 % that differ: 0.655
              bf16 bracket factor 0
    tanh      fp32 0.139 (5.6 % of the outputs differ from the correctly rounded
              tanh), bf16 bracket factor 0
    erf-GELU  fp32 0.387 (8.5 % differ), bf16 bracket factor 1/8
    Gaussian tier: fp32 C 0.007 on both MFMA kernels, 0.001 (row form) and 0.002
              (column form) on the matrix-vector kernels; bf16 C 0.969, which is
              the rounding to bf16 itself reaching half an ulp: the 2^-8 |ref|
              term is attained, the fp32 part of the bound is not visible there
"""
import numpy as np
import pytest
import torch

import gemm_reference as R
import gemm_small_reference as S

pytestmark = pytest.mark.gpu

SENT = {torch.float32: -7777.25, torch.bfloat16: -7744.0}
RATIOS = {}
DIFFER = {}


def _ratio(name, value):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(value))


def _sync():
    """A fault of an earlier launch surfaces here and is sticky: end the session
    rather than launch more work on a faulted device."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, stopping the session: {e}", returncode=3)


def _ibits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class OutBuf:
    """A [rows, cols] view, row stride cols + ex, inside a sentinel-filled flat
    buffer: two guard rows above and below, 8 + coff elements in."""

    def __init__(self, rows, cols, dtype, ex=0, coff=0, init=None):
        ld = cols + ex
        self.geom = ((rows, cols), (ld, 1), 2 * ld + 8 + coff)
        self.pre = torch.full((self.geom[2] + rows * ld + 2 * ld + 8,), SENT[dtype], dtype=dtype)
        v = self.pre.as_strided(*self.geom)
        if init is None:
            v.fill_(float("nan"))
        else:
            v.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(dtype))
        self.dev = self.pre.cuda()
        self.view = self.dev.as_strided(*self.geom)

    def finish(self, name, what="C"):
        """The view's bits after the call; asserts nothing outside it changed."""
        _sync()
        post = self.dev.cpu()
        out = post.as_strided(*self.geom).clone()
        post.as_strided(*self.geom).copy_(self.pre.as_strided(*self.geom))
        bad = (_ibits(post) != _ibits(self.pre)).nonzero()
        if bad.numel():
            ld, off = self.geom[1][0], self.geom[2]
            i = int(bad[0])
            raise AssertionError(f"{name}: {what}: {bad.numel()} elements outside the view were written; first at row "
                                 f"{(i - off) // ld}, column {(i - off) % ld} of the padded buffer (ld {ld})")
        return R.tensor_bits(out)

    def unchanged(self):
        _sync()
        return torch.equal(_ibits(self.dev.cpu()), _ibits(self.pre))


def _run(native, c, ex):
    """(C bits, Z bits or None) of one native.gemm call on case c."""
    A, B = S.operands(c)
    out = OutBuf(c.M, c.N, torch.bfloat16 if c.obf else torch.float32, c.exc, c.coff, ex.c0)
    zb = OutBuf(c.M, c.N, torch.float32, 0, 4) if c.has_Z else None
    bias = None if ex.bias is None else torch.from_numpy(ex.bias).float().cuda()
    native.gemm(R.on(A, "cuda"), c.tA, R.on(B, "cuda"), c.tB, out.view, bias=bias, act=c.act, alpha=c.alpha,
                beta=c.beta, Z=None if zb is None else zb.view)
    cb = out.finish(c.name)
    zbits = zb.finish(c.name, "Z") if zb is not None else None
    return cb, zbits


def _finite(c, bits, obf, what):
    v = R.bf16_val(bits) if obf else bits.view(np.float32)
    bad = np.argwhere(~np.isfinite(v))
    assert bad.size == 0, (f"{c.name}: {what}: {len(bad)} elements not written or poisoned by a read outside an "
                           f"operand; first {S.locate(c, *map(int, bad[0]))}")


@pytest.mark.parametrize("c", S.EXACT, ids=lambda c: c.name)
def test_exact(native, c):
    """Linear and ReLU epilogues of every group: bit for bit."""
    ex = S.exact(c)
    cb, zb = _run(native, c, ex)
    msg = S.check_exact(c, ex, cb, zb)
    assert msg is None, msg
    _finite(c, cb, c.obf, "C")


_ALIGN = sorted({c.seed for c in S.CASES["A"]})


@pytest.mark.parametrize("seed", _ALIGN)
def test_alignment_variants_are_bit_identical(native, seed):
    """Full 64x64x64 tiles through the vector loads (aligned, and ld = cols + 8)
    and through the masked scalar loads (a view one element off; ld = cols + 1)."""
    group = [c for c in S.CASES["A"] if c.seed == seed]
    assert len(group) == 5
    outs = [_run(native, c, S.exact(c))[0] for c in group]
    for c, o in zip(group[1:], outs[1:]):
        msg = S.first_mismatch(c, o, outs[0], f"C (against {group[0].name})")
        assert msg is None, msg


@pytest.mark.parametrize("c", [c for c in S.CASES["S"] if c.K in (777, 3073)], ids=lambda c: c.name)
def test_split_k_repeats(native, c):
    """Partial sums meet in atomics in any order: the result is the same every time."""
    ex = S.exact(c)
    for rep in range(3):
        cb, _ = _run(native, c, ex)
        msg = S.first_mismatch(c, cb, S.want_bits(c, ex)[0], f"C (run {rep})")
        assert msg is None, msg


_QUANTITY = {R.ACT_SIGMOID: "sigmoid", R.ACT_TANH: "tanh", R.ACT_GELU: "erf-GELU"}


@pytest.mark.parametrize("c", S.BOUNDED, ids=lambda c: c.name)
def test_activation_of_exact_preactivation(native, c):
    ex = S.exact(c)
    ref, E = R.pointwise("act", ex.z, c.act)
    cb, zb = _run(native, c, ex)
    if c.has_Z:
        msg = S.first_mismatch(c, zb, R.f32_bits(ex.z), "Z")
        assert msg is None, msg
    msg, fig = S.check_bounded(c, cb, ref, E, S.keys_of(ex), trans=R.apply_act_slow_f32(ex.z, c.act))
    n, of = fig.pop("differ", (0, 0))
    d = DIFFER.setdefault(_QUANTITY[c.act], [0, 0])
    d[0], d[1] = d[0] + n, d[1] + of
    for k, v in fig.items():
        _ratio(f"{_QUANTITY[c.act]} ({k})", v)
    assert msg is None, msg


@pytest.mark.parametrize("c", S.GAUSS, ids=lambda c: c.name)
def test_gaussian(native, c):
    ex = S.exact(c)
    cb, _ = _run(native, c, ex)
    _finite(c, cb, c.obf, "C")
    y = R.bf16_val(cb) if c.obf else cb.view(np.float32).astype(np.float64)
    r = np.abs(y.reshape(ex.z.shape) - ex.z) / S.gauss_bound(c, ex)
    _ratio(f"Gaussian {S.plan_of(c).kernel} C {'bf16' if c.obf else 'fp32'}", r.max())
    bad = np.argwhere(r > 1.0)
    assert bad.size == 0, (f"{c.name}: {len(bad)} outside the bound, worst {r.max():.3f}; first "
                           f"{S.locate(c, *map(int, bad[0]))}")


# ---- rejections: the binding throws before any launch; out, Z and their guards keep their bits

def _operand(rows, cols, dtype=torch.float32):
    return R.on(R.embed(torch.ones(rows, cols, dtype=dtype), 0), "cuda")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_z_with_a_padded_out_is_rejected(native, dtype):
    """The kernels store Z with out's leading dimension: a padded out would put Z past its end."""
    M, N, K = 5, 7, 9
    out = OutBuf(M, N, dtype, ex=8)
    zb = OutBuf(M, N, torch.float32)
    with pytest.raises(RuntimeError, match="Z.*out|out.*Z"):
        native.gemm(_operand(M, K, dtype), False, _operand(N, K, dtype), True, out.view, Z=zb.view)
    assert out.unchanged() and zb.unchanged()


@pytest.mark.parametrize("M,N,tA,dtype", [(5, 7, False, torch.float32), (5, 7, True, torch.bfloat16),
                                          (5, 1, False, torch.float32), (5, 1, True, torch.float32)])
def test_empty_inner_dimension_is_rejected(native, M, N, tA, dtype):
    out = OutBuf(M, N, dtype, ex=3)
    A = torch.empty((0, M) if tA else (M, 0), dtype=dtype, device="cuda")
    B = torch.empty((N, 0), dtype=dtype, device="cuda")
    with pytest.raises(RuntimeError, match="K == 0"):
        native.gemm(A, tA, B, True, out.view)
    with pytest.raises(RuntimeError, match="K == 0"):
        native.gemm(A, tA, B, True, out.view, beta=1.0, act=1)
    assert out.unchanged()


@pytest.mark.parametrize("M,N", [(0, 7), (5, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_empty_output_returns_without_a_write(native, M, N, dtype):
    K = 9
    out = OutBuf(M, N, dtype, ex=3)
    bias = torch.ones(N, device="cuda")
    native.gemm(_operand(M, K, dtype), False, _operand(N, K, dtype), True, out.view, bias=bias, beta=1.0)
    native.gemm(_operand(K, M, dtype), True, _operand(K, N, dtype), False, out.view)
    assert out.unchanged()


def test_zz_measured_ratios():
    """A reporting helper, not a check of its own: prints the worst error /
    allowance per quantity that the tests before it in this module recorded (the
    figures in the module docstring; run the whole file with -s to see them).
    Run alone, under -k or in another process than those tests it has nothing to
    print, and its assert only repeats what each case already asserted."""
    for k in sorted(RATIOS):
        print(f"RATIO {k}: {RATIOS[k]:.3f}")
    for k, (n, of) in sorted(DIFFER.items()):
        print(f"DIFFER {k}: {n} of {of} fp32 outputs differ from the transcription ({100.0 * n / max(of, 1):.1f} %)")
    assert all(v <= 1.0 for v in RATIOS.values())
