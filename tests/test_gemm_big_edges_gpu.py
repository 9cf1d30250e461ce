"""csrc/kernels/gemm_big.hip per element, at the smallest shapes where each of its
paths exists: both schedules, both tile widths, four layouts, the three
split-K mechanisms, every epilogue path and the three fused epilogues.

Reference and bounds: tests/gemm_reference.py (float64 on the CPU; its own
checks are in tests/test_gemm_reference_cpu.py).  Two tiers:

* exact: integer-valued bf16 operands, power-of-two alpha, bias / C0 on a
  power-of-two grid -- every partial sum the kernel can form is exact in fp32,
  so an fp32 output equals the reference bit for bit and a bf16 output equals
  its round-to-nearest-even bf16 bit for bit.  No tolerance.
* bounded: an activation of an exact argument (sigmoid / tanh / GELU, the fused
  GELU forward and backward) against float64 within the derived allowance, the
  monotone bf16 bracket of that allowance, and bit-identity of all outputs that
  have the same exact argument; Gaussian operands against the float64 bound.

Every output (C, aux, colpart, dbias) is a view inside a larger buffer filled
with a sentinel and is NaN before the call unless the kernel is to read it;
afterwards every sentinel bit is unchanged and every element of the view is
finite.  Operands sit in NaN-filled parents, 16 bytes in.

Measured on an MI355X (984 tests, 11 s), worst |error| / allowance per quantity,
always against the float64 reference; 1.0 would be a failure.  The allowance
of an fp32 quantity is E = A + H + FLOOR of gemm_reference.py.  A bf16 output
hides its fp32 value, so there the figure is the smallest multiple of E whose
bf16 bracket [bf16(ref - f E), bf16(ref + f E)] still holds every output
(steps of 1/8; 0 means every output is the rounded reference itself).

    sigmoid   fp32 1.000 -- reached only where the kernel returns the
              transcription's own bits (99 % of the outputs) at the point whose
              transcription error is the largest of its neighbourhood, which is
              A by definition; over the 1 % that differ: 0.884
              bf16 bracket factor 0
    tanh      fp32 0.137 (3.8 % of the outputs differ from the correctly rounded
              tanh), bf16 bracket factor 0
    erf-GELU  fp32 0.314 (5.8 % differ), bf16 bracket factor 1/8
    gelu_fwd_f (gemm_gelu_aux h)      bf16 bracket factor 1/8
    gelu_grad2 (gemm_dgelu dU)        bf16 bracket factor 5/8: |dh| reaches
              the thousands, so the bf16 dU still shows gelu' to its last fp32 bits
    dgelu colpart 0.010, dbias 0.006
    Gaussian tier: C fp32 0.003; stats partials 0.017; dgelu colpart < 0.001;
              bf16 outputs (C, stats y, aux, h, dU) 0.95 - 0.98, which is the
              rounding to bf16 itself reaching half an ulp: the 2^-8 |ref| term
              is attained, the fp32 part of those bounds is not visible there
"""
import numpy as np
import pytest
import torch

import gemm_reference as R

pytestmark = pytest.mark.gpu

SENT = {torch.float32: -7777.25, torch.bfloat16: -7744.0}
RATIOS = {}


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
    """A [rows, cols] view, row stride cols + 8 pc, inside a sentinel-filled flat
    buffer: two guard rows above and below, 8 (+ coff) elements in."""

    def __init__(self, rows, cols, dtype, pc=0, coff=0, init=None, flat_tail=0):
        ld = cols + 8 * pc
        self.geom = ((rows, cols), (ld, 1), 2 * ld + 8 + coff)
        self.pre = torch.full((self.geom[2] + rows * ld + 2 * ld + 8 + flat_tail,), SENT[dtype], dtype=dtype)
        v = self.pre.as_strided(*self.geom)
        if init is None:
            v.fill_(float("nan"))
        else:
            v.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(dtype))
        self.dev = self.pre.cuda()
        self.view = self.dev.as_strided(*self.geom)

    def finish(self, name, what="C"):
        """The view's content after the call (CPU); asserts nothing outside it changed."""
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
        return out

    def unchanged(self):
        _sync()
        return torch.equal(_ibits(self.dev.cpu()), _ibits(self.pre))


def _bias(b):
    return None if b is None else torch.from_numpy(b).float().cuda()


def _run(native, c, ex):
    A, B = R.operands(c)
    buf = OutBuf(c.M, c.N, torch.bfloat16 if c.obf else torch.float32, c.pc, c.coff, ex.c0)
    ok = native.gemm_big(R.on(A, "cuda"), c.tA, R.on(B, "cuda"), c.tB, buf.view, bias=_bias(ex.bias), act=c.act,
                         alpha=c.alpha, beta=c.beta, split_k=c.split_k, variant=c.variant)
    assert ok, f"{c.name}: rejected by the shape contract"
    return R.tensor_bits(buf.finish(c.name))


def _finite(bits, obf):
    v = R.bf16_val(bits) if obf else bits.view(np.float32)
    return bool(np.all(np.isfinite(v)))


def _w192(c):
    return c.variant == 9 or c.name.startswith("J-")


_EXACT = [c for g in "ABCDEFGI" for c in R.CASES[g] if c.act <= R.ACT_RELU]


@pytest.mark.parametrize("c", _EXACT, ids=lambda c: c.name)
def test_exact(native, c):
    """Groups A-G and I, and E with no activation / ReLU: bit for bit."""
    ex = R.exact(c)
    want = R.expected_bits(R.act64(ex.z, c.act), c.obf)
    got = _run(native, c, ex)
    msg = R.first_mismatch(c, got, want, w192=_w192(c))
    assert msg is None, msg


@pytest.mark.parametrize("c", R.CASES["H"], ids=lambda c: c.name)
def test_automatic_split_is_exact_and_repeatable(native, c):
    ex = R.exact(c)
    want = R.expected_bits(ex.z, c.obf)
    for rep in range(3):
        got = _run(native, c, ex)
        msg = R.first_mismatch(c, got, want, what=f"C (run {rep})")
        assert msg is None, msg


def test_automatic_192_wide_dispatch(native):
    (c,) = R.CASES["J"]
    ex = R.exact(c)
    want = R.expected_bits(ex.z, c.obf)
    for v in (0, 9, 8):
        cv = c._replace(variant=v)
        msg = R.first_mismatch(cv, _run(native, cv, ex), want, what=f"C (variant {v})", w192=v != 8)
        assert msg is None, msg


def _check_bounded(c, name, bits, obf, ref, E, keys, quantity, trans=None):
    """bits against ref within E at fp32 level (+ bf16 rounding), plus grouping."""
    assert _finite(bits, obf), f"{name}: non-finite output"
    if obf:
        y = R.bf16_val(bits)
        loose = E + R.HB * np.abs(ref)
        bad = np.argwhere(np.abs(y - ref) > loose)
        assert bad.size == 0, f"{name}: {len(bad)} outside E + 2^-8 |ref|; first {R.locate(c, *map(int, bad[0]))}"
        lo, hi = R.bf16_bracket(ref, E)
        k = R.bf16_key(bits)
        bad = np.argwhere((k < lo) | (k > hi))
        assert bad.size == 0, (f"{name}: {len(bad)} outside [bf16(ref - E), bf16(ref + E)]; first "
                               f"{R.locate(c, *map(int, bad[0]))}: got {y[tuple(bad[0])]!r}, ref {ref[tuple(bad[0])]!r}")
        # how much of E the kernel uses, seen through the rounding: the smallest
        # multiple of E whose bracket still holds every output
        for f in (0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0):
            lo, hi = R.bf16_bracket(ref, f * E)
            if not np.any((k < lo) | (k > hi)):
                break
        _ratio(quantity + " (bf16, bracket factor)", f)
    else:
        y = bits.view(np.float32).astype(np.float64)
        r = np.abs(y - ref) / E
        bad = np.argwhere(r > 1.0)
        assert bad.size == 0, (f"{name}: {len(bad)} outside E, worst ratio {r.max():.3f}; first "
                               f"{R.locate(c, *map(int, bad[0]))}: got {y[tuple(bad[0])]!r}, ref {ref[tuple(bad[0])]!r}")
        _ratio(quantity + " (fp32)", r.max())
        if trans is not None:      # A is the transcription's own error: where the kernel equals it, r is A / E
            off = bits != R.f32_bits(trans)
            _ratio(quantity + " (fp32, fraction of outputs that differ from the transcription)", off.mean())
            _ratio(quantity + " (fp32, over those)", r[off].max() if off.any() else 0.0)
    assert R.groups_identical(keys, bits), f"{name}: outputs with the same exact argument differ in their bits"


@pytest.mark.parametrize("c", [c for c in R.CASES["E"] if c.act >= R.ACT_SIGMOID], ids=lambda c: c.name)
def test_activation_of_exact_preactivation(native, c):
    ex = R.exact(c)
    ref, E = R.pointwise("act", ex.z, c.act)
    bits = _run(native, c, ex)
    keys = np.round(ex.z / ex.unit).astype(np.int64)
    _check_bounded(c, c.name, bits, c.obf, ref, E, keys, {2: "sigmoid", 3: "tanh", 4: "erf-GELU"}[c.act],
                   trans=R.apply_act_slow_f32(ex.z, c.act))


@pytest.mark.parametrize("c", R.CASES["K"], ids=lambda c: c.name)
def test_bn_stats_exact(native, c):
    ex = R.exact(c)
    A, B = R.operands(c)
    P = (c.M + 127) // 128
    assert native.gemm_bn_stat_rows(c.M) == P
    buf = OutBuf(c.M, c.N, torch.bfloat16, c.pc)
    part = torch.full((2 * P * c.N + 64,), SENT[torch.float32])
    part[:2 * P * c.N] = float("nan")
    dpart = part.cuda()
    assert native.gemm_bn_stats(R.on(A, "cuda"), c.tA, R.on(B, "cuda"), c.tB, buf.view, dpart)
    got = R.tensor_bits(buf.finish(c.name))
    msg = R.first_mismatch(c, got, R.bf16_rne(ex.z), what="y")
    assert msg is None, msg
    after = dpart.cpu()
    assert torch.equal(_ibits(after[2 * P * c.N:]), _ibits(part[2 * P * c.N:])), f"{c.name}: wrote past the 2 P N partials"
    gp = after[:2 * P * c.N].numpy().reshape(2, P, c.N)
    assert np.all(np.isfinite(gp)), f"{c.name}: {int(np.sum(~np.isfinite(gp)))} partials were not written"
    want = R.bn_partials(R.bf16_val(got), c.M)
    for t, what in ((0, "sum"), (1, "sum of squares")):
        bad = np.argwhere(R.f32_bits(gp[t]) != R.f32_bits(want[t]))
        assert bad.size == 0, (f"{c.name}: {what} partial differs at {len(bad)} entries; first (p={bad[0][0]}, "
                               f"n={bad[0][1]}): got {gp[t][tuple(bad[0])]!r}, stored values give {want[t][tuple(bad[0])]!r}")


def _ga(native, c, ex):
    A, B = R.operands(c)
    out = OutBuf(c.M, c.N, torch.bfloat16, c.pc)
    aux = OutBuf(c.M, c.N, torch.bfloat16, c.pc)
    assert native.gemm_gelu_aux(R.on(A, "cuda"), c.tA, R.on(B, "cuda"), c.tB, out.view, aux.view, _bias(ex.bias))
    return R.tensor_bits(out.finish(c.name, "h")), R.tensor_bits(aux.finish(c.name, "aux"))


@pytest.mark.parametrize("c", [c for c in R.CASES["L"] if c.kind == "ga"], ids=lambda c: c.name)
def test_gelu_aux(native, c):
    ex = R.exact(c)
    h, aux = _ga(native, c, ex)
    msg = R.first_mismatch(c, aux, R.bf16_rne(ex.z), what="aux")
    assert msg is None, msg
    ref, E = R.pointwise("gelu_fwd", ex.z)      # of the unrounded z, as the kernel uses it
    _check_bounded(c, c.name + " h", h, True, ref, E, np.round(ex.z / ex.unit).astype(np.int64), "gelu_fwd_f h")


def _dg(native, c):
    A, B = R.operands(c)
    aux64, bias64 = R.dg_inputs(c)
    P = c.M // 128
    out = OutBuf(c.M, c.N, torch.bfloat16, c.pc)
    aux = OutBuf(c.M, c.N, torch.bfloat16, c.pc, init=aux64)
    part = torch.full((P * c.N + 64,), SENT[torch.float32])
    part[:P * c.N] = float("nan")
    dpart = part.cuda()
    db0 = (((np.arange(c.N) * 29) % 41) - 20) / 8.0
    ddb = (torch.from_numpy(db0).float() if c.accumulate else torch.full((c.N,), float("nan"))).cuda()
    assert native.gemm_dgelu(R.on(A, "cuda"), c.tA, R.on(B, "cuda"), c.tB, out.view, aux.view, _bias(bias64), dpart,
                             ddb, c.accumulate)
    dU = R.tensor_bits(out.finish(c.name, "dU"))
    assert aux.unchanged(), f"{c.name}: aux (read-only) or its guards were written"
    after = dpart.cpu()
    assert torch.equal(_ibits(after[P * c.N:]), _ibits(part[P * c.N:])), f"{c.name}: wrote past the M/128 x N partials"
    return dU, after[:P * c.N].numpy().reshape(P, c.N).astype(np.float64), ddb.cpu().numpy().astype(np.float64), \
        aux64, bias64, db0


@pytest.mark.parametrize("c", [c for c in R.CASES["L"] if c.kind == "dg"], ids=lambda c: c.name)
def test_dgelu(native, c):
    dh = R.exact(c._replace(bias=False)).z
    dU, cp, db, aux64, bias64, db0 = _dg(native, c)
    s = aux64 + (0.0 if bias64 is None else bias64)
    ref, E, ref_cp, E_cp, ref_db, E_db = R.dgelu_bounds(dh, s, c.M)
    keys = (np.round(dh).astype(np.int64), np.round(s * 8).astype(np.int64))
    _check_bounded(c, c.name + " dU", dU, True, ref, E, keys, "gelu_grad2 dU")
    assert np.all(np.isfinite(cp)) and np.all(np.isfinite(db)), f"{c.name}: partials / dbias not all written"
    r = np.abs(cp - ref_cp) / E_cp
    _ratio("dgelu colpart", r.max())
    assert r.max() <= 1.0, f"{c.name}: colpart off by {r.max():.3f} of its bound at (p, n) = {np.unravel_index(r.argmax(), r.shape)}"
    if c.accumulate:      # one more fp32 add: db0 + sum
        E_db = E_db + R.U * (np.abs(db0 + ref_db) + E_db)
        ref_db = ref_db + db0
    r = np.abs(db - ref_db) / E_db
    _ratio("dgelu dbias", r.max())
    assert r.max() <= 1.0, f"{c.name}: dbias off by {r.max():.3f} of its bound at n = {int(r.argmax())}"


@pytest.mark.parametrize("c", [c for c in R.CASES["M"] if c.kind == "gemm"], ids=lambda c: c.name)
def test_gaussian_gemm(native, c):
    ex = R.exact(c)
    bits = _run(native, c, ex)
    assert _finite(bits, c.obf)
    y = R.bf16_val(bits) if c.obf else bits.view(np.float32).astype(np.float64)
    r = np.abs(y - ex.z) / R.gauss_bound(c, ex)
    _ratio("Gaussian C " + ("bf16" if c.obf else "fp32"), r.max())
    bad = np.argwhere(r > 1.0)
    assert bad.size == 0, f"{c.name}: {len(bad)} outside the bound, worst {r.max():.3f}; first {R.locate(c, *map(int, bad[0]))}"


def test_gaussian_bn_stats(native):
    c = next(c for c in R.CASES["M"] if c.kind == "stats")
    ex = R.exact(c)
    A, B = R.operands(c)
    P = (c.M + 127) // 128
    buf = OutBuf(c.M, c.N, torch.bfloat16, c.pc)
    dpart = torch.full((2 * P * c.N,), float("nan")).cuda()
    assert native.gemm_bn_stats(R.on(A, "cuda"), c.tA, R.on(B, "cuda"), c.tB, buf.view, dpart)
    y = R.bf16_val(R.tensor_bits(buf.finish(c.name)))
    r = np.abs(y - ex.z) / R.gauss_bound(c, ex)
    _ratio("Gaussian stats y", r.max())
    assert r.max() <= 1.0, r.max()
    gp = dpart.cpu().numpy().reshape(2, P, c.N).astype(np.float64)
    want = R.bn_partials(y, c.M)          # of the values the kernel stored
    mag = R.bn_partials(np.abs(y), c.M)
    # 128 terms: 127 additions, each rounding at most U times the running sum of magnitudes; a square is rounded once more
    r0 = np.abs(gp[0] - want[0]) / (127 * R.U * mag[0] + R.FLOOR)
    r1 = np.abs(gp[1] - want[1]) / (128 * R.U * mag[1] + R.FLOOR)
    _ratio("Gaussian stats partials", max(r0.max(), r1.max()))
    assert r0.max() <= 1.0 and r1.max() <= 1.0, (r0.max(), r1.max())


def test_gaussian_gelu_aux(native):
    c = next(c for c in R.CASES["M"] if c.kind == "ga")
    ex = R.exact(c)
    h, aux = _ga(native, c, ex)
    ez = R.gauss_bound(c._replace(obf=False), ex)          # of the fp32 z before it is rounded or activated
    r = np.abs(R.bf16_val(aux) - ex.z) / (ez + R.HB * np.abs(ex.z))
    _ratio("Gaussian gelu_aux aux", r.max())
    assert r.max() <= 1.0, r.max()
    ref, E = R.pointwise("gelu_fwd", ex.z.astype(np.float32).astype(np.float64))
    # |gelu'| <= 1.13: an error ez of z moves gelu(z) by at most 1.13 ez (U |z| more for the fp32 grid of the table)
    bound = E + 1.13 * (ez + R.U * np.abs(ex.z)) + R.HB * (np.abs(ref) + 1.13 * ez)
    r = np.abs(R.bf16_val(h) - R.gelu_fwd64(ex.z)) / bound
    _ratio("Gaussian gelu_aux h", r.max())
    assert r.max() <= 1.0, r.max()


def test_gaussian_dgelu(native):
    c = next(c for c in R.CASES["M"] if c.kind == "dg")
    ex = R.exact(c._replace(bias=False))
    dU, cp, db, aux64, bias64, _ = _dg(native, c)
    s = aux64 + bias64
    s32 = s.astype(np.float32).astype(np.float64)           # the kernel's fp32 sum: one rounding, U |s|
    g, Eg = R.pointwise("gelu_grad", s32)
    ez = R.gauss_bound(c._replace(obf=False), ex)
    ref = ex.z * R.gelu_grad64(s)
    # |gelu''| <= 1.2: the rounding of s moves g by at most 1.2 U |s|; |g| <= 1.13
    E = 1.13 * ez + (np.abs(ex.z) + ez) * (Eg + 1.2 * R.U * np.abs(s)) + R.ULP * np.abs(ref)
    r = np.abs(R.bf16_val(dU) - ref) / (E + R.HB * (np.abs(ref) + E))
    _ratio("Gaussian dgelu dU", r.max())
    assert r.max() <= 1.0, r.max()
    blk = lambda x: x.reshape(c.M // 128, 128, -1).sum(1)
    E_cp = blk(E) + 127 * R.U * (blk(np.abs(ref)) + blk(E))
    r = np.abs(cp - blk(ref)) / E_cp
    _ratio("Gaussian dgelu colpart", r.max())
    assert r.max() <= 1.0, r.max()
    E_db = E_cp.sum(0) + R.U * (np.abs(blk(ref)).sum(0) + E_cp.sum(0))
    r = np.abs(db - blk(ref).sum(0)) / E_db
    assert r.max() <= 1.0, r.max()


# ---- N: the contract.  Nothing is launched, False comes back, C and its guards keep their bits

def _strided(t, ld, off):
    parent = torch.zeros(off + t.shape[0] * ld + 8, dtype=t.dtype)
    parent.as_strided(t.shape, (ld, 1), off).copy_(t)
    return parent.cuda().as_strided(t.shape, (ld, 1), off)


def _ops(M, N, K, tA=False, tB=True, lda=None, ldb=None, offa=8):
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-3, 4, (K, M) if tA else (M, K), generator=g).bfloat16()
    b = torch.randint(-3, 4, (N, K) if tB else (K, N), generator=g).bfloat16()
    return _strided(a, lda or a.shape[1], offa), _strided(b, ldb or b.shape[1], 8)


_REJECT = {
    "K=100": dict(K=100),
    "lda%8": dict(K=128, lda=132),
    "A offset by 4 elements": dict(K=128, offa=4),
    "transA, M=12": dict(M=12, tA=True, tB=False, lda=16),
    "transB=False, N=12": dict(N=12, tB=False, ldb=16),
    "split_k=2, bf16 out": dict(K=1024, split_k=2, obf=True),
    "split_k=2, activation": dict(K=1024, split_k=2, act=1),
    "split_k=2, beta=0.5": dict(K=1024, split_k=2, beta=0.5),
}


@pytest.mark.parametrize("why", list(_REJECT), ids=lambda s: s.replace(" ", "_"))
def test_contract_rejects(native, why):
    kw = dict(M=256, N=256, K=128, tA=False, tB=True, offa=8, lda=None, ldb=None, split_k=1, obf=False, act=0,
              beta=0.0)
    kw.update(_REJECT[why])
    A, B = _ops(kw["M"], kw["N"], kw["K"], kw["tA"], kw["tB"], kw["lda"], kw["ldb"], kw["offa"])
    dt = torch.bfloat16 if kw["obf"] else torch.float32
    buf = OutBuf(kw["M"], kw["N"], dt, pc=1, init=np.ones((kw["M"], kw["N"])))
    for variant in (0, 4, 8):
        if variant == 8 and kw["K"] % 128:
            continue
        assert not native.gemm_big(A, kw["tA"], B, kw["tB"], buf.view, act=kw["act"], beta=kw["beta"],
                                   split_k=kw["split_k"], variant=variant)
    assert buf.unchanged()


@pytest.mark.parametrize("variant", [8, 9])
def test_8phase_variants_raise_on_odd_k_tiles(native, variant):
    A, B = _ops(256, 256, 192)
    buf = OutBuf(256, 256, torch.float32, pc=1)
    with pytest.raises(RuntimeError):
        native.gemm_big(A, False, B, True, buf.view, variant=variant)
    assert buf.unchanged()


@pytest.mark.parametrize("M,K", [(264, 128), (256, 192)])
def test_fused_gelu_contract(native, M, K):
    N = 256
    A, B = _ops(M, N, K)
    out = OutBuf(M, N, torch.bfloat16, pc=1)
    aux = OutBuf(M, N, torch.bfloat16, pc=1, init=np.ones((M, N)))
    bias = torch.zeros(N, device="cuda")
    part = torch.full((4 * N,), 5.0, device="cuda")
    db = torch.full((N,), 6.0, device="cuda")
    assert not native.gemm_gelu_aux(A, False, B, True, out.view, aux.view, bias)
    assert not native.gemm_dgelu(A, False, B, True, out.view, aux.view, bias, part, db, False)
    assert out.unchanged() and aux.unchanged()
    assert bool((part == 5.0).all()) and bool((db == 6.0).all())


def test_zz_measured_ratios():
    """Prints the worst error / allowance per quantity of this run (the figures
    in the module docstring); a ratio above 0.5 means the allowance is closer to
    the kernel than its derivation intends and wants a look."""
    for k in sorted(RATIOS):
        print(f"RATIO {k}: {RATIOS[k]:.3f}")
    assert all(v <= 1.0 for v in RATIOS.values())
