"""BatchNorm kernels (csrc/kernels/bn.hip) per element and per channel against
the float64 model of tests/bn_reference.py, at the tile, tail and grid edges.

The kernels are called directly on 2-D [M, C] bf16 tensors, so M is free.
Every output is the middle of a flat buffer with 4,096 sentinel elements on
each side (checked after every call); part / stats / coef are pre-filled with
NaN and must come back fully written.  The bounds are the derived ones of
bn_reference.py -- none is fitted to what the kernels give.

ReLU: the kernels recompute the mask in fp32, so an element whose float64
pre-activation lies within 4 * E_pre of zero may fall on either side; dy is set
to 0 there before the kernels run, and everywhere else g (= dres) must equal
dy * mask exactly.  Each ReLU case asserts <= 1 % ambiguous, >= 10 % masked and
>= 10 % unmasked elements, all from the reference alone.

Every case prints one JSON line of figures (pytest -s / -rP): the ambiguous and
masked shares and, per output, the worst observed error divided by its bound.

Figures on an MI355X when this file was written (worst error / bound over all
cases of a group):
  ReLU cases of A, B, D, H: ambiguous 0 ... 1.2e-4, masked 0.46 ... 0.53,
    unmasked 0.47 ... 0.54 of the elements.
  A, B, D, H, I (chain bounds): y 0.52 ... 0.995 and dx 0.59 ... 0.994 (the bf16
    rounding term b |ref| is reached by construction, at 1 / (1 + b)); mean 0.008,
    invstd 0.021, scale 0.030, shift 0.013, part 0.077, bpart 0.010, dgamma 0.0097,
    dbeta 0.0018, coef A / B / Cc 0.029 / 0.013 / 0.010 -- worst-case bounds
    against rounding errors that mostly cancel; one dropped row of 25,088 moves
    the mean by about ten times its bound.
  C (ulp bounds): mean, invstd, A and the plain dgamma / dbeta equal the
    fp32-rounded reference bit for bit; scale 0.13, shift 0.17, run_mean 0.25,
    run_var 0.28, B 0.25, Cc 0.20, accumulated dgamma / dbeta 0.50, y and dx 0.996.
  E: run_mean 0.038, run_var 0.039 (I: 0.14, 0.07).  F: invstd 0.18, scale 0.26, shift 0.23 (the
    constant channels, L = 0), the rest as A; the |mean| / std = 16 channels'
    invstd bound is 3.9e-3 relative.

`python tests/test_bn_edges_gpu.py child` is the body of test_env_selected_paths.
"""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import bn_reference as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = R.f32(1e-5)
MOM = R.f32(0.3)
GUARD = 4096          # multiple of 8 bf16 / 4 fp32: the middle stays 16-byte aligned
SENTINEL = -1024.0    # exact in bf16 and fp32
BIG = (65600, 512)    # 4,198,400 chunks > 16,384 blocks x 256 threads: the grid-stride trip
NAN = float("nan")
RR = [(False, True), (True, True), (False, False), (True, False)]


class Guarded:
    """n elements between two guards of GUARD sentinels; .t is the middle (a view)."""

    def __init__(self, n, dtype, shape=None, fill=NAN):
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill)
        else:
            self.t.fill_(fill)
        if shape is not None:
            self.t = self.t.view(shape)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        s = torch.full((), SENTINEL, dtype=self.buf.dtype, device="cuda")
        return bool((self.buf[:GUARD] == s).all()) and bool((self.buf[-GUARD:] == s).all())


class Report:
    """Figures (worst error / bound per output, shares) and failures of one case."""

    def __init__(self, name):
        self.name, self.fig, self.fail = name, {}, []

    def bound(self, what, got, ref, tol):
        got = got.to(ref.device).double().reshape(ref.shape)
        err = (got - ref).abs()
        tol = tol.expand_as(err)
        bad = ~(err <= tol)                      # a NaN is beyond every bound
        worst = float((err / tol.clamp_min(1e-300)).max())
        self.fig[what] = float("%.3g" % worst)
        if bool(bad.any()):
            i = int(bad.reshape(-1).nonzero()[0])
            self.fail.append("%s: %d of %d beyond the bound, worst error / bound %.3g, first at flat index %d "
                             "(got %r, reference %r, bound %r)" % (what, int(bad.sum()), bad.numel(), worst, i,
                                                                   float(got.reshape(-1)[i]),
                                                                   float(ref.reshape(-1)[i]),
                                                                   float(tol.reshape(-1)[i])))

    def true(self, what, cond):
        if not bool(cond):
            self.fail.append(what)

    def guards(self, **bufs):
        for k, b in bufs.items():
            if b is not None:
                self.true("guard of %s overwritten" % k, b.intact())

    def done(self):
        print(json.dumps({"case": self.name, **self.fig}))
        assert not self.fail, "%s:\n  %s" % (self.name, "\n  ".join(self.fail))


def ref_dev(M, C):
    """Small cases keep their float64 reference on the CPU, large ones on the device."""
    return "cpu" if M * C <= (1 << 20) else "cuda"


@functools.lru_cache(maxsize=3)
def make_inputs(M, C, seed=0):
    """x ~ N(0.5, 2^2), res ~ N(0, 1), dy ~ N(0, 1) as bf16; gamma in [0.5, 1.5],
    beta in [-0.5, 0.5].  Seeded; drawn where the reference will live."""
    dev = ref_dev(M, C)
    g = torch.Generator(device=dev).manual_seed(7919 * M + C + seed)
    x = (torch.randn(M, C, device=dev, generator=g) * 2 + 0.5).bfloat16().cuda()
    r = torch.randn(M, C, device=dev, generator=g).bfloat16().cuda()
    dy = torch.randn(M, C, device=dev, generator=g).bfloat16().cuda()
    gamma = (torch.rand(C, device=dev, generator=g) + 0.5).cuda()
    beta = (torch.rand(C, device=dev, generator=g) - 0.5).cuda()
    return x, r, dy, gamma, beta


def group_sums(P, grp, *terms):
    """[len(terms), P, C] float64 sums of the terms' rows over the groups grp."""
    out = torch.zeros(len(terms), P, terms[0].shape[1], dtype=torch.float64, device=terms[0].device)
    for i, t in enumerate(terms):
        out[i].index_add_(0, grp, t)
    return out


def launch(C_, x, r, dy, gamma, beta, relu, rm=None, rv=None, dg0=None, db0=None, backward=True):
    """bn_fwd then bn_bwd into guarded buffers; dg0 / db0: prefill, accum = 1."""
    M, C = x.shape
    P = C_.bn_partial_rows(M, C)
    o = dict(y=Guarded(M * C, torch.bfloat16, (M, C)), part=Guarded(2 * P * C, torch.float32),
             stats=Guarded(4 * C, torch.float32))
    C_.bn_fwd(x, r, gamma, beta, o["y"].t, o["part"].t, o["stats"].t, rm, rv, MOM, EPS, relu)
    if backward:
        o.update(dx=Guarded(M * C, torch.bfloat16, (M, C)),
                 dres=Guarded(M * C, torch.bfloat16, (M, C)) if r is not None else None,
                 bpart=Guarded(2 * P * C, torch.float32), coef=Guarded(3 * C, torch.float32),
                 dgamma=Guarded(C, torch.float32, fill=NAN if dg0 is None else dg0),
                 dbeta=Guarded(C, torch.float32, fill=NAN if db0 is None else db0))
        C_.bn_bwd(dy, x, r, gamma, o["stats"].t, o["bpart"].t, o["coef"].t, o["dx"].t,
                  o["dres"].t if r is not None else None, o["dgamma"].t, o["dbeta"].t, relu, dg0 is not None)
    torch.cuda.synchronize()
    return o


def run_full(C_, M, C, res, relu, name, inputs=None, accum=False, exact_sum_channels=None, keep=None):
    """bn_fwd + bn_bwd on [M, C] against the reference: statistics, the [2, P, C]
    partials per partial row, y, dx, dres, dgamma, dbeta, coef.  Returns the Report.
    exact_sum_channels: channels whose x and x^2 sums are exact in fp32 (constant
    small-integer-like values), so their statistics carry no chain error (L = 0).
    keep: a dict that receives the tensors a follow-up check needs."""
    rep = Report(name)
    x, r, dy, gamma, beta = inputs if inputs is not None else make_inputs(M, C)
    r = r if res else None
    dev = ref_dev(M, C)
    P = C_.bn_partial_rows(M, C)
    L = R.chain_len(M, P)
    xr, gr, br = x.to(dev), gamma.to(dev), beta.to(dev)
    rr = r.to(dev) if res else None

    mean, invstd, scale, shift, pre, yref, _, _ = R.fwd(xr, gr, br, rr, relu, EPS)
    Ls = torch.full((C,), float(L), dtype=torch.float64, device=dev)
    if exact_sum_channels is not None:
        Ls[exact_sum_channels] = 0.0
    t = R.tol_stats(xr, gr, br, mean, invstd, scale, EPS, Ls)
    epre = R.e_pre(xr, rr, scale, shift, t)
    if relu:
        amb = pre.abs() <= 4 * epre
        mask = pre > 0
        n = float(pre.numel())
        rep.fig["ambiguous"] = float("%.3g" % (float(amb.sum()) / n))
        rep.fig["masked"] = float("%.3g" % (float((~mask & ~amb).sum()) / n))
        rep.fig["unmasked"] = float("%.3g" % (float((mask & ~amb).sum()) / n))
        rep.true("more than 1 %% ambiguous: %r" % rep.fig["ambiguous"], rep.fig["ambiguous"] <= 0.01)
        rep.true("fewer than 10 %% masked: %r" % rep.fig["masked"], rep.fig["masked"] >= 0.10)
        rep.true("fewer than 10 %% unmasked: %r" % rep.fig["unmasked"], rep.fig["unmasked"] >= 0.10)
        dy = torch.where(amb.to(dy.device), torch.zeros_like(dy), dy)
    dyr = dy.to(dev)

    dg0 = db0 = None
    if accum:
        g0 = torch.Generator(device="cpu").manual_seed(M + C)
        dg0 = torch.randn(C, generator=g0).cuda()
        db0 = torch.randn(C, generator=g0).cuda()
    o = launch(C_, x, r, dy, gamma, beta, relu, dg0=dg0, db0=db0)
    rep.guards(**o)
    for k in ("part", "stats", "bpart", "coef", "dgamma", "dbeta"):
        rep.true("%s not fully written / not finite" % k, torch.isfinite(o[k].t).all())

    # forward statistics
    st = o["stats"].t.to(dev).double().reshape(4, C)
    rep.bound("mean", st[0], mean, t["mean"])
    rep.bound("invstd", st[1], invstd, t["invstd"])
    rep.bound("scale", st[2], scale, t["scale"])
    rep.bound("shift", st[3], shift, t["shift"])
    # the partials, per partial row: block (., p) sums rows p * 32 + lane, stepping 32 * P
    grp = (torch.arange(M, device=dev) // 32) % P
    xd = xr.double()
    sums = group_sums(P, grp, xd, xd * xd)
    mags = group_sums(P, grp, xd.abs(), xd * xd)
    rep.bound("part", o["part"].t.reshape(2, P, C), sums, 2 * Ls * R.U * mags + R.TINY)
    part2 = Guarded(2 * P * C, torch.float32)
    rep.true("bn_stat_partials returns P", C_.bn_stat_partials(x, part2.t) == P)
    rep.guards(part2=part2)
    rep.true("bn_stat_partials == bn_fwd's partials", torch.equal(part2.t, o["part"].t))
    # y
    rep.bound("y", o["y"].t, yref, R.tol_y(yref, epre))

    # backward
    g, dxr, dresr, dgamma, dbeta = R.bwd(dyr, xr, rr, gr, (mean, invstd, scale, shift), relu)
    coef = R.coef_of(gr, mean, invstd, dgamma, dbeta, M)
    dg0r = dg0.to(dev) if accum else None
    db0r = db0.to(dev) if accum else None
    tb = R.tol_bwd(g, xr, gr, mean, invstd, dgamma, dbeta, coef, t, L, M, dg0r, db0r)
    rep.bound("dgamma", o["dgamma"].t, dgamma + dg0r.double() if accum else dgamma, tb["dgamma"])
    rep.bound("dbeta", o["dbeta"].t, dbeta + db0r.double() if accum else dbeta, tb["dbeta"])
    kc = o["coef"].t.to(dev).double().reshape(3, C)
    rep.bound("coefA", kc[0], coef[0], tb["A"])
    rep.bound("coefB", kc[1], coef[1], tb["B"])
    rep.bound("coefC", kc[2], coef[2], tb["Cc"])
    xhat = (xd - mean) * invstd
    bsum = group_sums(P, grp, g, g * xhat)
    bmag = group_sums(P, grp, g.abs(), (g * xhat).abs())
    # the kernel's x_hat uses its own statistics: see tol_bwd
    btol = 2 * L * R.U * bmag + R.TINY
    btol[1] = btol[1] + bmag[0] * invstd * t["mean"] + bmag[1] * t["rel_invstd"]
    rep.bound("bpart", o["bpart"].t.reshape(2, P, C), bsum, btol)
    rep.bound("dx", o["dx"].t, dxr, R.tol_dx(dxr, g, xr, coef, tb))
    if res:
        rep.true("dres != dy * mask exactly", torch.equal(o["dres"].t, g.to(torch.bfloat16).cuda()))
    if keep is not None:
        keep.update(o=o, x=x, r=r, dy=dy, gamma=gamma, beta=beta, g=g, ref=(mean, invstd, scale, shift), tol=t,
                    yref=yref, dxr=dxr, dev=dev)
    return rep


def check_bwd_parts(C_, rep, tag, g, x, gamma, stats32, P, accum):
    """bn_bwd_parts on partials built in torch: float64 sums of g and g * x_hat
    over the row groups r % P, rounded to fp32; x_hat from the fp32 statistics
    the kernel is handed.  The reference finalises those same fp32 numbers in
    float64 and the kernel sums them in double, so only the final roundings
    differ: dgamma / dbeta within 2 ulp, coef within 8 ulp (Cc: of its terms)."""
    M, C = x.shape
    dev = ref_dev(M, C)
    xd, gd = x.to(dev).double(), g.to(dev).double()
    s32 = stats32.to(dev).reshape(4, C)
    mean, invstd = s32[0].double(), s32[1].double()
    grp = torch.arange(M, device=dev) % P
    part = group_sums(P, grp, gd, gd * (xd - mean) * invstd).float()
    dg0 = db0 = None
    if accum:
        g0 = torch.Generator(device="cpu").manual_seed(P + C)
        dg0, db0 = torch.randn(C, generator=g0), torch.randn(C, generator=g0)
    o = dict(coef=Guarded(3 * C, torch.float32), dx=Guarded(M * C, torch.bfloat16, (M, C)),
             dgamma=Guarded(C, torch.float32, fill=dg0.cuda() if accum else NAN),
             dbeta=Guarded(C, torch.float32, fill=db0.cuda() if accum else NAN))
    C_.bn_bwd_parts(g, x, gamma, stats32, part.cuda().contiguous(), P, o["coef"].t, o["dx"].t, o["dgamma"].t,
                    o["dbeta"].t, accum)
    torch.cuda.synchronize()
    rep.guards(**{tag + k: v for k, v in o.items()})
    rep.true(tag + "coef not fully written", torch.isfinite(o["coef"].t).all())
    gr = gamma.to(dev)
    dgamma, dbeta, (A, Bc, Cc) = R.finalize_from_parts_bwd(part, P, M, gr, mean, invstd,
                                                           dg0.to(dev) if accum else None,
                                                           db0.to(dev) if accum else None)
    sg, sgx = part.double()[0].sum(0), part.double()[1].sum(0)
    # the two double sums run in different orders: P * 2^-53 of the magnitudes
    dbl = P * 2.0 ** -53 * part.double().abs().sum(1)
    z = torch.zeros_like(sg)
    rep.bound(tag + "dbeta", o["dbeta"].t, dbeta.float().double(),
              R.ulps(2, sg, db0.to(dev).double() if accum else z) + dbl[0])
    rep.bound(tag + "dgamma", o["dgamma"].t, dgamma.float().double(),
              R.ulps(2, sgx, dg0.to(dev).double() if accum else z) + dbl[1])
    tb = dict(A=R.ulps(8, A), B=R.ulps(8, Bc), Cc=R.ulps(8, A * sg / M, Bc * mean))
    kc = o["coef"].t.to(dev).double().reshape(3, C)
    rep.bound(tag + "coefA", kc[0], A.float().double(), tb["A"])
    rep.bound(tag + "coefB", kc[1], Bc.float().double(), tb["B"])
    rep.bound(tag + "coefC", kc[2], Cc.float().double(), tb["Cc"])
    dxr = A * gd + Bc * xd + Cc
    rep.bound(tag + "dx", o["dx"].t, dxr, R.tol_dx(dxr, gd, xd, (A, Bc, Cc), tb))


# ---- A. partials-pass tiling ------------------------------------------------------------------

A_SHAPES = [
    ((3, 8), RR),            # one chunk; one row lane of 32 busy; M / (M - 1) = 1.5
    ((33, 72), RR),          # one row past the lanes; second channel tile 8 wide (c0 + c < C)
    ((257, 64), RR),         # P = 2: one Rows<4> trip, then a tail trip for a single lane
    ((1031, 136), RR),       # prime M, P = 5, ragged tails, C % 64 != 0
    ((8200, 2048), RR[:2]),  # 32 channel tiles, P = 33, FC = 16
    ((131075, 64), RR[:2]),  # bn_grid's 512 cap, FC = 4
]                            # (65600, 512), the cap = 2048 / ct branch (P = 256): test_grid_stride_passes
A_CASES = [(s, rr) for s, rrs in A_SHAPES for rr in rrs]
EXPECT_P = {(3, 8): 1, (33, 72): 1, (257, 64): 2, (1031, 136): 5, (8200, 2048): 33, (131075, 64): 512, BIG: 256}


@pytest.mark.parametrize("shape,rr", A_CASES, ids=lambda v: "-".join(str(int(i)) for i in v))
def test_tiling(native, shape, rr):
    M, C = shape
    assert native.bn_partial_rows(M, C) == EXPECT_P[shape]
    run_full(native, M, C, rr[0], rr[1], "A %dx%d res=%d relu=%d" % (M, C, rr[0], rr[1])).done()


# ---- B. grid-stride elementwise passes at the production cap ----------------------------------

@pytest.mark.parametrize("rr", RR[:3], ids=lambda v: "-".join(str(int(i)) for i in v))
def test_grid_stride_passes(native, rr):
    """(65600, 512): threads 0 ... 4,095 of the 16,384 x 256 take a second trip in
    bn_apply and bn_bwd_apply; also case A's cap = 2048 / ct branch (P = 256).
    Then bn_bwd_parts (bn_bwd_apply<false, false>) on the same tensors."""
    M, C = BIG
    assert native.bn_partial_rows(M, C) == EXPECT_P[BIG]
    assert M * C // 8 > 16384 * 256
    keep = {}
    rep = run_full(native, M, C, rr[0], rr[1], "B %dx%d res=%d relu=%d" % (M, C, rr[0], rr[1]), keep=keep)
    check_bwd_parts(native, rep, "parts.", keep["g"].to(torch.bfloat16).cuda(), keep["x"], keep["gamma"],
                    keep["o"]["stats"].t, 256, False)
    rep.done()


@functools.lru_cache(maxsize=1)
def exact_inputs():
    """x, res: bf16 N(0, 1) rounded to multiples of 2^-12 (still bf16: only values
    below 2^-5 lose bits), scale = +-2^k, k in -2 ... 2, shift a multiple of 1/8
    in [-4, 4].  Then x * scale + shift + res is a multiple of 2^-14 below 2^6:
    exact in fp32 in any association, fused or not."""
    M, C = BIG
    g = torch.Generator(device="cuda").manual_seed(99)
    q = lambda t: (torch.round(t.bfloat16().float() * 4096) / 4096).bfloat16()
    x = q(torch.randn(M, C, device="cuda", generator=g))
    r = q(torch.randn(M, C, device="cuda", generator=g))
    k = torch.randint(-2, 3, (C,), device="cuda", generator=g)
    sign = torch.randint(0, 2, (C,), device="cuda", generator=g) * 2 - 1
    scale = (sign * torch.pow(2.0, k.float())).float()
    shift = (torch.randint(-32, 33, (C,), device="cuda", generator=g).float() / 8)
    assert torch.equal(x.float() * 4096, torch.round(x.float() * 4096))
    return x, r, scale, shift


@pytest.mark.parametrize("rr", RR, ids=lambda v: "-".join(str(int(i)) for i in v))
def test_bn_apply_bit_exact(native, rr):
    """The bound bn_apply entry point, all four template variants: y must EQUAL the
    reference rounded to bf16, which pins every chunk of the two trips to its place."""
    M, C = BIG
    res, relu = rr
    x, r, scale, shift = exact_inputs()
    ref = x.double() * scale.double() + shift.double()
    if res:
        ref = ref + r.double()
    if relu:
        ref = ref.clamp_min(0)
    assert torch.equal(ref.float().double(), ref)          # exact in fp32, as claimed
    y = Guarded(M * C, torch.bfloat16, (M, C))
    native.bn_apply(x, r if res else None, scale, shift, y.t, relu)
    torch.cuda.synchronize()
    assert y.intact()
    want = ref.float().bfloat16()
    if not torch.equal(y.t, want):
        bad = (y.t != want) | torch.isnan(y.t)
        i = bad.reshape(-1).nonzero()
        raise AssertionError("%d elements differ, first at chunk %d, last at chunk %d of %d"
                             % (int(bad.sum()), int(i[0]) // 8, int(i[-1]) // 8, M * C // 8))


# ---- C. finalize kernels on producer-supplied partials ----------------------------------------

C_CASES = ([(64, P) for P in (1, 255, 256, 257, 1024, 1025, 3136)]      # FC 4, FG 256
           + [(520, P) for P in (127, 129, 513)]                        # FC 8, FG 128
           + [(1032, P) for P in (63, 65, 257, 3136)])                  # FC 16, FG 64, last block half empty


@pytest.mark.parametrize("C,P", C_CASES)
def test_finalize_on_supplied_partials(native, C, P):
    """bn_fwd_parts and bn_bwd_parts (accum 0 and 1) on partials built in torch over
    the row groups r % P of a real x with M = 2 P + 3 rows (P = 1: M = 64)."""
    M = 64 if P == 1 else 2 * P + 3
    rep = Report("C C=%d P=%d" % (C, P))
    x, r, dy, gamma, beta = make_inputs(M, C, seed=P)
    dev = ref_dev(M, C)
    xd, rd, gr, br = x.to(dev).double(), r.to(dev).double(), gamma.to(dev), beta.to(dev)
    grp = torch.arange(M, device=dev) % P
    part = group_sums(P, grp, xd, xd * xd).float()
    g0 = torch.Generator(device="cpu").manual_seed(C + P)
    rm0, rv0 = torch.randn(C, generator=g0), torch.rand(C, generator=g0) + 0.5
    mean, invstd, scale, shift, nrm, nrv = R.finalize_from_parts(part, P, M, gr, br, EPS, MOM, rm0.to(dev),
                                                                 rv0.to(dev))
    y = Guarded(M * C, torch.bfloat16, (M, C))
    stats = Guarded(4 * C, torch.float32)
    rm, rv = Guarded(C, torch.float32, fill=rm0.cuda()), Guarded(C, torch.float32, fill=rv0.cuda())
    native.bn_fwd_parts(x, r, gamma, beta, y.t, part.cuda().contiguous(), P, stats.t, rm.t, rv.t, MOM, EPS, True)
    torch.cuda.synchronize()
    rep.guards(y=y, stats=stats, run_mean=rm, run_var=rv)
    rep.true("stats not fully written", torch.isfinite(stats.t).all())
    dbl = P * 2.0 ** -53 * part.double().abs().sum(1) / M
    st = stats.t.to(dev).double().reshape(4, C)
    f = lambda v: v.float().double()
    t = dict(scale=R.ulps(8, scale), shift=R.ulps(8, br.double(), mean * scale))
    rep.bound("mean", st[0], f(mean), R.ulps(2, mean) + dbl[0])
    rep.bound("invstd", st[1], f(invstd), R.ulps(8, invstd))
    rep.bound("scale", st[2], f(scale), t["scale"])
    rep.bound("shift", st[3], f(shift), t["shift"])
    var = 1.0 / (invstd * invstd) - EPS
    unb = var * M / (M - 1)
    # run = (1 - m) run + m v in fp32: 1 - m, v's conversion, two products and the sum
    rep.bound("run_mean", rm.t, nrm, R.ulps(4, (1 - MOM) * rm0.to(dev).double(), MOM * mean))
    rep.bound("run_var", rv.t, nrv, R.ulps(4, (1 - MOM) * rv0.to(dev).double(), MOM * unb))
    pre = xd * scale + shift + rd
    yref = pre.clamp_min(0)
    rep.bound("y", y.t, yref, R.tol_y(yref, R.e_pre(xd, rd, scale, shift, t)))

    stats32 = torch.stack([mean, invstd, scale, shift]).float().reshape(-1).cuda()
    g = torch.where((pre > 0).to(dy.device), dy, torch.zeros_like(dy))
    for accum in (False, True):
        check_bwd_parts(native, rep, "accum%d." % accum, g, x, gamma, stats32, P, accum)
    rep.done()


# ---- D. accum = 1 on bn_bwd -------------------------------------------------------------------

def test_bwd_accumulates_into_prefilled_grads(native):
    run_full(native, 1031, 136, True, True, "D 1031x136 accum", accum=True).done()


# ---- E. running statistics --------------------------------------------------------------------

@pytest.mark.parametrize("M,C", [(3, 8), (1031, 136)])
def test_running_statistics_two_steps(native, M, C):
    """Random start values, momentum 0.3, two consecutive bn_fwd calls on different x;
    both buffers per channel after each.  Step 2 starts from what step 1 left (fp32).
    Then run_mean = run_var = None: nothing else may change."""
    rep = Report("E %dx%d" % (M, C))
    P = native.bn_partial_rows(M, C)
    L = R.chain_len(M, P)
    g0 = torch.Generator(device="cpu").manual_seed(M)
    rm = Guarded(C, torch.float32, fill=torch.randn(C, generator=g0).cuda())
    rv = Guarded(C, torch.float32, fill=(torch.rand(C, generator=g0) + 0.5).cuda())
    for step in (1, 2):
        x, r, dy, gamma, beta = make_inputs(M, C, seed=step)
        rm0, rv0 = rm.t.cpu().clone(), rv.t.cpu().clone()
        o = launch(native, x, r, dy, gamma, beta, True, rm=rm.t, rv=rv.t, backward=False)
        rep.guards(run_mean=rm, run_var=rv, **o)
        xr, gr, br = x.cpu(), gamma.cpu(), beta.cpu()
        mean, invstd, scale, shift, pre, yref, nrm, nrv = R.fwd(xr, gr, br, r.cpu(), True, EPS, MOM, rm0, rv0)
        t = R.tol_stats(xr, gr, br, mean, invstd, scale, EPS, L)
        d_rm, d_rv = R.tol_running(t, MOM, M, rm0, rv0, mean, 1.0 / (invstd * invstd) - EPS)
        rep.bound("run_mean.%d" % step, rm.t, nrm, d_rm)
        rep.bound("run_var.%d" % step, rv.t, nrv, d_rv)
        rep.bound("y.%d" % step, o["y"].t, yref, R.tol_y(yref, R.e_pre(xr, r.cpu(), scale, shift, t)))
    # the track_running_stats=False call on step 2's x
    n = launch(native, x, r, dy, gamma, beta, True, backward=False)
    rep.guards(**n)
    for k in ("y", "part", "stats"):
        rep.true("%s differs without running buffers" % k, torch.equal(n[k].t, o[k].t))
    rep.done()


# ---- F. numeric edges -------------------------------------------------------------------------

CONST = slice(128, 136)    # the 8-wide last channel tile
FAR = slice(8, 16)


def edge_inputs():
    x, r, dy, gamma, beta = (t.clone() for t in make_inputs(1031, 136, seed=5))
    g = torch.Generator(device="cpu").manual_seed(16)
    x[:, CONST] = 3.0
    x[:, FAR] = (torch.randn(1031, 8, generator=g) * 0.5 + 8.0).bfloat16().cuda()
    return x, r, dy, gamma, beta


@pytest.mark.parametrize("rr", [(False, False), (True, False)], ids=lambda v: "-".join(str(int(i)) for i in v))
def test_numeric_edges(native, rr):
    """Eight constant channels (3.0) and eight with |mean| / std = 16, on (1031, 136).
    Without ReLU: the wide derived E_pre of the |mean| / std = 16 channels would
    make 1.4 % of the case's elements ambiguous, over the 1 % every ReLU case allows.

    Constant channels: every sum of 3.0 and of 9.0 over up to 1031 rows is an
    integer below 2^24, exact in fp32 in any order, so the statistics carry no
    chain error (L = 0): invstd = 1 / sqrt(eps) to 4u, y = beta (+ res), no NaN.
    x_hat = 0 there, so dgamma = 0 and B = 0; dx itself is gamma / sqrt(eps) *
    (g - mean g), not 0 -- it is checked against the reference like every dx.

    |mean| / std = 16: the E[x^2] - mean^2 bound, d_var = 2Lu (E[x^2] + 2 |mean| E|x|)
    against var + eps, about 770 times the bound of a centred channel, holds as derived."""
    M, C = 1031, 136
    res, relu = rr
    keep = {}
    rep = run_full(native, M, C, res, relu, "F 1031x136 res=%d relu=%d" % rr, inputs=edge_inputs(),
                   exact_sum_channels=CONST, keep=keep)
    o, (mean, invstd, scale, shift) = keep["o"], keep["ref"]
    for k in ("y", "dx"):
        rep.true("NaN / Inf in %s" % k, torch.isfinite(o[k].t.float()).all())
    st = o["stats"].t.cpu().double().reshape(4, C)
    want = torch.full((8,), 1.0 / EPS ** 0.5, dtype=torch.float64)
    rep.bound("const.invstd", st[1, CONST], want, 4 * R.U * want)
    rep.bound("const.mean", st[0, CONST], torch.full((8,), 3.0, dtype=torch.float64), torch.zeros(8) + R.TINY)
    rep.bound("const.dgamma", o["dgamma"].t[CONST], torch.zeros(8, dtype=torch.float64), torch.zeros(8) + R.TINY)
    rep.bound("const.coefB", o["coef"].t[C:2 * C][CONST], torch.zeros(8, dtype=torch.float64),
              torch.zeros(8) + R.TINY)
    if not res and not relu:
        b = keep["beta"].cpu().double()[CONST].expand(M, 8)
        t = keep["tol"]
        ep = R.e_pre(keep["x"].cpu(), None, scale, shift, t)[:, CONST]
        rep.bound("const.y=beta", o["y"].t[:, CONST], b, R.tol_y(b, ep))
    far = keep["tol"]["rel_invstd"][FAR]
    rep.fig["far.rel_invstd_bound"] = float("%.3g" % float(far.max()))
    rep.true("the |mean| / std = 16 bound is vacuous (>= 1)", float(far.max()) < 1.0)
    rep.done()


# ---- G. determinism ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,C", [(1031, 136), BIG])
def test_two_runs_are_bit_identical(native, M, C):
    x, r, dy, gamma, beta = make_inputs(M, C)
    a = launch(native, x, r, dy, gamma, beta, True)
    b = launch(native, x, r, dy, gamma, beta, True)
    for k in a:
        assert a[k].intact() and b[k].intact(), k
        assert not torch.isnan(a[k].t.float()).any(), k
        assert torch.equal(a[k].t, b[k].t), k


# ---- H. the env-selected paths, in a fresh child process --------------------------------------

CHILD_ENV = {"DTF_BN_WRITE_G": "0", "DTF_BN_EW_CAP": "2"}


def _child():
    """Cases A on (1031, 136) and (257, 64), all four (res, relu), under CHILD_ENV:
    17,527 chunks on 2 x 256 threads (35 trips), and the (dy, x, res) backward
    bn_bwd_partials<true, true, false> + bn_bwd_apply<true, true>."""
    assert all(os.environ.get(k) == v for k, v in CHILD_ENV.items())
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    from distributed_tensorflow_example_amd import _native
    C_ = _native.load()
    cases = []
    for M, C in ((1031, 136), (257, 64)):
        for res, relu in RR:
            rep = run_full(C_, M, C, res, relu, "H %dx%d res=%d relu=%d" % (M, C, res, relu))
            cases.append({"case": rep.name, "fig": rep.fig, "fail": rep.fail})
    ok = all(not c["fail"] for c in cases)
    print(json.dumps({"ok": ok, "cases": cases}))
    return 0 if ok else 1


def test_env_selected_paths():
    env = dict(os.environ, **CHILD_ENV)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, cwd=REPO, timeout=180,
                       capture_output=True, text=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    out = json.loads(lines[-1])
    print(lines[-1])
    failed = [(c["case"], c["fail"]) for c in out["cases"] if c["fail"]]
    assert not failed, failed
    assert p.returncode == 0 and out["ok"], (p.returncode, p.stderr[-2000:])
    assert len(out["cases"]) == 8


# ---- I. module path ---------------------------------------------------------------------------

@pytest.mark.parametrize("track", [True, False])
def test_module_residual_without_relu(native, track):
    """FusedBatchNorm2d(residual=..., relu=False) on a channels_last (2, 72, 5, 7)
    input, with and without running statistics, per channel against the reference."""
    from distributed_tensorflow_example_amd.ops.bn import FusedBatchNorm2d

    N, C, H, W = 2, 72, 5, 7
    M = N * H * W
    rep = Report("I track=%d" % track)
    x2, r2, dy2, gamma, beta = make_inputs(M, C, seed=3)
    cl = lambda t: t.reshape(N, H, W, C).permute(0, 3, 1, 2)      # channels_last view of the [M, C] rows
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(M, C)
    bn = FusedBatchNorm2d(C, track_running_stats=track).cuda()
    mom = R.f32(bn.momentum)
    g0 = torch.Generator(device="cpu").manual_seed(4)
    rm0, rv0 = torch.randn(C, generator=g0), torch.rand(C, generator=g0) + 0.5
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        if track:
            bn.running_mean.copy_(rm0)
            bn.running_var.copy_(rv0)
    x = cl(x2).detach().requires_grad_()
    r = cl(r2).detach().requires_grad_()
    assert x.is_contiguous(memory_format=torch.channels_last)
    y = bn(x, residual=r, relu=False)
    y.backward(cl(dy2))
    torch.cuda.synchronize()
    assert y.is_contiguous(memory_format=torch.channels_last)

    xr, rr, gr, br = x2.cpu(), r2.cpu(), gamma.cpu(), beta.cpu()
    L = R.chain_len(M, native.bn_partial_rows(M, C))
    mean, invstd, scale, shift, pre, yref, nrm, nrv = R.fwd(xr, gr, br, rr, False, R.f32(bn.eps), mom,
                                                            rm0 if track else None, rv0 if track else None)
    t = R.tol_stats(xr, gr, br, mean, invstd, scale, R.f32(bn.eps), L)
    rep.bound("y", rows(y.detach()), yref, R.tol_y(yref, R.e_pre(xr, rr, scale, shift, t)))
    g, dxr, dresr, dgamma, dbeta = R.bwd(dy2.cpu(), xr, rr, gr, (mean, invstd, scale, shift), False)
    coef = R.coef_of(gr, mean, invstd, dgamma, dbeta, M)
    tb = R.tol_bwd(g, xr, gr, mean, invstd, dgamma, dbeta, coef, t, L, M)
    rep.bound("dx", rows(x.grad), dxr, R.tol_dx(dxr, g, xr, coef, tb))
    rep.true("residual gradient != dy", torch.equal(rows(r.grad), dy2))
    rep.bound("dgamma", bn.weight.grad, dgamma, tb["dgamma"])
    rep.bound("dbeta", bn.bias.grad, dbeta, tb["dbeta"])
    if track:
        d_rm, d_rv = R.tol_running(t, mom, M, rm0, rv0, mean, 1.0 / (invstd * invstd) - R.f32(bn.eps))
        rep.bound("run_mean", bn.running_mean, nrm, d_rm)
        rep.bound("run_var", bn.running_var, nrv, d_rv)
        assert int(bn.state_dict()["num_batches_tracked"]) == 1
    else:
        assert bn.running_mean is None and bn.running_var is None
    rep.done()


if __name__ == "__main__":
    if sys.argv[1:] != ["child"]:
        sys.exit("usage: %s child" % sys.argv[0])
    sys.exit(_child())
