"""The row kernels of csrc/kernels/transformer.hip per element against the float64
models of tests/transformer_reference.py, with its derived bounds -- none is fitted
to what the kernels give -- the dropout bits read off exactly, and the reducers
compared exactly on integer-valued data.

The raw bindings are called, so buffers, the ln_bwd / bias_gelu_bwd grid (the size
of the partial buffer) and seeds are the test's.  Every output is the middle of a
flat buffer with 4,096 sentinel elements on each side and is pre-filled with NaN:
after each call the guards must be intact and no NaN left.

  LN       bdrln_fwd (the 16-byte form), ln_fwd_f32in, emb_ln_fwd: y, s, mean, rstd at
           every template width (H = 256 ... 4096) and N = 1 ... 37 around the two-row
           tail and the eight-row block, a cancellation case, dropout on both hash
           branches; ln_bwd on the kernel's own s / mean / rstd with the partial
           buffer sized for grid = 1, ceil(N / 4) and ceil(N / 4) + 2, without dxb, with
           only some of dgamma / dbeta / dbias; dbeta exact on integer-valued dy.
  bits     the dropped set equals hash32's bit for bit: s == res (or 0), y == 0, dxb == 0,
           Pd == 0, dropout_bf16's y == 0 exactly there.
  emb      emb_bwd_aux exact on integer-valued ds, both values of accumulate.
  GELU     the 4-wide (H % 8 == 4) and 8-wide kernels around the 1024-column strip,
           backward with slices 1, 3, N, N + 2: y, dx, dbias.
  softmax  Sk = 4 ... 4096 (every template width and the tails just past them), 6 and 30
           rows, scale * s spanning +-30, a graded mask per batch row, one batch fully
           masked, no mask; backward from the kernel's own P.
  reducers colsum_bf16 (both first stages, a 4-byte-aligned view) and slab_sum (the
           vector and the scalar form), exact.
  wrap     one case per grid cap, inputs made on the device, a fixed row subset.
  8-byte   bdrln_fwd under DTF_LN16=0 in one fresh child process.
  refusals shapes and sizes the host refuses, outputs untouched.
  wrappers ops.transformer's autograd functions (_ln_part, the slices formula,
           rows_per_batch) against the same models.

Every case prints one JSON line (pytest -s) with the worst error / bound per output;
test_zz_worst_ratios prints the worst of the whole file.

Figures on an MI355X when this file was written (worst error / bound over the
cases; the 233 tests take 8 s): y 0.995, s 0.996, ds / dxb 0.996, GELU y 0.996 / dx 0.995,
P / Pd 0.993, dS 0.996 -- all limited by the bf16 store, as they should be, and equal
to the CPU emulation's to two digits; mean 0.11, rstd 0.081, dgamma 0.61, dbeta 0.10,
dbias 0.20 (LN) / 0.67 (GELU, N = 1) of their fp32 bounds; the 8-byte bdrln_fwd y 0.993,
s 0.995, mean 0.007, rstd 0.045.  Every exact comparison and every keep bit equal.

`python tests/test_transformer_edges_gpu.py child OUT` is the body of
test_eight_byte_bdrln_in_a_fresh_process.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import transformer_reference as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
SENTINEL = -1024.0
NAN = float("nan")
WORST = {}


class Guarded:
    """n elements between two guards of GUARD sentinels; .t is the middle (a view)."""

    def __init__(self, shape, dtype, fill=NAN):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill.reshape(-1))
        else:
            self.t.fill_(fill)
        self.t = self.t.view(shape)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        s = torch.full((), SENTINEL, dtype=self.buf.dtype, device="cuda")
        return bool((self.buf[:GUARD] == s).all()) and bool((self.buf[-GUARD:] == s).all())

    def cpu(self):
        return self.t.cpu()


class Report:
    """Figures and failures of one case."""

    def __init__(self, name, group):
        self.name, self.group, self.fig, self.fail = name, group, {}, []

    def bound(self, what, got, ref, tol):
        got = got.detach().cpu().double().reshape(ref.shape)
        err = (got - ref).abs()
        bad = ~(err <= tol)                      # a NaN is beyond every bound
        worst = R.elem_ratio(got, ref, tol)
        key = what.split("@")[0]
        self.fig[what] = float("%.3g" % worst)
        WORST["%s.%s" % (self.group, key)] = max(WORST.get("%s.%s" % (self.group, key), 0.0), worst)
        if bool(bad.any()):
            i = int(bad.reshape(-1).nonzero()[0])
            idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape))) if ref.dim() else ()
            self.fail.append("%s: %d of %d beyond the bound, worst error / bound %.3g, first at %r "
                             "(got %r, reference %r, bound %r)" % (what, int(bad.sum()), bad.numel(), worst, idx,
                                                                   float(got.reshape(-1)[i]),
                                                                   float(ref.reshape(-1)[i]),
                                                                   float(tol.reshape(-1)[i])))

    def true(self, what, cond):
        if not bool(cond):
            self.fail.append(what)

    def written(self, **bufs):
        for k, b in bufs.items():
            self.true("guard of %s overwritten" % k, b.intact())
            self.true("%s not fully written / not finite" % k, torch.isfinite(b.t.float()).all())

    def done(self):
        print(json.dumps({"case": self.name, **self.fig}))
        assert not self.fail, "%s:\n  %s" % (self.name, "\n  ".join(self.fail))


def dev(t):
    return None if t is None else t.cuda()


def bf(shape):
    return Guarded(shape, torch.bfloat16)


def fl(shape, fill=NAN):
    return Guarded(shape, torch.float32, fill)


# ---- the LayerNorm family ----------------------------------------------------------------------

def ln_rows(c):
    return c.B * c.S if c.kind == "emb" else c.N


def run_ln_fwd(C, c):
    """The forward kernel of a case into guarded NaN-filled buffers."""
    inp = R.inputs(c)
    N, H = ln_rows(c), c.H
    o = dict(y=bf((N, H)), s=bf((N, H)), mean=fl(N), rstd=fl(N))
    g, b = dev(inp["gamma"]), dev(inp["beta"])
    if c.kind == "bdrln":
        C.bdrln_fwd(dev(inp["x"]), dev(inp["bias"]), dev(inp["res"]), g, b, o["y"].t, o["s"].t, o["mean"].t,
                    o["rstd"].t, R.EPS, c.p, c.seed)
    elif c.kind == "f32in":
        C.ln_fwd_f32in(dev(inp["x"]), g, b, o["y"].t, o["s"].t, o["mean"].t, o["rstd"].t, R.EPS, c.p, c.seed)
    else:
        C.emb_ln_fwd(dev(inp["word"]), dev(inp["ids"].reshape(-1)), dev(inp["typ"]), dev(inp["tt"].reshape(-1)),
                     dev(inp["pos"]), c.S, g, b, o["y"].t, o["s"].t, o["mean"].t, o["rstd"].t, R.EPS, c.p, c.seed)
    torch.cuda.synchronize()
    return o


def check_ln_fwd(rep, c, got):
    """got: CPU tensors y, s, mean, rstd.  The bounds, then the dropped set bit for bit."""
    r = R.reference(c)
    for n in ("y", "s", "mean", "rstd"):
        rep.bound(n, got[n], r["ref"][n], r["tol"][n])
    if c.p > 0:
        dropped = r["keep"] == 0
        rep.true("no dropped element in the case", dropped.any())
        inp = R.inputs(c)
        if c.kind == "bdrln":
            want = inp["res"].float() if inp["res"] is not None else torch.zeros(dropped.shape)
            rep.true("s differs from the residual (or 0) on the dropped set",
                     torch.equal(got["s"].float()[dropped], want[dropped]))
            rep.true("s equals the residual (or 0) on most of the kept set: the bits are not hash32's",
                     float((got["s"].float()[~dropped] == want[~dropped]).double().mean()) < 0.01)
        else:
            rep.true("y is not exactly 0 on the dropped set", bool((got["y"].float()[dropped] == 0).all()))
            rep.true("y is 0 on the kept set", float((got["y"].float()[~dropped] == 0).double().mean()) < 0.01)


def run_ln_bwd(C, c, fwd, grid, dxb=True, outs=("dgamma", "dbeta", "dbias"), prior=None):
    """ln_bwd on the forward's own s / mean / rstd; part sized for `grid` blocks."""
    inp = R.inputs(c)
    N, H = ln_rows(c), c.H
    p, seed = (c.p, c.seed) if c.kind == "bdrln" else (0.0, 0)      # the embedding forms drop dy, not dxb
    o = dict(ds=bf((N, H)), part=fl(3 * grid * H))
    if dxb:
        o["dxb"] = bf((N, H))
    for n in outs:
        o[n] = fl(H, NAN if prior is None else prior)
    C.ln_bwd(dev(inp["dy"]), fwd["s"].t, fwd["mean"].t, fwd["rstd"].t, dev(inp["gamma"]), o["ds"].t,
             o["dxb"].t if dxb else None, o["part"].t, *[o[n].t if n in outs else None for n in
                                                          ("dgamma", "dbeta", "dbias")], p, seed, prior is not None)
    torch.cuda.synchronize()
    return o


def check_ln_bwd(rep, c, fwd, o, tag, prior=None):
    inp = R.inputs(c)
    r = R.reference(c)
    keep = r["keep"] if c.kind == "bdrln" else torch.ones_like(r["keep"])
    ref, tol = R.ln_bwd_model(inp["dy"], fwd["s"].cpu(), fwd["mean"].cpu(), fwd["rstd"].cpu(), inp["gamma"], keep)
    rep.written(**{k: v for k, v in o.items() if k != "part"})
    rep.true("guard of part overwritten", o["part"].intact())
    for n in R.LN_BWD_OUTPUTS:
        if n not in o:
            continue
        if prior is not None and n in ("dgamma", "dbeta", "dbias"):
            pr = prior.double()
            rep.bound(n + "+prior@" + tag, o[n].t, pr + ref[n], tol[n] + R.W * (pr.abs() + ref[n].abs() + tol[n]))
        else:
            rep.bound(n + "@" + tag, o[n].t, ref[n], tol[n])
    if c.kind == "bdrln" and c.p > 0 and "dxb" in o:
        dropped = keep == 0
        rep.true("dxb is not exactly 0 on the dropped set", bool((o["dxb"].cpu().float()[dropped] == 0).all()))
        rep.true("dxb is 0 on the kept set", float((o["dxb"].cpu().float()[~dropped] == 0).double().mean()) < 0.01)


LN_CASES = R.cases_of(*R.LN_KINDS)


@pytest.mark.parametrize("case", LN_CASES, ids=[c.name for c in LN_CASES])
def test_layernorm_forward_and_backward(native, case):
    c = case
    N, H = ln_rows(c), c.H
    fwd = run_ln_fwd(native, c)
    rep = Report(c.name, c.kind)
    rep.written(**fwd)
    check_ln_fwd(rep, c, {k: v.cpu() for k, v in fwd.items()})
    rows = (N + 3) // 4
    # grid = 1: one block strides over every row group; ceil(N / 4): one group each; + 2: two blocks
    # without rows, whose partial rows must be exact zeros
    o = run_ln_bwd(native, c, fwd, 1)
    check_ln_bwd(rep, c, fwd, o, "g1")
    o = run_ln_bwd(native, c, fwd, rows, dxb=False, outs=("dgamma", "dbeta"))
    check_ln_bwd(rep, c, fwd, o, "gN")
    prior = torch.randn(H, generator=torch.Generator().manual_seed(H + N))
    o = run_ln_bwd(native, c, fwd, rows + 2, outs=("dbias",), prior=prior)
    check_ln_bwd(rep, c, fwd, o, "gN+2", prior=prior)
    part = o["part"].cpu().view(3, rows + 2, H)
    rep.true("partial rows of blocks without rows are not exact zeros", bool((part[2, rows:] == 0).all()))
    rep.true("unrequested partials were written", torch.isnan(part[:2]).all())
    rep.done()


def integer_bf16(N, H, seed):
    """Integer-valued bf16 in [-8, 8]: the fp32 sums of far fewer than 2^20 of them are exact."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (N, H), generator=g).float().bfloat16()


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("N,H,extra", [(1, 256, 0), (9, 768, 2), (37, 512, 0), (37, 4096, 3)])
def test_ln_bwd_dbeta_exact_on_integer_dy(native, N, H, extra, accumulate):
    dy = integer_bf16(N, H, N + H)
    g = torch.Generator().manual_seed(1)
    s = torch.randn(N, H, generator=g).bfloat16()
    mean, rstd = s.float().mean(-1), 1.0 / s.float().std(-1)
    prior = torch.randint(-100, 100, (H,), generator=g).float()
    grid = (N + 3) // 4 + extra
    ds, part, dbeta = bf((N, H)), fl(3 * grid * H), fl(H, prior if accumulate else NAN)
    native.ln_bwd(dev(dy), dev(s), dev(mean), dev(rstd), torch.ones(H, device="cuda"), ds.t, None, part.t, None,
                  dbeta.t, None, 0.0, 0, accumulate)
    torch.cuda.synchronize()
    want = dy.double().sum(0) + (prior.double() if accumulate else 0)
    assert ds.intact() and part.intact() and dbeta.intact()
    assert torch.equal(dbeta.cpu().double(), want)


# ---- the embedding backward, exact -------------------------------------------------------------

EMB_AUX = [c for c in R.cases_of("emb") if c.H <= 1024 and c.p == 0]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", EMB_AUX, ids=[c.name for c in EMB_AUX])
def test_emb_bwd_aux_exact_on_integer_ds(native, case, accumulate):
    c = case
    inp = R.inputs(c)
    ds = integer_bf16(c.B * c.S, c.H, c.B * 100 + c.S)
    g = torch.Generator().manual_seed(2)
    ppos = torch.randint(-50, 50, (c.pos_rows, c.H), generator=g).float()
    ptyp = torch.randint(-50, 50, (2, c.H), generator=g).float()
    pos, typ, part = fl((c.pos_rows, c.H), ppos), fl((2, c.H), ptyp if accumulate else NAN), fl(2 * c.S * c.H)
    native.emb_bwd_aux(dev(ds), dev(inp["tt"].reshape(-1)), c.S, pos.t, typ.t, part.t, accumulate)
    torch.cuda.synchronize()
    wpos, wtyp = R.emb_bwd_aux_model(ds, inp["tt"], c.S)
    assert pos.intact() and typ.intact() and part.intact()
    want = ppos.double().clone()
    want[:c.S] = wpos + (ppos[:c.S].double() if accumulate else 0)          # rows from S on are never touched
    assert torch.equal(pos.cpu().double(), want)
    assert torch.equal(typ.cpu().double(), wtyp + (ptyp.double() if accumulate else 0))


# ---- bias + GELU -------------------------------------------------------------------------------

GELU_CASES = R.cases_of("gelu")


@pytest.mark.parametrize("case", GELU_CASES, ids=[c.name for c in GELU_CASES])
def test_bias_gelu_forward_and_backward(native, case):
    c = case
    inp, r = R.inputs(c), R.reference(c)
    x, bias, dy = dev(inp["x"]), dev(inp["bias"]), dev(inp["dy"])
    rep = Report(c.name, "gelu")
    y = bf((c.N, c.H))
    native.bias_gelu_fwd(x, bias, y.t)
    torch.cuda.synchronize()
    rep.written(y=y)
    rep.bound("y", y.t, r["ref"]["y"], r["tol"]["y"])
    for slices in (1, 3, c.N, c.N + 2):       # every rows_per % 4, and slices without rows
        dx, part, dbias = bf((c.N, c.H)), fl(slices * c.H), fl(c.H)
        native.bias_gelu_bwd(dy, x, bias, dx.t, part.t, dbias.t, False)
        torch.cuda.synchronize()
        rep.written(dx=dx, part=part, dbias=dbias)
        rep.bound("dx@%d" % slices, dx.t, r["ref"]["dx"], r["tol"]["dx"])
        rep.bound("dbias@%d" % slices, dbias.t, r["ref"]["dbias"], r["tol"]["dbias"])
    rep.done()


# ---- softmax -----------------------------------------------------------------------------------

SOFTMAX_CASES = R.cases_of("softmax")


@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=[c.name for c in SOFTMAX_CASES])
def test_softmax_forward_and_backward(native, case):
    c = case
    inp, r = R.inputs(c), R.reference(c)
    rows = inp["S"].shape[0]
    rep = Report(c.name, "softmax")
    P, Pd, dS = bf((rows, c.Sk)), bf((rows, c.Sk)), bf((rows, c.Sk))
    native.softmax_fwd(dev(inp["S"]), dev(inp["mask"]), P.t, Pd.t, inp["rows_per_batch"], inp["scale"], c.p, c.seed)
    torch.cuda.synchronize()
    rep.written(P=P, Pd=Pd)
    rep.bound("P", P.t, r["ref"]["P"], r["tol"]["P"])
    rep.bound("Pd", Pd.t, r["ref"]["Pd"], r["tol"]["Pd"])
    if c.p > 0:
        dropped = r["keep"] == 0
        rep.true("Pd is not exactly 0 on the dropped set", bool((Pd.cpu().float()[dropped] == 0).all()))
        open_kept = (~dropped) & (r["ref"]["P"] > 1e-30)
        rep.true("Pd is 0 on kept, open elements", bool((Pd.cpu().float()[open_kept] > 0).all()))
    # the backward from the P the forward stored
    native.softmax_bwd(dev(inp["dPd"]), P.t, dS.t, inp["scale"], c.p, c.seed)
    torch.cuda.synchronize()
    rep.written(dS=dS)
    bref, btol = R.softmax_bwd_model(inp["dPd"], P.cpu(), inp["scale"], r["keep"])
    rep.bound("dS", dS.t, bref["dS"], btol["dS"])
    rep.done()


# ---- dropout_bf16 ------------------------------------------------------------------------------

DROPOUT_CASES = R.cases_of("dropout")


@pytest.mark.parametrize("case", DROPOUT_CASES, ids=[c.name for c in DROPOUT_CASES])
def test_dropout_bits_and_values(native, case):
    c = case
    inp, r = R.inputs(c), R.reference(c)
    y = bf((c.N, c.H))
    native.dropout_bf16(dev(inp["x"]), y.t, c.p, c.seed)
    torch.cuda.synchronize()
    rep = Report(c.name, "dropout")
    rep.written(y=y)
    rep.bound("y", y.t, r["ref"]["y"], r["tol"]["y"])
    dropped = r["keep"] == 0
    rep.true("y is not exactly 0 on the dropped set", bool((y.cpu().float()[dropped] == 0).all()))
    rep.true("y is 0 on the kept set", float((y.cpu().float()[~dropped] == 0).double().mean()) < 0.01)
    rep.done()


# ---- the reducers, exact -----------------------------------------------------------------------

def _colsum_exact(C, x, P, accumulate, seed):
    N, H = x.shape
    prior = torch.randint(-100, 100, (H,), generator=torch.Generator().manual_seed(seed)).float()
    part, out = fl(P * H), fl(H, prior if accumulate else NAN)
    C.colsum_bf16(x, part.t, out.t, accumulate)
    torch.cuda.synchronize()
    want = x.cpu().double().sum(0) + (prior.double() if accumulate else 0)
    assert part.intact() and out.intact(), (N, H, P)
    assert torch.equal(out.cpu().double(), want), (N, H, P, accumulate)
    assert torch.equal(part.cpu().double().view(P, H).sum(0), x.cpu().double().sum(0)), (N, H, P)


@pytest.mark.parametrize("H", R.COLSUM_H)
def test_colsum_bf16_exact(native, H):
    """H % 8 == 0 and 16-byte aligned: colsum_bf16_partials; every other even H: the x2 form."""
    for N in R.COLSUM_N:
        x = integer_bf16(N, H, N + H).cuda()
        for i, P in enumerate(R.COLSUM_P):      # N < P: slices without rows
            _colsum_exact(native, x, P, bool((i + N) % 2), P)
    _colsum_exact(native, x, 3, True, 0)
    _colsum_exact(native, x, 3, False, 0)


@pytest.mark.parametrize("H", [8, 512, 520])
def test_colsum_bf16_exact_on_a_four_byte_aligned_view(native, H):
    for N in (3, 37):
        flat = torch.zeros(N * H + 8, dtype=torch.bfloat16, device="cuda")
        x = flat[2:2 + N * H].view(N, H)
        x.copy_(integer_bf16(N, H, N))
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
        for P in (1, 3, 65):
            _colsum_exact(native, x, P, False, P)
            _colsum_exact(native, x, P, True, P)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("S", R.SLAB_S)
def test_slab_sum_exact(native, S, offset):
    """offset 1: an out view one float past a 16-byte boundary takes the scalar form, as n % 4 != 0 does."""
    for n in R.SLAB_N:
        g = torch.Generator().manual_seed(S * 10000 + n)
        slabs = torch.randint(-1000, 1000, (S, n), generator=g).float()
        prior = torch.randint(-1000, 1000, (n,), generator=g).float()
        for accumulate in (False, True):
            buf = fl(n + 4, NAN)
            out = buf.t[offset:offset + n]
            if accumulate:
                out.copy_(prior)
            assert out.data_ptr() % 16 == 4 * offset
            native.slab_sum(dev(slabs), out, accumulate)
            torch.cuda.synchronize()
            assert buf.intact()
            assert torch.equal(out.cpu().double(), slabs.double().sum(0) + (prior.double() if accumulate else 0))
            rest = torch.cat([buf.t[:offset], buf.t[offset + n:]])
            assert bool(torch.isnan(rest).all())


# ---- the grid caps -----------------------------------------------------------------------------

def wrap_rows(N, wrap):
    """The first rows, the eight rows either side of each wrap point, the last rows."""
    rows = set(range(8)) | set(range(N - 8, N))
    for w in range(wrap, N, wrap):
        rows |= set(range(w - 8, min(N, w + 8)))
    return torch.tensor(sorted(rows))


def _dropout_keep(seed, p, rows, width):
    return R.keep_scale(R.keep_bits_rows(seed, p, rows.numpy(), width), p)


def _no_nan(rep, **outs):
    for k, b in outs.items():
        rep.true("guard of %s overwritten" % k, b.intact())
        rep.true("NaN left in %s" % k, not bool(torch.isnan(b.t).any()))


def test_grid_wrap_bdrln_fwd16(native):
    N, H = R.WRAP["bdrln"]
    p, seed = 0.1, R.SEEDS["h32"]
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(N, H, device="cuda", generator=g).bfloat16()
    res = torch.randn(N, H, device="cuda", generator=g).bfloat16()
    bias, gam, bet = (torch.randn(H, device="cuda", generator=g) * 0.1 + k for k in (0, 1, 0))
    o = dict(y=bf((N, H)), s=bf((N, H)), mean=fl(N), rstd=fl(N))
    native.bdrln_fwd(x, bias, res, gam, bet, o["y"].t, o["s"].t, o["mean"].t, o["rstd"].t, R.EPS, p, seed)
    torch.cuda.synchronize()
    rep = Report("wrap-bdrln_fwd16-N%d" % N, "wrap")
    _no_nan(rep, **o)
    rows = wrap_rows(N, 8192 * 8)
    inp = dict(x=x[rows.cuda()].cpu(), res=res[rows.cuda()].cpu(), bias=bias.cpu(), gamma=gam.cpu(), beta=bet.cpu())
    ref, tol = R.ln_fwd_model("bdrln", inp, _dropout_keep(seed, p, rows, H))
    for n in ("y", "s", "mean", "rstd"):
        rep.bound(n, o[n].t[rows.cuda()], ref[n], tol[n])
    rep.done()


@pytest.mark.parametrize("kind", ["f32in", "emb"])
def test_grid_wrap_ln_fwd_f32in_and_emb_ln_fwd(native, kind):
    N, H = R.WRAP[kind]
    p, seed = 0.1, R.SEEDS["h64"]
    g = torch.Generator(device="cuda").manual_seed(2)
    gam, bet = (torch.randn(H, device="cuda", generator=g) * 0.1 + k for k in (1, 0))
    o = dict(y=bf((N, H)), s=bf((N, H)), mean=fl(N), rstd=fl(N))
    rows = wrap_rows(N, 8192 * 4)
    rc = rows.cuda()
    if kind == "f32in":
        x = torch.randn(N, H, device="cuda", generator=g)
        native.ln_fwd_f32in(x, gam, bet, o["y"].t, o["s"].t, o["mean"].t, o["rstd"].t, R.EPS, p, seed)
        inp = dict(x=x[rc].cpu())
    else:       # B = 1, S = N: the position row is the row itself
        V = 64
        word, typ = torch.randn(V, H, device="cuda", generator=g), torch.randn(2, H, device="cuda", generator=g)
        pos = torch.randn(N, H, device="cuda", generator=g)
        ids = torch.randint(0, V, (N,), device="cuda", generator=g)
        tt = torch.randint(0, 2, (N,), device="cuda", generator=g)
        native.emb_ln_fwd(word, ids, typ, tt, pos, N, gam, bet, o["y"].t, o["s"].t, o["mean"].t, o["rstd"].t, R.EPS,
                          p, seed)
        inp = dict(word=word.cpu(), typ=typ.cpu(), pos=pos.cpu(), ids=ids[rc].cpu(), tt=tt[rc].cpu(), S=N, rows=rows)
    torch.cuda.synchronize()
    rep = Report("wrap-%s-N%d" % (kind, N), "wrap")
    _no_nan(rep, **o)
    inp.update(gamma=gam.cpu(), beta=bet.cpu())
    ref, tol = R.ln_fwd_model(kind, inp, _dropout_keep(seed, p, rows, H))
    for n in ("y", "s", "mean", "rstd"):
        rep.bound(n, o[n].t[rc], ref[n], tol[n])
    rep.done()


def test_grid_wrap_softmax(native):
    rows_n, Sk = R.WRAP["softmax"]
    rpb, p, seed, scale = 5, 0.1, R.SEEDS["h32"], 0.125
    B = (rows_n + rpb - 1) // rpb
    g = torch.Generator(device="cuda").manual_seed(3)
    S = (torch.randn(rows_n, Sk, device="cuda", generator=g) * 16).bfloat16()
    mask = -torch.randint(0, 3, (B, Sk), device="cuda", generator=g).float()
    dPd = torch.randn(rows_n, Sk, device="cuda", generator=g).bfloat16()
    P, Pd, dS = bf((rows_n, Sk)), bf((rows_n, Sk)), bf((rows_n, Sk))
    native.softmax_fwd(S, mask, P.t, Pd.t, rpb, scale, p, seed)
    native.softmax_bwd(dPd, P.t, dS.t, scale, p, seed)
    torch.cuda.synchronize()
    rep = Report("wrap-softmax-rows%d" % rows_n, "wrap")
    _no_nan(rep, P=P, Pd=Pd, dS=dS)
    rows = wrap_rows(rows_n, 8192 * 4)
    rc = rows.cuda()
    keep = _dropout_keep(seed, p, rows, Sk)
    mrows = mask.cpu()[rows // rpb]                         # one mask row per selected row
    ref, tol = R.softmax_fwd_model(S[rc].cpu(), mrows, 1, scale, keep)
    rep.bound("P", P.t[rc], ref["P"], tol["P"])
    rep.bound("Pd", Pd.t[rc], ref["Pd"], tol["Pd"])
    bref, btol = R.softmax_bwd_model(dPd[rc].cpu(), P.t[rc].cpu(), scale, keep)
    rep.bound("dS", dS.t[rc], bref["dS"], btol["dS"])
    rep.done()


def test_grid_wrap_bias_gelu_fwd8(native):
    N, H = R.WRAP["gelu8"]
    g = torch.Generator(device="cuda").manual_seed(4)
    x = (torch.randn(N, H, device="cuda", generator=g) * 3).bfloat16()
    bias = torch.randn(H, device="cuda", generator=g) * 0.02
    y = bf((N, H))
    native.bias_gelu_fwd(x, bias, y.t)
    torch.cuda.synchronize()
    rep = Report("wrap-bias_gelu_fwd8-N%d" % N, "wrap")
    _no_nan(rep, y=y)
    rows = wrap_rows(N, 32768 * 256 * 8 // H)
    rc = rows.cuda()
    ref, tol = R.gelu_model(x[rc].cpu(), bias.cpu(), torch.zeros(len(rows), H))
    rep.bound("gelu_y", y.t[rc], ref["y"], tol["y"])
    rep.done()


def test_grid_wrap_dropout_bf16(native):
    N, H = R.WRAP["dropout"]
    p, seed = 0.1, R.SEEDS["h32"]
    x = torch.randn(N, H, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).bfloat16()
    y = bf((N, H))
    native.dropout_bf16(x, y.t, p, seed)
    torch.cuda.synchronize()
    rep = Report("wrap-dropout_bf16-N%d" % N, "wrap")
    _no_nan(rep, y=y)
    rows = wrap_rows(N, 65536 * 256 * 4 // H)
    rc = rows.cuda()
    keep = _dropout_keep(seed, p, rows, H)
    ref, tol = R.dropout_model(x[rc].cpu(), keep)
    rep.bound("dropout_y", y.t[rc], ref["y"], tol["y"])
    rep.true("y is not exactly 0 on the dropped set", bool((y.t[rc].cpu().float()[keep == 0] == 0).all()))
    rep.done()


# ---- the 8-byte bdrln_fwd ----------------------------------------------------------------------

EIGHT_BYTE = [c for c in R.cases_of("bdrln") if c.H == 768 and not c.tags]


def _child(out_path):
    """bdrln_fwd<NC> (one row per wave, 8-byte accesses) on the N sweep at H = 768."""
    assert os.environ.get("DTF_LN16") == "0"
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    from distributed_tensorflow_example_amd import _native
    C = _native.load()
    outs, intact = {}, True
    for c in EIGHT_BYTE:
        o = run_ln_fwd(C, c)
        intact = intact and all(b.intact() for b in o.values())
        outs[c.name] = {k: v.cpu() for k, v in o.items()}
    torch.save(outs, out_path)
    print(json.dumps({"ok": intact, "cases": len(outs)}))
    return 0 if intact else 1


def test_eight_byte_bdrln_in_a_fresh_process(native):
    """DTF_LN16 is latched in a static on first use: one fresh child (never an exec) runs the
    8-byte form and writes its outputs to a temporary file; the bounds are the same."""
    assert os.environ.get("DTF_LN16", "1") != "0", "run this file without DTF_LN16=0; the child covers that path"
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ln8.pt")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", path],
                           env=dict(os.environ, DTF_LN16="0"), cwd=REPO, timeout=180, capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        outs = torch.load(path)
    assert sorted(outs) == sorted(c.name for c in EIGHT_BYTE) and len(outs) >= 2 * len(R.LN_N)
    fails = []
    for c in EIGHT_BYTE:
        rep = Report("ln8 " + c.name, "bdrln8")
        for n in ("y", "s", "mean", "rstd"):
            rep.true("%s not finite" % n, torch.isfinite(outs[c.name][n].float()).all())
        check_ln_fwd(rep, c, outs[c.name])
        print(json.dumps({"case": rep.name, **rep.fig}))
        fails += rep.fail
    assert not fails, fails


# ---- refusals ----------------------------------------------------------------------------------

def _refused(call, *outs):
    """call() raises RuntimeError and leaves every output as it was (all sentinel)."""
    with pytest.raises(RuntimeError):
        call()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.float() == 7.0).all())


def _sent(shape, dtype):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), 7.0, dtype=dtype, device="cuda")


def _ln_args(N, H, nb=None, ng=None, nm=None, res_n=None, s_n=None):
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")      # noqa: E731
    return dict(x=z((N, H), torch.bfloat16), bias=z(H if nb is None else nb), gamma=z(H if ng is None else ng),
                beta=z(H), res=None if res_n is None else z(res_n, torch.bfloat16), y=_sent((N, H), torch.bfloat16),
                s=_sent((N, H) if s_n is None else (s_n,), torch.bfloat16), mean=_sent(N if nm is None else nm,
                                                                                       torch.float32),
                rstd=_sent(N, torch.float32))


def _bdrln(C, a, p=0.0):
    return lambda: C.bdrln_fwd(a["x"], a["bias"], a["res"], a["gamma"], a["beta"], a["y"], a["s"], a["mean"],
                               a["rstd"], R.EPS, p, 0)


@pytest.mark.parametrize("H", R.REFUSED_LN_H)
def test_layernorm_family_refuses_unsupported_widths(native, H):
    N = 4
    a = _ln_args(N, H)
    outs = (a["y"], a["s"], a["mean"], a["rstd"])
    _refused(_bdrln(native, a), *outs)
    xf = torch.zeros(N, H, device="cuda")
    _refused(lambda: native.ln_fwd_f32in(xf, a["gamma"], a["beta"], a["y"], a["s"], a["mean"], a["rstd"], R.EPS, 0.0,
                                         0), *outs)
    ids = torch.zeros(N, dtype=torch.int64, device="cuda")
    _refused(lambda: native.emb_ln_fwd(xf, ids, xf[:2], ids, xf, 2, a["gamma"], a["beta"], a["y"], a["s"],
                                       a["mean"], a["rstd"], R.EPS, 0.0, 0), *outs)
    ds, part, dg = _sent((N, H), torch.bfloat16), _sent(3 * H, torch.float32), _sent(H, torch.float32)
    zm = torch.zeros(N, device="cuda")
    _refused(lambda: native.ln_bwd(a["x"], a["x"], zm, zm, a["gamma"], ds, None, part, dg, None, None, 0.0, 0,
                                   False), ds, part, dg)


def test_layernorm_family_refuses_short_buffers_and_bad_p(native):
    N, H = 4, 256
    for kw in (dict(nb=H - 1), dict(ng=H - 4), dict(nm=N - 1), dict(res_n=N * H - 8), dict(s_n=N * H - 8)):
        a = _ln_args(N, H, **kw)
        _refused(_bdrln(native, a), a["y"], a["s"], a["mean"], a["rstd"])
    for p in (1.0, -0.1, 1.5, float("nan")):
        a = _ln_args(N, H)
        _refused(_bdrln(native, a, p), a["y"], a["s"], a["mean"], a["rstd"])
    a = _ln_args(N, H)
    outs = (a["y"], a["s"], a["mean"], a["rstd"])
    xf = torch.zeros(N, H, device="cuda")
    f32in = lambda **k: (lambda: native.ln_fwd_f32in(      # noqa: E731
        xf, k.get("gamma", a["gamma"]), a["beta"], a["y"], k.get("s", a["s"]), k.get("mean", a["mean"]), a["rstd"],
        R.EPS, k.get("p", 0.0), 0))
    _refused(f32in(gamma=a["gamma"][:H - 1]), *outs)
    _refused(f32in(gamma=a["gamma"].double()), *outs)
    _refused(f32in(mean=_sent(N - 1, torch.float32)), *outs)
    _refused(f32in(s=_sent(N * H - 8, torch.bfloat16)), *outs)
    _refused(f32in(p=1.0), *outs)
    # ln_bwd
    zb = torch.zeros(N, H, dtype=torch.bfloat16, device="cuda")
    zm = torch.zeros(N, device="cuda")
    ds, dxb, part, dg = (_sent((N, H), torch.bfloat16), _sent((N, H), torch.bfloat16), _sent(3 * 2 * H, torch.float32),
                         _sent(H, torch.float32))
    bwd = lambda **k: (lambda: native.ln_bwd(      # noqa: E731
        zb, k.get("s", zb), k.get("mean", zm), zm, k.get("gamma", a["gamma"]), k.get("ds", ds), k.get("dxb", dxb),
        k.get("part", part), k.get("dg", dg), None, None, k.get("p", 0.0), 0, False))
    _refused(bwd(s=zb[:N - 1]), ds, dxb, part, dg)
    _refused(bwd(mean=zm[:N - 1]), ds, dxb, part, dg)
    _refused(bwd(gamma=a["gamma"][:H - 1]), ds, dxb, part, dg)
    _refused(bwd(ds=_sent((N - 1, H), torch.bfloat16)), dxb, part, dg)
    _refused(bwd(dxb=_sent((N - 1, H), torch.bfloat16)), ds, part, dg)
    _refused(bwd(part=_sent(3 * H - 1, torch.float32)), ds, dxb, dg)
    _refused(bwd(dg=_sent(H - 1, torch.float32)), ds, dxb, part)
    _refused(bwd(p=1.0), ds, dxb, part, dg)


def test_softmax_refusals(native):
    rows, rpb = 6, 3
    for Sk in R.REFUSED_SK:
        S = torch.zeros(rows, Sk, dtype=torch.bfloat16, device="cuda")
        P, dS = _sent((rows, Sk), torch.bfloat16), _sent((rows, Sk), torch.bfloat16)
        _refused(lambda: native.softmax_fwd(S, None, P, None, rpb, 1.0, 0.0, 0), P)
        _refused(lambda: native.softmax_bwd(S, S, dS, 1.0, 0.0, 0), dS)
    Sk = 64
    S = torch.zeros(rows, Sk, dtype=torch.bfloat16, device="cuda")
    P, Pd, dS = (_sent((rows, Sk), torch.bfloat16) for _ in range(3))
    mask = torch.zeros(2, Sk, device="cuda")
    fwd = lambda **k: (lambda: native.softmax_fwd(      # noqa: E731
        S, k.get("mask", mask), k.get("P", P), k.get("Pd", Pd), k.get("rpb", rpb), 1.0, k.get("p", 0.0), 0))
    _refused(fwd(rpb=0), P, Pd)
    _refused(fwd(rpb=-1), P, Pd)
    _refused(fwd(mask=mask[:1]), P, Pd)                    # one batch row short
    _refused(fwd(mask=mask.reshape(-1)[:2 * Sk - 1]), P, Pd)
    _refused(fwd(rpb=2), P, Pd)                            # three batch rows of mask needed, two given
    _refused(fwd(P=_sent((rows - 1, Sk), torch.bfloat16)), Pd)
    _refused(fwd(Pd=_sent((rows - 1, Sk), torch.bfloat16)), P)
    _refused(fwd(p=1.0), P, Pd)
    _refused(lambda: native.softmax_bwd(S[:rows - 1], S, dS, 1.0, 0.0, 0), dS)
    _refused(lambda: native.softmax_bwd(S, S, _sent((rows - 1, Sk), torch.bfloat16), 1.0, 0.0, 0))
    _refused(lambda: native.softmax_bwd(S, S, dS, 1.0, 1.0, 0), dS)


def test_bias_gelu_and_dropout_refusals(native):
    N = 4
    for H in (6, 1022):                                    # H % 4 != 0
        x = torch.zeros(N, H, dtype=torch.bfloat16, device="cuda")
        y, part, db = _sent((N, H), torch.bfloat16), _sent(H, torch.float32), _sent(H, torch.float32)
        bias = torch.zeros(H, device="cuda")
        _refused(lambda: native.bias_gelu_fwd(x, bias, y), y)
        _refused(lambda: native.bias_gelu_bwd(x, x, bias, y, part, db, False), y, part, db)
    H = 12
    x = torch.zeros(N, H, dtype=torch.bfloat16, device="cuda")
    y, part, db = _sent((N, H), torch.bfloat16), _sent(H, torch.float32), _sent(H, torch.float32)
    bias = torch.zeros(H, device="cuda")
    _refused(lambda: native.bias_gelu_fwd(x, bias[:H - 1], y), y)
    _refused(lambda: native.bias_gelu_fwd(x, bias, _sent((N - 1, H), torch.bfloat16)))
    _refused(lambda: native.bias_gelu_bwd(x, x, bias[:H - 1], y, part, db, False), y, part, db)
    _refused(lambda: native.bias_gelu_bwd(x[:N - 1], x, bias, y, part, db, False), y, part, db)
    _refused(lambda: native.bias_gelu_bwd(x, x, bias, _sent((N - 1, H), torch.bfloat16), part, db, False), part, db)
    _refused(lambda: native.bias_gelu_bwd(x, x, bias, y, part, _sent(H - 1, torch.float32), False), y, part)
    _refused(lambda: native.bias_gelu_bwd(x, x, bias, y, _sent(H - 1, torch.float32), db, False), y, db)
    for p in (1.0, -0.5):
        _refused(lambda: native.dropout_bf16(x, y, p, 0), y)
    _refused(lambda: native.dropout_bf16(x, _sent((N - 1, H), torch.bfloat16), 0.1, 0))


def test_colsum_bf16_refusals(native):
    N = 5
    for H in (7, 129):                                     # odd H
        x = torch.ones(N, H, dtype=torch.bfloat16, device="cuda")
        part, out = _sent(2 * H, torch.float32), _sent(H, torch.float32)
        _refused(lambda: native.colsum_bf16(x, part, out, False), part, out)
    H = 8
    flat = torch.ones(N * H + 8, dtype=torch.bfloat16, device="cuda")
    x = flat[1:1 + N * H].view(N, H)                       # 2-byte-misaligned
    assert x.data_ptr() % 4 == 2
    part, out = _sent(2 * H, torch.float32), _sent(H, torch.float32)
    _refused(lambda: native.colsum_bf16(x, part, out, False), part, out)
    _refused(lambda: native.colsum_bf16(flat[:N * H].view(N, H), part, out[:H - 1], False), part, out)


# ---- the autograd wrappers ---------------------------------------------------------------------

def test_wrapper_bias_dropout_residual_layernorm(native):
    """_BDRLN with _ln_part's grid (N = 37: three blocks) against the models, p = 0."""
    from distributed_tensorflow_example_amd.ops import transformer as T
    c = R.case("bdrln-N37-H512-res")
    inp, r = R.inputs(c), R.reference(c)
    x, res = dev(inp["x"]).requires_grad_(), dev(inp["res"]).requires_grad_()
    ps = [dev(inp[k]).requires_grad_() for k in ("bias", "gamma", "beta")]
    y = T.bias_dropout_residual_layernorm(x, ps[0], res, ps[1], ps[2], 0.0, R.EPS)
    y.backward(dev(inp["dy"]))
    torch.cuda.synchronize()
    rep = Report("wrapper " + c.name, "wrapper")
    rep.bound("y", y, r["ref"]["y"], r["tol"]["y"])
    fwd = run_ln_fwd(native, c)             # the same kernel on the same inputs: the s the wrapper saved
    ref, tol = R.ln_bwd_model(inp["dy"], fwd["s"].cpu(), fwd["mean"].cpu(), fwd["rstd"].cpu(), inp["gamma"], r["keep"])
    rep.bound("dxb", x.grad, ref["dxb"], tol["dxb"])
    rep.bound("ds", res.grad, ref["ds"], tol["ds"])
    for t, n in zip(ps, ("dbias", "dgamma", "dbeta")):
        rep.bound(n, t.grad, ref[n], tol[n])
    rep.done()


def test_wrapper_bias_gelu_slices_formula(native):
    """_BiasGelu: slices = max(1, min(512, N // 32)) -- N = 67 gives two slices of 34 and 33 rows."""
    from distributed_tensorflow_example_amd.ops import transformer as T
    for name in ("gelu-N67-H1028", "gelu-N5-H1032"):
        c = R.case(name)
        inp, r = R.inputs(c), R.reference(c)
        x, b = dev(inp["x"]).requires_grad_(), dev(inp["bias"]).requires_grad_()
        y = T.bias_gelu(x, b)
        y.backward(dev(inp["dy"]))
        torch.cuda.synchronize()
        rep = Report("wrapper " + name, "wrapper")
        rep.bound("gelu_y", y, r["ref"]["y"], r["tol"]["y"])
        rep.bound("gelu_dx", x.grad, r["ref"]["dx"], r["tol"]["dx"])
        rep.bound("gelu_dbias", b.grad, r["ref"]["dbias"], r["tol"]["dbias"])
        rep.done()


def test_wrapper_attention_softmax_rows_per_batch(native):
    """_AttnSoftmax hands rows_per_batch = heads * Sq: a different mask per batch row must land."""
    from distributed_tensorflow_example_amd.ops import transformer as T
    c = R.case("softmax-Sk260-Sq5-graded")
    inp, r = R.inputs(c), R.reference(c)
    S4 = dev(inp["S"]).view(R.SOFTMAX_B, R.SOFTMAX_HEADS, c.Sq, c.Sk).requires_grad_()
    P = T.attention_softmax(S4, dev(inp["mask"]), inp["scale"], 0.0)
    P.backward(dev(inp["dPd"]).view_as(P))
    torch.cuda.synchronize()
    rep = Report("wrapper " + c.name, "wrapper")
    rep.bound("P", P, r["ref"]["P"], r["tol"]["P"])
    bref, btol = R.softmax_bwd_model(inp["dPd"], P.detach().cpu().reshape(-1, c.Sk), inp["scale"], r["keep"])
    rep.bound("dS", S4.grad, bref["dS"], btol["dS"])
    rep.done()


def test_zz_worst_ratios(native):
    """The worst error / bound per kernel family and output over this file's run."""
    print(json.dumps({"worst": {k: float("%.3g" % v) for k, v in sorted(WORST.items())}}))
    assert all(v <= 1.0 for v in WORST.values()), WORST


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "child":
        sys.exit("usage: %s child OUT" % sys.argv[0])
    sys.exit(_child(sys.argv[2]))
