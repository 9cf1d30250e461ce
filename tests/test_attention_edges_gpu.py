"""Fused attention kernels (csrc/kernels/attention.hip: attn_fwd, attn_bwd_dq,
attn_bwd_dkv, attn_bwd_fused) per element against the float64 model of
tests/attention_reference.py, with its derived bounds -- none is fitted to what
the kernels give -- and the dropout bits read off exactly.

attn_fwd / attn_bwd are called through the binding, so seeds and scratch buffers
are the test's.  Every output (ctx, lse, dqkv, Dbuf, bpart, dbias) is the middle
of a flat buffer with 4,096 sentinel elements on each side and is pre-filled with
NaN: after each call the guards must be intact and no NaN left.  Dbuf is written
by the two-kernel backward only; after the one-workgroup kernel (S <= 128) it
must still be all NaN, which also proves which path ran.

  A  p = 0: O, lse, dQ, dK, dV, dbias per element, every S, (B, NH) = (1, 1), (2, 3),
     (2, 12); graded mask (0 / -1 / -2.5 / -0.75 / -10000 per key, shifted per batch
     element, a padding tail from S - 5); scale 1/8 and 1/4; without bias / mask.
     dK / dV rows of masked keys are exactly 0.
  B  dropout p = 0.1 / 0.5 on both hash branches, S = 64 ... 256, same checks: the
     backward must regenerate the forward's bits or dQ / dK / dV leave their bounds.
  C  the keep bits, exact: q = k = 0, V one-hot on a 64-key block, so
     out[b, q, h * 64 + d] > 0 exactly where key 64 j + d of that row is kept.  Every
     block of every S, both hash branches.  Not covered: element indices >= 2^32,
     which feed the hash's high word, need a [B, NH, S, S] of more than 6 GB.
  D  per (b, h, row) 64-vector ||err|| / ||bound|| of O, dQ, dK, dV at most twice the
     worst row of the reference's fp32 / bf16 emulation of the same case.
  E  the two-kernel backward at S <= 128 (DTF_ATTN_BWD_FUSED=0) in one fresh child
     process, DTF_ATTN_BIAS_PARTIALS on and off through ops.transformer,
     accumulate=True, and two runs of every kernel bit for bit.

Every case prints one JSON line (pytest -s): per output the worst element error /
bound, and "rows": [worst row ratio, the emulation's] per output.

Figures on an MI355X when this file was written (worst error / bound over the
cases of a group; the 65 tests take 7 s):
  A (19 cases): O 0.68 ... 0.81, dV 0.61 ... 0.83 (both limited by the bf16 store, as
    they should be), dQ 0.16 ... 0.26, dK 0.17 ... 0.28, lse 0.011 ... 0.025,
    dbias 0.040 ... 0.14, bpart 0.16 ... 0.33; S >= 192: Dbuf 0.027 ... 0.044 of its fp32
    bound, D 0.14 ... 0.21.
  B (16 cases): O 0.81 ... 0.91, dV 0.75 ... 0.89, dQ 0.29 ... 0.75, dK 0.21 ... 0.39,
    lse 0.014 ... 0.029, dbias 0.039 ... 0.14, bpart 0.30 ... 0.45, Dbuf 0.031 ... 0.049,
    D 0.15 ... 0.28.
  D, worst row of the kernels [of the emulation]: O 0.35 ... 0.56 [the same],
    dV 0.32 ... 0.55 [the same], dQ 0.062 ... 0.26 [0.062 ... 0.26], dK 0.076 ... 0.22
    [the same]: kernel / emulation between 0.955 and 1.000 in every case, against
    the 2 allowed -- the bf16 roundings both share decide the rows, not the order
    of the fp32 sums or __expf.
  E child (19 cases, two-kernel backward at S <= 128): the figures of A and B to
    three digits, Dbuf 0.018 ... 0.045, D 0.061 ... 0.23.  Bit-equality HOLDS: all 36
    SHA-256 digests (dqkv of every S <= 128 case, dbias of the 17 with a bias) equal the one-workgroup
    kernel's, so test_two_kernel_backward_at_short_sequences asserts it.
  E bias gradient: partials 0.063 ... 0.081 of the bound, column sums of the stored
    dqkv 0.044 ... 0.10 of theirs (and 0.0009 ... 0.0036 of the fp32 bound against the
    stored values themselves); prior + sums 0.063 ... 0.081.
  C: every keep bit of every block equal, both hash branches, p = 0.1 and 0.5.

`python tests/test_attention_edges_gpu.py child` is the body of
test_two_kernel_backward_at_short_sequences.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

import attention_reference as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096          # multiple of 8 bf16 / 4 fp32: the middle stays 16-byte aligned
SENTINEL = -1024.0    # exact in bf16 and fp32
NAN = float("nan")
FUSED_ENV = os.environ.get("DTF_ATTN_BWD_FUSED", "1") != "0"


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

    def bits(self):
        """The middle as integers on the CPU: NaN patterns compare like any other."""
        it = torch.int16 if self.t.dtype == torch.bfloat16 else torch.int32
        return self.t.contiguous().view(it).cpu()

    def sha(self):
        return hashlib.sha256(self.bits().numpy().tobytes()).hexdigest()


class Report:
    """Figures and failures of one case."""

    def __init__(self, name):
        self.name, self.fig, self.fail = name, {}, []

    def bound(self, what, got, ref, tol):
        got = got.detach().cpu().double().reshape(ref.shape)
        err = (got - ref).abs()
        bad = ~(err <= tol)                      # a NaN is beyond every bound
        worst = R.elem_ratio(got, ref, tol)
        self.fig[what] = float("%.3g" % worst)
        if bool(bad.any()):
            i = int(bad.reshape(-1).nonzero()[0])
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
            self.fail.append("%s: %d of %d beyond the bound, worst error / bound %.3g, first at %r "
                             "(got %r, reference %r, bound %r)" % (what, int(bad.sum()), bad.numel(), worst, idx,
                                                                   float(got.reshape(-1)[i]),
                                                                   float(ref.reshape(-1)[i]),
                                                                   float(tol.reshape(-1)[i])))

    def rows(self, what, got, ref, tol, yardstick):
        r = R.row_ratio(got.detach().cpu(), ref, tol)
        self.fig.setdefault("rows", {})[what] = [float("%.3g" % r), float("%.3g" % yardstick)]
        if not r <= 2.0 * yardstick:
            self.fail.append("%s: worst row ||err|| / ||bound|| %.3g above twice the emulation's %.3g"
                             % (what, r, yardstick))

    def true(self, what, cond):
        if not bool(cond):
            self.fail.append(what)

    def done(self):
        print(json.dumps({"case": self.name, **self.fig}))
        assert not self.fail, "%s:\n  %s" % (self.name, "\n  ".join(self.fail))


def gpu_inputs(case):
    return tuple(None if t is None else t.cuda() for t in R.inputs(case))


def launch(C_, case, tensors=None, dbias_prior=None, backward=True):
    """attn_fwd, then attn_bwd on its ctx and lse, into guarded NaN-filled buffers.
    Without a bias no bpart / dbias is passed (as ops.transformer calls it)."""
    qkv, bias, mask, dO = tensors if tensors is not None else gpu_inputs(case)
    B, S, NH = case.B, case.S, case.NH
    H, H3 = NH * R.HD, 3 * NH * R.HD
    o = dict(ctx=Guarded(B * S * H, torch.bfloat16, (B, S, H)), lse=Guarded(B * NH * S, torch.float32, (B, NH, S)))
    C_.attn_fwd(qkv, bias, mask, o["ctx"].t, o["lse"].t, NH, case.scale, case.p, case.seed)
    if backward:
        o.update(dqkv=Guarded(B * S * H3, torch.bfloat16, (B, S, H3)),
                 Dbuf=Guarded(B * NH * S, torch.float32, (B, NH, S)))
        if bias is not None:
            o.update(bpart=Guarded(B * S // 16 * H3, torch.float32),
                     dbias=Guarded(H3, torch.float32, fill=NAN if dbias_prior is None else dbias_prior))
        C_.attn_bwd(qkv, bias, mask, o["ctx"].t, dO, o["lse"].t, o["Dbuf"].t, o["dqkv"].t, NH, case.scale, case.p,
                    case.seed, o["bpart"].t if bias is not None else None,
                    o["dbias"].t if bias is not None else None, dbias_prior is not None)
    torch.cuda.synchronize()
    return o


def check(rep, case, o, fused, dbias_prior=None):
    """Sections A, B and D on the buffers of one launch."""
    r = R.reference(case)
    ref, tol = r["ref"], r["tol"]
    qkv, bias, mask, dO = R.inputs(case)
    for k, b in o.items():
        rep.true("guard of %s overwritten" % k, b.intact())
        if k != "Dbuf":
            rep.true("%s not fully written / not finite" % k, torch.isfinite(b.t.float()).all())
    if fused:
        rep.true("Dbuf touched by the one-workgroup backward", torch.isnan(o["Dbuf"].t).all())
    else:
        rep.true("Dbuf not fully written", torch.isfinite(o["Dbuf"].t).all())
        dref, dtol = R.dbuf_reference(o["ctx"].t.cpu(), dO, case.NH)
        rep.bound("Dbuf", o["Dbuf"].t, dref, dtol)               # fp32-sized: from the ctx it was handed
        rep.bound("D", o["Dbuf"].t, ref["D"], tol["D"])          # and against the model's D
    got = dict(O=R.heads(o["ctx"].t.cpu(), case.NH, 1)[0], lse=o["lse"].t.cpu())
    got["dQ"], got["dK"], got["dV"] = R.split_dqkv(o["dqkv"].t.cpu(), case.NH)
    for n in ("O", "lse", "dQ", "dK", "dV"):
        rep.bound(n, got[n], ref[n], tol[n])
    if "dbias" in o:
        bref, btol = R.bpart_reference(ref, tol)
        rep.bound("bpart", o["bpart"].t, bref, btol)
        if dbias_prior is None:
            rep.bound("dbias", o["dbias"].t, ref["dbias"], tol["dbias"])
        else:       # prior + sums: one more fp32 addition
            pr = dbias_prior.cpu().double()
            rep.bound("dbias+prior", o["dbias"].t, pr + ref["dbias"],
                      tol["dbias"] + R.W * (pr.abs() + ref["dbias"].abs() + tol["dbias"]))
    if mask is not None:
        dead = (mask == -10000.0)[:, None, :, None].expand_as(ref["dK"])
        rep.true("no masked key in the case", bool(dead.any()))
        for n in ("dK", "dV"):
            rep.true("%s of a masked key is not exactly 0" % n, bool((got[n].float()[dead] == 0).all()))
    for n in R.ROW_OUTPUTS:
        rep.rows(n, got[n], ref[n], tol[n], r["emu_rows"][n])
    return rep


_RUNS = {}


def run_case(C_, case):
    """One launch per case and process; the Report's figures and failures and the
    digests of dqkv / dbias are kept for the tests that compare paths."""
    if case not in _RUNS:
        fused = FUSED_ENV and case.S <= 128
        o = launch(C_, case)
        rep = check(Report(case.name), case, o, fused)
        _RUNS[case] = dict(rep=rep, sha_dqkv=o["dqkv"].sha(), sha_dbias=o["dbias"].sha() if "dbias" in o else None)
    return _RUNS[case]


# ---- A, B, D ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_outputs_within_derived_bounds(native, case):
    assert FUSED_ENV, "run this file without DTF_ATTN_BWD_FUSED=0; the child covers that path"
    run_case(native, case)["rep"].done()


# ---- C. the keep bits, exact ------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("hsh", ["h32", "h64"])
@pytest.mark.parametrize("S", R.ALL_S)
def test_keep_bits_exact(native, S, hsh, p):
    """q = k = 0 and no bias or mask: P = 1 / S everywhere.  V one-hot on the 64-key
    block j (v[64 j + d, d] = 1), so out[b, q, h, d] = keep(b, h, q, 64 j + d) / S:
    positive exactly where the bit is set.  Element indices >= 2^32 (the hash's high
    word) are not covered: they need a probability tensor of more than 6 GB."""
    B, NH = 2, 3
    seed = R.SEEDS[hsh]
    want = R.keep_bits(seed, p, B, NH, S)
    H = NH * R.HD
    for j in range((S + 63) // 64):
        n = min(64, S - 64 * j)
        qkv = torch.zeros(B, S, 3, NH, R.HD)
        for d in range(n):
            qkv[:, 64 * j + d, 2, :, d] = 1.0
        ctx = Guarded(B * S * H, torch.bfloat16, (B, S, H))
        lse = Guarded(B * NH * S, torch.float32, (B, NH, S))
        native.attn_fwd(qkv.reshape(B, S, 3 * H).bfloat16().cuda(), None, None, ctx.t, lse.t, NH, 0.125, p, seed)
        torch.cuda.synchronize()
        assert ctx.intact() and lse.intact()
        out = R.heads(ctx.t.cpu().float(), NH, 1)[0]                    # [B, NH, S(query), 64]
        assert torch.isfinite(out).all()
        got = out[..., :n] > 0
        exp = want[..., 64 * j:64 * j + n]
        if not torch.equal(got, exp):
            bad = (got != exp).nonzero()
            raise AssertionError("S=%d block %d: %d of %d keep bits differ, first at (b, h, q, d) = %r"
                                 % (S, j, len(bad), got.numel(), bad[0].tolist()))
        assert bool((out[..., n:] == 0).all())
        # kept elements all carry the same value, about inv_keep / S
        vals = out[..., :n][got].unique()
        assert vals.numel() == 1 and abs(float(vals[0]) * S / R.inv_keep(p) - 1) <= 2 * R.U_BF, vals
        assert torch.allclose(lse.t.cpu().double(), torch.full((B, NH, S), float(torch.tensor(float(S)).log()),
                                                                dtype=torch.float64), rtol=0, atol=1e-5)


# ---- E. paths ---------------------------------------------------------------------------------

SHORT = [c for c in R.CASES if c.S <= 128]
DET_CASES = ["B-S64-B2-NH3-p0.1-h32", "A-S192-B2-NH3", "B-S256-B2-NH3-p0.5-h64"]


def determinism_failures(C_, case):
    a, b = launch(C_, case), launch(C_, case)
    bad = [k for k in a if not (a[k].intact() and b[k].intact() and torch.equal(a[k].bits(), b[k].bits()))]
    for k in ("ctx", "lse", "dqkv"):
        if torch.isnan(a[k].t.float()).any():
            bad.append(k + " has NaN")
    return bad


@pytest.mark.parametrize("name", DET_CASES)
def test_two_runs_are_bit_identical(native, name):
    assert determinism_failures(native, R.CASES[R.CASE_IDS.index(name)]) == []


def _child():
    """The S <= 128 cases of A and B under DTF_ATTN_BWD_FUSED=0: attn_bwd_dq +
    attn_bwd_dkv with one 128-row tile that is partly (S = 32, 64) idle."""
    assert os.environ.get("DTF_ATTN_BWD_FUSED") == "0" and not FUSED_ENV
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    from distributed_tensorflow_example_amd import _native
    C_ = _native.load()
    cases = []
    for case in SHORT:
        run = run_case(C_, case)
        rep = run["rep"]
        rep.true("Dbuf was not checked", "Dbuf" in rep.fig and "D" in rep.fig)
        cases.append({"case": rep.name, "fig": rep.fig, "fail": rep.fail, "sha_dqkv": run["sha_dqkv"],
                      "sha_dbias": run["sha_dbias"]})
    det = determinism_failures(C_, R.CASES[R.CASE_IDS.index(DET_CASES[0])])
    ok = all(not c["fail"] for c in cases) and not det
    print(json.dumps({"ok": ok, "determinism": det, "cases": cases}))
    return 0 if ok else 1


def test_two_kernel_backward_at_short_sequences(native):
    """One fresh child (never an exec) reruns the S <= 128 cases on the two-kernel
    backward with the same assertions plus Dbuf, and reports SHA-256 digests of
    dqkv and dbias.  The kernel file claims 'same MFMA order per output' for the
    one-workgroup kernel, so the digests must equal this process's."""
    env = dict(os.environ, DTF_ATTN_BWD_FUSED="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, cwd=REPO, timeout=180,
                       capture_output=True, text=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    out = json.loads(lines[-1])
    for c in out["cases"]:
        print(json.dumps({"case": "child " + c["case"], **c["fig"]}))
    failed = [(c["case"], c["fail"]) for c in out["cases"] if c["fail"]]
    assert not failed, failed
    assert out["determinism"] == [], out["determinism"]
    assert p.returncode == 0 and out["ok"], (p.returncode, p.stderr[-2000:])
    assert [c["case"] for c in out["cases"]] == [c.name for c in SHORT]
    differ, compared = [], 0
    for case, c in zip(SHORT, out["cases"]):
        mine = run_case(native, case)
        for k in ("sha_dqkv", "sha_dbias"):
            assert (mine[k] is None) == (c[k] is None) == (k == "sha_dbias" and not case.bias), (case.name, k)
            compared += mine[k] is not None
            if mine[k] != c[k]:
                differ.append((case.name, k))
    print(json.dumps({"case": "fused vs two-kernel digests", "compared": compared, "differ": differ}))
    assert not differ, differ


@pytest.mark.parametrize("partials", [True, False])
@pytest.mark.parametrize("S", [64, 192])
def test_bias_gradient_on_both_settings(native, monkeypatch, S, partials):
    """ops.transformer.fused_attention forward and backward with the qkv bias
    gradient from the kernels' partials (default) and from the column sums of the
    stored dqkv (DTF_ATTN_BIAS_PARTIALS=0; read at call time)."""
    from distributed_tensorflow_example_amd.ops import transformer as T
    monkeypatch.setattr(T, "_ATTN_BIAS_PARTIALS", partials)
    case = R.CASES[R.CASE_IDS.index("A-S%d-B2-NH3" % S)]
    r = R.reference(case)
    qkv, bias, mask, dO = gpu_inputs(case)
    x, b = qkv.clone().requires_grad_(), bias.clone().requires_grad_()
    out = T.fused_attention(x, b, mask, case.NH, case.scale)
    out.backward(dO)
    torch.cuda.synchronize()
    rep = Report("E bias partials=%d S=%d" % (partials, S))
    rep.bound("O", R.heads(out.cpu(), case.NH, 1)[0], r["ref"]["O"], r["tol"]["O"])
    for n, g in zip(("dQ", "dK", "dV"), R.split_dqkv(x.grad.cpu(), case.NH)):
        rep.bound(n, g, r["ref"][n], r["tol"][n])
    rep.true("dbias dtype / shape", b.grad.dtype == torch.float32 and b.grad.shape == bias.shape)
    rep.bound("dbias", b.grad, r["ref"]["dbias"], r["tol"]["dbias" if partials else "dbias_stored"])
    if not partials:        # the column sums of the stored values themselves, fp32-sized
        stored = x.grad.cpu().double().sum((0, 1))
        rep.bound("dbias vs stored dqkv", b.grad, stored,
                  R.gamma(case.B * case.S) * x.grad.cpu().double().abs().sum((0, 1)) + R.TINY)
    rep.done()


@pytest.mark.parametrize("S", [64, 192])
def test_bias_gradient_accumulates_into_prior(native, S):
    case = R.CASES[R.CASE_IDS.index("A-S%d-B2-NH3" % S)]
    prior = torch.randn(3 * case.NH * R.HD, generator=torch.Generator().manual_seed(S)).cuda()
    o = launch(native, case, dbias_prior=prior)
    check(Report("E accumulate S=%d" % S), case, o, case.S <= 128, dbias_prior=prior).done()


if __name__ == "__main__":
    if sys.argv[1:] != ["child"]:
        sys.exit("usage: %s child" % sys.argv[0])
    sys.exit(_child())
