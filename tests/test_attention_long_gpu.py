"""The long-sequence fused attention (csrc/kernels/attention_long.hip: attn_long_fwd,
attn_long_bwd_dq, attn_long_bwd_dkv; S = 384 ... 2048) per element against the float64
model, within the derived bounds of tests/attention_long_reference.py -- none is fitted
to what the kernels give -- and with the dropout bits read off exactly.

The kernels are reached as the model reaches them, through attn_fwd / attn_bwd of the
binding, into guarded NaN-filled buffers (Guarded, Report and launch are
tests/test_attention_edges_gpu.py's).

  A  p = 0: O, lse, D, dQ, dK, dV, the bpart rows and dbias per element; S = 384 at
     (B, NH) = (1, 1) and (2, 3), 512 at (2, 3), 640 at (2, 2) (an odd count of 128-key
     blocks), 1024 at (1, 2); at 384 also without bias, without mask, scale 1/4, and a
     wholly masked first block.  Batch element 0 carries the ascending staircase mask,
     the others the graded one.  dK / dV rows of masked keys are exactly 0.
  B  dropout p = 0.1 / 0.5 on both hash branches at S = 384 and 512, same checks.
  C  the keep bits, exact, by the one-hot V of test_keep_bits_exact, every 64-key block.
  E  two runs bit for bit, dbias accumulated onto a prior, Dbuf against the ctx it was
     handed; through ops.transformer under autograd at 384 (against the model) and at
     2048 (against the fp32 reference on the GPU); fused and composed path drop the same
     elements; routing and the refusal of S = 320; DTF_ATTN_LONG=0 in one child
     process; a tiny BERT at S = 384 with the fused attention on and off.

Every case prints one JSON line (pytest -s) with the worst error / bound per output.

Figures on an MI355X when this file was written (worst error / bound over the 17 cases
of A and B; the 36 tests take 9 s): O 0.57 ... 0.84, dV 0.75 ... 0.88 (both limited by the
bf16 store), dQ 0.16 ... 0.50, dK 0.22 ... 0.41, lse 0.016 ... 0.026, D 0.10 ... 0.20,
Dbuf 0.031 ... 0.059, bpart 0.27 ... 0.56, dbias 0.018 ... 0.048 -- to three digits the
figures of the CPU emulation at 64-key blocks.  S = 2048 against the fp32 reference:
out 0.0056, dqkv 0.0076, dbias 0.0068 relative.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import attention_long_reference as L
import attention_reference as R
from test_attention_edges_gpu import Guarded, Report, launch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _long_form():
    if os.environ.get("DTF_ATTN_LONG") == "0":
        pytest.skip("DTF_ATTN_LONG=0: this process has no long form (the child test covers that setting)")


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def gpu_inputs(c):
    return tuple(None if t is None else t.cuda() for t in L.inputs(c))


def check(rep, c, o, dbias_prior=None):
    r = L.reference(c)
    ref, tol = r["ref"], r["tol"]
    qkv, bias, mask, dO = L.inputs(c)
    for k, b in o.items():
        rep.true("guard of %s overwritten" % k, b.intact())
        rep.true("%s not fully written / not finite" % k, torch.isfinite(b.t.float()).all())
    dref, dtol = R.dbuf_reference(o["ctx"].t.cpu(), dO, c.NH)
    rep.bound("Dbuf", o["Dbuf"].t, dref, dtol)               # fp32-sized: from the ctx it was handed
    rep.bound("D", o["Dbuf"].t, ref["D"], tol["D"])          # and against the model's D
    got = dict(O=R.heads(o["ctx"].t.cpu(), c.NH, 1)[0], lse=o["lse"].t.cpu())
    got["dQ"], got["dK"], got["dV"] = R.split_dqkv(o["dqkv"].t.cpu(), c.NH)
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
        if c.B > 1:
            rep.true("no masked key in the case", bool(dead.any()))
        for n in ("dK", "dV"):
            rep.true("%s of a masked key is not exactly 0" % n, bool((got[n].float()[dead] == 0).all()))
    return rep


# ---- A, B -------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", L.CASES, ids=L.CASE_IDS)
def test_outputs_within_derived_bounds(native, c):
    o = launch(native, c, tensors=gpu_inputs(c))
    check(Report(c.name), c, o).done()


# ---- C. the keep bits, exact ------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("hsh", ["h32", "h64"])
@pytest.mark.parametrize("S", [384, 512])
def test_keep_bits_exact(native, S, hsh, p):
    """q = k = 0 and no bias or mask: P = 1 / S everywhere.  V one-hot on the 64-key
    block j, so out[b, q, h, d] = keep(b, h, q, 64 j + d) / S: positive exactly where
    the bit is set."""
    B, NH = 2, 3
    seed = R.SEEDS[hsh]
    want = R.keep_bits(seed, p, B, NH, S)
    H = NH * R.HD
    lse_want = torch.full((B, NH, S), float(torch.tensor(float(S)).log()), dtype=torch.float64)
    for j in range(S // 64):
        qkv = torch.zeros(B, S, 3, NH, R.HD)
        for d in range(64):
            qkv[:, 64 * j + d, 2, :, d] = 1.0
        ctx = Guarded(B * S * H, torch.bfloat16, (B, S, H))
        lse = Guarded(B * NH * S, torch.float32, (B, NH, S))
        native.attn_fwd(qkv.reshape(B, S, 3 * H).bfloat16().cuda(), None, None, ctx.t, lse.t, NH, 0.125, p, seed)
        torch.cuda.synchronize()
        assert ctx.intact() and lse.intact()
        out = R.heads(ctx.t.cpu().float(), NH, 1)[0]                    # [B, NH, S(query), 64]
        assert torch.isfinite(out).all()
        got = out > 0
        exp = want[..., 64 * j:64 * j + 64]
        if not torch.equal(got, exp):
            bad = (got != exp).nonzero()
            raise AssertionError("S=%d block %d: %d of %d keep bits differ, first at (b, h, q, d) = %r"
                                 % (S, j, len(bad), got.numel(), bad[0].tolist()))
        vals = out[got].unique()
        # e = 1 exactly, bf16(inv_keep) is the PV operand, then one product with 1 / l
        assert vals.numel() == 1 and abs(float(vals[0]) * S / R.inv_keep(p) - 1) <= 2 * R.U_BF, vals
        assert torch.allclose(lse.t.cpu().double(), lse_want, rtol=0, atol=1e-5)


# ---- E. repeats, dbias, paths -----------------------------------------------------------------

@pytest.mark.parametrize("name", ["B-S384-B2-NH3-p0.1-h32", "A-S640-B2-NH2", "B-S512-B2-NH3-p0.5-h64"])
def test_two_runs_are_bit_identical(native, name):
    c = L.case(name)
    t = gpu_inputs(c)
    a, b = launch(native, c, tensors=t), launch(native, c, tensors=t)
    bad = [k for k in a if not (a[k].intact() and b[k].intact() and torch.equal(a[k].bits(), b[k].bits()))]
    for k in a:
        if torch.isnan(a[k].t.float()).any():
            bad.append(k + " has NaN")
    assert bad == []


def test_bias_gradient_accumulates_into_prior(native):
    c = L.case("A-S384-B2-NH3")
    prior = torch.randn(3 * c.NH * R.HD, generator=torch.Generator().manual_seed(384)).cuda()
    o = launch(native, c, tensors=gpu_inputs(c), dbias_prior=prior)
    check(Report("E accumulate S=384"), c, o, dbias_prior=prior).done()


def test_fused_attention_under_autograd_at_384(native):
    from distributed_tensorflow_example_amd.ops import transformer as T
    c = L.case("A-S384-B2-NH3")
    r = L.reference(c)
    qkv, bias, mask, dO = gpu_inputs(c)
    assert T.attention_supported(c.S, 64)
    x, b = qkv.clone().requires_grad_(), bias.clone().requires_grad_()
    out = T.fused_attention(x, b, mask, c.NH, c.scale)
    out.backward(dO)
    torch.cuda.synchronize()
    rep = Report("E autograd S=384")
    rep.bound("O", R.heads(out.cpu(), c.NH, 1)[0], r["ref"]["O"], r["tol"]["O"])
    for n, g in zip(("dQ", "dK", "dV"), R.split_dqkv(x.grad.cpu(), c.NH)):
        rep.bound(n, g, r["ref"][n], r["tol"][n])
    rep.true("dbias dtype / shape", b.grad.dtype == torch.float32 and b.grad.shape == bias.shape)
    rep.bound("dbias", b.grad, r["ref"]["dbias"], r["tol"]["dbias"])
    rep.done()


def test_fused_attention_matches_fp32_reference_at_2048(native):
    """The largest supported S, against ops.transformer.attention_reference in fp32 on
    the GPU, with the tolerances of test_fused_attention_matches_fp32_reference."""
    from distributed_tensorflow_example_amd.ops import transformer as T
    S, B, nh, scale = 2048, 1, 1, 1 / 8
    assert T.attention_supported(S, 64)
    torch.manual_seed(S)
    qkv = (torch.randn(B, S, 3 * nh * 64) * 2).bfloat16().cuda()
    bias = (torch.randn(3 * nh * 64) * 0.5).cuda()
    mask = torch.zeros(B, S)
    mask[0, S - 5:] = -10000.0
    mask = mask.cuda()
    xr, br = qkv.float().requires_grad_(), bias.clone().requires_grad_()
    ref = T.attention_reference(xr, br, mask, nh, scale)
    dy = torch.randn_like(ref)
    ref.backward(dy)
    xg, bg = qkv.clone().requires_grad_(), bias.clone().requires_grad_()
    out = T.fused_attention(xg, bg, mask, nh, scale)
    out.backward(dy.bfloat16())
    assert out.shape == (B, S, nh * 64) and out.dtype == torch.bfloat16
    fig = dict(out=rel(out, ref), dqkv=rel(xg.grad, xr.grad), dbias=rel(bg.grad, br.grad),
               dbias_vs_stored=rel(bg.grad, xg.grad.float().sum((0, 1))))
    print(json.dumps({"case": "E S=2048", **{k: float("%.3g" % v) for k, v in fig.items()}}))
    assert fig["out"] < 1e-2
    assert fig["dqkv"] < 3e-2
    for part in range(3):
        sl = slice(part * nh * 64, (part + 1) * nh * 64)
        assert rel(xg.grad[..., sl], xr.grad[..., sl]) < 3e-2, part
    assert fig["dbias"] < 3e-2
    assert fig["dbias_vs_stored"] < 5e-3


def _unfused_attention(qkv, bias, mask, nh, scale, p):
    """The model's composed GPU path: bias add, batched GEMMs, softmax kernel."""
    from distributed_tensorflow_example_amd.ops import transformer as T
    B, S, H3 = qkv.shape
    d = H3 // (3 * nh)
    x = (qkv + bias.to(qkv.dtype)).view(B, S, 3, nh, d)
    q, k, v = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 3, 1), x[:, :, 2].permute(0, 2, 1, 3)
    probs = T.attention_softmax(torch.matmul(q, k), mask, scale, p)
    return torch.matmul(probs.to(v.dtype), v).permute(0, 2, 1, 3).reshape(B, S, nh * d)


def test_fused_and_composed_paths_drop_the_same_elements_at_384(native):
    """Same seed -> the streamed kernels drop exactly the elements the softmax kernel
    drops (tolerances of test_fused_attention_dropout_matches_unfused_kernel_path)."""
    from distributed_tensorflow_example_amd.ops import transformer as T
    torch.manual_seed(0)
    B, S, nh, p = 2, 384, 4, 0.2
    qkv = torch.randn(B, S, 3 * nh * 64, device="cuda").bfloat16()
    bias = torch.randn(3 * nh * 64, device="cuda") * 0.3
    mask = torch.zeros(B, S, device="cuda")
    mask[0, 300:] = -10000.0
    dy = torch.randn(B, S, nh * 64, device="cuda").bfloat16()
    outs = []
    for fused in (True, False):
        T.set_dropout_seed(1234)
        x, b = qkv.clone().requires_grad_(), bias.clone().requires_grad_()
        o = T.fused_attention(x, b, mask, nh, 0.125, p) if fused else _unfused_attention(x, b, mask, nh, 0.125, p)
        o.backward(dy)
        outs.append((o, x.grad, b.grad))
    (o1, g1, b1), (o2, g2, b2) = outs
    assert rel(o1, o2) < 2e-2
    assert rel(g1, g2) < 4e-2
    assert rel(b1, b2) < 4e-2


def test_routing(native):
    from distributed_tensorflow_example_amd.ops import transformer as T
    for S in (384, 512, 640, 1024, 2048):
        assert T.attention_supported(S, 64) and native.attn_supported(S, 64), S
    for S in (320, 2176, 96):
        assert not T.attention_supported(S, 64), S
    for S in (384, 128):
        assert not T.attention_supported(S, 32), S
    for S in (32, 64, 128, 192, 256):
        assert T.attention_supported(S, 64), S


def test_refusal_at_320_leaves_outputs_untouched(native):
    B, S, NH = 1, 320, 2
    H, H3 = NH * R.HD, 3 * NH * R.HD
    qkv = torch.randn(B, S, H3, device="cuda").bfloat16()
    dO = torch.randn(B, S, H, device="cuda").bfloat16()
    o = dict(ctx=Guarded(B * S * H, torch.bfloat16, (B, S, H)), lse=Guarded(B * NH * S, torch.float32, (B, NH, S)),
             dqkv=Guarded(B * S * H3, torch.bfloat16, (B, S, H3)), Dbuf=Guarded(B * NH * S, torch.float32, (B, NH, S)))
    with pytest.raises(RuntimeError, match="unsupported sequence length"):
        native.attn_fwd(qkv, None, None, o["ctx"].t, o["lse"].t, NH, 0.125, 0.0, 0)
    with pytest.raises(RuntimeError, match="unsupported sequence length"):
        native.attn_bwd(qkv, None, None, o["ctx"].t, dO, o["lse"].t, o["Dbuf"].t, o["dqkv"].t, NH, 0.125, 0.0, 0)
    torch.cuda.synchronize()
    for k, b in o.items():
        assert b.intact() and bool(torch.isnan(b.t.float()).all()), k


def _tiny_bert_step(fused, S=384, seed=6):
    from distributed_tensorflow_example_amd.models.bert import BertConfig, BertForMLM, synthetic_mlm_batch
    c = BertConfig.tiny()
    c.max_position = S
    c.dropout = c.attn_dropout = 0.0
    c.fused_attention = fused
    b = [t.cuda() for t in synthetic_mlm_batch(2, S, c.vocab_size, "cpu", seed=4)]
    model = BertForMLM(c, seed=seed).cuda()
    loss = model(*b)
    loss.backward()
    torch.cuda.synchronize()
    return model, float(loss.detach())


def _child():
    """DTF_ATTN_LONG=0: the long form is refused as before and the model takes the composed path."""
    assert os.environ.get("DTF_ATTN_LONG") == "0"
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    from distributed_tensorflow_example_amd.ops import transformer as T
    out = dict(supported_384=T.attention_supported(384, 64), supported_512=T.attention_supported(512, 64),
               supported_256=T.attention_supported(256, 64))
    calls = []
    orig = T.fused_attention
    T.fused_attention = lambda *a, **k: calls.append(1) or orig(*a, **k)
    model, loss = _tiny_bert_step(True)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    out.update(loss=loss, fused_calls=len(calls), grads=len(grads),
               finite=all(bool(torch.isfinite(g).all()) for g in grads))
    print(json.dumps(out))
    return 0


def test_long_form_switched_off_in_a_child_process():
    """One fresh child (never an exec) with DTF_ATTN_LONG=0: attention_supported(384, 64)
    is false, S <= 256 stays, and a tiny BERT with max_position 384 still runs a step."""
    env = dict(os.environ, DTF_ATTN_LONG="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, cwd=REPO, timeout=180,
                       capture_output=True, text=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    out = json.loads(lines[-1])
    print(json.dumps({"case": "child DTF_ATTN_LONG=0", **out}))
    assert out["supported_384"] is False and out["supported_512"] is False and out["supported_256"] is True
    assert out["fused_calls"] == 0 and out["grads"] > 0 and out["finite"]
    assert out["loss"] == out["loss"] and 0 < out["loss"] < 20


def test_tiny_bert_at_384_fused_attention_on_and_off(native):
    """One forward and backward, no dropout: the streamed kernels against the composed
    path (tolerance of test_bert_residual_grad_slot_matches_autograd_add)."""
    from distributed_tensorflow_example_amd.ops import transformer as T
    calls = []
    orig = T.fused_attention
    T.fused_attention = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        fused, loss_f = _tiny_bert_step(True)
        n_fused = len(calls)
        plain, loss_p = _tiny_bert_step(False)
    finally:
        T.fused_attention = orig
    assert n_fused == 2 and len(calls) == 2, calls          # one per layer, none with the flag off
    assert abs(loss_f - loss_p) < 2e-2 * abs(loss_p), (loss_f, loss_p)
    for (n, p1), p2 in zip(plain.named_parameters(), fused.parameters()):
        if p1.grad is not None and p1.grad.norm() > 1e-6:
            assert rel(p2.grad, p1.grad) < 2e-2, n


if __name__ == "__main__":
    if sys.argv[1:] != ["child"]:
        sys.exit("usage: %s child" % sys.argv[0])
    sys.exit(_child())
