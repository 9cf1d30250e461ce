"""Float64 models of the row kernels of csrc/kernels/transformer.hip (the LayerNorm
family, bias + GELU, the attention softmax pair, dropout_bf16), the per-element
error bounds their outputs are held to, and an fp32 / bf16 emulation of the
kernels' arithmetic, with mutants, that shows on the CPU that the bounds are
attainable and have power.

A helper module, not a test file: `import transformer_reference` (pytest puts
tests/ on sys.path).  Nothing here imports the GPU or the package;
tests/test_transformer_reference_cpu.py checks the models against float64
autograd, tests/test_transformer_edges_gpu.py holds the kernels to them.

Conventions of the kernels that the models follow:
  * bf16 and fp32 inputs are taken exactly as given.
  * bdrln: v = dropout(x + bias) + res, y = LN(v) gamma + beta, s = v.
  * ln_fwd_f32in / emb_ln_fwd: v = x (or word[ids] + typ[tt] + pos[row % S]),
    y = dropout(LN(v) gamma + beta), s = v undropped.
  * the dropout element index is the flat row * H + col (softmax: row * Sk + col);
    keep(i) = hash32(seed, i) >= thresh, kept values are scaled by the C float
    1.f / (1.f - p).
  * the backward models take what the kernels are handed: ln_bwd the bf16 s and the
    fp32 mean / rstd, softmax_bwd the bf16 P the forward stored.
  * Pd is the rounding of the fp32 p * inv_keep, not of the stored P.

Bounds: first-order worst case, from the model's own quantities, nothing fitted.
u = 2^-8 per stored bf16 value, W = 2^-24 per fp32 operation, INTR ulps for
__expf / rsqrtf / rcp (attention_reference.INTR).  A row sum is held to
gamma(d) sum |x| with d the depth of the kernel's addition tree (the terms a lane
adds in sequence plus the shuffle steps); the emulation adds in a binary tree,
which is never deeper.  A column sum over N rows is held to gamma(N) in any order.
The LayerNorm bounds carry the row's conditioning: the error of v - mean is
multiplied by rstd, so a near-constant row gets a wide bound, not a false failure.

GELU: the kernels take the normal cdf from the Abramowitz-Stegun 7.1.26 polynomial,
whose documented error is absolute: 1.5e-7 on erf, so AS_CDF = 7.5e-8 on the cdf
(evaluated in float64 its worst cdf error is 6.97e-8).  y = z cdf therefore gets
u |y| + 7.5e-8 |z| plus the fp32 terms, gelu' gets 7.5e-8 plus the fp32 terms.  A
purely relative bound would be wrong below z = -6 or so: there y = z cdf(z) is
about 1e-8 and smaller, and the polynomial's absolute error reaches a bf16 ulp of
y itself.
"""
import collections
import functools
import math

import numpy as np
import torch

import attention_reference as A
from attention_reference import (INTR, SECOND_ORDER, SEEDS, TINY, U_BF, W, attn_thresh, elem_ratio, gamma, hash32,
                                 inv_keep)

AS_CDF = 7.5e-8      # Abramowitz-Stegun 7.1.26: |erf error| <= 1.5e-7, halved for the cdf
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
EPS = 1e-12          # BERT's LayerNorm epsilon
SO = SECOND_ORDER


def f32(x):
    """A Python float rounded to fp32, as a kernel argument is."""
    return float(np.float32(x))


# ---------------------------------------------------------------- dropout bits

def keep_bits_rows(seed, p, rows, width):
    """bool [len(rows), width]: element rows[r] * width + c is kept."""
    rows = np.asarray(rows, dtype=np.uint64)
    if attn_thresh(p) == 0:
        return torch.ones(len(rows), width, dtype=torch.bool)
    i = rows[:, None] * np.uint64(width) + np.arange(width, dtype=np.uint64)[None, :]
    return torch.from_numpy(hash32(seed, i) >= np.uint32(attn_thresh(p)))


def keep_bits(seed, p, n_rows, width):
    return keep_bits_rows(seed, p, np.arange(n_rows), width)


def keep_scale(bits, p):
    """float64: inv_keep where kept, else 0 (all 1 for p <= 0)."""
    return bits.double() * (inv_keep(p) if attn_thresh(p) else 1.0)


# ---------------------------------------------------------------- LayerNorm forward

LN_KINDS = ("bdrln", "f32in", "emb")


def ln_input(kind, inp, keep):
    """v (float64), the fp32 error of the kernel's v, and the dropout scale that
    acts on y (None for bdrln, whose dropout is inside v)."""
    if kind == "bdrln":
        t = inp["x"].double() + inp["bias"].double()
        d = t * keep                                     # fl(x + bias) * inv_keep: two roundings on |d|
        e = 2 * W * d.abs()
        if inp.get("res") is not None:
            v = d + inp["res"].double()
            e = e + W * v.abs()
        else:
            v = d
        return v, e, None
    if kind == "f32in":
        return inp["x"].double(), torch.zeros_like(inp["x"], dtype=torch.float64), keep
    rows = inp["rows"] if "rows" in inp else torch.arange(inp["ids"].numel())      # the rows' own numbers
    a = inp["word"].double()[inp["ids"].reshape(-1)] + inp["typ"].double()[inp["tt"].reshape(-1)]
    v = a + inp["pos"].double()[rows % inp["S"]]
    return v, W * (a.abs() + v.abs()), keep


def ln_fwd_model(kind, inp, keep, eps=EPS, u=U_BF):
    """ref and tol dicts over y, s, mean, rstd.  keep: keep_scale(...) [N, H]."""
    g, b = inp["gamma"].double(), inp["beta"].double()
    v, e_v, ykeep = ln_input(kind, inp, keep)
    H = v.shape[-1]
    G = gamma(H // 32 + 5)        # bdrln_fwd16: 8 NC = H / 32 terms per lane, 5 shuffles; the 8-byte forms H / 64 + 6
    eps = f32(eps)
    mean = v.mean(-1, keepdim=True)
    e_mean = SO * (e_v.mean(-1, keepdim=True) + G * v.abs().mean(-1, keepdim=True) + W * mean.abs())
    dl = v - mean
    e_d = e_v + e_mean + W * dl.abs()
    var = (dl * dl).mean(-1, keepdim=True)
    e_var = SO * ((2 * dl.abs() * e_d).mean(-1, keepdim=True) + (G + 2 * W) * var)
    q = var + eps
    rstd = q ** -0.5
    e_rstd = SO * rstd * (0.5 * (e_var + W * q) / q + 2 * W * INTR)
    xh = dl * rstd
    e_xh = e_d * rstd + dl.abs() * e_rstd + W * xh.abs()      # rstd * (error of v - mean): the conditioning
    y = xh * g + b
    e_y = SO * (g.abs() * (e_xh + W * xh.abs()) + W * y.abs())
    if ykeep is not None:
        y = y * ykeep
        e_y = ykeep * e_y + W * y.abs()
    ref = dict(y=y, s=v, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1))
    tol = dict(y=u * y.abs() + (1 + u) * e_y + TINY, s=u * v.abs() + (1 + u) * e_v + TINY,
               mean=e_mean.squeeze(-1) + TINY, rstd=e_rstd.squeeze(-1) + TINY)
    return ref, tol


def _bf(x):
    return x.bfloat16().float()


def tsum(x):
    """fp32 sum over the last axis in a binary tree (depth ceil(log2 n))."""
    n = x.shape[-1]
    m = 1 << max(0, (n - 1).bit_length())
    if m != n:
        x = torch.cat([x, x.new_zeros(x.shape[:-1] + (m - n,))], -1)
    while m > 1:
        m //= 2
        x = x[..., :m] + x[..., m:2 * m]
    return x


LN_FWD_MUTANTS = ("one_pass_var", "tail_row_stats", "drop_after_residual", "mask_no_row_base", "pos_row_mod_off")


def ln_fwd_emulate(kind, inp, seed, p, eps=EPS, mutant=None):
    """The kernels' arithmetic in torch float32, bf16 at the stores."""
    assert mutant is None or mutant in LN_FWD_MUTANTS
    g, b = inp["gamma"].float(), inp["beta"].float()
    N = inp["ids"].numel() if kind == "emb" else inp["x"].shape[0]
    H = g.numel()
    bits = keep_bits(seed, p, N, H)
    if mutant == "mask_no_row_base":
        bits = keep_bits(seed, p, 1, H).expand(N, H)
    kp = bits.float() * torch.tensor(inv_keep(p) if attn_thresh(p) else 1.0, dtype=torch.float32)
    if kind == "bdrln":
        t = inp["x"].float() + inp["bias"].float()
        r = inp["res"].float() if inp.get("res") is not None else None
        if mutant == "drop_after_residual" and r is not None:
            v = (t + r) * kp
        else:
            v = t * kp
            if r is not None:
                v = v + r
    elif kind == "f32in":
        v = inp["x"].float()
    else:
        rows = torch.arange(N)
        pr = (rows + 1) % inp["S"] if mutant == "pos_row_mod_off" else rows % inp["S"]
        v = (inp["word"][inp["ids"].reshape(-1)] + inp["typ"][inp["tt"].reshape(-1)]) + inp["pos"][pr]
    mean = tsum(v) / H
    if mutant == "one_pass_var":
        var = tsum(v * v) / H - mean * mean
    else:
        dl = v - mean
        var = tsum(dl * dl) / H
    rstd = (var + torch.tensor(f32(eps))).double().rsqrt().float()
    if mutant == "tail_row_stats" and N % 2 == 1 and N > 1:
        mean, rstd = mean.clone(), rstd.clone()
        mean[N - 1], rstd[N - 1] = mean[N - 2], rstd[N - 2]
    y = ((v - mean) * rstd) * g + b
    if kind != "bdrln":
        y = y * kp
    return dict(y=_bf(y).double(), s=_bf(v).double(), mean=mean.squeeze(-1).double(), rstd=rstd.squeeze(-1).double())


# ---------------------------------------------------------------- LayerNorm backward

LN_BWD_OUTPUTS = ("ds", "dxb", "dgamma", "dbeta", "dbias")


def ln_bwd_model(dy, s, mean, rstd, g, keep, u=U_BF):
    """dy, s bf16 [N, H]; mean, rstd fp32 [N] as ln_bwd is handed them; keep [N, H]."""
    dy, s, g = dy.double(), s.double(), g.double()
    mean, rstd = mean.double().unsqueeze(-1), rstd.double().unsqueeze(-1)
    N, H = dy.shape
    G = gamma(H // 64 + 6)
    xh = (s - mean) * rstd
    e_xh = 2 * W * xh.abs()
    gdy = dy * g
    s1 = gdy.mean(-1, keepdim=True)
    s2 = (gdy * xh).mean(-1, keepdim=True)
    e_s1 = SO * ((W + G) * gdy.abs().mean(-1, keepdim=True) + W * s1.abs())
    e_s2 = SO * ((4 * W + G) * (gdy * xh).abs().mean(-1, keepdim=True) + W * s2.abs())
    inner = gdy - s1 - xh * s2
    e_in = (W * gdy.abs() + e_s1 + xh.abs() * e_s2 + s2.abs() * e_xh + W * (xh * s2).abs()
            + 2 * W * (gdy.abs() + s1.abs() + (xh * s2).abs()))
    ds = rstd * inner
    e_ds = SO * (rstd * e_in + W * ds.abs())
    dxb = ds * keep
    e_dxb = keep * e_ds + W * dxb.abs()
    dg = dy * xh
    ref = dict(ds=ds, dxb=dxb, dgamma=dg.sum(0), dbeta=dy.sum(0), dbias=dxb.sum(0))
    tol = dict(ds=u * ds.abs() + (1 + u) * e_ds + TINY, dxb=u * dxb.abs() + (1 + u) * e_dxb + TINY,
               dgamma=SO * (3 * W + gamma(N)) * dg.abs().sum(0) + TINY,
               dbeta=gamma(N) * dy.abs().sum(0) + TINY,
               dbias=SO * (e_dxb.sum(0) + gamma(N) * dxb.abs().sum(0)) + TINY)
    return ref, tol


LN_BWD_MUTANTS = ("ds_no_s2", "colsum_skip_last_row", "dxb_unmasked")


def ln_bwd_emulate(dy, s, mean, rstd, g, keep, mutant=None):
    assert mutant is None or mutant in LN_BWD_MUTANTS
    dy, s, g, kp = dy.float(), s.float(), g.float(), keep.float()
    mean, rstd = mean.float().unsqueeze(-1), rstd.float().unsqueeze(-1)
    N, H = dy.shape
    xh = (s - mean) * rstd
    gdy = dy * g
    s1 = tsum(gdy) / H
    s2 = tsum(gdy * xh) / H
    d = rstd * (gdy - s1 - (0 if mutant == "ds_no_s2" else xh * s2))
    dx = d if mutant == "dxb_unmasked" else d * kp
    n = N - 1 if mutant == "colsum_skip_last_row" else N
    out = dict(ds=_bf(d), dxb=_bf(dx), dgamma=(dy * xh)[:n].sum(0), dbeta=dy[:n].sum(0), dbias=dx[:n].sum(0))
    return {k: t.double() for k, t in out.items()}


# ---------------------------------------------------------------- embedding backward (exact, integer-valued ds)

def emb_bwd_aux_model(ds, tt, S, mutant=None):
    """pos_grad [S, H] and typ_grad [2, H] of ds [B * S, H]."""
    assert mutant in (None, "typ_swapped")
    d = ds.double()
    H = d.shape[-1]
    one = (tt.reshape(-1) != 0)
    if mutant == "typ_swapped":
        one = ~one
    pos = d.reshape(-1, S, H).sum(0)
    typ = torch.stack([d[~one].sum(0), d[one].sum(0)])
    return pos, typ


# ---------------------------------------------------------------- bias + GELU

def _as_poly(t):
    a1, a2, a3, a4, a5 = AS_A
    p = t * (a1 + t * (a2 + t * (a3 + t * (a4 + t * a5))))
    mag = sum(abs(a) * t ** (i + 1) for i, a in enumerate(AS_A))
    dmag = sum((i + 1) * abs(a) * t ** (i + 1) for i, a in enumerate(AS_A))
    return p, mag, dmag


def gelu_model(x, bias, dy, u=U_BF):
    """y = z cdf(z), dx = dy (cdf + z pdf), dbias = column sums of the fp32 dx; z = x + bias."""
    z = x.double() + bias.double()
    dy = dy.double()
    N = z.shape[0]
    az = z.abs()
    cdf = 0.5 * torch.special.erfc(-z / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    tail = 0.5 * torch.special.erfc(az / math.sqrt(2.0))
    e_z = W * az                                           # fl(x + bias)
    # t = rcp(fma(P, |z| c, 1)): the constant c and the product (2 W), the fma (W), the rcp
    t = 1.0 / (1.0 + AS_P * az / math.sqrt(2.0))
    rel_t = W * (2 * INTR + 3)
    poly, mag, dmag = _as_poly(t)
    # Horner of degree 5 with separate or fused steps: gamma(10), the coefficients' rounding W
    rel_poly = ((gamma(10) + W) * mag + rel_t * dmag) / poly.abs()
    arg = 0.5 * z * z
    rel_e = 2 * W * arg + 2 * W * (INTR + arg)             # two products, then __expf
    e_tail = tail * (rel_poly + rel_e + 2 * W)
    e_cdf = AS_CDF + e_tail + W * cdf + pdf * e_z
    y = z * cdf
    e_y = SO * (az * e_cdf + cdf * e_z + W * y.abs())
    gp = cdf + z * pdf
    e_g = SO * (e_cdf + az * pdf * (rel_e + 2 * W) + (pdf * (1 - z * z)).abs() * e_z + W * gp.abs())
    dx = dy * gp
    e_dx = dy.abs() * e_g + W * dx.abs()
    ref = dict(y=y, dx=dx, dbias=dx.sum(0), z=z)
    tol = dict(y=u * y.abs() + (1 + u) * e_y + TINY, dx=u * dx.abs() + (1 + u) * e_dx + TINY,
               dbias=SO * (e_dx.sum(0) + gamma(N) * dx.abs().sum(0)) + TINY)
    return ref, tol


GELU_MUTANTS = ("bias_col_shift", "grad_cdf_only", "strip_tail_dropped")


def gelu_emulate(x, bias, dy, mutant=None):
    """gelu_cdf_pdf of csrc/kernels/common.h in torch float32."""
    assert mutant is None or mutant in GELU_MUTANTS
    c = lambda v: torch.tensor(v, dtype=torch.float32)      # noqa: E731
    bias = bias.float()
    if mutant == "bias_col_shift":
        bias = torch.roll(bias, -4)
    z = x.float() + bias
    ax = z.abs() * c(0.70710678118654752)
    t = 1.0 / (c(AS_P) * ax + 1.0)
    a1, a2, a3, a4, a5 = (c(a) for a in AS_A)
    poly = t * (t * (t * (t * (t * a5 + a4) + a3) + a2) + a1)
    e = torch.exp(c(-0.5) * z * z)
    tail = c(0.5) * poly * e
    cdf = torch.where(z >= 0, 1.0 - tail, tail)
    pdf = c(0.3989422804014327) * e
    y = z * cdf
    dx = dy.float() * (cdf if mutant == "grad_cdf_only" else z * pdf + cdf)
    y, dxs = _bf(y), _bf(dx)
    if mutant == "strip_tail_dropped":
        H = z.shape[-1]
        c0 = 1024 * (H // 1024)
        y, dxs, dx = y.clone(), dxs.clone(), dx.clone()
        y[:, c0:], dxs[:, c0:], dx[:, c0:] = 0, 0, 0
    return dict(y=y.double(), dx=dxs.double(), dbias=dx.sum(0).double())


# ---------------------------------------------------------------- attention softmax

def softmax_nc(Sk):
    """The template width the launcher picks (4 NC terms per lane)."""
    return 1 if Sk <= 256 else 2 if Sk <= 512 else 4 if Sk <= 1024 else 8 if Sk <= 2048 else 16


def _row_mask(mask, rows, rows_per_batch, dtype):
    if mask is None:
        return 0.0
    idx = torch.arange(rows) // rows_per_batch
    return mask.to(dtype)[idx]


def softmax_fwd_model(S, mask, rows_per_batch, scale, keep, u=U_BF):
    """S bf16 [rows, Sk]; mask fp32 [B, Sk] or None.  ref / tol over P, Pd, plus
    'rowsum' in tol: the relative bound of the fp32 row sum."""
    s = S.double()
    rows, Sk = s.shape
    scale = f32(scale)
    m = _row_mask(mask, rows, rows_per_batch, torch.float64)
    z = scale * s + m
    e_z = W * ((scale * s).abs() + z.abs())                 # the product and the sum; W |z| matters at -10000
    mx = z.max(-1, keepdim=True).values
    P = torch.softmax(z, -1)
    x1 = (z - mx).abs()
    r = e_z + W * x1 + 2 * W * (INTR + x1)                  # any mx cancels between e and sum(e)
    rho = (P * r).sum(-1, keepdim=True) + gamma(4 * softmax_nc(Sk) + 6)
    f = SO * (r + rho + 2 * W * INTR + W)                   # 1 / sum (INTR ulp) and the product
    Pd = P * keep
    ref = dict(P=P, Pd=Pd, z=z)
    tol = dict(P=P * (u + f * (1 + u)) + TINY, Pd=Pd * (u + (f + W) * (1 + u)) + TINY, rowsum=rho.squeeze(-1))
    return ref, tol


def softmax_bwd_model(dPd, P, scale, keep, u=U_BF):
    """dS = scale P (dP - sum(dP P)), dP = dPd keep, from the bf16 P it is handed."""
    dpd, P = dPd.double(), P.double()
    Sk = P.shape[-1]
    scale = f32(scale)
    dp = dpd * keep
    G = gamma(4 * softmax_nc(Sk) + 6)
    dot = (dp * P).sum(-1, keepdim=True)
    e_dot = SO * (2 * W + G) * (dp * P).abs().sum(-1, keepdim=True)
    dS = scale * P * (dp - dot)
    e_dS = SO * ((scale * P).abs() * (W * dp.abs() + e_dot + W * (dp.abs() + dot.abs())) + 2 * W * dS.abs())
    return dict(dS=dS), dict(dS=u * dS.abs() + (1 + u) * e_dS + TINY)


SOFTMAX_MUTANTS = ("mask_other_batch", "last_group_dropped", "bwd_dot_undropped")


def softmax_emulate(S, mask, rows_per_batch, scale, keep, dPd, mutant=None):
    """Forward, then the backward from the emulation's own stored P."""
    assert mutant is None or mutant in SOFTMAX_MUTANTS
    rows, Sk = S.shape
    sc = torch.tensor(f32(scale), dtype=torch.float32)
    kp = keep.float()
    if mask is not None and mutant == "mask_other_batch":
        mask = torch.roll(mask, 1, 0)
    z = S.float() * sc + _row_mask(mask, rows, rows_per_batch, torch.float32)
    zz = z[:, :Sk - 4] if mutant == "last_group_dropped" and Sk > 4 else z
    mx = zz.max(-1, keepdim=True).values
    e = torch.exp(z - mx)
    ssum = tsum(e[:, :zz.shape[-1]])
    p = e * (1.0 / ssum)
    P = _bf(p)
    dp = dPd.float() * kp
    dot = tsum((dPd.float() if mutant == "bwd_dot_undropped" else dp) * P)
    dS = sc * P * (dp - dot)
    return dict(P=P.double(), Pd=_bf(p * kp).double(), dS=_bf(dS).double(), rowsum=ssum.squeeze(-1).double())


# ---------------------------------------------------------------- dropout_bf16

def dropout_model(x, keep, u=U_BF):
    y = x.double() * keep
    return dict(y=y), dict(y=(u + W * (1 + u)) * y.abs() + TINY)


def dropout_emulate(x, keep):
    return dict(y=_bf(x.float() * keep.float()).double())


# ---------------------------------------------------------------- the cases

class Case(collections.namedtuple("Case", "name kind d p seed tags")):
    """d: the shape parameters as a tuple of (key, value); tags: a tuple of strings."""
    __slots__ = ()

    def __getattr__(self, k):
        for kk, v in self.d:
            if kk == k:
                return v
        raise AttributeError(k)


ALL_H = (256, 512, 768, 1024, 1536, 2048, 3072, 4096)
LN_N = (1, 2, 3, 7, 8, 9, 37)
DROP_P = (0.1, 0.5)
EMB_B, EMB_S, EMB_H = (1, 3, 4, 5, 9), (1, 7, 16), (256, 512, 768, 1024)
GELU_H4, GELU_H8, GELU_N = (4, 12, 516, 1020, 1028), (8, 1024, 1032, 3072), (1, 5, 31, 33, 64, 67)
SOFTMAX_SK = (4, 64, 252, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096)
SOFTMAX_B, SOFTMAX_HEADS, SOFTMAX_SQ = 2, 3, (1, 5)
SOFTMAX_SCALE = 0.125
GRADES = A.GRADES
# the exact reducer sweeps and the grid-wrap shapes of tests/test_transformer_edges_gpu.py
COLSUM_H = (2, 8, 126, 128, 130, 504, 512, 520, 1018)
COLSUM_P = (1, 3, 63, 64, 65, 255, 256, 257, 449)
COLSUM_N = (1, 3, 37, 300)
SLAB_S, SLAB_N = (1, 2, 5), (1, 3, 4, 1001, 1024, 1028)
WRAP = dict(bdrln=(65539, 256), f32in=(32771, 256), emb=(32771, 256), softmax=(32771, 8),
            gelu8=(32768 * 256 * 8 // 1024 + 3, 1024), dropout=(65536 * 256 * 4 // 1024 + 3, 1024))
REFUSED_LN_H, REFUSED_SK = (300, 1280), (6, 4100)


def _cases():
    out, seen = [], set()

    def add(kind, name, p=0.0, hsh=None, tags=(), **d):
        if p > 0:
            name += "-p%g-%s" % (p, hsh)
        if name in seen:
            return
        seen.add(name)
        out.append(Case(name, kind, tuple(sorted(d.items())), p, SEEDS[hsh] if hsh else 0, tuple(tags)))

    def drops():
        return [(p, h) for p in DROP_P for h in ("h32", "h64")]

    for kind in ("bdrln", "f32in"):
        res = (True, False) if kind == "bdrln" else (False,)
        for H in ALL_H:
            add(kind, "%s-N37-H%d%s" % (kind, H, "-res" if res[0] else ""), N=37, H=H, res=res[0])
        for N in LN_N:
            for H in (256, 768):
                for r in res:
                    add(kind, "%s-N%d-H%d%s" % (kind, N, H, "-res" if r else ""), N=N, H=H, res=r)
        add(kind, "%s-N37-H256-cancel" % kind, N=37, H=256, res=res[0], tags=("cancel",))
        add(kind, "%s-N9-H768-cancel" % kind, N=9, H=768, res=False, tags=("cancel",))
        for p, h in drops():
            add(kind, "%s-N37-H768%s" % (kind, "-res" if res[0] else ""), p, h, N=37, H=768, res=res[0])
            add(kind, "%s-N9-H256" % kind, p, h, N=9, H=256, res=False)
    # embedding: N = B * S; the width sweep at N = 37, then the B / S / tt edges (H <= 1024: emb_bwd_aux)
    for H in ALL_H:
        add("emb", "emb-B37-S1-H%d" % H, B=37, S=1, H=H, V=50, tt="mixed", pos_rows=4)
    for B, S, H, tt in ((1, 16, 256, "mixed"), (3, 7, 512, "zeros"), (4, 16, 768, "ones"), (5, 1, 1024, "mixed"),
                        (9, 7, 256, "mixed"), (3, 16, 1024, "mixed"), (9, 1, 512, "ones"), (4, 7, 768, "zeros"),
                        (5, 16, 512, "mixed"), (1, 1, 256, "ones")):
        add("emb", "emb-B%d-S%d-H%d-%s" % (B, S, H, tt), B=B, S=S, H=H, V=11, tt=tt, pos_rows=S + 3)
    for p, h in drops():
        add("emb", "emb-B5-S7-H256-mixed", p, h, B=5, S=7, H=256, V=11, tt="mixed", pos_rows=10)
    # bias + GELU: every H with two N, every N with both widths
    pairs4 = ((64, 4), (67, 4), (5, 12), (33, 12), (1, 516), (31, 516), (33, 1020), (5, 1020), (67, 1028), (64, 1028))
    pairs8 = ((67, 8), (31, 8), (1, 1024), (33, 1024), (5, 1032), (64, 1032), (31, 3072), (1, 3072))
    for N, H in pairs4 + pairs8:
        add("gelu", "gelu-N%d-H%d" % (N, H), N=N, H=H)
    # softmax: B = 2, heads = 3, Sq alternating, so 6 or 30 rows
    for i, Sk in enumerate(SOFTMAX_SK):
        add("softmax", "softmax-Sk%d-Sq%d-graded" % (Sk, SOFTMAX_SQ[i % 2]), Sk=Sk, Sq=SOFTMAX_SQ[i % 2], mask="graded")
        add("softmax", "softmax-Sk%d-Sq%d-graded" % (Sk, SOFTMAX_SQ[(i + 1) % 2]), Sk=Sk, Sq=SOFTMAX_SQ[(i + 1) % 2],
            mask="graded")
    for Sk in (64, 260, 1028, 4096):
        add("softmax", "softmax-Sk%d-Sq5-full" % Sk, Sk=Sk, Sq=5, mask="full")
        add("softmax", "softmax-Sk%d-Sq5-none" % Sk, Sk=Sk, Sq=5, mask="none")
    for p, h in drops():
        add("softmax", "softmax-Sk64-Sq5-graded", p, h, Sk=64, Sq=5, mask="graded")
        add("softmax", "softmax-Sk260-Sq5-graded", p, h, Sk=260, Sq=5, mask="graded")
    for p, h in drops():
        add("dropout", "dropout-N9-H260", p, h, N=9, H=260)
        add("dropout", "dropout-N300-H1028", p, h, N=300, H=1028)
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def cases_of(*kinds):
    return [c for c in CASES if c.kind in kinds]


def case(name):
    return CASES[CASE_IDS.index(name)]


def graded_mask(B, Sk):
    """A different graded mask per batch row: GRADES[(3 k + 5 b) % 8], key 0 open, the
    last batch row padded from Sk - 5 on (Sk > 8)."""
    kk = torch.arange(Sk)[None, :]
    bb = torch.arange(B)[:, None]
    m = torch.tensor(GRADES)[(3 * kk + 5 * bb) % 8].clone()
    m[:, 0] = 0.0
    if Sk > 8:
        m[B - 1, Sk - 5:] = -10000.0
    return m


def gelu_x(N, H, g):
    """bf16 x with x + bias covering [-9, 9]: a ramp over the flat index plus noise."""
    n = N * H
    ramp = (torch.arange(n, dtype=torch.float64) + 0.5) / n * 18.0 - 9.0
    ramp = ramp[torch.randperm(n, generator=g)]
    return (ramp + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)).float().reshape(N, H).bfloat16()


@functools.lru_cache(maxsize=None)
def inputs(c):
    """The CPU inputs of a case (a dict), seeded by its place in CASES."""
    g = torch.Generator().manual_seed(7001 + CASES.index(c))
    rn = lambda *s: torch.randn(*s, generator=g)             # noqa: E731
    if c.kind in ("bdrln", "f32in"):
        N, H = c.N, c.H
        if "cancel" in c.tags:          # rows of mean 3 and standard deviation 2^-6
            xv = 3.0 + rn(N, H) * 2.0 ** -6
            inp = dict(bias=torch.zeros(H), res=None)
        else:
            xv = rn(N, H)
            inp = dict(bias=rn(H) * 0.1, res=rn(N, H).bfloat16() if c.res else None)
        inp.update(x=xv.bfloat16() if c.kind == "bdrln" else xv, gamma=1 + 0.1 * rn(H), beta=0.1 * rn(H),
                   dy=rn(N, H).bfloat16())
        if c.kind == "f32in":
            inp.pop("bias"), inp.pop("res")
        return inp
    if c.kind == "emb":
        B, S, H, V = c.B, c.S, c.H, c.V
        ids = torch.randint(0, V, (B, S), generator=g)
        flat = ids.reshape(-1)
        flat[0] = 0
        flat[-1] = V - 1
        if flat.numel() > 3:
            flat[2] = flat[1]                                  # a repeat
        tt = dict(zeros=torch.zeros(B, S, dtype=torch.int64), ones=torch.ones(B, S, dtype=torch.int64),
                  mixed=torch.randint(0, 2, (B, S), generator=g))[c.tt]
        return dict(word=rn(V, H), typ=rn(2, H) * 0.5, pos=rn(c.pos_rows, H) * 0.5, ids=ids, tt=tt, S=S,
                    gamma=1 + 0.1 * rn(H), beta=0.1 * rn(H), dy=rn(B * S, H).bfloat16())
    if c.kind == "gelu":
        return dict(x=gelu_x(c.N, c.H, g), bias=rn(c.H) * 0.02, dy=rn(c.N, c.H).bfloat16())
    if c.kind == "softmax":
        rows = SOFTMAX_B * SOFTMAX_HEADS * c.Sq
        S = ((torch.rand(rows, c.Sk, generator=g) * 2 - 1) * (30.0 / SOFTMAX_SCALE)).bfloat16()
        S[:, 0] = 30.0 / SOFTMAX_SCALE                         # both ends of the span in every row
        S[:, c.Sk - 1] = -30.0 / SOFTMAX_SCALE
        mask = None
        if c.mask != "none":
            mask = graded_mask(SOFTMAX_B, c.Sk)
            if c.mask == "full":
                mask[SOFTMAX_B - 1] = -10000.0
        return dict(S=S, mask=mask, rows_per_batch=SOFTMAX_HEADS * c.Sq, scale=SOFTMAX_SCALE,
                    dPd=rn(rows, c.Sk).bfloat16())
    if c.kind == "dropout":
        return dict(x=rn(c.N, c.H).bfloat16())
    raise ValueError(c.kind)


def case_keep(c, rows, width):
    return keep_scale(keep_bits(c.seed, c.p, rows, width), c.p)


def _ratios(emu, ref, tol, names):
    return {n: elem_ratio(emu[n], ref[n], tol[n]) for n in names}


@functools.lru_cache(maxsize=None)
def reference(c):
    """The forward model of a case with its bounds (tol), their fp32 share (tol32), the
    emulation and its worst error / bound per output.  The backward of the LN family and
    of softmax is modelled from the emulation's own forward outputs here (on the GPU:
    from the kernel's)."""
    inp = inputs(c)
    if c.kind in LN_KINDS:
        N = inp["ids"].numel() if c.kind == "emb" else c.N
        keep = case_keep(c, N, c.H)
        ref, tol = ln_fwd_model(c.kind, inp, keep)
        _, tol32 = ln_fwd_model(c.kind, inp, keep, u=0.0)
        emu = ln_fwd_emulate(c.kind, inp, c.seed, c.p)
        bkeep = keep if c.kind == "bdrln" else torch.ones_like(keep)
        hand = (inp["dy"], emu["s"].bfloat16(), emu["mean"].float(), emu["rstd"].float(), inp["gamma"])
        bref, btol = ln_bwd_model(*hand, bkeep)
        _, btol32 = ln_bwd_model(*hand, bkeep, u=0.0)
        bemu = ln_bwd_emulate(*hand, bkeep)
        ref.update(bref), tol.update(btol), tol32.update(btol32), emu.update(bemu)
        names = ("y", "s", "mean", "rstd") + LN_BWD_OUTPUTS
        return dict(ref=ref, tol=tol, tol32=tol32, emu=emu, keep=keep, hand=hand, bkeep=bkeep,
                    emu_elem=_ratios(emu, ref, tol, names))
    if c.kind == "gelu":
        ref, tol = gelu_model(inp["x"], inp["bias"], inp["dy"])
        _, tol32 = gelu_model(inp["x"], inp["bias"], inp["dy"], u=0.0)
        emu = gelu_emulate(inp["x"], inp["bias"], inp["dy"])
        return dict(ref=ref, tol=tol, tol32=tol32, emu=emu, emu_elem=_ratios(emu, ref, tol, ("y", "dx", "dbias")))
    if c.kind == "softmax":
        rows = inp["S"].shape[0]
        keep = case_keep(c, rows, c.Sk)
        ref, tol = softmax_fwd_model(inp["S"], inp["mask"], inp["rows_per_batch"], inp["scale"], keep)
        _, tol32 = softmax_fwd_model(inp["S"], inp["mask"], inp["rows_per_batch"], inp["scale"], keep, u=0.0)
        emu = softmax_emulate(inp["S"], inp["mask"], inp["rows_per_batch"], inp["scale"], keep, inp["dPd"])
        bref, btol = softmax_bwd_model(inp["dPd"], emu["P"].bfloat16(), inp["scale"], keep)
        _, btol32 = softmax_bwd_model(inp["dPd"], emu["P"].bfloat16(), inp["scale"], keep, u=0.0)
        ref.update(bref), tol.update(btol), tol32.update(btol32)
        return dict(ref=ref, tol=tol, tol32=tol32, emu=emu, keep=keep,
                    emu_elem=_ratios(emu, ref, tol, ("P", "Pd", "dS")))
    if c.kind == "dropout":
        keep = case_keep(c, c.N, c.H)
        ref, tol = dropout_model(inp["x"], keep)
        _, tol32 = dropout_model(inp["x"], keep, u=0.0)
        emu = dropout_emulate(inp["x"], keep)
        return dict(ref=ref, tol=tol, tol32=tol32, emu=emu, keep=keep, emu_elem=_ratios(emu, ref, tol, ("y",)))
    raise ValueError(c.kind)
