"""Float64 model of the fused multi-head self-attention of csrc/kernels/attention.hip
(forward and backward, with the kernels' dropout bits), the per-element error
bounds its outputs are held to, and an fp32 / bf16 emulation of the kernels'
arithmetic that shows on the CPU that the bounds are attainable and have power.

A helper module, not a test file: `import attention_reference` (pytest puts tests/
on sys.path).  Nothing here imports the GPU or the package;
tests/test_attention_reference_cpu.py checks the model against float64 autograd,
tests/test_attention_edges_gpu.py holds the kernels to it.

Layouts: qkv [B, S, 3 * NH * 64] bf16 is the packed projection [B, S, 3, NH, 64];
everything per head is [B, NH, S, 64], probabilities [B, NH, S(query), S(key)],
lse and D [B, NH, S], dbias [3 * NH * 64] in the order of qkv's last axis.
"""
import collections
import functools
import math

import numpy as np
import torch

U_BF = 2.0 ** -8     # bf16 unit roundoff (round to nearest even, 8 significant bits)
W = 2.0 ** -24       # fp32 unit roundoff
TINY = 2.0 ** -126   # smallest normal fp32 (= bf16): a value below it may be flushed to zero
HD = 64              # head dimension of the kernels

# Allowance for the hardware transcendentals behind __expf, __logf and a possibly
# approximate reciprocal: the project states none.  The CDNA ISA guides give
# v_exp_f32, v_log_f32 and v_rcp_f32 as accurate to 1 ulp; twice that is assumed
# here (an ulp is at most 2 W relative, so INTR * 2 * W).  __expf(x) is
# exp2(x * log2(e)): the constant and the product round once each, which moves
# the result by 2 W |x| relative, so rel(__expf(x)) <= 2 W (INTR + |x|).
INTR = 2.0
SECOND_ORDER = 1.01  # the fp32 terms are summed to first order; products of them are below 1 %


def gamma(n):
    """Error constant of an fp32 sum of n terms in any order: n W / (1 - n W)."""
    return n * W / (1.0 - n * W)


# ---------------------------------------------------------------- dropout bits

M64 = (1 << 64) - 1


def hash32(seed, i):
    """csrc/kernels/common.h hash32 on an array of element indices (uint64).
    seed: a Python int, int64 or uint64 bits alike.  Returns uint32."""
    seed = int(seed) & M64
    i = np.asarray(i).astype(np.uint64)
    with np.errstate(over="ignore"):
        if seed >> 63:      # 32-bit lowbias32 finaliser of the index xor a mixed seed
            k = np.uint32(((seed & 0xFFFFFFFF) ^ (((seed >> 32) * 0x85EBCA6B) & 0xFFFFFFFF)) & 0xFFFFFFFF)
            lo = (i & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            hi = (i >> np.uint64(32)).astype(np.uint32)
            x = (lo ^ k) + hi * np.uint32(0x9E3779B9)
            x = x ^ (x >> np.uint32(16))
            x = x * np.uint32(0x7FEB352D)
            x = x ^ (x >> np.uint32(15))
            x = x * np.uint32(0x846CA68B)
            x = x ^ (x >> np.uint32(16))
            return x
        x = np.uint64(seed) ^ (i * np.uint64(0x9E3779B97F4A7C15))      # splitmix64 finaliser
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
        return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def attn_thresh(p):
    """attention.hip attn_thresh: floor(double(float(p)) * 2^32), clamped to 2^32 - 1."""
    pf = float(np.float32(p))
    if pf <= 0.0:
        return 0
    t = pf * 4294967296.0
    return 4294967295 if t >= 4294967295.0 else int(t)


def inv_keep(p):
    """The C float 1.f / (1.f - p) of the launchers: both steps round to fp32."""
    pf = np.float32(p)
    return float(np.float32(1.0) / (np.float32(1.0) - pf)) if pf > 0 else 1.0


def keep_bits(seed, p, B, NH, S):
    """bool [B, NH, S, S]: element i = ((b * NH + h) * S + q) * S + k is kept when
    hash32(seed, i) >= thresh (thresh == 0: everything)."""
    th = attn_thresh(p)
    n = B * NH * S * S
    if th == 0:
        return torch.ones(B, NH, S, S, dtype=torch.bool)
    h = hash32(seed, np.arange(n, dtype=np.uint64))
    return torch.from_numpy(h >= np.uint32(th)).reshape(B, NH, S, S)


def keep_mask(seed, p, B, NH, S):
    """float64 [B, NH, S, S]: inv_keep where kept, else 0 (all 1 for p <= 0)."""
    bits = keep_bits(seed, p, B, NH, S).double()
    return bits * (inv_keep(p) if attn_thresh(p) else 1.0)


# ---------------------------------------------------------------- the operation

def heads(t, nh, parts):
    """[B, S, parts * nh * 64] -> parts views [B, nh, S, 64]."""
    B, S, _ = t.shape
    t = t.reshape(B, S, parts, nh, HD)
    return [t[:, :, i].permute(0, 2, 1, 3) for i in range(parts)]


def operands(qkv, bias):
    """x = bf16(fp32(qkv) + bias): an fp32 add, then round to nearest even -- the
    operand both the staged (stage_store) and the per-wave (add_bias8) path build.
    Returned as float32 holding bf16 values."""
    x = qkv.float()
    if bias is not None:
        x = (x + bias.float()).bfloat16().float()
    return x


def _mask4(mask, B, S, dtype):
    if mask is None:
        return torch.zeros(B, 1, 1, S, dtype=dtype)
    return mask.to(dtype).reshape(B, 1, 1, S)


def model(qkv, bias, mask, dO, nh, scale, keep):
    """Everything in float64.  keep: keep_mask(...) or None (no dropout).
      z = scale q k^T + mask, P = softmax(z), lse = logsumexp(z), Pd = P keep, O = Pd V
      D = rowsum(dO O), dS = P (dO V^T keep - D)
      dQ = scale dS K, dK = scale dS^T Q, dV = Pd^T dO, dbias = column sums of dqkv."""
    B, S, _ = qkv.shape
    q, k, v = (t.double() for t in heads(operands(qkv, bias), nh, 3))
    do = heads(dO.double(), nh, 1)[0]
    m4 = _mask4(mask, B, S, torch.float64)
    keep = torch.ones(B, nh, S, S, dtype=torch.float64) if keep is None else keep.double()
    s = q @ k.transpose(-1, -2)
    z = scale * s + m4
    mx = z.max(-1, keepdim=True).values
    e = torch.exp(z - mx)
    lse = mx + torch.log(e.sum(-1, keepdim=True))
    P = torch.exp(z - lse)
    Pd = P * keep
    O = Pd @ v
    D = (do * O).sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)
    dS = P * (dP * keep - D)
    dQ = scale * (dS @ k)
    dK = scale * (dS.transpose(-1, -2) @ q)
    dV = Pd.transpose(-1, -2) @ do
    dbias = torch.stack([dQ.sum((0, 2)), dK.sum((0, 2)), dV.sum((0, 2))]).reshape(-1)
    return dict(q=q, k=k, v=v, dO=do, mask=m4, keep=keep, s=s, z=z, mx=mx, P=P, Pd=Pd, dP=dP, dS=dS,
                O=O, lse=lse.squeeze(-1), D=D.squeeze(-1), dQ=dQ, dK=dK, dV=dV, dbias=dbias)


OUTPUTS = ("O", "lse", "D", "dQ", "dK", "dV", "dbias")


# ---------------------------------------------------------------- bounds
#
# First-order worst-case forward error bounds of the kernels' arithmetic, from the
# reference's own quantities.  u = 2^-8 (bf16), W = 2^-24 (fp32).  bf16 x bf16
# products are exact in fp32, so an MFMA dot product of n terms errs by at most
# gamma(n + 1) sum |a_i b_i| (n additions, one into the accumulator).

def bounds(m, scale, u=U_BF):
    """dict of per-element bounds for OUTPUTS, plus 'dbias_stored' (the column sums
    taken from the stored bf16 dqkv instead of the fp32 accumulators).  u = 0 gives
    the fp32 share of each bound (every bf16 rounding removed)."""
    q, k, v, do, mask, keep = m["q"], m["k"], m["v"], m["dO"], m["mask"], m["keep"]
    P, Pd, z, mx = m["P"], m["Pd"], m["z"], m["mx"]
    B, NH, S, _ = q.shape
    aq, ak, av, ado = q.abs(), k.abs(), v.abs(), do.abs()
    so = SECOND_ORDER

    # z = fma(s, scale, mask) or a product and a sum: the dot product's error times
    # scale, then at most two roundings on the terms' magnitudes.  (A key at -10000
    # gets an absolute error of 1e-3 here; its P is exactly 0 and it drops out.)
    e_z = gamma(HD + 1) * scale * (aq @ ak.transpose(-1, -2)) + 2 * W * ((scale * m["s"]).abs() + mask.abs())

    # forward: e = __expf(z - mx).  Any mx cancels between e and sum(e), so only the
    # rounding of the subtraction W |z - mx| and the intrinsic's error remain.
    x1 = (z - mx).abs()
    r_f = e_z + W * x1 + 2 * W * (INTR + x1)
    # sum(e): a lane adds S / 4 terms, two shuffles finish the row; all terms positive.
    rho = (P * r_f).sum(-1, keepdim=True) + gamma(S // 4 + 2)
    # Pd = e * (1 / sum) * keep: the reciprocal (INTR ulp) and two products.
    f_f = so * (r_f + rho + 2 * W * INTR + 2 * W)
    # pack to bf16 before the PV MFMA: u on the fp32 value
    EPd = Pd * (u + f_f * (1 + u)) + TINY
    # O = sum_k Pd_k v_k over S keys in the accumulator, then the bf16 store
    E_O = (EPd + gamma(S + 1) * Pd) @ av
    b_O = u * m["O"].abs() + (1 + u) * E_O + TINY

    # lse = mx + __logf(sum): d log(sum) = rho; the intrinsic is a log2 (INTR ulp of
    # its result, and a product with ln 2), floored at an absolute INTR ulp of 1
    # where log(sum) is small; one rounding of the final sum.
    lsum = (m["lse"].unsqueeze(-1) - mx).abs()
    b_lse = so * (rho + 2 * W * (INTR + 1) * (1 + lsum) + W * m["lse"].unsqueeze(-1).abs())

    # backward: P~ = __expf(z - lse) with the forward's fp32 lse
    x2 = (z - m["lse"].unsqueeze(-1)).abs()
    r_b = so * (e_z + b_lse + W * (z.abs() + x2) + 2 * W * (INTR + x2))
    # D = rowsum(dO * O^) from the bf16 O the forward stored: its error b_O against
    # |dO|, plus the fp32 sum (16 exact products per lane, two shuffles)
    E_D = (ado * b_O).sum(-1, keepdim=True) + gamma(18) * (do * m["O"]).abs().sum(-1, keepdim=True)
    # dS = P~ * (dP * keep - D): dP's dot product, three roundings, P~'s error, D's error
    dPk = m["dP"] * keep
    D = m["D"].unsqueeze(-1)
    E_dS32 = so * ((r_b + 2 * W) * m["dS"].abs()
                   + P * (keep * gamma(HD + 1) * (ado @ av.transpose(-1, -2)) + 3 * W * (dPk.abs() + D.abs()))) + P * E_D
    # pack to bf16 before the dQ / dK MFMA
    E_dS = u * m["dS"].abs() + (1 + u) * E_dS32 + TINY
    # dQ = scale * sum_k dS_k k_k (S terms, one product with scale), dK alike over queries
    t = E_dS + (gamma(S + 1) + W) * m["dS"].abs()
    E_dQ = scale * (t @ ak)
    E_dK = scale * (t.transpose(-1, -2) @ aq)
    # dV = sum_q Pd~_q dO_q with Pd~ = P~ * keep packed to bf16
    EPdb = Pd * (u + (r_b + W) * (1 + u)) + TINY
    E_dV = (EPdb + gamma(S + 1) * Pd).transpose(-1, -2) @ ado
    out = dict(O=b_O, lse=b_lse.squeeze(-1), D=E_D.squeeze(-1))
    E = dict(dQ=E_dQ, dK=E_dK, dV=E_dV)
    for n in ("dQ", "dK", "dV"):
        out[n] = u * m[n].abs() + (1 + u) * E[n] + TINY
        out[n + "_acc"] = E[n] + TINY       # the fp32 accumulator, before the bf16 store
    # dbias: the kernels add the fp32 accumulators (before the bf16 store) of a
    # column's B * S values: their errors without the store term, plus the sum's own
    # error in whatever order.  From the stored dqkv: the full element bounds.
    mag = torch.stack([m[n].abs().sum((0, 2)) for n in ("dQ", "dK", "dV")]).reshape(-1)
    chain = gamma(B * S) * mag + TINY
    out["dbias"] = torch.stack([E[n].sum((0, 2)) for n in ("dQ", "dK", "dV")]).reshape(-1) + chain
    out["dbias_stored"] = torch.stack([out[n].sum((0, 2)) for n in ("dQ", "dK", "dV")]).reshape(-1) + chain
    return out


def dbuf_reference(ctx, dO, nh):
    """Dbuf as attn_bwd_dq must write it, from the bf16 ctx it was HANDED: float64
    rowsum(dO * ctx) [B, NH, S] and its fp32 bound, gamma(18) sum |dO ctx| (the
    products are exact, a lane adds 16, two shuffles finish) -- an fp32-sized bound."""
    o = heads(ctx.double(), nh, 1)[0]
    do = heads(dO.double(), nh, 1)[0]
    return (do * o).sum(-1), gamma(18) * (do * o).abs().sum(-1) + TINY


# ---------------------------------------------------------------- emulation

def _bf(x):
    return x.bfloat16().float()


MUTANTS = ("mask_neighbour", "drop_tile", "swap_dk_slabs", "lse_off", "dropout_fwd_only", "D_no_dropout")


def neighbour_key(mask):
    """A key of batch element 0 whose mask differs from its right neighbour's, both unmasked."""
    m = mask[0]
    for k0 in range(1, m.numel() - 1):
        if m[k0] != m[k0 + 1] and m[k0] > -100 and m[k0 + 1] > -100:
            return k0
    raise ValueError("no graded neighbours")


def emulate(qkv, bias, mask, dO, nh, scale, keep, mutant=None):
    """The kernels' computation in fp32 with bf16 roundings where they round: the
    operands, Pd and dS before their MFMA, O / dQ / dK / dV at the store; D from the
    stored O; P~ recomputed from the fp32 lse.  Accumulation order and the
    transcendentals are the CPU's.  mutant: one of MUTANTS -- a deliberately wrong
    variant for tests/test_attention_reference_cpu.py.  Returns OUTPUTS as float64."""
    assert mutant is None or mutant in MUTANTS
    B, S, _ = qkv.shape
    q, k, v = heads(operands(qkv, bias), nh, 3)
    do = heads(dO.float(), nh, 1)[0]
    if mutant == "mask_neighbour":
        k0 = neighbour_key(mask)
        mask = mask.clone()
        mask[0, k0] = mask[0, k0 + 1]
    m4 = _mask4(mask, B, S, torch.float32)
    kp = torch.ones(B, nh, S, S) if keep is None else keep.float()
    scale = float(np.float32(scale))
    z = (q @ k.transpose(-1, -2)) * scale + m4
    mx = z.max(-1, keepdim=True).values
    e = torch.exp(z - mx)
    s = e.sum(-1, keepdim=True)
    if mutant == "drop_tile":
        s[0, 0, 3] -= e[0, 0, 3, 16:32].sum()
    lse = mx + torch.log(s)
    pn = e * (1.0 / s)
    o32 = _bf(pn * kp) @ v
    o = _bf(o32)
    if mutant == "lse_off":
        lse[0, 0, 3] += 1e-2
    Pf = torch.exp(z - lse)
    D = (do * (_bf(_bf(pn) @ v) if mutant == "D_no_dropout" else o)).sum(-1, keepdim=True)
    dS = _bf(Pf * ((do @ v.transpose(-1, -2)) * kp - D))
    dq32 = (dS @ k) * scale
    dk32 = (dS.transpose(-1, -2) @ q) * scale
    dv32 = _bf(Pf if mutant == "dropout_fwd_only" else Pf * kp).transpose(-1, -2) @ do
    if mutant == "swap_dk_slabs":
        dk32 = dk32.clone()
        dk32[0, 0, 0:32] = torch.cat([dk32[0, 0, 16:32], dk32[0, 0, 0:16]])
    dbias = torch.stack([t.sum((0, 2)) for t in (dq32, dk32, dv32)]).reshape(-1)
    out = dict(O=o, lse=lse.squeeze(-1), D=D.squeeze(-1), dQ=_bf(dq32), dK=_bf(dk32), dV=_bf(dv32), dbias=dbias)
    return {n: t.double() for n, t in out.items()}


# ---------------------------------------------------------------- figures

def elem_ratio(got, ref, tol):
    """Worst |got - ref| / bound over the elements; a NaN counts as infinite.  An
    element whose bound is 0 (a fully masked key's dK / dV) must be exact."""
    err = (got.double().reshape(ref.shape) - ref).abs()
    r = err / tol.clamp_min(1e-300)
    r = torch.where(err == 0, torch.zeros_like(r), r)
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def row_ratio(got, ref, tol):
    """Worst ||err||_2 / ||bound||_2 over the 64-vectors of the last axis."""
    err = (got.double().reshape(ref.shape) - ref).norm(dim=-1)
    r = err / tol.norm(dim=-1).clamp_min(1e-300)
    r = torch.where(err == 0, torch.zeros_like(r), r)
    return float(torch.nan_to_num(r, nan=float("inf")).max())


ROW_OUTPUTS = ("O", "dQ", "dK", "dV")


# ---------------------------------------------------------------- the cases

Case = collections.namedtuple("Case", "name group B NH S p seed scale bias mask")
ALL_S = (32, 64, 128, 192, 256)
SEEDS = {"h32": -(1 << 63) + 0x1234567, "h64": 0x1234567}   # bit 63 set: 32-bit hash; clear: splitmix64
GRADES = (0.0, -1.0, -2.5, 0.0, -10000.0, 0.0, -0.75, 0.0)


def _cases():
    out = []

    def add(group, B, NH, S, p=0.0, hsh=None, scale=0.125, bias=True, mask=True):
        name = "%s-S%d-B%d-NH%d" % (group, S, B, NH)
        if p > 0:
            name += "-p%g-%s" % (p, hsh)
        if scale != 0.125:
            name += "-scale%g" % scale
        if not bias:
            name += "-nobias"
        if not mask:
            name += "-nomask"
        out.append(Case(name, group, B, NH, S, p, SEEDS[hsh] if hsh else 0, scale, bias, mask))

    for S in ALL_S:
        for B, NH in ((1, 1), (2, 3)):
            add("A", B, NH, S)
    add("A", 2, 12, 128)
    for S in (64, 192):                    # one per backward path: fused, two-kernel
        add("A", 2, 3, S, scale=0.25)
        add("A", 2, 3, S, bias=False)
        add("A", 2, 3, S, mask=False)
        add("A", 2, 3, S, bias=False, mask=False)
    for S in (64, 128, 192, 256):
        for p in (0.1, 0.5):
            for hsh in ("h32", "h64"):
                add("B", 2, 3, S, p=p, hsh=hsh)
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def graded_mask(B, S):
    """Per-key values GRADES[(3 k + 5 b) % 8] (key 0 open), so neighbouring keys
    differ and batch elements are shifted against each other; the last batch
    element is padded from S - 5 on, which is no multiple of the 16-key tile."""
    kk = torch.arange(S)[None, :]
    bb = torch.arange(B)[:, None]
    m = torch.tensor(GRADES)[(3 * kk + 5 * bb) % 8].clone()
    m[:, 0] = 0.0
    m[B - 1, S - 5:] = -10000.0
    return m


@functools.lru_cache(maxsize=None)
def inputs(case):
    """qkv ~ 2 randn (bf16), bias ~ 0.5 randn (fp32), the graded mask, dO ~ randn
    (bf16), on the CPU, seeded by the case's place in CASES."""
    g = torch.Generator().manual_seed(4099 + CASES.index(case))
    H3 = 3 * case.NH * HD
    qkv = (torch.randn(case.B, case.S, H3, generator=g) * 2).bfloat16()
    bias = torch.randn(H3, generator=g) * 0.5
    dO = torch.randn(case.B, case.S, case.NH * HD, generator=g).bfloat16()
    return qkv, (bias if case.bias else None), (graded_mask(case.B, case.S) if case.mask else None), dO


@functools.lru_cache(maxsize=None)
def reference(case):
    """The model, its bounds, their fp32 share and the emulation's figures for one
    case, computed once; only [B, NH, S, 64]-sized tensors are kept.
      ref, tol, tol32: dicts over OUTPUTS (tol also 'dbias_stored')
      emu_elem / emu_rows: the emulation's worst element / row ratio per output
      cond: the figures of the case conditions."""
    qkv, bias, mask, dO = inputs(case)
    keep = keep_mask(case.seed, case.p, case.B, case.NH, case.S) if case.p > 0 else None
    m = model(qkv, bias, mask, dO, case.NH, case.scale, keep)
    tol = bounds(m, case.scale)
    tol32 = bounds(m, case.scale, u=0.0)
    emu = emulate(qkv, bias, mask, dO, case.NH, case.scale, keep)
    ref = {n: m[n] for n in OUTPUTS}
    cond = {}
    if mask is not None:
        cond["open_keys_min"] = int((mask > -100).sum(1).min())
        cond["graded_share"] = float(((mask > -10) & (mask < 0)).double().mean())
    if case.p > 0:
        bits = keep_bits(case.seed, case.p, case.B, case.NH, case.S)
        n = bits.numel()
        cond["keep_share"] = float(bits.double().mean())
        cond["keep_sigma"] = (cond["keep_share"] - (1 - float(np.float32(case.p)))) / math.sqrt(case.p * (1 - case.p) / n)
        cond["kept_per_row_min"] = int(bits.sum(-1).min())
    return dict(ref=ref, tol=tol, tol32=tol32, emu=emu, cond=cond,
                emu_elem={n: elem_ratio(emu[n], ref[n], tol[n]) for n in OUTPUTS},
                emu_rows={n: row_ratio(emu[n], ref[n], tol[n]) for n in ROW_OUTPUTS})


def bpart_reference(ref, tol):
    """The per-wave partial column sums the backward kernels write for the bias
    gradient, [B * S / 16, 3 * NH * 64]: row b * S / 16 + r holds the sums of dQ / dK /
    dV over rows 16 r ... 16 r + 15 of batch element b, taken from the fp32
    accumulators.  Returns (float64 reference, bound): the accumulators' bounds
    summed, plus a 16-term fp32 sum in the kernels' order or any other."""
    def fold(t):            # [B, NH, S, 64] -> [B, S / 16, NH, 64]
        B, NH, S, d = t.shape
        return t.reshape(B, NH, S // 16, 16, d).sum(3).permute(0, 2, 1, 3)

    def pack(ts):
        t = torch.stack(ts, 2)                                   # [B, S / 16, 3, NH, 64]
        return t.reshape(t.shape[0] * t.shape[1], -1)

    names = ("dQ", "dK", "dV")
    want = pack([fold(ref[n]) for n in names])
    bound = pack([fold(tol[n + "_acc"]) + gamma(16) * fold(ref[n].abs()) for n in names])
    return want, bound


def split_dqkv(dqkv, nh):
    """[B, S, 3 * nh * 64] -> dQ, dK, dV as [B, nh, S, 64]."""
    return heads(dqkv, nh, 3)
