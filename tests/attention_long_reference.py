"""The long-sequence fused attention (csrc/kernels/attention_long.hip, S = 384 ... 2048)
against the float64 model of tests/attention_reference.py: its own cases and inputs,
the per-element bounds with the streamed forward's extra terms, and an fp32 / bf16
emulation of the streamed arithmetic with mutants.

A helper module, not a test file (`import attention_long_reference`).  The model, the
dropout hash, keep_mask and the figures are attention_reference's (R); nothing here
imports the GPU or the package.  tests/test_attention_long_reference_cpu.py checks
this module on the CPU, tests/test_attention_long_gpu.py holds the kernels to it.

What streaming changes.  The forward walks the keys in blocks with a running max m:
    alpha = exp(m_old - m),  e = exp(z - m),  l = alpha l + sum(e),
    acc = alpha acc + bf16(e keep) V,   O = acc (1 / l),   lse = m + log(l).
Against the one-pass kernel a key's weight carries, per rescale step after its block,
the rounding of m_old - m, the intrinsic's error at that argument and one product (on
l and on acc alike); O takes one more product (1 / l on the fp32 accumulator) and the
row sum has a different order with one more addition per block.  All of it is
fp32-sized.  The bounds count the steps at 32-key blocks (nblk = S / 32), which is at
least what any block size of 32, 64 or 128 keys needs: the arguments m_old - m
telescope to m_final - m(after the key's block), and a coarser block has a larger m
there.  The backward is attention.hip's and its terms follow from the new b_lse and
b_O unchanged.
"""
import collections
import functools

import numpy as np
import torch

import attention_reference as R

HD, W, U_BF, TINY, INTR, SECOND_ORDER = R.HD, R.W, R.U_BF, R.TINY, R.INTR, R.SECOND_ORDER
gamma = R.gamma
OUTPUTS, ROW_OUTPUTS = R.OUTPUTS, R.ROW_OUTPUTS
KERNEL_BLOCK = 64      # keys per streamed block in attention_long.hip (the bounds do not depend on it)
BLOCKS = (32, 64, 128)


# ---------------------------------------------------------------- bounds

def bounds(m, scale, nblk, u=U_BF):
    """R.bounds' derivation with the streamed forward's terms (module docstring).
    nblk: the number of rescale steps counted, S / 32; nblk = 0 leaves R.bounds
    itself (tests/test_attention_long_reference_cpu.py holds the two equal there)."""
    q, k, v, do, mask, keep = m["q"], m["k"], m["v"], m["dO"], m["mask"], m["keep"]
    P, Pd, z, mx = m["P"], m["Pd"], m["z"], m["mx"]
    B, NH, S, _ = q.shape
    aq, ak, av, ado = q.abs(), k.abs(), v.abs(), do.abs()
    so = SECOND_ORDER

    e_z = gamma(HD + 1) * scale * (aq @ ak.transpose(-1, -2)) + 2 * W * ((scale * m["s"]).abs() + mask.abs())
    x1 = (z - mx).abs()
    r_f = e_z + W * x1 + 2 * W * (INTR + x1)
    if nblk:
        # the rescale steps after a key's 32-key block: at most nblk - 1 - block(k) of them,
        # each W |d| (the subtraction) + 2 W (INTR + |d|) (the intrinsic) + W (the product),
        # with the |d| summing to m_final - m(after the key's block)
        blk = S // nblk
        run = torch.cummax(z.reshape(B, NH, S, nblk, blk).max(-1).values, -1).values     # m after each block
        rise = (mx - run).clamp_min(0.0)                                                  # [B, NH, S, nblk]
        steps = (nblk - 1 - torch.arange(nblk, dtype=torch.float64)).clamp_min(0.0)
        per_blk = steps * (2 * W * INTR + W) + 3 * W * rise
        r_f = r_f + per_blk.repeat_interleave(blk, -1)
    # the row sum: a lane's S / 4 terms and two shuffles, one more addition per block when streamed
    rho = (P * r_f).sum(-1, keepdim=True) + gamma(S // 4 + 2 + nblk)
    # the reciprocal (INTR ulp) and two products; streamed: e * keep before the pack, then
    # (1 / l) on the accumulator -- one more product
    f_f = so * (r_f + rho + 2 * W * INTR + 2 * W + (W if nblk else 0.0))
    EPd = Pd * (u + f_f * (1 + u)) + TINY
    E_O = (EPd + gamma(S + 1) * Pd) @ av
    b_O = u * m["O"].abs() + (1 + u) * E_O + TINY

    lsum = (m["lse"].unsqueeze(-1) - mx).abs()
    b_lse = so * (rho + 2 * W * (INTR + 1) * (1 + lsum) + W * m["lse"].unsqueeze(-1).abs())

    x2 = (z - m["lse"].unsqueeze(-1)).abs()
    r_b = so * (e_z + b_lse + W * (z.abs() + x2) + 2 * W * (INTR + x2))
    E_D = (ado * b_O).sum(-1, keepdim=True) + gamma(18) * (do * m["O"]).abs().sum(-1, keepdim=True)
    dPk = m["dP"] * keep
    D = m["D"].unsqueeze(-1)
    E_dS32 = so * ((r_b + 2 * W) * m["dS"].abs()
                   + P * (keep * gamma(HD + 1) * (ado @ av.transpose(-1, -2)) + 3 * W * (dPk.abs() + D.abs()))) + P * E_D
    E_dS = u * m["dS"].abs() + (1 + u) * E_dS32 + TINY
    t = E_dS + (gamma(S + 1) + W) * m["dS"].abs()
    E_dQ = scale * (t @ ak)
    E_dK = scale * (t.transpose(-1, -2) @ aq)
    EPdb = Pd * (u + (r_b + W) * (1 + u)) + TINY
    E_dV = (EPdb + gamma(S + 1) * Pd).transpose(-1, -2) @ ado
    out = dict(O=b_O, lse=b_lse.squeeze(-1), D=E_D.squeeze(-1))
    E = dict(dQ=E_dQ, dK=E_dK, dV=E_dV)
    for n in ("dQ", "dK", "dV"):
        out[n] = u * m[n].abs() + (1 + u) * E[n] + TINY
        out[n + "_acc"] = E[n] + TINY
    mag = torch.stack([m[n].abs().sum((0, 2)) for n in ("dQ", "dK", "dV")]).reshape(-1)
    chain = gamma(B * S) * mag + TINY
    out["dbias"] = torch.stack([E[n].sum((0, 2)) for n in ("dQ", "dK", "dV")]).reshape(-1) + chain
    out["dbias_stored"] = torch.stack([out[n].sum((0, 2)) for n in ("dQ", "dK", "dV")]).reshape(-1) + chain
    return out


# ---------------------------------------------------------------- emulation

MUTANTS = ("sum_after_dropout", "no_rescale_acc", "stale_v", "lse_first_max", "dq_skip_block", "dkv_skip_qblock",
           "D_no_dropout")
POSITIONS = ("second", "last")
MUT_B, MUT_H, MUT_ROWS = 0, 0, slice(16, 32)    # the 16 query (or key) rows a mutant touches


def _bf(x):
    return x.bfloat16().float()


def emulate(qkv, bias, mask, dO, nh, scale, keep, block=KERNEL_BLOCK, mutant=None, pos="second"):
    """The streamed arithmetic in fp32 with bf16 roundings where the kernels round: the
    operands, e * keep before the PV product, O at the store, dS and Pd~ before their
    products, dQ / dK / dV at the store; D from the stored O; P~ from the fp32 lse.
    block: keys (queries in the dK / dV pass) per streamed block.  mutant: one of
    MUTANTS, applied to rows MUT_ROWS of (MUT_B, MUT_H) at the second or the last
    block (pos).  Returns OUTPUTS as float64."""
    assert mutant is None or (mutant in MUTANTS and pos in POSITIONS)
    B, S, _ = qkv.shape
    nb = S // block
    jm = 1 if pos == "second" else nb - 1
    sel = (MUT_B, MUT_H, MUT_ROWS)
    q, k, v = R.heads(R.operands(qkv, bias), nh, 3)
    do = R.heads(dO.float(), nh, 1)[0]
    m4 = R._mask4(mask, B, S, torch.float32)
    kp = torch.ones(B, nh, S, S) if keep is None else keep.float()
    scale = float(np.float32(scale))
    z = (q @ k.transpose(-1, -2)) * scale + m4

    def forward(kpf, mut):
        mx = torch.full((B, nh, S, 1), -3.0e38)
        l = torch.zeros(B, nh, S, 1)
        acc = torch.zeros(B, nh, S, HD)
        m_first = None
        for j in range(nb):
            ks = slice(j * block, (j + 1) * block)
            zj = z[..., ks]
            mn = torch.maximum(mx, zj.max(-1, keepdim=True).values)
            alpha = torch.exp(mx - mn)
            e = torch.exp(zj - mn)
            esum = e.sum(-1, keepdim=True)
            a_acc = alpha
            vj = v[:, :, ks]
            pv = _bf(e * kpf[..., ks]) @ vj
            if mut is not None and j == jm:
                if mut == "sum_after_dropout":
                    esum = esum.clone()
                    esum[sel] = (e * kpf[..., ks]).sum(-1, keepdim=True)[sel]
                elif mut == "no_rescale_acc":
                    a_acc = alpha.clone()
                    a_acc[sel] = 1.0
                elif mut == "stale_v":
                    pv = pv.clone()
                    pv[sel] = (_bf(e * kpf[..., ks]) @ v[:, :, (j - 1) * block:j * block])[sel]
            l = alpha * l + esum
            acc = a_acc * acc + pv
            mx = mn
            if j == 0:
                m_first = mn
        ml = mx
        if mut == "lse_first_max":
            ml = mx.clone()
            ml[sel] = m_first[sel]
        return _bf(acc * (1.0 / l)), (ml + torch.log(l))

    o, lse = forward(kp, mutant)
    o_for_D = o
    if mutant == "D_no_dropout":
        o_for_D = o.clone()
        o_for_D[sel] = forward(torch.ones_like(kp), None)[0][sel]
    Pf = torch.exp(z - lse)
    D = (do * o_for_D).sum(-1, keepdim=True)
    dS = _bf(Pf * ((do @ v.transpose(-1, -2)) * kp - D))
    Pdb = _bf(Pf * kp)
    dSq = dS
    if mutant == "dq_skip_block":       # rows = queries: one key block missing from their dQ
        dSq = dS.clone()
        dSq[MUT_B, MUT_H, MUT_ROWS, jm * block:(jm + 1) * block] = 0.0
    dSk, Pdk = dS, Pdb
    if mutant == "dkv_skip_qblock":     # rows = keys: one query block missing from their dK / dV
        dSk, Pdk = dS.clone(), Pdb.clone()
        dSk[MUT_B, MUT_H, jm * block:(jm + 1) * block, MUT_ROWS] = 0.0
        Pdk[MUT_B, MUT_H, jm * block:(jm + 1) * block, MUT_ROWS] = 0.0
    dq32 = (dSq @ k) * scale
    dk32 = (dSk.transpose(-1, -2) @ q) * scale
    dv32 = Pdk.transpose(-1, -2) @ do
    dbias = torch.stack([t.sum((0, 2)) for t in (dq32, dk32, dv32)]).reshape(-1)
    out = dict(O=o, lse=lse.squeeze(-1), D=D.squeeze(-1), dQ=_bf(dq32), dK=_bf(dk32), dV=_bf(dv32), dbias=dbias)
    return {n: t.double() for n, t in out.items()}


# ---------------------------------------------------------------- the cases

Case = collections.namedtuple("Case", "name group B NH S p seed scale bias mask first_block")
SEEDS = R.SEEDS
ALL_S = (384, 512, 640, 1024)


def _cases():
    out = []

    def add(group, B, NH, S, p=0.0, hsh=None, scale=0.125, bias=True, mask=True, first_block=False):
        name = "%s-S%d-B%d-NH%d" % (group, S, B, NH)
        if p > 0:
            name += "-p%g-%s" % (p, hsh)
        if scale != 0.125:
            name += "-scale%g" % scale
        if not bias:
            name += "-nobias"
        if not mask:
            name += "-nomask"
        if first_block:
            name += "-firstblock"
        out.append(Case(name, group, B, NH, S, p, SEEDS[hsh] if hsh else 0, scale, bias, mask, first_block))

    add("A", 1, 1, 384)
    add("A", 2, 3, 384)
    add("A", 2, 3, 512)
    add("A", 2, 2, 640)           # an odd count of 128-key blocks
    add("A", 1, 2, 1024)
    add("A", 2, 3, 384, bias=False)
    add("A", 2, 3, 384, mask=False)
    add("A", 2, 3, 384, scale=0.25)
    add("A", 2, 3, 384, first_block=True)
    for S in (384, 512):
        for p in (0.1, 0.5):
            for hsh in ("h32", "h64"):
                add("B", 2, 3, S, p=p, hsh=hsh)
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def case(name):
    return CASES[CASE_IDS.index(name)]


def long_mask(B, S, first_block=False):
    """Batch element 0: a gentle ascending staircase, -0.25 ((S - 1 - k) // 32), so the
    running max rises in nearly every block while the first block still carries about
    e^-2 of the weight (a steeper one hides every early-block mutant).  The others:
    R.graded_mask, its padded tail off the 16-key tile.  first_block: keys 0 ... 127 of
    the last batch element at -10000 -- a wholly masked first block (of 32, 64 or 128
    keys), after which the max rises by 10^4."""
    m = R.graded_mask(B, S)
    m[0] = -0.25 * ((S - 1 - torch.arange(S)) // 32).float()
    if first_block:
        m[B - 1, :128] = -10000.0
    return m


@functools.lru_cache(maxsize=None)
def inputs(c):
    """qkv ~ 2 randn (bf16), bias ~ 0.5 randn (fp32), long_mask, dO ~ randn (bf16), on
    the CPU, seeded by the case's place in CASES."""
    g = torch.Generator().manual_seed(8191 + CASES.index(c))
    H3 = 3 * c.NH * HD
    qkv = (torch.randn(c.B, c.S, H3, generator=g) * 2).bfloat16()
    bias = torch.randn(H3, generator=g) * 0.5
    dO = torch.randn(c.B, c.S, c.NH * HD, generator=g).bfloat16()
    return qkv, (bias if c.bias else None), (long_mask(c.B, c.S, c.first_block) if c.mask else None), dO


def keep_of(c):
    return R.keep_mask(c.seed, c.p, c.B, c.NH, c.S) if c.p > 0 else None


@functools.lru_cache(maxsize=None)
def reference(c):
    """The model, its bounds and their fp32 share for one case, computed once; only
    [B, NH, S, 64]-sized tensors are kept.  ref, tol, tol32: dicts over OUTPUTS (tol
    also 'dbias_stored' and the '_acc' bounds of bpart_reference)."""
    qkv, bias, mask, dO = inputs(c)
    m = R.model(qkv, bias, mask, dO, c.NH, c.scale, keep_of(c))
    tol = bounds(m, c.scale, c.S // 32)
    tol32 = bounds(m, c.scale, c.S // 32, u=0.0)
    return dict(ref={n: m[n] for n in OUTPUTS}, tol=tol, tol32=tol32)


def figures(got, r):
    """Worst error / bound per output of one emulation (or kernel) result."""
    return {n: R.elem_ratio(got[n], r["ref"][n], r["tol"][n]) for n in OUTPUTS}
