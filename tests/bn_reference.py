"""Float64 model of the fused BatchNorm(+residual)(+ReLU) on [M, C] rows, and the
error bounds the bf16 / fp32 kernels of csrc/kernels/bn.hip are held to.

A helper module, not a test file: `import bn_reference` (pytest puts tests/ on
sys.path).  Everything is written from the formulas -- nothing here calls
torch.nn.BatchNorm2d or F.batch_norm; tests/test_bn_reference_cpu.py checks it
against those under autograd.  It works on whatever device its inputs are on.

Scalars the kernels receive as C floats (eps, momentum) must be given here as
the fp32-rounded value: `f32(1e-5)`.
"""
import math

import torch

U = 2.0 ** -24     # fp32 unit roundoff (round to nearest)
B = 2.0 ** -8      # bf16 unit roundoff (round to nearest, 8 significant bits)
TINY = 2.0 ** -126  # smallest normal fp32: floor of the ulp-based bounds


def f32(v):
    """The double that a C float holding v has."""
    return float(torch.tensor(v, dtype=torch.float32))


def _d(t):
    return None if t is None else t.double()


# ---------------------------------------------------------------- the operation

def _stats_tail(mean, var, gamma, beta, M, eps, momentum, run_mean, run_var):
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    new_rm = new_rv = None
    if run_mean is not None:
        unbiased = var * M / (M - 1) if M > 1 else var
        new_rm = (1.0 - momentum) * _d(run_mean) + momentum * mean
        new_rv = (1.0 - momentum) * _d(run_var) + momentum * unbiased
    return invstd, scale, shift, new_rm, new_rv


def fwd(x, gamma, beta, res=None, relu=False, eps=1e-5, momentum=0.1, run_mean=None, run_var=None):
    """Training-mode forward.  Returns mean, invstd, scale, shift, pre, y,
    new_run_mean, new_run_var (the last two None without running buffers).
    Variance is biased (two-pass, around the mean); the running variance takes
    the unbiased M / (M - 1) for M > 1.  pre is the value before the ReLU."""
    x, gamma, beta, res = _d(x), _d(gamma), _d(beta), _d(res)
    M = x.shape[0]
    mean = x.sum(0) / M
    var = ((x - mean) ** 2).sum(0) / M
    invstd, scale, shift, new_rm, new_rv = _stats_tail(mean, var, gamma, beta, M, eps, momentum, run_mean, run_var)
    pre = x * scale + shift
    if res is not None:
        pre = pre + res
    y = torch.clamp_min(pre, 0.0) if relu else pre
    return mean, invstd, scale, shift, pre, y, new_rm, new_rv


def bwd(dy, x, res, gamma, stats, relu):
    """Backward from stats = (mean, invstd, scale, shift).  Returns g, dx, dres,
    dgamma, dbeta: g = dy * [pre > 0] (dy without ReLU), dbeta = sum g,
    dgamma = sum g * x_hat, dx = gamma * invstd * (g - dbeta / M - x_hat * dgamma / M),
    dres = g when there is a residual, else None."""
    dy, x, res, gamma = _d(dy), _d(x), _d(res), _d(gamma)
    mean, invstd, scale, shift = (_d(s) for s in stats)
    M = x.shape[0]
    g = dy
    if relu:
        pre = x * scale + shift
        if res is not None:
            pre = pre + res
        g = dy * (pre > 0)
    xhat = (x - mean) * invstd
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    dx = gamma * invstd * (g - dbeta / M - xhat * dgamma / M)
    return g, dx, (g if res is not None else None), dgamma, dbeta


def _sum_parts(part, P):
    C = part.numel() // (2 * P)
    p = part.double().reshape(2, P, C)
    return p[0].sum(0), p[1].sum(0)


def finalize_from_parts(part, P, M, gamma, beta, eps=1e-5, momentum=0.1, run_mean=None, run_var=None):
    """Forward finalisation from fp32 partials [2, P, C] (sums of x and of x^2
    over P row groups), summed in float64: mean = s / M, var = max(q / M - mean^2, 0).
    Returns mean, invstd, scale, shift, new_run_mean, new_run_var."""
    s, q = _sum_parts(part, P)
    gamma, beta = _d(gamma), _d(beta)
    mean = s / M
    var = torch.clamp_min(q / M - mean * mean, 0.0)
    invstd, scale, shift, new_rm, new_rv = _stats_tail(mean, var, gamma, beta, M, eps, momentum, run_mean, run_var)
    return mean, invstd, scale, shift, new_rm, new_rv


def finalize_from_parts_bwd(part, P, M, gamma, mean, invstd, dgamma0=None, dbeta0=None):
    """Backward finalisation from fp32 partials [2, P, C] (sums of g and of
    g * x_hat), summed in float64.  Returns dgamma, dbeta, coef = (A, B, Cc) with
    dx = A * g + B * x + Cc: A = gamma * invstd, B = -A * invstd * dgamma / M,
    Cc = -A * dbeta / M - B * mean (the sums, not the accumulated outputs, enter
    the coefficients).  dgamma0 / dbeta0: what the outputs held before (accum)."""
    sg, sgx = _sum_parts(part, P)
    gamma, mean, invstd = _d(gamma), _d(mean), _d(invstd)
    A = gamma * invstd
    Bc = -A * invstd * sgx / M
    Cc = -A * sg / M - Bc * mean
    dgamma = sgx if dgamma0 is None else _d(dgamma0) + sgx
    dbeta = sg if dbeta0 is None else _d(dbeta0) + sg
    return dgamma, dbeta, (A, Bc, Cc)


# ---------------------------------------------------------------- tolerances
#
# All bounds are first-order forward error bounds of the kernels' arithmetic,
# computed from the reference's own quantities.  u = 2^-24, b = 2^-8.

def chain_len(M, P):
    """Longest fp32 summation chain behind one partial of bn_partials /
    bn_bwd_partials: a thread's rows (every 32 * P-th row), then the 32 row
    lanes summed from LDS.  Across the P partials the finalize sums in double."""
    return math.ceil(M / (32 * P)) + 32


def ulps(n, *terms):
    """n fp32 ulps of the magnitude sum |t1| + |t2| + ...: with ulp(v) <= 2u|v|.
    For a single term this is 'within n ulp of the value'.  A result formed as
    a sum of terms that may cancel (shift = beta - mean * scale, Cc, prefill +
    sum) carries the roundings of its terms, so its bound is taken on their
    magnitudes, not on the possibly much smaller result."""
    return n * 2.0 * U * sum(t.abs() for t in terms) + TINY


def tol_stats(x, gamma, beta, mean, invstd, scale, eps, L):
    """Bounds on mean, var, invstd, scale, shift from the sum bound
    |S - S_ref| <= 2 L u sum|t_i| (factor 2: the product roundings of x * x),
    propagated to first order through var = E[x^2] - mean^2 as the kernel
    forms it.  L = 0: the partials were given, only final roundings remain.
      d_mean  = 2Lu E|x| + u |mean|
      d_var   = 2Lu (E[x^2] + 2 |mean| E|x|)
      d_invstd / invstd = d_var / (var + eps) + 4u
        (the first-order factor is 1/2; the full ratio is kept as the margin
         for the higher orders, and 4u for sqrt, divide and the fp32 rounding)
      d_scale = |gamma| d_invstd + u |scale|
      d_shift = |mean| d_scale + |scale| d_mean + 2u (|beta| + |mean scale|)
    Returns a dict of per-channel tensors."""
    x, gamma, beta = _d(x), _d(gamma), _d(beta)
    M = x.shape[0]
    ex = x.abs().sum(0) / M
    ex2 = (x * x).sum(0) / M
    var = 1.0 / (invstd * invstd)      # = var + eps
    d_mean = 2 * L * U * ex + U * mean.abs() + TINY
    d_var = 2 * L * U * (ex2 + 2 * mean.abs() * ex)
    rel = d_var / var + 4 * U
    d_invstd = invstd * rel
    d_scale = gamma.abs() * d_invstd + U * scale.abs()
    d_shift = mean.abs() * d_scale + scale.abs() * d_mean + 2 * U * (beta.abs() + (mean * scale).abs()) + TINY
    return dict(mean=d_mean, var=d_var, rel_invstd=rel, invstd=d_invstd, scale=d_scale, shift=d_shift)


def tol_running(t, momentum, M, run_mean, run_var, mean, var):
    """run = (1 - m) run + m v in fp32: the statistic's error times m, plus three
    roundings (1 - m, two products, the sum) on the terms' magnitudes."""
    unb = M / (M - 1.0) if M > 1 else 1.0
    d_rm = momentum * t["mean"] + ulps(2, (1 - momentum) * _d(run_mean), momentum * mean)
    d_rv = momentum * unb * t["var"] + ulps(2, (1 - momentum) * _d(run_var), momentum * unb * var)
    return d_rm, d_rv


def e_pre(x, res, scale, shift, t):
    """Error of the kernel's fp32 pre-activation x * scale + shift (+ res):
    E_pre = |x| d_scale + d_shift + 4u (|x scale| + |shift| + |res|)."""
    x = _d(x)
    e = x.abs() * t["scale"] + t["shift"] + 4 * U * ((x * scale).abs() + shift.abs())
    if res is not None:
        e = e + 4 * U * _d(res).abs()
    return e


def tol_y(y_ref, epre):
    """|y - y_ref| <= b |y_ref| + (1 + b) E_pre: the bf16 rounding of the
    kernel's fp32 value o, b |o| <= b (|y_ref| + E_pre), plus |o - y_ref| <= E_pre
    (ReLU is 1-Lipschitz)."""
    return B * y_ref.abs() + (1 + B) * epre


def tol_bwd(g, x, gamma, mean, invstd, dgamma, dbeta, coef, t, L, M, dgamma0=None, dbeta0=None):
    """Bounds on dbeta, dgamma and the coefficients (A, B, Cc).  t: tol_stats of
    the statistics the kernel works from (its own, so their error enters x_hat
    and A); pass zeros when the kernel is handed the reference's fp32 stats.
      d_dbeta  = 2Lu sum|g| + u |dbeta|
      d_dgamma = 2Lu sum|g x_hat| + u |dgamma|
                 + sum|g| invstd d_mean + sum|g x_hat| rel_invstd
        (the kernel's x_hat = (x - mean') invstd' uses its own statistics:
         d x_hat = invstd d_mean + |x_hat| d_invstd / invstd, summed against |g|)
      with accumulation: + 2u (|prefill| + |sum|) for the fp32 add
      dA  = d_scale
      dB  = |B| (dA / |A| + rel_invstd + 4u) + |A| invstd d_dgamma / M
      dCc = dA |dbeta| / M + |A| d_dbeta / M + dB |mean| + |B| d_mean
            + 4u (|A dbeta / M| + |B mean|)
    dgamma / dbeta here are the plain sums (without the prefill)."""
    g, x, gamma = _d(g), _d(x), _d(gamma)
    A, Bc, _ = coef
    xhat = (x - mean) * invstd
    sg = g.abs().sum(0)
    sgx = (g * xhat).abs().sum(0)
    d_db = 2 * L * U * sg + U * dbeta.abs() + TINY
    d_dg = 2 * L * U * sgx + U * dgamma.abs() + sg * invstd * t["mean"] + sgx * t["rel_invstd"] + TINY
    dA = t["scale"] + U * A.abs()
    dB = Bc.abs() * (dA / A.abs().clamp_min(TINY) + t["rel_invstd"] + 4 * U) + A.abs() * invstd * d_dg / M
    dCc = (dA * dbeta.abs() / M + A.abs() * d_db / M + dB * mean.abs() + Bc.abs() * t["mean"]
           + 4 * U * ((A * dbeta / M).abs() + (Bc * mean).abs()) + TINY)
    if dbeta0 is not None:
        d_db = d_db + 2 * U * (_d(dbeta0).abs() + dbeta.abs())
        d_dg = d_dg + 2 * U * (_d(dgamma0).abs() + dgamma.abs())
    return dict(dbeta=d_db, dgamma=d_dg, A=dA, B=dB, Cc=dCc)


def zero_stats_tol(like):
    """tol_stats for statistics the kernel is handed exactly (cases where the
    reference's fp32-rounded stats are the kernel's input)."""
    z = torch.zeros_like(like)
    return dict(mean=z, var=z, rel_invstd=z, invstd=z, scale=z, shift=z)


def tol_dx(dx_ref, g, x, coef, tb):
    """|dx - dx_ref| <= b |dx_ref| + (1 + b) (|g| dA + |x| dB + dCc
                         + 4u (|A g| + |B x| + |Cc|)):
    the kernel evaluates A g + B x + Cc in fp32 (three roundings on the terms'
    magnitudes), then rounds to bf16."""
    g, x = _d(g), _d(x)
    A, Bc, Cc = coef
    e = g.abs() * tb["A"] + x.abs() * tb["B"] + tb["Cc"] + 4 * U * ((A * g).abs() + (Bc * x).abs() + Cc.abs())
    return B * dx_ref.abs() + (1 + B) * e


def coef_of(gamma, mean, invstd, dgamma, dbeta, M):
    """(A, B, Cc) of bn_bwd_finalize from the reference's sums."""
    A = _d(gamma) * invstd
    Bc = -A * invstd * dgamma / M
    return A, Bc, -A * dbeta / M - Bc * mean
