"""The float64 BatchNorm model of tests/bn_reference.py against
torch.nn.functional.batch_norm (+ add + ReLU) under autograd in float64, so that
the model can be trusted before it judges a kernel (tests/test_bn_edges_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

import bn_reference as R

C = 24
EPS = 1e-5
MOM = 0.3


def _close(a, b, what):
    err = float((a - b).abs().max())
    scale = max(1.0, float(b.abs().max()))
    assert err <= 1e-12 * scale, (what, err, scale)


def _inputs(M, res, seed=0):
    g = torch.Generator().manual_seed(1000 * M + seed)
    x = torch.randn(M, C, generator=g, dtype=torch.float64) * 2 + 0.5
    r = torch.randn(M, C, generator=g, dtype=torch.float64) if res else None
    dy = torch.randn(M, C, generator=g, dtype=torch.float64)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    rm = torch.randn(C, generator=g, dtype=torch.float64)
    rv = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    return x, r, dy, gamma, beta, rm, rv


@pytest.mark.parametrize("M", [2, 3, 257])
@pytest.mark.parametrize("res,relu", [(False, True), (True, True), (False, False), (True, False)])
def test_reference_matches_autograd(M, res, relu):
    x, r, dy, gamma, beta, rm, rv = _inputs(M, res)
    xa = x.clone().requires_grad_()
    ra = r.clone().requires_grad_() if res else None
    ga, ba = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    rm_a, rv_a = rm.clone(), rv.clone()
    # batch_norm wants [N, C, *]; rows as N
    y = F.batch_norm(xa, rm_a, rv_a, ga, ba, training=True, momentum=MOM, eps=EPS)
    if res:
        y = y + ra
    if relu:
        y = F.relu(y)
    y.backward(dy)

    mean, invstd, scale, shift, pre, yr, nrm, nrv = R.fwd(x, gamma, beta, r, relu, EPS, MOM, rm, rv)
    g, dx, dres, dgamma, dbeta = R.bwd(dy, x, r, gamma, (mean, invstd, scale, shift), relu)
    _close(yr, y.detach(), "y")
    _close(dx, xa.grad, "dx")
    _close(dgamma, ga.grad, "dgamma")
    _close(dbeta, ba.grad, "dbeta")
    _close(nrm, rm_a, "running_mean")
    _close(nrv, rv_a, "running_var")
    if res:
        _close(dres, ra.grad, "dres")
    else:
        assert dres is None
    _close(mean, x.mean(0), "mean")
    _close(invstd, (x.var(0, unbiased=False) + EPS).rsqrt(), "invstd")
    if relu:
        assert torch.equal(yr, pre.clamp_min(0))
        assert torch.equal(g, dy * (pre > 0))
    else:
        assert torch.equal(yr, pre) and torch.equal(g, dy)


def test_reference_without_running_buffers():
    x, r, dy, gamma, beta, rm, rv = _inputs(3, True)
    out = R.fwd(x, gamma, beta, r, True, EPS, MOM)
    assert out[6] is None and out[7] is None
    ref = R.fwd(x, gamma, beta, r, True, EPS, MOM, rm, rv)
    for a, b in zip(out[:6], ref[:6]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("M,P", [(2, 1), (3, 2), (257, 5), (257, 64)])
def test_finalize_from_parts_agrees_with_fwd_and_bwd(M, P):
    """Exact float64 group sums over rows r % P as the partials (kept in
    float64: finalize_from_parts converts with .double(), a no-op)."""
    x, r, dy, gamma, beta, rm, rv = _inputs(M, False, seed=1)
    grp = torch.arange(M) % P
    part = torch.zeros(2, P, C, dtype=torch.float64)
    part[0].index_add_(0, grp, x)
    part[1].index_add_(0, grp, x * x)
    mean, invstd, scale, shift, pre, y, nrm, nrv = R.fwd(x, gamma, beta, None, False, EPS, MOM, rm, rv)
    fm, fi, fsc, fsh, frm, frv = R.finalize_from_parts(part, P, M, gamma, beta, EPS, MOM, rm, rv)
    # E[x^2] - mean^2 in float64 loses E[x^2] / var of the 1e-16: 1e-12 holds for these inputs
    for a, b, w in ((fm, mean, "mean"), (fi, invstd, "invstd"), (fsc, scale, "scale"), (fsh, shift, "shift"),
                    (frm, nrm, "run_mean"), (frv, nrv, "run_var")):
        _close(a, b, w)

    g, dx, _, dgamma, dbeta = R.bwd(dy, x, None, gamma, (mean, invstd, scale, shift), False)
    xhat = (x - mean) * invstd
    bpart = torch.zeros(2, P, C, dtype=torch.float64)
    bpart[0].index_add_(0, grp, g)
    bpart[1].index_add_(0, grp, g * xhat)
    dg0, db0 = torch.randn(C, dtype=torch.float64), torch.randn(C, dtype=torch.float64)
    fdg, fdb, (A, Bc, Cc) = R.finalize_from_parts_bwd(bpart, P, M, gamma, mean, invstd)
    _close(fdg, dgamma, "dgamma")
    _close(fdb, dbeta, "dbeta")
    _close(A * g + Bc * x + Cc, dx, "dx from coef")
    for a, b in zip((A, Bc, Cc), R.coef_of(gamma, mean, invstd, dgamma, dbeta, M)):
        _close(a, b, "coef")
    adg, adb, coef2 = R.finalize_from_parts_bwd(bpart, P, M, gamma, mean, invstd, dg0, db0)
    _close(adg, dg0 + dgamma, "dgamma accum")
    _close(adb, db0 + dbeta, "dbeta accum")
    for a, b in zip(coef2, (A, Bc, Cc)):
        assert torch.equal(a, b)        # the prefill does not enter the coefficients


def test_tolerance_helpers_scale_as_documented():
    """ulps() is n * 2u on the magnitudes; the statistics bound is zero-chain
    (L = 0) tight to a few u and grows linearly with L."""
    v = torch.tensor([1.0, -4.0], dtype=torch.float64)
    assert torch.allclose(R.ulps(2, v), 4 * R.U * v.abs(), rtol=0, atol=1e-30)
    assert R.chain_len(1031, 5) == 7 + 32 and R.chain_len(3, 1) == 33
    x, r, dy, gamma, beta, rm, rv = _inputs(257, False)
    mean, invstd, scale, shift, *_ = R.fwd(x, gamma, beta, None, False, EPS)
    t0 = R.tol_stats(x, gamma, beta, mean, invstd, scale, EPS, 0)
    t1 = R.tol_stats(x, gamma, beta, mean, invstd, scale, EPS, 10)
    t2 = R.tol_stats(x, gamma, beta, mean, invstd, scale, EPS, 20)
    assert float((t0["invstd"] / invstd).max()) <= 4.0001 * R.U
    assert torch.allclose(t2["var"], 2 * t1["var"])
    assert bool((t1["shift"] > t0["shift"]).all())
