"""Input gradient of the stride-2 3x3 convolution on the in-tree implicit GEMM
(csrc/kernels/conv_igemm.hip, the parity-class mode): against fp32 autograd of
the same bf16 operands (odd sizes, partial and empty classes, both channel
tilings), accumulated into an existing gradient, with the BatchNorm-backward
epilogue, and through ShadowConv2d / FusedBatchNorm2d / a downsampling
Bottleneck.  Tolerances are those of tests/test_conv_igemm_gpu.py for the same
comparisons (the reduction here is at most 4 K terms against 9 K there)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _close(got, ref, tol=1e-2):
    err = (got.float() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= tol * scale + 1e-3, (err, scale)


@functools.lru_cache(maxsize=None)
def _case(N, C, H, W, K):
    """(dy, w, fp32 input gradient of conv2d(x, w, stride 2, pad 1)) -- shared, never written."""
    g = torch.Generator(device="cuda").manual_seed(17 + N + C + H * W + K)
    w = _cl((torch.randn(K, C, 3, 3, device="cuda", generator=g) * 0.05).bfloat16())
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = _cl(torch.randn(N, K, Ho, Wo, device="cuda", generator=g).bfloat16())
    xr = torch.zeros(N, C, H, W, device="cuda", requires_grad=True)
    F.conv2d(xr, w.float(), None, 2, 1).backward(dy.float())
    return dy, w, xr.grad.detach()


@pytest.mark.parametrize("N,C,H,W,K,bn", [(2, 64, 12, 10, 128, 0), (3, 64, 15, 13, 128, 0), (2, 128, 7, 7, 64, 64),
                                          (2, 128, 9, 7, 64, 128), (2, 64, 1, 3, 64, 0), (1, 64, 2, 1, 64, 0),
                                          (2, 64, 34, 16, 64, 0)])
def test_conv3x3_dx_stride2_matches_fp32(N, C, H, W, K, bn):
    """Every pixel of a NaN-filled dx is written, and equals fp32 autograd: odd
    sizes (classes of 168 / 147 / 144 / 126 rows: partial last tiles), the
    128-wide channel tile, empty classes (H or W = 1), several tiles per class."""
    from distributed_tensorflow_example_amd import _native
    from distributed_tensorflow_example_amd.ops import conv

    dy, w, ref = _case(N, C, H, W, K)
    assert _native.load().conv3x3_dx2_supported(dy, w, H, W)
    dx = _cl(torch.full((N, C, H, W), float("nan"), device="cuda", dtype=torch.bfloat16))
    _native.load().conv3x3_dx2(dy, conv._flipped(w), dx, bn=bn)
    assert not torch.isnan(dx).any()
    _close(dx, ref)
    got = conv.conv3x3_dx(dy, w, (N, C, H, W), stride=2, bn=bn)
    assert got.shape == ref.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got, dx)


def test_conv3x3_dx_stride2_accumulates_into():
    from distributed_tensorflow_example_amd.ops import conv

    N, C, H, W, K = 3, 64, 15, 13, 128
    dy, w, ref = _case(N, C, H, W, K)
    prior = _cl(torch.randn(N, C, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
                .bfloat16())
    into = prior.clone()
    out = conv.conv3x3_dx(dy, w, (N, C, H, W), into=into, stride=2)
    assert out is into
    _close(into, prior.float() + ref)


@pytest.mark.parametrize("N,C,H,W,K", [(3, 64, 15, 13, 128), (2, 128, 8, 8, 64)])
def test_conv3x3_dx_stride2_bn_backward_partials(N, C, H, W, K):
    """EPI 2 on the kernel itself: dx stored as g = dx * relu'(bn_x * scale + shift)
    and the tiles' [sum g, sum g * x_hat] rows (exactly [2, P, C], all written;
    invalid rows of a tile add nothing)."""
    from distributed_tensorflow_example_amd import _native
    from distributed_tensorflow_example_amd.ops import conv

    Cn = _native.load()
    dy, w, ref = _case(N, C, H, W, K)
    g = torch.Generator(device="cuda").manual_seed(23 + C)
    bn_x = _cl(torch.randn(N, C, H, W, device="cuda", generator=g).bfloat16())
    # scale a power of two and shift a multiple of 1/8: bn_x * scale + shift is exact
    # in fp32, fused or not, so the mask has no rounding-dependent borderline
    mean = torch.randn(C, device="cuda", generator=g) * 0.1
    invstd = torch.rand(C, device="cuda", generator=g) + 0.5
    scale = torch.tensor([0.5, 1.0, 2.0, -1.0], device="cuda").repeat(C // 4)
    shift = torch.randint(-4, 5, (C,), device="cuda", generator=g).float() / 8
    stats = torch.stack([mean, invstd, scale, shift]).contiguous()
    P = int(Cn.conv3x3_dx2_tiles(N, H, W))
    part = torch.full((2, P, C), float("nan"), device="cuda")
    dx = _cl(torch.full((N, C, H, W), float("nan"), device="cuda", dtype=torch.bfloat16))
    Cn.conv3x3_dx2(dy, conv._flipped(w), dx, part, bn_x=bn_x, bn_stats=stats)
    assert not torch.isnan(dx).any() and not torch.isnan(part).any()
    bc = lambda v: v.view(1, C, 1, 1)
    mask = (bn_x.float() * bc(scale) + bc(shift)) > 0
    _close(dx, ref * mask)
    gs = dx.float()
    torch.testing.assert_close(part[0].sum(0), gs.sum((0, 2, 3)), rtol=1e-4, atol=1e-2)
    xhat = (bn_x.float() - bc(mean)) * bc(invstd)
    torch.testing.assert_close(part[1].sum(0), (gs * xhat).sum((0, 2, 3)), rtol=1e-4, atol=1e-2)


def _spy_dx(monkeypatch, conv):
    calls = []
    orig = conv.conv3x3_dx

    def spy(*a, **kw):
        calls.append(kw.get("stride", 1))
        return orig(*a, **kw)
    monkeypatch.setattr(conv, "conv3x3_dx", spy)
    return calls


def _run_conv_s2(conv, cin, cout, x_shape):
    torch.manual_seed(0)
    m = conv.ShadowConv2d(cin, cout, 3, 2, 1, bias=False).cuda().to(memory_format=torch.channels_last)
    with torch.no_grad():
        m.weight.copy_(torch.linspace(-0.05, 0.05, m.weight.numel(), device="cuda").view_as(m.weight))
    conv.attach_shadows(m)
    n = x_shape[0] * x_shape[1] * x_shape[2] * x_shape[3]
    x = _cl(torch.linspace(-1, 1, n, device="cuda").view(x_shape).sin().bfloat16()).requires_grad_(True)
    y = m(x)
    y.float().square().sum().backward()
    return y.float(), x.grad.float(), m.weight.grad.float()


def test_shadow_conv_stride2_input_gradient_on_igemm(monkeypatch):
    """ShadowConv2d (3x3, stride 2) forced onto the in-tree kernel routes its
    input gradient to conv3x3_dx(stride=2) -- not with DTF_CONV_DX_S2 off -- and
    matches the MIOpen path of the same module."""
    from distributed_tensorflow_example_amd.ops import conv

    calls = _spy_dx(monkeypatch, conv)
    res = {}
    for mode in ("always", "never"):
        monkeypatch.setattr(conv, "_IGEMM", mode)
        calls.clear()
        res[mode] = _run_conv_s2(conv, 64, 128, (2, 64, 11, 9))
        assert calls == ([2] if mode == "always" else []), calls
    for a, b in zip(res["always"], res["never"]):
        _close(a, b, 2e-2)
    monkeypatch.setattr(conv, "_IGEMM", "always")
    monkeypatch.setattr(conv, "_DX_S2", False)
    calls.clear()
    off = _run_conv_s2(conv, 64, 128, (2, 64, 11, 9))
    assert calls == [], calls
    for a, b in zip(off, res["never"]):
        _close(a, b, 2e-2)


def _spy_take(monkeypatch, bn_mod):
    taken = []
    orig = bn_mod.BwdSlot.take

    def spy(self, dy):
        r = orig(self, dy)
        taken.append((tuple(self.x.shape), r is not None))
        return r
    monkeypatch.setattr(bn_mod.BwdSlot, "take", spy)
    return taken


def test_bn_backward_partials_from_stride2_conv(monkeypatch):
    """FusedBatchNorm2d(relu) -> ShadowConv2d(3x3, stride 2): the conv's
    input-gradient epilogue hands the BN its backward partials (taken exactly
    once); output and all gradients match the unfused path."""
    from distributed_tensorflow_example_amd.ops import bn as bn_mod
    from distributed_tensorflow_example_amd.ops import conv
    from distributed_tensorflow_example_amd.ops.bn import FusedBatchNorm2d

    monkeypatch.setattr(conv, "_IGEMM", "always")
    N, C, H, W, K = 4, 64, 15, 13, 128
    taken = _spy_take(monkeypatch, bn_mod)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(bn_mod, "_BWD_EPI", fused)
        taken.clear()
        torch.manual_seed(5)
        bn = FusedBatchNorm2d(C).cuda()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
        m = conv.ShadowConv2d(C, K, 3, 2, 1, bias=False).cuda().to(memory_format=torch.channels_last)
        conv.attach_shadows(m)
        x = _cl(torch.randn(N, C, H, W, device="cuda").bfloat16()).requires_grad_(True)
        h = bn(x, relu=True)
        assert hasattr(h, "_dtf_bn_bwd") == fused
        y = m(h)
        y.float().square().sum().backward()
        if fused:
            assert taken == [((N, C, H, W), True)], taken
        res[fused] = (y.float(), x.grad.float(), bn.weight.grad.float(), bn.bias.grad.float(), m.weight.grad.float())
    for a, b in zip(res[True], res[False]):
        _close(a, b, 1.5e-2)


def test_downsampling_bottleneck_on_igemm_matches_unfused(monkeypatch):
    """A downsampling bottleneck (models/resnet.py, stride on the 3x3) with every
    conv on the implicit GEMM: bn1 takes its backward partials from conv2's
    stride-2 input gradient (bn2 from conv3's).  Output, input gradient and
    every parameter gradient match the unfused path."""
    from distributed_tensorflow_example_amd.models.resnet import Bottleneck
    from distributed_tensorflow_example_amd.ops import bn as bn_mod
    from distributed_tensorflow_example_amd.ops import conv

    monkeypatch.setattr(conv, "_IGEMM", "always")
    N, H = 4, 8
    ch = {}
    for key in (((N, 128, H, H), 64), ((N, 64, H // 2, H // 2), 256)):   # conv1, conv3
        for role in ("fwd", "dx", "dw"):
            ch[(role,) + key] = "igemm"
    monkeypatch.setattr(conv, "_choice", ch)
    taken = _spy_take(monkeypatch, bn_mod)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(bn_mod, "_BWD_EPI", fused)
        taken.clear()
        torch.manual_seed(9)
        net = Bottleneck(128, 64, stride=2, down=True).cuda().to(memory_format=torch.channels_last)
        for m in net.modules():
            if isinstance(m, bn_mod.FusedBatchNorm2d):
                with torch.no_grad():
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-0.2, 0.2)
        conv.attach_shadows(net)
        x = _cl(torch.randn(N, 128, H, H, device="cuda").bfloat16()).requires_grad_(True)
        y = net(x)
        (y.float() * torch.linspace(-1, 1, H // 2, device="cuda")).square().sum().backward()
        if fused:
            assert ((N, 64, H, H), True) in taken, taken        # bn1, through conv2's stride-2 input gradient
        res[fused] = [y.float(), x.grad.float()] + [p.grad.float().clone() for p in net.parameters()]
    for a, b in zip(res[True], res[False]):
        _close(a, b, 1.5e-2)


def test_conv3x3_dx_rejects_unsupported_stride2(monkeypatch):
    from distributed_tensorflow_example_amd import _native
    from distributed_tensorflow_example_amd.ops import conv

    dy = _cl(torch.zeros(2, 64, 4, 4, device="cuda", dtype=torch.bfloat16))
    w1 = _cl(torch.zeros(64, 64, 1, 1, device="cuda", dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        conv.conv3x3_dx(dy, w1, (2, 64, 8, 8), stride=2)
    w32 = _cl(torch.zeros(64, 32, 3, 3, device="cuda", dtype=torch.bfloat16))
    assert not _native.load().conv3x3_dx2_supported(dy, w32, 8, 8)
    # 32 input channels: ShadowConv2d stays on MIOpen whatever the policy
    calls = _spy_dx(monkeypatch, conv)
    res = {}
    for mode in ("always", "never"):
        monkeypatch.setattr(conv, "_IGEMM", mode)
        res[mode] = _run_conv_s2(conv, 32, 64, (2, 32, 8, 8))
    assert calls == [], calls
    for a, b in zip(res["always"], res["never"]):
        _close(a, b, 2e-2)
