"""GPU: both gradients of the small nature CNN's second layer, Conv2d(16 -> 32, k 4, s 2), on the bf16 matrix pipe
(csrc/conv_small.hip: k_conv2s_bwd_data, k_conv2s_wrw) against aten.convolution_backward on float64 copies.  Small-integer
operands are exact in one bf16 part and every partial sum is exact in f32, so the tap / parity / octet addressing, the
uncovered rows and columns, the frame runs and the slab reduction are checked BIT-exactly; real operands to the project's
bar for split-bf16 products; reruns are bit-identical."""
import pytest
import torch

pytestmark = pytest.mark.gpu

C, F, K, S = 16, 32, 4, 2
# csrc/conv_small.hip: CS_WRW_WGS = 256 workgroups at most, each a contiguous run of ceil(N / CS_WRW_WGS) frames.  255 and 256
# frames are one frame per workgroup; 257 is the first count with runs of two (129 slabs, the last run one frame short)
WGS = 256
SHAPES = [(1, 4, 4), (3, 20, 20), (2, 5, 7), (2, 29, 19), (3, 8, 10), (WGS - 1, 20, 20), (WGS, 20, 20), (WGS + 1, 20, 20)]


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _want(g, x, wt):
    return torch.ops.aten.convolution_backward(g.double(), x.double(), wt.double(), None, [S, S], [0, 0], [1, 1], False, [0, 0], 1,
                                               [True, True, False])[:2]


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_integer_operands_are_bit_exact(n, h, w):
    from rltime_amd.models.torch import fused
    gen = torch.Generator(device="cuda").manual_seed(7 * n + h)
    oh, ow = (h - K) // S + 1, (w - K) // S + 1
    x = _cl(torch.randint(-8, 9, (n, C, h, w), device="cuda", generator=gen).float())
    g = _cl(torch.randint(-3, 4, (n, F, oh, ow), device="cuda", generator=gen).float())
    wt = _cl(torch.randint(-4, 5, (F, C, K, K), device="cuda", generator=gen).float())
    assert fused.conv2s_supported(x, wt, (S, S), g, min_frames=0)
    dx, dw = fused.conv2s_bwd_data(g, wt, x), fused.conv2s_wgrad(g, x, wt)
    want_dx, want_dw = _want(g, x, wt)
    assert dx.shape == x.shape and dx.stride() == x.stride()
    assert dw.shape == wt.shape and dw.stride() == wt.stride()
    assert torch.equal(dx.double(), want_dx)
    assert torch.equal(dw.double(), want_dw)
    # rows / columns the stride leaves uncovered
    assert not dx[:, :, 2 * oh + 2:, :].any() and not dx[:, :, :, 2 * ow + 2:].any()


@pytest.mark.parametrize("cl_weight", [False, True])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_real_operands_are_f32_gradients(n, h, w, cl_weight):
    from rltime_amd.models.torch import fused
    gen = torch.Generator(device="cuda").manual_seed(n + h + w)
    oh, ow = (h - K) // S + 1, (w - K) // S + 1
    x = _cl(torch.randn(n, C, h, w, device="cuda", generator=gen))
    g = _cl(torch.randn(n, F, oh, ow, device="cuda", generator=gen) * (torch.rand(n, F, oh, ow, device="cuda", generator=gen) < 0.5))
    wt = torch.randn(F, C, K, K, device="cuda", generator=gen)
    wt = _cl(wt) if cl_weight else wt
    want = _want(g, x, wt)
    lib = torch.ops.aten.convolution_backward(g, x, wt, None, [S, S], [0, 0], [1, 1], False, [0, 0], 1, [True, True, False])[:2]
    got = (fused.conv2s_bwd_data(g, wt, x), fused.conv2s_wgrad(g, x, wt))
    for what, a, b, ref in zip(("dx", "dw"), got, lib, want):
        scale = float(ref.abs().max())
        e = float((a.double() - ref).abs().max()) / scale
        el = float((b.double() - ref).abs().max()) / scale
        print(what, (n, h, w), "ours %.3e library %.3e" % (e, el))
        assert e <= max(2.0 * el, 2e-6), (what, e, el)
        assert e <= 1e-5, (what, e)
    again = (fused.conv2s_bwd_data(g, wt, x), fused.conv2s_wgrad(g, x, wt))          # fixed partition, fixed order
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


def _layer_backward(conv, x):
    """-> (kernel name -> calls of the backward pass, (dx, dW, db), float64 autograd's on the same ReLU mask)"""
    import torch.nn.functional as Fn
    from rltime_amd import _lib
    from rltime_amd.models.torch import fused
    y = fused.conv_bias_relu(x, conv)
    up = torch.randn_like(y)
    _lib.check(_lib.lib.mirl_profile_reset())
    _lib.check(_lib.lib.mirl_profile_set(2))
    try:
        (y * up).sum().backward()
        torch.cuda.synchronize()
        ran = {r["name"]: r["calls"] for r in _lib.profile_table()}
    finally:
        _lib.check(_lib.lib.mirl_profile_set(0))
    got = (x.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone())
    x2 = x.detach().clone().requires_grad_(True)
    pre = Fn.conv2d(x2.double(), conv.weight.double(), conv.bias.double(), conv.stride)
    want = torch.autograd.grad(pre, (x2, conv.weight, conv.bias), grad_outputs=(up * (y.detach() > 0)).double())
    return ran, got, want


def test_layer_backward_uses_them_and_matches_autograd(monkeypatch):
    """fused.conv_bias_relu's backward for Conv2d(16, 32, 4, 2): both new kernels run once and all three gradients equal
    autograd's (float64); the 32 -> 64 layer keeps the kernels it had."""
    import torch.nn as nn
    from rltime_amd.models.torch import fused
    monkeypatch.setattr(fused, "_CONV2S_MIN_FRAMES", 0)
    torch.manual_seed(13)
    n = 37
    conv = nn.Conv2d(C, F, K, S).cuda().to(memory_format=torch.channels_last)
    ran, got, want = _layer_backward(conv, _cl(torch.randn(n, C, 20, 20, device="cuda")).requires_grad_(True))
    assert ran.get("k_conv2s_bwd_data") == 1 and ran.get("k_conv2s_wrw") == 1 and ran.get("k_conv2s_wrw_reduce") == 1, ran
    assert got[1].stride() == conv.weight.stride()
    for a, b, what in zip(got, want, ("dx", "dW", "db")):
        err = float((a.double() - b.double()).abs().max()) / (float(b.abs().max()) + 1e-12)
        assert err <= (1e-4 if what == "dx" else 1e-5), (what, err)
    # the 32 -> 64 layer: its own data gradient, and its own weight gradient once that kernel's floor is lifted
    monkeypatch.setattr(fused, "_CONV_WRW_MIN_WORK", 0)
    conv2 = nn.Conv2d(32, 64, K, S).cuda().to(memory_format=torch.channels_last)
    ran, got, want = _layer_backward(conv2, _cl(torch.randn(n, 32, 20, 20, device="cuda")).requires_grad_(True))
    assert ran.get("k_conv2_bwd_data_b3") == 1 and ran.get("k_conv_wrw_b3") == 1, ran
    assert "k_conv2s_bwd_data" not in ran and "k_conv2s_wrw" not in ran, ran
    for a, b, what in zip(got, want, ("dx", "dW", "db")):
        err = float((a.double() - b.double()).abs().max()) / (float(b.abs().max()) + 1e-12)
        assert err <= (1e-4 if what == "dx" else 1e-5), (what, err)
