"""GPU: the kernels the shipped Flappy configs run, at the layer shapes those configs give them (tests/test_flappy_shapes_cpu.py
derives the shapes and pins every gate's answer): conv 2 (32, 29, 19) -> 64 @ 13 x 8 with a stride that leaves the last input
row and column uncovered, conv 3 (64, 13, 8) -> 64 @ 11 x 6, the DQN config's 32-filter conv 2 (32, 11, 7) -> 32 @ 9 x 5, the
acting LSTM step at K = 4224 + 16 + 512 and the projection's weight gradient 2048 x 4224 over 704 / 640 rows.

Every comparison is against float64 of the same operation (rltime/models/torch/modules/cnn.py:47-49, modules/lstm.py:60-116), and
every bound is the one the kernel's own test file holds it to at the Atari geometry — imported from there or restated word for
word, none is new: tests/test_conv3_gpu.py, test_conv_wrw_gpu.py, test_conv_mid_gpu.py, test_actnet_exact_gpu.py (with
tests/actnet_conv_driver.py) and test_gemm3_gpu.py.  Work thresholds are off throughout (min_work = 0, or the module floor
monkeypatched to 0): the gates decide."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import actnet_conv_driver as CD
from tests import pointwise_restate as R
from tests.test_flappy_shapes_cpu import DQN_CONV2, IQN_CONV2, IQN_CONV3, IQN_CONV3_OUT, LSTM_H, LSTM_K, PROJ_TN

pytestmark = pytest.mark.gpu


def _profiled(fn):
    from rltime_amd import _lib
    torch.cuda.synchronize()
    _lib.check(_lib.lib.mirl_profile_reset())
    _lib.check(_lib.lib.mirl_profile_set(2))
    try:
        out = fn()
        torch.cuda.synchronize()
        ran = {r["name"]: r["calls"] for r in _lib.profile_table()}
    finally:
        _lib.check(_lib.lib.mirl_profile_set(0))
    return out, ran


def _an_f32_result(got, want, lib, what):
    """tests/test_conv3_gpu.py test_real_operands_are_an_f32_convolution's bound (the same expression in test_conv_wrw_gpu.py and
    test_conv_mid_gpu.py's layer-3 test): errors as a fraction of the largest element; no further from float64 than twice the
    library's f32 evaluation on the same inputs or 2e-6, and within 1e-5."""
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max()) / scale
    err_lib = float((lib.double() - want).abs().max()) / scale
    print("%s: err %.3e of the largest element, library f32 %.3e" % (what, err, err_lib))
    assert err <= max(2.0 * err_lib, 2e-6), (what, err, err_lib)
    assert err <= 1e-5, (what, err)


# ---- forward of the middle conv layers (csrc/conv3.hip) ------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 37])
@pytest.mark.parametrize("c,h,w,f,k,s", [IQN_CONV2, IQN_CONV3, DQN_CONV2], ids=["iqn-conv2", "iqn-conv3", "dqn-conv2"])
def test_conv3_fwd_at_the_flappy_layers(c, h, w, f, k, s, n):
    """Small-integer operands bit-equal to float64 with and without bias + ReLU; real operands an f32 convolution.  At 29 x 19 the
    stride never reaches input row 28 and column 18: NaN there must not reach the output."""
    from rltime_amd.models.torch import fused
    from tests.test_conv3_gpu import _operands
    gen = torch.Generator(device="cuda").manual_seed(n * 13 + c + k + h)
    for integer in (True, False):
        x, wt, b = _operands(n, c, h, w, f, k, gen, integer)
        assert fused.conv3_supported(x, wt, (s, s), min_work=0)
        want = F.relu(F.conv2d(x.double(), wt.double(), b.double(), s))
        got = fused.conv3_bias_relu(x, wt, b, (s, s))
        assert got.shape == want.shape == (n, f, (h - k) // s + 1, (w - k) // s + 1) and got.is_contiguous(memory_format=torch.channels_last)
        if integer:
            assert torch.equal(got.double(), want)
            got2 = fused.conv3_bias_relu(x, wt.contiguous(), None, (s, s), relu=False)          # NCHW weights, repacked by the wrapper
            assert torch.equal(got2.double(), F.conv2d(x.double(), wt.double(), None, s))
        else:
            _an_f32_result(got, want, F.relu(F.conv2d(x, wt, b, s)), "k_conv3_fwd %s n=%d" % ((c, h, w, f, k, s), n))
        if (h - k) % s or (w - k) % s:
            assert (h - k) % s == 1 and (w - k) % s == 1
            dirty = x.clone()
            dirty[:, :, h - 1, :] = float("nan")
            dirty[:, :, :, w - 1] = float("nan")
            assert dirty.is_contiguous(memory_format=torch.channels_last) and int(torch.isnan(dirty).sum()) == n * c * (h + w - 1)
            again = fused.conv3_bias_relu(dirty, wt, b, (s, s))
            assert bool(torch.isfinite(again).all()) and torch.equal(again, got)


# ---- weight gradient of conv 3 (csrc/conv_wrw.hip) -----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 5, 9])
def test_conv_wrw_b3_at_the_flappy_conv3(n):
    from rltime_amd.models.torch import fused
    from tests.test_conv_wrw_gpu import _cl, _want
    c, h, w, f, k, s = IQN_CONV3
    oh, ow = IQN_CONV3_OUT
    gen = torch.Generator(device="cuda").manual_seed(5 * n + c + h)
    wt = _cl(torch.empty(f, c, k, k, device="cuda"))
    x = _cl(torch.randint(-8, 9, (n, c, h, w), device="cuda", generator=gen).float())
    g = _cl(torch.randint(-3, 4, (n, f, oh, ow), device="cuda", generator=gen).float())
    assert fused.conv_wrw_supported(x, wt, (s, s), g, min_work=0)
    dw = fused.conv_wgrad_b3(g, x, wt, (s, s))
    assert dw.shape == wt.shape and dw.stride() == wt.stride()
    assert torch.equal(dw.double(), _want(g, x, wt, s))
    x = _cl(torch.randn(n, c, h, w, device="cuda", generator=gen))
    g = _cl(torch.randn(n, f, oh, ow, device="cuda", generator=gen) * (torch.rand(n, f, oh, ow, device="cuda", generator=gen) < 0.5))
    lib = torch.ops.aten.convolution_backward(g, x, wt, None, [s, s], [0, 0], [1, 1], False, [0, 0], 1, [False, True, False])[1]
    dw = fused.conv_wgrad_b3(g, x, wt, (s, s))
    _an_f32_result(dw, _want(g, x, wt, s), lib, "k_conv_wrw_b3 13x8 n=%d" % n)
    assert torch.equal(dw, fused.conv_wgrad_b3(g, x, wt, (s, s)))          # fixed partition, fixed order


# ---- data gradient of conv 3 (csrc/conv_mid.hip) -------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 37])
def test_conv3_bwd_data_at_the_flappy_conv3(n):
    from rltime_amd._lib import lib
    from tests.test_conv_mid_gpu import _call3, _reference3
    oh, ow = IQN_CONV3_OUT
    assert lib.mirl_conv3_bwd_data_supported(64, 64, 3, 1, oh + 2, ow + 2, oh, ow) == 1 and (oh + 2, ow + 2) == IQN_CONV3[1:3]
    gen = torch.Generator(device="cuda").manual_seed(n * 17 + oh)
    g = torch.randint(-3, 4, (n, 64, oh, ow), device="cuda", generator=gen).float().contiguous(memory_format=torch.channels_last)
    w = torch.randint(-2, 3, (64, 64, 3, 3), device="cuda", generator=gen).float()
    want = _reference3(g, w).float()
    got = _call3(g, w)
    assert got.is_contiguous(memory_format=torch.channels_last) and torch.equal(got, want)
    assert torch.equal(_call3(g, w.contiguous(memory_format=torch.channels_last)), want)
    g = torch.randn(n, 64, oh, ow, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(64, 64, 3, 3, device="cuda", generator=gen) * 0.05).contiguous(memory_format=torch.channels_last)
    got = _call3(g, w)
    x = torch.empty(n, 64, oh + 2, ow + 2, device="cuda").contiguous(memory_format=torch.channels_last)
    lib_dx = torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [True, False, False])[0]
    _an_f32_result(got, _reference3(g, w), lib_dx, "k_conv3_bwd_data_b3 11x6 n=%d" % n)
    assert torch.equal(got, _call3(g, w))


# ---- the acting conv kernels (csrc/actnet.hip) ---------------------------------------------------------------------------------

@pytest.mark.parametrize("frames", [1, 4, 32, 256])
@pytest.mark.parametrize("layer,Hi,Wi", [(2,) + IQN_CONV2[1:3], (3,) + IQN_CONV3[1:3]], ids=["conv2-29x19", "conv3-13x8"])
def test_act_conv_at_the_flappy_layers(layer, Hi, Wi, frames):
    """tests/test_actnet_exact_gpu.py's two conv comparisons — dyadic operands bit-equal to float64, real ones inside the
    operation-count bound — through the same driver (NaN-filled output, 64 floats of padding behind every frame's pixels, a guard
    frame on either side).  M = frames * Ho * Wo: below 6144 rows k_act_conv<RT = 1> runs, from 6144 k_act_conv_wlds (256 frames:
    26 624 and 16 896 rows); the profile table names the launch per layer, the row count decides the kernel behind it
    (mirl_act_conv_fwd)."""
    from tests.test_actnet_exact_gpu import _conv_out
    Ho, Wo = _conv_out(layer, Hi, Wi)
    M = frames * Ho * Wo
    assert (Ho, Wo) == ((13, 8) if layer == 2 else (11, 6)) and (M >= 6144) == (frames == 256)
    name, other = ("k_act_conv2", "k_act_conv3") if layer == 2 else ("k_act_conv3", "k_act_conv2")
    (bad, zeros, neg, n), ran = _profiled(lambda: CD.dyadic_mismatches(layer, frames, Hi, Wi, 4600 + 7 * frames + Hi))
    assert ran.get(name) == 1 and not ran.get(other), ran
    assert zeros >= 1 and neg >= 1 and (M < 64 or zeros >= n // 200), "the bias plants no visible share of zeros"
    assert bad == 0, "%d of %d outputs differ from float64 (or are -0)" % (bad, n)
    ratio, ran = _profiled(lambda: CD.real_ratio(layer, frames, Hi, Wi, 4700 + frames))
    assert ran.get(name) == 1 and not ran.get(other), ran
    print("RATIO k_act_conv%s layer %d %dx%d, %d frames: worst err / bound = %.3f" % ("_wlds" if M >= 6144 else "<RT=1>", layer, Hi, Wi,
                                                                                        frames, ratio))
    assert ratio <= 1.0


# ---- the acting LSTM step (csrc/actnet.hip) ------------------------------------------------------------------------------------

@pytest.mark.parametrize("pad", [0, 16])
@pytest.mark.parametrize("E", [4, 32])
def test_act_lstm_at_the_flappy_row(E, pad):
    """H = 512, K = 4752: 297 K steps in 4 slices of 75, the last holding 72 (RT = 1 at 4 envs, RT = 2 at 32).  xh rows K and K + 16
    floats apart.  Dyadic products: h and c inside the cell's own bound with no slack for the product; real operands inside
    test_lstm_step_real_within_the_operation_count_bound's bound.  Three launches over one workspace are bit-identical: the
    arrival counters are back at zero."""
    import numpy as np
    from tests.test_actnet_exact_gpu import U, _lstm_check, _lstm_run, _lstm_slices
    H, K = LSTM_H, LSTM_K
    KB, SPB, kb0 = _lstm_slices(H, K)
    assert (KB, SPB, kb0) == (4, 75, 4) and (KB - 1) * SPB < K // 16 < KB * SPB
    d = R.dyadic_lstm(5200 + E + pad, E, H, K)
    assert d["margin"] < 2 ** 24
    pre = R.linear(d["xh"], d["w"], d["b"])
    assert torch.equal(pre.float().double(), pre)
    _lstm_check("k_act_lstm K=4752 dyadic", _lstm_run(d["xh"], d["w"], d["b"], d["c_in"], pad=pad), pre, torch.zeros_like(pre), d["c_in"])
    g = torch.Generator().manual_seed(5300 + E + pad)
    xh = (torch.randn(E, K, generator=g) * 0.3).double()
    w = (torch.randn(4 * H, K, generator=g) / np.sqrt(K)).double()
    b = (torch.randn(4 * H, generator=g) * 0.1).double()
    c_in = (torch.randn(E, H, generator=g) * 0.5).double()
    pre = R.linear(xh, w, b)
    chain = 16 * -(-SPB // 8) + 8 + KB + 1
    e_pre = chain * U * R.linear(xh.abs(), w.abs(), b.abs())
    _lstm_check("k_act_lstm<RT=%d> K=4752 real" % (1 if E <= 16 else 2), _lstm_run(xh, w, b, c_in, pad=pad), pre, e_pre, c_in)


# ---- the LSTM projection's weight gradient (csrc/gemm3.hip, TN) ----------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", PROJ_TN)
def test_gemm3_tn_at_the_flappy_projection(M, N, K):
    """g^T x for the 2048 x 4224 frames part of the projection over 704 / 640 rows: 44 / 40 K steps in 8 chunks of 6 (the last
    holding 2) / of 5.  Integer operands bit-exact; real operands by test_real_operands_are_an_f32_gemm's bound on its operands."""
    from rltime_amd.models.torch import gemm3
    from tests.test_gemm3_gpu import _held_to_the_library, _operands, _product
    gen = torch.Generator(device="cuda").manual_seed(M * 7 + N * 3 + K)
    a, b = _operands("tn", M, N, K, gen, integer=True)
    assert gemm3.supported(gemm3.TN, a, b, min_work=0)
    want = _product("tn", a.double(), b.double())
    assert float(want.abs().max()) < 2 ** 24
    got, ran = _profiled(lambda: gemm3.gemm(gemm3.TN, a, b))
    assert ran.get("k_gemm3_tn") == 1 and ran.get("k_gemm3_reduce") == 1, ran
    assert got.shape == (M, N) and torch.equal(got.double(), want)
    a, b = _operands("tn", M, N, K, gen)
    a[::7] *= 37.0                     # rows of very different magnitude inside one tile
    b[::5] *= 0.013
    got = gemm3.gemm(gemm3.TN, a, b)
    _held_to_the_library(got, _product("tn", a.double(), b.double()), _product("tn", a, b), "tn %d x %d x %d" % (M, N, K))
    assert torch.equal(got, gemm3.gemm(gemm3.TN, a, b))


# ---- a conv layer's backward as fused.conv_bias_relu assembles it --------------------------------------------------------------

def conv_layer_backward_check(monkeypatch, cin, cout, k, s, n, h, w, ran_yes, ran_no, seed):
    """fused.conv_bias_relu on nn.Conv2d(cin, cout, k, s) in channels_last with every work threshold off, forward and backward
    under the profile table: k_conv3_fwd ran; of the backward's kernels `ran_yes` ran and `ran_no` did not (what does not run
    here is the library's).  Against float64 convolution_backward of up * (y > 0) with the kernel's own y, so that no ReLU tie
    can flip and no row is exempted: dx and dW no further from it than twice the f32 library backward of the same masked
    gradient or 2e-6, and within 1e-5 of the largest element; db bit-exact on an integer-valued upstream gradient; dx exactly 0
    on the input rows and columns the stride leaves uncovered."""
    from rltime_amd.models.torch import fused
    monkeypatch.setattr(fused, "_CONV3_MIN_WORK", 0)
    monkeypatch.setattr(fused, "_CONV_WRW_MIN_WORK", 0)
    torch.manual_seed(seed)
    conv = nn.Conv2d(cin, cout, k, s).cuda().to(memory_format=torch.channels_last)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, cin, h, w, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    oh, ow = (h - k) // s + 1, (w - k) // s + 1
    ups = {"real": torch.randn(n, cout, oh, ow, device="cuda", generator=gen),
           "integer": torch.randint(-3, 4, (n, cout, oh, ow), device="cuda", generator=gen).float()}
    stride = [s, s]
    for kind, up in ups.items():
        up = up.contiguous(memory_format=torch.channels_last)
        conv.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        y, ran = _profiled(lambda: fused.conv_bias_relu(xi, conv))
        assert ran.get("k_conv3_fwd") == 1, ran
        assert y.shape == (n, cout, oh, ow)
        _, ran = _profiled(lambda: (y * up).sum().backward())
        assert ran.get("k_relu_bwd_bias_rows") == 1, ran
        for name in ran_yes:
            assert ran.get(name) == 1, (name, ran)
        for name in ran_no:
            assert not ran.get(name), (name, ran)
        dx, dw, db = xi.grad, conv.weight.grad, conv.bias.grad
        assert dx.shape == x.shape and dw.shape == conv.weight.shape and dw.stride() == conv.weight.stride()
        yd, wd = y.detach(), conv.weight.detach()
        kept = (yd > 0)
        assert 0.2 < float(kept.float().mean()) < 0.8
        g = up * kept
        want_dx, want_dw, _ = torch.ops.aten.convolution_backward(g.double(), x.double(), wd.double(), None, stride, [0, 0], [1, 1], False, [0, 0],
                                                                  1, [True, True, False])
        lib_dx, lib_dw, _ = torch.ops.aten.convolution_backward(g, x, wd, None, stride, [0, 0], [1, 1], False, [0, 0], 1, [True, True, False])
        what = "conv_bias_relu backward (%d -> %d, k %d, s %d) %d x %d x %d, %s up" % (cin, cout, k, s, n, h, w, kind)
        _an_f32_result(dx, want_dx, lib_dx, what + ": dx")
        _an_f32_result(dw, want_dw, lib_dw, what + ": dW")
        want_db = (up.double() * kept).sum((0, 2, 3))
        if kind == "integer":
            assert torch.equal(db.double(), want_db), what
        else:
            assert float((db.double() - want_db).abs().max()) <= 1e-5 * max(float(want_db.abs().max()), 1.0), what
        rows, cols = (oh - 1) * s + k, (ow - 1) * s + k                    # what the stride covers
        assert bool((dx[:, :, rows:, :] == 0).all()) and bool((dx[:, :, :, cols:] == 0).all()), what
        assert float(dx[:, :, :rows, :cols].abs().max()) > 0


@pytest.mark.parametrize("n", [3, 37])
def test_conv2_backward_is_the_hip_forward_the_mask_pass_and_the_library(n, monkeypatch):
    """Conv 2 of flappy_iqn_lstm at (n, 32, 29, 19): neither k_conv_wrw_b3 (one frame's fill is past its budget) nor
    k_conv2_bwd_data_b3 (the stride leaves row 28 and column 18 uncovered) takes the shape; dx must be exactly 0 there."""
    c, h, w, f, k, s = IQN_CONV2
    conv_layer_backward_check(monkeypatch, c, f, k, s, n, h, w, ran_yes=(),
                              ran_no=("k_conv_wrw_b3", "k_conv2_bwd_data_b3", "k_conv2_bwd_data", "k_conv3_bwd_data_b3"), seed=40 + n)


@pytest.mark.parametrize("n", [3, 37])
def test_conv3_backward_is_all_hip(n, monkeypatch):
    c, h, w, f, k, s = IQN_CONV3
    conv_layer_backward_check(monkeypatch, c, f, k, s, n, h, w, ran_yes=("k_conv_wrw_b3", "k_conv_wrw_reduce", "k_conv3_bwd_data_b3"),
                              ran_no=("k_conv2_bwd_data_b3", "k_conv2_bwd_data"), seed=50 + n)
