"""GPU: every split-bf16 entry point on operands that populate all three bf16 parts of both operands (tests/split3_probe.py),
bit for bit against float64.  The older bit-exact tests use integers that fit one bf16 part: their mid and lo planes are
all zero, five of the six MFMAs multiply zeros, and a mid / lo plane written or read at a wrong row, k group or plane, a
part paired with the wrong partner, a missing small product or a stale value in the split are invisible to them.  Here
the six-product method is exact in f32 in any summation order and every output depends on every one of the six products
(proved on the CPU by tests/test_split3_probe_cpu.py for exactly these operands), so any such error changes the result.

Non-finite inputs (csrc/gemm3.hip's header: not preserved): one inf / NaN in the last row of a ragged tile — the row the
clamped tail loads re-read into the padding rows — must make that output row non-finite and leave every other output
bit-equal."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import split3_probe as sp

pytestmark = pytest.mark.gpu

LAYOUTS = {"nt": 0, "nn": 1, "tn": 2}


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _pitched(t, pad):
    """the same values as a column-slice view of a wider tensor (row pitch = columns + pad), NaN in the padding"""
    if not pad:
        return t.cuda().contiguous()
    full = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device="cuda")
    full[:, :t.shape[1]] = t.cuda()
    return full[:, :t.shape[1]]


def _stored(lay, a, b, pad_a=0, pad_b=0):
    """a (M, K), b (K, N) as the layout stores them"""
    A = a if lay != "tn" else a.t()
    B = b.t() if lay == "nt" else b
    return _pitched(A, pad_a), _pitched(B, pad_b)


def _profiled(fn):
    from rltime_amd import _lib
    _lib.check(_lib.lib.mirl_profile_reset())
    _lib.check(_lib.lib.mirl_profile_set(2))
    try:
        out = fn()
        torch.cuda.synchronize()
        ran = {r["name"]: r["calls"] for r in _lib.profile_table()}
    finally:
        _lib.check(_lib.lib.mirl_profile_set(0))
    return out, ran


@pytest.mark.parametrize("name", list(sp.GEMM_CASES))
def test_gemm3_probe_operands_are_bit_exact(name):
    from rltime_amd import _lib
    from rltime_amd.models.torch import gemm3
    c = sp.gemm_case(name)
    lay, opt = c["lay"], c["opt"]
    A, B = _stored(lay, c["a"], c["b"], opt.get("pad_a", 0), opt.get("pad_b", 0))
    assert gemm3.supported(LAYOUTS[lay], A, B, min_work=0)
    bias = c["bias"].cuda() if c["bias"] is not None else None
    want = c["a"].cuda().double() @ c["b"].cuda().double()
    if bias is not None:
        want = torch.relu(want + bias.double())
    M, N = want.shape
    out, pad = None, opt.get("ldc_pad", 0)
    if pad:
        wide = torch.full((M, N + pad), float("nan"), device="cuda")
        out = wide[:, pad:]
    # the 256 x 256 tile unless the case asks for the 256 x 128 one; the launch table says which ran
    _lib.check(_lib.lib.mirl_gemm3_mid_set(1 if opt.get("mid") else 0))
    try:
        got, ran = _profiled(lambda: gemm3.gemm(LAYOUTS[lay], A, B, bias, relu=bias is not None, out=out))
    finally:
        _lib.check(_lib.lib.mirl_gemm3_mid_set(-1))
    kernel = "k_gemm3_nt_mid" if opt.get("mid") else "k_gemm3_" + lay
    assert ran.get(kernel) == 1 and sum(v for k, v in ran.items() if k.startswith("k_gemm3_") and k != "k_gemm3_reduce") == 1, ran
    assert bool(torch.isfinite(got).all())
    bad = (got.double() != want).nonzero()
    assert torch.equal(got.double(), want), (len(bad), bad[:8].tolist())
    if pad:
        assert bool(torch.isnan(wide[:, :pad]).all())


@pytest.mark.parametrize("name", list(sp.NT_MUL_CASES))
def test_quantile_product_probe_operands_are_bit_exact(name, monkeypatch):
    from rltime_amd.models.torch import gemm3
    monkeypatch.setattr(gemm3, "_MIN_WORK", 0)
    c = sp.nt_mul_case(name)
    phi, w, bias, x, n = c["phi"].cuda(), c["w"].cuda(), c["bias"].cuda(), c["x"].cuda(), c["n"]
    assert gemm3.quantile_product_supported(x, phi, w, bias, n)
    emb64 = torch.relu(phi.double() @ w.double().t() + bias.double())
    want = emb64 * x.double().repeat_interleave(n, dim=0)
    (out, emb), ran = _profiled(lambda: gemm3.quantile_product(x, phi, w, bias, n, True))
    assert ran.get("k_gemm3_nt_mul") == 1, ran
    assert torch.equal(emb.double(), emb64) and torch.equal(out.double(), want)
    out2, none = gemm3.quantile_product(x, phi, w, bias, n, False)
    assert none is None and torch.equal(out2, out)


@pytest.mark.parametrize("name", list(sp.NT_HEAD_CASES))
def test_following_layer_probe_operands_are_bit_exact(name, monkeypatch):
    from rltime_amd.models.torch import gemm3
    monkeypatch.setattr(gemm3, "_MIN_WORK", 0)
    c = {k: v.cuda() for k, v in sp.nt_head_case(name).items()}
    assert gemm3.head_supported(c["x"], c["w"], c["bias"], c["w2"])
    want_h = torch.relu(c["x"].double() @ c["w"].double().t() + c["bias"].double())
    want_o = want_h @ c["w2"].double().t() + c["b2"].double()
    (hid, out), ran = _profiled(lambda: gemm3.linear_relu_head(c["x"], c["w"], c["bias"], c["w2"], c["b2"], True))
    assert ran.get("k_gemm3_nt_head") == 1, ran
    assert 0.2 < float((want_h == 0).double().mean()) < 0.8                   # the ReLU cuts
    assert torch.equal(hid.double(), want_h) and torch.equal(out.double(), want_o)
    none, out2 = gemm3.linear_relu_head(c["x"], c["w"], c["bias"], c["w2"], c["b2"], False)
    assert none is None and torch.equal(out2, out)


@pytest.mark.parametrize("name", list(sp.NN_QP_CASES))
def test_feature_product_backward_probe_operands_are_bit_exact(name, monkeypatch):
    from rltime_amd.models.torch import gemm3
    monkeypatch.setattr(gemm3, "_MIN_WORK", 0)
    c = {k: v.cuda() for k, v in sp.nn_qp_case(name).items()}
    g, w = c["g"], c["w"]
    M, K = g.shape[0], w.shape[1]
    d = g.double() @ w.double()
    # every output of the product itself: the embedding all ones, any power of two per (row group, column)
    emb, x = c["emb_dense"], c["x_dense"]
    assert gemm3.grad_input_qp_supported(g, w, emb, x, 32)
    (d_pre, _, _), ran = _profiled(lambda: gemm3.grad_input_qp(g, w, emb, x))
    assert ran.get("k_gemm3_nn_qp") == 1, ran
    assert torch.equal(d_pre.double(), d * x.double().repeat_interleave(32, dim=0))
    # the three outputs together: two live rows per column
    emb, x = c["emb_sparse"], c["x_sparse"]
    d_pre, dx, db = gemm3.grad_input_qp(g, w, emb, x)
    want_pre = (emb > 0) * d * x.double().repeat_interleave(32, dim=0)
    assert torch.equal(d_pre.double(), want_pre)
    assert torch.equal(dx.double(), (d * emb.double()).view(M // 32, 32, K).sum(1))
    assert torch.equal(db.double(), want_pre.sum(0))


@pytest.mark.parametrize("name", list(sp.CONV_FWD_CASES))
def test_conv3_forward_probe_operands_are_bit_exact(name):
    from rltime_amd.models.torch import fused
    c = sp.conv_fwd_case(name)
    x, wt, s = _cl(c["x"]), _cl(c["w"]), c["s"]
    assert fused.conv3_supported(x, wt, (s, s), min_work=0)
    got, ran = _profiled(lambda: fused.conv3_bias_relu(x, wt, None, (s, s), relu=False))
    assert ran.get("k_conv3_fwd") == 1, ran
    assert torch.equal(got.double(), F.conv2d(x.double(), wt.double(), None, s))
    # bias + ReLU: the frames unscaled, the bias an integer of each filter's unit
    c = sp.conv_fwd_case(name, scale_x=False)
    x, wt = _cl(c["x"]), _cl(c["w"])
    gen = torch.Generator().manual_seed(1)
    bias = (torch.randint(-2 ** 19 + 1, 2 ** 19, (wt.shape[0],), generator=gen).float() * c["sw"]).cuda()
    want = F.relu(F.conv2d(x.double(), wt.double(), bias.double(), s))
    assert 0.2 < float((want == 0).double().mean()) < 0.8
    assert torch.equal(fused.conv3_bias_relu(x, wt, bias, (s, s)).double(), want)


def _bwd_call(which, g, w, pipe=1):
    from rltime_amd._lib import lib, check
    n, _, oh, ow = g.shape
    floats = C.c_int64()
    so, sc, sh, sw = w.stride()
    if which == 2:
        dx = torch.full((n, 32, 2 * oh + 2, 2 * ow + 2), float("nan"), device="cuda").contiguous(memory_format=torch.channels_last)
        check(lib.mirl_conv2_bwd_data_wpk_floats(C.byref(floats)))
        wpk = torch.empty(floats.value, device="cuda")
        check(lib.mirl_conv2_bwd_data_ex(n, oh, ow, _p(g), _p(w), so, sc, sh, sw, _p(wpk), wpk.numel(), _p(dx), pipe, _stream()), "conv2_bwd_data_ex")
    else:
        dx = torch.full((n, 64, oh + 2, ow + 2), float("nan"), device="cuda").contiguous(memory_format=torch.channels_last)
        check(lib.mirl_conv3_bwd_data_wpk_floats(C.byref(floats)))
        wpk = torch.empty(floats.value, device="cuda")
        check(lib.mirl_conv3_bwd_data(n, oh, ow, _p(g), _p(w), so, sc, sh, sw, _p(wpk), wpk.numel(), _p(dx), _stream()), "conv3_bwd_data")
    return dx


@pytest.mark.parametrize("name", list(sp.CONV_BWD_CASES))
def test_conv_data_gradient_probe_operands_are_bit_exact(name):
    c = sp.conv_bwd_case(name)
    which = 2 if c["s"] == 2 else 3
    g, w = _cl(c["g"]), c["w"].cuda().contiguous()
    want = F.conv_transpose2d(g.double(), w.double(), None, c["s"])
    got, ran = _profiled(lambda: _bwd_call(which, g, w))
    assert ran.get("k_conv%d_bwd_data_b3" % which) == 1, ran
    assert got.shape == want.shape and torch.equal(got.double(), want)
    assert torch.equal(_bwd_call(which, g, _cl(w)).double(), want)


@pytest.mark.parametrize("name", list(sp.CONV_WRW_CASES))
def test_conv_weight_gradient_probe_operands_are_bit_exact(name):
    from rltime_amd.models.torch import fused
    c = sp.conv_wrw_case(name)
    g, x, k, s = _cl(c["g"]), _cl(c["x"]), c["k"], c["s"]
    wt = _cl(torch.empty(g.shape[1], x.shape[1], k, k))
    assert fused.conv_wrw_supported(x, wt, (s, s), g, min_work=0)
    want = torch.ops.aten.convolution_backward(g.double(), x.double(), wt.double(), None, [s, s], [0, 0], [1, 1], False, [0, 0], 1,
                                               [False, True, False])[1]
    dw, ran = _profiled(lambda: fused.conv_wgrad_b3(g, x, wt, (s, s)))
    assert ran.get("k_conv_wrw_b3") == 1, ran
    assert torch.equal(dw.double(), want)


def _conv1_fwd(x, w, b, flags=None):
    from rltime_amd._lib import lib, check
    n, _, h, ww = x.shape
    y = torch.full((n, 32, (h - 8) // 4 + 1, (ww - 8) // 4 + 1), float("nan"), device="cuda").contiguous(memory_format=torch.channels_last)
    wpk = torch.empty(12288, device="cuda")
    so, sc, sh, sw = w.stride()
    if flags is None:
        check(lib.mirl_conv1_u8_fwd(n, h, ww, _p(x), _p(w), so, sc, sh, sw, _p(b), 1.0, _p(wpk), _p(y), _stream()), "conv1")
    else:
        check(lib.mirl_conv1_u8_fwd_ex(n, h, ww, _p(x), _p(w), so, sc, sh, sw, _p(b), 1.0, _p(wpk), _p(y), flags, _stream()), "conv1_ex")
    return y


@pytest.mark.parametrize("name", list(sp.CONV1_FWD_CASES))
def test_input_layer_forward_probe_weights_are_bit_exact(name):
    c = sp.conv1_fwd_case(name)
    x, w, b = c["x"].cuda(), c["w"].cuda(), c["bias"].cuda()
    want = F.relu(F.conv2d(x.double(), w.double(), b.double(), 4))
    assert 0.2 < float((want == 0).double().mean()) < 0.8
    got = _conv1_fwd(x, w, b)                                          # the default: the bf16-pipe kernel
    assert torch.equal(got.double(), want)
    assert torch.equal(_conv1_fwd(x, _cl(w), b).double(), want)
    # the launch shapes of test_conv_in_gpu.py::test_launch_shapes_agree_bitwise
    for fpi in (1, 2):
        for split in (0, 1, 3, 7):
            for cached in (0, 1):
                assert torch.equal(_conv1_fwd(x, w, b, flags=cached | (fpi << 8) | (split << 16)).double(), want), (fpi, split, cached)


def _conv1_wrw(x, g, y=None):
    from rltime_amd._lib import lib, check
    need = C.c_int64()
    check(lib.mirl_conv1_u8_wrw_scratch_floats(C.byref(need)))
    scratch = torch.empty(need.value, device="cuda")
    dw = torch.full((32, 4, 8, 8), float("nan"), device="cuda").contiguous(memory_format=torch.channels_last)
    db = torch.full((32,), float("nan"), device="cuda")
    n, _, h, w = x.shape
    so, sc, sh, sw = dw.stride()
    if y is None:
        check(lib.mirl_conv1_u8_wrw(n, h, w, _p(x), _p(g), 1.0, _p(scratch), _p(dw), so, sc, sh, sw, _stream()), "conv1_wrw")
    else:
        check(lib.mirl_conv1_u8_wrw_masked(n, h, w, _p(x), _p(g), _p(y), 1.0, _p(scratch), _p(dw), so, sc, sh, sw, _p(db), _stream()),
              "conv1_wrw_masked")
    return dw, db


@pytest.mark.parametrize("name", list(sp.CONV1_WRW_CASES))
def test_input_layer_weight_gradient_probe_gradient_is_bit_exact(name):
    from rltime_amd._lib import lib, check
    c = sp.conv1_wrw_case(name)
    x, g, y = c["x"].cuda(), _cl(c["g"]), _cl(c["y"])

    def ref(gg):
        w = torch.zeros(32, 4, 8, 8, dtype=torch.float64, device="cuda", requires_grad=True)
        (F.conv2d(x.double(), w, None, 4) * gg.double()).sum().backward()
        return w.grad
    check(lib.mirl_conv1_wrw_bf16_set(1))
    try:
        (dw, _), ran = _profiled(lambda: _conv1_wrw(x, g))
        assert ran.get("k_conv1_u8_wrw_b3") == 1, ran
        assert torch.equal(dw.double(), ref(g))
        (dw, db), ran = _profiled(lambda: _conv1_wrw(x, g, y))
        assert ran.get("k_conv1_u8_wrw_b3") == 1, ran
        kept = g * (y > 0)
        assert torch.equal(dw.double(), ref(kept)) and torch.equal(db.double(), kept.double().sum((0, 2, 3)))
    finally:
        check(lib.mirl_conv1_wrw_bf16_set(-1))


# ---- non-finite inputs -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lay", ["nt", "nn", "tn"])
@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_gemm3_non_finite_value_stays_in_its_row_or_column(lay, value):
    from rltime_amd.models.torch import gemm3
    M, N, K = 300, 264, 128                                            # ragged in both directions: rows 256.., columns 256..
    a, b, _, _ = sp.gemm_operands(M, N, K, 99, scale_a=False, scale_b=False)
    A, B = _stored(lay, a, b)
    base = gemm3.gemm(LAYOUTS[lay], A, B).clone()
    assert torch.equal(base.double(), a.cuda().double() @ b.cuda().double())
    a2 = a.clone()
    a2[M - 1, 37] = value                                              # the row the clamped tail loads re-read
    A2, _ = _stored(lay, a2, b)
    got = gemm3.gemm(LAYOUTS[lay], A2, B)
    assert not bool(torch.isfinite(got[M - 1]).any()) and torch.equal(got[:M - 1], base[:M - 1])
    b2 = b.clone()
    b2[53, N - 1] = value
    _, B2 = _stored(lay, a, b2)
    got = gemm3.gemm(LAYOUTS[lay], A, B2)
    assert not bool(torch.isfinite(got[:, N - 1]).any()) and torch.equal(got[:, :N - 1], base[:, :N - 1])


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_conv3_non_finite_value_stays_in_its_windows_or_filter(value):
    from rltime_amd.models.torch import fused
    c = sp.conv_fwd_case("layer3", scale_x=False)                      # 5 x 49 = 245 positions: one ragged tile
    x, wt, s = _cl(c["x"]), _cl(c["w"]), c["s"]
    base = fused.conv3_bias_relu(x, wt, None, (s, s), relu=False).clone()
    x2 = x.clone()
    x2[-1, 5, -1, -1] = value                                          # seen by the last position only
    got = fused.conv3_bias_relu(x2, wt, None, (s, s), relu=False)
    hit = torch.zeros_like(base, dtype=torch.bool)
    hit[-1, :, -1, -1] = True
    assert not bool(torch.isfinite(got[hit]).any()) and torch.equal(got[~hit], base[~hit])
    w2 = wt.clone()
    w2[-1, 7, 1, 2] = value                                            # the last filter
    got = fused.conv3_bias_relu(x, w2, None, (s, s), relu=False)
    assert not bool(torch.isfinite(got[:, -1]).any()) and torch.equal(got[:, :-1], base[:, :-1])
