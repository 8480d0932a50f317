"""GPU: the input layer from ONE-plane uint8 frames (csrc/conv_in_rows.hip) through its C entry points, against the reference's
expression for the layer, rltime/models/torch/modules/cnn.py:44-49 at Conv2d(1 -> 32, kernel 8, stride 4) — the shape of
configs/atari_iqn_lstm.json with env_wrappers/atari_lstm.json ("stack": 1).  Integer operands make every sum exact in f32 in
any order, so indexing is checked BIT-exactly against float64; the operands of tests/conv1p_probe.py do the same with all
three bf16 parts populated; real operands are held to the bars tests/test_conv_in_gpu.py holds the 4-plane family to."""
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import conv1p_probe as cp

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
# (1, 120, 80), (5, 120, 80): configs/flappy_iqn_lstm.json's frames, 29 x 19 = 551 positions = 34 tiles of 16 and 7 more; five
# frames are one four-frame fill of the weight gradient and a tail
FLAPPY = [(1, 120, 80), (5, 120, 80)]
SHAPES = [(1, 84, 84), (2, 84, 84), (33, 84, 84), (1025, 84, 84), (7, 36, 36), (5, 44, 52), (4, 12, 16), (6, 8, 8), (2, 100, 100)] + FLAPPY


def _p(t):
    return C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need(query):
    from rltime_amd._lib import lib, check
    need = C.c_int64()
    check(getattr(lib, query)(C.byref(need)))
    return need.value


def _layouts(w):
    """the (32, 1, 8, 8) tensor in contiguous memory, in channels_last memory and with kernel rows and columns swapped in memory"""
    w = w.contiguous()
    cl = torch.empty_strided((32, 1, 8, 8), (64, 1, 8, 1), device=w.device).copy_(w)
    tr = w.transpose(2, 3).contiguous().transpose(2, 3)
    assert cl.is_contiguous(memory_format=torch.channels_last) and tr.stride() == (64, 64, 1, 8)
    return w, cl, tr


def _fwd(x, w, b, scale, flags=0, wpk=None):
    from rltime_amd._lib import lib, check
    n, _, h, ww = x.shape
    oh, ow = (h - 8) // 4 + 1, (ww - 8) // 4 + 1
    y = torch.full((n, 32, oh, ow), float("nan"), device="cuda").contiguous(memory_format=torch.channels_last)
    if wpk is None:
        wpk = torch.empty(_need("mirl_conv1p_u8_wpk_floats"), device="cuda")
    so, _, sh, sw = w.stride()
    check(lib.mirl_conv1p_u8_fwd(n, h, ww, _p(x), _p(w), so, sh, sw, _p(b), scale, _p(wpk), _p(y), flags, _st()), "conv1p")
    return y


def _frames(gen, n, h, w):
    return torch.randint(0, 256, (n, 1, h, w), dtype=torch.uint8, device="cuda", generator=gen)


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_forward_integer_weights_are_bit_exact(n, h, w):
    """whole tiles, a tail tile, one partial tile, ONE output position, more frames than workgroups; 64 * 255 * 2 + 50 000 < 2^24"""
    g = torch.Generator(device="cuda").manual_seed(n * 1000 + h)
    x = _frames(g, n, h, w)
    wt = torch.randint(-2, 3, (32, 1, 8, 8), device="cuda", generator=g).float()
    b = torch.randint(-50000, 50000, (32,), device="cuda", generator=g).float()
    want = F.relu(F.conv2d(x.double(), wt.double(), b.double(), 4)).float()
    for lay in _layouts(wt):
        got = _fwd(x, lay, b, 1.0)
        assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got, want)


def test_forward_does_not_depend_on_the_launch_shape_and_flags_are_checked():
    from rltime_amd._lib import lib
    g = torch.Generator(device="cuda").manual_seed(7)
    x = _frames(g, 1025, 84, 84)
    wt = torch.randn(32, 1, 8, 8, device="cuda", generator=g) * 0.1
    b = torch.randn(32, device="cuda", generator=g) * 0.1
    scale = 1.0 / 255.0
    wpk = torch.empty(_need("mirl_conv1p_u8_wpk_floats"), device="cuda")
    big = _fwd(x, wt, b, scale, wpk=wpk)
    assert not bool(torch.isnan(big).any())
    # three frames alone (their tiles split across workgroups) against the same frames inside the big call
    assert torch.equal(_fwd(x[0:3], wt, b, scale), big[0:3])
    assert torch.equal(_fwd(x[1022:1025], wt, b, scale), big[1022:1025])
    # bit 3: the block the previous call packed
    assert torch.equal(_fwd(x, wt, b, scale, flags=8, wpk=wpk), big)
    assert torch.equal(_fwd(x[5:38], wt, b, scale, flags=8, wpk=wpk), big[5:38])
    # ... and a block this entry point never packed; every other bit is unknown: nothing is touched
    # (the library remembers packed blocks by address: a slice of a 4 MB allocation cannot be a recycled 12 KB scratch block)
    fresh = torch.full((1 << 20,), -54321.0, device="cuda")[4096:4096 + wpk.numel()]
    y = torch.full((1, 32, 20, 20), -12345.0, device="cuda").contiguous(memory_format=torch.channels_last)
    so, _, sh, sw = wt.stride()
    call = lambda flags: lib.mirl_conv1p_u8_fwd(1, 84, 84, _p(x), _p(wt), so, sh, sw, _p(b), scale, _p(fresh), _p(y), flags, _st())   # noqa: E731
    assert call(8) == ERR_STATE
    for flags in (1, 2, 4, 16, 32, 1 << 8, 1 << 24, 8 | 1):
        assert call(flags) == ERR_ARG, flags
    torch.cuda.synchronize()
    assert bool((y == -12345.0).all()) and bool((fresh == -54321.0).all())
    assert call(0) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, big[0:1])


@pytest.mark.parametrize("n,h,w", [(2, 84, 84), (257, 84, 84), (2050, 84, 84), (5, 44, 52)] + FLAPPY)
def test_forward_real_weights_within_tolerance(n, h, w):
    g = torch.Generator(device="cuda").manual_seed(n)
    x = _frames(g, n, h, w)
    torch.manual_seed(n)
    conv = nn.Conv2d(1, 32, 8, 4).cuda()
    with torch.no_grad():
        conv.bias.uniform_(-0.3, 0.3)
        want = F.relu(F.conv2d(x.double() * (1.0 / 255.0), conv.weight.double(), conv.bias.double(), 4))
        got = _fwd(x, conv.weight.detach(), conv.bias.detach(), 1.0 / 255.0)
        lib32 = F.relu(F.conv2d(x.float() * (1.0 / 255.0), conv.weight, conv.bias, 4))
    top = float(want.abs().max())
    err, err_lib = float((got.double() - want).abs().max()) / top, float((lib32.double() - want).abs().max()) / top
    print("conv1p forward n=%d %dx%d: err %.3e of the largest output, library f32 conv %.3e, ratio %.2f" % (n, h, w, err, err_lib, err / max(err_lib, 1e-30)))
    assert err <= 1e-5, err            # the 4-plane kernel's bar, ten times inside the per-op 1e-4: 64 f32 terms


@pytest.mark.parametrize("name", list(cp.FWD_CASES))
def test_forward_probe_operands_are_bit_equal_to_float64(name):
    c = cp.fwd_case(name)
    x, w, b = c["x"].cuda(), c["w"].cuda(), c["bias"].cuda()
    want = F.relu(F.conv2d(x.double(), w.double(), b.double(), 4))
    for lay in _layouts(w):
        assert torch.equal(_fwd(x, lay, b, 1.0).double(), want)


# ---- weight gradient ------------------------------------------------------------------------------------------------------------

def _likes():
    return torch.empty(32, 1, 8, 8, device="cuda"), torch.empty_strided((32, 1, 8, 8), (64, 1, 8, 1), device="cuda")


def _wrw(x, g, scale, like):
    from rltime_amd._lib import lib, check
    scratch = torch.empty(_need("mirl_conv1p_u8_wrw_scratch_floats"), device="cuda")
    dw = torch.full_like(like, float("nan"))
    assert dw.stride() == like.stride()
    n, _, h, w = x.shape
    so, _, sh, sw = dw.stride()
    check(lib.mirl_conv1p_u8_wrw(n, h, w, _p(x), _p(g), scale, _p(scratch), _p(dw), so, sh, sw, _st()), "conv1p_wrw")
    return dw


def _wrw_masked(x, dy, y, scale, like):
    from rltime_amd._lib import lib, check
    scratch = torch.empty(_need("mirl_conv1p_u8_wrw_scratch_floats"), device="cuda")
    dw, db = torch.full_like(like, float("nan")), torch.full((32,), float("nan"), device="cuda")
    n, _, h, w = x.shape
    so, _, sh, sw = dw.stride()
    check(lib.mirl_conv1p_u8_wrw_masked(n, h, w, _p(x), _p(dy), _p(y), scale, _p(scratch), _p(dw), so, sh, sw, _p(db), _st()), "conv1p_wrw_masked")
    return dw, db


def _wrw_reference(x, g, scale, dtype=torch.float64):
    # d/dW of sum(conv2d(x*scale, W) * g)
    w = torch.zeros(32, 1, 8, 8, dtype=dtype, device="cuda", requires_grad=True)
    (F.conv2d(x.to(dtype) * scale, w, None, 4) * g.to(dtype)).sum().backward()
    return w.grad


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("n,h,w", [(1, 84, 84), (2, 84, 84), (3, 36, 36), (2, 44, 52), (4, 12, 16), (3, 8, 8), (1, 100, 100)] + FLAPPY)
def test_weight_gradient_integer_case_is_bit_exact(n, h, w):
    g_ = torch.Generator(device="cuda").manual_seed(n * 100 + w)
    x = _frames(g_, n, h, w)
    oh, ow = (h - 8) // 4 + 1, (w - 8) // 4 + 1
    g = _cl(torch.randint(-3, 4, (n, 32, oh, ow), device="cuda", generator=g_).float())
    want = _wrw_reference(x, g, 1.0).float()          # |sums| <= n*oh*ow*255*3 < 2^24: exact in fp32 in any order
    for like in _likes():
        got = _wrw(x, g, 1.0, like)
        assert got.stride() == like.stride() and torch.equal(got, want)


@pytest.mark.parametrize("n,h,w", [(5, 84, 84), (1025, 84, 84), (2051, 84, 84), (1030, 44, 52)] + FLAPPY)
def test_weight_gradient_within_tolerance_and_reproducible(n, h, w):
    g_ = torch.Generator(device="cuda").manual_seed(n)
    x = _frames(g_, n, h, w)
    oh, ow = (h - 8) // 4 + 1, (w - 8) // 4 + 1
    g = _cl(torch.randn(n, 32, oh, ow, device="cuda", generator=g_) * (torch.rand(n, 32, oh, ow, device="cuda", generator=g_) < 0.5))
    like = _likes()[1]
    a, b = _wrw(x, g, 1.0 / 255.0, like), _wrw(x, g, 1.0 / 255.0, like)
    assert torch.equal(a, b)                          # fixed partition and order: bit-identical reruns
    want = _wrw_reference(x, g, 1.0 / 255.0)
    top = float(want.abs().max())
    err = float((a.double() - want).abs().max()) / top
    # the library's f32 weight gradient on the same inputs stands in for the f32-pipe kernel this family does not have
    err_lib = float((_wrw_reference(x, g, 1.0 / 255.0, torch.float32).double() - want).abs().max()) / top
    print("conv1p weight gradient n=%d %dx%d: err %.3e of the largest entry, library f32 %.3e" % (n, h, w, err, err_lib))
    assert err <= 1e-4, err
    assert err <= max(2.0 * err_lib, 2e-6), (err, err_lib)


@pytest.mark.parametrize("n,h,w", [(2, 84, 84), (3, 36, 36), (1, 8, 8), (1027, 84, 84), (1030, 44, 52)] + FLAPPY)
def test_masked_weight_gradient_equals_mask_pass_plus_weight_gradient(n, h, w):
    """mirl_conv1p_u8_wrw_masked against the two-launch form (k_relu_bwd_bias_rows, then mirl_conv1p_u8_wrw on its output):
    dW BIT-identical (the same masked values enter the same sums in the same order), db the masked gradient's column sums
    (bit-exact on integer dy, 1e-5 of scale on real dy), both bit-reproducible."""
    from rltime_amd.models.torch.fused import relu_bwd_bias_rows
    g_ = torch.Generator(device="cuda").manual_seed(7 * n + w)
    x = _frames(g_, n, h, w)
    oh, ow = (h - 8) // 4 + 1, (w - 8) // 4 + 1
    y = _cl(torch.randn(n, 32, oh, ow, device="cuda", generator=g_).clamp(min=0))
    like = _likes()[1]
    for integer in (True, False):
        dy = _cl(torch.randint(-3, 4, (n, 32, oh, ow), device="cuda", generator=g_).float() if integer
                 else torch.randn(n, 32, oh, ow, device="cuda", generator=g_))
        scale = 1.0 if integer else 1.0 / 255.0
        g, db_ref = relu_bwd_bias_rows(dy, y, 32)
        dw_ref = _wrw(x, g, scale, like)
        dw, db = _wrw_masked(x, dy, y, scale, like)
        assert torch.equal(dw, dw_ref)
        want_db = (dy.double() * (y > 0)).sum((0, 2, 3))
        if integer:
            assert torch.equal(db.double(), want_db) and torch.equal(db, db_ref)
        else:
            assert float((db.double() - want_db).abs().max()) <= 1e-5 * max(float(want_db.abs().max()), 1.0)
        dw2, db2 = _wrw_masked(x, dy, y, scale, like)
        assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("name", list(cp.WRW_CASES))
def test_weight_gradient_probe_operands_are_bit_equal_to_float64(name):
    c = cp.wrw_case(name)
    x, g, y = c["x"].cuda(), _cl(c["g"].cuda()), _cl(c["y"].cuda())
    for like in _likes():
        assert torch.equal(_wrw(x, g, 1.0, like).double(), _wrw_reference(x, g, 1.0))
        dw, db = _wrw_masked(x, g, y, 1.0, like)
        kept = g.double() * (y > 0)
        assert torch.equal(dw.double(), _wrw_reference(x, kept, 1.0))
        assert torch.equal(db.double(), kept.sum((0, 2, 3))) and bool((db != 0).all())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_coverage_and_refusals_before_any_launch():
    from rltime_amd._lib import lib
    for h, w in [(84, 84), (36, 36), (44, 52), (12, 16), (8, 8), (100, 100), (120, 80)]:
        assert lib.mirl_conv1p_u8_supported(h, w, 32, 8, 4) == 1, (h, w)
    for h, w, f, k, s in [(84, 84, 64, 8, 4), (84, 84, 32, 4, 4), (84, 84, 32, 8, 2), (84, 82, 32, 8, 4), (7, 84, 32, 8, 4),
                          (42, 42, 32, 8, 4), (256, 256, 32, 8, 4)]:
        assert lib.mirl_conv1p_u8_supported(h, w, f, k, s) == 0, (h, w, f, k, s)
    assert lib.mirl_conv1_u8_supported(1, 84, 84, 32, 8, 4) == 0                 # the 4-plane family's answer has not moved
    x = torch.zeros((2, 1, 84, 84), dtype=torch.uint8, device="cuda")
    wt, b = torch.zeros(32, 1, 8, 8, device="cuda"), torch.zeros(40, device="cuda")
    y = _cl(torch.full((2, 32, 20, 20), -12345.0, device="cuda"))
    wpk = torch.full((_need("mirl_conv1p_u8_wpk_floats") + 4,), -54321.0, device="cuda")
    scratch = torch.full((_need("mirl_conv1p_u8_wrw_scratch_floats") + 4,), -54321.0, device="cuda")
    dw, db = torch.full((32, 1, 8, 8), -12345.0, device="cuda"), torch.full((32,), -12345.0, device="cuda")
    off = lambda t: C.c_void_p(t.data_ptr() + 4)                                  # noqa: E731  (4 bytes off the 16-byte grid)
    fwd = [2, 84, 84, _p(x), _p(wt), 64, 8, 1, _p(b), 1.0, _p(wpk), _p(y), 0, _st()]
    for pos, bad in [(0, 0), (0, -3), (1, 82), (2, 82), (1, 7), (1, 5000), (3, None), (4, None), (8, None), (10, None), (11, None),
                     (3, off(x)), (8, off(b)), (10, off(wpk)), (11, off(y))]:
        a = list(fwd)
        a[pos] = bad
        assert lib.mirl_conv1p_u8_fwd(*a) == ERR_ARG, pos
    wrw = [2, 84, 84, _p(x), _p(y), 1.0, _p(scratch), _p(dw), 64, 8, 1, _st()]
    for pos, bad in [(0, 0), (1, 42), (2, 42), (3, None), (4, None), (6, None), (7, None), (3, off(x)), (4, off(y)), (6, off(scratch))]:
        a = list(wrw)
        a[pos] = bad
        assert lib.mirl_conv1p_u8_wrw(*a) == ERR_ARG, pos
    msk = [2, 84, 84, _p(x), _p(y), _p(y), 1.0, _p(scratch), _p(dw), 64, 8, 1, _p(db), _st()]
    for pos, bad in [(0, -1), (1, 42), (3, None), (4, None), (5, None), (7, None), (8, None), (12, None), (4, off(y)), (5, off(y))]:
        a = list(msk)
        a[pos] = bad
        assert lib.mirl_conv1p_u8_wrw_masked(*a) == ERR_ARG, pos
    torch.cuda.synchronize()
    for t, v in ((y, -12345.0), (wpk, -54321.0), (scratch, -54321.0), (dw, -12345.0), (db, -12345.0)):
        assert bool((t == v).all())
    assert lib.mirl_conv1p_u8_wpk_floats(None) == ERR_ARG and lib.mirl_conv1p_u8_wrw_scratch_floats(None) == ERR_ARG
