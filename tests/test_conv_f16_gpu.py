"""GPU: the 16-filter input layer from uint8 frames (csrc/conv_in_f16.hip) through its C entry points, per plane count, against
float64: the reference's expression for the layer, rltime/models/torch/modules/cnn.py:44-49 at Conv2d(P -> 16, kernel 8, stride
4), the first layer of models/modules/nature_cnn_small.json.  Integer operands make every sum exact in f32 in any order, so
indexing is checked BIT-exactly; real operands are held to the bound of what rounds: the products are exact in the
accumulator, so one rounding of w * scale, the f32 additions of the chain, the joins of the part chains and the bias remain."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ERR_ARG = -1
PREFIX = {1: "mirl_conv1f16p_u8_", 3: "mirl_conv1f16p3_u8_", 4: "mirl_conv1f16p4_u8_"}
PLANES = sorted(PREFIX)
# one position (the tile is almost all tail); 4 x 5 positions (a tile tail, a tail octet); 8 x 10; the workload's frame with more
# frames than one fill and at one frame (its tiles split across workgroups); more frames than resident workgroups at every P
# (two or four frames per LDS fill, then a remainder); the RGB Flappy frame (29 x 19 positions, 35 tiles)
SHAPES = [(1, 8, 8), (3, 20, 24), (5, 36, 44), (33, 84, 84), (1, 84, 84), (2051, 20, 24), (2, 120, 80)]
# (planes, n, h, w); four planes of 120 x 80 as bf16 are beyond the 64 KiB of LDS the weight gradient asks for: refused, below
CASES = [(p,) + s for p in PLANES for s in SHAPES if (p, s) != (4, (2, 120, 80))]
EPS = 2.0 ** -24


def _p(t):
    return C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _fn(planes, name):
    from rltime_amd._lib import lib
    return getattr(lib, PREFIX[planes] + name)


def _need(planes, query):
    from rltime_amd._lib import check
    need = C.c_int64()
    check(_fn(planes, query)(C.byref(need)))
    return need.value


def _strides(t):
    return t.stride() if t.shape[1] > 1 else (t.stride(0), t.stride(2), t.stride(3))      # no channel stride for one plane


def _out(h, w):
    return (h - 8) // 4 + 1, (w - 8) // 4 + 1


def _fwd(x, w, b, scale, flags=0, wpk=None):
    from rltime_amd._lib import check
    n, planes, h, ww = x.shape
    y = _cl(torch.full((n, 16) + _out(h, ww), float("nan"), device="cuda"))
    if wpk is None:
        wpk = torch.empty(_need(planes, "wpk_floats"), device="cuda")
    check(_fn(planes, "fwd")(n, h, ww, _p(x), _p(w), *_strides(w), _p(b), scale, _p(wpk), _p(y), flags, _st()), "fwd")
    return y


def _wrw(x, g, scale, like, y=None):
    """the plain form, or with the forward output y the masked one: -> dw, or (dw, db)"""
    from rltime_amd._lib import check
    n, planes, h, w = x.shape
    scratch = torch.empty(_need(planes, "wrw_scratch_floats"), device="cuda")
    dw, db = torch.full_like(like, float("nan")), torch.full((16,), float("nan"), device="cuda")
    assert dw.stride() == like.stride()
    if y is None:
        check(_fn(planes, "wrw")(n, h, w, _p(x), _p(g), scale, _p(scratch), _p(dw), *_strides(dw), _st()), "wrw")
        return dw
    check(_fn(planes, "wrw_masked")(n, h, w, _p(x), _p(g), _p(y), scale, _p(scratch), _p(dw), *_strides(dw), _p(db), _st()), "wrw_masked")
    return dw, db


def _wrw64(x, g, scale):
    """d/dW of sum(conv2d(x * scale, W) * g) in float64"""
    w = torch.zeros(16, x.shape[1], 8, 8, dtype=torch.float64, device="cuda", requires_grad=True)
    (F.conv2d(x.double() * scale, w, None, 4) * g.double()).sum().backward()
    return w.grad


@functools.lru_cache(maxsize=None)
def _frames(planes, n, h, w):
    """n frames and three more behind them, so that the same frames can be run at another N"""
    g = torch.Generator(device="cuda").manual_seed(1000 * planes + 10 * n + h)
    return torch.randint(0, 256, (n + 3, planes, h, w), dtype=torch.uint8, device="cuda", generator=g), g


@pytest.mark.parametrize("planes,n,h,w", CASES)
def test_forward_integer_operands_are_bit_equal_to_float64(planes, n, h, w):
    x, g = _frames(planes, n, h, w)
    x = x[:n]
    wt = torch.randint(-2, 3, (16, planes, 8, 8), device="cuda", generator=g).float()
    b = torch.randint(-50000, 50000, (16,), device="cuda", generator=g).float()
    assert 64 * planes * 255 * 2 + 50000 < 2 ** 24                         # every partial sum is an exact float32
    want = F.relu(F.conv2d(x.double(), wt.double(), b.double(), 4))
    for lay in (wt, _cl(wt)):
        got = _fwd(x, lay, b, 1.0)
        assert got.is_contiguous(memory_format=torch.channels_last) and torch.equal(got.double(), want)


@pytest.mark.parametrize("planes,n,h,w", CASES)
def test_forward_real_operands_within_the_rounding_bound_and_independent_of_the_launch(planes, n, h, w):
    xall, _ = _frames(planes, n, h, w)
    x, scale = xall[:n], 1.0 / 255.0
    torch.manual_seed(n + planes)
    conv = nn.Conv2d(planes, 16, 8, 4).cuda().requires_grad_(False)
    conv.bias.uniform_(-0.3, 0.3)
    wt, b = conv.weight, conv.bias
    want = F.relu(F.conv2d(x.double() * scale, wt.double(), b.double(), 4))
    bound = (64 * planes + 4) * EPS * (F.conv2d(x.double() * scale, wt.double().abs(), None, 4) + b.double().abs()[None, :, None, None])
    wpk = torch.empty(_need(planes, "wpk_floats"), device="cuda")
    got = _fwd(x, wt, b, scale, wpk=wpk)
    excess = ((got.double() - want).abs() - bound).max()
    print("conv f16 forward P=%d n=%d %dx%d: largest error / bound %.3f" % (planes, n, h, w, float(((got.double() - want).abs() / bound).max())))
    assert float(excess) <= 0.0
    assert torch.equal(_fwd(x, wt, b, scale, flags=8, wpk=wpk), got)       # the block the previous call packed
    assert torch.equal(_fwd(xall, wt, b, scale)[:n], got)                  # the same frames at another N
    assert torch.equal(_fwd(xall[n - 1:n + 1], wt, b, scale)[:1], got[n - 1:])


@pytest.mark.parametrize("planes,n,h,w", CASES)
def test_weight_gradient_plain_and_masked(planes, n, h, w):
    from rltime_amd.models.torch.fused import relu_bwd_bias_rows
    xall, gen = _frames(planes, n, h, w)
    x = xall[:n]
    oh, ow = _out(h, w)
    shape = (n, 16, oh, ow)
    likes = (torch.empty(16, planes, 8, 8, device="cuda"), _cl(torch.empty(16, planes, 8, 8, device="cuda")))
    # integer g, scale 1: bit-equal to the float64 sum
    top = 3 if n * oh * ow * 255 * 3 < 2 ** 24 else 1
    assert n * oh * ow * 255 * top < 2 ** 24
    gi = _cl(torch.randint(-top, top + 1, shape, device="cuda", generator=gen).float())
    want = _wrw64(x, gi, 1.0)
    for like in likes:
        got = _wrw(x, gi, 1.0, like)
        assert got.stride() == like.stride() and torch.equal(got.double(), want)
    # real g, half of it zero, scale 1/255: within the bound of N OH OW f32 additions, and bit-identical reruns
    scale = 1.0 / 255.0
    gr = _cl(torch.randn(shape, device="cuda", generator=gen) * (torch.rand(shape, device="cuda", generator=gen) < 0.5))
    a, b = _wrw(x, gr, scale, likes[1]), _wrw(x, gr, scale, likes[1])
    assert torch.equal(a, b)
    bound = (n * oh * ow + 4) * EPS * _wrw64(x, gr.abs(), scale)
    err = (a.double() - _wrw64(x, gr, scale)).abs()
    print("conv f16 weight gradient P=%d n=%d %dx%d: largest error / bound %.3f" % (planes, n, h, w, float((err / bound.clamp(min=1e-300)).max())))
    assert float((err - bound).max()) <= 0.0
    # masked: bit-equal to the mask pass followed by the plain form; db bit-equal on integer dy (exact in any order)
    y = _cl(torch.randn(shape, device="cuda", generator=gen).clamp(min=0))
    for dy, sc in ((gi, 1.0), (gr, scale)):
        g, db_ref = relu_bwd_bias_rows(dy, y, 16)
        dw, db = _wrw(x, dy, sc, likes[1], y=y)
        assert torch.equal(dw, _wrw(x, g, sc, likes[1]))
        kept = dy.double() * (y > 0)
        if dy is gi:
            assert torch.equal(db, db_ref) and torch.equal(db.double(), kept.sum((0, 2, 3)))
        else:
            assert float(((db.double() - kept.sum((0, 2, 3))).abs() - (n * oh * ow + 4) * EPS * kept.abs().sum((0, 2, 3))).max()) <= 0.0
        dw2, db2 = _wrw(x, dy, sc, likes[1], y=y)
        assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("planes", PLANES)
def test_refusals_before_any_launch(planes):
    """32 or 8 filters, W % 4 != 0 and H < 8 are not this family's: `supported` says so (it alone takes the filter count) and the
    launchers return MIRL_ERR_ARG with nothing written"""
    sup = _fn(planes, "supported")
    assert sup(84, 84, 16, 8, 4) == 1 and sup(8, 8, 16, 8, 4) == 1 and sup(36, 44, 16, 8, 4) == 1
    assert sup(120, 80, 16, 8, 4) == (planes < 4) and sup(100, 100, 16, 8, 4) == (planes < 4)
    for bad in [(84, 84, 32, 8, 4), (84, 84, 8, 8, 4), (84, 82, 16, 8, 4), (4, 84, 16, 8, 4), (84, 84, 16, 4, 4), (84, 84, 16, 8, 2), (42, 42, 16, 8, 4)]:
        assert sup(*bad) == 0, bad
    x = torch.zeros((2, planes, 84, 84), dtype=torch.uint8, device="cuda")
    wt, b = torch.zeros(16, planes, 8, 8, device="cuda"), torch.zeros(24, device="cuda")
    y = _cl(torch.full((2, 16, 20, 20), -12345.0, device="cuda"))
    wpk = torch.full((_need(planes, "wpk_floats") + 4,), -54321.0, device="cuda")
    scratch = torch.full((_need(planes, "wrw_scratch_floats") + 4,), -54321.0, device="cuda")
    dw, db = torch.full((16, planes, 8, 8), -12345.0, device="cuda"), torch.full((16,), -12345.0, device="cuda")
    off = lambda t: C.c_void_p(t.data_ptr() + 4)                                  # noqa: E731  (4 bytes off the 16-byte grid)
    s = len(_strides(wt))
    fwd = [2, 84, 84, _p(x), _p(wt), *_strides(wt), _p(b), 1.0, _p(wpk), _p(y), 0, _st()]
    for pos, bad in [(0, 0), (0, -3), (2, 82), (1, 4), (1, 7), (3, None), (4, None), (5 + s, None), (7 + s, None), (8 + s, None),
                     (3, off(x)), (5 + s, off(b)), (7 + s, off(wpk)), (8 + s, off(y)), (9 + s, 1), (9 + s, 16), (9 + s, 8 | 2)]:
        a = list(fwd)
        a[pos] = bad
        assert _fn(planes, "fwd")(*a) == ERR_ARG, pos
    wrw = [2, 84, 84, _p(x), _p(y), 1.0, _p(scratch), _p(dw), *_strides(dw), _st()]
    msk = [2, 84, 84, _p(x), _p(y), _p(y), 1.0, _p(scratch), _p(dw), *_strides(dw), _p(db), _st()]
    for name, args, cases in (("wrw", wrw, [(0, 0), (2, 82), (1, 4), (3, None), (4, None), (6, None), (7, None), (4, off(y)), (6, off(scratch))]),
                              ("wrw_masked", msk, [(0, -1), (2, 82), (1, 4), (3, None), (5, None), (7, None), (8, None), (9 + s, None), (5, off(y))])):
        for pos, bad in cases:
            a = list(args)
            a[pos] = bad
            assert _fn(planes, name)(*a) == ERR_ARG, (name, pos)
    torch.cuda.synchronize()
    for t, v in ((y, -12345.0), (wpk, -54321.0), (scratch, -54321.0), (dw, -12345.0), (db, -12345.0)):
        assert bool((t == v).all())
    assert _fn(planes, "wpk_floats")(None) == ERR_ARG and _fn(planes, "wrw_scratch_floats")(None) == ERR_ARG
