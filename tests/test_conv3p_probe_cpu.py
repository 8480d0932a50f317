"""CPU: the three-plane input layer (csrc/conv_in_rows.hip) as far as it can be held without a device.

The part-probing operands of tests/conv3p_probe.py are what tests/test_conv3p_gpu.py needs them to be.  For exactly the
operands the GPU tests send through the kernels:

  1. all terms of an output are integers of the output's unit and sum |terms| < 2^24 of it, so every partial sum in any order
     is an f32 number; three shuffled f32 summation orders are followed term by term and every prefix equals float64's;
  2. the method's emulation (three bf16 parts, f32 accumulation, also in the kernel's own 32-wide k steps: four kernel rows
     of one plane) equals float64;
  3. every output depends on each part: leaving out the mid or the lo plane changes it;
  4. the planted ReLU mask of the weight-gradient cases keeps between one and four positions per filter.

And mirl_conv1p3_u8_supported, which is host logic: what the family covers, what it refuses, and that the other two
families' queries answer as before."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv3p_probe as cp
from tests.split3_probe import split3


def _shuffled_orders_are_exact(terms, seed):
    """terms (T, ...): along three random orders of T every f32 prefix sum equals the float64 one"""
    gen = torch.Generator().manual_seed(seed)
    for _ in range(3):
        t = terms[torch.randperm(terms.shape[0], generator=gen)]
        assert torch.equal(torch.cumsum(t, 0, dtype=torch.float32).double(), torch.cumsum(t.double(), 0))


def _conv(w, x):
    return F.conv2d(x, w, None, 4)


def test_the_bounds_of_the_docstring():
    assert cp.FWD_BOUND == 6 * 2 * (2 ** 20 + 2 ** 12 + 2 ** 4) + 2 ** 20 < cp.LIMIT
    assert cp.WRW_BOUND == 15 * (2 ** 20 + 2 ** 12 + 2 ** 4) < cp.LIMIT
    # the one-plane density (four lit pixels of 1..3 per window and plane) would not hold for three planes
    assert 3 * 12 * (2 ** 20 + 2 ** 12 + 2 ** 4) > cp.LIMIT


@pytest.mark.parametrize("name", list(cp.FWD_CASES))
def test_forward_operands(name):
    c = cp.fwd_case(name)
    x, w, unit = c["x"].float(), c["w"], c["unit"].view(1, 32, 1, 1)
    n = x.shape[0]
    assert x.shape[1] == 3 and int(c["x"].max()) <= 2 and not any(bool(p.any()) for p in split3(x)[1:])
    # two lit positions in every 8 x 8 window of every plane, every weight part positive in the filter's unit
    lit = (x > 0).float()
    for p in range(3):
        assert bool((F.conv2d(lit[:, p:p + 1], torch.ones(1, 1, 8, 8), None, 4) == 2).all())
    assert len({tuple(lit[0, p].nonzero()[0].tolist()) for p in range(3)} | {tuple(lit[n - 1, p].nonzero()[0].tolist()) for p in range(3)}) > 1
    for part in split3(c["w_int"]):
        assert bool((part > 0).all())
    assert bool((c["w"] == c["w_int"] * c["unit"].view(32, 1, 1, 1)).all())
    # 1. integers of the unit, and the bound of the docstring
    bound = _conv(sum(p.abs().double() for p in split3(c["w_int"])), x.double()) + c["bias_int"].abs().double().view(1, 32, 1, 1)
    assert float(bound.max()) <= cp.FWD_BOUND < cp.LIMIT
    frames = [0, 1, n - 1]
    _shuffled_orders_are_exact(cp.fwd_terms(c, frames), 1)
    # 2. the method equals float64 (before the ReLU, which is exact)
    want = _conv(w.double(), x.double()) + c["bias"].double().view(1, 32, 1, 1)
    full = cp.emulate(_conv, w, x) + c["bias"].view(1, 32, 1, 1)
    assert full.dtype == torch.float32 and torch.equal(full.double(), want)
    assert 0.2 < float((want > 0).float().mean()) < 0.8                               # the ReLU cuts some outputs and keeps some
    # the kernel's own order: rows = positions, k = (c, kh, kw) in 32-wide steps (one MFMA = four kernel rows of one plane)
    cols = F.unfold(x[frames], 8, stride=4)                                            # (3, 192, positions)
    a = cols.permute(0, 2, 1).reshape(-1, cp.TAPS)
    got = cp.emulate_gemm(w.view(32, cp.TAPS), a.t().contiguous(), cp.PIXEL_PRODUCTS, kstep=32)     # (32, 3 * positions)
    assert torch.equal(got.view(32, 3, -1).permute(1, 0, 2).reshape(want[frames].shape).double() + c["bias"].double().view(1, 32, 1, 1),
                       want[frames])
    # 3. every output depends on each part
    for drop in ((1, 0), (2, 0)):
        rest = tuple(p for p in cp.PIXEL_PRODUCTS if p != drop)
        assert bool((cp.emulate(_conv, w, x, rest) + c["bias"].view(1, 32, 1, 1) != full).all()), drop


def test_coverage_is_host_logic():
    """mirl_conv1p3_u8_supported needs no device: the shapes the family covers, the ones it refuses — W % 4, H W % 16, H < 8,
    F, K, S, and a frame whose three bf16 planes pass the plan's 64 KiB of LDS — and the other families' unchanged answers."""
    from rltime_amd._lib import lib
    for h, w in [(8, 8), (12, 16), (36, 36), (44, 52), (84, 84), (100, 100), (120, 80)]:
        assert lib.mirl_conv1p3_u8_supported(h, w, 32, 8, 4) == 1, (h, w)
    for h, w, f, k, s in [(84, 82, 32, 8, 4), (42, 42, 32, 8, 4), (7, 84, 32, 8, 4), (84, 4, 32, 8, 4), (84, 84, 64, 8, 4),
                          (84, 84, 32, 4, 4), (84, 84, 32, 8, 2), (108, 104, 32, 8, 4), (128, 88, 32, 8, 4), (256, 256, 32, 8, 4),
                          (1 << 20, 1 << 20, 32, 8, 4)]:
        assert lib.mirl_conv1p3_u8_supported(h, w, f, k, s) == 0, (h, w, f, k, s)
    # the limit is the three staged bf16 planes with their tail over-read: 3 * 2 * pitch <= 65 536
    assert 3 * 2 * 10008 <= 65536 < 3 * 2 * (108 * 104)
    assert lib.mirl_conv1_u8_supported(3, 84, 84, 32, 8, 4) == 0                      # the four-plane family takes four planes
    assert lib.mirl_conv1_u8_supported(4, 84, 84, 32, 8, 4) == 1
    assert lib.mirl_conv1_u8_supported(1, 84, 84, 32, 8, 4) == 0
    assert lib.mirl_conv1p_u8_supported(84, 84, 32, 8, 4) == 1 and lib.mirl_conv1p_u8_supported(120, 80, 32, 8, 4) == 1
    assert lib.mirl_conv1p_u8_supported(256, 256, 32, 8, 4) == 0


def test_the_family_table_reaches_the_query():
    """fused.py's table has the third entry, with the channel stride among a weight's strides and no plane count in the query"""
    from rltime_amd.models.torch.fused import conv_u8_family
    fam = conv_u8_family(3)
    assert fam is not None and fam.planes == 3 and fam.prefix == "mirl_conv1p3_u8_"
    assert fam.supported(120, 80, 32, 8, 4) and not fam.supported(120, 82, 32, 8, 4)
    w = torch.empty(32, 3, 8, 8)
    assert fam.strides(w) == (192, 64, 8, 1)
    assert fam.strides(w.contiguous(memory_format=torch.channels_last)) == (192, 1, 24, 3)
    assert conv_u8_family(1).supported(84, 84, 32, 8, 4) and conv_u8_family(4).supported(84, 84, 32, 8, 4)
    assert conv_u8_family(2) is None


@pytest.mark.parametrize("name", list(cp.WRW_CASES))
def test_weight_gradient_operands(name):
    c = cp.wrw_case(name)
    x, g, g_int, y = c["x"].float(), c["g"], c["g_int"], c["y"]
    assert x.shape[1] == 3 and int(c["x"].max()) <= 3
    live = g_int != 0
    per_filter = min(5, live[:, 0].numel())
    assert bool((live.sum((0, 2, 3)) == per_filter).all())                             # five positions per filter
    for part in split3(g_int[live]):
        assert bool((part > 0).all())
    # 4. the planted mask
    kept_n = (live & (y > 0)).sum((0, 2, 3))
    assert bool((kept_n == per_filter - 1).all()) and 1 <= per_filter - 1 <= 4
    assert torch.equal(c["kept"], (live & (y > 0)).float())
    assert 0.3 < float((y > 0).float().mean()) < 0.95                                  # and an ordinary activation elsewhere
    for gg, gi in ((g, g_int), (g * (y > 0), g_int * (y > 0))):
        # 1.
        bound = cp.op_wrw(sum(p.abs().double() for p in split3(gi)), x.double())
        assert float(bound.max()) <= cp.WRW_BOUND < cp.LIMIT
        _shuffled_orders_are_exact(cp.wrw_terms(gg, x), 2)
        # 2.
        want = cp.op_wrw(gg.double(), x.double())
        full = cp.emulate(cp.op_wrw, gg, x)
        assert full.dtype == torch.float32 and torch.equal(full.double(), want)
        ref = torch.ops.aten.convolution_backward(gg.double(), x.double(), want, None, [4, 4], [0, 0], [1, 1], False, [0, 0], 1,
                                                  [False, True, False])[1]
        assert torch.equal(want, ref)                                                  # op_wrw restates the weight gradient
        # 3.
        for drop in ((1, 0), (2, 0)):
            rest = tuple(p for p in cp.PIXEL_PRODUCTS if p != drop)
            assert bool((cp.emulate(cp.op_wrw, gg, x, rest) != full).all()), drop
    # the masked form's bias gradient: the kept values' sum per filter, exact and depending on each part
    kept = g_int * (y > 0)
    assert float(sum(p.abs().double() for p in split3(kept)).sum((0, 2, 3)).max()) < cp.LIMIT
    for part in split3(kept)[1:]:
        assert bool((part.sum((0, 2, 3)) > 0).all())
