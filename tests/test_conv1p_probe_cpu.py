"""CPU: the part-probing operands of tests/conv1p_probe.py are what tests/test_conv1p_gpu.py needs them to be.  For exactly
the operands the GPU tests send through csrc/conv_in_rows.hip:

  1. all terms of an output are integers of the output's unit and sum |terms| < 2^24 of it, so every partial sum in any order
     is an f32 number; three shuffled f32 summation orders are followed term by term and every prefix equals float64's;
  2. the method's emulation (three bf16 parts, f32 accumulation, also in the kernel's own 32-wide k steps) equals float64;
  3. every output depends on each part: leaving out the mid or the lo plane changes it;
  4. the planted ReLU mask of the weight-gradient cases keeps between one and four positions per filter."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv1p_probe as cp
from tests.split3_probe import split3


def _shuffled_orders_are_exact(terms, seed):
    """terms (T, ...): along three random orders of T every f32 prefix sum equals the float64 one"""
    gen = torch.Generator().manual_seed(seed)
    for _ in range(3):
        t = terms[torch.randperm(terms.shape[0], generator=gen)]
        assert torch.equal(torch.cumsum(t, 0, dtype=torch.float32).double(), torch.cumsum(t.double(), 0))


def _conv(w, x):
    return F.conv2d(x, w, None, 4)


@pytest.mark.parametrize("name", list(cp.FWD_CASES))
def test_forward_operands(name):
    c = cp.fwd_case(name)
    x, w, unit = c["x"].float(), c["w"], c["unit"].view(1, 32, 1, 1)
    n = x.shape[0]
    assert x.shape[1] == 1 and int(c["x"].max()) <= 3 and not any(bool(p.any()) for p in split3(x)[1:])
    # four lit positions in every 8 x 8 window, every weight part positive in the filter's unit
    assert bool((F.conv2d((x > 0).float(), torch.ones(1, 1, 8, 8), None, 4) == 4).all())
    for part in split3(c["w_int"]):
        assert bool((part > 0).all())
    assert bool((c["w"] == c["w_int"] * c["unit"].view(32, 1, 1, 1)).all())
    # 1. integers of the unit, and the bound of the docstring
    bound = _conv(sum(p.abs().double() for p in split3(c["w_int"])), x.double()) + c["bias_int"].abs().double().view(1, 32, 1, 1)
    assert float(bound.max()) <= 12 * (2 ** 20 + 2 ** 12 + 2 ** 4) + 2 ** 20 < cp.LIMIT
    frames = [0, 1, n - 1]
    _shuffled_orders_are_exact(cp.fwd_terms(c, frames), 1)
    # 2. the method equals float64 (before the ReLU, which is exact)
    want = _conv(w.double(), x.double()) + c["bias"].double().view(1, 32, 1, 1)
    full = cp.emulate(_conv, w, x) + c["bias"].view(1, 32, 1, 1)
    assert full.dtype == torch.float32 and torch.equal(full.double(), want)
    assert 0.2 < float((want > 0).float().mean()) < 0.8                               # the ReLU cuts some outputs and keeps some
    # the kernel's own order: rows = positions, k = (kh, kw) in 32-wide steps (one MFMA = four kernel rows)
    cols = F.unfold(x[frames], 8, stride=4)                                            # (3, 64, positions)
    a = cols.permute(0, 2, 1).reshape(-1, 64)
    got = cp.emulate_gemm(w.view(32, 64), a.t().contiguous(), cp.PIXEL_PRODUCTS, kstep=32)     # (32, 3 * positions)
    assert torch.equal(got.view(32, 3, -1).permute(1, 0, 2).reshape(want[frames].shape).double() + c["bias"].double().view(1, 32, 1, 1),
                       want[frames])
    # 3. every output depends on each part
    for drop in ((1, 0), (2, 0)):
        rest = tuple(p for p in cp.PIXEL_PRODUCTS if p != drop)
        assert bool((cp.emulate(_conv, w, x, rest) + c["bias"].view(1, 32, 1, 1) != full).all()), drop


def test_coverage_is_host_logic():
    """mirl_conv1p_u8_supported needs no device: the shapes the family covers, the ones it refuses, and the 4-plane family's
    unchanged answer for one plane."""
    from rltime_amd._lib import lib
    for h, w in [(84, 84), (36, 36), (44, 52), (12, 16), (8, 8), (100, 100)]:
        assert lib.mirl_conv1p_u8_supported(h, w, 32, 8, 4) == 1, (h, w)
    for h, w, f, k, s in [(84, 84, 64, 8, 4), (84, 84, 32, 4, 4), (84, 84, 32, 8, 2), (84, 82, 32, 8, 4), (7, 84, 32, 8, 4),
                          (42, 42, 32, 8, 4), (256, 256, 32, 8, 4), (1 << 20, 1 << 20, 32, 8, 4)]:
        assert lib.mirl_conv1p_u8_supported(h, w, f, k, s) == 0, (h, w, f, k, s)
    assert lib.mirl_conv1_u8_supported(1, 84, 84, 32, 8, 4) == 0


@pytest.mark.parametrize("name", list(cp.WRW_CASES))
def test_weight_gradient_operands(name):
    c = cp.wrw_case(name)
    x, g, g_int, y = c["x"].float(), c["g"], c["g_int"], c["y"]
    assert x.shape[1] == 1 and int(c["x"].max()) <= 3
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
        assert float(bound.max()) <= 15 * (2 ** 20 + 2 ** 12 + 2 ** 4) < cp.LIMIT
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
