"""GPU: mirl_lstm_cell_fwd / mirl_lstm_cell_bwd (csrc/lstm.hip) at their C entry points, one step at a time, against the
float64 cell of tests/pointwise_restate.py (equal to torch.nn.LSTMCell and its autograd, tests/test_pointwise_restate_cpu.py).

First-order bounds, u = 2^-24, expf and tanhf within 1 ulp (2u relative):
  sigmoid s = 1 / (1 + expf(-x))   e_s = 4u s            (expf: 2u s (1 - s); the sum and the reciprocal: u s each)
  g = tanhf(x)                     e_g = 2u |g|
  c = f c_in + i g                 e_c = |c_in| e_f + |g| e_i + i e_g + u (|f c_in| + |i g| + |c|)
  h = o tanhf(c)                   e_h = |tanh c| e_o + o (2u |tanh c| + (1 - tanh^2 c) e_c) + u |h|
  h_next = h keep, c_next = c keep: the same bounds times keep; keep = 0 gives exact zeros.
Backward, against float64 autograd of the restated cell c = f c_in + i g, h = o tanh c at the float32 activated gates the
forward kernel wrote; the kernel reads the float32 c of the forward kernel, one evaluation of that c away:
  e_c = u (|f c_in| + |i g| + |c|),  tc = tanhf(c): e_tc = (1 - tc^2) e_c + 2u |tc|
  dh = d_out + dh_rec keep         e_dh = u |dh|
  1 - tc^2                         e_q = 2 |tc| e_tc + u tc^2 + u (1 - tc^2)      (the square, the difference)
  dc = dc_rec keep + dh o (1-tc^2) e_dc = |o (1 - tc^2)| e_dh + |dh o| e_q + 2u |dh o (1 - tc^2)| + u |dc|
  d i = dc g i (1 - i)             |g i (1 - i)| e_dc + 4u |d i|;   d f = dc c_in f (1 - f) alike
  d g = dc i (1 - g^2)             |i (1 - g^2)| e_dc + u |dc i| + 2u |d g|
  d o = dh tc o (1 - o)            |tc o (1 - o)| e_dh + |dh o (1 - o)| e_tc + 4u |d o|
  d c_in = dc f                    f e_dc + u |d c_in|"""
import ctypes as C

import pytest
import torch

from tests import pointwise_restate as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1, 1), (3, 5), (7, 37), (4, 64), (33, 100)]


def _lib():
    from rltime_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _within(what, got, want, bound):
    err = (got.cpu().double() - want).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print("RATIO %s: worst err / bound = %.3f" % (what, ratio))
    assert bool((err <= bound).all()), "%s: err / bound = %.3f" % (what, ratio)


def _fwd(pre, c_in, keep, outs=True):
    """-> (gates, h_out, c_out, h_next, c_next) on the device; buffers NaN-filled with a guard row."""
    L = _lib()
    B, H = c_in.shape
    gates = _nan(B + 1, 4 * H)
    gates[:B] = pre.float().cuda()
    cd = c_in.float().cuda()
    kd = keep.float().cuda() if keep is not None else None
    ho, co = (_nan(B + 1, H), _nan(B + 1, H)) if outs else (None, None)
    hn, cn = _nan(B + 1, H), _nan(B + 1, H)
    L.check(L.lib.mirl_lstm_cell_fwd(B, H, _p(gates), _p(cd), _p(kd), _p(ho), _p(co), _p(hn), _p(cn), _st()), "mirl_lstm_cell_fwd")
    torch.cuda.synchronize()
    for b in (gates, ho, co, hn, cn):
        assert b is None or bool(torch.isnan(b[B]).all()), "the guard row was written"
    return gates[:B], (ho[:B] if outs else None), (co[:B] if outs else None), hn[:B], cn[:B]


def _inputs(B, H, seed):
    g = torch.Generator().manual_seed(seed)
    pre = (torch.randn(B, 4 * H, generator=g) * 2).double()
    c_in = torch.randn(B, H, generator=g).double()
    keep = (torch.rand(B, generator=g) > 0.4).double()
    keep[0] = 0.0
    if B > 1:
        keep[1] = 1.0
    return g, pre, c_in, keep


@pytest.mark.parametrize("outs", [True, False], ids=["outs", "no-outs"])
@pytest.mark.parametrize("masked", [True, False], ids=["keep", "no-keep"])
@pytest.mark.parametrize("B,H", SHAPES)
def test_forward_against_float64(B, H, masked, outs):
    _, pre, c_in, keep = _inputs(B, H, 11 * B + H)
    keep = keep if masked else None
    gates, ho, co, hn, cn = _fwd(pre, c_in, keep, outs)
    wg, wh, wc, whn, wcn = R.lstm_cell_fwd(pre, c_in, keep)
    i, f, g, o = wg.chunk(4, dim=1)
    e_gates = torch.cat([4 * U * i, 4 * U * f, 2 * U * g.abs(), 4 * U * o], 1)
    _within("k_lstm_cell_fwd gates", gates, wg, e_gates)
    e_c = c_in.abs() * 4 * U * f + g.abs() * 4 * U * i + i * 2 * U * g.abs() + U * ((f * c_in).abs() + (i * g).abs() + wc.abs())
    tc = torch.tanh(wc)
    e_h = tc.abs() * 4 * U * o + o * (2 * U * tc.abs() + (1 - tc * tc) * e_c) + U * wh.abs()
    k = torch.ones(B, 1, dtype=torch.float64) if keep is None else keep.unsqueeze(1)
    _within("k_lstm_cell_fwd c_next", cn, wcn, e_c * k)
    _within("k_lstm_cell_fwd h_next", hn, whn, e_h * k)
    if outs:
        _within("k_lstm_cell_fwd c", co, wc, e_c)
        _within("k_lstm_cell_fwd h", ho, wh, e_h)
        assert torch.equal(hn, ho * k.float().cuda()) and torch.equal(cn, co * k.float().cuda())
    if masked:
        dead = keep == 0
        assert float(hn[dead.cuda()].abs().max()) == 0.0 and float(cn[dead.cuda()].abs().max()) == 0.0


def test_forward_saturates_without_nan():
    B, H = 3, 5
    pre = torch.full((B, 4 * H), 100.0, dtype=torch.float64)
    pre[1] = -100.0
    pre[2, ::2] = -100.0
    c_in = torch.full((B, H), 3.0, dtype=torch.float64)
    gates, ho, co, hn, cn = _fwd(pre, c_in, None)
    for t in (gates, ho, co, hn, cn):
        assert bool(torch.isfinite(t).all())
    lo = torch.cat([torch.zeros(B, 2 * H), -torch.ones(B, H), torch.zeros(B, H)], 1)
    assert torch.equal(gates.cpu(), torch.where(pre > 0, torch.ones(B, 4 * H), lo))    # exactly 1, and 0 / -1 (expf overflows to inf)
    assert torch.equal(co.cpu()[0], torch.full((H,), 4.0)) and torch.equal(co.cpu()[1], torch.zeros(H))
    # ... and the backward of saturated gates is exactly zero
    d = torch.randn(B, H, device="cuda")
    dc = torch.randn(B, H, device="cuda")
    dh = torch.randn(B, H, device="cuda")
    L = _lib()
    g2 = gates.clone().contiguous()
    L.check(L.lib.mirl_lstm_cell_bwd(B, H, _p(g2), _p(co.contiguous()), _p(c_in.float().cuda()), _p(d), _p(dh), _p(dc), None, 0, _st()), "mirl_lstm_cell_bwd")
    torch.cuda.synchronize()
    assert float(g2.abs().max()) == 0.0 and bool(torch.isfinite(dc).all())


@pytest.mark.parametrize("variant", ["full", "first", "no-d_out", "no-keep"])
@pytest.mark.parametrize("B,H", SHAPES)
def test_backward_against_float64_autograd_of_the_cell(B, H, variant):
    L = _lib()
    gen, pre, c_in, keep = _inputs(B, H, 13 * B + H)
    keep = None if variant == "no-keep" else keep
    first = variant == "first"
    gates, ho, co, _, _ = _fwd(pre, c_in, keep)
    d_out = None if variant == "no-d_out" else torch.randn(B, H, generator=gen).double()
    dh_rec, dc_rec = torch.randn(B, H, generator=gen).double(), torch.randn(B, H, generator=gen).double()
    ga = gates.cpu().double()                                             # what the forward kernel wrote
    ia, fa, gga, oa = ga.chunk(4, dim=1)
    c_t = fa * c_in + ia * gga                                            # the cell state of these gates in float64
    want_g, want_dc = R.lstm_cell_bwd(ga, c_t, c_in, d_out, dh_rec, dc_rec, keep, first)
    # float64 autograd of the restated cell at the same point: c and h as functions of (activated gates, c_in)
    gl, cl = ga.clone().requires_grad_(True), c_in.clone().requires_grad_(True)
    i, f, g, o = gl.chunk(4, dim=1)
    c = f * cl + i * g
    h = o * torch.tanh(c)
    k = torch.ones(B, 1, dtype=torch.float64) if keep is None else keep.unsqueeze(1)
    loss = (h * 0).sum() if d_out is None else (d_out * h).sum()
    if not first:
        loss = loss + (dh_rec * (h * k)).sum() + (dc_rec * (c * k)).sum()
    loss.backward()
    act_slope = torch.cat([ia * (1 - ia), fa * (1 - fa), 1 - gga * gga, oa * (1 - oa)], 1)
    assert float((want_g - gl.grad * act_slope).abs().max()) <= 1e-13 and float((want_dc - cl.grad).abs().max()) <= 1e-13
    # the kernel
    gd = _nan(B + 1, 4 * H)
    gd[:B] = gates
    dcd = _nan(B + 1, H)
    dcd[:B] = dc_rec.float().cuda()
    if first:
        dcd[:B] = float("nan")                                            # never read
    dd = d_out.float().cuda() if d_out is not None else None
    dhd = None if first else dh_rec.float().cuda()
    kd = keep.float().cuda() if keep is not None else None
    L.check(L.lib.mirl_lstm_cell_bwd(B, H, _p(gd), _p(co.contiguous()), _p(c_in.float().cuda()), _p(dd), _p(dhd), _p(dcd), _p(kd), int(first), _st()),
            "mirl_lstm_cell_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(gd[B]).all()) and bool(torch.isnan(dcd[B]).all()), "the guard row was written"
    zero = torch.zeros(B, H, dtype=torch.float64)
    dh = (zero if d_out is None else d_out) + (zero if first else dh_rec * k)
    tc = torch.tanh(c_t)
    q = 1 - tc * tc
    e_dh = U * dh.abs()
    e_c = U * ((fa * c_in).abs() + (ia * gga).abs() + c_t.abs())
    assert bool(((co.cpu().double() - c_t).abs() <= e_c).all())
    e_tc = q * e_c + 2 * U * tc.abs()
    e_q = 2 * tc.abs() * e_tc + U * tc * tc + U * q
    dc = (zero if first else dc_rec * k) + dh * oa * q
    e_dc = (oa * q).abs() * e_dh + (dh * oa).abs() * e_q + 2 * U * (dh * oa * q).abs() + U * dc.abs()
    wi, wf, wg_, wo = want_g.chunk(4, dim=1)
    bound = torch.cat([(gga * ia * (1 - ia)).abs() * e_dc + 4 * U * wi.abs(),
                       (c_in * fa * (1 - fa)).abs() * e_dc + 4 * U * wf.abs(),
                       (ia * (1 - gga * gga)).abs() * e_dc + U * (dc * ia).abs() + 2 * U * wg_.abs(),
                       (tc * oa * (1 - oa)).abs() * e_dh + (dh * oa * (1 - oa)).abs() * e_tc + 4 * U * wo.abs()], 1)
    _within("k_lstm_cell_bwd gates", gd[:B], want_g, bound)
    _within("k_lstm_cell_bwd dc_rec", dcd[:B], want_dc, fa * e_dc + U * want_dc.abs())
    if keep is not None and not first and d_out is None:
        dead = (keep == 0).cuda()
        assert float(gd[:B][dead].abs().max()) == 0.0 and float(dcd[:B][dead].abs().max()) == 0.0   # nothing flows through a reset


def test_entry_points_refuse_bad_arguments():
    L = _lib()
    x = torch.zeros(64, device="cuda")
    P, st = _p(x), _st()
    fwd = [2, 2, P, P, None, None, None, P, P, st]
    for pos, bad in [(0, 0), (1, 0), (0, -1), (2, None), (3, None), (7, None), (8, None)]:
        a = list(fwd)
        a[pos] = bad
        assert L.lib.mirl_lstm_cell_fwd(*a) == -1, pos
    bwd = [2, 2, P, P, P, None, P, P, None, 0, st]
    for pos, bad in [(0, 0), (1, -3), (2, None), (3, None), (4, None), (7, None), (6, None)]:
        a = list(bwd)
        a[pos] = bad
        assert L.lib.mirl_lstm_cell_bwd(*a) == -1, pos
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0
