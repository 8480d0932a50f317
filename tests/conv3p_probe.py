"""Part-probing operands for the three-plane input layer (csrc/conv_in_rows.hip), in the manner of tests/conv1p_probe.py: a
uint8 pixel is exact in ONE bf16 part, the other operand (w * scale in the forward, g in the weight gradient) is split three
ways, so hi.x, mid.x and lo.x are all the products there are.  The operands below populate all three parts at EVERY element
of the split operand, with every part positive in the element's unit, and stay exact in f32 in any summation order: float64
is the one right answer bit for bit, and an output that loses, misplaces or mispairs a part cannot equal it.

The lattice density, re-derived for 192 taps.  A weight's three parts sum to less than 2^20 + 2^12 + 2^4 in absolute value
(a 20-bit integer).  The one-plane probe lights four pixels of 1..3 per 8 x 8 window: 12 such weights and a bias below 2^20.
Three planes at that density would be 36 — past 2^24 = 16 * 2^20.  So each plane's lattice here has period (8, 4): exactly
TWO lit pixels per 8 x 8 window and plane, six per output over the three planes, and a lit pixel is 1 or 2:
  |output| <= 6 * 2 * (2^20 + 2^12 + 2^4) + 2^20 = 13.05 * 2^20 < 2^24 in the filter's unit.
The weight gradient's contraction runs over positions, not taps, so the one-plane derivation stands as it is: five wide g
values per filter and pixels 0..3, at most 15 (2^20 + 2^12 + 2^4) < 2^24 per weight.

tests/test_conv3p_probe_cpu.py proves these properties without a GPU; tests/test_conv3p_gpu.py sends the same operands
through the kernels.  A plain module, imported by both."""
import torch
import torch.nn.functional as F

from tests.conv1p_probe import LIMIT, PIXEL_PRODUCTS, emulate, wide
from tests.split3_probe import _choose, _lattice, _pow2, emulate_gemm, split3

PLANES, TAPS = 3, 192
LIT_PER_OUTPUT, LIT_MAX = 6, 2
FWD_BOUND = LIT_PER_OUTPUT * LIT_MAX * (2 ** 20 + 2 ** 12 + 2 ** 4) + 2 ** 20
WRW_BOUND = 15 * (2 ** 20 + 2 ** 12 + 2 ** 4)

# flappy: configs/flappy_iqn_lstm_rgb.json's frames (551 positions = 34 tiles of 16 and 7 more)
FWD_CASES = {"flappy": (2, 120, 80), "small": (5, 44, 52), "many_frames": (1025, 36, 36)}


def fwd_case(name):
    """relu(conv2d(x, W, b, 4)), scale 1: every weight wide (a signed power-of-two unit per filter), the bias below 2^20 in
    that unit; each plane of the image is zero except 1..2 on a lattice of period (8, 4) whose offset is drawn per frame
    AND plane — exactly two positions per 8 x 8 window and plane: at most FWD_BOUND < 2^24 per output, in the filter's unit."""
    n, h, w = FWD_CASES[name]
    gen = torch.Generator().manual_seed(27000 + n + h + w)
    wt = wide(gen, (32, PLANES, 8, 8))
    unit = _pow2(gen, (32,), 20)
    lit = _lattice(gen, n * PLANES, h, w, 8, 4).view(n, PLANES, h, w)
    x = (torch.randint(1, LIT_MAX + 1, (n, PLANES, h, w), generator=gen).float() * lit).to(torch.uint8)
    bias = torch.randint(-2 ** 20 + 1, 2 ** 20, (32,), generator=gen).float()
    return {"x": x, "w": wt * unit.view(32, 1, 1, 1), "bias": bias * unit, "w_int": wt, "bias_int": bias, "unit": unit}


WRW_CASES = {"flappy": (2, 120, 80), "small": (2, 44, 52), "tiny": (3, 8, 8)}


def op_wrw(g, x):
    """dW[f, c, kh, kw] = sum over (n, oh, ow) of g[n, f, oh, ow] x[n, c, 4 oh + kh, 4 ow + kw], bilinear in (g, x)"""
    cols = F.unfold(x.contiguous(), 8, stride=4)                                       # (n, 192, positions), rows (c, kh, kw)
    return torch.einsum("nfp,ntp->ft", g.reshape(g.shape[0], g.shape[1], -1), cols).view(g.shape[1], PLANES, 8, 8)


def wrw_case(name):
    """dW = sum over positions of g x (scale 1): g wide at FIVE positions per filter (all of them where the case has fewer; a
    signed power-of-two unit per filter), zero elsewhere; pixels 0..3 everywhere: at most WRW_BOUND < 2^24 per weight.  `y` is
    a forward activation whose planted mask drops exactly ONE of each filter's positions (and is random where g is zero
    anyway).  Where all the pixels one weight sees at its filter's KEPT positions came out zero, one of them is raised to
    1..3, so that every weight of both the plain and the masked gradient depends on g."""
    n, h, w = WRW_CASES[name]
    gen = torch.Generator().manual_seed(28000 + n + h + w)
    oh, ow = (h - 8) // 4 + 1, (w - 8) // 4 + 1
    P = n * oh * ow
    pick = _choose(gen, 32, P, 5)                                                       # (32, P) 0/1
    drop = torch.zeros(32, P)
    for f in range(32):
        live = pick[f].nonzero().flatten()
        drop[f, live[int(torch.randint(0, len(live), (1,), generator=gen))]] = 1.0
    to_nchw = lambda t: t.view(32, n, oh, ow).permute(1, 0, 2, 3).contiguous()          # noqa: E731
    pick, drop = to_nchw(pick), to_nchw(drop)
    g_int = wide(gen, (n, 32, oh, ow)) * pick
    unit = _pow2(gen, (1, 32, 1, 1), 20)
    x = torch.randint(0, 4, (n, PLANES, h, w), generator=gen).float()
    y = (torch.rand(n, 32, oh, ow, generator=gen) - 0.2).clamp(min=0)
    y = torch.where(pick > 0, 1.0 - drop, y)                                            # planted: one of the positions masked out
    kept = pick * (1.0 - drop)
    blind = (op_wrw(kept, (x > 0).float()) == 0).nonzero()                              # (f, c, kh, kw) that see only zero pixels
    for f, c, kh, kw in blind.tolist():
        i, _, a, b = kept[:, f:f + 1].nonzero()[0].tolist()
        if float(x[i, c, 4 * a + kh, 4 * b + kw]) == 0:                                 # (an earlier raise may have reached it)
            x[i, c, 4 * a + kh, 4 * b + kw] = float(1 + (kh + kw) % 3)
    return {"x": x.to(torch.uint8), "g": g_int * unit, "g_int": g_int, "y": y, "kept": kept, "unit": unit.view(32)}


# ---- the method on the CPU ----------------------------------------------------------------------------------------------------

def fwd_terms(c, frames):
    """every term one output of the forward sums — 3 parts x 192 taps and the bias — for the given frames: (T, n, 32, positions)"""
    cols = F.unfold(c["x"][frames].float(), 8, stride=4)                                # (n, 192, positions)
    parts = torch.stack(split3(c["w"].view(32, TAPS)))                                  # (3, 32, 192)
    t = torch.einsum("pfk,nkq->pknfq", parts, cols).reshape(3 * TAPS, cols.shape[0], 32, cols.shape[2])
    return torch.cat([t, c["bias"].view(1, 1, 32, 1).expand(1, cols.shape[0], 32, cols.shape[2])])


def wrw_terms(g, x):
    """every term one weight of the gradient sums — 3 parts x all positions: (T, 32, 192)"""
    cols = F.unfold(x.float(), 8, stride=4)                                             # (n, 192, positions)
    parts = torch.stack(split3(g.reshape(g.shape[0], 32, -1)))                          # (3, n, 32, positions)
    return torch.einsum("pnfq,nkq->pnqfk", parts, cols).reshape(-1, 32, TAPS)


__all__ = ["FWD_CASES", "WRW_CASES", "FWD_BOUND", "WRW_BOUND", "LIMIT", "PIXEL_PRODUCTS", "fwd_case", "wrw_case", "op_wrw", "emulate",
           "fwd_terms", "wrw_terms", "wide", "emulate_gemm"]
