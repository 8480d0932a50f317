"""GPU: the acting network's kernels (csrc/actnet.hip) at their C entry points against the float64 layers of
tests/pointwise_restate.py (equal to torch in float64: tests/test_pointwise_restate_cpu.py), on every launch path.

Dyadic operands (integers times a power of two, the largest possible |partial sum| below 2^24 units, asserted by the
generators' margins): every product and every partial sum is a float32 number, so the kernels must equal float64 bit for
bit — torch.equal on whole blocks, no tolerance, nothing left out.  Outputs are NaN-filled with padding and guard rows that
must stay NaN.

Real operands, first order, u = 2^-24, one 16x16x4 MFMA counted as four additions (so a K-long accumulator is K additions):
  conv (k_act_conv RT = 1, RT = 2, k_act_conv_wlds alike: one accumulator per output over K = 512 / 576, then the bias)
      e_y = (K + 1) u (sum |x w| + |b|)
  LSTM step: a wave adds ceil(SPB / 8) 16-wide steps, 8 waves meet in LDS, KB shares and the bias are added by the cell
      e_pre = (16 ceil(SPB / 8) + 8 + KB + 1) u (sum |x w| + |b|)
      sigmoid s = 1 / (1 + expf(-x)): e_s = 4u s + s (1 - s) e_pre;  g = tanhf(x): e_g = 2u |g| + (1 - g^2) e_pre
      c = f c_in + i g     e_c = |c_in| e_f + |g| e_i + i e_g + u (|f c_in| + |i g| + |c|)
      h = o tanhf(c)       e_h = |tanh c| e_o + o (2u |tanh c| + (1 - tanh^2 c) e_c) + u |h|
      (tests/test_lstm_cell_gpu.py's forward bounds; with dyadic xh, w, bias e_pre = 0: no slack for the product)
  quantile embedding: a = float32(freq tau), phi = cosf(a) within 1 ulp
      e_phi = 2u |cos a| + u |a sin a|
      e_pre = sum_i |wq_i| e_phi_i + (D + 1) u (sum_i |phi_i wq_i| + |bq|)
      x = relu(pre) h      e_x = |h| e_pre + u |x|;   x is exactly 0 where the float64 pre < -e_pre
  hidden layers: hid = relu(x wfc^T + bfc)   e_hid = (H + 1) u (sum |x wfc| + |bfc|)
      share cb: a wave adds its 32 columns (8 MFMAs), the two column halves add: 33 additions
      e_share = sum_j |wout_j| e_hid_j + 33 u sum_j |hid_j wout_j|;   the sum of the shares (added here in float64): sum_cb e_share
  selection: o = bout + P shares  e_o = P u (|bout| + sum_p |share|), then k_actor_head's bounds (tests/test_actor_head_gpu.py)
      with e_o carried: m = sum_a o_a  e_m = sum_a e_o + (A - 1) u sum_a |o_a|;  off = V - m / A  e_off = e_o(V) + e_m / A + u |m| / A + u |off|
      t = o_a + off  e_t = e_o + e_off + u |t| (plain head: e_t = e_o);  q = (sum_n t) / N  e_q = (sum_n e_t + (ceil(N / 64) + 6) u sum_n |t|) / N + u |q|
      actions compared where the float64 top two are further apart than their bounds together; at most 10 % of the envs left out.
Worst err / bound measured on an MI355X: conv 0.010 (RT = 1 and 2), 0.008 (LDS weights); LSTM 0.55 with dyadic products (the
cell's own bound), 0.008 with real ones; embedding 0.29; hidden shares 0.005; selection 0.05."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import actnet_conv_driver as CD
from tests import pointwise_restate as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from rltime_amd import _lib
    return _lib


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _within(what, got, want, bound):
    err = (got.cpu().double() - want).abs()
    assert not bool(torch.isnan(err).any()), "%s: NaN" % what
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print("RATIO %s: worst err / bound = %.3f" % (what, ratio))
    assert bool((err <= bound).all()), "%s: err / bound = %.3f" % (what, ratio)


# ---- 1. conv layers 2 and 3 ------------------------------------------------------------------------------------------------------
# M = frames * Ho * Wo; layer 2: Ho = (Hi - 4) / 2 + 1, layer 3: Ho = Hi - 2.  M < 6144: k_act_conv<RT = 1>, ceil(M / 16) workgroups.
#   (1, 4, 4) / (1, 3, 3): Ho = Wo = 1, M = 1: every lane clamped to the one pixel;  (17, ..): M = 17, a second, nearly empty tile
#   (3, 6, 12), (3, 12, 6): 2 x 5 and 5 x 2 output pixels;  (3, 5, 9), (3, 9, 5): 3 x 7 and 7 x 3 — Hi / Wi, Ho / Wo mix-ups show
#   (75, 20, 20): M = 75 * 81 = 6075;  (125, 9, 9): M = 125 * 49 = 6125: just below the 6144 threshold
PLAIN = [(2, 1, 4, 4), (2, 17, 4, 4), (2, 3, 6, 12), (2, 3, 12, 6), (2, 1, 20, 20), (2, 75, 20, 20),
         (3, 1, 3, 3), (3, 17, 3, 3), (3, 3, 5, 9), (3, 3, 9, 5), (3, 125, 9, 9)]
# M >= 6144: k_act_conv_wlds, grid = min(ceil(tiles / 4), CUs), 4 tile slots per workgroup.
#   (76, 20, 20): M = 6156, 385 tiles = 96 workgroups x 4 + 1: the last workgroup has three idle slots and a partial tile
#   (203, 20, 20): M = 16443, 1028 tiles, 257 > 256 CUs: the grid is capped and a slot takes a second tile
#   (38, 20, 38): 9 x 18 outputs, M = 6156;  (126, 9, 9): M = 6174, 386 tiles;  (335, 9, 9): M = 16415, 1026 tiles, capped
#   (64, 9, 16): 7 x 14 outputs, M = 6272
WLDS = [(2, 76, 20, 20), (2, 203, 20, 20), (2, 38, 20, 38), (3, 126, 9, 9), (3, 335, 9, 9), (3, 64, 9, 16)]


def _conv_out(layer, Hi, Wi):
    k, s = (4, 2) if layer == 2 else (3, 1)
    return (Hi - k) // s + 1, (Wi - k) // s + 1


@pytest.mark.parametrize("layer,frames,Hi,Wi", PLAIN + WLDS, ids=lambda v: str(v))
def test_conv_dyadic_is_bit_equal_to_float64(layer, frames, Hi, Wi):
    Ho, Wo = _conv_out(layer, Hi, Wi)
    M = frames * Ho * Wo
    assert (M >= 6144) == ((layer, frames, Hi, Wi) in WLDS)
    bad, zeros, neg, n = CD.dyadic_mismatches(layer, frames, Hi, Wi, 4000 + 7 * frames + Hi)
    assert zeros >= 1 and neg >= 1 and (M < 64 or zeros >= n // 200), "the bias plants no visible share of zeros"
    assert bad == 0, "%d of %d outputs differ from float64 (or are -0)" % (bad, n)


@pytest.mark.parametrize("layer,frames,Hi,Wi", [(2, 3, 12, 6), (3, 3, 9, 5), (2, 38, 20, 38), (3, 64, 9, 16)], ids=lambda v: str(v))
def test_conv_real_within_the_operation_count_bound(layer, frames, Hi, Wi):
    ratio = CD.real_ratio(layer, frames, Hi, Wi, 4300 + frames)
    Ho, Wo = _conv_out(layer, Hi, Wi)
    print("RATIO k_act_conv%s layer %d: worst err / bound = %.3f" % ("_wlds" if frames * Ho * Wo >= 6144 else "<RT=1>", layer, ratio))
    assert ratio <= 1.0


def test_conv_rt2_in_a_process_with_the_lds_kernel_switched_off():
    """k_act_conv<.., RT = 2>, both layers: only reachable with MIRL_ACT_CONV_WLDS=0 (read once per process) and M > 8192."""
    env = dict(os.environ, MIRL_ACT_CONV_WLDS="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "actnet_conv_driver.py")], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for layer, frames, _, _ in CD.RT2_SHAPES:
        assert "RT2 layer %d frames %d: 0 of " % (layer, frames) in p.stdout
        assert "RATIO k_act_conv<RT=2> layer %d real" % layer in p.stdout


# ---- 2. LSTM step ----------------------------------------------------------------------------------------------------------------
def _lstm_slices(H, K):
    """(KB, SPB) of the launch: KB = min(256 / (H / 8), 16, steps / 8) slices of SPB = ceil(steps / KB) steps, then only the
    ceil(steps / SPB) slices that hold a step."""
    steps = K // 16
    kb = max(1, min(256 // (H // 8), 16, steps // 8))
    spb = -(-steps // kb)
    return -(-steps // spb), spb, kb


# (E, H, Fin), K = Fin + H, steps = K / 16; RT = 1 / 2 / 4 at E <= 16 / 32 / 64
LSTM_OLD = [(16, 64, 3136), (32, 512, 3136), (7, 64, 48), (33, 64, 3136), (64, 512, 3136), (48, 128, 16), (32, 8, 8)]
# an empty trailing slice before the fix:  K = 1296: 81 steps, 10 slices of 9, slice 9 starts at 81;  K = 1424: 89 steps, 11 of 9,
# slice 10 starts at 90;  K = 3360: 210 steps, 16 of 14, slice 15 starts at 210
LSTM_EMPTY = [(1, 8, 1288), (20, 64, 1360), (40, 128, 3232)]
# KB > 1 and no empty slice, one per RT: K = 3200: 200 steps, 16 slices of 13 (the last holds 5);  K = 3648, H = 512: 228 steps, 4 of
# 57;  K = 2048: 128 steps, 16 of 8.  The last two divide evenly, so each RT also gets a ragged last slice:  K = 3664, H = 512: 229
# steps, 4 of 58 (the last holds 55);  K = 2176: 136 steps, 16 of 9 (the last holds 1)
LSTM_SLICED = [(16, 64, 3136), (17, 512, 3136), (64, 64, 1984)]
LSTM_RAGGED = [(16, 64, 3136), (17, 512, 3152), (64, 64, 2112)]


def _lstm_run(xh, w, b, c_in, pad=20):
    """Three launches over one zeroed workspace -> [(h, c)] on the CPU.  xh sits in a NaN buffer `pad` floats wider than K with a
    NaN row behind it; w and bias are each followed by a NaN row; h and c have a NaN guard row."""
    L = _lib()
    E, K = xh.shape
    H = c_in.shape[1]
    pitch = K + pad
    xb = _nan(E + 1, pitch)
    xb[:E, :K] = xh.float().cuda()
    wb = _nan(4 * H + 1, K)
    wb[:4 * H] = w.float().cuda()
    bb = _nan(2, 4 * H)
    bb[0] = b.float().cuda()
    cd = c_in.float().cuda()
    assert L.lib.mirl_act_lstm_supported(E, H, K) == 1
    need = C.c_int64()
    L.check(L.lib.mirl_act_lstm_workspace_bytes(E, H, K, C.byref(need)))
    ws = torch.zeros((need.value + 3) // 4, dtype=torch.int32, device="cuda")
    outs = []
    for _ in range(3):
        h, c = _nan(E + 1, H), _nan(E + 1, H)
        L.check(L.lib.mirl_act_lstm_fwd(E, H, K, _p(xb), pitch, _p(wb), _p(bb), _p(cd), _p(h), _p(c), _p(ws), _st()), "mirl_act_lstm_fwd")
        torch.cuda.synchronize()
        assert bool(torch.isnan(h[E]).all()) and bool(torch.isnan(c[E]).all()), "the guard row was written"
        outs.append((h[:E].cpu(), c[:E].cpu()))
    return outs


def _lstm_check(what, outs, pre, e_pre, c_in):
    for h, c in outs:
        assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(c).all()), "%s: %d non-finite outputs" % (
            what, int((~torch.isfinite(h)).sum() + (~torch.isfinite(c)).sum()))
    for h, c in outs[1:]:                                             # the arrival counters are back at zero: the same sums again
        assert torch.equal(h, outs[0][0]) and torch.equal(c, outs[0][1])
    gates, wh, wc, _, _ = R.lstm_cell_fwd(pre, c_in)
    i, f, g, o = gates.chunk(4, dim=1)
    pi, pf, pg, po = e_pre.chunk(4, dim=1)
    e_i, e_f, e_o = 4 * U * i + i * (1 - i) * pi, 4 * U * f + f * (1 - f) * pf, 4 * U * o + o * (1 - o) * po
    e_g = 2 * U * g.abs() + (1 - g * g) * pg
    e_c = c_in.abs() * e_f + g.abs() * e_i + i * e_g + U * ((f * c_in).abs() + (i * g).abs() + wc.abs())
    tc = torch.tanh(wc)
    e_h = tc.abs() * e_o + o * (2 * U * tc.abs() + (1 - tc * tc) * e_c) + U * wh.abs()
    _within(what + " c", outs[0][1], wc, e_c)
    _within(what + " h", outs[0][0], wh, e_h)


@pytest.mark.parametrize("E,H,Fin", LSTM_OLD + LSTM_EMPTY + LSTM_SLICED[1:] + LSTM_RAGGED[1:], ids=lambda v: str(v))
def test_lstm_step_dyadic_products_are_exact(E, H, Fin):
    K = Fin + H
    KB, SPB, kb0 = _lstm_slices(H, K)
    assert (KB - 1) * SPB < K // 16 <= KB * SPB
    assert ((kb0 - 1) * SPB >= K // 16) == ((E, H, Fin) in LSTM_EMPTY)
    assert (E, H, Fin) not in LSTM_SLICED + LSTM_RAGGED or KB > 1
    assert (E, H, Fin) not in LSTM_RAGGED or K // 16 < KB * SPB
    d = R.dyadic_lstm(5000 + E + H + Fin, E, H, K)
    assert d["margin"] < 2 ** 24
    pre = R.linear(d["xh"], d["w"], d["b"])
    assert torch.equal(pre.float().double(), pre)
    _lstm_check("k_act_lstm dyadic", _lstm_run(d["xh"], d["w"], d["b"], d["c_in"]), pre, torch.zeros_like(pre), d["c_in"])


@pytest.mark.parametrize("E,H,Fin", LSTM_SLICED, ids=lambda v: str(v))
def test_lstm_step_real_within_the_operation_count_bound(E, H, Fin):
    K = Fin + H
    KB, SPB, _ = _lstm_slices(H, K)
    g = torch.Generator().manual_seed(5100 + E)
    xh = (torch.randn(E, K, generator=g) * 0.3).double()
    w = (torch.randn(4 * H, K, generator=g) / np.sqrt(K)).double()
    b = (torch.randn(4 * H, generator=g) * 0.1).double()
    c_in = (torch.randn(E, H, generator=g) * 0.5).double()
    pre = R.linear(xh, w, b)
    chain = 16 * -(-SPB // 8) + 8 + KB + 1
    e_pre = chain * U * R.linear(xh.abs(), w.abs(), b.abs())
    _lstm_check("k_act_lstm<RT=%d> real" % (1 if E <= 16 else 2 if E <= 32 else 4), _lstm_run(xh, w, b, c_in), pre, e_pre, c_in)


# ---- 3. quantile embedding -------------------------------------------------------------------------------------------------------
def _embed_run(E, N, H, D, h, freq, taus, wq, bq, seed=99, step=5):
    """-> (x (R, H), tau_out (R,)) on the CPU; both sit between NaN guard rows."""
    L = _lib()
    Rr = E * N
    x, to = _nan(Rr + 2, H), _nan(Rr + 2)
    sd = torch.tensor([step], dtype=torch.int64, device="cuda")
    hd, fd, wd, bd = h.float().cuda().contiguous(), freq.cuda(), wq.float().cuda().contiguous(), bq.float().cuda()
    td = taus.cuda() if taus is not None else None
    L.check(L.lib.mirl_act_embed(E, N, H, D, _p(hd), _p(fd), _p(td), seed, _p(sd), _p(wd), _p(bd), _p(x, H), _p(to, 1), _st()), "mirl_act_embed")
    torch.cuda.synchronize()
    for buf in (x, to):
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[Rr + 1]).all()), "a guard row was written"
    return x[1:Rr + 1].cpu(), to[1:Rr + 1].cpu()


def _embed_operands(E, N, H, D, seed):
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(E, H, generator=g) * 0.5).double()
    taus = torch.rand(E * N, generator=g)
    freq = (torch.arange(1, D + 1, dtype=torch.float32) * np.pi).contiguous()
    wq = (torch.randn(H, D, generator=g) / np.sqrt(D)).double()
    bq = (torch.randn(H, generator=g) * 0.1).double()
    return h, taus, freq, wq, bq


# (E, N, H, D): tiles = ceil(R / 16), ycount = ceil(H / 128); groups doubles while (tiles / (2 groups)) * ycount >= 512.
#   (3, 5, 48, 32): H % 32 = 16: the wave that holds columns 32 .. 47 has no second column tile (on1 false)
#   (2, 7, 80, 48): waves 0, 1 full, wave 2 half, wave 3 without columns;  (5, 7, 128, 64): R = 35, a partial last tile
#   (257, 32, 512, 64): R = 8224, 514 tiles, ycount 4: groups = 4, 129 workgroups per column block; 514 % 4 = 2: the last one
#                       breaks out after two groups (row0 >= R)
#   (263, 31, 512, 64): R = 8153, 510 tiles: (510 / 4) * 4 = 508 < 512, groups = 2; the last workgroup's second group is partial (9 rows)
#   (265, 31, 512, 64): R = 8215, 514 tiles, groups = 4, R % 16 = 7: the last workgroup takes a full group, a partial one, and breaks
EMBED = [(1, 1, 16, 16), (3, 5, 48, 32), (2, 7, 80, 48), (5, 7, 128, 64), (257, 32, 512, 64), (263, 31, 512, 64), (265, 31, 512, 64)]


def _embed_groups(E, N, H):
    tiles, ycount, groups = -(-E * N // 16), -(-H // 128), 1
    while groups < 8 and (tiles // (2 * groups)) * ycount >= 512:
        groups *= 2
    return groups, tiles


@pytest.mark.parametrize("E,N,H,D", EMBED, ids=lambda v: str(v))
def test_embed_against_float64_within_the_cos_and_chain_bound(E, N, H, D):
    groups, tiles = _embed_groups(E, N, H)
    assert groups == {257: 4, 263: 2, 265: 4}.get(E, 1) and (groups == 1 or tiles % 4 == 2)
    h, taus, freq, wq, bq = _embed_operands(E, N, H, D, 6000 + E + N)
    x, tau_out = _embed_run(E, N, H, D, h, freq, taus, wq, bq)
    assert torch.equal(tau_out, taus)
    t64, f64 = taus.double(), freq.double()
    arg = f64.unsqueeze(0) * t64.unsqueeze(1)
    phi, pre = R.cos_embed_pre(t64, f64, wq, bq)
    e_phi = 2 * U * phi.abs() + U * (arg * torch.sin(arg)).abs()
    e_pre = R.linear(e_phi, wq.abs()) + (D + 1) * U * R.linear(phi.abs(), wq.abs(), bq.abs())
    hr = h.repeat_interleave(N, dim=0)
    want = R.cos_embed_product(t64, f64, wq, bq, h, N)
    _within("k_act_embed x", x, want, hr.abs() * e_pre + U * want.abs())
    dead = pre < -e_pre
    assert int(dead.sum()) > 0 or x.numel() < 256
    assert float(x[dead].abs().sum()) == 0.0


@pytest.mark.parametrize("E,N,H,D", [(3, 5, 48, 32), (265, 31, 512, 64)], ids=lambda v: str(v))
def test_embed_draws_the_fractions_it_would_be_handed(E, N, H, D):
    """taus NULL (R % 16 != 0): tau_out = the 24-bit Philox uniform of (seed ^ 0x7A5, step, row), x bit-equal to the run handed them."""
    h, _, freq, wq, bq = _embed_operands(E, N, H, D, 6100 + E)
    x1, t1 = _embed_run(E, N, H, D, h, freq, None, wq, bq, seed=1234, step=11)
    assert float(t1.min()) >= 0.0 and float(t1.max()) < 1.0
    for m in (0, 1, E * N // 2, E * N - 1):
        assert float(t1[m]) == (R.philox_4x32(1234 ^ 0x7A5, 11, m)[0] >> 8) / 16777216.0
    x2, t2 = _embed_run(E, N, H, D, h, freq, t1, wq, bq, seed=1234, step=11)
    assert torch.equal(t2, t1) and torch.equal(x2, x1)


# ---- 4. hidden layers and output shares ------------------------------------------------------------------------------------------
def _hidden_run(Rr, H, HID, NO, x, wfc, bfc, wout):
    """-> part (P, R, pitch) on the CPU: columns NO .. pitch - 1 and a guard block behind the P shares must stay NaN."""
    L = _lib()
    parts, pitch = C.c_int32(), C.c_int32()
    L.check(L.lib.mirl_act_head_parts(HID, NO, C.byref(parts), C.byref(pitch)))
    P, NOP = parts.value, pitch.value
    assert P == -(-HID // 64) and NOP == -(-NO // 8) * 8
    assert L.lib.mirl_act_head_supported(Rr, 1, H, 0, HID, NO) == 1
    part = _nan(P + 1, Rr, NOP)
    xd, wd, bd, od = (t.float().cuda().contiguous() for t in (x, wfc, bfc, wout))
    L.check(L.lib.mirl_act_head_hidden(Rr, H, HID, NO, _p(xd), _p(wd), _p(bd), _p(od), _p(part), _st()), "mirl_act_head_hidden")
    torch.cuda.synchronize()
    part = part.cpu()
    assert bool(torch.isnan(part[P]).all()), "the guard block was written"
    assert NOP == NO or bool(torch.isnan(part[:P, :, NO:]).all()), "the padding columns were written"
    return part[:P, :, :NO]


def _hidden_variant(Rr, H, HID):
    """(WR, HP): WR = 2 when ceil(R / 32) * ceil(HID / 64) > 384; HP = H / 64 passes of four K steps."""
    return (2 if -(-Rr // 32) * -(-HID // 64) > 384 else 1), H // 64


# (R, H, HID, NO) -> k_act_hidden<WR, HP>:
#   (1, 64, 16, 1) <1, 1>: one row, one quarter of a column block;  (33, 128, 80, 7) <1, 2>: HID % 64 = 16: a wave with one column tile
#   (40, 256, 272, 19) <1, 4>;  (70, 1024, 64, 31) <1, 16>;  (200, 512, 1024, 9) <1, 8>: 7 * 16 = 112 workgroups
#   (3100, 256, 256, 12) <2, 4>: ceil(3100 / 32) * 4 = 388 > 384, R % 64 = 28;  (1000, 64, 1024, 7) <2, 1>: 32 * 16 = 512 > 384
HIDDEN = [(1, 64, 16, 1, (1, 1)), (33, 128, 80, 7, (1, 2)), (40, 256, 272, 19, (1, 4)), (70, 1024, 64, 31, (1, 16)),
          (200, 512, 1024, 9, (1, 8)), (3100, 256, 256, 12, (2, 4)), (1000, 64, 1024, 7, (2, 1))]


@pytest.mark.parametrize("Rr,H,HID,NO,variant", HIDDEN, ids=lambda v: str(v))
def test_hidden_dyadic_shares_are_bit_equal_to_float64(Rr, H, HID, NO, variant):
    assert _hidden_variant(Rr, H, HID) == variant
    d = R.dyadic_hidden(7000 + Rr + HID, Rr, H, HID, NO)
    assert d["margin"] < 2 ** 24
    hid, shares = R.head_shares(d["x"], d["wfc"], d["bfc"], d["wout"])
    assert hid.numel() < 1000 or 0.2 < float((hid == 0).double().mean()) < 0.8
    part = _hidden_run(Rr, H, HID, NO, d["x"], d["wfc"], d["bfc"], d["wout"])
    assert torch.equal(part, shares.float()), "%d share elements differ" % int((part != shares.float()).sum())
    assert torch.equal(part.sum(0), R.linear(hid, d["wout"]).float())


@pytest.mark.parametrize("Rr,H,HID,NO,variant", [HIDDEN[4], HIDDEN[6]], ids=lambda v: str(v))
def test_hidden_real_within_the_operation_count_bound(Rr, H, HID, NO, variant):
    assert _hidden_variant(Rr, H, HID) == variant
    g = torch.Generator().manual_seed(7100 + Rr)
    x = (torch.randn(Rr, H, generator=g) * 0.5).double()
    wfc, bfc = (torch.randn(HID, H, generator=g) / np.sqrt(H)).double(), (torch.randn(HID, generator=g) * 0.1).double()
    wout = (torch.randn(NO, HID, generator=g) / np.sqrt(HID)).double()
    hid, shares = R.head_shares(x, wfc, bfc, wout)
    e_hid = (H + 1) * U * R.linear(x.abs(), wfc.abs(), bfc.abs())
    carried = torch.stack([e_hid[:, c:c + 64] @ wout[:, c:c + 64].abs().t() for c in range(0, HID, 64)])
    mag = torch.stack([hid[:, c:c + 64] @ wout[:, c:c + 64].abs().t() for c in range(0, HID, 64)])
    e_share = carried + 33 * U * mag
    part = _hidden_run(Rr, H, HID, NO, x, wfc, bfc, wout)
    _within("k_act_hidden<WR=%d> shares" % variant[0], part, shares, e_share)
    _within("k_act_hidden<WR=%d> sum of shares" % variant[0], part.double().sum(0), R.linear(hid, wout), e_share.sum(0))


# ---- 5. selection ----------------------------------------------------------------------------------------------------------------
def _select_run(E, N, A, has_val, parts, bout, eps=None, expo=None, eps_min=0.0, seed=99, step=5, cross=False):
    """parts (P, E * N, NO) float64 -> (actions, qvalues) on the CPU.  The shares sit `pitch` floats apart with NaN padding.
    cross: also (actions, qvalues, eps_used) of mirl_actor_head_rng on out = sum of the shares + bout."""
    L = _lib()
    P, Rr, NO = parts.shape
    pitch = -(-NO // 8) * 8
    part = _nan(P, Rr, pitch)
    part[:, :, :NO] = parts.float().cuda()
    bd = bout.float().cuda()
    acts = torch.full((E + 1,), -7, dtype=torch.int32, device="cuda")
    q = _nan(E + 1, A)
    ed = torch.tensor([eps], dtype=torch.float64, device="cuda") if eps is not None else None
    xd = expo.double().cuda() if expo is not None else None
    sd = torch.tensor([step], dtype=torch.int64, device="cuda")
    L.check(L.lib.mirl_act_head_select(E, N, A, P, pitch, _p(part), _p(bd), int(has_val), _p(ed), _p(xd), eps_min, seed, _p(sd), _p(acts), _p(q),
                                       _st()), "mirl_act_head_select")
    torch.cuda.synchronize()
    assert int(acts[E]) == -7 and bool(torch.isnan(q[E]).all()), "the guard row was written"
    got = (acts[:E].cpu().long(), q[:E].cpu())
    if not cross:
        return got
    out = _nan(Rr, pitch)
    out[:, :NO] = (parts.sum(0) + bout).float().cuda()
    acts2 = torch.full((E + 1,), -7, dtype=torch.int32, device="cuda")
    q2, used = _nan(E + 1, A), _nan(E + 1)
    L.check(L.lib.mirl_actor_head_rng(E, N, A, _p(out), pitch, _p(out, A) if has_val else None, pitch if has_val else 0, _p(ed), _p(xd), eps_min,
                                      seed, _p(sd), _p(acts2), _p(q2), _p(used), _st()), "mirl_actor_head_rng")
    torch.cuda.synchronize()
    return got + (acts2[:E].cpu().long(), q2[:E].cpu(), used[:E].cpu())


# (E, N, A, has_val) -> k_act_head_select<CH = pitch / 8>, pitch = NO rounded up to 8:
#   (1, 1, 1, 0) CH 1;  (5, 7, 8, 1) NO = 9: CH 2;  (3, 70, 12, 0) CH 2, N > 64: lanes 0 .. 5 take a second row
#   (6, 130, 18, 1) NO = 19: CH 3, three trips;  (4, 64, 31, 1) NO = 32: CH 4, no padding;  (9, 32, 6, 1) CH 1
SELECT = [(1, 1, 1, 0), (5, 7, 8, 1), (3, 70, 12, 0), (6, 130, 18, 1), (4, 64, 31, 1), (9, 32, 6, 1)]


@pytest.mark.parametrize("E,N,A,has_val", SELECT, ids=lambda v: str(v))
def test_select_dyadic_shares_are_bit_equal_and_ties_go_to_the_first_maximum(E, N, A, has_val):
    d = R.dyadic_head_parts(8000 + E + N + A, E, N, A, 2 + (E + A) % 3, bool(has_val))
    assert d["margin"] < 2 ** 24
    want = R.actor_qvalues(d["adv"], d["val"])
    acts, q, acts2, q2, _ = _select_run(E, N, A, has_val, d["parts"], d["bout"], cross=True)
    assert torch.equal(q, want.float()), "%d q-values differ" % int((q != want.float()).sum())
    assert torch.equal(acts, d["first"]) and torch.equal(acts, R.first_max(want))
    assert torch.equal(q2, q) and torch.equal(acts2, acts)              # k_actor_head on the summed shares


def test_select_epsilon_greedy_with_exponents_and_floor_at_the_threshold():
    """eps ** expo_e against eps_min per env, and the Philox uniform u_e one float32 below / on / above the threshold: the
    exponents are chosen so that float32(eps ** expo_e) is u_e's upper neighbour (explore), u_e itself and its lower neighbour
    (both greedy: u < eps is strict); the env with the smallest u gets a large exponent and eps_min = u's upper neighbour."""
    E, N, A, has_val, step, eps = 9, 32, 6, 1, 5, 0.5
    d = R.dyadic_head_parts(8100, E, N, A, 3, True)
    greedy = d["first"]
    seed = next(s for s in range(77, 200) if bool((R.philox_head_draws(s, step, E, A)[1] != greedy).all())
                and float(R.philox_head_draws(s, step, E, A)[0].min()) > 2.0 ** -10)
    u, rnd = R.philox_head_draws(seed, step, E, A)
    lo = int(u.argmin())
    kind = torch.arange(E) % 3                                          # 0: u below the threshold, 1: on it, 2: above it
    thr = torch.where(kind == 0, torch.nextafter(u, torch.ones(E)), torch.where(kind == 1, u, torch.nextafter(u, torch.zeros(E))))
    expo = torch.log(thr.double()) / np.log(eps)
    expo[lo] = 12.0                                                     # 0.5 ** 12 = 2^-12 < eps_min: the floor wins here
    eps_min = float(torch.nextafter(u, torch.ones(E))[lo])
    per32 = R.eps_per_actor(eps, expo, eps_min, E).float()
    assert float(per32[lo]) == eps_min and bool((per32[torch.arange(E) != lo] > eps_min).all())
    others = torch.arange(E) != lo
    assert torch.equal(per32[others], thr[others]), "the exponents do not land on the thresholds"
    explore = u < per32
    assert bool(explore[lo]) and torch.equal(explore[others], (kind == 0)[others]) and int(explore.sum()) >= 3 and int((~explore).sum()) >= 4
    acts, q, acts2, q2, used = _select_run(E, N, A, has_val, d["parts"], d["bout"], eps=eps, expo=expo, eps_min=eps_min, seed=seed, step=step,
                                           cross=True)
    assert torch.equal(q, R.actor_qvalues(d["adv"], d["val"]).float()) and torch.equal(q2, q)
    assert torch.equal(used, per32)
    assert torch.equal(acts, R.eps_greedy(greedy, per32, u, rnd))
    assert torch.equal(acts[explore], rnd[explore]) and torch.equal(acts[~explore], greedy[~explore])
    assert torch.equal(acts2, acts)
    # eps alone (expo NULL, eps_min 0): every u below 0.5 explores
    acts, _ = _select_run(E, N, A, has_val, d["parts"], d["bout"], eps=eps, seed=seed, step=step)
    assert torch.equal(acts, torch.where(u < 0.5, rnd, greedy))


def _select_real_operands(E, N, A, has_val, P, seed):
    """-> (parts, bout, float64 q-values, their bounds, envs whose best action is clear of the second best): CPU only."""
    g = torch.Generator().manual_seed(seed)
    NO = A + (1 if has_val else 0)
    parts = (torch.randn(P, E * N, NO, generator=g) / np.sqrt(P)).double()
    bout = (torch.randn(NO, generator=g) * 0.1).double()
    o = parts.sum(0) + bout
    e_o = P * U * (parts.abs().sum(0) + bout.abs())
    adv, e_adv = o[:, :A].reshape(E, N, A), e_o[:, :A].reshape(E, N, A)
    val = o[:, A].reshape(E, N) if has_val else None
    want = R.actor_qvalues(adv, val)
    if val is None:
        t, e_t = adv, e_adv
    else:
        m = adv.sum(-1, keepdim=True)
        off = val.unsqueeze(-1) - m / A
        e_m = e_adv.sum(-1, keepdim=True) + (A - 1) * U * adv.abs().sum(-1, keepdim=True)
        e_off = e_o[:, A].reshape(E, N, 1) + e_m / A + U * m.abs() / A + U * off.abs()
        t = adv + off
        e_t = e_adv + e_off + U * t.abs()
    bound = (e_t.sum(1) + (-(-N // 64) + 6) * U * t.abs().sum(1)) / N + U * want.abs()
    top = want.topk(2, dim=-1)
    rows = torch.arange(E)
    clear = (top.values[:, 0] - top.values[:, 1]) > bound[rows, top.indices[:, 0]] + bound[rows, top.indices[:, 1]]
    return parts, bout, want, bound, clear


@pytest.mark.parametrize("E,N,A,has_val", [(33, 70, 12, 0), (40, 130, 18, 1)], ids=lambda v: str(v))
def test_select_real_shares_within_the_operation_count_bound(E, N, A, has_val):
    parts, bout, want, bound, clear = _select_real_operands(E, N, A, has_val, 5, 8200 + E)
    assert int((~clear).sum()) <= E // 10, "pick another seed"
    acts, q = _select_run(E, N, A, has_val, parts, bout)
    _within("k_act_head_select qvalues", q, want, bound)
    assert torch.equal(acts[clear], R.first_max(want)[clear])
