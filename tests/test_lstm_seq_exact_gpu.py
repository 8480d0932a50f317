"""GPU: the persistent LSTM sweeps k_lstm_seq_fwd<H>, k_lstm_seq_fwd_narrow<H> and k_lstm_seq_bwd (csrc/lstm_seq.hip) at their C
entry points against the float64 time loop of tests/pointwise_restate.py (equal to a torch.nn.LSTMCell loop with per-step resets and
its autograd, tests/test_pointwise_restate_cpu.py, which also shows that the bounds below are kept by a float32 evaluation of the
same forms and broken by five planted errors).

Shapes come from mirl_lstm_seq_fwd_grid, not from an assumed compute-unit count: the wide kernel runs when row blocks x H / 4
exceed the compute units, so the smallest wide batch is 64 (CUs // (H / 4)) + 16.  Every case asserts through lds_bytes which form
it launched: wide (64 (H + 4) + 4 * 16 * 20) * 4 bytes, narrow (16 (H + 4) + 256) * 4.

Forward.  Structure is bit-exact: hm[0] = h0 keep[0], hm[t + 1] = out[t] keep[t + 1] (last row unmasked), the same for cm / c_all;
a row held in reset has exactly-zero step inputs.  Every step is then compared with float64 FROM THE KERNEL'S OWN STEP INPUTS
(pre = gx[t] + hm[t] W^T, c_in = cm[t]), so nothing compounds.  First-order bounds, u = 2^-24, v_exp_f32 and v_rcp_f32 within 1 ulp
(2u relative), L = float32(log2 e); tiny = 2^-126 stands for results below the smallest normal number (flushed):
  pre = gx + sum_k h_k w_k         e_pre = u |pre| + n u sum |h_k w_k| + tiny, n = H for a dense W (a chain of H products per
                                   accumulator, or four chains of H / 4 and their sum); n = 0 for the selector W, whose sum is ONE
                                   product with a power of two: exact
  E = exp2(fl(y L)) for exp(y)     relative 2u |y| (L rounded, the product rounded: 2u |y L| absolute, times ln 2) + 2u (v_exp_f32)
  s = rcp(1 + E), y = -x           e_s = s (1 - s) e_pre + u (s (1 - s) (2 |x| + 2) + 3 s) + tiny
                                   (d s / d E = -s^2, s^2 E = s (1 - s); the sum 1 + E: u s; v_rcp_f32: 2u s)
  g = 1 - 2 r, r = rcp(E + 1),     e_g = (1 - g^2) e_pre + u (2 (r (1 - r) (4 |x| + 2) + 3 r) + |g|)
      y = 2x                       (e_r as for s with |y| = 2 |x|; 2 r is exact; the difference: u |g|).  The term is ABSOLUTE:
                                   at x = 0, r = 1/2 and e_g = 4u however small g is — the form cancels, it is not 2u |g|
  c = f c_in + i g                 e_c = |c_in| e_f + |g| e_i + i e_g + u (|f c_in| + |i g| + |c|)
  h = o tanh(c)                    e_h = |tanh c| e_o + o e_tanh(c; e_c) + u |h|        (the tanh term above at x = c, e_pre = e_c)
Saturated pre-activations (+-100) give gates of exactly 0, 1 and -1 and an exact c; they satisfy the same bounds.

Backward, against lstm_sweep_bwd in float64 on the float32 gates, c and masked c_in the forward launch saved; the kernel reads
the same c, so tanhf(c) is one ulp away (e_tc = 2u |tc|).  The bound is carried from step t + 1 to step t:
  dh_rec = dgates(t + 1) W         e_dhr = E_dg(t + 1) |W| + n u |dgates(t + 1)| |W|, n = 64 + 32 for a dense W (64 products per
                                   partial block, 32 blocks added in source order), n = 4 for the selector W (four exact products)
  dh = d_out + dh_rec keep         e_dh = keep e_dhr + u |dh|
  q = 1 - tc^2                     e_q = 2 |tc| e_tc + u tc^2 + u q
  dc = dc_rec keep + dh o q        e_dc = keep e_dcr + |o q| e_dh + |dh o| e_q + 2u |dh o q| + u |dc|
  d i = dc g i (1 - i)             |g i (1 - i)| e_dc + 4u |d i|;   d f = dc c_in f (1 - f) alike
  d g = dc i (1 - g^2)             |i (1 - g^2)| e_dc + u |dc i| + 2u |d g|
  d o = dh tc o (1 - o)            |tc o (1 - o)| e_dh + |dh o (1 - o)| e_tc + 4u |d o|
  dc_rec' = dc f                   e_dcr' = f e_dc + u |dc_rec'|
With a dense W the E_dg |W| term multiplies the bound by about sum_c |slope_c w_ck| per step; the selector W keeps it within a few u
of the gradient's size, which is where a wrong block, lane or step of the partial exchange shows.  Exact: through a reset
(keep[t + 1] = 0) and at the last step dgates[t] is what mirl_lstm_cell_bwd gives with first = 1, bit for bit, and exactly 0 where
d_out[t] is 0 as well; a null d_out is a zero d_out; a second launch repeats the first.

No input is non-finite and no launch is retried: mirl_lstm_seq_status is read once after every launch and must be 0."""
import ctypes as C

import pytest
import torch

from tests import pointwise_restate as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -126
GUARD = 2048

# name -> (form, H, batch as a function of the compute-unit count); on 256 compute units: 16, 80, 128, 528, 272, 144, 192, 528
CASES = {
    "narrow128-one-tile": ("narrow", 128, lambda cus: 16),
    "narrow256-ragged": ("narrow", 256, lambda cus: 80),
    "narrow512-largest": ("narrow", 512, lambda cus: 64 * (cus // 128)),
    "wide128-smallest": ("wide", 128, lambda cus: 64 * (cus // 32) + 16),          # k_lstm_seq_fwd<128>; the last block is one tile
    "wide256-smallest": ("wide", 256, lambda cus: 64 * (cus // 64) + 16),          # k_lstm_seq_fwd<256>
    "wide512-ragged": ("wide", 512, lambda cus: 64 * (cus // 128) + 16),
    "wide512-full": ("wide", 512, lambda cus: 64 * (cus // 128) + 64),
    "wide512-looping": ("wide", 512, lambda cus: 64 * (cus // 32) + 16),           # more row blocks than clusters, ragged
}
SIX_STEPS = ("narrow128-one-tile", "narrow256-ragged", "narrow512-largest", "wide128-smallest", "wide256-smallest", "wide512-looping")
CASE_T = [(c, T) for c in CASES for T in (1, 2, 3, 4)] + [(c, 6) for c in SIX_STEPS]
FAMILIES = ("selector", "gaussian")
BWD_BATCHES = {"16": lambda cus: 16, "80": lambda cus: 80, "144": lambda cus: 144, "looping": lambda cus: 64 * (cus // 32) + 16}


# ---- the bounds (float64 tensors; no GPU needed: tests/test_pointwise_restate_cpu.py runs them too) ---------------------------------
def e_sigmoid(x, s, e_x):
    return s * (1 - s) * e_x + (s * (1 - s) * (2 * x.abs() + 2) + 3 * s) * U + TINY


def e_tanh(x, g, e_x):
    r = (1 - g) / 2
    return (1 - g * g) * e_x + (2 * (r * (1 - r) * (4 * x.abs() + 2) + 3 * r) + g.abs()) * U


def fwd_step_bound(pre, rec_abs, n, c_in):
    """pre (R, 4H): the exact pre-activations; rec_abs (R, 4H) = |h| |W|^T (or None with n = 0); c_in (R, H).
    -> the float64 step (gates, c, h) and its bounds (e_gates, e_c, e_h)."""
    e_pre = U * pre.abs() + TINY
    if n:
        e_pre = e_pre + n * U * rec_abs
    gates, h, c, _, _ = R.lstm_cell_fwd(pre, c_in)
    (xi, xf, xg, xo), (pi, pf, pg, po), (i, f, g, o) = pre.chunk(4, 1), e_pre.chunk(4, 1), gates.chunk(4, 1)
    e_i, e_f, e_g, e_o = e_sigmoid(xi, i, pi), e_sigmoid(xf, f, pf), e_tanh(xg, g, pg), e_sigmoid(xo, o, po)
    e_c = c_in.abs() * e_f + g.abs() * e_i + i * e_g + U * ((f * c_in).abs() + (i * g).abs() + c.abs())
    tc = torch.tanh(c)
    e_h = tc.abs() * e_o + o * e_tanh(c, tc, e_c) + U * h.abs()
    return gates, c, h, torch.cat([e_i, e_f, e_g, e_o], 1), e_c, e_h


def bwd_sweep_bound(gates, c_all, cm, d_out, keep, w, n):
    """-> (d pre-activations (T, B, 4H) in float64, their bound), the recurrence of lstm_sweep_bwd with e_dh / e_dc carried along."""
    T, B = gates.shape[0], gates.shape[1]
    want, bound = torch.zeros_like(gates), torch.zeros_like(gates)
    aw = w.abs()
    dhr = dcr = e_dhr = e_dcr = None
    for t in range(T - 1, -1, -1):
        first = t == T - 1
        i, f, g, o = gates[t].chunk(4, 1)
        c_in = cm[t]
        k = torch.ones(B, 1, dtype=gates.dtype) if first else keep[t + 1].unsqueeze(1)
        zero = torch.zeros_like(c_in)
        dh = d_out[t] + (zero if first else dhr * k)
        e_dh = (zero if first else k * e_dhr) + U * dh.abs()
        tc = torch.tanh(c_all[t])
        q = 1 - tc * tc
        e_tc = 2 * U * tc.abs()
        e_q = 2 * tc.abs() * e_tc + U * tc * tc + U * q
        dc = (zero if first else dcr * k) + dh * o * q
        e_dc = (zero if first else k * e_dcr) + (o * q).abs() * e_dh + (dh * o).abs() * e_q + 2 * U * (dh * o * q).abs() + U * dc.abs()
        di, df, dg, do = dc * g * i * (1 - i), dc * c_in * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)
        want[t] = torch.cat([di, df, dg, do], 1)
        bound[t] = torch.cat([(g * i * (1 - i)).abs() * e_dc + 4 * U * di.abs(),
                              (c_in * f * (1 - f)).abs() * e_dc + 4 * U * df.abs(),
                              (i * (1 - g * g)).abs() * e_dc + U * (dc * i).abs() + 2 * U * dg.abs(),
                              (tc * o * (1 - o)).abs() * e_dh + (dh * o * (1 - o)).abs() * e_tc + 4 * U * do.abs()], 1)
        dcr = dc * f
        e_dcr = f * e_dc + U * dcr.abs()
        dhr = want[t] @ w
        e_dhr = bound[t] @ aw + n * U * (want[t].abs() @ aw)
    return want, bound


def sweep_inputs(T, B, H, family, seed):
    """float32 CPU tensors.  keep: row 0 never resets, row 1 is held in reset, row 2 resets at step 0 only, row 3 at step T - 1
    only, the rest at random (20 %).  h0 holds +-2 and +-3.5: arbitrary user values with bit 30 of the float set."""
    g = torch.Generator().manual_seed(seed)
    if family == "selector":
        w = R.selector_whh(seed, H).float()
        gx = torch.randn(T, B, 4 * H, generator=g) * 2
    else:
        w = torch.randn(4 * H, H, generator=g) * (1.5 / H ** 0.5)
        gx = torch.randn(T, B, 4 * H, generator=g)
    h0, c0 = torch.randn(B, H, generator=g) * 0.5, torch.randn(B, H, generator=g)
    big = torch.tensor([2.0, -2.0, 3.5, -3.5])
    idx = torch.arange(0, B * H, 37)
    h0.view(-1)[idx] = big[torch.arange(idx.numel()) % 4]
    keep = (torch.rand(T, B, generator=g) > 0.2).float()
    keep[:, 0], keep[:, 1], keep[:, 2], keep[:, 3] = 1.0, 0.0, 1.0, 1.0
    keep[0, 2] = 0.0
    keep[T - 1, 3] = 0.0
    return dict(T=T, B=B, H=H, family=family, n=(0 if family == "selector" else H), gx=gx, w=w.contiguous(), h0=h0, c0=c0, keep=keep)


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def _lib():
    from rltime_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _buf(src=None, n=None):
    """A flat device buffer with a NaN guard behind it: a copy of src, or NaN all over."""
    n = src.numel() if src is not None else n
    b = torch.full((n + GUARD,), float("nan"), device="cuda")
    if src is not None:
        b[:n] = src.reshape(-1).cuda()
    return b


def _guard_intact(b, n):
    return bool(torch.isnan(b[n:]).all())


def _workspace(nbytes):
    n = (nbytes + 3) // 4
    ws = torch.full((n + GUARD,), 3.0, device="cuda")          # finite leftovers with bit 30 set; the launch clears what it must
    assert ws.data_ptr() % 256 == 0
    return ws, n


def _status_is_zero():
    L = _lib()
    st = C.c_int32(-1)
    L.check(L.lib.mirl_lstm_seq_status(C.byref(st)), "mirl_lstm_seq_status")
    assert st.value == 0, "a workgroup of the sweep gave up waiting (status %d)" % st.value


def _within(what, got, want, bound):
    err = (got.double() - want).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print("RATIO %s: worst err / bound = %.3f" % (what, ratio))
    assert bool((err <= bound).all()), "%s: err / bound = %.3f" % (what, ratio)


def _grid(B, H):
    L = _lib()
    wg, lds, cus, per = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int32()
    L.check(L.lib.mirl_lstm_seq_fwd_grid(B, H, C.byref(wg), C.byref(lds), C.byref(cus), C.byref(per)), "mirl_lstm_seq_fwd_grid")
    return wg.value, lds.value, cus.value, per.value


def _cus():
    return _grid(16, 128)[2]


def _shape(case):
    """-> (form, H, B) of a case on this device; fails (never skips) when the launch would take the other kernel."""
    form, H, rule = CASES[case]
    B = rule(_cus())
    lds = _grid(B, H)[1]
    want = (64 * (H + 4) + 4 * 16 * 20) * 4 if form == "wide" else (16 * (H + 4) + 256) * 4
    assert lds == want, "%s: B = %d, H = %d launches with %d bytes of LDS, the %s form has %d" % (case, B, H, lds, form, want)
    return form, H, B


def _fwd(inp, save, out=True, c_all=True, hm=True, last=False):
    """One launch of mirl_lstm_seq_fwd -> dict of float32 CPU tensors (gx: the buffer after the launch)."""
    L = _lib()
    T, B, H = inp["T"], inp["B"], inp["H"]
    n = T * B * H
    gxb = _buf(inp["gx"])
    w, h0, c0, keep = (inp[k].cuda().contiguous() for k in ("w", "h0", "c0", "keep"))
    size = {"out": n, "c_all": n, "hm": n + B * H, "cm": n + B * H, "h_last": B * H, "c_last": B * H}
    on = {"out": out, "c_all": c_all, "hm": hm, "cm": hm, "h_last": last, "c_last": last}
    bufs = {k: (_buf(n=size[k]) if on[k] else None) for k in size}
    need = C.c_int64()
    L.check(L.lib.mirl_lstm_seq_workspace_bytes(B, H, C.byref(need)), "mirl_lstm_seq_workspace_bytes")
    ws, nws = _workspace(need.value)
    L.check(L.lib.mirl_lstm_seq_fwd(T, B, H, _p(gxb), _p(w), _p(h0), _p(c0), _p(keep), _p(bufs["out"]), _p(bufs["c_all"]), _p(bufs["hm"]),
                                    _p(bufs["cm"]), _p(bufs["h_last"]), _p(bufs["c_last"]), int(save), _p(ws), _st()), "mirl_lstm_seq_fwd")
    torch.cuda.synchronize()
    _status_is_zero()
    assert _guard_intact(gxb, 4 * n), "the guard behind gx was written"
    for k, b in bufs.items():
        assert b is None or _guard_intact(b, size[k]), "the guard behind %s was written" % k
    assert bool((ws[nws:] == 3.0).all()), "the guard behind the workspace was written"
    res = {"gx": gxb[:4 * n].view(T, B, 4 * H).cpu()}
    for k, b in bufs.items():
        res[k] = None if b is None else b[:size[k]].view(-1, B, H).cpu()
    for k in ("h_last", "c_last"):
        res[k] = None if res[k] is None else res[k][0]
    return res


def _seed(case, T, family):
    return 1000 * list(CASES).index(case) + 10 * T + FAMILIES.index(family)


_SUMMARY = {}       # (case, T, family) -> (out, hm[T], cm[T]) of the saving launch, for the launch that saves nothing


def _saving_launch(case, T, family):
    form, H, B = _shape(case)
    inp = sweep_inputs(T, B, H, family, _seed(case, T, family))
    r = _fwd(inp, save=1)
    _SUMMARY[(case, T, family)] = (r["out"], r["hm"][T], r["cm"][T])
    return form, inp, r


def _check_structure(inp, r):
    T, B, H, k = inp["T"], inp["B"], inp["H"], inp["keep"]
    assert torch.equal(r["hm"][0], inp["h0"] * k[0].unsqueeze(1)) and torch.equal(r["cm"][0], inp["c0"] * k[0].unsqueeze(1))
    kn = torch.cat([k[1:], torch.ones(1, B)]).unsqueeze(2)                     # the last row is unmasked
    assert torch.equal(r["hm"][1:], r["out"] * kn), "hm[t + 1] != out[t] keep[t + 1]"
    assert torch.equal(r["cm"][1:], r["c_all"] * kn), "cm[t + 1] != c_all[t] keep[t + 1]"
    assert float(r["hm"][:T, 1].abs().max()) == 0.0 and float(r["cm"][:T, 1].abs().max()) == 0.0      # the row held in reset
    for v in r.values():
        assert v is None or bool(torch.isfinite(v).all())


def _check_steps(form, inp, r):
    """Every step against float64 from the step inputs the kernel wrote (hm[t], cm[t])."""
    T, B, H, n = inp["T"], inp["B"], inp["H"], inp["n"]
    w = inp["w"].double()
    hm, cm = r["hm"][:T].double().reshape(T * B, H), r["cm"][:T].double().reshape(T * B, H)
    pre = inp["gx"].double().reshape(T * B, 4 * H) + hm @ w.t()
    rec_abs = hm.abs() @ w.abs().t() if n else None
    gates, c, h, e_gates, e_c, e_h = fwd_step_bound(pre, rec_abs, n, cm)
    name = "k_lstm_seq_fwd%s<%d> %s" % ("_narrow" if form == "narrow" else "", H, inp["family"])
    _within(name + " gates", r["gx"].reshape(T * B, 4 * H), gates, e_gates)
    _within(name + " c", r["c_all"].reshape(T * B, H), c, e_c)
    _within(name + " h", r["out"].reshape(T * B, H), h, e_h)
    return gates, c, h


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case,T", CASE_T)
def test_forward_sweep_structure_and_every_step_against_float64(case, T, family):
    form, inp, r = _saving_launch(case, T, family)
    _check_structure(inp, r)
    _check_steps(form, inp, r)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case,T", CASE_T)
def test_forward_sweep_that_saves_nothing_equals_the_saving_one(case, T, family):
    if (case, T, family) not in _SUMMARY:
        _saving_launch(case, T, family)
    out, h_last, c_last = _SUMMARY[(case, T, family)]
    form, H, B = _shape(case)
    inp = sweep_inputs(T, B, H, family, _seed(case, T, family))
    r = _fwd(inp, save=0, out=True, c_all=False, hm=False, last=True)
    assert torch.equal(r["out"], out) and torch.equal(r["h_last"], h_last) and torch.equal(r["c_last"], c_last)
    assert torch.equal(r["gx"], inp["gx"]), "a launch that saves nothing wrote into gx"


@pytest.mark.parametrize("case", SIX_STEPS)
def test_forward_optional_outputs_leave_the_others_unchanged(case):
    form, inp, full = _saving_launch(case, 3, "selector")
    no_out = _fwd(inp, save=1, out=False)
    no_c = _fwd(inp, save=1, c_all=False)
    both = _fwd(inp, save=1, last=True)
    assert no_out["out"] is None and no_c["c_all"] is None
    for k in ("gx", "c_all", "hm", "cm"):
        assert torch.equal(no_out[k], full[k]), k
    for k in ("gx", "out", "hm", "cm"):
        assert torch.equal(no_c[k], full[k]), k
    for k in ("gx", "out", "c_all", "hm", "cm"):
        assert torch.equal(both[k], full[k]), k
    assert torch.equal(both["h_last"], full["hm"][3]) and torch.equal(both["c_last"], full["cm"][3])


@pytest.mark.parametrize("case", ["narrow256-ragged", "wide512-ragged"])
def test_forward_saturated_gates_are_exact(case):
    """gx = +-100 in planted blocks (the recurrent term of the selector W is at most 3.5), c0 = 3: gates of exactly 0, 1, -1, an
    exact c, h exactly 0 under a closed output gate; everything finite, and the float64 comparison holds with the same bound."""
    form, H, B = _shape(case)
    T = 3
    inp = sweep_inputs(T, B, H, "selector", 77)
    t_, r_, c_ = torch.arange(T).view(T, 1, 1), torch.arange(B).view(1, B, 1), torch.arange(4 * H).view(1, 1, 4 * H)
    inp["gx"] = torch.where((r_ // 3 + c_ // 5 + t_) % 3 == 0, torch.tensor(-100.0), torch.tensor(100.0)).contiguous()
    inp["c0"] = torch.full((B, H), 3.0)
    r = _fwd(inp, save=1)
    _check_structure(inp, r)
    gates, c, h = _check_steps(form, inp, r)
    lo = torch.cat([torch.zeros(H), torch.zeros(H), -torch.ones(H), torch.zeros(H)]).expand(T, B, 4 * H)
    assert torch.equal(r["gx"], torch.where(inp["gx"] > 0, torch.ones(T, B, 4 * H), lo))
    gi, gf, gg, go = r["gx"].double().chunk(4, dim=2)
    c_exact = gf * r["cm"][:T].double() + gi * gg                              # gates of 0 / 1 / -1 on an integer c_in: no rounding
    assert torch.equal(r["c_all"].double(), c_exact) and torch.equal(c_exact, c_exact.round()) and float(c_exact.abs().max()) >= 4.0
    closed, live = go == 0, (go == 1) & (c_exact != 0)
    assert bool(closed.any()) and bool(live.any()) and float(r["out"][closed].abs().max()) == 0.0
    assert float(r["out"][live].abs().min()) >= 0.76                           # tanh of an integer |c| >= 1


# ---- backward --------------------------------------------------------------------------------------------------------------------
def _bwd(inp, gates, c_all, cm, d_out):
    """One launch of mirl_lstm_seq_bwd on float32 CPU tensors -> d pre-activations (T, B, 4H) on the CPU."""
    L = _lib()
    T, B, H = inp["T"], inp["B"], inp["H"]
    gb = _buf(gates)
    w, keep, ca, cmd = inp["w"].cuda().contiguous(), inp["keep"].cuda().contiguous(), c_all.cuda().contiguous(), cm.cuda().contiguous()
    dd = None if d_out is None else d_out.cuda().contiguous()
    need = C.c_int64()
    L.check(L.lib.mirl_lstm_seq_bwd_workspace_bytes(B, H, C.byref(need)), "mirl_lstm_seq_bwd_workspace_bytes")
    ws, nws = _workspace(need.value)
    L.check(L.lib.mirl_lstm_seq_bwd(T, B, H, _p(gb), _p(w), _p(ca), _p(cmd), _p(dd), _p(keep), _p(ws), _st()), "mirl_lstm_seq_bwd")
    torch.cuda.synchronize()
    _status_is_zero()
    assert _guard_intact(gb, 4 * T * B * H), "the guard behind the gates was written"
    assert bool((ws[nws:] == 3.0).all()), "the guard behind the workspace was written"
    assert torch.equal(ca.cpu(), c_all) and torch.equal(cmd.cpu(), cm)
    return gb[:4 * T * B * H].view(T, B, 4 * H).cpu()


def _cell_first(gates, c_all, cm, d_out):
    """mirl_lstm_cell_bwd with first = 1 on all (t, row) at once: the gate gradients that d_out[t] alone gives."""
    L = _lib()
    T, B, H4 = gates.shape
    H = H4 // 4
    g = gates.reshape(T * B, H4).cuda().contiguous()
    dc = torch.empty(T * B, H, device="cuda")
    # named, so that each buffer lives until the launch has run: a temporary's block goes back to the allocator at once
    ca, cmd, dd = c_all.cuda().contiguous(), cm[:T].cuda().contiguous(), d_out.cuda().contiguous()
    L.check(L.lib.mirl_lstm_cell_bwd(T * B, H, _p(g), _p(ca), _p(cmd), _p(dd), None, _p(dc), None, 1, _st()), "mirl_lstm_cell_bwd")
    torch.cuda.synchronize()
    return g.view(T, B, H4).cpu()


def _bwd_inputs(batch, T, family):
    B = BWD_BATCHES[batch](_cus())
    inp = sweep_inputs(T, B, 512, family, 5000 + 100 * list(BWD_BATCHES).index(batch) + 10 * T + FAMILIES.index(family))
    fwd = _fwd(inp, save=1)
    g = torch.Generator().manual_seed(T + B)
    d_out = torch.randn(T, B, 512, generator=g)
    d_out[0::2, 1] = 0.0                                   # the row held in reset: no gradient from above at even steps
    return inp, fwd, d_out


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("T", [1, 2, 3, 5])
@pytest.mark.parametrize("batch", list(BWD_BATCHES))
def test_backward_sweep_against_float64_and_exact_through_resets(batch, T, family):
    inp, fwd, d_out = _bwd_inputs(batch, T, family)
    B, H, keep = inp["B"], inp["H"], inp["keep"]
    got = _bwd(inp, fwd["gx"], fwd["c_all"], fwd["cm"], d_out)
    args = [t.double() for t in (fwd["gx"], fwd["c_all"], fwd["cm"], d_out, keep, inp["w"])]
    want, bound = bwd_sweep_bound(*args, n=4 if family == "selector" else 96)
    assert float((want - R.lstm_sweep_bwd(*args)).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    for t in range(T):
        print("step %d of %d:" % (t, T), end=" ")
        _within("k_lstm_seq_bwd %s d pre-activations" % family, got[t], want[t], bound[t])
    # exact: nothing flows through a reset, and the last step has nothing behind it
    alone = _cell_first(fwd["gx"], fwd["c_all"], fwd["cm"], d_out)
    cut = torch.cat([keep[1:] == 0, torch.ones(1, B, dtype=torch.bool)])       # (T, B)
    assert bool(cut[:, 1].all()) and torch.equal(got[cut], alone[cut])
    if T == 1:
        assert torch.equal(got, alone)
    dead = cut & (d_out.abs().amax(2) == 0)
    assert bool(dead.any()) and float(got[dead].abs().max()) == 0.0


@pytest.mark.parametrize("batch", ["80", "144"])
def test_backward_null_d_out_is_a_zero_d_out_and_a_second_launch_repeats_the_first(batch):
    inp, fwd, d_out = _bwd_inputs(batch, 3, "gaussian")
    a = _bwd(inp, fwd["gx"], fwd["c_all"], fwd["cm"], d_out)
    b = _bwd(inp, fwd["gx"], fwd["c_all"], fwd["cm"], d_out)
    assert torch.equal(a, b) and float(a.abs().max()) > 0.0
    z = _bwd(inp, fwd["gx"], fwd["c_all"], fwd["cm"], torch.zeros_like(d_out))
    n = _bwd(inp, fwd["gx"], fwd["c_all"], fwd["cm"], None)
    assert torch.equal(z.view(torch.int32), n.view(torch.int32))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_what_they_cannot_run_and_write_nothing():
    L = _lib()
    T, B = 2, 32
    nan = lambda n: torch.full((n,), float("nan"), device="cuda")          # noqa: E731
    zeros = lambda n: torch.zeros(n, device="cuda")                         # noqa: E731

    def fwd_args(H, B=B):
        return dict(gx=zeros(T * B * 4 * H), w=zeros(4 * H * H + 4), h0=zeros(B * H), c0=zeros(B * H), keep=zeros(T * B) + 1, out=nan(T * B * H),
                    c_all=nan(T * B * H), hm=nan((T + 1) * B * H), cm=nan((T + 1) * B * H), h_last=nan(B * H), c_last=nan(B * H), ws=nan(1 << 20))

    def call_fwd(a, H, B=B, **over):
        v = dict(a, **over)
        w = v["w"][1:] if over.get("w_off") else v["w"][:4 * H * H]
        ws = v["ws"][4:] if over.get("ws_off") else v["ws"]
        rc = L.lib.mirl_lstm_seq_fwd(T, B, H, _p(v["gx"]), _p(w), _p(v["h0"]), _p(v["c0"]), _p(v["keep"]), _p(v["out"]), _p(v["c_all"]), _p(v["hm"]),
                                     _p(v["cm"]), _p(v["h_last"]), _p(v["c_last"]), 1, _p(ws), _st())
        torch.cuda.synchronize()
        for k in ("out", "c_all", "hm", "cm", "h_last", "c_last", "ws"):
            assert bool(torch.isnan(a[k]).all()), k
        assert float(a["gx"].abs().max()) == 0.0
        return rc

    a = fwd_args(384)
    assert call_fwd(a, 384) == -1                                             # H outside {128, 256, 512}
    a = fwd_args(128, 24)
    assert call_fwd(a, 128, 24) == -1                                         # B no multiple of 16
    a = fwd_args(128)
    assert a["w"].data_ptr() % 16 == 0 and a["ws"].data_ptr() % 256 == 0
    assert call_fwd(a, 128, cm=None) == -1 and call_fwd(a, 128, hm=None) == -1           # hm without cm, cm without hm
    assert call_fwd(a, 128, c_last=None) == -1 and call_fwd(a, 128, h_last=None) == -1
    assert call_fwd(a, 128, hm=None, cm=None, h_last=None, c_last=None) == -1            # neither output pair
    assert call_fwd(a, 128, ws_off=True) == -1                                            # workspace 16 bytes off 256-byte alignment
    assert call_fwd(a, 128, w_off=True) == -1                                             # w_hh 4 bytes off 16-byte alignment
    # backward: H = 256 is not built
    H = 256
    g, ws = nan(T * B * 4 * H), nan(1 << 20)
    x = zeros(max((T + 1) * B * H, 4 * H * H))
    assert L.lib.mirl_lstm_seq_bwd(T, B, H, _p(g), _p(x), _p(x), _p(x), _p(x), _p(x), _p(ws), _st()) == -1
    H = 512
    g = nan(T * B * 4 * H)
    x = zeros(max((T + 1) * B * H, 4 * H * H))
    assert L.lib.mirl_lstm_seq_bwd(T, B, H, _p(g), _p(x), _p(x), _p(x), _p(x), _p(x), _p(ws[4:]), _st()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(g).all()) and bool(torch.isnan(ws).all())
    _status_is_zero()
