"""GPU: mirl_lstm_ms_fwd / mirl_lstm_ms_bwd (csrc/lstm_multi.hip) driven directly on a projection built on the CPU, every
output of both — out, hm, cm, the activated gates, d pre-activation, S, dh_ws, dc_ws — element by element against the
float64 restatement (tests/lstm_multi_restate.py) at the shapes where the kernels take another branch, the contracts
include/mirl.h states for them (nothing needs initialising, rows are independent, reruns are bit-identical, h_last /
c_last, need_grad = 0 only reads), saturated gates, the refusals, and the routing of LSTM.forward around the op."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import lstm_multi_restate as R
from tests.test_lstm_multi_gpu import GRAD_TOL, OUT_TOL

pytestmark = pytest.mark.gpu

ERR_ARG = -1
SENT = -12345.0
# (T, B, N, H), each for the guard or constant of csrc/lstm_multi.hip named beside it (MS_WAVES = 4, MS_KC = 512, MS_PRE = 8)
SHAPES = [
    # k_lstm_ms_fwd ring: `16 * i < H` and `k + 16 * i < H` are false for i = 3 in the FIRST round (H < 64); H / 16 = 3
    # slabs over MS_WAVES = 4: three working waves, the fourth leaves at `if (j0 >= H) return`; backward K = 192 is one
    # chunk shorter than MS_KC
    (2, 3, 2, 48),
    # H = 64 + 16: a full round, then a ragged one (`k + 64 + 16 * i < H` and `k + 16 * i < H` hold for i = 0 only);
    # H / 16 = 5 slabs: blockIdx.y = 1 has one working wave and three that only stage; N = MS_PRE + 1: one sample through
    # `for (n = MS_PRE; n < N; ++n)` in both kernels; B = 18: two row tiles, the second with 2 valid rows (`b < B`)
    (2, 18, 9, 80),
    # k_lstm_ms_bwd: K = 4H = 576 = MS_KC + 64: a full chunk, then `kc = K - k0` = 64 behind `if (k0) __syncthreads()`,
    # staged with fewer columns, `k + 64 < kc` false in its only round; T = 3 runs that twice; H / 16 = 9: blockIdx.y = 0..2
    (3, 4, 2, 144),
    # N = 64, the largest ms_shape_ok takes: 56 samples through the loops past MS_PRE, the longest sums in one lane
    (2, 2, 64, 16),
    # H = 1024, the largest: 16 (H + 4) 4 = 65 792 bytes of dynamic LDS > 64 KB (`raise_lds_limit`), 16 forward rounds,
    # K = 4096 backward in eight full chunks; B = 17: a row tile with one valid row
    (2, 17, 2, 1024),
    # the actor's step of catch_iqn_lstm_pre / atari_iqn_lstm: T = 1, so `keep_in`, `h_last` and a null `keep_next` meet in
    # one launch and the backward runs with `s_next` null
    (1, 8, 8, 512),
]
FWD_KEYS, BWD_KEYS = ("out", "hm", "cm", "gates"), ("dg", "S", "dh_ws", "dc_ws")
CONTRACT_SHAPES = [(2, 18, 9, 80, 5), (3, 4, 2, 144, 1)]            # (T, B, N, H, B'): B' rows are kept


@functools.lru_cache(maxsize=None)
def _case(T, B, N, H):
    """((gx, w_hh, h0, c0, keep, d_out) in float32 on the CPU, the float64 restatement of all eight outputs)."""
    p, h0, c0, keep, up = R.inputs(T, B, N, H)
    args = (R.project(p, T, B, N), p["w_hh"], h0, c0, keep, up.reshape(T, B, N, H))
    return args, R.restate(*args)


def _guarded(lead, row, fill):
    """A (lead + row) device tensor of `fill` with one row tile (16 rows) of SENT behind it: (tensor, guard)."""
    n, tail = int(np.prod(lead + row)), 16 * int(np.prod(row))
    flat = torch.full((n + tail,), SENT, device="cuda")
    flat[:n] = fill
    return flat[:n].view(*(lead + row)), flat[n:]


def _run(gx, w_hh, h0, c0, keep, d_out, fill=float("nan"), last=False, need_grad=1, backward=True, keep_off=False):
    """One forward (and backward) sweep on fresh buffers prefilled with `fill`; everything the calls write, on the CPU.
    Every buffer the kernels write is followed by a guard tile that must come back untouched."""
    from rltime_amd._lib import lib, check, ptr, stream
    T, B, N, G = gx.shape
    H = G // 4
    guards = []

    def buf(lead, row, src=None):
        t, guard = _guarded(lead, row, fill)
        guards.append(guard)
        if src is not None:
            t.copy_(src)
        return t

    gates = buf((T, B), (N, G), gx)
    out, hm, cm = buf((T, B), (N, H)), buf((T + 1, B), (H,)), buf((T + 1, B), (H,))
    hl, cl = (buf((B,), (H,)), buf((B,), (H,))) if last else (None, None)
    wd, h0d, c0d, dd = (v.contiguous().cuda() for v in (w_hh, h0, c0, d_out))
    kd = torch.zeros(T * B + 4, device="cuda")
    kd[int(keep_off):int(keep_off) + T * B] = keep.reshape(-1).cuda()
    kp = C.c_void_p(kd.data_ptr() + 4 * int(keep_off))
    check(lib.mirl_lstm_ms_fwd(T, B, N, H, ptr(gates), ptr(wd), ptr(h0d), ptr(c0d), kp, ptr(out), ptr(hm), ptr(cm), ptr(hl), ptr(cl),
                               need_grad, stream()), "mirl_lstm_ms_fwd")
    res = dict(out=out, hm=hm, cm=cm, gates=gates.clone())
    if last:
        res.update(h_last=hl, c_last=cl)
    if backward:
        S, dh, dc = buf((T, B), (G,)), buf((B,), (H,)), buf((B,), (H,))
        check(lib.mirl_lstm_ms_bwd(T, B, N, H, ptr(gates), ptr(wd), ptr(cm), ptr(dd), kp, ptr(S), ptr(dh), ptr(dc), stream()),
              "mirl_lstm_ms_bwd")
        res.update(dg=gates, S=S, dh_ws=dh, dc_ws=dc)
    torch.cuda.synchronize()
    assert all(bool((g == SENT).all()) for g in guards), "a store past the last row"
    return {k: v.cpu() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def _base(T, B, N, H):
    """Forward with need_grad = 1 and backward on NaN-filled buffers, shared by the tests that compare runs with it."""
    return _run(*_case(T, B, N, H)[0])


def _against_restatement(got, want, shape):
    for k in FWD_KEYS + BWD_KEYS:
        assert got[k].shape == want[k].shape and bool(torch.isfinite(got[k]).all()), (k, shape)
        g, w = got[k].double().numpy(), want[k].numpy()
        if k in FWD_KEYS:
            print("%s %s: max abs err %.3g" % (shape, k, np.abs(g - w).max()))
            np.testing.assert_allclose(g, w, err_msg=k, **OUT_TOL)
        else:
            scale = float(np.abs(w).max()) + 1e-6
            print("%s %s: max abs err / scale %.3g (scale %.3g)" % (shape, k, np.abs(g - w).max() / scale, scale))
            np.testing.assert_allclose(g / scale, w / scale, err_msg=k, **GRAD_TOL)


def _same_bits(a, b, keys=FWD_KEYS + BWD_KEYS, what=""):
    for k in keys:
        assert torch.equal(a[k], b[k]), (k, what)


@pytest.mark.parametrize("T,B,N,H", SHAPES)
def test_every_output_against_float64(T, B, N, H):
    args, want = _case(T, B, N, H)
    got = _base(T, B, N, H)
    _against_restatement(got, want, (T, B, N, H))
    assert bool(got["dg"].any()) and not torch.equal(got["dg"], got["gates"])
    if T == 1:
        assert not bool(got["dh_ws"].any())                 # nothing flows back from the future


@pytest.mark.parametrize("T,B,N,H", SHAPES)
def test_h_last_c_last_and_need_grad_0(T, B, N, H):
    args, _ = _case(T, B, N, H)
    base = _base(T, B, N, H)
    for need_grad in (1, 0):
        got = _run(*args, last=True, need_grad=need_grad, backward=False)
        assert torch.equal(got["h_last"], got["hm"][T]) and torch.equal(got["c_last"], got["cm"][T]), need_grad
        _same_bits(got, base, ("out", "hm", "cm"), need_grad)
        if need_grad:
            assert torch.equal(got["gates"], base["gates"]) and not torch.equal(got["gates"], args[0])
        else:
            assert torch.equal(got["gates"], args[0])       # without need_grad the projection is only read
    plain = _run(*args, need_grad=0, backward=False)
    _same_bits(plain, base, ("out", "hm", "cm"))
    assert torch.equal(plain["gates"], args[0])


@pytest.mark.parametrize("T,B,N,H,Bp", CONTRACT_SHAPES)
def test_nothing_needs_initialising_and_reruns_are_bit_identical(T, B, N, H, Bp):
    args, _ = _case(T, B, N, H)
    nan = _base(T, B, N, H)
    for k in FWD_KEYS + BWD_KEYS:
        assert bool(torch.isfinite(nan[k]).all()), k
    _same_bits(_run(*args, fill=0.0), nan, what="zero-filled")
    _same_bits(_run(*(a.clone() for a in args)), nan, what="rerun")


@pytest.mark.parametrize("T,B,N,H,Bp", CONTRACT_SHAPES)
def test_rows_are_independent_and_rows_past_B_do_not_leak(T, B, N, H, Bp):
    args, _ = _case(T, B, N, H)
    gx, w_hh, h0, c0, keep, d_out = args
    full = _base(T, B, N, H)

    def kept(res):
        return {k: (v[:Bp] if k in ("dh_ws", "dc_ws") else v[:, :Bp]) for k, v in res.items()}

    alone = _run(gx[:, :Bp].contiguous(), w_hh, h0[:Bp], c0[:Bp], keep[:, :Bp].contiguous(), d_out[:, :Bp].contiguous())
    assert alone["out"].shape == (T, Bp, N, H) and alone["dc_ws"].shape == (Bp, H)
    _same_bits(alone, kept(full), what="the first B' sequences alone")
    poisoned = [a.clone() for a in (gx, h0, c0, d_out)]
    poisoned[0][:, Bp:], poisoned[1][Bp:], poisoned[2][Bp:], poisoned[3][:, Bp:] = 1e30, 1e30, 1e30, 1e30
    other = _run(poisoned[0], w_hh, poisoned[1], poisoned[2], keep, poisoned[3])
    _same_bits(kept(other), kept(full), what="the other rows at 1e30")
    assert not torch.equal(other["out"][:, Bp:], full["out"][:, Bp:])


def test_keep_needs_no_alignment():
    T, B, N, H = 2, 18, 9, 80
    _same_bits(_run(*_case(T, B, N, H)[0], keep_off=True), _base(T, B, N, H))


def test_saturated_gates():
    T, B, N, H = 3, 5, 3, 32
    args = R.saturated_inputs(T, B, N, H)
    want = R.restate(*args)
    got = _run(*args)
    _against_restatement(got, want, "saturated")
    sat = (got["gates"] == 0) | (got["gates"].abs() == 1)
    assert 0.05 < float(sat.float().mean()) < 0.5           # float32 gates that are exactly 0 or +-1, and most are not


def test_refusals_launch_nothing():
    from rltime_amd._lib import lib, ptr, stream
    T, B, N, H = 2, 3, 2, 16
    TM, BM, NM, HM = 2, 3, 65, 1040                         # every buffer holds the largest refused shape
    new = lambda n: torch.full((n + 4,), SENT, device="cuda")                      # noqa: E731
    gates, w, h0, c0, keep = new(TM * BM * NM * 4 * HM), new(4 * HM * HM), new(BM * HM), new(BM * HM), new(TM * BM)
    out, hm, cm, hl, cl = new(TM * BM * NM * HM), new((TM + 1) * BM * HM), new((TM + 1) * BM * HM), new(BM * HM), new(BM * HM)
    d_out, S, dh, dc = new(TM * BM * NM * HM), new(TM * BM * 4 * HM), new(BM * HM), new(BM * HM)
    off = lambda t: C.c_void_p(t.data_ptr() + 4)                                   # noqa: E731  (4 bytes off the 16-byte grid)
    fwd = [T, B, N, H, ptr(gates), ptr(w), ptr(h0), ptr(c0), ptr(keep), ptr(out), ptr(hm), ptr(cm), None, None, 1, stream()]
    bwd = [T, B, N, H, ptr(gates), ptr(w), ptr(cm), ptr(d_out), ptr(keep), ptr(S), ptr(dh), ptr(dc), stream()]
    assert lib.mirl_lstm_ms_supported(T, B, N, H) == 1
    shapes = [(0, 0), (0, -1), (1, 0), (1, -1), (2, 1), (2, 65), (2, 0), (3, 8), (3, 24), (3, 1040), (3, 0)]
    for pos, bad in shapes:
        dims = [T, B, N, H]
        dims[pos] = bad
        assert lib.mirl_lstm_ms_supported(*dims) == 0, dims
    fwd_last = list(fwd)
    fwd_last[12], fwd_last[13] = ptr(hl), ptr(cl)
    fwd_bad = shapes + [(p, None) for p in range(4, 12)] + [(12, ptr(hl)), (13, ptr(cl))] + \
        [(p, off(t)) for p, t in ((4, gates), (5, w), (6, h0), (7, c0), (9, out), (10, hm), (11, cm))]
    for need_grad in (0, 1):
        for pos, bad in fwd_bad:
            a = list(fwd)
            a[pos], a[14] = bad, need_grad
            assert lib.mirl_lstm_ms_fwd(*a) == ERR_ARG, (pos, bad)
    for pos, bad in shapes + [(12, None), (13, None), (12, off(hl)), (13, off(cl))]:
        a = list(fwd_last)
        a[pos] = bad
        assert lib.mirl_lstm_ms_fwd(*a) == ERR_ARG, (pos, bad)
    bwd_bad = shapes + [(p, None) for p in range(4, 12)] + \
        [(p, off(t)) for p, t in ((4, gates), (5, w), (6, cm), (7, d_out), (9, S), (10, dh), (11, dc))]
    for pos, bad in bwd_bad:
        a = list(bwd)
        a[pos] = bad
        assert lib.mirl_lstm_ms_bwd(*a) == ERR_ARG, (pos, bad)
    torch.cuda.synchronize()
    for name, t in dict(gates=gates, out=out, hm=hm, cm=cm, hl=hl, cl=cl, S=S, dh=dh, dc=dc, w=w, h0=h0, c0=c0, d_out=d_out).items():
        assert bool((t == SENT).all()), name


def _module_pass(m, T, B, N, H, grad=True):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(T * B * N, R.I, generator=g).cuda()
    hx, cx = torch.randn(T * B, H, generator=g).cuda(), torch.randn(T * B, H, generator=g).cuda()
    initials = (torch.rand(T * B, generator=g) < 0.3).float().cuda()
    up = torch.randn(T * B * N, H, generator=g).cuda()
    if not grad:
        with torch.no_grad():
            out = m(x, hx=hx, cx=cx, initials=initials, timesteps=T)
        return [out, m.last_state[0], m.last_state[1]]
    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    out = m(xi, hx=hx, cx=cx, initials=initials, timesteps=T)
    (out * up).sum().backward()
    return [out.detach(), m.last_state[0], m.last_state[1], xi.grad] + [q.grad for q in m.parameters()]


def _spy(monkeypatch):
    from rltime_amd.models.torch import lstm_seq
    calls = []
    real = lstm_seq.lib.mirl_lstm_ms_fwd
    monkeypatch.setattr(lstm_seq.lib, "mirl_lstm_ms_fwd", lambda *a: calls.append(a[:4] + (a[14],)) or real(*a))
    return calls


def test_an_unsupported_width_takes_the_torch_loop(monkeypatch):
    from rltime_amd.models.torch import lstm_seq
    from rltime_amd.models.torch.modules import LSTM
    T, B, N, H = 3, 5, 3, 24
    assert not lstm_seq.multi_supported(T, B, N, H)
    calls = _spy(monkeypatch)
    torch.manual_seed(5)
    a = LSTM((R.I,), H, multi_sample_merge_mode="inner").cuda()
    b = copy.deepcopy(a)
    b.fused = False
    res = [_module_pass(m, T, B, N, H) for m in (a, b)]
    assert not calls
    assert len(res[0]) == 8 and all(torch.equal(u, v) for u, v in zip(*res))


def test_no_grad_reaches_the_op_with_need_grad_0(monkeypatch):
    from rltime_amd.models.torch.modules import LSTM
    T, B, N, H = 3, 5, 3, 32
    calls = _spy(monkeypatch)
    torch.manual_seed(5)
    m = LSTM((R.I,), H, multi_sample_merge_mode="inner").cuda()
    quiet = _module_pass(m, T, B, N, H, grad=False)
    assert calls == [(T, B, N, H, 0)]
    assert not any(t.requires_grad for t in quiet)
    tracked = _module_pass(m, T, B, N, H)
    assert calls == [(T, B, N, H, 0), (T, B, N, H, 1)]
    assert all(torch.equal(u, v) for u, v in zip(quiet, tracked[:3]))
