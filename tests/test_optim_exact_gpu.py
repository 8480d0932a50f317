"""GPU: mirl_adam_clip_step (csrc/optim.hip: k_adam_sqsum, k_adam_update) at its C entry point against the float64
restatement of clip_grad_norm_ + Adam in tests/pointwise_restate.py.

Norm: with dyadic gradients (small integers * 2^-3, sum of squares exact in float32 per lane and in float64 across lanes)
norm_out[0] is bit-equal to float32(sqrt(float64 sum)); with real gradients within 17 u relative (16 float32 additions per
lane, the final rounding), u = 2^-24.

One step, first order, per element (w1 = 1 - beta1, w2 = 1 - beta2, bs = sqrt(1 - beta2^t), ss = lr / (1 - beta1^t), t from
the tensor's own counter; the bias corrections are formed in float64 and rounded once):
  g' = g coef            e_g = 21 u |g'| when the clip bites (norm 17 u, + 1e-6, float32(clip), the division, the product), else 0
  m' = m + w1 (g' - m)   e_m = w1 e_g + 3 u |w1 (g' - m)| + u |m'|                 (float32(w1), difference, product; the sum)
  v' = v b2 + w2 g' g'   e_v = 2 u |v b2| + 3 u w2 g'^2 + 2 w2 |g'| e_g + u |v'|
  den = sqrt(v') / bs + eps   e_den = (e_v / (2 sqrt v') + 3 u sqrt v') / bs + u eps + u den
  r = m' / den           e_r = e_m / den + |r| e_den / den + u |r|
  p' = p - ss r          e_p = ss e_r + 2 u |ss r| + u |p'|
Over 5 steps the kernel's distance from float64 torch Adam is at most 4 x that of float32 torch Adam, or the sum of the
one-step bounds of the steps taken (the floor)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import pointwise_restate as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ERR_ARG = -1
SIZES = [1, 255, 4095, 4096, 4097, 8192, 12289]
HYP = dict(lr=float(np.float32(2.5e-4)), b1=0.9, b2=0.999, eps=1.5e-4)


def _lib():
    from rltime_amd import _lib
    return _lib


def _view(x64, offset):
    """A float32 device copy; offset: a view starting one float into its storage (4 bytes off the 16-byte boundary)."""
    if not offset:
        return x64.float().cuda()
    store = torch.zeros(x64.numel() + 1, device="cuda")
    store[1:] = x64.float().cuda()
    return store[1:]


class Tensors:
    def __init__(self, seed, sizes, steps, dyadic=False, gscale=0.1, offset=()):
        g = torch.Generator().manual_seed(seed)
        self.sizes, self.n = list(sizes), len(sizes)
        self.g64 = R.dyadic_grads(seed, sizes, k=3, amp=5)[0] if dyadic else [(torch.randn(n, generator=g) * gscale).double() for n in sizes]
        self.margin = R.dyadic_grads(seed, sizes, k=3, amp=5)[1] if dyadic else None
        self.p64 = [(torch.randn(n, generator=g) * 0.1).double() for n in sizes]
        self.m64 = [(torch.randn(n, generator=g) * 0.01).double() * (s > 0) for n, s in zip(sizes, steps)]
        self.v64 = [(torch.rand(n, generator=g) * 1e-4).double() * (s > 0) for n, s in zip(sizes, steps)]
        self.steps = list(steps)
        off = [i in offset for i in range(self.n)]
        self.p, self.g, self.m, self.v = ([_view(x, o) for x, o in zip(xs, off)] for xs in (self.p64, self.g64, self.m64, self.v64))
        self.step = [torch.tensor([float(s)], device="cuda") for s in steps]
        for i in offset:
            assert self.g[i].data_ptr() % 16 == 4 and self.p[i].data_ptr() % 16 == 4

    def run(self, clip, lr_dev=None, ws=None, ws_bytes=None, hyp=HYP):
        L = _lib()
        n = self.n
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])                   # noqa: E731
        numel = (C.c_int64 * n)(*self.sizes)
        if ws is None:
            need = C.c_int64()
            L.check(L.lib.mirl_adam_clip_workspace_bytes(n, numel, C.byref(need)), "mirl_adam_clip_workspace_bytes")
            chunks = sum(-(-s // 4096) for s in self.sizes)
            assert need.value == 8 * (chunks + n)
            ws, ws_bytes = torch.zeros(need.value // 8, dtype=torch.float64, device="cuda"), need.value
        out = torch.full((3,), float("nan"), device="cuda")
        rc = L.lib.mirl_adam_clip_step(n, arr(self.p), arr(self.g), arr(self.m), arr(self.v), arr(self.step), numel, hyp["lr"],
                                       C.c_void_p(lr_dev.data_ptr()) if lr_dev is not None else None, hyp["b1"], hyp["b2"], hyp["eps"],
                                       float(clip), C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(out.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        self.ws = ws
        return rc, out.cpu()


def _bound(p, g, m, v, step, coef, biting, hyp=HYP):
    """-> ((p', g', m', v') in float64, their first-order bounds) following the module docstring."""
    lr, b1, b2, eps = hyp["lr"], hyp["b1"], hyp["b2"], hyp["eps"]
    p2, gc, m2, v2, t = R.adam_step(p, g, m, v, step, lr, b1, b2, eps, coef)
    ss, bs, w1, w2 = lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t), 1 - b1, 1 - b2
    e_g = 21 * U * gc.abs() if biting else torch.zeros_like(gc)
    e_m = w1 * e_g + 3 * U * (w1 * (gc - m)).abs() + U * m2.abs()
    e_v = 2 * U * (v * b2).abs() + 3 * U * w2 * gc * gc + 2 * w2 * gc.abs() * e_g + U * v2.abs()
    sq = v2.sqrt()
    e_sq = torch.where(sq > 0, e_v / (2 * sq).clamp(min=1e-300), torch.zeros_like(sq))
    den = sq / bs + eps
    e_den = (e_sq + 3 * U * sq) / bs + U * eps + U * den
    r = m2 / den
    e_r = e_m / den + r.abs() * e_den / den + U * r.abs()
    e_p = ss * e_r + 2 * U * (ss * r).abs() + U * p2.abs()
    return (p2, gc, m2, v2), (e_p, e_g, e_m, e_v)


def _check_step(ts, clip, tag):
    """One call on `ts`: every tensor's p, g, m, v inside the one-step bound of ITS step counter; counters advanced by one."""
    rc, out = ts.run(clip)
    assert rc == 0, _lib().last_error()
    norm = R.global_norm(ts.g64)
    coef = R.clip_coef(norm, clip)
    worst = {}
    for i in range(ts.n):
        want, bnd = _bound(ts.p64[i], ts.g64[i], ts.m64[i], ts.v64[i], ts.steps[i], coef, coef < 1.0)
        for name, got, w, b in zip("pgmv", (ts.p[i], ts.g[i], ts.m[i], ts.v[i]), want, bnd):
            err = (got.cpu().double() - w).abs()
            ok = err <= b
            worst[name] = max(worst.get(name, 0.0), float((err / b.clamp(min=1e-300)).max()))
            assert bool(ok.all()), "%s tensor %d (%d elements, step %d) %s: err / bound %.3f at element %d" % (
                tag, i, ts.sizes[i], ts.steps[i], name, float((err / b.clamp(min=1e-300)).max()), int((~ok).nonzero()[0]))
        assert float(ts.step[i]) == ts.steps[i] + 1
    print("RATIO k_adam_update %s: worst err / bound p %.3f g %.3f m %.3f v %.3f" % (tag, worst["p"], worst["g"], worst["m"], worst["v"]))
    # the latched steps sit behind the chunk partials, at tensor_base + k
    chunks = sum(-(-s // 4096) for s in ts.sizes)
    assert ts.ws.cpu()[chunks:chunks + ts.n].tolist() == [float(s + 1) for s in ts.steps]
    return out, norm, coef


def _layout(count):
    sizes = [SIZES[-1]] if count == 1 else [SIZES[i % 7] for i in range(count)]
    steps = [(0, 9, 999)[i % 3] for i in range(count)]                  # i and i + 32 always differ
    return sizes, steps


@pytest.mark.parametrize("clip", [0.0, 1e6, 0.25], ids=["noclip", "slack", "biting"])
@pytest.mark.parametrize("count", [1, 32, 33, 64, 65])
def test_launch_split_steps_and_exact_norm(count, clip):
    """1, 2 and 3 launches per pass; dyadic gradients: the norm over every launch's partials is exact."""
    sizes, steps = _layout(count)
    offset = (sizes.index(8192),) if 8192 in sizes else ()
    ts = Tensors(10 + count, sizes, steps, dyadic=True, offset=offset)
    assert ts.margin < 2 ** 24
    g_before = [g.clone() for g in ts.g]
    out, norm, coef = _check_step(ts, clip, "count %d clip %g" % (count, clip))
    want_norm = np.float32(np.sqrt(np.float64(sum(float((g ** 2).sum()) for g in ts.g64))))
    assert float(out[0]) == float(want_norm), (float(out[0]), float(want_norm))
    assert math.isnan(float(out[2]))
    if clip == 0.25:
        assert coef < 0.9
        c32 = torch.minimum(torch.tensor(clip, dtype=torch.float32) / (out[0] + torch.tensor(1e-6, dtype=torch.float32)), torch.tensor(1.0))
        assert abs(float(c32) - coef) <= 4 * U * coef
        for a, b in zip(ts.g, g_before):
            assert torch.equal(a.cpu(), b.cpu() * c32), "the clipped gradient is not the float32 product with the coefficient"
        assert float(out[1]) == float(out[0] * c32)
    else:
        assert coef == 1.0 and float(out[1]) == float(out[0])
        assert all(torch.equal(a, b) for a, b in zip(ts.g, g_before)), "a clip that does not bite changed the gradients"


@pytest.mark.parametrize("count", [7, 33])
def test_real_gradient_norm_within_17_u(count):
    sizes, steps = _layout(count)
    ts = Tensors(50 + count, sizes, steps, offset=(sizes.index(8192),))
    out, norm, _ = _check_step(ts, 0.0, "real count %d" % count)
    rel = abs(float(out[0]) - norm) / norm
    print("RATIO k_adam_sqsum norm: rel err / (17 u) = %.3f" % (rel / (17 * U)))
    assert rel <= 17 * U


def test_lr_from_a_device_pointer_equals_lr_by_value():
    sizes, steps = _layout(7)
    a, b = Tensors(60, sizes, steps), Tensors(60, sizes, steps)
    assert a.run(0.3)[0] == 0
    bad = dict(HYP, lr=-1.0)                                           # ignored when the pointer is given
    assert b.run(0.3, lr_dev=torch.tensor([HYP["lr"]], device="cuda"), hyp=bad)[0] == 0
    for x, y in zip(a.p + a.m + a.v + a.g, b.p + b.m + b.v + b.g):
        assert torch.equal(x, y)


@pytest.mark.parametrize("clip", [None, 0.25])
def test_five_steps_against_float64_torch_adam(clip):
    sizes, steps = _layout(7)
    ts = Tensors(70, sizes, [0] * 7, offset=(sizes.index(8192),))
    lr, b1, b2, eps = HYP["lr"], HYP["b1"], HYP["b2"], HYP["eps"]
    r64 = [torch.nn.Parameter(p.clone()) for p in ts.p64]
    r32 = [torch.nn.Parameter(p.float()) for p in ts.p64]
    o64, o32 = (torch.optim.Adam(ps, lr=lr, betas=(b1, b2), eps=eps) for ps in (r64, r32))
    gen = torch.Generator().manual_seed(71)
    floor = [torch.zeros(n, dtype=torch.float64) for n in sizes]
    for step in range(5):
        grads = [(torch.randn(n, generator=gen) * (0.3 if step % 2 else 0.01)).double() for n in sizes]
        norm = R.global_norm(grads)
        coef = R.clip_coef(norm, clip)
        for i in range(7):
            st = o64.state[r64[i]]
            m, v = (st["exp_avg"], st["exp_avg_sq"]) if st else (torch.zeros_like(grads[i]), torch.zeros_like(grads[i]))
            floor[i] += _bound(r64[i].detach(), grads[i], m, v, step, coef, coef < 1.0)[1][0]
            r64[i].grad, r32[i].grad = grads[i].clone(), grads[i].float()
            ts.g[i].copy_(grads[i].float())
        ts.g64 = grads
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(r64, clip), torch.nn.utils.clip_grad_norm_(r32, clip)
        o64.step(), o32.step()
        assert ts.run(clip or 0.0)[0] == 0
    worst = 0.0
    for i in range(7):
        err = (ts.p[i].cpu().double() - r64[i].detach()).abs()
        err32 = float((r32[i].detach().double() - r64[i].detach()).abs().max())
        worst = max(worst, float(err.max()) / max(err32, 1e-300))
        assert bool((err <= torch.clamp(floor[i], min=4 * err32)).all()), (i, float(err.max()), err32, float(floor[i].max()))
        for mine, key in ((ts.m[i], "exp_avg"), (ts.v[i], "exp_avg_sq")):
            w64, w32 = o64.state[r64[i]][key], o32.state[r32[i]][key]
            e, e32 = float((mine.cpu().double() - w64).abs().max()), float((w32.double() - w64).abs().max())
            assert e <= max(4 * e32, 25 * U * float(w64.abs().max())), (i, key, e, e32)
        assert float(ts.step[i]) == 5.0
    print("RATIO k_adam_update 5 steps clip %s: worst err / float32 torch Adam err = %.3f" % (clip, worst))


def test_refusals():
    L = _lib()
    sizes, steps = [4097, 5], [0, 3]
    ts = Tensors(80, sizes, steps)
    before = [x.clone() for x in ts.p + ts.g + ts.m + ts.v]
    need = 8 * (3 + 2)
    ws = torch.zeros(need // 8 + 2, dtype=torch.float64, device="cuda")
    assert ts.run(1.0, ws=ws, ws_bytes=need - 1)[0] == ERR_ARG and "workspace" in L.last_error()
    mis = ws.view(torch.float32)[1:]                                   # 4 bytes off an 8-byte boundary
    assert mis.data_ptr() % 8 == 4
    assert ts.run(1.0, ws=mis, ws_bytes=need)[0] == ERR_ARG and "misaligned" in L.last_error()
    assert ts.run(1.0, hyp=dict(HYP, b1=1.0))[0] == ERR_ARG
    assert ts.run(1.0, hyp=dict(HYP, b2=1.0))[0] == ERR_ARG
    assert ts.run(1.0, hyp=dict(HYP, lr=-1e-3))[0] == ERR_ARG
    numel = (C.c_int64 * 2)(*sizes)
    arr = (C.c_void_p * 2)(*[t.data_ptr() for t in ts.p])
    assert L.lib.mirl_adam_clip_step(0, arr, arr, arr, arr, arr, numel, 1e-3, None, 0.9, 0.999, 1e-8, 1.0, C.c_void_p(ws.data_ptr()), need, None, None) == ERR_ARG
    ts.sizes = [4097, 0]
    assert ts.run(1.0, ws=ws, ws_bytes=need)[0] == ERR_ARG and "empty" in L.last_error()
    out = C.c_int64(-7)
    assert L.lib.mirl_adam_clip_workspace_bytes(2, (C.c_int64 * 2)(4097, 0), C.byref(out)) == ERR_ARG and out.value == -7
    assert L.lib.mirl_adam_clip_workspace_bytes(0, (C.c_int64 * 2)(4097, 5), C.byref(out)) == ERR_ARG
    torch.cuda.synchronize()
    for x, y in zip(ts.p + ts.g + ts.m + ts.v, before):
        assert torch.equal(x, y), "a refused call changed a tensor"
    assert [float(s) for s in ts.step] == [0.0, 3.0]
