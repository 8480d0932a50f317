"""GPU: the three kernels of csrc/actor_critic.hip through their C entry points (ctypes) against the float64 restatements of
tests/actor_critic_restate.py (proved on the CPU by tests/test_actor_critic_restate_cpu.py).

The kernels compute in float64 on float32 inputs and round every output once (include/mirl.h), so the bounds are first
order and short: 2^-24 of the value for the rounding, 2^-40 of the magnitudes added up for the float64 operations (exp, log
and pow of the device library are within an ulp of float64).  Output buffers are NaN-filled (integers: a sentinel) with one
guard row that must stay untouched.  Every quantity prints a RATIO line (largest error over its bound); above 1 fails."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import actor_critic_restate as R

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _lib():
    from rltime_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ratio(name, got, want, bound):
    r = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / bound)) if np.size(want) else 0.0
    print("RATIO %s %.4f" % (name, r))
    assert np.all(np.isfinite(np.asarray(got, dtype=np.float64))), name
    return r


# ---- head --------------------------------------------------------------------------------------------------------------------
def _head(logits, values, u, greedy, pitch=None):
    L = _lib()
    E, A = logits.shape
    pitch = pitch or A
    z = torch.full((E, pitch), NAN, device="cuda")
    z[:, :A] = _dev(logits)
    acts = torch.full((E + 1,), -7, dtype=torch.int32, device="cuda")
    block = torch.full((E + 1, 2), NAN, device="cuda")
    vd, ud = _dev(values), (_dev(u) if u is not None else None)           # (named: a temporary would be freed before the launch)
    L.check(L.lib.mirl_actor_head_ac(E, A, _p(z), pitch, _p(vd), _p(ud), int(greedy),
                                     _p(acts), _p(block), _p(block[:, 1]), 2, _st()), "mirl_actor_head_ac")
    torch.cuda.synchronize()
    assert int(acts[E]) == -7 and bool(torch.isnan(block[E]).all()), "the guard row was written"
    return acts[:E].cpu().numpy().astype(np.int64), block[:E, 0].cpu().numpy(), block[:E, 1].cpu().numpy()


@pytest.mark.parametrize("A", R.HEAD_A)
@pytest.mark.parametrize("E", R.HEAD_E)
def test_head_samples_the_restatements_action(E, A):
    logits, values, u = R.head_case(E, A)
    want_a, want_lp = R.head(logits, u)
    margin, bound = R.head_margin(logits, u)
    keep = margin > bound
    assert keep.sum() >= np.ceil(0.99 * E)                       # (all of them: test_actor_critic_restate_cpu.py)
    for pitch in (A, A + 3):
        acts, lp, vals = _head(logits, values, u, False, pitch)
        assert np.array_equal(acts[keep], want_a[keep])
        assert _ratio("head.logp E=%d A=%d" % (E, A), lp[keep], want_lp[keep], R.head_logp_bound(want_lp[keep])) <= 1.0
        assert np.array_equal(vals, values)
    acts, lp, _ = _head(logits, values, None, True, A + 1)
    want_g, want_glp = R.head(logits, greedy=True)
    assert np.array_equal(acts, want_g)
    assert _ratio("head.greedy_logp", lp, want_glp, R.head_logp_bound(want_glp)) <= 1.0


def test_head_greedy_takes_the_first_maximum_and_bad_shapes_are_refused():
    L = _lib()
    logits, values, first = R.head_tie_case(65, 18)
    acts, lp, _ = _head(logits, values, None, True)
    assert np.array_equal(acts, first)
    z, v, u = torch.zeros(4, 65, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    a, b = torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((4, 2), NAN, device="cuda")
    for E, A, uu, greedy in [(4, 65, u, 0), (0, 6, u, 0), (4, 0, u, 0), (4, 6, None, 0), (4, 6, u, 2)]:
        rc = L.lib.mirl_actor_head_ac(E, A, _p(z), 65, _p(v), _p(uu), greedy, _p(a), _p(b), _p(b[:, 1]), 2, _st())
        assert rc == L.MIRL_ERR_ARG, (E, A)
    assert L.lib.mirl_actor_head_ac(4, 6, _p(z), 5, _p(v), _p(u), 0, _p(a), _p(b), _p(b[:, 1]), 2, _st()) == L.MIRL_ERR_ARG
    torch.cuda.synchronize()
    assert bool((a == -7).all()) and bool(torch.isnan(b).all())


def test_head_action_frequencies_follow_the_softmax():
    n = 65536
    row = np.array([0.3, -1.2, 2.0, 0.0, -3.0, 1.1], dtype=np.float32)
    p = np.exp(row.astype(np.float64) - row.max())
    p /= p.sum()
    g = torch.Generator(device="cuda").manual_seed(12)
    u = torch.rand(n, device="cuda", generator=g)
    acts, lp, _ = _head(np.tile(row, (n, 1)), np.zeros(n, np.float32), u.cpu().numpy(), False)
    counts = np.bincount(acts, minlength=6)
    assert np.all(np.abs(counts - n * p) <= 5.0 * np.sqrt(n * p * (1 - p))), (counts, n * p)
    assert np.allclose(lp, np.log(p)[acts], rtol=1e-6, atol=1e-7)


# ---- window ------------------------------------------------------------------------------------------------------------------
_KINDS = ("u8", "f32", "u8odd")


def _window(T, B, n, gamma, lam, c):
    L = _lib()
    obs = _dev(c["obs"])
    row_bytes = int(np.prod(c["obs"].shape[2:])) * c["obs"].itemsize
    pol = torch.stack([_dev(c["logp"]), _dev(c["values"])], dim=-1).contiguous()           # (cap, E, 2): [log-prob | value]
    f32 = lambda: torch.full((T + 1, B), NAN, device="cuda")                                # noqa: E731
    ret, ns, mk, lp, val = f32(), f32(), f32(), f32(), f32()
    acts = torch.full((T + 1, B), -7, dtype=torch.int32, device="cuda")
    st = torch.full((2, T + 1, B, row_bytes), 0xA5, dtype=torch.uint8, device="cuda")
    plan, ra, rr, rd = _dev(c["plan"]), _dev(c["actions"]), _dev(c["rewards"]), _dev(c["dones"])
    L.check(L.lib.mirl_online_window(T, B, c["E"], c["cap"], n, gamma, lam, row_bytes, _p(plan), _p(obs), _p(ra),
                                     _p(rr), _p(rd), _p(pol), _p(pol.view(-1)[1:]), 2, _p(ret), _p(ns), _p(mk),
                                     _p(acts), _p(lp), _p(val), _p(st[0]), _p(st[1]), _st()), "mirl_online_window")
    torch.cuda.synchronize()
    for t in (ret, ns, mk, lp, val):
        assert bool(torch.isnan(t[T]).all()), "the guard row was written"
    assert bool((acts[T] == -7).all()) and bool((st[:, T] == 0xA5).all()), "the guard row was written"
    shape = (T, B) + c["obs"].shape[2:]
    view = lambda x: x[:T].contiguous().cpu().numpy().view(c["obs"].dtype).reshape(shape)   # noqa: E731
    return {"returns": ret[:T].cpu().numpy(), "nsteps": ns[:T].cpu().numpy(), "target_masks": mk[:T].cpu().numpy(),
            "actions": acts[:T].cpu().numpy(), "action_log_probs": lp[:T].cpu().numpy(), "values": val[:T].cpu().numpy(),
            "states": view(st[0]), "target_states": view(st[1])}


@pytest.mark.parametrize("B", R.WINDOW_B)
@pytest.mark.parametrize("T", R.WINDOW_T)
def test_window_equals_the_restatement(T, B):
    gamma, lam = 0.99, 0.95
    for i, n in enumerate(R.window_nsteps(T)):
        kind = _KINDS[(i + T + B) % 3] if T > 5 else None
        for kd in ((kind,) if kind else _KINDS):
            c = R.window_case(T, B, kd, seed=31 * T + 7 * B + n)
            want = R.window(T, B, c["E"], c["cap"], n, gamma, lam, c["plan"], c["obs"], c["actions"], c["rewards"], c["dones"],
                            c["logp"], c["values"])
            got = _window(T, B, n, gamma, lam, c)
            for key in ("nsteps", "target_masks", "actions", "action_log_probs", "values", "states", "target_states"):
                assert np.array_equal(got[key], want[key]), (key, T, B, n, kd)
            assert _ratio("window.returns T=%d B=%d n=%d" % (T, B, n), got["returns"], want["returns"], R.window_bound(want) + 1e-300) <= 1.0
            again = _window(T, B, n, gamma, lam, c)
            assert all(np.array_equal(got[k], again[k]) for k in got)


def test_window_refuses_bad_arguments():
    L = _lib()
    x = torch.zeros(64, device="cuda")
    xi = torch.zeros(64, dtype=torch.int32, device="cuda")
    xb = torch.zeros(256, dtype=torch.uint8, device="cuda")

    def call(T=2, B=1, E=1, cap=4, n=1, obs_bytes=4, plan=xi):
        return L.lib.mirl_online_window(T, B, E, cap, n, 0.99, 0.95, obs_bytes, _p(plan), _p(xb), _p(xi), _p(x), _p(xb), _p(x), _p(x), 1,
                                        _p(x), _p(x), _p(x), _p(xi), _p(x), _p(x), _p(xb), _p(xb), _st())
    for kw in (dict(T=0), dict(B=0), dict(E=0), dict(cap=1), dict(n=0), dict(obs_bytes=0), dict(plan=None)):
        assert call(**kw) == L.MIRL_ERR_ARG, kw


# ---- loss --------------------------------------------------------------------------------------------------------------------
def _loss(c, old, vf, ef, clip, adv_norm, pitch_extra=0, want_logp=True):
    L = _lib()
    M, A = c["logits"].shape
    z = torch.full((M, A + pitch_extra), NAN, device="cuda")
    z[:, :A] = _dev(c["logits"])
    dz = torch.full((M + 1, A + pitch_extra), NAN, device="cuda")
    dv, lp = torch.full((M + 1,), NAN, device="cuda"), torch.full((M + 1,), NAN, device="cuda")
    stats = torch.full((6,), NAN, device="cuda")
    v, a, t, b = _dev(c["values"]), _dev(c["actions"]), _dev(c["targets"]), _dev(c["acting"])
    o = _dev(old) if old is not None else None
    L.check(L.lib.mirl_ac_loss(M, A, _p(z), A + pitch_extra, _p(v), _p(a), _p(t),
                               _p(b), _p(o), vf, ef, clip if clip is not None else 0.0,
                               int(adv_norm), _p(dz), A + pitch_extra, _p(dv), _p(lp) if want_logp else None, _p(stats), _st()), "mirl_ac_loss")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dz[M]).all()) and bool(torch.isnan(dv[M])) and bool(torch.isnan(lp[M])) and bool(torch.isnan(stats[5]))
    assert pitch_extra == 0 or bool(torch.isnan(dz[:M, A:]).all())
    return {"stats": stats[:5].cpu().numpy(), "dlogits": dz[:M, :A].cpu().numpy(), "dvalues": dv[:M].cpu().numpy(),
            "log_probs": lp[:M].cpu().numpy()}


@pytest.mark.parametrize("A", R.LOSS_A)
@pytest.mark.parametrize("M", R.LOSS_M)
def test_loss_stays_inside_its_bounds(M, A):
    vf, clip = 0.5, 0.2
    worst = 0.0
    for ppo in (False, True):
        c = R.loss_case(M, A, seed=1000 * M + 10 * A + ppo, ppo=ppo)
        for adv_norm in (False, True):
            for ef in (0.0, 0.01):
                want = R.loss(c["logits"], c["values"], c["actions"], c["targets"], c["acting"], c["old"], vf, ef, clip if ppo else None, adv_norm)
                got = _loss(c, c["old"], vf, ef, clip if ppo else None, adv_norm, pitch_extra=(M + A) % 3)
                bounds = R.loss_bounds(want, vf, ef, ppo)
                tag = "M=%d A=%d %s norm=%d ef=%g" % (M, A, "ppo" if ppo else "a2c", adv_norm, ef)
                assert np.array_equal(got["log_probs"].astype(np.float64), want["log_probs"]), tag
                for key in ("stats", "dlogits", "dvalues"):
                    worst = max(worst, _ratio("loss.%s %s" % (key, tag), got[key], want[key], bounds[key]))
                # exact: no value gradient where the target equals the value; nothing flows where the clamped term is strictly smaller
                assert np.all(got["dvalues"][c["targets"] == c["values"]] == 0)
                if ppo and ef == 0.0:
                    clipped = (want["coef"] == 0) & (want["adv"] != 0)
                    assert M < 255 or clipped.sum() > 0
                    assert np.all(got["dlogits"][clipped] == 0), tag
                again = _loss(c, c["old"], vf, ef, clip if ppo else None, adv_norm, pitch_extra=(M + A) % 3)
                assert all(np.array_equal(got[k], again[k]) for k in got), tag
    assert worst <= 1.0


@pytest.mark.parametrize("M,A", [(7, 2), (257, 6), (2048, 18)])
def test_loss_fed_its_own_log_probs_has_ratio_one(M, A):
    """The kernel's log_probs as old_log_probs: every ratio is exactly 1, so the PPO policy gradient is the A2C one bit for
    bit, and the gain is the mean advantage."""
    c = R.loss_case(M, A, seed=77 + M, ppo=False)
    for adv_norm in (False, True):
        a2c = _loss(c, None, 0.5, 0.01, None, adv_norm)
        ppo = _loss(c, a2c["log_probs"], 0.5, 0.01, 0.2, adv_norm)
        assert np.array_equal(ppo["dlogits"], a2c["dlogits"]) and np.array_equal(ppo["dvalues"], a2c["dvalues"])
        assert np.array_equal(ppo["log_probs"], a2c["log_probs"])
        want = R.loss(c["logits"], c["values"], c["actions"], c["targets"], c["acting"], a2c["log_probs"], 0.5, 0.01, 0.2, adv_norm)
        assert np.all(want["ratio"] == 1.0)
        b = R.loss_bounds(want, 0.5, 0.01, True)
        assert _ratio("loss.stats ratio-one M=%d" % M, ppo["stats"], want["stats"], b["stats"]) <= 1.0
        none = _loss(c, None, 0.5, 0.01, None, adv_norm, want_logp=False)           # log_probs is optional
        assert np.array_equal(none["dlogits"], a2c["dlogits"]) and np.all(np.isnan(none["log_probs"]))


def test_loss_refuses_bad_arguments():
    L = _lib()
    x = torch.zeros(64, device="cuda")
    xi = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.full((64,), NAN, device="cuda")

    def call(M=4, A=2, pitch=2, adv_norm=0, old=None, clip=0.2, values=x):
        return L.lib.mirl_ac_loss(M, A, _p(x), pitch, _p(values), _p(xi), _p(x), _p(x), _p(old), 0.5, 0.01, clip, adv_norm, _p(out), pitch,
                                  _p(out), _p(out), _p(out), _st())
    for kw in (dict(M=1, adv_norm=1), dict(M=0), dict(A=0), dict(A=65, pitch=65), dict(pitch=1), dict(adv_norm=2), dict(values=None),
               dict(old=x, clip=-0.1)):
        assert call(**kw) == L.MIRL_ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call(M=1, adv_norm=0) == 0                                # one row without normalisation is fine
