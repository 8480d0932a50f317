"""GPU: the Normal-head kernels of csrc/actor_critic.hip through their C entry points (ctypes) against the float64
restatements of tests/normal_head_restate.py (proved on the CPU by tests/test_normal_head_restate_cpu.py).

The kernels compute in float64 on float32 inputs and round every output once (include/mirl.h), so the bounds are first
order and short: 2^-24 of the value for the rounding, 2^-40 of the magnitudes added up for the float64 operations.  Output
buffers are NaN-filled with one guard row that must stay untouched.  Every quantity prints a RATIO line (largest error over
its bound); above 1 fails.  Helpers are tests/test_actor_critic_kernels_gpu.py's."""
import numpy as np
import pytest
import torch

from tests import actor_critic_restate as R
from tests import normal_head_restate as N
from tests import test_actor_critic_kernels_gpu as K

pytestmark = pytest.mark.gpu

NAN = float("nan")
_lib, _p, _st, _dev, _ratio = K._lib, K._p, K._st, K._dev, K._ratio


# ---- head --------------------------------------------------------------------------------------------------------------------
def _head(mean, logstd, values, eps, pitch):
    L = _lib()
    E, D = mean.shape
    m = torch.full((E, pitch), NAN, device="cuda")
    m[:, :D] = _dev(mean)
    acts = torch.full((E + 1, D), NAN, device="cuda")
    block = torch.full((E + 1, 2), NAN, device="cuda")
    ls, vd, ed = _dev(logstd), _dev(values), _dev(eps)
    L.check(L.lib.mirl_actor_head_normal(E, D, _p(m), pitch, _p(ls), _p(vd), _p(ed), _p(acts), _p(block), _p(block[:, 1]), 2, _st()),
            "mirl_actor_head_normal")
    torch.cuda.synchronize()
    assert bool(torch.isnan(acts[E]).all()) and bool(torch.isnan(block[E]).all()), "the guard row was written"
    return acts[:E].cpu().numpy(), block[:E, 0].cpu().numpy(), block[:E, 1].cpu().numpy()


@pytest.mark.parametrize("D", N.HEAD_D)
@pytest.mark.parametrize("E", N.HEAD_E)
def test_head_equals_the_restatement(E, D):
    mean, logstd, values, eps = N.head_case(E, D)
    want_a, want_lp, mag = N.head(mean, logstd, eps)
    for pitch in (D, D + 3):
        acts, logp, vals = _head(mean, logstd, values, eps, pitch)
        assert np.array_equal(acts.view(np.int32), want_a.view(np.int32)), (E, D, pitch)
        assert np.array_equal(vals, values)
        assert _ratio("head_normal.logp E=%d D=%d pitch=%d" % (E, D, pitch), logp, want_lp, N.head_logp_bound(want_lp, mag)) <= 1.0
        again = _head(mean, logstd, values, eps, pitch)
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip((acts, logp, vals), again))


def test_head_refuses_bad_arguments():
    L = _lib()
    x = torch.full((64,), NAN, device="cuda")

    def call(E=2, D=2, pitch=2, mean=x, logstd=x, values=x, eps=x, actions=x, logp=x, vout=x, out_pitch=2):
        return L.lib.mirl_actor_head_normal(E, D, _p(mean), pitch, _p(logstd), _p(values), _p(eps), _p(actions), _p(logp), _p(vout),
                                            out_pitch, _st())
    for kw in (dict(E=0), dict(E=2 ** 24 + 1), dict(D=0), dict(D=17), dict(pitch=1), dict(out_pitch=0), dict(mean=None), dict(logstd=None),
               dict(values=None), dict(eps=None), dict(actions=None), dict(logp=None), dict(vout=None)):
        assert call(**kw) == L.MIRL_ERR_ARG, kw
        assert "actor_head_normal" in L.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all())                                        # nothing was launched


# ---- window ------------------------------------------------------------------------------------------------------------------
def _window(T, B, n, c, W, box):
    L = _lib()
    obs = _dev(c["obs"])
    row_bytes = c["obs"].shape[2]
    pol = torch.stack([_dev(c["logp"]), _dev(c["values"])], dim=-1).contiguous()
    f32 = lambda: torch.full((T + 1, B), NAN, device="cuda")                                # noqa: E731
    ret, ns, mk, lp, val = f32(), f32(), f32(), f32(), f32()
    acts = torch.full((T + 1, B, W), -7, dtype=torch.int32, device="cuda")
    st = torch.full((2, T + 1, B, row_bytes), 0xA5, dtype=torch.uint8, device="cuda")
    plan, ra, rr, rd = _dev(c["plan"]), _dev(c["action_words"][:, :, :W]), _dev(c["rewards"]), _dev(c["dones"])
    args = [T, B, c["E"], c["cap"], n, 0.99, 0.95, row_bytes, _p(plan), _p(obs), _p(ra), _p(rr), _p(rd), _p(pol), _p(pol.view(-1)[1:]), 2,
            _p(ret), _p(ns), _p(mk), _p(acts), _p(lp), _p(val), _p(st[0]), _p(st[1])]
    if box:
        L.check(L.lib.mirl_online_window_box(*args, W, _st()), "mirl_online_window_box")
    else:
        L.check(L.lib.mirl_online_window(*args, _st()), "mirl_online_window")
    torch.cuda.synchronize()
    for t in (ret, ns, mk, lp, val):
        assert bool(torch.isnan(t[T]).all()), "the guard row was written"
    assert bool((acts[T] == -7).all()) and bool((st[:, T] == 0xA5).all()), "the guard row was written"
    return {"returns": ret[:T].cpu().numpy(), "nsteps": ns[:T].cpu().numpy(), "target_masks": mk[:T].cpu().numpy(),
            "actions": acts[:T].cpu().numpy(), "action_log_probs": lp[:T].cpu().numpy(), "values": val[:T].cpu().numpy(),
            "states": st[0, :T].cpu().numpy(), "target_states": st[1, :T].cpu().numpy()}


@pytest.mark.parametrize("obs_bytes", [8, 16])
@pytest.mark.parametrize("T,B", [(1, 1), (5, 3), (2, 16), (32, 3)])
def test_window_box_moves_the_action_words(T, B, obs_bytes):
    """action_words = 1: every output is mirl_online_window's byte for byte.  3: the words are gathered exactly — arbitrary
    bit patterns, NaN patterns among them — and everything else is unchanged.  The rings are wrapped by some sequences;
    obs_bytes = 8 (this env's row) takes the byte path, 16 the 16-byte path."""
    for n in R.window_nsteps(T)[:3]:
        c = N.window_box_case(T, B, obs_bytes, 3, seed=31 * T + 7 * B + n)
        assert B == 1 or any((c["plan"][b, 1] + T) > c["cap"] for b in range(B))
        one = dict(c, action_words=np.ascontiguousarray(c["action_words"][:, :, :1]))
        base, box1 = _window(T, B, n, one, 1, box=False), _window(T, B, n, one, 1, box=True)
        for k in base:
            assert np.array_equal(base[k].view(np.uint8), box1[k].view(np.uint8)), (k, T, B, n)
        want = N.window_box(T, B, c["E"], c["cap"], n, 0.99, 0.95, c["plan"], c["obs"], c["action_words"], c["rewards"], c["dones"],
                            c["logp"], c["values"])
        got = _window(T, B, n, c, 3, box=True)
        assert np.array_equal(got["actions"], want["actions"])
        for k in base:
            if k != "actions":
                assert np.array_equal(got[k].view(np.uint8), base[k].view(np.uint8)), (k, T, B, n)
        for key in ("nsteps", "target_masks", "action_log_probs", "values", "states", "target_states"):
            assert np.array_equal(got[key], want[key]), key
        assert _ratio("window_box.returns T=%d B=%d n=%d" % (T, B, n), got["returns"], want["returns"], R.window_bound(want) + 1e-300) <= 1.0


def test_window_box_refuses_bad_arguments():
    L = _lib()
    x = torch.zeros(64, device="cuda")
    xi = torch.zeros(64, dtype=torch.int32, device="cuda")
    xb = torch.zeros(256, dtype=torch.uint8, device="cuda")

    def call(T=2, B=1, E=1, cap=4, n=1, obs_bytes=4, plan=xi, W=2):
        return L.lib.mirl_online_window_box(T, B, E, cap, n, 0.99, 0.95, obs_bytes, _p(plan), _p(xb), _p(xi), _p(x), _p(xb), _p(x), _p(x), 1,
                                            _p(x), _p(x), _p(x), _p(xi), _p(x), _p(x), _p(xb), _p(xb), W, _st())
    for kw in (dict(T=0), dict(B=0), dict(E=0), dict(cap=1), dict(n=0), dict(obs_bytes=0), dict(plan=None), dict(W=0), dict(W=17)):
        assert call(**kw) == L.MIRL_ERR_ARG, kw
        assert "online_window_box" in L.last_error()


# ---- loss --------------------------------------------------------------------------------------------------------------------
def _loss(c, vf, ef, clip, adv_norm, pitch_extra=0, want_logp=True):
    L = _lib()
    M, D = c["mean"].shape
    m = torch.full((M, D + pitch_extra), NAN, device="cuda")
    m[:, :D] = _dev(c["mean"])
    dm = torch.full((M + 1, D + pitch_extra), NAN, device="cuda")
    dls = torch.full((D + 1,), NAN, device="cuda")
    dv, lp = torch.full((M + 1,), NAN, device="cuda"), torch.full((M + 1,), NAN, device="cuda")
    stats = torch.full((6,), NAN, device="cuda")
    ls, v, a, t, b = _dev(c["logstd"]), _dev(c["values"]), _dev(c["actions"]), _dev(c["targets"]), _dev(c["acting"])
    o = _dev(c["old"]) if c["old"] is not None else None
    L.check(L.lib.mirl_ac_loss_normal(M, D, _p(m), D + pitch_extra, _p(ls), _p(v), _p(a), _p(t), _p(b), _p(o), vf, ef,
                                      clip if clip is not None else 0.0, int(adv_norm), _p(dm), D + pitch_extra, _p(dls), _p(dv),
                                      _p(lp) if want_logp else None, _p(stats), _st()), "mirl_ac_loss_normal")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dm[M]).all()) and bool(torch.isnan(dv[M])) and bool(torch.isnan(lp[M])) and bool(torch.isnan(stats[5]))
    assert bool(torch.isnan(dls[D])) and (pitch_extra == 0 or bool(torch.isnan(dm[:M, D:]).all()))
    assert want_logp or bool(torch.isnan(lp).all())
    return {"stats": stats[:5].cpu().numpy(), "dmean": dm[:M, :D].cpu().numpy(), "dlogstd": dls[:D].cpu().numpy(),
            "dvalues": dv[:M].cpu().numpy(), "log_probs": lp[:M].cpu().numpy()}


@pytest.mark.parametrize("D", N.LOSS_D)
@pytest.mark.parametrize("M", N.LOSS_M)
def test_loss_stays_inside_its_bounds(M, D):
    """A2C and PPO, adv_norm off and on (M = 1: off only), entropy_factor 0 and > 0, pitches D and D + 3, log_probs asked for
    and NULL.  The kernel's float32 log-probabilities are held to their own bound; the other outputs to theirs against the
    restatement evaluated on those log-probabilities (the rows are the PPO mask's: none within the clip margin).  The
    launch without log_probs and a second launch repeat the first bit for bit."""
    vf, clip = 0.5, 0.2
    worst = 0.0
    for ppo in (False, True):
        c = N.loss_case(M, D, seed=1000 * M + 10 * D + ppo, ppo=ppo)
        for adv_norm in ((False, True) if M >= 2 else (False,)):
            for ef in (0.0, 0.01):
                tag = "M=%d D=%d %s norm=%d ef=%g" % (M, D, "ppo" if ppo else "a2c", adv_norm, ef)
                extra = 3 if (M + D + adv_norm) % 2 else 0
                got = _loss(c, vf, ef, clip if ppo else None, adv_norm, pitch_extra=extra)
                blind = N.loss(c["mean"], c["logstd"], c["values"], c["actions"], c["targets"], c["acting"], c["old"], vf, ef,
                               clip if ppo else None, adv_norm)
                worst = max(worst, _ratio("loss_normal.log_probs " + tag, got["log_probs"], blind["log_probs"],
                                          N.head_logp_bound(blind["log_probs"], blind["logp_mag"])))
                want = N.loss(c["mean"], c["logstd"], c["values"], c["actions"], c["targets"], c["acting"], c["old"], vf, ef,
                              clip if ppo else None, adv_norm, log_probs=got["log_probs"])
                bounds = N.loss_bounds(want, vf, ef)
                for key in ("stats", "dmean", "dlogstd", "dvalues"):
                    worst = max(worst, _ratio("loss_normal.%s %s" % (key, tag), got[key], want[key], bounds[key]))
                assert np.all(got["dvalues"][c["targets"] == c["values"]] == 0)
                if ppo:
                    clipped = (want["coef"] == 0) & (want["adv"] != 0)
                    assert M < 1023 or clipped.sum() > 0
                    assert np.all(got["dmean"][clipped] == 0), tag
                for other in (_loss(c, vf, ef, clip if ppo else None, adv_norm, pitch_extra=extra),
                              _loss(c, vf, ef, clip if ppo else None, adv_norm, pitch_extra=3 - extra, want_logp=False)):
                    for k in ("stats", "dmean", "dlogstd", "dvalues"):
                        assert np.array_equal(got[k].view(np.int32), other[k].view(np.int32)), (tag, k)
    assert worst <= 1.0


def test_loss_refuses_bad_arguments():
    L = _lib()
    x = torch.full((64,), NAN, device="cuda")

    def call(M=4, D=2, pitch=2, dpitch=2, adv_norm=0, clip=0.2, mean=x, logstd=x, values=x, actions=x, targets=x, acting=x, old=x,
             dmean=x, dlogstd=x, dvalues=x, stats=x):
        return L.lib.mirl_ac_loss_normal(M, D, _p(mean), pitch, _p(logstd), _p(values), _p(actions), _p(targets), _p(acting), _p(old),
                                         0.5, 0.01, clip, adv_norm, _p(dmean), dpitch, _p(dlogstd), _p(dvalues), None, _p(stats), _st())
    for kw in (dict(M=0), dict(M=2 ** 22 + 1), dict(D=0), dict(D=17), dict(pitch=1), dict(dpitch=1), dict(adv_norm=2), dict(M=1, adv_norm=1),
               dict(clip=-0.1), dict(clip=NAN), dict(mean=None), dict(logstd=None), dict(values=None), dict(actions=None),
               dict(targets=None), dict(acting=None), dict(dmean=None), dict(dlogstd=None), dict(dvalues=None), dict(stats=None)):
        assert call(**kw) == L.MIRL_ERR_ARG, kw
        assert "ac_loss_normal" in L.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all())                                        # nothing was launched
