"""GPU: Flappy in colour (csrc/acting.hip k_flappy_env_step with FlappyArgs.rgb through mirl_flappy_env_step_rgb /
mirl_flappy_env_step_pre_rgb; rltime_amd/acting/flappy_env.py rgb=True) against the NumPy restatement of
tests/flappy_rgb_restate.py (proved on hand-built frames by tests/test_flappy_rgb_cpu.py), in the harness of
tests/test_flappy_env_gpu.py: guarded buffers, every output compared bit for bit after every launch.  Dynamics, record, clock,
rewards and dones are that test's restatement untouched (tests/flappy_restate.py): only the frames are rendered in colour."""
import numpy as np
import pytest
import torch

from tests import flappy_restate as FR
from tests import flappy_rgb_restate as RGB
from tests import test_acting_kernels_gpu as K
from tests import test_flappy_env_gpu as FE

pytestmark = pytest.mark.gpu


class _FlappyRGB(FE._Flappy):
    """tests/test_flappy_env_gpu.py's harness with P = 3 colour planes: the same mirrors, the frames from render_rgb, the
    launches through the rgb entry points."""

    def expect(self, actions=None):
        r, d = super().expect(actions)                                      # state, rewards, dones, records, clock
        P, H, W, cell, gap, spacing = self.geo
        assert P == 3
        self.obs[:self.E * self.fb] = RGB.render_rgb(self.state, self.seed, H, W, cell, gap, spacing).reshape(-1)
        return r, d

    def launch(self, actions=None, tail=None):
        L = K._lib()
        if actions is not None:
            self.act_d[:self.E] = torch.from_numpy(np.asarray(actions, dtype=np.int32)).cuda()
        a = self.args(1 if actions is None else 0)
        if tail is None:
            L.check(L.lib.mirl_flappy_env_step_rgb(*a, K._st()), "mirl_flappy_env_step_rgb")
        else:
            L.check(L.lib.mirl_flappy_env_step_pre_rgb(*a, *tail), "mirl_flappy_env_step_pre_rgb")
        out = self.expect(actions)
        self.check("t = %d" % self.t)
        return out


@pytest.mark.parametrize("H,W,cell,steps,limit", [(24, 16, 2, 300, 9), (120, 80, 10, 200, 9)], ids=["24x16-s2", "120x80-s10"])
def test_rgb_random_stream_equals_the_restatement(H, W, cell, steps, limit):
    """E = 3, a few hundred steps of integers from [-1, A] inclusive (anything but 1 is no flap), every third step steered at
    the next gap so that pipes are passed: frames, rewards, dones, both state halves and both clock words after every launch —
    the reset frame (drawn, not zero), deaths on the floor and on pipes, passes, and the max_episode_steps end."""
    E, A = 3, 3
    env = _FlappyRGB(E, 3, H, W, cell, A, seed=2 ** 63 + 4242 + H, max_steps=limit, death_reward=-5.0, t0=3, slot=1)
    g = np.random.default_rng(H)
    r, d = env.launch()
    assert not r.any() and d.all()
    first = env.obs[:E * env.fb].reshape(E, 3, H, W)
    assert (first[:, 0] == 78).any() and (first[:, 0] == 250).any() and not (first == 0).any()        # drawn, not zero
    ends = 0
    for t in range(steps):
        acts = g.integers(-1, A + 1, E).astype(np.int32)
        if t % 3 == 0 or (t // 40) % 2:
            acts = FR.seeking_action(env.state, env.seed, H, W, cell, FE.GAP, FE.SPACING)
        r, d = env.launch(acts)
        ends += int(d.sum())
    # (the time limit, 9, falls two steps behind the first pipe: an episode that passes it ends by the limit)
    assert ends >= 20 and {"floor", "plain", "pass", "limit", "above", "below", "ceiling"} <= env.seen, env.seen


def test_rgb_env_against_the_intensity_env_and_its_three_ways_to_step():
    """FlappyVecEnv(rgb=True) beside FlappyVecEnv(frame_shape (1, H, W)) under the same seed and actions: rewards, dones and
    records identical, and every colour pixel mapped back through the palette gives the intensity frame.  step_device, step_into
    on a bound action buffer and step_pre (the env step with the actor's pre-step in the launch) give the same frames, rewards
    and dones; ExtraFeaturesVecEnv wraps the colour env unchanged."""
    from rltime_amd.acting.extra_features import ExtraFeaturesVecEnv
    from rltime_amd.acting.flappy_env import FlappyVecEnv
    E, H, W, A = 3, 24, 16, 2
    kw = dict(cell=2, gap=3, spacing=4, n_actions=A, max_episode_steps=30, death_reward=-5.0, seed=2 ** 41 + 5)
    grey = FlappyVecEnv(E, frame_shape=(1, H, W), **kw)
    envs = [FlappyVecEnv(E, frame_shape=(3, H, W), rgb=True, **kw) for _ in range(3)]
    assert all(e.rgb and e.frame_stack is False and tuple(e.observation_space.shape) == (3, H, W) for e in envs)
    assert not grey.rgb and not hasattr(grey, "frame_stack")
    wrapped = ExtraFeaturesVecEnv(FlappyVecEnv(E, frame_shape=(3, H, W), rgb=True, **kw))
    assert wrapped.frame_stack is False and tuple(wrapped.observation_space.spaces[0].shape) == (3, H, W)
    f0 = grey.reset().cpu().numpy()
    firsts = [e.reset() for e in envs]
    wf, _ = wrapped.reset()
    for f in firsts + [wf]:
        assert np.array_equal(RGB.to_classes(f.cpu().numpy()), f0)
    bound = torch.zeros(E, dtype=torch.int32, device="cuda")
    envs[1].bind_actions(bound)
    pre_acts = torch.zeros(E, dtype=torch.int32, device="cuda")
    envs[2].bind_actions(pre_acts)
    # the pre-step's buffers (no recurrent carry: H = 0), as tests/test_flappy_env_gpu.py builds them
    state = K._pre_state(E, 0, 37, A, 81)
    dev = {k: K._up(v) for k, v in state.items()}
    dev["h"], dev["c"] = K._up(None), K._up(None)
    dev["actions"] = pre_acts
    obs_i, rew_i, don_i = envs[1]._fresh()
    obs_p, rew_p, don_p = envs[2]._fresh()
    g = np.random.default_rng(9)
    state_r, _, _, _ = FR.flappy_reset(kw["seed"], E, 1, H, W, 2, 3, 4)
    ends = passes = 0
    for t in range(120):
        acts = g.integers(0, A, E).astype(np.int32) if t % 2 else FR.seeking_action(state_r, kw["seed"], H, W, 2, 3, 4)
        a = torch.from_numpy(acts).cuda()
        fg, rg, dg, _ = grey.step_device(a)
        fd, rd, dd, _ = envs[0].step_device(a)
        (fw, _), rw, dw, _ = wrapped.step_device(a)
        bound.copy_(a)
        envs[1].step_into(obs_i, rew_i, don_i)
        pre_acts.copy_(a)
        envs[2].step_pre(obs_p, rew_p, don_p, [0, A] + K._pre_tail(0, A, 37, 1, dev, 500 + t))
        torch.cuda.synchronize()
        state_r, f_r, r_r, d_r = FR.flappy_step(state_r, acts, kw["seed"], 1, H, W, 2, 3, 4, 30, -5.0)
        assert np.array_equal(fg.cpu().numpy(), f_r) and np.array_equal(dg.cpu().numpy().astype(np.uint8), d_r), t
        for f, r, d in ((fd, rd, dd.view(torch.uint8)), (fw, rw, dw.view(torch.uint8)), (obs_i, rew_i, don_i), (obs_p, rew_p, don_p)):
            assert torch.equal(r.view(torch.int32), rg.view(torch.int32)) and torch.equal(d, dg.view(torch.uint8)), t
            assert torch.equal(f, fd), t
        assert np.array_equal(RGB.to_classes(fd.cpu().numpy()), fg.cpu().numpy()), t
        assert np.array_equal(fd.cpu().numpy(), RGB.render_rgb(state_r, kw["seed"], H, W, 2, 3, 4)), t
        ends += int(d_r.sum())
        passes += int((r_r == 1.0).sum())
    assert ends >= 3 and passes >= 3
    for e in envs:
        assert torch.equal(e.get_state()["records"], grey.get_state()["records"]) and e.get_state()["t"] == grey.get_state()["t"] == 120


def test_the_existing_entry_points_are_untouched_and_rgb_refuses_other_plane_counts():
    """One case of tests/test_flappy_env_gpu.py's scripted streams through mirl_flappy_env_step again (three HISTORY planes: the
    same P as the colour env, the old rendering), then the rgb entry points' own refusal — P != 3 — with nothing written."""
    env = FE.run_script(5, (3, 20, 12, 2), "seek")
    assert FE.SCRIPTS["seek"][1] <= env.seen
    L = K._lib()
    for P in (1, 2, 4):
        bad = _FlappyRGB(2, 3, 24, 16, 2, 2, seed=1, obs_guard=2 * 4 * 24 * 16 + 64)
        a = bad.args(1)
        a[1] = P
        assert L.lib.mirl_flappy_env_step_rgb(*a, K._st()) == FE.ERR_ARG
        bad.check("P = %d refused" % P)
    x, u8 = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    i32, w64 = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    pre = K._pre_valid_args(x, u8, i32, w64)
    bad = _FlappyRGB(2, 3, 24, 16, 2, 2, seed=1, obs_guard=2 * 4 * 24 * 16 + 64)
    a = bad.args(1)
    a[1] = 4
    assert L.lib.mirl_flappy_env_step_pre_rgb(*a, pre[1], pre[2], *pre[5:]) == FE.ERR_ARG
    bad.check("fused form, P = 4 refused")
    assert not x.any() and not u8.any() and not i32.any() and not w64.any()
