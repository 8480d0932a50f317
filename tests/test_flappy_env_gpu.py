"""GPU: the Flappy vector env (csrc/acting.hip k_flappy_env_step, rltime_amd/acting/flappy_env.py) against the NumPy
restatement of tests/flappy_restate.py (proved on hand-worked cases by tests/test_flappy_restate_cpu.py).

The kernel moves integers and writes bytes, so every comparison is bit for bit: frames as bytes, rewards as int32 patterns,
the 16-byte state records and the clock words value by value, return codes exactly.  Every output buffer is longer than the
kernel may write and starts out filled with a pattern (0xA5 bytes); the restatement is applied to a host copy of the same
buffer, so a write into a guard element, into the half of a pair that is only read, or by a refused call shows as a
difference.  Helpers shared with tests/test_acting_kernels_gpu.py are taken from that module."""
import copy

import numpy as np
import pytest
import torch

from tests import flappy_restate as FR
from tests import pointwise_restate as R
from tests import test_acting_kernels_gpu as K
from tests.extra_features_restate import ExtraFeatures

pytestmark = pytest.mark.gpu

ERR_ARG = K.ERR_ARG
STATE_FILL = 0xA5A5A5A5
GAP, SPACING = 3, 4
SHAPES = [(1, 24, 16, 2), (3, 20, 12, 2), (4, 48, 32, 4)]            # (P, H, W, cell); (3,20,12): 16-pixel chunks straddle rows


class _Flappy:
    """Device buffers of one Flappy env and their host mirrors: the state pair (2 x E records + two guard records), the clock
    pair (+ two guard words), obs / rewards / dones with guards, the action buffer.  device=False keeps the mirrors only
    (the scripts' branch coverage can be checked without a GPU)."""

    def __init__(self, E, P, H, W, cell, A, seed, gap=GAP, spacing=SPACING, max_steps=1000, death_reward=-1.0, t0=0, slot=0,
                 obs_guard=64, device=True):
        self.E, self.A, self.seed, self.slot, self.t = E, A, seed, slot, t0
        self.geo = (P, H, W, cell, gap, spacing)
        self.max_steps, self.death_reward = max_steps, death_reward
        self.fb = P * H * W
        self.rec = np.full((2 * E + 2, 4), STATE_FILL, dtype=np.uint32)
        self.rec[slot * E:(slot + 1) * E, 3] = np.arange(E) * 7             # the episode numbers a reset_all keeps
        self.clock = np.full(4, K.CLOCK_FILL, dtype=np.uint64)
        self.clock[slot] = t0
        self.obs, self.rew, self.don = K._fill(E * self.fb + obs_guard, np.uint8), K._fill(E + 9, np.float32), K._fill(E + 9, np.uint8)
        self.device = device
        if device:
            self.rec_d, self.clock_d = K._up(self.rec.reshape(-1)), K._up(self.clock)
            self.obs_d, self.rew_d, self.don_d = K._up(self.obs), K._up(self.rew), K._up(self.don)
            self.act_d = torch.zeros(E + 9, dtype=torch.int32, device="cuda")
        self.state = None
        self.seen = set()

    def args(self, reset_all=0):
        P, H, W, cell, gap, spacing = self.geo
        return [self.E, P, H, W, cell, gap, spacing, self.A, self.max_steps, self.death_reward,
                None if reset_all else K._p(self.act_d), K._p(self.rec_d), K._p(self.clock_d), self.slot, self.seed, reset_all,
                K._p(self.obs_d), K._p(self.rew_d), K._p(self.don_d)]

    def expect(self, actions=None):
        """Advance the host mirrors by one launch (actions None: reset_all) -> (rewards, dones)."""
        P, H, W, cell, gap, spacing = self.geo
        E = self.E
        if actions is None:
            n = self.rec[self.slot * E:(self.slot + 1) * E, 3]
            self.state, frames, r, d = FR.flappy_reset(self.seed, E, P, H, W, cell, gap, spacing, n=n)
        else:
            self.t += 1
            for names in FR.branches(self.state, actions, self.seed, H, W, cell, gap, spacing, self.max_steps):
                self.seen |= names
            self.state, frames, r, d = FR.flappy_step(self.state, actions, self.seed, P, H, W, cell, gap, spacing, self.max_steps,
                                                      self.death_reward)
        self.obs[:E * self.fb] = frames.reshape(-1)
        self.rew[:E], self.don[:E] = r, d
        self.slot ^= 1                                                  # the halves read stay, the other ones are written
        self.rec[self.slot * E:(self.slot + 1) * E] = FR.records(self.state)
        self.clock[self.slot] = self.t
        return r, d

    def check(self, what):
        torch.cuda.synchronize()
        K._same(K._down(self.rew_d, self.rew), self.rew, what + ": rewards")
        K._same(K._down(self.don_d, self.don), self.don, what + ": dones")
        K._same(K._down(self.clock_d, self.clock), self.clock, what + ": clock pair")
        K._same(K._down(self.rec_d, self.rec).reshape(-1, 4), self.rec, what + ": state pair")
        K._same(K._down(self.obs_d, self.obs), self.obs, what + ": obs")

    def launch(self, actions=None, tail=None):
        """One mirl_flappy_env_step[_pre] launch (actions None: reset_all), mirrored on the host and compared."""
        if not self.device:
            return self.expect(actions)
        L = K._lib()
        if actions is not None:
            self.act_d[:self.E] = torch.from_numpy(np.asarray(actions, dtype=np.int32)).cuda()
        a = self.args(1 if actions is None else 0)
        if tail is None:
            L.check(L.lib.mirl_flappy_env_step(*a, K._st()), "mirl_flappy_env_step")
        else:
            L.check(L.lib.mirl_flappy_env_step_pre(*a, *tail), "mirl_flappy_env_step_pre")
        out = self.expect(actions)
        self.check("t = %d" % self.t)
        return out


# script -> (max_episode_steps as a function of (C, D), the branches its stream must have reached)
SCRIPTS = {
    "seek": (lambda C, D: C - 1 + D, {"pass", "pass+limit", "plain"}),      # the limit falls on the step that passes pipe 1
    "seek-short": (lambda C, D: 3, {"limit"}),                             # the time limit alone
    "flap": (lambda C, D: 1000, {"ceiling", "above"}),
    "fall": (lambda C, D: 1000, {"floor"}),
    "low": (lambda C, D: 1000, {"below"}),
}


def run_script(E, shape, script, device=True):
    """reset_all, then 3 (C + 3 D) scripted steps with every output compared after every launch -> the harness."""
    P, H, W, cell = shape
    C = W // cell
    limit, _ = SCRIPTS[script]
    env = _Flappy(E, P, H, W, cell, 2, seed=(0xF00D << 32) + 1000 + 7 * H + E, max_steps=limit(C, SPACING), death_reward=-5.0,
                  t0=(E + H) % 5, slot=(E + C) % 2, device=device)
    r, d = env.launch()
    assert not r.any() and d.all()
    for _ in range(3 * (C + 3 * SPACING)):
        r, d = env.launch(FR.scripted_action(script.split("-")[0], env.state, env.seed, H, W, cell, GAP, SPACING))
    return env


@pytest.mark.parametrize("script", sorted(SCRIPTS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "P%d-%dx%d-s%d" % s)
@pytest.mark.parametrize("E", [1, 5])
def test_flappy_step_stream_equals_the_restatement(E, shape, script):
    """Frames, rewards, dones, both state halves and both clock words after every launch of a scripted stream that reaches
    the branches the script is for (tests/flappy_restate.py `branches`)."""
    env = run_script(E, shape, script)
    assert SCRIPTS[script][1] <= env.seen, (script, env.seen)


def test_flappy_random_stream_equals_the_restatement():
    """E = 5, 300 steps of integers from [-1, A] inclusive (anything but 1 is no flap), one plane."""
    A = 3
    env = _Flappy(5, 1, 24, 16, 2, A, seed=2 ** 63 + 12345, max_steps=40, death_reward=-1.0, t0=3, slot=1)
    g = np.random.default_rng(17)
    env.launch()
    ends = 0
    for _ in range(300):
        r, d = env.launch(g.integers(-1, A + 1, 5).astype(np.int32))
        ends += int(d.sum())
    assert ends >= 20 and {"floor", "plain", "ceiling"} <= env.seen and env.seen & {"above", "below"} and "pass" in env.seen, env.seen


def test_flappy_planes_larger_than_one_grid_stride():
    """(4, 128, 128): 4096 chunks per env against a grid of 8 x 256 threads — every thread stores two chunks."""
    env = _Flappy(2, 4, 128, 128, 8, 2, seed=5, gap=4, spacing=5, max_steps=9, death_reward=-1.0)
    env.launch()
    for n in range(20):
        env.launch(FR.seeking_action(env.state, env.seed, 128, 128, 8, 4, 5))
    assert "limit" in env.seen and env.state["tau"].max() >= 1


def test_flappy_uses_every_bit_of_the_seed():
    """Two seeds that differ only above bit 32 give different gap streams (and the kernel's are the restatement's)."""
    frames = []
    for seed in (77, 77 + 2 ** 40, 77 + 2 ** 63):
        env = _Flappy(3, 1, 24, 16, 2, 2, seed=seed, gap=2, spacing=2)
        env.launch()
        for n in range(4):                                                   # tau = 4: pipes 0 and 1 are on screen, every bird alive
            env.launch(np.array([n % 2] * 3, dtype=np.int32))
        assert not env.don[:3].any()
        frames.append(env.obs.copy())
        assert (env.obs == FR.PIPE).any()
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[0], frames[2]) and not np.array_equal(frames[1], frames[2])


def test_flappy_refuses_bad_arguments_and_writes_nothing():
    L = K._lib()
    env = _Flappy(2, 2, 24, 16, 2, 2, seed=1, t0=5, slot=0, obs_guard=2 * 5 * 24 * 20 + 64)        # room for P = 5 or W = 20, were it launched
    env.launch()
    env.launch(np.array([1, 0], dtype=np.int32))
    rec8, clock8, obs8 = env.rec_d[2:], env.clock_d[1:], env.obs_d[8:]
    assert rec8.data_ptr() % 16 == 8 and clock8.data_ptr() % 16 == 8 and obs8.data_ptr() % 16 == 8
    # positions: 0 E, 1 P, 2 H, 3 W, 4 cell, 5 gap, 6 spacing, 7 A, 8 max_episode_steps, 10 actions, 11 state, 12 clock, 13 slot,
    # 15 reset_all, 16 obs, 17 rewards, 18 dones
    bad = [(0, 0), (0, -1), (0, 65536), (1, 0), (1, 5), (2, 25), (2, 6), (2, 0), (3, 18), (3, 17), (3, 4), (3, 0), (4, 0), (4, -2),
           (4, 16), (5, 12), (5, 13), (5, 0), (6, 1), (6, 0), (7, 1), (8, 0), (10, None), (11, None), (12, None), (16, None), (17, None),
           (18, None), (11, K._p(rec8)), (12, K._p(clock8)), (16, K._p(obs8)), (13, 2), (13, -1), (15, 2), (15, -1)]
    for pos, value in bad:
        a = env.args() + [K._st()]
        a[pos] = value
        assert L.lib.mirl_flappy_env_step(*a) == ERR_ARG, (pos, value)
    a = env.args() + [K._st()]                                               # (H, cell) = (1024, 4): R = 256 rows
    a[2], a[4] = 1024, 4
    assert L.lib.mirl_flappy_env_step(*a) == ERR_ARG
    x, u8 = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    i32, w64 = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    for pos, value in bad:                                                   # the fused form refuses the same env arguments ...
        a = env.args()
        a[pos] = value
        pre = K._pre_valid_args(x, u8, i32, w64)
        assert L.lib.mirl_flappy_env_step_pre(*a, pre[1], pre[2], *pre[5:]) == ERR_ARG, (pos, value)
    for pos, value in K.PRE_BAD:                                             # ... and what mirl_actor_pre refuses
        if pos in (0, 3, 4):                                                 # E, rewards_raw, dones: the env's own arguments here
            continue
        pre = K._pre_valid_args(x, u8, i32, w64)
        pre[pos] = value
        assert L.lib.mirl_flappy_env_step_pre(*env.args(), pre[1], pre[2], *pre[5:]) == ERR_ARG, pos
    env.check("after refusals")
    assert not x.any() and not u8.any() and not i32.any() and not w64.any()
    a = env.args(reset_all=1) + [K._st()]                                    # reset_all = 1 takes NULL actions
    assert L.lib.mirl_flappy_env_step(*a) == 0
    env.expect(None)
    env.check("reset_all with NULL actions")


@pytest.mark.parametrize("H", [0, 16])
def test_flappy_step_pre_equals_step_followed_by_actor_pre(H):
    """Two sets of device buffers from the same start: one takes mirl_flappy_env_step_pre, the other mirl_flappy_env_step and
    then mirl_actor_pre on its rewards / dones.  After every step of a stream that contains a done, every buffer of the
    two is bit-equal, and equal to the restatements."""
    L = K._lib()
    E, A, pitch, clip = 3, 4, H + 37, 1
    envs = [_Flappy(E, 2, 20, 12, 2, A, seed=31 + H, max_steps=4, death_reward=-5.0, t0=20 + H, slot=H % 2) for _ in range(2)]
    h, c = K._carry(E, H, 70 + H) if H else (None, None)
    state = K._pre_state(E, H, pitch, A, 80 + H)
    devs = []
    for _ in range(2):
        dev = {k: K._up(v) for k, v in state.items()}
        dev["h"], dev["c"] = K._up(h), K._up(c)
        devs.append(dev)
    for env in envs:
        env.launch()
    seen = set()
    for n in range(9):
        actions = K._actions(E, A, n, 90 + n)
        step = R.STEP_ADVANCE if n % 2 else 500 + n
        for dev in devs:
            dev["actions"] = envs[0].act_d                                   # the pre-step counts the actions the env applied
        envs[0].launch(actions, tail=[H, A] + K._pre_tail(H, A, pitch, clip, devs[0], step))
        raw, dones = envs[1].launch(actions)
        devs[1]["actions"] = envs[1].act_d
        L.check(L.lib.mirl_actor_pre(E, H, A, K._p(envs[1].rew_d), K._p(envs[1].don_d), *K._pre_tail(H, A, pitch, clip, devs[1], step)),
                "mirl_actor_pre")
        torch.cuda.synchronize()
        seen |= set(dones.tolist())
        state = R.actor_pre(raw, dones, H, h, c, state["xh"], pitch, state["c_in"], state["state_pack"], state["initials"],
                            state["rewards_out"], state["dones_out"], clip, actions=actions, A=A, ep_reward=state["ep_reward"],
                            ep_len=state["ep_len"], out_reward=state["out_reward"], out_len=state["out_len"],
                            action_counts=state["action_counts"], rng_step=state["rng_step"], step=step)
        for k in K.PRE_KEYS:
            K._same(K._down(devs[0][k], state[k]), state[k], "step %d, fused: %s" % (n, k))
            K._same(K._down(devs[1][k], state[k]), state[k], "step %d, two launches: %s" % (n, k))
    assert seen == {0, 1}, "the carry must be both kept and reset"


# ---- through the actor -------------------------------------------------------------------------------------------------------
TINY = {"type": "sequential", "args": {"layer_configs": [
    {"type": "cnn", "args": {"channels_last": True, "layers": [{"filters": 32, "kernel": 8, "stride": 4},
                                                               {"filters": 16, "kernel": 3, "stride": 1}]}},
    {"type": "fc", "args": {"fc_size": 32}}]}}
EXPL = {"type": "epsilon_greedy", "args": {"eps_start": 0.5, "eps_final": 0.5, "exploration_fraction": 0.5}}
ENV_SEED = 21
ENV_KW = dict(frame_shape=(4, 48, 32), cell=4, gap=3, spacing=4, n_actions=2, max_episode_steps=6, death_reward=-1.0)


def _stored(hist, E, steps):
    """Everything the replay holds about the first `steps` vector steps, read back with one gather of E * steps windows of
    one transition (nstep_train = nstep_target = 1): window (env, o) returns the action, reward and done stored at offset o
    and, as its target state, the frames stored there (csrc/replay.hip row_src_off)."""
    env = torch.arange(E, dtype=torch.int32, device="cuda").repeat(steps)
    start = torch.arange(steps, dtype=torch.int64, device="cuda").repeat_interleave(E)
    batch = hist._gather(E * steps, env, start, torch.ones(E * steps, device="cuda"))
    torch.cuda.synchronize()
    frames = batch["target_states"]["x"][0].cpu().numpy().reshape((steps, E) + tuple(batch["target_states"]["x"].shape[2:]))
    return (frames, batch["policy_outputs"]["actions"][0].cpu().numpy().reshape(steps, E),
            batch["returns"][0].cpu().numpy().reshape(steps, E), 1.0 - batch["target_masks"][0].cpu().numpy().reshape(steps, E))


@pytest.mark.parametrize("iters", [5, 4], ids=["K5", "K4"])
def test_flappy_rides_in_the_rollout_graph(iters, monkeypatch):
    """E = 4, (4,48,32), a tiny CNN -> FC DQN on the fused acting step writing into a device replay: two get_samples calls of
    K steps from the captured rollout graph and the same with `rollout_graphs` off on the FastActingStep instance store
    identical frames, actions, rewards and dones and leave identical env records — and the frames, rewards and dones are
    the restatement's on the stored actions.  An odd K alternates the clock parity between the calls (two captures), an
    even K keeps it (one)."""
    from rltime_amd.acting import fast_step
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.flappy_env import FlappyVecEnv
    from rltime_amd.history import ReplayHistoryBuffer
    from rltime_amd.policies.dqn import DQNPolicy
    E, calls = 4, 2
    plain_init = fast_step.FastActingStep.__init__
    runs, records = [], []
    for graph in (True, False):
        def init(self, *a, _graph=graph, **kw):
            plain_init(self, *a, **kw)
            self.rollout_graphs = _graph
        monkeypatch.setattr(fast_step.FastActingStep, "__init__", init)
        torch.manual_seed(0)
        env = FlappyVecEnv(E, seed=ENV_SEED, **ENV_KW)
        assert not hasattr(env, "frame_stack")
        pol = DQNPolicy.create(model_config=TINY, observation_space=env.observation_space, action_space=env.action_space, dueling=False)
        actor = Actor(env, exploration_config=EXPL, device=True, use_graph=True)
        actor.set_actor_policy(pol)
        hist = ReplayHistoryBuffer(size=E * 40, train_frequency=1, nstep_target=1, nstep_train=1, prefix_steps=0, gamma=0.99,
                                   device_rng=True, keep_policy_outputs=False)
        actor.set_sink(hist)
        for _ in range(calls):
            s = actor.get_samples(E * iters)
            assert getattr(s, "ingested", False)
            hist.update(s)
        fs = actor._fast
        assert isinstance(fs, fast_step.FastActingStep) and fs.env_into and fs.env_pre and fs.rollout_graphs == graph
        captured = [v[1] is not None for v in fs._rollouts.values()]
        assert (len(captured) == (2 if iters % 2 else 1) and all(captured)) if graph else captured == [], fs._rollouts.keys()
        runs.append(_stored(hist, E, iters * calls))
        records.append(env.get_state())
        hist.close()
    for a, b, what in zip(runs[0], runs[1], ("frames", "actions", "rewards", "dones")):
        assert np.array_equal(a, b), what
    assert records[0]["t"] == records[1]["t"] == iters * calls and torch.equal(records[0]["records"], records[1]["records"])
    frames, actions, rewards, dones = runs[0]
    assert len(set(actions.reshape(-1).tolist())) >= 2 and dones.any() and not dones.all()
    geo = (4, 48, 32, 4, 3, 4)
    state, _, _, _ = FR.flappy_reset(ENV_SEED, E, *geo)
    for k in range(iters * calls):
        state, f, r, d = FR.flappy_step(state, actions[k], ENV_SEED, *geo, 6, -1.0)
        assert np.array_equal(frames[k], f), k
        K._same(rewards[k].astype(np.float32), r, "reward %d" % k)
        assert np.array_equal(dones[k].astype(np.uint8), d), k
    assert np.array_equal(records[0]["records"].numpy().view(np.uint32), FR.records(state))


def test_flappy_resumes_bit_identically():
    """get_state -> a fresh FlappyVecEnv -> set_state continues with identical outputs from both parities (and the class's
    reset, the stepping and the bound action buffer equal the restatement on the way)."""
    from rltime_amd.acting.flappy_env import FlappyVecEnv
    E = 5
    kw = dict(frame_shape=(4, 24, 16), cell=2, gap=3, spacing=4, n_actions=2, max_episode_steps=11, death_reward=-2.5, seed=2 ** 40 + 9)
    geo = (4, 24, 16, 2, 3, 4)
    g = np.random.default_rng(4)
    acts = g.integers(0, 2, (40, E)).astype(np.int32)
    for first in (8, 9):                                                     # the saving env is at parity 1, then 0
        a = FlappyVecEnv(E, **kw)
        state, f, _, _ = FR.flappy_reset(kw["seed"], E, *geo)
        assert np.array_equal(a.reset().cpu().numpy(), f)
        for n in range(first):
            obs, r, d, info = a.step_device(torch.from_numpy(acts[n]).cuda())
            state, f, rr, dd = FR.flappy_step(state, acts[n], kw["seed"], *geo, 11, -2.5)
            assert info is None and np.array_equal(obs.cpu().numpy(), f) and np.array_equal(d.cpu().numpy(), dd.astype(bool))
            K._same(r.cpu().numpy(), rr, "reward %d" % n)
        assert a.clock_parity() == (first + 1) % 2
        saved = a.get_state()
        assert saved["t"] == first and np.array_equal(saved["records"].numpy().view(np.uint32), FR.records(state))
        b = FlappyVecEnv(E, **kw)
        b.set_state(copy.deepcopy(saved))
        assert b.clock_parity() == 0
        bound = torch.zeros(E, dtype=torch.int32, device="cuda")
        b.bind_actions(bound)                                                # the static buffer a captured step reads
        out = (torch.empty((E, 4, 24, 16), dtype=torch.uint8, device="cuda"), torch.empty(E, device="cuda"),
               torch.empty(E, dtype=torch.uint8, device="cuda"))
        ends = 0
        for n in range(first, first + 20):
            obs, r, d, _ = a.step_device(torch.from_numpy(acts[n]).cuda())
            bound.copy_(torch.from_numpy(acts[n]))
            b.step_into(*out)
            assert torch.equal(obs, out[0]) and torch.equal(r.view(torch.int32), out[1].view(torch.int32)) and torch.equal(d.view(torch.uint8), out[2])
            ends += int(d.sum())
        assert ends > 0 and a.get_state()["t"] == b.get_state()["t"] == first + 20
        assert torch.equal(a.get_state()["records"], b.get_state()["records"])


def test_flappy_extras_equal_the_restatement():
    """make_vec_env with extra_features: 60 steps; the extras rows are tests/extra_features_restate.py applied to the
    restatement's (action, reward, done) stream — death_reward -5 goes through the wrapper's reward clip."""
    from rltime_amd.acting.extra_features import ExtraFeaturesVecEnv
    from rltime_amd.train import make_vec_env
    E, seed = 5, 13
    env = make_vec_env("flappy", {"frame_shape": [1, 24, 16], "cell": 2, "gap": 3, "spacing": 4, "n_actions": 2,
                                  "max_episode_steps": 9, "extra_features": True, "death_reward": -5.0}, E, "cuda", seed=seed)
    assert isinstance(env, ExtraFeaturesVecEnv) and env.extra_size == 4
    geo = (1, 24, 16, 2, 3, 4)
    a, r, t = (bool(f) for f in env._flags)
    ef = ExtraFeatures(E, env.action_space.n, a, r, t, bool(env._clip), env._scale)
    assert ef.inc == (True, True, True) and bool(env._clip)
    frames, rows = env.reset()
    state, f, _, _ = FR.flappy_reset(seed, E, *geo)
    ef.reset()
    assert np.array_equal(frames.cpu().numpy(), f)
    g = np.random.default_rng(8)
    raw = set()
    for s in range(60):
        acts = g.integers(0, 2, E).astype(np.int32)
        (frames, rows), rewards, dones, _ = env.step_device(torch.from_numpy(acts).cuda())
        state, f, rr, dd = FR.flappy_step(state, acts, seed, *geo, 9, -5.0)
        assert np.array_equal(frames.cpu().numpy(), f), s
        K._same(rewards.cpu().numpy(), rr, "reward %d" % s)
        assert np.array_equal(dones.cpu().numpy().astype(np.uint8), dd), s
        want = ef.step(acts, rr, dd)
        assert np.array_equal(rows.cpu().numpy().view(np.uint32), want.view(np.uint32)), s
        raw |= set(rr.tolist())
    assert raw == {-5.0, 0.0, 1.0}


def test_two_learner_iterations_on_the_shipped_recurrent_config():
    """rltime_amd.train.train on configs/flappy_iqn_lstm.json at 4 envs with warmup_steps / total_steps cut to a few hundred:
    (1, 120, 80) frames + extras through the fused acting step, the device replay and the recurrent IQN learner.  A smoke
    test that the pieces fit together at the config's shapes (conv 29 x 19 -> 13 x 8 -> 11 x 6, LSTM projection
    K = 4224 + 16 + 512), not a learning claim; the kernels are held to float64 at these shapes one by one in
    tests/test_flappy_shapes_gpu.py (tests/test_flappy_shapes_cpu.py derives the shapes and pins the gates)."""
    import random
    from rltime_amd.acting.fast_step import FastActingStep
    from rltime_amd.general.config import load_config
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.train import train
    random.seed(0); np.random.seed(0); torch.manual_seed(0)      # noqa: E702
    cfg = load_config("flappy_iqn_lstm.json")
    assert cfg["env_args"]["frame_shape"] == [1, 120, 80] and cfg["env_args"]["extra_features"] is True
    cfg["acting"]["actor_envs"] = 4
    # a learner iteration follows every mbatch_size * nstep_train / train_frequency = 160 acted steps; the row logged when
    # step 800 is crossed holds the losses of the iterations since the warm-up ended at 200
    cfg["training"]["args"].update(total_steps=1040, warmup_steps=200, log_freq=800)
    logger = NullLogger()
    trainer = train(copy.deepcopy(cfg), logger, use_graph=True)
    fs = trainer.actors._fast
    assert isinstance(fs, FastActingStep) and fs.X == 4 and fs.F == 4224 and fs.K == 4224 + 16 + 512
    assert trainer.history_buffer._layout.frame_bytes == 9600 and trainer.history_buffer._layout.extra_f32 == 4
    losses = [row["train"]["qloss"] for name, _, row in logger.rows if name == "train" and "qloss" in row.get("train", {})]
    assert len(losses) >= 1 and all(np.isfinite(float(v)) for v in losses), losses
    assert all(bool(torch.isfinite(p).all()) for p in trainer.policy.parameters())
