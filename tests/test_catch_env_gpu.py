"""GPU: the Catch vector env (csrc/acting.hip k_catch_env_step, rltime_amd/acting/catch_env.py) against the NumPy restatement
of tests/catch_restate.py (proved on hand-worked cases by tests/test_catch_restate_cpu.py).

The kernel moves integers and writes bytes, so every comparison is bit for bit: frames as bytes, rewards as int32 patterns,
the 16-byte state records and the clock words value by value, return codes exactly.  Every output buffer is longer than the
kernel may write and starts out filled with a pattern (0xA5 bytes); the restatement is applied to a host copy of the same
buffer, so a write into a guard element, into the half of a pair that is only read, or by a refused call shows as a
difference.  Helpers shared with tests/test_acting_kernels_gpu.py are taken from that module."""
import numpy as np
import pytest
import torch

from tests import catch_restate as CR
from tests import pointwise_restate as R
from tests import test_acting_kernels_gpu as K

pytestmark = pytest.mark.gpu

ERR_ARG = K.ERR_ARG
STATE_FILL = 0xA5A5A5A5
SHAPES = [(4, 84, 12, 12), (4, 36, 12, 12), (4, 32, 8, 8), (2, 20, 5, 5), (1, 16, 4, 4), (3, 12, 12, 12), (4, 36, 6, 3)]


class _Catch:
    """Device buffers of one Catch env and their host mirrors: the state pair (2 x E records + two guard records), the clock
    pair (+ two guard words), obs / rewards / dones with guards, the action buffer."""

    def __init__(self, E, P, S, G, V, A, seed, t0=0, slot=0, obs_guard=64):
        self.E, self.P, self.S, self.G, self.V, self.A, self.seed, self.slot, self.t = E, P, S, G, V, A, seed, slot, t0
        self.fb = P * S * S
        self.rec = np.full((2 * E + 2, 4), STATE_FILL, dtype=np.uint32)
        self.clock = np.full(4, K.CLOCK_FILL, dtype=np.uint64)
        self.clock[slot] = t0
        self.obs, self.rew, self.don = K._fill(E * self.fb + obs_guard, np.uint8), K._fill(E + 9, np.float32), K._fill(E + 9, np.uint8)
        self.rec_d, self.clock_d = K._up(self.rec.reshape(-1)), K._up(self.clock)
        self.obs_d, self.rew_d, self.don_d = K._up(self.obs), K._up(self.rew), K._up(self.don)
        self.act_d = torch.zeros(E + 9, dtype=torch.int32, device="cuda")
        self.state = None

    def args(self, reset_all=0):
        return [self.E, self.P, self.S, self.G, self.V, self.A, None if reset_all else K._p(self.act_d), K._p(self.rec_d),
                K._p(self.clock_d), self.slot, self.seed, reset_all, K._p(self.obs_d), K._p(self.rew_d), K._p(self.don_d)]

    def expect(self, actions=None):
        """Advance the host mirrors by one launch (actions None: reset_all) -> (rewards, dones)."""
        dims = (self.P, self.S, self.G, self.V)
        if actions is None:
            self.state, frames, r, d = CR.catch_reset(self.seed, self.t, self.E, *dims)
        else:
            self.t += 1
            self.state, frames, r, d = CR.catch_step(self.state, actions, self.seed, self.t, *dims)
        E = self.E
        self.obs[:E * self.fb] = frames.reshape(-1)
        self.rew[:E], self.don[:E] = r, d
        self.slot ^= 1                                                  # the halves read stay, the other ones are written
        self.rec[self.slot * E:(self.slot + 1) * E] = CR.records(self.state)
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
        """One mirl_catch_env_step[_pre] launch (actions None: reset_all), mirrored on the host and compared."""
        L = K._lib()
        if actions is not None:
            self.act_d[:self.E] = torch.from_numpy(np.asarray(actions, dtype=np.int32)).cuda()
        a = self.args(1 if actions is None else 0)
        if tail is None:
            L.check(L.lib.mirl_catch_env_step(*a, K._st()), "mirl_catch_env_step")
        else:
            L.check(L.lib.mirl_catch_env_step_pre(*a, *tail), "mirl_catch_env_step_pre")
        out = self.expect(actions)
        self.check("t = %d" % self.t)
        return out


@pytest.mark.parametrize("script", ["random", "tracking"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "P%d-S%d-G%d-V%d" % s)
@pytest.mark.parametrize("E", [1, 3, 64])
def test_catch_step_stream_equals_the_restatement(E, shape, script):
    """reset_all, then 3 (G - 1) + 2 steps — every env resets three times — with obs, rewards, dones, both state halves and
    both clock words compared after every launch.  `random`: integers from [-1, A] inclusive (out-of-range values are
    no-ops); `tracking`: every paddle follows its ball and catches it."""
    P, S, G, V = shape
    A = 4 if script == "random" else 3
    env = _Catch(E, P, S, G, V, A, seed=1000 + 7 * S + G + E, t0=(E + S) % 5, slot=(E + G) % 2)
    g = np.random.default_rng(E * 100 + S)
    r, d = env.launch()
    assert not r.any() and d.all()
    ends = []
    for n in range(3 * (G - 1) + 2):
        actions = g.integers(-1, A + 1, E).astype(np.int32) if script == "random" else CR.tracking_action(env.state)
        r, d = env.launch(actions)
        assert d.tolist() == [1 if (n + 1) % (G - 1) == 0 else 0] * E
        ends += r[d == 1].tolist()
    assert len(ends) == 3 * E
    if script == "tracking":
        assert ends == [1.0] * (3 * E)
    elif E == 64:
        assert -1.0 in ends


def test_catch_uses_the_high_word_of_the_clock():
    """The column draw is keyed by the whole 64-bit step number: resets at t = 2^32 + k draw other columns than at t = k, and
    a stream of one-step episodes (G = 2: every step draws) carries the counter across 2^32."""
    for k in range(3):
        env = _Catch(3, 1, 128, 128, 128, 3, seed=77, t0=2 ** 32 + k, slot=k % 2)
        env.launch()
        low = [CR.draw_column(77, k, e, 128) for e in range(3)]
        assert env.state["ball_col"].tolist() != low
    env = _Catch(3, 1, 4, 2, 2, 3, seed=78, t0=2 ** 32 - 2, slot=1)
    env.launch()
    for n in range(4):
        r, d = env.launch(np.array([n % 3, 2, 1], dtype=np.int32))
        assert d.all()
    assert env.t == 2 ** 32 + 2


def test_catch_refuses_bad_arguments_and_writes_nothing():
    L = K._lib()
    env = _Catch(2, 2, 36, 6, 6, 3, seed=1, t0=5, slot=0, obs_guard=3 * 2 * 36 * 36 + 64)      # room for P = 5, were it launched
    env.launch()
    env.launch(np.array([1, 2], dtype=np.int32))
    rec8, clock8, obs8 = env.rec_d[2:], env.clock_d[1:], env.obs_d[8:]
    assert rec8.data_ptr() % 16 == 8 and clock8.data_ptr() % 16 == 8 and obs8.data_ptr() % 16 == 8
    bad = [(0, 0), (0, -1), (0, 65536), (1, 0), (1, 5), (2, 35), (2, 18), (2, 0), (3, 1), (3, 129), (3, 5), (4, 0), (4, 7), (5, 2), (5, 0),
           (6, None), (7, None), (8, None), (12, None), (13, None), (14, None), (7, K._p(rec8)), (8, K._p(clock8)), (12, K._p(obs8)),
           (9, 2), (9, -1), (11, 2), (11, -1)]
    for pos, value in bad:
        a = env.args() + [K._st()]
        a[pos] = value
        assert L.lib.mirl_catch_env_step(*a) == ERR_ARG, (pos, value)
    x, u8 = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    i32, w64 = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    for pos, value in bad:                                                   # the fused form refuses the same env arguments ...
        a = env.args()
        a[pos] = value
        pre = K._pre_valid_args(x, u8, i32, w64)
        assert L.lib.mirl_catch_env_step_pre(*a, pre[1], pre[2], *pre[5:]) == ERR_ARG, (pos, value)
    for pos, value in K.PRE_BAD:                                             # ... and what mirl_actor_pre refuses
        if pos in (0, 3, 4):                                                 # E, rewards_raw, dones: the env's own arguments here
            continue
        pre = K._pre_valid_args(x, u8, i32, w64)
        pre[pos] = value
        assert L.lib.mirl_catch_env_step_pre(*env.args(), pre[1], pre[2], *pre[5:]) == ERR_ARG, pos
    env.check("after refusals")
    assert not x.any() and not u8.any() and not i32.any() and not w64.any()
    a = env.args(reset_all=1) + [K._st()]                                    # reset_all = 1 takes NULL actions
    assert L.lib.mirl_catch_env_step(*a) == 0
    env.expect(None)
    env.check("reset_all with NULL actions")


@pytest.mark.parametrize("H", [0, 100, 515])
def test_catch_step_pre_equals_step_followed_by_actor_pre(H):
    """Two sets of device buffers from the same start: one takes mirl_catch_env_step_pre, the other mirl_catch_env_step and
    then mirl_actor_pre on its rewards / dones.  After every step of a stream that contains a done, every buffer of the
    two is bit-equal, and equal to the restatements."""
    L = K._lib()
    E, A, pitch, clip = 3, 6, H + 37, 1
    P, S, G, V = 2, 20, 5, 5
    envs = [_Catch(E, P, S, G, V, A, seed=31 + H, t0=20 + H, slot=H % 2) for _ in range(2)]
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
    for n in range(6):
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
ENV_SEED, GRID = 21, 6


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


def test_catch_rides_in_the_rollout_graph(monkeypatch):
    """E = 8, (4,36,36), a tiny CNN -> FC DQN on the fused acting step writing into a device replay: two get_samples calls of
    5 steps from the captured rollout graph and the same with the rollout graph off store identical frames, actions, rewards
    and dones — and the frames, rewards and dones are the restatement's on the stored actions (an action stored one step
    late, or a captured step that reads another action buffer, would break this)."""
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.catch_env import CatchVecEnv
    from rltime_amd.history import ReplayHistoryBuffer
    from rltime_amd.policies.dqn import DQNPolicy
    E, iters, calls = 8, 5, 2
    runs = []
    for graph in ("1", "0"):
        monkeypatch.setenv("MIRL_ROLLOUT_GRAPH", graph)
        torch.manual_seed(0)
        env = CatchVecEnv(E, frame_shape=(4, 36, 36), grid=GRID, n_actions=3, seed=ENV_SEED)
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
        assert fs and fs.env_into and fs.env_pre
        captured = [v[1] is not None for v in fs._rollouts.values()]
        assert (captured and all(captured)) if graph == "1" else captured == []
        runs.append(_stored(hist, E, iters * calls))
        hist.close()
    for a, b, what in zip(runs[0], runs[1], ("frames", "actions", "rewards", "dones")):
        assert np.array_equal(a, b), what
    frames, actions, rewards, dones = runs[0]
    assert len(set(actions.reshape(-1).tolist())) >= 2 and dones.any() and not dones.all()
    state, _, _, _ = CR.catch_reset(ENV_SEED, 0, E, 4, 36, GRID, GRID)
    for k in range(iters * calls):
        state, f, r, d = CR.catch_step(state, actions[k], ENV_SEED, k + 1, 4, 36, GRID, GRID)
        assert np.array_equal(frames[k], f), k
        K._same(rewards[k].astype(np.float32), r, "reward %d" % k)
        assert np.array_equal(dones[k].astype(np.uint8), d), k


def test_catch_resumes_bit_identically():
    """get_state -> a fresh CatchVecEnv -> set_state continues with identical outputs for G steps (and the class's reset, the
    stepping and the bound action buffer equal the restatement on the way)."""
    from rltime_amd.acting.catch_env import CatchVecEnv
    E, G = 5, 8
    kw = dict(frame_shape=(4, 32, 32), grid=G, n_actions=3, visible_rows=5, seed=9)
    a = CatchVecEnv(E, **kw)
    state, f, _, _ = CR.catch_reset(9, 0, E, 4, 32, G, 5)
    assert np.array_equal(a.reset().cpu().numpy(), f)
    g = np.random.default_rng(4)
    acts = g.integers(0, 3, (2 * G, E)).astype(np.int32)
    for n in range(G):
        obs, r, d, info = a.step_device(torch.from_numpy(acts[n]).cuda())
        state, f, rr, dd = CR.catch_step(state, acts[n], 9, n + 1, 4, 32, G, 5)
        assert info is None and np.array_equal(obs.cpu().numpy(), f) and np.array_equal(d.cpu().numpy(), dd.astype(bool))
        K._same(r.cpu().numpy(), rr, "reward %d" % n)
    saved = a.get_state()
    assert saved["t"] == G and np.array_equal(saved["records"].numpy().view(np.uint32), CR.records(state))
    b = CatchVecEnv(E, **kw)
    b.set_state(saved)
    bound = torch.zeros(E, dtype=torch.int32, device="cuda")
    b.bind_actions(bound)                                                    # the static buffer a captured step reads
    out = (torch.empty((E, 4, 32, 32), dtype=torch.uint8, device="cuda"), torch.empty(E, device="cuda"),
           torch.empty(E, dtype=torch.uint8, device="cuda"))
    for n in range(G, 2 * G):
        obs, r, d, _ = a.step_device(torch.from_numpy(acts[n]).cuda())
        bound.copy_(torch.from_numpy(acts[n]))
        b.step_into(*out)
        assert torch.equal(obs, out[0]) and torch.equal(r.view(torch.int32), out[1].view(torch.int32)) and torch.equal(d.view(torch.uint8), out[2])
    assert a.clock_parity() == 1 and b.clock_parity() == 0 and a.get_state()["t"] == b.get_state()["t"] == 2 * G
