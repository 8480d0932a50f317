"""GPU: the device CartPole (csrc/acting.hip k_cartpole_env_step, rltime_amd/acting/cartpole_device_env.py) against the NumPy
restatement of tests/cartpole_device_restate.py (proved by tests/test_cartpole_device_restate_cpu.py).

The kernel's float64 arithmetic is restated operation by operation, so every comparison is bit for bit: observations and
rewards as int32 patterns, dones as bytes, the 48-byte records word by word.  Every buffer is longer than the kernel may
write and starts out filled with a pattern; the restatement is applied to a host copy of the same buffer, so a write into a
guard element or by a refused call shows as a difference.  Helpers shared with tests/test_acting_kernels_gpu.py are taken
from that module."""
import numpy as np
import pytest
import torch

from tests import cartpole_device_restate as CP
from tests import test_acting_kernels_gpu as K

pytestmark = pytest.mark.gpu

ERR_ARG = K.ERR_ARG
REC_FILL = 0x5A5A5A5A5A5A5A5A
GUARD = 4                                    # guard records / rows behind the E the launch covers


class _CartPole:
    """Device buffers of one env set and their host mirrors: E records (+ guard records), obs / rewards / dones with
    guards, the action buffer.  The records start zeroed, like a fresh CartPoleDeviceVecEnv's."""

    def __init__(self, E, limit, seed):
        self.E, self.limit, self.seed = E, limit, seed
        self.rec = np.full((E + GUARD, 6), REC_FILL, dtype=np.int64)
        self.rec[:E] = 0
        self.obs, self.rew, self.don = K._fill(4 * (E + GUARD), np.float32), K._fill(E + 9, np.float32), K._fill(E + 9, np.uint8)
        self.rec_d = K._up(self.rec.reshape(-1))
        self.obs_d, self.rew_d, self.don_d = K._up(self.obs), K._up(self.rew), K._up(self.don)
        self.act_d = torch.zeros(E + 9, dtype=torch.int32, device="cuda")
        self.state = CP.new_state(E)

    def args(self, reset_all=0):
        return [self.E, self.limit, None if reset_all else K._p(self.act_d), K._p(self.rec_d), self.seed, reset_all,
                K._p(self.obs_d), K._p(self.rew_d), K._p(self.don_d)]

    def expect(self, actions=None):
        """Advance the host mirrors by one launch (actions None: reset_all) -> (rewards, dones)."""
        if actions is None:
            self.state, obs, r, d = CP.cartpole_reset(self.state, self.seed)
        else:
            self.state, obs, r, d = CP.cartpole_step(self.state, actions, self.seed, self.limit)
        E = self.E
        self.obs[:4 * E] = obs.reshape(-1)
        self.rew[:E], self.don[:E] = r, d
        self.rec[:E] = CP.records(self.state)
        return r, d

    def check(self, what):
        torch.cuda.synchronize()
        K._same(K._down(self.don_d, self.don), self.don, what + ": dones")
        K._same(K._down(self.rew_d, self.rew), self.rew, what + ": rewards")
        K._same(K._down(self.rec_d, self.rec).reshape(-1, 6), self.rec, what + ": records")
        K._same(K._down(self.obs_d, self.obs), self.obs, what + ": obs")

    def launch(self, actions=None, compare=True):
        L = K._lib()
        if actions is not None:
            self.act_d[:self.E] = torch.from_numpy(np.asarray(actions, dtype=np.int32)).cuda()
        L.check(L.lib.mirl_cartpole_env_step(*self.args(1 if actions is None else 0), K._st()), "mirl_cartpole_env_step")
        out = self.expect(actions)
        if compare:
            self.check("launch")
        return out


@pytest.mark.parametrize("limit", [7, 9, 200])
@pytest.mark.parametrize("E", [1, 5, 64, 70])
def test_cartpole_rollout_equals_the_restatement(E, limit):
    """reset_all, then 300 steps of seeded random actions from [-1, 3] (everything but 1 pushes left), with obs, rewards,
    dones and the records compared bit for bit after every launch — a trajectory that left the restatement's by one bit
    would end its episode at another step sooner or later.  No episode can end in a fall before its 8th step (the fastest
    fall from the start box, under a constant push), so limit 7 ends every episode on the time limit, limit 200 ends them
    on falls, and limit 9 — with the runs of constant pushes below — has both kinds in one rollout.  E = 70 takes a second
    wave with a ragged tail."""
    env = _CartPole(E, limit, seed=300 + 11 * E + limit)
    g = np.random.default_rng(E * 1000 + limit)
    r, d = env.launch()
    assert not r.any() and d.all()
    assert np.array_equal(env.state["episodes_started"], np.ones(E, np.int64))
    timed, fell, ends = 0, 0, 0
    for n in range(300):
        t_before = env.state["t"].copy()
        # ten constant pushes in every fifty steps: the pole falls at the 8th or 9th of them
        actions = g.integers(-1, 4, E).astype(np.int32) if n % 50 >= 10 else np.zeros(E, np.int32)
        r, d = env.launch(actions)
        assert np.all(r == 1.0)
        ends += int(d.sum())
        timed += int(((t_before + 1 >= limit) & (d == 1)).sum())
        fell += int(((t_before + 1 < limit) & (d == 1)).sum())
    assert ends == int(env.state["episodes_started"].sum()) - E
    assert (fell == 0 and timed > 0) if limit == 7 else (fell > 0 and timed > 0) if limit == 9 else (fell > 0 and timed == 0)
    r, d = env.launch()                                                      # reset_all mid-run: the NEXT episode of every env
    assert not r.any() and d.all() and not env.state["t"].any()


def test_cartpole_refuses_bad_arguments_and_writes_nothing():
    L = K._lib()
    env = _CartPole(6, 50, seed=4)
    env.launch()
    env.launch(np.array([1, 0, 1, 1, 0, 2], dtype=np.int32))
    rec8, obs4 = env.rec_d[1:], env.obs_d[1:]
    assert rec8.data_ptr() % 16 == 8 and obs4.data_ptr() % 16 == 4
    bad = [(0, 0), (0, -1), (0, 2 ** 24 + 1), (1, 0), (1, -5), (2, None), (3, None), (3, K._p(rec8)), (5, 2), (5, -1), (6, None),
           (6, K._p(obs4)), (7, None), (8, None)]
    for pos, value in bad:
        a = env.args() + [K._st()]
        a[pos] = value
        assert L.lib.mirl_cartpole_env_step(*a) == ERR_ARG, (pos, value)
        assert "cartpole_env_step" in L.last_error()
    env.check("after refusals")
    a = env.args(reset_all=1) + [K._st()]                                    # reset_all = 1 takes NULL actions
    assert L.lib.mirl_cartpole_env_step(*a) == 0
    env.expect(None)
    env.check("reset_all with NULL actions")


def _rollout_eager(E, limit, seed, acts):
    """The class, eagerly: reset, then step_device on every row of `acts` -> list of (obs, rewards, dones) host arrays."""
    from rltime_amd.acting.cartpole_device_env import CartPoleDeviceVecEnv
    env = CartPoleDeviceVecEnv(E, max_episode_steps=limit, seed=seed)
    first = env.reset().cpu().numpy()
    out = []
    for a in acts:
        obs, r, d, info = env.step_device(torch.from_numpy(a).cuda())
        assert info is None and d.dtype == torch.bool
        out.append((obs.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy().astype(np.uint8)))
    return env, first, out


def test_cartpole_class_static_buffers_and_captured_graph_equal_the_eager_rollout():
    """step_into on static buffers with the bound action buffer, and the same steps replayed from ONE captured
    torch.cuda.graph, return what the eager step_device rollout returns — which is the restatement's.  The launch has no
    host-side parity: one capture replays for every step."""
    from rltime_amd.acting.cartpole_device_env import CartPoleDeviceVecEnv
    E, limit, seed, steps = 70, 9, 21, 40
    acts = np.random.default_rng(8).integers(-1, 3, (steps, E)).astype(np.int32)
    ref_env, first, eager = _rollout_eager(E, limit, seed, acts)
    state, obs0, _, _ = CP.cartpole_reset(CP.new_state(E), seed)
    K._same(first, obs0, "reset obs")
    for n in range(steps):
        state, o, r, d = CP.cartpole_step(state, acts[n], seed, limit)
        K._same(eager[n][0], o, "obs %d" % n), K._same(eager[n][1], r, "rewards %d" % n), K._same(eager[n][2], d, "dones %d" % n)
    assert any(e[2].any() for e in eager)
    K._same(ref_env.get_state()["records"].numpy(), CP.records(state), "records")
    for mode in ("static", "graph"):
        env = CartPoleDeviceVecEnv(E, max_episode_steps=limit, seed=seed)
        assert env.supports_step_into()
        with pytest.raises(RuntimeError):
            env.step_into(*env._fresh())                                     # no reset yet
        K._same(env.reset().cpu().numpy(), obs0, "reset obs")
        bound = torch.zeros(E, dtype=torch.int32, device="cuda")
        env.bind_actions(bound)
        out = env._fresh()
        graph = None
        if mode == "graph":
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                env.step_into(*out)
        for n in range(steps):
            bound.copy_(torch.from_numpy(acts[n]))
            if graph is None:
                env.step_into(*out)
            else:
                graph.replay()
            got = [t.cpu().numpy() for t in out]
            for g_, w_, what in zip(got, eager[n], ("obs", "rewards", "dones")):
                K._same(g_, w_, "%s, step %d: %s" % (mode, n, what))
        K._same(env.get_state()["records"].numpy(), CP.records(state), mode + ": records")


def test_cartpole_resumes_bit_identically():
    """get_state -> a fresh env -> set_state continues with identical outputs, and the host step() wrapper returns the same
    transitions as step_device."""
    from rltime_amd.acting.cartpole_device_env import CartPoleDeviceVecEnv
    E, limit, seed = 5, 12, 33
    acts = np.random.default_rng(2).integers(0, 2, (60, E)).astype(np.int32)
    a, _, _ = _rollout_eager(E, limit, seed, acts[:30])
    saved = a.get_state()
    assert saved["records"].shape == (E, 6) and saved["started"]
    b = CartPoleDeviceVecEnv(E, max_episode_steps=limit, seed=seed)
    b.set_state(saved)
    ends = 0
    for n in range(30, 60):
        oa, ra, da, _ = a.step_device(torch.from_numpy(acts[n]).cuda())
        ob, rb, db, infos = b.step(acts[n])
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)) and np.array_equal(ra.cpu().numpy(), rb) \
            and np.array_equal(da.cpu().numpy(), db) and infos == [dict()] * E
        ends += int(db.sum())
    assert ends > 0 and torch.equal(a.get_state()["records"], b.get_state()["records"])
    assert a.observation_space.shape == (4,) and a.observation_space.dtype == np.float32 and a.action_space.n == 2
