"""GPU: the device MountainCarContinuous (csrc/acting.hip k_mountaincar_env_step, rltime_amd/acting/mountaincar_device_env.py)
against the NumPy restatement of tests/mountaincar_restate.py (proved by tests/test_mountaincar_restate_cpu.py).

The kernel's float64 arithmetic is restated operation by operation, so every comparison is bit for bit: observations and
rewards as int32 patterns, dones as bytes, the 32-byte records word by word.  Every buffer is longer than the kernel may
write and starts out filled with a pattern; the restatement is applied to a host copy of the same buffer, so a write into a
guard element or by a refused call shows as a difference.  Helpers shared with tests/test_acting_kernels_gpu.py are taken
from that module."""
import numpy as np
import pytest
import torch

from tests import mountaincar_restate as MC
from tests import test_acting_kernels_gpu as K

pytestmark = pytest.mark.gpu

ERR_ARG = K.ERR_ARG
REC_FILL = 0x5A5A5A5A5A5A5A5A
GUARD = 4                                    # guard records / rows behind the E the launch covers
LIMIT, STEPS = 40, 150


class _MountainCar:
    """Device buffers of one env set and their host mirrors: E records (+ guard records), obs / rewards / dones with
    guards, the action buffer.  The records start zeroed, like a fresh MountainCarDeviceVecEnv's."""

    def __init__(self, E, limit, seed):
        self.E, self.limit, self.seed = E, limit, seed
        self.rec = np.full((E + GUARD, 4), REC_FILL, dtype=np.int64)
        self.rec[:E] = 0
        self.obs, self.rew, self.don = K._fill(2 * (E + GUARD), np.float32), K._fill(E + 9, np.float32), K._fill(E + 9, np.uint8)
        self.rec_d = K._up(self.rec.reshape(-1))
        self.obs_d, self.rew_d, self.don_d = K._up(self.obs), K._up(self.rew), K._up(self.don)
        self.act_d = torch.zeros(E + 9, dtype=torch.float32, device="cuda")

    def args(self, reset_all=0):
        return [self.E, self.limit, None if reset_all else K._p(self.act_d), K._p(self.rec_d), self.seed, reset_all,
                K._p(self.obs_d), K._p(self.rew_d), K._p(self.don_d)]

    def put(self, state):
        """set_state: the records of `state` into the device buffer and its mirror."""
        self.rec[:self.E] = MC.records(state)
        self.rec_d.view(-1, 4)[:self.E] = torch.from_numpy(self.rec[:self.E]).cuda()

    def expect(self, state, obs, r, d):
        E = self.E
        self.obs[:2 * E] = obs.reshape(-1)
        self.rew[:E], self.don[:E] = r, d
        self.rec[:E] = MC.records(state)

    def check(self, what):
        torch.cuda.synchronize()
        K._same(K._down(self.don_d, self.don), self.don, what + ": dones")
        K._same(K._down(self.rew_d, self.rew), self.rew, what + ": rewards")
        K._same(K._down(self.rec_d, self.rec).reshape(-1, 4), self.rec, what + ": records")
        K._same(K._down(self.obs_d, self.obs), self.obs, what + ": obs")

    def launch(self, actions=None):
        L = K._lib()
        if actions is not None:
            self.act_d[:self.E] = torch.from_numpy(np.asarray(actions, dtype=np.float32)).cuda()
        L.check(L.lib.mirl_mountaincar_env_step(*self.args(1 if actions is None else 0), K._st()), "mirl_mountaincar_env_step")


@pytest.fixture(scope="module")
def rollouts():
    """The pinned trajectories, computed once per E and never modified."""
    cache = {}

    def get(E):
        if E not in cache:
            cache[E] = MC.pinned_rollout(E, seed=17 + E, limit=LIMIT, steps=STEPS)
        return cache[E]
    return get


@pytest.mark.parametrize("E", [1, 64, 65, 200])
def test_mountaincar_rollout_equals_the_restatement(E, rollouts):
    """reset_all, then 150 steps (limit 40) on the restatement's fixed action stream — |a| > 1 on both sides included —
    with the set_state placements (left wall, goal, both speed clips, right wall), obs, rewards, dones and the records
    compared bit for bit after every launch, guard elements included.  E = 65 and 200 take more than one workgroup with a
    ragged tail."""
    (state0, obs0), steps, reached = rollouts(E)
    for name in ("goal", "time_limit", "wall_left", "wall_right", "speed_high", "speed_low", "action_low", "action_high", "action_inside"):
        assert reached.get(name, 0) > 0, (name, reached)
    env = _MountainCar(E, LIMIT, seed=17 + E)
    env.launch()
    env.expect(state0, obs0, np.zeros(E, np.float32), np.ones(E, np.uint8))
    env.check("reset_all")
    for n, s in enumerate(steps):
        if s["placed"] is not None:
            env.put(s["placed"])
        env.launch(s["actions"])
        env.expect(s["state"], s["obs"], s["rewards"], s["dones"])
        env.check("step %d" % n)
    state, obs, r, d = MC.mountaincar_reset(steps[-1]["state"], 17 + E)      # reset_all mid-run: the NEXT episode of every env
    env.launch()
    env.expect(state, obs, r, d)
    env.check("reset_all mid-run")


def test_mountaincar_refuses_bad_arguments_and_writes_nothing():
    L = K._lib()
    E = 6
    env = _MountainCar(E, 50, seed=4)
    state, obs, r, d = MC.mountaincar_reset(MC.new_state(E), 4)
    env.launch()
    env.expect(state, obs, r, d)
    acts = np.array([1.5, -0.25, 0.0, -3.0, 1.0, 0.5], dtype=np.float32)
    state, obs, r, d = MC.mountaincar_step(state, acts, 4, 50)
    env.launch(acts)
    env.expect(state, obs, r, d)
    env.check("one step")
    rec8 = env.rec_d[1:]
    assert rec8.data_ptr() % 16 == 8
    bad = [(0, 0), (0, -1), (0, 2 ** 24 + 1), (1, 0), (1, -5), (2, None), (3, None), (3, K._p(rec8)), (5, 2), (5, -1), (6, None),
           (7, None), (8, None)]
    for pos, value in bad:
        a = env.args() + [K._st()]
        a[pos] = value
        assert L.lib.mirl_mountaincar_env_step(*a) == ERR_ARG, (pos, value)
        assert "mountaincar_env_step" in L.last_error()
    env.check("after refusals")
    a = env.args(reset_all=1) + [K._st()]                                    # reset_all = 1 takes NULL actions
    assert L.lib.mirl_mountaincar_env_step(*a) == 0
    env.expect(*MC.mountaincar_reset(state, 4))
    env.check("reset_all with NULL actions")


def _class_rollout(E, seed, steps_list, mode):
    """MountainCarDeviceVecEnv over the pinned steps.  mode "eager": step_device; "static": step_into on static buffers
    with a bound action buffer; "graph": ONE captured torch.cuda.graph of that step replayed for every step.  Placements go
    through get_state / set_state.  -> (env, reset obs, list of (obs, rewards, dones) host arrays)."""
    from rltime_amd.acting.mountaincar_device_env import MountainCarDeviceVecEnv
    env = MountainCarDeviceVecEnv(E, max_episode_steps=LIMIT, seed=seed)
    assert env.supports_step_into() and env.action_space.shape == (1,) and not hasattr(env.action_space, "n")
    assert env.observation_space.shape == (2,) and env.observation_space.dtype == np.float32
    with pytest.raises(RuntimeError):
        env.step_into(*env._fresh())                                         # no reset yet
    first = env.reset().cpu().numpy()
    bound, out, graph = None, None, None
    if mode != "eager":
        bound = torch.zeros((E, 1), dtype=torch.float32, device="cuda")
        env.bind_actions(bound)
        out = env._fresh()
        if mode == "graph":
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):                                    # (a capture runs nothing: the records stay)
                env.step_into(*out)
    got = []
    for s in steps_list:
        if s["placed"] is not None:
            env.set_state({"records": torch.from_numpy(MC.records(s["placed"])), "started": True})
        a = torch.from_numpy(s["actions"].reshape(E, 1))
        if mode == "eager":
            obs, r, d, info = env.step_device(a.cuda())
            assert info is None and d.dtype == torch.bool and obs.shape == (E, 2)
            got.append((obs.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy().astype(np.uint8)))
            continue
        bound.copy_(a)
        if graph is None:
            env.step_into(*out)
        else:
            graph.replay()
        got.append(tuple(t.cpu().numpy() for t in out))
    return env, first, got


@pytest.mark.parametrize("mode", ["eager", "static", "graph"])
def test_mountaincar_class_eager_static_and_captured_steps_equal_the_restatement(mode, rollouts):
    """The class over the pinned E = 65 trajectory: step_device, step_into on static buffers with the bound float32 [E, 1]
    action buffer, and the same step replayed from ONE captured torch.cuda.graph all return the restatement's bytes, the
    records included.  The launch has no host-side parity: one capture replays for every step."""
    E = 65
    (state0, obs0), steps, _ = rollouts(E)
    env, first, got = _class_rollout(E, 17 + E, steps, mode)
    K._same(first, obs0, "reset obs")
    for n, (s, g) in enumerate(zip(steps, got)):
        K._same(g[0], s["obs"], "%s obs %d" % (mode, n))
        K._same(g[1], s["rewards"], "%s rewards %d" % (mode, n))
        K._same(g[2], s["dones"], "%s dones %d" % (mode, n))
    K._same(env.get_state()["records"].numpy(), MC.records(steps[-1]["state"]), mode + ": records")
    with pytest.raises(ValueError, match="float32"):
        env.bind_actions(torch.zeros(E, dtype=torch.int32, device="cuda"))


def test_mountaincar_resumes_bit_identically(rollouts):
    """get_state -> a fresh env -> set_state continues with identical outputs, and the host step() wrapper returns the same
    transitions as step_device."""
    from rltime_amd.acting.mountaincar_device_env import MountainCarDeviceVecEnv
    E = 1
    (_, _), steps, _ = rollouts(E)
    a, _, _ = _class_rollout(E, 17 + E, steps[:60], "eager")
    saved = a.get_state()
    assert saved["records"].shape == (E, 4) and saved["started"]
    b = MountainCarDeviceVecEnv(E, max_episode_steps=LIMIT, seed=17 + E)
    b.set_state(saved)
    ends = 0
    for s in steps[60:110]:
        if s["placed"] is not None:
            for env in (a, b):
                env.set_state({"records": torch.from_numpy(MC.records(s["placed"])), "started": True})
        oa, ra, da, _ = a.step_device(torch.from_numpy(s["actions"].reshape(E, 1)).cuda())
        ob, rb, db, infos = b.step(s["actions"].reshape(E, 1))
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)) and np.array_equal(ra.double().cpu().numpy(), rb) \
            and np.array_equal(da.cpu().numpy(), db) and infos == [dict()] * E
        K._same(oa.cpu().numpy(), s["obs"], "resumed obs")
        ends += int(db.sum())
    assert ends > 0 and torch.equal(a.get_state()["records"], b.get_state()["records"])


def test_train_builds_the_device_env_from_the_env_string():
    from rltime_amd import train
    from rltime_amd.acting.mountaincar_device_env import MountainCarDeviceVecEnv
    env = train.make_vec_env("MountainCarContinuous-v0", {"device": True, "max_episode_steps": 40}, 3, "cuda", seed=5)
    assert isinstance(env, MountainCarDeviceVecEnv) and env.max_episode_steps == 40 and env.seed == 5 and env.num_envs == 3
    assert train.make_vec_env("MountainCarContinuous-v0", {"device": True}, 2, "cuda").max_episode_steps == 999
