"""MountainCarContinuous-v0 as a host-side vector env for the CPU config `mountaincar_continuous_ppo.json` (the reference's
config of that name, rltime/configs/mountaincar_continuous_ppo.json), the way acting/cartpole_env.py serves `cartpole_ppo.json`.

gym is not installed here, so this is the build's own statement of the task (Moore 1990; gym's Continuous_MountainCarEnv):
an under-powered car in a valley, state (position p, velocity v), one unbounded float32 action component a per step:

    f = clip(a, -1, 1);  v += f * 0.0015 - 0.0025 * cos(3 p);  v = clip(v, -0.07, 0.07)
    p += v;  p = clip(p, -1.2, 0.6);  at the left wall (p == -1.2) a negative velocity is zeroed
    done = p >= 0.45 and v >= 0;  reward = (100 if done else 0) - 0.1 a^2  (the RAW action's cost, not the clipped force's)

An episode starts at p uniform in [-0.6, -0.4) with v = 0 and also ends after `max_episode_steps` (999: gym's TimeLimit for
this id).  Vectorised over envs with NumPy float64 and auto-resetting like CartPoleVecEnv: a finished env returns the NEW
episode's first observation with done=True, and each transition's info carries `episode_info`."""
import numpy as np

from rltime_amd.spaces import Box

MIN_ACTION, MAX_ACTION = -1.0, 1.0
MIN_POSITION, MAX_POSITION, MAX_SPEED = -1.2, 0.6, 0.07
GOAL_POSITION, GOAL_VELOCITY = 0.45, 0.0
POWER, GRAVITY_TERM = 0.0015, 0.0025
START_LOW, START_HIGH = -0.6, -0.4
GOAL_REWARD, ACTION_COST = 100.0, 0.1
MAX_EPISODE_STEPS = 999


def observation_space():
    return Box(np.array([MIN_POSITION, -MAX_SPEED], np.float32), np.array([MAX_POSITION, MAX_SPEED], np.float32), (2,), np.float32)


def action_space():
    return Box(np.array([MIN_ACTION], np.float32), np.array([MAX_ACTION], np.float32), (1,), np.float32)


class MountainCarVecEnv:
    def __init__(self, num_envs, max_episode_steps=MAX_EPISODE_STEPS, seed=0):
        self.num_envs = int(num_envs)
        self.max_episode_steps = int(max_episode_steps)
        if self.num_envs < 1 or self.max_episode_steps < 1:
            raise ValueError("mountaincar: num_envs >= 1 and max_episode_steps >= 1")
        self.observation_space = observation_space()
        self.action_space = action_space()
        self._rng = np.random.RandomState(seed)
        self._x = np.zeros((self.num_envs, 2), np.float64)       # position, velocity
        self._t = np.zeros(self.num_envs, np.int64)
        self._ret = np.zeros(self.num_envs, np.float64)

    def _fresh(self, count):
        return np.stack([self._rng.uniform(START_LOW, START_HIGH, size=count), np.zeros(count)], axis=1)

    def reset(self):
        self._x[:] = self._fresh(self.num_envs)
        self._t[:] = 0
        self._ret[:] = 0
        return self._x.astype(np.float32)

    def step(self, actions):
        a = np.asarray(actions, dtype=np.float32).reshape(self.num_envs).astype(np.float64)
        p, v = self._x.T
        f = np.where(a < MIN_ACTION, MIN_ACTION, np.where(a > MAX_ACTION, MAX_ACTION, a))
        v = v + (f * POWER - GRAVITY_TERM * np.cos(3.0 * p))
        v = np.where(v > MAX_SPEED, MAX_SPEED, v)
        v = np.where(v < -MAX_SPEED, -MAX_SPEED, v)
        p = p + v
        p = np.where(p > MAX_POSITION, MAX_POSITION, p)
        p = np.where(p < MIN_POSITION, MIN_POSITION, p)
        v = np.where((p == MIN_POSITION) & (v < 0.0), 0.0, v)
        goal = (p >= GOAL_POSITION) & (v >= GOAL_VELOCITY)
        self._x = np.stack([p, v], axis=1)
        self._t += 1
        rewards = np.where(goal, GOAL_REWARD, 0.0) - (a * a) * ACTION_COST
        self._ret += rewards
        dones = goal | (self._t >= self.max_episode_steps)
        infos = [{"episode_info": {"reward": float(self._ret[i]), "length": int(self._t[i]), "done": bool(dones[i])}}
                 for i in range(self.num_envs)]
        if dones.any():
            idx = np.nonzero(dones)[0]
            self._x[idx] = self._fresh(len(idx))
            self._t[idx] = 0
            self._ret[idx] = 0
        return self._x.astype(np.float32), rewards, dones, infos

    # -- placement (tests; a resumed run) ----------------------------------------------------------------
    def get_state(self):
        return {"x": self._x.copy(), "t": self._t.copy(), "ret": self._ret.copy(), "rng": self._rng.get_state()}

    def set_state(self, state):
        self._x = np.array(state["x"], dtype=np.float64).reshape(self.num_envs, 2)
        self._t = np.array(state["t"], dtype=np.int64).reshape(self.num_envs)
        self._ret = np.array(state.get("ret", np.zeros(self.num_envs)), dtype=np.float64).reshape(self.num_envs)
        if state.get("rng") is not None:
            self._rng.set_state(state["rng"])

    def close(self):
        pass
