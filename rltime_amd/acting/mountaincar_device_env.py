"""MountainCarContinuous-v0 as a device-native vector environment: the car of acting/mountaincar_env.py stepping on the GPU.

A step is ONE kernel (csrc/acting.hip k_mountaincar_env_step, one thread per env) that applies the raw float32 actions,
advances the car in float64, writes the float32 observation, reward and done and — where an episode ended — starts the
next one in the same step, returning the NEW episode's first observation with done = True like MountainCarVecEnv does.  The
env's state is one 32-byte record per env {p, v float64, episodes_started int64, t int32, pad} that the launch updates in
place: no step clock and no host-side parity, so a step captured into a HIP graph replays as it is, with the actions read
from a static buffer bound once (`bind_actions`).  Start positions are Philox draws keyed by (seed, episodes_started, env);
cos(3p) is a fixed polynomial, so tests/mountaincar_restate.py restates whole trajectories bit for bit.  The interface is
CartPoleDeviceVecEnv's; the action buffer is float32 [E, 1].  This class has no CPU implementation."""
import numpy as np
import torch

from rltime_amd._lib import lib, check, ptr, stream
from rltime_amd.acting.mountaincar_env import MAX_EPISODE_STEPS, action_space, observation_space

RECORD_WORDS = 4          # the 32-byte record as int64 words: p, v (float64 bit patterns), episodes_started, t | pad << 32


class MountainCarDeviceVecEnv:
    def __init__(self, num_envs, max_episode_steps=MAX_EPISODE_STEPS, device="cuda", seed=0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("MountainCarDeviceVecEnv steps on the GPU only (csrc/acting.hip k_mountaincar_env_step); "
                             "acting/mountaincar_env.MountainCarVecEnv is the CPU env")
        self.num_envs = int(num_envs)
        self.max_episode_steps = int(max_episode_steps)
        if self.num_envs < 1 or self.max_episode_steps < 1:
            raise ValueError("mountaincar: num_envs >= 1 and max_episode_steps >= 1")
        self.observation_space = observation_space()
        self.action_space = action_space()
        self.seed = int(seed) & 0x7FFFFFFFFFFFFFFF
        self._state = torch.zeros((self.num_envs, RECORD_WORDS), dtype=torch.int64, device=self.device)
        self._actions = None          # the static float32 buffer a step reads (bind_actions), else an own one
        self._own_actions = None
        self._started = False

    # -- launches ---------------------------------------------------------------------------------------
    def _launch(self, obs_out, rewards_out, dones_out, reset_all=0):
        act = None if reset_all else ptr(self._actions if self._actions is not None else self._own_actions)
        check(lib.mirl_mountaincar_env_step(self.num_envs, self.max_episode_steps, act, ptr(self._state), self.seed, reset_all,
                                            ptr(obs_out), ptr(rewards_out), ptr(dones_out), stream()), "mirl_mountaincar_env_step")

    def _fresh(self):
        E = self.num_envs
        return (torch.empty((E, 2), dtype=torch.float32, device=self.device),
                torch.empty(E, dtype=torch.float32, device=self.device), torch.empty(E, dtype=torch.uint8, device=self.device))

    def reset(self):
        """Every env starts an episode (its next one: the draw is keyed by the env's count of episodes started)."""
        obs, rewards, dones = self._fresh()
        self._launch(obs, rewards, dones, reset_all=1)
        self._started = True
        return obs

    def bind_actions(self, actions):
        """The static float32 [E, 1] device buffer every later step reads its actions from (what a captured step needs)."""
        if not (actions.dtype == torch.float32 and actions.is_cuda and actions.is_contiguous() and actions.numel() == self.num_envs):
            raise ValueError("bind_actions: a contiguous float32 device tensor of num_envs elements ([E, 1])")
        self._actions = actions

    def supports_step_into(self):
        """A step writes caller-owned static buffers with a fixed launch (HIP-graph capturable)."""
        return True

    def step_into(self, obs_out, rewards_out, dones_out):
        """obs_out float32 [E, 2], rewards_out float32 [E], dones_out uint8 [E] <- one step on the bound actions."""
        if not self._started:
            raise RuntimeError("MountainCarDeviceVecEnv: reset() before the first step")
        if self._actions is None and self._own_actions is None:
            raise RuntimeError("MountainCarDeviceVecEnv.step_into reads the bound action buffer: bind_actions() first (or use step_device)")
        for t, dtype, n in ((obs_out, torch.float32, 2 * self.num_envs), (rewards_out, torch.float32, self.num_envs),
                            (dones_out, torch.uint8, self.num_envs)):
            if not (t.is_cuda and t.is_contiguous() and t.dtype == dtype and t.numel() == n):
                raise ValueError("step_into: contiguous device tensors obs float32 [E, 2], rewards float32 [E], dones uint8 [E]")
        self._launch(obs_out, rewards_out, dones_out)

    def _as_actions(self, actions):
        a = torch.as_tensor(actions, device=self.device)
        if a.numel() != self.num_envs:
            raise ValueError("mountaincar: one action component per env ([E, 1]), got shape %s" % (tuple(a.shape),))
        return a.reshape(self.num_envs, 1)

    def step_device(self, actions):
        if self._actions is None:
            if self._own_actions is None:
                self._own_actions = torch.zeros((self.num_envs, 1), dtype=torch.float32, device=self.device)
            self._own_actions.copy_(self._as_actions(actions))
        elif actions is not self._actions:
            self._actions.view(self.num_envs, 1).copy_(self._as_actions(actions))
        obs, rewards, dones8 = self._fresh()
        self.step_into(obs, rewards, dones8)
        return obs, rewards, dones8.view(torch.bool), None

    def step(self, actions):
        obs, rewards, dones, _ = self.step_device(torch.as_tensor(np.asarray(actions, dtype=np.float32), device=self.device))
        return obs, rewards.double().cpu().numpy(), dones.cpu().numpy(), [dict() for _ in range(self.num_envs)]

    # -- resume -------------------------------------------------------------------------------------------
    def get_state(self):
        return {"records": self._state.cpu(), "started": self._started}

    def set_state(self, state):
        """The records back in place, so that a resumed run continues bit-identically."""
        self._state.copy_(state["records"].to(self.device))
        self._started = bool(state.get("started", True))

    def close(self):
        pass
