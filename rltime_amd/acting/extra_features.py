"""The reference's ExtraFeaturesEnvWrapper (rltime/env_wrappers/common.py:221-332) for a device-native vector env: the
observation becomes (frames, extras), where extras is a float32 row per env holding the one-hot last action, the scaled
timestep since the env's last reset and the (clipped) last reward — typically the extra input of the model's LSTM layer
(models/torch/sequential.py).

A vector step's rows are ONE launch after the inner env's step (csrc/acting.hip k_extra_features): it reads the actions
just executed, the env's raw rewards and dones and the wrapper's per-env timestep counters, and writes the rows of the
observation that follows — the reset row wherever the auto-resetting vector env reset (vec_env/simple.py:25-29).  The
launch has no host state, so it rides in the captured rollout graph of acting/fast_step.py, which hands it its own two
destinations (`write_extras`: the compact block the replay ingests as `extra`, and the extras columns of the LSTM
product's input rows); `step_device` / `reset` are the same launch into a fresh [E, X] tensor."""
import ctypes as C

import numpy as np
import torch

from rltime_amd._lib import lib, ptr, stream, check
from rltime_amd.spaces import Box, Tuple

# what the fast acting step probes on an env (acting/fast_step.py), answered by the wrapped env
_FORWARDED = ("supports_step_into", "step_into", "step_pre", "step_into_args", "bind_actions", "clock_parity", "skip_host",
              "advance_host", "frame_stack")


class ExtraFeaturesVecEnv:
    def __init__(self, env, include_action=True, include_reward=True, include_timestep=True, clip_reward=True,
                 timestep_scale=1. / 100000, use_real_done=True):
        """The reference wrapper's arguments and defaults.  `use_real_done` tells the reference to restart the timestep
        only on real episode ends and not on simulated ones (end-of-life dones); the device envs have no simulated
        dones, so it is accepted with either value and changes nothing."""
        if not hasattr(env, "step_device") or torch.device(getattr(env, "device", "cpu")).type != "cuda":
            raise ValueError("ExtraFeaturesVecEnv wraps an env that steps on the device ('catch', 'synthetic-atari'): the "
                             "feature rows are written by a HIP kernel and there is no CPU implementation")
        if not hasattr(env.action_space, "n"):
            raise ValueError("ExtraFeaturesVecEnv: discrete action spaces only (the device actors are discrete)")
        if hasattr(env.observation_space, "spaces"):
            raise ValueError("ExtraFeaturesVecEnv: the wrapped env already has a tuple observation")
        self.env = env
        self.num_envs = int(env.num_envs)
        self.device = torch.device(env.device)
        self.action_space = env.action_space
        self._flags = (int(bool(include_action)), int(bool(include_reward)), int(bool(include_timestep)))
        self._clip = int(bool(clip_reward))
        self._scale = float(timestep_scale)
        self.use_real_done = bool(use_real_done)
        X = C.c_int32()
        if lib.mirl_extra_features_size(int(self.action_space.n), *self._flags, C.byref(X)) < 0:
            raise ValueError("extra_features: at least one of include_action / include_reward / include_timestep "
                             "(and 1 <= number of actions <= 4096)")
        self.extra_size = int(X.value)
        self.observation_space = Tuple((env.observation_space, Box(-np.inf, np.inf, (self.extra_size,), np.float32)))
        E = self.num_envs
        self._counters = torch.zeros(E, dtype=torch.int32, device=self.device)      # timesteps since reset
        self._rows = torch.zeros((E, self.extra_size), dtype=torch.float32, device=self.device)
        self._all_done = torch.ones(E, dtype=torch.uint8, device=self.device)
        self._no_reward = torch.zeros(E, dtype=torch.float32, device=self.device)
        self._no_action = torch.zeros(E, dtype=torch.int32, device=self.device)

    def __getattr__(self, name):
        if name in _FORWARDED and "env" in self.__dict__:
            return getattr(self.__dict__["env"], name)
        raise AttributeError(name)

    # -- the launch -------------------------------------------------------------------------------------
    def write_extras(self, actions, rewards, dones, compact=None, pitched=None, pitch=0, col0=0):
        """This step's rows, after the inner env's step: actions int32 [E] (the ones just executed), rewards float32 [E]
        (raw), dones uint8 [E] -> compact float32 [E, X] and / or columns [col0, col0 + X) of the float32 matrix `pitched`
        with rows of `pitch` floats.  Advances the timestep counters.  Stream-ordered, capturable."""
        check(lib.mirl_extra_features_step(self.num_envs, int(self.action_space.n), *self._flags, self._clip, self._scale,
                                           ptr(actions), ptr(rewards), ptr(dones), ptr(self._counters), ptr(compact), ptr(pitched),
                                           int(pitch), int(col0), stream()), "mirl_extra_features_step")

    def reset_extras(self, compact=None, pitched=None, pitch=0, col0=0):
        """Every env starts an episode: the reset rows (one-hot of action 0, timestep 0, reward 0), counters 0."""
        self.write_extras(self._no_action, self._no_reward, self._all_done, compact, pitched, pitch, col0)

    def _fresh(self):
        return torch.empty((self.num_envs, self.extra_size), dtype=torch.float32, device=self.device)

    # -- the vector env -----------------------------------------------------------------------------------
    def reset(self):
        frames = self.env.reset()
        self._rows = self._fresh()
        self.reset_extras(self._rows)
        return frames, self._rows

    def step_device(self, actions):
        acts = torch.as_tensor(actions, device=self.device).reshape(-1).to(torch.int32).contiguous()
        frames, rewards, dones, stats = self.env.step_device(acts)
        self._rows = self._fresh()
        self.write_extras(acts, rewards.to(torch.float32).contiguous(), dones.to(torch.uint8), self._rows)
        return (frames, self._rows), rewards, dones, stats

    def step(self, actions):
        obs, rewards, dones, _ = self.step_device(torch.as_tensor(np.asarray(actions), device=self.device))
        return obs, rewards.double().cpu().numpy(), dones.cpu().numpy(), [dict() for _ in range(self.num_envs)]

    # -- resume -------------------------------------------------------------------------------------------
    def get_state(self):
        return {"env": self.env.get_state(), "counters": self._counters.cpu(), "rows": self._rows.cpu()}

    def set_state(self, state):
        self.env.set_state(state["env"])
        self._counters.copy_(state["counters"].to(self.device))
        self._rows = state["rows"].to(self.device).clone()

    def close(self):
        self.env.close()
