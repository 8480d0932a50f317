"""Catch as a device-native vector environment: the one game in the tree a policy can be better or worse at.

A ball falls one cell row per step down a G x G grid from a uniformly drawn column; the paddle on the bottom row moves
left (action 1), right (action 2) or stays (any other action).  After G - 1 steps the episode ends with reward +1 when
the paddle is under the ball and -1 otherwise, and the next episode starts in the same step.  Observations are P history
planes of S x S uint8 (plane P - 1 newest; ball 255, paddle 128; planes from before the episode began are zero, as the
frame-stack wrapper returns them); `visible_rows` < G hides the ball on its last rows, which makes the game partially
observable.  The ball column is independent of everything before it, so a policy whose actions carry no information
about the ball catches with probability exactly 1 / G.

A step is ONE kernel (csrc/acting.hip k_catch_env_step) that applies the actions, renders the frames and writes reward
and done; the env's state is one 16-byte record per env that lives on the device next to the step counter, both as
pairs read / written alternately.  Like the synthetic env's step it writes caller-owned static buffers with a fixed
launch, so it rides in the captured rollout graph (acting/fast_step.py) — with the actions read from a static buffer
bound once (`bind_actions`).  There is no CPU implementation."""
import numpy as np
import torch

from rltime_amd._lib import lib, check, ptr, stream
from rltime_amd.spaces import Box, Discrete


class CatchVecEnv:
    def __init__(self, num_envs, frame_shape=(4, 36, 36), grid=6, n_actions=3, visible_rows=None, device="cuda", seed=0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("CatchVecEnv steps on the GPU only (csrc/acting.hip k_catch_env_step): there is no CPU implementation")
        P, S, S2 = (int(v) for v in frame_shape)
        G = int(grid)
        V = G if visible_rows is None else int(visible_rows)
        if not (S == S2 and 1 <= P <= 4 and 2 <= G <= 128 and S % G == 0 and (S * S) % 16 == 0 and n_actions >= 3 and 1 <= V <= G):
            raise ValueError("catch: frame_shape (P <= 4, S, S) with S % grid == 0 and S * S % 16 == 0, 2 <= grid <= 128, "
                             "n_actions >= 3, 1 <= visible_rows <= grid")
        self.num_envs = int(num_envs)
        self.observation_space = Box(0, 255, (P, S, S), np.uint8)
        self.action_space = Discrete(int(n_actions))
        self.grid, self.visible_rows = G, V
        self.seed = int(seed) & 0x7FFFFFFFFFFFFFFF
        self._dims = (self.num_envs, P, S, G, V, int(n_actions))
        E = self.num_envs
        # the state records and the step counter: PAIRS of device blocks read / written alternately (a launch reads half
        # `slot`, writes half slot ^ 1: no workgroup sees the new values, no atomics); the host only tracks the parity
        self._state = torch.zeros((2, E, 4), dtype=torch.int32, device=self.device)
        self._clock = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._slot = 0
        self._actions = None          # the static int32 buffer a step reads (bind_actions), else an own one
        self._own_actions = None
        self._started = False

    # -- launches ---------------------------------------------------------------------------------------
    def _args(self, obs_out, rewards_out, dones_out, reset_all=0):
        act = None if reset_all else ptr(self._actions if self._actions is not None else self._own_actions)
        return (*self._dims, act, ptr(self._state), ptr(self._clock), self._slot, self.seed, reset_all,
                ptr(obs_out), ptr(rewards_out), ptr(dones_out))

    def _fresh(self):
        E = self.num_envs
        return (torch.empty((E,) + tuple(self.observation_space.shape), dtype=torch.uint8, device=self.device),
                torch.empty(E, dtype=torch.float32, device=self.device), torch.empty(E, dtype=torch.uint8, device=self.device))

    def reset(self):
        """Every env starts an episode keyed by the current step counter (0 for a new env), which is not advanced."""
        obs, rewards, dones = self._fresh()
        check(lib.mirl_catch_env_step(*self._args(obs, rewards, dones, reset_all=1), stream()), "mirl_catch_env_step")
        self._slot ^= 1
        self._started = True
        return obs

    def bind_actions(self, actions):
        """The static int32 [E] device buffer every later step reads its actions from (what a captured step needs)."""
        if not (actions.dtype == torch.int32 and actions.is_cuda and actions.is_contiguous() and actions.numel() == self.num_envs):
            raise ValueError("bind_actions: a contiguous int32 device tensor of num_envs elements")
        self._actions = actions

    def supports_step_into(self):
        """A step writes caller-owned static buffers with a fixed launch (HIP-graph capturable)."""
        return True

    def _need_actions(self):
        if not self._started:
            raise RuntimeError("CatchVecEnv: reset() before the first step")
        if self._actions is None and self._own_actions is None:
            raise RuntimeError("CatchVecEnv.step_into reads the bound action buffer: bind_actions() first (or use step_device)")

    def step_into(self, obs_out, rewards_out, dones_out):
        """obs_out uint8 [E, P, S, S], rewards_out float32 [E], dones_out uint8 [E] <- step t = clock + 1 on the bound actions."""
        self._need_actions()
        check(lib.mirl_catch_env_step(*self._args(obs_out, rewards_out, dones_out), stream()), "mirl_catch_env_step")
        self._slot ^= 1

    def step_pre(self, obs_out, rewards_out, dones_out, pre_args):
        """The env step and the actor's pre-step as ONE launch; pre_args: mirl_actor_pre's arguments from H on."""
        self._need_actions()
        check(lib.mirl_catch_env_step_pre(*self._args(obs_out, rewards_out, dones_out), *pre_args), "mirl_catch_env_step_pre")
        self._slot ^= 1

    def advance_host(self):
        self._slot ^= 1

    def clock_parity(self):
        """Which half of the clock / state pairs the NEXT step reads: part of the identity of a captured rollout."""
        return self._slot

    def skip_host(self, steps):
        """`steps` steps were replayed from a captured graph: advance the host-side parity like step_into would have."""
        self._slot ^= steps & 1

    def step_device(self, actions):
        if self._actions is None:
            if self._own_actions is None:
                self._own_actions = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
            self._own_actions.copy_(torch.as_tensor(actions, device=self.device).reshape(-1))
        elif actions is not self._actions:
            self._actions.copy_(torch.as_tensor(actions, device=self.device).reshape(-1))
        obs, rewards, dones8 = self._fresh()
        self.step_into(obs, rewards, dones8)
        return obs, rewards, dones8.view(torch.bool), None

    def step(self, actions):
        obs, rewards, dones, _ = self.step_device(torch.as_tensor(np.asarray(actions), device=self.device))
        return obs, rewards.double().cpu().numpy(), dones.cpu().numpy(), [dict() for _ in range(self.num_envs)]

    # -- resume -------------------------------------------------------------------------------------------
    def get_state(self):
        return {"t": int(self._clock[self._slot].item()), "records": self._state[self._slot].cpu(), "started": self._started}

    def set_state(self, state):
        """Written back into half 0, so that a resumed run continues bit-identically."""
        self._clock.zero_()
        self._clock[0] = int(state["t"])
        self._state.zero_()
        self._state[0].copy_(state["records"].to(self.device))
        self._slot = 0
        self._started = bool(state.get("started", True))

    def close(self):
        pass
