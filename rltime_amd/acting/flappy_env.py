"""Flappy as a device-native vector environment: long episodes, control under gravity, velocity hidden from one frame.

A bird in column 1 of an R x C grid of `cell`-pixel cells (R = H / cell rows, row 0 on top; C = W / cell columns) flaps
(action 1: velocity -2) or falls (any other action: velocity + 1, at most +2) while pipes `spacing` columns apart scroll
left one column per step.  Each pipe spans every row but a gap of `gap` rows whose top is drawn uniformly from
[0, R - gap] by Philox keyed with (seed, env, episode number, pipe number) and nothing else.  Passing a pipe gives +1;
hitting one or the floor ends the episode with `death_reward`; the ceiling clamps; `max_episode_steps` ends it with the
step's own reward; the next episode starts in the same step.  Observations are P history planes of H x W uint8 (plane
P - 1 newest; bird 255, pipes 128; planes from before the episode began are zero, as the frame-stack wrapper returns
them).  One plane shows the bird's row but not its velocity, so P = 1 is partially observable; P = 4 shows it.  A pipe's
gap is independent of everything drawn before it, so a policy whose actions carry no information about the frames passes
each pipe with probability at most gap / (R - gap + 1) (tests/flappy_restate.py derives the bound).

A step is ONE kernel (csrc/acting.hip k_flappy_env_step) that applies the actions, renders the frames and writes reward
and done; the env's state is one 16-byte record per env that lives on the device next to the step counter, both as
pairs read / written alternately.  Like Catch's step it writes caller-owned static buffers with a fixed launch, so it
rides in the captured rollout graph (acting/fast_step.py) — with the actions read from a static buffer bound once
(`bind_actions`).  There is no CPU implementation.

`rgb=True` (the reference's ple_flappy_bird_iqn_lstm.json trains on RGB frames): frame_shape is (3, H, W) and the
observation is ONE step's frame — the current state's, history depth 1, the reset frame drawn like any other — in red,
green and blue planes with a fixed palette (PALETTE below; the bird still wins over a pipe).  The same kernel body
renders it (mirl_flappy_env_step_rgb); dynamics, record, Philox keying, rewards and dones are exactly those of the
intensity env, and the planes are NOT a history stack (`frame_stack` is False: frame_stack_dedup storage is refused)."""
import numpy as np
import torch

from rltime_amd._lib import lib, check, ptr, stream
from rltime_amd.spaces import Box, Discrete


# rgb=True: (red, green, blue) of a background, pipe and bird pixel
PALETTE = {"background": (78, 192, 202), "pipe": (84, 168, 40), "bird": (250, 200, 30)}


def check_geometry(frame_shape, cell, gap, spacing, n_actions, max_episode_steps, rgb=False):
    """-> (P, H, W, R, C) or a ValueError that names the rule broken (nothing is allocated before this passes)."""
    if len(tuple(frame_shape)) != 3:
        raise ValueError("flappy: frame_shape is (P, H, W)")
    P, H, W = (int(v) for v in frame_shape)
    s = int(cell)
    if s < 1:
        raise ValueError("flappy: cell >= 1")
    if not 1 <= P <= 4:
        raise ValueError("flappy: 1 <= P <= 4 history planes (frame_shape[0] = %d)" % P)
    if rgb and P != 3:
        raise ValueError("flappy: rgb frames are (3, H, W), one frame in three colour planes (frame_shape[0] = %d)" % P)
    if H < 1 or W < 1 or H % s or W % s:
        raise ValueError("flappy: H %% cell == 0 and W %% cell == 0 (H = %d, W = %d, cell = %d)" % (H, W, s))
    if W % 4 or (H * W) % 16:
        raise ValueError("flappy: W %% 4 == 0 and H * W %% 16 == 0, the input layer's own gates (H = %d, W = %d)" % (H, W))
    R, C = H // s, W // s
    if not 4 <= R <= 255:
        raise ValueError("flappy: 4 <= R = H / cell <= 255 rows (R = %d)" % R)
    if not 3 <= C <= 255:
        raise ValueError("flappy: 3 <= C = W / cell <= 255 columns (C = %d)" % C)
    if not 1 <= int(gap) < R:
        raise ValueError("flappy: 1 <= gap < R (gap = %d, R = %d)" % (int(gap), R))
    if int(spacing) < 2:
        raise ValueError("flappy: spacing >= 2 (spacing = %d)" % int(spacing))
    if int(n_actions) < 2:
        raise ValueError("flappy: n_actions >= 2 (n_actions = %d)" % int(n_actions))
    if not 1 <= int(max_episode_steps) < 2 ** 31:
        raise ValueError("flappy: max_episode_steps >= 1 (max_episode_steps = %d)" % int(max_episode_steps))
    return P, H, W, R, C


class FlappyVecEnv:
    def __init__(self, num_envs, frame_shape=(4, 48, 32), cell=4, gap=3, spacing=4, n_actions=2, max_episode_steps=54000,
                 death_reward=-1.0, device="cuda", seed=0, rgb=False):
        P, H, W, R, C = check_geometry(frame_shape, cell, gap, spacing, n_actions, max_episode_steps, rgb)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("FlappyVecEnv steps on the GPU only (csrc/acting.hip k_flappy_env_step): there is no CPU implementation")
        self.num_envs = int(num_envs)
        self.rgb = bool(rgb)
        if self.rgb:
            # what the fast acting step's trusted_stack reads (frame_stack_dedup storage): colour planes are no history
            self.frame_stack = False
        self._step, self._step_pre = (("mirl_flappy_env_step_rgb", "mirl_flappy_env_step_pre_rgb") if self.rgb else
                                      ("mirl_flappy_env_step", "mirl_flappy_env_step_pre"))
        self.observation_space = Box(0, 255, (P, H, W), np.uint8)
        self.action_space = Discrete(int(n_actions))
        self.rows, self.columns, self.gap, self.spacing = R, C, int(gap), int(spacing)
        self.max_episode_steps, self.death_reward = int(max_episode_steps), float(death_reward)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._dims = (self.num_envs, P, H, W, int(cell), self.gap, self.spacing, int(n_actions), self.max_episode_steps,
                      self.death_reward)
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
        """Every env restarts the episode its record numbers (0 for a new env); neither that number nor the step counter
        is advanced."""
        obs, rewards, dones = self._fresh()
        check(getattr(lib, self._step)(*self._args(obs, rewards, dones, reset_all=1), stream()), self._step)
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
            raise RuntimeError("FlappyVecEnv: reset() before the first step")
        if self._actions is None and self._own_actions is None:
            raise RuntimeError("FlappyVecEnv.step_into reads the bound action buffer: bind_actions() first (or use step_device)")

    def step_into(self, obs_out, rewards_out, dones_out):
        """obs_out uint8 [E, P, H, W], rewards_out float32 [E], dones_out uint8 [E] <- one step on the bound actions."""
        self._need_actions()
        check(getattr(lib, self._step)(*self._args(obs_out, rewards_out, dones_out), stream()), self._step)
        self._slot ^= 1

    def step_pre(self, obs_out, rewards_out, dones_out, pre_args):
        """The env step and the actor's pre-step as ONE launch; pre_args: mirl_actor_pre's arguments from H on."""
        self._need_actions()
        check(getattr(lib, self._step_pre)(*self._args(obs_out, rewards_out, dones_out), *pre_args), self._step_pre)
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
