"""NumPy restatement of the Catch vector env (rltime_amd/acting/catch_env.py, csrc/acting.hip k_catch_env_step), written from
the game's definition, one env and one pixel cell at a time.  Proved on hand-worked cases by tests/test_catch_restate_cpu.py;
the kernel is held to it bit for bit by tests/test_catch_env_gpu.py.

The game: a G x G grid of s x s pixel cells (s = S / G) on P history planes of S x S uint8, plane P - 1 newest.
  state per env    ball_col, ball_row (= steps since the episode began), paddle[0..3] (the paddle column now and at the three
                   previous steps)
  episode start    at step counter t: ball_col = (word 0 of philox_4x32(seed ^ 0xCA7C, t, env) * G) >> 32, ball_row = 0,
                   paddle[*] = G // 2
  one step         shift the paddle history; move the paddle by -1 (action 1) / +1 (action 2) / 0 (anything else), clamped to
                   [0, G - 1]; ball_row += 1; at ball_row == G - 1: reward +1 if ball_col == paddle[0] else -1, done, and a new
                   episode starts in the same step (keyed by this step's t); otherwise reward 0
  observation      plane P - 1 - k: zeros if ball_row - k < 0 (before the episode), else the ball cell (255) at cell row
                   ball_row - k, column ball_col — only if ball_row - k < V — and the paddle cell (128) at cell row G - 1,
                   column paddle[k]"""
import numpy as np

from tests.pointwise_restate import philox_4x32

DRAW_KEY = 0xCA7C


def draw_column(seed, t, e, G):
    return (philox_4x32(seed ^ DRAW_KEY, t, e)[0] * G) >> 32


def _start(state, e, seed, t, G):
    state["ball_col"][e] = draw_column(seed, t, e, G)
    state["ball_row"][e] = 0
    state["paddle"][e, :] = G // 2


def render(state, P, S, G, V):
    """-> frames (E, P, S, S) uint8 of `state`."""
    E, s = len(state["ball_col"]), S // G
    frames = np.zeros((E, P, S, S), dtype=np.uint8)
    for e in range(E):
        for k in range(P):
            row = int(state["ball_row"][e]) - k
            if row < 0:
                continue                                              # the plane predates the episode
            plane = frames[e, P - 1 - k]
            if row < V:
                col = int(state["ball_col"][e])
                plane[row * s:(row + 1) * s, col * s:(col + 1) * s] = 255
            pad = int(state["paddle"][e, k])
            plane[(G - 1) * s:G * s, pad * s:(pad + 1) * s] = 128
    return frames


def catch_reset(seed, t, E, P, S, G, V):
    """Every env starts an episode keyed by t.  -> (state, frames, rewards (float32, 0), dones (uint8, 1))."""
    state = {"ball_col": np.zeros(E, np.int64), "ball_row": np.zeros(E, np.int64), "paddle": np.zeros((E, 4), np.int64)}
    for e in range(E):
        _start(state, e, seed, t, G)
    return state, render(state, P, S, G, V), np.zeros(E, np.float32), np.ones(E, np.uint8)


def catch_step(state, actions, seed, t, P, S, G, V):
    """Step number t (= the counter before the step + 1) on `actions`.  -> (new state, frames, rewards, dones); `state` is
    left unchanged."""
    E = len(state["ball_col"])
    new = {k: v.copy() for k, v in state.items()}
    rewards, dones = np.zeros(E, np.float32), np.zeros(E, np.uint8)
    for e in range(E):
        a = int(actions[e])
        new["paddle"][e, 1:] = state["paddle"][e, :3]
        new["paddle"][e, 0] = min(max(int(state["paddle"][e, 0]) + {1: -1, 2: 1}.get(a, 0), 0), G - 1)
        new["ball_row"][e] += 1
        if new["ball_row"][e] == G - 1:
            rewards[e] = 1.0 if new["ball_col"][e] == new["paddle"][e, 0] else -1.0
            dones[e] = 1
            _start(new, e, seed, t, G)
    return new, render(new, P, S, G, V), rewards, dones


def records(state):
    """The 16-byte device record per env: uint32 {ball_col, ball_row, paddle now | 1 | 2 | 3 steps ago as bytes 0..3, 0}."""
    E = len(state["ball_col"])
    out = np.zeros((E, 4), dtype=np.uint32)
    out[:, 0], out[:, 1] = state["ball_col"], state["ball_row"]
    pad = state["paddle"].astype(np.uint32)
    out[:, 2] = pad[:, 0] | (pad[:, 1] << 8) | (pad[:, 2] << 16) | (pad[:, 3] << 24)
    return out


def from_records(rec):
    rec = np.asarray(rec).astype(np.int64) & 0xFFFFFFFF
    return {"ball_col": rec[:, 0].copy(), "ball_row": rec[:, 1].copy(),
            "paddle": np.stack([(rec[:, 2] >> (8 * k)) & 0xFF for k in range(4)], axis=1)}


def tracking_action(state):
    """The action that moves each paddle towards its ball: a policy that follows it from the start catches every ball (the
    paddle starts at most G / 2 columns away and has G - 1 steps)."""
    d = state["ball_col"] - state["paddle"][:, 0]
    return np.where(d < 0, 1, np.where(d > 0, 2, 0)).astype(np.int32)
