"""NumPy restatement of the Flappy vector env (rltime_amd/acting/flappy_env.py, csrc/acting.hip k_flappy_env_step), written
from the game's definition, one env and one grid cell at a time, in integers.  Proved on hand-worked cases by
tests/test_flappy_restate_cpu.py; the kernel is held to it bit for bit by tests/test_flappy_env_gpu.py.

The game: an R x C grid of s x s pixel cells (R = H / s rows, row 0 on top; C = W / s columns) on P history planes of
H x W uint8, plane P - 1 newest.  The bird lives in column B = 1.
  state per env    rows[0..3] (the bird's row now and at the three previous steps), v in [-2, 2], tau (steps since the
                   episode began), n (the env's episode number, counted from 0, never reset)
  episode start    tau = 0, rows[*] = R // 2, v = 0; n is whatever the record says (reset) or n + 1 (after a done)
  one step on a    v = -2 if a == 1 else min(v + 1, 2);  y = rows[0] + v, and y < 0 -> y = 0, v = 0;  tau += 1;
                   pipe j = 0, 1, .. stands in column C + j D - tau and is AT THE BIRD when that equals B;
                   dead = y > R - 1 or (a pipe j at the bird and not top_j <= y < top_j + g);
                   passed = a pipe at the bird and not dead;
                   reward = death_reward if dead else 1 if passed else 0;  done = dead or tau == max_episode_steps;
                   done: n += 1 and a new episode starts in the same step (its reset frame is what the step returns)
  gaps             top_j = (word 0 of philox_4x32(seed ^ 0xF1A9, call = n << 32 | j, lane = env) * (R - g + 1)) >> 32: the
                   Philox key is the two halves of seed ^ 0xF1A9, the counter (env, j, n, tag) — a function of
                   (seed, env, n, j) and nothing else
  observation      plane P - 1 - k: zeros if k > tau (before the episode), else the bird cell (255) at (rows[k], B) and, for
                   every pipe j with column c = C + j D - (tau - k) in [0, C - 1], the cells of column c outside
                   [top_j, top_j + g) (128).  A live bird in a pipe's column is inside its gap, so the two never coincide;
                   the bird is drawn last and would win.

The bound for a blind policy (tests/test_flappy_learns_gpu.py rests on it).  top_j is uniform on the R - g + 1 values
0 .. R - g and independent of everything drawn before it (its own Philox block).  A pipeline that passes no information
from the frames to the actions reaches pipe j at a row y that is a function of its actions and of earlier pipes' gaps (by
surviving them) only, hence independent of top_j.  It passes with probability #{tops : top <= y < top + g} / (R - g + 1);
the tops that contain y are max(0, y - g + 1) .. min(y, R - g), at most g of them, so the probability is at most
p = g / (R - g + 1) whatever happened before.  The number of pipes passed per episode is therefore stochastically below a
Geometric variable with P(N >= k) = p^k: mean p / (1 - p), variance p / (1 - p)^2.  With death_reward = 0 an episode's
reward IS its number of pipes passed (the time limit only cuts it short), so over a window of N episodes the blind mean
exceeds blind_bar(R, g, N) = p / (1 - p) + 6 sqrt(p / (1 - p)^2 / N) with negligible probability: 0.577 for R = 12, g = 3,
N = 1000."""
import math

import numpy as np

from tests.pointwise_restate import philox_4x32

DRAW_KEY = 0xF1A9
BIRD_COLUMN = 1
BIRD, PIPE = 255, 128


def gap_top(seed, e, n, j, R, g):
    return (philox_4x32(seed ^ DRAW_KEY, ((int(n) & 0xFFFFFFFF) << 32) | int(j), e)[0] * (R - g + 1)) >> 32


def blind_bar(R, g, N):
    p = g / (R - g + 1.0)
    return p / (1.0 - p) + 6.0 * math.sqrt(p / (1.0 - p) ** 2 / N)


def pipes_on_screen(tau, C, D):
    """-> [(j, column)] of the pipes standing in columns 0 .. C - 1 at episode time tau."""
    out, j = [], 0
    while C + j * D - tau <= C - 1:
        if C + j * D - tau >= 0:
            out.append((j, C + j * D - tau))
        j += 1
    return out


def _start(state, e, R):
    state["rows"][e, :] = R // 2
    state["v"][e] = 0
    state["tau"][e] = 0


def render(state, seed, P, H, W, s, g, D):
    """-> frames (E, P, H, W) uint8 of `state`."""
    E, R, C = len(state["v"]), H // s, W // s
    frames = np.zeros((E, P, H, W), dtype=np.uint8)
    for e in range(E):
        tau, n = int(state["tau"][e]), int(state["n"][e])
        for k in range(P):
            if k > tau:
                continue                                              # the plane predates the episode
            plane = frames[e, P - 1 - k]
            for j, col in pipes_on_screen(tau - k, C, D):
                top = gap_top(seed, e, n, j, R, g)
                plane[:top * s, col * s:(col + 1) * s] = PIPE
                plane[(top + g) * s:, col * s:(col + 1) * s] = PIPE
            y = int(state["rows"][e, k])
            plane[y * s:(y + 1) * s, BIRD_COLUMN * s:(BIRD_COLUMN + 1) * s] = BIRD
    return frames


def flappy_reset(seed, E, P, H, W, s, g, D, n=None):
    """Every env restarts episode n[e] (default 0).  -> (state, frames, rewards (float32, 0), dones (uint8, 1))."""
    state = {"rows": np.zeros((E, 4), np.int64), "v": np.zeros(E, np.int64), "tau": np.zeros(E, np.int64),
             "n": np.zeros(E, np.int64) if n is None else np.asarray(n, np.int64).copy()}
    for e in range(E):
        _start(state, e, H // s)
    return state, render(state, seed, P, H, W, s, g, D), np.zeros(E, np.float32), np.ones(E, np.uint8)


def flappy_step(state, actions, seed, P, H, W, s, g, D, max_steps, death_reward):
    """One step on `actions`.  -> (new state, frames, rewards, dones); `state` is left unchanged."""
    E, R, C = len(state["v"]), H // s, W // s
    new = {k: v.copy() for k, v in state.items()}
    rewards, dones = np.zeros(E, np.float32), np.zeros(E, np.uint8)
    for e in range(E):
        v = -2 if int(actions[e]) == 1 else min(int(state["v"][e]) + 1, 2)
        y = int(state["rows"][e, 0]) + v
        if y < 0:
            y, v = 0, 0
        tau = int(state["tau"][e]) + 1
        at = [j for j, col in pipes_on_screen(tau, C, D) if col == BIRD_COLUMN]
        dead = y > R - 1
        for j in at:
            top = gap_top(seed, e, int(state["n"][e]), j, R, g)
            dead = dead or not (top <= y < top + g)
        passed = bool(at) and not dead
        rewards[e] = np.float32(death_reward) if dead else (1.0 if passed else 0.0)
        new["rows"][e, 1:] = state["rows"][e, :3]
        new["rows"][e, 0], new["v"][e], new["tau"][e] = y, v, tau
        if dead or tau == max_steps:
            dones[e] = 1
            new["n"][e] = (int(state["n"][e]) + 1) & 0xFFFFFFFF
            _start(new, e, R)
    return new, render(new, seed, P, H, W, s, g, D), rewards, dones


def records(state):
    """The 16-byte device record per env: uint32 {rows now | 1 | 2 | 3 steps ago as bytes 0..3, v + 2, tau, n}."""
    E = len(state["v"])
    out = np.zeros((E, 4), dtype=np.uint32)
    rows = state["rows"].astype(np.uint32)
    out[:, 0] = rows[:, 0] | (rows[:, 1] << 8) | (rows[:, 2] << 16) | (rows[:, 3] << 24)
    out[:, 1], out[:, 2], out[:, 3] = state["v"] + 2, state["tau"], state["n"]
    return out


def from_records(rec):
    rec = np.asarray(rec).astype(np.int64) & 0xFFFFFFFF
    return {"rows": np.stack([(rec[:, 0] >> (8 * k)) & 0xFF for k in range(4)], axis=1), "v": rec[:, 1] - 2,
            "tau": rec[:, 2].copy(), "n": rec[:, 3].copy()}


def branches(state, actions, seed, H, W, s, g, D, max_steps):
    """Which of the rules' branches the step from `state` on `actions` takes, as one set of names per env (what a test of
    the kernel asserts its scripts have reached): ceiling, floor, above, below, pass, limit, pass+limit, plain."""
    R, C = H // s, W // s
    out = []
    for e in range(len(state["v"])):
        v = -2 if int(actions[e]) == 1 else min(int(state["v"][e]) + 1, 2)
        y = int(state["rows"][e, 0]) + v
        tau = int(state["tau"][e]) + 1
        names = set()
        if y < 0:
            names.add("ceiling")
            y = 0
        at = (tau + BIRD_COLUMN - C) >= 0 and (tau + BIRD_COLUMN - C) % D == 0
        top = gap_top(seed, e, int(state["n"][e]), (tau + BIRD_COLUMN - C) // D, R, g) if at else None
        if y > R - 1:
            names.add("floor")
        elif at and y < top:
            names.add("above")
        elif at and y >= top + g:
            names.add("below")
        elif at:
            names.add("pass+limit" if tau == max_steps else "pass")
        elif tau == max_steps:
            names.add("limit")
        else:
            names.add("plain")
        out.append(names)
    return out


def scripted_action(script, state, seed, H, W, s, g, D):
    """The scripts of tests/test_flappy_env_gpu.py: `seek` steers for the next gap, `flap` always flaps (ceiling, pipes hit
    above the gap), `fall` never does (floor), `low` flaps only to stay off the floor (pipes hit below the gap)."""
    if script == "seek":
        return seeking_action(state, seed, H, W, s, g, D)
    if script == "flap":
        return np.ones(len(state["v"]), np.int32)
    if script == "fall":
        return np.zeros(len(state["v"]), np.int32)
    assert script == "low"
    R = H // s
    fall = state["rows"][:, 0] + np.minimum(state["v"] + 1, 2)
    return (fall > R - 1).astype(np.int32)


def seeking_action(state, seed, H, W, s, g, D):
    """A sighted policy: the first action of an action sequence (enumerated, at most 8 steps deep) that keeps the bird off
    the floor and ends nearest the middle of the next pipe's gap when that pipe reaches the bird.  It passes most pipes (not
    every one: gaps D columns apart can be further apart in rows than the bird can travel)."""
    E, R, C = len(state["v"]), H // s, W // s
    out = np.zeros(E, np.int32)
    for e in range(E):
        tau = int(state["tau"][e])
        j = max(0, -(-(tau + 1 + BIRD_COLUMN - C) // D))              # the first pipe at or right of the bird after this step
        steps = C - BIRD_COLUMN + j * D - tau                         # .. which reaches the bird after this many steps
        target = gap_top(seed, e, int(state["n"][e]), j, R, g) + g // 2
        best = None
        for code in range(1 << min(steps, 8)):
            y, v = int(state["rows"][e, 0]), int(state["v"][e])
            for k in range(min(steps, 8)):
                v = -2 if (code >> k) & 1 else min(v + 1, 2)
                y += v
                if y < 0:
                    y, v = 0, 0
                if y > R - 1:
                    break
            else:
                score = (abs(y - target), abs(v), code)
                if best is None or score < best:
                    best = score
        out[e] = best[2] & 1 if best is not None else 1
    return out
