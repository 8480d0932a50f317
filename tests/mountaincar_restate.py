"""NumPy restatement of the device MountainCarContinuous (rltime_amd/acting/mountaincar_device_env.py, csrc/acting.hip
k_mountaincar_env_step), written from the entry point's statement in include/mirl.h.  Proved against MountainCarVecEnv and
math.cos by tests/test_mountaincar_restate_cpu.py; the kernel is held to it bit for bit by tests/test_mountaincar_env_gpu.py.

  state per env    p, v float64 (position, velocity), episodes_started, t
  episode start    word w_0 of philox_4x32(seed ^ 0xC0A7CA2E, episodes_started, env):
                   p = (float64(w_0) + 0.5) * 2^-32 * 0.2 - 0.6, v = 0; episodes_started += 1; t = 0
  one step         a = float64(float32 action);  f = a < -1 ? -1 : (a > 1 ? 1 : a)
                   v = v + (f * 0.0015 - 0.0025 * C(3.0 * p));  v = min(v, 0.07) then max(v, -0.07)
                   p = p + v;  p = min(p, 0.6) then max(p, -1.2);  p == -1.2 and v < 0: v = 0
                   goal = p >= 0.45 and v >= 0;  t += 1;  reward = float32((100 | 0) - (a * a) * 0.1)
                   done = goal or t >= limit; a finished env starts its next episode in the same step
  observation      (p, v) rounded to float32

C(x) is the Taylor polynomial of cos in z = x * x through x^34, Horner from the highest coefficient down to the constant 1.
Every operation is an IEEE float64 +, -, * on NumPy arrays — nothing fused — which is what the kernel executes (the library
builds with -ffp-contract=off).

The bound on C.  x = 3.0 * p lies in [-3.6, 1.8]; for |x| <= 3.6, with u = 2^-53 and c_k = 1 / (2k)!:
  truncation       the first dropped term over (1 - ratio of the next): 3.6^36 / 36! / (1 - 3.6^2 / (37 * 38))      < 3e-22
  Horner rounding  17 multiply-adds = 34 roundings, one more for the rounded coefficients: the computed value is the exact
                   value of a polynomial whose coefficients are off by at most gamma_35 = 35 u / (1 - 35 u) relatively
                   (Higham, Accuracy and Stability of Numerical Algorithms, section 5.1), so the error is at most
                   gamma_35 * sum_k c_k |x|^2k <= gamma_35 * cosh(3.6)                                              < 7.12e-14
  z = fl(x * x)    a relative u in z moves the polynomial by at most |z p'(z)| u <= |x| sinh|x| / 2 * u                < 3.7e-15
  libm             math.cos is within one ulp of the exact cosine: 2^-53 * 2                                        < 2.3e-16
COS_BOUND is their sum rounded up.  It is an a-priori bound — Horner's worst case over 35 roundings — and pessimistic: the
worst difference on a grid of 2 * 10^6 points is 1.6e-15."""
import math

import numpy as np

from tests.catch_restate import philox_4x32

DRAW_KEY = 0xC0A7CA2E
MIN_POSITION, MAX_POSITION, MAX_SPEED = -1.2, 0.6, 0.07
GOAL_POSITION = 0.45
POWER, GRAVITY_TERM = 0.0015, 0.0025
# -1/2!, +1/4!, ..., -1/34!: the correctly rounded quotients, as the kernel's literals
COS_COEFFS = [(-1.0) ** (k // 2) / math.factorial(k) for k in range(2, 35, 2)]
KERNEL_COS_LITERALS = [-0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07,
                       2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14, -1.5619206968586225e-16,
                       4.110317623312165e-19, -8.896791392450574e-22, 1.6117375710961184e-24, -2.4795962632247972e-27,
                       3.279889237069838e-30, -3.7699876288159054e-33, 3.800390754854744e-36, -3.387157535521162e-39]
X_MAX = 3.6
_U = 2.0 ** -53
COS_BOUND_TERMS = {
    "truncation": X_MAX ** 36 / math.factorial(36) / (1.0 - X_MAX ** 2 / (37 * 38)),
    "horner": 35 * _U / (1 - 35 * _U) * math.cosh(X_MAX),
    "square": X_MAX * math.sinh(X_MAX) / 2 * _U,
    "libm": 2 * _U,
}
COS_BOUND = 7.6e-14
assert sum(COS_BOUND_TERMS.values()) < COS_BOUND < 1.02 * sum(COS_BOUND_TERMS.values())


def poly_cos(x):
    x = np.asarray(x, dtype=np.float64)
    z = x * x
    p = np.full_like(z, COS_COEFFS[-1])
    for c in COS_COEFFS[-2::-1]:
        p = p * z + c
    return p * z + 1.0


def start_position(seed, episode, env):
    w = philox_4x32(seed ^ DRAW_KEY, int(episode), int(env))
    return (np.float64(w[0]) + 0.5) * 2.0 ** -32 * 0.2 - 0.6


def physics(p, v, actions, cos=poly_cos):
    """(E,) float64 positions and velocities, (E,) float32 raw actions -> (p, v, goal, reward float64); `cos` is replaceable
    for the comparison with MountainCarVecEnv."""
    p, v = np.asarray(p, dtype=np.float64), np.asarray(v, dtype=np.float64)
    a = np.asarray(actions, dtype=np.float32).reshape(-1).astype(np.float64)
    f = np.where(a < -1.0, -1.0, np.where(a > 1.0, 1.0, a))
    v = v + (f * POWER - GRAVITY_TERM * cos(3.0 * p))
    v = np.where(v > MAX_SPEED, MAX_SPEED, v)
    v = np.where(v < -MAX_SPEED, -MAX_SPEED, v)
    p = p + v
    p = np.where(p > MAX_POSITION, MAX_POSITION, p)
    p = np.where(p < MIN_POSITION, MIN_POSITION, p)
    v = np.where((p == MIN_POSITION) & (v < 0.0), 0.0, v)
    goal = (p >= GOAL_POSITION) & (v >= 0.0)
    reward = np.where(goal, 100.0, 0.0) - (a * a) * 0.1
    return p, v, goal, reward


def branches(p, v, actions):
    """Which branch of the step each env takes from (p, v) under `actions`: a dict of (E,) bool arrays.  The tests assert
    that their pinned trajectories reach every one."""
    p, v = np.asarray(p, dtype=np.float64), np.asarray(v, dtype=np.float64)
    a = np.asarray(actions, dtype=np.float32).reshape(-1).astype(np.float64)
    f = np.where(a < -1.0, -1.0, np.where(a > 1.0, 1.0, a))
    v1 = v + (f * POWER - GRAVITY_TERM * poly_cos(3.0 * p))
    v2 = np.clip(v1, -MAX_SPEED, MAX_SPEED)
    p1 = p + v2
    p2, v3, goal, _ = physics(p, v, actions)
    return {"action_low": a < -1.0, "action_high": a > 1.0, "action_inside": (a >= -1.0) & (a <= 1.0),
            "speed_high": v1 > MAX_SPEED, "speed_low": v1 < -MAX_SPEED,
            "wall_left": (p1 <= MIN_POSITION) & (v2 < 0.0) & (v3 == 0.0), "wall_right": p1 > MAX_POSITION, "goal": goal}


def _start(state, e, seed):
    state["p"][e] = start_position(seed, state["episodes_started"][e], e)
    state["v"][e] = 0.0
    state["episodes_started"][e] += 1
    state["t"][e] = 0


def new_state(E):
    """What a fresh env's zeroed records hold."""
    return {"p": np.zeros(E, np.float64), "v": np.zeros(E, np.float64), "episodes_started": np.zeros(E, np.int64),
            "t": np.zeros(E, np.int32)}


def _obs(state):
    return np.stack([state["p"], state["v"]], axis=1).astype(np.float32)


def mountaincar_reset(state, seed):
    """reset_all: every env starts its next episode.  -> (new state, obs float32 (E, 2), rewards (0), dones (1))."""
    new = {k: v.copy() for k, v in state.items()}
    E = len(new["t"])
    for e in range(E):
        _start(new, e, seed)
    return new, _obs(new), np.zeros(E, np.float32), np.ones(E, np.uint8)


def mountaincar_step(state, actions, seed, max_episode_steps):
    """-> (new state, obs float32 (E, 2), rewards float32, dones uint8); `state` is left unchanged."""
    new = {k: v.copy() for k, v in state.items()}
    new["p"], new["v"], goal, reward = physics(state["p"], state["v"], actions)
    new["t"] += 1
    dones = (goal | (new["t"] >= max_episode_steps)).astype(np.uint8)
    for e in np.nonzero(dones)[0]:
        _start(new, e, seed)
    return new, _obs(new), reward.astype(np.float32), dones


def records(state):
    """The 32-byte device record per env as four int64 words: the bit patterns of p and v, episodes_started, t (pad 0)."""
    E = len(state["t"])
    out = np.zeros((E, 4), dtype=np.int64)
    out[:, 0] = state["p"].view(np.int64)
    out[:, 1] = state["v"].view(np.int64)
    out[:, 2] = state["episodes_started"]
    out[:, 3] = state["t"].astype(np.int64) & 0xFFFFFFFF
    return out


def from_records(rec):
    rec = np.ascontiguousarray(np.asarray(rec, dtype=np.int64))
    return {"p": rec[:, 0].copy().view(np.float64), "v": rec[:, 1].copy().view(np.float64), "episodes_started": rec[:, 2].copy(),
            "t": (rec[:, 3] & 0xFFFFFFFF).astype(np.int32)}


def place(state, env, p, v):
    """`state` with env `env` put at (p, v), its counters kept — what set_state does for the tests' placements."""
    new = {k: x.copy() for k, x in state.items()}
    new["p"][env], new["v"][env] = p, v
    return new


def action_stream(seed, steps, E):
    """The tests' fixed action stream, float32 (steps, E): normal draws of scale 1.5 (about half of them outside [-1, 1],
    on both sides), with every seventh step an exact bound or zero so that a == -1, a == 1 and a == 0 occur."""
    g = np.random.default_rng(seed)
    a = (g.standard_normal((steps, E)) * 1.5).astype(np.float32)
    a[::7] = g.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=a[::7].shape)
    return a


# the placements both the CPU and the GPU test use: (p, v) from which one step takes the named branch WHATEVER the action
# (the force moves v by at most 0.0015)
PLACEMENTS = {
    "wall_left": (-1.19, -0.07),       # v' in [-0.0692, -0.0662]: p + v' < -1.2, clipped to the wall, the velocity zeroed
    "goal": (0.44, 0.06),              # v' in [0.0579, 0.0609]: p + v' >= 0.45 with v' > 0: +100, done
    "speed_high": (-0.9, 0.0699),      # -0.0025 cos(-2.7) = +0.00226: v' >= 0.07066, clipped to +0.07
    "speed_low": (0.0, -0.0699),       # -0.0025 cos(0) = -0.0025: v' <= -0.0709, clipped to -0.07
    "wall_right": (0.59, 0.07),        # v' clipped to 0.07: p + v' > 0.6, clipped (and the goal)
}


def placement_schedule(E):
    """step number -> (placement name, env): spread over the rollout and over the envs (all on env 0 when E == 1)."""
    return {10: ("wall_left", 0), 25: ("goal", E // 2), 50: ("speed_high", E - 1), 75: ("speed_low", 0), 100: ("wall_right", E // 2)}


def pinned_rollout(E, seed, limit, steps=150):
    """The pinned trajectory of both tests: reset, then `steps` steps on action_stream(seed, steps, E) with the placements
    of placement_schedule applied before their step.  -> (state after the reset with its obs, a list of per-step dicts
    {placed: the state written before the step or None, actions, state, obs, rewards, dones: after the step}, reached:
    branch name -> how many env-steps took it, plus "time_limit")."""
    state, obs0, _, _ = mountaincar_reset(new_state(E), seed)
    first = (state, obs0)
    acts = action_stream(seed, steps, E)
    schedule = placement_schedule(E)
    reached = {"time_limit": 0}
    out = []
    for n in range(steps):
        placed = None
        if n in schedule:
            name, env = schedule[n]
            state = placed = place(state, env, *PLACEMENTS[name])
        for k, hit in branches(state["p"], state["v"], acts[n]).items():
            reached[k] = reached.get(k, 0) + int(hit.sum())
        t_before = state["t"].copy()
        goal = branches(state["p"], state["v"], acts[n])["goal"]
        state, obs, r, d = mountaincar_step(state, acts[n], seed, limit)
        reached["time_limit"] += int(((t_before + 1 >= limit) & ~goal & (d == 1)).sum())
        out.append({"placed": placed, "actions": acts[n], "state": state, "obs": obs, "rewards": r, "dones": d})
    return first, out, reached
