"""NumPy restatement of the device CartPole (rltime_amd/acting/cartpole_device_env.py, csrc/acting.hip k_cartpole_env_step),
written from the entry point's statement in include/mirl.h.  Proved against CartPoleVecEnv and np.sin / np.cos by
tests/test_cartpole_device_restate_cpu.py; the kernel is held to it bit for bit by tests/test_cartpole_env_gpu.py.

  state per env    x[4] float64 (cart position, cart velocity, pole angle, pole angular velocity), episodes_started, t
  episode start    words w_0..w_3 of philox_4x32(seed ^ 0xCA27901E, episodes_started, env):
                   x[k] = (float64(w_k) + 0.5) * 2^-32 * 0.1 - 0.05; episodes_started += 1; t = 0
  one step         the physics of CartPoleVecEnv.step in float64, in its operation order, with sin / cos the Taylor
                   polynomials below (Horner in theta^2, from the highest coefficient down to the constant 1); any action
                   other than 1 pushes left; t += 1; reward 1; done = |x| > 2.4 or |theta| > 24 pi / 360 or t >= limit;
                   a finished env starts its next episode in the same step
  observation      the float64 state rounded to float32

Every operation is an IEEE float64 +, -, *, / on NumPy arrays — nothing fused — which is what the kernel executes
(the library builds with -ffp-contract=off)."""
import math

import numpy as np

from tests.catch_restate import philox_4x32

DRAW_KEY = 0xCA27901E
GRAVITY, CART_MASS, POLE_MASS, POLE_HALF_LENGTH, PUSH, DT = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
ANGLE_LIMIT, POSITION_LIMIT = 24.0 * math.pi / 360.0, 2.4
# -1/3!, +1/5!, ..., +1/17!  and  -1/2!, +1/4!, ..., +1/16!: the correctly rounded quotients, as the kernel's literals
SIN_COEFFS = [(-1.0) ** ((k - 1) // 2) / math.factorial(k) for k in range(3, 18, 2)]
COS_COEFFS = [(-1.0) ** (k // 2) / math.factorial(k) for k in range(2, 17, 2)]
KERNEL_SIN_LITERALS = [-0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06,
                       -2.505210838544172e-08, 1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15]
KERNEL_COS_LITERALS = [-0.5, 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07,
                       2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14]


def _horner(z, coeffs):
    p = np.full_like(z, coeffs[-1])
    for c in coeffs[-2::-1]:
        p = p * z + c
    return p * z + 1.0


def poly_sin(theta):
    theta = np.asarray(theta, dtype=np.float64)
    return theta * _horner(theta * theta, SIN_COEFFS)


def poly_cos(theta):
    theta = np.asarray(theta, dtype=np.float64)
    return _horner(theta * theta, COS_COEFFS)


def start_state(seed, episode, env):
    w = philox_4x32(seed ^ DRAW_KEY, int(episode), int(env))
    return (np.array(w, dtype=np.float64) + 0.5) * 2.0 ** -32 * 0.1 - 0.05


def physics(x4, actions, sin=poly_sin, cos=poly_cos):
    """(E, 4) float64 states, (E,) actions -> the next (E, 4) states; `sin` / `cos` are replaceable for the comparison with
    CartPoleVecEnv."""
    x, v, th, w = np.asarray(x4, dtype=np.float64).T
    force = np.where(np.asarray(actions) == 1, PUSH, -PUSH)
    total = CART_MASS + POLE_MASS
    ml = POLE_MASS * POLE_HALF_LENGTH
    sn, cs = sin(th), cos(th)
    tmp = (force + ml * w * w * sn) / total
    th_acc = (GRAVITY * sn - cs * tmp) / (POLE_HALF_LENGTH * (4.0 / 3.0 - POLE_MASS * cs * cs / total))
    x_acc = tmp - ml * th_acc * cs / total
    return np.stack([x + DT * v, v + DT * x_acc, th + DT * w, w + DT * th_acc], axis=1)


def _start(state, e, seed):
    state["x"][e] = start_state(seed, state["episodes_started"][e], e)
    state["episodes_started"][e] += 1
    state["t"][e] = 0


def new_state(E):
    """What a fresh env's zeroed records hold."""
    return {"x": np.zeros((E, 4), np.float64), "episodes_started": np.zeros(E, np.int64), "t": np.zeros(E, np.int32)}


def cartpole_reset(state, seed):
    """reset_all: every env starts its next episode.  -> (new state, obs float32, rewards (0), dones (1))."""
    new = {k: v.copy() for k, v in state.items()}
    E = len(new["t"])
    for e in range(E):
        _start(new, e, seed)
    return new, new["x"].astype(np.float32), np.zeros(E, np.float32), np.ones(E, np.uint8)


def cartpole_step(state, actions, seed, max_episode_steps):
    """-> (new state, obs float32 (E, 4), rewards float32, dones uint8); `state` is left unchanged."""
    new = {k: v.copy() for k, v in state.items()}
    E = len(new["t"])
    new["x"] = physics(state["x"], actions)
    new["t"] += 1
    fell = (np.abs(new["x"][:, 0]) > POSITION_LIMIT) | (np.abs(new["x"][:, 2]) > ANGLE_LIMIT)
    dones = (fell | (new["t"] >= max_episode_steps)).astype(np.uint8)
    for e in np.nonzero(dones)[0]:
        _start(new, e, seed)
    return new, new["x"].astype(np.float32), np.ones(E, np.float32), dones


def records(state):
    """The 48-byte device record per env as six int64 words: the bit patterns of x[0..3], episodes_started, t (pad 0)."""
    E = len(state["t"])
    out = np.zeros((E, 6), dtype=np.int64)
    out[:, :4] = state["x"].view(np.int64)
    out[:, 4] = state["episodes_started"]
    out[:, 5] = state["t"].astype(np.int64) & 0xFFFFFFFF
    return out


def from_records(rec):
    rec = np.ascontiguousarray(np.asarray(rec, dtype=np.int64))
    return {"x": rec[:, :4].copy().view(np.float64), "episodes_started": rec[:, 4].copy(), "t": (rec[:, 5] & 0xFFFFFFFF).astype(np.int32)}


# ---- observation-blind policies: the yardstick of tests/test_cartpole_learns_gpu.py ------------------------------------------
def blind_words(max_period=6):
    """Every periodic binary action word of period <= max_period, as tuples, without repeats of the same infinite sequence
    start (a word that is a power of a shorter one is dropped); the two constants are the period-1 words."""
    out = []
    for n in range(1, max_period + 1):
        for code in range(2 ** n):
            w = tuple((code >> i) & 1 for i in range(n))
            if any(n % d == 0 and w == w[:d] * (n // d) for d in range(1, n)):
                continue
            out.append(w)
    return out


def blind_mean_lengths(episodes, max_episode_steps, seed, max_period=6):
    """Mean episode length over `episodes` episodes (one per env, envs 0 .. episodes - 1 of `seed`, each env's first episode)
    of every observation-blind policy: {"random": ..., word: ...}.  Vectorised over the episodes."""
    state, _, _, _ = cartpole_reset(new_state(episodes), seed)
    x0 = state["x"]

    def run(action_at):
        x = x0.copy()
        alive = np.ones(episodes, bool)
        length = np.zeros(episodes, np.int64)
        for t in range(max_episode_steps):
            x = np.where(alive[:, None], physics(x, action_at(t)), x)
            length += alive
            done = (np.abs(x[:, 0]) > POSITION_LIMIT) | (np.abs(x[:, 2]) > ANGLE_LIMIT)
            alive &= ~done
            if not alive.any():
                break
        return float(length.mean())

    g = np.random.default_rng(seed)
    table = {"random": run(lambda t: g.integers(0, 2, episodes))}
    for w in blind_words(max_period):
        table[w] = run(lambda t, w=w: np.full(episodes, w[t % len(w)]))
    return table
