"""CPU: the NumPy restatement of the device CartPole (tests/cartpole_device_restate.py) against what it restates — np.sin /
np.cos, CartPoleVecEnv.step, the start-state range — and the observation-blind yardstick of the learning test."""
import math
import os
import re

import numpy as np

from rltime_amd.acting.cartpole_env import CartPoleVecEnv
from tests import cartpole_device_restate as CP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulps(got, want):
    return float(np.max(np.abs(got - want) / np.spacing(np.abs(want))))


def _kernel_literals(function):
    """The Horner coefficients of `function` in csrc/acting.hip, read from its source in the order the restatement keeps
    them (lowest power first): every `p = p * z + <literal>;` line but the last (the constant 1), and the initial value."""
    src = open(os.path.join(ROOT, "rltime_amd", "csrc", "acting.hip")).read()
    body = re.search(r"double %s\(double th\) \{(.*?)\n\}" % function, src, flags=re.S).group(1)
    first = re.search(r"double p = ([-+0-9.e]+);", body).group(1)
    rest = re.findall(r"p = p \* z \+ ([-+0-9.e]+);", body)
    assert len(rest) == 8 and float(rest[-1]) == 1.0, rest
    return [float(v) for v in ([first] + rest[:-1])[::-1]]


def test_coefficients_are_the_kernels_literals():
    """+-1/k! as correctly rounded float64 quotients == the literals in the kernel's SOURCE, value for value (a decimal
    literal of 16-17 significant digits names one float64)."""
    sin, cos = _kernel_literals("cartpole_sin"), _kernel_literals("cartpole_cos")
    assert sin == CP.SIN_COEFFS and cos == CP.COS_COEFFS
    assert sin == [(-1.0) ** ((k - 1) // 2) / math.factorial(k) for k in range(3, 18, 2)]
    assert cos == [(-1.0) ** (k // 2) / math.factorial(k) for k in range(2, 17, 2)]
    assert CP.SIN_COEFFS == CP.KERNEL_SIN_LITERALS and CP.COS_COEFFS == CP.KERNEL_COS_LITERALS


def test_polynomials_within_one_ulp_of_libm():
    g = np.random.default_rng(0)
    th = np.concatenate([g.uniform(-0.5, 0.5, 2_000_000), np.linspace(-0.5, 0.5, 100_001), [0.0, 0.5, -0.5, 0.2095, -0.2095]])
    assert _ulps(CP.poly_sin(th[th != 0.0]), np.sin(th[th != 0.0])) <= 1.0
    assert _ulps(CP.poly_cos(th), np.cos(th)) <= 1.0
    assert CP.poly_sin(0.0) == 0.0 and CP.poly_cos(0.0) == 1.0


def test_one_step_equals_the_cpu_env():
    """From the same float64 state, one restated step equals CartPoleVecEnv.step's float64 state (`env._x` after the step,
    on the envs it did not reset) to 1e-14 RELATIVE TO EACH VALUE ITSELF — |ours - env| <= 1e-14 |env|, component by
    component, no absolute floor — the only difference being sin / cos.  With np.sin / np.cos put in their place the
    restated step is the env's bit for bit, which proves the operation order."""
    E = 4096
    g = np.random.default_rng(1)
    x0 = np.stack([g.uniform(-2.4, 2.4, E), g.uniform(-3, 3, E), g.uniform(-0.2095, 0.2095, E), g.uniform(-3, 3, E)], axis=1)
    actions = g.integers(-1, 3, E)                                  # values outside {0, 1} push left in both
    env = CartPoleVecEnv(E, max_episode_steps=10 ** 6)
    env.reset()
    env._x = x0.copy()
    obs, rewards, dones, _ = env.step(actions)
    keep = ~dones                                                   # the env overwrote the others with their next start state
    assert keep.sum() > E // 2 and dones.any() and np.all(rewards == 1.0)
    env64 = env._x[keep]
    assert np.array_equal(obs[keep], env64.astype(np.float32))
    assert np.array_equal(CP.physics(x0, actions, sin=np.sin, cos=np.cos)[keep], env64)
    ours = CP.physics(x0, actions)[keep]
    assert np.all(env64 != 0.0) and np.all(np.abs(ours - env64) <= 1e-14 * np.abs(env64))
    assert not np.array_equal(ours, env64)                          # (the polynomials are not libm: some last bits differ)
    state = {"x": x0, "episodes_started": np.ones(E, np.int64), "t": np.zeros(E, np.int32)}
    new, o, r, d = CP.cartpole_step(state, actions, 5, 10 ** 6)
    assert np.array_equal(d.astype(bool), dones) and np.all(r == 1.0)
    assert np.array_equal(new["x"][keep], ours) and np.array_equal(o, new["x"].astype(np.float32))
    # a finished env returns its NEW episode's first observation, and only it moved on
    assert np.array_equal(new["episodes_started"], 1 + d) and np.all(new["t"][d == 1] == 0) and np.all(new["t"][d == 0] == 1)
    assert np.all(np.abs(o[d == 1]) <= 0.05)


def test_time_limit_ends_an_episode():
    state, obs, r, d = CP.cartpole_reset(CP.new_state(3), 9)
    assert not r.any() and d.all() and np.array_equal(obs, state["x"].astype(np.float32))
    for n in range(3):
        state, obs, r, d = CP.cartpole_step(state, np.array([n % 2, 1, 0]), 9, 3)
        assert d.tolist() == ([1, 1, 1] if n == 2 else [0, 0, 0])
    assert state["episodes_started"].tolist() == [2, 2, 2] and state["t"].tolist() == [0, 0, 0]
    assert np.array_equal(state["x"][1], CP.start_state(9, 1, 1))
    rec = CP.records(state)
    back = CP.from_records(rec)
    assert all(np.array_equal(back[k], state[k]) for k in state)


def test_start_draws_lie_in_the_start_box():
    draws = np.stack([CP.start_state(seed, ep, env) for seed in (0, 7, 2 ** 40 + 3) for ep in range(40) for env in range(40)])
    assert draws.min() >= -0.05 and draws.max() < 0.05
    assert abs(draws.mean()) < 2e-3 and draws.std() > 0.025        # uniform on the box: sd 0.1 / sqrt(12) = 0.0289
    w = np.array([0, 2 ** 32 - 1], dtype=np.float64)                  # the extreme words
    ends = (w + 0.5) * 2.0 ** -32 * 0.1 - 0.05
    assert -0.05 <= ends[0] and ends[1] < 0.05


def test_theta_at_the_start_of_a_step_stays_below_0_21():
    """10^5 random-action steps (50 envs x 2000 steps): the polynomials are only ever evaluated inside their proven range."""
    E = 50
    g = np.random.default_rng(3)
    state, _, _, _ = CP.cartpole_reset(CP.new_state(E), 11)
    worst, ends = 0.0, 0
    for _ in range(2000):
        worst = max(worst, float(np.abs(state["x"][:, 2]).max()))
        state, _, _, d = CP.cartpole_step(state, g.integers(0, 2, E), 11, 200)
        ends += int(d.sum())
    assert worst < 0.21 and ends > 1000


def test_blind_policy_table():
    """The yardstick of tests/test_cartpole_learns_gpu.py: the best mean episode length over 2000 episodes of any
    observation-blind policy — uniform random, the two constants, every periodic binary word of period <= 6 — is not above
    the constant that test's bar is three times of."""
    from tests.test_cartpole_learns_gpu import L_BLIND, EPISODE_CAP
    words = CP.blind_words(6)
    assert (0,) in words and (1,) in words and (0, 1) in words and (1, 0) in words and (0, 0) not in words and (0, 1, 0, 1) not in words
    assert len(words) == 2 + 2 + 6 + 12 + 30 + 54
    table = CP.blind_mean_lengths(2000, EPISODE_CAP, seed=0)
    best = max(table.values())
    print("blind policies: random %.2f, constants %.2f / %.2f, best %.2f (%s)"
          % (table["random"], table[(0,)], table[(1,)], best, max(table, key=table.get)))
    assert len(table) == 1 + len(words)
    assert L_BLIND >= best
    assert 3 * L_BLIND <= EPISODE_CAP / 2
