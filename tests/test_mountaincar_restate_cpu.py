"""CPU: the NumPy restatement of the device MountainCarContinuous (tests/mountaincar_restate.py) against what it restates —
math.cos, MountainCarVecEnv.step, the start-position range — and the condition that its pinned trajectory reaches every
branch of the step."""
import math
import os
import re

import numpy as np
import pytest

from rltime_amd.acting.mountaincar_env import MountainCarVecEnv
from tests import mountaincar_restate as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 40


def _kernel_literals():
    """The Horner coefficients of mountaincar_cos in csrc/acting.hip, read from its source in the order the restatement
    keeps them (lowest power first): every `p = p * z + <literal>;` line but the last (the constant 1), and the initial
    value."""
    src = open(os.path.join(ROOT, "rltime_amd", "csrc", "acting.hip")).read()
    body = re.search(r"double mountaincar_cos\(double x\) \{(.*?)\n\}", src, flags=re.S).group(1)
    first = re.search(r"double p = ([-+0-9.e]+);", body).group(1)
    rest = re.findall(r"p = p \* z \+ ([-+0-9.e]+);", body)
    assert len(rest) == 17 and float(rest[-1]) == 1.0, rest
    return [float(v) for v in ([first] + rest[:-1])[::-1]]


def test_coefficients_are_the_kernels_literals():
    """+-1/k! as correctly rounded float64 quotients == the literals in the kernel's SOURCE, value for value."""
    got = _kernel_literals()
    assert got == MC.COS_COEFFS == MC.KERNEL_COS_LITERALS
    assert got == [(-1.0) ** (k // 2) / math.factorial(k) for k in range(2, 35, 2)]


def test_cos_polynomial_holds_its_stated_bound_on_a_dense_grid():
    """|C(x) - math.cos(x)| <= COS_BOUND on 200 001 grid points of [-3.6, 1.8] plus the ends, 0 and 3 * every placement —
    and on the mirrored grid, since the bound is derived for |x| <= 3.6.  The bound is the sum of its four derived terms."""
    assert 7.4e-14 < sum(MC.COS_BOUND_TERMS.values()) < MC.COS_BOUND == 7.6e-14
    assert MC.COS_BOUND_TERMS["horner"] < 7.12e-14 and MC.COS_BOUND_TERMS["truncation"] < 3e-22
    assert MC.COS_BOUND_TERMS["square"] < 3.7e-15 and MC.COS_BOUND_TERMS["libm"] < 2.3e-16
    grid = np.concatenate([np.linspace(-3.6, 1.8, 200_001), [0.0, -3.6, 1.8], [3.0 * p for p, _ in MC.PLACEMENTS.values()]])
    assert len(grid) >= 10 ** 5 and grid.min() == -3.6 and grid.max() == 1.8
    for x in (grid, -grid):
        want = np.array([math.cos(t) for t in x])
        worst = float(np.max(np.abs(MC.poly_cos(x) - want)))
        print("cos polynomial: worst |C(x) - math.cos(x)| = %.3e, bound %.3e, RATIO %.4f" % (worst, MC.COS_BOUND, worst / MC.COS_BOUND))
        assert worst <= MC.COS_BOUND
    assert MC.poly_cos(0.0) == 1.0


def test_start_positions_lie_in_the_start_interval():
    draws = np.array([MC.start_position(seed, ep, env) for seed in (0, 7, 2 ** 40 + 3) for ep in range(40) for env in range(40)])
    assert draws.min() >= -0.6 and draws.max() < -0.4
    assert abs(draws.mean() + 0.5) < 4e-3 and draws.std() > 0.05          # uniform on the interval: sd 0.2 / sqrt(12) = 0.0577
    w = np.array([0, 2 ** 32 - 1], dtype=np.float64)                        # the extreme words
    ends = (w + 0.5) * 2.0 ** -32 * 0.2 - 0.6
    assert -0.6 <= ends[0] and ends[1] < -0.4


@pytest.mark.parametrize("E", [1, 5])
def test_pinned_trajectory_reaches_every_branch(E):
    """The condition under which the step-for-step comparisons (here and on the GPU) mean something: goal with +100, time
    limit, left wall with the velocity zeroed, both speed clips, the right wall, the action clipped on both sides and
    unclipped — each taken at least once by the trajectory both tests pin."""
    first, steps, reached = MC.pinned_rollout(E, seed=17 + E, limit=LIMIT)
    for name in ("goal", "time_limit", "wall_left", "wall_right", "speed_high", "speed_low", "action_low", "action_high",
                 "action_inside"):
        assert reached.get(name, 0) > 0, (name, reached)
    goals = [s for s in steps if (s["rewards"] > 50).any()]
    assert goals and all(s["dones"][s["rewards"] > 50].all() for s in goals)
    for s in goals:                                   # +100 minus the raw action's cost, rounded once
        a = s["actions"].astype(np.float64)
        hit = s["rewards"] > 50
        assert np.array_equal(s["rewards"][hit], (100.0 - (a * a) * 0.1).astype(np.float32)[hit])
    # a finished env returned its NEW episode's first observation
    for s in steps:
        d = s["dones"] == 1
        assert np.all(s["state"]["t"][d] == 0) and np.all(s["state"]["v"][d] == 0.0)
        assert np.all((s["obs"][d, 0] >= -0.6) & (s["obs"][d, 0] < -0.4))
    rec = MC.records(steps[-1]["state"])
    back = MC.from_records(rec)
    assert all(np.array_equal(back[k], steps[-1]["state"][k]) for k in back)


def test_host_env_matches_the_restatement_step_for_step():
    """MountainCarVecEnv against the restated step from the SAME float64 state, 150 steps on the fixed action stream with
    the placements put in by set_state: with np.cos in the polynomial's place the restated step is the env's bit for bit —
    state, reward, done — which proves the operation order; with the polynomial the velocity differs by at most
    0.0025 * COS_BOUND plus one rounding of the sum (an ulp of 0.07), the position by that plus an ulp of 1.2."""
    E, seed, steps = 5, 22, 150
    env = MountainCarVecEnv(E, max_episode_steps=LIMIT, seed=3)
    obs = env.reset()
    assert obs.dtype == np.float32 and obs.shape == (E, 2) and np.all((obs[:, 0] >= -0.6) & (obs[:, 0] < -0.4)) and not obs[:, 1].any()
    assert env.observation_space.shape == (2,) and env.action_space.shape == (1,) and not hasattr(env.action_space, "n")
    assert env.observation_space.low.tolist() == [np.float32(-1.2), np.float32(-0.07)]
    acts = MC.action_stream(seed, steps, E)
    schedule = MC.placement_schedule(E)
    reached, timed, ret = {}, 0, np.zeros(E)
    v_tol = MC.GRAVITY_TERM * MC.COS_BOUND + np.spacing(0.07)
    p_tol = v_tol + np.spacing(1.2)
    for n in range(steps):
        if n in schedule:
            name, e = schedule[n]
            st = env.get_state()
            st["x"][e] = MC.PLACEMENTS[name]
            env.set_state(st)
        st = env.get_state()
        p0, v0, t0 = st["x"][:, 0], st["x"][:, 1], st["t"]
        for k, hit in MC.branches(p0, v0, acts[n]).items():
            reached[k] = reached.get(k, 0) + int(hit.sum())
        obs, rewards, dones, infos = env.step(acts[n].reshape(E, 1))
        p1, v1, goal, r1 = MC.physics(p0, v0, acts[n], cos=np.cos)
        assert np.array_equal(dones, goal | (t0 + 1 >= LIMIT)) and np.array_equal(rewards, r1)
        keep = ~dones                                 # the env overwrote the others with their next start state
        after = env.get_state()["x"]
        assert np.array_equal(after[keep, 0], p1[keep]) and np.array_equal(after[keep, 1], v1[keep])
        assert np.array_equal(obs, after.astype(np.float32))
        assert np.all((after[dones, 0] >= -0.6) & (after[dones, 0] < -0.4)) and not after[dones, 1].any()
        p2, v2, goal2, r2 = MC.physics(p0, v0, acts[n])
        assert np.array_equal(goal2, goal) and np.array_equal(r2, r1)
        assert np.all(np.abs(v2 - v1) <= v_tol) and np.all(np.abs(p2 - p1) <= p_tol)
        timed += int((dones & ~goal).sum())
        ret += rewards
        for i in range(E):
            info = infos[i]["episode_info"]
            assert info["done"] == bool(dones[i]) and info["length"] == int(t0[i]) + 1 and info["reward"] == ret[i]
        ret[dones] = 0
    for name in ("goal", "wall_left", "wall_right", "speed_high", "speed_low", "action_low", "action_high", "action_inside"):
        assert reached.get(name, 0) > 0, (name, reached)
    assert timed > 0
