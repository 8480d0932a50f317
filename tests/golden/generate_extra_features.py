#!/usr/bin/env python3
"""Fixture generator for the extra-features observation.  Runs ONLY in the development container.

Imports the *unmodified* reference's ExtraFeaturesEnvWrapper through the oracle/ref_shims import path (like
generate_eval.py) and drives it with a scripted inner env that replays seeded (reward, done) streams and fills
info["episode_info"]["done"] the way the reference's EpisodeTracker wrapper does; the env is reset when done the way the
reference's auto-resetting vector env does it (the observation of a done step is the reset's).  Written to
extra_features_cases.npz: per case the parameters, the actions, rewards and dones of every step and the feature rows
(row 0: after the first reset; row 1 + t: the observation that follows step t), plus the wrapper's __init__ parameter
list.  While writing, tests/extra_features_restate.py is asserted equal to the wrapper bit for bit.  Data only.

    python tests/golden/generate_extra_features.py <path of the reference checkout>
"""
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("RLTIME_REFERENCE", "")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "ref_shims"), REFERENCE]

import gym  # noqa: E402  (the shim)
from rltime.env_wrappers.common import ExtraFeaturesEnvWrapper  # noqa: E402
from tests.extra_features_restate import ExtraFeatures, feature_size  # noqa: E402

ACTIONS = (1, 3, 6, 18)
FLAGS = [(a, r, t) for a in (1, 0) for r in (1, 0) for t in (1, 0) if a or r or t]      # (action, reward, timestep)
SCALES = {"default": None, "seventh": 1. / 7}
REWARDS = np.array([-2.5, -1.0, -0.3, 0.0, 0.0, 0.0, 0.1, 0.75, 1.0, 3.0], np.float32)     # fractional, zero, both signs


def make_cases():
    """Short cases: every A x every non-empty flag set, each with two (clip, scale) pairs chosen so that every A and every
    flag set meets all four pairs.  Long cases: one per A (and both scales for A = 3) with an episode of more than 300
    steps — the counter leaves the range where every product with the scale is exact."""
    cases = []
    for ia, A in enumerate(ACTIONS):
        for jf, flags in enumerate(FLAGS):
            pairs = [(1, "default"), (0, "seventh")] if (ia + jf) % 2 == 0 else [(1, "seventh"), (0, "default")]
            for clip, scale in pairs:
                cases.append(dict(A=A, flags=flags, clip=clip, scale=scale, T=40, long=0))
    for A, clip, scale in ((1, 1, "seventh"), (3, 0, "default"), (3, 1, "seventh"), (6, 0, "seventh"), (18, 1, "default")):
        cases.append(dict(A=A, flags=(1, 1, 1), clip=clip, scale=scale, T=400, long=1))
    return cases


def make_stream(case, k):
    rng = np.random.RandomState(1000 + k)
    T, A = case["T"], case["A"]
    actions = rng.randint(0, A, size=T).astype(np.int32)
    rewards = REWARDS[rng.randint(0, len(REWARDS), size=T)]
    dones = rng.random_sample(T) < 0.15
    if case["long"]:
        dones[8:330] = False                       # one episode of more than 300 steps
        dones[330] = True
    if k % 2 == 0:
        dones[0] = True                            # a done on the first step
    dones[5:8] = True                              # dones on consecutive steps
    return actions, rewards, dones.astype(np.uint8)


class ScriptedEnv(gym.Env):
    def __init__(self, A, rewards, dones):
        self.action_space = gym.spaces.Discrete(A)
        self.observation_space = gym.spaces.Box(0, 255, (1,), np.uint8)
        self.rewards, self.dones, self.t = rewards, dones, 0

    def reset(self):
        return np.zeros(1, np.uint8)

    def step(self, action):
        r, d = float(self.rewards[self.t]), bool(self.dones[self.t])     # what a gym env hands a wrapper: Python scalars
        self.t += 1
        return np.zeros(1, np.uint8), r, d, {"episode_info": {"done": d}}


def run_reference(case, actions, rewards, dones):
    kw = dict(include_action=bool(case["flags"][0]), include_reward=bool(case["flags"][1]),
              include_timestep=bool(case["flags"][2]), clip_reward=bool(case["clip"]))
    if SCALES[case["scale"]] is not None:
        kw["timestep_scale"] = SCALES[case["scale"]]
    env = ExtraFeaturesEnvWrapper(ScriptedEnv(case["A"], rewards, dones), **kw)
    assert env.observation_space.spaces[1].shape == (feature_size(case["A"], *case["flags"]),)
    rows = [env.reset()[1]]
    for t in range(case["T"]):
        obs, r, d, info = env.step(int(actions[t]))
        if d:
            obs = env.reset()                      # the auto-resetting vector env
        rows.append(obs[1])
    rows = np.stack(rows)
    assert rows.dtype == np.float32
    return rows, kw


def main():
    sig = [[n, None if q.default is inspect.Parameter.empty else q.default]
           for n, q in inspect.signature(ExtraFeaturesEnvWrapper.__init__).parameters.items()]
    default_scale = dict((n, d) for n, d in sig)["timestep_scale"]
    out, params = {}, []
    cases = make_cases()
    for k, case in enumerate(cases):
        actions, rewards, dones = make_stream(case, k)
        rows, kw = run_reference(case, actions, rewards, dones)
        scale = kw.get("timestep_scale", default_scale)
        mine = ExtraFeatures(1, case["A"], kw["include_action"], kw["include_reward"], kw["include_timestep"], kw["clip_reward"], scale)
        got = [mine.reset()[0]]
        for t in range(case["T"]):
            got.append(mine.step(actions[t:t + 1], rewards[t:t + 1], dones[t:t + 1])[0])
        got = np.stack(got)
        assert got.dtype == np.float32 and got.shape == rows.shape and np.array_equal(got.view(np.uint32), rows.view(np.uint32)), k
        out["c%d_actions" % k], out["c%d_rewards" % k], out["c%d_dones" % k], out["c%d_rows" % k] = actions, rewards, dones, rows
        params.append(dict(A=case["A"], include_action=kw["include_action"], include_reward=kw["include_reward"],
                           include_timestep=kw["include_timestep"], clip_reward=kw["clip_reward"], timestep_scale=scale,
                           T=case["T"], long=case["long"]))
    out["num_cases"] = np.int64(len(cases))
    out["params"] = np.array(json.dumps(params))
    out["wrapper_signature"] = np.array(json.dumps(sig))
    first = ExtraFeaturesEnvWrapper(ScriptedEnv(3, np.zeros(1, np.float32), np.zeros(1, np.uint8))).reset()[1]
    assert first.tolist() == [1, 0, 0, 0, 0]       # index 0 is set after a reset: _last_action = 0
    path = os.path.join(HERE, "extra_features_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
