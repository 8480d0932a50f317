#!/usr/bin/env python3
"""Fixture generator for the evaluation counting rule.  Runs ONLY in the development container.

Imports the *unmodified* reference through the oracle/ref_shims import path (like generate.py) and runs its OWN
eval_policy(..., eps=0).  Only the collaborators eval_policy looks up in its module are replaced, on the imported module
object: make_env_creator / make_sub_proc_vec_env give a scripted vector env that replays seeded (rewards, dones) streams
and fills info[i]["episode_info"] the way the reference's EpisodeTracker wrapper does (running sums of the step rewards
as Python floats), create_policy_from_config a stub policy, DirectoryLogger a stub that keeps the logged record.  The
counting loop, the printed episode lines and the record are the reference's.  Written to eval_cases.npz: per case the
streams, N, the per-episode rewards in counting order (parsed from the reference's `Episode k/N finished with reward:`
lines), the env steps consumed and the logged record; plus eval_policy's parameter list.  Data only.

    python tests/golden/generate_eval.py
"""
import contextlib
import inspect
import io
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "ref_shims"), "/root/reference"]

import rltime.eval as ref_eval  # noqa: E402

# (E, N, done probability, seed)
CASES = [(1, 1, 0.5, 1), (1, 3, 0.4, 2), (3, 7, 0.3, 3),
         (63, 64, 1.0, 4), (64, 64, 1.0, 5), (65, 66, 1.0, 6),
         (255, 256, 0.5, 7), (257, 300, 0.9, 8), (600, 601, 0.7, 9),
         (600, 1500, 0.05, 10)]
STAT_KEYS = ("mean", "min", "max", "median", "std")


def make_stream(E, N, p, seed):
    """Long enough for every one of the N counted episodes to end (with p < 1 an env's episode ends within 400 steps with
    probability 1 - 0.95^400 > 1 - 2e-9; the generator asserts it did), trimmed after the run."""
    rng = np.random.RandomState(seed)
    T = 16 if p == 1.0 else 400 + 3 * int(np.ceil(N / (E * p)))
    rewards = (rng.randint(-10, 11, size=(T, E)).astype(np.float32) * np.float32(0.1)).astype(np.float32)
    dones = rng.random_sample((T, E)) < p
    return rewards, dones


class ScriptedVecEnv:
    action_space = observation_space = None

    def __init__(self, rewards, dones):
        self.rewards, self.dones = rewards, dones
        self.num_envs = rewards.shape[1]
        self.t = 0
        self.acc = [0] * self.num_envs            # EpisodeTracker.reset: reward = 0, len = 0
        self.len = [0] * self.num_envs

    def reset(self):
        return np.zeros((self.num_envs, 1), np.float32)

    def step(self, actions):
        r, d = self.rewards[self.t], self.dones[self.t]
        self.t += 1
        infos = []
        for i in range(self.num_envs):
            self.acc[i] += float(r[i])            # what a gym env hands the wrapper: a Python float of the float32 reward
            self.len[i] += 1
            infos.append({"episode_info": {"reward": self.acc[i], "length": self.len[i], "done": bool(d[i])}})
            if d[i]:                              # the auto-resetting vector env resets the wrapper
                self.acc[i], self.len[i] = 0, 0
        return np.zeros((self.num_envs, 1), np.float32), r.copy(), d.copy(), infos

    def close(self):
        pass


class StubPolicy:
    def load_state(self, state):
        pass

    def make_input_state(self, obs, dones):
        return len(obs)

    def actor_predict(self, state, timesteps):
        return {"actions": np.zeros(state, np.int64)}


class StubLogger:
    last = None

    def __init__(self, path, **kwargs):
        pass

    def get_config(self):
        return {"env": "scripted"}

    def get_checkpoint(self):
        return 12345, {"policy_state": None}

    def log_result(self, name, result, step):
        assert name == "eval" and step is None
        StubLogger.last = result


def run_reference(rewards, dones, N):
    env = ScriptedVecEnv(rewards, dones)
    ref_eval.make_env_creator = lambda *a, **k: None
    ref_eval.make_sub_proc_vec_env = lambda creator, num_envs: env
    ref_eval.create_policy_from_config = lambda *a, **k: StubPolicy()
    ref_eval.DirectoryLogger = StubLogger
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ref_eval.eval_policy("unused", rewards.shape[1], N, eps=0)
    eps = [float(m) for m in re.findall(r"^Episode \d+/\d+ finished with reward: (\S+)$", out.getvalue(), re.M)]
    return np.array(eps, np.float64), env.t, StubLogger.last


def main():
    out = {}
    for k, (E, N, p, seed) in enumerate(CASES):
        rewards, dones = make_stream(E, N, p, seed)
        ep, steps, rec = run_reference(rewards, dones, N)
        assert len(ep) == N and rec["episodes"] == N and rec["envs"] == E and rec["step"] == 12345
        assert np.mean(ep) == rec["reward"]["mean"]          # repr round-trips a float64 exactly
        T = steps + 12                                       # the steps consumed plus a few more (over-run checks)
        assert T <= rewards.shape[0]
        out["c%d_rewards" % k] = rewards[:T]
        out["c%d_dones" % k] = dones[:T].astype(np.uint8)
        out["c%d_n" % k] = np.int64(N)
        out["c%d_ep_reward" % k] = ep
        out["c%d_steps" % k] = np.int64(steps)
        out["c%d_reward_stats" % k] = np.array([rec["reward"][s] for s in STAT_KEYS], np.float64)
        out["c%d_length_stats" % k] = np.array([rec["length"][s] for s in STAT_KEYS], np.float64)
        print("case %d: E=%d N=%d p=%.2f steps=%d kept T=%d mean reward %r" % (k, E, N, p, steps, T, rec["reward"]["mean"]))
    out["num_cases"] = np.int64(len(CASES))
    sig = [[n, None if q.default is inspect.Parameter.empty else q.default]
           for n, q in inspect.signature(ref_eval.eval_policy).parameters.items()]
    out["eval_policy_signature"] = np.array(json.dumps(sig))
    out["record_keys"] = np.array(json.dumps(sorted(rec.keys())))
    path = os.path.join(HERE, "eval_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
