#!/usr/bin/env python3
"""Golden-vector generator for the recurrent on-policy case.  Runs ONLY in the development container, like generate.py:
it imports the *unmodified* reference through the import shims of oracle/ref_shims, feeds its OnlineHistoryBuffer the seeded
stream of tests/online_lstm_restate.py (ONLINE_LSTM_CASE: 3 envs, T = 4, an fc16 -> lstm8 policy, episode ends inside the
sequences, recurrent next_state pytrees) and writes what it produced to tests/golden/online_ppo_lstm.npz:

  every leaf of every batch (states / target_states with hx, cx, initials of the recurrent layer),
  calc_target_values with timesteps = 1 (every target row starts from its own stored state),
  PPO._compute_grads gradients and logged losses at timesteps = T and at timesteps = T / 2.

The fixture is data only; the inputs are re-derived from the seeds.

    python tests/golden/generate_online_lstm.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle", "ref_shims"), "/root/reference"]

from tests.golden.streams import seeded_weights  # noqa: E402
from tests.online_lstm_restate import ONLINE_LSTM_CASE as case, online_lstm_vector_steps  # noqa: E402

from rltime.general.backend import StateStore  # noqa: E402
from rltime.general.value_log import ValueLog  # noqa: E402


def flatten(prefix, tree, out):
    if isinstance(tree, dict):
        for k, v in tree.items():
            flatten(prefix + "." + k if prefix else k, v, out)
    elif isinstance(tree, (tuple, list)):
        for i, v in enumerate(tree):
            flatten("%s.%d" % (prefix, i), v, out)
    else:
        out[prefix] = tree.numpy() if isinstance(tree, torch.Tensor) else np.asarray(tree)


def tree_map(tree, f):
    if isinstance(tree, dict):
        return {k: tree_map(v, f) for k, v in tree.items()}
    if isinstance(tree, (tuple, list)):
        return type(tree)(tree_map(v, f) for v in tree)
    return f(tree)


def run():
    import gym
    from rltime.history.online_history import OnlineHistoryBuffer
    from rltime.training.torch.ppo import PPO
    from rltime.policies.torch.actor_critic import ActorCriticPolicy
    T, gamma, lam = case["nstep_train"], case["gamma"], case["advlam"]
    tr = PPO.__new__(PPO)
    tr.gamma, tr.advlam, tr.vf_coef, tr.adv_norm = gamma, lam, case["vf_coef"], True
    tr.entropy_factor, tr.entropy_anneal = case["entropy_factor"], None
    tr._clip_value, tr._clip_anneal = case["clip_value"], None
    tr.vf_scale_epsilon = None
    tr.steps, tr.total_steps = 0, 1
    tr.value_log = ValueLog()
    policy = ActorCriticPolicy.create(
        model_config=case["model"], observation_space=gym.spaces.Box(-10, 10, (case["obs_dim"],), np.float32),
        action_space=gym.spaces.Discrete(case["n_actions"]), cuda=False)
    policy.load_state_dict(seeded_weights(policy.state_dict(), case["weights_seed"]))
    assert policy.is_recurrent()
    tr.policy = tr.target_policy = policy
    ref = OnlineHistoryBuffer(nstep_target=T, nstep_train=T, discount_function=tr._get_discount_function(gamma),
                              state_store=StateStore("cpu"))
    out, step_no, rnd, mid_initials = {}, 0, 0, 0
    for op in case["script"]:
        if op[0] == "feed":
            for samples in online_lstm_vector_steps(case, op[1], step_no):
                ref.update(samples)
            step_no += op[1]
            continue
        tag = "r%d" % rnd
        rnd += 1
        B = op[1]
        feed = ref.needed_feed_count(B, case["num_envs"])
        out[tag + ".feed_count"] = np.array(-1 if feed is None else case["num_envs"])
        got = ref.get_train_data(B)
        out[tag + ".is_none"] = np.array(got is None)
        if got is None:
            continue
        flat = {}
        flatten("", got, flat)
        for k, v in flat.items():
            out[tag + ".batch." + k] = v
        mid_initials += int(flat["states.layer1_state.initials"][1:].sum())
        # multi_step_trainer.py:290-320: flatten (T, B) -> (T*B), targets with single-step target states
        f = lambda x: x.reshape((x.shape[0] * x.shape[1],) + tuple(x.shape[2:]))                # noqa: E731
        data = {k: tree_map(v, f) for k, v in got.items() if k != "extra_data"}
        targets = tr.calc_target_values(data["returns"], data["target_states"], data["target_masks"], data["nsteps"], 1)
        out[tag + ".targets"] = targets.detach().numpy()
        for steps in (T, T // 2):
            policy.zero_grad()
            tr.value_log.get()
            tr._compute_grads(data["states"], targets, data["policy_outputs"], {}, steps)
            for name, prm in policy.named_parameters():
                out["%s.t%d.grad.%s" % (tag, steps, name)] = prm.grad.detach().numpy().copy()
            log = tr.value_log.get()["train"]
            for key in ("value_loss", "policy_loss", "policy_entropy", "state_value_mean"):
                out["%s.t%d.log.%s" % (tag, steps, key)] = np.array(log[key])
    assert mid_initials > 0, "no episode end inside a sequence: pick another seed"
    out["rounds"] = np.array(rnd)
    path = os.path.join(HERE, "online_ppo_lstm.npz")
    np.savez_compressed(path, **out)
    print("recurrent online / PPO case: %d draws, %d keys, %d initials inside sequences, %d bytes"
          % (rnd, len(out), mid_initials, os.path.getsize(path)))


if __name__ == "__main__":
    torch.manual_seed(0)
    run()
