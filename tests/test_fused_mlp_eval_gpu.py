"""GPU: evaluation of the CartPole MLP policies on the fused MLP step (Evaluator(fused_mlp=True), rltime_amd.eval on a run of
cartpole_dqn_fused.json).

Hand-made policies make the outcome known in advance.  The controller pushes right iff 0.1 x + 0.3 v + theta + 0.5 omega >
0: FC1's unit 0 is 10 x that form and unit 1 its negative, FC2 passes both through, Q1 reads unit 0 and Q0 unit 1 (the
quantile layer has weight 0 and bias 1: the product multiplies by one; the dueling value stream is left random: it ranks
nothing).  On the CPU env (acting/cartpole_env.py, 64 envs, seed 3) that controller reached a 200-step cap in 192 of 192
episodes, and a 1000-step cap in all 192 too; tests/test_fused_mlp_cpu.py confirms it on the NumPy restatement of the device
env for the seed used here.  With that margin one rounding flip changes nothing, so the test asserts the cap, not a
trajectory.  A policy that ignores the observation (bias only: always action 1) must reproduce the restatement's episode
lengths exactly: the device env's dynamics are pinned bit for bit (tests/test_cartpole_env_gpu.py)."""
import copy
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import cartpole_device_restate as CP
from tests.eval_restate import EvalCount

pytestmark = pytest.mark.gpu

MLP = {"type": "sequential", "args": {"layer_configs": [{"type": "fc", "args": {"fc_size": 64}}, {"type": "fc", "args": {"fc_size": 64}}]}}
E, N, CAP, SEED = 16, 32, 200, 0


def _env():
    from rltime_amd.acting.cartpole_device_env import CartPoleDeviceVecEnv
    return CartPoleDeviceVecEnv(E, max_episode_steps=CAP, seed=SEED)


def _policy(kind, env, what):
    """what: controller | mirrored (the two output rows swapped) | always-1 (bias only)."""
    from rltime_amd.policies.dqn import DQNPolicy
    from rltime_amd.policies.iqn import IQNPolicy
    torch.manual_seed(4)
    kw = dict(model_config=MLP, observation_space=env.observation_space, action_space=env.action_space, cuda=True)
    pol = IQNPolicy.create(dueling=True, **kw) if kind == "iqn-dueling" else DQNPolicy.create(**kw)
    fc1, fc2 = pol.model.layers[0].layers[0][0], pol.model.layers[1].layers[0][0]
    with torch.no_grad():
        for lin in (fc1, fc2, pol.out_layer):
            lin.weight.zero_()
            lin.bias.zero_()
        if kind == "iqn-dueling":
            pol.quantile_layer.weight.zero_()
            pol.quantile_layer.bias.fill_(1.0)
        if what == "always-1":
            pol.out_layer.bias[1] = 1.0
            return pol
        form = torch.tensor([0.1, 0.3, 1.0, 0.5], device=fc1.weight.device) * 10.0
        fc1.weight[0], fc1.weight[1] = form, -form
        fc2.weight[0, 0] = fc2.weight[1, 1] = 1.0
        q1, q0 = (1, 0) if what == "controller" else (0, 1)
        pol.out_layer.weight[q1, 0] = 1.0
        pol.out_layer.weight[q0, 1] = 1.0
    return pol


def _run(kind, what, steps_per_launch=32):
    from rltime_amd.acting.evaluator import Evaluator
    from rltime_amd.acting.fast_mlp_step import FastMlpStep
    env = _env()
    ev = Evaluator(_policy(kind, env, what), env, N, eps=0.0, seed=SEED, steps_per_launch=steps_per_launch, fused_mlp=True)
    rec = ev.run()
    assert ev.fused is True and isinstance(ev.actor._fast, FastMlpStep)
    graphs = [g for _, g in ev.actor._fast._rollouts.values()]
    assert len(graphs) >= 1 and all(g is not None for g in graphs)      # every replay was the captured rollout
    return ev, rec


@pytest.mark.parametrize("kind", ["dqn", "iqn-dueling"])
def test_the_controller_holds_every_episode_to_the_cap(kind):
    ev, rec = _run(kind, "controller")
    assert set(ev.ep_len.tolist()) == {CAP} and set(ev.ep_reward.tolist()) == {float(CAP)}
    assert rec["episodes"] == N and rec["envs"] == E and rec["length"]["mean"] == CAP
    ev, rec = _run(kind, "mirrored")
    print(kind, "mirrored controller: mean length", rec["length"]["mean"])
    assert rec["length"]["mean"] < 15


@pytest.mark.parametrize("kind", ["dqn", "iqn-dueling"])
def test_a_blind_policy_reproduces_the_restatements_episodes(kind):
    """Always action 1: the evaluator's lists equal the NumPy restatement's under the same seed, episode for episode, and
    steps_per_launch 1 and 32 give the same record."""
    ec = EvalCount(E, N)
    state, _, _, _ = CP.cartpole_reset(CP.new_state(E), SEED)
    while not ec.finished:
        state, _, r, d = CP.cartpole_step(state, np.ones(E, np.int32), SEED, CAP)
        ec.step(r, d)
    ev32, rec32 = _run(kind, "always-1", 32)
    ev1, rec1 = _run(kind, "always-1", 1)
    for ev in (ev32, ev1):
        assert np.array_equal(ev.ep_len, ec.ep_len) and np.array_equal(ev.ep_reward, ec.ep_reward)
        assert ev.steps == int(ec.counters[2])
    assert 8 <= int(ev32.ep_len.min()) and int(ev32.ep_len.max()) <= 11
    assert rec1 == rec32


def test_the_opt_in_on_an_uncovered_policy_says_why():
    from rltime_amd.acting.evaluator import Evaluator
    from rltime_amd.policies.dqn import DQNPolicy
    env = _env()
    model = {"type": "sequential", "args": {"layer_configs": [{"type": "fc", "args": {"fc_size": 64, "fc_count": 2}}]}}
    pol = DQNPolicy.create(model_config=model, observation_space=env.observation_space, action_space=env.action_space, cuda=True)
    with pytest.raises(ValueError, match="fused_mlp was asked for.*single Linear"):
        Evaluator(pol, env, N, fused_mlp=True)
    with pytest.raises(ValueError, match="float32 vector observations"):
        Evaluator(pol, env, N)


def _train(tmp_path, name):
    from rltime_amd.general.config import load_config
    from rltime_amd.general.loggers import DirectoryLogger
    from rltime_amd.train import train
    random.seed(0); np.random.seed(0); torch.manual_seed(0)      # noqa: E702
    config = copy.deepcopy(load_config(name + ".json"))
    config["training"]["args"].update(total_steps=480, log_freq=240, warmup_steps=128, eval_episodes=16 if name.endswith("fused") else 0)
    config["env_args"]["max_episode_steps"] = 100
    logger = DirectoryLogger(str(tmp_path / name), echo=False)
    trainer = train(config, logger)
    return trainer, logger


def test_eval_entry_points_on_a_run_of_the_fused_config(tmp_path):
    """A few hundred steps of cartpole_dqn_fused.json with a periodic evaluation, then eval_policy on the run directory:
    the actor acted on the fused MLP step, every log row has its `eval` row, and eval_policy appends one more record."""
    from rltime_amd.acting.fast_mlp_step import FastMlpStep
    from rltime_amd.eval import eval_policy
    trainer, logger = _train(tmp_path, "cartpole_dqn_fused")
    assert isinstance(trainer.actors._fast, FastMlpStep)
    evals = [row for name, _, row in logger.rows if name == "eval"]
    trains = [row for name, _, row in logger.rows if name == "train"]
    assert len(evals) == len(trains) >= 2 and all(row["episodes"] == 16 for row in evals)
    assert trains[-1]["total"]["steps_trained"] > 0
    path = os.path.join(logger.path, "eval.json")
    before = open(path).read().splitlines()
    got = eval_policy(logger.path, 16, 32, eps=0)
    lines = open(path).read().splitlines()
    assert len(lines) == len(before) + 1 and lines[:-1] == before
    line = json.loads(lines[-1])
    assert line["episodes"] == 32 and line["envs"] == 16 and line["reward"]["mean"] == got["reward"]["mean"]
    assert 1 <= line["length"]["min"] <= line["length"]["max"] <= 100


def test_eval_policy_still_refuses_a_run_of_the_parent_config(tmp_path):
    from rltime_amd.eval import eval_policy
    trainer, logger = _train(tmp_path, "cartpole_dqn")
    assert not trainer.actors._fast                              # the generic device path, as before
    with pytest.raises(ValueError, match="float32 vector observations"):
        eval_policy(logger.path, 16, 32, eps=0)
