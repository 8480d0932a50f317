"""GPU: the evaluation entry points.  A Catch DQN run through rltime_amd.train.train with a periodic evaluation
(training args eval_episodes) into a directory logger, then rltime_amd.eval.eval_policy on that directory.

Both greedy scores — the last periodic `eval` row's and eval_policy's — must reach the bar DERIVED in
tests/test_catch_learns_gpu.py's docstring: a pipeline that passes no information from the frames to the actions exceeds
a mean reward of 2 (1 / G + 6 sigma) - 1 = -0.525 over N = 1000 episodes (G = 6) with probability below 1e-9.  The bar is
not tuned to what the policy reaches.

Measured on an MI355X (docs/measurement.md, "Catch on the device"): seed 0, 30 016 acted steps with four log rows.
Greedy mean reward over 1000 episodes on 32 envs (eps = 0): +0.67 after 7 520 acted steps, +1.000 after 15 008, 22 528 and
30 016 (the training window's last-1000 reward under the exploration schedule: -0.36, +0.91, +0.98, +0.99); eval_policy on
the run directory: +1.000.  One evaluation is 160 vector steps (five replays of the 32-step rollout graph) and took
0.15-0.27 s inside training and 0.36 s through eval_policy, building its env, actor and graph each time; the whole
30 016-step run took 5.77 s without evaluation (5.83-6.02 s at the parent commit) and 6.34-6.68 s with the four of them."""
import copy
import json
import math
import os
import random

import numpy as np
import pytest
import torch

from tests.test_catch_learns_gpu import CONFIG, G, N

pytestmark = pytest.mark.gpu

TOTAL_STEPS = 30000
REFERENCE_KEYS = {"step", "date", "episodes", "envs", "reward", "length"}
STAT_KEYS = {"mean", "min", "max", "median", "std"}


def _config(total_steps, log_freq, **training):
    config = copy.deepcopy(CONFIG)
    config["training"]["args"].update(total_steps=total_steps, log_freq=log_freq, **training)
    return config


def _seed():
    random.seed(0); np.random.seed(0); torch.manual_seed(0)      # noqa: E702


def test_trained_catch_policy_scores_above_the_blind_bar_greedily(tmp_path):
    from rltime_amd.eval import eval_policy
    from rltime_amd.general.loggers import DirectoryLogger
    from rltime_amd.train import train
    _seed()
    logger = DirectoryLogger(str(tmp_path / "run"), echo=False)
    train(_config(TOTAL_STEPS, TOTAL_STEPS // 4, eval_episodes=N), logger)
    evals = [(step, row) for name, step, row in logger.rows if name == "eval"]
    trains = [step for name, step, _ in logger.rows if name == "train"]
    assert len(evals) == len(trains) == 4 and [s for s, _ in evals] == trains
    for step, row in evals:
        print("steps %6d  greedy mean reward over %d episodes %+.3f  (%d vector steps, %.3f s)"
              % (step, row["episodes"], row["reward"]["mean"], row["steps"], row["seconds"]))
    p = 1.0 / G
    bar = 2.0 * (p + 6.0 * math.sqrt(p * (1.0 - p) / N)) - 1.0
    assert abs(bar - (-0.525)) < 1e-3
    path = os.path.join(logger.path, "eval.json")
    lines_before = open(path).read().splitlines()
    assert len(lines_before) == 4
    got = eval_policy(logger.path, 32, N, eps=0)
    print("eval_policy: mean reward %+.3f over %d episodes on %d envs, %d vector steps, %.3f s"
          % (got["reward"]["mean"], got["episodes"], got["envs"], got["steps"], got["seconds"]))
    lines = open(path).read().splitlines()
    assert len(lines) == len(lines_before) + 1 and lines[:-1] == lines_before
    line = json.loads(lines[-1])
    assert set(line) == REFERENCE_KEYS | {"steps", "seconds"}
    assert set(line["reward"]) == STAT_KEYS == set(line["length"])
    # (the checkpoint is the last log row's: the acted steps at which the TOTAL_STEPS boundary was crossed)
    assert line["step"] == trains[-1] == got["step"] >= TOTAL_STEPS and line["episodes"] == N and line["envs"] == 32
    assert line["reward"]["mean"] == got["reward"]["mean"]
    assert line["length"]["min"] == line["length"]["max"] == G - 1
    assert evals[-1][1]["reward"]["mean"] >= bar, (evals[-1][1]["reward"]["mean"], bar)
    assert got["reward"]["mean"] >= bar, (got["reward"]["mean"], bar)


def test_periodic_evaluation_perturbs_nothing():
    """The final weights of a 2000-step run with eval_episodes = 64 and of the same run without: bit-identical.

    Seen on the MI355X: on one machine seven such runs (eval_episodes 0 and 64 mixed, one process and fresh processes) ended
    in the same weights, byte for byte.  On another machine, before the deterministic-solver setting below was made, three
    runs with eval_episodes = 0 in one process ended in three different sets of weights: there the training run did not
    repeat ITSELF, so this comparison failed for a reason that is not the evaluation's.  Whether the setting removes that
    was not seen (the later visits met the machine that repeats either way)."""
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.train import train
    states, evals = [], []
    for episodes in (64, 0):
        _seed()
        logger = NullLogger()
        # (the library convolutions without atomically-accumulating solvers, as tests/resume_driver.py asks for them: the
        # comparison needs a training run that repeats itself)
        keep = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True
        try:
            trainer = train(_config(2000, 500, warmup_steps=500, eval_episodes=episodes), logger)
        finally:
            torch.backends.cudnn.deterministic = keep
        last = [row for name, _, row in logger.rows if name == "train"][-1]
        assert last["total"]["steps_trained"] > 0             # the learner ran: the weights are trained ones
        states.append({k: v.detach().cpu() for k, v in trainer.policy.state_dict().items()})
        evals.append([row for name, _, row in logger.rows if name == "eval"])
    assert len(evals[0]) == 4 and not evals[1]
    a, b = states
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_periodic_evaluation_is_refused_where_it_is_not_built():
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.train import train
    with pytest.raises(ValueError, match="process group"):
        train(_config(2000, 500, eval_episodes=64), NullLogger(), data_parallel=object())
    with pytest.raises(ValueError, match="eval_envs"):
        train(_config(2000, 500, eval_episodes=16, eval_envs=32), NullLogger())
