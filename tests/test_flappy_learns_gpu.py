"""GPU: the device pipeline LEARNS a game with long episodes and control under gravity.  One DQN run on Flappy
(rltime_amd/acting/flappy_env.py) through rltime_amd.train.train — device env in the captured rollout graph, fused acting
step, device replay, learner — must end far above what any policy that gets no information from the pixels can reach, and
the device evaluator on a fresh env must confirm it.

The bar is derived, not tuned (tests/flappy_restate.py, proved by tests/test_flappy_restate_cpu.py): a pipe's gap is
independent of everything drawn before it, so a pipeline that passes no information from the frames to the actions passes
each pipe with probability at most p = g / (R - g + 1); pipes per episode are stochastically below a Geometric variable
of mean p / (1 - p) and variance p / (1 - p)^2, and with death_reward = 0 an episode's reward is its pipes passed.  Over N
episodes the blind mean exceeds p / (1 - p) + 6 sqrt(p / (1 - p)^2 / N) with negligible probability: 0.577 pipes per
episode for R = 12, g = 3, N = 1000 (0.722 for the evaluator's N = 256).

Measured on an MI355X (docs/measurement.md, "Flappy on the device"), 60 000 acted steps, last-1000 mean episode reward per
log row (15 008 / 30 016 / 45 024 / 60 000 acted steps):
  seed 0: +0.50 (1 769 episodes), +2.20 (2 653), +4.49 (3 141), +6.47 (3 540); greedy evaluation 10.04; train 12.2 s cold
  seed 1: +0.37 (1 824 episodes), +1.75 (2 878), +3.76 (3 508), +5.14 (3 980); greedy evaluation 9.36; train 7.6 s
Both end above three times the bar (1.73); the test takes 8.9 s inside the whole suite.  Tried first, seed 0 at 100 000
steps: 8.01 (this config), 8.29 (100-step limit), 8.25 (gamma 0.95) — nothing needed tuning, `gap` was not enlarged."""
import copy
import random

import numpy as np
import pytest
import torch

from tests.flappy_restate import blind_bar

pytestmark = pytest.mark.gpu

ROWS, GAP, N, EVAL_N = 12, 3, 1000, 256
TOTAL_STEPS = 60000
ENV_ARGS = {"frame_shape": [4, 48, 32], "cell": 4, "gap": GAP, "spacing": 4, "n_actions": 2, "max_episode_steps": 300,
            "death_reward": 0.0}
CONFIG = {
    "acting": {"actor_envs": 32, "exploration": {"type": "epsilon_greedy", "args": {
        "eps_start": 1.0, "eps_final": 0.02, "exploration_fraction": 0.4}}},
    "env": "flappy", "env_args": ENV_ARGS,
    "model": {"type": "sequential", "args": {"layer_configs": [
        {"type": "cnn", "args": {"channels_last": True, "layers": [{"filters": 32, "kernel": 8, "stride": 4},
                                                                   {"filters": 32, "kernel": 3, "stride": 1}]}},
        {"type": "fc", "args": {"fc_size": 64}}]}},
    "policy_args": {},
    "training": {"type": "dqn", "args": {
        "clip_rewards": False, "gamma": 0.9, "mbatch_size": 64, "nstep_train": 1, "nstep_target": 2,
        "lr": 1e-3, "double_q": True, "clip_grad": 10.0, "target_update_freq": 1000,
        "total_steps": TOTAL_STEPS, "log_freq": TOTAL_STEPS // 4, "warmup_steps": 2000,
        "episode_history_windows": [N],
        "history_mode": {"type": "replay", "args": {"size": 20000, "train_frequency": 4}}}},
}


def run(config, seed):
    """-> (trainer, the logger's rows) of one training run with every generator seeded."""
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.train import train
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)      # noqa: E702
    logger = NullLogger()
    trainer = train(copy.deepcopy(config), logger)
    for _, _, row in logger.rows:
        print("steps %6d  episodes %6d  last%d reward %+.3f" % (row["total"].get("steps_acted", 0), row["total"]["episodes"], N,
                                                                  row["last%d" % N]["reward"]))
    return trainer, logger.rows


def evaluate(trainer, config, seed=1):
    from rltime_amd.acting.evaluator import Evaluator
    from rltime_amd.train import make_vec_env
    env = make_vec_env(config["env"], config["env_args"], 32, "cuda", seed=seed)
    ev = Evaluator(trainer.policy, env, EVAL_N, eps=0.0)
    rec = ev.run()
    print("evaluator: %d episodes, mean reward %.3f, mean length %.1f, fused %s" % (rec["episodes"], rec["reward"]["mean"],
                                                                                  rec["length"]["mean"], ev.fused))
    return ev, rec


def test_dqn_on_flappy_beats_every_blind_policy():
    trainer, rows = run(CONFIG, 0)
    assert rows, "no log interval was reached"
    last = rows[-1][2]
    bar = blind_bar(ROWS, GAP, N)
    assert ENV_ARGS["frame_shape"][1] // ENV_ARGS["cell"] == ROWS and abs(bar - 0.577) < 1e-3
    assert last["total"]["episodes"] >= 2 * N
    assert last["last%d" % N]["reward"] >= bar, (last["last%d" % N]["reward"], bar)
    # the evaluator (and with it the eval entry points) takes the env as it is: greedy episodes on a fresh env of 32
    ev, rec = evaluate(trainer, CONFIG)
    assert ev.fused and rec["episodes"] == EVAL_N
    assert rec["reward"]["mean"] > blind_bar(ROWS, GAP, EVAL_N), (rec["reward"]["mean"], blind_bar(ROWS, GAP, EVAL_N))
