"""GPU: the device pipeline LEARNS.  One DQN run on Catch (rltime_amd/acting/catch_env.py) through rltime_amd.train.train —
device env in the captured rollout graph, fused acting step, device replay, learner — must end far above what any policy
that gets no information from the pixels can reach.

The bar is derived, not tuned.  The ball column is uniform and independent of everything before it, so a pipeline that
passes no information from the frames to the actions (actions stored one step late, an actor reading stale weights, a
target net never synced, frames that are not the env's) catches independent Bernoulli(1 / G) balls
(tests/test_catch_restate_cpu.py proves the 1 / G exactly).  Over a window of N = 1000 episodes the catch rate of such a
pipeline exceeds 1 / G + 6 sigma, sigma = sqrt((1 / G)(1 - 1 / G) / N), with probability below 1e-9; as a mean reward
(+1 catch, -1 miss) that is 2 (1 / G + 6 sigma) - 1 = -0.525 for G = 6.  The optimal policy's mean reward is +1.

Measured on an MI355X (docs/measurement.md, "Catch on the device"): seed 0, 60 000 acted steps, 11 968 episodes, 10.8 s:
last-1000 mean reward +0.18 after 15 000 steps, +0.99 after 30 000, +0.96 at the end."""
import copy
import math
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G, N = 6, 1000
TOTAL_STEPS = 60000
CONFIG = {
    "acting": {"actor_envs": 32, "exploration": {"type": "epsilon_greedy", "args": {
        "eps_start": 1.0, "eps_final": 0.02, "exploration_fraction": 0.4}}},
    "env": "catch", "env_args": {"frame_shape": [4, 36, 36], "grid": G, "n_actions": 3},
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


def test_dqn_on_catch_beats_every_blind_policy():
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.train import train
    random.seed(0); np.random.seed(0); torch.manual_seed(0)      # noqa: E702
    logger = NullLogger()
    train(copy.deepcopy(CONFIG), logger)
    assert logger.rows, "no log interval was reached"
    for _, _, row in logger.rows:
        print("steps %6d  episodes %6d  last%d reward %+.3f" % (row["total"].get("steps_acted", 0), row["total"]["episodes"], N,
                                                                  row["last%d" % N]["reward"]))
    last = logger.rows[-1][2]
    p = 1.0 / G
    bar = 2.0 * (p + 6.0 * math.sqrt(p * (1.0 - p) / N)) - 1.0
    assert abs(bar - (-0.525)) < 1e-3
    assert last["total"]["episodes"] >= 2 * N
    assert last["last%d" % N]["reward"] >= bar, (last["last%d" % N]["reward"], bar)
