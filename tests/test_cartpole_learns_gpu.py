"""GPU: the device pipeline LEARNS CartPole.  One seeded cartpole_dqn-style run through rltime_amd.train.train — CartPole as
a HIP kernel (csrc/acting.hip k_cartpole_env_step), the generic device acting path, float32 observations through the device
replay as bytes, the 2x64 MLP learner — must end far above what any policy that gets no information from the observations
can reach.

The bar is not tuned against the code under test.  tests/test_cartpole_device_restate_cpu.py computes, with the NumPy
restatement of the env, the mean episode length over 2000 episodes of observation-blind policies: uniform random (22.3), both
constants (9.35, 9.36) and every periodic binary action word of period <= 6 (106 words; the best, left-right-right-left,
reaches 41.125).  L_BLIND is that best value rounded up, and that test asserts it is not below what it measures.  The run's
last-100 mean episode length must reach 3 x L_BLIND: the upright pole is unstable, so no open-loop action sequence balances
it, and the factor 3 covers blind policies outside the enumerated family while staying far below what a working pipeline
reaches.  3 x L_BLIND = 123.6 is under half of the 500-step episode cap.  A pipeline that loses the link between
observations and actions — observations cast to bytes, an actor on stale weights, actions stored one step late — is a blind
policy and cannot pass.

Measured on an MI355X (docs/measurement.md, "CartPole on the device"): seed 0, 100 000 acted steps, 819 episodes, 9.6 s:
last-100 mean length 87 after 25 000 steps, 253 after 50 000, 338 after 75 000, 341 at the end."""
import copy
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L_BLIND = 41.2            # best observation-blind policy, mean episode length (measured 41.125; see the module docstring)
EPISODE_CAP = 500
TOTAL_STEPS = 100000
CONFIG = {
    "acting": {"actor_envs": 16, "exploration": {"type": "epsilon_greedy", "args": {
        "eps_start": 1.0, "eps_final": 0.01, "exploration_fraction": 0.3}}},
    "env": "CartPole-v0", "env_args": {"max_episode_steps": EPISODE_CAP, "device": True},
    "model": {"type": "sequential", "args": {"layer_configs": [{"type": "fc", "args": {"fc_size": 64}},
                                                               {"type": "fc", "args": {"fc_size": 64}}]}},
    "policy_args": {"cuda": True},
    "training": {"type": "dqn", "args": {
        "gamma": 0.99, "mbatch_size": 128, "nstep_train": 1, "nstep_target": 10, "target_update_freq": 2000, "lr": 1e-3,
        "lr_anneal": True, "warmup_steps": 2000, "total_steps": TOTAL_STEPS, "log_freq": TOTAL_STEPS // 8,
        "episode_history_windows": [100],
        "history_mode": {"type": "replay", "args": {"size": 50000, "train_frequency": 8}}}},
}


def test_dqn_on_device_cartpole_beats_every_blind_policy():
    from rltime_amd.acting.cartpole_device_env import CartPoleDeviceVecEnv
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.train import train
    random.seed(0); np.random.seed(0); torch.manual_seed(0)      # noqa: E702
    logger = NullLogger()
    seen = {}
    trainer = train(copy.deepcopy(CONFIG), logger, on_trainer=lambda t: seen.update(trainer=t))
    assert logger.rows, "no log interval was reached"
    for _, _, row in logger.rows:
        print("steps %6d  episodes %5d  last100 episode length %.1f" % (row["total"].get("steps_acted", 0), row["total"]["episodes"],
                                                                        row["last100"]["episode_length"]))
    # the run went through the pieces it is about
    assert isinstance(trainer.actors._vec_env, CartPoleDeviceVecEnv)
    assert trainer.history_buffer._layout.float_obs and trainer.history_buffer._layout.frame_bytes == 16
    last = logger.rows[-1][2]
    bar = 3.0 * L_BLIND
    assert bar <= EPISODE_CAP / 2
    assert last["total"]["episodes"] >= 200
    assert last["last100"]["episode_length"] >= bar, (last["last100"]["episode_length"], bar)
