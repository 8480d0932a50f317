"""CPU: the shipped mountaincar_continuous_ppo.json loads, validates, holds the reference's values (written out here
literally from rltime/configs/mountaincar_continuous_ppo.json and models/mlp_2x64.json) and trains on the host env; the env
string resolves to the host or the device class; what a Box action space does not run under is refused with ValueError
before optimizer or history are built."""
import copy

import numpy as np
import pytest

from rltime_amd.general.config import load_config, validate_config

_FC64 = {"type": "fc", "args": {"fc_size": 64}}
REFERENCE = {
    "acting": {"actor_envs": 16, "extra_args": {"use_proc": False}},
    "model": {"type": "sequential", "args": {"layer_configs": [_FC64, _FC64]}},
    "env": "MountainCarContinuous-v0",
    "policy_args": {"cuda": False},
    "training": {"type": "ppo", "args": {
        "gamma": 0.99, "nstep_train": 32, "entropy_factor": 1e-2, "lr": 1e-3, "lr_anneal": True, "clip_value": 0.2,
        "epochs": 4, "minibatches": 4, "advlam": 0.95, "vf_coef": 0.5, "total_steps": 500000}},
}


def _config():
    config = load_config("mountaincar_continuous_ppo.json")
    validate_config(config)
    return config


def _small(config, **training):
    """The shipped config at 4 envs x 8 steps per iteration with 10-step episodes."""
    config = copy.deepcopy(config)
    config.pop("_comment", None)
    config["acting"]["actor_envs"] = 4
    config["env_args"] = {"max_episode_steps": 10}
    config["training"]["args"].update(nstep_train=8, total_steps=64, log_freq=32)
    config["training"]["args"].update(training)
    return config


def test_shipped_config_is_the_reference():
    config = _config()
    config.pop("_comment", None)
    assert config == REFERENCE


def test_device_config_is_the_reference_plus_the_device_keys():
    config = load_config("mountaincar_continuous_ppo_device.json")
    validate_config(config)
    config.pop("_comment", None)
    want = copy.deepcopy(REFERENCE)
    want["env_args"] = {"device": True}
    want["policy_args"]["cuda"] = True
    assert config == want


def test_normal_head_is_no_longer_refused_on_the_device_path():
    """why_not_on_device keeps its other refusals and adds D > 16 (a CPU policy answers the same questions)."""
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    from rltime_amd.spaces import Box
    config = _config()
    obs = Box(-np.ones(2, np.float32), np.ones(2, np.float32), (2,), np.float32)

    def make(dims, **kw):
        space = Box(-np.ones(dims, np.float32), np.ones(dims, np.float32), (dims,), np.float32)
        return ActorCriticPolicy.create(model_config=config["model"], observation_space=obs, action_space=space, cuda=False, **kw)
    assert make(1).why_not_on_device() is None and make(16).why_not_on_device() is None and make(1).has_normal_head()
    assert "16 action components" in make(17).why_not_on_device()
    assert "critic_separate_model" in make(1, critic_separate_model=True).why_not_on_device()
    with pytest.raises(ValueError, match="Categorical"):
        make(1).actor_head_ac_raw(None, 1)


def test_host_config_trains_two_iterations_on_the_cpu():
    """Two iterations of 4 envs x 8 steps, each 4 epochs x 4 minibatches of PPO updates on the Normal head: the weights —
    logstd among them — move, the log rows carry the mean of the action component where the Discrete runs carry the
    histogram, and finished 10-step episodes are counted."""
    import torch
    from rltime_amd import train
    from rltime_amd.acting.mountaincar_env import MountainCarVecEnv
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.policies.actor_critic import NormalHead

    rows = []

    class Rows(NullLogger):
        def log_result(self, name, row, step):
            rows.append((name, step, row))

    torch.manual_seed(0)
    np.random.seed(0)
    start = {}
    trainer = train.train(_small(_config()), Rows(echo=False), device="cpu",
                          on_trainer=lambda t: start.setdefault("hook", t))
    pol = trainer.policy
    assert isinstance(trainer.actors._vec_env, MountainCarVecEnv) and trainer.actors._vec_env.max_episode_steps == 10
    assert isinstance(pol.actor, NormalHead) and pol.actor.logstd.shape == (1,) and not pol.is_cuda()
    assert trainer.steps == 64
    assert float(pol.actor.logstd.detach().abs().max()) > 0.0                # it started at 0 and was trained
    assert all(bool(torch.isfinite(p).all()) for p in pol.parameters())
    train_rows = [r for name, _, r in rows if name == "train"]
    assert len(train_rows) == 2
    for r in train_rows:
        acts = r["acting"]["actions"]
        assert len(acts) == 1 and isinstance(acts[0], float) and abs(acts[0]) < 3.0
    last = train_rows[-1]                       # (the first row is written while the first rollout is still being acted)
    assert np.isfinite(last["train"]["policy_entropy"]) and np.isfinite(last["train"]["value_loss"])
    assert last["total"]["steps_trained"] >= 4 * 32                           # the first iteration's 4 epochs at the least
    assert last["total"]["episodes"] >= 4                                     # 64 steps of 10-step episodes


def test_env_string_resolves_to_the_host_or_the_device_env(monkeypatch):
    from rltime_amd import train
    from rltime_amd.acting import mountaincar_device_env
    from rltime_amd.acting.mountaincar_env import MountainCarVecEnv
    built = []
    monkeypatch.setattr(mountaincar_device_env, "MountainCarDeviceVecEnv", lambda n, **kw: built.append((n, kw)) or "device env")
    assert train.make_vec_env("MountainCarContinuous-v0", {"max_episode_steps": 40, "device": True}, 16, "cuda", seed=3) == "device env"
    assert train.make_vec_env("MountainCarContinuous-v0", {"device": True}, 2, "cuda") == "device env"
    assert built == [(16, {"max_episode_steps": 40, "device": "cuda", "seed": 3}), (2, {"max_episode_steps": 999, "device": "cuda", "seed": 0})]
    for args in ({"max_episode_steps": 40}, {"max_episode_steps": 40, "device": False}, None):
        env = train.make_vec_env("MountainCarContinuous-v0", args, 4, "cuda")
        assert isinstance(env, MountainCarVecEnv) and env.max_episode_steps == (40 if args else 999)
    assert len(built) == 2
    with pytest.raises(ValueError, match="extra_features"):
        train.make_vec_env("MountainCarContinuous-v0", {"device": True, "extra_features": True}, 4, "cuda")
    with pytest.raises(ValueError, match="unknown env_args"):
        train.make_vec_env("MountainCarContinuous-v0", {"frame_shape": [4, 84, 84]}, 4, "cuda")
    with pytest.raises(ValueError, match="MountainCarContinuous-v0"):
        train.make_vec_env("Pendulum-v0", None, 4, "cuda")                   # the list of shipped envs names the new one
    assert len(built) == 2


def test_device_env_needs_a_gpu_device():
    from rltime_amd.acting.mountaincar_device_env import MountainCarDeviceVecEnv
    with pytest.raises(ValueError, match="GPU only"):
        MountainCarDeviceVecEnv(4, device="cpu")


@pytest.mark.parametrize("trainer", ["dqn", "dist_dqn", "iqn"])
def test_q_learning_trainers_refuse_a_box_action_space(trainer):
    """Before optimizer or history exist: the trainer has neither attribute when the ValueError arrives."""
    from rltime_amd import train
    config = _small(_config())
    config["training"] = {"type": trainer, "args": {
        "gamma": 0.99, "nstep_train": 1, "lr": 1e-3, "total_steps": 64, "mbatch_size": 8,
        "history_mode": {"type": "replay", "args": {"size": 100, "train_frequency": 4}}}}
    seen = {}
    with pytest.raises(ValueError, match="Discrete action space"):
        train.train(config, device="cpu", on_trainer=lambda t: seen.setdefault("t", t))
    assert not hasattr(seen["t"], "optimizer") and not hasattr(seen["t"], "history_buffer")


@pytest.mark.parametrize("history", ["replay", "prioritized_replay"])
def test_actor_critic_trainers_refuse_a_replay_history_for_box_actions(history):
    from rltime_amd import train
    config = _small(_config(), history_mode={"type": history, "args": {"size": 100, "train_frequency": 4}})
    seen = {}
    with pytest.raises(ValueError, match="Box action space needs history_mode type 'online'"):
        train.train(config, device="cpu", on_trainer=lambda t: seen.setdefault("t", t))
    assert not hasattr(seen["t"], "optimizer") and not hasattr(seen["t"], "history_buffer")


def test_evaluator_and_greedy_acting_refuse_a_box_action_space():
    from rltime_amd.acting.evaluator import Evaluator
    from rltime_amd.acting.mountaincar_env import MountainCarVecEnv
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    env = MountainCarVecEnv(2, max_episode_steps=10)
    config = _config()
    pol = ActorCriticPolicy.create(model_config=config["model"], observation_space=env.observation_space,
                                   action_space=env.action_space, cuda=False)
    with pytest.raises(ValueError, match="not Discrete"):
        Evaluator(pol, env, 4)
    state = pol.make_input_state(env.reset(), np.array([True, True]))
    with pytest.raises(ValueError, match="force_best"):
        pol.actor_predict(state, timesteps=1, force_best=True)
    out = pol.actor_predict(state, timesteps=1)
    assert out["actions"].shape == (2, 1) and out["actions"].dtype == np.float32 and out["action_log_probs"].shape == (2,)
