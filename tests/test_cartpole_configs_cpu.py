"""CPU: the shipped cartpole_dqn.json / cartpole_iqn.json load, validate and hold the reference's values — written out here
literally from rltime/configs/cartpole_dqn.json, cartpole_iqn.json, cartpole_common.json, models/mlp_2x64.json and
exploration/decay_0.01_50p.json — except for the two documented keys: env_args.device (both) and policy_args.cuda (dqn; the
reference's iqn config already sets it)."""
import copy

import pytest

from rltime_amd.general.config import load_config, validate_config

_TRAINING_ARGS = {
    "gamma": 0.99, "mbatch_size": 128, "nstep_train": 1, "nstep_target": 10, "target_update_freq": 10000,
    "lr": 1e-3, "lr_anneal": True, "warmup_steps": 20000, "total_steps": 500000,
    "history_mode": {"type": "replay", "args": {"size": 10000, "train_frequency": 4}}}
_FC64 = {"type": "fc", "args": {"fc_size": 64}}
REFERENCE = {
    "cartpole_dqn.json": {
        "acting": {"actor_envs": 16,
                   "exploration": {"type": "epsilon_greedy", "args": {"eps_start": 1.0, "eps_final": 0.01, "exploration_fraction": 0.5}},
                   "extra_args": {"use_proc": False}},
        "model": {"type": "sequential", "args": {"layer_configs": [_FC64, _FC64]}},
        "env": "CartPole-v0",
        "env_args": {"max_episode_steps": 1000},
        "policy_args": {"cuda": False},
        "training": {"type": "dqn", "args": _TRAINING_ARGS}},
    "cartpole_iqn.json": {
        "acting": {"actor_envs": 16,
                   "exploration": {"type": "epsilon_greedy", "args": {"eps_start": 1.0, "eps_final": 0.01, "exploration_fraction": 0.5}},
                   "extra_args": {"use_proc": False}},
        "model": {"type": "sequential", "args": {"layer_configs": [_FC64, _FC64]}},
        "env": "CartPole-v0",
        "env_args": {"max_episode_steps": 1000},
        "policy_args": {"cuda": True, "dueling": True},
        "training": {"type": "iqn", "args": _TRAINING_ARGS}},
}


@pytest.mark.parametrize("name", sorted(REFERENCE))
def test_shipped_config_is_the_reference_plus_the_device_keys(name):
    config = load_config(name)
    validate_config(config)
    want = copy.deepcopy(REFERENCE[name])
    want["env_args"]["device"] = True
    want["policy_args"]["cuda"] = True
    assert config == want


def test_device_key_selects_the_device_env(monkeypatch):
    """env_args.device builds CartPoleDeviceVecEnv (with the step limit); without the key the CPU env, as before; the
    extra-features wrapper still refuses every CartPole env."""
    from rltime_amd import train
    from rltime_amd.acting import cartpole_device_env
    from rltime_amd.acting.cartpole_env import CartPoleVecEnv
    built = []
    monkeypatch.setattr(cartpole_device_env, "CartPoleDeviceVecEnv",
                        lambda n, **kw: built.append((n, kw)) or "device env")
    assert train.make_vec_env("CartPole-v0", {"max_episode_steps": 1000, "device": True}, 16, "cuda", seed=3) == "device env"
    assert train.make_vec_env("CartPole-v1", {"device": True}, 2, "cuda") == "device env"
    assert built == [(16, {"max_episode_steps": 1000, "device": "cuda", "seed": 3}), (2, {"max_episode_steps": 500, "device": "cuda", "seed": 0})]
    for args in ({"max_episode_steps": 1000}, {"max_episode_steps": 1000, "device": False}, None):
        env = train.make_vec_env("CartPole-v0", args, 4, "cuda")
        assert isinstance(env, CartPoleVecEnv) and env.max_episode_steps == (1000 if args else 200)
    with pytest.raises(ValueError, match="extra_features"):
        train.make_vec_env("CartPole-v0", {"device": True, "extra_features": True}, 4, "cuda")
    assert len(built) == 2


def test_device_env_needs_a_gpu_device():
    from rltime_amd.acting.cartpole_device_env import CartPoleDeviceVecEnv
    with pytest.raises(ValueError, match="GPU only"):
        CartPoleDeviceVecEnv(4, device="cpu")
