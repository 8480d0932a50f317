"""CPU: the actor-critic configs and the trainers' refusals that need no GPU.

The device configs are the shipped CPU configs with exactly two keys changed; catch_ppo.json carries the reference's
atari_ppo.json hyper-parameters; the training switches that the actor-critic trainers do not cover are refused before
anything is built; the device history has no CPU fallback."""
import pytest

from rltime_amd.general.config import load_config, validate_config


@pytest.mark.parametrize("kind", ["ppo", "a2c"])
def test_device_config_is_the_cpu_config_with_two_keys_changed(kind):
    cpu, dev = load_config("cartpole_%s.json" % kind), load_config("cartpole_%s_device.json" % kind)
    validate_config(dev)
    assert cpu["policy_args"] == {"cuda": False} and dev["policy_args"] == {"cuda": True}
    assert dev["env_args"] == dict(cpu["env_args"], device=True)
    for key in set(cpu) | set(dev):
        if key not in ("policy_args", "env_args", "_comment"):
            assert cpu[key] == dev[key], key


def test_catch_ppo_carries_the_reference_atari_ppo_settings():
    cfg = load_config("catch_ppo.json")
    validate_config(cfg)
    assert cfg["env"] == "catch" and cfg["acting"]["actor_envs"] == 16 and cfg["policy_args"] == {"cuda": True}
    assert cfg["model"] == load_config("models/nature_cnn_fc512.json")
    assert cfg["training"] == {"type": "ppo", "args": {
        "clip_rewards": True, "gamma": 0.99, "nstep_train": 128, "entropy_factor": 1e-2, "lr": 2.5e-4, "lr_anneal": True,
        "clip_value": 0.2, "clip_anneal": True, "epochs": 4, "minibatches": 4, "advlam": 0.95, "vf_coef": 0.5, "clip_grad": 0.5,
        "total_steps": 50000000}}


@pytest.mark.parametrize("key", ["graph_learner_step", "skip_invalid_steps", "overlap_acting"])
def test_actor_critic_trainers_refuse_the_switches_they_do_not_cover(key):
    from rltime_amd.train import train_from_config
    with pytest.raises(ValueError, match=key):
        train_from_config("cartpole_ppo.json", num_envs=2, conf_update={"training": {"args": {key: True, "total_steps": 64}}})


def test_online_plan_serves_round_robin_and_discards():
    """The host bookkeeping of the device history on its own (online_history.py:61-120): the `not last_env` restart, envs
    without a full sequence are passed over, an env over max_delayed_steps loses its oldest transitions."""
    from rltime_amd.history.online_device import OnlinePlan
    plan = OnlinePlan(nstep_train=2, max_delayed_steps=6)
    for _ in range(4):
        assert plan.feed(range(3)) == 0
    assert plan.serve(1) == [(0, 0, 1)] and plan.last_env == 0
    assert plan.serve(1) == [(0, 2, 0)] and plan.last_env == 0            # `not 0`: the walk restarts at the first env
    assert [e for e, _, _ in plan.serve(2)] == [1, 2] and plan.last_env == 2
    assert plan.serve(1) == [(1, 2, 0)]                                    # after env 2 comes env 0 (empty) -> env 1
    assert plan.serve(2) is None and plan.sequences_ready() == 1
    lost = [plan.feed(range(3)) for _ in range(7)]
    assert lost == [0, 0, 0, 0, 1, 1, 3] and plan.pending == {0: 6, 1: 6, 2: 6} and plan.live_steps() == 7


def test_device_history_has_no_cpu_fallback():
    from rltime_amd import _lib
    if _lib.device_count() > 0:
        return
    from rltime_amd.general.type_registry import get_registered_type
    cls = get_registered_type("history", "online_device")
    with pytest.raises(_lib.MirlError, match="no CPU fallback"):
        cls(nstep_target=1, nstep_train=1)
