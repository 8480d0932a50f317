"""CPU: mountaincar_continuous_ppo_fused.json loads, differs from mountaincar_continuous_ppo_device.json only by the opt-in
(acting.extra_args.fused_step), and what stays out of scope for it — periodic evaluation, a process group — is refused with its
message before optimizer or history are built."""
import copy

import pytest

from rltime_amd.general.config import load_config, validate_config


def _config(name="mountaincar_continuous_ppo_fused.json"):
    config = copy.deepcopy(load_config(name))
    validate_config(config)
    config.pop("_comment", None)
    return config


def test_fused_config_is_the_device_config_plus_the_opt_in(monkeypatch):
    from rltime_amd import train
    from rltime_amd.acting.mountaincar_env import MountainCarVecEnv
    config, parent = _config(), _config("mountaincar_continuous_ppo_device.json")
    monkeypatch.setattr(train, "make_vec_env", lambda env, env_args, n, device, seed=0: MountainCarVecEnv(n))
    for cfg, want in ((config, True), (parent, False)):          # the key reaches the actor as its flags
        actor = train.create_actors(cfg, device="cpu", device_acting=False)
        assert actor.fused_normal is want and actor._fused_actor_critic is want
    assert config["acting"]["extra_args"].pop("fused_step") is True and config == parent


@pytest.mark.parametrize("case,message", [("eval_episodes", "eval_episodes is not supported with an actor-critic trainer"),
                                          ("process group", "do not run under a process group")])
def test_out_of_scope_settings_are_refused_before_anything_is_built(case, message, monkeypatch):
    """The refusals are the actor-critic trainers' own (training/a2c.py).  This box has no GPU: the policy is built on the CPU and
    answers is_cuda() as the config's device policy would, so that the trainer asks its device-path questions."""
    from rltime_amd import train
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    from rltime_amd.training.a2c import A2C
    group = type("Group", (), {"active": True, "broadcast_parameters": lambda self, p: None, "attach": lambda self, p: None})()
    config = _config()
    config.update(env_args={"max_episode_steps": 10}, policy_args={"cuda": False})
    config["training"]["args"].update(nstep_train=8, total_steps=64, **({"eval_episodes": 4} if case == "eval_episodes" else {}))
    monkeypatch.setattr(ActorCriticPolicy, "is_cuda", lambda self: True)
    monkeypatch.setattr(A2C, "_on_device", lambda self: True)
    seen = []
    with pytest.raises(ValueError, match=message):
        train.train(config, device="cpu", on_trainer=lambda t: seen.append(t) or (case == "process group" and setattr(t, "data_parallel", group)))
    assert not hasattr(seen[0], "optimizer") and not hasattr(seen[0], "history_buffer")
