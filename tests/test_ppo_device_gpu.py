"""GPU: A2C / PPO on the device path, end to end.

(a) one learner_step of A2C and of PPO on a fixed (T = 4, B = 8) batch — a 2x64 MLP on 4-float observations and the nature CNN
    on (4, 36, 36) uint8 frames — against the same step evaluated in float64 on a CPU copy of the policy (targets of
    a2c.py:68-82, loss of oracle.qmath.actor_critic_loss under autograd).  The logged losses equal the restatement of the loss
    kernel on the operands the kernel was given, within the kernel's bounds (tests/actor_critic_restate.py), and the float64
    step's losses within the project's 1e-4; every parameter's gradient within 1e-4 of that parameter's largest entry
    (the per-op bar of docs/parity.md).  The launch table shows the loss kernel: this fails without the feature.
(b) cartpole_ppo_device.json learns: the settings and the bar of tests/test_online_ppo_cpu.py::test_cartpole_ppo_config_trains.
(c) catch_ppo.json runs two learner iterations at 4 envs, T = 8: finite losses, and all three kernels in the launch table."""
import copy
import json
import math

import numpy as np
import pytest
import torch

from tests import actor_critic_restate as R

pytestmark = pytest.mark.gpu

BAR = 1e-4


def _profile(on):
    from rltime_amd import _lib
    if on:
        _lib.check(_lib.lib.mirl_profile_reset())
    _lib.check(_lib.lib.mirl_profile_set(2 if on else 0))


def _ran():
    from rltime_amd import _lib
    return {r["name"]: r["calls"] for r in _lib.profile_table()}


def _trainer(kind, frames):
    from rltime_amd.general.config import load_config
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.general.type_registry import get_registered_type
    from rltime_amd.general.utils import deep_dictionary_update
    from rltime_amd.train import create_actors
    cfg = load_config("cartpole_%s_device.json" % kind)
    deep_dictionary_update(cfg, {"acting": {"actor_envs": 8}, "training": {"args": {"nstep_train": 4, "epochs": 1, "minibatches": 1,
                                                                                   "total_steps": 1000}}})
    if frames:
        cfg["env"], cfg["env_args"] = "catch", {"frame_shape": [4, 36, 36], "grid": 12, "n_actions": 3}
        cfg["model"] = load_config("catch_ppo.json")["model"]
    actors = create_actors(cfg, "cuda")
    tr = get_registered_type("trainers", kind)(logger=NullLogger(echo=False), actors=actors, model_config=cfg["model"],
                                               policy_args=cfg["policy_args"])
    tr.setup(**cfg["training"]["args"])
    return tr


def _batch(tr, frames, T=4, B=8):
    g = torch.Generator().manual_seed(5)
    A = tr.actors.get_spaces()[1].n
    if frames:
        obs = torch.randint(0, 256, (2, T, B, 4, 36, 36), generator=g, dtype=torch.uint8)
    else:
        obs = torch.randn(2, T, B, 4, generator=g) * 0.5
    obs = obs.cuda()
    with torch.no_grad():
        logits, values = tr.policy.get_logits_and_state_value({"x": obs[0].reshape((T * B,) + tuple(obs.shape[3:]))}, 1)
        dist = torch.distributions.Categorical(logits=logits)
        actions = dist.sample()
        logp = dist.log_prob(actions) + torch.randn(T * B, generator=g).cuda() * 0.2        # ratios on both sides of the clip range
    tree = lambda x: {"x": x, "layer0_state": {}, "layer1_state": {}}                        # noqa: E731
    n = torch.tensor([min(4, T - t) for t in range(T)], dtype=torch.float32).unsqueeze(1).expand(T, B).contiguous()
    mask = (torch.rand(T, B, generator=g) > 0.2).float()
    return {"states": tree(obs[0]), "target_states": tree(obs[1]), "returns": (torch.randn(T, B, generator=g) * 0.5).cuda(),
            "nsteps": n.cuda(), "target_masks": mask.cuda(),
            "policy_outputs": {"actions": actions.to(torch.int32).reshape(T, B), "action_log_probs": logp.reshape(T, B),
                               "values": (values + torch.randn(T * B, generator=g).cuda() * 0.1).reshape(T, B)},
            "extra_data": {}}


def _float64_step(tr, ref, batch, frames, kind):
    """The same learner step on the CPU copy in float64 -> (logged scalars, gradients by parameter name)."""
    from oracle import qmath
    flat = lambda x: x.reshape((-1,) + tuple(x.shape[2:])).cpu()                              # noqa: E731
    prep = (lambda x: flat(x).double() * (1.0 / 255.0)) if frames else (lambda x: flat(x).double())
    with torch.no_grad():
        boot = ref.get_state_value({"x": prep(batch["target_states"]["x"])}, 1)
    ret, ns, mk = (flat(batch[k]).double() for k in ("returns", "nsteps", "target_masks"))
    targets = ret + (tr.gamma ** ns) * (tr.advlam ** (ns - 1)) * boot * mk
    po = batch["policy_outputs"]
    lp, vals, ent = ref.evaluate_actions({"x": prep(batch["states"]["x"])}, 1, flat(po["actions"]).long())
    ppo = kind == "ppo"
    total, vloss, gain = qmath.actor_critic_loss(lp, vals, ent, targets, flat(po["values"]).double(),
                                                 flat(po["action_log_probs"]).double() if ppo else None, tr.vf_coef,
                                                 tr._calc_entropy_factor(), tr.adv_norm, tr._calc_clip_value() if ppo else None)
    ref.zero_grad()
    total.backward()
    log = {"value_loss": vloss.item(), "policy_loss": -gain.item(), "policy_entropy": ent.mean().item(), "state_value_mean": vals.mean().item()}
    return log, {k: p.grad.clone() for k, p in ref.named_parameters()}


@pytest.mark.parametrize("frames", [False, True], ids=["mlp", "cnn"])
@pytest.mark.parametrize("kind", ["a2c", "ppo"])
def test_one_learner_step_matches_float64(kind, frames):
    from rltime_amd.training import qops
    tr = _trainer(kind, frames)
    try:
        assert type(tr.history_buffer).__name__ == "DeviceOnlineHistory" and tr.policy.is_cuda() and tr.actors._device_mode
        batch = _batch(tr, frames)
        ref = copy.deepcopy(tr.policy).cpu().double()
        if frames:
            ref.model.layers[0].scale = None              # the float64 copy is fed frames / 255 in float64
        seen = []
        real = qops.ac_loss

        def tap(logits, values, actions, targets, acting_values, **kw):
            seen.append((logits.detach().clone(), values.detach().clone(), actions.clone(), targets.clone(), acting_values.clone(), kw))
            return real(logits, values, actions, targets, acting_values, **kw)
        qops.ac_loss = tap
        _profile(True)
        try:
            tr.value_log.get()
            tr.learner_step({k: (dict(v) if isinstance(v, dict) else v) for k, v in batch.items()}, 4, 4, epochs=1, minibatches=1)
            torch.cuda.synchronize()
            ran = _ran()
        finally:
            qops.ac_loss = real
            _profile(False)
        assert ran.get("k_ac_loss", 0) == 1, ran
        logged = tr.value_log.get()["train"]
        grads = {k: p.grad.detach().cpu().double() for k, p in tr.policy.named_parameters()}
        # the logged losses are the loss kernel's: inside its bounds on the operands it was given
        (logits, values, actions, targets, acting, kw), = seen
        np32 = lambda t: t.float().cpu().numpy()                                              # noqa: E731
        old = kw["old_log_probs"]
        want = R.loss(np32(logits), np32(values), actions.cpu().numpy().astype(np.int64), np32(targets), np32(acting),
                      None if old is None else np32(old), kw["vf_coef"], kw["entropy_factor"], kw["clip_value"], kw["adv_norm"])
        b = R.loss_bounds(want, kw["vf_coef"], kw["entropy_factor"], old is not None)["stats"]
        assert (old is not None) == (kind == "ppo") and kw["adv_norm"] == (kind == "ppo")
        for i, key in ((1, "value_loss"), (2, "policy_loss"), (3, "policy_entropy"), (4, "state_value_mean")):
            ratio = abs(float(logged[key]) - want["stats"][i]) / b[i]
            print("RATIO step.%s %s %s %.4f" % (key, kind, "cnn" if frames else "mlp", ratio))
            assert ratio <= 1.0, key
        # the whole step against float64
        log64, grads64 = _float64_step(tr, ref, batch, frames, kind)
        for key, w in log64.items():
            err = abs(float(logged[key]) - w) / max(abs(w), 1.0)
            print("FIGURE step.%s %s %s rel %.3e" % (key, kind, "cnn" if frames else "mlp", err))
            assert err <= BAR, (key, float(logged[key]), w)
        assert set(grads) == set(grads64)
        for name, w in grads64.items():
            top = float(w.abs().max())
            err = float((grads[name] - w).abs().max()) / max(top, 1e-30)
            print("FIGURE grad %s %s %s rel-to-max %.3e" % (name, kind, "cnn" if frames else "mlp", err))
            assert top > 0 and err <= BAR, name
    finally:
        tr.actors.close()
        tr.history_buffer.close()


def test_cartpole_ppo_device_config_learns(tmp_path):
    import time
    from rltime_amd.train import train_from_config
    t0 = time.time()
    trainer = train_from_config("cartpole_ppo_device.json", num_envs=4, env="CartPole-v1", log_dir=str(tmp_path), log_name="run", seed=1,
                                conf_update={"training": {"args": {"total_steps": 24000, "log_freq": 4000}}})
    wall = time.time() - t0
    assert type(trainer.history_buffer).__name__ == "DeviceOnlineHistory" and trainer.policy.is_cuda() and trainer.actors._device_mode
    rows = [json.loads(line) for line in open(tmp_path / "run" / "train.json")]
    curve = [r["last100"]["reward"] for r in rows]
    print("CURVE cartpole_ppo_device seed 1: %s wall %.1f s" % (["%.1f" % c for c in curve], wall))
    assert len(rows) == 6
    assert rows[-1]["this_interval"]["steps_trained"] > 0 and "policy_entropy" in rows[-1]["train"]
    first, last = curve[0], curve[-1]
    assert last > 2.0 * first and last > 50.0, curve


def test_catch_ppo_config_runs_two_iterations(tmp_path):
    from rltime_amd.train import train_from_config
    _profile(True)
    try:
        trainer = train_from_config("catch_ppo.json", num_envs=4, log_dir=str(tmp_path), log_name="run", seed=3,
                                    conf_update={"training": {"args": {"nstep_train": 8, "total_steps": 64, "log_freq": 32}}})
        torch.cuda.synchronize()
        ran = _ran()
    finally:
        _profile(False)
    assert type(trainer.history_buffer).__name__ == "DeviceOnlineHistory"
    rows = [json.loads(line) for line in open(tmp_path / "run" / "train.json")]
    # (a row is written when the acted steps cross log_freq, before that iteration trains: the second row holds the first iteration)
    assert len(rows) == 2 and rows[-1]["this_interval"]["steps_trained"] == 4 * 32                       # 4 epochs x (4 envs x 8 steps)
    for key in ("value_loss", "policy_loss", "policy_entropy", "state_value_mean", "grad_norm"):
        assert math.isfinite(rows[-1]["train"][key]), (key, rows[-1]["train"])
    assert all(bool(torch.isfinite(p).all()) for p in trainer.policy.parameters())
    # 16 vector steps, 2 windows, 2 iterations x 4 epochs x 4 minibatches
    assert ran.get("k_actor_head_ac", 0) >= 16 and ran.get("k_online_window", 0) == 2 and ran.get("k_ac_loss", 0) == 2 * 16, ran


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graphed"])
def test_device_actor_carries_the_policy_outputs(use_graph):
    """Actor._select for an actor-critic policy: the vector steps carry [log-probability | value] of the action taken, eagerly
    and through GraphedStep; both equal the policy's own evaluation of the state the action was chosen in."""
    from rltime_amd.general.config import load_config
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    from rltime_amd.train import create_actors
    cfg = load_config("cartpole_ppo_device.json")
    cfg["acting"]["actor_envs"] = 5
    actors = create_actors(cfg, "cuda", use_graph=use_graph)
    try:
        obs_space, act_space = actors.get_spaces()
        torch.manual_seed(3)
        policy = ActorCriticPolicy.create(model_config=cfg["model"], observation_space=obs_space, action_space=act_space, cuda=True)
        actors.set_actor_policy(policy)
        _profile(True)
        try:
            steps = actors.get_samples(5 * 6).vector_steps + actors.get_samples(5 * 3).vector_steps
            torch.cuda.synchronize()
            ran = _ran()
        finally:
            _profile(False)
        assert ran.get("k_actor_head_ac", 0) >= 1 and (use_graph or ran["k_actor_head_ac"] == 9)
        assert actors._fast is False and (actors._graphed is not None) == use_graph
        assert len(steps) == 9 and all(tuple(s["policy"].shape) == (5, 2) and s["actions"].dtype == torch.int32 for s in steps)
        seen = set()
        for prev, step in zip(steps[:-1], steps[1:]):
            with torch.no_grad():
                logits, values = policy.get_logits_and_state_value({"x": prev["frames"]}, 1)
                want = torch.distributions.Categorical(logits=logits).log_prob(step["actions"].long())
            assert torch.allclose(step["policy"][:, 0], want, rtol=1e-5, atol=1e-6)
            assert torch.allclose(step["policy"][:, 1], values, rtol=1e-5, atol=1e-6)
            seen.update(step["actions"].tolist())
        assert seen == {0, 1}                      # sampled, not arg-max: both actions of a fresh policy occur within 40 draws
    finally:
        actors.close()


def test_device_path_refuses_what_is_out_of_scope():
    from rltime_amd.general.config import load_config
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.general.type_registry import get_registered_type
    from rltime_amd.general.utils import deep_dictionary_update
    from rltime_amd.train import create_actors

    def run(update, match):
        cfg = load_config("cartpole_ppo_device.json")
        deep_dictionary_update(cfg, {"acting": {"actor_envs": 2}, "training": {"args": {"total_steps": 100}}})
        deep_dictionary_update(cfg, update)
        actors = create_actors(cfg, "cuda")
        try:
            tr = get_registered_type("trainers", "ppo")(logger=NullLogger(echo=False), actors=actors, model_config=cfg["model"],
                                                       policy_args=cfg["policy_args"])
            with pytest.raises(ValueError, match=match):
                tr.setup(**cfg["training"]["args"])
            assert getattr(tr, "history_buffer", None) is None and getattr(tr, "optimizer", None) is None      # nothing was built
        finally:
            actors.close()
    run({"policy_args": {"critic_separate_model": True}}, "critic_separate_model")
    run({"training": {"args": {"history_mode": {"type": "online", "args": {"fixed_target": False}}}}}, "fixed_target")
    run({"training": {"args": {"history_mode": {"type": "replay", "args": {"size": 100, "train_frequency": 1}}}}}, "online")
    for key in ("graph_learner_step", "skip_invalid_steps", "overlap_acting"):
        run({"training": {"args": {key: True}}}, key)
    run({"training": {"args": {"eval_episodes": 4}}}, "eval_episodes")
    lstm = {"type": "sequential", "args": {"layer_configs": [{"type": "fc", "args": {"fc_size": 16}}, {"type": "lstm", "args": {"num_units": 16}}]}}
    run({"model": lstm}, "recurrent")
