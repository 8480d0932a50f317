"""GPU: the Box-action device path end to end — DeviceOnlineHistory with vector actions against the host history, one
learner step of A2C and of PPO with the Normal head against float64, the device actor carrying float actions, and
mountaincar_continuous_ppo_device.json training.

(a) DeviceOnlineHistory fed Box vector steps (float32 actions [E, D]) against OnlineHistoryBuffer on the same stream, the
    pattern of tests/test_online_device_gpu.py at E = 3, T = 4, D = 1 and 2.
(b) one learner_step on a fixed (T = 4, B = 8) batch against the same step in float64 on a CPU copy of the policy running the
    plain-torch expression (evaluate_actions + oracle.qmath.actor_critic_loss under autograd): logged losses within the
    project's 1e-4, every parameter's gradient — logstd's among them — within 1e-4 of that parameter's largest entry (the rule
    of tests/test_ppo_device_gpu.py).  The launch table shows the Normal loss kernel: this fails without the feature.
(c) the device actor hands float32 actions [E, 1] and the [log-probability | value] block to the history, use_graph off and on.
(d) the shipped device config runs two iterations with all three kernels in the launch table, and learns (see the test)."""
import copy
import json
import math

import numpy as np
import pytest
import torch

from tests import test_online_device_gpu as O
from tests import test_ppo_device_gpu as P

pytestmark = pytest.mark.gpu

BAR = P.BAR


# ---- (a) history -------------------------------------------------------------------------------------------------------------
def _box_step(seed, t, E, D):
    s = O._step(seed, t, E, "f32")
    s["obs"] = np.ascontiguousarray(s["obs"][:, :2])                     # this env's 8-byte rows
    s["actions"] = np.random.RandomState(31 * seed + t).randn(E, D).astype(np.float32) * 1.5
    return s


@pytest.mark.parametrize("D", [1, 2])
def test_device_history_with_box_actions_equals_the_host_history(D):
    from rltime_amd.history.online_device import DeviceOnlineHistory
    from rltime_amd.history.online_history import OnlineHistoryBuffer
    E, T = 3, 4
    rng = np.random.RandomState(90 + D)
    batches = 0
    for case, (n, delay) in enumerate([(4, 5000), (2, 9)]):
        kw = dict(max_delayed_steps=delay, fixed_target=True, nstep_target=n, nstep_train=T)
        dev = DeviceOnlineHistory(discount_function=O._gae(), **kw)
        host = OnlineHistoryBuffer(discount_function=O._gae(), **kw)
        mag = OnlineHistoryBuffer(discount_function=O._gae(absolute=True), **kw)
        t = 0
        for _ in range(24):
            if rng.rand() < 0.7:
                steps = [_box_step(100 * D + case, t + i, E, D) for i in range(int(rng.randint(1, 4)))]
                t += len(steps)
                a, b = dev.update(O._device_samples(steps, E)), host.update(O._dicts(steps, E))
                mag.update(O._dicts(steps, E, absolute=True))
                assert a == b
                continue
            for B in (E - 1, E, E + 1):
                a, b, m = dev.get_train_data(B), host.get_train_data(B), mag.get_train_data(B)
                assert (a is None) == (b is None)
                if a is None:
                    continue
                batches += 1
                acts = a["policy_outputs"]["actions"]
                assert acts.dtype == torch.float32 and tuple(acts.shape) == (T, B, D) and acts.is_cuda
                O._compare(a, b, np.asarray(m["returns"], dtype=np.float64), "box D=%d case=%d B=%d" % (D, case, B))
        assert dev._rings["actions"].dtype == torch.float32 and tuple(dev._rings["actions"].shape[1:]) == (E, D)
        dev.close()
    assert batches >= 4


# ---- (b) one learner step ----------------------------------------------------------------------------------------------------
def _trainer(kind):
    from rltime_amd.general.config import load_config
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.general.type_registry import get_registered_type
    from rltime_amd.general.utils import deep_dictionary_update
    from rltime_amd.train import create_actors
    cfg = load_config("mountaincar_continuous_ppo_device.json")
    deep_dictionary_update(cfg, {"acting": {"actor_envs": 8}, "env_args": {"max_episode_steps": 40},
                                 "training": {"args": {"nstep_train": 4, "epochs": 1, "minibatches": 1, "total_steps": 1000}}})
    if kind == "a2c":
        cfg["training"]["type"] = "a2c"
        cfg["training"]["args"].pop("clip_value")
    actors = create_actors(cfg, "cuda")
    tr = get_registered_type("trainers", kind)(logger=NullLogger(echo=False), actors=actors, model_config=cfg["model"],
                                               policy_args=cfg["policy_args"])
    tr.setup(**cfg["training"]["args"])
    return tr


def _batch(tr, T=4, B=8):
    g = torch.Generator().manual_seed(5)
    obs = (torch.randn(2, T, B, 2, generator=g) * torch.tensor([0.5, 0.03])).cuda()
    with torch.no_grad():
        tr.policy.actor.logstd.copy_(torch.tensor([-0.3]))                # (away from 0: exp(2 logstd) matters)
        mean, logstd, values = tr.policy.get_mean_logstd_and_state_value({"x": obs[0].reshape(T * B, 2)}, 1)
        dist = torch.distributions.Normal(mean, logstd.exp().expand_as(mean))
        actions = dist.sample()
        logp = dist.log_prob(actions).sum(-1) + torch.randn(T * B, generator=g).cuda() * 0.2      # ratios on both sides of the clip range
    tree = lambda x: {"x": x, "layer0_state": {}, "layer1_state": {}}                        # noqa: E731
    n = torch.tensor([min(4, T - t) for t in range(T)], dtype=torch.float32).unsqueeze(1).expand(T, B).contiguous()
    mask = (torch.rand(T, B, generator=g) > 0.2).float()
    return {"states": tree(obs[0]), "target_states": tree(obs[1]), "returns": (torch.randn(T, B, generator=g) * 0.5).cuda(),
            "nsteps": n.cuda(), "target_masks": mask.cuda(),
            "policy_outputs": {"actions": actions.reshape(T, B, 1), "action_log_probs": logp.reshape(T, B),
                               "values": (values + torch.randn(T * B, generator=g).cuda() * 0.1).reshape(T, B)},
            "extra_data": {}}


def _float64_step(tr, ref, batch, kind):
    from oracle import qmath
    flat = lambda x: x.reshape((-1,) + tuple(x.shape[2:])).cpu()                              # noqa: E731
    with torch.no_grad():
        boot = ref.get_state_value({"x": flat(batch["target_states"]["x"]).double()}, 1)
    ret, ns, mk = (flat(batch[k]).double() for k in ("returns", "nsteps", "target_masks"))
    targets = ret + (tr.gamma ** ns) * (tr.advlam ** (ns - 1)) * boot * mk
    po = batch["policy_outputs"]
    lp, vals, ent = ref.evaluate_actions({"x": flat(batch["states"]["x"]).double()}, 1, flat(po["actions"]).double())
    assert ent.shape == (lp.shape[0], 1)
    ppo = kind == "ppo"
    total, vloss, gain = qmath.actor_critic_loss(lp, vals, ent, targets, flat(po["values"]).double(),
                                                 flat(po["action_log_probs"]).double() if ppo else None, tr.vf_coef,
                                                 tr._calc_entropy_factor(), tr.adv_norm, tr._calc_clip_value() if ppo else None)
    ref.zero_grad()
    total.backward()
    log = {"value_loss": vloss.item(), "policy_loss": -gain.item(), "policy_entropy": ent.mean().item(), "state_value_mean": vals.mean().item()}
    return log, {k: p.grad.clone() for k, p in ref.named_parameters()}


@pytest.mark.parametrize("kind", ["a2c", "ppo"])
def test_one_learner_step_matches_float64(kind):
    tr = _trainer(kind)
    try:
        assert type(tr.history_buffer).__name__ == "DeviceOnlineHistory" and tr.policy.is_cuda() and tr.actors._device_mode
        assert tr.policy.has_normal_head() and tr.policy.why_not_on_device() is None
        batch = _batch(tr)
        ref = copy.deepcopy(tr.policy).cpu().double()
        P._profile(True)
        try:
            tr.value_log.get()
            tr.learner_step({k: (dict(v) if isinstance(v, dict) else v) for k, v in batch.items()}, 4, 4, epochs=1, minibatches=1)
            torch.cuda.synchronize()
            ran = P._ran()
        finally:
            P._profile(False)
        assert ran.get("k_ac_loss_normal", 0) == 1 and ran.get("k_ac_loss", 0) == 0, ran
        logged = tr.value_log.get()["train"]
        grads = {k: p.grad.detach().cpu().double() for k, p in tr.policy.named_parameters()}
        log64, grads64 = _float64_step(tr, ref, batch, kind)
        for key, w in log64.items():
            err = abs(float(logged[key]) - w) / max(abs(w), 1.0)
            print("FIGURE box step.%s %s rel %.3e" % (key, kind, err))
            assert err <= BAR, (key, float(logged[key]), w)
        assert set(grads) == set(grads64) and "actor.logstd" in grads64
        for name, w in grads64.items():
            top = float(w.abs().max())
            err = float((grads[name] - w).abs().max()) / max(top, 1e-30)
            print("FIGURE box grad %s %s rel-to-max %.3e" % (name, kind, err))
            assert top > 0 and err <= BAR, name
    finally:
        tr.actors.close()
        tr.history_buffer.close()


# ---- (c) the device actor ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graphed"])
def test_device_actor_carries_float_actions_and_the_policy_outputs(use_graph):
    from rltime_amd.general.config import load_config
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    from rltime_amd.train import create_actors
    cfg = load_config("mountaincar_continuous_ppo_device.json")
    cfg["acting"]["actor_envs"] = 5
    cfg["env_args"]["max_episode_steps"] = 4
    actors = create_actors(cfg, "cuda", use_graph=use_graph)
    try:
        obs_space, act_space = actors.get_spaces()
        torch.manual_seed(3)
        policy = ActorCriticPolicy.create(model_config=cfg["model"], observation_space=obs_space, action_space=act_space, cuda=True)
        actors.set_actor_policy(policy)
        P._profile(True)
        try:
            steps = actors.get_samples(5 * 6).vector_steps + actors.get_samples(5 * 3).vector_steps
            torch.cuda.synchronize()
            ran = P._ran()
        finally:
            P._profile(False)
        assert ran.get("k_actor_head_normal", 0) >= 1 and (use_graph or ran["k_actor_head_normal"] == 9)
        assert ran.get("k_mountaincar_env_step", 0) >= 9 and ran.get("k_actor_head_ac", 0) == 0
        assert actors._fast is False and (actors._graphed is not None) == use_graph
        assert len(steps) == 9
        assert all(tuple(s["policy"].shape) == (5, 2) and s["actions"].dtype == torch.float32 and tuple(s["actions"].shape) == (5, 1)
                   and tuple(s["frames"].shape) == (5, 2) for s in steps)
        assert any(bool(s["dones"].any()) for s in steps)
        for prev, step in zip(steps[:-1], steps[1:]):
            with torch.no_grad():
                mean, logstd, values = policy.get_mean_logstd_and_state_value({"x": prev["frames"]}, 1)
                want = torch.distributions.Normal(mean, logstd.exp().expand_as(mean)).log_prob(step["actions"]).sum(-1)
            assert torch.allclose(step["policy"][:, 0], want, rtol=1e-5, atol=1e-6)
            assert torch.allclose(step["policy"][:, 1], values, rtol=1e-5, atol=1e-6)
        acts = torch.cat([s["actions"] for s in steps]).reshape(-1)
        assert float(acts.std()) > 0.3                                     # sampled with std 1, not the mean
        # the tracker beside the episode statistics: per-component sums and the transition count
        sums, count = actors._tracker.take_action_sums()
        assert count == 45 and abs(sums[0] - float(acts.double().sum())) < 1e-9
    finally:
        actors.close()


# ---- (d) the shipped config --------------------------------------------------------------------------------------------------
def test_device_config_runs_two_iterations(tmp_path):
    from rltime_amd.general.config import load_config, validate_config
    from rltime_amd.train import train_from_config
    cfg = load_config("mountaincar_continuous_ppo_device.json")
    validate_config(cfg)
    host = load_config("mountaincar_continuous_ppo.json")
    assert cfg["env_args"] == {"device": True} and cfg["policy_args"] == {"cuda": True}
    assert all(cfg[k] == host[k] for k in ("acting", "model", "env", "training"))
    P._profile(True)
    try:
        trainer = train_from_config("mountaincar_continuous_ppo_device.json", num_envs=4, log_dir=str(tmp_path), log_name="run", seed=3,
                                    conf_update={"env_args": {"max_episode_steps": 6},
                                                 "training": {"args": {"nstep_train": 8, "total_steps": 64, "log_freq": 32}}})
        torch.cuda.synchronize()
        ran = P._ran()
    finally:
        P._profile(False)
    assert type(trainer.history_buffer).__name__ == "DeviceOnlineHistory"
    rows = [json.loads(line) for line in open(tmp_path / "run" / "train.json")]
    assert len(rows) == 2 and rows[-1]["this_interval"]["steps_trained"] == 4 * 32                       # 4 epochs x (4 envs x 8 steps)
    for key in ("value_loss", "policy_loss", "policy_entropy", "state_value_mean", "grad_norm"):
        assert math.isfinite(rows[-1]["train"][key]), (key, rows[-1]["train"])
    assert all(bool(torch.isfinite(p).all()) for p in trainer.policy.parameters())
    assert float(trainer.policy.actor.logstd.detach().abs().max()) > 0.0
    for r in rows:                                                            # the mean of the action component, not a histogram
        assert len(r["acting"]["actions"]) == 1 and abs(r["acting"]["actions"][0]) < 3.0
    assert rows[-1]["total"]["episodes"] >= 4
    # 16 vector steps, 2 windows, 2 iterations x 4 epochs x 4 minibatches
    assert ran.get("k_actor_head_normal", 0) >= 16 and ran.get("k_online_window", 0) == 2 and ran.get("k_ac_loss_normal", 0) == 2 * 16, ran
    assert ran.get("k_mountaincar_env_step", 0) >= 16
