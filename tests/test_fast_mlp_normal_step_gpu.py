"""GPU: PPO acting on the fused MLP vector step under a Normal head (acting/fast_mlp_step.FastMlpNormalStep) on the device
MountainCar, with history/online_device.py as its sink: captured rollouts against the same steps issued one by one; the step's
means and value against the policy's float64 forward within the operation-count bound of docs/parity.md; what the opt-in covers."""
import copy

import numpy as np
import pytest
import torch

from tests import act_mlp_ac_restate as A
from tests import act_mlp_restate as R

pytestmark = pytest.mark.gpu


def _make(fused=True, E=4):
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.mountaincar_device_env import MountainCarDeviceVecEnv
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    env = MountainCarDeviceVecEnv(E, max_episode_steps=7, seed=5)
    torch.manual_seed(0)
    pol = ActorCriticPolicy.create(model_config=A.MLP, observation_space=env.observation_space, action_space=env.action_space, cuda=True)
    with torch.no_grad():
        pol.actor.logstd.fill_(-0.5)                   # (not the initial 0: exp(logstd) takes part)
    actor = Actor(env, device=True, use_graph=True, fused_actor_critic=fused)
    actor.fused_normal = fused                         # as train.create_actors sets it from acting.extra_args.fused_step
    actor._rng_seed = 0xB0C5EED
    actor.set_actor_policy(pol)
    return actor, pol, env


def test_rollout_graph_equals_the_per_step_path(monkeypatch):
    """E = 4, T = 5, three windows (captured rollouts replayed at several ring positions): the same rings, batches, action and
    policy buffers, env records, episodes and action sums as MIRL_ROLLOUT_GRAPH=0; the batch's actions are the float32
    [T B, 1] words the kernel wrote."""
    from rltime_amd.acting.fast_mlp_step import FastMlpNormalStep
    from rltime_amd.history.online_device import DeviceOnlineHistory
    E, T, runs = 4, 5, []
    discount = lambda n, r, po: 0.0                    # noqa: E731  (the device history evaluates the return itself)
    discount.gamma, discount.lam = 0.99, 0.95
    for graph in ("1", "0"):
        monkeypatch.setenv("MIRL_ROLLOUT_GRAPH", graph)
        actor, pol, env = _make()
        hist = DeviceOnlineHistory(nstep_target=T, nstep_train=T, discount_function=discount)
        actor.set_sink(hist)
        seen, total = [], 0.0
        for it in range(3):
            while hist.needed_feed_count(E, E) is not None:
                assert hist.update(actor.get_samples(hist.needed_feed_count(E, E))) == {"discarded_steps": 0}
            head, cap, ring = hist.plan.head, hist.capacity, hist._rings["actions"]
            assert head == T * (it + 1) and ring.dtype == torch.float32 and tuple(ring.shape[1:]) == (E, 1)
            live = torch.as_tensor([s % cap for s in range(max(0, head - cap), head)], device="cuda")
            seen += [r[live].clone() for r in hist._rings.values()]
            batch = hist.get_train_data(E)
            acts = batch["policy_outputs"]["actions"]
            assert acts.dtype == torch.float32 and tuple(acts.reshape(T * E, -1).shape) == (T * E, 1)
            assert torch.equal(acts, ring[live[-T:]][:, torch.as_tensor(hist._served, device="cuda")])
            total += float(acts.double().sum())
            seen += [batch["states"]["x"], batch["returns"], acts, batch["policy_outputs"]["action_log_probs"], batch["policy_outputs"]["values"]]
        fs = actor._fast
        assert isinstance(fs, FastMlpNormalStep) and fs.actions.dtype == torch.float32 and tuple(fs.actions.shape) == (E, 1)
        assert bool(fs._rollouts) == (graph == "1") and all(g is not None for _, g in fs._rollouts.values())      # every rollout captured
        sums, count = actor._tracker.take_action_sums()
        assert count == 3 * T * E and abs(sums[0] - total) < 1e-9       # the tracker's float64 sum: the actions the batches handed out
        seen += [fs.actions.clone(), fs.qvalues.clone(), env.get_state()["records"].cuda(), torch.tensor(sums)]
        runs.append((seen, actor._tracker.drain(wait=True), int(fs.rng_step), fs.step_no))
        actor.close()
    (a, *rest_a), (b, *rest_b) = runs
    assert rest_a == rest_b and len(rest_a[0]) > 0 and len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_means_and_value_within_the_operation_count_bound():
    """E = 16 after three vector steps: the raw row of the step's own refreshed operands against the float64 forward of a copy
    of the policy, element by element within the bound of its three products (tests/act_mlp_restate._dense64: u = 2^-24 per
    operation, ReLU passes a bound on); the value the step stored is the row's last column."""
    from rltime_amd._lib import lib, check, ptr, stream
    actor, pol, env = _make(E=16)
    actor.get_samples(3 * 16)
    fs = actor._fast
    raw, acts, block = torch.empty((16, 2), device="cuda"), torch.empty((16, 1), device="cuda"), torch.empty((16, 2), device="cuda")
    check(lib.mirl_act_mlp_normal_fwd(*fs._ac_args(fs.shape), ptr(fs.x_in), ptr(fs.lwT[0]), ptr(fs.leading[0].bias), None, None,
                                      ptr(fs.fcT), ptr(fs.fc_b), ptr(fs.outT), ptr(fs.out_b), ptr(fs.logstd), fs.rng_seed,
                                      ptr(fs.rng_step), ptr(acts), ptr(block), 2, ptr(raw), None, stream()), "mirl_act_mlp_normal_fwd")
    assert torch.equal(block, fs.qvalues) and torch.equal(acts, fs.actions) and torch.equal(block[:, 1], raw[:, 1])
    p64 = copy.deepcopy(pol).to("cpu").double()
    x = fs.x_in.cpu().double()
    with torch.no_grad():
        mean, _, value = p64.get_mean_logstd_and_state_value(A.input_tree(x), 1)
        f, e_f = x, torch.zeros_like(x)
        for fc in p64.model.layers:
            y, e_f = R._dense64(f, e_f, fc.layers[0][0].weight, fc.layers[0][0].bias)
            f = torch.clamp(y, min=0)
        out, bound = R._dense64(f, e_f, torch.cat([p64.actor.mean_layer.weight, p64.critic.weight]),
                                torch.cat([p64.actor.mean_layer.bias, p64.critic.bias]))
    want = torch.cat([mean, value.unsqueeze(1)], dim=1)
    err = (raw.cpu().double() - want).abs()
    print("FIGURE max |row - f64| %.3g, max err / bound %.3g" % (float(err.max()), float((err / bound).max())))
    assert torch.allclose(out, want, rtol=0, atol=1e-12) and bool((err <= bound).all())
    actor.close()


def test_what_the_opt_in_covers():
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.cartpole_device_env import CartPoleDeviceVecEnv
    from rltime_amd.acting.fast_mlp_step import FastMlpNormalStep
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    from rltime_amd.spaces import Box
    actor, pol, env = _make(fused=False, E=16)          # without the opt-in the actor does not construct the fused step
    assert len(actor.get_samples(2 * 16).vector_steps) == 2 and actor._fast is False and actor._fast_cls is None
    actor.close()
    actor, pol, env = _make(fused=True, E=16)           # with it the shipped shape is covered and acts on the step
    assert FastMlpNormalStep.why_not(actor) is None
    step = actor.get_samples(2 * 16).vector_steps[0]
    assert isinstance(actor._fast, FastMlpNormalStep) and step["actions"].dtype == torch.float32 and tuple(step["actions"].shape) == (16, 1)
    make = lambda e, space: ActorCriticPolicy.create(model_config=A.MLP, observation_space=e.observation_space, action_space=space, cuda=True)  # noqa: E731
    wide = make(env, Box(-np.ones(17, np.float32), np.ones(17, np.float32), (17,), np.float32))
    assert "16 action components" in FastMlpNormalStep.why_not(actor, wide)
    cart = CartPoleDeviceVecEnv(4, seed=1)
    assert "Normal head" in FastMlpNormalStep.why_not(actor, make(cart, cart.action_space))      # a Categorical policy
    actor.close()


def test_fused_config_runs_two_iterations(tmp_path):
    from rltime_amd.acting.fast_mlp_step import FastMlpNormalStep
    from rltime_amd.train import train_from_config
    trainer = train_from_config("mountaincar_continuous_ppo_fused.json", num_envs=4, log_dir=str(tmp_path), log_name="run", seed=3,
                                conf_update={"env_args": {"max_episode_steps": 10},
                                             "training": {"args": {"nstep_train": 8, "total_steps": 64, "log_freq": 32}}})
    fs = trainer.actors._fast
    assert isinstance(fs, FastMlpNormalStep) and fs._rollouts and all(g is not None for _, g in fs._rollouts.values())
    assert type(trainer.history_buffer).__name__ == "DeviceOnlineHistory" and trainer.steps == 64
    assert all(bool(torch.isfinite(p).all()) for p in trainer.policy.parameters())
