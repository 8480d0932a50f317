"""GPU: A2C / PPO acting on the fused vector step (acting.extra_args.fused_step; acting/fast_step.py with the actor-critic head,
history/online_device.py as its sink).

  4. the fused step against the policy's own evaluation and against the generic device path, on `synthetic-atari` (its frames,
     rewards and dones do not depend on the actions, so both paths see one stream);
  5. a rollout captured into one graph against the same steps issued one by one (MIRL_ROLLOUT_GRAPH=0), through three
     iterations of feed + get_train_data on Catch;
  6. catch_ppo_fused.json / catch_ppo_lstm_fused.json run two learner iterations with the new kernels in the launch table;
  7. catch_ppo.json without the opt-in still takes the generic path and launches neither new kernel."""
import copy
import json
import math

import numpy as np
import pytest
import torch

from tests import actor_critic_restate as R
from tests import pointwise_restate as PR

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-4, 2e-5            # what tests/test_fast_acting_gpu.py grants the same merged GEMM
NATURE = {"type": "cnn", "args": {"channels_last": True, "layers": [
    {"filters": 32, "kernel": 8, "stride": 4}, {"filters": 64, "kernel": 4, "stride": 2}, {"filters": 64, "kernel": 3, "stride": 1}]}}
LSTM, FC = {"type": "lstm", "args": {"num_units": 64}}, {"type": "fc", "args": {"fc_size": 64}}
MODELS = {"cnn-fc": [NATURE, FC], "cnn-lstm": [NATURE, LSTM], "cnn-lstm-fc": [NATURE, LSTM, FC]}


def _profile(on):
    from rltime_amd import _lib
    if on:
        _lib.check(_lib.lib.mirl_profile_reset())
    _lib.check(_lib.lib.mirl_profile_set(2 if on else 0))


def _ran():
    from rltime_amd import _lib
    return {r["name"]: r["calls"] for r in _lib.profile_table()}


# ---- 4. the fused step against the policy's own evaluation ---------------------------------------------------------------------------
def _synthetic_actor(model, planes, E, fused):
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.synthetic_env import SyntheticAtariVecEnv
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    torch.manual_seed(0)
    env = SyntheticAtariVecEnv(E, frame_shape=(planes, 84, 84), n_actions=6, seed=5, done_prob=0.05)
    pol = ActorCriticPolicy.create(model_config={"type": "sequential", "args": {"layer_configs": MODELS[model]}},
                                   observation_space=env.observation_space, action_space=env.action_space, cuda=True)
    actor = Actor(env, device=True, use_graph=True, fused_actor_critic=fused)
    actor.set_actor_policy(pol)
    return actor, pol


def _stored_tree(step, model, H=64):
    tree = {"x": step["frames"], "layer0_state": {}, "layer1_state": {}}
    if "lstm" in model:
        tree["layer1_state"] = {"hx": step["state"][:, :H].contiguous(), "cx": step["state"][:, H:].contiguous(), "initials": step["initials"]}
    if model == "cnn-lstm-fc":
        tree["layer2_state"] = {}
    return tree


def _act(actor, pol, E):
    """1 + 3 steps, a weight change, 4 steps -> (8 vector steps, policies [before, after] the change, the Philox step word
    the action of vector step 1 was drawn at)."""
    steps = list(actor.get_samples(E).vector_steps)
    word = int(actor._fast.rng_step) if actor._fast else None
    steps += actor.get_samples(3 * E).vector_steps
    before = copy.deepcopy(pol)
    with torch.no_grad():
        pol.actor.logits_layer.weight.mul_(4.0)
        pol.critic.bias.add_(0.5)
    steps += actor.get_samples(4 * E).vector_steps
    return steps, [before, copy.deepcopy(pol)], word


@pytest.mark.parametrize("model,planes", [("cnn-fc", 4), ("cnn-lstm", 4), ("cnn-lstm-fc", 4), ("cnn-lstm", 1)])
def test_fused_step_equals_the_policys_own_evaluation(model, planes):
    E, A = 8, 6
    fa, fpol = _synthetic_actor(model, planes, E, True)
    ga, gpol = _synthetic_actor(model, planes, E, False)
    fused, pols, word = _act(fa, fpol, E)
    generic, _, _ = _act(ga, gpol, E)
    fs = fa._fast
    assert fs and fs.ac and ga._fast is False and len(fused) == len(generic) == 8
    rec = "lstm" in model
    rows, excluded, seen = 0, 0, set()
    for i in range(1, 8):                                  # 7 vector steps, each chosen in the state the step before stored
        a, b, prev = fused[i], generic[i], fused[i - 1]
        for key in ("frames", "rewards", "dones") + (("initials",) if rec else ()):
            assert torch.equal(a[key], b[key]), (i, key)
        assert ("state" in a) == ("state" in b) == rec and tuple(a["policy"].shape) == (E, 2) and a["actions"].dtype == torch.int32
        if rec:
            np.testing.assert_allclose(a["state"].cpu().numpy(), b["state"].cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg="state %d" % i)
            assert torch.all(a["state"][a["dones"].bool()] == 0)
        np.testing.assert_allclose(a["policy"][:, 1].cpu().numpy(), b["policy"][:, 1].cpu().numpy(), rtol=RTOL, atol=ATOL,
                                   err_msg="value %d" % i)
        pol = pols[0] if i <= 3 else pols[1]               # steps 4.. were selected after the weight change
        with torch.no_grad():
            logits, values = pol.get_logits_and_state_value(_stored_tree(prev, model), 1)
        acts = a["actions"].long()
        want_lp = torch.log_softmax(logits.double(), dim=1).gather(1, acts.unsqueeze(1)).squeeze(1)
        np.testing.assert_allclose(a["policy"][:, 0].cpu().numpy(), want_lp.cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg="logp %d" % i)
        np.testing.assert_allclose(a["policy"][:, 1].cpu().numpy(), values.cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg="own value %d" % i)
        # the action: the restatement's inverse CDF of those logits on the Philox uniform of (seed, step, env)
        u = PR.philox_head_draws(fs.rng_seed, word + i - 1, E, A)[0].numpy()
        z = logits.float().cpu().numpy()
        want_a, _ = R.head(z, u)
        margin, bound = R.head_margin(z, u)
        S = R.softmax_parts(z)[3]
        clear = margin > RTOL * S + bound
        rows, excluded = rows + E, excluded + int((~clear).sum())
        assert np.array_equal(acts.cpu().numpy()[clear], want_a[clear]), i
        seen.update(acts.tolist())
    print("FIGURE fused-ac %s planes=%d rows excluded near a CDF boundary: %d of %d" % (model, planes, excluded, rows))
    assert excluded <= 0.02 * rows
    assert len(seen) >= 2
    # the change of weights reached the step: the value moved by the critic's bias
    shift = float((fused[4]["policy"][:, 1] - pols[0].get_logits_and_state_value(_stored_tree(fused[3], model), 1)[1].detach()).mean())
    assert abs(shift - 0.5) < 1e-3
    fa.close()
    ga.close()


# ---- 5. the rollout graph against the per-step path ------------------------------------------------------------------------------------
def _catch_actor_and_history(T):
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.catch_env import CatchVecEnv
    from rltime_amd.general.config import load_config
    from rltime_amd.history.online_device import DeviceOnlineHistory
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    torch.manual_seed(11)
    env = CatchVecEnv(4, device="cuda", seed=0, frame_shape=(4, 84, 84), grid=12, n_actions=3)
    pol = ActorCriticPolicy.create(model_config=load_config("catch_ppo.json")["model"], observation_space=env.observation_space,
                                   action_space=env.action_space, cuda=True)
    actor = Actor(env, device=True, use_graph=True, fused_actor_critic=True)
    actor.set_actor_policy(pol)

    def discount(nstep, reward, policy_output):
        raise AssertionError("the device history evaluates the return itself")
    discount.gamma, discount.lam = 0.99, 0.95
    hist = DeviceOnlineHistory(nstep_target=T, nstep_train=T, discount_function=discount)
    actor.set_sink(hist, clip_rewards=True)
    return actor, hist


def _leaves(tree, path=""):
    if isinstance(tree, dict):
        for k, v in tree.items():
            yield from _leaves(v, path + "." + k)
    else:
        yield path, tree


def test_rollout_graph_equals_the_per_step_path(monkeypatch):
    T, E = 8, 4
    runs = []
    for graph in ("1", "0"):
        monkeypatch.setenv("MIRL_ROLLOUT_GRAPH", graph)
        monkeypatch.setenv("MIRL_ROLLOUT_EAGER_CALLS", "0")
        actor, hist = _catch_actor_and_history(T)
        batches = []
        for it in range(3):
            # (one step until the fused actor has configured the history, whole windows from then on)
            assert hist.needed_feed_count(E, E) == (E if it == 0 else E * T)
            while hist.needed_feed_count(E, E) is not None:
                samples = actor.get_samples(hist.needed_feed_count(E, E))
                assert getattr(samples, "ingested", False) and len(samples) > 0
                assert hist.update(samples) == {"discarded_steps": 0}
            batch = hist.get_train_data(E)
            assert batch is not None and int(hist._head_word) == hist.plan.head
            batches.append({k: v.clone() for k, v in _leaves(batch)})
        fs = actor._fast
        assert fs and fs.ac and fs.rollout_graphs == (graph == "1")
        captured = [key for key, (calls, g) in fs._rollouts.items() if g is not None]
        assert graph == "0" or [calls for key, (calls, g) in fs._rollouts.items() if key[0] == T] == [2]
        runs.append((batches, captured, hist.plan.head))
        actor.close()
        hist.close()
    (ga, cap_a, head_a), (gb, cap_b, head_b) = runs
    assert head_a == head_b == 3 * T
    for x, y in zip(ga, gb):
        assert set(x) == set(y)
        for key in x:
            assert torch.equal(x[key], y[key]), key
    assert cap_b == []
    # exactly one capture per (iters, generation of the sink's rings): 1 + 7 steps of the first window, then 8 + 8 on one graph
    assert len(cap_a) == len({(k[0], k[3]) for k in cap_a}) and sorted(k[0] for k in cap_a) == [1, T - 1, T], cap_a
    assert len({k[3] for k in cap_a}) == 1


# ---- 6. / 7. the configs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["catch_ppo_fused.json", "catch_ppo_lstm_fused.json"])
def test_fused_config_runs_two_iterations(name, tmp_path, monkeypatch):
    """(Launches inside a captured graph are not in the launch table: the rollouts are issued eagerly here, the same launches.)"""
    from rltime_amd.train import train_from_config
    monkeypatch.setenv("MIRL_ROLLOUT_EAGER_CALLS", "1000")
    _profile(True)
    try:
        trainer = train_from_config(name, num_envs=4, log_dir=str(tmp_path), log_name="run", seed=3,
                                    conf_update={"training": {"args": {"nstep_train": 8, "total_steps": 64, "log_freq": 32}}})
        torch.cuda.synchronize()
        ran = _ran()
    finally:
        _profile(False)
    assert type(trainer.history_buffer).__name__ == "DeviceOnlineHistory" and trainer.actors._fast and trainer.actors._fast.ac
    rows = [json.loads(line) for line in open(tmp_path / "run" / "train.json")]
    assert rows and rows[-1]["this_interval"]["steps_trained"] > 0
    for key in ("value_loss", "policy_loss", "policy_entropy", "state_value_mean", "grad_norm"):
        assert math.isfinite(rows[-1]["train"][key]), (key, rows[-1]["train"])
    assert all(bool(torch.isfinite(p).all()) for p in trainer.policy.parameters())
    assert ran.get("k_actor_head_ac_rng", 0) >= 16 and ran.get("k_actor_head_ac", 0) == 0, ran
    assert ran.get("k_online_append", 0) == 16 and ran.get("k_online_window", 0) == 2 and ran.get("k_ac_loss", 0) == 32, ran


def test_default_config_is_unchanged(tmp_path):
    from rltime_amd.train import train_from_config
    _profile(True)
    try:
        trainer = train_from_config("catch_ppo.json", num_envs=4, log_dir=str(tmp_path), log_name="run", seed=3,
                                    conf_update={"training": {"args": {"nstep_train": 8, "total_steps": 64, "log_freq": 32}}})
        torch.cuda.synchronize()
        ran = _ran()
    finally:
        _profile(False)
    assert trainer.actors._fast is False and trainer.actors._fused_actor_critic is False
    assert ran.get("k_actor_head_ac", 0) >= 16 and ran.get("k_online_window", 0) == 2
    assert "k_actor_head_ac_rng" not in ran and "k_online_append" not in ran and "k_online_advance" not in ran, ran
