"""GPU: the fused MLP acting step (acting/fast_mlp_step.py, Actor(fused_mlp=True)) on the device CartPole: against a
float64 copy of the policy on each step's own observation, the rollout graph against the same launches issued one by one,
and resume.  The pattern is tests/test_fast_acting_gpu.py's."""
import numpy as np
import pytest
import torch

from tests import act_mlp_restate as R

pytestmark = pytest.mark.gpu

MLP = {"type": "sequential", "args": {"layer_configs": [{"type": "fc", "args": {"fc_size": 64}}, {"type": "fc", "args": {"fc_size": 64}}]}}
EXPL = {"type": "epsilon_greedy", "args": {"eps_start": 0.3, "eps_final": 0.3, "exploration_fraction": 0.5}}
E, NQ = 16, 32


def _policy(kind, env):
    from rltime_amd.policies.dqn import DQNPolicy
    from rltime_amd.policies.iqn import IQNPolicy
    torch.manual_seed(0)
    kw = dict(model_config=MLP, observation_space=env.observation_space, action_space=env.action_space, cuda=True)
    if kind == "iqn-dueling":
        return IQNPolicy.create(dueling=True, num_sampling_quantiles=NQ, **kw)      # cartpole_iqn.json: 64 cos features, 32 rows
    return DQNPolicy.create(**kw)


def _make(kind, fused=True, exploration=None, max_episode_steps=200, pol=None, env_seed=5):
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.cartpole_device_env import CartPoleDeviceVecEnv
    env = CartPoleDeviceVecEnv(E, max_episode_steps=max_episode_steps, seed=env_seed)
    pol = pol if pol is not None else _policy(kind, env)
    actor = Actor(env, exploration_config=exploration, device=True, use_graph=True, fused_mlp=fused)
    actor.set_actor_policy(pol)
    return actor, pol, env


@pytest.mark.parametrize("kind", ["dqn", "iqn-dueling"])
def test_fused_step_equals_the_policys_own_evaluation(kind):
    """8 greedy vector steps: the q-values a step carries were computed on the observation before it (the previous step's
    frames, the reset observation for the first) — held to the float64 copy of the policy on that observation within
    max(4 x the policy's own float32 distance, 5e-6 x scale); the actions agree wherever the float64 top-two gap exceeds
    1e-4, with at most one row in eight excluded."""
    from rltime_amd.acting.fast_mlp_step import FastMlpStep
    actor, pol, env = _make(kind)
    fixed = None
    if kind.startswith("iqn"):
        fixed = torch.rand(E * NQ, generator=torch.Generator().manual_seed(9)).cuda()
        pol.tau_source = lambda n: fixed[:n]
    steps = actor.get_samples(E * 3).vector_steps + actor.get_samples(E * 5).vector_steps
    assert isinstance(actor._fast, FastMlpStep) and len(steps) == 8
    obs = actor._reset_obs
    for t, s in enumerate(steps):
        assert s["frames"].dtype == torch.float32 and tuple(s["frames"].shape) == (E, 4) and "state" not in s
        q64 = R.policy_q64(pol, obs, fixed)
        with torch.no_grad():
            own = pol.actor_predict({"x": obs, "layer0_state": {}, "layer1_state": {}}, 1, as_numpy=False)["qvalues"]
        print(kind, t, "err, policy f32 err, scale:", R.check_bar(s["policy"].cpu(), q64, own.cpu()))
        clear = R.clear_rows(q64)
        assert int((~clear).sum()) * 8 <= E, t
        assert torch.equal(s["actions"].cpu().long()[clear], q64.argmax(1)[clear]), t
        obs = s["frames"]
    # the default actor on the same policy keeps the generic graphed path
    pol.tau_source = None
    plain, _, _ = _make(kind, fused=False, pol=pol)
    plain.get_samples(E * 2)
    assert plain._fast is False and plain._graphed is not None


def test_an_uncovered_policy_takes_the_generic_path():
    """The opt-in on a policy the step does not cover (two Linear blocks in one FC module): a warning and the generic path."""
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.cartpole_device_env import CartPoleDeviceVecEnv
    from rltime_amd.acting.fast_mlp_step import FastMlpStep
    from rltime_amd.policies.dqn import DQNPolicy
    env = CartPoleDeviceVecEnv(E, seed=1)
    model = {"type": "sequential", "args": {"layer_configs": [{"type": "fc", "args": {"fc_size": 64, "fc_count": 2}}]}}
    pol = DQNPolicy.create(model_config=model, observation_space=env.observation_space, action_space=env.action_space, cuda=True)
    actor = Actor(env, device=True, use_graph=True, fused_mlp=True)
    actor.set_actor_policy(pol)
    assert not FastMlpStep.supports(actor) and "single Linear" in FastMlpStep.why_not(actor)
    out = actor.get_samples(E * 2)
    assert actor._fast is False and len(out.vector_steps) == 2


def _flat(tree):
    if tree is None:
        return []
    if isinstance(tree, torch.Tensor):
        return [tree]
    return [x for v in (tree.values() if isinstance(tree, dict) else tree) for x in _flat(v)]


@pytest.mark.parametrize("kind", ["dqn", "iqn-dueling"])
def test_rollout_graph_equals_the_per_step_path(kind, monkeypatch):
    """A whole get_samples call from ONE captured graph (env step -> pre-step -> planned ingest -> mirl_act_mlp_fwd, x iters)
    against the same launches issued one by one (MIRL_ROLLOUT_GRAPH=0): the replay (a sampled batch: frames as float32,
    actions, returns, masks; the shard's statistics), the episode statistics, the action histogram and the step counters
    are bit-identical — epsilon-greedy draws and quantile fractions made in the kernel from the device-side step word."""
    from rltime_amd.acting.fast_mlp_step import FastMlpStep
    from rltime_amd.history import ReplayHistoryBuffer
    calls, iters = 7, 6
    results = []
    for mode in ("graph", "eager-then-graph", "per-step"):
        monkeypatch.setenv("MIRL_ROLLOUT_GRAPH", "0" if mode == "per-step" else "1")
        monkeypatch.setenv("MIRL_ROLLOUT_EAGER_CALLS", "2" if mode == "eager-then-graph" else "0")
        actor, pol, env = _make(kind, exploration=EXPL, max_episode_steps=20)
        hist = ReplayHistoryBuffer(size=E * 30, train_frequency=1, nstep_target=3, nstep_train=1, prefix_steps=0, gamma=0.99,
                                   device_rng=True, keep_policy_outputs=False)
        actor.set_sink(hist)
        for c in range(calls):                                     # E * 30 slots, 42 steps per env: evictions included
            s = actor.get_samples(E * iters)
            assert getattr(s, "ingested", False)
            hist.update(s)
            if c == 3:
                with torch.no_grad():                              # a "learner update" between calls: refresh() + reselect()
                    for p in pol.parameters():
                        p.mul_(1.01)
        fs = actor._fast
        assert isinstance(fs, FastMlpStep)
        captured = [v[1] is not None for v in fs._rollouts.values()]
        assert (captured == []) if mode == "per-step" else (captured and all(captured)), (mode, fs._rollouts)
        torch.cuda.synchronize()
        episodes = actor._tracker.drain(wait=True)
        counts = actor._tracker.take_action_counts()
        hist._seed = 77
        batch = hist.get_train_data(64, train_progress=0.5)
        results.append((batch, hist.stats(), episodes, counts, int(fs.rng_step.item()), fs.step_no, env.get_state()["records"]))
        hist.close()
    bb, sb, eb, cb, rb, nb, envb = results[-1]                     # the per-step path
    assert bb["states"]["x"].dtype == torch.float32 and tuple(bb["states"]["x"].shape[-1:]) == (4,)
    for ba, sa, ea, ca, ra, na, enva in results[:-1]:
        assert sa == sb and ea == eb and ca == cb and ra == rb == na == nb
        assert len(ea) > 0 and sum(ca) == E * calls * iters
        assert torch.equal(enva, envb)
        fa, fb = _flat(ba), _flat(bb)
        assert len(fa) == len(fb) > 4
        for x, y in zip(fa, fb):
            assert torch.equal(x, y)


@pytest.mark.parametrize("kind", ["dqn", "iqn-dueling"])
def test_resume_continues_to_the_bit(kind):
    """get_state after two rollouts, set_state into a fresh actor on a fresh env: two more rollouts on each leave the same
    actions, q-values, observations, rewards, dones, env records and episode rows."""
    from rltime_amd.history import ReplayHistoryBuffer
    iters = 6
    kw = dict(size=E * 30, train_frequency=1, nstep_target=3, nstep_train=1, prefix_steps=0, gamma=0.99, device_rng=True,
              keep_policy_outputs=True)

    def snapshot(actor, env):
        fs = actor._fast
        torch.cuda.synchronize()
        return ([t.clone() for t in (fs.actions, fs.qvalues, fs.x_in, fs.rewards, fs.dones, fs.rng_step)],
                env.get_state()["records"].clone(), actor._tracker.drain(wait=True), fs.step_no)

    a, pol, env_a = _make(kind, exploration=EXPL, max_episode_steps=20)
    hist_a = ReplayHistoryBuffer(**kw)
    a.set_sink(hist_a)
    for _ in range(2):
        hist_a.update(a.get_samples(E * iters))
    torch.cuda.synchronize()
    a._tracker.drain(wait=True)
    state = a.get_state()
    b, _, env_b = _make(kind, exploration=EXPL, max_episode_steps=20, pol=pol, env_seed=5)
    hist_b = ReplayHistoryBuffer(**kw)
    b.set_sink(hist_b)
    b.set_state(state)
    assert torch.equal(env_b.get_state()["records"], env_a.get_state()["records"])
    for _ in range(2):
        hist_a.update(a.get_samples(E * iters))
        hist_b.update(b.get_samples(E * iters))
        (ta, ra, ea, na), (tb, rb, eb, nb) = snapshot(a, env_a), snapshot(b, env_b)
        assert na == nb and ea == eb and torch.equal(ra, rb)
        for x, y in zip(ta, tb):
            assert torch.equal(x, y)
    assert all(v[1] is not None for v in b._fast._rollouts.values()) and len(b._fast._rollouts) >= 1
    hist_a.close()
    hist_b.close()
