"""GPU: the fused acting vector step (acting/fast_step.py + csrc/acting.hip k_actor_pre,
in-kernel-RNG head) and the one-launch ingest (csrc/replay.hip k_ingest_fused) against the
generic device path they replace (reference order: rltime/acting/actor.py:108-147,
history.py:123-176)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NATURE = {"type": "cnn", "args": {"channels_last": True, "layers": [
    {"filters": 32, "kernel": 8, "stride": 4}, {"filters": 64, "kernel": 4, "stride": 2}, {"filters": 64, "kernel": 3, "stride": 1}]}}
MODEL = {"type": "sequential", "args": {"layer_configs": [
    NATURE, {"type": "lstm", "args": {"num_units": 64}}, {"type": "fc", "args": {"fc_size": 64}}]}}
MODEL_FF = {"type": "sequential", "args": {"layer_configs": [NATURE, {"type": "fc", "args": {"fc_size": 64}}]}}       # no recurrent layer
EXPL = {"type": "epsilon_greedy", "args": {"eps_start": 0.3, "eps_final": 0.3, "exploration_fraction": 0.5}}


def _make(kind, E, fast, exploration=None, seed=5, use_graph=True):
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.synthetic_env import SyntheticAtariVecEnv
    from rltime_amd.policies.dqn import DQNPolicy
    from rltime_amd.policies.iqn import IQNPolicy
    torch.manual_seed(0)
    env = SyntheticAtariVecEnv(E, frame_shape=(4, 84, 84), n_actions=6, seed=seed, done_prob=0.05)
    # kind: dqn | iqn [-ff: CNN -> FC, the T = 1 configs' model] [-plain: no dueling value stream]
    kw = dict(model_config=MODEL_FF if "-ff" in kind else MODEL, observation_space=env.observation_space, action_space=env.action_space,
              dueling="-plain" not in kind)
    pol = IQNPolicy.create(embedding_dim=16, num_sampling_quantiles=8, **kw) if kind.startswith("iqn") else DQNPolicy.create(**kw)
    if kind.startswith("iqn"):
        g = torch.Generator().manual_seed(9)
        fixed = torch.rand(E * 8, generator=g).cuda()
        pol.tau_source = lambda n: fixed[:n]                 # the same quantile fractions on both paths
    actor = Actor(env, exploration_config=exploration, device=True, use_graph=use_graph)
    actor.fast_step = fast
    actor.set_actor_policy(pol)
    return actor, pol, env


@pytest.mark.parametrize("kind", ["dqn", "iqn", "dqn-ff", "iqn-ff", "dqn-ff-plain", "iqn-ff-plain"])
def test_fused_step_matches_the_generic_device_path(kind):
    """Greedy acting (no exploration noise): the fused step and the generic graph path emit the same
    frames / rewards / dones, the same actions, and q-values / stored recurrent state within the
    rounding of one merged GEMM ([features | h] x [W_ih | W_hh]^T)."""
    E, steps = 32, 7
    outs = []
    for fast in (True, False):
        actor, pol, env = _make(kind, E, fast)
        batch = actor.get_samples(E * 3)
        more = actor.get_samples(E * (steps - 3))            # a second call: re-selection with the "current" weights
        assert (actor._fast is not None and actor._fast is not False) == fast
        outs.append(batch.vector_steps + more.vector_steps)
    assert len(outs[0]) == len(outs[1]) == steps
    for t, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a["frames"], b["frames"]) and torch.equal(a["dones"], b["dones"]), t
        assert torch.equal(a["rewards"], b["rewards"]), t
        np.testing.assert_allclose(a["policy"].cpu().numpy(), b["policy"].cpu().numpy(), rtol=2e-4, atol=2e-5, err_msg="q %d" % t)
        assert ("state" in a) == ("state" in b) == ("-ff" not in kind)
        if "-ff" not in kind:
            assert torch.equal(a["initials"], b["initials"]), t
            np.testing.assert_allclose(a["state"].cpu().numpy(), b["state"].cpu().numpy(), rtol=2e-4, atol=2e-5, err_msg="state %d" % t)
        # actions agree wherever the greedy choice is not a near-tie
        q = b["policy"].cpu()
        top2 = q.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 1e-4
        assert torch.equal(a["actions"].cpu()[clear], b["actions"].cpu()[clear]), t
        # a reset env stores a zero recurrent state
        assert "-ff" in kind or torch.all(a["state"][a["dones"].bool()] == 0)


def test_fused_step_epsilon_greedy_draws():
    """In-kernel Philox draws: the explored fraction matches epsilon, random actions are uniform,
    different steps / envs draw differently, and greedy envs still take the arg-max."""
    E = 256
    actor, pol, env = _make("dqn", E, True, exploration=EXPL)
    steps = actor.get_samples(E * 40).vector_steps
    acts = torch.stack([s["actions"] for s in steps]).cpu()
    greedy = torch.stack([s["policy"].argmax(1) for s in steps]).cpu().to(torch.int32)
    explored = (acts != greedy).float().mean().item()
    # per-actor epsilon = eps ** (1 + i / (N - 1) * 7): between eps^8 and eps; random picks hit the greedy action 1 / 6 of the time
    expo = actor._exploration._device_exponents(actor._env_ids, acts.device).cpu().double()
    want = ((0.3 ** expo).clamp(min=actor._exploration.eps_min) * (5.0 / 6.0)).mean().item()
    assert abs(explored - want) < 0.02, (explored, want)
    rand_acts = acts[acts != greedy]
    counts = torch.bincount(rand_acts.long(), minlength=6).float()
    assert counts.min() > 0 and (counts.max() / counts.sum()) < 0.4
    assert not torch.equal(acts[3], acts[4])


@pytest.mark.parametrize("per", [False, True])
def test_direct_ingest_equals_tensor_hand_over(per):
    """Actor.set_sink: the fused step writing straight into the replay leaves exactly the shard that
    feeding the same DeviceSamples through History.update leaves (frames, state, scalars, tree)."""
    from rltime_amd.history import PrioritizedReplayHistoryBuffer, ReplayHistoryBuffer
    E, calls = 16, 5
    shards = []
    for direct in (True, False):
        actor, pol, env = _make("dqn", E, True)
        kw = dict(size=E * 40, train_frequency=4, nstep_target=2, nstep_train=4, prefix_steps=2, gamma=0.99,
                  device_rng=True, keep_policy_outputs=True)
        hist = PrioritizedReplayHistoryBuffer(alpha=0.9, beta=0.6, **kw) if per else ReplayHistoryBuffer(**kw)
        if direct:
            actor.set_sink(hist)
        for _ in range(calls):
            s = actor.get_samples(E * 6)
            assert bool(getattr(s, "ingested", False)) == direct
            hist.update(s)
        batch = hist.get_train_data(8, train_progress=0.5)
        shards.append((batch, hist.stats(), hist.tree_nodes() if per else None))
        hist.close()
    (ba, sa, ta), (bb, sb, tb) = shards
    assert sa == sb
    flat = lambda tree: [tree] if isinstance(tree, torch.Tensor) else [x for v in (tree.values() if isinstance(tree, dict) else tree) for x in flat(v)] if tree is not None else []   # noqa: E731
    for x, y in zip(flat(ba), flat(bb)):
        assert torch.equal(x, y)
    if per:
        for x, y in zip(ta, tb):
            assert np.array_equal(x, y)


def test_in_kernel_quantile_fractions():
    """mirl_cos_embed_rng: tau ~ U[0, 1) drawn in the kernel (Philox keyed by seed, step, row) and the
    cos features of exactly those taus (iqn.py:76-81); a new step draws new fractions."""
    from rltime_amd._lib import lib, check
    rows, D = 8192, 64
    freq = (torch.arange(1, D + 1, dtype=torch.float32, device="cuda") * np.pi).contiguous()
    step = torch.tensor([3], dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                     # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for s in (3, 3, 4):
        step.fill_(s)
        phi = torch.empty((rows, D), device="cuda")
        tau = torch.empty(rows, device="cuda")
        check(lib.mirl_cos_embed_rng(rows, D, 1234, p(step), p(freq), p(phi), p(tau), st))
        outs.append((phi, tau))
    assert torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][1], outs[2][1])
    phi, tau = outs[0]
    assert 0.0 <= float(tau.min()) and float(tau.max()) < 1.0
    assert abs(float(tau.mean()) - 0.5) < 0.02 and abs(float(tau.var()) - 1.0 / 12.0) < 0.01
    hist = torch.histc(tau, bins=16, min=0, max=1)
    assert float(hist.min()) > rows / 16 * 0.8
    want = torch.cos(freq * tau.unsqueeze(1))
    assert torch.allclose(phi, want, rtol=0, atol=2e-6)


@pytest.mark.parametrize("done_prob", [0.02, 0.4])
def test_dedup_newest_plane_ingest_equals_verified_whole_stacks(done_prob):
    """De-duplicated storage fed (a) whole stacks, verified against the ring (k_dedup_depth), (b) only the
    newest plane of every stack + the primed reset observation (mirl_ingest.newest_plane_only), (c) whole
    stacks into a plain shard: the same gathered batches, bit for bit — episodes that end inside an env's
    first steps (done_prob 0.4) included."""
    from rltime_amd.acting.synthetic_env import SyntheticAtariVecEnv
    from rltime_amd.history import ReplayHistoryBuffer
    E, steps = 6, 70
    env = SyntheticAtariVecEnv(E, frame_shape=(4, 84, 84), n_actions=4, seed=11, done_prob=done_prob, frame_stack=True)
    obs0 = env.reset()
    kw = dict(size=E * 50, train_frequency=0, nstep_target=2, nstep_train=3, prefix_steps=1, gamma=0.99, device_rng=True,
              keep_policy_outputs=False)
    bufs = [ReplayHistoryBuffer(frame_stack_dedup=True, **kw), ReplayHistoryBuffer(frame_stack_dedup=True, **kw), ReplayHistoryBuffer(**kw)]
    example = {"x": obs0[0].cpu().numpy()}
    for b in bufs:
        b.configure(example, E, 0)
    bufs[1].prime_stack(obs0)
    g = torch.Generator(device="cuda").manual_seed(1)
    for t in range(steps):
        actions = torch.randint(0, 4, (E,), dtype=torch.int32, device="cuda", generator=g)
        obs, rewards, dones, _ = env.step_device(actions)
        obs = obs.contiguous()
        d8 = dones.to(torch.uint8)
        for i, b in enumerate(bufs):
            b.update_batch(obs, actions, rewards.float(), d8, newest_plane_only=(i == 1))
    batches = []
    for b in bufs:
        b._seed = 77
        batches.append(b.get_train_data(16))
        b.close()
    for k in ("returns", "nsteps", "target_masks"):
        assert torch.equal(batches[0][k], batches[2][k]) and torch.equal(batches[1][k], batches[2][k])
    for key in ("states", "target_states"):
        assert torch.equal(batches[0][key]["x"], batches[2][key]["x"]), "verified whole-stack form"
        assert torch.equal(batches[1][key]["x"], batches[2][key]["x"]), "newest-plane form"


@pytest.mark.parametrize("kind,per", [("dqn", True), ("iqn", False), ("iqn", True), ("dqn-ff-plain", False), ("iqn-ff", True)])
def test_rollout_graph_equals_the_per_step_path(kind, per, monkeypatch):
    """A whole get_samples call from ONE captured HIP graph (FastActingStep.rollout: env step -> pre-step kernel ->
    planned ingest -> input layer -> network -> head, x iters; host bookkeeping planned ahead by
    mirl_replay_ingest_plan) against the same steps issued one by one (MIRL_ROLLOUT_GRAPH=0): the replay shard (rings,
    scalars, priority tree, free list), a sampled batch, the episode statistics and the action histogram are
    bit-identical — with epsilon-greedy draws and IQN quantile fractions made inside the kernels from the device-side
    step counter.  Reference order of one step: rltime/acting/actor.py:108-147, history.py:123-176."""
    from rltime_amd.history import PrioritizedReplayHistoryBuffer, ReplayHistoryBuffer
    E, calls, iters = 16, 7, 6
    results = []
    # "graph, selection redone every call": the weight buffers and the pending selection are rebuilt before every call
    # instead of only after a learner update (actor._fast_steps keeps them while the parameters' version counters stand
    # still) — the re-selection is idempotent, so nothing may change
    for mode in ("graph", "eager-then-graph", "graph, selection redone every call", "per-step"):
        monkeypatch.setenv("MIRL_ROLLOUT_GRAPH", "0" if mode == "per-step" else "1")
        monkeypatch.setenv("MIRL_ROLLOUT_EAGER_CALLS", "2" if mode == "eager-then-graph" else "0")
        actor, pol, env = _make(kind, E, True, exploration=EXPL)
        if kind.startswith("iqn"):
            pol.tau_source = None                                  # quantile fractions drawn in the kernel (Philox, step counter)
        kw = dict(size=E * 30, train_frequency=4, nstep_target=2, nstep_train=4, prefix_steps=2, gamma=0.99,
                  device_rng=True, keep_policy_outputs=False)
        if "-ff" in kind:                                          # transitions, not sequences: the T = 1 configs
            kw.update(nstep_train=1, prefix_steps=0, nstep_target=3, train_frequency=1)      # (the quota guard allows 100 batches of drift)
        hist = PrioritizedReplayHistoryBuffer(alpha=0.9, beta=0.6, **kw) if per else ReplayHistoryBuffer(**kw)
        actor.set_sink(hist)
        for c in range(calls):                                     # E * 30 slots, 42 steps per env: evictions included
            if mode.endswith("every call") and actor._fast:
                actor._fast.selected_with = None
            s = actor.get_samples(E * iters)
            assert getattr(s, "ingested", False)
            hist.update(s)
            if c == 3:
                with torch.no_grad():                              # a "learner update" between calls: refresh() + reselect()
                    for p in pol.parameters():
                        p.mul_(1.01)
        fs = actor._fast
        captured = [v[1] is not None for v in fs._rollouts.values()]
        assert (captured == []) if mode == "per-step" else (captured and all(captured)), (mode, fs._rollouts)
        torch.cuda.synchronize()
        episodes = actor._tracker.drain(wait=True)
        counts = actor._tracker.take_action_counts()
        batch = hist.get_train_data(8, train_progress=0.5)
        results.append((batch, hist.stats(), hist.tree_nodes() if per else None, hist.free_slots() if per else None,
                        episodes, counts, int(fs.rng_step.item()), fs.step_no))
        hist.close()
    flat = lambda tree: [tree] if isinstance(tree, torch.Tensor) else [x for v in (tree.values() if isinstance(tree, dict) else tree) for x in flat(v)] if tree is not None else []   # noqa: E731
    (bb, sb, tb, fb, eb, cb, rb, nb) = results[-1]                 # the per-step path
    for (ba, sa, ta, fa, ea, ca, ra, na) in results[:-1]:
        assert sa == sb and ea == eb and ca == cb and ra == rb == na == nb
        assert len(ea) > 0 and sum(ca) == E * calls * iters
        for x, y in zip(flat(ba), flat(bb)):
            assert torch.equal(x, y)
        if per:
            assert np.array_equal(fa, fb)
            for x, y in zip(ta, tb):
                assert np.array_equal(x, y)


def test_synthetic_env_steps_are_a_function_of_seed_and_step():
    """csrc/acting.hip k_synth_env_step: the env's step counter lives on the device and advances once per launch;
    frames cycle through the pool, rewards / dones are Philox draws of (seed, step, env) with the configured
    probabilities; step_into (static buffers) and step_device (fresh tensors) are the same stream."""
    from rltime_amd.acting.synthetic_env import SyntheticAtariVecEnv
    E = 64
    a = SyntheticAtariVecEnv(E, frame_shape=(4, 84, 84), seed=3, done_prob=0.1)
    b = SyntheticAtariVecEnv(E, frame_shape=(4, 84, 84), seed=3, done_prob=0.1)
    obs = torch.empty((E, 4, 84, 84), dtype=torch.uint8, device="cuda")
    rew = torch.empty(E, device="cuda")
    don = torch.empty(E, dtype=torch.uint8, device="cuda")
    rs, ds = [], []
    for t in range(1, 300):
        o1, r1, d1, _ = a.step_device(None)
        b.step_into(obs, rew, don)
        assert torch.equal(o1, obs) and torch.equal(r1, rew) and torch.equal(d1.view(torch.uint8), don)
        assert torch.equal(o1, a._pool[t % a._pool.shape[0]])
        rs.append(r1.clone()); ds.append(d1.clone())          # noqa: E702
    assert int(a._clock[a._slot].item()) == 299 and a._slot == 1 and int(a._clock[0].item()) == 298
    r, d = torch.stack(rs).cpu(), torch.stack(ds).cpu().float()
    assert abs(float((r == -1).float().mean()) - 0.1) < 0.01 and abs(float((r == 1).float().mean()) - 0.1) < 0.01
    assert abs(float(d.mean()) - 0.1) < 0.01
    assert not torch.equal(rs[0], rs[1])
    st = a.get_state()
    nxt = a.step_device(None)
    a.set_state(st)
    again = a.step_device(None)
    assert all(torch.equal(x, y) for x, y in zip(nxt[:3], again[:3]))


def test_refused_rollout_plan_leaves_the_book_untouched():
    """mirl_replay_ingest_plan is transactional (csrc/replay.hip): a call it refuses — more steps than the plan buffer was
    sized for, an env id outside the shard — returns MIRL_ERR_ARG BEFORE the host bookkeeping moves (History.update's ring
    heads, FIFO, free list: history.py:123-176), so per-step ingest can go on; a planned step then still lands where the
    per-step path would have put it."""
    from rltime_amd import _lib
    from rltime_amd.history import PrioritizedReplayHistoryBuffer
    E = 8
    kw = dict(size=E * 30, train_frequency=4, nstep_target=2, nstep_train=4, prefix_steps=2, gamma=0.99, device_rng=True,
              keep_policy_outputs=False, alpha=0.9, beta=0.6)
    bufs = [PrioritizedReplayHistoryBuffer(**kw), PrioritizedReplayHistoryBuffer(**kw)]
    example = {"x": np.zeros((4, 84, 84), np.uint8)}
    for b in bufs:
        b.configure(example, E, 0)
    g = torch.Generator(device="cuda").manual_seed(3)

    def step():
        return (torch.randint(0, 256, (E, 4, 84, 84), dtype=torch.uint8, device="cuda", generator=g),
                torch.randint(0, 6, (E,), dtype=torch.int32, device="cuda", generator=g),
                torch.randn(E, device="cuda", generator=g), (torch.rand(E, device="cuda", generator=g) < 0.1).to(torch.uint8))
    steps = [step() for _ in range(12)]
    a, b = bufs
    a.plan_ingest(4, E)                                        # sizes the plan buffer: 64 steps of E transitions
    for k in range(4):
        a.ingest_planned(k, *steps[k])
    before = a.stats()
    for bad in (lambda: a.plan_ingest(100, E), lambda: a.plan_ingest(4, E, env_ids=np.arange(E) + 1)):
        with pytest.raises(_lib.MirlError) as err:
            bad()
        assert err.value.code == _lib.MIRL_ERR_ARG
        assert a.stats() == before
    for k in range(4, 12):                                     # per-step ingest goes on after the refusals
        a.update_batch(*steps[k])
    for k in range(12):
        b.update_batch(*steps[k])
    assert a.stats() == b.stats()
    for x, y in zip(a.tree_nodes(), b.tree_nodes()):
        assert np.array_equal(x, y)
    a._seed = b._seed = 5
    ba, bb = a.get_train_data(4, 0.5), b.get_train_data(4, 0.5)
    assert torch.equal(ba["states"]["x"], bb["states"]["x"]) and torch.equal(ba["returns"], bb["returns"])
    for buf in bufs:
        buf.close()
