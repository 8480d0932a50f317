"""GPU: the extra-features observation on the device — csrc/acting.hip k_extra_features behind mirl_extra_features_step against
the reference wrapper's rows (tests/golden/extra_features_cases.npz, bit for bit), the env wrapper
(acting/extra_features.py), and the fast acting step taking the rows into the LSTM product (acting/fast_step.py) against the
generic device path, the per-step path and a resumed run."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests.extra_features_restate import ExtraFeatures, feature_size

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extra_features_cases.npz")
SENTINEL = -559038737                      # 0xDEADBEEF as int32: no feature row holds this bit pattern
GUARD = 32                                 # elements before and after the compact block
ERR_ARG = -1

NATURE = {"type": "cnn", "args": {"channels_last": True, "layers": [
    {"filters": 32, "kernel": 8, "stride": 4}, {"filters": 64, "kernel": 4, "stride": 2}, {"filters": 64, "kernel": 3, "stride": 1}]}}
MODEL = {"type": "sequential", "args": {"layer_configs": [
    NATURE, {"type": "lstm", "args": {"num_units": 64}}, {"type": "fc", "args": {"fc_size": 64}}]}}
MODEL_FF = {"type": "sequential", "args": {"layer_configs": [NATURE, {"type": "fc", "args": {"fc_size": 64}}]}}
EXPL = {"type": "epsilon_greedy", "args": {"eps_start": 0.3, "eps_final": 0.3, "exploration_fraction": 0.5}}


@pytest.fixture(scope="module")
def cases():
    with np.load(GOLDEN) as z:
        out = {k: z[k] for k in z.files}
    out["params"] = json.loads(str(out["params"]))
    return out


def _flags(p):
    return int(p["include_action"]), int(p["include_reward"]), int(p["include_timestep"])


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tile(cases, k, E):
    """The case's stream over E envs, env e delayed by (3 e) % 5 steps so that neighbours differ: before its stream starts
    and after it ends an env is fed done = 1 (with a garbage action and reward), which yields the fixture's reset row.
    -> actions, rewards, dones [G, E] and the wanted rows [G, E, X], all from the fixture."""
    p = cases["params"][k]
    T, rows = p["T"], cases["c%d_rows" % k]
    G = T + 4
    j = np.arange(G)[:, None] - ((3 * np.arange(E)) % 5)[None, :]
    valid = (j >= 0) & (j < T)
    jc = np.clip(j, 0, T - 1)
    actions = np.where(valid, cases["c%d_actions" % k][jc], 7).astype(np.int32)
    rewards = np.where(valid, cases["c%d_rewards" % k][jc], np.float32(9.5)).astype(np.float32)
    dones = np.where(valid, cases["c%d_dones" % k][jc], 1).astype(np.uint8)
    want = np.where(valid[:, :, None], rows[1 + jc], rows[0][None, None, :]).astype(np.float32)
    return actions, rewards, dones, want


@pytest.mark.parametrize("mode", ["both", "compact", "pitched"])
@pytest.mark.parametrize("E", [1, 3, 65, 257])
def test_kernel_equals_the_reference_rows(cases, E, mode):
    """Every fixture case step by step through the C-ABI: each step writes a compact block and a pitched block of its own
    (sentinel-filled, the compact one between guard bands), so that after the last step every row ever written is compared
    with the reference's, and every byte outside the X columns with the sentinel."""
    from rltime_amd._lib import lib, check
    col0, tail = 7, 5
    for k, p in enumerate(cases["params"]):
        A, X = p["A"], cases["c%d_rows" % k].shape[1]
        actions, rewards, dones, want = _tile(cases, k, E)
        G = actions.shape[0]
        # the NumPy restatement on the tiled stream: the same rows, and the counters the kernel must end with
        ef = ExtraFeatures(E, A, *[bool(f) for f in _flags(p)], p["clip_reward"], p["timestep_scale"])
        first = ef.reset()
        assert np.array_equal(first.view(np.uint32), np.broadcast_to(cases["c%d_rows" % k][0], (E, X)).view(np.uint32))
        for s in range(G):
            got = ef.step(actions[s], rewards[s], dones[s])
            assert np.array_equal(got.view(np.uint32), want[s].view(np.uint32)), (k, s)
        a_d, r_d, d_d = (torch.from_numpy(v).cuda() for v in (actions, rewards, dones))
        counters = torch.full((E,), 12345, dtype=torch.int32, device="cuda")          # the first launch (dones all 1) resets them
        pitch = col0 + X + tail
        block = E * X + 2 * GUARD
        compact = torch.full((G + 1, block), SENTINEL, dtype=torch.int32, device="cuda")
        pitched = torch.full((G + 1, E, pitch), SENTINEL, dtype=torch.int32, device="cuda")
        ones = torch.ones(E, dtype=torch.uint8, device="cuda")

        def launch(s, a, r, d):
            cp = C.c_void_p(compact.data_ptr() + 4 * (s * block + GUARD)) if mode != "pitched" else None
            pp = C.c_void_p(pitched.data_ptr() + 4 * s * E * pitch) if mode != "compact" else None
            check(lib.mirl_extra_features_step(E, A, *_flags(p), int(p["clip_reward"]), float(p["timestep_scale"]), C.c_void_p(a.data_ptr()),
                                               C.c_void_p(r.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(counters.data_ptr()), cp, pp,
                                               pitch, col0, _st()), "mirl_extra_features_step")

        launch(0, a_d[0], r_d[0], ones)                                              # every env starts an episode
        for s in range(G):
            launch(s + 1, a_d[s], r_d[s], d_d[s])
        torch.cuda.synchronize()
        full = np.concatenate([np.broadcast_to(first, (1, E, X)), want]).view(np.int32)
        c_h, p_h = compact.cpu().numpy(), pitched.cpu().numpy()
        if mode != "pitched":
            assert np.array_equal(c_h[:, GUARD:GUARD + E * X].reshape(G + 1, E, X), full), k
            assert np.all(c_h[:, :GUARD] == SENTINEL) and np.all(c_h[:, GUARD + E * X:] == SENTINEL), k
        else:
            assert np.all(c_h == SENTINEL), k
        if mode != "compact":
            assert np.array_equal(p_h[:, :, col0:col0 + X], full), k
            assert np.all(p_h[:, :, :col0] == SENTINEL) and np.all(p_h[:, :, col0 + X:] == SENTINEL), k
        else:
            assert np.all(p_h == SENTINEL), k
        assert np.array_equal(counters.cpu().numpy(), ef.counters), k


def test_out_of_range_actions_set_no_element_and_write_nothing_else():
    from rltime_amd._lib import lib, check
    E, A, col0, tail = 70, 6, 3, 9
    X = feature_size(A)
    pitch = col0 + X + tail
    actions = np.tile(np.array([-1, A, 1 << 30, -2 ** 31, 2, 0, A + 1], np.int64), E // 7).astype(np.int32)
    rewards = np.linspace(-2, 2, E).astype(np.float32)
    dones = np.zeros(E, np.uint8)
    ef = ExtraFeatures(E, A)
    ef.counters[:] = 41
    want = ef.step(actions, rewards, dones)
    assert np.all(want[actions >= A, :A] == 0) and np.all(want[actions < 0, :A] == 0) and want[4, 2] == 1
    a_d, r_d, d_d = (torch.from_numpy(v).cuda() for v in (actions, rewards, dones))
    counters = torch.full((E,), 41, dtype=torch.int32, device="cuda")
    compact = torch.full((E * X + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    pitched = torch.full((E, pitch), SENTINEL, dtype=torch.int32, device="cuda")
    p_ = lambda t: C.c_void_p(t.data_ptr())            # noqa: E731
    check(lib.mirl_extra_features_step(E, A, 1, 1, 1, 1, 1e-5, p_(a_d), p_(r_d), p_(d_d), p_(counters),
                                       C.c_void_p(compact.data_ptr() + 4 * GUARD), p_(pitched), pitch, col0, _st()), "mirl_extra_features_step")
    torch.cuda.synchronize()
    c_h, p_h = compact.cpu().numpy(), pitched.cpu().numpy()
    assert np.array_equal(c_h[GUARD:GUARD + E * X].reshape(E, X), want.view(np.int32))
    assert np.all(c_h[:GUARD] == SENTINEL) and np.all(c_h[GUARD + E * X:] == SENTINEL)
    assert np.array_equal(p_h[:, col0:col0 + X], want.view(np.int32))
    assert np.all(p_h[:, :col0] == SENTINEL) and np.all(p_h[:, col0 + X:] == SENTINEL)
    assert np.all(counters.cpu().numpy() == 42)
    # refused before any launch: the row would not fit the pitch, a negative column, a null input
    args = [E, A, 1, 1, 1, 1, 1e-5, p_(a_d), p_(r_d), p_(d_d), p_(counters), None, p_(pitched), pitch, col0, _st()]
    for pos, bad in ((13, col0 + X - 1), (14, -1), (14, pitch - X + 1), (7, None), (8, None), (9, None), (10, None), (0, 0), (1, 0), (5, 2)):
        a = list(args)
        a[pos] = bad
        assert lib.mirl_extra_features_step(*a) == ERR_ARG, pos
    torch.cuda.synchronize()
    assert np.array_equal(pitched.cpu().numpy(), p_h) and np.all(counters.cpu().numpy() == 42)


# ---- the wrapper and the fast acting step ------------------------------------------------------------------------------------
def _make(kind, env_kind, E, fast, exploration=None, seed=5, extra_args=None, model=None, done_prob=0.3):
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.catch_env import CatchVecEnv
    from rltime_amd.acting.extra_features import ExtraFeaturesVecEnv
    from rltime_amd.acting.synthetic_env import SyntheticAtariVecEnv
    from rltime_amd.policies.dqn import DQNPolicy
    from rltime_amd.policies.iqn import IQNPolicy
    torch.manual_seed(0)
    if env_kind == "catch":
        base = CatchVecEnv(E, frame_shape=(4, 84, 84), grid=6, n_actions=3, seed=seed)        # episodes of 5 steps
    elif env_kind == "flappy":
        # configs/flappy_iqn_lstm.json's game on its (1, 120, 80) frames, the time limit cut to 7 steps so that every env resets
        from rltime_amd.acting.flappy_env import FlappyVecEnv
        from rltime_amd.general.config import load_config
        args = dict(load_config("flappy_iqn_lstm.json")["env_args"])
        assert args.pop("extra_features") is True and args["frame_shape"] == [1, 120, 80]
        args["max_episode_steps"] = 7
        base = FlappyVecEnv(E, device="cuda", seed=seed, **args)
    else:
        # (-stack: the frame-stack contract; such an env has no capturable step, so the fast step goes through step_device)
        base = SyntheticAtariVecEnv(E, frame_shape=(4, 84, 84), n_actions=6, seed=seed, done_prob=done_prob,
                                    frame_stack=env_kind == "synthetic-stack")
    env = ExtraFeaturesVecEnv(base, **(extra_args or {}))
    kw = dict(model_config=model or MODEL, observation_space=env.observation_space, action_space=env.action_space, dueling=True)
    pol = IQNPolicy.create(embedding_dim=16, num_sampling_quantiles=8, **kw) if kind == "iqn" else DQNPolicy.create(**kw)
    if kind == "iqn":
        g = torch.Generator().manual_seed(9)
        fixed = torch.rand(E * 8, generator=g).cuda()
        pol.tau_source = lambda n: fixed[:n]                 # the same quantile fractions on both paths
    actor = Actor(env, exploration_config=exploration, device=True, use_graph=True)
    actor.fast_step = fast
    actor.set_actor_policy(pol)
    return actor, pol, env


def _restate_for(env, E):
    a, r, t = (bool(f) for f in env._flags)
    return ExtraFeatures(E, env.action_space.n, a, r, t, bool(env._clip), env._scale)


def test_wrapper_observation_space_and_reset_rows():
    from rltime_amd.acting.extra_features import ExtraFeaturesVecEnv
    from rltime_amd.train import make_vec_env
    env = make_vec_env("catch", {"frame_shape": [4, 36, 36], "grid": 6, "extra_features": {"timestep_scale": 1. / 7, "use_real_done": False}}, 5, "cuda")
    assert isinstance(env, ExtraFeaturesVecEnv) and env.extra_size == 5
    frames_space, extra_space = env.observation_space.spaces
    assert tuple(frames_space.shape) == (4, 36, 36) and tuple(extra_space.shape) == (5,) and extra_space.dtype == np.float32
    frames, rows = env.reset()
    assert frames.shape == (5, 4, 36, 36) and rows.cpu().tolist() == [[1, 0, 0, 0, 0]] * 5
    ef = _restate_for(env, 5)
    ef.reset()
    for s in range(8):
        acts = torch.tensor([(s + e) % 3 for e in range(5)], dtype=torch.int32, device="cuda")
        (frames, rows), rewards, dones, _ = env.step_device(acts)
        want = ef.step(acts.cpu().numpy(), rewards.cpu().numpy(), dones.cpu().numpy())
        assert np.array_equal(rows.cpu().numpy().view(np.uint32), want.view(np.uint32)), s
    assert np.array_equal(env._counters.cpu().numpy(), ef.counters)
    plain = make_vec_env("synthetic-atari", {"frame_shape": [4, 84, 84]}, 2, "cuda")
    assert not hasattr(plain.observation_space, "spaces")


@pytest.mark.parametrize("kind,env_kind", [("iqn", "synthetic"), ("dqn", "synthetic"), ("iqn", "catch"), ("dqn", "synthetic-stack")])
def test_fast_step_takes_the_extras_and_matches_the_generic_device_path(kind, env_kind):
    """CNN -> LSTM -> FC dueling policies on (frames, extras) observations, greedy: the fast step (extras written by the
    kernel into the LSTM product's input rows, X = 8 padded to 16 / X = 5 padded to 16) against the generic device path
    (the model's torch.cat) on the same weights and streams."""
    from rltime_amd.acting.fast_step import FastActingStep
    E, steps = 6, 12
    outs = []
    for fast in (True, False):
        actor, pol, env = _make(kind, env_kind, E, fast)
        assert pol.model.extra_input_layer == 1
        assert FastActingStep.supports(actor)
        batch = actor.get_samples(E * 5)
        more = actor.get_samples(E * (steps - 5))            # a second call: re-selection on the current input state
        assert (actor._fast is not None and actor._fast is not False) == fast
        if fast:
            fs = actor._fast
            assert fs.X == env.extra_size and fs.Xp == 16 and fs.K == fs.F + 16 + fs.H and fs.f_lstm and fs.f_conv
            pad = fs.xh[:, fs.F + fs.X:fs.F + fs.Xp]
            assert pad.numel() > 0 and torch.all(pad == 0) and torch.all(fs.wcat[:, fs.F + fs.X:fs.F + fs.Xp] == 0)
            assert torch.equal(fs.xh[:, fs.F:fs.F + fs.X], fs.extra)
            assert fs.env_into == (env_kind != "synthetic-stack")
        outs.append((batch.vector_steps + more.vector_steps, env))
    (sa, _), (sb, env_b) = outs
    assert len(sa) == len(sb) == steps
    ef = _restate_for(env_b, E)
    ef.reset()
    n_done = 0
    for t, (a, b) in enumerate(zip(sa, sb)):
        assert torch.equal(a["frames"], b["frames"]) and torch.equal(a["dones"], b["dones"]), t
        assert torch.equal(a["rewards"], b["rewards"]), t
        assert torch.equal(a["actions"].cpu(), b["actions"].cpu()), t
        np.testing.assert_allclose(a["policy"].cpu().numpy(), b["policy"].cpu().numpy(), rtol=2e-4, atol=2e-5, err_msg="q %d" % t)
        assert torch.equal(a["initials"], b["initials"]), t
        np.testing.assert_allclose(a["state"].cpu().numpy(), b["state"].cpu().numpy(), rtol=2e-4, atol=2e-5, err_msg="state %d" % t)
        assert a["extra"].dtype == torch.float32 and torch.equal(a["extra"].view(torch.int32), b["extra"].view(torch.int32)), t
        want = ef.step(b["actions"].cpu().numpy(), b["rewards"].cpu().numpy(), b["dones"].cpu().numpy())
        assert np.array_equal(a["extra"].cpu().numpy().view(np.uint32), want.view(np.uint32)), t
        n_done += int(b["dones"].sum())
    assert n_done >= 6                                       # resets happened


def test_fast_step_on_the_flappy_frames_matches_the_generic_device_path():
    """test_fast_step_takes_the_extras_and_matches_the_generic_device_path on the shipped Flappy set-up: (1, 120, 80) frames +
    extras (X = 4 padded to 16) into configs/flappy_iqn_lstm.json's own model — conv 29 x 19 -> 13 x 8 -> 11 x 6, F = 4224, LSTM
    512, K = 4752 — dueling IQN, 4 envs, greedy, 12 steps over two get_samples calls.  Everything the env and the selection
    produce is identical on the two paths; q-values and the stored state within that test's rtol 2e-4 / atol 2e-5."""
    from rltime_amd.acting.fast_step import FastActingStep
    from rltime_amd.general.config import load_config
    from tests.test_flappy_shapes_cpu import LSTM_F, LSTM_H, LSTM_K, LSTM_X, LSTM_XP
    E, steps = 4, 12
    model = load_config("flappy_iqn_lstm.json")["model"]
    outs = []
    for fast in (True, False):
        actor, pol, env = _make("iqn", "flappy", E, fast, model=model)
        assert pol.model.extra_input_layer == 1
        assert FastActingStep.supports(actor)
        batch = actor.get_samples(E * 5)
        more = actor.get_samples(E * (steps - 5))            # a second call: re-selection on the current input state
        assert (actor._fast is not None and actor._fast is not False) == fast
        if fast:
            fs = actor._fast
            assert (fs.X, fs.Xp, fs.F, fs.H, fs.K) == (LSTM_X, LSTM_XP, LSTM_F, LSTM_H, LSTM_K) == (env.extra_size, 16, 4224, 512, 4752)
            assert fs.f_lstm and fs.f_conv and fs.conv_dims == (29, 19, 13, 8, 11, 6) and fs.y1.shape == (E, 32, 29, 19)
            pad = fs.xh[:, fs.F + fs.X:fs.F + fs.Xp]
            assert pad.numel() > 0 and torch.all(pad == 0) and torch.all(fs.wcat[:, fs.F + fs.X:fs.F + fs.Xp] == 0)
            assert torch.equal(fs.xh[:, fs.F:fs.F + fs.X], fs.extra)
        outs.append((batch.vector_steps + more.vector_steps, env))
    (sa, _), (sb, env_b) = outs
    assert len(sa) == len(sb) == steps
    ef = _restate_for(env_b, E)
    ef.reset()
    n_done = 0
    for t, (a, b) in enumerate(zip(sa, sb)):
        assert a["frames"].shape == (E, 1, 120, 80)
        assert torch.equal(a["frames"], b["frames"]) and torch.equal(a["dones"], b["dones"]), t
        assert torch.equal(a["rewards"], b["rewards"]), t
        assert torch.equal(a["actions"].cpu(), b["actions"].cpu()), t
        np.testing.assert_allclose(a["policy"].cpu().numpy(), b["policy"].cpu().numpy(), rtol=2e-4, atol=2e-5, err_msg="q %d" % t)
        assert torch.equal(a["initials"], b["initials"]), t
        np.testing.assert_allclose(a["state"].cpu().numpy(), b["state"].cpu().numpy(), rtol=2e-4, atol=2e-5, err_msg="state %d" % t)
        assert a["extra"].dtype == torch.float32 and torch.equal(a["extra"].view(torch.int32), b["extra"].view(torch.int32)), t
        want = ef.step(b["actions"].cpu().numpy(), b["rewards"].cpu().numpy(), b["dones"].cpu().numpy())
        assert np.array_equal(a["extra"].cpu().numpy().view(np.uint32), want.view(np.uint32)), t
        n_done += int(b["dones"].sum())
    assert n_done >= E                                       # the 7-step limit at the latest: every env was reset


def _check_batch_extras(batch, ef_factory):
    """A sampled batch of a replay with nstep_target = 1: row t of the target states is the observation that follows step t
    of the sequence, so its extras must be the restatement applied to the stored action, reward (the 1-step return) and
    done (the stored `initials`) of that step, continuing from the counter row t of the states shows."""
    x, xt = batch["states"]["x"], batch["target_states"]["x"]
    assert isinstance(x, tuple) and len(x) == 2 and x[1].dtype == torch.float32
    cur, nxt = x[1].cpu().numpy(), xt[1].cpu().numpy()
    L, B, X = cur.shape
    actions = batch["policy_outputs"]["actions"].cpu().numpy()
    rewards = batch["returns"].cpu().numpy()
    dones = batch["target_states"]["layer1_state"]["initials"].cpu().numpy() if "layer1_state" in batch["target_states"] \
        and "initials" in batch["target_states"]["layer1_state"] else None
    ef = ef_factory(B)
    assert ef.inc == (True, True, True)
    ts_col = ef.A
    checked = 0
    for t in range(L):
        ticks = np.rint(cur[t, :, ts_col].astype(np.float64) / ef.scale).astype(np.int32)
        assert np.array_equal((ticks.astype(np.float64) * ef.scale).astype(np.float32), cur[t, :, ts_col])
        ef.counters = ticks
        d = dones[t] if dones is not None else (nxt[t, :, ts_col] == 0)
        want = ef.step(actions[t].astype(np.int32), rewards[t], d.astype(np.uint8))
        assert np.array_equal(nxt[t].view(np.uint32), want.view(np.uint32)), t
        checked += B
    return checked


@pytest.mark.parametrize("per", [False, True])
def test_rollout_graph_equals_the_per_step_path_with_extras(per, monkeypatch):
    """tests/test_fast_acting_gpu.py test_rollout_graph_equals_the_per_step_path for the recurrent IQN policy on (frames,
    extras) observations: the extras launch rides in the captured rollout; shard, sampled batch (with its `extra` rows),
    episode statistics and counters are bit-identical to the per-step path, and the `extra` rows read back are the
    restatement applied to the stored actions, rewards and dones."""
    from rltime_amd.history import PrioritizedReplayHistoryBuffer, ReplayHistoryBuffer
    E, calls, iters = 16, 7, 6
    results = []
    for mode in ("graph", "eager-then-graph", "per-step"):
        monkeypatch.setenv("MIRL_ROLLOUT_GRAPH", "0" if mode == "per-step" else "1")
        monkeypatch.setenv("MIRL_ROLLOUT_EAGER_CALLS", "2" if mode == "eager-then-graph" else "0")
        actor, pol, env = _make("iqn", "synthetic", E, True, exploration=EXPL, done_prob=0.1)
        pol.tau_source = None                                      # quantile fractions drawn in the kernel
        kw = dict(size=E * 30, train_frequency=4, nstep_target=1, nstep_train=4, prefix_steps=2, gamma=0.99,
                  device_rng=True, keep_policy_outputs=False)
        hist = PrioritizedReplayHistoryBuffer(alpha=0.9, beta=0.6, **kw) if per else ReplayHistoryBuffer(**kw)
        actor.set_sink(hist)
        for c in range(calls):
            s = actor.get_samples(E * iters)
            assert getattr(s, "ingested", False)
            hist.update(s)
            if c == 3:
                with torch.no_grad():                              # a "learner update" between calls
                    for p in pol.parameters():
                        p.mul_(1.01)
        fs = actor._fast
        assert fs.X == 8 and hist._layout.extra_f32 == 8
        captured = [v[1] is not None for v in fs._rollouts.values()]
        assert (captured == []) if mode == "per-step" else (captured and all(captured)), (mode, fs._rollouts)
        torch.cuda.synchronize()
        episodes = actor._tracker.drain(wait=True)
        counts = actor._tracker.take_action_counts()
        batch = hist.get_train_data(8, train_progress=0.5)
        assert _check_batch_extras(batch, lambda B: _restate_for(env, B)) > 0
        results.append((batch, hist.stats(), hist.tree_nodes() if per else None, hist.free_slots() if per else None,
                        episodes, counts, int(fs.rng_step.item()), fs.step_no, env._counters.cpu().numpy(), fs.extra.cpu().numpy(),
                        fs.xh[:, fs.F:].cpu().numpy()))
        hist.close()
    flat = lambda tree: [tree] if isinstance(tree, torch.Tensor) else [x for v in (tree.values() if isinstance(tree, dict) else tree) for x in flat(v)] if tree is not None else []   # noqa: E731
    (bb, sb, tb, fb, eb, cb, rb, nb, kb, xb, hb) = results[-1]     # the per-step path
    for (ba, sa, ta, fa, ea, ca, ra, na, ka, xa, ha) in results[:-1]:
        assert sa == sb and ea == eb and ca == cb and ra == rb == na == nb
        assert len(ea) > 0 and sum(ca) == E * calls * iters
        assert np.array_equal(ka, kb) and np.array_equal(xa.view(np.uint32), xb.view(np.uint32)) and np.array_equal(ha.view(np.uint32), hb.view(np.uint32))
        assert len(flat(ba)) == len(flat(bb)) > 0
        for x, y in zip(flat(ba), flat(bb)):
            assert torch.equal(x, y)
        if per:
            assert np.array_equal(fa, fb)
            for x, y in zip(ta, tb):
                assert np.array_equal(x, y)


def test_generic_path_takes_the_extras_at_the_last_layer():
    """CNN -> FC: the extras go into the last FC layer, which the fast step does not cover — the actor takes the generic
    device path on the wrapper's tuple observations, and what reaches the replay's `extra` ring is the restatement."""
    from rltime_amd.acting.fast_step import FastActingStep
    from rltime_amd.history import ReplayHistoryBuffer
    E, iters = 6, 10
    actor, pol, env = _make("dqn", "synthetic", E, True, exploration=EXPL, model=MODEL_FF)
    assert pol.model.extra_input_layer == 1 and not FastActingStep.supports(actor)
    hist = ReplayHistoryBuffer(size=E * 30, train_frequency=4, nstep_target=1, nstep_train=4, prefix_steps=0, gamma=0.99, device_rng=True)
    ef = _restate_for(env, E)
    ef.reset()
    for _ in range(3):
        s = actor.get_samples(E * iters)
        assert actor._fast is False and not getattr(s, "ingested", False)
        for step in s.vector_steps:
            want = ef.step(step["actions"].cpu().numpy(), step["rewards"].cpu().numpy(), step["dones"].cpu().numpy())
            assert np.array_equal(step["extra"].cpu().numpy().view(np.uint32), want.view(np.uint32))
        hist.update(s)
    assert hist._layout.extra_f32 == env.extra_size == 8
    batch = hist.get_train_data(8, train_progress=0.5)
    x, xt = batch["states"]["x"], batch["target_states"]["x"]
    # (no recurrent layer, so no stored `initials`: a done shows as timestep 0 in the row that follows)
    assert _check_batch_extras(batch, lambda B: _restate_for(env, B)) > 0
    assert x[0].dtype == torch.uint8 and xt[1].shape[-1] == 8
    hist.close()


def test_state_round_trip_continues_identically():
    """get_state after k steps -> a fresh actor and env -> set_state: both continue with identical actions, extras and
    counters."""
    E, k = 6, 9
    actor, pol, env = _make("dqn", "synthetic", E, True, exploration=EXPL)
    actor.get_samples(E * k)
    state = copy.deepcopy(actor.get_state())
    assert "extra" in state["fast"] and "extra_counters" in state["fast"] and "counters" in state["env"]
    assert np.array_equal(state["fast"]["extra_counters"].numpy(), state["env"]["counters"].numpy())
    assert state["env"]["counters"].numpy().max() > 0
    cont_a = actor.get_samples(E * k).vector_steps
    actor2, pol2, env2 = _make("dqn", "synthetic", E, True, exploration=EXPL)
    actor2.set_state(state)
    cont_b = actor2.get_samples(E * k).vector_steps
    assert actor._fast and actor2._fast and len(cont_a) == len(cont_b) == k
    for t, (a, b) in enumerate(zip(cont_a, cont_b)):
        for key in ("frames", "actions", "rewards", "dones", "extra", "policy", "state", "initials"):
            assert torch.equal(a[key], b[key]), (t, key)
    assert torch.equal(env._counters, env2._counters)
    assert torch.equal(actor._fast.xh[:, actor._fast.F:], actor2._fast.xh[:, actor2._fast.F:])


def test_train_loop_and_evaluation_on_the_shipped_config():
    """rltime_amd.train.train on configs/catch_iqn_lstm.json cut down: the actor runs the fast step from a captured rollout,
    the replay lays out the extras, the losses are finite, and a device evaluation of the trained policy completes."""
    from rltime_amd.acting.evaluator import Evaluator
    from rltime_amd.general.config import load_config
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.train import make_vec_env, train
    import random
    random.seed(0); np.random.seed(0); torch.manual_seed(0)      # noqa: E702
    cfg = load_config("catch_iqn_lstm.json")
    cfg["acting"]["actor_envs"] = 8
    cfg["policy_args"]["num_sampling_quantiles"] = 8
    cfg["training"]["args"].update(mbatch_size=4, nstep_train=8, burn_in_timesteps=0, total_steps=520, warmup_steps=200,
                                   log_freq=260, target_update_freq=100)
    cfg["training"]["args"]["history_mode"]["args"].update(size=400, train_frequency=4)
    logger = NullLogger()
    trainer = train(copy.deepcopy(cfg), logger, use_graph=True)
    X = 3 + 2
    fs = trainer.actors._fast
    assert fs and fs.X == X and fs.Xp == 16
    assert any(v[1] is not None for v in fs._rollouts.values())          # a captured rollout
    assert trainer.history_buffer._layout.extra_f32 == X
    losses = [row["train"]["qloss"] for name, _, row in logger.rows if name == "train" and "qloss" in row.get("train", {})]
    assert losses and all(np.isfinite(float(v)) for v in losses), losses
    assert all(bool(torch.isfinite(p).all()) for p in trainer.policy.parameters())
    env = make_vec_env(cfg["env"], cfg["env_args"], 8, "cuda", seed=1)
    ev = Evaluator(trainer.policy, env, 16, eps=0.0, steps_per_launch=16)
    rec = ev.run()
    assert ev.fused and rec["episodes"] == 16 and rec["length"]["mean"] == 11 and -1.0 <= rec["reward"]["mean"] <= 1.0
