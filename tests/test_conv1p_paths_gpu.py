"""GPU: one-plane frames through the layers above the kernels of csrc/conv_in_rows.hip — the CNN module and its autograd function
(models/torch/fused.py), the fast acting step and its captured rollout (acting/fast_step.py), and the train loop on the shipped
configs/catch_iqn_lstm_stack1.json: the reference's recurrent set-up on unstacked frames (configs/atari_iqn_lstm.json with
env_wrappers/atari_lstm.json, "stack": 1)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LAYERS = [{"filters": 32, "kernel": 8, "stride": 4}, {"filters": 64, "kernel": 4, "stride": 2}, {"filters": 64, "kernel": 3, "stride": 1}]
NATURE = {"type": "cnn", "args": {"channels_last": True, "layers": LAYERS}}
MODEL = {"type": "sequential", "args": {"layer_configs": [
    NATURE, {"type": "lstm", "args": {"num_units": 64}}, {"type": "fc", "args": {"fc_size": 64}}]}}
EXPL = {"type": "epsilon_greedy", "args": {"eps_start": 0.3, "eps_final": 0.3, "exploration_fraction": 0.5}}


def _profiled(fn):
    from rltime_amd import _lib
    torch.cuda.synchronize()
    _lib.check(_lib.lib.mirl_profile_reset())
    _lib.check(_lib.lib.mirl_profile_set(2))
    try:
        out = fn()
        torch.cuda.synchronize()
        ran = {r["name"]: r["calls"] for r in _lib.profile_table()}
    finally:
        _lib.check(_lib.lib.mirl_profile_set(0))
    return out, ran


class _MisalignedGrad(torch.autograd.Function):
    """Identity whose backward hands the incoming gradient on as a channels_last view that starts 4 bytes into a fresh
    buffer: what an upstream op may legitimately produce, and what the masked weight-gradient kernel does not take."""

    @staticmethod
    def forward(ctx, y):
        return y.view_as(y)

    @staticmethod
    def backward(ctx, grad):
        n, c, h, w = grad.shape
        buf = torch.empty(grad.numel() + 1, dtype=grad.dtype, device=grad.device)
        view = buf.as_strided((n, c, h, w), (h * w * c, 1, w * c, c), 1)
        view.copy_(grad)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous(memory_format=torch.channels_last)
        return view


def test_module_takes_one_plane_frames_and_the_autograd_function_matches_the_plain_expression():
    from rltime_amd.models.torch.fused import conv_u8_bias_relu, conv_u8_supported
    from rltime_amd.models.torch.modules import CNN
    torch.manual_seed(0)
    cnn = CNN((1, 84, 84), LAYERS, channels_last=True).cuda()
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randint(0, 256, (37, 1, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
    conv = cnn.layers[0]
    assert conv.in_channels == 1 and conv_u8_supported(x, conv)
    assert cnn.prepare_input(x) is None                                     # nothing to convert: forward() reads the uint8 rows
    with torch.no_grad():
        out, ran = _profiled(lambda: cnn(x))
    assert ran.get("k_conv1p_u8_fwd") == 1 and ran.get("k_conv1p_pack_w") == 1, ran
    assert "k_frames_to_f32_nhwc" not in ran and "k_conv1_u8_fwd" not in ran, ran
    with torch.no_grad():
        plain = F.relu(conv(x.float() * (1.0 / 255.0)))
        for layer in cnn.layers[1:]:
            plain = F.relu(layer(plain))
    assert out.shape == plain.shape and float((out - plain).abs().max()) <= 1e-4 * float(plain.abs().max())
    for misaligned in (False, True):
        conv.zero_grad(set_to_none=True)
        y = conv_u8_bias_relu(x, conv, 1.0 / 255.0)
        up = torch.randn(y.shape, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
        loss = ((_MisalignedGrad.apply(y) if misaligned else y) * up).sum()
        _, ran = _profiled(loss.backward)
        # the masked kernel needs no separate mask pass; the fallback is exactly that pass in front of the unmasked kernel
        assert ran.get("k_conv1p_u8_wrw") == 1 and bool(ran.get("k_relu_bwd_bias_rows")) == misaligned, ran
        fused = (y.detach(), conv.weight.grad.clone(), conv.bias.grad.clone())
        assert fused[1].stride() == conv.weight.stride()
        # the plain expression; its backward gets the FUSED forward's ReLU mask (an output within an ulp of zero may sit on the
        # other side in the two forwards, which would move a whole filter's gradient)
        pre = conv(x.float() * (1.0 / 255.0))
        dw, db = torch.autograd.grad(pre, (conv.weight, conv.bias), grad_outputs=up * (fused[0] > 0))
        for a, b, what in zip(fused, (F.relu(pre).detach(), dw, db), ("y", "dW", "db")):
            err = float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)
            assert err <= 1e-4, (what, misaligned, err)
    # a 4-plane block in the same process still runs the 4-plane family
    cnn4 = CNN((4, 84, 84), LAYERS, channels_last=True).cuda()
    x4 = torch.randint(0, 256, (5, 4, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
    with torch.no_grad():
        _, ran = _profiled(lambda: cnn4(x4))
    assert ran.get("k_conv1_u8_fwd") == 1 and "k_conv1p_u8_fwd" not in ran, ran


# ---- acting ---------------------------------------------------------------------------------------------------------------------

def _make(kind, env_kind, extras, E, fast, exploration=None, seed=5, done_prob=0.3):
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.catch_env import CatchVecEnv
    from rltime_amd.acting.extra_features import ExtraFeaturesVecEnv
    from rltime_amd.acting.synthetic_env import SyntheticAtariVecEnv
    from rltime_amd.policies.dqn import DQNPolicy
    from rltime_amd.policies.iqn import IQNPolicy
    torch.manual_seed(0)
    if env_kind == "catch":
        env = CatchVecEnv(E, frame_shape=(1, 84, 84), grid=6, n_actions=3, seed=seed)           # episodes of 5 steps
    else:
        env = SyntheticAtariVecEnv(E, frame_shape=(1, 84, 84), n_actions=6, seed=seed, done_prob=done_prob)
    if extras:
        env = ExtraFeaturesVecEnv(env)
    kw = dict(model_config=MODEL, observation_space=env.observation_space, action_space=env.action_space, dueling=True)
    pol = IQNPolicy.create(embedding_dim=16, num_sampling_quantiles=8, **kw) if kind == "iqn" else DQNPolicy.create(**kw)
    if kind == "iqn":
        g = torch.Generator().manual_seed(9)
        fixed = torch.rand(E * 8, generator=g).cuda()
        pol.tau_source = lambda n: fixed[:n]                 # the same quantile fractions on both paths
    actor = Actor(env, exploration_config=exploration, device=True, use_graph=True)
    actor.fast_step = fast
    actor.set_actor_policy(pol)
    return actor, pol, env


@pytest.mark.parametrize("extras", [True, False], ids=["extras", "frames-only"])
@pytest.mark.parametrize("kind,env_kind", [("iqn", "catch"), ("dqn", "catch"), ("iqn", "synthetic"), ("dqn", "synthetic")])
def test_fast_step_takes_one_plane_frames_and_matches_the_generic_device_path(kind, env_kind, extras):
    """tests/test_extra_features_gpu.py test_fast_step_takes_the_extras_and_matches_the_generic_device_path on (1, 84, 84)
    observations, with and without the extras: the fast step (input layer: mirl_conv1p_u8_fwd) against the generic device path
    on the same weights and streams, greedy, 12 steps over two get_samples calls."""
    from rltime_amd.acting.fast_step import FastActingStep
    E, steps = 6, 12
    outs = []
    for fast in (True, False):
        actor, pol, env = _make(kind, env_kind, extras, E, fast)
        assert (pol.model.extra_input_layer == 1) == extras
        assert FastActingStep.supports(actor)
        batch = actor.get_samples(E * 5)
        more = actor.get_samples(E * (steps - 5))            # a second call: re-selection on the current input state
        assert (actor._fast is not None and actor._fast is not False) == fast
        if fast:
            from rltime_amd._lib import lib
            import ctypes as C
            need = C.c_int64()
            assert lib.mirl_conv1p_u8_wpk_floats(C.byref(need)) == 0 and actor._fast.wpk.numel() == need.value
            assert actor._fast.y1.shape == (E, 32, 20, 20)
        outs.append(batch.vector_steps + more.vector_steps)
    sa, sb = outs
    assert len(sa) == len(sb) == steps
    n_done = 0
    for t, (a, b) in enumerate(zip(sa, sb)):
        assert a["frames"].shape[1:] == (1, 84, 84)
        assert torch.equal(a["frames"], b["frames"]) and torch.equal(a["dones"], b["dones"]), t
        assert torch.equal(a["rewards"], b["rewards"]), t
        assert torch.equal(a["actions"].cpu(), b["actions"].cpu()), t
        np.testing.assert_allclose(a["policy"].cpu().numpy(), b["policy"].cpu().numpy(), rtol=2e-4, atol=2e-5, err_msg="q %d" % t)
        assert torch.equal(a["initials"], b["initials"]), t
        np.testing.assert_allclose(a["state"].cpu().numpy(), b["state"].cpu().numpy(), rtol=2e-4, atol=2e-5, err_msg="state %d" % t)
        if extras:
            assert torch.equal(a["extra"].view(torch.int32), b["extra"].view(torch.int32)), t
        n_done += int(b["dones"].sum())
    assert n_done >= 6                                       # resets happened


def test_rollout_graph_equals_the_per_step_path_on_one_plane_frames(monkeypatch):
    """tests/test_extra_features_gpu.py test_rollout_graph_equals_the_per_step_path_with_extras for the recurrent IQN policy on
    (1, 84, 84) frames with extras: shard, sampled batch, episode statistics and counters of the captured rollout are
    bit-identical to the per-step path."""
    from rltime_amd.history import ReplayHistoryBuffer
    E, calls, iters = 16, 7, 6
    results = []
    for mode in ("graph", "per-step"):
        monkeypatch.setenv("MIRL_ROLLOUT_GRAPH", "0" if mode == "per-step" else "1")
        monkeypatch.setenv("MIRL_ROLLOUT_EAGER_CALLS", "0")
        actor, pol, env = _make("iqn", "synthetic", True, E, True, exploration=EXPL, done_prob=0.1)
        pol.tau_source = None                                      # quantile fractions drawn in the kernel
        hist = ReplayHistoryBuffer(size=E * 30, train_frequency=4, nstep_target=1, nstep_train=4, prefix_steps=2, gamma=0.99,
                                   device_rng=True, keep_policy_outputs=False)
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
        assert hist._layout.frame_bytes == 7056
        captured = [v[1] is not None for v in fs._rollouts.values()]
        assert (captured == []) if mode == "per-step" else (captured and all(captured)), (mode, fs._rollouts)
        torch.cuda.synchronize()
        episodes = actor._tracker.drain(wait=True)
        counts = actor._tracker.take_action_counts()
        batch = hist.get_train_data(8, train_progress=0.5)
        results.append((batch, hist.stats(), episodes, counts, int(fs.rng_step.item()), fs.step_no, fs.xh.cpu().numpy()))
        hist.close()
    flat = lambda tree: [tree] if isinstance(tree, torch.Tensor) else [x for v in (tree.values() if isinstance(tree, dict) else tree) for x in flat(v)] if tree is not None else []   # noqa: E731
    (ba, sa, ea, ca, ra, na, ha), (bb, sb, eb, cb, rb, nb, hb) = results
    assert sa == sb and ea == eb and ca == cb and ra == rb == na == nb
    assert len(ea) > 0 and sum(ca) == E * calls * iters
    assert np.array_equal(ha.view(np.uint32), hb.view(np.uint32))
    assert len(flat(ba)) == len(flat(bb)) > 0
    for x, y in zip(flat(ba), flat(bb)):
        assert torch.equal(x, y)


def test_train_loop_and_evaluation_on_the_shipped_stack1_config():
    """rltime_amd.train.train on configs/catch_iqn_lstm_stack1.json cut down as tests/test_extra_features_gpu.py cuts
    catch_iqn_lstm.json: the actor runs the fast step from a captured rollout, the replay stores one plane per transition, the
    learner runs the one-plane forward and weight-gradient kernels, losses and weights stay finite, and a device evaluation
    of the trained policy completes."""
    from rltime_amd.acting.evaluator import Evaluator
    from rltime_amd.general.config import load_config
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.train import make_vec_env, train
    import random
    random.seed(0); np.random.seed(0); torch.manual_seed(0)      # noqa: E702
    cfg = load_config("catch_iqn_lstm_stack1.json")
    assert cfg["env_args"]["frame_shape"] == [1, 84, 84]
    base = load_config("catch_iqn_lstm.json")
    base["env_args"]["frame_shape"] = [1, 84, 84]
    assert {k: v for k, v in cfg.items() if k != "_comment"} == {k: v for k, v in base.items() if k != "_comment"}
    cfg["acting"]["actor_envs"] = 8
    cfg["policy_args"]["num_sampling_quantiles"] = 8
    cfg["training"]["args"].update(mbatch_size=4, nstep_train=8, burn_in_timesteps=0, total_steps=520, warmup_steps=200,
                                   log_freq=260, target_update_freq=100)
    cfg["training"]["args"]["history_mode"]["args"].update(size=400, train_frequency=4)
    logger = NullLogger()
    trainer, ran = _profiled(lambda: train(copy.deepcopy(cfg), logger, use_graph=True))
    fs = trainer.actors._fast
    assert fs and fs.X == 5 and fs.y1.shape[1:] == (32, 20, 20)
    assert any(v[1] is not None for v in fs._rollouts.values())          # a captured rollout
    assert trainer.history_buffer._layout.frame_bytes == 7056 and trainer.history_buffer._layout.extra_f32 == 5
    assert ran.get("k_conv1p_u8_fwd") and ran.get("k_conv1p_u8_wrw"), ran
    assert "k_conv1_u8_fwd" not in ran and "k_frames_to_f32_nhwc" not in ran, ran
    losses = [row["train"]["qloss"] for name, _, row in logger.rows if name == "train" and "qloss" in row.get("train", {})]
    assert losses and all(np.isfinite(float(v)) for v in losses), losses
    assert all(bool(torch.isfinite(p).all()) for p in trainer.policy.parameters())
    env = make_vec_env(cfg["env"], cfg["env_args"], 8, "cuda", seed=1)
    ev = Evaluator(trainer.policy, env, 16, eps=0.0, steps_per_launch=16)
    rec = ev.run()
    assert ev.fused and rec["episodes"] == 16 and rec["length"]["mean"] == 11 and -1.0 <= rec["reward"]["mean"] <= 1.0
