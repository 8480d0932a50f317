"""GPU: three-plane frames through the layers above the kernels of csrc/conv_in_rows.hip — the CNN module and its autograd function
(models/torch/fused.py), the fast acting step, its captured rollout and the fused evaluation (acting/fast_step.py,
acting/evaluator.py) on Flappy in colour, and the train loop on the shipped configs/flappy_iqn_lstm_rgb.json: the reference's
ple_flappy_bird_iqn_lstm.json set-up, one (3, 120, 80) RGB frame per step."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_conv1p_paths_gpu import LAYERS, _MisalignedGrad, _profiled

pytestmark = pytest.mark.gpu

# the shrunk set-up of the acting tests: (3, 24, 16) frames on a 12 x 8 grid of 2-pixel cells, conv 5 x 3 -> 3 x 1, LSTM 32
SMALL_MODEL = {"type": "sequential", "args": {"layer_configs": [
    {"type": "cnn", "args": {"channels_last": True, "layers": [{"filters": 32, "kernel": 8, "stride": 4}, {"filters": 16, "kernel": 3, "stride": 1}]}},
    {"type": "lstm", "args": {"num_units": 32}}, {"type": "fc", "args": {"fc_size": 32}}]}}
SMALL_ENV = dict(frame_shape=(3, 24, 16), rgb=True, cell=2, gap=3, spacing=4, n_actions=2, max_episode_steps=7, death_reward=-5.0)
EXPL = {"type": "epsilon_greedy", "args": {"eps_start": 0.3, "eps_final": 0.3, "exploration_fraction": 0.5}}


def _held(got, want, lib, what, bar):
    """error as a fraction of the largest element: within `bar`, and no further from float64 than twice the library's f32
    evaluation of the same expression or 2e-6 (the weight-gradient bars of tests/test_conv3p_gpu.py)"""
    top = float(want.abs().max())
    err, err_lib = float((got.double() - want).abs().max()) / top, float((lib.double() - want).abs().max()) / top
    print("%s: err %.3e of the largest element, library f32 %.3e" % (what, err, err_lib))
    assert err <= bar, (what, err)
    return err, err_lib


def test_module_takes_three_plane_frames_and_matches_the_converted_path():
    """CNN((3, 120, 80), nature layers, channels_last) forward + backward against the same module with direct_u8=False (the
    conversion + library convolution this family replaces) and against float64: outputs within the forward bar (1e-5 of the
    largest), layer 1's weight.grad / bias.grad within the gradient bars (1e-4 of the largest entry, and 2 x the library's own
    error or 2e-6); an upstream gradient off the 16-byte grid takes the unmasked route and agrees."""
    from rltime_amd.models.torch.fused import conv_u8_bias_relu, conv_u8_supported
    from rltime_amd.models.torch.modules import CNN
    torch.manual_seed(0)
    cnn = CNN((3, 120, 80), LAYERS, channels_last=True).cuda()
    ref = CNN((3, 120, 80), LAYERS, channels_last=True, direct_u8=False).cuda()
    ref.load_state_dict(cnn.state_dict())
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randint(0, 256, (37, 3, 120, 80), dtype=torch.uint8, device="cuda", generator=g)
    conv = cnn.layers[0]
    assert conv.in_channels == 3 and conv_u8_supported(x, conv) and cnn._takes_u8(x) and not ref._takes_u8(x)
    assert cnn.out_shape == (64, 11, 6)
    assert cnn.prepare_input(x) is None and ref.prepare_input(x) is not None         # nothing to convert: forward() reads the uint8 rows
    with torch.no_grad():
        out, ran = _profiled(lambda: cnn(x))
        out_ref, ran_ref = _profiled(lambda: ref(x))
    assert ran.get("k_conv1p3_u8_fwd") == 1 and ran.get("k_conv1p3_pack_w") == 1, ran
    assert not any(k in ran for k in ("k_frames_to_f32_nhwc", "k_conv1_u8_fwd", "k_conv1p_u8_fwd")), ran
    assert ran_ref.get("k_frames_to_f32_nhwc") == 1 and "k_conv1p3_u8_fwd" not in ran_ref, ran_ref
    assert out.shape == out_ref.shape == (37, 64, 11, 6)
    err_out = float((out - out_ref).abs().max()) / float(out_ref.abs().max())
    print("CNN (3, 120, 80) output against the converted path: %.3e of the largest output" % err_out)
    assert err_out <= 1e-5, err_out
    with torch.no_grad():
        y = conv_u8_bias_relu(x, conv, 1.0 / 255.0)
        y_ref = F.relu(ref.layers[0](x.float() * (1.0 / 255.0)))
        want_y = F.relu(F.conv2d(x.double() * (1.0 / 255.0), conv.weight.double(), conv.bias.double(), 4))
    _held(y, want_y, y_ref, "layer 1 forward", 1e-5)
    for misaligned in (False, True):
        conv.zero_grad(set_to_none=True)
        y = conv_u8_bias_relu(x, conv, 1.0 / 255.0)
        up = torch.randn(y.shape, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
        loss = ((_MisalignedGrad.apply(y) if misaligned else y) * up).sum()
        _, ran = _profiled(loss.backward)
        # the masked kernel needs no separate mask pass; the fallback is exactly that pass in front of the unmasked kernel
        assert ran.get("k_conv1p3_u8_wrw") == 1 and ran.get("k_conv1p3_wrw_reduce") == 1, ran
        assert bool(ran.get("k_relu_bwd_bias_rows")) == misaligned, ran
        dw, db = conv.weight.grad.clone(), conv.bias.grad.clone()
        assert dw.stride() == conv.weight.stride()
        # the converted path's backward gets the FUSED forward's ReLU mask (an output within an ulp of zero may sit on the other
        # side in the two forwards, which would move a whole filter's gradient)
        kept = up * (y.detach() > 0)
        c0 = ref.layers[0]
        pre = c0(x.float() * (1.0 / 255.0))
        dw_lib, db_lib = torch.autograd.grad(pre, (c0.weight, c0.bias), grad_outputs=kept)
        w64 = conv.weight.detach().double().requires_grad_(True)
        b64 = conv.bias.detach().double().requires_grad_(True)
        dw64, db64 = torch.autograd.grad(F.conv2d(x.double() * (1.0 / 255.0), w64, b64, 4), (w64, b64), grad_outputs=kept.double())
        err, err_lib = _held(dw, dw64, dw_lib, "layer 1 dW, misaligned=%s" % misaligned, 1e-4)
        assert err <= max(2.0 * err_lib, 2e-6), (err, err_lib)
        assert float((db.double() - db64).abs().max()) <= 1e-5 * max(float(db64.abs().max()), 1.0)
    # a three-plane HISTORY stack (no colour anywhere) takes the same family; one- and four-plane blocks keep theirs
    for planes, name in ((1, "k_conv1p_u8_fwd"), (4, "k_conv1_u8_fwd")):
        other = CNN((planes, 84, 84), LAYERS, channels_last=True).cuda()
        xo = torch.randint(0, 256, (5, planes, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
        with torch.no_grad():
            _, ran = _profiled(lambda: other(xo))
        assert ran.get(name) == 1 and "k_conv1p3_u8_fwd" not in ran, ran


# ---- acting ---------------------------------------------------------------------------------------------------------------------

def _make(E, fast, exploration=None, seed=5, extras=True, rgb=True):
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.extra_features import ExtraFeaturesVecEnv
    from rltime_amd.acting.flappy_env import FlappyVecEnv
    from rltime_amd.policies.iqn import IQNPolicy
    torch.manual_seed(0)
    env = FlappyVecEnv(E, seed=seed, **dict(SMALL_ENV, rgb=rgb))
    if extras:
        env = ExtraFeaturesVecEnv(env)
    pol = IQNPolicy.create(embedding_dim=16, num_sampling_quantiles=8, model_config=SMALL_MODEL, observation_space=env.observation_space,
                           action_space=env.action_space, dueling=True)
    g = torch.Generator().manual_seed(9)
    fixed = torch.rand(E * 8, generator=g).cuda()
    pol.tau_source = lambda n: fixed[:n]                     # the same quantile fractions on both paths
    actor = Actor(env, exploration_config=exploration, device=True, use_graph=True)
    actor.fast_step = fast
    actor.set_actor_policy(pol)
    return actor, pol, env


@pytest.mark.parametrize("rgb", [True, False], ids=["rgb", "three-plane-history"])
def test_fast_step_takes_three_plane_frames_and_matches_the_generic_device_path(rgb):
    """tests/test_conv1p_paths_gpu.py's comparison on the shrunk colour set-up — (3, 24, 16) frames, extras, LSTM 32, 4 envs,
    greedy, 12 steps over two get_samples calls: the fast step (input layer: mirl_conv1p3_u8_fwd) against the generic device
    path on the same weights and streams, within that test's tolerance.  The kernels do not care what the planes mean: the
    same frames as a three-plane HISTORY stack (no shipped config has one) take the family too."""
    from rltime_amd.acting.fast_step import FastActingStep
    E, steps = 4, 12
    outs = []
    for fast in (True, False):
        actor, pol, env = _make(E, fast, rgb=rgb)
        assert pol.model.extra_input_layer == 1
        assert FastActingStep.supports(actor)
        (batch, more), ran = _profiled(lambda: (actor.get_samples(E * 5), actor.get_samples(E * (steps - 5))))
        assert (actor._fast is not None and actor._fast is not False) == fast
        if fast:
            import ctypes as C
            from rltime_amd._lib import lib
            fs = actor._fast
            need = C.c_int64()
            assert lib.mirl_conv1p3_u8_wpk_floats(C.byref(need)) == 0 and fs.wpk.numel() == need.value
            assert fs.conv1_family.planes == 3 and fs.y1.shape == (E, 32, 5, 3) and fs.X == env.extra_size and fs.H == 32
            assert ran.get("k_conv1p3_u8_fwd") and "k_frames_to_f32_nhwc" not in ran, ran
            assert ran.get("k_flappy_env_step_pre") or ran.get("k_flappy_env_step"), ran
        else:
            assert "k_conv1p3_u8_fwd" in ran, ran            # the generic path's module forward takes the family as well
        outs.append(batch.vector_steps + more.vector_steps)
    sa, sb = outs
    assert len(sa) == len(sb) == steps
    n_done = 0
    for t, (a, b) in enumerate(zip(sa, sb)):
        assert a["frames"].shape[1:] == (3, 24, 16)
        assert torch.equal(a["frames"], b["frames"]) and torch.equal(a["dones"], b["dones"]), t
        assert torch.equal(a["rewards"], b["rewards"]), t
        assert torch.equal(a["actions"].cpu(), b["actions"].cpu()), t
        np.testing.assert_allclose(a["policy"].cpu().numpy(), b["policy"].cpu().numpy(), rtol=2e-4, atol=2e-5, err_msg="q %d" % t)
        assert torch.equal(a["initials"], b["initials"]), t
        np.testing.assert_allclose(a["state"].cpu().numpy(), b["state"].cpu().numpy(), rtol=2e-4, atol=2e-5, err_msg="state %d" % t)
        assert torch.equal(a["extra"].view(torch.int32), b["extra"].view(torch.int32)), t
        n_done += int(b["dones"].sum())
        if rgb:
            assert not bool((a["frames"] == 0).any())        # colour frames have no zero pixel: drawn after every reset too
    assert n_done >= E                                       # the 7-step limit at the latest: every env was reset


def test_get_samples_is_one_rollout_graph_and_the_evaluation_runs_fused():
    """The shrunk colour set-up writing into a device replay: every get_samples call goes out as ONE captured rollout graph,
    and what the replay stores is the restatement's colour frames on the stored actions; then a device evaluation of the same
    policy on fresh colour envs runs on the fused step."""
    from rltime_amd.acting.evaluator import Evaluator
    from rltime_amd.acting.extra_features import ExtraFeaturesVecEnv
    from rltime_amd.acting.flappy_env import FlappyVecEnv
    from rltime_amd.history import ReplayHistoryBuffer
    from tests import flappy_restate as FR
    from tests import flappy_rgb_restate as RGB
    E, iters, calls = 4, 6, 3
    actor, pol, env = _make(E, True, exploration=EXPL, seed=21)
    pol.tau_source = None                                      # quantile fractions drawn in the kernel
    hist = ReplayHistoryBuffer(size=E * 40, train_frequency=1, nstep_target=1, nstep_train=1, prefix_steps=0, gamma=0.99,
                               device_rng=True, keep_policy_outputs=False)
    actor.set_sink(hist)
    for _ in range(calls):
        s = actor.get_samples(E * iters)
        assert getattr(s, "ingested", False)
        hist.update(s)
    fs = actor._fast
    assert fs and fs.env_into and fs.env_pre and fs.conv1_family.planes == 3 and not fs.trusted_stack
    captured = [v[1] is not None for v in fs._rollouts.values()]
    assert captured and all(captured), fs._rollouts.keys()
    assert hist._layout.frame_bytes == 3 * 24 * 16
    # everything the replay holds about those vector steps, read back with one gather of windows of one transition
    # (tests/test_flappy_env_gpu.py _stored, for a (frames, extras) observation)
    steps = iters * calls
    batch = hist._gather(E * steps, torch.arange(E, dtype=torch.int32, device="cuda").repeat(steps),
                         torch.arange(steps, dtype=torch.int64, device="cuda").repeat_interleave(E), torch.ones(E * steps, device="cuda"))
    torch.cuda.synchronize()
    x = batch["target_states"]["x"]
    assert isinstance(x, tuple) and len(x) == 2
    frames = x[0][0].cpu().numpy().reshape(steps, E, 3, 24, 16)
    actions = batch["policy_outputs"]["actions"][0].cpu().numpy().reshape(steps, E)
    dones = 1.0 - batch["target_masks"][0].cpu().numpy().reshape(steps, E)
    hist.close()
    geo = (24, 16, 2, 3, 4)
    state, _, _, _ = FR.flappy_reset(21, E, 1, *geo)
    for k in range(iters * calls):
        state, _, r, d = FR.flappy_step(state, actions[k], 21, 1, *geo, 7, -5.0)
        assert np.array_equal(frames[k], RGB.render_rgb(state, 21, *geo)), k
        assert np.array_equal(dones[k].astype(np.uint8), d), k
    assert dones.any() and not dones.all()
    ev_env = ExtraFeaturesVecEnv(FlappyVecEnv(E, seed=1, **SMALL_ENV))
    ev = Evaluator(pol, ev_env, 8, eps=0.0, steps_per_launch=8)
    rec = ev.run()
    assert ev.fused and rec["episodes"] == 8 and 1 <= rec["length"]["mean"] <= 7


# ---- training -------------------------------------------------------------------------------------------------------------------

def test_train_loop_on_the_shipped_rgb_config():
    """rltime_amd.train.train on configs/flappy_iqn_lstm_rgb.json shrunk to 4 envs, mbatch 4, T = 8, a few hundred steps, at the
    config's own (3, 120, 80) frames and model: the actor runs the fused step from a captured rollout, the learner runs the
    three-plane forward and weight-gradient kernels and never converts a frame (the conversion is what precedes a library
    convolution of layer 1), losses and weights stay finite."""
    from rltime_amd.general.config import load_config
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.train import train
    import random
    random.seed(0); np.random.seed(0); torch.manual_seed(0)      # noqa: E702
    cfg = load_config("flappy_iqn_lstm_rgb.json")
    assert cfg["env_args"]["frame_shape"] == [3, 120, 80] and cfg["env_args"]["rgb"] is True
    cfg["acting"]["actor_envs"] = 4
    cfg["policy_args"]["num_sampling_quantiles"] = 8
    cfg["training"]["args"].update(mbatch_size=4, nstep_train=8, total_steps=320, warmup_steps=120, log_freq=160, target_update_freq=80)
    cfg["training"]["args"]["history_mode"]["args"].update(size=400, train_frequency=4)
    logger = NullLogger()
    trainer, ran = _profiled(lambda: train(copy.deepcopy(cfg), logger, use_graph=True))
    fs = trainer.actors._fast
    assert fs and fs.conv1_family.planes == 3 and fs.X == 4 and fs.y1.shape[1:] == (32, 29, 19) and fs.F == 4224
    assert any(v[1] is not None for v in fs._rollouts.values())          # a captured rollout
    assert trainer.history_buffer._layout.frame_bytes == 3 * 120 * 80 and trainer.history_buffer._layout.extra_f32 == 4
    assert ran.get("k_conv1p3_u8_fwd") and ran.get("k_conv1p3_u8_wrw") and ran.get("k_conv1p3_wrw_reduce"), ran
    assert not any(k in ran for k in ("k_frames_to_f32_nhwc", "k_conv1_u8_fwd", "k_conv1p_u8_fwd", "k_conv1_u8_wrw", "k_conv1p_u8_wrw")), ran
    assert ran.get("k_flappy_env_step_pre") or ran.get("k_flappy_env_step"), ran
    losses = [row["train"]["qloss"] for name, _, row in logger.rows if name == "train" and "qloss" in row.get("train", {})]
    assert losses and all(np.isfinite(float(v)) for v in losses), losses
    assert all(bool(torch.isfinite(p).all()) for p in trainer.policy.parameters())
