"""GPU: the small nature CNN (configs/models/modules/nature_cnn_small.json, 16 k8 s4 -> 32 k4 s2) through the layers above the
kernels of csrc/conv_in_f16.hip: the CNN module and its autograd function (models/torch/fused.py) and the fast acting step
(acting/fast_step.py)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

KERNEL = {1: "k_conv1f16p_u8_", 3: "k_conv1f16p3_u8_", 4: "k_conv1f16p4_u8_"}


def _module():
    from rltime_amd.general.config import load_config
    return load_config("models/modules/nature_cnn_small.json")


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


@pytest.mark.parametrize("planes", [1, 3, 4])
def test_module_converts_nothing_and_its_gradients_match_float64(planes):
    from rltime_amd.models.torch.fused import conv_u8_family, conv_u8_supported
    from rltime_amd.models.torch.modules import CNN
    torch.manual_seed(planes)
    cnn = CNN((planes, 36, 44), **_module()["args"]).cuda()
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randint(0, 256, (5, planes, 36, 44), dtype=torch.uint8, device="cuda", generator=g)
    conv = cnn.layers[0]
    assert conv.out_channels == 16 and conv_u8_supported(x, conv) and conv_u8_family(planes, 16).planes == planes
    assert cnn.prepare_input(x) is None                                     # nothing to convert: forward() reads the uint8 rows
    up = torch.randn((5,) + tuple(cnn.out_shape), device="cuda", generator=g)
    out, ran = _profiled(lambda: cnn(x))
    assert ran.get(KERNEL[planes] + "fwd") == 1 and "k_frames_to_f32_nhwc" not in ran, ran
    _, ran = _profiled((out * up).sum().backward)
    assert ran.get(KERNEL[planes] + "wrw") == 1, ran
    # the plain expression in float64, through both layers
    ref = copy.deepcopy(cnn).double()
    h = x.double() * cnn.scale
    for layer in ref.layers:
        layer.zero_grad(set_to_none=True)
        h = F.relu(layer(h))
    (h * up.double()).sum().backward()
    np.testing.assert_allclose(out.detach().cpu().numpy(), h.detach().cpu().numpy(), rtol=2e-4, atol=2e-5)
    for (name, a), b in zip(cnn.named_parameters(), ref.parameters()):
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.cpu().numpy(), rtol=2e-4, atol=2e-5, err_msg=name)


def test_fast_step_takes_the_small_stack_and_its_input_layer_is_the_autograd_forward():
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.catch_env import CatchVecEnv
    from rltime_amd.acting.fast_step import FastActingStep
    from rltime_amd.models.torch.fused import conv_u8_bias_relu, conv_u8_family
    from rltime_amd.policies.dqn import DQNPolicy
    torch.manual_seed(0)
    E = 6
    env = CatchVecEnv(E, frame_shape=(4, 84, 84), grid=6, n_actions=3, seed=5)
    model = {"type": "sequential", "args": {"layer_configs": [_module(), {"type": "fc", "args": {"fc_size": 64}}]}}
    pol = DQNPolicy.create(model_config=model, observation_space=env.observation_space, action_space=env.action_space, dueling=True)
    actor = Actor(env, exploration_config=None, device=True, use_graph=True)
    actor.fast_step = True
    actor.set_actor_policy(pol)
    assert FastActingStep.supports(actor)
    actor.get_samples(E)
    fs = actor._fast
    assert fs and fs.conv1_family is conv_u8_family(4, 16) and fs.y1.shape == (E, 16, 20, 20)
    with torch.no_grad():
        want = conv_u8_bias_relu(fs.last_obs, fs.cnn.layers[0], fs.cnn.scale)
    torch.cuda.synchronize()
    assert torch.equal(fs.y1, want)
