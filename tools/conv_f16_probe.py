"""The 16-filter input layer (csrc/conv_in_f16.hip) against what ran for the layer before it existed, in alternating windows on one
GPU: forward = frame conversion + library convolution + bias / ReLU pass, weight gradient = the library's, masked weight
gradient = mask pass + the library's; then the vector step of configs/catch_dqn_small.json at 16 envs, fused against generic.
Both sides are first checked against the former path run in chunks of 2048 frames (the library's results on inputs beyond
4 GB are not trusted: docs/measurement.md).

    python tools/conv_f16_probe.py [--frames 41472] [--planes 1,3,4] [--out conv_f16_probe.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rltime_amd import _lib as L                                            # noqa: E402
from rltime_amd.models.torch import fused                                   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=41472)
ap.add_argument("--planes", default="1,3,4")
ap.add_argument("--out", default="conv_f16_probe.json")
args = ap.parse_args()
N = args.frames
WINDOWS = 7
out = {}


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def compare(name, new, old, reps_new, reps_old):
    for _ in range(3):
        new(); old()                                                        # noqa: E702
    torch.cuda.synchronize()
    tn, to = [], []
    for _ in range(WINDOWS):
        tn.append(window(new, reps_new))
        to.append(window(old, reps_old))
    rec = {"new_ms": [statistics.median(tn), min(tn), max(tn)], "parent_ms": [statistics.median(to), min(to), max(to)]}
    out[name] = rec
    print(name, json.dumps(rec), flush=True)


SHAPE = {1: (84, 84), 4: (84, 84), 3: (120, 80)}
for planes in [int(v) for v in args.planes.split(",") if v]:
    h, w = SHAPE[planes]
    torch.manual_seed(planes)
    g = torch.Generator(device="cuda").manual_seed(planes)
    x = torch.randint(0, 256, (N, planes, h, w), dtype=torch.uint8, device="cuda", generator=g)
    conv = nn.Conv2d(planes, 16, 8, 4).cuda().to(memory_format=torch.channels_last).requires_grad_(False)
    scale = 1.0 / 255.0
    fam = fused.conv_u8_family(planes, 16)
    assert fused.conv_u8_supported(x, conv)
    with torch.no_grad():
        xf = fused.frames_to_f32_nhwc(x, scale)
        y = fused.conv_u8_bias_relu(x, conv, scale)
        y_old = fused.conv_bias_relu(xf, conv)
        # the parent's path in chunks of 2048 frames (its inputs stay below 4 GB) is what both are held to
        e_new = e_old = 0.0
        for i in range(0, N, 2048):
            yc = fused.conv_bias_relu(fused.frames_to_f32_nhwc(x[i:i + 2048], scale), conv)
            e_new = max(e_new, float((y[i:i + 2048] - yc).abs().max()))
            e_old = max(e_old, float((y_old[i:i + 2048] - yc).abs().max()))
        print("P=%d fwd check: new vs chunked parent %.3e, whole-batch parent vs chunked %.3e, of the largest output %.3e"
              % (planes, e_new, e_old, float(y.abs().max())), flush=True)
        assert e_new <= 1e-4 * float(y.abs().max())
        dy = torch.randn(y.shape, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
        gm, _ = fused.relu_bwd_bias_rows(dy, y, 16)
        scratch = torch.empty(fam.wrw_scratch_floats(), device="cuda")
        dw, db = torch.empty_like(conv.weight), torch.empty(16, device="cuda")
        n = x.shape[0]

        def new_fwd():
            fused.conv_u8_bias_relu(x, conv, scale)

        def old_fwd():
            fused.conv_bias_relu(fused.frames_to_f32_nhwc(x, scale), conv)

        def new_wrw():
            fam.call("wrw", n, h, w, L.ptr(x), L.ptr(gm), scale, L.ptr(scratch), L.ptr(dw), *fam.strides(dw))

        def lib_wrw(gg, xx=None):
            return torch.ops.aten.convolution_backward(gg, xf if xx is None else xx, conv.weight, None, [4, 4], [0, 0], [1, 1], False, [0, 0], 1,
                                                       [False, True, False])[1]

        def old_wrw():
            lib_wrw(gm)

        def new_msk():
            fam.call("wrw_masked", n, h, w, L.ptr(x), L.ptr(dy), L.ptr(y), scale, L.ptr(scratch), L.ptr(dw), *fam.strides(dw), L.ptr(db))

        def old_msk():
            lib_wrw(fused.relu_bwd_bias_rows(dy, y, 16)[0])

        new_wrw()
        # the library's weight gradient in chunks of 2048 frames, summed in float64 (its inputs stay below 4 GB)
        ref = sum(lib_wrw(gm[i:i + 2048], xf[i:i + 2048]).double() for i in range(0, n, 2048))
        top = float(ref.abs().max())
        print("P=%d wrw check: new vs chunked library %.3e, whole-batch library vs chunked %.3e, of the largest entry %.3e"
              % (planes, float((dw.double() - ref).abs().max()), float((lib_wrw(gm).double() - ref).abs().max()), top), flush=True)
        assert float((dw.double() - ref).abs().max()) <= 1e-3 * top
        tag = "P=%d %dx%d N=%d " % (planes, h, w, N)
        compare(tag + "fwd", new_fwd, old_fwd, 60, 12)
        compare(tag + "wrw", new_wrw, old_wrw, 40, 8)
        compare(tag + "wrw_masked", new_msk, old_msk, 40, 8)
    del x, xf, y, y_old, dy, gm
    torch.cuda.empty_cache()


# the vector step of configs/catch_dqn_small.json at 16 envs: the fused acting step against the generic device path
def make_actor(fast):
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.catch_env import CatchVecEnv
    from rltime_amd.general.config import load_config
    from rltime_amd.policies.dqn import DQNPolicy
    cfg = load_config("catch_dqn_small.json")
    torch.manual_seed(0)
    env = CatchVecEnv(16, frame_shape=tuple(cfg["env_args"]["frame_shape"]), grid=cfg["env_args"]["grid"], n_actions=3, seed=1)
    pol = DQNPolicy.create(model_config=cfg["model"], observation_space=env.observation_space, action_space=env.action_space, dueling=True)
    actor = Actor(env, exploration_config=cfg["acting"]["exploration"], device=True, use_graph=True)
    actor.fast_step = fast
    actor.set_actor_policy(pol)
    return actor


actors = {fast: make_actor(fast) for fast in (True, False)}
STEPS = 200
ts = {True: [], False: []}
for fast in (True, False):
    actors[fast].get_samples(16 * 20)
torch.cuda.synchronize()
for _ in range(WINDOWS):
    for fast in (True, False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        actors[fast].get_samples(16 * STEPS)
        torch.cuda.synchronize()
        ts[fast].append((time.perf_counter() - t0) / STEPS * 1e3)
assert actors[True]._fast and not actors[False]._fast
out["vector step 16 envs"] = {"fused_ms": [statistics.median(ts[True]), min(ts[True]), max(ts[True])],
                              "generic_ms": [statistics.median(ts[False]), min(ts[False]), max(ts[False])]}
print("vector step 16 envs", json.dumps(out["vector step 16 envs"]), flush=True)
json.dump(out, open(args.out, "w"), indent=1)
