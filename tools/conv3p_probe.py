"""Timing probe for the input layer on three-plane frames (csrc/conv_in_rows.hip) against the path such frames took before the
family existed: conversion (csrc/convert.hip) + library convolution + bias / ReLU pass forward, mask + bias-gradient pass +
the library's weight gradient backward (CNN(direct_u8=False)), and for acting the generic device path (no fused step, no
rollout graph).  The former path is run from this tree by taking the three-plane entry out of fused._CONV_U8 for the
duration of its arm — the code that then runs is line for line what ran before.  HIP events around whole arms with the
profiler off, warm-up rounds first, the arms alternating inside every repeat; a separate profiled pass for the kernels
themselves.  One JSON line per measurement.

Usage: python tools/conv3p_probe.py [layer] [acting] [frames ...]     (default: both, 704 and 41472 frames of (3, 120, 80))"""
import contextlib
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from rltime_amd import _lib
from rltime_amd.models.torch import fused

H, W = 120, 80
OHW = 29 * 19


@contextlib.contextmanager
def former_path():
    fam = fused._CONV_U8.pop(3)
    try:
        yield
    finally:
        fused._CONV_U8[3] = fam


def alternating(arms, warm=3, repeats=9, inner=1):
    """arms: {name: fn}; -> {name: (median, min, max)} ms per call, the arms alternating inside every repeat"""
    times = {k: [] for k in arms}
    for r in range(warm + repeats):
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warm:
                times[name].append(a.elapsed_time(b) / inner)
    return {k: (round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)) for k, v in times.items()}


def profiled(fn, calls):
    torch.cuda.synchronize()
    _lib.check(_lib.lib.mirl_profile_reset())
    _lib.check(_lib.lib.mirl_profile_set(2))
    try:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return _lib.profile_table()
    finally:
        _lib.check(_lib.lib.mirl_profile_set(0))


def layer(n):
    from rltime_amd.models.torch.modules import CNN
    torch.manual_seed(0)
    spec = [{"filters": 32, "kernel": 8, "stride": 4}]
    new = CNN((3, H, W), spec, channels_last=True).cuda()
    old = CNN((3, H, W), spec, channels_last=True, direct_u8=False).cuda()
    old.load_state_dict(new.state_dict())
    g = torch.Generator(device="cuda").manual_seed(n)
    x = torch.randint(0, 256, (n, 3, H, W), dtype=torch.uint8, device="cuda", generator=g)
    dy = torch.randn((n, 32, 29, 19), device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    assert new._takes_u8(x) and not old._takes_u8(x)
    inner = 1 if n > 4096 else 20
    with torch.no_grad():
        fwd = alternating({"new": lambda: new(x), "former": lambda: old(x)}, inner=inner)
        err = float((new(x) - old(x)).abs().max()) / float(old(x).abs().max())
        # each arm against float64 on a few frames of the block (first, middle, last)
        rows = [0, n // 2, n - 1]
        c0 = new.layers[0]
        want = torch.relu(torch.nn.functional.conv2d(x[rows].double() * (1.0 / 255.0), c0.weight.double(), c0.bias.double(), 4))
        errs = {k: float((m(x)[rows].double() - want).abs().max()) / float(want.abs().max()) for k, m in (("new", new), ("former", old))}
        print(json.dumps({"what": "layer 1 forward against float64 on frames %s" % rows, "frames": n, **errs}), flush=True)
    print(json.dumps({"what": "layer 1 forward", "frames": n, "ms_new": fwd["new"], "ms_former": fwd["former"],
                      "ratio": round(fwd["former"][0] / fwd["new"][0], 2), "arms_differ_by": err}), flush=True)
    y_new, y_old = new(x), old(x)
    bwd = alternating({"new": lambda: torch.autograd.grad(y_new, list(new.parameters()), dy, retain_graph=True),
                       "former": lambda: torch.autograd.grad(y_old, list(old.parameters()), dy, retain_graph=True)}, inner=inner)
    print(json.dumps({"what": "layer 1 weight + bias gradient from dy", "frames": n, "ms_new": bwd["new"], "ms_former": bwd["former"],
                      "ratio": round(bwd["former"][0] / bwd["new"][0], 2)}), flush=True)

    def both():
        with torch.no_grad():
            new(x)
        torch.autograd.grad(y_new, list(new.parameters()), dy, retain_graph=True)

    calls = 5
    for row in profiled(both, calls):
        if row["name"].startswith("k_conv1p3"):
            print(json.dumps({"what": "kernel", "frames": n, "calls": calls, **row}), flush=True)


def acting(E=32, K=20):
    from rltime_amd.acting.actor import Actor
    from rltime_amd.general.config import load_config
    from rltime_amd.history import ReplayHistoryBuffer
    from rltime_amd.policies.iqn import IQNPolicy
    from rltime_amd.train import make_vec_env
    cfg = load_config("flappy_iqn_lstm_rgb.json")
    expl = {"type": "epsilon_greedy", "args": {"eps_start": 0.1, "eps_final": 0.1, "exploration_fraction": 0.5}}

    def build(graphs):
        torch.manual_seed(0)
        env = make_vec_env(cfg["env"], copy.deepcopy(cfg["env_args"]), E, "cuda")
        pol = IQNPolicy.create(model_config=copy.deepcopy(cfg["model"]), observation_space=env.observation_space, action_space=env.action_space,
                               **cfg["policy_args"])
        actor = Actor(env, exploration_config=expl, device=True, use_graph=True)
        actor.set_actor_policy(pol)
        hist = ReplayHistoryBuffer(size=E * 400, train_frequency=4, nstep_target=2, nstep_train=20, gamma=0.99, device_rng=True,
                                   keep_policy_outputs=False)
        actor.set_sink(hist)

        def call():
            s = actor.get_samples(E * K)
            hist.update(s)
        # (the fast step reads MIRL_ROLLOUT_GRAPH when the first call builds it)
        os.environ["MIRL_ROLLOUT_GRAPH"] = "0" if graphs is False else "1"
        try:
            call()
        finally:
            os.environ.pop("MIRL_ROLLOUT_GRAPH")
        return actor, call

    with former_path():
        a_old, old = build(None)
        assert not a_old._fast, "the former path must be the generic device path"
    a_step, per_step = build(False)
    a_graph, graph = build(True)
    assert a_step._fast and a_graph._fast and a_graph._fast.conv1_family.planes == 3
    assert any(v[1] is not None for v in a_graph._fast._rollouts.values()) and not any(v[1] is not None for v in a_step._fast._rollouts.values())

    def former():
        with former_path():
            old()

    t = alternating({"former generic path": former, "fused step, per step": per_step, "fused step, one rollout graph": graph})
    print(json.dumps({"what": "acting: one get_samples call of %d vector steps at %d envs, ms per VECTOR STEP (median, min, max)" % (K, E),
                      **{k: tuple(round(x / K, 4) for x in v) for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    sizes = [int(a) for a in args if a.isdigit()] or [704, 41472]
    if "acting" not in args or "layer" in args:
        for n in sizes:
            layer(n)
    if "layer" not in args or "acting" in args:
        acting()
