"""Timings of the actor-critic device path on one GPU (docs/measurement.md, "A2C / PPO on the device"):

  loss      M = 512 rows, A = 6 and 18, from logits / values to their gradients: the fused call (training/qops.py ac_loss +
            backward) against the plain-torch expression of A2C._compute_grads / PPO._calc_action_gain on the same GPU tensors,
            alternating, host clock around a synchronised window of `--iters` calls each, repeated `--repeats` times
  window    one DeviceOnlineHistory.get_train_data at T = 128, B = 16 on (4, 84, 84) uint8 frames, and the same with a
            recurrent state of S = 1024 float32 words (hx, cx of an LSTM 512) and the initials flag moved beside every row
  acting    one vector step of the device actor at 16 envs (catch_ppo.json's network, generic device path)
  acting_sides   the same vector step, fed into the rollout window, four ways in ONE call, alternating, `--repeats` windows of
            2 x 64 steps each: the generic device path eager and graphed (Actor.use_graph), the fused step per step
            (acting.extra_args.fused_step with MIRL_ROLLOUT_GRAPH=0) and the fused rollout graph, 64 steps per launch — for
            catch_ppo.json's network, for catch_ppo_lstm.json's and for the MLP of cartpole_ppo_device.json (the fused sides
            are then acting/fast_mlp_step.FastMlpAcStep: the whole network as one launch); `--configs` narrows the list
  iteration   (`--only iteration`) wall time of one learner iteration (32 vector steps of acting at 16 envs + 16 minibatch
            updates) of cartpole_ppo_device.json and of cartpole_ppo_fused.json, alternating in one call, `--repeats` runs each:
            from the `total.seconds` of the runs' own log rows, the first 20 iterations (start-up, captures) left out

    python tools/actor_critic_probe.py [--iters 200] [--repeats 5]      -> one JSON line
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6          # microseconds per call


def _torch_loss(logits, values, actions, targets, acting, old, vf, ef, clip):
    """A2C._compute_grads with PPO's gain, as the trainers write it."""
    dist = torch.distributions.Categorical(logits=logits)
    log_probs, entropy = dist.log_prob(actions), dist.entropy().mean()
    adv = targets - acting
    adv = (adv - adv.mean()) / (adv.std() + 1e-5)
    ratio = torch.exp(log_probs - old)
    gain = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv).mean()
    value_loss = (targets - values).pow(2).mean()
    return value_loss * vf - gain - ef * entropy


def loss_times(M, A, iters, repeats):
    from rltime_amd.training import qops
    g = torch.Generator(device="cuda").manual_seed(1)
    logits = torch.randn(M, A, device="cuda", generator=g).requires_grad_(True)
    values = torch.randn(M, device="cuda", generator=g).requires_grad_(True)
    actions = torch.randint(0, A, (M,), device="cuda", generator=g)
    a32 = actions.to(torch.int32)
    targets, acting = values.detach() + torch.randn(M, device="cuda", generator=g), values.detach() + 0.3
    old = torch.log_softmax(logits.detach(), 1).gather(1, actions[:, None])[:, 0] + 0.2 * torch.randn(M, device="cuda", generator=g)

    def fused():
        logits.grad = values.grad = None
        loss, _ = qops.ac_loss(logits, values, a32, targets, acting, old_log_probs=old, vf_coef=0.5, entropy_factor=0.01,
                               clip_value=0.2, adv_norm=True)
        loss.backward()

    def plain():
        logits.grad = values.grad = None
        _torch_loss(logits, values, actions, targets, acting, old, 0.5, 0.01, 0.2).backward()
    fused()
    g_f = logits.grad.clone()
    fused()
    diff = float((logits.grad - g_f).abs().max())           # (a rerun repeats the first run bit for bit: 0.0)
    plain()
    agree = float((logits.grad - g_f).abs().max() / g_f.abs().max())
    for _ in range(20):
        fused()
        plain()
    f, p = [], []
    for _ in range(repeats):                                  # alternating, same process
        f.append(_timed(fused, iters))
        p.append(_timed(plain, iters))
    return {"M": M, "A": A, "fused_us": [round(x, 1) for x in f], "torch_us": [round(x, 1) for x in p],
            "fused_us_median": round(sorted(f)[len(f) // 2], 1), "torch_us_median": round(sorted(p)[len(p) // 2], 1),
            "rerun_max_diff": diff, "fused_vs_torch_grad_rel": agree}


def _torch_loss_normal(mean, logstd, values, actions, targets, acting, old, vf, ef, clip):
    """The same with the Normal head: joint log-probability, entropy .mean() over all M * D elements."""
    dist = torch.distributions.Normal(mean, logstd.exp().expand_as(mean))
    log_probs, entropy = dist.log_prob(actions).sum(-1), dist.entropy().mean()
    adv = targets - acting
    adv = (adv - adv.mean()) / (adv.std() + 1e-5)
    ratio = torch.exp(log_probs - old)
    gain = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv).mean()
    value_loss = (targets - values).pow(2).mean()
    return value_loss * vf - gain - ef * entropy


def normal_loss_times(M, D, iters, repeats):
    """mountaincar_continuous_ppo's loss: M = 128 is one minibatch of the config (16 envs x 32 steps / 4)."""
    from rltime_amd.training import qops
    g = torch.Generator(device="cuda").manual_seed(2)
    mean = torch.randn(M, D, device="cuda", generator=g).requires_grad_(True)
    logstd = (torch.rand(D, device="cuda", generator=g) - 0.7).requires_grad_(True)
    values = torch.randn(M, device="cuda", generator=g).requires_grad_(True)
    actions = (mean + logstd.exp() * torch.randn(M, D, device="cuda", generator=g)).detach()
    targets, acting = values.detach() + torch.randn(M, device="cuda", generator=g), values.detach() + 0.3
    with torch.no_grad():
        old = torch.distributions.Normal(mean, logstd.exp().expand_as(mean)).log_prob(actions).sum(-1) \
            + 0.2 * torch.randn(M, device="cuda", generator=g)

    def fused():
        mean.grad = logstd.grad = values.grad = None
        loss, _ = qops.ac_loss_normal(mean, logstd, values, actions, targets, acting, old_log_probs=old, vf_coef=0.5,
                                      entropy_factor=0.01, clip_value=0.2, adv_norm=True)
        loss.backward()

    def plain():
        mean.grad = logstd.grad = values.grad = None
        _torch_loss_normal(mean, logstd, values, actions, targets, acting, old, 0.5, 0.01, 0.2).backward()
    fused()
    g_m, g_s = mean.grad.clone(), logstd.grad.clone()
    fused()
    diff = max(float((mean.grad - g_m).abs().max()), float((logstd.grad - g_s).abs().max()))
    plain()
    agree = max(float((mean.grad - g_m).abs().max() / g_m.abs().max()), float((logstd.grad - g_s).abs().max() / g_s.abs().max()))
    for _ in range(20):
        fused()
        plain()
    f, p = [], []
    for _ in range(repeats):                                  # alternating, same process
        f.append(_timed(fused, iters))
        p.append(_timed(plain, iters))
    return {"M": M, "D": D, "fused_us": [round(x, 1) for x in f], "torch_us": [round(x, 1) for x in p],
            "fused_us_median": round(sorted(f)[len(f) // 2], 1), "torch_us_median": round(sorted(p)[len(p) // 2], 1),
            "rerun_max_diff": diff, "fused_vs_torch_grad_rel": agree}


def normal_head_time(E, D, iters, repeats):
    """One launch of the Normal sampling head on ready operands against the torch expression of actor_predict."""
    from rltime_amd._lib import lib, check, ptr as p, stream
    g = torch.Generator(device="cuda").manual_seed(3)
    mean, values = torch.randn(E, D, device="cuda", generator=g), torch.randn(E, device="cuda", generator=g)
    logstd, eps = torch.zeros(D, device="cuda"), torch.randn(E, D, device="cuda", generator=g)
    actions, block = torch.empty(E, D, device="cuda"), torch.empty(E, 2, device="cuda")

    def kernel():
        check(lib.mirl_actor_head_normal(E, D, p(mean), D, p(logstd), p(values), p(eps), p(actions), p(block), p(block[:, 1]), 2,
                                         stream()), "mirl_actor_head_normal")

    def plain():
        dist = torch.distributions.Normal(mean, logstd.exp().expand_as(mean))
        a = dist.sample()
        return a, dist.log_prob(a).sum(-1)
    for _ in range(20):
        kernel()
        plain()
    k, t = [], []
    for _ in range(repeats):
        k.append(_timed(kernel, iters))
        t.append(_timed(plain, iters))
    return {"E": E, "D": D, "kernel_us_median": round(sorted(k)[len(k) // 2], 1), "torch_us_median": round(sorted(t)[len(t) // 2], 1)}


def mountaincar_step_time(E, iters, repeats):
    """One env step (step_into on static buffers with a bound action buffer)."""
    from rltime_amd.acting.mountaincar_device_env import MountainCarDeviceVecEnv
    env = MountainCarDeviceVecEnv(E, max_episode_steps=999, seed=0)
    env.reset()
    env.bind_actions(torch.randn(E, 1, device="cuda"))
    out = env._fresh()
    for _ in range(20):
        env.step_into(*out)
    s = [_timed(lambda: env.step_into(*out), iters) for _ in range(repeats)]
    return {"E": E, "step_us_median": round(sorted(s)[len(s) // 2], 1)}


def window_time(iters, state_f32=0):
    from rltime_amd.acting.acting_interface import DeviceSamples
    from rltime_amd.history.online_device import DeviceOnlineHistory
    T, B = 128, 16

    def discount(n, r, po):
        return 0.0
    discount.gamma, discount.lam = 0.99, 0.95
    hist = DeviceOnlineHistory(nstep_target=T, nstep_train=T, discount_function=discount)
    frames = torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, device="cuda")
    step = dict(frames=frames, actions=torch.zeros(B, dtype=torch.int32, device="cuda"), policy=torch.zeros(B, 2, device="cuda"),
                rewards=torch.ones(B, device="cuda"), dones=torch.zeros(B, dtype=torch.uint8, device="cuda"))
    example = {"x": frames[0].cpu().numpy(), "layer0_state": {}}
    if state_f32:
        H = state_f32 // 2
        step.update(state=torch.randn(B, state_f32, device="cuda"), initials=torch.zeros(B, device="cuda"))
        example["layer1_state"] = {"hx": step["state"][0, :H].cpu().numpy(), "cx": step["state"][0, H:].cpu().numpy(),
                                   "initials": step["initials"][0].cpu().numpy()}
    times = []
    for _ in range(iters):
        s = DeviceSamples(example, B, 0)
        for _ in range(T):
            s.append(**step)
        hist.update(s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch = hist.get_train_data(B)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
        assert batch is not None
    times = sorted(times[1:])
    nbytes = 4 * T * B * 4 * 84 * 84                          # both blocks read and written
    med = times[len(times) // 2]
    return {"T": T, "B": B, "state_f32": state_f32, "state_MB": round(4 * T * B * 4 * state_f32 / 1e6, 1),
            "get_train_data_us_median": round(med, 1), "get_train_data_us_min": round(times[0], 1),
            "observation_GBps_at_median": round(nbytes / med / 1e3, 1), "ring_capacity_steps": hist.capacity}


def acting_time(iters):
    from rltime_amd.general.config import load_config
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    from rltime_amd.train import create_actors
    cfg = load_config("catch_ppo.json")
    actors = create_actors(cfg, "cuda")
    try:
        obs_space, act_space = actors.get_spaces()
        policy = ActorCriticPolicy.create(model_config=cfg["model"], observation_space=obs_space, action_space=act_space, cuda=True)
        actors.set_actor_policy(policy)
        E = actors.get_env_count()
        actors.get_samples(E * 20)
        us = _timed(lambda: actors.get_samples(E * 10), max(1, iters // 10)) / 10
    finally:
        actors.close()
    return {"envs": E, "vector_step_us": round(us, 1)}


def acting_sides(config, repeats, steps=64):
    """Microseconds per vector step, get_samples + History.update, host clock around synchronised windows."""
    import copy
    from rltime_amd.general.config import load_config
    from rltime_amd.history.online_device import DeviceOnlineHistory
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    from rltime_amd.train import create_actors

    def discount(n, r, po):
        return 0.0
    discount.gamma, discount.lam = 0.99, 0.95
    base = load_config(config)
    sides, made = {}, []
    try:
        for name, fused, graph, env_graph in (("generic_eager", False, False, "1"), ("generic_graphed", False, True, "1"),
                                              ("fused_per_step", True, True, "0"), ("fused_rollout", True, True, "1")):
            cfg = copy.deepcopy(base)
            if fused:
                cfg["acting"]["extra_args"] = {"fused_step": True}
            torch.manual_seed(0)
            actors = create_actors(cfg, "cuda", use_graph=graph)
            made.append(actors)
            obs_space, act_space = actors.get_spaces()
            policy = ActorCriticPolicy.create(model_config=cfg["model"], observation_space=obs_space, action_space=act_space, cuda=True)
            actors.set_actor_policy(policy)
            hist = DeviceOnlineHistory(nstep_target=128, nstep_train=128, max_delayed_steps=256, discount_function=discount)
            if fused:
                actors.set_sink(hist, clip_rewards=True)
            E = actors.get_env_count()

            def call(actors=actors, hist=hist, E=E):
                hist.update(actors.get_samples(E * steps))
            keep = os.environ.get("MIRL_ROLLOUT_GRAPH")
            os.environ["MIRL_ROLLOUT_GRAPH"] = env_graph          # read when the fused step is built: the first call
            try:
                for _ in range(3):
                    call()
            finally:
                os.environ.pop("MIRL_ROLLOUT_GRAPH") if keep is None else os.environ.__setitem__("MIRL_ROLLOUT_GRAPH", keep)
            assert bool(actors._fast) == fused and (not fused or actors._fast.rollout_graphs == (env_graph == "1"))
            sides[name] = (call, [])
        for _ in range(repeats):                                  # alternating, same process
            for name, (call, times) in sides.items():
                times.append(_timed(call, 2) / steps)
    finally:
        for actors in made:
            actors.close()
    out = {"config": config, "envs": E, "steps_per_call": steps}
    for name, (_, times) in sides.items():
        out[name + "_us"] = [round(t, 1) for t in times]
        out[name + "_us_median"] = round(sorted(times)[len(times) // 2], 1)
    return out


ACTING_CONFIGS = ("catch_ppo.json", "catch_ppo_lstm.json", "cartpole_ppo_device.json")


def iteration_times(repeats, iters=120, log_iters=20):
    """Milliseconds per learner iteration of the two CartPole PPO configs, steady state: (seconds at the last log row -
    seconds at the first) / the iterations between them."""
    import tempfile
    from rltime_amd.general.config import load_config
    from rltime_amd.train import train_from_config
    names = ("cartpole_ppo_device.json", "cartpole_ppo_fused.json")
    times = {n: [] for n in names}
    for r in range(repeats):
        for name in names:
            cfg = load_config(name)
            per_iter = cfg["acting"]["actor_envs"] * cfg["training"]["args"]["nstep_train"]
            with tempfile.TemporaryDirectory() as tmp:
                train_from_config(name, log_dir=tmp, log_name="run", seed=1 + r,
                                  conf_update={"training": {"args": {"total_steps": per_iter * iters, "log_freq": per_iter * log_iters}}})
                torch.cuda.synchronize()
                rows = [json.loads(line) for line in open(os.path.join(tmp, "run", "train.json"))]
            secs = [row["total"]["seconds"] for row in rows]
            assert len(secs) == iters // log_iters, len(secs)
            times[name].append((secs[-1] - secs[0]) / (iters - log_iters) * 1e3)
    out = {"iterations": iters - log_iters, "steps_per_iteration": per_iter}
    for name, t in times.items():
        out[name + "_ms"] = [round(x, 2) for x in t]
        out[name + "_ms_median"] = round(sorted(t)[len(t) // 2], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, help="acting_sides | iteration: that row alone")
    ap.add_argument("--configs", default=",".join(ACTING_CONFIGS), help="acting_sides: the configs, comma-separated")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("actor_critic_probe: no GPU visible; timings are taken on the device only")
    configs = [c for c in a.configs.split(",") if c]
    if a.only == "acting_sides":
        print(json.dumps({"acting_sides": [acting_sides(c, a.repeats) for c in configs]}))
        return
    if a.only == "iteration":
        print(json.dumps({"iteration": iteration_times(a.repeats)}))
        return
    out = {"loss": [loss_times(512, A, a.iters, a.repeats) for A in (6, 18)], "window": window_time(max(8, a.iters // 10)),
           "window_recurrent": window_time(max(8, a.iters // 10), state_f32=1024),
           "acting": acting_time(a.iters),
           "acting_sides": [acting_sides(c, a.repeats) for c in configs],
           "normal_loss": [normal_loss_times(M, 1, a.iters, a.repeats) for M in (128, 512)],
           "normal_head": [normal_head_time(E, 1, a.iters, a.repeats) for E in (128, 512)],
           "mountaincar_step": [mountaincar_step_time(E, a.iters, a.repeats) for E in (128, 512)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
