"""GPU: recurrent A2C / PPO on the device path, end to end.

(a) wiring: the device actor runs a seeded fc16 -> lstm16 policy on device CartPole (5 envs, episodes of 4 steps, so that
    resets fall inside the sequences), eagerly and through GraphedStep; DeviceOnlineHistory builds one T = 4 window from its
    vector steps.  Re-evaluating the window's states with unchanged weights — the stored recurrent state of row 0, the stored
    `initials` of every row — reproduces the acting-time [log-probability | value] block within 1e-4 of max(|w|, 1)
    (docs/parity.md's per-op bar), at timesteps = T and, segment by segment from the stored states of rows 0 and 2, at
    timesteps = 2.  Controls: with the state rows taken one slot late, and with the initials zeroed, the same comparison
    misses that bar by at least 100x — the check sees both blocks.  (Weight seed and scale were chosen on a CPU copy of the
    policy with the same helper functions.)
(b) one learner_step of A2C and of PPO (fc16 -> lstm16, T = 4, B = 8, initials set in mid-sequence rows; 1 and 2 minibatches,
    rnn_steps_train 4 and 2) against the same step in float64 on a CPU copy: the logged losses inside the loss kernel's bounds
    on its operands, losses and every parameter's gradient within 1e-4, as tests/test_ppo_device_gpu.py holds the MLP to.
(c) catch_ppo_lstm.json runs two learner iterations at 4 envs, T = 8: finite losses and weights, the window kernel twice, a
    state ring of S = 1024; a minibatch count that cannot hold whole sequences is refused before anything is built."""
import copy
import json
import math

import numpy as np
import pytest
import torch

from tests import actor_critic_restate as R
from tests.golden.streams import seeded_weights

pytestmark = pytest.mark.gpu

BAR = 1e-4
LSTM16 = {"type": "sequential", "args": {"layer_configs": [{"type": "fc", "args": {"fc_size": 16}},
                                                           {"type": "lstm", "args": {"num_units": 16}}]}}
WIRING_SEED, WIRING_SCALE = 11, 4.0


def _profile(on):
    from rltime_amd import _lib
    if on:
        _lib.check(_lib.lib.mirl_profile_reset())
    _lib.check(_lib.lib.mirl_profile_set(2 if on else 0))


def _ran():
    from rltime_amd import _lib
    return {r["name"]: r["calls"] for r in _lib.profile_table()}


# ---- (a) the wiring ----------------------------------------------------------------------------------------------------------------
def wiring_weights(policy):
    """Seeded weights with every matrix scaled up: an LSTM at its initialisation scale barely reads its state, and the
    controls need a policy whose outputs depend on it."""
    sd = seeded_weights(policy.state_dict(), WIRING_SEED)
    return {k: (v * WIRING_SCALE if v.dim() == 2 else v) for k, v in sd.items()}


def reevaluate(policy, states, actions, steps):
    """states: the (T, B, ...) pytree of a window; -> (log-probabilities, values) (T, B) of `actions` from ONE pass of the
    policy at timesteps = `steps`.  The model reads a flat batch as (steps, rows / steps) — time-major — and starts every
    column from the state stored with its first row, so the window's T / steps segments are laid side by side:
    column k B + b holds rows steps k ... steps k + steps - 1 of sequence b."""
    T, B = actions.shape
    K = T // steps

    def lay(x):            # (T, B, ...) -> (steps, K * B, ...) -> flat
        x = x.reshape((K, steps, B) + tuple(x.shape[2:])).transpose(0, 1)
        return x.reshape((steps * K * B,) + tuple(x.shape[3:]))
    from rltime_amd.general.utils import deep_apply
    with torch.no_grad():
        logits, values = policy.get_logits_and_state_value(deep_apply(states, lay), steps)
        logp = torch.log_softmax(logits.double(), dim=-1).gather(1, lay(actions).long().unsqueeze(1)).squeeze(1)

    def back(y):           # flat (steps, K, B) -> (T, B)
        return y.reshape(steps, K, B).transpose(0, 1).reshape(T, B)
    return back(logp), back(values.double())


def one_slot_late(states, target_states):
    """The window's states with the recurrent STATE rows (hx, cx) of the next slot: row t + 1 for t < T - 1, and the last
    row's own target state (it covers one step: the next_state of the transition itself).  x and initials stay."""
    out = {}
    for k, sub in states.items():
        if k == "x" or not sub:
            out[k] = sub
            continue
        out[k] = {name: (v if name == "initials" else torch.cat([v[1:], target_states[k][name][-1:]])) for name, v in sub.items()}
    return out


def initials_zeroed(states):
    return {k: (sub if k == "x" or not sub else dict(sub, initials=torch.zeros_like(sub["initials"]))) for k, sub in states.items()}


def worst(got, want):
    """Largest |got - want| / max(|want|, 1) over (log-probabilities, values)."""
    return max(float(((g.double() - w.double()).abs() / w.double().abs().clamp(min=1.0)).max()) for g, w in zip(got, want))


def _gae():
    def discount(nstep, reward, po):
        v = po["values"]
        return (0.99 ** nstep) * (0.95 ** (nstep - 1)) * (v + 0.95 * (reward - v))
    discount.gamma, discount.lam = 0.99, 0.95
    return discount


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graphed"])
def test_reevaluating_the_window_reproduces_acting(use_graph):
    from rltime_amd.general.config import load_config
    from rltime_amd.history.online_device import DeviceOnlineHistory
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    from rltime_amd.train import create_actors
    T, E = 4, 5
    cfg = load_config("cartpole_ppo_device.json")
    cfg["acting"]["actor_envs"], cfg["model"] = E, LSTM16
    cfg["env_args"]["max_episode_steps"] = 4
    actors = create_actors(cfg, "cuda", use_graph=use_graph)
    hist = None
    try:
        obs_space, act_space = actors.get_spaces()
        torch.manual_seed(3)
        policy = ActorCriticPolicy.create(model_config=cfg["model"], observation_space=obs_space, action_space=act_space, cuda=True)
        policy.load_state_dict(wiring_weights(policy))
        assert policy.is_recurrent() and policy.why_not_on_device() is None
        actors.set_actor_policy(policy)
        first, second = actors.get_samples(E * 6), actors.get_samples(E * 3)
        steps = first.vector_steps + second.vector_steps
        assert len(steps) == 9 and (actors._graphed is not None) == use_graph and actors._fast is False
        assert all(tuple(s["state"].shape) == (E, 32) and tuple(s["initials"].shape) == (E,) for s in steps)
        done_at = [bool(s["dones"].any()) for s in steps]
        # the history is fed from vector step k on: its first window (an env's first ever transition starts from its own
        # next_state, not from the state it was acted in) is drawn and dropped, the second holds transitions k + 4 ... k + 7,
        # whose states are the next_states of steps k + 3 ... k + 6; k puts a reset on row 1 or 3: inside the sequence and inside
        # a two-step segment (a reset on a segment's first row is already in its stored, zeroed state)
        k = next((k for k in (0, 1) if done_at[k + 4] or done_at[k + 6]), None)
        assert k is not None, "no reset falls on row 1 or 3 of a window: the seeded CartPole episodes moved (dones per step %s)" % done_at
        hist = DeviceOnlineHistory(nstep_target=T, nstep_train=T, discount_function=_gae())
        from rltime_amd.acting.acting_interface import DeviceSamples
        fed = DeviceSamples(first.example_state, E, 0)
        fed.vector_steps = steps[k:k + 8]
        hist.update(fed)
        assert hist.get_train_data(E) is not None
        batch = hist.get_train_data(E)
        assert batch is not None and hist._served == list(range(E))
        acted = [steps[k + 4 + t] for t in range(T)]
        po = batch["policy_outputs"]
        want = (torch.stack([s["policy"][:, 0] for s in acted]), torch.stack([s["policy"][:, 1] for s in acted]))
        assert torch.equal(po["action_log_probs"], want[0]) and torch.equal(po["values"], want[1])
        assert torch.equal(po["actions"], torch.stack([s["actions"] for s in acted]))
        ini = batch["states"]["layer1_state"]["initials"]
        assert float(ini[1::2].sum()) > 0 and float((1 - ini).sum()) > 0, "no reset inside the window"
        assert torch.equal(ini, torch.stack([steps[k + 3 + t]["initials"] for t in range(T)]))
        for seg in (T, 2):
            err = worst(reevaluate(policy, batch["states"], po["actions"], seg), want)
            print("FIGURE wiring %s timesteps=%d worst rel %.3e" % ("graphed" if use_graph else "eager", seg, err))
            assert err <= BAR, (seg, err)
            late = worst(reevaluate(policy, one_slot_late(batch["states"], batch["target_states"]), po["actions"], seg), want)
            zeroed = worst(reevaluate(policy, initials_zeroed(batch["states"]), po["actions"], seg), want)
            print("FIGURE wiring control timesteps=%d: state one slot late %.3e, initials zeroed %.3e" % (seg, late, zeroed))
            assert late >= 100 * BAR and zeroed >= 100 * BAR, (seg, late, zeroed)
    finally:
        actors.close()
        if hist is not None:
            hist.close()


# ---- (b) one learner step against float64 ---------------------------------------------------------------------------------------
def _trainer(kind, minibatches, rnn_steps):
    from rltime_amd.general.config import load_config
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.general.type_registry import get_registered_type
    from rltime_amd.general.utils import deep_dictionary_update
    from rltime_amd.train import create_actors
    cfg = load_config("cartpole_%s_device.json" % kind)
    deep_dictionary_update(cfg, {"acting": {"actor_envs": 8},
                                 "training": {"args": {"nstep_train": 4, "epochs": 1, "minibatches": minibatches,
                                                       "rnn_steps_train": rnn_steps, "total_steps": 1000}}})
    cfg["model"] = LSTM16
    actors = create_actors(cfg, "cuda")
    tr = get_registered_type("trainers", kind)(logger=NullLogger(echo=False), actors=actors, model_config=cfg["model"],
                                               policy_args=cfg["policy_args"])
    tr.setup(**cfg["training"]["args"])
    return tr


def _batch(tr, T=4, B=8, H=16):
    g = torch.Generator().manual_seed(5)
    obs = (torch.randn(2, T, B, 4, generator=g) * 0.5).cuda()

    def tree(i):
        ini = (torch.rand(T, B, generator=g) < 0.3).float()
        ini[1, 0] = ini[2, 3] = ini[3, 5] = 1.0                   # episode starts inside sequences
        ini[:, 1] = 0.0                                           # and one sequence without any
        keep = (1 - ini).unsqueeze(-1)
        return {"x": obs[i], "layer0_state": {},
                "layer1_state": {"hx": (torch.randn(T, B, H, generator=g) * 0.5 * keep).cuda(),
                                 "cx": (torch.randn(T, B, H, generator=g) * keep).cuda(), "initials": ini.cuda()}}
    states, target_states = tree(0), tree(1)
    flat = lambda x: x.reshape((T * B,) + tuple(x.shape[2:]))                                  # noqa: E731
    from rltime_amd.general.utils import deep_apply
    with torch.no_grad():
        logits, values = tr.policy.get_logits_and_state_value(deep_apply(states, flat), 1)
        dist = torch.distributions.Categorical(logits=logits)
        actions = dist.sample()
        logp = dist.log_prob(actions) + torch.randn(T * B, generator=g).cuda() * 0.2        # ratios on both sides of the clip range
    n = torch.tensor([min(4, T - t) for t in range(T)], dtype=torch.float32).unsqueeze(1).expand(T, B).contiguous()
    mask = (torch.rand(T, B, generator=g) > 0.2).float()
    return {"states": states, "target_states": target_states, "returns": (torch.randn(T, B, generator=g) * 0.5).cuda(),
            "nsteps": n.cuda(), "target_masks": mask.cuda(),
            "policy_outputs": {"actions": actions.to(torch.int32).reshape(T, B), "action_log_probs": logp.reshape(T, B),
                               "values": (values + torch.randn(T * B, generator=g).cuda() * 0.1).reshape(T, B)},
            "extra_data": {}}


def _float64_minibatch(tr, ref, batch, kind, rows, rnn_steps):
    """The rows `rows` of the flattened batch as one training pass in float64 on the CPU copy -> (logged scalars, gradients)."""
    from oracle import qmath
    from rltime_amd.general.utils import deep_apply
    flat = lambda x: x.reshape((-1,) + tuple(x.shape[2:])).cpu()                              # noqa: E731
    f64 = lambda x: x.double() if x.is_floating_point() else x                                # noqa: E731
    data = deep_apply(deep_apply({k: v for k, v in batch.items() if k != "extra_data"}, flat), f64)
    with torch.no_grad():
        boot = ref.get_state_value(data["target_states"], 1)          # every target row from its own stored state
    ns = data["nsteps"]
    targets = data["returns"] + (tr.gamma ** ns) * (tr.advlam ** (ns - 1)) * boot * data["target_masks"]
    idx = torch.as_tensor(rows)
    pick = lambda y: deep_apply(y, lambda x: x[idx])                                            # noqa: E731
    po = pick(data["policy_outputs"])
    lp, vals, ent = ref.evaluate_actions(pick(data["states"]), rnn_steps, po["actions"].long())
    ppo = kind == "ppo"
    total, vloss, gain = qmath.actor_critic_loss(lp, vals, ent, targets[idx], po["values"], po["action_log_probs"] if ppo else None,
                                                 tr.vf_coef, tr._calc_entropy_factor(), tr.adv_norm,
                                                 tr._calc_clip_value() if ppo else None)
    ref.zero_grad()
    total.backward()
    log = {"value_loss": vloss.item(), "policy_loss": -gain.item(), "policy_entropy": ent.mean().item(), "state_value_mean": vals.mean().item()}
    return log, {k: p.grad.clone() for k, p in ref.named_parameters()}


@pytest.mark.parametrize("rnn_steps", [4, 2])
@pytest.mark.parametrize("minibatches", [1, 2])
@pytest.mark.parametrize("kind", ["a2c", "ppo"])
def test_one_recurrent_learner_step_matches_float64(kind, minibatches, rnn_steps):
    from rltime_amd.training import qops
    tr = _trainer(kind, minibatches, rnn_steps)
    try:
        assert type(tr.history_buffer).__name__ == "DeviceOnlineHistory" and tr.policy.is_cuda() and tr.policy.is_recurrent()
        assert tr.rnn_steps_train == rnn_steps
        batch = _batch(tr)
        ref = copy.deepcopy(tr.policy).cpu().double()
        tr.set_lr(0.0)                        # the minibatches of one step are then all evaluated on the weights `ref` holds
        seen, taken, per_batch = [], [], []
        real_loss, real_indexes, real_grads = qops.ac_loss, tr.get_train_indexes, tr._compute_grads

        def tap(logits, values, actions, targets, acting_values, **kw):
            seen.append((logits.detach().clone(), values.detach().clone(), actions.clone(), targets.clone(), acting_values.clone(), kw))
            return real_loss(logits, values, actions, targets, acting_values, **kw)

        def indexes(*a):
            taken.append(real_indexes(*a))
            return taken[-1]

        def grads(*a, **k):
            tr.value_log.get()
            real_grads(*a, **k)
            per_batch.append((tr.value_log.get()["train"], {n: p.grad.detach().cpu().double() for n, p in tr.policy.named_parameters()}))
        qops.ac_loss, tr.get_train_indexes, tr._compute_grads = tap, indexes, grads
        _profile(True)
        np.random.seed(17)
        try:
            tr.learner_step({k: (dict(v) if isinstance(v, dict) else v) for k, v in batch.items()}, 4, 4, rnn_steps_train=rnn_steps,
                            epochs=1, minibatches=minibatches)
            torch.cuda.synchronize()
            ran = _ran()
        finally:
            qops.ac_loss = real_loss
            del tr.get_train_indexes, tr._compute_grads
            _profile(False)
        assert ran.get("k_ac_loss", 0) == minibatches and len(seen) == len(per_batch) == minibatches and len(taken) == 1
        mini = 32 // minibatches
        tag = "%s mb=%d rnn=%d" % (kind, minibatches, rnn_steps)
        for i in range(minibatches):
            # (one minibatch: the shuffle is consumed but the batch is taken as it is)
            rows = np.asarray(taken[0][i * mini:(i + 1) * mini]) if minibatches > 1 else np.arange(32)
            # whole sequences, time-major: what the recurrent index shuffle promises the model
            assert np.array_equal(rows.reshape(4, -1) // 8, np.arange(4)[:, None] * np.ones((1, mini // 4), dtype=np.int64))
            logged, got = per_batch[i]
            logits, values, actions, targets, acting, kw = seen[i]
            np32 = lambda t: t.float().cpu().numpy()                                              # noqa: E731
            old = kw["old_log_probs"]
            want = R.loss(np32(logits), np32(values), actions.cpu().numpy().astype(np.int64), np32(targets), np32(acting),
                          None if old is None else np32(old), kw["vf_coef"], kw["entropy_factor"], kw["clip_value"], kw["adv_norm"])
            b = R.loss_bounds(want, kw["vf_coef"], kw["entropy_factor"], old is not None)["stats"]
            for j, key in ((1, "value_loss"), (2, "policy_loss"), (3, "policy_entropy"), (4, "state_value_mean")):
                ratio = abs(float(logged[key]) - want["stats"][j]) / b[j]
                print("RATIO lstm_step.%s %s #%d %.4f" % (key, tag, i, ratio))
                assert ratio <= 1.0, key
            log64, grads64 = _float64_minibatch(tr, ref, batch, kind, rows, rnn_steps)
            for key, w in log64.items():
                err = abs(float(logged[key]) - w) / max(abs(w), 1.0)
                print("FIGURE lstm_step.%s %s #%d rel %.3e" % (key, tag, i, err))
                assert err <= BAR, (key, float(logged[key]), w)
            assert set(got) == set(grads64)
            for name, w in grads64.items():
                top = float(w.abs().max())
                err = float((got[name] - w).abs().max()) / max(top, 1e-30)
                print("FIGURE lstm_grad %s %s #%d rel-to-max %.3e" % (name, tag, i, err))
                assert top > 0 and err <= BAR, name
    finally:
        tr.actors.close()
        tr.history_buffer.close()


# ---- (c) the shipped config ------------------------------------------------------------------------------------------------------
def test_catch_ppo_lstm_config_runs_two_iterations(tmp_path):
    from rltime_amd.train import train_from_config
    update = {"training": {"args": {"nstep_train": 8, "total_steps": 64, "log_freq": 32}}}
    _profile(True)
    try:
        trainer = train_from_config("catch_ppo_lstm.json", num_envs=4, log_dir=str(tmp_path), log_name="run", seed=3, conf_update=update)
        torch.cuda.synchronize()
        ran = _ran()
    finally:
        _profile(False)
    hist = trainer.history_buffer
    assert type(hist).__name__ == "DeviceOnlineHistory" and trainer.policy.is_recurrent()
    assert hist._layout.state_f32 == 1024 and hist._layout.has_initials
    rows = [json.loads(line) for line in open(tmp_path / "run" / "train.json")]
    assert len(rows) == 2 and rows[-1]["this_interval"]["steps_trained"] == 4 * 32                       # 4 epochs x (4 envs x 8 steps)
    for key in ("value_loss", "policy_loss", "policy_entropy", "state_value_mean", "grad_norm"):
        assert math.isfinite(rows[-1]["train"][key]), (key, rows[-1]["train"])
    assert all(bool(torch.isfinite(p).all()) for p in trainer.policy.parameters())
    # 16 vector steps, 2 windows, 2 iterations x 4 epochs x 4 minibatches of one whole sequence
    assert ran.get("k_actor_head_ac", 0) >= 16 and ran.get("k_online_window", 0) == 2 and ran.get("k_ac_loss", 0) == 2 * 16, ran


def test_catch_ppo_lstm_state_ring_and_geometry_refusal():
    from rltime_amd.general.config import load_config
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.general.type_registry import get_registered_type
    from rltime_amd.general.utils import deep_dictionary_update
    from rltime_amd.train import create_actors

    def build(update):
        cfg = load_config("catch_ppo_lstm.json")
        deep_dictionary_update(cfg, {"acting": {"actor_envs": 4}, "training": {"args": {"nstep_train": 8, "total_steps": 64}}})
        deep_dictionary_update(cfg, update)
        actors = create_actors(cfg, "cuda")
        tr = get_registered_type("trainers", "ppo")(logger=NullLogger(echo=False), actors=actors, model_config=cfg["model"],
                                                   policy_args=cfg["policy_args"])
        return cfg, actors, tr
    for update, match in (({"training": {"args": {"minibatches": 3}}}, "recurrent"),
                          ({"training": {"args": {"rnn_steps_train": 3}}}, "recurrent"),
                          ({"training": {"args": {"burn_in_timesteps": 2}}}, "burn_in_timesteps"),
                          ({"training": {"args": {"rnn_bootstrap": True}}}, "rnn_bootstrap")):
        cfg, actors, tr = build(update)
        try:
            with pytest.raises(ValueError, match=match):
                tr.setup(**cfg["training"]["args"])
            assert getattr(tr, "history_buffer", None) is None and getattr(tr, "optimizer", None) is None      # nothing was built
        finally:
            actors.close()
    cfg, actors, tr = build({})
    try:
        tr.setup(**cfg["training"]["args"])
        while not tr.loop_iteration():
            pass
        ring = tr.history_buffer._rings["state"]
        assert type(tr.history_buffer).__name__ == "DeviceOnlineHistory" and ring.shape[1:] == (4, 1024) and ring.dtype == torch.float32
        assert tuple(tr.history_buffer._rings["initials"].shape) == (ring.shape[0], 4)
    finally:
        actors.close()
        tr.history_buffer.close()


def test_cartpole_ppo_lstm_device_config_sets_up_and_takes_a_learner_step():
    """The second shipped recurrent config as it stands (16 envs, T = 32, 4 minibatches of 4 whole sequences): it passes the
    geometry check, builds a DeviceOnlineHistory with a state ring of S = 2 x 64 and takes one learner step with finite losses."""
    from rltime_amd.general.config import load_config, validate_config
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.general.type_registry import get_registered_type
    from rltime_amd.train import create_actors
    cfg = load_config("cartpole_ppo_lstm_device.json")
    validate_config(cfg)
    args = cfg["training"]["args"]
    assert cfg["acting"]["actor_envs"] == 16 and args["minibatches"] == 4 and args["nstep_train"] == 32
    assert [c["type"] for c in cfg["model"]["args"]["layer_configs"]] == ["fc", "lstm"]
    actors = create_actors(cfg, "cuda")
    tr = get_registered_type("trainers", "ppo")(logger=NullLogger(echo=False), actors=actors, model_config=cfg["model"],
                                               policy_args=cfg["policy_args"])
    try:
        tr.setup(**args)
        assert tr.policy.is_recurrent() and tr.policy.is_cuda() and type(tr.history_buffer).__name__ == "DeviceOnlineHistory"
        tr.value_log.get()
        while not tr.loop_iteration():
            pass
        torch.cuda.synchronize()
        assert tuple(tr.history_buffer._rings["state"].shape[1:]) == (16, 128)
        logged = tr.value_log.get()["train"]
        for key in ("value_loss", "policy_loss", "policy_entropy", "state_value_mean", "grad_norm"):
            assert math.isfinite(float(logged[key])), (key, logged)
        assert all(bool(torch.isfinite(p).all()) for p in tr.policy.parameters())
    finally:
        actors.close()
        if getattr(tr, "history_buffer", None) is not None:
            tr.history_buffer.close()
