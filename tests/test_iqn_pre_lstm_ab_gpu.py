"""GPU: the learner evaluation and the actor's T = 1 step of IQNPolicy(injection_layer=1) — the quantile layer in FRONT of
the LSTM (configs/catch_iqn_lstm_pre.json) — on a tiny stack, three ways on the same weights, batch and quantile fractions:

  hip   gemm3._MIN_WORK = 0, the fused modules as shipped: the LSTM over B * N rows on csrc/lstm_multi.hip
  lib   MIRL_GEMM3=0, LSTM.fused = False (the torch time loop), the conv kernels off as in test_network_ab_gpu.py
  f64   oracle/network64.py Net64(injection_layer=1), pinned to the reference by tests/test_oracle_golden.py

Compared: n-step targets, their bootstrap part, loss, reported mean |td| per row, the state stored at row P of both state
trees, every parameter gradient, the global gradient norm.  Bars (test_network_ab_gpu.py's; none measured on the code under
test): forward quantities hip within 1e-4 of float64 and no further from it than max(2 x lib's distance, 1e-6); per
parameter hip's largest gradient deviation <= max(2 x lib's, 1e-6 of the parameter's largest entry); global norm within
max(2 x lib, 1e-5).  No ReLU escape and no excluded rows: the inputs (tests/iqn_pre_lstm_case.py, chosen on the CPU) have no
ReLU unit within float32 rounding of zero and a smallest double-Q margin >= 1e-3, both asserted here on the float64 result.

Shapes: CNN 16@4x4/2, 16@3x3/1 on (3, 16, 16) uint8 frames (400 features), LSTM 32, FC 32, A = 3, embedding 64;
nstep_train 6, burn-in 3, n = 2; (B, N) = (5, 3), (17, 3), (5, 4).  k_gemm3_nt_mul takes a power-of-two N only: at N = 3
the product is relu(linear) and a broadcast multiply, at N = 4 it is that kernel.

Measured on the MI355X (records, not thresholds; docs/parity.md "IQN before the LSTM ..." holds the table)."""
import json
import os

import pytest
import torch

from tests import iqn_pre_lstm_case as case
from tests.test_network_ab_gpu import _dev, _grad_facts, _kernels_that_ran, _set_mode

pytestmark = pytest.mark.gpu

T, P, NSTEP, H = case.T, case.P, case.NSTEP, case.H


def _trainer(n):
    from rltime_amd.general.config import load_config
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.general.utils import deep_dictionary_update
    from rltime_amd.train import create_actors
    from rltime_amd.training.iqn import IQN
    config = load_config("catch_iqn_lstm_pre.json")
    assert config["policy_args"]["injection_layer"] == 1 and config["training"]["args"]["double_q"]
    config["model"] = case.MODEL
    config["env_args"] = {"frame_shape": list(case.FRAME), "grid": 8, "n_actions": case.A, "visible_rows": 5}
    deep_dictionary_update(config, {"acting": {"actor_envs": 4}, "policy_args": {"num_sampling_quantiles": n},
                                    "training": {"args": {"mbatch_size": 4, "nstep_train": T, "burn_in_timesteps": P,
                                                          "nstep_target": NSTEP, "warmup_steps": 0, "total_steps": 10 ** 12,
                                                          "log_freq": 10 ** 12,
                                                          "history_mode": {"args": {"size": 4 * 64}}}}})
    ta = config["training"]["args"]
    assert ta["gamma"] == case.GAMMA and ta.get("huber_kappa", 1.0) == 1.0 and ta.get("vf_scale_epsilon") is None
    actors = create_actors(config, "cuda", device_acting=True, use_graph=False)
    tr = IQN(logger=NullLogger(), actors=actors, model_config=config["model"], policy_args=config["policy_args"])
    tr.setup(**ta)
    assert tr.target_policy is not tr.policy and tr.double_q and tr.selection_advantage_only
    for pol, sd in zip((tr.policy, tr.target_policy), case.weights()):
        have = {k: tuple(v.shape) for k, v in pol.state_dict().items()}
        assert have == {k: tuple(v.shape) for k, v in sd.items()}, have
        pol.load_state_dict(sd)
        assert pol.model.layers[0].channels_last and pol.model.layers[1].multi_sample_merge_mode == "inner"
    return tr


def _device_batch(b):
    """The block in the layout the replay's gather returns: `states` and `target_states` are rows [0, L) and [n, L + n) of
    ONE set of (R, B) device arrays (fresh copies: the burn-in writes the row-P state into them)."""
    L = case.L
    frames, state, initials = (b[k].cuda().contiguous() for k in ("frames", "state", "initials"))

    def tree(cut):
        s = cut(state)
        return {"x": cut(frames), "layer0_state": {}, "layer2_state": {},
                "layer1_state": {"hx": s[..., :H], "cx": s[..., H:], "initials": cut(initials)}}
    return {"returns": b["returns"].cuda(), "nsteps": b["nsteps"].cuda(), "target_masks": b["masks"].cuda(),
            "policy_outputs": {"actions": b["actions"].cuda()},
            "states": tree(lambda t: t[:L]), "target_states": tree(lambda t: t[NSTEP:]),
            "extra_data": {"importance_weights": b["weights"].cuda(),
                           "loss_indices": torch.zeros(L, b["returns"].shape[1], 2, dtype=torch.int64, device="cuda")}}


def _evaluate(tr, b, fr):
    """The real learner_step up to the gradients on a fresh device copy of the block."""
    got = {}
    src = {"online": case.Replay(fr["online"]), "target": case.Replay(fr["target"])}
    tr.policy.tau_source, tr.target_policy.tau_source = src["online"], src["target"]
    data = _device_batch(b)

    def train_batch(states, targets, policy_outputs, extra_data, timesteps):
        got["targets"] = targets.detach().clone()
        tr.optimizer.zero_grad(set_to_none=True)
        tr._compute_grads(states, targets, policy_outputs, extra_data, timesteps)

    def report(losses, extra):
        got["report"] = losses.detach().clone()

    log = tr.value_log.log

    def tap(key, value, *a, **k):
        if key == "qloss":
            got["loss"] = value.detach().double().clone()
        return log(key, value, *a, **k)
    keep = (tr.train_batch, tr._report_losses_if_needed, tr.value_log.log)
    tr.train_batch, tr._report_losses_if_needed, tr.value_log.log = train_batch, report, tap
    try:
        tr.learner_step(data, T, NSTEP, P, T, True, 1, 1)
    finally:
        tr.train_batch, tr._report_losses_if_needed, tr.value_log.log = keep
    torch.cuda.synchronize()
    assert src["online"].at == 3 and src["target"].at == 2           # prefix, selection, training | prefix, target pass
    got["grads"] = {k: p.grad.detach().clone() for k, p in tr.policy.named_parameters()}
    got["bootstrap"] = got["targets"] - data["returns"][P:].reshape(-1, 1)
    for key, name in (("state_P", "states"), ("target_state_P", "target_states")):
        st = data[name]["layer1_state"]
        got[key] = (st["hx"][P].clone(), st["cx"][P].clone())
    return got


def _forward_facts(o, ref):
    return {"targets_dev": _dev(o["targets"], ref["targets"]), "bootstrap_dev": _dev(o["bootstrap"], ref["bootstrap"]),
            "loss_rel_dev": abs(float(o["loss"]) - float(ref["loss"])) / abs(float(ref["loss"])),
            "report_dev": _dev(o["report"], ref["report"]),
            "state_P_dev": max(_dev(a, b) for a, b in zip(o["state_P"], ref["state_P"])),
            "target_state_P_dev": max(_dev(a, b) for a, b in zip(o["target_state_P"], ref["target_state_P"]))}


FORWARD = ("targets_dev", "bootstrap_dev", "loss_rel_dev", "report_dev", "state_P_dev", "target_state_P_dev")


@pytest.mark.parametrize("B,N", case.CASES)
def test_learner_evaluation_hip_vs_library_vs_float64(B, N, monkeypatch):
    from rltime_amd import _lib
    from rltime_amd.models.torch import lstm_seq
    tr = _trainer(N)
    b, fr = case.batch(B), case.fractions(B, N)
    lstms = [pol.model.layers[1] for pol in (tr.policy, tr.target_policy)]
    steps = []
    real = lstm_seq.lib.mirl_lstm_ms_fwd
    monkeypatch.setattr(lstm_seq.lib, "mirl_lstm_ms_fwd", lambda *a: steps.append(tuple(a[:4])) or real(*a))
    out, ran = {}, {}
    try:
        for mode in ("hip", "lib"):
            _set_mode(monkeypatch, mode)
            for m in lstms:
                m.fused = mode == "hip"
            del steps[:]
            _lib.check(_lib.lib.mirl_profile_reset())
            _lib.check(_lib.lib.mirl_profile_set(2))
            out[mode] = _evaluate(tr, b, fr)
            ran[mode] = _kernels_that_ran()
            _lib.check(_lib.lib.mirl_profile_set(0))
            if mode == "hip":
                # one entry-point call per pass (the launch table counts those), one k_lstm_ms_fwd launch per time step of
                # it: P + T steps for each net's prefix + target / training pass, T more for the online net's selection pass
                assert sorted(steps) == sorted([(P, B, N, H)] * 2 + [(T, B, N, H)] * 3), steps
                assert ran[mode].get("k_lstm_ms_fwd") == 5 and ran[mode].get("k_lstm_ms_bwd") == 1, ran[mode]
                assert bool(ran[mode].get("k_gemm3_nt_mul")) == (N & (N - 1) == 0), ran[mode]
                assert ran[mode].get("k_gemm3_nt") and ran[mode].get("k_gemm3_nn"), ran[mode]      # the LSTM's projection and d_x
            else:
                assert not steps and not [k for k in ran[mode] if k.startswith("k_lstm_ms_") or k.startswith("k_gemm3")], ran[mode]
        # the double-Q selection from the full dueling head picks the same actions (margins >= 1e-3 by construction)
        _set_mode(monkeypatch, "hip")
        for m in lstms:
            m.fused = True
        tr.selection_advantage_only = False
        full = _evaluate(tr, b, fr)
        tr.selection_advantage_only = True
    finally:
        _lib.check(_lib.lib.mirl_profile_set(0))
        _lib.check(_lib.lib.mirl_conv1_bf16_set(-1))
        for m in lstms:
            m.fused = True

    ref, _, _ = case.float64_eval(B, N, device="cuda")
    # the conditions the bars below rely on, on the float64 result itself: no excused rows, no escape
    assert ref["relu_near_zero"] == 0, ref["relu_near_zero"]
    assert ref["min_double_q_margin"] >= 1e-3, ref["min_double_q_margin"]
    facts = {"B": B, "N": N, "relu_near_zero": int(ref["relu_near_zero"]), "min_double_q_margin": ref["min_double_q_margin"],
             "scales": {"targets": float(ref["targets"].abs().max()), "bootstrap": float(ref["bootstrap"].abs().max()),
                        "loss": float(ref["loss"]), "state_P": float(ref["state_P"][0].abs().max())},
             "product_backward_kernel": ("k_gemm3_nn_qp" if ran["hip"].get("k_gemm3_nn_qp") else
                                         "k_iqn_mul_bwd" if ran["hip"].get("k_iqn_mul_bwd") else "neither"),
             "product_forward_kernel": "k_gemm3_nt_mul" if ran["hip"].get("k_gemm3_nt_mul") else
                                       "k_iqn_mul_fwd" if ran["hip"].get("k_iqn_mul_fwd") else "neither",
             "hip_kernels": {k: v for k, v in sorted(ran["hip"].items())}}
    for mode in ("hip", "lib"):
        f = _forward_facts(out[mode], ref)
        per, gn = _grad_facts(out[mode]["grads"], ref["grads"])
        f.update({"grad_dev": per, "grad_dev_max": max(v["max"] for v in per.values()), "grad_norm_rel_dev": gn})
        facts[mode] = f
    facts["full_head_selection_targets_dev"] = _dev(full["targets"], out["hip"]["targets"])
    art = os.environ.get("MIRL_TEST_ARTIFACTS")
    if art:
        os.makedirs(art, exist_ok=True)
        path = os.path.join(art, "iqn_pre_lstm_ab.json")
        have = {}
        if os.path.exists(path):
            with open(path) as fh:
                have = json.load(fh)
        have["B%d_N%d" % (B, N)] = facts
        with open(path, "w") as fh:
            json.dump(have, fh, indent=1)
    print(json.dumps({k: v for k, v in facts.items() if k not in ("hip", "lib", "hip_kernels")}))
    print(json.dumps({m: {k: v for k, v in facts[m].items() if k != "grad_dev"} for m in ("hip", "lib")}))
    print(json.dumps({k: (facts["hip"]["grad_dev"][k]["max"], facts["lib"]["grad_dev"][k]["max"]) for k in facts["hip"]["grad_dev"]}))

    # ---- the bars -------------------------------------------------------------------------------------------------------
    assert set(ref["grads"]) == set(out["hip"]["grads"]) and len(ref["grads"]) == 18
    # the stored state is zero exactly where a reset sits at row P (sequence 0 of `states`, the last of `target_states`)
    for key, row in (("state_P", P), ("target_state_P", P + NSTEP)):
        reset = (b["initials"][row] != 0).cuda()
        for mode in ("hip", "lib"):
            assert torch.equal(out[mode][key][0].abs().sum(1) == 0, reset), (key, mode)
    fh_, fl_ = facts["hip"], facts["lib"]
    for key in FORWARD:
        assert fh_[key] <= 1e-4, (key, fh_[key], fl_[key])
        assert fh_[key] <= max(2.0 * fl_[key], 1e-6), (key, fh_[key], fl_[key])
    for k, v in fh_["grad_dev"].items():
        assert v["max"] <= max(2.0 * fl_["grad_dev"][k]["max"], 1e-6), (k, v, fl_["grad_dev"][k])
    assert fh_["grad_norm_rel_dev"] <= max(2.0 * fl_["grad_norm_rel_dev"], 1e-5), (fh_["grad_norm_rel_dev"], fl_["grad_norm_rel_dev"])
    assert facts["full_head_selection_targets_dev"] <= 1e-6, facts["full_head_selection_targets_dev"]


def test_acting_two_steps_with_a_reset_against_float64(monkeypatch):
    """E = 5 envs, two consecutive actor_predict calls with a reset on env 2 between them, on the fused route and on
    fused = False, against Net64: the action values are the mean over N, the state handed on is the merged state, the
    reset env starts from zeros."""
    from rltime_amd import _lib
    from rltime_amd.policies.iqn import IQNPolicy
    from rltime_amd.models.torch import lstm_seq
    from rltime_amd.spaces import Box, Discrete
    import numpy as np
    E, N = case.E, case.N
    acting = case.acting()
    want = case.acting64("cuda")
    calls = []
    real = lstm_seq.lib.mirl_lstm_ms_fwd
    res = {}
    try:
        lstm_seq.lib.mirl_lstm_ms_fwd = lambda *a: calls.append(tuple(a[:4])) or real(*a)
        for mode in ("hip", "lib"):
            _set_mode(monkeypatch, mode)
            pol = IQNPolicy.create(model_config=case.MODEL, observation_space=Box(0, 255, case.FRAME, np.uint8),
                                   action_space=Discrete(case.A), cuda=True, dueling=True, embedding_dim=case.D,
                                   num_sampling_quantiles=N, injection_layer=1)
            pol.load_state_dict(case.weights()[0])
            lstm = pol.model.layers[1]
            lstm.fused = mode == "hip"
            pol.tau_source = case.Replay(acting["taus"])
            del calls[:]
            steps = []
            for t in range(2):
                state = pol.make_input_state(acting["frames"][t].cuda(), acting["initials"][t].numpy() != 0)
                hx = state["layer1_state"]["hx"]
                assert hx.shape == (E, H)
                if t == 1:
                    zero = hx.abs().sum(1) == 0
                    assert zero.tolist() == [e == case.RESET_ENV for e in range(E)], zero
                pred = pol.actor_predict(state, timesteps=1, as_numpy=False)
                assert pred["qvalues"].shape == (E, case.A)
                steps.append({"q": pred["qvalues"].clone(), "h": lstm.last_state[0].clone(), "c": lstm.last_state[1].clone(),
                              "h_in": hx.clone()})
            assert calls == ([(1, E, N, H)] * 2 if mode == "hip" else []), calls
            # the state handed to step 1 is step 0's merged state, zeroed on the reset env
            keep = (1.0 - acting["initials"][1]).cuda().unsqueeze(-1)
            assert torch.equal(steps[1]["h_in"], steps[0]["h"] * keep)
            res[mode] = steps
    finally:
        lstm_seq.lib.mirl_lstm_ms_fwd = real
        _lib.check(_lib.lib.mirl_conv1_bf16_set(-1))
    facts = {}
    for mode in ("hip", "lib"):
        facts[mode] = {"%s%d" % (k, t): _dev(res[mode][t][k], want[t][k]) for t in range(2) for k in ("q", "h", "c")}
    print(json.dumps(facts))
    for key, dh in facts["hip"].items():
        assert dh <= 1e-4, (key, dh, facts["lib"][key])
        assert dh <= max(2.0 * facts["lib"][key], 1e-6), (key, dh, facts["lib"][key])
