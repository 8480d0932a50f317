"""CPU: the on-policy history and PPO with a RECURRENT policy against the unmodified reference.

tests/golden/online_ppo_lstm.npz (tests/golden/generate_online_lstm.py) holds what the reference produced on the seeded stream
of tests/online_lstm_restate.py — 3 envs, T = 4, episode ends inside the sequences, every next_state carrying the recurrent
layer's hx, cx and `initials`: every batch leaf of OnlineHistoryBuffer.get_train_data, calc_target_values with
timesteps = 1, and PPO._compute_grads' gradients and logged losses on a seeded fc16 -> lstm8 ActorCriticPolicy at
timesteps = T and timesteps = T / 2.  The host mirror (history/online_history.py) must reproduce the batches bit for bit,
dtypes included; the CPU trainer the targets, gradients and losses within the 1e-5 of tests/test_online_ppo_cpu.py (same
torch on both sides).  No GPU, no HIP library."""
import os

import numpy as np

from tests import scenario
from tests.golden.streams import seeded_weights
from tests.online_lstm_restate import ONLINE_LSTM_CASE as CASE, online_lstm_vector_steps

GOLD = os.path.join(scenario.GOLDEN, "online_ppo_lstm.npz")
RTOL = 1e-5


def _flat(x):
    return x.reshape((x.shape[0] * x.shape[1],) + tuple(x.shape[2:]))


def _mirror():
    from rltime_amd.general.value_log import ValueLog
    from rltime_amd.history.online_history import OnlineHistoryBuffer
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    from rltime_amd.spaces import Box, Discrete
    from rltime_amd.training.ppo import PPO
    tr = PPO.__new__(PPO)
    tr.gamma, tr.advlam, tr.vf_coef, tr.adv_norm = CASE["gamma"], CASE["advlam"], CASE["vf_coef"], True
    tr.entropy_factor, tr.entropy_anneal = CASE["entropy_factor"], None
    tr._clip_value, tr._clip_anneal = CASE["clip_value"], None
    tr.vf_scale_epsilon = None
    tr.steps, tr.total_steps = 0, 1
    tr.value_log = ValueLog()
    policy = ActorCriticPolicy.create(model_config=CASE["model"], observation_space=Box(-10, 10, (CASE["obs_dim"],), np.float32),
                                      action_space=Discrete(CASE["n_actions"]), cuda=False)
    policy.load_state_dict(seeded_weights(policy.state_dict(), CASE["weights_seed"]))
    assert policy.is_recurrent() and policy.why_not_on_device() is None
    tr.policy = tr.target_policy = policy
    T = CASE["nstep_train"]
    hist = OnlineHistoryBuffer(nstep_target=T, nstep_train=T, discount_function=tr._get_discount_function(CASE["gamma"]))
    return tr, policy, hist


def _check_batch(gold, tag, batch):
    got = {k: scenario.to_numpy(v) for k, v in scenario.flatten("", batch, {}).items()}
    want = {k[len(tag + ".batch."):]: gold[k] for k in gold.files if k.startswith(tag + ".batch.")}
    assert set(got) == set(want), (sorted(got), sorted(want))
    assert {"states.layer1_state.hx", "states.layer1_state.cx", "states.layer1_state.initials",
            "target_states.layer1_state.hx", "target_states.layer1_state.cx", "target_states.layer1_state.initials"} <= set(got)
    for key, w in want.items():
        assert got[key].dtype == w.dtype and got[key].shape == w.shape, (tag, key, got[key].dtype, w.dtype)
        assert np.array_equal(got[key], w), (tag, key)


def test_recurrent_online_history_and_ppo_match_the_reference_fixture():
    from rltime_amd.general.utils import deep_apply
    gold = np.load(GOLD)
    tr, policy, hist = _mirror()
    T = CASE["nstep_train"]
    step_no, rnd, drawn, inside = 0, 0, 0, 0
    for op in CASE["script"]:
        if op[0] == "feed":
            for samples in online_lstm_vector_steps(CASE, op[1], step_no):
                assert hist.update(samples) == {"discarded_steps": 0}
            step_no += op[1]
            continue
        tag = "r%d" % rnd
        rnd += 1
        feed = hist.needed_feed_count(op[1], CASE["num_envs"])
        assert (-1 if feed is None else feed) == int(gold[tag + ".feed_count"]), tag
        batch = hist.get_train_data(op[1])
        assert (batch is None) == bool(gold[tag + ".is_none"]), tag
        if batch is None:
            continue
        drawn += 1
        _check_batch(gold, tag, batch)
        inside += int(np.asarray(batch["states"]["layer1_state"]["initials"])[1:].sum())
        data = {k: deep_apply(v, _flat) for k, v in batch.items() if k != "extra_data"}
        targets = tr.calc_target_values(data["returns"], data["target_states"], data["target_masks"], data["nsteps"], 1)
        np.testing.assert_allclose(targets.numpy(), gold[tag + ".targets"], rtol=RTOL, atol=1e-6)
        for steps in (T, T // 2):
            policy.zero_grad()
            tr.value_log.get()
            tr._compute_grads(data["states"], targets, data["policy_outputs"], {}, steps)
            for name, prm in policy.named_parameters():
                want = gold["%s.t%d.grad.%s" % (tag, steps, name)]
                np.testing.assert_allclose(prm.grad.numpy(), want, rtol=RTOL, atol=1e-6 * float(np.abs(want).max() + 1e-12),
                                           err_msg="%s timesteps=%d" % (name, steps))
            log = tr.value_log.get()["train"]
            for key in ("value_loss", "policy_loss", "policy_entropy", "state_value_mean"):
                np.testing.assert_allclose(log[key], float(gold["%s.t%d.log.%s" % (tag, steps, key)]), rtol=RTOL, atol=1e-7,
                                           err_msg="%s timesteps=%d" % (key, steps))
        # the two sequence lengths are different computations: the fixture would not notice a `timesteps` that is ignored
        a, b = (gold["%s.t%d.grad.model.layers.1.lstm_cell.weight_hh" % (tag, s)] for s in (T, T // 2))
        assert float(np.abs(a - b).max()) > 1e-4 * float(np.abs(a).max())
    assert rnd == int(gold["rounds"]) and drawn >= 2 and inside > 0
