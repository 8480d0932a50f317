"""CPU: the float64 restatements of the actor-critic kernels (tests/actor_critic_restate.py) are what the reference computes.

  window   OnlinePlan (history/online_device.py, the host bookkeeping) + restate.window on NumPy rings against
           OnlineHistoryBuffer AND oracle.replay.OracleOnline on seeded random streams fed with np.float64 rewards (the mirror's
           own arithmetic is then float64): states, target states, actions, policy outputs, nsteps and masks bit for bit, returns
           equal after rounding to float32 (they are equal in float64 too), feed decisions, discards and served order.
  loss     restate.loss against float64 autograd of oracle.qmath.actor_critic_loss: A2C and PPO, adv_norm on and off, rows
           planted exactly on both clip bounds and rows with ratio exactly 1.
  head     restate.head against torch.distributions.Categorical and the inverse-CDF choice.
  operands for exactly the operands the GPU tests send, no row's u S lies within the head's rounding bound of a cumulative
           boundary: the GPU test excludes 0 rows.
No GPU, no HIP library."""
import numpy as np
import pytest
import torch

from tests import actor_critic_restate as R
from tests import scenario


# ---- window ------------------------------------------------------------------------------------------------------------------
def _vector_step(case, t, E):
    g = np.random.RandomState(100000 * case + t)
    return {"obs": g.randn(E, 3).astype(np.float32), "actions": g.randint(0, 4, size=E).astype(np.int64),
            "values": g.randn(E).astype(np.float32), "logp": (-g.rand(E)).astype(np.float32),
            # (float32 numbers held as np.float64: the device rings keep rewards in float32)
            "rewards": g.choice([0.0, 1.0, -0.5, 0.25], size=E).astype(np.float64), "dones": g.rand(E) < 0.15}


def _dicts(step, E):
    return [{"policy_output": {"actions": step["actions"][e], "values": step["values"][e], "action_log_probs": step["logp"][e]},
             "next_state": {"x": step["obs"][e], "layer0_state": {}}, "reward": step["rewards"][e], "done": bool(step["dones"][e]),
             "info": {}, "env_id": e} for e in range(E)]


def test_window_restatement_equals_the_host_history_and_the_oracle():
    from oracle import replay as orc
    from rltime_amd.history.online_device import OnlinePlan
    from rltime_amd.history.online_history import OnlineHistoryBuffer
    rng = np.random.RandomState(11)
    batches = 0
    for case in range(30):
        E, T = int(rng.randint(1, 6)), int(rng.randint(1, 8))
        n = int(rng.choice([1, 2, T, T + 3]))
        cap_steps = int(rng.choice([5000, 3 * T, T + 1]))
        gamma, lam = 0.97, float(rng.choice([1.0, 0.9]))
        kw = dict(max_delayed_steps=cap_steps, fixed_target=True, nstep_target=n, nstep_train=T)
        host = OnlineHistoryBuffer(discount_function=orc.make_gae_discount(gamma, lam), **kw)
        ref = orc.OracleOnline(discount_function=orc.make_gae_discount(gamma, lam), **kw)
        plan = OnlinePlan(T, cap_steps)
        cap = 64                                    # ring slots: more than the test ever keeps pending
        rings = {"obs": np.zeros((cap, E, 3), np.float32), "actions": np.zeros((cap, E), np.int64), "rewards": np.zeros((cap, E), np.float32),
                 "dones": np.zeros((cap, E), np.uint8), "logp": np.zeros((cap, E), np.float32), "values": np.zeros((cap, E), np.float32)}
        t = 0
        for _ in range(45):
            if rng.rand() < 0.7:
                step = _vector_step(case, t, E)
                a, b = host.update(_dicts(step, E)), ref.update(_dicts(step, E))
                lost = plan.feed(range(E))
                assert a == b == {"discarded_steps": lost}
                assert plan.live_steps() <= cap
                for k in rings:
                    rings[k][t % cap] = step[k]
                t += 1
                continue
            B = int(rng.randint(1, E + 2))
            feed = host.needed_feed_count(B, E)
            assert feed == ref.needed_feed_count(B, E) == (None if plan.sequences_ready() >= B else E)
            a, b = host.get_train_data(B), ref.get_train_data(B)
            served = plan.serve(B)
            assert (a is None) == (b is None) == (served is None)
            if a is None:
                continue
            batches += 1
            assert plan.last_env == host.last_env == ref.last_env
            rows = np.array([(env, start % cap, own) for env, start, own in served], dtype=np.int32)
            w = R.window(T, B, E, cap, n, gamma, lam, rows, rings["obs"], rings["actions"], rings["rewards"], rings["dones"],
                         rings["logp"], rings["values"])
            for other in (a, b):
                flat = {k: scenario.to_numpy(v) for k, v in scenario.flatten("", other, {}).items()}
                assert np.array_equal(flat["states.x"], w["states"]) and np.array_equal(flat["target_states.x"], w["target_states"])
                assert np.array_equal(flat["policy_outputs.actions"], w["actions"])
                assert np.array_equal(flat["policy_outputs.action_log_probs"], w["action_log_probs"])
                assert np.array_equal(flat["policy_outputs.values"], w["values"])
                assert np.array_equal(flat["nsteps"], w["nsteps"]) and np.array_equal(flat["target_masks"], w["target_masks"])
                assert flat["returns"].dtype == np.float64
                assert np.array_equal(flat["returns"].astype(np.float32), w["returns"].astype(np.float32))
                assert np.array_equal(flat["returns"], w["returns"])
    assert batches >= 60


# ---- loss --------------------------------------------------------------------------------------------------------------------
def _plant(lp, old, rows, x):
    """old[row] = lp[row] - x on the rows where that difference is exact, so that lp - old is exactly x there: a short x
    (a few bits) makes exp(x) one float64 number, from which the test takes its clip value — the rows then sit exactly on
    that clip bound.  -> the rows planted."""
    done = []
    for i in rows:
        if lp[i] - (lp[i] - x) == x:
            old[i] = lp[i] - x
            done.append(i)
    return done


@pytest.mark.parametrize("gain_kind", ["a2c", "ppo_hi", "ppo_lo"])
@pytest.mark.parametrize("adv_norm", [False, True])
@pytest.mark.parametrize("M,A", [(2, 2), (7, 6), (64, 18), (33, 1)])
def test_loss_restatement_equals_float64_autograd(gain_kind, adv_norm, M, A):
    from oracle import qmath
    ppo = gain_kind != "a2c"
    g = np.random.RandomState(7 * M + A + 100 * ppo + 1000 * adv_norm)
    case = R.loss_case(M, A, seed=int(g.randint(1 << 30)), ppo=False)
    vf, ef, c = 0.5, 0.01, 0.2
    z = torch.tensor(case["logits"].astype(np.float64), requires_grad=True)
    v = torch.tensor(case["values"].astype(np.float64), requires_grad=True)
    act = torch.from_numpy(case["actions"].astype(np.int64))
    tg, base = (torch.from_numpy(case[k].astype(np.float64)) for k in ("targets", "acting"))
    dist = torch.distributions.Categorical(logits=z)
    lp = dist.log_prob(act)
    old, on_bound, ones = None, [], []
    if ppo:
        lp_np = lp.detach().numpy().copy()
        old_np = lp_np + g.randn(M) * 0.3
        ones = list(range(0, M, 5))
        old_np[ones] = lp_np[ones]                               # ratio exactly 1
        free = [i for i in range(M) if i not in ones]
        if A > 1 and len(free) >= 4:
            # the clip value comes from the planted ratio: 1 + (r - 1) == r for r in [1, 2) and 1 - (1 - r) == r for r in [0.5, 1)
            on_bound = _plant(lp_np, old_np, free[:8], 0.1875 if gain_kind == "ppo_hi" else -0.25)
            assert len(on_bound) >= 2
            r0 = float(R.ratio_of(lp_np, old_np)[on_bound[0]])
            c = r0 - 1.0 if gain_kind == "ppo_hi" else 1.0 - r0
            assert (1.0 + c == r0) if gain_kind == "ppo_hi" else (1.0 - c == r0)
        old = torch.from_numpy(old_np)
        ratio = torch.exp(lp.detach() - old)
        assert all(float(ratio[i]) == 1.0 for i in ones)
        if on_bound:
            on_bound = [i for i in on_bound if float(ratio[i]) == r0]
            assert len(on_bound) >= 2
    total, vloss, gain = qmath.actor_critic_loss(lp, v, dist.entropy(), tg, base, old, vf, ef, adv_norm, c if ppo else None)
    total.backward()
    r = R.loss(case["logits"], case["values"], case["actions"], case["targets"], case["acting"], None if old is None else old.numpy(),
               vf, ef, c if ppo else None, adv_norm, round_logp=False, log_probs=lp.detach().numpy() if ppo else None)
    want = np.array([x.item() for x in (total.detach(), vloss.detach(), -gain.detach(), dist.entropy().mean().detach(), v.mean().detach())])
    np.testing.assert_allclose(r["stats"], want, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(r["dlogits"], z.grad.numpy(), rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(r["dvalues"], v.grad.numpy(), rtol=1e-12, atol=1e-16)
    if ppo:
        assert np.array_equal(r["ratio"], ratio.numpy())
        # on a bound the two terms tie and the full gradient flows: coef = ratio * adv there
        for i in on_bound + ones:
            assert r["coef"][i] == r["ratio"][i] * r["adv"][i]


def test_loss_restatement_rounds_the_log_probability_once():
    """round_logp (what the kernel does): the log-probability is the float32 nearest to the float64 one, and feeding it back
    as the old log-probability gives ratio exactly 1 and the A2C form of the policy gradient."""
    case = R.loss_case(257, 6, seed=5, ppo=True)
    a2c = R.loss(case["logits"], case["values"], case["actions"], case["targets"], case["acting"], None, 0.5, 0.01, None, True)
    assert np.array_equal(a2c["log_probs"], a2c["log_probs"].astype(np.float32).astype(np.float64))
    ppo = R.loss(case["logits"], case["values"], case["actions"], case["targets"], case["acting"], a2c["log_probs"], 0.5, 0.01, 0.2, True)
    assert np.all(ppo["ratio"] == 1.0) and np.array_equal(ppo["dlogits"], a2c["dlogits"])
    # the shipped PPO operands: rows on both sides of the clip range and rows with ratio exactly 1
    full = R.loss(case["logits"], case["values"], case["actions"], case["targets"], case["acting"], case["old"], 0.5, 0.0, 0.2, True)
    clipped = (full["coef"] == 0) & (full["adv"] != 0)
    assert clipped.sum() >= 10 and np.all(full["dlogits"][clipped] == 0)
    assert (full["ratio"] == 1.0).sum() >= 10 and (full["ratio"] > 1.2).sum() >= 5 and (full["ratio"] < 0.8).sum() >= 5
    assert np.all(full["dvalues"][case["targets"] == case["values"]] == 0) and (case["targets"] == case["values"]).sum() >= 10


# ---- head --------------------------------------------------------------------------------------------------------------------
def test_head_restatement_equals_categorical_and_the_inverse_cdf():
    for E, A in [(257, 6), (65, 18), (64, 64), (3, 2), (5, 1)]:
        logits, _, u = R.head_case(E, A)
        actions, logp = R.head(logits, u)
        dist = torch.distributions.Categorical(logits=torch.from_numpy(logits.astype(np.float64)))
        np.testing.assert_allclose(logp, dist.log_prob(torch.from_numpy(actions)).numpy(), rtol=1e-12, atol=1e-13)
        # the inverse-CDF choice on normalised probabilities: the smallest a whose cumulative probability exceeds u
        cdf = np.cumsum(dist.probs.numpy(), axis=1)
        margin, bound = R.head_margin(logits, u)
        clear = margin > 1e-9
        want = np.minimum((cdf <= u.astype(np.float64)[:, None]).sum(axis=1), A - 1)
        assert clear.sum() >= E - 1 and np.array_equal(actions[clear], want[clear])
        greedy, glogp = R.head(logits, greedy=True)
        assert np.array_equal(greedy, dist.logits.argmax(dim=1).numpy())
        np.testing.assert_allclose(glogp, dist.log_prob(torch.from_numpy(greedy)).numpy(), rtol=1e-12, atol=1e-13)
    logits, _, first = R.head_tie_case(33, 6)
    assert np.array_equal(R.head(logits, greedy=True)[0], first)
    assert R.head(np.zeros((1, 4), np.float32), np.array([0.0], np.float32))[0][0] == 0
    assert R.head(np.zeros((1, 4), np.float32), np.array([1.0 - 2.0 ** -24], np.float32))[0][0] == 3


def test_no_gpu_head_row_is_within_the_rounding_bound_of_a_boundary():
    """For the operands tests/test_actor_critic_kernels_gpu.py sends: every row's u S is further from every cumulative
    boundary than the float64 sums of the kernel can move it, so the GPU test compares the action of every row."""
    for E in R.HEAD_E:
        for A in R.HEAD_A:
            logits, _, u = R.head_case(E, A)
            margin, bound = R.head_margin(logits, u)
            assert np.all(margin > bound), (E, A, int((margin <= bound).sum()))
            assert np.all((u >= 0) & (u < 1))
