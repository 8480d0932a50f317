"""CPU: the restatements of the Normal-head kernels (tests/normal_head_restate.py) against torch.distributions.Normal and
float64 autograd of the reference's A2C / PPO expression, the vector-action window against the scalar one, and the claims
made about the GPU tests' operands (the PPO mask keeps at least 99 % of the drawn rows)."""
import numpy as np
import pytest
import torch

from tests import actor_critic_restate as R
from tests import normal_head_restate as N


def _t(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


@pytest.mark.parametrize("D", N.HEAD_D)
@pytest.mark.parametrize("E", N.HEAD_E)
def test_head_equals_torch_normal(E, D):
    """The sampled action is torch's rsample expression rounded to float32, the log-probability is Normal.log_prob of that
    ROUNDED action summed over the components (actor_critic.py:57-58) — to 1e-13 of the magnitudes in float64."""
    mean, logstd, values, eps = N.head_case(E, D)
    actions, logp, mag = N.head(mean, logstd, eps)
    assert actions.dtype == np.float32 and actions.shape == (E, D)
    dist = torch.distributions.Normal(_t(mean), _t(logstd).exp().expand(E, D))
    want_a = (_t(mean) + _t(logstd).exp() * _t(eps)).to(torch.float32)
    assert np.array_equal(actions, want_a.numpy())
    want = dist.log_prob(want_a.double()).sum(-1).numpy()
    assert np.all(np.abs(logp - want) <= 1e-13 * (1.0 + mag))
    assert np.all(N.head_logp_bound(logp, mag) < 2.0 ** -22 * (1.0 + mag))
    assert logstd[0] == 0.0 and eps[-1, -1] == 5.0                          # std exactly 1; a 5-sigma draw
    assert E * D == 1 or actions[0, 0] == mean[0, 0]                        # eps 0: the mean itself


def _torch_loss(c, vf_coef, entropy_factor, clip_value, adv_norm):
    """training/torch/a2c.py:101-141 with the gain of a2c.py:90-99 or ppo.py:39-56, float64, on evaluate_actions' outputs:
    joint log-probability (sum over the components), un-summed entropy [M, D] and its .mean()."""
    mean, logstd, values = (_t(c[k]).requires_grad_(True) for k in ("mean", "logstd", "values"))
    M, D = mean.shape
    dist = torch.distributions.Normal(mean, logstd.exp().expand(M, D))
    log_probs = dist.log_prob(_t(c["actions"])).sum(-1)
    entropy = dist.entropy()
    assert entropy.shape == (M, D)
    targets, baseline = _t(c["targets"]), _t(c["acting"])
    adv = targets - baseline
    if adv_norm:
        adv = (adv - adv.mean()) / (adv.std() + 1e-5)
    if c["old"] is None:
        gain = (log_probs * adv).mean()
    else:
        ratio = torch.exp(log_probs - _t(c["old"]))
        gain = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip_value, 1.0 + clip_value) * adv).mean()
    vl = (targets - values).pow(2).mean()
    loss = vl * vf_coef - gain - entropy_factor * entropy.mean()
    loss.backward()
    return {"stats": np.array([loss.item(), vl.item(), -gain.item(), entropy.mean().item(), values.mean().item()]),
            "dmean": mean.grad.numpy(), "dlogstd": logstd.grad.numpy(), "dvalues": values.grad.numpy(),
            "entropy_sum": entropy.sum(-1).mean().item()}


@pytest.mark.parametrize("ppo", [False, True])
@pytest.mark.parametrize("D", N.LOSS_D)
@pytest.mark.parametrize("M", [2, 257, 1025])
def test_loss_and_gradients_equal_float64_autograd(M, D, ppo):
    """Loss, the four logged scalars and all three gradients — dlogstd, the reduction over the rows, among them — against
    autograd of the reference's expression; the entropy is the mean over the components, which for D > 1 is not their sum."""
    c = N.loss_case(M, D, seed=31 * M + D + (1000 if ppo else 0), ppo=ppo)
    for adv_norm in (False, True):
        for ef in (0.0, 0.01):
            got = N.loss(c["mean"], c["logstd"], c["values"], c["actions"], c["targets"], c["acting"], c["old"], 0.5, ef,
                         c["clip_value"], adv_norm, round_logp=False)
            want = _torch_loss(c, 0.5, ef, c["clip_value"], adv_norm)
            scale = 1.0 + np.abs(want["stats"]).max()
            assert np.all(np.abs(got["stats"] - want["stats"]) <= 1e-11 * scale)
            for k in ("dmean", "dlogstd", "dvalues"):
                assert got[k].shape == want[k].shape
                assert np.all(np.abs(got[k] - want[k]) <= 1e-11 * (1.0 + np.abs(want[k]).max())), k
            if D > 1:
                assert abs(want["entropy_sum"] - D * got["stats"][3]) <= 1e-11 * D * (1 + abs(got["stats"][3]))
                assert abs(want["entropy_sum"] - got["stats"][3]) > 0.5
            if ef:
                assert np.all(np.abs(got["dlogstd"]) > 0)


@pytest.mark.parametrize("D", N.LOSS_D)
@pytest.mark.parametrize("M", N.LOSS_M)
def test_ppo_mask_keeps_at_least_99_percent(M, D):
    """So that the GPU test cannot hide a failure behind the mask: of the rows drawn for every PPO case it sends, at least
    99 % lie outside the clip margin, rows on both sides of both bounds and inside remain, and the margin is tiny."""
    c = N.loss_case(M, D, seed=7 * M + D, ppo=True)
    assert c["kept"] >= 0.99 * c["drawn"] and c["mean"].shape == (M, D) and c["old"].shape == (M,)
    r = N.loss(c["mean"], c["logstd"], c["values"], c["actions"], c["targets"], c["acting"], c["old"], 0.5, 0.01, 0.2, M >= 2)
    margin = N.clip_margin(r["ratio"], r["log_probs"])
    assert np.all(np.abs(r["ratio"] - 0.8) > margin) and np.all(np.abs(r["ratio"] - 1.2) > margin)
    assert margin.max() < 1e-4
    if M >= 1023:
        assert (r["ratio"] < 0.8).any() and (r["ratio"] > 1.2).any() and (r["ratio"] == 1.0).any()
        assert ((r["ratio"] > 0.8) & (r["ratio"] < 1.2) & (r["ratio"] != 1.0)).any()
    b = N.loss_bounds(r, 0.5, 0.01)
    assert np.all(b["dlogstd"] < 2.0 ** -22 * (r["mag_dlogstd"] + 1e-300))


def test_window_box_is_the_scalar_window_plus_gathered_words():
    """W = 1: R.window on the same rings, field for field; W = 3: the words of the transition, everything else unchanged."""
    for T, B, obs_bytes in ((5, 3, 8), (2, 16, 16)):
        for W in (1, 3):
            c = N.window_box_case(T, B, obs_bytes, W, seed=T + B + W)
            got = N.window_box(T, B, c["E"], c["cap"], 3, 0.99, 0.95, c["plan"], c["obs"], c["action_words"], c["rewards"], c["dones"],
                               c["logp"], c["values"])
            ref = R.window(T, B, c["E"], c["cap"], 3, 0.99, 0.95, c["plan"], c["obs"], c["action_words"][:, :, 0].copy(), c["rewards"],
                           c["dones"], c["logp"], c["values"])
            for k in ref:
                if k != "actions":
                    assert np.array_equal(got[k], ref[k]), k
            assert got["actions"].shape == (T, B, W) and np.array_equal(got["actions"][:, :, 0], ref["actions"])
            assert any((c["plan"][b, 1] + T) > c["cap"] for b in range(B))       # a wrapped sequence
