"""Float64 restatements of the Normal-head kernels (csrc/actor_critic.hip: k_actor_head_normal, the window kernel with vector
actions, k_ac_loss_normal), written from the reference's formulas:

  sampling head     rltime/policies/torch/actor_critic.py:37-71 over distributions/normal.py:9-36: independent Gaussians with
                    a state-independent log-std, the action sampled as mean + std * eps, the joint log-probability the sum
                    over the components of the log-density of the SAMPLED float32 action
  window            tests/actor_critic_restate.py `window`, with `action_words` opaque 4-byte words per transition
  A2C / PPO loss    training/torch/a2c.py:101-141 and ppo.py:39-56; the entropy is the mean over ALL M * D elements of the
                    un-summed per-component entropies (a2c.py:113 takes .mean() of what evaluate_actions returns)

tests/test_normal_head_restate_cpu.py proves them against torch.distributions.Normal and float64 autograd; the GPU tests
compare the kernels with them.  The module also holds the operands the GPU tests send and the derived rounding bounds.

Rounding model (tests/actor_critic_restate.py): inputs are float32, every operation is float64, each output is rounded to
float32 once: U24 = 2^-24 of the output for that rounding, SLACK = 2^-40 of the magnitudes that were added up for the
float64 operations and the device library's exp (at most 2^-52 each, a few hundred per row at the most).

The action is ONE float64 expression rounded once, mean + exp(logstd) * eps: the kernel's and NumPy's exp agree to the last
bit or differ by one ulp of float64, which moves the float32 rounding only when the sum lies within 2^-52 of a rounding
boundary (about one element in 2^28) — the GPU test compares the actions bit for bit.

The PPO mask.  The kernel decides a row's side of the clip bounds on ratio = exp(logp32 - old): its float32 logp32 may be the
restatement's neighbour (one float32 ulp, 2^-23 |logp|, when the float64 sum lies at a rounding boundary) and its exp is
within 2^-52, so a row whose restated ratio lies within  ratio * (2^-23 (|logp| + 1) + SLACK)  of 1 - clip or 1 + clip may
take the other branch in the kernel.  `loss_case` draws a few rows more than it needs and keeps only rows outside that
margin; the CPU test asserts that at least 99 % of the drawn rows are kept."""
import math

import numpy as np

from tests import actor_critic_restate as R

U24, SLACK = R.U24, R.SLACK
HALF_LOG_2PI = 0.9189385332046727            # log(2 pi) / 2, the kernel's literal
assert HALF_LOG_2PI == 0.5 * math.log(2.0 * math.pi)
MAX_D = 16


# ---- the pieces the head and the loss share ------------------------------------------------------------------------------------
def log_prob_terms(actions, mean, logstd):
    """(M, D) float64 terms  -(a - mean)^2 / (2 exp(2 logstd)) - logstd - log(2 pi) / 2  and their magnitudes."""
    a, m = np.asarray(actions, dtype=np.float64), np.asarray(mean, dtype=np.float64)
    ls = np.asarray(logstd, dtype=np.float64)[None, :]
    diff = a - m
    q = -(diff * diff) / (2.0 * np.exp(2.0 * ls))
    return q - ls - HALF_LOG_2PI, np.abs(q) + np.abs(ls) + HALF_LOG_2PI


def joint(terms):
    """The sum over the components in ascending d, sequentially: the order the kernel adds in."""
    out = np.zeros(terms.shape[0])
    for d in range(terms.shape[1]):
        out = out + terms[:, d]
    return out


# ---- sampling head ---------------------------------------------------------------------------------------------------------------
def head(mean, logstd, eps):
    """-> (actions float32 (E, D), log-probabilities float64 (E,), magnitudes (E,))."""
    m, e = np.asarray(mean, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    ls = np.asarray(logstd, dtype=np.float64)[None, :]
    actions = (m + np.exp(ls) * e).astype(np.float32)
    terms, mags = log_prob_terms(actions, mean, logstd)
    return actions, joint(terms), mags.sum(axis=1)


def head_logp_bound(logp, mag):
    """One float32 rounding of a float64 sum of D terms."""
    return U24 * np.abs(logp) + SLACK * (1.0 + mag)


# ---- window with vector actions --------------------------------------------------------------------------------------------------
def window_box(T, B, E, cap, nstep_target, gamma, lam, plan, obs, action_words, rewards, dones, logp, values):
    """R.window with action rings of shape (cap, E, W) of opaque int32 words: everything but the actions is R.window's on
    the same rings, the action words of a transition are gathered exactly."""
    out = R.window(T, B, E, cap, nstep_target, gamma, lam, plan, obs, np.zeros((cap, E), np.int32), rewards, dones, logp, values)
    W = action_words.shape[2]
    acts = np.zeros((T, B, W), action_words.dtype)
    for b in range(B):
        env, first, _ = (int(x) for x in plan[b])
        for t in range(T):
            acts[t, b] = action_words[(first + t) % cap, env]
    out["actions"] = acts
    return out


# ---- loss ------------------------------------------------------------------------------------------------------------------------
def loss(mean, logstd, values, actions, targets, acting_values, old_log_probs, vf_coef, entropy_factor, clip_value, adv_norm,
         round_logp=True, log_probs=None):
    """float64 NumPy on float32-valued inputs -> dict(stats (5,), dmean (M, D), dlogstd (D,), dvalues (M,), log_probs (M,) — the
    float32 the kernel rounds the log-probability to and then uses —, and the magnitudes the bounds need).  log_probs given:
    used as they are (the kernel's own float32 values)."""
    m, a = np.asarray(mean, dtype=np.float64), np.asarray(actions, dtype=np.float64)
    ls = np.asarray(logstd, dtype=np.float64)
    v, t, base = (np.asarray(x, dtype=np.float64) for x in (values, targets, acting_values))
    M, D = m.shape
    terms, mags = log_prob_terms(a, m, ls)
    lp = joint(terms) if log_probs is None else np.asarray(log_probs, dtype=np.float64)
    if round_logp:
        lp = lp.astype(np.float32).astype(np.float64)
    ent = 0.0
    for d in range(D):
        ent = ent + ((0.5 + HALF_LOG_2PI) + ls[d])
    mag_ent = sum((0.5 + HALF_LOG_2PI) + abs(ls[d]) for d in range(D)) / D
    ent = ent / D
    adv = t - base
    if adv_norm:
        mu = adv.sum() / M
        std = np.sqrt(((adv - mu) ** 2).sum() / (M - 1))
        adv = (adv - mu) / (std + 1e-5)
    if old_log_probs is None:
        gain, coef, ratio = lp * adv, adv.copy(), None
    else:
        ratio = R.ratio_of(lp, old_log_probs)
        lo, hi = 1.0 - clip_value, 1.0 + clip_value
        s1, s2 = ratio * adv, np.clip(ratio, lo, hi) * adv
        gain = np.minimum(s1, s2)
        inside = (ratio >= lo) & (ratio <= hi)
        share = np.where(inside, 1.0, np.where(s1 < s2, 1.0, np.where(s1 == s2, 0.5, 0.0)))
        coef = share * (ratio * adv)
    s2d = np.exp(2.0 * ls)[None, :]
    diff = a - m
    w = (coef / M)[:, None]
    dmean = -(w * (diff / s2d))
    per_row = -(w * ((diff * diff) / s2d - 1.0))
    dlogstd = per_row.sum(axis=0) - entropy_factor / D
    vl = ((t - v) ** 2).sum() / M
    g, vm = gain.sum() / M, v.sum() / M
    return {"stats": np.array([vf_coef * vl - g - entropy_factor * ent, vl, -g, ent, vm]), "dmean": dmean, "dlogstd": dlogstd,
            "dvalues": vf_coef * 2.0 * (v - t) / M, "log_probs": lp, "logp_mag": mags.sum(axis=1), "ratio": ratio, "adv": adv, "coef": coef,
            "mag_dlogstd": (np.abs(w) * ((diff * diff) / s2d + 1.0)).sum(axis=0) + abs(entropy_factor) / D,
            "mag_gain": np.abs(gain).sum() / M, "mag_vl": vl, "mag_ent": mag_ent, "mag_vm": np.abs(v).sum() / M}


def loss_bounds(r, vf_coef, entropy_factor):
    """First-order bounds of the kernel's outputs against `loss` evaluated ON THE KERNEL'S OWN float32 log-probabilities: each
    output is one float32 rounding (2^-24 of its value) of float64 arithmetic on the same operands (2^-40 of the magnitudes
    that were added up).  The log-probabilities themselves are held to head_logp_bound."""
    mag_loss = vf_coef * r["mag_vl"] + r["mag_gain"] + abs(entropy_factor) * r["mag_ent"]
    s = r["stats"]
    stats = U24 * np.abs(s) + SLACK * np.array([mag_loss, r["mag_vl"], r["mag_gain"], r["mag_ent"], r["mag_vm"]]) + 1e-300
    return {"stats": stats, "dmean": (U24 + SLACK) * np.abs(r["dmean"]) + 1e-300,
            "dlogstd": U24 * np.abs(r["dlogstd"]) + SLACK * r["mag_dlogstd"] + 1e-300,
            "dvalues": (U24 + SLACK) * np.abs(r["dvalues"]) + 1e-300,
            "log_probs": head_logp_bound(r["log_probs"], r["logp_mag"])}


def clip_margin(ratio, log_probs):
    """How close to a clip bound a restated ratio may lie before the kernel may put the row on the other side (module text)."""
    return ratio * (2.0 ** -23 * (np.abs(log_probs) + 1.0) + SLACK)


# ---- operands of the GPU tests (the CPU test checks the claims made about them) ---------------------------------------------------
HEAD_E = (1, 63, 64, 65, 130)
HEAD_D = (1, 2, 3, 16)
LOSS_M = (1, 2, 1023, 1024, 1025, 2049)
LOSS_D = (1, 3, 16)


def head_case(E, D, seed=None):
    """Means (E, D) of a few units, log-stds in [-1.5, 0.5] (one exactly 0: std exactly 1), values, standard-normal draws with
    a zero and a 5-sigma one planted."""
    g = np.random.RandomState(2000 + 97 * E + D if seed is None else seed)
    mean = (g.randn(E, D) * 1.5).astype(np.float32)
    logstd = g.uniform(-1.5, 0.5, size=D).astype(np.float32)
    logstd[0] = 0.0
    values = g.randn(E).astype(np.float32)
    eps = g.randn(E, D).astype(np.float32)
    eps[0, 0] = 0.0
    eps[-1, -1] = 5.0
    return mean, logstd, values, eps


def window_box_case(T, B, obs_bytes, W, seed):
    """R.window_case's rings (cap = T + 3, E = B + 1, wrapped starts, planted dones) with observation rows of `obs_bytes`
    bytes and action rings of W float32 words whose bit patterns are arbitrary (NaN patterns included: opaque words)."""
    c = R.window_case(T, B, "u8", seed)
    g = np.random.RandomState(seed + 1)
    c["obs"] = g.randint(0, 256, size=(c["cap"], c["E"], obs_bytes)).astype(np.uint8)
    c["action_words"] = g.randint(-2 ** 31, 2 ** 31, size=(c["cap"], c["E"], W)).astype(np.int32)
    return c


def loss_case(M, D, seed, ppo, clip_value=0.2):
    """M rows kept of M + max(8, M // 50) drawn (the PPO mask of the module text; A2C keeps the first M) -> dict of operands
    and `drawn`, `kept` (of the drawn rows, how many lie outside the margin)."""
    g = np.random.RandomState(seed)
    N = M + max(8, M // 50)
    mean = (g.randn(N, D) * 1.5).astype(np.float32)
    logstd = g.uniform(-1.0, 0.5, size=D).astype(np.float32)
    actions = (mean + np.exp(logstd)[None, :] * g.randn(N, D)).astype(np.float32)
    values = g.randn(N).astype(np.float32)
    targets = (values + g.randn(N) * 0.7).astype(np.float32)
    acting = (values + g.randn(N) * 0.3).astype(np.float32)
    hit = g.rand(N) < 0.1
    targets[hit] = values[hit]                                   # dvalues exactly 0 there
    old, keep = None, np.ones(N, bool)
    if ppo:
        terms, _ = log_prob_terms(actions, mean, logstd)
        lp = joint(terms).astype(np.float32).astype(np.float64)
        old = (lp + g.randn(N) * 0.25).astype(np.float32)
        same = g.rand(N) < 0.2
        old[same] = lp[same].astype(np.float32)                  # ratio exactly 1 where the kernel rounds alike, 1 +- 2^-23 |logp| else
        ratio = R.ratio_of(lp, old)
        margin = clip_margin(ratio, lp)
        keep = (np.abs(ratio - (1.0 - clip_value)) > margin) & (np.abs(ratio - (1.0 + clip_value)) > margin)
    rows = np.flatnonzero(keep)[:M]
    assert len(rows) == M, "too few rows outside the clip margin"
    pick = lambda x: None if x is None else np.ascontiguousarray(x[rows])      # noqa: E731
    return dict(mean=pick(mean), logstd=logstd, actions=pick(actions), values=pick(values), targets=pick(targets),
                acting=pick(acting), old=pick(old), clip_value=clip_value, drawn=N, kept=int(keep.sum()))
