"""Float64 restatements of the three actor-critic kernels (csrc/actor_critic.hip), written from the reference's formulas:

  sampling head       rltime/policies/torch/actor_critic.py:37-71 over distributions/categorical.py (softmax, inverse-CDF
                      choice for a given uniform, first maximum under force_best, log-probability of the action)
  on-policy window    rltime/history/history.py:71-108,178-201 and online_history.py:81-120 under the GAE(lambda) discount
                      of training/torch/a2c.py:48-66, on rings of whole vector steps
  A2C / PPO loss      training/torch/a2c.py:101-141 and ppo.py:39-56 with autograd's rules for minimum() and clamp()

tests/test_actor_critic_restate_cpu.py proves them against OnlineHistoryBuffer, oracle.replay.OracleOnline, float64
autograd of oracle.qmath.actor_critic_loss and torch.distributions.Categorical; the GPU tests compare the kernels with them.
The module also holds the operands the GPU tests send and the derived rounding bounds.

Rounding model of the kernels (include/mirl.h): inputs are float32, every operation is float64, each output is rounded to
float32 once.  A float64 operation contributes 2^-53 relative, exp / log / pow of the device library at most 2^-52: against
the 2^-24 of the final rounding these are covered by a flat 2^-40 of the magnitudes involved, which is what the bounds use.
"""
import numpy as np
import torch

U24 = 2.0 ** -24            # half an ulp of float32, relative: one rounding to nearest
SLACK = 2.0 ** -40          # covers every float64 operation of a row (a few hundred at 2^-52 each)


# ---- sampling head -----------------------------------------------------------------------------------------------------------
def softmax_parts(logits):
    """logits (E, A) float64 holding float32 values -> (d = z - max, e = exp(d), cumulative sums in ascending j, S)."""
    z = np.asarray(logits, dtype=np.float64)
    d = z - z.max(axis=1, keepdims=True)
    e = np.exp(d)
    cum = np.cumsum(e, axis=1)               # sequential, ascending: the order the kernel adds in
    return d, e, cum, cum[:, -1]


def first_max(z):
    z = np.asarray(z)
    return np.array([int(np.flatnonzero(row == row.max())[0]) for row in z], dtype=np.int64)


def head(logits, u=None, greedy=False):
    """-> (actions (E,), log-probabilities (E,) float64).  Sampled: the smallest a with u S < sum_{j <= a} e_j, the last
    action as the fallback; greedy: the first maximum of the logits."""
    d, e, cum, S = softmax_parts(logits)
    E, A = d.shape
    if greedy:
        actions = first_max(logits)
    else:
        want = np.asarray(u, dtype=np.float64) * S
        hit = want[:, None] < cum
        actions = np.where(hit.any(axis=1), hit.argmax(axis=1), A - 1).astype(np.int64)
    return actions, d[np.arange(E), actions] - np.log(S)


def head_margin(logits, u):
    """Per row: (distance of u S to the nearest cumulative boundary, the bound inside which the kernel's float64 sums may
    put it on the other side).  A partial sum of a <= A terms, each exp within 2^-52, carries at most (A + 1) 2^-52 S;
    u S one more rounding: (A + 4) 2^-52 S covers both sides."""
    d, e, cum, S = softmax_parts(logits)
    want = np.asarray(u, dtype=np.float64) * S
    return np.abs(want[:, None] - cum).min(axis=1), (d.shape[1] + 4) * 2.0 ** -52 * S


def head_logp_bound(logp):
    """One float32 rounding of d_a - log S, both float64."""
    return U24 * np.abs(logp) + SLACK * (1.0 + np.abs(logp))


# ---- on-policy window --------------------------------------------------------------------------------------------------------
def window(T, B, E, cap, nstep_target, gamma, lam, plan, obs, actions, rewards, dones, logp, values):
    """Rings of whole vector steps: obs (cap, E, ...) the transitions' next_state, the rest (cap, E).  plan (B, 3) = env, ring
    slot of the sequence's first transition, 1 when that transition is the env's first ever (it starts from its own
    next_state; every other one from the next_state one slot earlier).  fixed_target: transition t of a sequence covers
    n = min(nstep_target, T - t) steps.  -> dict of (T, B, ...) arrays: returns (float64) and `terms` (sum of |terms|),
    nsteps, target_masks, actions, action_log_probs, values, states, target_states."""
    out = {"returns": np.zeros((T, B)), "terms": np.zeros((T, B)), "nsteps": np.zeros((T, B), np.float32),
           "target_masks": np.zeros((T, B), np.float32), "actions": np.zeros((T, B), actions.dtype),
           "action_log_probs": np.zeros((T, B), np.float32), "values": np.zeros((T, B), np.float32),
           "states": np.zeros((T, B) + obs.shape[2:], obs.dtype), "target_states": np.zeros((T, B) + obs.shape[2:], obs.dtype)}
    for b in range(B):
        env, first, own = (int(x) for x in plan[b])
        at = lambda i: (first + i) % cap                                            # noqa: E731
        for t in range(T):
            n = min(nstep_target, T - t)
            ret = float(rewards[at(t), env])
            total = abs(ret)
            mask = 0.0 if dones[at(t), env] else 1.0
            for k in range(1, n):
                s = at(t + k)
                if mask:
                    v, r = float(values[s, env]), float(rewards[s, env])
                    term = ((gamma ** k) * (lam ** (k - 1))) * (v + lam * (r - v))
                    ret += term
                    total += abs(term)
                if dones[s, env]:
                    mask = 0.0
            out["returns"][t, b], out["terms"][t, b] = ret, total
            out["nsteps"][t, b], out["target_masks"][t, b] = n, mask
            out["actions"][t, b] = actions[at(t), env]
            out["action_log_probs"][t, b], out["values"][t, b] = logp[at(t), env], values[at(t), env]
            out["states"][t, b] = obs[at(0) if (t == 0 and own) else at(t - 1), env]
            out["target_states"][t, b] = obs[at(t + n - 1), env]
    return out


def window_bound(w):
    """One float32 rounding of a float64 sum whose pow() factors are within an ulp."""
    return U24 * np.abs(w["returns"]) + SLACK * w["terms"]


# ---- loss --------------------------------------------------------------------------------------------------------------------
def ratio_of(log_probs, old_log_probs):
    """exp(logp - old) through torch's float64 exp on the whole (M,) vector: bit for bit what the reference's expression
    gives for the same rows, so that a row planted exactly on a clip bound is on it for both."""
    x = torch.from_numpy(np.asarray(log_probs, dtype=np.float64)) - torch.from_numpy(np.asarray(old_log_probs, dtype=np.float64))
    return torch.exp(x).numpy()


def loss(logits, values, actions, targets, acting_values, old_log_probs, vf_coef, entropy_factor, clip_value, adv_norm,
         round_logp=True, log_probs=None):
    """float64 NumPy on float32-valued inputs -> dict(stats (5,) = loss, value loss, policy loss, entropy, value mean;
    dlogits (M, A), dvalues (M,), log_probs (M,) — the float32 the kernel rounds the log-probability to and then uses — and
    the magnitudes the bounds need).  round_logp=False keeps the log-probability in float64 (the reference's own expression)."""
    z = np.asarray(logits, dtype=np.float64)
    v, t, base = (np.asarray(x, dtype=np.float64) for x in (values, targets, acting_values))
    M, A = z.shape
    rows = np.arange(M)
    d, e, _, S = softmax_parts(z)
    logS = np.log(S)
    lp_all = d - logS[:, None]
    p = e / S[:, None]
    lp = lp_all[rows, actions] if log_probs is None else np.asarray(log_probs, dtype=np.float64)     # (given: used as they are)
    if round_logp:
        lp = lp.astype(np.float32).astype(np.float64)
    H = -(p * lp_all).sum(axis=1)
    adv = t - base
    if adv_norm:
        mean = adv.sum() / M
        std = np.sqrt(((adv - mean) ** 2).sum() / (M - 1))
        adv = (adv - mean) / (std + 1e-5)
    if old_log_probs is None:
        gain, coef, ratio = lp * adv, adv.copy(), None
    else:
        ratio = ratio_of(lp, old_log_probs)
        lo, hi = 1.0 - clip_value, 1.0 + clip_value
        s1, s2 = ratio * adv, np.clip(ratio, lo, hi) * adv
        gain = np.minimum(s1, s2)
        inside = (ratio >= lo) & (ratio <= hi)
        share = np.where(inside, 1.0, np.where(s1 < s2, 1.0, np.where(s1 == s2, 0.5, 0.0)))
        coef = share * (ratio * adv)
    onehot = np.zeros((M, A))
    onehot[rows, actions] = 1.0
    dz = -(coef / M)[:, None] * (onehot - p)
    dz_ent = (entropy_factor / M) * p * (lp_all + H[:, None])
    vl = ((t - v) ** 2).sum() / M
    g, ent, vm = gain.sum() / M, H.sum() / M, v.sum() / M
    return {"stats": np.array([vf_coef * vl - g - entropy_factor * ent, vl, -g, ent, vm]), "dlogits": dz + dz_ent,
            "dvalues": vf_coef * 2.0 * (v - t) / M, "log_probs": lp, "ratio": ratio, "adv": adv, "coef": coef,
            # (1 - p and log p + H cancel: the magnitudes are those of the numbers subtracted, not of the difference)
            "mag_dlogits": (np.abs(coef) / M)[:, None] * (onehot + p) + (abs(entropy_factor) / M) * p * (np.abs(lp_all) + np.abs(H)[:, None]), "mag_gain": np.abs(gain).sum() / M, "mag_vl": vl, "mag_ent": np.abs(H).sum() / M,
            "mag_vm": np.abs(v).sum() / M, "p": p}


def loss_bounds(r, vf_coef, entropy_factor, clipped):
    """First-order bounds of the kernel's outputs against `loss`: each output is one float32 rounding (2^-24 of its
    value) of float64 arithmetic on the same operands (2^-40 of the magnitudes that were added up).  The PPO ratio is exp of
    a difference of float32 numbers, and the normalised advantage a float64 quotient: both inside the 2^-40."""
    mag_loss = vf_coef * r["mag_vl"] + r["mag_gain"] + entropy_factor * r["mag_ent"]
    s = r["stats"]
    stats = U24 * np.abs(s) + SLACK * np.array([mag_loss, r["mag_vl"], r["mag_gain"], r["mag_ent"], r["mag_vm"]]) + 1e-300
    return {"stats": stats, "dlogits": U24 * np.abs(r["dlogits"]) + SLACK * r["mag_dlogits"] + 1e-300,
            "dvalues": U24 * np.abs(r["dvalues"]) + SLACK * np.abs(r["dvalues"]) + 1e-300,
            "log_probs": 0.0}


# ---- operands of the GPU tests (the CPU test checks the claims made about them) -------------------------------------------------
HEAD_E = (1, 3, 64, 65, 257)
HEAD_A = (1, 2, 6, 18, 64)


def head_case(E, A, seed=None):
    """Logits (E, A) float32 with a spread of a few nats, values, 24-bit uniforms."""
    g = np.random.RandomState(1000 + 97 * E + A if seed is None else seed)
    logits = (g.randn(E, A) * 2.0).astype(np.float32)
    values = g.randn(E).astype(np.float32)
    u = (g.randint(0, 2 ** 24, size=E).astype(np.float64) / 2 ** 24).astype(np.float32)
    if E >= 3:
        u[0], u[1] = 0.0, np.float32(1.0 - 2.0 ** -24)          # the two ends of [0, 1)
    return logits, values, u


def head_tie_case(E, A):
    """Every row's maximum planted on two actions: the first must win under `greedy`."""
    g = np.random.RandomState(77 + E + A)
    logits = (g.randn(E, A)).astype(np.float32)
    first = np.zeros(E, dtype=np.int64)
    for e in range(E):
        a, b = sorted(g.choice(A, 2, replace=False).tolist()) if A >= 2 else (0, 0)
        logits[e, a] = logits[e, b] = np.float32(5.0)
        first[e] = a
    return logits, g.randn(E).astype(np.float32), first


WINDOW_T = (1, 2, 5, 32, 128)
WINDOW_B = (1, 3, 16)


def window_nsteps(T):
    return sorted({1, 2, T, T + 3})


def window_case(T, B, obs_kind, seed):
    """A ring of cap = T + 3 vector steps of E = B + 1 envs, filled completely; sequence b reads env b from a start
    that wraps the ring for some b.  Dones: sequence 0 at its step 0, sequence 1 at its step T - 1, sequence 2 on two
    consecutive steps, sequence 3 none at all, the others at random."""
    g = np.random.RandomState(seed)
    E, cap = B + 1, T + 3
    if obs_kind == "u8":
        obs = g.randint(0, 256, size=(cap, E, 2, 4, 6)).astype(np.uint8)         # 48 bytes: the 16-byte path
    elif obs_kind == "u8odd":
        obs = g.randint(0, 256, size=(cap, E, 3, 7)).astype(np.uint8)            # 21 bytes: the byte path
    else:
        obs = g.randn(cap, E, 4).astype(np.float32)
    actions = g.randint(0, 6, size=(cap, E)).astype(np.int32)
    rewards = g.choice([0.0, 1.0, -0.5, 0.25], size=(cap, E)).astype(np.float32)
    values = g.randn(cap, E).astype(np.float32)
    logp = (-g.rand(cap, E)).astype(np.float32)
    dones = (g.rand(cap, E) < 0.1).astype(np.uint8)
    plan = np.zeros((B, 3), dtype=np.int32)
    for b in range(B):
        env, first = b, (1 + 2 * b) % cap
        own = 1 if b % 4 == 1 else 0
        plan[b] = (env, first, own)
        slots = [(first + i) % cap for i in range(T)]
        if b % 5 < 4:
            dones[slots, env] = 0
        if b % 5 == 0:
            dones[slots[0], env] = 1
        elif b % 5 == 1:
            dones[slots[T - 1], env] = 1
        elif b % 5 == 2 and T >= 2:
            dones[slots[T // 2 - 1], env] = dones[slots[T // 2], env] = 1
    return dict(E=E, cap=cap, plan=plan, obs=obs, actions=actions, rewards=rewards, dones=dones, logp=logp, values=values)


LOSS_M = (2, 7, 255, 256, 257, 2048, 4099)
LOSS_A = (1, 2, 6, 18)


def loss_case(M, A, seed, ppo, clip_value=0.2):
    """Random rows; for PPO the old log-probabilities put rows inside, outside (both sides) and — planted through
    `plant_clip_rows` by the caller, which needs the kernel's own float32 log-probabilities — exactly on the clip bounds."""
    g = np.random.RandomState(seed)
    logits = (g.randn(M, A) * 1.5).astype(np.float32)
    values = g.randn(M).astype(np.float32)
    targets = (values + g.randn(M) * 0.7).astype(np.float32)
    acting = (values + g.randn(M) * 0.3).astype(np.float32)
    actions = g.randint(0, A, size=M).astype(np.int32)
    hit = g.rand(M) < 0.1
    targets[hit] = values[hit]                                   # dvalues exactly 0 there
    targets[0] = values[0]
    old = None
    if ppo:
        lp = loss(logits, values, actions, targets, acting, None, 1.0, 0.0, None, False)["log_probs"]
        old = (lp + g.randn(M) * 0.25).astype(np.float32)
        same = g.rand(M) < 0.2
        old[same] = lp[same].astype(np.float32)                  # ratio exactly 1
    return dict(logits=logits, values=values, actions=actions, targets=targets, acting=acting, old=old, clip_value=clip_value)

