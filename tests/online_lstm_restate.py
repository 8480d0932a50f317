"""The recurrent on-policy window: restatement, operands and streams shared by the recurrent actor-critic tests.

  window_rec          tests/actor_critic_restate.py `window` extended by the two blocks a recurrent policy adds to every stored
                      next_state: the packed recurrent state (S float32 words: hx, cx of each recurrent layer) and the
                      `initials` flag.  Both are read from exactly the ring row the observation is read from, so the
                      restatement IS `window` run on those rings: the row rule is stated once, there.
  REC_WINDOW_CASES    the shapes at which the kernel can go wrong (csrc/actor_critic.hip k_online_window with S > 0).
  rec_step / ...      a seeded stream of whole vector steps with recurrent pytrees, as the device actor's DeviceSamples and
                      as the host history's per-env dicts.
  ONLINE_LSTM_CASE    the seeded stream and policy of tests/golden/online_ppo_lstm.npz (tests/golden/generate_online_lstm.py
                      feeds them to the reference, tests/test_online_lstm_cpu.py to the mirror classes).
"""
import numpy as np

from tests import actor_critic_restate as R


# ---- the window ----------------------------------------------------------------------------------------------------------------
def window_rec(T, B, E, cap, nstep_target, gamma, lam, plan, obs, actions, rewards, dones, logp, values, state, initials):
    """state (cap, E, S) float32, initials (cap, E) float32 -> R.window's dict plus states_state / target_state (T, B, S) and
    states_initials / target_initials (T, B)."""
    out = R.window(T, B, E, cap, nstep_target, gamma, lam, plan, obs, actions, rewards, dones, logp, values)
    s = R.window(T, B, E, cap, nstep_target, gamma, lam, plan, state, actions, rewards, dones, logp, values)
    i = R.window(T, B, E, cap, nstep_target, gamma, lam, plan, initials, actions, rewards, dones, logp, values)
    out.update(states_state=s["states"], target_state=s["target_states"], states_initials=i["states"],
               target_initials=i["target_states"])
    return out


# name -> T, B, E, cap, S, nstep_target, plan rows (env, first slot, own), float32 words the state ring view is shifted by
REC_WINDOW_CASES = {
    # 4-byte words (S % 4 != 0); sequence 0 plain, sequence 1 an env's first ever transition, sequence 2 wraps the ring
    "words": (4, 3, 3, 7, 6, 4, [(0, 1, 0), (1, 5, 1), (2, 6, 0)], 0),
    # 16-byte accesses; nstep_target < T
    "vec16": (5, 3, 4, 8, 32, 2, [(3, 2, 0), (0, 7, 0), (1, 4, 1)], 0),
    # two recurrent layers of widths 3 and 8: S = 2 * 3 + 2 * 8
    "two_layers": (3, 2, 2, 5, 22, 3, [(1, 3, 0), (0, 0, 1)], 0),
    # cap = T + 1: a sequence and the slot before it fill the whole ring, wrapped
    "tight_ring": (4, 2, 2, 5, 8, 4, [(0, 3, 0), (1, 1, 0)], 0),
    # B > E: two sequences of each env
    "two_per_env": (2, 4, 2, 6, 6, 2, [(0, 1, 0), (1, 1, 0), (0, 3, 0), (1, 3, 0)], 0),
    "T1": (1, 2, 2, 2, 32, 1, [(0, 0, 1), (1, 1, 0)], 0),
    # S % 4 == 0 but the ring starts 4 bytes off a 16-byte boundary: the launcher must take the word path
    "offset_ring": (3, 2, 3, 5, 32, 3, [(2, 4, 0), (0, 1, 1)], 1),
    # rows longer than one pass of the 256-thread workgroup, on either path
    "long_vec16": (2, 2, 2, 4, 2052, 2, [(0, 3, 0), (1, 1, 1)], 0),
    "long_words": (2, 2, 2, 4, 1030, 1, [(1, 2, 0), (0, 0, 1)], 0),
}


def rec_window_case(name):
    """Rings filled completely with seeded values (every in-range read is defined), dones inside the sequences."""
    T, B, E, cap, S, n, plan, shift = REC_WINDOW_CASES[name]
    g = np.random.RandomState(4000 + sum(map(ord, name)))
    obs = g.randn(cap, E, 4).astype(np.float32) if len(name) % 2 == 0 else g.randint(0, 256, size=(cap, E, 3, 7)).astype(np.uint8)
    return dict(T=T, B=B, E=E, cap=cap, S=S, n=n, shift=shift, plan=np.array(plan, dtype=np.int32), obs=obs,
                actions=g.randint(0, 6, size=(cap, E)).astype(np.int32),
                rewards=g.choice([0.0, 1.0, -0.5, 0.25], size=(cap, E)).astype(np.float32),
                values=g.randn(cap, E).astype(np.float32), logp=(-g.rand(cap, E)).astype(np.float32),
                dones=(g.rand(cap, E) < 0.3).astype(np.uint8),
                state=g.randn(cap, E, S).astype(np.float32), initials=(g.rand(cap, E) < 0.3).astype(np.float32))


# ---- a stream of whole vector steps with recurrent pytrees ------------------------------------------------------------------------
REC_WIDTHS = (3, 8)               # recurrent layers 1 and 2 (layer 0 is stateless): S = 22


def rec_step(seed, t, E, kind):
    """One vector step: tests/test_online_device_gpu.py's fields plus, per recurrent layer, hx / cx (E, H) and the shared
    `initials` (E,) of the stored next_state — 1 where this step ended the env's episode, with hx / cx zeroed there as
    LSTM.get_state stores them."""
    g = np.random.RandomState(7919 * seed + t)
    obs = g.randint(0, 256, size=(E, 2, 4, 4)).astype(np.uint8) if kind == "u8" else g.randn(E, 4).astype(np.float32)
    obs.reshape(E, -1)[:, 0] = np.arange(E)
    out = {"obs": obs, "actions": g.randint(0, 3, size=E).astype(np.int32), "values": g.randn(E).astype(np.float32),
           "logp": (-g.rand(E)).astype(np.float32), "rewards": g.choice([0.0, 1.0, -0.5, 0.25], size=E).astype(np.float32),
           "dones": (g.rand(E) < 0.2).astype(np.uint8)}
    out["initials"] = out["dones"].astype(np.float32)         # the stored next_state opens an episode where this step ended one
    keep = (1.0 - out["initials"])[:, None].astype(np.float32)
    for i, H in enumerate(REC_WIDTHS):
        out["hx%d" % i] = g.randn(E, H).astype(np.float32) * keep
        out["cx%d" % i] = g.randn(E, H).astype(np.float32) * keep
    return out


def rec_state_tree(step, e=None, wrap=lambda a: a):
    """The next_state pytree of a vector step (e = None: all envs, batched) or of one env's transition."""
    pick = (lambda a: wrap(a)) if e is None else (lambda a: a[e])
    tree = {"x": pick(step["obs"]), "layer0_state": {}}
    for i in range(len(REC_WIDTHS)):
        tree["layer%d_state" % (i + 1)] = {"hx": pick(step["hx%d" % i]), "cx": pick(step["cx%d" % i]),
                                           "initials": pick(step["initials"])}
    return tree


def rec_device_samples(steps, E):
    """The steps as the device actor hands them over: packed by acting/actor.py's own _pack_state."""
    import torch
    from rltime_amd.acting.acting_interface import DeviceSamples
    from rltime_amd.acting.actor import _pack_state
    out = DeviceSamples(rec_state_tree(steps[0], 0), E, 0)
    for s in steps:
        fields = _pack_state(rec_state_tree(s, wrap=lambda a: torch.from_numpy(a).cuda()))
        out.append(actions=torch.from_numpy(s["actions"]).cuda(),
                   policy=torch.from_numpy(np.stack([s["logp"], s["values"]], axis=1)).cuda(),
                   rewards=torch.from_numpy(s["rewards"]).cuda(), dones=torch.from_numpy(s["dones"]).cuda(), **fields)
    return out


def rec_dicts(steps, E, absolute=False):
    """The steps as the host history takes them (np.float64 rewards: its arithmetic is float64)."""
    out = []
    for s in steps:
        for e in range(E):
            r = np.float64(s["rewards"][e])
            out.append({"policy_output": {"actions": s["actions"][e], "values": s["values"][e], "action_log_probs": s["logp"][e],
                                          "raw_reward": r},
                        "next_state": rec_state_tree(s, e), "reward": abs(r) if absolute else r, "done": bool(s["dones"][e]),
                        "info": {}, "env_id": e})
    return out


# ---- the reference fixture's case (tests/golden/online_ppo_lstm.npz) ----------------------------------------------------------------
ONLINE_LSTM_CASE = {
    "seed": 61, "num_envs": 3, "obs_dim": 4, "n_actions": 2, "done_prob": 0.2, "lstm_units": 8,
    "nstep_train": 4, "gamma": 0.99, "advlam": 0.95, "vf_coef": 0.5, "entropy_factor": 1e-2, "clip_value": 0.2,
    "weights_seed": 9,
    "model": {"type": "sequential", "args": {"layer_configs": [{"type": "fc", "args": {"fc_size": 16}},
                                                               {"type": "lstm", "args": {"num_units": 8}}]}},
    # feed N vector steps / draw a batch of B sequences (None expected where the buffer cannot serve it)
    "script": [["feed", 3], ["draw", 1], ["feed", 2], ["draw", 3], ["feed", 9], ["draw", 5], ["draw", 2]],
}


def online_lstm_vector_steps(case, count, start_step=0):
    """`count` vector steps of the recurrent on-policy case as the reference's per-env sample dicts: tests/golden/streams.py
    online_vector_steps with a recurrent next_state — hx / cx (H,) float32 drawn from the seed, zeroed where the step ended
    the episode, and `initials` = that done flag as float32 (modules/lstm.py:131-161)."""
    E, H = case["num_envs"], case["lstm_units"]
    for s in range(start_step, start_step + count):
        rng = np.random.RandomState((case["seed"] * 1000003 + s) % (2 ** 31))
        obs = rng.randn(E, case["obs_dim"]).astype(np.float32)
        dones = rng.rand(E) < case["done_prob"]
        actions = rng.randint(0, case["n_actions"], size=E)
        logp = np.log(rng.uniform(0.2, 0.8, size=E)).astype(np.float32)
        values = (rng.randn(E) * 3 + 10).astype(np.float32)
        rewards = np.where(rng.rand(E) < 0.9, 1.0, 0.5)
        initials = dones.astype(np.float32)
        hx = (rng.randn(E, H) * 0.5).astype(np.float32) * (1 - initials)[:, None]
        cx = rng.randn(E, H).astype(np.float32) * (1 - initials)[:, None]
        yield [{"policy_output": {"actions": actions[e], "action_log_probs": logp[e], "values": values[e]},
                "next_state": {"x": obs[e], "layer0_state": {}, "layer1_state": {"hx": hx[e], "cx": cx[e], "initials": initials[e]}},
                "reward": rewards[e], "done": dones[e], "info": {}, "env_id": e} for e in range(E)]
