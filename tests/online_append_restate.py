"""NumPy restatement of the on-policy history's append launch (csrc/actor_critic.hip k_online_append) and of its slot rule.

  slot_of      vector step number s (counted from 0) lives in ring slot s mod cap.  The kernel reads s as
               head word + k, the head word being the number of vector steps stored before the launch sequence.
  append       one vector step into that slot of the seven rings, nothing else touched.
  regrow       what DeviceOnlineHistory._grow does to the rings: the `written` steps stored so far, as far as the old ring
               still holds them, keep their slot number modulo the new capacity.

tests/test_online_append_cpu.py checks the rule against OnlinePlan (the slot get_train_data reads a step from is the slot
`append` put it in, across a regrow); tests/test_online_append_gpu.py compares the kernel with `append`.
"""
import numpy as np

RINGS = ("obs", "actions", "rewards", "dones", "policy", "state", "initials")


def slot_of(head_word, k, cap):
    return int((int(head_word) + int(k)) % int(cap))


def new_rings(cap, E, obs_bytes, S, canary=None):
    """Seven rings; with `canary` every element holds a value no step carries."""
    r = {"obs": np.zeros((cap, E, obs_bytes), np.uint8), "actions": np.zeros((cap, E), np.int32),
         "rewards": np.zeros((cap, E), np.float32), "dones": np.zeros((cap, E), np.uint8),
         "policy": np.zeros((cap, E, 2), np.float32), "state": np.zeros((cap, E, S), np.float32),
         "initials": np.zeros((cap, E), np.float32)}
    if canary is not None:
        r["obs"][:] = 0xA5
        r["actions"][:] = -77
        r["rewards"][:] = -1234.5
        r["dones"][:] = 9
        r["policy"][:] = -4321.25
        r["state"][:] = 777.75
        r["initials"][:] = -3.0
    return r


def append(rings, head_word, k, step):
    """step: obs (E, obs_bytes) uint8, actions (E,) int32, rewards (E,) float32, dones (E,) uint8, policy (E, 2) float32
    [log-probability | value], and with a recurrent state: state (E, S) float32, initials (E,) float32."""
    cap = rings["obs"].shape[0]
    s = slot_of(head_word, k, cap)
    for name in RINGS:
        if name in step and rings[name].size:
            rings[name][s] = step[name]
    return s


def regrow(rings, cap_new, written):
    cap = rings["obs"].shape[0]
    out = {k: np.zeros((cap_new,) + v.shape[1:], v.dtype) for k, v in rings.items()}
    for s in range(max(0, written - cap), written):
        for k in rings:
            out[k][s % cap_new] = rings[k][s % cap]
    return out


def step_case(seed, t, E, obs_bytes, S):
    """A seeded vector step whose every field identifies (t, env)."""
    g = np.random.RandomState(100003 * seed + t)
    step = {"obs": g.randint(0, 256, size=(E, obs_bytes)).astype(np.uint8), "actions": g.randint(0, 6, size=E).astype(np.int32),
            "rewards": g.choice([0.0, 1.0, -0.5, 0.25], size=E).astype(np.float32), "dones": (g.rand(E) < 0.3).astype(np.uint8),
            "policy": g.randn(E, 2).astype(np.float32)}
    step["obs"][:, 0] = t % 256
    if S:
        step["state"] = g.randn(E, S).astype(np.float32)
        step["initials"] = step["dones"].astype(np.float32)
    return step
