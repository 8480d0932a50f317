"""NumPy restatement of the extra-features step (what csrc/acting.hip k_extra_features computes): the reference's
ExtraFeaturesEnvWrapper (env_wrappers/common.py:221-332) under an auto-resetting vector env (vec_env/simple.py:25-29),
as a function of the vector step's (actions, raw rewards, dones) and a per-env counter.  tests/golden/
generate_extra_features.py asserts it equal to the unmodified wrapper, bit for bit, while it writes the fixture."""
import numpy as np


def feature_size(A, include_action=True, include_reward=True, include_timestep=True):
    return (int(A) if include_action else 0) + int(bool(include_reward)) + int(bool(include_timestep))


class ExtraFeatures:
    """State: counters int32 [E].  reset() / step() return the float32 [E, X] rows, laid out
    [one-hot action (A) | timestep | reward] with each part present only when included."""

    def __init__(self, E, A, include_action=True, include_reward=True, include_timestep=True, clip_reward=True,
                 timestep_scale=1. / 100000):
        self.E, self.A = int(E), int(A)
        self.inc = (bool(include_action), bool(include_reward), bool(include_timestep))
        self.clip, self.scale = bool(clip_reward), float(timestep_scale)
        self.X = feature_size(A, *self.inc)
        if self.X == 0:
            raise ValueError("no feature included")
        self.counters = np.zeros(self.E, np.int32)

    def reset(self):
        """Every env starts an episode: the launch with dones all 1."""
        z = np.zeros(self.E, np.float32)
        return self.step(np.zeros(self.E, np.int32), z, np.ones(self.E, np.uint8))

    def step(self, actions, rewards, dones):
        actions, rewards = np.asarray(actions, np.int32), np.asarray(rewards, np.float32)
        dn = np.asarray(dones).astype(bool)
        self.counters = np.where(dn, 0, self.counters + 1).astype(np.int32)
        a = np.where(dn, 0, actions)
        r = np.where(dn, np.float32(0), rewards).astype(np.float32)
        if self.clip:
            r = np.sign(r)
        # a Python int times a Python float: the product in double, then the row's astype("float32")
        ts = (self.counters.astype(np.float64) * np.float64(self.scale)).astype(np.float32)
        inc_a, inc_r, inc_t = self.inc
        parts = []
        if inc_a:
            parts.append((np.arange(self.A, dtype=np.int32)[None, :] == a[:, None]).astype(np.float32))   # out of range: no element
        if inc_t:
            parts.append(ts[:, None])
        if inc_r:
            parts.append(r[:, None])
        return np.concatenate(parts, axis=1).astype(np.float32)
