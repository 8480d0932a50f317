"""NumPy restatement of the evaluation counting kernel (csrc/acting.hip k_eval_count), in the prefix-sum form the
kernel uses — not the reference's sequential loop.

Of E envs stepping in parallel, the first N episodes that STARTED are counted, in the order a host loop over
(step, env) would meet their ends.  Per vector step, with c = done & open:

    position of env i's episode in the lists   counted + (number of c before i)
    env i closes when                          done_i and started + (number of dones up to and including i) > N

tests/test_eval_restate_cpu.py holds this to the unmodified reference's own eval_policy on every fixture case
(tests/golden/eval_cases.npz), bit for bit; the GPU tests hold the kernel to this after every step."""
import numpy as np

STAT_KEYS = ("mean", "min", "max", "median", "std")


class EvalCount:
    def __init__(self, E, N):
        if not 1 <= E <= N:
            raise ValueError("1 <= E <= N (the reference asserts num_envs <= episode_count)")
        self.E, self.N = int(E), int(N)
        self.reset()

    def reset(self):
        E, N = self.E, self.N
        self.acc = np.zeros(E, np.float64)
        self.len = np.zeros(E, np.int32)
        self.open = np.ones(E, np.uint8)
        self.counters = np.array([E, 0, 0, 0], np.int32)          # started, counted, steps, 0
        self.ep_reward = np.zeros(N, np.float64)
        self.ep_len = np.zeros(N, np.int32)

    def step(self, rewards, dones):
        """rewards float32 [E] (raw), dones [E] (anything truthy)."""
        started, counted = int(self.counters[0]), int(self.counters[1])
        if counted == self.N:
            return
        rewards = np.asarray(rewards)
        assert rewards.dtype == np.float32 and rewards.shape == (self.E,)
        d = np.asarray(dones).astype(bool)
        self.counters[2] += 1
        self.acc += rewards.astype(np.float64)
        self.len += 1
        c = d & (self.open != 0)
        pos = counted + np.cumsum(c) - c                          # exclusive scan
        self.ep_reward[pos[c]] = self.acc[c]
        self.ep_len[pos[c]] = self.len[c]
        self.open[d & (started + np.cumsum(d) > self.N)] = 0      # inclusive scan
        self.counters[1] = counted + int(c.sum())
        self.counters[0] = started + int(d.sum())
        self.acc[d] = 0.0
        self.len[d] = 0

    @property
    def finished(self):
        return int(self.counters[1]) == self.N


def run_stream(rewards, dones, N):
    """Feed (rewards [T, E], dones [T, E]) until N episodes are counted -> the EvalCount."""
    ec = EvalCount(rewards.shape[1], N)
    for t in range(rewards.shape[0]):
        if ec.finished:
            break
        ec.step(rewards[t], dones[t])
    return ec


def stats(values):
    """The five statistics of the reference's record (eval.py:169-177) of one list."""
    return {"mean": np.mean(values), "min": np.min(values), "max": np.max(values), "median": np.median(values),
            "std": np.std(values)}
