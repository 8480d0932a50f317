"""GPU: the evaluation counting kernel (csrc/acting.hip k_eval_count behind mirl_eval_count) against the NumPy restatement
of tests/eval_restate.py, which tests/test_eval_restate_cpu.py holds to the unmodified reference's eval_policy.

Every fixture case (tests/golden/eval_cases.npz) is fed step by step through the C-ABI; the lists, the counters, the open
mask and the accumulators must equal the restatement after EVERY step, bit for bit, and the reference's own list at the
end.  Every buffer is longer than the kernel may write and its tail holds a pattern, so a store past E or N shows."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.eval_restate import EvalCount

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_cases.npz")
ERR_ARG = -1                                  # include/mirl.h MIRL_ERR_ARG
GUARD = 9
FILL = {np.dtype(np.float64): 0x7FF8A5A5A5A5A5A5, np.dtype(np.int32): -77777, np.dtype(np.uint8): 0xA5}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(a):
    """a followed by GUARD pattern elements (float64: a quiet NaN no sum produces)."""
    tail = np.full(GUARD, FILL[a.dtype], np.uint64 if a.dtype == np.float64 else a.dtype).view(a.dtype)
    return np.concatenate([a, tail])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class _Dev:
    """Device state of one evaluation and the host mirror it must equal."""
    KEYS = ("acc", "len", "open", "counters", "ep_reward", "ep_len")

    def __init__(self, E, N, garbage=False):
        self.E, self.N = E, N
        self.ec = EvalCount(E, N)
        rng = np.random.default_rng(E * 7919 + N)
        start = {k: getattr(self.ec, k).copy() for k in self.KEYS}
        if garbage:                             # what a reset must overwrite (the lists are not the reset's business)
            start["acc"] = rng.standard_normal(E)
            start["len"] = rng.integers(1, 99, E).astype(np.int32)
            start["open"] = rng.integers(0, 2, E).astype(np.uint8)
            start["counters"] = np.array([5, 3, 11, 0], np.int32)
        self.host = {k: _guarded(v) for k, v in start.items()}
        self.dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in self.host.items()}

    def call(self, reset, rewards=None, dones=None, E=None, N=None, null=None):
        from rltime_amd._lib import lib
        d = dict(self.dev)
        if null is not None:
            d[null] = None
        return lib.mirl_eval_count(self.E if E is None else E, self.N if N is None else N, reset, _p(rewards), _p(dones),
                                   _p(d["acc"]), _p(d["len"]), _p(d["open"]), _p(d["counters"]), _p(d["ep_reward"]),
                                   _p(d["ep_len"]), _st())

    def mirror(self):
        for k in self.KEYS:
            v = getattr(self.ec, k)
            self.host[k][:len(v)] = v

    def check(self, what):
        for k in self.KEYS:
            got = self.dev[k].cpu().numpy()
            assert got.dtype == self.host[k].dtype and np.array_equal(_bits(got), _bits(self.host[k])), (what, k)


@pytest.fixture(scope="module")
def cases():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _case_ids():
    with np.load(GOLDEN) as z:
        return list(range(int(z["num_cases"])))


@pytest.mark.parametrize("k", _case_ids())
def test_kernel_equals_the_restatement_after_every_step(cases, k):
    rewards, dones, N = cases["c%d_rewards" % k], cases["c%d_dones" % k], int(cases["c%d_n" % k])
    T, E = rewards.shape
    steps = int(cases["c%d_steps" % k])
    st = _Dev(E, N, garbage=True)
    r_d, d_d = torch.from_numpy(rewards.reshape(-1).copy()).cuda(), torch.from_numpy(dones.reshape(-1).copy()).cuda()
    assert st.call(1) == 0
    st.ec.reset()
    st.ec.ep_reward[:], st.ec.ep_len[:] = st.host["ep_reward"][:N], st.host["ep_len"][:N]
    st.mirror()
    st.check("reset")
    for t in range(steps):
        assert st.call(0, r_d[t * E:], d_d[t * E:]) == 0
        st.ec.step(rewards[t], dones[t])
        st.mirror()
        st.check("step %d" % t)
    assert st.ec.finished and int(st.ec.counters[2]) == steps
    got = st.dev["ep_reward"].cpu().numpy()[:N]
    assert np.array_equal(got.view(np.uint64), cases["c%d_ep_reward" % k].view(np.uint64))       # the reference's own list
    # ten more launches after the quota change nothing
    for t in range(steps, steps + 10):
        assert st.call(0, r_d[t * E:], d_d[t * E:]) == 0
    st.check("over-run")
    # a reset restores the initial state (the lists keep their contents: the next evaluation overwrites all N entries)
    assert st.call(1) == 0
    keep = (st.ec.ep_reward.copy(), st.ec.ep_len.copy())
    st.ec.reset()
    st.ec.ep_reward[:], st.ec.ep_len[:] = keep
    st.mirror()
    st.check("second reset")
    assert st.ec.counters.tolist() == [E, 0, 0, 0] and bool(st.ec.open.all())


def test_bad_arguments_are_refused_before_any_launch():
    E, N = 5, 8
    st = _Dev(E, N, garbage=True)
    r = torch.ones(E, dtype=torch.float32, device="cuda")
    d = torch.ones(E, dtype=torch.uint8, device="cuda")
    assert st.call(0, r, d, E=9, N=8) == ERR_ARG and st.call(1, E=9, N=8) == ERR_ARG         # E > N (eval.py:74)
    assert st.call(0, r, d, E=0) == ERR_ARG and st.call(0, r, d, E=65536, N=70000) == ERR_ARG
    assert st.call(2, r, d) == ERR_ARG
    assert st.call(0, None, d) == ERR_ARG and st.call(0, r, None) == ERR_ARG
    for name in _Dev.KEYS:
        assert st.call(0, r, d, null=name) == ERR_ARG and st.call(1, null=name) == ERR_ARG, name
    from rltime_amd._lib import last_error
    assert "eval_count" in last_error()
    torch.cuda.synchronize()
    st.check("refused calls")
