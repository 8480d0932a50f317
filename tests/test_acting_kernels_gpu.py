"""GPU: the code around the network in the acting vector step, through its C entry points, against the NumPy restatements of
tests/pointwise_restate.py (proved on hand-worked cases by tests/test_pointwise_restate_cpu.py):

  mirl_actor_pre, mirl_episode_track, mirl_synth_env_step, mirl_synth_env_step_pre, mirl_stack_shift      csrc/acting.hip
  mirl_copy_bytes, mirl_copy_bytes_ex (all eight launch forms)                                            csrc/replay.hip
  mirl_frames_to_f32_nhwc_ex (four load / store forms x tiles per workgroup, and the generic kernel)      csrc/convert.hip

These kernels move bytes, count, and do at most one float32 operation per value, so every comparison is bit for bit: floats
are compared as their int32 patterns (-0.0 is not +0.0), and there is no tolerance anywhere in this file.  Every output buffer
is longer than the kernel may write and starts out filled with a pattern; the restatement is applied to a copy of the same
buffer, so a write into a guard element, a pitch gap or an output that was passed as NULL shows as a difference.

NaN rewards are left out on purpose: the kernel's sign clip (r > 0 ? 1 : r < 0 ? -1 : 0) maps NaN to 0 where np.sign gives NaN,
and no environment produces one.  Infinite h / c are left out too (inf * 0 is NaN on both sides, with unspecified payload)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pointwise_restate as R

pytestmark = pytest.mark.gpu

ERR_ARG = -1                                  # include/mirl.h MIRL_ERR_ARG
F32_FILL = 0x7FC5A5A5                         # a quiet NaN no kernel here produces
G = 256                                       # guard bytes around byte buffers (keeps the inner pointer 16-byte aligned)


def _lib():
    from rltime_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _fill(n, dtype):
    """n elements of the pattern a kernel must leave alone."""
    if dtype == np.float32:
        return np.full(n, F32_FILL, np.int32).view(np.float32)
    return np.full(n, {np.uint8: 0xA5, np.int32: -77777, np.uint64: 0x5A5A5A5A5A5A5A5A}[dtype], dtype)


def _with_guard(a, extra=9):
    """a, followed by `extra` pattern elements."""
    return np.concatenate([a, _fill(extra, a.dtype.type)])


_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}


def _up(a):
    """NumPy array -> device tensor with the same bytes (None stays None)."""
    if a is None:
        return None
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype)).copy()).cuda()


def _down(t, like):
    return None if t is None else t.cpu().numpy().view(like.dtype)


def _same(got, want, what):
    """Bit equality of two arrays of one dtype (floats as int32)."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    a, b = got.view(np.uint8), want.view(np.uint8)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(got.view(_bits_of(got)) != want.view(_bits_of(want)))
        raise AssertionError("%s: %d of %d elements differ, first at %d: got %r, want %r"
                             % (what, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))


def _bits_of(a):
    return {4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize]


_RANDOM = {}


PERIOD = 8_500_003                            # odd: no frame, plane or pool batch size divides it


def _bytes(n, offset=0):
    """n reproducible random bytes from position `offset` of one 8.5 MB draw repeated with period PERIOD (shared by the whole
    module, never modified; only the largest env pools, up to 16.8 MB, reach past the first period)."""
    if "b" not in _RANDOM:
        _RANDOM["b"] = np.random.default_rng(20240).integers(0, 256, PERIOD, dtype=np.uint8)
    b, offset = _RANDOM["b"], offset % PERIOD
    if offset + n <= PERIOD:
        return b[offset:offset + n]
    return np.concatenate([b[offset:], np.resize(b, offset + n - PERIOD)])


def _guarded(n):
    """-> (whole, inner): a device uint8 buffer of G + n + G pattern bytes and its inner n bytes (16-byte aligned)."""
    whole = torch.full((G + n + G,), 0xA5, dtype=torch.uint8, device="cuda")
    inner = whole[G:G + n]
    assert inner.data_ptr() % 16 == 0
    return whole, inner


def _guards_intact(whole, n):
    return bool((whole[:G] == 0xA5).all()) and bool((whole[G + n:] == 0xA5).all())


# ---- mirl_actor_pre ----------------------------------------------------------------------------------------------------------
PRE_KEYS = ("xh", "c_in", "state_pack", "initials", "rewards_out", "dones_out", "ep_reward", "ep_len", "out_reward", "out_len",
            "action_counts", "rng_step")
REWARDS5 = np.array([0.0, -0.0, 1e-45, 3e38, -3e38], dtype=np.float32)      # both zeros, a positive subnormal, large of both signs


def _carry(E, H, seed):
    """h, c (E * H) with negative values and zeros of both signs."""
    g = np.random.default_rng(seed)
    h, c = g.standard_normal(E * H).astype(np.float32), g.standard_normal(E * H).astype(np.float32)
    h[0::5], h[1::7], c[2::5], c[3::7] = -0.0, 0.0, -0.0, 0.0
    return h, c


def _pre_state(E, H, pitch, A, seed, with_ep=True, with_counts=True, with_step=True, null_state=False):
    """The output buffers before the first launch: pattern everywhere but in the accumulators' first E (A) elements."""
    g = np.random.default_rng(seed)
    st = dict.fromkeys(PRE_KEYS)
    if not (H == 0 and null_state):
        st["xh"], st["c_in"], st["state_pack"] = _fill(E * pitch + 9, np.float32), _fill(E * H + 9, np.float32), _fill(2 * E * H + 9, np.float32)
    st["initials"], st["rewards_out"], st["dones_out"] = _fill(E + 9, np.float32), _fill(E + 9, np.float32), _fill(E + 9, np.uint8)
    if with_ep:
        st["ep_reward"] = _with_guard((g.standard_normal(E) * 4).astype(np.float32))
        st["ep_len"] = _with_guard(g.integers(0, 1000, E).astype(np.int32))
        st["out_reward"], st["out_len"] = _fill(E + 9, np.float32), _fill(E + 9, np.int32)
    if with_counts:
        st["action_counts"] = _with_guard(g.integers(0, 50, max(A, 1)).astype(np.int32)[:A])
    if with_step:
        st["rng_step"] = _with_guard(np.array([41], dtype=np.uint64), 3)
    return st


def _pre_tail(H, A, pitch, clip, dev, step):
    """mirl_actor_pre's arguments from `actions` on (shared with mirl_synth_env_step_pre)."""
    return [_p(dev["actions"]), _p(dev["h"]), _p(dev["c"]), _p(dev["xh"]), pitch, _p(dev["c_in"]), _p(dev["state_pack"]),
            _p(dev["initials"]), _p(dev["rewards_out"]), _p(dev["dones_out"]), clip, _p(dev["ep_reward"]), _p(dev["ep_len"]),
            _p(dev["out_reward"]), _p(dev["out_len"]), _p(dev["action_counts"]), _p(dev["rng_step"]), step, _st()]


def _pre_stream(E, H, pitch, A, h, c, state, steps, clip):
    """Launch mirl_actor_pre once per (raw, dones, actions, step) of `steps` on ONE set of device buffers; after every launch
    every buffer equals the restatement applied to the buffers before it.  -> the final state."""
    L = _lib()
    dev = {k: _up(v) for k, v in state.items()}
    dev["h"], dev["c"] = (_up(h), _up(c)) if h is not None else (None, None)
    for n, (raw, dones, actions, step) in enumerate(steps):
        dev["actions"] = _up(actions)
        rd, dd = _up(raw), _up(dones)
        L.check(L.lib.mirl_actor_pre(E, H, A, _p(rd), _p(dd), *_pre_tail(H, A, pitch, clip, dev, step)), "mirl_actor_pre")
        torch.cuda.synchronize()
        with np.errstate(over="ignore"):
            want = R.actor_pre(raw, dones, H, h, c, state["xh"], pitch, state["c_in"], state["state_pack"], state["initials"],
                               state["rewards_out"], state["dones_out"], clip, actions=actions, A=A, ep_reward=state["ep_reward"],
                               ep_len=state["ep_len"], out_reward=state["out_reward"], out_len=state["out_len"],
                               action_counts=state["action_counts"], rng_step=state["rng_step"], step=step)
        for k in PRE_KEYS:
            if want[k] is not None:
                _same(_down(dev[k], want[k]), want[k], "launch %d: %s" % (n, k))
        state = want
    return state


def _dones(kind, E, k):
    if kind == "zeros":
        return np.zeros(E, dtype=np.uint8)
    if kind == "ones":
        return np.array([(1, 255, 2)[(e + k) % 3] for e in range(E)], dtype=np.uint8)       # any non-zero byte is a done
    return np.array([(e + k) % 2 for e in range(E)], dtype=np.uint8)


def _actions(E, A, k, seed):
    a = np.random.default_rng(seed).integers(0, A, E).astype(np.int32)
    a[0] = (-1, A)[k % 2]
    if E > 1:
        a[1] = (A, -1)[k % 2]
    return a


PRE_VARIANTS = [  # dones, clip, episode pointers, actions, action_counts, the step word, NULL state pointers at H = 0
    dict(dones="zeros", clip=0, ep=True, act=True, counts=True, step="explicit", null_state=False),
    dict(dones="ones", clip=1, ep=True, act=False, counts=True, step="advance", null_state=True),
    dict(dones="mixed", clip=1, ep=False, act=True, counts=True, step="null", null_state=False),
    dict(dones="mixed", clip=0, ep=True, act=True, counts=False, step="advance", null_state=True),
    dict(dones="ones", clip=0, ep=False, act=False, counts=False, step="explicit", null_state=True),
    dict(dones="mixed", clip=1, ep=True, act=True, counts=True, step="explicit", null_state=False),
    dict(dones="zeros", clip=1, ep=True, act=True, counts=True, step="advance", null_state=False),
]


@pytest.mark.parametrize("gap", [0, 37])
@pytest.mark.parametrize("H", [0, 1, 255, 256, 257, 515])
@pytest.mark.parametrize("E", [1, 5])
def test_actor_pre_equals_the_restatement_bit_for_bit(E, H, gap):
    """Every variant of PRE_VARIANTS at this (E, H, xh_pitch = H + gap).  'advance' launches MIRL_STEP_ADVANCE twice on the same
    buffers (the counter ends at + 2 and the statistics see two steps)."""
    A, pitch = 6, H + gap
    h, c = _carry(E, H, 31 * E + H) if H else (None, None)
    for k, v in enumerate(PRE_VARIANTS):
        state = _pre_state(E, H, pitch, A, 100 + k, v["ep"], v["counts"], v["step"] != "null", v["null_state"])
        raw = np.roll(REWARDS5, k)[:E].copy()
        dones = _dones(v["dones"], E, k)
        actions = _actions(E, A, k, 7 + k) if v["act"] else None
        steps = {"explicit": [(raw, dones, actions, 1000 + k)], "null": [(raw, dones, actions, 5)],
                 "advance": [(raw, dones, actions, R.STEP_ADVANCE)] * 2}[v["step"]]
        end = _pre_stream(E, H, pitch, A, h, c, state, steps, v["clip"])
        if v["step"] == "advance":
            assert int(end["rng_step"][0]) == 43
        if v["step"] == "explicit":
            assert int(end["rng_step"][0]) == 1000 + k
        if H and v["dones"] == "ones":                                      # a reset gives the signed zero of x * 0.0f
            want_zero = np.where(np.signbit(h), np.float32(-0.0), np.float32(0.0)).astype(np.float32)
            _same(end["state_pack"][:2 * E * H].reshape(E, 2 * H)[:, :H].reshape(-1), want_zero, "reset h")


def _reward_stream(T, E, seed):
    """float32 rewards, dones with an episode ending mid-stream (env 0, step 17), a done on the first step (env 1) and an env
    that never ends (env 2), actions in [-1, A]."""
    g = np.random.default_rng(seed)
    raw = (g.standard_normal((T, E)) * 3).astype(np.float32) + np.float32(0.1)
    dones = (g.random((T, E)) < 0.1).astype(np.uint8)
    dones[:, 0] = 0
    dones[17 % T, 0] = 1
    if E > 1:
        dones[0, 1] = 1
    if E > 2:
        dones[:, 2] = 0
    actions = g.integers(-1, 7, (T, E)).astype(np.int32)
    return raw, dones, actions


def test_actor_pre_40_step_stream_keeps_sequential_float32_sums():
    E, H, A, T = 5, 3, 6, 40
    raw, dones, actions = _reward_stream(T, E, 3)
    seq = np.float32(0.0)
    for t in range(T):
        seq = seq + raw[t, 2]
    assert seq.dtype == np.float32 and seq != np.float32(raw[:, 2].astype(np.float64).sum()), "pick another seed"
    state = _pre_state(E, H, H + 37, A, 11)
    state["ep_reward"][:E], state["ep_len"][:E] = 0.0, 0
    h, c = _carry(E, H, 12)
    steps = [(raw[t], dones[t], actions[t], R.STEP_ADVANCE) for t in range(T)]
    end = _pre_stream(E, H, H + 37, A, h, c, state, steps, clip=1)
    assert end["ep_reward"][2].view(np.int32) == seq.view(np.int32) and int(end["ep_len"][2]) == T
    assert int(end["rng_step"][0]) == 41 + T


def _pre_valid_args(x, u8, i32, w64):
    """Valid mirl_actor_pre arguments (E = 2, H = 2): every buffer its own 8-element stretch of the zeroed x (64 floats), u8, i32."""
    X, U, I = (lambda k: _p(x[8 * k:])), (lambda k: _p(u8[8 * k:])), (lambda k: _p(i32[8 * k:]))
    return [2, 2, 2, X(0), U(0), I(0), X(1), X(2), X(3), 2, X(4), X(5), X(6), X(7), U(1), 1, _p(x[60:]), I(1),
            _p(x[62:]), I(2), I(3), _p(w64), 3, _st()]


PRE_BAD = [(0, 0), (0, -1), (1, -1), (3, None), (4, None), (6, None), (7, None), (8, None), (10, None), (11, None), (12, None),
           (13, None), (14, None), (17, None), (18, None), (19, None)]


def test_actor_pre_refuses_bad_arguments_and_writes_nothing():
    L = _lib()
    x, u8 = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    i32, w64 = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    for pos, bad in PRE_BAD:
        a = _pre_valid_args(x, u8, i32, w64)
        a[pos] = bad
        assert L.lib.mirl_actor_pre(*a) == ERR_ARG, pos
    torch.cuda.synchronize()
    assert not x.any() and not u8.any() and not i32.any() and not w64.any()
    a = _pre_valid_args(x, u8, i32, w64)                                      # the same list without a fault is accepted
    assert L.lib.mirl_actor_pre(*a) == 0
    a[1], a[6], a[7], a[8], a[10], a[11] = 0, None, None, None, None, None   # H = 0: the state pointers may be NULL
    assert L.lib.mirl_actor_pre(*a) == 0
    torch.cuda.synchronize()
    assert int(w64[0]) == 3


# ---- mirl_episode_track ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 255, 256, 257, 513])
def test_episode_track_equals_the_restatement_and_actor_pre(E):
    """A 20-step stream through mirl_episode_track and, on a second set of buffers, through mirl_actor_pre (H = 0): both equal
    the restatement after every step, hence each other; the histogram gained one count per action in [0, A)."""
    L = _lib()
    A, T = 6, 20
    raw, dones, actions = _reward_stream(T, E, 50 + E)
    names = ("ep_reward", "ep_len", "out_reward", "out_len", "action_counts")
    state = _pre_state(E, 0, 0, A, 60 + E, with_step=False, null_state=True)
    counts0 = state["action_counts"].copy()
    trk = {k: _up(state[k]) for k in names}
    pre = {k: _up(v) for k, v in state.items()}
    pre["h"] = pre["c"] = None
    cur = tuple(state[k] for k in names)
    for t in range(T):
        rd, dd, ad = _up(raw[t]), _up(dones[t]), _up(actions[t])
        pre["actions"] = ad
        L.check(L.lib.mirl_episode_track(E, A, _p(rd), _p(dd), _p(ad), *[_p(trk[k]) for k in names], _st()), "mirl_episode_track")
        L.check(L.lib.mirl_actor_pre(E, 0, A, _p(rd), _p(dd), *_pre_tail(0, A, 0, 1, pre, 0)), "mirl_actor_pre")
        torch.cuda.synchronize()
        cur = R.episode_track(raw[t], dones[t], actions[t], A, *cur)
        for k, w in zip(names, cur):
            _same(_down(trk[k], w), w, "step %d: episode_track %s" % (t, k))
            _same(_down(pre[k], w), w, "step %d: actor_pre %s" % (t, k))
    assert int(cur[4][:A].sum() - counts0[:A].sum()) == int(((actions >= 0) & (actions < A)).sum())
    # NULL actions, then NULL action_counts: the statistics go on, the histogram stands still
    rd, dd = _up(raw[0]), _up(dones[0])
    for ad, cd in ((None, trk["action_counts"]), (_up(actions[0]), None)):
        L.check(L.lib.mirl_episode_track(E, A, _p(rd), _p(dd), _p(ad), *[_p(trk[k]) for k in names[:4]], _p(cd), _st()), "mirl_episode_track")
        torch.cuda.synchronize()
        cur = R.episode_track(raw[0], dones[0], None, A, *cur)
        for k, w in zip(names, cur):
            _same(_down(trk[k], w), w, "NULL histogram argument: %s" % k)


def test_episode_track_refuses_bad_arguments():
    L = _lib()
    x, u8, i32 = torch.zeros(8, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    X, U, I = _p(x), _p(u8), _p(i32)
    for pos, bad in [(0, 0), (2, None), (3, None), (5, None), (6, None), (7, None), (8, None)]:
        a = [2, 2, X, U, I, X, I, X, I, I, _st()]
        a[pos] = bad
        assert L.lib.mirl_episode_track(*a) == ERR_ARG, pos
    torch.cuda.synchronize()
    assert not x.any() and not i32.any()


# ---- mirl_synth_env_step -----------------------------------------------------------------------------------------------------
PROBS = (0.3, 0.7, 0.25)
CLOCK_FILL = 0x5A5A5A5A5A5A5A5A


class _Env:
    """Device buffers of one synthetic env: pool (pool_n, E, frame_bytes), the clock pair (followed by two guard words),
    obs / rewards / dones with guards."""

    def __init__(self, E, fb, pool_n, t0, slot, seed, offset=0):
        self.E, self.fb, self.pool_n, self.slot, self.seed, self.t = E, fb, pool_n, slot, seed, t0
        self.pool = _bytes(pool_n * E * fb, offset).reshape(pool_n, E * fb)
        self.pool_d = _up(self.pool.reshape(-1))
        clock = np.full(4, CLOCK_FILL, dtype=np.uint64)
        clock[slot] = t0
        self.clock = clock
        self.clock_d = _up(clock)
        self.obs, self.rew, self.don = _fill(E * fb + 64, np.uint8), _fill(E + 9, np.float32), _fill(E + 9, np.uint8)
        self.obs_d, self.rew_d, self.don_d = _up(self.obs), _up(self.rew), _up(self.don)

    def args(self, probs):
        return [self.E, self.fb, _p(self.pool_d), self.pool_n, _p(self.clock_d), self.slot, self.seed, float(probs[0]), float(probs[1]),
                float(probs[2]), _p(self.obs_d), _p(self.rew_d), _p(self.don_d)]

    def expect(self, probs):
        """Advance the host copies by one step -> (rewards, dones) of that step."""
        self.t += 1
        r, d, idx, _, _ = R.synth_env_draws(self.seed, self.t, self.E, *probs, pool_n=self.pool_n)
        self.obs[:self.E * self.fb] = self.pool[idx]
        self.rew[:self.E], self.don[:self.E] = r, d
        self.clock[self.slot ^ 1] = self.t                                  # the word read stays, the other one becomes t
        self.slot ^= 1
        return r, d

    def check(self, what):
        torch.cuda.synchronize()
        _same(_down(self.rew_d, self.rew), self.rew, what + ": rewards")
        _same(_down(self.don_d, self.don), self.don, what + ": dones")
        _same(_down(self.clock_d, self.clock), self.clock, what + ": clock pair")
        _same(_down(self.obs_d, self.obs), self.obs, what + ": obs")


def _step(env, probs=PROBS):
    L = _lib()
    L.check(L.lib.mirl_synth_env_step(*env.args(probs), _st()), "mirl_synth_env_step")
    out = env.expect(probs)
    env.check("t = %d" % env.t)
    return out


@pytest.mark.parametrize("pool_n", [1, 3, 8])
@pytest.mark.parametrize("fb", [16, 4080, 4096, 4112, 28224, 32784])
@pytest.mark.parametrize("E", [1, 3, 64])
def test_synth_env_step_values_frames_and_clock(E, fb, pool_n):
    """Four steps with alternating slot: rewards and dones value by value, obs byte-equal to pool batch t % pool_n (32784 bytes
    = 2049 quads per env: the copy loop takes a second stride), the word read untouched and the other word = t."""
    env = _Env(E, fb, pool_n, t0=5 + E, slot=(E + fb // 16 + pool_n) % 2, seed=900 + fb + pool_n, offset=977 * (E + pool_n))
    seen_r, seen_d = set(), set()
    for _ in range(4):
        r, d = _step(env)
        seen_r |= set(r.tolist())
        seen_d |= set(d.tolist())
    if E == 64:
        assert seen_r == {-1.0, 0.0, 1.0} and seen_d == {0, 1}


def test_synth_env_step_uses_the_high_word_of_the_clock():
    env = _Env(3, 16, 3, t0=2 ** 32 - 2, slot=1, seed=77)
    for _ in range(4):
        _step(env)
    assert env.t == 2 ** 32 + 2
    for k in range(3):                                                       # t mod 2^32 alone would give other draws
        assert not np.array_equal(R.synth_env_draws(77, 2 ** 32 + k, 3, *PROBS)[3], R.synth_env_draws(77, k, 3, *PROBS)[3])


def test_synth_env_step_thresholds_are_strict_and_the_extremes_hold():
    E, seed, t0 = 64, 4242, 9
    _, _, _, u0, u1 = R.synth_env_draws(seed, t0 + 1, E, *PROBS)
    k0, k1 = int(np.argsort(u0)[E // 2]), int(np.argsort(u1)[E // 2])
    assert u0[k0] > 0 and u1[k1] > 0
    up0, up1 = np.nextafter(u0[k0], np.float32(2)), np.nextafter(u1[k1], np.float32(2))

    def one(probs):
        return _step(_Env(E, 16, 1, t0, 0, seed), probs)

    assert one((0.0, 1.0, u1[k1]))[1][k1] == 0 and one((0.0, 1.0, up1))[1][k1] == 1           # u1 < p_done, not <=
    assert one((u0[k0], 1.0, 0.5))[0][k0] == 0.0 and one((up0, 1.0, 0.5))[0][k0] == -1.0      # u0 < p_neg
    assert one((0.0, u0[k0], 0.5))[0][k0] == 1.0 and one((0.0, up0, 0.5))[0][k0] == 0.0       # u0 < p_nonpos
    r, d = one((0.0, 1.0, 0.0))
    assert not r.any() and not d.any()
    r, d = one((0.0, 1.0, 1.0))
    assert not r.any() and d.all()


def test_synth_env_step_refuses_bad_arguments_and_writes_nothing():
    L = _lib()
    env = _Env(2, 32, 2, 5, 0, 1)
    pool8, obs8, clock8 = env.pool_d[8:], env.obs_d[8:], env.clock_d[1:]
    assert pool8.data_ptr() % 16 == 8 and obs8.data_ptr() % 16 == 8 and clock8.data_ptr() % 16 == 8
    for pos, bad in [(1, 24), (5, 2), (3, 0), (2, _p(pool8)), (10, _p(obs8)), (4, _p(clock8)), (0, 0), (1, 0), (5, -1), (11, None), (12, None)]:
        a = env.args(PROBS) + [_st()]
        a[pos] = bad
        assert L.lib.mirl_synth_env_step(*a) == ERR_ARG, pos
    env.check("after refusals")


# ---- mirl_synth_env_step_pre -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [0, 100, 515])
def test_synth_env_step_pre_is_the_draws_composed_with_actor_pre(H):
    L = _lib()
    E, A, pitch, clip = 3, 6, H + 37, 1
    env = _Env(E, 4112, 3, t0=20 + H, slot=H % 2, seed=31 + H)
    probs = (0.3, 0.7, 0.5)
    h, c = _carry(E, H, 70 + H) if H else (None, None)
    state = _pre_state(E, H, pitch, A, 80 + H)
    dev = {k: _up(v) for k, v in state.items()}
    dev["h"], dev["c"] = _up(h), _up(c)
    seen = set()
    for n in range(4):
        actions = _actions(E, A, n, 90 + n)
        dev["actions"] = _up(actions)
        step = R.STEP_ADVANCE if n % 2 else 500 + n
        L.check(L.lib.mirl_synth_env_step_pre(*env.args(probs), H, A, *_pre_tail(H, A, pitch, clip, dev, step)), "mirl_synth_env_step_pre")
        raw, dones = env.expect(probs)
        env.check("step %d" % n)
        seen |= set(dones.tolist())
        state = R.actor_pre(raw, dones, H, h, c, state["xh"], pitch, state["c_in"], state["state_pack"], state["initials"],
                            state["rewards_out"], state["dones_out"], clip, actions=actions, A=A, ep_reward=state["ep_reward"],
                            ep_len=state["ep_len"], out_reward=state["out_reward"], out_len=state["out_len"],
                            action_counts=state["action_counts"], rng_step=state["rng_step"], step=step)
        for k in PRE_KEYS:
            _same(_down(dev[k], state[k]), state[k], "step %d: %s" % (n, k))
    assert seen == {0, 1}, "pick another seed: the carry must be both kept and reset"


def test_synth_env_step_pre_refuses_what_actor_pre_refuses():
    L = _lib()
    env = _Env(2, 32, 2, 5, 0, 1)
    x, u8 = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    i32, w64 = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    for pos, bad in PRE_BAD:
        if pos in (0, 3, 4):                                                  # E, rewards_raw, dones: the env's own arguments here
            continue
        pre = _pre_valid_args(x, u8, i32, w64)
        pre[pos] = bad
        assert L.lib.mirl_synth_env_step_pre(*env.args(PROBS), pre[1], pre[2], *pre[5:]) == ERR_ARG, pos
    for pos, bad in [(0, 0), (1, 24), (5, 2), (3, 0)]:
        a = env.args(PROBS)
        a[pos] = bad
        pre = _pre_valid_args(x, u8, i32, w64)
        assert L.lib.mirl_synth_env_step_pre(*a, pre[1], pre[2], *pre[5:]) == ERR_ARG, pos
    env.check("after refusals")
    assert not x.any() and not u8.any() and not i32.any() and not w64.any()


# ---- mirl_stack_shift --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 5])
@pytest.mark.parametrize("plane", [16, 7056, 16384])
@pytest.mark.parametrize("P", [2, 3, 4])
def test_stack_shift_equals_the_restatement(P, plane, E):
    """P = 4 with 16384-byte planes is 4096 quads per env: twice what the capped grid covers in one stride."""
    L = _lib()
    inp = _bytes(E * P * plane, 13 * P).reshape(E, P, plane)
    newest = _bytes(E * plane, 5_000_000 + plane).reshape(E, plane)
    in_d, new_d = _up(inp.reshape(-1)), _up(newest.reshape(-1))
    for k in range(2):
        dones = np.array([(e + k) % 2 for e in range(E)], dtype=np.uint8)
        whole, out_d = _guarded(E * P * plane)
        dones_d = _up(dones)
        L.check(L.lib.mirl_stack_shift(E, P, plane, _p(in_d), _p(out_d), _p(new_d), _p(dones_d), _st()), "mirl_stack_shift")
        torch.cuda.synchronize()
        _same(out_d.cpu().numpy().reshape(E, P, plane), R.stack_shift(inp, newest, dones), "dones %s" % dones.tolist())
        assert _guards_intact(whole, E * P * plane)
        assert np.array_equal(in_d.cpu().numpy(), inp.reshape(-1)) and np.array_equal(new_d.cpu().numpy(), newest.reshape(-1))


def test_stack_shift_refuses_bad_arguments_and_writes_nothing():
    L = _lib()
    buf = torch.zeros(3 * 2 * 32 + 64, dtype=torch.uint8, device="cuda")
    whole, out = _guarded(2 * 2 * 32 + 64)
    d = torch.zeros(2, dtype=torch.uint8, device="cuda")
    I, O, N, D = _p(buf), _p(out), _p(buf[128:]), _p(d)
    for pos, bad in [(1, 1), (4, I), (2, 24), (3, _p(buf[8:])), (4, _p(out[8:])), (5, _p(buf[136:])), (0, 0), (2, 0), (3, None), (4, None),
                     (5, None), (6, None)]:
        a = [2, 2, 32, I, O, N, D, _st()]
        a[pos] = bad
        assert L.lib.mirl_stack_shift(*a) == ERR_ARG, pos
    torch.cuda.synchronize()
    assert bool((whole == 0xA5).all()) and not buf.any()


# ---- mirl_copy_bytes / mirl_copy_bytes_ex ------------------------------------------------------------------------------------
COPY_QUADS = [1, 255, 256, 257, 511, 512, 513, 1023, 1025, 2047, 2048, 2049, 524288 + 1]
_COPY_SRC = {}


def _copy_src(quads):
    if quads not in _COPY_SRC:
        _COPY_SRC[quads] = _up(_bytes(16 * quads, 3 * quads % 1000))
    return _COPY_SRC[quads]


@pytest.mark.parametrize("quads", COPY_QUADS)
@pytest.mark.parametrize("nt", ["plain", 0, 1, 2, 3, 4, 5, 6, 7])
def test_copy_bytes_every_launch_form_copies_exactly_the_bytes(nt, quads):
    """Sizes on both sides of 256 * PER for PER = 2, 4, 8 and of the 2048 quads a k_copy16_nt workgroup covers; 524289 quads is
    one more than k_copy16's fixed grid holds, so it takes a second stride.  'plain' is mirl_copy_bytes."""
    L = _lib()
    n = 16 * quads
    src = _copy_src(quads)
    whole, dst = _guarded(n)
    if nt == "plain":
        L.check(L.lib.mirl_copy_bytes(_p(dst), _p(src), n, _st()), "mirl_copy_bytes")
    else:
        L.check(L.lib.mirl_copy_bytes_ex(_p(dst), _p(src), n, nt, _st()), "mirl_copy_bytes_ex")
    torch.cuda.synchronize()
    assert torch.equal(dst, src), "%d bytes differ" % int((dst != src).sum())
    assert _guards_intact(whole, n)
    assert np.array_equal(src[:4096].cpu().numpy(), _bytes(16 * quads, 3 * quads % 1000)[:4096])        # the source is not written


def test_copy_bytes_refuses_bad_arguments_and_writes_nothing():
    L = _lib()
    src = _copy_src(256)
    whole, dst = _guarded(4096)
    assert L.lib.mirl_copy_bytes_ex(_p(dst), _p(src), 4096, 8, _st()) == ERR_ARG
    for nt in range(8):
        assert L.lib.mirl_copy_bytes_ex(_p(dst), _p(src), 24, nt, _st()) == ERR_ARG
        assert L.lib.mirl_copy_bytes_ex(_p(dst[8:]), _p(src), 64, nt, _st()) == ERR_ARG
        assert L.lib.mirl_copy_bytes_ex(_p(dst), _p(src[8:]), 64, nt, _st()) == ERR_ARG
        assert L.lib.mirl_copy_bytes_ex(_p(dst), _p(src), 0, nt, _st()) == ERR_ARG
        assert L.lib.mirl_copy_bytes_ex(None, _p(src), 64, nt, _st()) == ERR_ARG
        assert L.lib.mirl_copy_bytes_ex(_p(dst), None, 64, nt, _st()) == ERR_ARG
    assert L.lib.mirl_copy_bytes(_p(dst), _p(src), 24, _st()) == ERR_ARG
    assert L.lib.mirl_copy_bytes(_p(dst[8:]), _p(src), 64, _st()) == ERR_ARG
    assert L.lib.mirl_copy_bytes(_p(dst), _p(src[8:]), 64, _st()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((whole == 0xA5).all())


# ---- mirl_frames_to_f32_nhwc_ex ----------------------------------------------------------------------------------------------
def _convert(x_d, N, Cn, HW, scale, per_wg=None, flags=None):
    """-> the whole output buffer (N * HW * Cn floats + 9 guard floats) as float32 on the host; per_wg None: the default call."""
    L = _lib()
    out = _up(_fill(N * HW * Cn + 9, np.float32))
    if per_wg is None:
        L.check(L.lib.mirl_frames_to_f32_nhwc(N, Cn, HW, _p(x_d), float(scale), _p(out), _st()), "mirl_frames_to_f32_nhwc")
    else:
        L.check(L.lib.mirl_frames_to_f32_nhwc_ex(N, Cn, HW, _p(x_d), float(scale), _p(out), per_wg, flags, _st()), "mirl_frames_to_f32_nhwc_ex")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.float32)


def _convert_want(x, scale):
    return _with_guard(R.frames_to_f32_nhwc(x, scale).reshape(-1))


@pytest.mark.parametrize("scale", [1.0 / 255.0, 1.0, 0.3])
@pytest.mark.parametrize("N,HW", [(3, 7056), (2, 1024), (2, 1040), (1, 16), (5, 2064)])
def test_frames_to_f32_every_variant_is_one_float32_product(N, HW, scale):
    """flags 0 .. 3 (non-temporal or plain loads / stores) x 0, 1, 2, 3, 7, 8 tiles per workgroup: 7056 pixels are 7 tiles with
    a partial last one, 1040 and 2064 end in a 16-pixel tile, 7 and 8 cover the whole frame in one workgroup."""
    scale = np.float32(scale)
    x = _bytes(N * 4 * HW, 31 * HW).reshape(N, 4, HW).copy()
    x[0, :, 0], x[-1, :, -1] = 0, 255
    x_d = _up(x.reshape(-1))
    want = _convert_want(x, scale)
    _same(_convert(x_d, N, 4, HW, scale), want, "default call")
    for flags in range(4):
        for per_wg in (0, 1, 2, 3, 7, 8):
            _same(_convert(x_d, N, 4, HW, scale, per_wg, flags), want, "flags %d, per_wg %d" % (flags, per_wg))


@pytest.mark.parametrize("Cn,HW,shift", [(1, 1003, 0), (3, 1003, 0), (5, 1003, 0), (4, 1003, 0), (5, 1024, 0), (4, 1024, 1), (4, 2064, 1)])
def test_frames_to_f32_generic_kernel(Cn, HW, shift):
    """Channel counts other than 4, a plane size that is no multiple of 16, and 4-channel frames whose source starts one byte off
    a 16-byte boundary (shift = 1): all take the one-lane-per-pixel kernel."""
    N, scale = 2, np.float32(0.3)
    x = _bytes(N * Cn * HW, 17 * Cn).reshape(N, Cn, HW)
    x_d = _up(np.concatenate([np.zeros(shift, np.uint8), x.reshape(-1)]))[shift:]
    assert x_d.data_ptr() % 16 == shift
    want = _convert_want(x, scale)
    _same(_convert(x_d, N, Cn, HW, scale), want, "default call")
    for per_wg, flags in ((0, 0), (3, 2), (8, 3)):
        _same(_convert(x_d, N, Cn, HW, scale, per_wg, flags), want, "flags %d, per_wg %d" % (flags, per_wg))


def test_frames_to_f32_refuses_bad_arguments_and_writes_nothing():
    L = _lib()
    x = torch.zeros(4 * 16, dtype=torch.uint8, device="cuda")
    out = _up(_fill(64 + 9, np.float32))
    for pos, bad in [(0, 0), (1, 0), (2, 0), (3, None), (5, None), (0, -1)]:
        a = [1, 4, 16, _p(x), 1.0, _p(out), 1, 1, _st()]
        a[pos] = bad
        assert L.lib.mirl_frames_to_f32_nhwc_ex(*a) == ERR_ARG, pos
        assert L.lib.mirl_frames_to_f32_nhwc(*(a[:6] + a[8:])) == ERR_ARG, pos
    torch.cuda.synchronize()
    _same(out.cpu().numpy().view(np.float32), _fill(64 + 9, np.float32), "output after refusals")
