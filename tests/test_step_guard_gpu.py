"""GPU: the step guard (csrc/optim.hip k_step_guard_open / k_adam_update_guarded, csrc/replay.hip k_loss_*_guarded,
mirl_lstm_seq_status_device) at its C entry points, and TorchTrainer's skip_invalid_steps on top of it.

The rule under test: with the guard on, an invalid learner step — a non-finite per-transition error, a non-finite gradient
norm, a non-zero status word — reaches neither the parameters, the gradients, the Adam moments, the step counters nor the
priority tree; a valid step with the guard on is the step without it, bit for bit.  Floats are compared as int32
patterns (NaN payloads and -0.0 count), every output buffer sits between fences that must stay as they were, NaN and Inf
are only ever values in buffers, and a failed sweep is simulated by the test's own int32 device word."""
import copy
import ctypes as C
import random

import numpy as np
import pytest
import torch

from tests.test_graph_step_gpu import BASE, CNN, deterministic_library            # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ERR_ARG = -1
VETO_LOSS, VETO_NORM, VETO_STATUS = 1, 2, 4
FENCE = 4                                     # words on either side of every buffer (16 bytes: alignment is kept)
FENCE_BITS = 0x7FC0BEEF                       # a NaN with a payload: a float op on it would not leave it alone
HYP = dict(lr=float(np.float32(2.5e-4)), b1=0.9, b2=0.999, eps=1.5e-4)
SIZES = [1, 4095, 4096, 4097, 9000]


def _lib():
    from rltime_amd import _lib
    return _lib


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Fenced:
    """`n` 4-byte words on the device between two fences; off = 1 starts the view 4 bytes off the 16-byte boundary."""
    def __init__(self, host, off=0):
        host = np.ascontiguousarray(host)
        assert host.dtype.itemsize == 4
        n = host.size
        store = np.full(FENCE + off + n + FENCE, FENCE_BITS, dtype=np.int32)
        store[FENCE + off:FENCE + off + n] = host.reshape(-1).view(np.int32)
        self.store = torch.from_numpy(store).cuda()
        self.lo, self.n, self.dtype = FENCE + off, n, host.dtype
        self.t = self.store[self.lo:self.lo + n].view(torch.float32 if host.dtype == np.float32 else torch.int32)
        assert self.t.data_ptr() % 16 == 4 * off

    def bits(self):
        """The whole store, fences included, as int32 on the host."""
        return self.store.cpu().numpy().copy()

    def fences_intact(self):
        b = self.bits()
        return bool((b[:self.lo] == FENCE_BITS).all() and (b[self.lo + self.n:] == FENCE_BITS).all())

    def words(self):
        return self.bits()[self.lo:self.lo + self.n]


def _guard(words=None):
    g = Fenced(np.zeros(8, dtype=np.int32) if words is None else np.asarray(words, dtype=np.int32))
    assert g.t.data_ptr() % 16 == 0
    return g


class AdamCase:
    """`count` tensors (sizes cycling through SIZES, steps 0 and 9 mixed, tensor `off_tensor` 4 bytes off alignment) as
    host arrays; device() makes one fenced device copy of all of it."""
    def __init__(self, count, seed=0):
        rng = np.random.RandomState(seed)
        self.count = count
        self.sizes = [SIZES[i % len(SIZES)] for i in range(count)]
        self.steps = [0 if i % 2 == 0 else 9 for i in range(count)]
        self.off_tensor = min(1, count - 1)
        self.p = [(rng.randn(n) * 0.1).astype(np.float32) for n in self.sizes]
        self.g = [(rng.randn(n) * 0.1).astype(np.float32) for n in self.sizes]
        self.m = [(rng.randn(n) * 0.01).astype(np.float32) * np.float32(s > 0) for n, s in zip(self.sizes, self.steps)]
        self.v = [(rng.rand(n) * 1e-4).astype(np.float32) * np.float32(s > 0) for n, s in zip(self.sizes, self.steps)]
        self.p[0][0] = np.float32(-0.0)                    # a pattern that only a bitwise comparison tells from 0.0

    def device(self):
        d = {k: [Fenced(x, off=int(i == self.off_tensor)) for i, x in enumerate(getattr(self, k))] for k in "pgmv"}
        d["step"] = [Fenced(np.array([s], dtype=np.float32)) for s in self.steps]
        d["out"] = Fenced(np.array([7.0, 7.0], dtype=np.float32))
        return d

    def run(self, d, clip, guard=None):
        L = _lib()
        n = self.count
        arr = lambda fs: (C.c_void_p * n)(*[f.t.data_ptr() for f in fs])                   # noqa: E731
        numel = (C.c_int64 * n)(*self.sizes)
        need = C.c_int64()
        L.check(L.lib.mirl_adam_clip_workspace_bytes(n, numel, C.byref(need)), "mirl_adam_clip_workspace_bytes")
        ws = torch.zeros(need.value // 8, dtype=torch.float64, device="cuda")
        args = (n, arr(d["p"]), arr(d["g"]), arr(d["m"]), arr(d["v"]), arr(d["step"]), numel, HYP["lr"], None, HYP["b1"],
                HYP["b2"], HYP["eps"], float(clip), _vp(ws), need.value, _vp(d["out"].t))
        if guard is None:
            rc = L.lib.mirl_adam_clip_step(*args, _stream())
        else:
            rc = L.lib.mirl_adam_clip_step_guarded(*args, _vp(guard.t) if isinstance(guard, Fenced) else guard, _stream())
        torch.cuda.synchronize()
        return rc


def _all_bits(d):
    return {k: [f.bits() for f in d[k]] for k in ("p", "g", "m", "v", "step")}


def _same_bits(a, b, keys=("p", "g", "m", "v", "step")):
    for k in keys:
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert np.array_equal(x, y), "%s of tensor %d differs" % (k, i)


def _fences(d):
    assert all(f.fences_intact() for k in ("p", "g", "m", "v", "step") for f in d[k]) and d["out"].fences_intact()


def _total_norm(case):
    return float(np.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in case.g)))


# -- 1. a clean step is the unguarded step -------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip_kind", ["off", "slack", "biting"])
@pytest.mark.parametrize("count", [1, 3, 33, 40])
def test_clean_guarded_step_is_the_unguarded_step(count, clip_kind):
    case = AdamCase(count, seed=count)
    norm = _total_norm(case)
    clip = {"off": 0.0, "slack": 4.0 * norm, "biting": 0.25 * norm}[clip_kind]
    a, b, guard = case.device(), case.device(), _guard()
    assert case.run(a, clip) == 0, _lib().last_error()
    assert case.run(b, clip, guard) == 0, _lib().last_error()
    _same_bits(_all_bits(a), _all_bits(b))
    assert np.array_equal(a["out"].bits(), b["out"].bits())
    _fences(a), _fences(b)
    assert [float(s.t[0]) for s in b["step"]] == [s + 1.0 for s in case.steps]
    out = b["out"].t.cpu().numpy()
    assert np.isfinite(out).all() and abs(out[0] - norm) <= 1e-4 * norm
    if clip_kind == "biting":
        assert out[1] < 0.5 * out[0]                      # the clip did bite: the gradients were rewritten in both
    assert guard.words().tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and guard.fences_intact()


# -- 2. a non-finite norm vetoes -----------------------------------------------------------------------------------------------
_WHERE = {"first_of_tensor_0": (0, 0), "last_of_4097_scalar_tail": (3, 4096), "tensor_35_second_launch": (35, 0)}


@pytest.mark.parametrize("clip", [0.0, 1.0])
@pytest.mark.parametrize("where", sorted(_WHERE))
@pytest.mark.parametrize("poison", ["nan", "+inf", "-inf", "3e19"])
def test_non_finite_norm_vetoes_the_step(poison, where, clip):
    case = AdamCase(40, seed=2)
    t, e = _WHERE[where]
    assert case.sizes[3] == 4097 and case.sizes[t] > e
    case.g[t][e] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "3e19": 3e19}[poison]     # 3e19: finite, its square is not
    if poison == "3e19":
        assert np.isfinite(case.g[t][e]) and float(case.g[t][e]) ** 2 > float(np.finfo(np.float32).max)
    d, guard = case.device(), _guard()
    before = _all_bits(d)
    assert case.run(d, clip, guard) == 0, _lib().last_error()
    _same_bits(before, _all_bits(d))                        # p, m, v, step AND g: the clip must not have scaled anything
    _fences(d)
    w = guard.words().tolist()
    assert w[0] == VETO_NORM and w[1] == 1 and w[2] == 1 and w[3] == 0 and w[4] == 1 and w[5] == 0 and w[6:] == [0, 0]
    assert guard.fences_intact()
    assert not np.isfinite(d["out"].t.cpu().numpy()[0])


# -- 3. - 6. guard_open ----------------------------------------------------------------------------------------------------------
def _open(guard, rows=None, count=None, status=(), n_status=None):
    L = _lib()
    n = len(status)
    arr = (C.c_void_p * max(n, 1))(*[s.data_ptr() for s in status]) if n else None
    if count is None:
        count = rows.n if rows is not None else 0
    rc = L.lib.mirl_step_guard_open(_vp(guard.t) if isinstance(guard, Fenced) else guard,
                                    _vp(rows.t) if isinstance(rows, Fenced) else rows, count, arr,
                                    n if n_status is None else n_status, _stream())
    torch.cuda.synchronize()
    return rc


def _finite_rows(count, seed=0):
    rows = (np.random.RandomState(seed).randn(count) * 3).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -1e-40, 3.4e38, -3.4e38, 1.17549435e-38], dtype=np.float32)    # incl. subnormals
    k = min(count, special.size)
    rows[:k] = special[:k]
    if count > 8:
        rows[-3:] = special[4:7]
    assert np.isfinite(rows).all()
    return rows


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("count", [0, 1, 5, 1023, 1024, 1025, 4099, 40960])
def test_guard_open_scans_every_row_count(count, off):
    if count == 0:
        guard = _guard([VETO_LOSS] + [0] * 7)
        assert _open(guard, None, 0) == 0, _lib().last_error()
        assert guard.words().tolist() == [0] * 8 and guard.fences_intact()
        return
    host = _finite_rows(count, seed=count)
    rows, guard = Fenced(host, off=off), _guard([VETO_NORM] + [0] * 7)
    before = rows.bits()
    assert _open(guard, rows) == 0, _lib().last_error()
    assert guard.words().tolist() == [0] * 8                  # finite rows (0, -0.0, subnormals, +-3.4e38 among them): no veto
    host[-1] = np.inf                                          # the LAST row: the tail of whichever path took it
    rows2 = Fenced(host, off=off)
    assert _open(guard, rows2) == 0
    assert guard.words().tolist() == [VETO_LOSS] + [0] * 7
    assert _open(guard, rows2, count=count - 1) == 0 and guard.words()[0] == 0   # ... and a row past `count` is not read
    assert np.array_equal(rows.bits(), before) and guard.fences_intact()       # the rows are read, never written


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("at", ["first", "middle", "last"])
@pytest.mark.parametrize("value", ["nan", "+inf", "-inf", "nan_payload"])
def test_guard_open_row_values(value, at, off):
    count = 4099
    host = _finite_rows(count, seed=5)
    i = {"first": 0, "middle": count // 2, "last": count - 1}[at]
    bits = {"nan": 0x7FC00000, "+inf": 0x7F800000, "-inf": -8388608, "nan_payload": 0x7F800001}[value]     # -8388608 = 0xFF800000
    host.view(np.int32)[i] = bits
    assert not np.isfinite(host[i])
    guard = _guard()
    assert _open(guard, Fenced(host, off=off)) == 0, _lib().last_error()
    assert guard.words().tolist() == [VETO_LOSS] + [0] * 7 and guard.fences_intact()


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_guard_open_status_words(n):
    words = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(n)]
    guard = _guard([VETO_STATUS] + [0] * 7)
    rows = Fenced(_finite_rows(5))
    assert _open(guard, rows, status=words) == 0, _lib().last_error()
    assert guard.words().tolist() == [0] * 8                                        # 0 to 4 words, all zero: no veto
    for value in (1, -1, -2 ** 31):                                                 # -2**31: only bit 31 set
        for pos in range(n):
            for w in words:
                w.zero_()
            words[pos].fill_(value)
            assert _open(guard, rows, status=words) == 0
            assert guard.words().tolist() == [VETO_STATUS] + [0] * 7, (value, pos)
    if n:
        bad = Fenced(np.array([1.0, np.nan], dtype=np.float32))
        assert _open(guard, bad, status=words) == 0 and guard.words()[0] == VETO_LOSS | VETO_STATUS
        for w in words:
            w.zero_()
        assert _open(guard, rows, status=words) == 0 and guard.words()[0] == 0
    assert guard.fences_intact()


def test_guard_open_status_list_limits():
    guard = _guard([VETO_NORM, 3, 0, 0, 0, 0, 0, 0])
    words = [torch.ones(1, dtype=torch.int32, device="cuda") for _ in range(5)]
    assert _open(guard, None, 0, status=words) == ERR_ARG                           # five status words: refused
    assert guard.words().tolist() == [VETO_NORM, 3, 0, 0, 0, 0, 0, 0]               # ... and nothing written
    assert _open(guard, None, 0, status=(), n_status=0) == 0                        # NULL list, n_status 0: accepted
    assert guard.words().tolist() == [0, 3, 0, 0, 0, 0, 0, 0]
    assert _open(guard, None, 0, status=(), n_status=2) == ERR_ARG                  # NULL list with words announced
    assert _open(guard, None, 0, status=words[:2], n_status=-1) == ERR_ARG
    assert guard.words().tolist() == [0, 3, 0, 0, 0, 0, 0, 0] and guard.fences_intact()


def test_guard_open_overwrites_word_0_and_nothing_else():
    guard = _guard([VETO_LOSS | VETO_NORM | VETO_STATUS, 11, 12, 13, 14, 15, 16, 17])
    rows = Fenced(_finite_rows(1025))
    assert _open(guard, rows) == 0, _lib().last_error()
    assert guard.words().tolist() == [0, 11, 12, 13, 14, 15, 16, 17] and guard.fences_intact()
    bad = Fenced(np.array([np.inf], dtype=np.float32))
    assert _open(guard, bad) == 0 and guard.words().tolist() == [VETO_LOSS, 11, 12, 13, 14, 15, 16, 17]
    assert _open(guard, rows) == 0 and guard.words().tolist() == [0, 11, 12, 13, 14, 15, 16, 17]        # a clean open clears it


# -- 7. a pre-set word vetoes Adam with a finite norm --------------------------------------------------------------------------
@pytest.mark.parametrize("count", [3, 40])
@pytest.mark.parametrize("bits", [VETO_LOSS, VETO_STATUS, VETO_LOSS | VETO_STATUS])
def test_preset_word_vetoes_adam_with_a_finite_norm(bits, count):
    case = AdamCase(count, seed=7)
    norm = _total_norm(case)
    d, guard = case.device(), _guard([bits, 0, 0, 0, 0, 0, 0, 0])
    before = _all_bits(d)
    assert case.run(d, 0.25 * norm, guard) == 0, _lib().last_error()
    _same_bits(before, _all_bits(d))
    _fences(d)
    out = d["out"].t.cpu().numpy()
    assert np.isfinite(out).all() and abs(out[0] - norm) <= 1e-4 * norm             # norm_out as the unguarded call writes it
    ref = case.device()
    assert case.run(ref, 0.25 * norm) == 0
    assert np.array_equal(ref["out"].bits(), d["out"].bits())
    assert guard.words().tolist() == [bits, 1, 1, int(bool(bits & VETO_LOSS)), 0, int(bool(bits & VETO_STATUS)), 0, 0]
    assert guard.fences_intact()


# -- 8. / 9. the guarded priority update ---------------------------------------------------------------------------------------
def _replay(T):
    from rltime_amd.history import PrioritizedReplayHistoryBuffer
    from tests.golden.streams import StreamSpec, vector_steps, as_reference_samples
    spec = StreamSpec(seed=5, num_envs=2, frame_shape=(1, 4, 4), done_prob=0.0)
    buf = PrioritizedReplayHistoryBuffer(size=64, train_frequency=4, nstep_target=1, nstep_train=T, prefix_steps=0, alpha=0.7,
                                         max_weight_factor=0.9, gamma=0.9)
    for st in vector_steps(spec, 24):
        buf.update(as_reference_samples(spec, st))
    return buf


def _replay_state(buf):
    from rltime_amd._lib import lib, check, np_ptr
    v, k, m = buf.tree_nodes()
    loss = np.zeros((2, 24), dtype=np.float32)
    for e in range(2):
        check(lib.mirl_replay_losses_peek(buf._h, e, 0, 24, np_ptr(loss[e])))
    return v.view(np.int64).copy(), k.copy(), m.view(np.int64).copy(), loss.view(np.int32).copy()


def _update(buf, idx, losses, guard=None):
    L = _lib()
    idx_d = torch.from_numpy(np.asarray(idx, dtype=np.int64)).cuda()
    los_d = torch.from_numpy(np.asarray(losses, dtype=np.float32)).cuda()
    if guard is None:
        rc = L.lib.mirl_replay_update_losses(buf._h, len(losses), _vp(idx_d), _vp(los_d), _stream())
    else:
        rc = L.lib.mirl_replay_update_losses_guarded(buf._h, len(losses), _vp(idx_d), _vp(los_d),
                                                     _vp(guard.t) if isinstance(guard, Fenced) else guard, _stream())
    torch.cuda.synchronize()
    return rc


def _same_state(a, b):
    for x, y, name in zip(a, b, ("tree values", "tree kinds", "tree min", "loss ring")):
        assert np.array_equal(x, y), name


@pytest.mark.parametrize("T", [4, 8])                     # 4: k_recalc_flagged, 8: k_recalc_flagged_wave
def test_guarded_priority_update(T):
    buf, twin = _replay(T), _replay(T)
    try:
        start = _replay_state(buf)
        _same_state(start, _replay_state(twin))
        idx1 = [[0, 4], [0, 5], [1, 8], [1, 17], [0, 11], [-1, -1], [1, 9]]
        los1 = [0.5, np.nan, 2.0, np.inf, -np.inf, 9.0, 0.3]                         # values in a buffer, nothing more
        # with the word set: losses and tree (values, kinds, min) stay as they were
        guard = _guard([VETO_NORM, 5, 0, 0, 0, 0, 0, 0])
        assert _update(buf, idx1, los1, guard) == 0, _lib().last_error()
        _same_state(start, _replay_state(buf))
        assert guard.words().tolist() == [VETO_NORM, 5, 0, 0, 0, 0, 0, 0] and guard.fences_intact()     # the guard is only read
        # a vetoed call followed by a clean one with duplicated rows = the twin that only saw the clean one, unguarded:
        # the last writer wins, and the epoch the vetoed call spent without stamping does no harm
        idx2 = [[0, 4], [0, 5], [0, 4], [1, 8], [0, 5], [0, 4], [-1, -1], [1, 9], [1, 16], [0, 13]]
        los2 = [0.5, -0.25, 2.0, 0.1, 3.5, -0.75, 9.0, 0.3, 1.25, 0.0]
        clear = _guard()
        assert _update(buf, idx2, los2, clear) == 0
        assert _update(twin, idx2, los2) == 0
        after = _replay_state(buf)
        _same_state(after, _replay_state(twin))
        assert not np.array_equal(after[0], start[0]) and not np.array_equal(after[3], start[3])     # the clean call did write
        # with the word clear: the unguarded call
        idx3 = [[1, 3], [0, 7], [1, 3], [0, 20]]
        los3 = [0.75, 1.5, 0.125, 4.0]
        assert _update(buf, idx3, los3, clear) == 0 and _update(twin, idx3, los3) == 0
        _same_state(_replay_state(buf), _replay_state(twin))
        assert clear.words().tolist() == [0] * 8 and clear.fences_intact()
        # refusals write nothing
        assert _update(buf, idx3, [9.0] * 4, C.c_void_p(None)) == ERR_ARG
        assert _update(buf, idx3, [9.0] * 4, C.c_void_p(clear.t.data_ptr() + 4)) == ERR_ARG
        _same_state(_replay_state(buf), _replay_state(twin))
    finally:
        buf.close(), twin.close()


# -- 10. the sweeps' status word -----------------------------------------------------------------------------------------------
def test_lstm_seq_status_device_word():
    L = _lib()
    a, b = C.c_void_p(), C.c_void_p()
    assert L.lib.mirl_lstm_seq_status_device(C.byref(a)) == 0, L.last_error()
    assert L.lib.mirl_lstm_seq_status_device(C.byref(b)) == 0
    assert a.value and a.value == b.value
    assert L.lib.mirl_lstm_seq_status_device(None) == ERR_ARG
    host = C.c_int32(-1)
    assert L.lib.mirl_lstm_seq_status(C.byref(host)) == 0 and host.value == 0

    class Word:
        def data_ptr(self):
            return a.value
    guard = _guard([VETO_STATUS] + [0] * 7)
    assert _open(guard, None, 0, status=[Word()]) == 0, L.last_error()
    assert guard.words().tolist() == [0] * 8 and guard.fences_intact()


# -- 11. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    guard = _guard([VETO_LOSS, 1, 2, 3, 4, 5, 0, 0])
    rows = Fenced(np.array([np.nan] * 8, dtype=np.float32))
    off_guard = C.c_void_p(guard.t.data_ptr() + 4)
    assert _open(C.c_void_p(None), rows) == ERR_ARG                                   # NULL guard
    assert _open(off_guard, rows, count=2) == ERR_ARG                                 # misaligned guard
    assert _open(guard, rows, count=-1) == ERR_ARG                                    # negative count
    assert _open(guard, None, count=3) == ERR_ARG                                     # NULL rows with count > 0
    case = AdamCase(3, seed=1)
    d = case.device()
    before = _all_bits(d)
    assert case.run(d, 1.0, C.c_void_p(None)) == ERR_ARG
    assert case.run(d, 1.0, off_guard) == ERR_ARG
    _same_bits(before, _all_bits(d))
    assert d["out"].words().view(np.float32).tolist() == [7.0, 7.0]
    assert guard.words().tolist() == [VETO_LOSS, 1, 2, 3, 4, 5, 0, 0] and guard.fences_intact()


# =============================================================================================================================
# the trainer: TorchTrainer._train(skip_invalid_steps=True)
# =============================================================================================================================
def _config(kind, graphed, guard, total_steps):
    cfg = copy.deepcopy(BASE)
    cfg["model"] = {"type": "sequential", "args": {"layer_configs": [CNN, {"type": "fc", "args": {"fc_size": 64}}]}}
    common = {"clip_rewards": True, "gamma": 0.99, "mbatch_size": 32, "nstep_train": 1, "nstep_target": 3, "lr": 1e-3, "lr_anneal": True,
              "double_q": True, "clip_grad": 10.0, "target_update_freq": 24, "total_steps": total_steps, "log_freq": 10 ** 9,
              "warmup_steps": 96, "graph_learner_step": graphed}
    if guard is not None:
        common["skip_invalid_steps"] = guard
    if kind == "iqn_lstm":
        cfg["model"]["args"]["layer_configs"] = [CNN, {"type": "lstm", "args": {"num_units": 128}}, {"type": "fc", "args": {"fc_size": 64}}]
        cfg["acting"]["actor_envs"] = 16
        cfg["policy_args"] = {"dueling": True, "embedding_dim": 16, "num_sampling_quantiles": 8}
        cfg["training"] = {"type": "iqn", "args": dict(
            common, mbatch_size=16, nstep_train=8, burn_in_timesteps=4, nstep_target=2, rnn_bootstrap=True, vf_scale_epsilon=1e-3,
            clip_rewards=False, warmup_steps=480,
            history_mode={"type": "prioritized_replay", "args": {
                "size": 1600, "train_frequency": 4, "alpha": 0.9, "beta": 0.6, "max_weight_factor": 0.9, "device_rng": True}})}
    else:
        cfg["policy_args"] = {"dueling": True}
        cfg["training"] = {"type": "dqn", "args": dict(common, history_mode={"type": "prioritized_replay", "args": {
            "size": 400, "train_frequency": 8, "alpha": 0.6, "beta": 0.4, "beta_anneal": True, "device_rng": True}})}
    return cfg


# acted steps: the warm-up, then 16 / 14 learner steps (one per mbatch_size x nstep_train / train_frequency acted steps)
TOTAL = {"dqn": 96 + 4 * 16, "iqn_lstm": 480 + 32 * 14}


def _snapshot(tr):
    """Everything a vetoed step must leave alone, as bit patterns on the host (synchronises)."""
    ps = list(tr.policy.parameters())
    st = tr.optimizer.state
    bits = lambda t: t.detach().reshape(-1).view(torch.int32).cpu().numpy().copy()              # noqa: E731
    out = {"params": [bits(p) for p in ps],
           "exp_avg": [bits(st[p]["exp_avg"]) for p in ps if p in st and "exp_avg" in st[p]],
           "exp_avg_sq": [bits(st[p]["exp_avg_sq"]) for p in ps if p in st and "exp_avg_sq" in st[p]],
           "step": [bits(st[p]["step"].float()) for p in ps if p in st and "step" in st[p]]}
    v, k, m = tr.history_buffer.tree_nodes()
    out["tree"] = [v.view(np.int64).copy(), k.copy(), m.view(np.int64).copy()]
    return out


def _same_snapshot(a, b, keys=("params", "exp_avg", "exp_avg_sq", "step", "tree")):
    for key in keys:
        assert len(a[key]) == len(b[key]) and len(a[key]) > 0, key
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            assert np.array_equal(x, y), "%s[%d]" % (key, i)


def _run(kind, graphed, guard, poison_step=None, status_step=None, untrained_step=None, setup_hook=None):
    """THE LOOP at a small shape.  poison_step j: a wrapper around _compute_grads multiplies one gradient entry by a device
    flag that is 1.0 on every step (x * 1.0 is exact) and NaN on learner step j — a tensor, so a captured step carries it;
    status_step j: a status word of the test's own, appended to _guard_status, reads 1 during step j; untrained_step j: step
    j's batch is sampled like every other and then simply not trained (the yardstick a vetoed step is compared with)."""
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.general.type_registry import get_registered_type
    from rltime_amd.train import create_actors
    cfg = _config(kind, graphed, guard, TOTAL[kind])
    torch.manual_seed(11)
    np.random.seed(11)
    random.seed(11)
    actors = create_actors(cfg, torch.device("cuda", 0), device_acting=True, use_graph=True)
    logger = NullLogger()
    tr = get_registered_type("trainers", cfg["training"]["type"])(logger=logger, actors=actors, model_config=cfg["model"],
                                                                 policy_args=cfg.get("policy_args", {}))
    tr.data_parallel = None
    series = {"qloss": [], "grad_norm": []}
    orig_log = tr.value_log.log

    def tap(key, value, *a, **k):
        if key in series and k.get("group") == "train":
            series[key].append(value.detach().clone() if isinstance(value, torch.Tensor) else torch.tensor(float(value)))
        return orig_log(key, value, *a, **k)
    tr.value_log.log = tap
    out = {"around": None}
    try:
        tr.setup(**cfg["training"]["args"])
        if setup_hook is not None:
            setup_hook(tr)
        flag = torch.ones(1, device="cuda")
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        if status_step is not None:
            tr._guard_status.append(word)
        if poison_step is not None:
            compute = tr._compute_grads

            def poisoned(*a, **k):
                r = compute(*a, **k)
                g = next(p for p in tr.policy.parameters() if p.grad is not None and p.dim() == 1).grad
                g[3:4].mul_(flag)
                return r
            tr._compute_grads = poisoned
        learner_step = tr.learner_step
        k_step = [0]

        def stepped(train_data, nstep_train, *a, **k):
            j = k_step[0]
            k_step[0] += 1
            marked = j in (poison_step, status_step)
            if j == untrained_step:
                # the batch was sampled and gathered; what the step would have consumed on the host is consumed
                rows = train_data["returns"].shape[0] - tr.burn_in_timesteps
                batch = rows * train_data["returns"].shape[1]
                tr.get_train_indexes(batch, batch, nstep_train)
                tr._update_steps_trained(batch)
                tr.ts_learner_steps += 1
                return None
            if marked:
                flag.fill_(float("nan")) if j == poison_step else word.fill_(1)
                before = _snapshot(tr)
            r = learner_step(train_data, nstep_train, *a, **k)
            if marked:
                out["around"] = (before, _snapshot(tr))
                flag.fill_(1.0), word.zero_()
            return r
        tr.learner_step = stepped
        while not tr.train_is_done():
            tr.loop_iteration()
        torch.cuda.synchronize()
        out["steps"] = k_step[0]
        assert out["steps"] > J + 3, out["steps"]
        out.update({k: torch.stack([t.float().cpu() for t in v]).numpy().view(np.int32) for k, v in series.items()})
        out["final"] = _snapshot(tr)
        out["captured"] = tr._gstep is not None and tr._gstep["graph"] is not None
        out["counters"] = tr._step_guard_counters()
        if guard:
            tr._log_checkpoint()
            out["log_row"] = logger.rows[-1][2]["train"]
    finally:
        if getattr(tr, "history_buffer", None) is not None:
            tr.history_buffer.close()
        actors.close()
    return out


def _same_run(a, b):
    assert a["steps"] == b["steps"] > 8
    for key in ("qloss", "grad_norm"):
        assert len(a[key]) == a["steps"]
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    _same_snapshot(a["final"], b["final"])


# -- 12. guard on, no veto = guard off -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("kind", ["dqn", "iqn_lstm"])
def test_guard_on_without_a_veto_is_the_run_without_it(deterministic_library, kind, graphed):
    on, off = _run(kind, graphed, True), _run(kind, graphed, None)
    assert on["captured"] == off["captured"] == bool(graphed)
    _same_run(on, off)
    assert off["counters"] is None
    c = on["counters"]
    assert c["skipped_steps"] == c["skipped_loss"] == c["skipped_norm"] == c["skipped_status"] == 0 and c["closed"] == on["steps"]
    assert [on["log_row"][k] for k in ("skipped_steps", "skipped_loss", "skipped_norm", "skipped_status")] == [0, 0, 0, 0]
    assert np.isfinite(on["qloss"].view(np.float32)).all()


# -- 13. one poisoned step is dropped, the run continues -----------------------------------------------------------------------
J = 6          # a replayed step in the graphed runs (three eager steps, the fourth is captured)


def _dropped(run, cause):
    before, after = run["around"]
    _same_snapshot(before, after)                                     # weights, moments, step counters, tree: as before step J
    c = run["counters"]
    want = {"skipped_steps": 1, "skipped_loss": 0, "skipped_norm": 0, "skipped_status": 0, "closed": run["steps"]}
    want[cause] = 1
    assert c == want
    assert run["log_row"][cause] == 1 and run["log_row"]["skipped_steps"] == 1
    for key in ("qloss", "grad_norm"):
        vals = run[key].view(np.float32)
        rest = np.delete(vals, J) if key == "grad_norm" and cause == "skipped_norm" else vals
        assert np.isfinite(rest).all(), key                           # the later steps are finite ...
    if cause == "skipped_norm":
        assert not np.isfinite(run["grad_norm"].view(np.float32)[J])   # ... and step J's norm was logged as it was
    assert any(not np.array_equal(x, y) for x, y in zip(after["params"], run["final"]["params"]))       # the run went on
    steps = [float(s.view(np.float32)[0]) for s in run["final"]["step"]]
    assert steps == [run["steps"] - 1.0] * len(steps)                 # every Adam counter missed exactly the dropped step


def test_poisoned_step_is_dropped_dqn_eager(deterministic_library):
    """... and the trajectory after it is that of a run in which step J's batch was never trained: checkable here, because
    nothing of a DQN step but the weights, the Adam state and the tree feeds the next one, and the replay's Philox draws are
    keyed by the call count."""
    got = _run("dqn", "no-capture", True, poison_step=J)
    _dropped(got, "skipped_norm")
    want = _run("dqn", "no-capture", None, untrained_step=J)
    assert got["steps"] == want["steps"]
    for key in ("qloss", "grad_norm"):
        np.testing.assert_array_equal(np.delete(got[key], J), want[key], err_msg=key)
    _same_snapshot(got["final"], want["final"])


def test_poisoned_step_is_dropped_plain_eager_trainer(deterministic_library):
    """graph_learner_step=False: the learning rate on the host, no static batches — train_batch's own deferred flush."""
    got = _run("dqn", False, True, poison_step=J)
    assert not got["captured"]
    _dropped(got, "skipped_norm")


def test_poisoned_step_is_dropped_dqn_graphed(deterministic_library):
    """The same poisoning through the captured step (the flag is a device tensor the capture carries): the replayed, vetoed
    step leaves everything alone, and the whole run is the eager poisoned run bit for bit."""
    got = _run("dqn", True, True, poison_step=J)
    assert got["captured"]
    _dropped(got, "skipped_norm")
    eager = _run("dqn", "no-capture", True, poison_step=J)
    _same_run(got, eager)


@pytest.mark.parametrize("graphed", ["no-capture", True])
def test_poisoned_step_is_dropped_recurrent(deterministic_library, graphed):
    """Recurrent IQN + sequence priorities.  The quantile fractions of the dropped step are drawn all the same, so a run
    without step J is not the yardstick here: the state around step J is exact, the rest is finite and the counters advance."""
    got = _run("iqn_lstm", graphed, True, poison_step=J)
    assert got["captured"] == (graphed is True)
    _dropped(got, "skipped_norm")


# -- 14. a sweep failure vetoes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphed", [False, True])
def test_status_word_vetoes_the_step(deterministic_library, graphed):
    got = _run("dqn", graphed, True, status_step=J)
    assert got["captured"] == bool(graphed)
    _dropped(got, "skipped_status")


# -- 15. refusals --------------------------------------------------------------------------------------------------------------
def test_dynamic_clip_is_refused(deterministic_library):
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.general.type_registry import get_registered_type
    from rltime_amd.train import create_actors
    cfg = _config("dqn", False, True, TOTAL["dqn"])
    cfg["training"]["args"]["clip_grad_dynamic_alpha"] = 0.99
    actors = create_actors(cfg, torch.device("cuda", 0), device_acting=True, use_graph=True)
    tr = get_registered_type("trainers", "dqn")(logger=NullLogger(), actors=actors, model_config=cfg["model"],
                                                policy_args=cfg["policy_args"])
    try:
        with pytest.raises(ValueError, match="clip_grad_dynamic_alpha"):
            tr.setup(**cfg["training"]["args"])
    finally:
        actors.close()


def test_a_step_that_would_fall_back_to_torch_adam_is_refused(deterministic_library):
    """Never a silent unguarded step: the error carries why_not_fused()'s text, and nothing was applied."""
    seen = {}

    def hook(tr):
        tr.optimizer.why_not_fused = lambda: "a reason only this test gives"
        seen["before"] = [p.detach().clone() for p in tr.policy.parameters()]
        seen["tr"] = tr
    with pytest.raises(ValueError, match="a reason only this test gives"):
        _run("dqn", False, True, setup_hook=hook)
    assert all(torch.equal(p, q) for p, q in zip(seen["tr"].policy.parameters(), seen["before"]))
