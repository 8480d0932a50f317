"""GPU: the two kernels acting on the fused step adds to csrc/actor_critic.hip, and DeviceOnlineHistory as their sink.

  1. mirl_actor_head_ac_rng against mirl_actor_head_ac fed the uniforms of tests/pointwise_restate.philox_head_draws at the same
     (seed, step): actions, log-probabilities and values bit for bit — one body behind both entries.
  2. mirl_online_append against tests/online_append_restate.py: the seven rings bit for bit, every other slot still its canary;
     mirl_online_advance adds exactly `steps`.
  3. a history fed through update_batch / plan_ingest + ingest_planned against one handed the same vector steps as
     DeviceSamples: every leaf of every batch torch.equal, the served order, the discards and the head word."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import actor_critic_restate as R
from tests import online_append_restate as AR
from tests import online_lstm_restate as LR
from tests import pointwise_restate as PR

pytestmark = pytest.mark.gpu

NAN = float("nan")
SEED = 0x5EED0000AC7


def _lib():
    from rltime_amd import _lib
    return _lib


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the head -------------------------------------------------------------------------------------------------------------------
def _both_heads(logits, values, step, greedy, pad):
    """pad = 1: the value is the last column of the [E][A + 1] block; pad = 4: a padded pitch, the value still at column A."""
    L = _lib()
    E, A = logits.shape
    pitch = A + pad
    z = torch.full((E, pitch), NAN, device="cuda")
    z[:, :A] = _dev(logits)
    z[:, A] = _dev(values)
    u = PR.philox_head_draws(SEED, step, E, A)[0].cuda()
    vd = _dev(values)
    word = torch.tensor([step], dtype=torch.int64, device="cuda")
    out = []
    for rng in (False, True):
        acts = torch.full((E + 1,), -7, dtype=torch.int32, device="cuda")
        block = torch.full((E + 1, 2), NAN, device="cuda")
        if rng:
            L.check(L.lib.mirl_actor_head_ac_rng(E, A, _p(z), pitch, _p(z, 4 * A), pitch, SEED, _p(word), int(greedy), _p(acts), _p(block),
                                                 _p(block, 4), 2, _st()), "mirl_actor_head_ac_rng")
        else:
            L.check(L.lib.mirl_actor_head_ac(E, A, _p(z), pitch, _p(vd), _p(u), int(greedy), _p(acts), _p(block), _p(block, 4), 2, _st()),
                    "mirl_actor_head_ac")
        torch.cuda.synchronize()
        assert int(acts[E]) == -7 and bool(torch.isnan(block[E]).all()), "the guard row was written"
        out.append((acts[:E].clone(), block[:E].clone()))
    assert int(word) == step                                     # the head reads the step word, the pre-step kernel moves it
    return out


@pytest.mark.parametrize("A", [1, 2, 3, 64])
@pytest.mark.parametrize("E", [1, 5, 67])
def test_head_with_its_own_draw_equals_the_head_given_the_draw(E, A):
    logits, values, _ = R.head_case(E, A)
    seen = set()
    for step in (0, 1, 2 ** 32 + 7):
        for pad in (1, 4):
            for greedy in (0, 1):
                (a0, b0), (a1, b1) = _both_heads(logits, values, step, greedy, pad)
                assert torch.equal(a0, a1), (step, pad, greedy)
                assert torch.equal(b0.view(torch.int32), b1.view(torch.int32)), (step, pad, greedy)      # bits, not values
                assert np.array_equal(b1[:, 1].cpu().numpy(), values)
                if not greedy:
                    seen.add(tuple(a1.tolist()))
    # the three steps draw different uniforms (the high word of the counter included): with 5 envs or more the actions differ
    assert A == 1 or E < 5 or len(seen) >= 2


@pytest.mark.parametrize("E,A", [(5, 2), (67, 3), (67, 64)])
def test_head_with_its_own_draw_takes_the_first_maximum(E, A):
    logits, values, first = R.head_tie_case(E, A)
    (a0, b0), (a1, b1) = _both_heads(logits, values, 3, 1, 1)
    assert np.array_equal(a1.cpu().numpy().astype(np.int64), first)
    assert torch.equal(a0, a1) and torch.equal(b0.view(torch.int32), b1.view(torch.int32))


# ---- 2. the append -------------------------------------------------------------------------------------------------------------------
def _append(rings, head, k, step, E, cap, obs_bytes, S):
    L = _lib()
    word = torch.tensor([head], dtype=torch.int64, device="cuda")
    d = {name: _dev(v) for name, v in step.items()}
    L.check(L.lib.mirl_online_append(E, cap, _p(word), k, obs_bytes, _p(d["obs"]), _p(d["actions"]), _p(d["rewards"]), _p(d["dones"]),
                                     _p(d["policy"]), 2, S, _p(d.get("state")), _p(d.get("initials")), _p(rings["obs"]),
                                     _p(rings["actions"]), _p(rings["rewards"]), _p(rings["dones"]), _p(rings["policy"]),
                                     _p(rings["state"]) if S else None, _p(rings["initials"]) if S else None, _st()),
            "mirl_online_append")
    torch.cuda.synchronize()
    assert int(word) == head                                     # the append reads the word; only the advance moves it


@pytest.mark.parametrize("S", [0, 22, 24], ids=["S0", "S22-words", "S24-vec16"])
@pytest.mark.parametrize("obs_bytes", [7056, 37], ids=["vec16", "bytes"])
@pytest.mark.parametrize("E", [1, 3])
def test_append_writes_its_slot_and_nothing_else(E, obs_bytes, S):
    cap = 5
    for head in (cap - 1, cap, 2 ** 31 + 3):
        for k in (0, 2):
            want = AR.new_rings(cap, E, obs_bytes, S, canary=True)
            rings = {name: _dev(v) for name, v in want.items()}
            step = AR.step_case(11, head + k, E, obs_bytes, S)
            _append(rings, head, k, step, E, cap, obs_bytes, S)
            slot = AR.append(want, head, k, step)
            assert slot == (head + k) % cap
            for name in AR.RINGS:
                got = rings[name].cpu().numpy()
                assert np.array_equal(got.view(np.uint8), want[name].view(np.uint8)), (name, head, k)


def test_advance_adds_exactly_its_steps():
    L = _lib()
    word = torch.tensor([2 ** 31 - 2, -5], dtype=torch.int64, device="cuda")
    for steps, want in ((5, 2 ** 31 + 3), (0, 2 ** 31 + 3), (64, 2 ** 31 + 67)):
        L.check(L.lib.mirl_online_advance(_p(word), steps, _st()), "mirl_online_advance")
        assert word.tolist() == [want, -5]


# ---- 3. the sink against the hand-over ------------------------------------------------------------------------------------------------
def _gae():
    def discount(nstep, reward, policy_output):
        raise AssertionError("the device history evaluates the return itself")
    discount.gamma, discount.lam = 0.99, 0.95
    return discount


def _tree(step, rec, e=None, wrap=lambda a: a):
    if rec:
        return LR.rec_state_tree(step, e, wrap)
    pick = wrap if e is None else (lambda a: a[e])
    return {"x": pick(step["obs"]), "layer0_state": {}, "layer1_state": {}}


def _samples(steps, E, rec):
    from rltime_amd.acting.acting_interface import DeviceSamples
    from rltime_amd.acting.actor import _pack_state
    out = DeviceSamples(_tree(steps[0], rec, 0), E, 0)
    for s in steps:
        fields = _pack_state(_tree(s, rec, wrap=lambda a: torch.from_numpy(a).cuda()))
        out.append(actions=torch.from_numpy(s["actions"]).cuda(), policy=torch.from_numpy(np.stack([s["logp"], s["values"]], axis=1)).cuda(),
                   rewards=torch.from_numpy(s["rewards"]).cuda(), dones=torch.from_numpy(s["dones"]).cuda(), **fields)
    return out


class _Ingested:
    ingested = True


def _leaves(tree, path=""):
    if isinstance(tree, dict):
        for k, v in tree.items():
            yield from _leaves(v, path + "." + k)
    else:
        yield path, tree


@pytest.mark.parametrize("rec", [False, True], ids=["plain", "recurrent"])
def test_sink_routes_equal_the_hand_over(rec):
    """E = 3, T = 4, max_delayed_steps = 6: the rings grow 5 -> 7 and wrap more than twice in 24 steps; the groups of 5 and 6
    steps without a draw in between discard.  Route by group: update_batch, planned, DeviceSamples."""
    from rltime_amd.history.online_device import DeviceOnlineHistory
    E, T = 3, 4
    kw = dict(max_delayed_steps=6, fixed_target=True, nstep_target=4, nstep_train=T)
    a, b = DeviceOnlineHistory(discount_function=_gae(), **kw), DeviceOnlineHistory(discount_function=_gae(), **kw)
    steps = [LR.rec_step(23, t, E, "u8") for t in range(24)]
    b.configure(_tree(steps[0], rec, 0), E, 0, policy_f32=2)
    assert b._h is not None and b.supports_planned_ingest() and b._keep_policy and b._policy_f32 == 2
    groups = [("batch", 2), ("planned", 3), ("samples", 2), ("planned", 5), ("batch", 2), ("samples", 1), ("planned", 6), ("batch", 3)]
    at, batches, lost, handles = 0, 0, 0, set()
    for route, n in groups:
        chunk = steps[at:at + n]
        at += n
        want_lost = a.update(_samples(chunk, E, rec))["discarded_steps"]
        packed = _samples(chunk, E, rec).vector_steps
        payload = [dict(frames=s["frames"], actions=s["actions"], rewards=s["rewards"], dones=s["dones"], policy=s["policy"],
                        state=s.get("state"), initials=s.get("initials")) for s in packed]
        if route == "samples":
            got_lost = b.update(_samples(chunk, E, rec))["discarded_steps"]
        else:
            if route == "batch":
                for pl in payload:
                    b.update_batch(pl.pop("frames"), pl.pop("actions"), pl.pop("rewards"), pl.pop("dones"), transient=True, **pl)
            else:
                b.plan_ingest(n, E)
                for k, pl in enumerate(payload):
                    b.ingest_planned(k, pl.pop("frames"), pl.pop("actions"), pl.pop("rewards"), pl.pop("dones"), **pl)
                b.finish_planned(n)
            got_lost = b.update(_Ingested())["discarded_steps"]
        handles.add(b._h.value)
        assert got_lost == want_lost, (route, n)
        lost += got_lost
        assert int(b._head_word) == b.plan.head == a.plan.head == at
        assert b.capacity == a.capacity
        for B in (2, 3, 1):
            x, y = a.get_train_data(B), b.get_train_data(B)
            assert (x is None) == (y is None)
            if x is None:
                continue
            batches += 1
            assert a._served == b._served
            lx, ly = dict(_leaves(x)), dict(_leaves(y))
            assert set(lx) == set(ly)
            for key in lx:
                assert torch.equal(lx[key], ly[key]), (route, n, B, key)
    assert batches >= 6 and lost > 0 and a.capacity == 7 and at == 24 > 3 * a.capacity
    assert len(handles) == 2                                     # one handle per allocation of the rings: 5 slots, then 7
    a.close()
    b.close()


def test_sink_refuses_what_it_does_not_cover():
    from rltime_amd.history.online_device import DeviceOnlineHistory
    h = DeviceOnlineHistory(nstep_target=2, nstep_train=2, discount_function=_gae())
    x = np.zeros((2, 4, 4), np.uint8)
    with pytest.raises(ValueError, match="policy_f32"):
        h.configure({"x": x, "layer0_state": {}}, 2, 0, policy_f32=3)
    with pytest.raises(ValueError, match="extra-feature"):
        h.configure({"x": (x, np.zeros(3, np.float32)), "layer0_state": {}}, 2, 0, policy_f32=2)
    assert h._h is None and not h.supports_planned_ingest()
    h.configure({"x": x, "layer0_state": {}}, 2, 0, policy_f32=2)
    z = torch.zeros(2, device="cuda")
    with pytest.raises(ValueError, match="extra-feature"):
        h.update_batch(torch.zeros((2, 2, 4, 4), dtype=torch.uint8, device="cuda"), z.int(), z, z.to(torch.uint8),
                       extra=torch.zeros((2, 3), device="cuda"), policy=torch.zeros((2, 2), device="cuda"))
    assert h.plan.head == 0
    h.close()
