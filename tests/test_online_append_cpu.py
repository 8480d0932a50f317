"""CPU: the host side of acting on the fused step for A2C / PPO.

  * the three new entry points (mirl_actor_head_ac_rng, mirl_online_append, mirl_online_advance) refuse bad arguments with
    MIRL_ERR_ARG before anything touches a device (host logic, as in tests/test_abi.py);
  * tests/online_append_restate.py's slot rule against OnlinePlan: whatever route a vector step takes, get_train_data reads it
    from slot `step mod capacity`, across a reallocation of the rings;
  * DeviceOnlineHistory.needed_feed_count's closed form for a fused actor against feeding one step at a time;
  * the two opt-in configs differ from their parents in the opt-in alone."""
import copy
import ctypes as C

import numpy as np
import pytest

from rltime_amd import _lib
from rltime_amd.history.online_device import DeviceOnlineHistory, OnlinePlan
from tests import online_append_restate as AR

FAKE = C.c_void_p(4096)              # a non-null address: every call below is refused before any launch


# ---- argument refusals -----------------------------------------------------------------------------------------------------------
def _head_args(**over):
    a = dict(E=5, A=3, logits=FAKE, pitch=4, values=FAKE, value_pitch=4, seed=7, step=FAKE, greedy=0, actions=FAKE, logp=FAKE,
             values_out=FAKE, out_pitch=2)
    a.update(over)
    return tuple(a.values()) + (None,)


@pytest.mark.parametrize("over", [dict(logits=None), dict(values=None), dict(step=None), dict(actions=None), dict(logp=None),
                                  dict(values_out=None), dict(A=0), dict(A=65, pitch=65), dict(pitch=2), dict(value_pitch=0),
                                  dict(E=0), dict(greedy=2), dict(out_pitch=0)],
                         ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_head_rng_refuses(over):
    assert _lib.lib.mirl_actor_head_ac_rng(*_head_args(**over)) == _lib.MIRL_ERR_ARG
    assert "actor_head_ac_rng" in _lib.last_error()


def _append_args(**over):
    a = dict(E=3, cap=5, head=FAKE, k=0, obs_bytes=37, obs=FAKE, actions=FAKE, rewards=FAKE, dones=FAKE, policy=FAKE, policy_pitch=2,
             S=0, state=None, initials=None, obs_ring=FAKE, actions_ring=FAKE, rewards_ring=FAKE, dones_ring=FAKE, policy_ring=FAKE,
             state_ring=None, initials_ring=None)
    a.update(over)
    return tuple(a.values()) + (None,)


_REC = dict(S=22, state=FAKE, initials=FAKE, state_ring=FAKE, initials_ring=FAKE)


@pytest.mark.parametrize("over", [dict(head=None), dict(obs=None), dict(actions=None), dict(rewards=None), dict(dones=None),
                                  dict(policy=None), dict(obs_ring=None), dict(actions_ring=None), dict(rewards_ring=None),
                                  dict(dones_ring=None), dict(policy_ring=None), dict(cap=0), dict(cap=-1), dict(k=-1), dict(E=0),
                                  dict(obs_bytes=0), dict(policy_pitch=1), dict(S=-1),
                                  dict(_REC, state=None), dict(_REC, initials=None), dict(_REC, state_ring=None),
                                  dict(_REC, initials_ring=None), dict(_REC, state=C.c_void_p(4098))],
                         ids=lambda o: ",".join("%s=%s" % (k, getattr(v, "value", v)) for k, v in o.items()))
def test_append_refuses(over):
    assert _lib.lib.mirl_online_append(*_append_args(**over)) == _lib.MIRL_ERR_ARG
    assert "online_append" in _lib.last_error()


def test_advance_refuses():
    assert _lib.lib.mirl_online_advance(None, 1, None) == _lib.MIRL_ERR_ARG
    assert _lib.lib.mirl_online_advance(FAKE, -1, None) == _lib.MIRL_ERR_ARG
    assert "online_advance" in _lib.last_error()


# ---- the slot rule against OnlinePlan --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["per_step", "planned"])
def test_every_live_step_sits_in_its_slot(route):
    """11 vector steps through capacities 5 -> 10 (nstep_train 4, max_delayed_steps 9, nothing served): after every feed,
    each step a pending transition or its first state can still need is in slot `step mod capacity`, and a sequence served
    from the plan names exactly that slot."""
    E, T, D, obs_bytes, S = 2, 4, 9, 5, 3
    plan, cap, rings, caps = OnlinePlan(T, D), 0, None, []
    fed = 0
    while fed < 11:
        iters = 1 if route == "per_step" else min(3, 11 - fed)
        before = plan.head
        for _ in range(iters):
            plan.feed(range(E))
        if plan.live_steps() > cap:
            new = DeviceOnlineHistory._next_capacity(plan.live_steps(), cap, T, D)
            rings = AR.new_rings(new, E, obs_bytes, S, canary=True) if rings is None else AR.regrow(rings, new, before)
            cap = new
            caps.append(cap)
        for k in range(iters):
            assert AR.append(rings, before, k, AR.step_case(3, before + k, E, obs_bytes, S)) == (before + k) % cap
        fed += iters
        for s in range(max(0, plan.head - plan.live_steps()), plan.head):
            want = AR.step_case(3, s, E, obs_bytes, S)
            for name in AR.RINGS:
                assert np.array_equal(rings[name][s % cap], want[name]), (name, s, cap)
    assert caps == [5, 10] and plan.head == 11 and plan.pending == {0: 9, 1: 9}
    served = plan.serve(2)
    assert [(env, start % cap) for env, start, _ in served] == [(0, 2), (1, 2)]     # step 2 = 11 - 9, still in slot 2 of 10


# ---- needed_feed_count for a fused actor -----------------------------------------------------------------------------------------
def _history(plan, E):
    h = DeviceOnlineHistory.__new__(DeviceOnlineHistory)       # (the constructor needs a GPU; the count is host arithmetic)
    h.plan, h.num_envs, h.env_base, h._fused = plan, E, 0, True
    return h


def _brute(plan, mbatch, E, limit=200):
    plan = copy.deepcopy(plan)
    for n in range(limit + 1):
        if plan.sequences_ready() >= mbatch:
            return n
        plan.feed(range(E))
    return None


@pytest.mark.parametrize("D", [5000, 7, 5])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("T", [1, 4, 5])
def test_needed_feed_count_is_the_fewest_whole_steps(T, E, D):
    for mbatch in sorted({1, E, 2 * E}):
        for uneven in (0, 1, 3):
            plan = OnlinePlan(T, D)
            for _ in range(uneven):                    # env 0 alone is ahead of the others (and of a multiple of T)
                plan.feed([0])
            steps = 0
            while steps < 40:
                h = _history(plan, E)
                want = _brute(plan, mbatch, E)
                got = h.needed_feed_count(mbatch, E)
                if want == 0:
                    assert got is None
                    assert plan.serve(mbatch) is not None
                    continue
                if want is None:                       # max_delayed_steps discards before a batch forms: one step, as before
                    assert got == E and plan.steps_until_ready(mbatch, range(E)) is None
                    break
                assert got == E * want, (T, E, D, mbatch, uneven, plan.pending, got, want)
                for _ in range(want):
                    plan.feed(range(E))
                steps += want
                assert plan.sequences_ready() >= mbatch


def test_needed_feed_count_without_a_fused_actor_is_one_step():
    plan = OnlinePlan(8, 5000)
    h = _history(plan, 4)
    h._fused = False
    assert h.needed_feed_count(4, 4) == 4
    h._fused = True
    assert h.needed_feed_count(4, 4) == 32


# ---- configs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["catch_ppo", "catch_ppo_lstm"])
def test_fused_config_is_its_parent_plus_the_opt_in(name):
    from rltime_amd.general.config import load_config, validate_config
    fused, parent = load_config(name + "_fused.json"), load_config(name + ".json")
    validate_config(fused)
    assert fused["acting"]["extra_args"] == {"fused_step": True}
    assert "extra_args" not in parent["acting"]
    del fused["acting"]["extra_args"]
    assert fused == parent


def test_create_actors_reads_the_opt_in():
    import inspect
    from rltime_amd.acting.actor import Actor
    p = inspect.signature(Actor.__init__).parameters
    assert list(p)[-1] == "fused_actor_critic" and p["fused_actor_critic"].default is False
