"""GPU: the on-policy window with a recurrent state (csrc/actor_critic.hip k_online_window through mirl_online_window_rec)
against the NumPy restatement of tests/online_lstm_restate.py (actor_critic_restate.window extended by the state and initials
blocks).  The state and initials outputs are copies: bit-exact.  Everything the two older entries write is checked as there
(returns within window_bound, the rest exact), and mirl_online_window on the same rings still gives those outputs byte for
byte.  Output buffers are NaN-filled with one guard row that must stay untouched; the state outputs carry a guard row too."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import actor_critic_restate as R
from tests import online_lstm_restate as RL

pytestmark = pytest.mark.gpu

NAN = float("nan")
GAMMA, LAM = 0.99, 0.95


def _lib():
    from rltime_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(c, rec, shift_out=0):
    """One launch on the case's rings.  rec: through mirl_online_window_rec, else mirl_online_window.  `shift` float32 words
    put the state ring (shift_out: the two state outputs) off the allocation's 16-byte boundary."""
    L = _lib()
    T, B, E, cap, S = c["T"], c["B"], c["E"], c["cap"], c["S"]
    obs = _dev(c["obs"])
    row_bytes = int(np.prod(c["obs"].shape[2:])) * c["obs"].itemsize
    pol = torch.stack([_dev(c["logp"]), _dev(c["values"])], dim=-1).contiguous()
    f32 = lambda: torch.full((T + 1, B), NAN, device="cuda")                                # noqa: E731
    ret, ns, mk, lp, val, ini_s, ini_t = f32(), f32(), f32(), f32(), f32(), f32(), f32()
    acts = torch.full((T + 1, B), -7, dtype=torch.int32, device="cuda")
    st = torch.full((2, T + 1, B, row_bytes), 0xA5, dtype=torch.uint8, device="cuda")
    plan, ra, rr, rd = _dev(c["plan"]), _dev(c["actions"]), _dev(c["rewards"]), _dev(c["dones"])
    args = (T, B, E, cap, c["n"], GAMMA, LAM, row_bytes, _p(plan), _p(obs), _p(ra), _p(rr), _p(rd), _p(pol), _p(pol.view(-1)[1:]), 2,
            _p(ret), _p(ns), _p(mk), _p(acts), _p(lp), _p(val), _p(st[0]), _p(st[1]))
    out_s = out_t = None
    if rec:
        shift = c["shift"]
        ring_buf = torch.full((cap * E * S + shift,), NAN, device="cuda")
        ring = ring_buf[shift:].view(cap, E, S)
        ring.copy_(_dev(c["state"]))
        assert ring.data_ptr() % 16 == 4 * shift and ring_buf.data_ptr() % 16 == 0
        ini = _dev(c["initials"])
        bufs = [torch.full(((T + 1) * B * S + shift_out,), NAN, device="cuda") for _ in range(2)]
        out_s, out_t = (b[shift_out:].view(T + 1, B, S) for b in bufs)
        L.check(L.lib.mirl_online_window_rec(*args, 1, _p(ring), _p(ini), S, _p(out_s), _p(out_t), _p(ini_s), _p(ini_t), _st()),
                "mirl_online_window_rec")
    else:
        L.check(L.lib.mirl_online_window(*args, _st()), "mirl_online_window")
    torch.cuda.synchronize()
    for t in (ret, ns, mk, lp, val) + ((ini_s, ini_t) if rec else ()):
        assert bool(torch.isnan(t[T]).all()), "the guard row was written"
    assert bool((acts[T] == -7).all()) and bool((st[:, T] == 0xA5).all()), "the guard row was written"
    shape = (T, B) + c["obs"].shape[2:]
    view = lambda x: x[:T].contiguous().cpu().numpy().view(c["obs"].dtype).reshape(shape)   # noqa: E731
    out = {"returns": ret[:T].cpu().numpy(), "nsteps": ns[:T].cpu().numpy(), "target_masks": mk[:T].cpu().numpy(),
           "actions": acts[:T].cpu().numpy(), "action_log_probs": lp[:T].cpu().numpy(), "values": val[:T].cpu().numpy(),
           "states": view(st[0]), "target_states": view(st[1])}
    if rec:
        assert bool(torch.isnan(out_s[T]).all()) and bool(torch.isnan(out_t[T]).all()), "the state guard row was written"
        assert shift_out == 0 or (bool(torch.isnan(bufs[0][:shift_out]).all()) and bool(torch.isnan(bufs[1][:shift_out]).all()))
        out.update(states_state=out_s[:T].cpu().numpy(), target_state=out_t[:T].cpu().numpy(),
                   states_initials=ini_s[:T].cpu().numpy(), target_initials=ini_t[:T].cpu().numpy())
    return out


_EXACT = ("nsteps", "target_masks", "actions", "action_log_probs", "values", "states", "target_states")
_STATE = ("states_state", "target_state", "states_initials", "target_initials")


@pytest.mark.parametrize("name", sorted(RL.REC_WINDOW_CASES))
def test_recurrent_window_equals_the_restatement(name):
    c = RL.rec_window_case(name)
    want = RL.window_rec(c["T"], c["B"], c["E"], c["cap"], c["n"], GAMMA, LAM, c["plan"], c["obs"], c["actions"], c["rewards"],
                         c["dones"], c["logp"], c["values"], c["state"], c["initials"])
    # the case holds what it is named for
    if name in ("words", "two_per_env", "two_layers", "long_words"):
        assert c["S"] % 4 != 0
    else:
        assert c["S"] % 4 == 0
    assert name != "tight_ring" or c["cap"] == c["T"] + 1
    assert name != "two_per_env" or c["B"] > c["E"]
    got = _run(c, rec=True)
    for key in _EXACT + _STATE:
        assert got[key].dtype == want[key].dtype or key in _EXACT, key
        assert np.array_equal(got[key].view(np.uint32) if key in _STATE else got[key],
                              want[key].view(np.uint32) if key in _STATE else want[key]), (name, key)
    bound = R.window_bound(want) + 1e-300
    ratio = float(np.max(np.abs(got["returns"].astype(np.float64) - want["returns"]) / bound))
    print("RATIO window_rec.returns %s %.4f" % (name, ratio))
    assert np.all(np.isfinite(got["returns"])) and ratio <= 1.0
    # the older entry on the same rings: its outputs, and the recurrent entry's, byte for byte
    old = _run(c, rec=False)
    for key in old:
        assert np.array_equal(old[key].view(np.uint8), got[key].view(np.uint8)), (name, key)
    again = _run(c, rec=True)
    assert all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got)
    if c["S"] % 4 == 0:
        # outputs off the 16-byte boundary: the launcher takes the word path for these too
        off = _run(c, rec=True, shift_out=1)
        assert all(np.array_equal(got[k].view(np.uint8), off[k].view(np.uint8)) for k in got)


def test_recurrent_window_refuses_bad_arguments():
    L = _lib()
    x = torch.zeros(256, device="cuda")
    xi = torch.zeros(64, dtype=torch.int32, device="cuda")
    xb = torch.zeros(256, dtype=torch.uint8, device="cuda")
    o = torch.zeros(256, device="cuda")

    def call(S=4, ring=x, ini=x, out=o, T=2):
        return L.lib.mirl_online_window_rec(T, 1, 1, 4, 1, 0.99, 0.95, 4, _p(xi), _p(xb), _p(xi), _p(x), _p(xb), _p(x), _p(x), 1,
                                            _p(x), _p(x), _p(x), _p(xi), _p(x), _p(x), _p(xb), _p(xb), 1,
                                            _p(ring), _p(ini), S, _p(out), _p(o), _p(o), _p(o), _st())
    for kw in (dict(S=0), dict(S=-1), dict(ring=None), dict(ini=None), dict(out=None), dict(T=0)):
        assert call(**kw) == L.MIRL_ERR_ARG, kw
        assert "online_window_rec" in L.last_error()
    torch.cuda.synchronize()
    assert bool((o == 0).all()), "a refused call wrote"
