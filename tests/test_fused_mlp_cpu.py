"""No GPU: the opt-in wiring of the fused MLP acting step (acting.extra_args.fused_step -> Actor(fused_mlp=...),
Evaluator(fused_mlp=...)), the host-only shape gate of csrc/act_mlp.hip, and the two facts the GPU tests lean on that can
be established here: the float64 reference's rows are clear for the seeds tests/act_mlp_restate.py uses, and the
hand-made controller of tests/test_fused_mlp_eval_gpu.py holds the pole to the cap in the NumPy restatement of the device
CartPole under the seed that test uses."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import act_mlp_restate as R
from tests import cartpole_device_restate as CP
from tests.eval_restate import EvalCount


# ---- configs and the flag's way to the actor ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole_dqn", "cartpole_iqn"])
def test_fused_config_is_its_parent_plus_the_opt_in(name):
    from rltime_amd.general.config import load_config, validate_config
    fused, parent = load_config(name + "_fused.json"), load_config(name + ".json")
    validate_config(fused)
    assert fused["acting"]["extra_args"]["fused_step"] is True
    assert "fused_step" not in parent["acting"]["extra_args"]
    del fused["acting"]["extra_args"]["fused_step"]
    assert fused == parent


class _Env:
    num_envs = 16

    def __init__(self):
        from rltime_amd.spaces import Box, Discrete
        self.observation_space, self.action_space = Box(-1.0, 1.0, (4,), np.float32), Discrete(2)


@pytest.mark.parametrize("name,want", [("cartpole_dqn_fused", True), ("cartpole_iqn_fused", True), ("cartpole_dqn", False),
                                       ("cartpole_iqn", False)])
def test_create_actors_passes_the_opt_in(name, want, monkeypatch):
    from rltime_amd import train
    from rltime_amd.general.config import load_config
    monkeypatch.setattr(train, "make_vec_env", lambda *a, **k: _Env())
    actor = train.create_actors(load_config(name + ".json"), device="cpu", device_acting=False)
    assert actor._fused_mlp is want and actor._fast_cls is None


def test_the_defaults_stay_off():
    from rltime_amd.acting.actor import Actor
    from rltime_amd.acting.evaluator import Evaluator
    p = inspect.signature(Actor.__init__).parameters
    assert p["fused_mlp"].default is False and p["fused_actor_critic"].default is False
    assert inspect.signature(Evaluator.__init__).parameters["fused_mlp"].default is False
    assert Actor(_Env())._fused_mlp is False


# ---- the shape gate ------------------------------------------------------------------------------------------------------------
def _gate(E, O, widths, N, D, HID, A, dueling):
    from rltime_amd._lib import lib
    w = (C.c_int32 * 3)(*(list(widths) + [0, 0, 0])[:3])
    return lib.mirl_act_mlp_supported(E, O, len(widths), w, N, D, HID, A + (1 if dueling else 0), A)


def test_shape_gate_is_host_logic():
    from rltime_amd._lib import lib
    for name, shape in R.SHAPES.items():
        assert _gate(*shape) == 1, name
    iqn = (16, 4, [64], 32, 64, 128, 2, True)
    for what, bad in [("O = 65", (16, 65, [64], 32, 64, 128, 2, True)), ("width 257", (16, 4, [257], 32, 64, 128, 2, True)),
                      ("second width 257", (16, 4, [64, 257], 32, 64, 128, 2, True)), ("N = 65", (16, 4, [64], 65, 64, 128, 2, True)),
                      ("D = 68", (16, 4, [64], 32, 68, 128, 2, True)), ("D = 6", (16, 4, [64], 32, 6, 128, 2, True)),
                      ("HID = 513", (16, 4, [64], 32, 64, 513, 2, True)), ("A = 33", (16, 4, [64], 32, 64, 128, 33, True)),
                      ("L = 3", (16, 4, [64, 64, 64], 32, 64, 128, 2, True)), ("E = 0", (0, 4, [64], 32, 64, 128, 2, True))]:
        assert _gate(*bad) == 0, what
    assert _gate(*iqn) == 1
    # each limit itself is taken
    assert _gate(1, 64, [256, 256], 64, 64, 512, 32, True) == 1
    # the LDS block: 2 x 256 + 64 floats, the 4096-float weight tile, CH rows of phi, x and hid, N rows of outputs; under the
    # CU's 160 KB at every limit at once (CH = 16 there), under the 64 KB a kernel gets unasked for the shipped shapes (CH = 32)
    need = C.c_int64()
    w = (C.c_int32 * 2)(256, 256)
    assert lib.mirl_act_mlp_lds_bytes(64, 2, w, 64, 64, 512, 33, 32, C.byref(need)) == 0
    assert need.value == 4 * (576 + 4096 + 16 * (64 + 256 + 512) + 64 * 33) <= 160 * 1024
    w = (C.c_int32 * 2)(64, 0)
    assert lib.mirl_act_mlp_lds_bytes(4, 1, w, 32, 64, 128, 3, 2, C.byref(need)) == 0
    assert need.value == 4 * (576 + 4096 + 32 * (64 + 64 + 128) + 32 * 3) <= 65536
    assert lib.mirl_act_mlp_lds_bytes(65, 1, w, 32, 64, 128, 3, 2, C.byref(need)) < 0
    # a launch with an unsupported shape or a null operand is refused before anything touches a device
    args = [None] * 14 + [None, None, 0.0, 0, None, None, None, None, None]
    assert lib.mirl_act_mlp_fwd(16, 65, 1, w, 32, 64, 128, 3, 2, 64, 1, *args[1:]) < 0
    assert lib.mirl_act_mlp_fwd(16, 4, 1, w, 32, 64, 128, 3, 2, 64, 1, *args[1:]) < 0


# ---- the seeds of the kernel tests ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_the_seeds_leave_clear_rows(name):
    """At most one row in eight of the float64 reference has a top-two gap <= 1e-4, for the full head and for the
    advantage means that need_q = 0 selects on."""
    case = R.Case(name)
    q, adv = R.reference(case, torch.float64)
    for rows in (R.clear_rows(q), R.clear_rows(adv), R.clear_rows(q) & R.clear_rows(adv)):
        assert int((~rows).sum()) * 8 <= case.E, (name, rows)
    assert q.shape == (case.E, case.A) and torch.isfinite(q).all()


# ---- the controller of the evaluation test ---------------------------------------------------------------------------------------
def _run(policy, E, N, seed, cap):
    """The device CartPole's restatement under `policy` (obs float32 (E, 4) -> actions) with the evaluator's counting rule."""
    ec = EvalCount(E, N)
    state, obs, _, _ = CP.cartpole_reset(CP.new_state(E), seed)
    while not ec.finished:
        state, obs, r, d = CP.cartpole_step(state, policy(obs), seed, cap)
        ec.step(r, d)
    return ec


def controller(obs):
    """Push right iff 0.1 x + 0.3 v + theta + 0.5 omega > 0 (float32 products, as FC1's two units form them)."""
    s = (obs.astype(np.float32) * np.array([0.1, 0.3, 1.0, 0.5], np.float32) * np.float32(10.0)).sum(1)
    return (s > 0).astype(np.int32)


def test_the_controller_reaches_the_cap_in_the_restatement():
    """E = 16, N = 32, seed 0, cap 200 — what tests/test_fused_mlp_eval_gpu.py runs on the GPU: every counted episode is 200
    steps long; the mirrored controller falls within 15 steps on average; constant action 1 falls in 8 - 11 steps."""
    ec = _run(controller, 16, 32, 0, 200)
    assert set(ec.ep_len.tolist()) == {200} and set(ec.ep_reward.tolist()) == {200.0}
    ec = _run(lambda obs: 1 - controller(obs), 16, 32, 0, 200)
    assert float(np.mean(ec.ep_len)) < 15
    ec = _run(lambda obs: np.ones(len(obs), np.int32), 16, 32, 0, 200)
    assert 8 <= int(ec.ep_len.min()) and int(ec.ep_len.max()) <= 11
