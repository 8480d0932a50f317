"""No GPU: the opt-in wiring of the fused MLP acting step for actor-critic policies (acting.extra_args.fused_step ->
Actor(fused_actor_critic=...) -> acting/fast_mlp_step.FastMlpAcStep), the host-only shape gate and refusals of
mirl_act_mlp_ac_fwd, the step's reasons on CPU policies, and the facts the GPU tests lean on that can be established here:
the restatement's head is tests/actor_critic_restate.head on the Philox uniform, no row of the remap test sits within a
float32 ulp of uf = per at the seeds used, and the step test's rollout, replayed on the NumPy restatement of the device
CartPole with torch's float32 logits, keeps the rows near a CDF boundary inside the 2 % cap."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import act_mlp_ac_restate as R
from tests import actor_critic_restate as AR
from tests import cartpole_device_restate as CP
from tests import pointwise_restate as PR

RTOL = 2e-4                        # tests/test_fused_actor_critic_gpu.py's, as tests/test_fused_mlp_ac_step_gpu.py uses it


# ---- configs and the flag's way to the actor ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cartpole_ppo", "cartpole_a2c"])
def test_fused_config_is_its_parent_plus_the_opt_in(name):
    from rltime_amd.general.config import load_config, validate_config
    fused, parent = load_config(name + "_fused.json"), load_config(name + "_device.json")
    validate_config(fused)
    assert fused["acting"]["extra_args"]["fused_step"] is True
    assert "fused_step" not in parent["acting"]["extra_args"]
    del fused["acting"]["extra_args"]["fused_step"]
    assert fused == parent


class _Env:
    num_envs = 16

    def __init__(self, box_actions=False):
        from rltime_amd.spaces import Box, Discrete
        self.observation_space = Box(-1.0, 1.0, (4,), np.float32)
        self.action_space = Box(-1.0, 1.0, (1,), np.float32) if box_actions else Discrete(2)


@pytest.mark.parametrize("name,want", [("cartpole_ppo_fused", True), ("cartpole_a2c_fused", True), ("cartpole_ppo_device", False),
                                       ("cartpole_a2c_device", False)])
def test_create_actors_passes_the_opt_in(name, want, monkeypatch):
    from rltime_amd import train
    from rltime_amd.general.config import load_config
    monkeypatch.setattr(train, "make_vec_env", lambda *a, **k: _Env())
    actor = train.create_actors(load_config(name + ".json"), device="cpu", device_acting=False)
    assert actor._fused_actor_critic is want and actor._fast_cls is None


# ---- the shape gate and the launcher's refusals ----------------------------------------------------------------------------------
def _gate(E, O, widths, HID, A):
    from rltime_amd._lib import lib
    w = (C.c_int32 * 3)(*(list(widths) + [0, 0, 0])[:3])
    return lib.mirl_act_mlp_ac_supported(E, O, len(widths), w, HID, A)


def test_shape_gate_is_host_logic():
    from rltime_amd._lib import lib
    for name, shape in R.SHAPES.items():
        assert _gate(*shape) == 1, name
    for what, bad in [("O = 65", (16, 65, [64], 64, 2)), ("O = 0", (16, 0, [64], 64, 2)), ("width 257", (16, 4, [257], 64, 2)),
                      ("second width 257", (16, 4, [64, 257], 64, 2)), ("HID = 513", (16, 4, [64], 513, 2)),
                      ("HID = 0", (16, 4, [64], 0, 2)), ("A = 33", (16, 4, [64], 64, 33)), ("A = 0", (16, 4, [64], 64, 0)),
                      ("L = 3", (16, 4, [64, 64, 64], 64, 2)), ("E = 0", (0, 4, [64], 64, 2))]:
        assert _gate(*bad) == 0, what
    assert _gate(1, 64, [256, 256], 512, 32) == 1                 # each limit itself is taken
    assert lib.mirl_act_mlp_ac_supported(16, 4, 1, None, 64, 2) == 0
    # the gate is mirl_act_mlp_supported's with N = 1, D = 0, NO = A + 1
    w = (C.c_int32 * 2)(64, 0)
    for HID, A in [(64, 2), (512, 32), (513, 2), (64, 33)]:
        assert lib.mirl_act_mlp_ac_supported(16, 4, 1, w, HID, A) == lib.mirl_act_mlp_supported(16, 4, 1, w, 1, 0, HID, A + 1, A)


def test_the_launcher_refuses_before_anything_touches_a_device():
    """An unsupported shape, a null operand, a missing step word (also with greedy), greedy outside 0 | 1, out_pitch < 2:
    MIRL_ERR_ARG from host logic (the pointers here are never dereferenced: every call is refused)."""
    from rltime_amd._lib import lib, MIRL_ERR_ARG
    w = (C.c_int32 * 2)(64, 0)
    x = C.c_void_p(64)                                            # a non-null operand that is never read
    good = dict(obs=x, lw0T=x, lb0=x, lw1T=None, lb1=None, fcT=x, fcb=x, outT=x, outb=x, eps=None, expo=None, eps_min=0.0, seed=1,
                step=x, greedy=0, actions=x, policy=x, out_pitch=2, logits_out=None, stream=None)

    def call(shape=(16, 4, 1, w, 64, 2), **kw):
        a = dict(good, **kw)
        return lib.mirl_act_mlp_ac_fwd(*shape, *a.values())

    assert call(shape=(16, 65, 1, w, 64, 2)) == MIRL_ERR_ARG
    assert call(shape=(16, 4, 1, w, 64, 33)) == MIRL_ERR_ARG
    for key in ("obs", "lw0T", "lb0", "fcT", "fcb", "outT", "outb", "step", "actions", "policy"):
        assert call(**{key: None}) == MIRL_ERR_ARG, key
    assert call(step=None, greedy=1) == MIRL_ERR_ARG
    assert call(greedy=2) == MIRL_ERR_ARG and call(out_pitch=1) == MIRL_ERR_ARG
    w2 = (C.c_int32 * 2)(64, 64)
    assert call(shape=(16, 4, 2, w2, 64, 2)) == MIRL_ERR_ARG      # the second leading layer's operands are null


# ---- why_not on CPU policies ----------------------------------------------------------------------------------------------------------
def _actor(env):
    from rltime_amd.acting.actor import Actor
    return Actor(env, fused_actor_critic=True)


def _ac_policy(env, **kw):
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    return ActorCriticPolicy.create(model_config=R.MLP, observation_space=env.observation_space, action_space=env.action_space,
                                    cuda=False, **kw)


def test_why_not_reasons_on_cpu_policies():
    from rltime_amd.acting.fast_mlp_step import FastMlpAcStep, FastMlpStep
    from rltime_amd.policies.dqn import DQNPolicy
    env = _Env()
    actor = _actor(env)
    assert FastMlpAcStep.AC is True and FastMlpStep.AC is False and issubclass(FastMlpAcStep, FastMlpStep)
    assert FastMlpAcStep.why_not(actor, _ac_policy(env)) == "the policy is not on the GPU"
    assert "critic_separate_model" in FastMlpAcStep.why_not(actor, _ac_policy(env, critic_separate_model=True))
    dqn = DQNPolicy.create(model_config=R.MLP, observation_space=env.observation_space, action_space=env.action_space, cuda=False)
    assert FastMlpAcStep.why_not(actor, dqn) == "the policy is not an actor-critic policy"
    box = _Env(box_actions=True)
    assert FastMlpAcStep.why_not(_actor(box), _ac_policy(box)) == "the action space is not Discrete"
    # the Q-learning step keeps its own answer for an actor-critic policy
    assert FastMlpStep.why_not(actor, _ac_policy(env)) == "the policy is not on the GPU"
    # the parts query is host logic on the module tree: the shipped model's parts and shape
    pol = _ac_policy(env)
    lins = FastMlpStep._fc_stack(pol)
    assert isinstance(lins, str) and "GPU" in lins               # (a CPU Linear is the reason on the CPU)
    two = {"type": "sequential", "args": {"layer_configs": [{"type": "fc", "args": {"fc_size": 64, "fc_count": 2}}]}}
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    pol2 = ActorCriticPolicy.create(model_config=two, observation_space=env.observation_space, action_space=env.action_space, cuda=False)
    assert "single Linear" in FastMlpStep._fc_stack(pol2)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_the_restatements_head_is_actor_critic_restates(name):
    case = R.Case(name)
    rows = R.reference(case, torch.float32).numpy()
    assert rows.shape == (case.E, case.A + 1) and np.isfinite(rows).all()
    for step in R.STEPS:
        u = PR.philox_head_draws(R.RNG_SEED, step, case.E, case.A)[0].numpy()
        assert np.array_equal(u, R.uniform24(R.philox_words(R.RNG_SEED, step, case.E)[:, 0]))
        for greedy in (False, True):
            a, lp, v = R.head(rows, R.RNG_SEED, step, greedy=greedy)
            wa, wlp = AR.head(rows[:, :case.A].astype(np.float64), u, greedy=greedy)
            assert np.array_equal(a, wa) and np.array_equal(lp, wlp) and np.array_equal(v, rows[:, case.A])
    if case.A == 1:
        assert np.all(a == 0) and np.all(lp == 0.0)


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_no_row_of_the_remap_test_is_within_an_ulp(name):
    """eps = 1, 0 and 0.5 at the kernel tests' key and step words: per is exact (pow(x, 1) = x) and no uniform lies within one
    float32 ulp of it; eps = 1 remaps every row, eps = 0 none."""
    case = R.Case(name)
    sampled = np.arange(case.E) % case.A
    for step in R.STEPS:
        for eps in (1.0, 0.0, 0.5):
            got, near = R.eps_remap(sampled, R.RNG_SEED, step, case.A, eps)
            assert not near.any(), (name, step, eps)
            assert got.min() >= 0 and got.max() < case.A
            words = R.philox_words(R.RNG_SEED, step, case.E)
            rnd = ((words[:, 3] * np.uint64(case.A)) >> np.uint64(32)).astype(np.int64)
            if eps == 1.0:
                assert np.array_equal(got, rnd)
            if eps == 0.0:
                assert np.array_equal(got, sampled)
    # a per-actor exponent and a floor: eps 0.5, exponents 1 .. E, floor 0.1
    expo = np.arange(1, case.E + 1, dtype=np.float64)
    got, near = R.eps_remap(sampled, R.RNG_SEED, R.STEPS[0], case.A, 0.5, expo=expo, eps_min=0.1)
    assert not near.any()


def test_the_remap_takes_both_branches_at_eps_half():
    case = R.Case("shipped")
    words = R.philox_words(R.RNG_SEED, R.STEPS[0], case.E)
    hit = R.uniform24(words[:, 2]) < np.float32(0.5)
    assert 2 <= int(hit.sum()) <= case.E - 2


# ---- the step test's rollout on the CPU -------------------------------------------------------------------------------------------------
def test_the_step_tests_seeds_stay_inside_the_cap():
    """tests/test_fused_mlp_ac_step_gpu.py's 8 vector steps at E = 16 with the weight change after step 4, on the NumPy device
    CartPole with torch's float32 logits and the float64 head: the rows whose uniform lies within RTOL S + bound of a CDF
    boundary are at most 2 % of the rows, and both actions are taken."""
    E = R.STEP_E
    env = _Env()
    pol = R.step_policy(env, cuda=False)
    state, obs, _, _ = CP.cartpole_reset(CP.new_state(E), R.STEP_ENV_SEED)
    rows = excluded = 0
    seen = set()
    for i in range(8):
        if i == 4:
            R.change_weights(pol)
        with torch.no_grad():
            logits, _ = pol.get_logits_and_state_value(R.input_tree(torch.from_numpy(obs)), 1)
        z = logits.float().numpy()
        u = PR.philox_head_draws(R.STEP_RNG_SEED, R.FIRST_WORD + i, E, 2)[0].numpy()
        actions, _ = AR.head(z, u)
        margin, bound = AR.head_margin(z, u)
        clear = margin > RTOL * AR.softmax_parts(z)[3] + bound
        rows, excluded = rows + E, excluded + int((~clear).sum())
        seen.update(actions.tolist())
        state, obs, _, _ = CP.cartpole_step(state, actions, R.STEP_ENV_SEED, 200)
    assert rows == 128 and excluded <= 0.02 * rows, excluded
    assert seen == {0, 1}
