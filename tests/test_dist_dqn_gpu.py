"""GPU: the distributional DQN (C51) trainer on its HIP kernels (csrc/c51.hip) against the
reference: the target projection and the loss against dist_dqn_cases.npz (recorded from the
unmodified reference by tests/golden/generate_dist_dqn.py) and against the CPU restatement
(tests/c51_restate.py) over a shape sweep, the acting head against actor_predict, the fused
acting step against the generic device path, the reference's C51 training trajectory, the
graphed learner step against the eager one, and a short run of the shipped config."""
import copy
import io
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import c51_restate as c51
from tests import scenario

pytestmark = pytest.mark.gpu

CASES = os.path.join(scenario.GOLDEN, "dist_dqn_cases.npz")


def _cuda(x, dt=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(dt).cuda()


@pytest.mark.parametrize("tag", ["z11", "z11_dq", "z51", "z51_dq", "z101_dq"])
def test_target_kernel_matches_reference(tag):
    from rltime_amd.training import qops
    d = np.load(CASES)
    g = lambda k: d["tg.%s.%s" % (tag, k)]  # noqa: E731
    Z, gamma, vmin, vmax, dq = g("meta")
    lt = _cuda(g("logits_target"))
    ls = _cuda(g("logits_select")) if dq else lt
    y = qops.q_target_c51(lt, ls, torch.linspace(vmin, vmax, int(Z)).cuda(), _cuda(g("returns")), _cuda(g("nsteps")),
                          _cuda(g("masks")), float(gamma), int(vmin), int(vmax)).cpu().numpy()
    want = g("target")
    np.testing.assert_allclose(y, want, rtol=0, atol=1e-6)
    assert np.array_equal(y == 0, want == 0)                  # the dropped bins, exactly


@pytest.mark.parametrize("M,A,Z", [(m, a, z) for m in (1, 7, 512) for a in (2, 6, 18) for z in (11, 51, 101)]
                         + [(40960, 6, 51), (40960, 18, 101), (40960, 2, 11)])
def test_target_kernel_shape_sweep(M, A, Z):
    from rltime_amd.training import qops
    g = torch.Generator().manual_seed(M * 7 + A * 3 + Z)
    lt, ls = torch.randn(M, A, Z, generator=g) * 2, torch.randn(M, A, Z, generator=g) * 2
    r = torch.where(torch.rand(M, generator=g) < 0.5, torch.randint(-1, 2, (M,), generator=g).float(), torch.randn(M, generator=g))
    n = torch.randint(1, 4, (M,), generator=g).float()
    mk = (torch.rand(M, generator=g) > 0.3).float()
    sup = torch.linspace(-10, 10, Z)
    want = c51.target(lt, ls, sup, r, n, mk, 0.99, -10, 10)
    got = qops.q_target_c51(lt.cuda(), ls.cuda(), sup.cuda(), r.cuda(), n.cuda(), mk.cuda(), 0.99, -10, 10).cpu()
    # rows whose selection is a near-tie of two actions' expected values may pick either
    ev = (torch.softmax(ls, -1) * sup).sum(2)
    top = ev.topk(min(2, A), dim=1).values
    clear = (top[:, 0] - top[:, -1]) > 1e-5 if A > 1 else torch.ones(M, dtype=torch.bool)
    assert clear.float().mean() > 0.99
    np.testing.assert_allclose(got[clear].numpy(), want[clear].numpy(), rtol=0, atol=1e-6)
    # the paper's projection against a float64 restatement: all of the mass stays
    best = c51.select_actions(ls.double(), sup.double())
    p64 = torch.softmax(lt.double()[torch.arange(M), best], -1)
    want64 = c51.project(p64, r.double(), n.double(), mk.double(), sup.double(), 0.99, -10, 10, "paper")
    got_p = qops.q_target_c51(lt.cuda(), ls.cuda(), sup.cuda(), r.cuda(), n.cuda(), mk.cuda(), 0.99, -10, 10, "paper").cpu()
    np.testing.assert_allclose(got_p[clear].double().numpy(), want64[clear].numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(got_p.sum(1).numpy(), 1.0, atol=1e-5)


def _sweep_inputs(M, A, Z, seed):
    """The input recipe of test_target_kernel_shape_sweep."""
    g = torch.Generator().manual_seed(seed)
    lt, ls = torch.randn(M, A, Z, generator=g) * 2, torch.randn(M, A, Z, generator=g) * 2
    r = torch.where(torch.rand(M, generator=g) < 0.5, torch.randint(-1, 2, (M,), generator=g).float(), torch.randn(M, generator=g))
    n = torch.randint(1, 4, (M,), generator=g).float()
    mk = (torch.rand(M, generator=g) > 0.3).float()
    return lt, ls, r, n, mk


# a lane owns atoms l, l + 64, l + 128, l + 192: every strip boundary, the smallest supports and a single action
STRIP_Z = (2, 3, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256)


@pytest.mark.parametrize("M,A,Z", [(m, a, z) for m in (7, 512, 4099) for a in (1, 2, 18) for z in STRIP_Z])
def test_target_kernel_strip_boundaries(M, A, Z):
    from rltime_amd.training import qops
    lt, ls, r, n, mk = _sweep_inputs(M, A, Z, M * 7 + A * 3 + Z)
    sup = torch.linspace(-10, 10, Z)
    want = c51.target(lt, ls, sup, r, n, mk, 0.99, -10, 10)
    if A == 1 or M < 512:
        # one left-out row of 7 would be 14 %: nothing is left out, the float64 reference itself has no near-tie
        if A > 1:
            top64 = (torch.softmax(ls.double(), -1) * sup.double()).sum(2).topk(2, dim=1).values
            assert bool(((top64[:, 0] - top64[:, 1]) > 1e-5).all())
        clear = torch.ones(M, dtype=torch.bool)
    else:
        ev = (torch.softmax(ls, -1) * sup).sum(2)
        top = ev.topk(2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > 1e-5
        assert clear.float().mean() > 0.99
    dev = [t.cuda() for t in (lt, ls, sup, r, n, mk)]
    got = qops.q_target_c51(*dev, 0.99, -10, 10).cpu()
    err = float((got[clear] - want[clear]).abs().max())
    print("reference projection M=%d A=%d Z=%d: max |kernel - restatement| %.3e" % (M, A, Z, err))
    np.testing.assert_allclose(got[clear].numpy(), want[clear].numpy(), rtol=0, atol=1e-6)
    assert np.array_equal(got[clear].numpy() == 0, want[clear].numpy() == 0)          # the dropped bins, exactly
    # the paper's projection against float64: the float32 arithmetic of the restatement itself is e_ref away from it (up to
    # 1.9e-5 at Z = 256 on these inputs), the kernel may be as far again
    best = c51.select_actions(ls.double(), sup.double())
    p64 = torch.softmax(lt.double()[torch.arange(M), best], -1)
    want64 = c51.project(p64, r.double(), n.double(), mk.double(), sup.double(), 0.99, -10, 10, "paper")
    ref_p = c51.target(lt, ls, sup, r, n, mk, 0.99, -10, 10, "paper")
    e_ref = float((ref_p[clear].double() - want64[clear]).abs().max())
    got_p = qops.q_target_c51(*dev, 0.99, -10, 10, "paper").cpu()
    e_got = float((got_p[clear].double() - want64[clear]).abs().max())
    print("paper projection M=%d A=%d Z=%d: e_ref %.3e kernel %.3e" % (M, A, Z, e_ref, e_got))
    assert e_got <= 2.0 * e_ref + 1e-6, (e_got, e_ref)
    np.testing.assert_allclose(got_p.sum(1).numpy(), 1.0, atol=1e-5)


def test_target_kernel_refuses_too_many_atoms():
    from rltime_amd._lib import MirlError
    from rltime_amd.training import qops
    x = torch.zeros(2, 2, 257, device="cuda")
    with pytest.raises(MirlError):
        qops.q_target_c51(x, x, torch.linspace(-10, 10, 257, device="cuda"), *(torch.zeros(2, device="cuda"),) * 3, 0.99, -10, 10)


def test_loss_kernel_matches_reference():
    from rltime_amd.training import qops
    d = np.load(CASES)
    logits, targets = d["ls.logits"], d["ls.targets"]
    actions, weights, T = d["ls.actions"], d["ls.weights"].astype(np.float32), int(d["ls.timesteps"])
    for bm, tm in [("mean", None), ("sum", None), ("mean", "mean"), ("sum", "mean"), ("mean", "sum")]:
        for use_w in (False, True):
            for mode in ("crossentropy", "huber", "mse"):
                tag = "ls.%s.%s.w%d.%s" % (bm, tm, use_w, mode)
                x = _cuda(logits).requires_grad_(True)
                loss, rep = qops.c51_loss(x, _cuda(actions, torch.int64), _cuda(targets), _cuda(weights) if use_w else None,
                                          mode, 1.0, T, bm, tm)
                loss.backward()
                np.testing.assert_allclose(float(loss.detach()), float(d[tag + ".loss"]), rtol=1e-5, atol=1e-5, err_msg=tag)
                np.testing.assert_allclose(rep.cpu().numpy(), d[tag + ".report"], rtol=1e-5, atol=1e-5, err_msg=tag)
                np.testing.assert_allclose(x.grad.cpu().numpy(), d[tag + ".grad"], rtol=0, atol=1e-5, err_msg=tag)
                # and against autograd of the reference formula in float64
                x64 = torch.from_numpy(logits).double().requires_grad_(True)
                l64, _ = c51.loss(x64, actions, torch.from_numpy(targets).double(),
                                  torch.from_numpy(weights).double() if use_w else None, mode, 1.0, T, bm, tm)
                l64.backward()
                np.testing.assert_allclose(x.grad.cpu().double().numpy(), x64.grad.numpy(), rtol=0, atol=1e-5, err_msg=tag)
    # the fixture's rows 0 and 1 sit in the clamp: some atoms below 1e-5, one above 1 - 1e-5
    p = torch.softmax(torch.from_numpy(logits[[0, 1], 0]), -1)
    assert (p < 1e-5).any() and (p > 1 - 1e-5).any()


@pytest.mark.parametrize("M", [1, 513])
@pytest.mark.parametrize("A", [1, 18])
@pytest.mark.parametrize("Z", [2, 64, 65, 128, 129, 256])
def test_loss_kernel_strip_boundaries(M, A, Z):
    """loss, report and gradient of the three modes against float64 autograd of the restatement, with rows in the clamp of
    the cross-entropy whose peak sits in the last strip a lane owns."""
    from rltime_amd.training import qops
    g = torch.Generator().manual_seed(M * 5 + A * 3 + Z)
    logits = torch.randn(M, A, Z, generator=g) * 2
    actions = torch.randint(0, A, (M,), generator=g)
    targets = torch.softmax(torch.randn(M, Z, generator=g) * 2, -1)
    weights = torch.rand(M, generator=g) + 0.5
    peaks = []
    if M > 1:
        # rows 0 and 1: one atom above 1 - 1e-5, every other below 1e-5; the peak in the highest strip and one strip lower
        peaks = [Z - 1, max(Z - 1 - 64, 0)]
        for row, j in enumerate(peaks):
            logits[row, actions[row], j] = 40.0
    p64 = torch.softmax(logits.double()[torch.arange(M), actions], -1)
    for row, j in enumerate(peaks):
        assert float(p64[row, j]) > 1 - 1e-5 and bool((p64[row, torch.arange(Z) != j] < 1e-5).all())
        assert j // 64 == (Z - 1) // 64 - (row if Z > 64 else 0)
    # no probability so close to a clamp bound that float32 and float64 could pass the gradient on different sides: a float32
    # softmax of logits below 16 in magnitude is within about 16 * 2^-23 = 2e-6 of the exact one, relatively
    assert float(torch.minimum((p64 - 1e-5).abs() / 1e-5, (p64 - (1 - 1e-5)).abs() / 1e-5).min()) > 5e-6
    for use_w in (False, True):
        for mode in ("crossentropy", "huber", "mse"):
            tag = "M=%d A=%d Z=%d w%d %s" % (M, A, Z, use_w, mode)
            x = logits.cuda().requires_grad_(True)
            loss, rep = qops.c51_loss(x, actions.cuda(), targets.cuda(), weights.cuda() if use_w else None, mode, 1.0, 1, "mean", None)
            loss.backward()
            x64 = logits.double().requires_grad_(True)
            l64, rep64 = c51.loss(x64, actions, targets.double(), weights.double() if use_w else None, mode, 1.0, 1, "mean", None)
            l64.backward()
            np.testing.assert_allclose(float(loss.detach()), float(l64.detach()), rtol=1e-5, atol=1e-5, err_msg=tag)
            np.testing.assert_allclose(rep.cpu().double().numpy(), rep64.detach().numpy(), rtol=1e-5, atol=1e-5, err_msg=tag)
            np.testing.assert_allclose(x.grad.cpu().double().numpy(), x64.grad.numpy(), rtol=0, atol=1e-5, err_msg=tag)


@pytest.mark.parametrize("dueling", [False, True])
@pytest.mark.parametrize("A", [1, 18])
@pytest.mark.parametrize("Z", [64, 65, 129, 256])
def test_acting_head_strip_boundaries(Z, A, dueling):
    """mirl_actor_head_c51 against the dueling combine written out in float64: q_a = sum_j softmax_j(V_j + A_aj - mean_a A_aj) z_j,
    without a value stream softmax_j(A_aj); greedy actions wherever the float64 q-values have a clear maximum."""
    import ctypes as C
    from rltime_amd._lib import lib, check
    E = 67
    g = torch.Generator().manual_seed(Z * 3 + A + dueling)
    adv = torch.randn(E, A, Z, generator=g) * 3
    val = torch.randn(E, Z, generator=g) * 3 if dueling else None
    sup = torch.linspace(-10, 10, Z)
    x64 = adv.double()
    if dueling:
        x64 = val.double().unsqueeze(1) + x64 - x64.mean(1, keepdim=True)
    q64 = (torch.softmax(x64, -1) * sup.double()).sum(-1)
    if A > 1:
        top = q64.topk(2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > 1e-4
    else:
        clear = torch.ones(E, dtype=torch.bool)
    assert clear.float().mean() > 0.9
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)  # noqa: E731
    adv_d, val_d, sup_d = adv.cuda(), (val.cuda() if dueling else None), sup.cuda()
    acts = torch.full((E,), -1, dtype=torch.int32, device="cuda")
    q = torch.full((E, A), float("nan"), device="cuda")
    check(lib.mirl_actor_head_c51(E, A, Z, p(adv_d), A * Z, p(val_d), Z, p(sup_d), None, None, 0.0, None, None, 0, None,
                                  p(acts), p(q), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mirl_actor_head_c51")
    np.testing.assert_allclose(q.cpu().double().numpy(), q64.numpy(), rtol=0, atol=1e-5)
    assert torch.equal(acts.cpu().long()[clear], q64.argmax(1)[clear])


def _policy(dueling, A=6, Z=51, fc=64):
    from rltime_amd.policies.dist_dqn import DistDQNPolicy
    from rltime_amd.acting.synthetic_env import SyntheticAtariVecEnv
    torch.manual_seed(0)
    env = SyntheticAtariVecEnv(8, frame_shape=(4, 84, 84), n_actions=A, seed=5, done_prob=0.05)
    mc = {"type": "sequential", "args": {"layer_configs": [NATURE, {"type": "fc", "args": {"fc_size": fc}}]}}
    pol = DistDQNPolicy.create(model_config=mc, observation_space=env.observation_space, action_space=env.action_space,
                               dueling=dueling, num_atoms=Z)
    with torch.no_grad():                        # spread the distributions: a visible argmax
        pol.out_layer.weight.mul_(20.0)
    return pol, env


NATURE = {"type": "cnn", "args": {"channels_last": True, "layers": [
    {"filters": 32, "kernel": 8, "stride": 4}, {"filters": 64, "kernel": 4, "stride": 2}, {"filters": 64, "kernel": 3, "stride": 1}]}}


@pytest.mark.parametrize("dueling", [False, True])
def test_acting_head_matches_actor_predict(dueling):
    import ctypes as C
    from rltime_amd._lib import lib, check
    pol, env = _policy(dueling)
    E, A, Z = 64, 6, 51
    obs = torch.randint(0, 256, (E, 4, 84, 84), dtype=torch.uint8, device="cuda")
    state = pol.make_input_state(obs, torch.ones(E, device="cuda"))
    want = pol.actor_predict(state, 1, as_numpy=False)
    adv, val, n = pol.actor_head_raw(state, 1)
    adv = adv.contiguous()
    val = val.contiguous() if val is not None else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    acts = torch.empty(E, dtype=torch.int32, device="cuda")
    q = torch.empty((E, A), device="cuda")
    check(lib.mirl_actor_head_c51(E, A, Z, p(adv), A * Z, p(val), Z, p(pol.support), None, None, 0.0, None, None, 0, None,
                                  p(acts), p(q), None, st), "mirl_actor_head_c51")
    np.testing.assert_allclose(q.cpu().numpy(), want["qvalues"].cpu().numpy(), rtol=0, atol=1e-5)
    wq = want["qvalues"].cpu()
    top = wq.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-4
    assert clear.float().mean() > 0.9
    assert torch.equal(acts.cpu().long()[clear], want["actions"].cpu()[clear])
    # epsilon-greedy: the same Philox draws as the DQN head (mirl_actor_head_rng fed these q-values as its advantages)
    eps = torch.tensor(0.9, dtype=torch.float64, device="cuda")
    expo = torch.linspace(1, 8, E, dtype=torch.float64, device="cuda")
    step = torch.tensor([17], dtype=torch.int64, device="cuda")
    a51, q51 = torch.empty_like(acts), torch.empty_like(q)
    a1, q1 = torch.empty_like(acts), torch.empty_like(q)
    used51, used1 = torch.empty(E, device="cuda"), torch.empty(E, device="cuda")
    check(lib.mirl_actor_head_c51(E, A, Z, p(adv), A * Z, p(val), Z, p(pol.support), p(eps), p(expo), 0.01, None, None, 1234,
                                  p(step), p(a51), p(q51), p(used51), st), "mirl_actor_head_c51")
    qin = q.clone()
    check(lib.mirl_actor_head_rng(E, 1, A, p(qin), A, None, 0, p(eps), p(expo), 0.01, 1234, p(step), p(a1), p(q1), p(used1), st),
          "mirl_actor_head_rng")
    assert torch.equal(a51, a1) and torch.equal(used51, used1)
    assert (a51 != acts).any()


def _actor(fast, exploration=None, E=16):
    from rltime_amd.acting.actor import Actor
    pol, env = _policy(True)
    from rltime_amd.acting.synthetic_env import SyntheticAtariVecEnv
    env = SyntheticAtariVecEnv(E, frame_shape=(4, 84, 84), n_actions=6, seed=5, done_prob=0.05)
    actor = Actor(env, exploration_config=exploration, device=True, use_graph=True)
    actor.fast_step = fast
    actor.set_actor_policy(pol)
    return actor


def test_fused_acting_step_equals_the_generic_device_path():
    """get_samples through FastActingStep (engaged, the A * Z head routed to mirl_actor_head_c51) ingests into a replay
    exactly what the generic device path (actor_head_raw + the same kernel) ingests."""
    from rltime_amd.history import ReplayHistoryBuffer
    E = 16
    expl = {"type": "epsilon_greedy", "args": {"eps_start": 0.3, "eps_final": 0.3, "exploration_fraction": 0.5}}
    shards = []
    for fast in (True, False):
        actor = _actor(fast, exploration=None, E=E)
        hist = ReplayHistoryBuffer(size=E * 40, train_frequency=4, nstep_target=2, nstep_train=1, prefix_steps=0, gamma=0.99,
                                   device_rng=True, keep_policy_outputs=True)
        for _ in range(4):
            hist.update(actor.get_samples(E * 5))
        assert (actor._fast is not None and actor._fast is not False) == fast
        shards.append((hist.get_train_data(32, train_progress=0.5), hist.stats()))
        hist.close()
    (ba, sa), (bb, sb) = shards
    assert sa == sb
    flat = lambda tree: [tree] if isinstance(tree, torch.Tensor) else [x for v in (tree.values() if isinstance(tree, dict) else tree) for x in flat(v)] if tree is not None else []   # noqa: E731
    la, lb = flat(ba), flat(bb)
    assert len(la) == len(lb)
    for x, y in zip(la, lb):
        if x.is_floating_point():
            np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=2e-4, atol=2e-5)
        else:
            assert torch.equal(x, y)
    # with exploration the fused step's in-kernel draws explore at the configured rate
    actor = _actor(True, exploration=expl, E=64)
    steps = actor.get_samples(64 * 20).vector_steps
    a = torch.stack([s["actions"] for s in steps]).cpu()
    greedy = torch.stack([s["policy"].argmax(1) for s in steps]).cpu().to(torch.int32)
    assert 0.01 < (a != greedy).float().mean().item() < 0.3


def _scripted(spec):
    from rltime_amd.acting.acting_interface import ActingInterface
    from rltime_amd.spaces import Box, Discrete
    from tests.golden.streams import vector_steps, as_reference_samples

    class ScriptedActor(ActingInterface):
        def __init__(self):
            super().__init__(Box(0, 255, spec.frame_shape, np.uint8), Discrete(spec.n_actions))
            self.t = 0

        def get_env_count(self):
            return spec.num_envs

        def set_actor_policy(self, p):
            pass

        def update_state(self, progress, policy_state=None):
            pass

        def close(self):
            pass

        def get_samples(self, min_samples):
            iters = (max(1, min_samples) + spec.num_envs - 1) // spec.num_envs
            out = []
            for step in vector_steps(spec, iters, start_step=self.t):
                out.extend(as_reference_samples(spec, step, empty_layers=(0, 2)))
            self.t += iters
            return out
    return ScriptedActor()


def test_training_series_follows_reference():
    """The reference's DistDQN (recurrent, dueling, double-Q, burn-in, prioritized replay) trained on CPU: same number of
    learner steps, qloss / grad_norm within 2e-3 over the first 40 steps (the bar test_e2e_gpu.py holds DQN to)."""
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.training.dist_dqn import DistDQN
    from tests.golden.streams import StreamSpec
    d = np.load(os.path.join(scenario.GOLDEN, "e2e_dist_dqn_lstm_per.npz"))
    cfg = json.loads(str(d["config"]))
    spec = StreamSpec(**cfg["spec"])
    random.seed(cfg["seed"]); np.random.seed(cfg["seed"]); torch.manual_seed(cfg["seed"])
    pargs = dict(cfg["policy_args"], cuda=True)
    tr = DistDQN(logger=NullLogger(), actors=_scripted(spec), model_config=cfg["model"], policy_args=pargs)
    series = {"qloss": [], "grad_norm": []}
    orig = tr.value_log.log

    def tap(key, value, *a, **k):
        if key in series and k.get("group") == "train":
            series[key].append(float(value.item() if hasattr(value, "item") else value))
        return orig(key, value, *a, **k)
    tr.value_log.log = tap
    real_init = tr.init_policies

    def init_from_reference():
        real_init()
        tr.policy.load_state_dict(torch.load(io.BytesIO(d["init_online"].tobytes()), map_location="cuda"))
        tr.target_policy.load_state_dict(torch.load(io.BytesIO(d["init_target"].tobytes()), map_location="cuda"))
    tr.init_policies = init_from_reference
    tr.train(**copy.deepcopy(cfg["train"]))
    n = 40
    assert len(series["qloss"]) == len(d["qloss"])
    np.testing.assert_allclose(series["qloss"][:n], d["qloss"][:n], rtol=2e-3, atol=1e-5)
    np.testing.assert_allclose(series["grad_norm"][:n], d["grad_norm"][:n], rtol=2e-3, atol=1e-5)


BASE = {
    "acting": {"actor_envs": 8, "exploration": {"type": "epsilon_greedy", "args": {"eps_start": 1.0, "eps_final": 1.0, "exploration_fraction": 0.5}}},
    "env": "synthetic-atari", "env_args": {"frame_shape": [4, 84, 84], "n_actions": 6, "done_prob": 0.02},
}


def _series(graphed, steps=600):
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.general.type_registry import get_registered_type
    from rltime_amd.train import create_actors
    cfg = copy.deepcopy(BASE)
    cfg["model"] = {"type": "sequential", "args": {"layer_configs": [NATURE, {"type": "fc", "args": {"fc_size": 64}}]}}
    cfg["policy_args"] = {"dueling": True, "num_atoms": 51}
    cfg["training"] = {"type": "dist_dqn", "args": {
        "clip_rewards": True, "gamma": 0.99, "mbatch_size": 32, "nstep_train": 1, "nstep_target": 3, "lr": 1e-3, "lr_anneal": True,
        "double_q": True, "clip_grad": 10.0, "target_update_freq": 24, "total_steps": steps, "log_freq": 10 ** 9, "warmup_steps": 96,
        "graph_learner_step": graphed,
        "history_mode": {"type": "prioritized_replay", "args": {"size": 400, "train_frequency": 8, "alpha": 0.6, "beta": 0.4,
                                                                "device_rng": True}}}}
    torch.manual_seed(11); np.random.seed(11); random.seed(11)
    actors = create_actors(cfg, torch.device("cuda", 0), device_acting=True, use_graph=True)
    tr = get_registered_type("trainers", "dist_dqn")(logger=NullLogger(), actors=actors, model_config=cfg["model"],
                                                     policy_args=cfg["policy_args"])
    tr.data_parallel = None
    series = {"qloss": [], "grad_norm": []}
    orig = tr.value_log.log

    def tap(key, value, *a, **k):
        if key in series and k.get("group") == "train":
            series[key].append(value.detach().clone() if isinstance(value, torch.Tensor) else torch.tensor(float(value)))
        return orig(key, value, *a, **k)
    tr.value_log.log = tap
    tr.train(**cfg["training"]["args"])
    torch.cuda.synchronize()
    out = {k: torch.stack([t.float().cpu() for t in v]).numpy() for k, v in series.items()}
    out["params"] = [p.detach().cpu().clone() for p in tr.policy.parameters()]
    out["captured"] = tr._gstep is not None and tr._gstep["graph"] is not None
    out["tree"] = tr.history_buffer.tree_nodes()
    tr.history_buffer.close()
    return out


def test_graphed_learner_step_is_the_eager_step(monkeypatch):
    from rltime_amd.models.torch import fused
    monkeypatch.setattr(fused, "_CONV_WRW_MIN_WORK", 0)          # deterministic weight gradients (test_graph_step_gpu.py)
    a, b = _series(True), _series("no-capture")
    assert a["captured"] and not b["captured"]
    assert len(a["qloss"]) == len(b["qloss"]) > 100
    for key in ("qloss", "grad_norm"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        assert np.isfinite(a[key]).all()
    assert all(torch.equal(x, y) for x, y in zip(a["params"], b["params"]))
    for x, y in zip(a["tree"], b["tree"]):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def test_nature_cnn_learner_evaluation_hip_vs_library(monkeypatch):
    """The C51 learner evaluation of synthetic_atari_c51.json's network (nature CNN, FC 512, A * Z = 306 outputs) with
    every product on the hand-written kernels (the settings test_network_ab_gpu.py calls `hip`) against the library
    path (MIRL_GEMM3=0): targets, loss, report and gradients agree."""
    from tests.test_network_ab_gpu import _set_mode
    from rltime_amd.policies.dist_dqn import DistDQNPolicy
    from rltime_amd.spaces import Box, Discrete
    from rltime_amd.training import qops
    from rltime_amd.general.config import load_config
    model = load_config("synthetic_atari_c51.json")["model"]
    torch.manual_seed(3)
    B, A, Z = 256, 6, 51
    pol = DistDQNPolicy.create(model_config=model, observation_space=Box(0, 255, (4, 84, 84), np.uint8),
                               action_space=Discrete(A), num_atoms=Z)
    tgt = DistDQNPolicy.create(model_config=model, observation_space=Box(0, 255, (4, 84, 84), np.uint8),
                               action_space=Discrete(A), num_atoms=Z)
    g = torch.Generator().manual_seed(4)
    x = torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, generator=g).cuda()
    xt = torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, generator=g).cuda()
    r = torch.randint(-1, 2, (B,), generator=g).float().cuda()
    n = torch.ones(B, device="cuda")
    mk = (torch.rand(B, generator=g) > 0.1).float().cuda()
    acts = torch.randint(0, A, (B,), generator=g).cuda()
    w = torch.rand(B, generator=g).cuda()
    outs = {}
    for mode in ("hip", "lib"):
        with monkeypatch.context() as mp:
            _set_mode(mp, mode)
            pol.zero_grad(set_to_none=True)
            with torch.no_grad():
                lt = tgt.predict({"x": xt}, 1)
                ls = pol.predict({"x": xt}, 1)
                y = qops.q_target_c51(lt, ls, pol.support, r, n, mk, 0.99, -10, 10)
            loss, rep = qops.c51_loss(pol.predict({"x": x}, 1), acts, y, w)
            loss.backward()
            torch.cuda.synchronize()
            outs[mode] = dict(y=y.cpu(), loss=float(loss.detach()), rep=rep.cpu(), ls=ls.cpu(),
                              grads={k: p.grad.detach().cpu().clone() for k, p in pol.named_parameters()})
    h, lb = outs["hip"], outs["lib"]
    ev = (torch.softmax(lb["ls"], -1) * pol.support.cpu()).sum(2)
    top = ev.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-5
    assert clear.float().mean() > 0.95
    np.testing.assert_allclose(h["y"][clear].numpy(), lb["y"][clear].numpy(), rtol=0, atol=1e-5)
    assert abs(h["loss"] - lb["loss"]) <= 1e-5 * abs(lb["loss"]) + 1e-6
    np.testing.assert_allclose(h["rep"].numpy(), lb["rep"].numpy(), rtol=1e-4, atol=1e-5)
    gn = lambda d: torch.sqrt(sum((v.double() ** 2).sum() for v in d.values()))  # noqa: E731
    assert abs(gn(h["grads"]) - gn(lb["grads"])) <= 1e-4 * gn(lb["grads"])
    for k in h["grads"]:
        d = (h["grads"][k].double() - lb["grads"][k].double()).norm()
        assert d <= 1e-3 * lb["grads"][k].double().norm() + 1e-7, k


def test_shipped_config_trains(tmp_path):
    """python -m rltime_amd.train synthetic_atari_c51.json, shrunk: a few hundred learner steps, finite losses."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    upd = {"acting": {"actor_envs": 16}, "training": {"args": {
        "mbatch_size": 64, "total_steps": 3200, "warmup_steps": 320, "log_freq": 800, "target_update_freq": 800,
        "history_mode": {"args": {"size": 4000, "train_frequency": 8}}}}}
    rc = subprocess.run([sys.executable, "-m", "rltime_amd.train", "synthetic_atari_c51.json", "--conf-update", json.dumps(upd),
                         "--log-dir", str(tmp_path)], cwd=root, capture_output=True, text=True, timeout=600)
    assert rc.returncode == 0, rc.stderr[-3000:]
    rows = []
    for dirpath, _, files in os.walk(tmp_path):
        for f in files:
            if f.endswith(".json") or f.endswith(".jsonl") or f.endswith(".csv"):
                rows.append(open(os.path.join(dirpath, f)).read())
    text = "\n".join(rows) + rc.stdout
    assert "qloss" in text, text[-2000:]
    assert "nan" not in text.lower().replace("nanos", "")
