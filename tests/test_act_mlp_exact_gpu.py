"""GPU: k_act_mlp (csrc/act_mlp.hip) through mirl_act_mlp_fwd against float64 on every branch of its one loop, `dense_rb`, and
of its head (tests/act_mlp_restate.py; the CPU side of every claim is tests/test_act_mlp_restate_cpu.py).

Every case first asserts, from the launcher's own LDS size, that its shape takes the branch it is named after.

Dyadic operands (integers, cosine features exactly 1, every row's maximum planted on two actions): the q-values equal
float32(float64) with torch.equal and the first of the tied actions wins on every row, need_q = 1 and 0, all thirteen shapes.

Real operands at the seven branch shapes, u = 2^-24, per element (R.forward_bound):
  product     s_j = sum_k x_k w_kj, ascending k, a multiply and an add per term:  e_s = sum_k |w_kj| e_x,k + K u sum_k |x_k w_kj|
  bias        + u |s + b|;  ReLU passes the bound on
  features    the float32 values mirl_cos_embed writes for the same freq and taus, taken as exact
  x = r f     |f| e_r + |r| e_f + u |x|
  head        off = V - m / A: e_V + sum_a e_a / A + u ((A - 1) sum_a |A_a| / A + |m| / A + |off|);  t = A_a + off: e_a + e_off + u |t|;
              q = sum_n t / N: (sum_n e_t + 7 u sum_n |t|) / N + u |q|      (need_q = 0, no value stream: t = A_a, e_t = e_a)
The actions are the float64 arg-max; a row whose two best q-values are closer than their two bounds may take either (at most
one row in eight).  The bar of tests/test_act_mlp_gpu.py (check_bar) is held at these shapes as well."""
import ctypes as C
import functools

import pytest
import torch

from tests import act_mlp_restate as R
from tests import pointwise_restate as PR

pytestmark = pytest.mark.gpu

NAMES = sorted(R.ALL_SHAPES)
BRANCH_NAMES = sorted(R.BRANCH_SHAPES)
PAD = 64


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch_under_guards(dc, **kw):
    """One launch into NaN / -1 filled outputs with a guard tail that must stay untouched -> (actions, q) on the CPU."""
    c = dc.case
    qbuf = torch.full((c.E * c.A + PAD,), float("nan"), device="cuda")
    abuf = torch.full((c.E + PAD,), -1, dtype=torch.int32, device="cuda")
    tbuf = torch.full((c.E * c.N + PAD,), float("nan"), device="cuda")
    dc.launch(actions=abuf, qvalues=qbuf, taus_out=tbuf, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(qbuf[c.E * c.A:]).all()) and bool((abuf[c.E:] == -1).all()), "written past the outputs"
    assert bool(torch.isnan(tbuf[c.E * c.N if c.D else 0:]).all()), "written past the fractions"
    return abuf[:c.E].cpu(), qbuf[:c.E * c.A].view(c.E, c.A).cpu()


@functools.lru_cache(maxsize=None)
def _dyadic(name, need_q):
    R.assert_branches(name)
    case = R.DyadicCase(name, need_q)
    return case, R.DeviceCase(case), R.forward_bound(case, need_q)["q"]


@pytest.mark.parametrize("need_q", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_dyadic_values_are_bit_equal_and_ties_go_to_the_first_maximum(name, need_q):
    case, dc, q64 = _dyadic(name, need_q)
    actions, q = _launch_under_guards(dc, need_q=need_q)
    assert torch.equal(q, q64.float()), "%d of %d q-values differ" % (int((q != q64.float()).sum()), q.numel())
    assert torch.equal(actions.long(), R.first_max(q64))


@functools.lru_cache(maxsize=None)
def _real(name):
    """The case on the device, the cosine features as mirl_cos_embed writes them, and the references of check_bar."""
    from rltime_amd.models.torch.fused import cos_embed
    R.assert_branches(name)
    case = R.Case(name)
    dc = R.DeviceCase(case)
    phi = cos_embed(dc.taus, dc.freq).cpu() if case.D else None
    if case.D:
        assert phi.dtype == torch.float32 and phi.shape == (case.E * case.N, case.D)
    bars = [R.reference(case, dt, device="cuda") for dt in (torch.float64, torch.float32)]
    return case, dc, phi, bars


@pytest.mark.parametrize("need_q", [1, 0])
@pytest.mark.parametrize("name", BRANCH_NAMES)
def test_real_values_within_the_operation_count_bound(name, need_q):
    case, dc, phi, (r64, r32) = _real(name)
    fb = R.forward_bound(case, need_q, phi=phi)
    actions, q = _launch_under_guards(dc, need_q=need_q)
    R.check_bound(q, fb, actions, "%s need_q=%d" % (name, need_q))
    which = 0 if (need_q or not case.dueling) else 1
    print(name, "err, torch f32 err, scale:", R.check_bar(q.cuda(), r64[which], r32[which]))


def test_per_env_exponents_and_the_floor_draw_like_the_actor_head():
    """E = 512, eps = 0.4, a per-env exponent from 0.5 to 8 and eps_min = 0.02 (eps ** expo runs from 0.63 down to 0.0007, the
    floor takes over at expo = 4.27): the actions equal mirl_actor_head_rng's on the same key and the same q-values row for
    row, that kernel's eps_used equals float32(max(eps ** expo, eps_min)), and both equal the host restatement of the remap
    on the Philox block of (seed, step, env)."""
    from rltime_amd._lib import lib, check
    E, eps, eps_min, seed, step_no = 512, 0.4, 0.02, 77, 11
    g = torch.Generator().manual_seed(31)
    case = R.Case("ragged-chunk-of-32")
    case.E, case.obs, case.taus = E, torch.randn(E, case.O, generator=g) * 0.7, torch.rand(E * case.N, generator=g)
    A = case.A
    dc = R.DeviceCase(case)
    expo = torch.linspace(0.5, 8.0, E, dtype=torch.float64)[torch.randperm(E, generator=g)]
    per64 = PR.eps_per_actor(eps, expo, eps_min, E)
    assert int((per64 > eps).sum()) >= 16 and int((per64 == eps_min).sum()) >= 64 and int(((per64 > eps_min) & (per64 < eps)).sum()) >= 64
    xd = expo.cuda()
    greedy, q = dc.launch(seed=seed, step=step_no)
    acts, q_e = dc.launch(seed=seed, step=step_no, eps=eps, expo=xd, eps_min=eps_min)
    assert torch.equal(q.view(torch.int32), q_e.view(torch.int32))
    assert torch.equal(greedy.cpu().long(), R.first_max(q.double().cpu()))
    # the companion kernel on the same q-values
    step = torch.tensor([step_no], dtype=torch.int64, device="cuda")
    ed = torch.tensor(eps, dtype=torch.float64, device="cuda")
    acts2 = torch.full((E,), -1, dtype=torch.int32, device="cuda")
    q2, used = torch.empty(E, A, device="cuda"), torch.full((E,), float("nan"), device="cuda")
    check(lib.mirl_actor_head_rng(E, 1, A, _p(q.contiguous()), A, None, 0, _p(ed), _p(xd), eps_min, seed, _p(step), _p(acts2), _p(q2),
                                  _p(used), _st()), "mirl_actor_head_rng")
    assert torch.equal(acts, acts2)
    assert torch.equal(used.cpu(), per64.float()), "eps_used is not float32(max(eps ** expo, eps_min))"
    # the remap restated on the host
    u, rnd = PR.philox_head_draws(seed, step_no, E, A)
    want = PR.eps_greedy(greedy.cpu().long(), per64.float(), u, rnd)
    assert torch.equal(acts.cpu().long(), want)
    explored = u < per64.float()
    floor = per64 == eps_min
    # both sides of the floor decide rows: some explored only because of it, some not although eps alone would have
    assert int((explored & floor & (u >= PR.eps_per_actor(eps, expo, 0.0, E).float())).sum()) >= 1
    assert int((~explored & (u < eps)).sum()) >= 16 and int((explored & (u >= eps)).sum()) >= 1
    assert int((acts.cpu().long() != greedy.cpu().long()).sum()) >= 8
