"""GPU: k_actor_head (csrc/acting.hip) through mirl_actor_head and mirl_actor_head_rng against the float64 head of
tests/pointwise_restate.py: dueling combine V + A - mean_a A, mean over the N quantile rows, first-maximum argmax, and the
epsilon-greedy remap with the per-actor exponent and eps_min.

Dyadic values (multiples of 1/8, N and A powers of two): every sum and both means are exact, qvalues must equal float64 bit
for bit and the planted tie must go to the first of the two actions.

Real values, first order, u = 2^-24, per (env, quantile row n) and action a:
  m = sum_a A_a (A - 1 additions)          off = V - m / A:   e_off = u ((A - 1) sum_a |A_a| / A + |m| / A + |off|)   (plain head: 0)
  t = A_a + off                            e_t = e_off + u |t|                                                       (plain head: 0)
  q = (sum_n t) / N, a lane adds ceil(N / 64) rows, then 6 shuffle steps:  e_q = (sum_n e_t + (ceil(N / 64) + 6) u sum_n |t|) / N + u |q|
Actions are compared where the two best float64 q-values are further apart than their bounds together (at most 1 % of the
envs may be left out: none at these sizes, asserted from the float64 values alone)."""
import ctypes as C

import pytest
import torch

from tests import pointwise_restate as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ES = (1, 3, 4, 5, 33)


def _lib():
    from rltime_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _head(adv, val, Q=1, pitch=None, eps=None, expo=None, eps_min=0.0, u=None, rnd=None):
    """pitch None: mirl_actor_head; else mirl_actor_head_rng with rows `pitch` floats apart (padding NaN).  val (E, N) sits in
    the first of Q columns.  -> (actions, qvalues, eps_used) on the CPU."""
    L = _lib()
    E, N, A = adv.shape
    if pitch is None:
        ad = adv.float().cuda().contiguous()
    else:
        ad = torch.full((E, N, pitch), float("nan"), device="cuda")
        ad[:, :, :A] = adv.float().cuda()
    vd = None
    if val is not None:
        vd = torch.full((E, N, Q), float("nan"), device="cuda")
        vd[:, :, 0] = val.float().cuda()
    acts = torch.full((E + 1,), -7, dtype=torch.int32, device="cuda")
    q = torch.full((E + 1, A), float("nan"), device="cuda")
    used = torch.full((E + 1,), float("nan"), device="cuda")
    ed = torch.tensor([eps], dtype=torch.float64, device="cuda") if eps is not None else None
    xd = expo.double().cuda() if expo is not None else None
    if pitch is None:
        ud, rd = (u.float().cuda(), rnd.long().cuda()) if u is not None else (None, None)
        L.check(L.lib.mirl_actor_head(E, N, A, _p(ad), _p(vd), Q if val is not None else 0, _p(ed), _p(xd), eps_min, _p(ud), _p(rd),
                                      _p(acts), _p(q), _p(used), _st()), "mirl_actor_head")
    else:
        step = torch.tensor([5], dtype=torch.int64, device="cuda")
        L.check(L.lib.mirl_actor_head_rng(E, N, A, _p(ad), pitch, _p(vd), Q if val is not None else 0, _p(ed), _p(xd), eps_min, 99, _p(step),
                                          _p(acts), _p(q), _p(used), _st()), "mirl_actor_head_rng")
    torch.cuda.synchronize()
    assert int(acts[E]) == -7 and bool(torch.isnan(q[E]).all()) and bool(torch.isnan(used[E]).all()), "the guard row was written"
    return acts[:E].cpu().long(), q[:E].cpu(), used[:E].cpu()


@pytest.mark.parametrize("entry", ["plain-Q1", "plain-Q3", "rng-pitchA", "rng-pitchA+5"])
@pytest.mark.parametrize("case", R.actor_head_dyadic_cases(), ids=lambda c: "E%d-N%d-A%d-d%d" % (c["E"], c["N"], c["A"], c["dueling"]))
def test_dyadic_values_are_bit_equal_and_ties_go_to_the_first_maximum(case, entry):
    d = R.dyadic_actor_head(**case)
    A = case["A"]
    pitch = None if entry.startswith("plain") else (A if entry == "rng-pitchA" else A + 5)
    acts, q, _ = _head(d["adv"], d["val"], Q=3 if entry == "plain-Q3" else 1, pitch=pitch)
    want = R.actor_qvalues(d["adv"], d["val"])
    assert torch.equal(q, want.float()), "%d q-values differ" % int((q != want.float()).sum())
    assert torch.equal(acts, d["first"]) and torch.equal(acts, R.first_max(want))


def _real_cases():
    out, k = [], 0
    for N in (1, 32, 64, 65, 200):
        for A in (1, 6, 8, 9, 18, 30):
            for dueling in (False, True):
                out.append(dict(seed=1900 + k, E=ES[k % 5], N=N, A=A, dueling=dueling, Q=(1, 3)[(k // 2) % 2],
                                entry=("plain", "rng")[(k // 5 + k) % 2]))
                k += 1
    return out


def _real_operands(case):
    """-> (adv, val, float64 q-values, their bounds, envs whose best action is clear of the second best): CPU only."""
    E, N, A = case["E"], case["N"], case["A"]
    g = torch.Generator().manual_seed(case["seed"])
    adv = torch.randn(E, N, A, generator=g).double()
    val = torch.randn(E, N, generator=g).double() if case["dueling"] else None
    want = R.actor_qvalues(adv, val)
    if val is None:
        t, e_t = adv, torch.zeros_like(adv)
    else:
        m = adv.sum(-1, keepdim=True)
        off = val.unsqueeze(-1) - m / A
        e_off = U * ((A - 1) * adv.abs().sum(-1, keepdim=True) / A + m.abs() / A + off.abs())
        t = adv + off
        e_t = e_off + U * t.abs()
    depth = -(-N // 64) + 6
    bound = (e_t.sum(1) + depth * U * t.abs().sum(1)) / N + U * want.abs()
    clear = torch.ones(E, dtype=torch.bool)
    if A >= 2:
        top = want.topk(2, dim=-1)
        rows = torch.arange(E)
        clear = (top.values[:, 0] - top.values[:, 1]) > bound[rows, top.indices[:, 0]] + bound[rows, top.indices[:, 1]]
    return adv, val, want, bound, clear


@pytest.mark.parametrize("case", _real_cases(), ids=lambda c: "E%d-N%d-A%d-d%d-Q%d-%s" % (c["E"], c["N"], c["A"], c["dueling"], c["Q"], c["entry"]))
def test_real_values_within_the_operation_count_bound(case):
    E, A = case["E"], case["A"]
    adv, val, want, bound, clear = _real_operands(case)
    assert int((~clear).sum()) <= E // 100, "pick another seed"
    acts, q, _ = _head(adv, val, Q=case["Q"], pitch=A + 5 if case["entry"] == "rng" else None)
    err = (q.double() - want).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print("RATIO k_actor_head qvalues: worst err / bound = %.3f" % ratio)
    assert bool((err <= bound).all()), "err / bound = %.3f" % ratio
    if A >= 2:
        assert torch.equal(acts[clear], R.first_max(want)[clear])
    else:
        assert int(acts.abs().max()) == 0


@pytest.mark.parametrize("with_expo", [False, True])
def test_epsilon_greedy_on_the_u_rnd_path(with_expo):
    E, N, A = 33, 8, 6
    g = torch.Generator().manual_seed(40 + with_expo)
    adv = torch.randn(E, N, A, generator=g).double()
    greedy = R.first_max(R.actor_qvalues(adv))
    rnd = (greedy + 1 + torch.randint(0, A - 1, (E,), generator=g)) % A          # never the greedy action
    eps, eps_min = 0.4, 0.02
    expo = torch.linspace(1, 8, E, dtype=torch.float64) if with_expo else None
    per64 = R.eps_per_actor(eps, expo, eps_min, E)
    per32 = per64.float()
    if with_expo:
        assert float(per64[0]) == eps and int((per64 == eps_min).sum()) >= 5 and int((per64 > eps_min).sum()) >= 5   # the floor holds
    below, above = torch.nextafter(per32, torch.zeros(E)), torch.nextafter(per32, torch.ones(E))
    u = torch.where(torch.arange(E) % 2 == 0, below, above)
    acts, _, used = _head(adv, None, eps=eps, expo=expo, eps_min=eps_min, u=u, rnd=rnd)
    assert torch.equal(used, per32), "eps_used is not float32(max(eps ** expo, eps_min))"
    assert torch.equal(acts, R.eps_greedy(greedy, per32, u, rnd))
    assert torch.equal(acts[::2], rnd[::2]) and torch.equal(acts[1::2], greedy[1::2])
    # u == eps is not below it: the greedy action stays
    acts, _, _ = _head(adv, None, eps=eps, expo=expo, eps_min=eps_min, u=used, rnd=rnd)
    assert torch.equal(acts, greedy)
    # eps NULL: greedy, eps_used untouched
    acts, _, used = _head(adv, None, eps=None, u=torch.zeros(E), rnd=rnd)
    assert torch.equal(acts, greedy) and bool(torch.isnan(used).all())


def test_rng_entry_with_eps_draws_valid_actions_and_reports_eps():
    E, N, A = 33, 8, 6
    g = torch.Generator().manual_seed(44)
    adv = torch.randn(E, N, A, generator=g).double()
    expo = torch.linspace(1, 8, E, dtype=torch.float64)
    acts, q, used = _head(adv, None, pitch=A + 5, eps=0.9, expo=expo, eps_min=0.05)
    assert torch.equal(used, R.eps_per_actor(0.9, expo, 0.05, E).float())
    assert int(acts.min()) >= 0 and int(acts.max()) < A and bool((acts != R.first_max(R.actor_qvalues(adv))).any())


def test_entry_points_refuse_bad_arguments():
    L = _lib()
    x = torch.zeros(64, device="cuda")
    i32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    e64 = torch.zeros(8, dtype=torch.float64, device="cuda")
    P, I, D, st = _p(x), _p(i32), _p(e64), _st()
    plain = [2, 2, 2, P, None, 0, None, None, 0.0, None, None, I, P, None, st]
    for pos, bad in [(0, 0), (1, 0), (2, -1), (3, None), (11, None), (12, None)]:
        a = list(plain)
        a[pos] = bad
        assert L.lib.mirl_actor_head(*a) == -1, pos
    a = list(plain)
    a[6] = D                                                           # eps without u / rnd
    assert L.lib.mirl_actor_head(*a) == -1
    a = list(plain)
    a[4], a[5] = P, 0                                                  # a value stream without its pitch
    assert L.lib.mirl_actor_head(*a) == -1
    rng = [2, 2, 2, P, 2, None, 0, None, None, 0.0, 1, None, I, P, None, st]
    for pos, bad in [(0, 0), (1, -2), (2, 0), (3, None), (4, 1), (12, None), (13, None)]:
        a = list(rng)
        a[pos] = bad
        assert L.lib.mirl_actor_head_rng(*a) == -1, pos
    a = list(rng)
    a[7] = D                                                           # eps without the step counter
    assert L.lib.mirl_actor_head_rng(*a) == -1
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0 and int(i32.abs().max()) == 0
