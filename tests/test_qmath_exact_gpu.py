"""GPU: the target and loss kernels of csrc/qmath.hip (with vfscale.hpp) at their C entry points against the float64
restatements of tests/pointwise_restate.py (proved on the CPU by tests/test_pointwise_restate_cpu.py).

Bit-exact cases: theta, y multiples of 1/2 in [-2, 2], tau multiples of 1/16, kappa in {0.5, 1, 2}, weights and row_scale
powers of two, N * Nt <= 8192, gamma = 1, vf_eps off.  Every product and every partial sum is then a float32 number, so the
kernel must give float32(float64 result) whatever its summation order.  The only roundings are single divisions by a
count: row_loss = fl(sum / Nt) * w, abs_td = fl(sum / (Nt N)), the selection mean fl(sum / Ns), and the gradient factor,
which the kernels form as c = fl(w * row_scale / Nt) before dz = fl(gsum * c): the expected gradient repeats exactly these
two roundings on the exact gsum of the restatement.  Outputs are pre-filled with NaN and one guard row longer than needed.

Real operands (randn * 2, gamma in {0.97, 0.99}, n in 1..5, masks 0 / 1, vf_eps in {none, 1e-3, 1e-2}, M = 257): first-order
bounds from the kernels' own operation count, u = 2^-24, powf within 1 ulp (2u relative):

  target, vf_eps off   x = disc * v * mask, t = ret + x:   e_t = 3u |x| + u |t|                 (powf 2u, one product, one sum)
  target, vf_eps on    v' = float32(h^-1(v)):              e_v = u |v'| + 8 * 2^-53 * B         (B = the sum of the magnitudes of
                                                           the three terms of the closed form, which cancel in float64)
                       t as above from v':                 e_t = disc mask e_v + 3u |x| + u |t|
                       y = s (sqrtf(|t| + 1) - 1) + eps t: e_y = (1/2 + eps) e_t + u (3/2 r + |r - 1| + 2 eps |t| + |y|),  r = sqrt(|t| + 1)
                       (|t| + 1 rounded: u r / 2 through the root; the root: u r; the difference; float32(eps) and eps t; the sum)
  IQN selection mean   fl(sum_n z / Ns):                   e_a = u ((Ns - 1) sum_n |z_na| / Ns + |mean_a|); a row whose two best
                       float64 means are closer than e_best + e_second may take either action (at most 1 % of the rows)
  DQN loss             td = q - y: u |td|; huber: e_val = u (3 val + kappa |td|) (quadratic: td twice and one product; linear:
                       |td|, the difference, the product); mse: 3u val; row = val w: w e_val + u |row|; dq = grad w row_scale: 3u |dq|
  IQN loss, per pair   l = pen val / kappa:                e_l = pen e_val / kappa + 3u l      (tau - 1, product, division)
           row_loss    (w / Nt) (sum e_l + d u sum l) + 2u |row|      d = summation depth: wave kernel ceil(Nt / parts) + 6,
                                                                      generic kernel Nt + ceil(N / 64) + 6
           abs_td      u (d + 1) mean |td| + u |abs_td|
           dz          |c| (4u + d_g u) sum_i |g_i| + 3u |dz|,  g = pen huber' / kappa, d_g = ceil(Nt / parts) + log2(parts) (wave), Nt (generic)
  Gradients are compared where no pair of the element lies within 2u |td| of the Huber kink (the derivative is continuous
  there; the rows left out are at most 1 % of M, asserted from the float64 reference alone).  td = y - theta of two float32
  numbers has the sign of the exact difference, so no pair can cross td = 0."""
import ctypes as C
import math

import pytest
import torch

from tests import pointwise_restate as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ERR_ARG = -1


def _lib():
    from rltime_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype=torch.float32):
    return None if t is None else t.to(dtype).cuda().contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _guard_ok(*bufs):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(b[-1]).all()) for b in bufs)


def _report(what, err, bound):
    ratio = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print("RATIO %s: worst err / bound = %.3f" % (what, ratio))
    return ratio


def _within(what, got, want64, bound, keep=None):
    err = (got.cpu().double() - want64).abs()
    if keep is not None:
        err, bound = err[keep], bound[keep]
    ratio = _report(what, err, bound)
    assert bool((err <= bound).all()), "%s: err / bound = %.3f" % (what, ratio)


# ---- calls -------------------------------------------------------------------------------------------------------------------
def _loss_iqn(z, taus, actions, targets, weights, kappa, row_scale):
    L = _lib()
    M, N, A = z.shape
    Nt = targets.shape[1]
    zd, td_, yd, wd, ad = _dev(z), _dev(taus), _dev(targets), _dev(weights), actions.cuda()
    row, rep, dz = _nan(M + 1), _nan(M + 1), _nan(M + 1, N, A)
    L.check(L.lib.mirl_loss_iqn(M, N, Nt, A, _p(zd), _p(td_), _p(ad), _p(yd), _p(wd), kappa, row_scale, _p(row), _p(dz), _p(rep), _st()), "mirl_loss_iqn")
    assert _guard_ok(row, rep, dz), "the guard row was written"
    return row[:M].cpu(), rep[:M].cpu(), dz[:M].cpu()


def _loss_dqn(q, actions, targets, weights, kappa, mode, row_scale):
    L = _lib()
    M, A = q.shape
    qd, yd, wd, ad = _dev(q), _dev(targets), _dev(weights), actions.cuda()
    row, td, dq = _nan(M + 1), _nan(M + 1), _nan(M + 1, A)
    L.check(L.lib.mirl_loss_dqn(M, A, _p(qd), _p(ad), _p(yd), _p(wd), kappa, 1 if mode == "mse" else 0, row_scale, _p(row), _p(dq), _p(td), _st()), "mirl_loss_dqn")
    assert _guard_ok(row, td, dq), "the guard row was written"
    return row[:M].cpu(), td[:M].cpu(), dq[:M].cpu()


def _target_iqn(zt, zs, ret, ns, mk, gamma, vf_eps):
    L = _lib()
    M, Nt, A = zt.shape
    a = [_dev(t) for t in (zt, zs, ret, ns, mk)]
    out = _nan(M + 1, Nt)
    L.check(L.lib.mirl_q_target_iqn(M, Nt, zs.shape[1], A, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), gamma, vf_eps or 0.0, _p(out), _st()), "mirl_q_target_iqn")
    assert _guard_ok(out), "the guard row was written"
    return out[:M].cpu()


def _target_dqn(qt, qs, ret, ns, mk, gamma, vf_eps):
    L = _lib()
    M, A = qt.shape
    a = [_dev(t) for t in (qt, qs, ret, ns, mk)]
    out = _nan(M + 1)
    L.check(L.lib.mirl_q_target_dqn(M, A, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), gamma, vf_eps or 0.0, _p(out), _st()), "mirl_q_target_dqn")
    assert _guard_ok(out), "the guard row was written"
    return out[:M].cpu()


# ---- bit-exact ---------------------------------------------------------------------------------------------------------------
def _iqn_loss_exact(case):
    d = R.dyadic_loss_iqn(**case)
    M, N, Nt, A = case["M"], case["N"], case["Nt"], case["A"]
    row, rep, dz = _loss_iqn(d["z"], d["taus"], d["actions"], d["targets"], d["weights"], d["kappa"], d["row_scale"])
    s = R.iqn_pairs(d["z"], d["taus"], d["actions"], d["targets"], d["kappa"])
    w = torch.ones(M, dtype=torch.float64) if d["weights"] is None else d["weights"]
    want_row = (s["loss_sum"] / Nt).float() * w.float()
    want_rep = (s["abs_sum"] / (Nt * N)).float()
    c32 = (w * d["row_scale"]).float() / torch.tensor(float(Nt), dtype=torch.float32)           # one float32 division
    want_dz = torch.zeros(M, N, A)
    want_dz[torch.arange(M), :, d["actions"]] = (s["gsum"] * c32.double().unsqueeze(1)).float()
    assert torch.equal(row, want_row), "row_loss: %d rows differ" % int((row != want_row).sum())
    assert torch.equal(rep, want_rep), "abs_td: %d rows differ" % int((rep != want_rep).sum())
    assert torch.equal(dz, want_dz), "dz: %d elements differ" % int((dz != want_dz).sum())
    off = torch.ones(M, N, A, dtype=torch.bool)
    off[torch.arange(M), :, d["actions"]] = False
    assert float(dz[off].abs().max() if off.any() else 0.0) == 0.0
    assert bool((s["gsum"] != 0).any()) and bool((dz[~off] != 0).any())


_ID_IQN = lambda c: "N%d-Nt%d-A%d-M%d-k%g-%s-w%d" % (c["N"], c["Nt"], c["A"], c["M"], c["kappa"], c["acted"], c["weights"])  # noqa: E731


@pytest.mark.parametrize("case", R.loss_iqn_wave_cases(), ids=_ID_IQN)
def test_loss_iqn_wave_kernel_is_bit_equal_to_float64(case):
    assert case["N"] <= 64 and case["Nt"] <= 64 and 64 % case["N"] == 0          # the shapes mirl_loss_iqn gives k_loss_iqn_wave
    _iqn_loss_exact(case)


@pytest.mark.parametrize("case", R.loss_iqn_generic_cases(), ids=_ID_IQN)
def test_loss_iqn_generic_kernel_is_bit_equal_to_float64(case):
    assert case["N"] > 64 or case["Nt"] > 64 or 64 % case["N"]                   # ... and k_loss_iqn
    _iqn_loss_exact(case)


@pytest.mark.parametrize("case", R.loss_dqn_cases(), ids=lambda c: "A%d-M%d-%s-w%d" % (c["A"], c["M"], c["mode"], c["weights"]))
def test_loss_dqn_is_bit_equal_to_float64(case):
    d = R.dyadic_loss_dqn(case["seed"], case["M"], case["A"], case["kappa"], case["weights"])
    row, td, dq = _loss_dqn(d["q"], d["actions"], d["targets"], d["weights"], d["kappa"], case["mode"], d["row_scale"])
    want = R.dqn_loss(d["q"], d["actions"], d["targets"], d["weights"], d["kappa"], case["mode"], d["row_scale"])
    for name, got, w64 in zip(("row_loss", "td", "dq"), (row, td, dq), want):
        assert torch.equal(w64.float().double(), w64), name
        assert torch.equal(got, w64.float()), "%s: %d elements differ" % (name, int((got != w64.float()).sum()))
    assert bool((dq != 0).any()) and int((dq != 0).sum(1).max()) == 1


@pytest.mark.parametrize("case", R.target_iqn_cases(), ids=lambda c: "Ns%d-Nt%d-A%d-M%d" % (c["Ns"], c["Nt"], c["A"], c["M"]))
def test_target_iqn_is_bit_equal_to_float64(case):
    d = R.dyadic_target_iqn(**case)
    got = _target_iqn(d["zt"], d["zs"], d["returns"], d["nsteps"], d["masks"], 1.0, None)
    want = R.nstep_target(R.iqn_bootstrap(d["zt"], d["zs"]), d["returns"], d["nsteps"], d["masks"], 1.0, None)
    assert torch.equal(got, want.float()), "%d targets differ" % int((got != want.float()).sum())


def test_target_iqn_lds_limit():
    """Ns * A + A = 4096 floats per wave (64 KiB per workgroup) is accepted and right; 4097 is refused before any launch."""
    L = _lib()
    d = R.dyadic_target_iqn(seed=77, M=5, Nt=3, Ns=63, A=64)
    got = _target_iqn(d["zt"], d["zs"], d["returns"], d["nsteps"], d["masks"], 1.0, None)
    want = R.nstep_target(R.iqn_bootstrap(d["zt"], d["zs"]), d["returns"], d["nsteps"], d["masks"], 1.0, None)
    assert torch.equal(got, want.float())
    M, Nt, Ns, A = 2, 3, 4096, 1
    zt, zs = torch.zeros(M, Nt, A, device="cuda"), torch.zeros(M, Ns, A, device="cuda")
    v = torch.ones(M, device="cuda")
    out = _nan(M, Nt)
    rc = L.lib.mirl_q_target_iqn(M, Nt, Ns, A, _p(zt), _p(zs), _p(v), _p(v), _p(v), 1.0, 0.0, _p(out), _st())
    torch.cuda.synchronize()
    assert rc == ERR_ARG and "LDS" in L.last_error()
    assert bool(torch.isnan(out).all()), "a refused call wrote its output"


@pytest.mark.parametrize("case", R.target_dqn_cases(), ids=lambda c: "A%d-M%d" % (c["A"], c["M"]))
def test_target_dqn_is_bit_equal_to_float64(case):
    d = R.dyadic_target_dqn(**case)
    got = _target_dqn(d["qt"], d["qs"], d["returns"], d["nsteps"], d["masks"], 1.0, None)
    want = R.nstep_target(R.dqn_bootstrap(d["qt"], d["qs"]), d["returns"], d["nsteps"], d["masks"], 1.0, None)
    assert torch.equal(got, want.float()), "%d targets differ" % int((got != want.float()).sum())


def test_entry_points_refuse_null_pointers_and_empty_sizes():
    L = _lib()
    f = torch.zeros(64, device="cuda")
    i64 = torch.zeros(8, dtype=torch.int64, device="cuda")
    out = _nan(64)
    P, I, O, st = _p(f), _p(i64), _p(out), _st()
    calls = {     # name -> (argument list, positions of the sizes, positions of the required pointers)
        "mirl_q_target_dqn": ([2, 2, P, P, P, P, P, 1.0, 0.0, O, st], (0, 1), (2, 3, 4, 5, 6, 9)),
        "mirl_q_target_iqn": ([2, 2, 2, 2, P, P, P, P, P, 1.0, 0.0, O, st], (0, 1, 2, 3), (4, 5, 6, 7, 8, 11)),
        "mirl_loss_dqn": ([2, 2, P, I, P, None, 1.0, 0, 1.0, O, O, O, st], (0, 1), (2, 3, 4, 9, 10, 11)),
        "mirl_loss_iqn": ([2, 2, 2, 2, P, P, I, P, None, 1.0, 1.0, O, O, O, st], (0, 1, 2, 3), (4, 5, 6, 7, 11, 12, 13)),
    }
    for name, (args, sizes, ptrs) in calls.items():
        fn = getattr(L.lib, name)
        for pos in sizes:
            for bad in (0, -1):
                a = list(args)
                a[pos] = bad
                assert fn(*a) == ERR_ARG, (name, pos, bad)
                assert "bad" in L.last_error()
        for pos in ptrs:
            a = list(args)
            a[pos] = None
            assert fn(*a) == ERR_ARG, (name, pos)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote its output"


# ---- real operands -----------------------------------------------------------------------------------------------------------
SHAPES = [(32, 32, 6), (8, 64, 18), (70, 5, 9)]
M_REAL = 257


def _real(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 2).double()          # float32 numbers, held in float64


def _tail(seed, M):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, generator=g).double(), torch.randint(1, 6, (M,), generator=g).double(),
            torch.randint(0, 2, (M,), generator=g).double())


def _target_bound(v, ret, ns, mk, gamma, eps):
    """-> (float64 target, bound) of the tail on the bootstrap values v, following the module docstring."""
    if v.dim() == 2:
        ret, ns, mk = (t.unsqueeze(-1) for t in (ret, ns, mk))
    disc = torch.pow(torch.full_like(ns, R.gamma32(gamma)), ns)
    if eps:
        a = v.abs()
        big = a / eps + torch.sqrt(4 * eps * a + (2 * eps + 1) ** 2) / (2 * eps ** 2) + (2 * eps + 1) / (2 * eps ** 2)
        vu = R.vf_unscale(v, eps)
        e_v = U * vu.abs() + 8 * 2.0 ** -53 * big
    else:
        vu, e_v = v, torch.zeros_like(v)
    x = disc * vu * mk
    t = ret + x
    e_t = disc * mk * e_v + 3 * U * x.abs() + U * t.abs()
    if not eps:
        return t, e_t
    r = torch.sqrt(t.abs() + 1)
    y = R.vf_scale(t, eps)
    return y, (0.5 + eps) * e_t + U * (1.5 * r + (r - 1).abs() + 2 * eps * t.abs() + y.abs())


@pytest.mark.parametrize("vf_eps", [None, 1e-3, 1e-2])
@pytest.mark.parametrize("gamma", [0.97, 0.99])
@pytest.mark.parametrize("N,Nt,A", SHAPES)
def test_real_targets_within_the_operation_count_bound(N, Nt, A, gamma, vf_eps):
    M = M_REAL
    seed = 1000 + N + A
    ret, ns, mk = _tail(seed, M)
    # DQN: the selection compares the inputs themselves, no rounding and no ambiguity
    qt, qs = _real(seed + 1, M, A), _real(seed + 2, M, A)
    want, bound = _target_bound(R.dqn_bootstrap(qt, qs), ret, ns, mk, gamma, vf_eps)
    assert torch.allclose(want, R.nstep_target(R.dqn_bootstrap(qt, qs), ret, ns, mk, gamma, vf_eps), rtol=0, atol=0)
    _within("k_target_dqn", _target_dqn(qt, qs, ret, ns, mk, gamma, vf_eps), want, bound)
    # IQN: argmax of a float32 mean; rows whose two best float64 means are closer than their bounds may take either action
    zt, zs = _real(seed + 3, M, Nt, A), _real(seed + 4, M, N, A)
    mean = zs.sum(1) / N
    e_mean = U * ((N - 1) * zs.abs().sum(1) / N + mean.abs())
    top = mean.topk(2, dim=-1)
    rows = torch.arange(M)
    unclear = (top.values[:, 0] - top.values[:, 1]) < e_mean[rows, top.indices[:, 0]] + e_mean[rows, top.indices[:, 1]]
    assert int(unclear.sum()) <= M // 100, "pick another seed: %d near-ties" % int(unclear.sum())
    assert torch.equal(top.indices[:, 0][~unclear], R.iqn_select(zs)[~unclear])
    got = _target_iqn(zt, zs, ret, ns, mk, gamma, vf_eps).double()
    want, bound = _target_bound(R.iqn_bootstrap(zt, zs, top.indices[:, 0]), ret, ns, mk, gamma, vf_eps)
    want2, bound2 = _target_bound(R.iqn_bootstrap(zt, zs, top.indices[:, 1]), ret, ns, mk, gamma, vf_eps)
    err, err2 = (got - want).abs(), (got - want2).abs()
    ok = (err <= bound).all(1) | (unclear & (err2 <= bound2).all(1))
    ratio = _report("k_target_iqn", err[~unclear], bound[~unclear])
    assert bool(ok.all()), "k_target_iqn: err / bound = %.3f" % ratio


@pytest.mark.parametrize("mode", ["huber", "mse"])
@pytest.mark.parametrize("kappa", [0.5, 1.0])
@pytest.mark.parametrize("A", [6, 18, 9])
def test_real_dqn_loss_within_the_operation_count_bound(A, kappa, mode):
    M = M_REAL
    seed = 2000 + A
    q, y = _real(seed, M, A), _real(seed + 1, M)
    g = torch.Generator().manual_seed(seed + 2)
    act = torch.randint(0, A, (M,), generator=g)
    w = (torch.rand(M, generator=g) + 0.5).double()
    rs = 1.0 / M
    rs32 = float(torch.tensor(rs, dtype=torch.float32))                 # the entry point takes a double and rounds it once
    row, td, dq = _loss_dqn(q, act, y, w, kappa, mode, rs)
    want_row, want_td, want_dq = R.dqn_loss(q, act, y, w, kappa, mode, rs32)
    a = want_td.abs()
    val = want_row / w
    e_val = 3 * U * val if mode == "mse" else U * (3 * val + kappa * a)
    _within("k_loss_dqn td", td, want_td, U * a)
    _within("k_loss_dqn row_loss", row, want_row, w * e_val + U * want_row.abs())
    near = (a - kappa).abs() <= 2 * U * a if mode == "huber" else torch.zeros(M, dtype=torch.bool)
    assert int(near.sum()) <= M // 100
    _within("k_loss_dqn dq", dq, want_dq, 3 * U * want_dq.abs(), keep=~near)
    assert bool((dq != 0).sum(1).le(1).all())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kappa", [0.5, 1.0])
@pytest.mark.parametrize("N,Nt,A", SHAPES)
def test_real_iqn_loss_within_the_operation_count_bound(N, Nt, A, kappa, weighted):
    M = M_REAL
    seed = 3000 + N + A
    z, y = _real(seed, M, N, A), _real(seed + 1, M, Nt)
    g = torch.Generator().manual_seed(seed + 2)
    taus = torch.rand(M, N, generator=g).double()
    act = torch.randint(0, A, (M,), generator=g)
    w = (torch.rand(M, generator=g) + 0.5).double() if weighted else None
    rs = 1.0 / M
    rs32 = float(torch.tensor(rs, dtype=torch.float32))
    row, rep, dz = _loss_iqn(z, taus, act, y, w, kappa, rs)
    want_row, want_rep, want_dz = R.iqn_loss(z, taus, act, y, w, kappa, rs32)
    s = R.iqn_pairs(z, taus, act, y, kappa)
    wave = N <= 64 and Nt <= 64 and 64 % N == 0
    parts = 64 // N if wave else 1
    per = -(-Nt // parts)
    d = per + 6 if wave else Nt + -(-N // 64) + 6
    d_g = per + int(math.log2(parts)) if wave else Nt
    a = s["td"].abs()
    val, _ = R.huber(s["td"], kappa)
    pen = (taus.view(M, 1, N) - (s["td"] < 0).double()).abs()
    e_l = pen * (U * (3 * val + kappa * a)) / kappa + 3 * U * s["loss_terms"]
    w1 = torch.ones(M, dtype=torch.float64) if w is None else w
    _within("k_loss_iqn%s row_loss" % ("_wave" if wave else ""), row, want_row,
            w1 / Nt * (e_l.sum((1, 2)) + d * U * s["loss_sum"]) + 2 * U * want_row.abs())
    _within("k_loss_iqn%s abs_td" % ("_wave" if wave else ""), rep, want_rep, U * (d + 1) * want_rep + U * want_rep)
    c = (w1 * rs32 / Nt).unsqueeze(1)
    theta_bound = c * (4 * U + d_g * U) * s["g_terms"].abs().sum(1)                     # (M, N)
    rows = torch.arange(M)
    bound = torch.zeros(M, N, A, dtype=torch.float64)
    bound[rows, :, act] = theta_bound + 3 * U * want_dz[rows, :, act].abs()
    near = ((a - kappa).abs() <= 2 * U * a).any(1)                                      # (M, N): a pair of theta_j on the kink
    assert int(near.any(1).sum()) <= M // 100, "pick another seed"
    keep = torch.ones(M, N, A, dtype=torch.bool)
    keep[rows, :, act] = ~near
    _within("k_loss_iqn%s dz" % ("_wave" if wave else ""), dz, want_dz, bound, keep=keep)
