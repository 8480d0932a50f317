"""No GPU: tests/pointwise_restate.py is what it claims to be.  Targets and losses equal oracle/qmath.py run in float64,
gradients equal float64 autograd of the plain expression, the Adam step equals clip_grad_norm_ + torch.optim.Adam, the cell
equals torch.nn.LSTMCell with masked state and its autograd, the actor head equals the plain torch expression, the acting
network's layers (conv + ReLU over channels-last frames, linear, quantile-embedding product, output shares) equal torch's in
float64; and the dyadic operands of the bit-exact GPU tests keep every sum exact in float32 and hold the ties and kinks they promise.
The LSTM time loop (forward sweep and its backward) equals a torch.nn.LSTMCell loop with per-step resets and its autograd; the
selector W_hh has the properties it promises; and the bounds of tests/test_lstm_seq_exact_gpu.py are kept by a float32 evaluation
of the kernels' forms and broken by each of five planted single-step errors.
The acting step's bookkeeping (pre-step, episode statistics, frame-stack shift, synthetic env draws, frame conversion) gives the
arrays worked out by hand for small cases, and the stack shift equals the synthetic env's torch expression of it."""
import numpy as np
import pytest
import torch

from oracle import qmath
from tests import pointwise_restate as R
from tests import test_lstm_seq_exact_gpu as SQ         # the sweeps' derived bounds and input families (imports no GPU code)

F64 = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=1e-13):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ---- targets -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vf_eps", [None, 1e-3, 1e-2])
@pytest.mark.parametrize("gamma", [0.97, 0.99])
def test_targets_equal_the_oracle_in_float64(vf_eps, gamma):
    g = _g(1)
    M, N, Nt, A = 37, 8, 5, 6
    ret, mk = torch.randn(M, generator=g, dtype=F64), torch.randint(0, 2, (M,), generator=g).double()
    ns = torch.randint(1, 6, (M,), generator=g).double()
    qt, qs = torch.randn(M, A, generator=g, dtype=F64) * 2, torch.randn(M, A, generator=g, dtype=F64) * 2
    qs[0, 1] = qs[0, 4] = 9.0                                         # a tie: the first maximum
    g32 = R.gamma32(gamma)
    want = qmath.nstep_target(qmath.dqn_bootstrap(qt, qs), ret, mk, ns, g32, vf_eps)
    got = R.nstep_target(R.dqn_bootstrap(qt, qs), ret, ns, mk, gamma, vf_eps, round32=True)
    assert want.dtype == F64 and torch.equal(got, want)
    assert int(R.first_max(qs)[0]) == 1
    zt, zs = torch.randn(M, Nt, A, generator=g, dtype=F64) * 2, torch.randn(M, N, A, generator=g, dtype=F64) * 2
    want = qmath.nstep_target(qmath.iqn_bootstrap(zt, zs), ret, mk, ns, g32, vf_eps)
    got = R.nstep_target(R.iqn_bootstrap(zt, zs), ret, ns, mk, gamma, vf_eps, round32=True)
    assert torch.equal(got, want)
    # without the reference's float32 rounding of h^-1 the target moves by that rounding through h (slope <= 1/2 + eps)
    full = R.nstep_target(R.iqn_bootstrap(zt, zs), ret, ns, mk, gamma, vf_eps)
    v = R.vf_unscale(R.iqn_bootstrap(zt, zs), vf_eps)
    assert bool(((full - got).abs() <= 2.0 ** -24 * v.abs() * (0.5 + (vf_eps or 0)) + 1e-15).all())
    if vf_eps:                                                        # h^-1 inverts h
        x = torch.randn(100, generator=g, dtype=F64) * 30
        _close(R.vf_unscale(R.vf_scale(x, vf_eps), vf_eps), x, 1e-9)


def test_first_max_is_argmax_with_ties():
    q = torch.tensor([[1., 3., 3., 2.], [5., 5., 5., 5.], [0., -1., 0., 0.], [-2., -3., -1., -1.]], dtype=F64)
    assert R.first_max(q).tolist() == [1, 0, 0, 2] == q.argmax(-1).tolist()


# ---- losses ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["huber", "mse"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kappa", [0.5, 1.0, 2.0])
def test_dqn_loss_equals_the_oracle_and_autograd(mode, weighted, kappa):
    g = _g(2)
    M, A = 41, 5
    q, y = torch.randn(M, A, generator=g, dtype=F64) * 2, torch.randn(M, generator=g, dtype=F64)
    act = torch.randint(0, A, (M,), generator=g)
    w = torch.rand(M, generator=g, dtype=F64) + 0.5 if weighted else None
    q[0, act[0]], q[1, act[1]], q[2, act[2]] = y[0], y[1] + kappa, y[2] - kappa       # on the kinks
    rs = 0.37
    rows, td, dq = R.dqn_loss(q, act, y, w, kappa, mode, rs)
    q1 = q.clone().requires_grad_(True)
    loss, td_o = qmath.dqn_loss(q1, act, y, w, kappa, mode, 1, "sum", None)
    assert torch.equal(td, td_o) and abs(float(rows.sum() - loss.detach())) <= 1e-12 * float(loss.detach().abs())
    (loss * rs).backward()
    _close(dq, q1.grad)
    if mode == "huber":                                               # |td| == kappa is the quadratic branch, value and slope
        assert float(rows[1]) == 0.5 * kappa * kappa * (float(w[1]) if weighted else 1.0) and float(rows[0]) == 0.0
        assert float(dq[1, act[1]]) == kappa * (float(w[1]) if weighted else 1.0) * rs


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kappa", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("N,Nt", [(8, 8), (5, 7), (70, 3)])
def test_iqn_loss_equals_the_oracle_and_autograd(N, Nt, kappa, weighted):
    g = _g(3)
    M, A = 19, 4
    z, y = torch.randn(M, N, A, generator=g, dtype=F64) * 2, torch.randn(M, Nt, generator=g, dtype=F64) * 2
    taus = torch.rand(M, N, generator=g, dtype=F64)
    act = torch.randint(0, A, (M,), generator=g)
    w = torch.rand(M, generator=g, dtype=F64) + 0.5 if weighted else None
    z[0, 0, act[0]] = y[0, 0]                                          # td == 0
    z[1, 0, act[1]] = y[1, 0] - kappa                                  # td == +kappa
    z[2, 0, act[2]] = y[2, 0] + kappa                                  # td == -kappa
    rs = 1.7
    rows, rep, dz = R.iqn_loss(z, taus, act, y, w, kappa, rs)
    z1 = z.clone().requires_grad_(True)
    loss, rep_o = qmath.iqn_loss(z1, taus.reshape(-1), act, y, w, kappa, 1, "sum", None)
    _close(rep, rep_o)
    assert abs(float(rows.sum() - loss.detach())) <= 1e-12 * float(loss.detach().abs())
    (loss * rs).backward()
    _close(dz, z1.grad)
    # on the kinks: td == 0 has penalty tau and gradient 0, |td| == kappa the quadratic value kappa / 2 (per kappa)
    s = R.iqn_pairs(z, taus, act, y, kappa)
    assert float(s["td"][0, 0, 0]) == 0.0 and float(s["loss_terms"][0, 0, 0]) == 0.0 and float(s["g_terms"][0, 0, 0]) == 0.0
    assert float(s["loss_terms"][1, 0, 0]) == float(taus[1, 0] * (0.5 * kappa * kappa) / kappa)
    assert float(s["loss_terms"][2, 0, 0]) == float((taus[2, 0] - 1).abs() * (0.5 * kappa * kappa) / kappa)
    assert float(s["g_terms"][1, 0, 0]) == float(taus[1, 0] * kappa / kappa)


# ---- clip + Adam -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, 0.05, 40.0])
def test_adam_step_equals_clip_grad_norm_and_torch_adam(clip):
    g = _g(4)
    sizes = [7, 130, 33]
    lr, b1, b2, eps = 2.5e-4, 0.9, 0.999, 1.5e-4
    ref = [torch.nn.Parameter(torch.randn(n, generator=g, dtype=F64)) for n in sizes]
    opt = torch.optim.Adam(ref, lr=lr, betas=(b1, b2), eps=eps)
    state = [[p.detach().clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64), 0] for p, n in zip(ref, sizes)]
    for step in range(3):
        grads = [torch.randn(n, generator=g, dtype=F64) * (0.3 if step % 2 else 0.01) for n in sizes]
        live = [not (step == 1 and i == 1) for i in range(3)]                       # parameter 1 sits step 1 out
        for p, gr, lv in zip(ref, grads, live):
            p.grad = gr.clone() if lv else None
        norm = R.global_norm([gr for gr, lv in zip(grads, live) if lv])
        if clip is not None:
            total = torch.nn.utils.clip_grad_norm_(ref, clip)
            assert abs(float(total) - norm) <= 1e-13 * norm
        opt.step()
        coef = R.clip_coef(norm, clip)
        for i, (st, gr, lv) in enumerate(zip(state, grads, live)):
            if lv:
                st[0], gc, st[1], st[2], st[3] = R.adam_step(st[0], gr, st[1], st[2], st[3], lr, b1, b2, eps, coef)
                _close(gc, ref[i].grad)
            _close(st[0], ref[i].detach(), 1e-12)
            if opt.state[ref[i]]:
                _close(st[1], opt.state[ref[i]]["exp_avg"])
                _close(st[2], opt.state[ref[i]]["exp_avg_sq"])
                assert float(opt.state[ref[i]]["step"]) == st[3]
    assert [st[3] for st in state] == [3, 2, 3]
    assert R.clip_coef(3.0, 0) == 1.0 and R.clip_coef(3.0, None) == 1.0


# ---- LSTM cell ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", [(1, 1), (3, 5), (7, 37)])
def test_cell_equals_torch_lstmcell_with_masked_state_and_its_autograd(B, H):
    g = _g(5)
    cell = torch.nn.LSTMCell(4 * H, H).double()
    with torch.no_grad():                                             # gates = x: W_ih = I, W_hh = 0, no bias
        cell.weight_ih.copy_(torch.eye(4 * H, dtype=F64))
        cell.weight_hh.zero_(), cell.bias_ih.zero_(), cell.bias_hh.zero_()
    pre = (torch.randn(B, 4 * H, generator=g, dtype=F64) * 2).requires_grad_(True)
    c_prev = torch.randn(B, H, generator=g, dtype=F64)
    keep, keep_next = (torch.rand(B, generator=g) > 0.4).double(), (torch.rand(B, generator=g) > 0.4).double()
    keep_next[0] = 0.0
    c_in = (c_prev * keep.unsqueeze(1)).requires_grad_(True)          # the masked state the step is given
    h, c = cell(pre, (torch.zeros(B, H, dtype=F64), c_in))
    gates, h_r, c_r, hn_r, cn_r = R.lstm_cell_fwd(pre.detach(), c_in.detach(), keep_next)
    _close(h_r, h.detach()), _close(c_r, c.detach())
    _close(hn_r, h.detach() * keep_next.unsqueeze(1)), _close(cn_r, c.detach() * keep_next.unsqueeze(1))
    assert float(hn_r[0].abs().max()) == 0.0 and float(cn_r[0].abs().max()) == 0.0
    d_out, dh_rec, dc_rec = (torch.randn(B, H, generator=g, dtype=F64) for _ in range(3))
    loss = (d_out * h).sum() + (dh_rec * (h * keep_next.unsqueeze(1))).sum() + (dc_rec * (c * keep_next.unsqueeze(1))).sum()
    loss.backward()
    dpre, dcin = R.lstm_cell_bwd(gates, c_r, c_in.detach(), d_out, dh_rec, dc_rec, keep_next, first=False)
    _close(dpre, pre.grad), _close(dcin, c_in.grad)
    # first = 1 (nothing flows back from a later step), and no output gradient
    pre.grad = c_in.grad = None
    h, c = cell(pre, (torch.zeros(B, H, dtype=F64), c_in))
    (d_out * h).sum().backward()
    dpre, dcin = R.lstm_cell_bwd(gates, c_r, c_in.detach(), d_out, None, None, keep_next, first=True)
    _close(dpre, pre.grad), _close(dcin, c_in.grad)
    pre.grad = c_in.grad = None
    h, c = cell(pre, (torch.zeros(B, H, dtype=F64), c_in))
    ((dh_rec * h).sum() + (dc_rec * c).sum()).backward()
    dpre, dcin = R.lstm_cell_bwd(gates, c_r, c_in.detach(), None, dh_rec, dc_rec, None, first=False)
    _close(dpre, pre.grad), _close(dcin, c_in.grad)


# ---- actor head --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dueling", [False, True])
def test_actor_head_equals_the_plain_expression(dueling):
    g = _g(6)
    E, N, A = 9, 5, 7
    adv = torch.randn(E, N, A, generator=g, dtype=F64)
    val = torch.randn(E, N, generator=g, dtype=F64) if dueling else None
    want = (val.unsqueeze(-1) + adv - adv.mean(-1, keepdim=True)).mean(1) if dueling else adv.mean(1)
    got = R.actor_qvalues(adv, val)
    _close(got, want)
    got[0, 2] = got[0, 5] = 50.0
    assert torch.equal(R.first_max(got), got.argmax(-1)) and int(R.first_max(got)[0]) == 2
    expo = torch.linspace(1, 8, E, dtype=F64)
    used = R.eps_per_actor(0.4, expo, 0.01, E)
    assert torch.equal(used, torch.tensor([max(0.4 ** float(x), 0.01) for x in expo], dtype=F64))
    assert float(used.min()) == 0.01 and float(used[0]) == 0.4
    assert torch.equal(R.eps_per_actor(0.4, None, 0.01, E), torch.full((E,), 0.4, dtype=F64))
    greedy, rnd = R.first_max(got), torch.randint(0, A, (E,), generator=g)
    u = used.float().clone()                                          # u == eps: not below, keeps the greedy action
    u[::2] = torch.nextafter(u[::2], torch.zeros(()))
    act = R.eps_greedy(greedy, used.float(), u, rnd)
    assert torch.equal(act[::2], rnd[::2]) and torch.equal(act[1::2], greedy[1::2])


# ---- the acting network's layers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer,frames,Hi,Wi", [(2, 3, 6, 12), (2, 2, 12, 6), (2, 1, 4, 4), (3, 3, 5, 9), (3, 2, 9, 5), (3, 1, 3, 3)])
def test_conv_relu_nhwc_equals_torch_conv2d(layer, frames, Hi, Wi):
    g = _g(7)
    ci, k, s = (32, 4, 2) if layer == 2 else (64, 3, 1)
    x = torch.randn(frames, ci, Hi, Wi, generator=g, dtype=F64)
    w, b = torch.randn(64, ci, k, k, generator=g, dtype=F64) * 0.05, torch.randn(64, generator=g, dtype=F64)
    want = torch.nn.functional.conv2d(x, w, b, stride=s).permute(0, 2, 3, 1)
    got = R.conv_relu_nhwc(x.permute(0, 2, 3, 1), w, b, k, s, pre=True)
    _close(got, want)
    _close(R.conv_relu_nhwc(x.permute(0, 2, 3, 1), w, b, k, s), torch.relu(want))
    assert bool((want < 0).any()) and got.shape == (frames, (Hi - k) // s + 1, (Wi - k) // s + 1, 64)


def test_linear_embedding_product_and_output_shares_equal_torch():
    g = _g(8)
    E, N, H, D, HID, NO = 3, 5, 48, 32, 144, 7
    h, taus = torch.randn(E, H, generator=g, dtype=F64), torch.rand(E * N, generator=g, dtype=F64)
    freq = torch.arange(1, D + 1, dtype=F64) * np.pi
    wq, bq = torch.randn(H, D, generator=g, dtype=F64), torch.randn(H, generator=g, dtype=F64)
    Fn = torch.nn.functional
    _close(R.linear(h, wq.t().contiguous()[:, :H]), Fn.linear(h, wq.t().contiguous()[:, :H]))
    _close(R.linear(taus.view(-1, 1) * freq, wq, bq), Fn.linear(taus.view(-1, 1) * freq, wq, bq))
    phi = torch.cos(taus.unsqueeze(1) * freq.unsqueeze(0))
    want = torch.relu(Fn.linear(phi, wq, bq)) * h.repeat_interleave(N, dim=0)
    _close(R.cos_embed_product(taus, freq, wq, bq, h, N), want)
    assert torch.equal(R.cos_embed_pre(taus, freq, wq, bq)[0], phi)
    wfc, bfc = torch.randn(HID, H, generator=g, dtype=F64), torch.randn(HID, generator=g, dtype=F64)
    wout = torch.randn(NO, HID, generator=g, dtype=F64)
    hid, shares = R.head_shares(want, wfc, bfc, wout)
    _close(hid, torch.relu(Fn.linear(want, wfc, bfc)))
    assert shares.shape == (3, E * N, NO)                             # 64 + 64 + 16 columns
    _close(shares.sum(0), Fn.linear(hid, wout), 1e-12)
    _close(shares[2], Fn.linear(hid[:, 128:], wout[:, 128:]))


def test_philox_words_are_the_replay_test_generator():
    from tests.test_replay_gpu import _philox_u53
    for seed, call, lane in [(0, 0, 0), (99, 5, 3), (0xFFFFFFFF12345678, 1 << 40, 77)]:
        c = R.philox_4x32(seed, call, lane)
        assert ((c[0] >> 5) * 67108864.0 + (c[1] >> 6)) / 9007199254740992.0 == _philox_u53(seed, call, lane)
    u, rnd = R.philox_head_draws(77, 5, 9, 6)
    assert float(u.min()) >= 0 and float(u.max()) < 1 and int(rnd.min()) >= 0 and int(rnd.max()) < 6 and len(set(u.tolist())) == 9


# ---- the dyadic operands of the bit-exact GPU tests --------------------------------------------------------------------------
def _three_orders(terms, want64, seed):
    """terms (rows, n) float64 dyadics: added one after the other in float32, in three shuffled orders, they give `want64`."""
    t32 = terms.float().numpy()
    assert np.array_equal(t32.astype(np.float64), terms.numpy())
    rng = np.random.RandomState(seed)
    for _ in range(3):
        perm = rng.permutation(t32.shape[1])
        got = np.cumsum(t32[:, perm], axis=1, dtype=np.float32)[:, -1]
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want64.numpy())


@pytest.mark.parametrize("case", R.loss_iqn_wave_cases() + R.loss_iqn_generic_cases(), ids=lambda c: "N%d-Nt%d-A%d-M%d" % (c["N"], c["Nt"], c["A"], c["M"]))
def test_dyadic_iqn_loss_operands(case):
    d = R.dyadic_loss_iqn(**case)
    assert d["margin"] < 2 ** 24
    s = R.iqn_pairs(d["z"], d["taus"], d["actions"], d["targets"], d["kappa"])
    M = case["M"]
    assert float(s["loss_terms"].abs().max()) <= 4.0 and bool((s["loss_terms"] * 256 == (s["loss_terms"] * 256).round()).all())
    _three_orders(s["loss_terms"].reshape(M, -1), s["loss_sum"], case["seed"])
    _three_orders(s["td"].abs().reshape(M, -1), s["abs_sum"], case["seed"])
    _three_orders(-s["g_terms"].permute(0, 2, 1).reshape(M * case["N"], -1), s["gsum"].reshape(-1), case["seed"])
    assert bool((s["td"] == 0).any()) and bool((s["td"].abs() == d["kappa"]).any())
    for t in (d["z"], d["targets"]):
        assert float(t.abs().max()) <= 2.0 and bool((t * 2 == (t * 2).round()).all())
    assert bool((d["taus"] * 16 == (d["taus"] * 16).round()).all())
    assert d["weights"] is None or bool((torch.log2(d["weights"]) == torch.log2(d["weights"]).round()).all())


@pytest.mark.parametrize("case", R.loss_dqn_cases(), ids=lambda c: "A%d-M%d-%s-w%d" % (c["A"], c["M"], c["mode"], c["weights"]))
def test_dyadic_dqn_loss_operands(case):
    d = R.dyadic_loss_dqn(case["seed"], case["M"], case["A"], case["kappa"], case["weights"])
    td = d["q"][torch.arange(case["M"]), d["actions"]] - d["targets"]
    assert bool((td.abs() == d["kappa"]).any()) and (case["M"] == 1 or bool((td == 0).any()))
    assert (case["M"] == 1 or int(d["actions"][0]) == 0) and int(d["actions"][-1]) == case["A"] - 1


@pytest.mark.parametrize("case", R.target_iqn_cases(), ids=lambda c: "Ns%d-Nt%d-A%d-M%d" % (c["Ns"], c["Nt"], c["A"], c["M"]))
def test_dyadic_iqn_target_operands(case):
    d = R.dyadic_target_iqn(**case)
    assert d["margin"] < 2 ** 24 and case["Ns"] * case["A"] + case["A"] <= 4096
    M, Ns, A = case["M"], case["Ns"], case["A"]
    sums = d["zs"].sum(1)
    _three_orders(d["zs"].permute(0, 2, 1).reshape(M * A, Ns), sums.reshape(-1), case["seed"])
    top = sums.max(-1, keepdim=True).values
    tied = ((sums == top).sum(-1) >= 2)
    assert int(tied[:2].sum()) == d["ties"] == (0 if A == 1 else min(M, 2))
    best = R.iqn_select(d["zs"])
    if A >= 2:
        assert int(best[0]) == 0 and (M < 2 or int(best[1]) == A - 2)
        # the tied actions carry different targets: taking the other one shows
        assert not torch.equal(d["zt"][0, :, 0], d["zt"][0, :, A - 1])


@pytest.mark.parametrize("case", R.target_dqn_cases(), ids=lambda c: "A%d-M%d" % (c["A"], c["M"]))
def test_dyadic_dqn_target_operands(case):
    d = R.dyadic_target_dqn(**case)
    A, M = case["A"], case["M"]
    tied = (d["qs"] == d["qs"].max(-1, keepdim=True).values).sum(-1) >= 2
    assert int(tied[:2].sum()) == d["ties"] == (0 if A == 1 else min(M, 2))
    if A >= 2:
        assert int(R.first_max(d["qs"])[0]) == 0 and float(d["qt"][0, 0]) != float(d["qt"][0, A - 1])
        assert M < 2 or (int(R.first_max(d["qs"])[1]) == A - 2 and float(d["qt"][1, A - 2]) != float(d["qt"][1, A - 1]))


@pytest.mark.parametrize("case", R.actor_head_dyadic_cases(), ids=lambda c: "E%d-N%d-A%d-d%d" % (c["E"], c["N"], c["A"], c["dueling"]))
def test_dyadic_actor_head_operands(case):
    d = R.dyadic_actor_head(**case)
    assert d["margin"] < 2 ** 24
    E, N, A = case["E"], case["N"], case["A"]
    adv, val = d["adv"], d["val"]
    x = adv if val is None else val.unsqueeze(-1) + adv - adv.sum(-1, keepdim=True) / A
    q = R.actor_qvalues(adv, val)
    _three_orders(x.permute(0, 2, 1).reshape(E * A, N), (q * N).reshape(-1), case["seed"])
    assert torch.equal(q.float().double(), q)
    if A >= 2:
        assert bool(((q == q.max(-1, keepdim=True).values).sum(-1) == 2).all()) and torch.equal(R.first_max(q), d["first"])


def test_dyadic_gradients_have_an_exact_sum_of_squares():
    sizes = [1, 255, 4095, 4096, 4097, 8192, 12289] * 9 + [7, 33]
    gs, margin = R.dyadic_grads(9, sizes)
    assert margin < 2 ** 24
    sq = torch.cat(gs) ** 2
    _three_orders(sq.reshape(1, -1), sq.sum().reshape(1), 9)


@pytest.mark.parametrize("layer,frames,Hi,Wi", [(2, 1, 4, 4), (2, 3, 12, 6), (2, 20, 20, 20), (3, 1, 3, 3), (3, 3, 5, 9), (3, 30, 9, 9)])
def test_dyadic_conv_operands(layer, frames, Hi, Wi):
    d = R.dyadic_conv(900 + frames, layer, frames, Hi, Wi)
    assert d["margin"] < 2 ** 24
    patches = R.conv_patches_nhwc(d["x"], d["k"], d["s"]).reshape(-1, d["k"] ** 2 * d["x"].shape[-1])
    w_taps = d["w"].permute(0, 2, 3, 1).reshape(64, -1)
    pre = R.conv_relu_nhwc(d["x"], d["w"], d["b"], d["k"], d["s"], pre=True).reshape(-1, 64)
    for co in (0, 1, 63):                                             # products and bias in three orders: the float64 sum
        terms = torch.cat([patches * w_taps[co], d["b"][co].expand(patches.shape[0], 1)], 1)
        _three_orders(terms, pre[:, co], 900 + co)
    assert bool((pre[:, 0::2] == 0).any(0).all()) and bool((pre[:, 1::2] == -0.125).any(0).all())
    assert pre.shape[0] < 64 or int((pre == 0).sum()) >= pre.numel() // 200


@pytest.mark.parametrize("E,H,K", [(1, 8, 1296), (20, 64, 1424), (7, 64, 112)])
def test_dyadic_lstm_operands(E, H, K):
    d = R.dyadic_lstm(910 + E, E, H, K)
    assert d["margin"] < 2 ** 24 and torch.equal(d["c_in"].float().double(), d["c_in"])
    pre = R.linear(d["xh"], d["w"], d["b"])
    for j in (0, 4 * H - 1):
        _three_orders(torch.cat([d["xh"] * d["w"][j], d["b"][j].expand(E, 1)], 1), pre[:, j], 910 + j)
    assert 0.5 < float(pre.std()) < 4.0                               # the gates are not saturated


@pytest.mark.parametrize("Rr,H,HID,NO", [(33, 128, 80, 7), (70, 1024, 64, 31), (40, 64, 1024, 7)])
def test_dyadic_hidden_operands(Rr, H, HID, NO):
    d = R.dyadic_hidden(920 + Rr, Rr, H, HID, NO)
    assert d["margin"] < 2 ** 24
    hid, shares = R.head_shares(d["x"], d["wfc"], d["bfc"], d["wout"])
    _three_orders(torch.cat([d["x"] * d["wfc"][0], d["bfc"][0].expand(Rr, 1)], 1), R.linear(d["x"], d["wfc"], d["bfc"])[:, 0], 920)
    _three_orders(hid * d["wout"][NO - 1], shares.sum(0)[:, NO - 1], 921)
    assert torch.equal(shares.float().double(), shares) and float(hid.abs().max()) <= H / 2 + 2


@pytest.mark.parametrize("E,N,A,has_val", [(1, 1, 1, 0), (5, 7, 8, 1), (3, 70, 12, 0), (6, 130, 18, 1), (4, 64, 31, 1), (9, 32, 6, 1), (3, 5, 2, 1)])
def test_dyadic_head_parts_operands(E, N, A, has_val):
    d = R.dyadic_head_parts(930 + E, E, N, A, 3, bool(has_val))
    assert d["margin"] < 2 ** 24
    adv, val = d["adv"], d["val"]
    out = d["parts"].sum(0) + d["bout"]
    assert torch.equal(out[:, :A].reshape(E, N, A), adv) and (val is None or torch.equal(out[:, A].reshape(E, N), val))
    _three_orders(torch.cat([d["parts"].permute(1, 2, 0).reshape(-1, 3), d["bout"].repeat(E * N).unsqueeze(1)], 1), out.reshape(-1), 930)
    mean = adv.sum(-1) / A
    unit = 8 * A if A & (A - 1) == 0 else 8                               # mean_a A: a multiple of 1 / (8 A) at a power of two, else of 1/8
    assert val is None or bool((mean * unit == (mean * unit).round()).all())
    x = adv if val is None else val.unsqueeze(-1) + adv - mean.unsqueeze(-1)
    q = R.actor_qvalues(adv, val)
    _three_orders(x.permute(0, 2, 1).reshape(E * A, N), x.sum(1).reshape(-1), 931)
    # the one division: float32(sum) / float32(N) correctly rounded is the rounded float64 quotient
    s32 = x.sum(1).reshape(-1).numpy().astype(np.float32)
    assert np.array_equal(s32 / np.float32(N), q.reshape(-1).float().numpy())
    if A >= 2:
        assert bool(((q == q.max(-1, keepdim=True).values).sum(-1) == 2).all()) and torch.equal(R.first_max(q), d["first"])
        assert torch.equal(R.first_max(q.float()), d["first"])


# ---- LSTM time loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 5])
def test_sweep_equals_an_lstmcell_time_loop_with_resets_and_its_autograd(T):
    g = _g(40 + T)
    B, H = 6, 16
    cell = torch.nn.LSTMCell(4 * H, H).double()
    w = torch.randn(4 * H, H, generator=g, dtype=F64) * 0.4
    with torch.no_grad():                                             # gates = gx + h W_hh^T: W_ih = I, no bias
        cell.weight_ih.copy_(torch.eye(4 * H, dtype=F64)), cell.weight_hh.copy_(w)
        cell.bias_ih.zero_(), cell.bias_hh.zero_()
    gx = torch.randn(T, B, 4 * H, generator=g, dtype=F64).requires_grad_(True)
    h0, c0 = torch.randn(B, H, generator=g, dtype=F64), torch.randn(B, H, generator=g, dtype=F64)
    keep = (torch.rand(T, B, generator=g) > 0.3).double()
    keep[:, 0], keep[:, 1] = 1.0, 1.0
    keep[0, 0] = 0.0                                                  # a reset at step 0 ...
    keep[T - 1, 1] = 0.0                                              # ... and one at step T - 1
    hx, cx, outs, cs = h0, c0, [], []
    for t in range(T):                                                # modules/lstm.py:84-103
        hx, cx = hx * keep[t].unsqueeze(1), cx * keep[t].unsqueeze(1)
        hx, cx = cell(gx[t], (hx, cx))
        outs.append(hx), cs.append(cx)
    out, c_all = torch.stack(outs), torch.stack(cs)
    out_r, c_r, gates, hm, cm = R.lstm_sweep_fwd(gx.detach(), w, h0, c0, keep)
    _close(out_r, out.detach()), _close(c_r, c_all.detach())
    assert hm.shape == cm.shape == (T + 1, B, H)
    assert torch.equal(hm[0], h0 * keep[0].unsqueeze(1)) and torch.equal(cm[0], c0 * keep[0].unsqueeze(1))
    assert torch.equal(hm[1:T], out_r[:T - 1] * keep[1:].unsqueeze(2)) and torch.equal(cm[1:T], c_r[:T - 1] * keep[1:].unsqueeze(2))
    assert torch.equal(hm[T], out_r[T - 1]) and torch.equal(cm[T], c_r[T - 1])
    assert float(hm[0, 0].abs().max()) == 0.0 and (T == 1 or float(hm[T - 1, 1].abs().max()) == 0.0)
    pre = gx.detach() + hm[:T] @ w.t()
    _close(gates, torch.cat([torch.sigmoid(pre[..., :2 * H]), torch.tanh(pre[..., 2 * H:3 * H]), torch.sigmoid(pre[..., 3 * H:])], -1))
    d_out = torch.randn(T, B, H, generator=g, dtype=F64)
    (d_out * out).sum().backward()
    _close(R.lstm_sweep_bwd(gates, c_r, cm, d_out, keep, w), gx.grad)
    assert float(R.lstm_sweep_bwd(gates, c_r, cm, None, keep, w).abs().max()) == 0.0


@pytest.mark.parametrize("H", [16, 128, 256, 512])
def test_selector_whh_keeps_its_promises(H):
    for seed in (H, H + 1, H + 2, H + 3, H + 4):
        w = R.selector_whh(seed, H)
        nz = w != 0
        assert w.shape == (4 * H, H) and bool((nz.sum(1) == 1).all()) and bool((nz.sum(0) == 4).all())
        mags = set(w[nz].abs().tolist())
        assert mags <= {1.0, 0.5, 0.25, 0.125} and len(mags) == 4 and bool((w[nz] > 0).any()) and bool((w[nz] < 0).any())
        k = nz.int().argmax(1).view(4, H)                                 # k[gate, hidden unit]
        for gate in range(4):
            assert sorted(k[gate].tolist()) == list(range(H))             # every k is read by exactly one row of each gate
        assert all(len(set(k[:, j].tolist())) == 4 for j in range(H))     # the four gates of a unit read four different k
        step = set(((k[:, 1:] - k[:, :-1]) % H).reshape(-1).tolist())
        assert len(step) == 1 and step.pop() not in (0, 1, H - 1)         # neighbouring units do not read neighbouring k
        assert len(set((k[:, 0] % H).tolist())) == 4                      # a per-gate offset
        # one exact product per gate column, a four-term sum per column of the backward contraction
        h = torch.randn(7, H, generator=_g(seed))
        assert torch.equal((h @ w.float().t()).double(), h.double() @ w.t())
        assert float(((h.double() @ w.t()).abs() - h.double().abs() @ w.abs().t()).abs().max()) == 0.0


def test_activation_emulations_follow_the_forms():
    x = np.linspace(-30, 30, 4001).astype(np.float32)
    assert R.sq_sigmoid_f32(x).dtype == np.float32 and R.sq_tanh_f32(x).dtype == np.float32
    assert float(np.abs(R.sq_sigmoid_f32(x) - 1 / (1 + np.exp(-x.astype(np.float64)))).max()) <= 3e-7
    assert float(np.abs(R.sq_tanh_f32(x) - np.tanh(x.astype(np.float64))).max()) <= 3e-7
    big = np.array([-100, 100], dtype=np.float32)
    assert R.sq_sigmoid_f32(big).tolist() == [0.0, 1.0] and R.sq_tanh_f32(big).tolist() == [-1.0, 1.0] and float(R.sq_tanh_f32(np.float32(0))) == 0.0
    tiny = np.float32(3e-6)                                               # the form cancels: an absolute error of u-size, far above 2u |g|
    assert abs(float(R.sq_tanh_f32(tiny)) - 3e-6) > 2 * 2.0 ** -24 * 3e-6


def _one_step(H, family, seed, B=32):
    """A step's inputs as the GPU test sends them (float32 values, rows 1-3 in reset, h with +-2 / +-3.5) and a keep_next."""
    inp = SQ.sweep_inputs(1, B, H, family, seed)
    k0 = inp["keep"][0].unsqueeze(1)
    kn = (torch.rand(B, generator=_g(seed + 1)) > 0.3).float()
    kn[0], kn[4], kn[5] = 1.0, 0.0, 0.0
    return dict(gx=inp["gx"][0], w=inp["w"], h=inp["h0"] * k0, c_in=inp["c0"] * k0, kn=kn, n=inp["n"])


def _ref_step(s, planted=None):
    """The float64 step and its bound; `planted`: one of the five errors, in float64.  -> (values, bounds) per quantity."""
    gx, w, h, c_in, kn = (s[k].double() for k in ("gx", "w", "h", "c_in", "kn"))
    H = h.shape[1]
    hh = h.clone()
    if planted == "swapped":
        hh[:, [3, H // 2 + 1]] = h[:, [H // 2 + 1, 3]]
    if planted == "bit30":
        word = s["h"][0, 1:2].clone()
        assert 0 < abs(float(word)) < 2
        hh[0, 1] = float((word.view(torch.int32) | 0x40000000).view(torch.float32))
    pre = gx + hh @ w.t()
    if planted == "dropped":
        col = H + 5
        k = int(w[col].abs().argmax())
        pre[:, col] -= hh[:, k] * w[col, k]
    gates, c, out, e_g, e_c, e_h = SQ.fwd_step_bound(pre, (hh.abs() @ w.abs().t()) if s["n"] else None, s["n"], c_in)
    if planted == "i-f":
        i, f, g, o = gates.chunk(4, 1)
        c = i * c_in + f * g
        out = o * torch.tanh(c)
    k = kn.unsqueeze(1)
    vals = dict(gates=gates, c=c, h=out, h_next=out * k, c_next=c if planted == "c-unmasked" else c * k)
    return vals, dict(gates=e_g, c=e_c, h=e_h, h_next=e_h * k, c_next=e_c * k)


def _f32_step(s):
    """The step as the sweep kernels evaluate it, every operation in float32 (NumPy)."""
    gx, w, h, c_in, kn = (s[k].numpy() for k in ("gx", "w", "h", "c_in", "kn"))
    H = h.shape[1]
    pre = h @ w.T + gx
    assert pre.dtype == np.float32
    i, f, o = R.sq_sigmoid_f32(pre[:, :H]), R.sq_sigmoid_f32(pre[:, H:2 * H]), R.sq_sigmoid_f32(pre[:, 3 * H:])
    g = R.sq_tanh_f32(pre[:, 2 * H:3 * H])
    c = f * c_in + i * g
    out = o * R.sq_tanh_f32(c)
    k = kn[:, None]
    return {n: torch.from_numpy(np.ascontiguousarray(v)).double() for n, v in
            dict(gates=np.concatenate([i, f, g, o], 1), c=c, h=out, h_next=out * k, c_next=c * k).items()}


@pytest.mark.parametrize("family", SQ.FAMILIES)
@pytest.mark.parametrize("H", [128, 512])
def test_forward_bound_is_kept_by_a_float32_evaluation(H, family):
    s = _one_step(H, family, 50 + H)
    want, bound = _ref_step(s)
    got = _f32_step(s)
    for name in want:
        err = (got[name] - want[name]).abs()
        assert bool((err <= bound[name]).all()), (name, float((err / bound[name].clamp(min=1e-300)).max()))
    # a pre-activation of the saturated kind: exact gates inside the same bound
    s["gx"] = torch.where(torch.arange(4 * H) % 3 == 0, torch.tensor(-100.0), torch.tensor(100.0)).expand_as(s["gx"]).contiguous()
    want, bound = _ref_step(s)
    got = _f32_step(s)
    assert set(got["gates"].reshape(-1).tolist()) == {0.0, 1.0, -1.0}
    for name in want:
        assert bool(((got[name] - want[name]).abs() <= bound[name]).all()), name


@pytest.mark.parametrize("H,family,planted", [(512, "selector", p) for p in ("dropped", "swapped", "c-unmasked", "i-f", "bit30")]
                         + [(128, "gaussian", p) for p in ("dropped", "swapped", "c-unmasked", "i-f", "bit30")] + [(512, "gaussian", "dropped")])
def test_forward_bound_catches_a_planted_error(H, family, planted):
    """One k-term dropped from one column's sum, two h columns swapped, keep applied to h but not to c, gates i and f exchanged,
    one h word left with bit 30 set: each breaks the bound of at least one quantity of the step.  With the dense W at H = 512 the
    summation-order term n u sum |h_k w_k| is about 3e-4 of a pre-activation: the dropped term here is the column's LARGEST weight
    (about 0.2 |h_k|) and shows, a term below that size would hide behind it — such terms rest on the selector W, where the
    one product is the whole sum and the bound is u |pre|."""
    s = _one_step(H, family, 60 + H)
    want, bound = _ref_step(s)
    bad, _ = _ref_step(s, planted)
    assert any(bool(((bad[name] - want[name]).abs() > bound[name]).any()) for name in want)


def _f32_bwd(gates, c_all, cm, d_out, keep, w):
    """The backward recurrence in float32 in the sweep kernel's order: partial dh of 64 gate columns (4 gates x 16 hidden units of a
    column group) per owner, the 32 partials added in source order; tanhf correctly rounded."""
    T, _, H4 = gates.shape
    H = H4 // 4
    cols = [np.array([g * H + 16 * cg + j for g in range(4) for j in range(16)]) for cg in range(H // 16)]
    dg = np.zeros_like(gates)
    dhr = dcr = None
    for t in range(T - 1, -1, -1):
        first = t == T - 1
        i, f, g, o = (gates[t][:, n * H:(n + 1) * H] for n in range(4))
        kn = np.float32(1) if first else keep[t + 1][:, None]
        dh = d_out[t] + (np.float32(0) if first else dhr * kn)
        tc = np.tanh(c_all[t].astype(np.float64)).astype(np.float32)
        dc = (np.float32(0) if first else dcr * kn) + dh * o * (np.float32(1) - tc * tc)
        one = np.float32(1)
        dg[t] = np.concatenate([dc * g * i * (one - i), dc * cm[t] * f * (one - f), dc * i * (one - g * g), dh * tc * o * (one - o)], 1)
        dcr = dc * f
        dhr = np.zeros_like(dh)
        for cs in cols:
            dhr = dhr + dg[t][:, cs] @ w[cs, :]
        assert dhr.dtype == np.float32 and dg.dtype == np.float32
    return dg


@pytest.mark.parametrize("family", SQ.FAMILIES)
def test_backward_bound_is_kept_by_a_float32_evaluation_and_broken_by_a_misplaced_partial(family):
    T, B, H = 4, 16, 512
    inp = SQ.sweep_inputs(T, B, H, family, 70)
    saved = [t.float() for t in R.lstm_sweep_fwd(*(inp[k].double() for k in ("gx", "w", "h0", "c0", "keep")))]      # what a forward launch saves
    _, c_all, gates, _, cm = saved
    d_out = torch.randn(T, B, H, generator=_g(71))
    args = [t.double() for t in (gates, c_all, cm, d_out, inp["keep"], inp["w"])]
    want, bound = SQ.bwd_sweep_bound(*args, n=4 if family == "selector" else 96)
    _close(want, R.lstm_sweep_bwd(*args))
    got = torch.from_numpy(_f32_bwd(*(t.numpy() for t in (gates, c_all, cm, d_out, inp["keep"], inp["w"])))).double()
    err = (got - want).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
    if family == "selector":
        # two 16-unit blocks of dh_rec handed to each other's owner at one step: far outside the bound
        w2 = args[5].clone()
        w2[:, 0:16], w2[:, 16:32] = args[5][:, 16:32], args[5][:, 0:16]
        bad = R.lstm_sweep_bwd(*args[:5], w2)
        assert bool(((bad - want).abs() > bound).any())


# ---- the acting step's bookkeeping (csrc/acting.hip): hand-worked cases, every expected array written out ------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _f(*v):
    return np.array(v, dtype=np.float32)


def _i(*v):
    return np.array(v, dtype=np.int32)


def test_episode_track_on_a_hand_worked_stream():
    """E = 3, A = 3, four steps.  Env 0: an episode ends mid-stream (step 1) and the next one starts from 0; env 1: done on the
    very first step; env 2: every reward is -0.0 and its accumulator starts at -0.0 (-0.0 + -0.0 = -0.0 is reported, the restart
    is +0.0 and +0.0 + -0.0 = +0.0).  Actions -1 and A = 3 are not counted."""
    A = 3
    steps = [  # rewards, dones, actions -> ep_reward, ep_len, out_reward, out_len, action_counts
        (_f(1.0, 0.25, -0.0), [0, 1, 0], _i(-1, 3, 1), _f(1.0, 0.0, -0.0), _i(1, 0, 1), _f(0.0, 0.25, 0.0), _i(0, 1, 0), _i(0, 1, 0)),
        (_f(2.0, -1.0, -0.0), [1, 0, 1], _i(0, 2, 2), _f(0.0, -1.0, 0.0), _i(0, 1, 0), _f(3.0, 0.0, -0.0), _i(2, 0, 2), _i(1, 1, 2)),
        (_f(-0.5, -0.0, -0.0), [0, 0, 0], _i(1, 1, 1), _f(-0.5, -1.0, 0.0), _i(1, 2, 1), _f(0.0, 0.0, 0.0), _i(0, 0, 0), _i(1, 4, 2)),
        (_f(4.0, 1.0, 0.0), [0, 1, 0], _i(3, -1, 0), _f(3.5, 0.0, 0.0), _i(2, 0, 2), _f(0.0, 0.0, 0.0), _i(0, 3, 0), _i(2, 4, 2)),
    ]
    epr, epl, counts = _f(0.0, 0.0, -0.0), _i(0, 0, 0), _i(0, 0, 0)
    outr, outl = _f(9.0, 9.0, 9.0), _i(9, 9, 9)
    for k, (r, d, a, w_epr, w_epl, w_outr, w_outl, w_counts) in enumerate(steps):
        before = (epr.copy(), epl.copy(), counts.copy())
        epr, epl, outr, outl, counts = R.episode_track(r, d, a, A, epr, epl, outr, outl, counts)
        assert np.array_equal(_bits(epr), _bits(w_epr)) and np.array_equal(epl, w_epl), k
        assert np.array_equal(_bits(outr), _bits(w_outr)) and np.array_equal(outl, w_outl), k
        assert np.array_equal(counts, w_counts), k
        assert epr.dtype == np.float32 and epl.dtype == np.int32 and counts.dtype == np.int32
        assert np.array_equal(_bits(before[0]), _bits(steps[k - 1][3] if k else _f(0.0, 0.0, -0.0)))       # inputs are not modified
    # no histogram without actions or without counts; buffers longer than E keep their tail
    got = R.episode_track(_f(1.0), [1], None, A, _f(2.0, 7.0), _i(4, 7), _f(9.0, 9.0), _i(9, 9), _i(5, 5, 5))
    for g, w in zip(got, (_f(0.0, 7.0), _i(0, 7), _f(3.0, 9.0), _i(5, 9), _i(5, 5, 5))):
        assert np.array_equal(g, w)
    assert R.episode_track(_f(1.0), [0], _i(1), A, _f(2.0), _i(4), _f(9.0), _i(9), None)[4] is None


def test_episode_reward_is_a_sequential_float32_sum():
    """Three rewards whose float32 running sum differs from the float64 sum rounded once: 2^24 + 1 + 1 stays 2^24 in float32."""
    epr, epl, outr, outl = _f(0.0), _i(0), _f(0.0), _i(0)
    for k, r in enumerate((16777216.0, 1.0, 1.0)):
        epr, epl, outr, outl, _ = R.episode_track(_f(r), [k == 2], None, 1, epr, epl, outr, outl, None)
    assert float(outr[0]) == 16777216.0 and int(outl[0]) == 3
    assert float(np.float32(16777216.0 + 1.0 + 1.0)) == 16777218.0              # the float64 sum, rounded once, is another number


def _pre_buffers():
    return dict(xh=_f(*[9.0] * 7), c_in=_f(*[9.0] * 5), state_pack=_f(*[9.0] * 9), initials=_f(9.0, 9.0, 9.0),
                rewards_out=_f(9.0, 9.0, 9.0), dones_out=np.array([7, 7, 7], dtype=np.uint8))


def test_actor_pre_on_a_hand_worked_step():
    """E = 2, H = 2, xh_pitch = 3; env 0 is done.  Its carry becomes the signed zero of x * 0: 1.5 -> +0.0, -2.0 -> -0.0,
    -1.0 -> -0.0, 0.0 -> +0.0; env 1 keeps -0.0 as it is.  Column 2 of each xh row and every guard element keep the 9.0 / 7."""
    h, c = _f(1.5, -2.0, -0.0, 3.0), _f(-1.0, 0.0, 4.0, -0.5)
    raw, dones = _f(-2.5, -0.0), np.array([1, 0], dtype=np.uint8)
    stats = dict(actions=_i(-1, 2), A=2, ep_reward=_f(1.0, 2.0), ep_len=_i(3, 4), out_reward=_f(9.0, 9.0), out_len=_i(9, 9),
                 action_counts=_i(0, 0))
    step = np.array([5], dtype=np.uint64)
    got = R.actor_pre(raw, dones, 2, h, c, xh_pitch=3, clip=1, rng_step=step, step=11, **_pre_buffers(), **stats)
    want = dict(xh=_f(0.0, -0.0, 9.0, -0.0, 3.0, 9.0, 9.0), c_in=_f(-0.0, 0.0, 4.0, -0.5, 9.0),
                state_pack=_f(0.0, -0.0, -0.0, 0.0, -0.0, 3.0, 4.0, -0.5, 9.0), initials=_f(1.0, 0.0, 9.0),
                rewards_out=_f(-1.0, 0.0, 9.0), ep_reward=_f(0.0, 2.0), out_reward=_f(-1.5, 0.0))
    for k, w in want.items():
        assert got[k].dtype == np.float32 and np.array_equal(_bits(got[k]), _bits(w)), k
    assert np.array_equal(got["dones_out"], np.array([1, 0, 7], dtype=np.uint8))
    assert np.array_equal(got["ep_len"], _i(0, 5)) and np.array_equal(got["out_len"], _i(4, 0))
    assert np.array_equal(got["action_counts"], _i(0, 0))                 # -1 and A = 2: neither is counted
    assert int(got["rng_step"][0]) == 11 and int(step[0]) == 5
    # no clipping: the raw reward passes through with its sign bit; actions 1, 0 are counted; the counter advances by one
    stats["actions"] = _i(1, 0)
    got = R.actor_pre(raw, dones, 2, h, c, xh_pitch=3, clip=0, rng_step=step, step=R.STEP_ADVANCE, **_pre_buffers(), **stats)
    assert np.array_equal(_bits(got["rewards_out"]), _bits(_f(-2.5, -0.0, 9.0)))
    assert np.array_equal(got["action_counts"], _i(1, 1)) and int(got["rng_step"][0]) == 6
    top = np.array([2 ** 64 - 1], dtype=np.uint64)
    assert int(R.actor_pre(raw, dones, 2, h, c, xh_pitch=3, clip=0, rng_step=top, step=R.STEP_ADVANCE, **_pre_buffers())["rng_step"][0]) == 0
    # clip is np.sign: a positive subnormal is +1, huge values are +-1, both zeros give +0.0
    raw5 = _f(0.0, -0.0, 1e-45, 3e38, -3e38)
    b = dict(initials=_f(*[9.0] * 5), rewards_out=_f(*[9.0] * 5), dones_out=np.zeros(5, dtype=np.uint8))
    got = R.actor_pre(raw5, [0] * 5, 0, None, None, None, 0, None, None, clip=1, **b)
    assert np.array_equal(_bits(got["rewards_out"]), _bits(_f(0.0, 0.0, 1.0, 1.0, -1.0)))
    # H = 0, no statistics, no counter: nothing but initials / rewards / dones
    assert all(got[k] is None for k in ("xh", "c_in", "state_pack", "ep_reward", "ep_len", "out_reward", "out_len", "action_counts", "rng_step"))


def test_actor_pre_statistics_are_episode_track():
    g = np.random.default_rng(5)
    E, A = 7, 4
    epr, epl = g.standard_normal(E).astype(np.float32), g.integers(0, 50, E).astype(np.int32)
    outr, outl, counts = np.full(E + 1, 9, np.float32), np.full(E + 1, 9, np.int32), g.integers(0, 9, A).astype(np.int32)
    raw, dones = g.standard_normal(E).astype(np.float32), g.integers(0, 2, E).astype(np.uint8)
    actions = g.integers(-1, A + 1, E).astype(np.int32)
    b = dict(initials=np.zeros(E, np.float32), rewards_out=np.zeros(E, np.float32), dones_out=np.zeros(E, np.uint8))
    got = R.actor_pre(raw, dones, 0, None, None, None, 0, None, None, clip=1, actions=actions, A=A, ep_reward=epr, ep_len=epl,
                      out_reward=outr, out_len=outl, action_counts=counts, **b)
    want = R.episode_track(raw, dones, actions, A, epr, epl, outr, outl, counts)
    for k, w in zip(("ep_reward", "ep_len", "out_reward", "out_len", "action_counts"), want):
        assert np.array_equal(got[k], w), k
    assert int(want[4].sum() - counts.sum()) == int(((actions >= 0) & (actions < A)).sum())


def test_stack_shift_by_hand_and_against_the_env_fallback():
    inp = np.array([[[1, 2], [3, 4], [5, 6]], [[7, 8], [9, 10], [11, 12]]], dtype=np.uint8)       # E = 2, P = 3, 2-byte planes
    newest = np.array([[21, 22], [23, 24]], dtype=np.uint8)
    want = np.array([[[3, 4], [5, 6], [21, 22]], [[0, 0], [0, 0], [23, 24]]], dtype=np.uint8)
    assert np.array_equal(R.stack_shift(inp, newest, [0, 1]), want)
    # the non-kernel branch of SyntheticAtariVecEnv._shift (a CPU env): the same operation in torch
    from rltime_amd.acting.synthetic_env import SyntheticAtariVecEnv
    g = np.random.default_rng(9)
    for P, shape in ((2, (3, 5)), (4, (4, 4))):
        env = SyntheticAtariVecEnv(5, frame_shape=(P,) + shape, device="cpu", pool=2, frame_stack=True)
        stack = g.integers(0, 256, (5, P) + shape).astype(np.uint8)
        newest = g.integers(0, 256, (5,) + shape).astype(np.uint8)
        dones = np.array([0, 1, 1, 0, 1], dtype=bool)
        env._stack = torch.from_numpy(stack.copy())
        got = env._shift(torch.from_numpy(newest), torch.from_numpy(dones))
        assert np.array_equal(got.numpy(), R.stack_shift(stack, newest, dones))


def test_synth_env_draws_are_words_0_and_1_with_strict_thresholds():
    seed, t, E = 1234, (1 << 32) + 5, 16                                  # the high word of t takes part
    r, d, idx, u0, u1 = R.synth_env_draws(seed, t, E, 0.1, 0.9, 0.25, pool_n=3)
    assert idx == t % 3 and r.dtype == np.float32 and d.dtype == np.uint8 and u0.dtype == np.float32
    for e in range(E):
        w = R.philox_4x32(seed ^ 0xE17, t, e)
        assert float(u0[e]) == (w[0] >> 8) / 16777216.0 and float(u1[e]) == (w[1] >> 8) / 16777216.0
        assert float(r[e]) == (-1.0 if u0[e] < np.float32(0.1) else 0.0 if u0[e] < np.float32(0.9) else 1.0)
        assert int(d[e]) == int(u1[e] < np.float32(0.25))
    assert torch.equal(torch.from_numpy(u0), R.philox_head_draws(seed ^ 0xE17, t, E, 6)[0])
    assert not np.array_equal(u0, R.synth_env_draws(seed, 5, E, 0.1, 0.9, 0.25)[3])                # t mod 2^32 alone is another block
    assert len(set(r.tolist())) == 3 and 0 < int(d.sum()) < E and not np.array_equal(u0, u1)
    # a threshold equal to the uniform is not below it; the next float32 above is
    k = int(np.argmax(u1))
    up = np.nextafter(u1[k], np.float32(2))
    assert R.synth_env_draws(seed, t, E, 0.1, 0.9, u1[k])[1][k] == 0 and R.synth_env_draws(seed, t, E, 0.1, 0.9, up)[1][k] == 1
    k = int(np.argmax(u0))
    up = np.nextafter(u0[k], np.float32(2))
    assert R.synth_env_draws(seed, t, E, u0[k], 1.0, 0.0)[0][k] == 0.0 and R.synth_env_draws(seed, t, E, up, 1.0, 0.0)[0][k] == -1.0
    assert R.synth_env_draws(seed, t, E, 0.0, u0[k], 0.0)[0][k] == 1.0 and R.synth_env_draws(seed, t, E, 0.0, up, 0.0)[0][k] == 0.0
    # p_neg = 0, p_nonpos = 1: every reward is 0; p_done 0 / 1: nobody / everybody
    r0, d0, _, _, _ = R.synth_env_draws(seed, t, E, 0.0, 1.0, 0.0)
    assert not r0.any() and not d0.any() and R.synth_env_draws(seed, t, E, 0.0, 1.0, 1.0)[1].all()


def test_frames_to_f32_nhwc_is_one_rounding_in_channels_last():
    x = np.arange(24, dtype=np.uint8).reshape(1, 4, 6) * 11
    got = R.frames_to_f32_nhwc(x, 0.3)
    assert got.shape == (1, 6, 4) and got.dtype == np.float32
    for p in range(6):
        for ch in range(4):
            assert got[0, p, ch] == np.float32(float(x[0, ch, p])) * np.float32(0.3)
