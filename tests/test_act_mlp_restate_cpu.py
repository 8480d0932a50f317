"""No GPU: what tests/test_act_mlp_exact_gpu.py leans on, for exactly the operands it sends (tests/act_mlp_restate.py).

The launch geometry names the intended branch of csrc/act_mlp.hip for every shape (CH from the launcher's own host logic).
The product-by-product float64 walk that carries the bound is the layer-by-layer float64 reference.  The dyadic operands:
every partial sum of every product and of the head is a float32 number, three shuffled float32 summation orders equal float64
bit for bit, every input reaches every column pass, every row's maximum is tied.  The real operands: at most one row in eight
has its two best float64 q-values closer than their bounds, and a NumPy float32 restatement of the kernel's operation order
lies inside the bound on every element (and on the dyadic operands equals float64 to the bit)."""
import functools

import numpy as np
import pytest
import torch

from tests import act_mlp_restate as R

NAMES = sorted(R.ALL_SHAPES)
BRANCH_NAMES = sorted(R.BRANCH_SHAPES)          # the real-operand tier: the earlier six keep check_bar
MODES = [1, 0]


@functools.lru_cache(maxsize=None)
def _dyadic(name, need_q):
    case = R.DyadicCase(name, need_q)
    return case, R.forward_bound(case, need_q)


@functools.lru_cache(maxsize=None)
def _real(name, need_q):
    case = R.Case(name)
    return case, R.forward_bound(case, need_q)


# ---- geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_geometry_names_the_intended_branch(name):
    g1, g0 = R.assert_branches(name)
    d = R.Dims(name)
    # the launcher's rule itself: 32 rows where that fits 64 KB, 16 otherwise
    fits = 4 * (576 + 4096 + 32 * (d.D + d.W + d.HID) + d.N * d.NO) <= 65536
    assert g1["CH"] == g0["CH"] == (32 if fits else 16)


def test_every_branch_of_the_issue_is_named_by_a_shape():
    geo = {n: R.assert_branches(n) for n in R.BRANCH_SHAPES}
    every = lambda key: [p for g in geo.values() for m in g for p in m[key]]          # noqa: E731
    assert any(len(p["row_passes"]) > 1 for p in every("quant"))                        # the second row pass
    assert any(n0 > 0 and r < g[0]["CH"] for g in geo.values() for n0, r in g[0]["chunks"])      # a ragged last chunk
    assert any(p["J"] > 256 and p["passes"][-1]["Jt"] % 64 for p in every("fc"))        # a last column pass off the wave
    assert any(p["JP"] == 192 for key in ("lead", "quant", "fc") for p in every(key))   # JP = 192
    assert any(t["Jt"] == 256 and p["K"] % t["TK"] for p in every("lead") for t in p["passes"])  # a ragged K tile at Jt = 256
    assert any(len(t["tiles"]) > 1 and t["Jt"] < 64 for p in every("fc") for t in p["passes"])   # tiles under a narrow pass
    dims = [R.Dims(n) for n in R.BRANCH_SHAPES]
    assert any(len(d.widths) == 2 and d.widths[0] != d.widths[1] for d in dims)
    assert any(d.dueling and d.h1 % 64 for d in dims)                                   # need_q = 0 off a pass boundary
    assert any(9 <= d.A <= 31 and d.A % 8 for d in dims) and any(d.A == 1 for d in dims)
    assert any(33 <= d.N <= 63 for d in dims) and any(not d.widths and d.D == 0 for d in dims)
    # the six earlier shapes reach none of the first four
    old = {n: R.assert_branches(n) for n in R.SHAPES}
    assert all(len(p["row_passes"]) == 1 for g in old.values() for m in g for key in ("lead", "quant", "fc", "out") for p in m[key])
    assert all(r == g[0]["CH"] or n0 == 0 for g in old.values() for n0, r in g[0]["chunks"])
    assert not any(p["JP"] == 192 for g in old.values() for m in g for key in ("lead", "quant", "fc", "out") for p in m[key])


def test_a_shape_off_its_branch_fails(monkeypatch):
    monkeypatch.setitem(R.ALL_SHAPES, "two-row-passes", (8, 6, [64], 27, 16, 96, 3, True))       # W = 64: G = 4, one row pass
    with pytest.raises(AssertionError):
        R.assert_branches("two-row-passes")


# ---- the walk that carries the bound is the reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("need_q", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_the_product_walk_is_the_float64_reference(name, need_q):
    case = R.Case(name)
    phi = torch.cos(case.freq.double() * case.taus.double().unsqueeze(1)).float() if case.D else None
    fb = R.forward_bound(case, need_q, phi=phi)
    saved = case.taus
    if case.D:                                                        # the reference on the same (float32) features
        ref = _reference_on(case, phi)
    else:
        ref = R.reference(case, torch.float64)
    assert case.taus is saved
    want = ref[0] if (need_q or not case.dueling) else ref[1]
    assert fb["q"].shape == (case.E, case.A)
    assert float((fb["q"] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert bool((fb["bound"] > 0).all()) and bool(torch.isfinite(fb["bound"]).all())


def _reference_on(case, phi32):
    """R.reference's layers in float64 with the cosine features handed in."""
    import torch.nn.functional as F
    c, d = case, (lambda t: t.double())
    f = d(c.obs)
    for w, b in c.leading:
        f = F.relu(F.linear(f, d(w), d(b)))
    x = F.relu(F.linear(d(phi32), d(c.wq), d(c.bq))) * f.repeat_interleave(c.N, dim=0)
    out = F.linear(F.relu(F.linear(x, d(c.wfc), d(c.bfc))), d(c.wout), d(c.bout))
    adv = out[:, :c.A]
    q = out[:, c.A:c.A + 1] + adv - adv.mean(1, keepdim=True) if c.dueling else adv
    return q.reshape(c.E, c.N, c.A).mean(1), adv.reshape(c.E, c.N, c.A).mean(1)


# ---- the bound function ----------------------------------------------------------------------------------------------------------
def test_the_product_bound_is_zero_on_zero_terms_carries_no_input_error_for_exact_inputs_and_grows_with_k():
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(5, 24, generator=g).double(), torch.randn(7, 24, generator=g).double(), torch.randn(7, generator=g).double()
    zero = torch.zeros_like(x)
    y, e = R._dense64(x, zero, w, b)
    # exact inputs: nothing but this product's own K roundings per term and the bias addition
    assert torch.equal(e, 24 * R.U * (x.abs() @ w.abs().t()) + R.U * y.abs())
    # no term, no bias: no error
    y0, e0 = R._dense64(zero, zero, w, torch.zeros(7, dtype=torch.float64))
    assert float(y0.abs().max()) == 0.0 and float(e0.abs().max()) == 0.0
    # an input error passes through |w|
    _, e1 = R._dense64(x, torch.full_like(x, 1e-3), w, b)
    assert torch.allclose(e1 - e, 1e-3 * w.abs().sum(1).expand(5, 7), rtol=1e-9, atol=0)
    # the same terms in two halves: K doubles, the sum of magnitudes stays, the rounding part doubles
    y2, e2 = R._dense64(torch.cat([x, x], 1), torch.cat([zero, zero], 1), torch.cat([w, w], 1) / 2, b)
    assert torch.allclose(y2, y, rtol=1e-12, atol=1e-12)
    assert bool((e2 > e).all()) and torch.allclose(e2 - R.U * y2.abs(), 2 * (e - R.U * y.abs()), rtol=1e-9, atol=0)
    for K in (8, 64, 512):                                            # and in K alone, terms of the same size
        _, ek = R._dense64(torch.ones(1, K, dtype=torch.float64) / K, torch.zeros(1, K, dtype=torch.float64),
                           torch.ones(1, K, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))
        assert abs(float(ek) - (K + 1) * R.U) < 1e-20


# ---- dyadic operands ------------------------------------------------------------------------------------------------------------
def _three_orders(terms, want64, seed):
    """terms (rows, n) float64 dyadics: added one after the other in float32, in three shuffled orders, they give `want64`."""
    t32 = terms.float().numpy()
    assert np.array_equal(t32.astype(np.float64), terms.numpy())
    rng = np.random.RandomState(seed)
    for _ in range(3):
        perm = rng.permutation(t32.shape[1])
        got = np.cumsum(t32[:, perm], axis=1, dtype=np.float32)[:, -1]
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want64.numpy())


@pytest.mark.parametrize("need_q", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_dyadic_operands_are_exact_cover_every_pass_and_tie_every_row(name, need_q):
    case, fb = _dyadic(name, need_q)
    if need_q and case.dueling:
        assert case.A & (case.A - 1) == 0                              # m / A is exact
    if case.D:
        assert float(case.freq.abs().max()) == 0.0
    # every product: integers, every partial sum below 2^24 in magnitude whatever the order
    worst = 0.0
    for pname, x, w, b in fb["products"]:
        for t in (x, w, b):
            assert torch.equal(t, t.round())
        mag = float((x.abs() @ w.abs().t() + b.abs()).max())
        worst = max(worst, mag)
        assert mag < 2 ** 24, (pname, mag)
        # three shuffled float32 orders of the products and the bias, on the first rows and a unit of every 64
        rows = x[:: max(1, x.shape[0] // 4)][:4]
        for j in range(0, w.shape[0], 61):
            terms = torch.cat([rows * w[j], b[j].expand(rows.shape[0], 1)], 1)
            _three_orders(terms, terms.sum(1), 7 + j)
    # the head: t a multiple of 1 / A (dueling) or an integer, the sum over the N rows exact, one division
    t = fb["t"]
    gran = 1.0 / case.A if (case.dueling and need_q) else 1.0
    assert torch.equal(t / gran, (t / gran).round())
    head = float(t.abs().sum(1).max()) / gran
    assert head < 2 ** 24
    _three_orders(t.permute(0, 2, 1).reshape(case.E * case.A, case.N)[:64], (fb["q"] * case.N).reshape(-1)[:64], 11)
    print("%s need_q=%d: largest sum of magnitudes in a product %.0f, in the head / granularity %.0f" % (name, need_q, worst, head))
    # coverage and ties
    assert R.coverage_gaps(case, need_q) == []
    q = fb["q"]
    if case.A >= 2:
        assert bool(((q == q.max(1, keepdim=True).values).sum(1) >= 2).all())
        first = R.first_max(q)
        h = (case.A + 1) // 2
        assert int(first.max()) < h                                    # the first of a tied pair, never its copy
        assert bool((q[torch.arange(case.E), first] == q[torch.arange(case.E), (first + h).clamp(max=case.A - 1)]).all()) or case.A % 2
    # the float64 walk and the layer-by-layer reference agree to the bit here
    ref = R.reference(case, torch.float64)
    assert torch.equal(fb["q"], ref[0] if (need_q or not case.dueling) else ref[1])
    # the kernel's operation order in float32 gives float32(float64) and takes the first maximum
    acts, q32 = R.emulate32(case, need_q)
    assert torch.equal(q32, q.float()) and torch.equal(acts, R.first_max(q))


def test_dyadic_ties_are_not_all_on_action_0_and_the_features_vary():
    case, fb = _dyadic("every-limit", 1)
    assert fb["products"][-1][1].count_nonzero() > 0
    for name in ("every-limit", "hid-192", "ragged-chunks-of-16"):
        case, fb = _dyadic(name, 0)
        assert len(set(R.first_max(fb["q"]).tolist())) >= 2 or case.E == 1
    # at least half of every case's hidden units are alive on some row: a wrong weight shows
    for name in NAMES:
        for need_q in MODES:
            hid = _dyadic(name, need_q)[1]["products"][-1][1]
            assert float((hid > 0).any(0).double().mean()) >= 0.5, (name, need_q)


# ---- real operands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("need_q", MODES)
@pytest.mark.parametrize("name", BRANCH_NAMES)
def test_the_seeds_leave_rows_clear_of_their_bounds(name, need_q):
    """At most one row in eight has its two best float64 q-values closer than the sum of their bounds: a condition on the seed,
    checked from the float64 reference alone."""
    case, fb = _real(name, need_q)
    _, _, close = R.allowed_actions(fb["q"], fb["bound"])
    assert int(close.sum()) * 8 <= case.E, (name, need_q, int(close.sum()))
    print("%s need_q=%d: largest bound %.2e at a largest |q| of %.2f" % (name, need_q, float(fb["bound"].max()), float(fb["q"].abs().max())))


@pytest.mark.parametrize("need_q", MODES)
@pytest.mark.parametrize("name", BRANCH_NAMES)
def test_the_kernels_operation_order_in_float32_lies_inside_the_bound(name, need_q):
    case, fb = _real(name, need_q)
    acts, q32 = R.emulate32(case, need_q)
    ratio = R.check_bound(q32, fb, acts, "%s need_q=%d (NumPy float32)" % (name, need_q))
    assert 0.0 < ratio <= 1.0
