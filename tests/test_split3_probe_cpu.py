"""CPU: the part-probing operands of tests/split3_probe.py are what tests/test_split3_exact_gpu.py needs them to be — for
every generator and every case the GPU tests run, in a restatement of the method (csrc/split3.hpp's split as bf16
round trips, csrc/gemm3.hip's six part products accumulated in f32):

  1. the emulated result equals float64, bit for bit;
  2. sum_k (|hi|+|mid|+|lo|)(a_k) (|hi|+|mid|+|lo|)(b_k) < 2^24 in the output's unit (which bounds sum |a||b| and every
     partial sum of part products in any order), likewise every epilogue sum a GPU test compares bit-exactly;
  3. hi, mid and lo are non-zero in at least MIN_SHARE of each split operand's elements;
  4. leaving out any ONE of the six products changes at least 90 % of the outputs;
  5. each of the three dropped products (mid.lo, lo.mid, lo.lo) is zero at every output.

So a GPU test that fails on these operands has found the kernel wrong, and a kernel that loses, misplaces or mispairs a
part cannot pass."""
import pytest
import torch

from tests import split3_probe as sp

# hi, mid, lo.  The dense classes cover half of the contraction indexes of each operand (class 0 or 1: a third, wide; class 2a or
# 2b: a sixth, 10 bits); a wide value has a non-zero lo when its low 4 bits survive the two roundings: ~88 % of a third.
MIN_SHARE = (0.4, 0.4, 0.2)
CHANGED = 0.9


def _mm(a, b):
    return a @ b


def _check(op, a, b, a_int, b_int, emul=None, products=sp.SIX, shares=(True, True), extra_int=0.0):
    emul = emul or (lambda prods: sp.emulate(op, a, b, prods))
    want = op(a.double(), b.double())
    full = emul(products)
    assert full.dtype == torch.float32 and torch.equal(full.double(), want)                        # 1
    bound = sp.line_bound(op, a_int, b_int) + extra_int                                            # 2
    assert float(op(a_int.abs().double(), b_int.abs().double()).max()) <= bound < sp.LIMIT, bound
    for t, on in zip((a_int, b_int), shares):                                                      # 3
        if on:
            for part, least in zip(sp.split3(t), MIN_SHARE):
                assert float((part != 0).float().mean()) >= least
    for drop in products:                                                                          # 4
        rest = tuple(p for p in products if p != drop)
        changed = float((emul(rest) != full).float().mean())
        assert changed >= CHANGED, (sp.NAMES[drop], changed)
    pa, pb = sp.split3(a), sp.split3(b)
    for i, j in sp.DROPPED:                                                                        # 5
        assert not bool(op(pa[i].double(), pb[j].double()).any())
    return want


def test_the_split_is_exact_and_wide_values_fill_all_three_parts():
    gen = torch.Generator().manual_seed(0)
    x = sp._odd(gen, (1 << 16,), 20) * sp._pow2(gen, (1 << 16,))
    hi, mid, lo = sp.split3(x)
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    assert float((lo != 0).float().mean()) > 0.8 and bool((mid != 0).float().mean() > 0.95)
    # 17 bits are not enough: round-to-nearest with signed remainders lets hi + mid hold them all
    narrow = torch.randint(2 ** 15, 2 ** 16, (1 << 16,), generator=gen).float() * 2 + 1
    assert not bool(sp.split3(narrow)[2].any()) and not bool(sp.split3(-narrow)[2].any())
    m = sp._odd(gen, (1 << 12,), 10)
    assert bool((sp.split3(m)[1] != 0).all()) and not bool(sp.split3(m)[2].any())


@pytest.mark.parametrize("name", list(sp.GEMM_CASES))
def test_gemm_cases(name):
    c = sp.gemm_case(name)
    extra = float(c["bias_int"].abs().max()) if c["bias"] is not None else 0.0
    _check(_mm, c["a"], c["b"], c["a_int"], c["b_int"], emul=lambda prods: sp.emulate_gemm(c["a"], c["b"], prods), extra_int=extra)
    if c["opt"].get("bias"):
        assert bool((c["a"].abs() == c["a_int"]).all())           # one unit per column: the bias is an integer of it


@pytest.mark.parametrize("name", list(sp.NT_MUL_CASES))
def test_quantile_product_cases(name):
    c = sp.nt_mul_case(name)
    a, b = c["phi"], c["w"].t()
    _check(_mm, a, b, c["a_int"], c["b_int"], emul=lambda prods: sp.emulate_gemm(a, b, prods), extra_int=float(c["bias_int"].abs().max()))
    x = c["x"].abs().log2()
    assert torch.equal(x, x.round()) and float(x.abs().max()) <= sp.EXP                  # powers of two: the product stays exact


@pytest.mark.parametrize("name", list(sp.NT_HEAD_CASES))
def test_following_layer_cases(name):
    c = sp.nt_head_case(name)
    a, b = c["x"], c["w"].t()
    pre = _check(_mm, a, b, a, b, emul=lambda prods: sp.emulate_gemm(a, b, prods), extra_int=float(c["bias"].abs().max()))
    hidden = torch.relu(pre + c["bias"].double())
    assert float((hidden.abs() @ c["w2"].abs().double().t()).max()) + float(c["b2"].abs().max()) < sp.LIMIT
    assert bool(((c["w2"] != 0).sum(1) == 2).all()) and set(c["w2"].unique().tolist()) <= {-1.0, 0.0, 1.0}
    blocks = [set((c["w2"][o] != 0).nonzero().flatten().div(64, rounding_mode="floor").tolist()) for o in range(c["w2"].shape[0])]
    assert all(len(s) == 2 for s in blocks)                                              # the sum crosses 64-column blocks


@pytest.mark.parametrize("name", list(sp.NN_QP_CASES))
def test_feature_product_backward_cases(name):
    c = sp.nn_qp_case(name)
    g, w = c["g"], c["w"]
    d = _check(_mm, g, w, g, w, emul=lambda prods: sp.emulate_gemm(g, w, prods))
    assert set(c["emb_sparse"].unique().tolist()) == {0.0, 1.0} and bool((c["emb_dense"] == 1).all())
    # sparse setting: the column sums (db) bound the 32-row group sums (dx); x is one power of two per column
    bound = sp.abs_parts(g) @ sp.abs_parts(w)
    assert float((bound * c["emb_sparse"].double()).sum(0).max()) < sp.LIMIT
    assert bool((c["x_sparse"] == c["x_sparse"][:1]).all())
    assert bool((c["emb_sparse"].sum(0) == 2).all()) and float((d != 0).float().mean()) > 0.99
    for x in (c["x_dense"], c["x_sparse"]):
        e = x.abs().log2()
        assert torch.equal(e, e.round()) and float(e.abs().max()) <= sp.EXP


@pytest.mark.parametrize("name", list(sp.CONV_FWD_CASES))
@pytest.mark.parametrize("scale_x", [True, False])
def test_conv_forward_cases(name, scale_x):
    c = sp.conv_fwd_case(name, scale_x)
    op = sp.op_conv_fwd(c["s"])
    # the unscaled frames also run with a bias below 2^19 of each filter's unit in the epilogue
    _check(op, c["x"], c["w"], c["a_int"], c["b_int"], extra_int=0.0 if scale_x else float(2 ** 19))
    # the kernel's own index order, rows (n, oh, ow) x k = (kh, kw, c), as a GEMM in 16-wide k steps
    k = c["w"].shape[2]
    cols = torch.nn.functional.unfold(c["x"], k, stride=c["s"])                                   # (n, (c, kh, kw), positions)
    n, _, pos = cols.shape
    ch = c["x"].shape[1]
    a = cols.view(n, ch, k, k, pos).permute(0, 4, 2, 3, 1).reshape(n * pos, k * k * ch)
    b = c["w"].permute(2, 3, 1, 0).reshape(k * k * ch, -1)
    got = sp.emulate_gemm(a, b).view(n, pos, -1).permute(0, 2, 1).reshape(op(c["x"], c["w"]).shape)
    assert torch.equal(got.double(), op(c["x"].double(), c["w"].double()))


@pytest.mark.parametrize("name", list(sp.CONV_BWD_CASES))
def test_conv_data_gradient_cases(name):
    c = sp.conv_bwd_case(name)
    _check(sp.op_conv_bwd_data(c["s"]), c["g"], c["w"], c["a_int"], c["b_int"])


@pytest.mark.parametrize("name", list(sp.CONV_WRW_CASES))
def test_conv_weight_gradient_cases(name):
    c = sp.conv_wrw_case(name)
    op = sp.op_conv_wrw(c["k"], c["s"])
    want = _check(op, c["g"], c["x"], c["a_int"], c["b_int"])
    ref = torch.ops.aten.convolution_backward(c["g"].double(), c["x"].double(), want, None, [c["s"]] * 2, [0, 0], [1, 1], False, [0, 0], 1,
                                              [False, True, False])[1]
    assert torch.equal(want, ref)                                                                # op restates the weight gradient


PIXEL_PRODUCTS = ((2, 0), (1, 0), (0, 0))       # a uint8 pixel is exact in one bf16 part: lo.x, mid.x, hi.x are all there is


@pytest.mark.parametrize("name", list(sp.CONV1_FWD_CASES))
def test_input_layer_forward_cases(name):
    c = sp.conv1_fwd_case(name)
    x = c["x"].float()
    assert not any(bool(p.any()) for p in sp.split3(x)[1:])
    op = lambda w, px: torch.nn.functional.conv2d(px, w, None, 4)                                 # noqa: E731
    _check(op, c["w"], x, c["w_int"], x, products=PIXEL_PRODUCTS, shares=(True, False), extra_int=float(c["bias_int"].abs().max()))
    assert 0.0 < float((c["x"] != 0).float().mean()) < 0.02                                       # a mostly-zero image


@pytest.mark.parametrize("name", list(sp.CONV1_WRW_CASES))
def test_input_layer_weight_gradient_cases(name):
    c = sp.conv1_wrw_case(name)
    x = c["x"].float()
    op = sp.op_conv_wrw(8, 4)
    _check(op, c["g"], x, c["g_int"], x, products=PIXEL_PRODUCTS, shares=(False, False))
    live = c["g_int"] != 0
    assert bool((live.sum((0, 2, 3)) == min(5, live[:, 0].numel())).all())                         # five positions per filter
    for part, least in zip(sp.split3(c["g_int"][live]), (1.0, 0.9, 0.8)):
        assert float((part != 0).float().mean()) >= least
    kept = c["g_int"] * (c["y"] > 0)
    assert float(sp.abs_parts(kept).sum((0, 2, 3)).max()) < sp.LIMIT                               # the masked form's bias gradient
    assert 0.5 < float(((c["y"] > 0) & live).sum()) / float(live.sum()) < 1.0
    _check(op, c["g"] * (c["y"] > 0), x, kept, x, products=PIXEL_PRODUCTS, shares=(False, False))
