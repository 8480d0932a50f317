"""GPU: the streaming glue kernels of csrc/nnops.hip at their C entry points (rltime_amd._lib.lib.mirl_*), against the formula
in each kernel's header comment restated in plain torch float64.

Outputs that are ONE rounding of one operation (relu(y + b), emb * x, the masked gradients) are compared bit for bit with the
float32 torch expression.  Sums are held twice: on small-integer operands, for which every float32 partial sum is exact,
bit-equal to float64; on real operands within the first-order bound of the kernel's own fixed summation order,
|got - want64| <= depth * 2^-24 * S per output element (S = float64 sum of the absolute values of that element's terms, depth =
the longest chain of roundings the partition gives one term: the _depth_* functions below), and never further from float64
than twice torch's own float32 sum unless inside that bound.  A column whose terms are all masked has S = 0: its sum must
be exactly 0.  Reruns of the fixed-order kernels are bit-identical."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                       # unit roundoff of float32
WORST = {}                           # kernel output -> (worst |err| / (U * S), its depth bound): printed, not asserted


def _L():
    from rltime_amd import _lib
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, device="cuda", generator=g).float()


def _bits_equal(a, b):
    """Same float32 bit patterns (so +0.0 and -0.0 differ)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _relu_ref(v):
    return torch.where(v > 0, v, torch.zeros_like(v))           # the header's relu: +0.0 for everything not above zero


def _mask_ref(grad, act):
    return torch.where(act > 0, grad, torch.zeros_like(grad))   # g = act > 0 ? grad : 0


def _ceil(a, b):
    return -(-a // b)


# ---- depth of the fixed summation orders (roundings on the longest path of one term into the result) ------------------------
def _depth_colsum(blocks):
    """k_colsum_partials: wave w adds the partials of blocks w, w + 16, ... one after the other (at most ceil(blocks / 16) of
    them), then lane 0..63 of wave 0 adds the 16 wave sums in wave order (15 additions)."""
    return _ceil(blocks, 16) + 15


def _depth_rows(rows, blocks, c):
    """k_relu_bwd_bias_rows: a block takes rpb = ceil(rows / blocks) rows; RL = 256 / (C / 4) lanes share a column quad and lane 0
    of them adds ceil(rpb / RL) rows into its register, the LDS step adds the RL lane sums in order (RL - 1 additions), then
    the partials of all blocks go through k_colsum_partials."""
    rl = 256 // (c // 4)
    return _ceil(_ceil(rows, blocks), rl) + (rl - 1) + _depth_colsum(blocks)


def _tail_lane_rows(rpb, rl):
    """Both tail kernels walk a block's rows in chunks of 16; lane (rl = 0, cq) takes rows 0, RL, 2 RL, ... of each chunk."""
    return (rpb // 16) * _ceil(16, rl) + _ceil(rpb % 16, rl)


def _depth_tail(rows, blocks, c):
    rl = 256 // (c // 4)
    return _tail_lane_rows(_ceil(rows, blocks), rl) + (rl - 1) + _depth_colsum(blocks)


def _depth_iqn_dx(n, c):
    """k_iqn_mul_bwd, dx[m]: one rounding of the product g * emb, lane (rl, cq) adds its ceil(N / RL) rows, then RL - 1 LDS adds."""
    rl = 256 // (c // 4)
    return 1 + _ceil(n, rl) + (rl - 1)


def _depth_iqn_db(m, n, blocks, c):
    """k_iqn_mul_bwd, db: one rounding of g * x, a lane adds ceil(N / RL) rows of each of the block's gpb = ceil(M / blocks)
    groups into one register, RL - 1 LDS adds, then k_colsum_partials."""
    rl = 256 // (c // 4)
    return 1 + _ceil(m, blocks) * _ceil(n, rl) + (rl - 1) + _depth_colsum(blocks)


def _check_exact(got, want64, s_abs, what):
    assert float(s_abs.max()) < 2 ** 24, "%s: the integer operands leave the range where float32 sums are exact" % what
    assert torch.equal(got.double(), want64), "%s: %d elements differ from float64 on integer operands" % (
        what, int((got.double() != want64).sum()))


def _check_sum(got, want64, s_abs, depth, lib32, what, key):
    err = (got.double() - want64).abs()
    bound = depth * U * s_abs
    ratio = float((err / (U * s_abs).clamp(min=1e-300)).max()) if err.numel() else 0.0
    print("%s: worst |err| / (2^-24 S) = %.3f, depth bound %d" % (what, ratio, depth))
    if ratio >= WORST.get(key, (-1.0, 0))[0]:
        WORST[key] = (ratio, depth)
    assert bool((err <= bound).all()), "%s: %.3f x 2^-24 S with depth %d" % (what, ratio, depth)
    err_lib = (lib32.double() - want64).abs()
    assert bool((err <= torch.maximum(2.0 * err_lib, bound)).all()), what


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


# ---- mirl_bias_relu_rows ----------------------------------------------------------------------------------------------------
def _bias_relu_case(rows, c, seed, misalign=False):
    L = _L()
    g = _gen(seed)
    y = _randn(g, rows, c)
    b = _randn(g, c)
    flat = y.view(-1)
    n = flat.numel()
    if c > 1:
        b[c // 2] = 0.0
        b[c - 1] = -0.0
    # exact +0.0 / -0.0 inputs and sums that cancel to zero
    flat[0::7] = 0.0
    flat[3::11] = -0.0
    idx = torch.arange(n, device="cuda")[5::13]
    flat[idx] = -b[idx % c]
    assert n < 32 or (bool(((y + b) == 0).any()) and bool((y == 0).any()))
    want = _relu_ref(y + b)
    if misalign:
        buf = torch.empty(n + 4, device="cuda")
        work = buf[1:1 + n]
        work.copy_(flat)
        assert work.data_ptr() % 16 == 4
    else:
        work = y.clone().view(-1)
        assert work.data_ptr() % 16 == 0
    L.check(L.lib.mirl_bias_relu_rows(rows, c, _p(work), _p(b), _st()), "mirl_bias_relu_rows")
    assert _bits_equal(work.view(rows, c), want), (rows, c, int((work.view(rows, c) != want).sum()))


@pytest.mark.parametrize("rows,c", [
    (1, 4), (37, 4), (1023, 4), (1024, 4), (1025, 4), (4095, 4), (4097, 4),     # quad counts around the 1024-quad block
    (1, 12), (53, 12), (341, 12), (683, 12),                                     # C / 4 = 3: 1023 and 2049 quads
    (1, 20), (205, 20), (819, 20),                                               # C / 4 = 5: 1025 and 4095 quads
    (1, 64), (257, 64), (3, 512), (33, 512), (1, 1024), (17, 1024)])
def test_bias_relu_rows_vector_kernel(rows, c):
    _bias_relu_case(rows, c, 11 * rows + c)


@pytest.mark.parametrize("rows,c", [(1, 1), (300, 1), (5, 6), (171, 6), (1, 7), (147, 7), (37, 7)])
def test_bias_relu_rows_scalar_kernel(rows, c):
    _bias_relu_case(rows, c, 13 * rows + c)


@pytest.mark.parametrize("rows", [1, 4, 65])
def test_bias_relu_rows_misaligned_view_takes_the_scalar_kernel(rows):
    _bias_relu_case(rows, 64, 17 * rows, misalign=True)


def test_bias_relu_rows_past_two_to_the_31_elements():
    """The one large case: rows * C a little over 2^31 floats, in place; every index in nnops.hip is an int64_t built from int
    factors.  The last 4096 rows and rows either side of element 2^31 against torch."""
    L = _L()
    c = 1024
    rows = (1 << 21) + 4096                                   # rows * C = 2^31 + 2^22 floats, 8.6 GB
    free = torch.cuda.mem_get_info()[0]
    if free < 24 * (1 << 30):
        pytest.skip("needs 24 GB of free device memory for an 8.6 GB tensor and its checks, %.1f GB free" % (free / 2 ** 30))
    g = _gen(31)
    y = torch.empty(rows, c, device="cuda")
    chunk = 1 << 18
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        y[r0:r1] = _randn(g, r1 - r0, c)
    b = _randn(g, c)
    mid = 1 << 21                                             # the row whose first element has index 2^31
    spans = [(0, 64), (mid - 1024, mid + 1024), (rows - 4096, rows)]
    spans += [(r, r + 1) for r in range(1 << 17, mid, (1 << 17) + 4099)]
    want = [_relu_ref(y[a:z] + b) for a, z in spans]
    L.check(L.lib.mirl_bias_relu_rows(rows, c, _p(y), _p(b), _st()), "mirl_bias_relu_rows")
    for (a, z), w in zip(spans, want):
        assert _bits_equal(y[a:z], w), (a, z)
    del y, want
    torch.cuda.empty_cache()


# ---- mirl_relu_bwd_bias_rows ------------------------------------------------------------------------------------------------
def _relu_bwd(rows, c, dy, y, blocks):
    L = _L()
    g, db, partial = _nan(rows, c), _nan(c), _nan(blocks, c)
    L.check(L.lib.mirl_relu_bwd_bias_rows(rows, c, _p(dy), _p(y), _p(g), _p(db), _p(partial), blocks, _st()), "mirl_relu_bwd_bias_rows")
    return g, db


def _colsum_blocks(rows, c):
    L = _L()
    blocks = C.c_int32()
    L.check(L.lib.mirl_colsum_blocks(rows, c, C.byref(blocks)))
    return blocks.value


RELU_BWD = [(1, 4, 1), (1, 64, 1), (63, 4, 1), (63, 512, 15), (64, 64, 16), (64, 1024, 17), (65, 4, 17), (65, 64, 112),
            (65, 512, 113), (5, 64, 17), (40961, 4, 128), (40961, 64, 129), (40961, 512, 2048), (40961, 1024, 113), (40961, 64, 1),
            (40961, 512, 15), (40961, 1024, 16), (40961, 4, 112), (4000, 1024, 2048), (3000, 64, 2048), (200, 512, 128), (130, 4, 129)]


@pytest.mark.parametrize("rows,c,blocks", RELU_BWD)
def test_relu_bwd_bias_rows_integer_operands_are_bit_exact(rows, c, blocks):
    g = _gen(rows * 3 + c + blocks)
    y = _ints(g, -2, 2, rows, c)
    y.view(-1)[1::5] = -0.0                                   # both zeros: mask off
    y.view(-1)[2::9] = 0.0
    dy = _ints(g, -3, 3, rows, c)
    got, db = _relu_bwd(rows, c, dy, y, blocks)
    want = _mask_ref(dy, y)
    assert _bits_equal(got, want)
    _check_exact(db, want.double().sum(0), want.double().abs().sum(0), "db rows=%d C=%d blocks=%d" % (rows, c, blocks))
    own = _colsum_blocks(rows, c)                             # and at the block count fused.py passes
    got2, db2 = _relu_bwd(rows, c, dy, y, own)
    assert _bits_equal(got2, want) and torch.equal(db2, db)


@pytest.mark.parametrize("rows,c,blocks", RELU_BWD)
def test_relu_bwd_bias_rows_real_operands_stay_inside_the_summation_bound(rows, c, blocks):
    g = _gen(rows * 5 + c + blocks)
    y = _randn(g, rows, c).clamp(min=0)                       # about half the mask off
    y.view(-1)[1::5] = -0.0
    y[:, 1::3] = 0.0                                          # all-masked columns: their sum is exactly 0
    dy = _randn(g, rows, c)
    got, db = _relu_bwd(rows, c, dy, y, blocks)
    want = _mask_ref(dy, y)
    assert _bits_equal(got, want)
    s_abs = want.double().abs().sum(0)
    assert bool((s_abs == 0).any()) and (rows < 8 or bool((s_abs > 0).any()))
    _check_sum(db, want.double().sum(0), s_abs, _depth_rows(rows, blocks, c), want.sum(0),
               "db rows=%d C=%d blocks=%d" % (rows, c, blocks), "k_relu_bwd_bias_rows db")
    got2, db2 = _relu_bwd(rows, c, dy, y, blocks)
    assert _bits_equal(got2, got) and _bits_equal(db2, db)    # fixed partition, fixed order


# ---- mirl_iqn_mul_fwd / mirl_iqn_mul_bwd ------------------------------------------------------------------------------------
# (N, C): N below, at and above 4 * RL rows (RL = 1024 / C lanes per column quad) wherever N <= 200 reaches it
IQN_NC = [(1, 4), (3, 4), (200, 4), (7, 8), (8, 8), (200, 8), (32, 64), (33, 64), (64, 64), (200, 64), (1, 512), (7, 512), (8, 512),
          (33, 512), (200, 512), (3, 1024), (7, 1024), (8, 1024), (64, 1024)]
IQN_FWD = [(5, n, c) for n, c in IQN_NC] + [(1, 7, 4), (1, 33, 64), (4096, 3, 8), (4097, 8, 64), (8193, 1, 8), (8193, 3, 512),
                                            (4097, 1, 1024), (4096, 7, 4)]


@pytest.mark.parametrize("m,n,c", IQN_FWD)
def test_iqn_mul_fwd_in_place_and_out_of_place(m, n, c):
    L = _L()
    g = _gen(m + 7 * n + c)
    x = _randn(g, m, c)
    emb = _randn(g, m * n, c).clamp(min=0)
    x.view(-1)[0::5] = 0.0
    want = (x.unsqueeze(1) * emb.view(m, n, c)).view(m * n, c)
    out = _nan(m * n, c)
    keep = emb.clone()
    L.check(L.lib.mirl_iqn_mul_fwd(m, n, c, _p(x), _p(emb), _p(out), _st()), "mirl_iqn_mul_fwd")
    assert _bits_equal(out, want) and _bits_equal(emb, keep)
    L.check(L.lib.mirl_iqn_mul_fwd(m, n, c, _p(x), _p(emb), _p(emb), _st()), "mirl_iqn_mul_fwd")      # out == emb: in place
    assert _bits_equal(emb, want) and _bits_equal(emb, out)


def _iqn_bwd(m, n, c, g, emb, x, blocks):
    L = _L()
    d_pre, dx, db, partial = _nan(m * n, c), _nan(m, c), _nan(c), _nan(blocks, c)
    L.check(L.lib.mirl_iqn_mul_bwd(m, n, c, _p(g), _p(emb), _p(x), _p(d_pre), _p(dx), _p(db), _p(partial), blocks, _st()), "mirl_iqn_mul_bwd")
    return d_pre, dx, db


IQN_BWD = [(5, n, c) for n, c in IQN_NC] + [(1, 7, 4), (1, 33, 64), (1, 8, 1024), (2048, 3, 8), (2049, 8, 64), (5000, 7, 4), (5000, 3, 512),
                                            (2049, 1, 1024), (2048, 33, 64)]


def _iqn_ref(m, n, c, g, emb, x):
    g3, e3, x3 = g.double().view(m, n, c), emb.double().view(m, n, c), x.double().unsqueeze(1)
    on = emb.view(m, n, c) > 0
    terms_pre = torch.where(on, g3 * x3, torch.zeros_like(g3))
    return dict(d_pre32=_mask_ref((g.view(m, n, c) * x.unsqueeze(1)), emb.view(m, n, c)).view(m * n, c),
                dx=(g3 * e3).sum(1), dx_abs=(g3 * e3).abs().sum(1),
                db=terms_pre.sum((0, 1)), db_abs=terms_pre.abs().sum((0, 1)))


@pytest.mark.parametrize("m,n,c", IQN_BWD)
def test_iqn_mul_bwd_integer_operands_are_bit_exact(m, n, c):
    gen = _gen(m * 3 + n * 5 + c)
    lim = 1 if m * n > 20000 else 3
    g = _ints(gen, -lim, lim, m * n, c)
    emb = _ints(gen, -1, 3, m * n, c).clamp(min=0)            # exact zeros: mask off, the term still counts in dx (as zero)
    x = _ints(gen, -3, 3, m, c)
    ref = _iqn_ref(m, n, c, g, emb, x)
    for blocks in sorted({min(m, 2048), 1}):
        d_pre, dx, db = _iqn_bwd(m, n, c, g, emb, x, blocks)
        what = "M=%d N=%d C=%d blocks=%d" % (m, n, c, blocks)
        assert _bits_equal(d_pre, ref["d_pre32"]), what
        _check_exact(dx, ref["dx"], ref["dx_abs"], "dx " + what)
        _check_exact(db, ref["db"], ref["db_abs"], "db " + what)


@pytest.mark.parametrize("m,n,c", IQN_BWD)
def test_iqn_mul_bwd_real_operands_stay_inside_the_summation_bound(m, n, c):
    gen = _gen(m * 7 + n * 3 + c)
    g = _randn(gen, m * n, c)
    emb = _randn(gen, m * n, c).clamp(min=0)                  # about half exact zeros
    emb[:, 0] = 0.0                                           # an all-masked column: db[0] == 0 and dx[:, 0] == 0 exactly
    x = _randn(gen, m, c)
    ref = _iqn_ref(m, n, c, g, emb, x)
    lib_dx = (g.view(m, n, c) * emb.view(m, n, c)).sum(1)
    lib_db = ref["d_pre32"].sum(0)
    for blocks in sorted({min(m, 2048), 1}):
        d_pre, dx, db = _iqn_bwd(m, n, c, g, emb, x, blocks)
        what = "M=%d N=%d C=%d blocks=%d" % (m, n, c, blocks)
        assert _bits_equal(d_pre, ref["d_pre32"]), what
        assert float(ref["db_abs"][0]) == 0.0 and float(ref["dx_abs"][:, 0].max()) == 0.0
        _check_sum(dx, ref["dx"], ref["dx_abs"], _depth_iqn_dx(n, c), lib_dx, "dx " + what, "k_iqn_mul_bwd dx")
        _check_sum(db, ref["db"], ref["db_abs"], _depth_iqn_db(m, n, blocks, c), lib_db, "db " + what, "k_iqn_mul_bwd db")
        again = _iqn_bwd(m, n, c, g, emb, x, blocks)
        assert all(_bits_equal(a, b) for a, b in zip(again, (d_pre, dx, db))), what


# ---- mirl_dueling_tail_bwd / mirl_dueling_tail_bwd_w ------------------------------------------------------------------------
def _tail(rows, h1, hv, a, q, ga, gv, wo, wq, both, blocks, wgrad):
    """-> (rc, g, db, dwj); every output NaN-filled before the call."""
    L = _L()
    c = h1 + hv
    kw = max(a, q)
    g, db, partial = _nan(rows, c), _nan(c), _nan(blocks, c)
    if wgrad:
        dwj, partial_w = _nan(kw, c), _nan(blocks, kw, c)
        rc = L.lib.mirl_dueling_tail_bwd_w(rows, h1, hv, a, q, _p(ga), _p(gv), _p(wo), _p(wq), _p(both), _p(g), _p(db), _p(partial),
                                           blocks, _p(dwj), _p(partial_w), _st())
    else:
        dwj = None
        rc = L.lib.mirl_dueling_tail_bwd(rows, h1, hv, a, q, _p(ga), _p(gv), _p(wo), _p(wq), _p(both), _p(g), _p(db), _p(partial),
                                         blocks, _st())
    return rc, g, db, dwj


def _tail_ref(h1, ga, gv, wo, wq, both):
    """Float64 restatement of the header comment of k_tail_bwd / k_tail_bwd_w, with the sums of absolute terms."""
    ga, gv, wo, wq, b64 = ga.double(), gv.double(), wo.double(), wq.double(), both.double()
    d = torch.cat([ga @ wo, gv @ wq], 1)
    d_abs = torch.cat([ga.abs() @ wo.abs(), gv.abs() @ wq.abs()], 1)
    on = both > 0
    zero = torch.zeros_like(d)
    g = torch.where(on, d, zero)
    return dict(d=d, d_abs=d_abs, on=on, g=g, db=g.sum(0), db_abs=torch.where(on, d_abs, zero).sum(0),
                dwo=ga.t() @ b64[:, :h1], dwo_abs=ga.abs().t() @ b64[:, :h1].abs(),
                dwq=gv.t() @ b64[:, h1:], dwq_abs=gv.abs().t() @ b64[:, h1:].abs())


# (rows, H1, Hv, A, Q): joint widths 16 .. 1024 (RL = 64 .. 1 rows per pass), both orders of unequal branches, K <= 8
TAIL_BOTH = [(1, 8, 8, 1, 1), (15, 4, 12, 6, 1), (16, 12, 4, 1, 8), (17, 32, 32, 8, 8), (33, 48, 16, 6, 1), (1000, 16, 48, 8, 8),
             (17, 96, 32, 6, 1), (1000, 32, 96, 1, 8), (33, 64, 64, 8, 8), (40961, 96, 32, 1, 1),
             (15, 128, 128, 6, 1), (1000, 192, 64, 8, 8), (33, 64, 192, 1, 8), (16, 252, 4, 1, 1),
             (17, 256, 256, 8, 8), (1000, 384, 128, 6, 1), (33, 128, 384, 1, 8), (1, 500, 12, 6, 1),
             (16, 512, 512, 6, 1), (1000, 768, 256, 8, 8), (33, 256, 768, 1, 8), (15, 512, 512, 1, 1), (40961, 768, 256, 6, 1),
             (40961, 4, 12, 8, 8)]
# K in 9 .. 16: only the plain kernel
TAIL_PLAIN = [(1, 8, 8, 9, 1), (17, 4, 12, 16, 1), (33, 32, 32, 1, 16), (1000, 96, 32, 16, 16), (15, 32, 96, 13, 5),
              (16, 128, 128, 9, 1), (1000, 64, 192, 13, 5), (33, 256, 256, 16, 16), (1000, 384, 128, 9, 1), (17, 128, 384, 1, 16),
              (16, 512, 512, 16, 1), (1000, 768, 256, 13, 5), (33, 256, 768, 16, 16), (40961, 512, 512, 9, 1), (40961, 32, 96, 5, 13),
              (1000, 768, 256, 5, 13)]


def _tail_inputs(rows, h1, hv, a, q, integer, seed):
    g = _gen(seed)
    c = h1 + hv
    if integer:
        ga, gv = _ints(g, -2, 2, rows, a), _ints(g, -2, 2, rows, q)
        wo, wq = _ints(g, -2, 2, a, h1), _ints(g, -2, 2, q, hv)
        both = _ints(g, -2, 3, rows, c).clamp(min=0)
    else:
        ga, gv = _randn(g, rows, a), _randn(g, rows, q)
        wo, wq = _randn(g, a, h1), _randn(g, q, hv)
        both = _randn(g, rows, c).clamp(min=0)
        both[:, 1::7] = 0.0                                   # all-masked columns
    assert bool((both == 0).any())
    return ga, gv, wo, wq, both


def _tail_blocks(rows, c):
    """The block count fused.py passes and, for rows that allow it, one that leaves trailing blocks empty."""
    own = _colsum_blocks(rows, c)
    return sorted({own, 17 if rows <= 33 else 113})


@pytest.mark.parametrize("rows,h1,hv,a,q", TAIL_BOTH + TAIL_PLAIN)
def test_dueling_tail_bwd_integer_operands_are_bit_exact(rows, h1, hv, a, q):
    L = _L()
    ga, gv, wo, wq, both = _tail_inputs(rows, h1, hv, a, q, True, rows + h1 * 3 + hv * 5 + a * 7 + q)
    ref = _tail_ref(h1, ga, gv, wo, wq, both)
    assert float(ref["d_abs"].max()) < 2 ** 24
    for wgrad in ((False, True) if max(a, q) <= 8 else (False,)):
        for blocks in _tail_blocks(rows, h1 + hv):
            what = "rows=%d H1=%d Hv=%d A=%d Q=%d blocks=%d w=%d" % (rows, h1, hv, a, q, blocks, wgrad)
            rc, g, db, dwj = _tail(rows, h1, hv, a, q, ga, gv, wo, wq, both, blocks, wgrad)
            L.check(rc, what)
            assert torch.equal(g.double(), ref["g"]), "g " + what
            assert bool((g[~ref["on"]].view(torch.int32) == 0).all()), "masked elements are +0.0 " + what
            _check_exact(db, ref["db"], ref["db_abs"], "db " + what)
            if wgrad:
                _check_exact(dwj[:a, :h1], ref["dwo"], ref["dwo_abs"], "dwo " + what)
                _check_exact(dwj[:q, h1:], ref["dwq"], ref["dwq_abs"], "dwq " + what)


@pytest.mark.parametrize("rows,h1,hv,a,q", TAIL_BOTH + TAIL_PLAIN)
def test_dueling_tail_bwd_real_operands_stay_inside_the_summation_bounds(rows, h1, hv, a, q):
    L = _L()
    c = h1 + hv
    ga, gv, wo, wq, both = _tail_inputs(rows, h1, hv, a, q, False, rows * 3 + h1 + hv * 7 + a * 5 + q)
    ref = _tail_ref(h1, ga, gv, wo, wq, both)
    # per element K roundings of the K <= 16 term dot product (one product and up to K - 1 additions per term)
    kcol = torch.cat([torch.full((h1,), float(a)), torch.full((hv,), float(q))]).cuda().double()
    d32 = torch.cat([ga @ wo, gv @ wq], 1)
    lib_g = _mask_ref(d32, both)
    for wgrad in ((False, True) if max(a, q) <= 8 else (False,)):
        for blocks in _tail_blocks(rows, c):
            what = "rows=%d H1=%d Hv=%d A=%d Q=%d blocks=%d w=%d" % (rows, h1, hv, a, q, blocks, wgrad)
            rc, g, db, dwj = _tail(rows, h1, hv, a, q, ga, gv, wo, wq, both, blocks, wgrad)
            L.check(rc, what)
            assert bool((g[~ref["on"]].view(torch.int32) == 0).all()), "masked elements are +0.0 " + what
            err = (g.double() - ref["g"]).abs()
            assert bool((err <= kcol * U * ref["d_abs"]).all()), "g " + what
            # db: the terms are those dot products (K roundings each) and then go through the row partition
            depth = _depth_tail(rows, blocks, c)
            assert bool((ref["db_abs"][1::7] == 0).all())
            _check_sum(db, ref["db"], ref["db_abs"], depth + max(a, q), lib_g.sum(0), "db " + what, "k_tail_bwd%s db" % ("_w" if wgrad else ""))
            if wgrad:
                # dwj: one rounding of the product ga * both, then the same partition
                _check_sum(dwj[:a, :h1], ref["dwo"], ref["dwo_abs"], depth + 1, ga.t() @ both[:, :h1], "dwo " + what, "k_tail_bwd_w dwo")
                _check_sum(dwj[:q, h1:], ref["dwq"], ref["dwq_abs"], depth + 1, gv.t() @ both[:, h1:], "dwq " + what, "k_tail_bwd_w dwq")
            rc2, g2, db2, dwj2 = _tail(rows, h1, hv, a, q, ga, gv, wo, wq, both, blocks, wgrad)
            assert _bits_equal(g2, g) and _bits_equal(db2, db) and (not wgrad or _bits_equal(dwj2, dwj)), what


@pytest.mark.parametrize("h1,hv,a,q,wgrad", [
    (32, 32, 17, 1, False), (32, 32, 1, 17, False), (32, 32, 9, 1, True), (32, 32, 1, 9, True), (32, 32, 17, 1, True),
    (30, 34, 4, 1, False), (30, 34, 4, 1, True), (32, 16, 4, 1, False), (32, 16, 4, 1, True), (6, 10, 4, 1, False)])
def test_dueling_tail_bwd_refusals_write_nothing(h1, hv, a, q, wgrad):
    """Outputs per branch above 16 (8 with weight gradients), H1 % 4 != 0 and joint widths that are not 4 * 2^k: MIRL_ERR_ARG,
    and every output buffer keeps its NaN fill.  All pointers are valid, nothing is launched."""
    L = _L()
    rows = 40
    ga, gv, wo, wq, both = _tail_inputs(rows, h1, hv, a, q, False, 5)
    rc, g, db, dwj = _tail(rows, h1, hv, a, q, ga, gv, wo, wq, both, 3, wgrad)
    torch.cuda.synchronize()
    assert rc == L.MIRL_ERR_ARG
    assert bool(torch.isnan(g).all()) and bool(torch.isnan(db).all())
    assert dwj is None or bool(torch.isnan(dwj).all())


def test_print_worst_observed_ratios():
    """Record only: the worst |err| / (2^-24 S) seen by the real-operand tests of this run, next to the depth bound it was held
    to (docs/parity.md keeps the table)."""
    for key in sorted(WORST):
        print("%-28s worst %.3f  depth %d" % (key, WORST[key][0], WORST[key][1]))
