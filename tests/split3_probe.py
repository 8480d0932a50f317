"""Part-probing operands for the split-bf16 kernels (csrc/split3.hpp: x = hi + mid + lo, three bf16 parts; six of the
nine part products accumulated in f32: lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi) and a CPU restatement of the method.

The small-integer operands of the older bit-exact tests fit ONE bf16 part: their mid and lo planes are all zero and only
hi.hi carries the addressing.  The operands made here populate all three parts of BOTH operands and are still exact in
f32 in any summation order, so float64 is the one right answer bit for bit.  Every contraction index k belongs to one of
three classes:

  class 0  wide x sparse-hi   a = odd integer in [2^(W-1), 2^W) (W = 20: hi, mid and lo non-zero), b in {0, 1}
  class 1  sparse-hi x wide   the same with the roles swapped
  class 2  mid x mid          both odd integers in [2^9, 2^10) (hi and mid non-zero, lo zero); the sparse side
                              alternates (2a: b sparse, 2b: a sparse)

and along every contraction line the sparse operand has at most `pairs` non-zeros per class, which keeps
sum_k (|hi|+|mid|+|lo|)(a_k) (|hi|+|mid|+|lo|)(b_k) below 2^24: all parts and part products are integers, every partial
sum of them in any order is an integer below 2^24, and the three products the method drops (mid.lo, lo.mid, lo.lo)
are identically zero.  Scaling rows of either operand by powers of two keeps all of that true.

tests/test_split3_probe_cpu.py proves these properties for every case below (no GPU needed); tests/test_split3_exact_gpu.py
sends the same operands through the kernels.  A plain module, imported by both."""
import torch
import torch.nn.functional as F

SIX = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))        # (part of a, part of b), the kernels' order: smallest first
DROPPED = ((1, 2), (2, 1), (2, 2))
NAMES = {(2, 0): "lo.hi", (0, 2): "hi.lo", (1, 1): "mid.mid", (1, 0): "mid.hi", (0, 1): "hi.mid", (0, 0): "hi.hi"}
LIMIT = float(2 ** 24)
PAIRS = (5, 5, (3, 2))           # non-zero pairs per contraction line: class 0, class 1, class (2a, 2b)
# where an epilogue adds two outputs again (following layer, column sums): 2 + 2 + 2 pairs, at most
# 2 x 6 x 2^20 (1 + 2^-6) + a bias below 2^19
PAIRS_EPILOGUE, WIDE_EPILOGUE = (2, 2, (1, 1)), 20
EXP = 30                         # row / column scales 2^-EXP .. 2^EXP: the smallest part 2^-30, the largest output < 2^84


def split3(x):
    """csrc/split3.hpp g3_split4 per element: three round-to-nearest-even bf16 parts, both subtractions exact."""
    x = x.float()
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return hi, mid, lo


def abs_parts(x):
    return sum(p.abs().double() for p in split3(x))


def emulate_gemm(a, b, products=SIX, kstep=16):
    """a (M, K) . b (K, N) by the method: the chosen part products of each 16-wide k step, accumulated in f32."""
    pa, pb = split3(a), split3(b)
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k0 in range(0, a.shape[1], kstep):
        for i, j in products:
            acc += pa[i][:, k0:k0 + kstep] @ pb[j][k0:k0 + kstep, :]
    return acc


def emulate(op, a, b, products=SIX):
    """The same for any bilinear `op` (a convolution form): one f32 evaluation per part product, smallest first."""
    pa, pb = split3(a), split3(b)
    acc = None
    for i, j in products:
        t = op(pa[i], pb[j])
        acc = t if acc is None else acc + t
    return acc


# ---- value classes ------------------------------------------------------------------------------------------------------

def _odd(gen, shape, bits):
    """Odd integers in [2^(bits-1), 2^bits) whose smallest non-zero part is POSITIVE: 20 bits -> lo > 0, 10 bits -> mid = 1
    (drawn again where it is not).  With every operand entry positive no part product can cancel along a contraction line,
    so an output depends on a product as soon as ONE of its pairs carries it; signs come from the row / column scales."""
    part = 2 if bits > 16 else 1
    v = torch.randint(2 ** (bits - 2), 2 ** (bits - 1), shape, generator=gen, dtype=torch.int64).float() * 2 + 1
    for _ in range(200):
        bad = split3(v)[part] <= 0
        if not bool(bad.any()):
            return v
        v[bad] = torch.randint(2 ** (bits - 2), 2 ** (bits - 1), (int(bad.sum()),), generator=gen, dtype=torch.int64).float() * 2 + 1
    raise AssertionError("no value with a positive smallest part")


def _sign(gen, shape):
    return (torch.randint(0, 2, shape, generator=gen, dtype=torch.int64) * 2 - 1).float()


def _pow2(gen, shape, span=EXP):
    """+-2^e, e in [-span, span]"""
    return torch.exp2(torch.randint(-span, span + 1, shape, generator=gen, dtype=torch.int64).float()) * _sign(gen, shape)


def _scale(gen, shape, how):
    """how: True -> +-2^e, "sign" -> +-1, False -> 1"""
    return _pow2(gen, shape) if how is True else _sign(gen, shape) if how == "sign" else torch.ones(shape)


def _choose(gen, lines, cand, count):
    """(lines, cand) 0/1 mask with min(count, cand) ones per line."""
    if cand == 0 or count <= 0:
        return torch.zeros(lines, cand)
    order = torch.rand(lines, cand, generator=gen).argsort(1)
    return (order < count).float()


def _classes(n):
    """class of contraction index i: 0, 1, 2 (2a) and 3 (2b), interleaved so that every k quad / k half holds several"""
    i = torch.arange(n)
    c = i % 3
    return torch.where((c == 2) & (i % 6 == 5), torch.full_like(c, 3), c)


def _fill(gen, dense, sparse, cls_mask, sparse_pick, dense_bits, sparse_bits):
    """dense[..., cls] <- odd integers of dense_bits; sparse[..., cls] <- sparse_pick * (odd integers of sparse_bits, or +-1)"""
    dense[cls_mask] = _odd(gen, dense[cls_mask].shape, dense_bits)
    vals = torch.ones(sparse[cls_mask].shape) if sparse_bits == 1 else _odd(gen, sparse[cls_mask].shape, sparse_bits)
    sparse[cls_mask] = vals * sparse_pick


# ---- GEMM form -----------------------------------------------------------------------------------------------------------

def gemm_operands(M, N, K, seed, pairs=PAIRS, wide=20, scale_a=True, scale_b=True):
    """-> integer-valued a (M, K), b (K, N) float32 on the CPU, class per k, and power-of-two scales sa (M, 1) for a's rows
    and sb (1, N) for b's columns (see _scale): the operands are a * sa and b * sb."""
    gen = torch.Generator().manual_seed(seed)
    cls = _classes(K)
    a, b = torch.zeros(K, M), torch.zeros(K, N)                       # k-major while filling
    for c, (dense, sparse, count, db, sb) in enumerate(((a, b, pairs[0], wide, 1), (b, a, pairs[1], wide, 1),
                                                        (a, b, pairs[2][0], 10, 10), (b, a, pairs[2][1], 10, 10))):
        m = cls == c
        pick = _choose(gen, sparse.shape[1], int(m.sum()), count).t()   # per line of the sparse operand: `count` of the class's k
        _fill(gen, dense, sparse, m, pick, db, sb)
    a, b = a.t().contiguous(), b.contiguous()
    sa, sb = _scale(gen, (M, 1), scale_a), _scale(gen, (1, N), scale_b)
    return a, b, sa, sb


def line_bound(op, a, b):
    """max over outputs of sum (|hi|+|mid|+|lo|)(a) (|hi|+|mid|+|lo|)(b), in units of the output's power-of-two scale:
    callers pass UNSCALED operands (scales are exact and cancel)."""
    return float(op(abs_parts(a), abs_parts(b)).max())


# name -> (layout, M, N, K, options).  Options: pad_a / pad_b (operand row pitch beyond its row), ldc_pad (output into a
# column block of a wider tensor), bias (bias + ReLU epilogue: a's rows then stay unscaled), mid (the 256 x 128 tile).
GEMM_CASES = {
    "nt_one_tile":         ("nt", 256, 256, 16, {}),
    "nt_persistent_walk":  ("nt", 256 * 33, 2048, 32, {}),            # 320 workgroups wanted, 256 resident: a second tile per workgroup
    "nt_ragged":           ("nt", 300, 264, 48, {}),
    "nt_ragged_scalar":    ("nt", 300, 262, 48, {}),                  # N % 4 != 0: the scalar-store instantiation
    "nt_bias_relu":        ("nt", 513, 260, 64, {"bias": True}),
    "nt_pitched_ldc":      ("nt", 520, 328, 64, {"pad_a": 64, "pad_b": 32, "ldc_pad": 72, "bias": True}),
    "nt_mid_tile":         ("nt", 300, 260, 48, {"mid": True, "bias": True}),
    "nt_mid_tile_long":    ("nt", 6200, 900, 80, {"mid": True}),
    "nn_one_tile":         ("nn", 256, 256, 16, {}),
    "nn_ragged":           ("nn", 777, 260, 48, {}),
    "nn_ragged_scalar":    ("nn", 300, 262, 32, {}),
    "nn_pitched":          ("nn", 520, 328, 64, {"pad_a": 64, "pad_b": 24, "ldc_pad": 8}),
    "tn_one_tile":         ("tn", 256, 256, 128, {}),
    "tn_ragged_last_chunk": ("tn", 300, 260, 4112, {}),               # 257 K-steps over 8 chunks of 33: the last one holds 26
    "tn_pitched":          ("tn", 384, 512, 2048, {"pad_a": 128, "pad_b": 4, "ldc_pad": 4}),
    "tn_narrow":           ("tn", 300, 60, 1040, {}),
    "tn_narrow_full":      ("tn", 512, 64, 2064, {}),
}


def gemm_case(name):
    lay, M, N, K, opt = GEMM_CASES[name]
    seed = sum(ord(ch) for ch in name) * 7919 + M + N + K
    a, b, sa, sb = gemm_operands(M, N, K, seed, scale_a="sign" if opt.get("bias") else True)
    out = {"lay": lay, "a": a * sa, "b": b * sb, "a_int": a, "b_int": b, "opt": opt, "bias": None, "bias_int": None}
    if opt.get("bias"):
        gen = torch.Generator().manual_seed(seed + 1)
        # an integer below 2^19 in each column's own unit: sum + bias stays below 2^24 of that unit
        out["bias_int"] = torch.randint(-2 ** 19 + 1, 2 ** 19, (N,), generator=gen).float()
        out["bias"] = out["bias_int"] * sb.view(N)
    return out


# ---- the epilogue forms ------------------------------------------------------------------------------------------------

NT_MUL_CASES = {"groups_of_32": (256 + 96, 264, 64, 32), "groups_of_8": (300 * 8, 512, 64, 8), "scalar_stores": (96, 262, 32, 32)}


def nt_mul_case(name):
    """relu(phi W^T + b) * x[row // n]: phi (R, K), W (N, K), b (N,), x (R / n, N) powers of two."""
    R, N, K, n = NT_MUL_CASES[name]
    seed = 1000 + R + N + K + n
    a, b, sa, sb = gemm_operands(R, N, K, seed, scale_a="sign")
    gen = torch.Generator().manual_seed(seed + 1)
    bias = torch.randint(-2 ** 19 + 1, 2 ** 19, (N,), generator=gen).float()
    return {"phi": a * sa, "w": (b * sb).t().contiguous(), "bias": bias * sb.view(N), "x": _pow2(gen, (R // n, N)),
            "n": n, "a_int": a, "b_int": b, "bias_int": bias}


NT_HEAD_CASES = {"two_column_tiles": (300, 512, 64, 7), "ragged_columns": (257, 328, 32, 3), "one_unit": (256, 256, 16, 1)}


def nt_head_case(name):
    """hidden = relu(x W^T + b), out = hidden W2^T + b2 with W2 in {0, +-1}, two non-zeros per unit in different
    64-column blocks: |out| <= 2 max|hidden| + |b2| < 2^24."""
    M, N, K, O = NT_HEAD_CASES[name]
    seed = 2000 + M + N + K + O
    a, b, sa, sb = gemm_operands(M, N, K, seed, pairs=PAIRS_EPILOGUE, wide=WIDE_EPILOGUE, scale_a="sign", scale_b="sign")
    a, b = a * sa, b * sb
    gen = torch.Generator().manual_seed(seed + 1)
    bias = torch.randint(-2 ** 19 + 1, 2 ** 19, (N,), generator=gen).float()
    w2 = torch.zeros(O, N)
    for o in range(O):
        cols = torch.randperm(N // 64, generator=gen)[:2] * 64 + torch.randint(0, 64, (2,), generator=gen)
        w2[o, cols] = _sign(gen, (2,))
    b2 = torch.randint(-2 ** 19 + 1, 2 ** 19, (O,), generator=gen).float()
    return {"x": a, "w": b.t().contiguous(), "bias": bias, "w2": w2, "b2": b2}


NN_QP_CASES = {"one_tile_and_tail": (256 + 64, 64, 264), "two_column_tiles": (96, 32, 520)}


def nn_qp_case(name):
    """d = g w (g (M, N), w (N, K), d never stored); d_pre = (emb > 0) d x[row // 32], dx = 32-row group sums of d emb,
    db = column sums of d_pre.  Two settings of (emb, x) on the same g, w:
      dense:  emb = 1 everywhere, x = any powers of two per (group, column): d_pre exact at every output (dx, db are sums
              of up to M wide values: not exact, not compared bit for bit)
      sparse: emb in {0, 1} with two ones per column in all, x = one power of two per column: d_pre, dx and db all exact."""
    M, N, K = NN_QP_CASES[name]
    seed = 3000 + M + N + K
    g, w, sg, sw = gemm_operands(M, K, N, seed, pairs=PAIRS_EPILOGUE, wide=WIDE_EPILOGUE, scale_a="sign", scale_b="sign")   # contraction over g's N columns
    g, w = g * sg, w * sw
    gen = torch.Generator().manual_seed(seed + 1)
    emb_sparse = _choose(gen, K, M, 2).t().contiguous()
    x_cols = _pow2(gen, (1, K))
    return {"g": g, "w": w, "emb_dense": torch.ones(M, K), "x_dense": _pow2(gen, (M // 32, K)),
            "emb_sparse": emb_sparse, "x_sparse": x_cols.expand(M // 32, K).contiguous()}


# ---- convolution forms ----------------------------------------------------------------------------------------------------

def _lattice(gen, n, h, w, ph, pw):
    """(n, h, w) 0/1: one position per (ph, pw) cell, the cell offset drawn per frame: any ph x pw window holds exactly one"""
    oh, ow = torch.randint(0, ph, (n, 1, 1), generator=gen), torch.randint(0, pw, (n, 1, 1), generator=gen)
    ih, iw = torch.arange(h).view(1, h, 1), torch.arange(w).view(1, 1, w)
    return ((ih % ph == oh) & (iw % pw == ow)).float()


def conv_fwd_operands(n, c, h, w, f, k, s, seed, pairs=PAIRS, scale_x=True):
    """conv2d(x, W, stride s): contraction over (c, kh, kw), class per c.  The windowed operand x is sparse on a lattice of
    period k (exactly one position per k x k window) with `pairs` of the class's channels non-zero there; W is sparse with
    `pairs` of the class's (c, kh, kw) per filter.  -> integer-valued x (n, c, h, w), W (f, c, k, k) and their power-of-two
    scales per frame / per filter."""
    gen = torch.Generator().manual_seed(seed)
    cls = _classes(c)
    x, wt = torch.zeros(n, h, w, c), torch.zeros(f, k, k, c)
    for q, (x_dense, count, db, sb) in enumerate(((True, pairs[0], 20, 1), (False, pairs[1], 20, 1), (True, pairs[2][0], 10, 10),
                                                   (False, pairs[2][1], 10, 10))):
        m = cls == q
        nc = int(m.sum())
        if x_dense:
            pick = _choose(gen, f, k * k * nc, count).view(f, k, k, nc)
            _fill(gen, x, wt, (Ellipsis, m), pick, db, sb)
        else:
            pick = _choose(gen, n * h * w, nc, count).view(n, h, w, nc) * _lattice(gen, n, h, w, k, k).unsqueeze(-1)
            _fill(gen, wt, x, (Ellipsis, m), pick, db, sb)
    sx = _scale(gen, (n, 1, 1, 1), True if scale_x else "sign")
    sw = _pow2(gen, (f, 1, 1, 1))
    return x.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2), sx, sw     # logical NCHW, channels_last memory


CONV_FWD_CASES = {"layer2": (4, 32, 20, 20, 64, 4, 2), "layer3": (5, 64, 9, 9, 64, 3, 1), "odd": (3, 8, 11, 13, 20, 2, 1)}


def conv_fwd_case(name, scale_x=True):
    n, c, h, w, f, k, s = CONV_FWD_CASES[name]
    x, wt, sx, sw = conv_fwd_operands(n, c, h, w, f, k, s, 4000 + n + c + h + k, scale_x=scale_x)
    return {"x": x * sx, "w": wt * sw, "a_int": x, "b_int": wt, "sw": sw.view(f), "s": s}


def conv_bwd_data_operands(n, c, f, k, s, oh, ow, seed, pairs=PAIRS):
    """Data gradient of conv2d(x, W, stride s): dx[n, c, ih, iw] = sum over (f, kh, kw) of g[n, f, (ih - kh) / s, (iw - kw) / s]
    W[f, c, kh, kw]; class per f.  An input pixel gathers from ceil(k / s)^2 positions of g: g is sparse on a lattice of that
    period (at most one position per pixel); W is sparse with `pairs` of the class's (f, kh, kw) per channel AND tap residue
    (kh % s, kw % s) — the taps one pixel sees.  -> g (n, f, oh, ow), W (f, c, k, k)."""
    gen = torch.Generator().manual_seed(seed)
    cls = _classes(f)
    p = -(-k // s)
    g, wt = torch.zeros(n, oh, ow, f), torch.zeros(c, k, k, f)
    res = (torch.arange(k).view(k, 1) % s) * s + (torch.arange(k).view(1, k) % s)          # tap residue class, (k, k)
    for q, (g_dense, count, db, sb) in enumerate(((True, pairs[0], 20, 1), (False, pairs[1], 20, 1), (True, pairs[2][0], 10, 10),
                                                   (False, pairs[2][1], 10, 10))):
        m = cls == q
        nf = int(m.sum())
        if g_dense:
            pick = torch.zeros(c, k, k, nf)
            for r in range(s * s):
                taps = (res == r).nonzero()
                sel = _choose(gen, c, len(taps) * nf, count).view(c, len(taps), nf)
                pick[:, taps[:, 0], taps[:, 1]] = sel
            _fill(gen, g, wt, (Ellipsis, m), pick, db, sb)
        else:
            # lattice offset 0: it reaches the first pixel rows / columns and, for sizes 1 mod p, the last ones
            pick = _choose(gen, n * oh * ow, nf, count).view(n, oh, ow, nf) * \
                ((torch.arange(oh).view(1, oh, 1, 1) % p == 0) & (torch.arange(ow).view(1, 1, ow, 1) % p == 0)).float()
            _fill(gen, wt, g, (Ellipsis, m), pick, db, sb)
    sg, sw = _pow2(gen, (n, 1, 1, 1)), _pow2(gen, (1, c, 1, 1))
    return g.permute(0, 3, 1, 2), wt.permute(3, 0, 1, 2), sg, sw     # g NCHW-logical / channels_last memory; W (f, c, k, k)


CONV_BWD_CASES = {"layer2": (3, 32, 64, 4, 2, 9, 9), "layer2_tail": (5, 32, 64, 4, 2, 5, 7),
                  "layer3": (3, 64, 64, 3, 1, 7, 7), "layer3_tail": (5, 64, 64, 3, 1, 10, 7)}


def conv_bwd_case(name):
    n, c, f, k, s, oh, ow = CONV_BWD_CASES[name]
    g, wt, sg, sw = conv_bwd_data_operands(n, c, f, k, s, oh, ow, 5000 + n + oh + ow + k)
    return {"g": g * sg, "w": wt * sw, "a_int": g, "b_int": wt, "s": s}


def conv_wrw_operands(n, c, h, w, f, k, s, seed, pairs=PAIRS):
    """Weight gradient dW[f, c, kh, kw] = sum over (n, oh, ow) of g[n, f, oh, ow] x[n, c, s oh + kh, s ow + kw]; the class
    goes per FRAME n (a pixel is shared by overlapping windows, so a class per position would give it two).  g is sparse
    with `pairs` of the class's positions per filter; x is sparse with `pairs` interior pixels of the class's frames per
    channel and pixel residue (ih % s, iw % s) — the pixels one tap sees.  -> g (n, f, oh, ow), x (n, c, h, w)."""
    gen = torch.Generator().manual_seed(seed)
    cls = _classes(n)
    oh, ow = (h - k) // s + 1, (w - k) // s + 1
    g, x = torch.zeros(n, oh, ow, f), torch.zeros(n, h, w, c)
    ih, iw = torch.arange(h).view(h, 1), torch.arange(w).view(1, w)
    inner = ((ih >= k - 1) & (ih <= s * (oh - 1)) & (iw >= k - 1) & (iw <= s * (ow - 1)))       # seen by every tap of its residue
    if not bool(inner.any()):
        inner = torch.ones(h, w, dtype=torch.bool)
    res = (ih % s) * s + (iw % s)
    for q, (g_dense, count, db, sb) in enumerate(((True, pairs[0], 20, 1), (False, pairs[1], 20, 1), (True, pairs[2][0], 10, 10),
                                                   (False, pairs[2][1], 10, 10))):
        frames = (cls == q).nonzero().flatten()
        nfr = len(frames)
        if nfr == 0:
            continue
        if g_dense:
            pick = torch.zeros(nfr, h, w, c)
            for r in range(s * s):
                pix = ((res == r) & inner).nonzero()
                if len(pix) == 0:
                    continue
                sel = _choose(gen, c, nfr * len(pix), count).view(c, nfr, len(pix))
                pick[:, pix[:, 0], pix[:, 1]] = sel.permute(1, 2, 0)
            dense_v = _odd(gen, (nfr, oh, ow, f), db)
            sparse_v = (torch.ones(pick.shape) if sb == 1 else _odd(gen, pick.shape, sb)) * pick
            g[frames], x[frames] = dense_v, sparse_v
        else:
            pick = _choose(gen, f, nfr * oh * ow, count).view(f, nfr, oh, ow).permute(1, 2, 3, 0)
            dense_v = _odd(gen, (nfr, h, w, c), db)
            sparse_v = (torch.ones(pick.shape) if sb == 1 else _odd(gen, pick.shape, sb)) * pick
            x[frames], g[frames] = dense_v, sparse_v
    sg, sx = _pow2(gen, (1, f, 1, 1)), _pow2(gen, (1, c, 1, 1))
    return g.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2), sg, sx


CONV_WRW_CASES = {"layer2": (7, 32, 20, 20, 64, 4, 2), "layer3": (8, 64, 9, 9, 64, 3, 1), "odd": (9, 16, 11, 13, 64, 2, 1)}


def conv_wrw_case(name):
    n, c, h, w, f, k, s = CONV_WRW_CASES[name]
    g, x, sg, sx = conv_wrw_operands(n, c, h, w, f, k, s, 6000 + n + c + h + k)
    return {"g": g * sg, "x": x * sx, "a_int": g, "b_int": x, "k": k, "s": s}


# ---- the input layer: uint8 pixels (exact in one bf16 part) against split weights / a split gradient ------------------------

CONV1_FWD_CASES = {"atari": (3, 84, 84), "small": (5, 44, 52), "many_frames": (1025, 84, 84)}


def conv1_fwd_case(name):
    """relu(conv2d(x, W, b, 4)), scale 1: every weight wide (20 bits, a power-of-two scale per filter); the image is zero
    except on a lattice of period 4 — four positions per 8 x 8 window — with ONE channel there holding 1, 2 or 3: at
    most 12 (2^20 + 2^12 + 2^4) + |b| < 2^24 per output."""
    n, h, w = CONV1_FWD_CASES[name]
    gen = torch.Generator().manual_seed(7000 + n + h + w)
    wt = _odd(gen, (32, 4, 8, 8), 20)
    unit = _pow2(gen, (32,), 20)                        # signed
    lat = _lattice(gen, n, h, w, 4, 4)
    ch = torch.randint(0, 4, (n, h, w), generator=gen)
    val = torch.randint(1, 4, (n, h, w), generator=gen).float() * lat
    x = torch.zeros(n, 4, h, w).scatter_(1, ch.unsqueeze(1), val.unsqueeze(1)).to(torch.uint8)
    bias = torch.randint(-2 ** 20 + 1, 2 ** 20, (32,), generator=gen).float()
    return {"x": x, "w": wt * unit.view(32, 1, 1, 1), "bias": bias * unit, "w_int": wt, "bias_int": bias}


CONV1_WRW_CASES = {"atari": (3, 84, 84), "small": (2, 44, 52), "tiny": (3, 8, 8)}


def conv1_wrw_case(name):
    """dW = sum over positions of g x (scale 1): g wide at FIVE positions per filter (a power-of-two scale per filter), zero
    elsewhere; pixels 0..3 everywhere: at most 15 (2^20 + 2^12 + 2^4) < 2^24 per weight.  `y` is a forward activation whose
    ReLU mask keeps about four of the five positions (the masked entry point); db = the kept values' sum per filter."""
    n, h, w = CONV1_WRW_CASES[name]
    gen = torch.Generator().manual_seed(8000 + n + h + w)
    oh, ow = (h - 8) // 4 + 1, (w - 8) // 4 + 1
    pick = _choose(gen, 32, n * oh * ow, 5).view(32, n, oh, ow).permute(1, 0, 2, 3)
    g_int = _odd(gen, (n, 32, oh, ow), 20) * pick
    unit = _pow2(gen, (1, 32, 1, 1), 20)
    x = torch.randint(0, 4, (n, 4, h, w), generator=gen).to(torch.uint8)
    y = (torch.rand(n, 32, oh, ow, generator=gen) - 0.2).clamp(min=0)
    return {"x": x, "g": g_int * unit, "g_int": g_int, "y": y}


# ---- the same operations on the CPU, bilinear in (a, b) ----------------------------------------------------------------------

def op_conv_fwd(s):
    return lambda x, w: F.conv2d(x, w, None, s)


def op_conv_bwd_data(s):
    return lambda g, w: F.conv_transpose2d(g, w, None, s)


def op_conv_wrw(k, s):
    def op(g, x):
        cols = F.unfold(x.contiguous(), k, stride=s)                                    # (n, c k k, positions)
        return torch.einsum("nfp,ntp->ft", g.reshape(g.shape[0], g.shape[1], -1), cols).view(g.shape[1], x.shape[1], k, k)
    return op
