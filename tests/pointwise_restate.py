"""Float64 restatements of the pointwise arithmetic that decides what is learned, written from the reference's formulas
(not from the kernels), for tests/test_pointwise_restate_cpu.py (which proves them against oracle/qmath.py, torch autograd,
torch.optim.Adam and torch.nn.LSTMCell) and the GPU tests of csrc/qmath.hip, optim.hip, lstm.hip, acting.hip and convert.hip:

  value rescaling h / h^-1            rltime/training/torch/torch_trainer.py:46-78
  n-step target tail                  torch_trainer.py:96-147: h(ret + float32(gamma)^n * h^-1(v) * mask)
  double-Q selection (first maximum)  training/torch/dqn.py:52-71
  IQN selection (argmax of the mean)  training/torch/iqn.py:36-52
  Huber / MSE and their derivative    dqn.py:105-111
  pairwise quantile-Huber loss        iqn.py:77-120 (the indicator td < 0 is detached: td == 0 has penalty tau and gradient
                                      0, |td| == kappa is the quadratic branch)
  clip_grad_norm_ + Adam              torch_trainer.py:177-199, coef = min(clip / (norm + 1e-6), 1), bias corrections from
                                      each tensor's own step
  LSTM cell with state reset          models/torch/modules/lstm.py:83-116
  LSTM time loop over T steps         the same lines: forward sweep and its backward (for csrc/lstm_seq.hip)
  actor head                          policies/torch/dqn.py:74-87,140-141, policies/torch/iqn.py, exploration/
                                      epsilon_greedy.py:74-100
  conv + ReLU, linear layers          models/torch/modules/cnn.py:43-50, dqn.py:50-66 (for csrc/actnet.hip)
  quantile embedding product          policies/torch/iqn.py:67-106: relu(cos(pi i tau) W^T + b) * features
  acting pre-step, episode statistics acting/actor.py:124-131, modules/lstm.py:131-161, training/policy_trainer.py:75-136,252-254
  frame-stack shift                   env_wrappers/common.py:141-178 under an auto-resetting vector env
  synthetic env draws, frame -> f32   acting/synthetic_env.py; modules/cnn.py:44-45 (NumPy, exact: for csrc/acting.hip, convert.hip)

Every function computes in the dtype of its inputs (call it with float64 tensors).  The module also holds the dyadic
operand generators: operands for which every sum a kernel can form is a float32 number, so that float32 arithmetic in any
order equals float64 bit for bit, with the ties and kinks planted that a kernel must break the reference's way."""
import math

import numpy as np
import torch


# ---- value rescaling and the target tail ---------------------------------------------------------------------------------------
def vf_scale(x, eps):
    if not eps:
        return x
    return torch.sign(x) * (torch.sqrt(torch.abs(x) + 1) - 1) + eps * x


def vf_unscale(y, eps, round32=False):
    """The closed-form h^-1.  The reference evaluates it in float64 and returns float32: round32 repeats that rounding."""
    if not eps:
        return y
    a = torch.abs(y)
    x = a / eps - (1 / (2. * eps ** 2)) * torch.sqrt(4 * eps * a + (2. * eps + 1) ** 2) + (2. * eps + 1) / (2. * eps ** 2)
    x = x * torch.sign(y)
    return x.float().to(y.dtype) if round32 else x


def gamma32(gamma):
    """The base the reference's float32 tensor arithmetic raises to the n-th power."""
    return float(np.float32(gamma))


def nstep_target(v, returns, nsteps, masks, gamma, vf_eps, round32=False):
    """v (M,) or (M, Nt); returns / nsteps / masks (M,)."""
    if v.dim() == 2:
        returns, nsteps, masks = (t.unsqueeze(-1) for t in (returns, nsteps, masks))
    disc = torch.pow(torch.full_like(nsteps, gamma32(gamma)), nsteps)
    return vf_scale(returns + disc * vf_unscale(v, vf_eps, round32) * masks, vf_eps)


def first_max(q):
    """Index of the first maximum along the last dimension (what torch.argmax documents), without argmax."""
    A = q.shape[-1]
    idx = torch.arange(A).expand(q.shape)
    return torch.where(q == q.max(-1, keepdim=True).values, idx, torch.full_like(idx, A)).min(-1).values


def dqn_bootstrap(q_target, q_select):
    return q_target.gather(-1, first_max(q_select).unsqueeze(-1)).squeeze(-1)


def iqn_select(z_select):
    """(M, Ns, A) -> (M,) first maximum of the quantile mean."""
    return first_max(z_select.sum(1) / z_select.shape[1])


def iqn_bootstrap(z_target, z_select, best=None):
    best = iqn_select(z_select) if best is None else best
    return z_target[torch.arange(z_target.shape[0]), :, best]                 # (M, Nt)


# ---- losses ------------------------------------------------------------------------------------------------------------------
def huber(e, kappa):
    """-> (value, derivative); |e| == kappa is the quadratic branch."""
    a = e.abs()
    quad = a <= kappa
    return torch.where(quad, 0.5 * e * e, kappa * (a - 0.5 * kappa)), torch.where(quad, e, kappa * torch.sign(e))


def mse(e):
    return e * e, 2 * e


def dqn_loss(q, actions, targets, weights=None, kappa=1.0, mode="huber", row_scale=1.0):
    """-> (weighted row loss (M,), signed td (M,), dense d(row_scale * sum_m row_m) / dq (M, A))."""
    M, A = q.shape
    rows = torch.arange(M)
    td = q[rows, actions] - targets
    val, grad = mse(td) if mode == "mse" else huber(td, kappa)
    w = torch.ones_like(td) if weights is None else weights
    dq = torch.zeros_like(q)
    dq[rows, actions] = grad * w * row_scale
    return val * w, td, dq


def iqn_pairs(z, taus, actions, targets, kappa=1.0):
    """The pairwise sums of one transition: td[m, i, j] = y_i - theta_j, penalty |tau_j - 1{td < 0}|.
    -> dict(td, loss_sum (M,) = sum_ij pen huber / kappa, abs_sum (M,) = sum_ij |td|,
            gsum (M, N) = -sum_i pen huber' / kappa, the derivative of loss_sum in theta_j)."""
    M, N, _ = z.shape
    theta = z[torch.arange(M), :, actions]                                    # (M, N)
    td = targets.unsqueeze(2) - theta.unsqueeze(1)                            # (M, Nt, N)
    val, grad = huber(td, kappa)
    pen = (taus.view(M, 1, N) - (td < 0).to(z.dtype)).abs()
    return {"td": td, "loss_sum": (pen * val / kappa).sum((1, 2)), "abs_sum": td.abs().sum((1, 2)),
            "gsum": -(pen * grad / kappa).sum(1), "loss_terms": pen * val / kappa, "g_terms": pen * grad / kappa}


def iqn_loss(z, taus, actions, targets, weights=None, kappa=1.0, row_scale=1.0):
    """-> (weighted row loss (M,), mean |td| (M,), dense d(row_scale * sum_m row_m) / dz (M, N, A))."""
    M, N, _ = z.shape
    Nt = targets.shape[1]
    s = iqn_pairs(z, taus, actions, targets, kappa)
    w = torch.ones_like(s["loss_sum"]) if weights is None else weights
    dz = torch.zeros_like(z)
    dz[torch.arange(M), :, actions] = s["gsum"] * (w * row_scale / Nt).unsqueeze(1)
    return s["loss_sum"] / Nt * w, s["abs_sum"] / (Nt * N), dz


# ---- clip + Adam -------------------------------------------------------------------------------------------------------------
def global_norm(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


def clip_coef(norm, clip):
    """clip_grad_norm_: min(clip / (norm + 1e-6), 1); clip 0 or None: no clipping."""
    return min(clip / (norm + 1e-6), 1.0) if clip else 1.0


def adam_step(p, g, m, v, step, lr, beta1, beta2, eps, coef=1.0):
    """One Adam step (amsgrad off, no weight decay) of one tensor whose counter stands at `step` before it.
    -> (p, clipped g, exp_avg, exp_avg_sq, step + 1)."""
    t = step + 1
    g = g * coef
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    return p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps), g, m, v, t


# ---- LSTM cell ---------------------------------------------------------------------------------------------------------------
def lstm_cell_fwd(pre, c_in, keep_next=None):
    """pre (B, 4H) pre-activations in the order i, f, g, o -> (activated gates (B, 4H), h, c, h_next, c_next)."""
    i, f, g, o = pre.chunk(4, dim=1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_in + i * g
    h = o * torch.tanh(c)
    k = 1.0 if keep_next is None else keep_next.unsqueeze(1)
    return torch.cat([i, f, g, o], 1), h, c, h * k, c * k


def lstm_cell_bwd(gates, c_t, c_in, d_out=None, dh_rec=None, dc_rec=None, keep_next=None, first=False):
    """gates: ACTIVATED (B, 4H).  d_out: gradient of the step's output h; dh_rec / dc_rec: gradients w.r.t. the next step's
    masked inputs h * keep, c * keep (ignored when `first`, the sweep's first = the sequence's last step).
    -> (d pre-activation (B, 4H), d c_in)."""
    i, f, g, o = gates.chunk(4, dim=1)
    k = 1.0 if keep_next is None else keep_next.unsqueeze(1)
    zero = torch.zeros_like(c_t)
    dh = (zero if d_out is None else d_out) + (zero if first else dh_rec * k)
    tc = torch.tanh(c_t)
    dc = (zero if first else dc_rec * k) + dh * o * (1 - tc * tc)
    return torch.cat([dc * g * i * (1 - i), dc * c_in * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1), dc * f


# ---- LSTM time loop ----------------------------------------------------------------------------------------------------------
def lstm_sweep_fwd(gx, w_hh, h0, c0, keep):
    """The reference's time loop (modules/lstm.py:83-116) on given input projections: gx (T, B, 4H) = x W_ih^T + b, w_hh (4H, H),
    h0 / c0 (B, H) the state before step 0, keep (T, B) = 1 - initials.  Step t multiplies the state by keep[t], then runs the cell.
    -> (out (T, B, H), c_all (T, B, H), activated gates (T, B, 4H), hm, cm (T + 1, B, H)): hm[t] / cm[t] are the masked state
    step t is given (hm[0] = h0 keep[0], hm[t + 1] = out[t] keep[t + 1]); row T is the final state, unmasked."""
    T, B, _ = gx.shape
    H = h0.shape[1]
    hm, cm = gx.new_zeros(T + 1, B, H), gx.new_zeros(T + 1, B, H)
    out, c_all, gates = gx.new_zeros(T, B, H), gx.new_zeros(T, B, H), torch.zeros_like(gx)
    hm[0], cm[0] = h0 * keep[0].unsqueeze(1), c0 * keep[0].unsqueeze(1)
    for t in range(T):
        kn = keep[t + 1] if t + 1 < T else None
        gates[t], out[t], c_all[t], hm[t + 1], cm[t + 1] = lstm_cell_fwd(gx[t] + hm[t] @ w_hh.t(), cm[t], kn)
    return out, c_all, gates, hm, cm


def lstm_sweep_bwd(gates, c_all, cm, d_out, keep, w_hh):
    """gates: ACTIVATED (T, B, 4H); c_all (T, B, H); cm (T + 1, B, H) as lstm_sweep_fwd returns them; d_out (T, B, H) the gradient
    of out, or None.  -> d loss / d pre-activation (T, B, 4H): the cell's backward from the last step to the first, with
    dh_rec(t) = dgates(t + 1) @ w_hh and dc_rec(t) = d c_in(t + 1), both through keep[t + 1]."""
    T = gates.shape[0]
    dg = torch.zeros_like(gates)
    dh_rec = dc_rec = None
    for t in range(T - 1, -1, -1):
        first = t == T - 1
        dg[t], dc_rec = lstm_cell_bwd(gates[t], c_all[t], cm[t], None if d_out is None else d_out[t], dh_rec, dc_rec,
                                      None if first else keep[t + 1], first)
        dh_rec = dg[t] @ w_hh
    return dg


def selector_whh(seed, H):
    """A (4H, H) recurrent matrix with ONE non-zero per row, +- 2^-e with e in 0..3: row gate * H + j reads column
    k = (stride j + offset(gate)) mod H.  stride is odd, coprime to H and neither 1 nor -1 mod H (neighbouring hidden units do not
    read neighbouring k); the offsets gate * (H / 4 + 1) differ, so the four gates of a hidden unit read four different k, and every
    k is read by exactly one row of each gate.  The recurrent sum of a gate column is then ONE exact product (a pre-activation
    carries a single rounding) and a backward dh_rec a four-term sum."""
    assert H % 4 == 0 and H >= 16
    g = torch.Generator().manual_seed(seed)
    cands = (5, 7, 11, 13, 3)
    stride = next(s for s in (cands[(seed + n) % 5] for n in range(5)) if math.gcd(s, H) == 1 and s % H not in (1, H - 1))
    j = torch.arange(H)
    w = torch.zeros(4 * H, H, dtype=torch.float64)
    for gate in range(4):
        k = (stride * j + gate * (H // 4 + 1)) % H
        val = (2.0 * torch.randint(0, 2, (H,), generator=g).double() - 1) * 2.0 ** -torch.randint(0, 4, (H,), generator=g).double()
        w[gate * H + j, k] = val
    return w


# float32 emulations (NumPy, CPU only) of the activation forms of csrc/lstm_seq.hip: exp as exp2 of the log2(e)-scaled argument,
# every operation rounded to float32.  Correctly rounded where the hardware instructions are within 1 ulp: they are used to show
# that a float32 evaluation of these forms stays inside the derived bounds of tests/test_lstm_seq_exact_gpu.py.
_LOG2E_F32 = np.float32(1.4426950408889634)


def _exp_f32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2((x * _LOG2E_F32).astype(np.float64)).astype(np.float32)


def sq_sigmoid_f32(x):
    """1 / (1 + exp(-x))."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + _exp_f32(-x))).astype(np.float32)


def sq_tanh_f32(x):
    """1 - 2 / (exp(2x) + 1): cancels near 0, its error there is absolute."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        r = (np.float32(1) / (_exp_f32(np.float32(2) * x) + np.float32(1))).astype(np.float32)
    return (np.float32(1) - np.float32(2) * r).astype(np.float32)


# ---- actor head --------------------------------------------------------------------------------------------------------------
def actor_qvalues(adv, val=None):
    """adv (E, N, A), val (E, N) or None -> (E, A): dueling combine V + A - mean_a A, then the mean over N."""
    x = adv if val is None else val.unsqueeze(-1) + adv - adv.sum(-1, keepdim=True) / adv.shape[-1]
    return x.sum(1) / x.shape[1]


def eps_per_actor(eps, expo, eps_min, E):
    """max(eps ** expo_e, eps_min) per actor in float64 (expo None: exponent 1)."""
    ex = torch.ones(E, dtype=torch.float64) if expo is None else expo.double()
    return torch.clamp(torch.pow(torch.full((E,), float(eps), dtype=torch.float64), ex), min=eps_min)


def eps_greedy(greedy, eps_used32, u, rnd):
    """Remap: the random action where u < float32(eps used)."""
    return torch.where(u.float() < eps_used32.float(), rnd.to(greedy.dtype), greedy)


# ---- the acting network's layers -----------------------------------------------------------------------------------------------
def conv_patches_nhwc(x, k, s):
    """x (F, Hi, Wi, C) -> (F, Ho, Wo, k * k * C): the input pixels under every output pixel, tap-major, channel fastest."""
    F_, Hi, Wi, _ = x.shape
    Ho, Wo = (Hi - k) // s + 1, (Wi - k) // s + 1
    taps = [x[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s, :] for ky in range(k) for kx in range(k)]
    return torch.cat(taps, dim=-1)


def conv_relu_nhwc(x, w, b, k, s, pre=False):
    """Conv2d (no padding) + ReLU over channels-last frames: x (F, Hi, Wi, C), w (Co, C, k, k), b (Co,) -> (F, Ho, Wo, Co);
    y[f, oy, ox, o] = relu(b[o] + sum_{ky, kx, c} x[f, oy s + ky, ox s + kx, c] w[o, c, ky, kx]).  pre: without the ReLU."""
    w_taps = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    y = conv_patches_nhwc(x, k, s) @ w_taps.t() + b
    return y if pre else torch.clamp(y, min=0)


def linear(x, w, b=None):
    y = x @ w.t()
    return y if b is None else y + b


def cos_embed_pre(taus, freq, wq, bq):
    """taus (R,), freq (D,) -> (phi (R, D) = cos(freq tau), phi wq^T + bq (R, H))."""
    phi = torch.cos(freq.unsqueeze(0) * taus.unsqueeze(1))
    return phi, linear(phi, wq, bq)


def cos_embed_product(taus, freq, wq, bq, h, N):
    """x[m] = relu(cos(freq tau_m) wq^T + bq) * h[m // N]."""
    return torch.clamp(cos_embed_pre(taus, freq, wq, bq)[1], min=0) * h.repeat_interleave(N, dim=0)


def head_shares(x, wfc, bfc, wout):
    """hid = relu(x wfc^T + bfc) (R, HID); share cb of the output layer = hid[:, 64 cb : 64 cb + 64] wout[:, the same]^T.
    -> (hid, shares (ceil(HID / 64), R, NO))."""
    hid = torch.clamp(linear(x, wfc, bfc), min=0)
    HID = hid.shape[1]
    return hid, torch.stack([hid[:, c:c + 64] @ wout[:, c:c + 64].t() for c in range(0, HID, 64)])


def philox_4x32(seed, call, lane):
    """Philox4x32-10 (Salmon et al., SC'11), key (seed lo, seed hi), counter (lane, call lo, call hi, tag) -> four 32-bit
    words: the acting heads draw u = (word 0 >> 8) / 2^24 and the random action (word 1 * A) >> 32 per env."""
    M0, M1, MASK = 0xD2511F53, 0xCD9E8D57, 0xFFFFFFFF
    c = [lane & MASK, call & MASK, (call >> 32) & MASK, 0x52544D45]
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c[3] ^ k1) & MASK, p0 & MASK]
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c


def philox_head_draws(seed, step, E, A):
    """-> (u (E,) float32, random action (E,) int64) of one (seed, step)."""
    w = [philox_4x32(seed, step, e) for e in range(E)]
    u = torch.tensor([(x[0] >> 8) / 16777216.0 for x in w], dtype=torch.float64).float()
    return u, torch.tensor([(x[1] * A) >> 32 for x in w], dtype=torch.int64)


# ---- dyadic operands ---------------------------------------------------------------------------------------------------------
def _ints(g, lo, hi, *shape):
    return torch.randint(int(lo), int(hi) + 1, shape, generator=g).double()


def dyadic_conv(seed, layer, frames, Hi, Wi):
    """Layer 2 (32 -> 64 channels, 4x4, stride 2) or 3 (64 -> 64, 3x3, stride 1) of the acting network.  x in {-1, 0, 1} / 2 (half
    of them 0), w in {-2 .. 2} / 4: products are multiples of 1/8 bounded by 1/2, K = 512 / 576 of them per output.  The bias is
    planted per channel: minus the most frequent value of the channel's sums (even channels: that many pre-activations are
    exactly 0) and one eighth less (odd channels: the same pixels come out at -1/8)."""
    ci, k, s = (32, 4, 2) if layer == 2 else (64, 3, 1)
    g = torch.Generator().manual_seed(seed)
    x = _ints(g, -1, 1, frames, Hi, Wi, ci) * _ints(g, 0, 1, frames, Hi, Wi, ci) / 2
    w = _ints(g, -2, 2, 64, ci, k, k) / 4
    sums = conv_relu_nhwc(x, w, torch.zeros(64, dtype=torch.float64), k, s, pre=True).reshape(-1, 64)
    b = -sums.mode(dim=0).values
    b[1::2] -= 0.125
    return {"x": x, "w": w, "b": b, "k": k, "s": s, "margin": exact_sum_margin(k * k * ci, 0.5, 0.125) + float(b.abs().max()) * 8}


def dyadic_lstm(seed, E, H, K):
    """xh in {-1, 0, 1} / 2, w in {-2 .. 2} / 16, bias multiples of 1/32 in [-1, 1]: products are multiples of 1/32 bounded by
    1/16, K of them per gate: the pre-activations are exact whatever the slices, waves and shares add first.  c_in is real."""
    g = torch.Generator().manual_seed(seed)
    xh, w = _ints(g, -1, 1, E, K) / 2, _ints(g, -2, 2, 4 * H, K) / 16
    b = _ints(g, -32, 32, 4 * H) / 32
    c_in = torch.randn(E, H, generator=g).double()
    return {"xh": xh, "w": w, "b": b, "c_in": c_in, "margin": exact_sum_margin(K, 1.0 / 16, 1.0 / 32) + 32}


def dyadic_hidden(seed, R, H, HID, NO):
    """x in {-1, 0, 1} / 2, wfc in {-2 .. 2} / 4, bfc multiples of 1/8 in [-2, 2]: hid is a multiple of 1/8 bounded by H / 2 + 2;
    wout in {-2 .. 2} / 2: a share adds 64 multiples of 1/16 bounded by H / 2 + 2, all shares HID of them."""
    g = torch.Generator().manual_seed(seed)
    x, wfc = _ints(g, -1, 1, R, H) / 2, _ints(g, -2, 2, HID, H) / 4
    bfc, wout = _ints(g, -16, 16, HID) / 8, _ints(g, -2, 2, NO, HID) / 2
    return {"x": x, "wfc": wfc, "bfc": bfc, "wout": wout,
            "margin": max(exact_sum_margin(H, 0.5, 0.125) + 16, exact_sum_margin(HID, H / 2 + 2, 1.0 / 16))}


def dyadic_head_parts(seed, E, N, A, P, has_val):
    """Output shares for the selection: adv, val multiples of 1/8 as in dyadic_actor_head, any N and A.  Where A is no power of
    two every row's advantages are made to add up to a multiple of A / 8 (one untied action takes up the remainder), so that
    mean_a A is a multiple of 1/8; the quantile mean is ONE division of an exact sum, correctly rounded in float32 and equal to the
    rounded float64 quotient (53 >= 2 * 24 + 2 bits).  Every env has its best q-value planted on two actions (A >= 2), the first
    must win.  out = bout + P shares: bout multiples of 1/8, shares multiples of 1/8.
    -> dict(adv (E, N, A), val (E, N) or None, first (E,), parts (P, E * N, NO), bout (NO,))."""
    g = torch.Generator().manual_seed(seed)
    adv = _ints(g, -32, 24, E, N, A) / 8
    val = _ints(g, -32, 32, E, N) / 8 if has_val else None
    first = torch.zeros(E, dtype=torch.int64)
    fix = has_val and A & (A - 1) != 0
    if A >= 2:
        for e in range(E):
            a, b, c = torch.randperm(A, generator=g)[:3].tolist() if A >= 3 else (0, 1, 0)
            a, b = min(a, b), max(a, b)
            adv[e, :, a] = 3.5
            adv[e, :, b] = 3.5
            if N >= 2:
                adv[e, 0, a], adv[e, 1, a] = 4.0, 3.0
            if fix:
                adv[e, :, c] = -2.0
                rem = torch.remainder(adv[e].sum(-1) * 8, A)
                adv[e, :, c] -= rem / 8
            first[e] = a
    NO = A + (1 if has_val else 0)
    out = adv.reshape(E * N, A) if val is None else torch.cat([adv.reshape(E * N, A), val.reshape(E * N, 1)], 1)
    bout = _ints(g, -16, 16, NO) / 8
    parts = _ints(g, -64, 64, P, E * N, NO) / 8
    parts[P - 1] = out - bout - parts[:P - 1].sum(0)
    return {"adv": adv, "val": val, "first": first, "parts": parts, "bout": bout,
            "margin": max(exact_sum_margin(N, 16.0, 1.0 / 8), exact_sum_margin(A, 6.0, 1.0 / 8),
                          exact_sum_margin(P + 1, float(parts.abs().max()), 1.0 / 8))}


def _halves(g, lo, hi, *shape):
    """Multiples of 1/2 in [lo, hi]."""
    return torch.randint(int(2 * lo), int(2 * hi) + 1, shape, generator=g).double() / 2


def exact_sum_margin(n_terms, max_term, granularity):
    """max |partial sum| / granularity of any partial sum of n_terms multiples of `granularity` bounded by max_term: below
    2^24 every such sum is a float32 number."""
    return n_terms * max_term / granularity


def dyadic_loss_iqn(seed, M, N, Nt, A, kappa, acted="lo", weights=True):
    """theta, y: multiples of 1/2 in [-2, 2]; tau: multiples of 1/16 in [0, 1]; weights / row_scale: powers of two.
    Planted: one pair with td == 0 and one with |td| == kappa (M * N * Nt >= 2).
    Terms pen * huber / kappa are multiples of 2^-8 bounded by 4 (kappa in {0.5, 1, 2}), N * Nt <= 8192 of them."""
    assert kappa in (0.5, 1.0, 2.0) and N * Nt <= 8192 and M * N * Nt >= 2
    g = torch.Generator().manual_seed(seed)
    z = _halves(g, -2, 2, M, N, A)
    y = _halves(g, -2, 2, M, Nt)
    taus = torch.randint(0, 17, (M, N), generator=g).double() / 16
    actions = torch.full((M,), 0 if acted == "lo" else A - 1, dtype=torch.int64)
    w = (2.0 ** torch.randint(-3, 3, (M,), generator=g).double()) if weights else None
    a0, a1 = int(actions[0]), int(actions[M - 1])
    if M == 1 and N == 1:                                    # one theta: plant through two targets (Nt >= 2)
        th = float(z[0, 0, a0])
        y[0, 0] = th
        y[0, Nt - 1] = th + kappa if th + kappa <= 2 else th - kappa
    else:
        z[0, 0, a0] = y[0, 0]
        yk = float(y[M - 1, Nt - 1])
        z[M - 1, N - 1, a1] = yk - kappa if yk - kappa >= -2 else yk + kappa
    return {"z": z, "taus": taus, "actions": actions, "targets": y, "weights": w, "kappa": kappa, "row_scale": 2.0 ** -(seed % 4),
            "margin": exact_sum_margin(N * Nt, 4.0, 2.0 ** -8)}


def dyadic_loss_dqn(seed, M, A, kappa, weights=True):
    """q, y multiples of 1/2 in [-2, 2]; row 0 has td == 0, row M - 1 |td| == kappa when M >= 2 (M == 1: |td| == kappa)."""
    g = torch.Generator().manual_seed(seed)
    q, y = _halves(g, -2, 2, M, A), _halves(g, -2, 2, M)
    actions = torch.randint(0, A, (M,), generator=g)
    actions[0], actions[M - 1] = 0, A - 1
    w = (2.0 ** torch.randint(-3, 3, (M,), generator=g).double()) if weights else None
    if M >= 2:
        q[0, 0] = y[0]
    yk = float(y[M - 1])
    q[M - 1, A - 1] = yk - kappa if yk - kappa >= -2 else yk + kappa
    return {"q": q, "actions": actions, "targets": y, "weights": w, "kappa": kappa, "row_scale": 2.0 ** -(seed % 4)}


def _tail(g, M):
    """returns: multiples of 1/2, nsteps 1..5, masks 0 / 1 with both values present when M >= 2."""
    ret, ns = _halves(g, -2, 2, M), torch.randint(1, 6, (M,), generator=g).double()
    mk = torch.randint(0, 2, (M,), generator=g).double()
    mk[0] = 1.0
    if M >= 3:
        mk[2] = 0.0
    return ret, ns, mk


def dyadic_target_dqn(seed, M, A):
    """Row 0: the maximum of q_select tied between the first and the last action; row 1: between the last two actions."""
    g = torch.Generator().manual_seed(seed)
    qt, qs = _halves(g, -2, 2, M, A), _halves(g, -2, 1.5, M, A)
    ret, ns, mk = _tail(g, M)
    ties = 0
    if A >= 2:
        qs[0, 0] = qs[0, A - 1] = 2.0
        qt[0, 0], qt[0, A - 1] = 1.0, -1.0
        ties = 1
        if M >= 2:
            qs[1, A - 2] = qs[1, A - 1] = 2.0
            qt[1, A - 2], qt[1, A - 1] = -1.5, 0.5
            ties = 2
    return {"qt": qt, "qs": qs, "returns": ret, "nsteps": ns, "masks": mk, "ties": ties}


def dyadic_target_iqn(seed, M, Nt, Ns, A):
    """z multiples of 1/2 in [-2, 2]: column sums over Ns <= 65 quantiles are multiples of 1/2 below 130.  Row 0: the largest
    quantile MEAN tied between the first and the last action (different columns, equal sums when Ns >= 2); row 1 between the
    last two."""
    g = torch.Generator().manual_seed(seed)
    zt, zs = _halves(g, -2, 2, M, Nt, A), _halves(g, -2, 1.0, M, Ns, A)
    ret, ns, mk = _tail(g, M)
    ties = 0
    if A >= 2:
        for row, (a, b) in enumerate([(0, A - 1), (A - 2, A - 1)][:min(M, 2)]):
            zs[row, :, a] = 1.5
            zs[row, :, b] = 1.5
            if Ns >= 2:                                      # same sum, other summands
                zs[row, 0, a], zs[row, 1, a] = 2.0, 1.0
                zs[row, Ns - 1, b], zs[row, Ns - 2, b] = (2.0, 1.0) if Ns > 2 else (1.0, 2.0)
            zt[row, :, a] = _halves(g, 0.5, 2, Nt)
            zt[row, :, b] = -zt[row, :, a]
            ties += 1
    return {"zt": zt, "zs": zs, "returns": ret, "nsteps": ns, "masks": mk, "ties": ties,
            "margin": exact_sum_margin(Ns, 2.0, 0.5)}


def dyadic_actor_head(seed, E, N, A, dueling):
    """adv, val multiples of 1/8 in [-4, 4], N and A powers of two: mean_a and mean_n are exact.  Every env has its maximum
    planted on two actions (A >= 2), the first of them must win."""
    assert N & (N - 1) == 0 and A & (A - 1) == 0
    g = torch.Generator().manual_seed(seed)
    adv = torch.randint(-32, 25, (E, N, A), generator=g).double() / 8          # <= 3
    val = torch.randint(-32, 33, (E, N), generator=g).double() / 8 if dueling else None
    first = torch.zeros(E, dtype=torch.int64)
    if A >= 2:
        for e in range(E):
            a, b = sorted(torch.randperm(A, generator=g)[:2].tolist())
            adv[e, :, a] = 3.5
            adv[e, :, b] = 3.5
            if N >= 2:
                adv[e, 0, a], adv[e, 1, a] = 4.0, 3.0
            first[e] = a
    return {"adv": adv, "val": val, "first": first, "margin": exact_sum_margin(N, 12.0, 1.0 / (8 * A))}


def dyadic_grads(seed, sizes, k=3, amp=7):
    """Integers in [-amp, amp] times 2^-k: squares are multiples of 2^-2k, their sum over all tensors stays exact in float32
    per lane and in float64 across lanes."""
    g = torch.Generator().manual_seed(seed)
    gs = [torch.randint(-amp, amp + 1, (n,), generator=g).double() * 2.0 ** -k for n in sizes]
    return gs, exact_sum_margin(sum(sizes), (amp * 2.0 ** -k) ** 2, 2.0 ** (-2 * k))


# ---- the cases of the bit-exact GPU tests (the CPU test proves the generators' claims on exactly these) ------------------------
def loss_iqn_wave_cases():
    """N x Nt over everything k_loss_iqn_wave takes; A, M, kappa, the acted action and the weights cycle through their values."""
    out, k = [], 0
    for N in (1, 2, 4, 8, 16, 32, 64):
        for Nt in (1, 5, 31, 32, 33, 63, 64):
            A, M = (1, 6, 18, 65)[k % 4], (1, 3, 5, 258)[(k // 4 + k) % 4]
            if M * N * Nt < 2:
                M = 3
            out.append(dict(seed=100 + k, M=M, N=N, Nt=Nt, A=A, kappa=(0.5, 1.0, 2.0)[k % 3], acted=("lo", "hi")[(k // 3) % 2],
                            weights=bool((k // 5) % 2)))
            k += 1
    return out


def loss_iqn_generic_cases():
    out = []
    for k, (N, Nt) in enumerate([(3, 7), (24, 32), (48, 64), (65, 8), (70, 5), (128, 64), (32, 65), (8, 100)]):
        out.append(dict(seed=200 + k, M=(1, 2, 3, 7)[k % 4], N=N, Nt=Nt, A=(6, 1, 18, 9)[(k // 2) % 4], kappa=(1.0, 0.5, 2.0)[k % 3],
                        acted=("hi", "lo")[k % 2], weights=bool((k // 2) % 2)))
        out.append(dict(seed=300 + k, M=(1, 2, 3, 7)[(k + 2) % 4], N=N, Nt=Nt, A=(6, 1, 18, 9)[(k // 2 + 1) % 4], kappa=(1.0, 0.5, 2.0)[(k + 1) % 3],
                        acted=("hi", "lo")[(k + 1) % 2], weights=not bool((k // 2) % 2)))
    return out


def loss_dqn_cases():
    return [dict(seed=400 + 16 * i + 4 * j + 2 * h + w, M=M, A=A, kappa=(0.5, 1.0, 2.0)[(i + j) % 3], mode=("huber", "mse")[h], weights=bool(w))
            for i, A in enumerate((1, 2, 18)) for j, M in enumerate((1, 255, 256, 257)) for h in (0, 1) for w in (0, 1)]


def target_iqn_cases():
    """Ns, Nt and A each take all their values, M cycles; Ns * A + A <= 4096 (the LDS strip)."""
    out, k = [], 0
    for Ns in (1, 8, 63, 64, 65):
        for j, Nt in enumerate((1, 32, 64, 65, 130)):
            for A in ((1, 6, 64, 65, 100)[(k + j) % 5], (1, 6, 64, 65, 100)[(k + j + 2) % 5]):
                if Ns * A + A <= 4096:
                    out.append(dict(seed=500 + len(out), M=(1, 3, 6)[len(out) % 3], Nt=Nt, Ns=Ns, A=A))
        k += 1
    return out


def target_dqn_cases():
    return [dict(seed=600 + 4 * i + j, M=M, A=A) for i, A in enumerate((1, 2, 18)) for j, M in enumerate((1, 256, 257))]


def actor_head_dyadic_cases():
    return [dict(seed=700 + 8 * i + 2 * j + d, E=(1, 3, 4, 5, 33)[(i + j + d) % 5], N=N, A=A, dueling=bool(d))
            for i, N in enumerate((1, 32, 64)) for j, A in enumerate((1, 8)) for d in (0, 1)]


# ---- the acting step's bookkeeping and byte movers (csrc/acting.hip, convert.hip) ---------------------------------------------
# NumPy: everything here is exact (bytes, integers, one float32 multiply or add per value), so the GPU tests compare whole
# buffers bit for bit.  A function takes the buffers as they are BEFORE the step and returns them as they must be after it:
# whatever it does not assign (guard rows, pitch gaps, NULL outputs) must come back unchanged.
STEP_ADVANCE = 2 ** 64 - 1                   # include/mirl.h MIRL_STEP_ADVANCE


def episode_track(rewards, dones, actions, A, ep_reward, ep_len, out_reward, out_len, action_counts):
    """PolicyTrainer._track_rewards (policy_trainer.py:93-136, no monitor env) and _format_action_hist's counts (:75-91) for
    one vector step of E envs: the RAW reward joins the env's running sum, kept in float32 one addition per step, the length
    grows by one; where `done`, (sum, length) is reported and both restart at 0, elsewhere (0.0, 0) is reported.  An action
    outside [0, A) is not counted; actions or action_counts None: no histogram.
    -> (ep_reward, ep_len, out_reward, out_len, action_counts); each buffer may be longer than E."""
    E = len(rewards)
    ep_reward, ep_len, out_reward, out_len = ep_reward.copy(), ep_len.copy(), out_reward.copy(), out_len.copy()
    for e in range(E):
        total = np.float32(ep_reward[e]) + np.float32(rewards[e])
        length = int(ep_len[e]) + 1
        if dones[e]:
            out_reward[e], out_len[e] = total, length
            total, length = np.float32(0.0), 0
        else:
            out_reward[e], out_len[e] = np.float32(0.0), 0
        ep_reward[e], ep_len[e] = total, length
    if action_counts is not None:
        action_counts = action_counts.copy()
        if actions is not None:
            for a in actions[:E]:
                if 0 <= int(a) < A:
                    action_counts[int(a)] += 1
    return ep_reward, ep_len, out_reward, out_len, action_counts


def actor_pre(rewards_raw, dones, H, h, c, xh, xh_pitch, c_in, state_pack, initials, rewards_out, dones_out, clip,
              actions=None, A=0, ep_reward=None, ep_len=None, out_reward=None, out_len=None, action_counts=None,
              rng_step=None, step=0):
    """Between env.step and the policy forward (acting/actor.py:124-131, modules/lstm.py:131-161, policy_trainer.py:93-136,
    :252-254).  Per env e with mask = 1 - done (float32): h_in = h * mask, c_in = c * mask (a reset keeps the sign of the
    zero); xh[e * xh_pitch + j] = h_in (the [features | h] tail; xh points at its first column), state_pack[e] = [h_in | c_in],
    initials = float(done), dones_out = uint8(done), rewards_out = np.sign(raw) when clip else raw; the episode statistics
    on the RAW reward when ep_reward is given; rng_step[0] = step, or + 1 (mod 2^64) when step == STEP_ADVANCE.
    Flat buffers in, a dict of the same buffers after the step out (None stays None)."""
    E = len(rewards_raw)
    done = np.array([1 if d else 0 for d in dones[:E]], dtype=np.uint8)
    out = {k: (None if v is None else v.copy()) for k, v in dict(
        xh=xh, c_in=c_in, state_pack=state_pack, initials=initials, rewards_out=rewards_out, dones_out=dones_out,
        ep_reward=ep_reward, ep_len=ep_len, out_reward=out_reward, out_len=out_len, action_counts=action_counts,
        rng_step=rng_step).items()}
    if H > 0:
        mask = (np.float32(1.0) - done.astype(np.float32))[:, None]
        h_in = h[:E * H].reshape(E, H) * mask
        cc = c[:E * H].reshape(E, H) * mask
        for e in range(E):
            out["xh"][e * xh_pitch:e * xh_pitch + H] = h_in[e]
        out["c_in"][:E * H] = cc.reshape(-1)
        out["state_pack"][:2 * E * H] = np.concatenate([h_in, cc], axis=1).reshape(-1)
    out["initials"][:E] = done.astype(np.float32)
    out["dones_out"][:E] = done
    raw = np.asarray(rewards_raw, dtype=np.float32)
    out["rewards_out"][:E] = np.sign(raw) if clip else raw
    if ep_reward is not None:
        (out["ep_reward"], out["ep_len"], out["out_reward"], out["out_len"], out["action_counts"]) = episode_track(
            raw, done, actions, A, ep_reward, ep_len, out_reward, out_len, action_counts)
    if rng_step is not None:
        out["rng_step"][0] = (int(rng_step[0]) + 1) % 2 ** 64 if step == STEP_ADVANCE else step
    return out


def stack_shift(inp, newest, dones):
    """The frame-stack wrapper under an auto-resetting vector env (env_wrappers/common.py:141-178): inp (E, P, ...) uint8,
    newest (E, ...), dones (E,) -> out[e] = [inp[e][1:], or zeros when done[e]; newest[e]]."""
    out = np.empty_like(inp)
    for e in range(inp.shape[0]):
        out[e, :-1] = 0 if dones[e] else inp[e, 1:]
        out[e, -1] = newest[e]
    return out


def synth_env_draws(seed, t, E, p_neg, p_nonpos, p_done, pool_n=1):
    """Step t of the synthetic env (acting/synthetic_env.py): one Philox block per env keyed (seed ^ 0xE17, t, e); u0, u1 =
    the top 24 bits of words 0 and 1 over 2^24; reward -1 where u0 < p_neg, else 0 where u0 < p_nonpos, else +1; done
    where u1 < p_done (the thresholds as float32, both comparisons strict); the observation is pool batch t % pool_n.
    -> (rewards float32 (E,), dones uint8 (E,), pool index, u0, u1)."""
    w = [philox_4x32(seed ^ 0xE17, t, e) for e in range(E)]
    u0 = np.array([(x[0] >> 8) / 16777216.0 for x in w], dtype=np.float32)
    u1 = np.array([(x[1] >> 8) / 16777216.0 for x in w], dtype=np.float32)
    p_neg, p_nonpos, p_done = np.float32(p_neg), np.float32(p_nonpos), np.float32(p_done)
    rewards = np.where(u0 < p_neg, -1.0, np.where(u0 < p_nonpos, 0.0, 1.0)).astype(np.float32)
    return rewards, (u1 < p_done).astype(np.uint8), t % pool_n, u0, u1


def frames_to_f32_nhwc(x, scale):
    """The CNN's input conversion (models/torch/modules/cnn.py:44-45) into channels-last: x (N, C, HW) uint8 ->
    (N, HW, C) float32 = float32(x) * float32(scale), one rounding per value."""
    return np.ascontiguousarray(x.transpose(0, 2, 1)).astype(np.float32) * np.float32(scale)
