"""Oracle: the recurrent dueling-IQN network and one learner evaluation in float64
(TEST INFRASTRUCTURE ONLY — nothing under rltime_amd/ imports this).

Plain-torch float64 restatement, from a float32 state_dict, of

  * rltime/models/torch/modules/cnn.py:43-50       uint8 -> float * scale, conv + ReLU stack
  * rltime/models/torch/modules/lstm.py:60-116     LSTMCell time loop, state reset on `initials`,
                                                   stored state consumed from timestep 0 only
  * rltime/policies/torch/iqn.py:67-106            cos(pi i tau) embedding -> Linear + ReLU ->
                                                   product with the interleaved repeat of the features,
                                                   injected before the LAST model layer
  * rltime/models/torch/modules/fc.py:33-35        Linear + ReLU
  * rltime/policies/torch/dqn.py:50-112            advantage outputs; dueling value branch off the
                                                   INPUT of the last model layer; V + A - mean_a A
  * rltime/training/multi_step_trainer.py:90-131   burn-in: prefix forward, the state stored at row P
                                                   replaced by the fresh one (zeroed where initials[P])
  * rltime/training/torch/iqn.py:15-52,54-129 and torch_trainer.py:101-147 through oracle.qmath

It is the independent anchor of tests/test_network_ab_gpu.py: the HIP path (products on the bf16 matrix
pipe, persistent LSTM sweeps) and the library path are both measured against THIS evaluation of the same
weights on the same gathered batch.  PINNED: tests/golden/generate.py run_network64_pin runs the reference's own
SequentialModel + IQNPolicy (float32, CPU) and Net64 on the same seeded weights, frames, stored state, initials and
quantile fractions and asserts outputs within 1e-5 and gradients within 1e-4 (measured 1.4e-6); the reference's
outputs travel as tests/golden/network64_pin.npz and tests/test_oracle_golden.py repeats the check without it.

Net64(injection_layer=1) is the other layout of policies/torch/iqn.py: the quantile product on the conv features, the LSTM
over B * N rows ordered (t, b, n) in merge mode "inner" (modules/lstm.py:83-116: the state entering a step is the mean over
n of the previous step's per-sample h and c, masked by initials[t, b]), FC and dueling head on the LSTM's output rows; the
state stored at row P is the merged one.  It is the anchor of tests/test_iqn_pre_lstm_ab_gpu.py and is pinned the same way
(run_network64_pre_lstm_pin, tests/golden/network64_pre_lstm_pin.npz: the reference's float32 run, 1.1e-6).
"""
import math

import torch
import torch.nn.functional as F

from . import qmath


def _d(t):
    return t.detach().double()


def _conv64(x, w, b, stride):
    """Valid-padding conv2d as im2col + matmul (no library convolution involved: float64 convolutions are not
    something MIOpen offers, and the anchor should not share a kernel with either path under test)."""
    n, _, h, wd = x.shape
    f, _, k, _ = w.shape
    cols = F.unfold(x, k, stride=stride)                       # (n, c*k*k, positions)
    y = w.reshape(f, -1) @ cols + b.view(1, f, 1)
    return y.reshape(n, f, (h - k) // stride + 1, (wd - k) // stride + 1)


class Net64:
    """state_dict of rltime_amd.policies.iqn.IQNPolicy (same parameter names as the reference's
    policies/torch/iqn.py + models/torch/sequential.py) -> float64 leaves with requires_grad."""

    def __init__(self, state_dict, conv_strides, n_quantiles, device, injection_layer=-1):
        """injection_layer: -1 / 2 = the quantile layer before the LAST model layer (the head, as above);
        1 = before the LSTM (IQNPolicy(injection_layer=1): the LSTM runs B * N rows over B stored states)."""
        assert injection_layer in (-1, 1, 2), injection_layer
        self.p = {k: _d(v).to(device).requires_grad_(v.dtype.is_floating_point and "embedding_range" not in k)
                  for k, v in state_dict.items()}
        self.strides = list(conv_strides)
        self.N = n_quantiles
        self.dev = device
        self.pre_lstm = injection_layer == 1
        self.relu_near_zero = 0

    def params(self):
        return {k: v for k, v in self.p.items() if v.requires_grad}

    def features(self, frames_u8, scale=1.0 / 255.0):
        """cnn.py:43-50 on (rows, C, H, W) uint8 -> (rows, C'*H'*W') in the reference's (C, H, W) flatten."""
        x = frames_u8.to(self.dev).double() * scale
        i = 0
        while "model.layers.0.layers.%d.weight" % i in self.p:
            x = _conv64(x, self.p["model.layers.0.layers.%d.weight" % i],
                        self.p["model.layers.0.layers.%d.bias" % i], self.strides[i])
            if self.pre_lstm:
                self._near_zero(x)
            x = F.relu(x)
            i += 1
        return x.reshape(x.shape[0], -1)

    def _near_zero(self, *pre):
        """Counts, into self.relu_near_zero, the ReLU units whose pre-activation is within float32 rounding of zero
        (|pre| <= 4e-7 of the layer's largest): a float32 evaluation may take the other branch there."""
        with torch.no_grad():
            self.relu_near_zero += sum(int((t.abs() <= 4e-7 * t.abs().max()).sum()) for t in pre)

    def lstm(self, feats, h0, c0, initials, T):
        """lstm.py:60-116: feats (T*B, F) time-major, h0 / c0 (B, H) = the state stored with timestep 0,
        initials (T, B).  -> (out (T*B, H), (h_T, c_T))."""
        p = self.p
        w_ih, w_hh = p["model.layers.1.lstm_cell.weight_ih"], p["model.layers.1.lstm_cell.weight_hh"]
        b_ih, b_hh = p["model.layers.1.lstm_cell.bias_ih"], p["model.layers.1.lstm_cell.bias_hh"]
        B = feats.shape[0] // T
        x = feats.reshape(T, B, -1)
        keep = (1.0 - initials.to(self.dev).double()).reshape(T, B, 1)
        h, c = h0.to(self.dev).double(), c0.to(self.dev).double()
        out = []
        for t in range(T):
            h, c = h * keep[t], c * keep[t]                      # lstm.py:95-97
            g = x[t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh     # torch.nn.LSTMCell
            i, f, gg, o = g.chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            out.append(h)
        return torch.cat(out), (h, c)

    def head(self, x, taus):
        """iqn.py:67-106 + fc.py:33-35 + dqn.py:50-112: x (M, H), taus (M*N,) -> Z (M, N, A)."""
        p, N = self.p, self.N
        rng = p["embedding_range"].double()
        phi = torch.cos(taus.to(self.dev).double().unsqueeze(1) * rng.unsqueeze(0) * math.pi)   # iqn.py:78-81
        emb = F.relu(phi @ p["quantile_layer.weight"].t() + p["quantile_layer.bias"])
        inner = (x.unsqueeze(1) * emb.reshape(x.shape[0], N, -1)).reshape(x.shape[0] * N, -1)    # iqn.py:84,102
        pre_h = inner @ p["model.layers.2.layers.0.0.weight"].t() + p["model.layers.2.layers.0.0.bias"]
        h = F.relu(pre_h)
        adv = h @ p["out_layer.weight"].t() + p["out_layer.bias"]
        pre_v = inner @ p["value_hidden_layer.weight"].t() + p["value_hidden_layer.bias"]
        hv = F.relu(pre_v)                                                                       # dqn.py:50-66
        # ReLU units whose pre-activation is within float32 rounding of zero: a float32 evaluation may take the other
        # branch there, which switches that unit's whole gradient row (tests/test_network_ab_gpu.py conditions its
        # per-parameter gradient bar on this count)
        with torch.no_grad():
            self.relu_near_zero = sum(int((t.abs() <= 4e-7 * t.abs().max()).sum()) for t in (pre_h, pre_v))
        val = hv @ p["value_layer.weight"].t() + p["value_layer.bias"]
        z = val + adv - adv.mean(1, keepdim=True)                                                # dqn.py:74-87
        return z.reshape(x.shape[0], N, -1)

    # ---- the quantile layer BEFORE the LSTM (injection_layer = 1) ------------------------------------------------
    def quantile_product(self, x, taus):
        """iqn.py:67-106 on the conv features: x (M, F), taus (M*N,) -> (M*N, F), rows grouped (m, n): row m*N + j
        is x[m] * relu(linear(cos(pi i tau[m*N + j])))."""
        p, N = self.p, self.N
        M = x.shape[0]
        tau = taus.to(self.dev).double().reshape(M, N)
        i = p["embedding_range"].double()
        phi = torch.cos(math.pi * i.view(1, 1, -1) * tau.unsqueeze(-1))                       # (M, N, D)   iqn.py:92-94
        pre = phi @ p["quantile_layer.weight"].t() + p["quantile_layer.bias"]                  # (M, N, F)
        self._near_zero(pre)
        return (x.unsqueeze(1) * F.relu(pre)).reshape(M * N, -1)                               # iqn.py:84,100

    def lstm_multi(self, rows, h0, c0, initials, T):
        """lstm.py:83-116 in merge mode "inner": rows (T*B*N, F) ordered (t, b, n); h0 / c0 (B, H) = the state stored
        with timestep 0; initials (T, B) of the B sequences.  Before each step the state of sequence b is the mean over
        n of the previous step's per-sample h and c, zeroed where initials[t, b] is set, and handed to each of its N
        samples.  -> (out (T*B*N, H) in the same row order, the merged (h_T, c_T) (B, H))."""
        p, N = self.p, self.N
        w_ih, w_hh = p["model.layers.1.lstm_cell.weight_ih"], p["model.layers.1.lstm_cell.weight_hh"]
        b_ih, b_hh = p["model.layers.1.lstm_cell.bias_ih"], p["model.layers.1.lstm_cell.bias_hh"]
        B = rows.shape[0] // (T * N)
        assert rows.shape[0] == T * B * N and tuple(h0.shape) == tuple(c0.shape) == (B, w_hh.shape[1])
        x = rows.reshape(T, B, N, -1)
        keep = (1.0 - initials.to(self.dev).double()).reshape(T, B, 1)
        h, c = h0.to(self.dev).double(), c0.to(self.dev).double()
        out = []
        for t in range(T):
            hm, cm = h * keep[t], c * keep[t]                                                  # (B, H)   lstm.py:95-97
            g = x[t] @ w_ih.t() + b_ih + (hm @ w_hh.t() + b_hh).unsqueeze(1)                   # (B, N, 4H)
            i, f, gg, o = g.chunk(4, dim=-1)
            cs = torch.sigmoid(f) * cm.unsqueeze(1) + torch.sigmoid(i) * torch.tanh(gg)
            hs = torch.sigmoid(o) * torch.tanh(cs)
            out.append(hs.reshape(B * N, -1))
            h, c = hs.mean(1), cs.mean(1)                                                      # lstm.py:115-116
        return torch.cat(out), (h, c)

    def head_rows(self, x):
        """fc.py:33-35 + dqn.py:50-112 on the LSTM's output rows (M*N, H), grouped (m, n) -> Z (M, N, A)."""
        p, N = self.p, self.N
        pre_h = x @ p["model.layers.2.layers.0.0.weight"].t() + p["model.layers.2.layers.0.0.bias"]
        adv = F.relu(pre_h) @ p["out_layer.weight"].t() + p["out_layer.bias"]
        pre_v = x @ p["value_hidden_layer.weight"].t() + p["value_hidden_layer.bias"]          # dqn.py:50-66
        self._near_zero(pre_h, pre_v)
        val = F.relu(pre_v) @ p["value_layer.weight"].t() + p["value_layer.bias"]
        z = val + adv - adv.mean(1, keepdim=True)                                              # dqn.py:74-87
        return z.reshape(x.shape[0] // N, N, -1)

    def predict(self, frames, h0, c0, initials, taus, T):
        """frames (T, B, C, H, W) uint8 -> Z (T*B, N, A).  self.last_state: the LSTM's final (h, c) — with the quantile
        layer before the LSTM the MERGED state (lstm.py:120)."""
        self.relu_near_zero = 0                   # of THIS pass (pre-LSTM layout: conv stack and quantile layer included)
        feats = self.features(frames.reshape((-1,) + tuple(frames.shape[2:])))
        if self.pre_lstm:
            out, state = self.lstm_multi(self.quantile_product(feats, taus), h0, c0, initials, T)
            self.last_state = tuple(s.detach() for s in state)
            return self.head_rows(out)
        out, state = self.lstm(feats, h0, c0, initials, T)
        self.last_state = tuple(s.detach() for s in state)
        return self.head(out, taus)

    def burn_in_state(self, frames, h0, c0, initials, P, taus=None):
        """multi_step_trainer.py:90-131 (head-less: only the recurrent state is consumed): the state to store
        at row P = the LSTM state after the P prefix steps, zeroed where initials[P] is set (lstm.py:142-153).
        With the quantile layer before the LSTM the prefix pass draws fractions of its own (taus (P*B*N,)) and the
        state is the merged one."""
        with torch.no_grad():
            feats = self.features(frames[:P].reshape((-1,) + tuple(frames.shape[2:])))
            if self.pre_lstm:
                _, (h, c) = self.lstm_multi(self.quantile_product(feats, taus), h0, c0, initials[:P], P)
            else:
                _, (h, c) = self.lstm(feats, h0, c0, initials[:P], P)
            keep = (1.0 - initials[P].to(self.dev).double()).unsqueeze(-1)
            return h * keep, c * keep


def learner_eval(online, target, batch, taus, gamma, P, kappa=1.0, double_q=True, burn_taus=None):
    """One learner evaluation (multi_step_trainer.py:278-353 up to the gradients) in float64.

    batch: the (L, b, ...) time-major tensors of History._make_train_batch (history.py:203-286):
      x, tx (L, b, C, H, W) uint8 states / target_states frames; hx, cx, thx, tcx (L, b, H); initials,
      tinitials (L, b); returns, nsteps, masks, actions, weights (L, b).
    taus: [target pass, selection pass, training pass], each (T*b*N,), in the reference's draw order
      (training/torch/iqn.py:18,32,70).
    burn_taus: (online prefix pass, target prefix pass), each (P*b*N,): only with the quantile layer before the LSTM,
      where the prefix passes run it too.
    -> dict(targets (T*b, N'), bootstrap (the gamma^n v part of the targets), loss, report (T*b,),
            grads {name: tensor}, state_P / target_state_P (the (h, c) stored at row P), relu_near_zero,
            min_double_q_margin)."""
    L = batch["x"].shape[0]
    T = L - P
    bt = burn_taus if burn_taus is not None else (None, None)
    h, c = online.burn_in_state(batch["x"], batch["hx"][0], batch["cx"][0], batch["initials"], P, bt[0])
    th, tc = target.burn_in_state(batch["tx"], batch["thx"][0], batch["tcx"][0], batch["tinitials"], P, bt[1])

    def flat(t):
        t = t[P:]
        return t.reshape((t.shape[0] * t.shape[1],) + tuple(t.shape[2:])).to(online.dev).double()

    with torch.no_grad():
        z_t = target.predict(batch["tx"][P:], th, tc, batch["tinitials"][P:], taus[0], T)
        # the selection pass reads the SAME target_states tree, i.e. the state the TARGET net's burn-in stored at
        # row P (multi_step_trainer.py:117-125 writes it into target_states; iqn.py:32 then feeds that tree to the
        # online net)
        sel = online if double_q else target
        z_s = sel.predict(batch["tx"][P:], th, tc, batch["tinitials"][P:], taus[1], T)
        y = qmath.nstep_target(qmath.iqn_bootstrap(z_t, z_s), flat(batch["returns"]), flat(batch["masks"]),
                               flat(batch["nsteps"]), gamma, None)
        # the smallest double-Q margin: (best - second best) of the mean over N of the selection values (iqn.py:36-45)
        # over all target rows, as a fraction of the largest such mean — a float32 evaluation may pick the other action
        # of a row whose margin is within its rounding
        q_s = z_s.mean(1)
        top = q_s.topk(2, dim=1).values
        margin = float((top[:, 0] - top[:, 1]).min() / q_s.abs().max())
    z = online.predict(batch["x"][P:], h, c, batch["initials"][P:], taus[2], T)
    loss, report = qmath.iqn_loss(z, taus[2].to(online.dev).double(), flat(batch["actions"]).long(), y,
                                  flat(batch["weights"]), kappa, T, "mean", None)
    names = list(online.params())
    grads = torch.autograd.grad(loss, [online.p[k] for k in names])
    return {"targets": y, "loss": loss.detach(), "report": report, "grads": dict(zip(names, grads)),
            "relu_near_zero": online.relu_near_zero,       # of the training pass (the last head evaluated on `online`)
            "bootstrap": y - flat(batch["returns"]).unsqueeze(-1), "state_P": (h, c), "target_state_P": (th, tc),
            "min_double_q_margin": margin}
