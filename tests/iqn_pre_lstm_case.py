"""The inputs of tests/test_iqn_pre_lstm_ab_gpu.py and of the two input conditions in tests/test_oracle_golden.py: the tiny
CNN -> LSTM -> FC stack with the quantile layer before the LSTM, its seeded weights, hand-built learner batches in the layout
of the replay's gather, and the quantile fractions of every pass.  Everything is drawn by CPU torch.Generators, so the CPU
test (float64 alone) and the GPU test (which copies the tensors to the device) see the very same numbers.  Plain torch, no
import from rltime_amd/."""
import torch

FRAME, A, N, H, FC, D, F = (3, 16, 16), 3, 3, 32, 32, 64, 400
T, P, NSTEP, GAMMA = 6, 3, 2, 0.99
L, R = T + P, T + P + NSTEP                 # rows of `states`; rows of the gathered block (target_states = rows [NSTEP, R))
BATCHES = (5, 17)                           # one sequence tile with 11 empty rows; two tiles, the second holding one row
# (B, N) of the learner cases.  N = 3: odd, the shape the kernels' row maps cannot take with a shift — the quantile product
# then runs as relu(linear) + a broadcast multiply, because the product GEMM's epilogue (k_gemm3_nt_mul) takes powers of two
# only; N = 4 at the small batch is the case in which that kernel runs
CASES = ((5, 3), (17, 3), (5, 4))
STRIDES = [2, 1]
MODEL = {"type": "sequential", "args": {"layer_configs": [
    {"type": "cnn", "args": {"channels_last": True, "layers": [{"filters": 16, "kernel": 4, "stride": 2}, {"filters": 16, "kernel": 3, "stride": 1}]}},
    {"type": "lstm", "args": {"num_units": H}},
    {"type": "fc", "args": {"fc_size": FC}}]}}
# chosen on the CPU (tests/test_oracle_golden.py asserts it): at every (B, N) of CASES the float64 evaluation has no ReLU unit
# within float32 rounding of zero in the training pass and a smallest double-Q margin >= 1e-3
SEED = 79

SHAPES = {
    "model.layers.0.layers.0.weight": (16, 3, 4, 4), "model.layers.0.layers.0.bias": (16,),
    "model.layers.0.layers.1.weight": (16, 16, 3, 3), "model.layers.0.layers.1.bias": (16,),
    "model.layers.1.lstm_cell.weight_ih": (4 * H, F), "model.layers.1.lstm_cell.weight_hh": (4 * H, H),
    "model.layers.1.lstm_cell.bias_ih": (4 * H,), "model.layers.1.lstm_cell.bias_hh": (4 * H,),
    "model.layers.2.layers.0.0.weight": (FC, H), "model.layers.2.layers.0.0.bias": (FC,),
    "out_layer.weight": (A, FC), "out_layer.bias": (A,),
    "value_hidden_layer.weight": (FC, H), "value_hidden_layer.bias": (FC,),
    "value_layer.weight": (1, FC), "value_layer.bias": (1,),
    "quantile_layer.weight": (F, D), "quantile_layer.bias": (F,),
}


def weights(seed=SEED):
    """-> (online, target) float32 state dicts.  Weights ~ N(0, 2 / fan_in), biases ~ N(0, 0.1^2); the target net is the
    online net plus noise of 5 % of each parameter's mean magnitude (a different set of weights, as after some training)."""
    g = torch.Generator().manual_seed(1000 + seed)
    online = {}
    for k, shape in SHAPES.items():
        if len(shape) == 1:
            online[k] = torch.randn(shape, generator=g) * 0.1
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            online[k] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
    target = {k: v + torch.randn(v.shape, generator=g) * v.abs().mean() * 0.05 for k, v in online.items()}
    for sd in (online, target):
        sd["embedding_range"] = torch.arange(1, D + 1, dtype=torch.float32)
    return online, target


def batch(B, seed=SEED):
    """One gathered block of B sequences, CPU tensors: frames (R, B) + FRAME uint8, state (R, B, 2H) = hx | cx, initials
    (R, B); returns, nsteps, masks, actions, weights (L, B).  Resets in the burn-in rows, at row P and in the training rows
    of both views; importance weights != 1; some target masks at 0."""
    g = torch.Generator().manual_seed(2000 + 100 * seed + B)
    out = {"frames": torch.randint(0, 256, (R, B) + FRAME, generator=g, dtype=torch.uint8),
           "state": torch.randn(R, B, 2 * H, generator=g) * 0.5,
           "initials": (torch.rand(R, B, generator=g) < 0.2).float(),
           "returns": torch.randn(L, B, generator=g),
           "nsteps": torch.randint(1, NSTEP + 1, (L, B), generator=g).float(),
           "masks": (torch.rand(L, B, generator=g) > 0.2).float(),
           "actions": torch.randint(0, A, (L, B), generator=g),
           "weights": 0.3 + 0.7 * torch.rand(L, B, generator=g)}
    ini = out["initials"]
    ini[P, 0] = 1.0                                       # the state stored at row P of sequence 0 is zeroed ...
    ini[P + NSTEP, B - 1] = 1.0                           # ... and the target view's of the last sequence
    for view in (ini[:L], ini[NSTEP:]):
        assert view[1:P].any() and view[P].any() and not view[P].all() and view[P + 1:].any()
    assert (out["masks"][P:] == 0).any() and (out["masks"][P:] == 1).any()
    return out


def raw(b):
    """The block as oracle.network64.learner_eval reads it."""
    s, i = b["state"], b["initials"]
    return {"x": b["frames"][:L], "tx": b["frames"][NSTEP:], "hx": s[:L, :, :H], "cx": s[:L, :, H:], "thx": s[NSTEP:, :, :H],
            "tcx": s[NSTEP:, :, H:], "initials": i[:L], "tinitials": i[NSTEP:], "returns": b["returns"], "nsteps": b["nsteps"],
            "masks": b["masks"], "actions": b["actions"], "weights": b["weights"]}


def fractions(B, n=N, seed=SEED):
    """The quantile fractions of one learner step, per network in the order it draws them: the online net's prefix pass,
    double-Q selection pass and training pass; the target net's prefix pass and target pass."""
    go, gt = torch.Generator().manual_seed(3000 + 100 * seed + B + 7 * n), torch.Generator().manual_seed(4000 + 100 * seed + B + 7 * n)
    return {"online": [torch.rand(rows * B * n, generator=go) for rows in (P, T, T)],
            "target": [torch.rand(rows * B * n, generator=gt) for rows in (P, T)]}


class Replay:
    """A policy's `tau_source` that hands out prepared draws in order and refuses any other."""

    def __init__(self, draws):
        self.draws, self.at = list(draws), 0

    def __call__(self, count):
        assert self.at < len(self.draws), "more draws than the %d prepared" % len(self.draws)
        t = self.draws[self.at]
        assert t.shape == (count,), (self.at, tuple(t.shape), count)
        self.at += 1
        return t


def float64_eval(B, n=N, device="cpu", seed=SEED):
    """oracle.network64.learner_eval on this case -> (result, online Net64, target Net64)."""
    from oracle.network64 import Net64, learner_eval
    w_on, w_tg = weights(seed)
    online, target = (Net64(w, STRIDES, n, device, injection_layer=1) for w in (w_on, w_tg))
    fr = fractions(B, n, seed)
    ref = learner_eval(online, target, raw(batch(B, seed)), [fr["target"][1], fr["online"][1], fr["online"][2]], GAMMA, P,
                       kappa=1.0, double_q=True, burn_taus=(fr["online"][0], fr["target"][0]))
    return ref, online, target


# ---- acting at T = 1 -----------------------------------------------------------------------------------------------------
E = 5
RESET_ENV = 2


def acting(seed=SEED):
    """Two consecutive vector steps of E envs: frames (2, E) + FRAME uint8 and the fractions of each step (E * N,).  The
    first step starts every env (initials all 1); env RESET_ENV starts a new episode at the second."""
    g = torch.Generator().manual_seed(5000 + seed)
    return {"frames": torch.randint(0, 256, (2, E) + FRAME, generator=g, dtype=torch.uint8),
            "taus": [torch.rand(E * N, generator=g) for _ in range(2)],
            "initials": torch.stack([torch.ones(E), torch.eye(E)[RESET_ENV]])}


def acting64(device="cpu", seed=SEED):
    """Net64 on acting(): per step the action values (E, A) = mean over N of Z, and the merged state handed on (before
    the next step's reset).  The state entering a step is the previous step's, zeroed where the step's initials are set
    (lstm.py:131-161)."""
    from oracle.network64 import Net64
    net = Net64(weights(seed)[0], STRIDES, N, device, injection_layer=1)
    case = acting(seed)
    h = c = torch.zeros(E, H, dtype=torch.float64, device=device)
    steps = []
    with torch.no_grad():
        for t in range(2):
            ini = case["initials"][t].to(device).double()
            keep = (1.0 - ini).unsqueeze(-1)
            # the stored state is already zeroed by get_state; forward() zeroes it again through `initials`: idempotent
            z = net.predict(case["frames"][t:t + 1], h * keep, c * keep, ini.view(1, E), case["taus"][t], 1)
            h, c = net.last_state
            steps.append({"q": z.mean(1), "h": h, "c": c})
    return steps
