"""GPU: the extra-feature columns of the LSTM's input projection without the concatenation (csrc/lstm_extras.hip).

Kernel level, through the C ABI: mirl_lstm_extras_add bit for bit against its NumPy restatement
(tests/lstm_extras_restate.py), mirl_lstm_extras_wgrad against float64 (exactly on integer operands), the refusals.
Model level: the LSTM layer, SequentialModel and an IQN / DQN learner step with `split_extras` against the concatenating
formulation (the reference's, rltime/models/torch/sequential.py:155-166) within the project's 1e-4 of the tensor's scale
(docs/parity.md), and what must not happen on the new path: no K = F + X product, no (rows, F + X) block."""
import copy
import ctypes as C
import random

import numpy as np
import pytest
import torch
import torch.utils._python_dispatch

from tests.lstm_extras_restate import extras_add, one_hot_extras, wgrad_bound, wgrad_f64

pytestmark = pytest.mark.gpu

ERR_ARG = -1
SENTINEL = 12345.5
F0 = 64                                     # feature columns in front of the extras in the weight block: ldwx = F0 + X


def _p(t, offset_floats=0):
    return C.c_void_p(t.data_ptr() + 4 * offset_floats)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _misaligned(e_host, lde):
    """(M, X) host rows -> a device buffer holding them with row pitch `lde` from float offset 1 (the pointer is not
    16-byte aligned), the rest NaN: reading outside the X columns of a row shows."""
    M, X = e_host.shape
    buf = np.full(M * lde + 1, np.nan, np.float32)
    view = buf[1:].reshape(M, lde)
    view[:, :X] = e_host
    dev = torch.from_numpy(buf).cuda()
    assert (dev.data_ptr() + 4) % 16 != 0
    return dev


# ---- mirl_lstm_extras_add ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", [1, 5, 20, 32])
@pytest.mark.parametrize("N", [4, 260, 2048])
@pytest.mark.parametrize("M", [1, 67, 300])
def test_add_equals_the_restatement_bit_for_bit(M, N, X):
    """Out of place and in place, one-hot and dense extras: src is a window of a wider block (ldsrc > N), e has lde > X and
    a pointer that is not 16-byte aligned, wx is the strided view W[:, F0:] (ldwx = F0 + X).  Out of place src stays as
    it was and every element of the wider dst block outside the M x N window keeps its sentinel."""
    from rltime_amd._lib import check, lib
    rng = np.random.default_rng(M * 100003 + N * 101 + X)
    lds, ldd, lde = N + 8, N + 12, X + 3
    w_host = rng.standard_normal((N, F0 + X)).astype(np.float32)
    w_dev = torch.from_numpy(w_host).cuda()
    for dense in (False, True):
        e_host = rng.standard_normal((M, X)).astype(np.float32) if dense else one_hot_extras(rng, M, X)
        src_block = (rng.standard_normal((M + 2, lds)) * 2).astype(np.float32)
        want = extras_add(src_block[1:M + 1, 4:4 + N], e_host, w_host[:, F0:])
        e_dev = _misaligned(e_host, lde)
        src_dev = torch.from_numpy(src_block).cuda()
        dst_dev = torch.full((M + 2, ldd), SENTINEL, dtype=torch.float32, device="cuda")
        check(lib.mirl_lstm_extras_add(M, N, X, _p(src_dev, lds + 4), lds, _p(e_dev, 1), lde, _p(w_dev, F0), F0 + X,
                                       _p(dst_dev, ldd + 8), ldd, _st()), "mirl_lstm_extras_add")
        torch.cuda.synchronize()
        got = dst_dev.cpu().numpy()
        assert np.array_equal(_bits(got[1:M + 1, 8:8 + N]), _bits(want)), ("out of place", dense)
        outside = got.copy()
        outside[1:M + 1, 8:8 + N] = SENTINEL
        assert np.all(outside == SENTINEL), ("written outside the window", dense)
        assert np.array_equal(_bits(src_dev.cpu().numpy()), _bits(src_block)), ("src changed", dense)
        # in place on the window of the wider block
        check(lib.mirl_lstm_extras_add(M, N, X, _p(src_dev, lds + 4), lds, _p(e_dev, 1), lde, _p(w_dev, F0), F0 + X,
                                       _p(src_dev, lds + 4), lds, _st()), "mirl_lstm_extras_add")
        torch.cuda.synchronize()
        got = src_dev.cpu().numpy()
        assert np.array_equal(_bits(got[1:M + 1, 4:4 + N]), _bits(want)), ("in place", dense)
        rest_got, rest_want = got.copy(), src_block.copy()
        rest_got[1:M + 1, 4:4 + N] = 0
        rest_want[1:M + 1, 4:4 + N] = 0
        assert np.array_equal(_bits(rest_got), _bits(rest_want)), ("in place: written outside the window", dense)


# ---- mirl_lstm_extras_wgrad ----------------------------------------------------------------------------------------------------
def _wgrad(M, N, X, g_dev, ldg, e_dev, lde, short=0):
    from rltime_amd._lib import lib
    need = C.c_int64()
    assert lib.mirl_lstm_extras_wgrad_workspace_bytes(M, N, X, C.byref(need)) == 0
    ws = torch.empty(max(need.value, 1), dtype=torch.uint8, device="cuda")
    out = torch.full((N * X + 16,), SENTINEL, dtype=torch.float32, device="cuda")
    rc = lib.mirl_lstm_extras_wgrad(M, N, X, _p(g_dev), ldg, _p(e_dev, 1), lde, _p(out), _p(ws), need.value - short, _st())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), need.value


@pytest.mark.parametrize("X", [1, 5, 32])
@pytest.mark.parametrize("N", [4, 260])
@pytest.mark.parametrize("M", [1, 257, 300, 4099])
def test_wgrad_equals_float64(M, N, X):
    """dwx = g^T e from one read of g.  Integer operands in [-8, 8]: every partial sum is an integer of magnitude at
    most 4099 x 64 < 2^24, exact in float32 in any order — equality with float64 is exact, so a
    misindexed row, column or chunk cannot pass.  Random operands: within (M + 2) 2^-24 sum |g e|.  M = 257 is one chunk
    of 256 rows and a chunk of one row; two calls give the same bits; a workspace one byte short is refused."""
    rng = np.random.default_rng(M * 1009 + N * 31 + X)
    ldg, lde = N + 4, X + 2
    for integer in (True, False):
        if integer:
            g_host = rng.integers(-8, 9, size=(M, N)).astype(np.float32)
            e_host = rng.integers(-8, 9, size=(M, X)).astype(np.float32)
        else:
            g_host = rng.standard_normal((M, N)).astype(np.float32)
            e_host = rng.standard_normal((M, X)).astype(np.float32)
        g_block = np.full((M, ldg), np.nan, np.float32)
        g_block[:, :N] = g_host
        g_dev, e_dev = torch.from_numpy(g_block).cuda(), _misaligned(e_host, lde)
        rc, got, need = _wgrad(M, N, X, g_dev, ldg, e_dev, lde)
        assert rc == 0
        assert need == (0 if M <= 256 else -(-M // 256) * N * X * 4)
        assert np.all(got[N * X:] == SENTINEL)
        got = got[:N * X].reshape(N, X)
        want = wgrad_f64(g_host, e_host)
        err = np.abs(got.astype(np.float64) - want)
        if integer:
            assert np.array_equal(got.astype(np.float64), want), float(err.max())
        else:
            bound = wgrad_bound(g_host, e_host)
            print("M=%d N=%d X=%d max err / bound = %.4f" % (M, N, X, float(np.max(err / bound))))
            assert np.all(err <= bound)
        rc2, again, _ = _wgrad(M, N, X, g_dev, ldg, e_dev, lde)
        assert rc2 == 0 and np.array_equal(_bits(again[:N * X].reshape(N, X)), _bits(got))
        if need:
            rc3, untouched, _ = _wgrad(M, N, X, g_dev, ldg, e_dev, lde, short=1)
            assert rc3 == ERR_ARG and np.all(untouched == SENTINEL)


def test_launchers_refuse_bad_shapes_and_null_operands():
    from rltime_amd._lib import lib
    M, N, X = 8, 8, 5
    a = torch.zeros((M, N), dtype=torch.float32, device="cuda")
    e = torch.zeros((M, X), dtype=torch.float32, device="cuda")
    w = torch.zeros((N, X), dtype=torch.float32, device="cuda")
    d = torch.full((M, N), SENTINEL, dtype=torch.float32, device="cuda")
    add = lambda m, n, x, s, ev, wv, o, lds=N, ldd=N: lib.mirl_lstm_extras_add(      # noqa: E731
        m, n, x, s, lds, ev, max(x, 1), wv, max(x, 1), o, ldd, _st())
    assert add(M, N, X, _p(a), _p(e), _p(w), _p(d)) == 0
    for m, n, x in [(M, N, 0), (M, N, 33), (M, 6, X), (0, N, X)]:
        assert add(m, n, x, _p(a), _p(e), _p(w), _p(d)) == ERR_ARG, (m, n, x)
    for k in range(4):
        ops = [_p(a), _p(e), _p(w), _p(d)]
        ops[k] = None
        assert add(M, N, X, *ops) == ERR_ARG, k
    assert add(M, N, X, _p(a, 1), _p(e), _p(w), _p(d)) == ERR_ARG                    # src not 16-byte aligned
    assert add(M, 4, X, _p(a), _p(e), _p(w), _p(d), lds=6) == ERR_ARG                # leading dimension not a multiple of 4
    assert add(M, N, X, _p(a), _p(e), _p(w), _p(d), ldd=4) == ERR_ARG                # leading dimension below N
    out = torch.zeros((N, X), dtype=torch.float32, device="cuda")
    wg = lambda m, n, x, g, ev, o: lib.mirl_lstm_extras_wgrad(m, n, x, g, n, ev, max(x, 1), o, None, 0, _st())      # noqa: E731
    assert wg(M, N, X, _p(a), _p(e), _p(out)) == 0
    for m, n, x in [(M, N, 0), (M, N, 33), (M, 6, X), (0, N, X)]:
        assert wg(m, n, x, _p(a), _p(e), _p(out)) == ERR_ARG, (m, n, x)
    for k in range(3):
        ops = [_p(a), _p(e), _p(out)]
        ops[k] = None
        assert wg(M, N, X, *ops) == ERR_ARG, k
    assert wg(300, N, X, _p(a), _p(e), _p(out)) == ERR_ARG                           # two chunks and no workspace
    torch.cuda.synchronize()


# ---- the LSTM layer --------------------------------------------------------------------------------------------------------------
def _close(got, want, what):
    """The project's bar for a fused network op (docs/parity.md): 1e-4 of the tensor's scale."""
    got, want = got.detach().double(), want.detach().double()
    assert got.shape == want.shape, what
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print("%s: max err %.3e, scale %.3e" % (what, err, scale))
    assert err <= 1e-4 * max(scale, 1e-30), (what, err, scale)


def _lstm_case(nhwc):
    from rltime_amd.models.torch.modules import LSTM
    T, B, H, X = 4, 3, 32, 5
    torch.manual_seed(7)
    layer = LSTM((F0 + X,), H).cuda()
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(T * B, 4, 4, 4, device="cuda", generator=g)
    x = x.contiguous(memory_format=torch.channels_last) if nhwc else x.reshape(T * B, F0)
    extra = torch.from_numpy(one_hot_extras(np.random.default_rng(5), T * B, X)).cuda()
    hx = torch.randn(T * B, H, device="cuda", generator=g) * 0.5
    cx = torch.randn(T * B, H, device="cuda", generator=g)
    initials = torch.zeros(T * B, device="cuda")
    initials[2 * B + 1] = 1.0                     # a reset in the middle of sequence 1
    initials[0] = 1.0
    d_out = torch.randn(T * B, H, device="cuda", generator=g)
    return layer, x, extra, hx, cx, initials, d_out, T


def _lstm_pass(layer, x, extra, hx, cx, initials, d_out, T, split, via_projection=False):
    layer.split_extras = split
    layer.zero_grad(set_to_none=True)
    x = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    if via_projection:
        proj = layer.project_input(x)
        assert proj.shape == (x.shape[0], 4 * layer.num_units)
        before = proj.detach().clone()
        out = layer(x, hx, cx, initials, T, projected=proj, extra=extra)
    else:
        out = layer(x, hx, cx, initials, T, extra=extra)
    (out * d_out).sum().backward()
    if via_projection:
        assert torch.equal(proj.detach(), before)                   # the shared projection is left as it was, to the bit
    cell = layer.lstm_cell
    assert cell.weight_ih.grad.shape == (4 * layer.num_units, F0 + extra.shape[1])
    res = {"out": out.detach(), "h": layer.last_state[0], "c": layer.last_state[1], "d_x": x.grad.reshape(x.shape[0], -1),
           "d_w_features": cell.weight_ih.grad[:, :F0].clone(), "d_w_extras": cell.weight_ih.grad[:, F0:].clone(),
           "d_whh": cell.weight_hh.grad.clone(), "d_bih": cell.bias_ih.grad.clone(), "d_bhh": cell.bias_hh.grad.clone()}
    return res


@pytest.mark.parametrize("lowered", [False, True])
@pytest.mark.parametrize("nhwc", [True, False])
def test_lstm_layer_with_split_extras_equals_the_concatenation(nhwc, lowered, monkeypatch):
    """F = 64 features (a channels-last (T B, 4, 4, 4) activation, or flat rows), H = 32, X = 5, T = 4, B = 3, a reset in the
    middle, the stored state taken from timestep 0: output, last state and every gradient of the split path against the
    concatenating path, directly and through project_input + forward(projected=, extra=).  `lowered`: the split-bf16
    kernel's work thresholds at 0, so that the K = F product really runs on it."""
    from rltime_amd.models.torch import gemm3
    calls = []
    if lowered:
        monkeypatch.setattr(gemm3, "_MIN_WORK", 0)
        real = gemm3.gemm
        monkeypatch.setattr(gemm3, "gemm", lambda layout, a, b, *r, **k: (calls.append((layout, tuple(a.shape), tuple(b.shape))), real(layout, a, b, *r, **k))[1])
    case = _lstm_case(nhwc)
    layer, x, extra = case[0], case[1], case[2]
    assert layer.split_extras is True and layer.takes_extra(x, extra)
    want = _lstm_pass(*case, split=False)
    concat_calls, calls[:] = list(calls), []
    assert not layer.takes_extra(x, extra)
    for via in (False, True):
        got = _lstm_pass(*case, split=True, via_projection=via)
        for k in want:
            _close(got[k], want[k], "%s (projection %s)" % (k, via))
        if lowered:
            nt = [c for c in calls if c[0] == gemm3.NT]
            assert nt and all(c[2][1] == F0 for c in nt), calls               # the K = F product ran on the split-bf16 kernel
        calls[:] = []
    if lowered:
        assert not any(c[0] == gemm3.NT for c in concat_calls)               # K = F + X = 69 is not a multiple of 16


@pytest.mark.parametrize("nhwc", [True, False])
def test_project_input_with_extras_equals_the_concatenated_projection(nhwc):
    """project_input(x, extra): the whole input projection, extras included, against F.linear on the concatenated rows —
    values and the gradients of the features and of both column blocks of weight_ih."""
    layer, x, extra, _, _, _, _, _ = _lstm_case(nhwc)
    cell = layer.lstm_cell
    d = torch.randn(x.shape[0], 4 * layer.num_units, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    res = []
    for split in (True, False):
        layer.zero_grad(set_to_none=True)
        xi = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
        if split:
            proj = layer.project_input(xi, extra)
        else:
            proj = torch.nn.functional.linear(torch.cat([xi.reshape(xi.shape[0], -1), extra], -1), cell.weight_ih, cell.bias_ih + cell.bias_hh)
        (proj * d).sum().backward()
        res.append({"proj": proj.detach(), "d_x": xi.grad.reshape(xi.shape[0], -1), "d_w_features": cell.weight_ih.grad[:, :F0].clone(),
                    "d_w_extras": cell.weight_ih.grad[:, F0:].clone(), "d_bias": cell.bias_ih.grad.clone()})
    for k in res[1]:
        _close(res[0][k], res[1][k], k)


def test_lstm_layer_concatenates_where_the_split_does_not_apply():
    """X > 32 and CPU tensors take the concatenation: the same values as handing the layer the concatenated rows."""
    from rltime_amd.models.torch.modules import LSTM
    T, B, H, X = 2, 3, 8, 33
    torch.manual_seed(1)
    layer = LSTM((16 + X,), H).cuda()
    x, extra = torch.randn(T * B, 16, device="cuda"), torch.randn(T * B, X, device="cuda")
    hx, cx, ini = torch.zeros(T * B, H, device="cuda"), torch.zeros(T * B, H, device="cuda"), torch.zeros(T * B, device="cuda")
    assert not layer.takes_extra(x, extra)
    with torch.no_grad():
        a = layer(x, hx, cx, ini, T, extra=extra)
        b = layer(torch.cat([x, extra], -1), hx, cx, ini, T)
    assert torch.equal(a, b)
    cpu = copy.deepcopy(layer).cpu()
    assert not cpu.takes_extra(x.cpu(), extra.cpu()[:, :5])


# ---- SequentialModel ---------------------------------------------------------------------------------------------------------------
NATURE = {"type": "cnn", "args": {"channels_last": True, "layers": [
    {"filters": 32, "kernel": 8, "stride": 4}, {"filters": 64, "kernel": 4, "stride": 2}, {"filters": 64, "kernel": 3, "stride": 1}]}}
LAYERS = [NATURE, {"type": "lstm", "args": {"num_units": 64}}, {"type": "fc", "args": {"fc_size": 32}}]
LAYERS_FF = [NATURE, {"type": "fc", "args": {"fc_size": 32}}]


class _Shapes(torch.utils._python_dispatch.TorchDispatchMode):
    """Records the shape of every tensor an operator produces."""

    def __init__(self):
        super().__init__()
        self.seen = set()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        for t in (out if isinstance(out, (tuple, list)) else (out,)):
            if isinstance(t, torch.Tensor):
                self.seen.add(tuple(t.shape))
        return out


def _model_and_input(layers, X=8, T=4, B=3, seed=0):
    from rltime_amd.models.torch.sequential import SequentialModel
    from rltime_amd.spaces import Box, Tuple
    torch.manual_seed(seed)
    space = Tuple((Box(0, 255, (4, 84, 84), np.uint8), Box(-np.inf, np.inf, (X,), np.float32)))
    model = SequentialModel(space, layers).cuda()
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    frames = torch.randint(0, 256, (T * B, 4, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
    extra = torch.from_numpy(one_hot_extras(np.random.default_rng(seed), T * B, X)).cuda()
    inp = {"x": (frames, extra)}
    for i, layer in enumerate(model.layers):
        inp["layer%d_state" % i] = {}
        if layer.is_recurrent():
            H = layer.num_units
            ini = torch.zeros(T * B, device="cuda")
            ini[B + 1] = 1.0
            inp["layer%d_state" % i] = {"hx": torch.randn(T * B, H, device="cuda", generator=g) * 0.3,
                                        "cx": torch.randn(T * B, H, device="cuda", generator=g) * 0.3, "initials": ini}
    return model, inp, T


def test_sequential_model_hands_the_extras_to_the_lstm_without_the_concatenation(monkeypatch):
    """CNN -> LSTM -> FC on (frames, extras): with the split-bf16 kernel's thresholds at 0 the LSTM's input projection is an
    NT product with K = F = 3136 and none with K = F + X; no operator produces a (T B, F + X) tensor, with or without
    grad; output and weight gradients follow the concatenating model within 1e-4 of scale."""
    from rltime_amd.models.torch import gemm3
    model, inp, T = _model_and_input(LAYERS)
    F, X, rows = 3136, 8, inp["x"][0].shape[0]
    assert model.extra_input_layer == 1 and model.layers[1].inp_size == F + X
    monkeypatch.setattr(gemm3, "_MIN_WORK", 0)
    nt = []
    real = gemm3.gemm
    monkeypatch.setattr(gemm3, "gemm", lambda layout, a, b, *r, **k: (nt.append(a.shape[1]) if layout == gemm3.NT else None, real(layout, a, b, *r, **k))[1])
    res = {}
    for split in (True, False):
        model.layers[1].split_extras = split
        model.zero_grad(set_to_none=True)
        nt.clear()
        with _Shapes() as shapes:
            with torch.no_grad():
                quiet = model(inp, T)["output"]
            out = model(inp, T)
            out["output"].square().sum().backward()
        _close(quiet, out["output"], "no-grad pass against the grad pass (split %s)" % split)
        if split:
            assert F in nt and F + X not in nt, nt
            assert (rows, F + X) not in shapes.seen
            assert len(out["layer_inputs"]) == 3 and out["layer_inputs"][-1].shape == (rows, 64)
        else:
            assert (rows, F + X) in shapes.seen and F not in nt
        res[split] = (out["output"].detach().clone(), [p.grad.clone() for p in model.parameters()])
    _close(res[True][0], res[False][0], "output")
    for (name, _), a, b in zip(model.named_parameters(), res[True][1], res[False][1]):
        _close(a, b, name)


def test_sequential_model_still_concatenates_elsewhere():
    """Extras at the last FC layer, and a pre-processor on the LSTM layer: the model concatenates as before — outputs equal,
    to the bit, to torch.cat + the layer written out."""
    model, inp, T = _model_and_input(LAYERS_FF, seed=2)
    assert model.extra_input_layer == 1
    with torch.no_grad():
        got = model(inp, 1)
        feats = model.layers[0](inp["x"][0])
        rows = torch.cat([feats.reshape(feats.shape[0], -1), inp["x"][1]], dim=-1)
        want = model.layers[1](rows, timesteps=1)
    assert torch.equal(got["output"], want) and torch.equal(got["layer_inputs"][1], rows)

    model, inp, T = _model_and_input(LAYERS, seed=3)
    seen = []

    def pre(x):
        seen.append(tuple(x.shape))
        return x * 0.5, {"pre": True}
    model.set_layer_preprocessor(1, pre)
    with torch.no_grad():
        got = model(inp, T)
        feats = model.layers[0](inp["x"][0])
        rows = torch.cat([feats.reshape(feats.shape[0], -1), inp["x"][1]], dim=-1)
        mid = model.layers[1](rows * 0.5, timesteps=T, **inp["layer1_state"])
        want = model.layers[2](mid, timesteps=T)
    assert seen == [(rows.shape[0], 3136 + 8)] and got["pre"] is True
    assert torch.equal(got["output"], want)


# ---- the learner step --------------------------------------------------------------------------------------------------------------
def _learner(kind, graphed, split, steps):
    """A trainer on the synthetic env with the extra-features wrapper, built from fixed seeds; the first batch it would
    train on is taken aside and `steps` learner steps run on that same batch.  -> per-step records."""
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.general.type_registry import get_registered_type
    from rltime_amd.train import create_actors
    cfg = {"acting": {"actor_envs": 8, "exploration": {"type": "epsilon_greedy", "args": {
               "eps_start": 1.0, "eps_final": 1.0, "exploration_fraction": 0.5}}},
           "env": "synthetic-atari", "env_args": {"frame_shape": [4, 84, 84], "n_actions": 6, "done_prob": 0.05, "extra_features": True},
           "model": {"type": "sequential", "args": {"layer_configs": LAYERS}}}
    cfg["policy_args"] = {"dueling": True, "embedding_dim": 16, "num_sampling_quantiles": 8} if kind == "iqn" else {"dueling": True}
    targs = {"clip_rewards": False, "gamma": 0.99, "mbatch_size": 4, "nstep_train": 6, "burn_in_timesteps": 2, "nstep_target": 2,
             "lr": 1e-3, "double_q": True, "rnn_bootstrap": True, "clip_grad": 10.0, "target_update_freq": 10 ** 6,
             "total_steps": 10 ** 9, "log_freq": 10 ** 9, "warmup_steps": 0, "graph_learner_step": graphed,
             "history_mode": {"type": "prioritized_replay", "args": {
                 "size": 400, "train_frequency": 4, "alpha": 0.9, "beta": 0.6, "device_rng": True}}}
    random.seed(1); np.random.seed(2); torch.manual_seed(3)           # noqa: E702
    actors = create_actors(copy.deepcopy(cfg), torch.device("cuda", 0), device_acting=True)
    tr = get_registered_type("trainers", kind)(logger=NullLogger(), actors=actors, model_config=cfg["model"],
                                               policy_args=cfg["policy_args"])
    tr.data_parallel = None
    tr.setup(**copy.deepcopy(targs))
    for pol in (tr.policy, tr.target_policy):
        assert pol.model.extra_input_layer == 1
        pol.model.layers[1].split_extras = split
    if not split:
        tr.share_online_projection = False
    held = []
    real_step = tr.learner_step
    tr.learner_step = lambda *a, **k: held.append((a, k))
    while not held:
        tr.loop_iteration()
    tr.learner_step = real_step
    rec = {"qloss": [], "priorities": [], "grads": [], "projected": [], "params": None}
    log = tr.value_log.log

    def tap(key, value, *a, **k):
        if key == "qloss" and k.get("group") == "train":
            rec["qloss"].append(value.detach().float().reshape(()).clone() if isinstance(value, torch.Tensor) else torch.tensor(float(value)))
        return log(key, value, *a, **k)
    tr.value_log.log = tap
    upd = tr.history_buffer.update_losses

    def update(idx, losses, *a, **k):
        rec["priorities"].append(losses.detach().float().reshape(-1).clone())
        return upd(idx, losses, *a, **k)
    tr.history_buffer.update_losses = update
    share = tr._share_online_features

    def shared(train_data, nstep_target):
        share(train_data, nstep_target)
        rec["projected"].append("x_projected" in train_data["states"] and "x_projected" in train_data["target_states"])
    tr._share_online_features = shared
    (args, kwargs) = held[0]
    for _ in range(steps):
        tr.learner_step(*args, **kwargs)
        rec["grads"].append([p.grad.detach().clone() for p in tr.policy.parameters()])
    torch.cuda.synchronize()
    rec["params"] = [p.detach().clone() for p in tr.policy.parameters()]
    rec["names"] = [n for n, _ in tr.policy.named_parameters()]
    rec["captured"] = tr._gstep is not None and tr._gstep["graph"] is not None
    x = args[0]["states"]["x"]
    rec["extras"] = isinstance(x, (tuple, list)) and x[1].shape[-1] == 8
    tr.history_buffer.close()
    actors.close()
    return rec


@pytest.mark.parametrize("kind", ["iqn", "dqn"])
def test_learner_step_with_split_extras(kind, monkeypatch):
    """A recurrent, prioritized, double-Q learner step with extras (T = 6, burn-in 2, n = 2, B = 4 sequences): the online
    net's projection is hoisted for extra_input_layer == 1; loss, the priorities written back and every parameter
    gradient follow the step with split_extras = False and share_online_projection = False within 1e-4 of scale; a
    second trainer from the same state gives the same bits; and with graph_learner_step the captured step (steps 4 and
    5, each after an optimizer update — the cached feature-weight copy is refreshed inside the graph) equals the eager
    step bit for bit.  (This library's own conv weight-gradient kernels at every size, as in tests/test_graph_step_gpu.py:
    the vendor library's add their K-splits with atomics and are not reproducible to the bit.)"""
    from rltime_amd.models.torch import fused
    monkeypatch.setattr(fused, "_CONV_WRW_MIN_WORK", 0)
    eager = _learner(kind, "no-capture", True, 5)
    graph = _learner(kind, True, True, 5)
    plain = _learner(kind, "no-capture", False, 1)
    assert eager["extras"] and graph["extras"] and plain["extras"]
    assert eager["projected"] and all(eager["projected"]) and all(graph["projected"])
    assert plain["projected"] == [False]
    assert graph["captured"] and not eager["captured"]
    assert len(eager["qloss"]) == len(graph["qloss"]) == 5 and len(eager["priorities"]) == 5
    # against the concatenating step
    _close(eager["qloss"][0], plain["qloss"][0], "qloss")
    _close(eager["priorities"][0], plain["priorities"][0], "priorities")
    assert float(eager["priorities"][0].abs().max()) > 0
    for name, a, b in zip(eager["names"], eager["grads"][0], plain["grads"][0]):
        _close(a, b, "grad " + name)
    # the same state, the same bits: eager steps of two trainers, then the captured steps against the eager ones
    for s in range(5):
        assert torch.equal(eager["qloss"][s], graph["qloss"][s]), s
        assert torch.equal(eager["priorities"][s], graph["priorities"][s]), s
        for name, a, b in zip(eager["names"], eager["grads"][s], graph["grads"][s]):
            assert torch.equal(a, b), (s, name)
    for name, a, b in zip(eager["names"], eager["params"], graph["params"]):
        assert torch.equal(a, b), name
    assert not torch.equal(eager["qloss"][0], eager["qloss"][4])              # the optimizer moved the weights in between
