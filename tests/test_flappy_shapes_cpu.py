"""CPU: the layer shapes of the two shipped Flappy configs (configs/flappy_iqn_lstm.json, configs/flappy_dqn.json) derived
from the configs themselves, and what every kernel family's `*_supported` query answers at them.  Both configs leave the Atari
geometry (84 x 84 -> 20 x 20 -> 9 x 9 -> 7 x 7) that the per-kernel tests were written at; tests/test_flappy_shapes_gpu.py
imports the shapes from here and holds the kernels to float64 at them.  A config or gate change that moves a layer onto or
off a kernel shows up here first.

The work thresholds above the gates (fused._CONV3_MIN_WORK, fused._CONV_WRW_MIN_WORK, gemm3._MIN_WORK) are restated as the
multiply-add counts the Python wrappers compare them with, at the shipped batches: 32 acting envs; 32 sequences x 22 rows
(nstep_train 20 + nstep_target 2) = 704 frames per learner pass, 32 x 20 = 640 in the passes over the loss rows alone; 64
frames per pass for the feed-forward DQN."""
import ctypes as C

from rltime_amd.general.config import load_config
from tests.extra_features_restate import feature_size


def conv_out(h, k, s):
    return (h - k) // s + 1


def derive(name):
    """-> dict(frame (P, H, W), convs [(C, H, W, F, k, s, OH, OW) per conv layer], features, lstm units or 0, A, X extras or 0,
    envs, mbatch, nstep_train, nstep_target)."""
    cfg = load_config(name)
    layers = cfg["model"]["args"]["layer_configs"]
    assert layers[0]["type"] == "cnn" and layers[0]["args"]["channels_last"] is True
    p, h, w = cfg["env_args"]["frame_shape"]
    convs, c = [], p
    for lay in layers[0]["args"]["layers"]:
        f, k, s = lay["filters"], lay["kernel"], lay["stride"]
        oh, ow = conv_out(h, k, s), conv_out(w, k, s)
        convs.append((c, h, w, f, k, s, oh, ow))
        c, h, w = f, oh, ow
    lstm = [lay["args"]["num_units"] for lay in layers if lay["type"] == "lstm"]
    a = cfg["env_args"]["n_actions"]
    t = cfg["training"]["args"]
    return dict(frame=tuple(cfg["env_args"]["frame_shape"]), convs=convs, features=c * h * w, lstm=lstm[0] if lstm else 0, A=a,
                X=feature_size(a) if cfg["env_args"].get("extra_features") else 0, envs=cfg["acting"]["actor_envs"],
                mbatch=t["mbatch_size"], nstep_train=t["nstep_train"], nstep_target=t["nstep_target"])


IQN = derive("flappy_iqn_lstm.json")
DQN = derive("flappy_dqn.json")

# what the GPU tests run, as (C, H, W, F, k, s)
IQN_FRAME, DQN_FRAME = IQN["frame"], DQN["frame"]                    # (1, 120, 80), (4, 48, 32)
IQN_CONV2, IQN_CONV3 = IQN["convs"][1][:6], IQN["convs"][2][:6]      # (32, 29, 19, 64, 4, 2), (64, 13, 8, 64, 3, 1)
DQN_CONV2 = DQN["convs"][1][:6]                                      # (32, 11, 7, 32, 3, 1)
IQN_CONV3_OUT = IQN["convs"][2][6:]                                  # (11, 6)
LSTM_H, LSTM_F, LSTM_X = IQN["lstm"], IQN["features"], IQN["X"]      # 512, 4224, 4
LSTM_XP = (LSTM_X + 15) // 16 * 16                                   # the extras padded to a 16-wide K step
LSTM_K = LSTM_F + LSTM_XP + LSTM_H                                   # 4752: the acting step's [features | extras | h] row
LEARNER_ROWS = (IQN["mbatch"] * (IQN["nstep_train"] + IQN["nstep_target"]), IQN["mbatch"] * IQN["nstep_train"])   # (704, 640)
PROJ_TN = [(4 * LSTM_H, LSTM_F, rows) for rows in LEARNER_ROWS]      # the projection's weight gradient, frames part: (M, N, K)
TN = 2


def _lib():
    from rltime_amd._lib import lib
    return lib


def test_shapes_follow_from_the_configs():
    assert IQN["frame"] == (1, 120, 80) and IQN["envs"] == 32 and IQN["A"] == 2 and IQN["X"] == 4
    assert IQN["convs"] == [(1, 120, 80, 32, 8, 4, 29, 19), (32, 29, 19, 64, 4, 2, 13, 8), (64, 13, 8, 64, 3, 1, 11, 6)]
    assert IQN["features"] == 64 * 11 * 6 == 4224 and IQN["lstm"] == 512
    assert DQN["frame"] == (4, 48, 32) and DQN["envs"] == 32 and DQN["lstm"] == 0 and DQN["X"] == 0
    assert DQN["convs"] == [(4, 48, 32, 32, 8, 4, 11, 7), (32, 11, 7, 32, 3, 1, 9, 5)]
    assert DQN["features"] == 32 * 9 * 5
    assert (IQN_CONV2, IQN_CONV3, DQN_CONV2) == ((32, 29, 19, 64, 4, 2), (64, 13, 8, 64, 3, 1), (32, 11, 7, 32, 3, 1))
    # the input layer's 29 x 19 positions are 34 sixteen-position tiles and 7 more
    assert 29 * 19 == 551 == 34 * 16 + 7
    # conv 2 of the recurrent config: the stride leaves the last input row and the last input column uncovered
    c, h, w, f, k, s = IQN_CONV2
    assert (h - k) % s == 1 and (w - k) % s == 1 and (conv_out(h, k, s) - 1) * s + k == h - 1 and (conv_out(w, k, s) - 1) * s + k == w - 1
    assert (LSTM_XP, LSTM_K) == (16, 4224 + 16 + 512) and LSTM_K == 4752
    assert LEARNER_ROWS == (704, 640) and PROJ_TN == [(2048, 4224, 704), (2048, 4224, 640)]


def test_input_layer_gates():
    from rltime_amd.models.torch.fused import conv_u8_family
    lib = _lib()
    for d in (IQN, DQN):
        p, h, w, f, k, s = d["convs"][0][:6]
        assert conv_u8_family(p).supported(h, w, f, k, s), d["frame"]
    assert lib.mirl_conv1p_u8_supported(120, 80, 32, 8, 4) == 1 and lib.mirl_conv1_u8_supported(4, 48, 32, 32, 8, 4) == 1
    assert lib.mirl_conv1_u8_supported(1, 120, 80, 32, 8, 4) == 0          # one plane is the other family's


def test_middle_conv_gates():
    lib = _lib()
    fwd = lambda c, h, w, f, k, s: lib.mirl_conv3_fwd_supported(c, f, k, k, s, h, w)                   # noqa: E731
    wrw = lambda c, h, w, f, k, s: lib.mirl_conv_wrw_b3_supported(c, f, k, k, s, h, w)                 # noqa: E731
    dx2 = lambda c, h, w, f, k, s: lib.mirl_conv2_bwd_data_supported(c, f, k, s, h, w, conv_out(h, k, s), conv_out(w, k, s))   # noqa: E731
    dx3 = lambda c, h, w, f, k, s: lib.mirl_conv3_bwd_data_supported(c, f, k, s, h, w, conv_out(h, k, s), conv_out(w, k, s))   # noqa: E731
    # conv 2 of the recurrent config: HIP forward; one frame's fill is past the weight gradient's 150 KiB budget, and the data
    # gradient takes only inputs the stride covers (28 x 18 would be taken): both stay on the library
    assert fwd(*IQN_CONV2) == 1 and wrw(*IQN_CONV2) == 0 and dx2(*IQN_CONV2) == 0 and dx3(*IQN_CONV2) == 0
    assert lib.mirl_conv2_bwd_data_supported(32, 64, 4, 2, 28, 18, 13, 8) == 1
    # conv 3 of the recurrent config: all three on HIP
    assert fwd(*IQN_CONV3) == 1 and wrw(*IQN_CONV3) == 1 and dx3(*IQN_CONV3) == 1 and dx2(*IQN_CONV3) == 0
    # conv 2 of the DQN config, 32 filters: the forward alone
    assert fwd(*DQN_CONV2) == 1 and wrw(*DQN_CONV2) == 0 and dx3(*DQN_CONV2) == 0 and dx2(*DQN_CONV2) == 0


def test_acting_gates():
    from tests.test_actnet_exact_gpu import _lstm_slices
    lib = _lib()
    c, h, w, f, k, s = IQN_CONV2
    assert lib.mirl_act_conv_supported(2, c, f, k, s, h, w) == 1
    c, h, w, f, k, s = IQN_CONV3
    assert lib.mirl_act_conv_supported(3, c, f, k, s, h, w) == 1
    c, h, w, f, k, s = DQN_CONV2                                           # 32 filters: neither acting kernel
    assert lib.mirl_act_conv_supported(2, c, f, k, s, h, w) == 0 and lib.mirl_act_conv_supported(3, c, f, k, s, h, w) == 0
    # rows per launch against the 6144 above which the weights-in-LDS kernel runs: 32 envs below it in both layers, 256 above
    assert 32 * 13 * 8 == 3328 < 6144 and 32 * 11 * 6 == 2112 < 6144
    assert 256 * 13 * 8 == 26624 >= 6144 and 256 * 11 * 6 == 16896 >= 6144
    for envs in (4, 32):
        assert lib.mirl_act_lstm_supported(envs, LSTM_H, LSTM_K) == 1
    assert lib.mirl_act_lstm_supported(IQN["envs"], LSTM_H, LSTM_F + LSTM_X + LSTM_H) == 0     # unpadded extras: K % 16 = 4
    # 297 K steps in 4 slices of 75, the last holding 72
    assert LSTM_K // 16 == 297 and _lstm_slices(LSTM_H, LSTM_K) == (4, 75, 4) and 297 - 3 * 75 == 72


def test_projection_weight_gradient_gate_and_chunks():
    lib = _lib()
    for (m, n, k), per_chunk, last in zip(PROJ_TN, (6, 5), (2, 5)):
        assert lib.mirl_gemm3_supported(TN, m, n, k) == 1
        need = C.c_int64()
        assert lib.mirl_gemm3_workspace_bytes(TN, m, n, k, C.byref(need)) == 0
        chunks = need.value // (4 * m * n)                                 # one (M, N) partial per K chunk
        steps = k // 16
        assert chunks == 8 and -(-steps // chunks) == per_chunk and steps - (chunks - 1) * per_chunk == last, (m, n, k)


def test_what_the_work_thresholds_decide_at_the_shipped_batches():
    """The wrappers' multiply-add counts against their floors: which of the gated kernels the shipped configs actually run."""
    from rltime_amd.models.torch import fused, gemm3

    def conv_work(n, shape):
        c, h, w, f, k, s = shape
        return n * conv_out(h, k, s) * conv_out(w, k, s) * f * c * k * k

    assert (fused._CONV3_MIN_WORK, fused._CONV_WRW_MIN_WORK, gemm3._MIN_WORK) == (400000000, 1 << 31, 1 << 31)
    for rows in LEARNER_ROWS:
        assert conv_work(rows, IQN_CONV2) >= fused._CONV3_MIN_WORK         # k_conv3_fwd
        assert conv_work(rows, IQN_CONV3) >= fused._CONV3_MIN_WORK         # k_conv3_fwd
        # 704 frames: 1.71e9 multiply-adds, 640: 1.56e9, both under 2^31: layer 3's weight gradient stays on the library
        assert conv_work(rows, IQN_CONV3) < fused._CONV_WRW_MIN_WORK
        assert 4 * LSTM_H * LSTM_F * rows >= gemm3._MIN_WORK               # k_gemm3 TN
    assert conv_work(704, IQN_CONV3) == 1712848896 and conv_work(640, IQN_CONV3) == 1557135360
    # the frames at which layer 3's weight gradient would move onto k_conv_wrw_b3
    assert -(-fused._CONV_WRW_MIN_WORK // conv_work(1, IQN_CONV3)) == 883
    # the DQN config's conv 2: 64 frames per pass (128 with the target pass folded in) against the 965 the floor asks for
    assert DQN["mbatch"] * DQN["nstep_train"] == 64
    assert conv_work(128, DQN_CONV2) < fused._CONV3_MIN_WORK and -(-fused._CONV3_MIN_WORK // conv_work(1, DQN_CONV2)) == 965
