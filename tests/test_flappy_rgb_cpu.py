"""CPU: Flappy in colour as far as it can be held without a device — the restatement of the RGB rendering
(tests/flappy_rgb_restate.py) against frames built pixel by pixel from the definition, the `rgb` refusals by name on both
devices, and the shipped configs/flappy_iqn_lstm_rgb.json: flappy_iqn_lstm.json at the reference's observation shape
(ple_flappy_bird_iqn_lstm.json: one (3, 120, 80) frame per step), with only the first conv layer's input differing."""
import copy

import numpy as np
import pytest

from tests import flappy_restate as FR
from tests import flappy_rgb_restate as RGB

BG, PIPE, BIRD = (78, 192, 202), (84, 168, 40), (250, 200, 30)


def _by_hand(state, seed, H, W, s, g, D):
    """the definition, one pixel at a time: the bird's cell, else a pipe cell outside its gap, else background"""
    E, R, C = len(state["v"]), H // s, W // s
    out = np.zeros((E, 3, H, W), dtype=np.uint8)
    for e in range(E):
        tau, n = int(state["tau"][e]), int(state["n"][e])
        tops = {}
        for j in range(tau + 2):
            col = C + j * D - tau
            if 0 <= col <= C - 1:
                tops[col] = FR.gap_top(seed, e, n, j, R, g)
        for py in range(H):
            for px in range(W):
                ry, cx = py // s, px // s
                colour = BG
                if cx in tops and not (tops[cx] <= ry < tops[cx] + g):
                    colour = PIPE
                if cx == 1 and ry == int(state["rows"][e, 0]):
                    colour = BIRD
                out[e, :, py, px] = colour
    return out


def test_palette_is_the_issue_s():
    assert (RGB.BACKGROUND_RGB, RGB.PIPE_RGB, RGB.BIRD_RGB) == (BG, PIPE, BIRD)
    from rltime_amd.acting.flappy_env import PALETTE
    assert PALETTE == {"background": BG, "pipe": PIPE, "bird": BIRD}


@pytest.mark.parametrize("H,W,s,g,D", [(8, 8, 2, 2, 2), (24, 16, 2, 3, 4), (20, 12, 2, 3, 4)])
def test_rgb_rendering_against_frames_built_by_hand(H, W, s, g, D):
    """The reset frame (drawn: background and the bird, no pipe is on screen yet), then a stream long enough for pipes to
    scroll across, pass the bird's column and for episodes to end; the colour frame maps back to the intensity env's."""
    E, seed = 3, 2 ** 40 + 77 + H
    state, frames1, _, _ = FR.flappy_reset(seed, E, 1, H, W, s, g, D, n=[0, 5, 2 ** 31])
    got = RGB.render_rgb(state, seed, H, W, s, g, D)
    assert got.shape == (E, 3, H, W) and got.dtype == np.uint8
    R = H // s
    want = np.empty_like(got)
    for p in range(3):
        want[:, p] = BG[p]
        want[:, p, (R // 2) * s:(R // 2 + 1) * s, s:2 * s] = BIRD[p]
    assert np.array_equal(got, want)                                        # no pipe at tau = 0: column C is off screen
    rng = np.random.default_rng(5)
    pipes = birds_on_pipe_column = ends = 0
    for t in range(3 * (W // s + 3 * D)):
        actions = rng.integers(0, 2, E).astype(np.int32) if t % 3 else FR.seeking_action(state, seed, H, W, s, g, D)
        state, frames1, _, dones = FR.flappy_step(state, actions, seed, 1, H, W, s, g, D, 40, -1.0)
        got = RGB.render_rgb(state, seed, H, W, s, g, D)
        assert np.array_equal(got, _by_hand(state, seed, H, W, s, g, D)), t
        assert np.array_equal(RGB.to_classes(got), frames1), t              # the intensity env's frame through the palette
        pipes += int((frames1 == FR.PIPE).any())
        birds_on_pipe_column += int(((frames1[:, 0, :, s:2 * s] == FR.PIPE).any(axis=(1, 2))).sum())
        ends += int(dones.sum())
        assert all(int((got[e, 0] == BIRD[0]).sum()) == s * s for e in range(E))    # exactly one bird cell, never hidden
    assert pipes > 0 and birds_on_pipe_column > 0 and ends > 0


def test_to_classes_refuses_a_pixel_off_the_palette():
    state, _, _, _ = FR.flappy_reset(1, 1, 1, 8, 8, 2, 2, 2)
    f = RGB.render_rgb(state, 1, 8, 8, 2, 2, 2)
    f[0, 1, 3, 3] ^= 1
    with pytest.raises(AssertionError):
        RGB.to_classes(f)


@pytest.mark.parametrize("planes", [1, 2, 4])
def test_rgb_needs_three_planes_by_name_on_both_devices(planes):
    from rltime_amd.acting.flappy_env import check_geometry
    from rltime_amd.train import make_vec_env
    for device in ("cpu", "cuda"):
        with pytest.raises(ValueError, match=r"flappy: rgb frames are \(3, H, W\).*frame_shape\[0\] = %d" % planes):
            make_vec_env("flappy", {"frame_shape": [planes, 24, 16], "cell": 2, "rgb": True}, 2, device)
        with pytest.raises(ValueError, match=r"flappy: rgb frames are \(3, H, W\)"):
            make_vec_env("flappy", {"frame_shape": [planes, 24, 16], "cell": 2, "rgb": True, "extra_features": True}, 2, device)
    assert check_geometry((3, 24, 16), 2, 3, 4, 2, 100, rgb=True) == (3, 24, 16, 12, 8)
    assert check_geometry((3, 24, 16), 2, 3, 4, 2, 100) == (3, 24, 16, 12, 8)                    # a three-plane HISTORY stack stays legal
    # the other rules keep their names with rgb on
    with pytest.raises(ValueError, match="flappy: W % 4 == 0"):
        make_vec_env("flappy", {"frame_shape": [3, 24, 18], "cell": 2, "rgb": True}, 2, "cpu")
    # rgb is a known key now; the unknown-keys message still lists exactly the unknown ones
    with pytest.raises(ValueError, match=r"flappy: unknown env_args \['colour', 'grid'\]"):
        make_vec_env("flappy", {"frame_shape": [3, 24, 16], "cell": 2, "rgb": True, "grid": 6, "colour": 1}, 2, "cpu")
    with pytest.raises(ValueError, match="steps on the GPU only"):                               # a well-formed rgb env: the device rule is next
        make_vec_env("flappy", {"frame_shape": [3, 24, 16], "cell": 2, "rgb": True}, 2, "cpu")


def test_frame_stack_dedup_with_rgb_is_refused_before_anything_is_built(monkeypatch):
    from rltime_amd import train as T
    from rltime_amd.general.config import load_config
    cfg = load_config("flappy_iqn_lstm_rgb.json")
    built = []
    monkeypatch.setattr(T, "make_vec_env", lambda *a, **k: built.append(a) or (_ for _ in ()).throw(AssertionError("an env was built")))
    T.check_rgb_storage(cfg)                                                                      # the shipped config passes
    bad = copy.deepcopy(cfg)
    bad["training"]["args"]["history_mode"]["args"]["frame_stack_dedup"] = True
    with pytest.raises(ValueError, match="frame_stack_dedup.*rgb"):
        T.create_actors(bad)
    with pytest.raises(ValueError, match="frame_stack_dedup.*rgb"):
        T.train(bad)
    assert built == []
    grey = copy.deepcopy(bad)                                                                     # without rgb the storage option is the env's business
    grey["env_args"]["rgb"] = False
    T.check_rgb_storage(grey)


def test_the_shipped_rgb_config_is_the_intensity_config_at_the_reference_shape():
    from rltime_amd.general.config import load_config
    from rltime_amd.models.torch.fused import conv_u8_family
    from rltime_amd.models.torch.modules import CNN
    from tests.test_flappy_shapes_cpu import IQN, derive
    cfg, base = load_config("flappy_iqn_lstm_rgb.json"), load_config("flappy_iqn_lstm.json")
    assert cfg["env_args"]["frame_shape"] == [3, 120, 80] and cfg["env_args"]["rgb"] is True
    base["env_args"]["frame_shape"] = [3, 120, 80]
    base["env_args"]["rgb"] = True
    assert {k: v for k, v in cfg.items() if k != "_comment"} == {k: v for k, v in base.items() if k != "_comment"}
    d = derive("flappy_iqn_lstm_rgb.json")
    assert d["frame"] == (3, 120, 80) and d["convs"][0] == (3, 120, 80, 32, 8, 4, 29, 19)
    assert d["convs"][1:] == IQN["convs"][1:] and d["features"] == IQN["features"] == 64 * 11 * 6 == 4224      # only layer 1 differs
    assert {k: d[k] for k in d if k not in ("frame", "convs")} == {k: IQN[k] for k in IQN if k not in ("frame", "convs")}
    cnn = CNN((3, 120, 80), cfg["model"]["args"]["layer_configs"][0]["args"]["layers"], channels_last=True)
    assert cnn.out_shape == (64, 11, 6) and int(np.prod(cnn.out_shape)) == 4224 and cnn.layers[0].in_channels == 3
    p, h, w, f, k, s = d["convs"][0][:6]
    assert conv_u8_family(p).planes == 3 and conv_u8_family(p).supported(h, w, f, k, s)
