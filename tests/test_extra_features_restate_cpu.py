"""CPU: the extra-features step in NumPy (tests/extra_features_restate.py, what csrc/acting.hip k_extra_features computes)
against the unmodified reference's ExtraFeaturesEnvWrapper on every fixture case (tests/golden/extra_features_cases.npz,
written by tests/golden/generate_extra_features.py), bit for bit.  Plus the host side: the device wrapper's parameter list
against the reference's and the argument checks of make_vec_env, all of which are made before any env is built."""
import inspect
import json
import os

import numpy as np
import pytest

from tests.extra_features_restate import ExtraFeatures, feature_size

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extra_features_cases.npz")


@pytest.fixture(scope="module")
def cases():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def load_params(cases):
    return json.loads(str(cases["params"]))


def flags_of(p):
    return p["include_action"], p["include_reward"], p["include_timestep"]


def test_fixture_covers_the_cases_the_kernel_can_go_wrong_at(cases):
    params = load_params(cases)
    assert len(params) == int(cases["num_cases"])
    default = dict(json.loads(str(cases["wrapper_signature"])))["timestep_scale"]
    assert default == 1. / 100000
    assert {p["A"] for p in params} == {1, 3, 6, 18}
    every = {(a, r, t) for a in (True, False) for r in (True, False) for t in (True, False)} - {(False, False, False)}
    for A in (1, 3, 6, 18):
        assert {flags_of(p) for p in params if p["A"] == A} == every
        assert {(p["clip_reward"], p["timestep_scale"]) for p in params if p["A"] == A} == \
            {(c, s) for c in (True, False) for s in (default, 1. / 7)}
    first_done, long_episode = 0, 0
    for k, p in enumerate(params):
        rewards, dones, rows = cases["c%d_rewards" % k], cases["c%d_dones" % k], cases["c%d_rows" % k]
        assert rewards.dtype == np.float32 and dones.dtype == np.uint8 and rows.dtype == np.float32
        assert cases["c%d_actions" % k].dtype == np.int32 and rows.shape == (p["T"] + 1, feature_size(p["A"], *flags_of(p)))
        assert np.any(rewards == 0) and np.any(rewards != np.rint(rewards))          # zero and fractional rewards
        assert np.all(dones[5:8] == 1)                                                # dones on consecutive steps
        first_done += int(dones[0])
        run = np.diff(np.flatnonzero(np.concatenate([[1], dones, [1]])))              # gaps between dones
        long_episode += int(run.max() >= 300)
    assert first_done >= 10 and long_episode >= 4
    # the long episodes tell a double product from a float one: some timestep differs when the multiply is made in float32
    differs = 0
    for k, p in enumerate(params):
        if p["long"] and p["include_timestep"]:
            col = cases["c%d_rows" % k][:, p["A"]]
            n = np.rint(col.astype(np.float64) / p["timestep_scale"]).astype(np.int64)
            differs += int(np.any((n.astype(np.float32) * np.float32(p["timestep_scale"])) != col))
    assert differs >= 1


def test_restatement_equals_the_reference(cases):
    for k, p in enumerate(load_params(cases)):
        ef = ExtraFeatures(1, p["A"], *flags_of(p), p["clip_reward"], p["timestep_scale"])
        want = cases["c%d_rows" % k]
        got = [ef.reset()[0]]
        for t in range(p["T"]):
            got.append(ef.step(cases["c%d_actions" % k][t:t + 1], cases["c%d_rewards" % k][t:t + 1], cases["c%d_dones" % k][t:t + 1])[0])
        got = np.stack(got)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), k


def test_reset_row_sets_the_first_action_element():
    assert ExtraFeatures(2, 3).reset().tolist() == [[1, 0, 0, 0, 0]] * 2


def test_out_of_range_action_sets_no_element():
    ef = ExtraFeatures(3, 4)
    rows = ef.step(np.array([-1, 4, 2], np.int32), np.array([2.0, -0.5, 0.0], np.float32), np.zeros(3, np.uint8))
    assert rows[:, :4].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0]]
    assert rows[:, 5].tolist() == [1.0, -1.0, 0.0] and np.all(rows[:, 4] == np.float32(1e-5))


def test_wrapper_keeps_the_reference_parameters(cases):
    from rltime_amd.acting.extra_features import ExtraFeaturesVecEnv
    want = json.loads(str(cases["wrapper_signature"]))
    got = [[n, None if p.default is inspect.Parameter.empty else p.default]
           for n, p in inspect.signature(ExtraFeaturesVecEnv.__init__).parameters.items()]
    assert got == want


def test_size_helper_is_host_logic():
    import ctypes as C
    from rltime_amd._lib import lib, MIRL_ERR_ARG
    X = C.c_int32()
    for A in (1, 3, 6, 18):
        for a in (0, 1):
            for r in (0, 1):
                for t in (0, 1):
                    rc = lib.mirl_extra_features_size(A, a, r, t, C.byref(X))
                    if a or r or t:
                        assert rc == 0 and X.value == feature_size(A, a, r, t)
                    else:
                        assert rc == MIRL_ERR_ARG
    assert lib.mirl_extra_features_size(0, 1, 1, 1, C.byref(X)) == MIRL_ERR_ARG
    assert lib.mirl_extra_features_size(3, 2, 1, 1, C.byref(X)) == MIRL_ERR_ARG
    assert lib.mirl_extra_features_size(3, 1, 1, 1, None) == MIRL_ERR_ARG
    # the launch refuses before anything touches a device
    assert lib.mirl_extra_features_step(4, 3, 0, 0, 0, 1, 1e-5, None, None, None, None, None, None, 0, 0, None) == MIRL_ERR_ARG
    assert lib.mirl_extra_features_step(4, 3, 1, 1, 1, 1, 1e-5, None, None, None, None, None, None, 0, 0, None) == MIRL_ERR_ARG


@pytest.mark.parametrize("env,args,match", [
    ("catch", {"extra_features": {"include_actions": True}}, "unknown arguments"),
    ("synthetic-atari", {"extra_features": {"scale": 0.5}}, "unknown arguments"),
    ("CartPole-v1", {"extra_features": True}, "CartPole"),
    ("CartPole-v0", {"extra_features": {"clip_reward": False}}, "CartPole"),
    ("catch", {"extra_features": {"include_action": False, "include_reward": False, "include_timestep": False}}, "at least one"),
    ("synthetic-atari", {"extra_features": {"include_action": False, "include_reward": False, "include_timestep": False}}, "at least one"),
    ("catch", {"extra_features": "yes"}, "true"),
])
def test_make_vec_env_refuses_before_building_an_env(env, args, match):
    from rltime_amd.train import make_vec_env
    with pytest.raises(ValueError, match=match):
        make_vec_env(env, args, 4, "cuda")


def test_cartpole_without_extra_features_is_unchanged():
    from rltime_amd.train import make_vec_env
    env = make_vec_env("CartPole-v1", {"extra_features": False}, 2, "cpu")
    assert not hasattr(env.observation_space, "spaces")
    env.close()


def test_shipped_config_asks_for_the_wrapper():
    from rltime_amd.general.config import load_config, validate_config
    cfg = load_config("catch_iqn_lstm.json")
    validate_config(cfg)
    assert cfg["env"] == "catch" and cfg["env_args"]["extra_features"] is True
    assert cfg["env_args"]["visible_rows"] < cfg["env_args"]["grid"]
    assert cfg["training"]["type"] == "iqn" and cfg["training"]["args"]["history_mode"]["type"] == "prioritized_replay"
    assert [layer["type"] for layer in cfg["model"]["args"]["layer_configs"]] == ["cnn", "lstm", "fc"]
