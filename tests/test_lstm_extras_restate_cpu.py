"""CPU: the float32 restatement of the extras add (tests/lstm_extras_restate.py, what csrc/lstm_extras.hip
k_lstm_extras_add computes) against float64 within the bound its fixed order implies, and the host logic of the C ABI:
the shape gate, the workspace size and the refusals, none of which touches a device."""
import ctypes as C

import numpy as np
import pytest

from tests.lstm_extras_restate import extras_add, extras_add_bound, extras_add_f64, one_hot_extras


@pytest.mark.parametrize("X", [1, 5, 20, 32])
@pytest.mark.parametrize("dense", [False, True])
def test_restatement_is_within_its_bound_of_float64(X, dense):
    rng = np.random.default_rng(100 * X + dense)
    M, N = 67, 260
    src = (rng.standard_normal((M, N)) * 3).astype(np.float32)
    wx = rng.standard_normal((N, X)).astype(np.float32)
    e = rng.standard_normal((M, X)).astype(np.float32) if dense else one_hot_extras(rng, M, X)
    got = extras_add(src, e, wx)
    assert got.dtype == np.float32 and got.shape == (M, N)
    err = np.abs(got.astype(np.float64) - extras_add_f64(src, e, wx))
    bound = extras_add_bound(src, e, wx)
    print("X=%d dense=%d max err / bound = %.3f" % (X, dense, float(np.max(err / np.maximum(bound, 1e-300)))))
    assert np.all(err <= bound)
    assert np.any(got != src)


def test_restatement_order_is_the_stated_one():
    """Three terms whose float32 sum depends on the order: ascending x from src is the one the restatement takes."""
    src = np.array([[2.0 ** 24]], np.float32)
    e = np.array([[1.0, 1.0, -2.0 ** 24]], np.float32)
    wx = np.ones((1, 3), np.float32)
    assert extras_add(src, e, wx)[0, 0] == 0.0            # (2^24 + 1) rounds to 2^24 twice, then - 2^24
    assert extras_add_f64(src, e, wx)[0, 0] == 2.0
    zero = np.zeros((2, 4), np.float32)
    assert np.array_equal(extras_add(zero + 1.5, zero[:, :3], np.ones((4, 3), np.float32)), zero + 1.5)


def test_shape_gate_workspace_and_refusals_are_host_logic():
    from rltime_amd._lib import MIRL_ERR_ARG, lib
    for ok in [(1, 4, 1), (1, 4, 32), (300, 2048, 20), (40960, 2048, 5), (67, 260, 5), (1 << 33, 8, 3)]:
        assert lib.mirl_lstm_extras_supported(*ok) == 1, ok
    for bad in [(0, 4, 1), (-1, 4, 1), (1, 0, 1), (1, 2, 1), (1, 6, 1), (1, 262, 5), (1, 4, 0), (1, 4, 33), (1, 4, -1), (1, -4, 1)]:
        assert lib.mirl_lstm_extras_supported(*bad) == 0, bad
    need = C.c_int64(-1)
    assert lib.mirl_lstm_extras_wgrad_workspace_bytes(1, 4, 1, C.byref(need)) == 0 and need.value == 0
    assert lib.mirl_lstm_extras_wgrad_workspace_bytes(256, 260, 5, C.byref(need)) == 0 and need.value == 0      # one chunk
    assert lib.mirl_lstm_extras_wgrad_workspace_bytes(257, 260, 5, C.byref(need)) == 0 and need.value == 2 * 260 * 5 * 4
    assert lib.mirl_lstm_extras_wgrad_workspace_bytes(4099, 2048, 32, C.byref(need)) == 0 and need.value == 17 * 2048 * 32 * 4
    assert lib.mirl_lstm_extras_wgrad_workspace_bytes(257, 260, 5, None) == MIRL_ERR_ARG
    assert lib.mirl_lstm_extras_wgrad_workspace_bytes(257, 262, 5, C.byref(need)) == MIRL_ERR_ARG
    assert lib.mirl_lstm_extras_wgrad_workspace_bytes(257, 260, 33, C.byref(need)) == MIRL_ERR_ARG
    # the launchers refuse before anything touches a device: shapes outside the gate, null operands
    for M, N, X in [(4, 8, 0), (4, 8, 33), (4, 6, 5), (0, 8, 5), (4, 8, 5)]:
        assert lib.mirl_lstm_extras_add(M, N, X, None, N, None, X, None, X, None, N, None) == MIRL_ERR_ARG
        assert lib.mirl_lstm_extras_wgrad(M, N, X, None, N, None, X, None, None, 0, None) == MIRL_ERR_ARG
