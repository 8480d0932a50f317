"""The shape gate, scratch size and argument checks of csrc/conv_small.hip (mirl_conv2s_*) are pure host logic: callable
without a GPU, and the launchers refuse bad arguments before anything reaches a device."""
import ctypes as C
import os
import re

import pytest

from rltime_amd import _lib
from rltime_amd._lib import lib

NAMES = ("mirl_conv2s_supported", "mirl_conv2s_bwd_data", "mirl_conv2s_wrw_scratch_bytes", "mirl_conv2s_wrw")


@pytest.mark.parametrize("h,w", [(4, 4), (20, 20), (5, 7), (29, 19), (8, 10), (25, 25)])
def test_gate_takes_the_layer(h, w):
    assert lib.mirl_conv2s_supported(16, 32, 4, 2, h, w) == 1          # 25 x 25: the largest square frame inside the LDS plan


@pytest.mark.parametrize("bad", [(32, 32, 4, 2, 20, 20), (16, 64, 4, 2, 20, 20), (16, 16, 4, 2, 20, 20), (16, 32, 3, 2, 20, 20),
                                 (16, 32, 4, 1, 20, 20), (16, 32, 4, 2, 3, 20), (16, 32, 4, 2, 20, 3),
                                 (16, 32, 4, 2, 26, 26)])                # 26 x 26: the first square frame past the 150 KiB plan
def test_gate_refuses(bad):
    assert lib.mirl_conv2s_supported(*bad) == 0


def test_launchers_refuse_before_any_device_call():
    need = C.c_int64()
    assert lib.mirl_conv2s_wrw_scratch_bytes(C.byref(need)) == 0 and need.value == 256 * 32 * 4 * 4 * 16 * 4   # 256 slabs
    assert lib.mirl_conv2s_wrw_scratch_bytes(None) == _lib.MIRL_ERR_ARG
    assert lib.mirl_conv2s_bwd_data(4, 20, 20, None, None, 256, 1, 64, 16, None, None) == _lib.MIRL_ERR_ARG
    assert lib.mirl_conv2s_wrw(4, 20, 20, None, None, None, need.value, None, None) == _lib.MIRL_ERR_ARG
    buf = (C.c_float * 64)()
    p, odd = C.addressof(buf) + (-C.addressof(buf)) % 16, C.addressof(buf) + (-C.addressof(buf)) % 16 + 4
    for args in [(0, 20, 20, p, p, 256, 1, 64, 16, p, None),             # N <= 0
                 (4, 26, 26, p, p, 256, 1, 64, 16, p, None),             # a shape outside the LDS plan
                 (4, 20, 20, odd, p, 256, 1, 64, 16, p, None)]:          # g off the 16-byte grid
        assert lib.mirl_conv2s_bwd_data(*args) == _lib.MIRL_ERR_ARG and "conv2s_bwd_data" in _lib.last_error()
    for args in [(0, 20, 20, p, p, p, need.value, p, None), (4, 3, 20, p, p, p, need.value, p, None),
                 (4, 20, 20, p, odd, p, need.value, p, None),
                 (4, 20, 20, p, p, p, 4 * 32768 - 1, p, None)]:          # scratch smaller than the launch's four slabs
        assert lib.mirl_conv2s_wrw(*args) == _lib.MIRL_ERR_ARG and "conv2s_wrw" in _lib.last_error()


def test_header_and_binding_declare_the_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mirl.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib._SIGNATURES and hasattr(lib, name), name
