"""The three-plane input layer's launch plans (rltime_amd/csrc/host_util.hpp c3p_fwd_plan / c3p_wrw_plan / c3p_shape_ok),
checked by a stand-alone C++ program built with the host compiler under AddressSanitizer + UBSan and run directly: grid
within the cap, LDS within the limit, and the forward's work split walked as the kernel walks it — every frame and every
tile exactly once for N in {1, 2, 3, 5, 33, 1025} at (8, 8), (44, 52) and (120, 80)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_three_plane_launch_plans_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "host_util_check3p")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "host_util_check3p.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "host_util 3p ok" in run.stdout, run.stdout
