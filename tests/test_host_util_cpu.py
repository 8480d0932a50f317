"""The launchers' host arithmetic (rltime_amd/csrc/host_util.hpp: magic_u32, aligned16, capped_grid), checked by a
stand-alone C++ program built with the host compiler under AddressSanitizer + UBSan and run directly."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_host_util_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "host_util_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "host_util_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "host_util ok" in run.stdout, run.stdout
