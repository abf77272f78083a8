"""The level follower (csrc/levels.h, levels.cpp: the host side soft stereo and quieting share: the level
rows' strides, the carry, hold, the copy back and the counting) checked without a GPU by
tools/check_level_follower.cpp, a stand-alone program built with g++ from the follower and stub HIP calls."""
import os
import subprocess

from conftest import REPO

CSRC = os.path.join(REPO, "software-defined-radio-course-project_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_follower_against_stub_hip_calls(tmp_path):
    """K = 1 and 2, 1 and 3 streams, 1, 3, 4 and 5 frames: two calls in a row, bytes above 16, hold from
    whole and broken granules, the reset, refused allocations, and both forms of the levels primitive."""
    exe = str(tmp_path / "check_level_follower")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(ROCM, "include"), "-o", exe, os.path.join(REPO, "tools", "check_level_follower.cpp"),
                    os.path.join(CSRC, "levels.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "failures=0" in r.stdout, r.stdout[-4000:]
    assert int(r.stdout.split("checks=")[1].split()[0]) > 500
