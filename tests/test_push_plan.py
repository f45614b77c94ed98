"""The packet walk's one-step child push of csrc/rt_push_plan.h
(rt_push_lane, rt_push_wanted, rt_push_rank, rt_push_commit) on the CPU: the
stand-alone program tests/native/push_plan.cpp, built plain and with
AddressSanitizer + UBSan.  It compares the plan with a literal copy of the
serial far-to-near loop it replaced over every child mask, every wanted subset,
every near octant and every room 0..8 left on the stack (472,392 cases): the
same children in the same slots, the same sp, the same overflow count, nothing
written past the stack.  No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def _run(tmp_path, name, flags, env=None):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags + [
        "-I" + os.path.join(REPO, "raytracing-gpu_amd", "csrc"),
        os.path.join(REPO, "tests", "native", "push_plan.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "push plan ok (472392 cases)" in r.stdout


def test_push_plan(tmp_path):
    _run(tmp_path, "push_plan", [])


def test_push_plan_sanitized(tmp_path):
    """The same program under the CPU AddressSanitizer + UBSan build."""
    _run(tmp_path, "push_plan_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"],
         {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
