"""The packet walk's box verdicts of host/rt_cull.h (rt_box_wants at the push,
rt_box_within at a popped node's re-test) on the CPU: the stand-alone program
tests/native/box_verdict.cpp, built plain and with AddressSanitizer + UBSan.
It compares both helpers with the formulas they replaced (a miss folded into an
entry parameter of +inf, then asked about again) over a full cross of special
values at the verdict's own inputs, a cross of special values through
rt_box_hit (box and origin components of +-0 and denormals, planes at +-3e38,
inv at rt_inv's +-1e30 clamp, dlen tiny and huge, limits of 0, finite and +inf,
inputs that produce NaN) and two million random slabs.  No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def _run(tmp_path, name, flags, env=None):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags + [
        "-I" + os.path.join(REPO, "raytracing-gpu_amd", "host"),
        os.path.join(REPO, "tests", "native", "box_verdict.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "box verdict ok (2203240 cases)" in r.stdout


def test_box_verdict(tmp_path):
    _run(tmp_path, "box_verdict", [])


def test_box_verdict_sanitized(tmp_path):
    """The same program under the CPU AddressSanitizer + UBSan build."""
    _run(tmp_path, "box_verdict_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"],
         {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
