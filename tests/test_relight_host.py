"""The relight bookkeeping (csrc/rt_relight.h: which stored visibility bits
are current, which light buffers an edit rebuilds, which lights the next
relight queries and which of its paths runs) on the CPU: the stand-alone
table program tests/native/relight_plan.cpp, built plain and with
AddressSanitizer + UBSan.  No GPU: the GPU tests see the plan only through
images and query counts."""
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
        "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "raytracing-gpu_amd", "csrc"),
        os.path.join(REPO, "tests", "native", "relight_plan.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "relight plan table ok" in r.stdout


def test_relight_plan_table(tmp_path):
    """Colour-only edits, a moved light, type changes, insert / remove /
    append, 0 lights, 33 and more lights, every invalidating event."""
    _run(tmp_path, "relight_plan", [])


def test_relight_plan_table_sanitized(tmp_path):
    """The same program under the CPU AddressSanitizer + UBSan build."""
    _run(tmp_path, "relight_plan_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"],
         {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
