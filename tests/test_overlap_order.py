"""Which stream a frame's candidate-list build goes to (csrc/rt_overlap.h
ListOverlap) on the CPU: the stand-alone program tests/native/overlap_order.cpp,
built plain and with AddressSanitizer + UBSan.  It enumerates every sequence of
up to six calls (renders whose build may overlap or reads its sizes back,
readers, lists built outside a render, the switch, a setting that changes the
lists, the destroy after any prefix), lays out the launches they make on the
caller's stream and the side stream with their event edges, and checks that no
list buffer or flag word is written while a frame that reads it is unfinished
and that no build stays in flight.  No GPU."""
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
        os.path.join(REPO, "tests", "native", "overlap_order.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "overlap order ok (55986 sequences" in r.stdout


def test_overlap_order(tmp_path):
    _run(tmp_path, "overlap_order", [])


def test_overlap_order_sanitized(tmp_path):
    """The same program under the CPU AddressSanitizer + UBSan build."""
    _run(tmp_path, "overlap_order_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"],
         {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
