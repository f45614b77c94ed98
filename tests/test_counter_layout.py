"""The layouts of csrc/rt_counters.h (render-stat slots, candidate-list counter
block, light-buffer counters) on the CPU: the stand-alone table program
tests/native/counter_layout.cpp, built plain and with AddressSanitizer +
UBSan, and the rt_stats ABI as rtgpu.Stats mirrors it.  No GPU: the kernels'
side of the same numbers is their unchanged assembly (profiles/r13_counters/)."""
import ctypes as C
import os
import re
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
        os.path.join(REPO, "tests", "native", "counter_layout.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "counter layout ok" in r.stdout


def test_counter_layout_table(tmp_path):
    """Every slot's number, rt_stats member, pass and frame flag; the
    candidate block's words and regions; the light-buffer words."""
    _run(tmp_path, "counter_layout", [])


def test_counter_layout_table_sanitized(tmp_path):
    """The same program under the CPU AddressSanitizer + UBSan build."""
    _run(tmp_path, "counter_layout_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"],
         {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})


def test_stats_mirror_matches_the_header():
    """rtgpu.Stats names rt_stats' members in the header's order, all 64-bit."""
    import rtgpu
    with open(os.path.join(REPO, "include", "rt_hip.h")) as f:
        body = re.search(r"typedef struct rt_stats \{(.*?)\} rt_stats;", f.read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            m = re.fullmatch(r"\s*unsigned long long\s+(.*)", decl, re.S)
            assert m, decl
            names += [n.strip() for n in m.group(1).split(",")]
    assert len(names) == 29 and all(re.fullmatch(r"[a-z_]+", n) for n in names), names
    assert [n for n, _ in rtgpu.Stats._fields_] == names
    assert all(t is C.c_ulonglong for _, t in rtgpu.Stats._fields_)
    assert C.sizeof(rtgpu.Stats) == 8 * len(names)
