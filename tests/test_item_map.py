"""The trace kernel's work-item map of csrc/rt_tiles.h (rt_item_pixel,
rt_item_slot, rt_pixel_slots) on the CPU: the stand-alone program
tests/native/item_map.cpp, built plain and with AddressSanitizer + UBSan.  It
checks the bijection of a tile's 4 x 64 (item, lane) slots onto its 64 x 4
(pixel, sample) pairs, the sample order of cpu/raytracer.c:55-58, and that
fold_kernel's and gbuffer_kernel's slots are the ones the trace writes,
contiguous and 16-byte aligned per pixel.  No GPU."""
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
        os.path.join(REPO, "tests", "native", "item_map.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "item map ok" in r.stdout


def test_item_map(tmp_path):
    _run(tmp_path, "item_map", [])


def test_item_map_sanitized(tmp_path):
    """The same program under the CPU AddressSanitizer + UBSan build."""
    _run(tmp_path, "item_map_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"],
         {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
