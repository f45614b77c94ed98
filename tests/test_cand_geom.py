"""The proof geometry of the camera rays' candidate lists (csrc/rt_cand_geom.h)
and its frame constants (csrc/rt_cand_host.cpp cand_params) on the CPU: the
stand-alone program tests/native/cand_geom.cpp, built plain and with
AddressSanitizer + UBSan and linked with csrc/rt_cand_host.cpp and
host/rt_error.c alone.  For 1000 generated triangles (small, slivers, grazing
the eye, holding the eye, crossing the frame), the frames 64x40, 474x266,
266x476 and 474x270 in compatibility mode, and every rank of 1, 2, 3 and 8: the
raster's tiles, raster_count and row_ivs agree and stay below ntiles_local; the
ranks of a split partition the one-rank frame's tiles; Q_SAFE implies SAFE;
tile_keep equals its two-part form and does not depend on the rank split.  The
set is not vacuous -- the program prints, per frame:

    64x40: safe 400 footprint 556 global 44 | entries 3436, footprints over 32 tiles 23 | tile_keep kept 3141 dropped 295
    474x266: safe 239 footprint 715 global 46 | entries 133399, footprints over 32 tiles 410 | tile_keep kept 66556 dropped 66843
    266x476: safe 234 footprint 722 global 44 | entries 126712, footprints over 32 tiles 410 | tile_keep kept 71066 dropped 55646
    474x270 compat: safe 239 footprint 715 global 46 | entries 134013, footprints over 32 tiles 400 | tile_keep kept 65006 dropped 69007

No GPU, no librtgpu.so."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

HIP_INCLUDE = "/opt/rocm/include"


def _run(tmp_path, name, flags, env=None):
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.skip("g++ missing")
    if not os.path.exists(os.path.join(HIP_INCLUDE, "hip", "hip_runtime.h")):
        pytest.skip("the HIP headers (CandParams' vector types) are missing")
    pkg = os.path.join(REPO, "raytracing-gpu_amd")
    inc = ["-I" + os.path.join(REPO, "include"), "-I" + os.path.join(pkg, "csrc"), "-I" + os.path.join(pkg, "host")]
    common = ["-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags
    err_o = str(tmp_path / (name + "_rt_error.o"))  # C11 (_Thread_local): compiled as C, linked below
    subprocess.run(["gcc", "-std=c11"] + common + inc + ["-c", os.path.join(pkg, "host", "rt_error.c"), "-o", err_o],
                   check=True)
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17"] + common + ["-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE] + inc + [
        os.path.join(REPO, "tests", "native", "cand_geom.cpp"), os.path.join(pkg, "csrc", "rt_cand_host.cpp"), err_o,
        "-o", exe, "-lpthread"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "cand geom ok" in r.stdout


def test_cand_geom(tmp_path):
    _run(tmp_path, "cand_geom", [])


def test_cand_geom_sanitized(tmp_path):
    """The same program under the CPU AddressSanitizer + UBSan build."""
    _run(tmp_path, "cand_geom_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"],
         {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
