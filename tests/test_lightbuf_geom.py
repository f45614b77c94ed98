"""The light buffers' contract between build and query on the CPU: the
footprint geometry (csrc/rt_lightbuf_geom.h), the grid and the host survey
(csrc/rt_lightbuf_host.cpp) and the query's cell map (csrc/rt_lightbuf_cell.h)
against the reference's float Moller-Trumbore test (host/rt_mt.h) -- the
stand-alone program tests/native/lightbuf_geom.cpp, built plain and with
AddressSanitizer + UBSan and linked with csrc/rt_lightbuf_host.cpp and
host/rt_error.c alone.  400 generated triangles (small, slivers, edge-on to the
directional light, in a plane through the point light, spanning the box), one
directional and one point light, slack-grown and proven footprints, lb_fill's
cell count and 16 times as many: every row's count equals what the emission's
own loop writes; the survey's totals are those; and every (shadow ray,
triangle) pair that the float test accepts -- eight rays per triangle, all
pairs, both modes -- is global, or listed in the query's first cell with a key
within the query's limit, or (point light) listed in its second cell.  The set
is not vacuous -- the program prints, per light, mode and cell count:

    dir slack x1: cells 4288 entries 4049 | accepted pairs 8254: global 0, first cell 8254 (0 within a float step of the limit, nearest 0.00127), second cell 0 | global 0 never 0 band 0 big 1
    dir slack x16: cells 66264 entries 44139 | accepted pairs 8254: global 0, first cell 8254 (0 within a float step of the limit, nearest 0.00127), second cell 0 | global 0 never 0 band 0 big 17
    dir proven x1: cells 4278 entries 4178 | accepted pairs 8254: global 0, first cell 8254 (0 within a float step of the limit, nearest 0.0011), second cell 0 | global 14 never 56 band 0 big 1
    dir proven x16: cells 66368 entries 46071 | accepted pairs 8254: global 0, first cell 8254 (0 within a float step of the limit, nearest 0.0011), second cell 0 | global 14 never 56 band 0 big 18
    point slack x1: cells 4374 entries 6562 | accepted pairs 31480: global 30738, first cell 533 (0 within a float step of the limit, nearest 0.0155), second cell 209 | global 34 never 0 band 0 big 6
    point slack x16: cells 66150 entries 58686 | accepted pairs 31480: global 30738, first cell 533 (0 within a float step of the limit, nearest 0.0155), second cell 209 | global 34 never 0 band 0 big 89
    point proven x1: cells 4374 entries 58111 | accepted pairs 31480: global 30748, first cell 524 (0 within a float step of the limit, nearest 0.072), second cell 208 | global 50 never 0 band 75 big 79
    point proven x16: cells 66150 entries 680324 | accepted pairs 31480: global 30766, first cell 506 (0 within a float step of the limit, nearest 0.072), second cell 208 | global 54 never 0 band 72 big 114

(No accepted pair's key comes within a float step of its limit: the nearest
is 1.1e-3 below it.)  No GPU, no librtgpu.so."""
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
        pytest.skip("the HIP headers (float4) are missing")
    pkg = os.path.join(REPO, "raytracing-gpu_amd")
    inc = ["-I" + os.path.join(REPO, "include"), "-I" + os.path.join(pkg, "csrc"), "-I" + os.path.join(pkg, "host")]
    common = ["-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags
    err_o = str(tmp_path / (name + "_rt_error.o"))  # C11 (_Thread_local): compiled as C, linked below
    subprocess.run(["gcc", "-std=c11"] + common + inc + ["-c", os.path.join(pkg, "host", "rt_error.c"), "-o", err_o],
                   check=True)
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17"] + common + ["-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE] + inc + [
        os.path.join(REPO, "tests", "native", "lightbuf_geom.cpp"), os.path.join(pkg, "csrc", "rt_lightbuf_host.cpp"),
        err_o, "-o", exe, "-lpthread"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "lightbuf geom ok" in r.stdout


def test_lightbuf_geom(tmp_path):
    _run(tmp_path, "lightbuf_geom", [])


def test_lightbuf_geom_sanitized(tmp_path):
    """The same program under the CPU AddressSanitizer + UBSan build."""
    _run(tmp_path, "lightbuf_geom_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"],
         {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
