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
is 1.1e-3 below it.)

A second pass puts every row of tests/light_edges_util.py's light table in the
lights' place (the program holds the vectors as a C array, positions scaled by
5 to its box; the row names and vectors it prints must be the module's) and
adds the 1,331 points of the box's integer lattice to the origins.  Checks 1-3
hold for every row, both modes, 1 and 16 times the cells; non-vacuity is per
row.  Where the reference accepts pairs: at least 1,000 accepted and at least
50 found through a cell, the first and the second cell counted apart (observed,
slack x1: directions 10,415 to 15,011, all through the first cell; lattice
centre 55,050 = 54,133 global + 582 + 335, wall vertex 21,728 = 20,281 + 1,445
+ 2, wall plane 14,433 = 7,486 + 6,947 + 0, box corner 18,477 = 3,498 + 14,979
+ 0, inside the box 23,135 = 22,073 + 975 + 87, 1e6: 6,626 and 10,796, the
control 16,311).  Exactly 0 accepted under the directions 1e-20, 3e-39 and
1e30 and the point lights 1e9 and 3e38 away (|a| < 1e-7, or t = distance /
|d| < 1e-7: what the reference's test gives); 400 of 400 triangles `never`
under 1e-20 and the denormal in proven mode; the zero vector refused with its
message.  The five lattice lights run again over 1,200 triangles on the
lattice (edges exactly in the cube map's face boundaries): 1,573 to 9,944
accepted, 264 to 5,232 through a cell.  A third pass: +-inf and NaN in one
component, both kinds of light and both modes (36 cases), are refused by
lb_derive_grid with "light with a non-finite vector" -- host only.  The
sanitized build adds -fsanitize=float-cast-overflow.  No GPU, no librtgpu.so."""
import os
import re
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
    return r.stdout


def _check_rows(out):
    """The program's table is tests/light_edges_util.py's, row for row, and
    every row printed its four builds (or its four refusals)."""
    import numpy as np

    import light_edges_util as lu
    heads = re.findall(r"^row (.+?) \| v = (\S+) (\S+) (\S+)$", out, re.M)
    assert [h[0] for h in heads] == lu.ROW_NAMES
    for (name, t, v), h in zip(lu.geom_rows(), heads):
        got = np.array([float(x) for x in h[1:]], np.float32)
        assert got.tobytes() == np.array(v, np.float32).tobytes(), (name, got, v)
    lattice_rows = re.findall(r"^lattice row (.+?) \| point (slack|proven) x(1|16): ", out, re.M)
    assert [n for n, _, _ in lattice_rows[::4]] == [r[0] for r in lu.ROWS if r[1] == lu.POINT and r[3]], lattice_rows[::4]
    for name, t, _ in lu.geom_rows():
        kind = "dir" if t == lu.DIRECTIONAL else "point"
        lines = re.findall(rf"^row {re.escape(name)} \| (?:{kind} )?(slack|proven) x(1|16): (.*)$", out, re.M)
        assert [(m, x) for m, x, _ in lines] == [("slack", "1"), ("slack", "16"), ("proven", "1"), ("proven", "16")], name
        if name == "dir zero":
            assert all(rest == "refused: directional light with a zero vector" for _, _, rest in lines)
    # the cube map's side as light_edges_util restates it (tie and cell counts depend on it) is the build's:
    # 400 generated and 1,200 lattice triangles, lb_fill's target and 16 times it
    cells = re.findall(r"^(lattice row|row) .+? \| point (?:slack|proven) x(1|16): cells (\d+) ", out, re.M)
    assert len(cells) == 4 * 10 + 4 * 5
    for tag, mul, n in cells:
        assert int(n) == 6 * lu.cube_side(1200 if tag == "lattice row" else 400, int(mul)) ** 2, (tag, mul, n)
    assert "non-finite vectors: 36 of 36 refused" in out


def test_lightbuf_geom(tmp_path):
    _check_rows(_run(tmp_path, "lightbuf_geom", []))


def test_lightbuf_geom_sanitized(tmp_path):
    """The same program under the CPU AddressSanitizer + UBSan build, with
    -fsanitize=float-cast-overflow (a NaN or an out-of-range float turned into
    an unsigned cell coordinate is reported, not only undefined)."""
    _check_rows(_run(tmp_path, "lightbuf_geom_asan",
                     ["-fsanitize=address,undefined,float-cast-overflow", "-fno-omit-frame-pointer"],
                     {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1",
                      "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}))
