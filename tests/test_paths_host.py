"""The path export (include/rt_hip.h rt_hip_path_records) without a GPU: the
numpy twins rtgpu.path_fold, color_mul, bounce_dir and path_coefs against
hand-written tables, the arithmetic of csrc/rt_path_items.h as a stand-alone
program (plain and under AddressSanitizer + UBSan), and where the entry points
are declared."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

SAN = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
F = np.float32


def words(a, b):
    """Equal as 32-bit words, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the twins, by hand ----
def test_path_fold_by_hand():
    """Deepest first from +0, the reference's clamp after each add: an order
    that shows in float32, the clamp in mid-path, -0.0 alone, a NaN, an empty
    path between two others and at both ends."""
    import rtgpu
    a, b = F(1.0), F(2.0 ** -24)
    assert F(F(b + b) + a) == F(1.0 + 2.0 ** -23) and F(F(a + b) + b) == F(1.0), "the order shows in float32"
    nan = F(np.nan)
    #          ray 0: empty | ray 1: three vertices       | ray 2: empty | ray 3: one vertex | ray 4: two | ray 5: empty
    offsets = np.array([0, 0, 3, 3, 4, 6, 6], np.uint32)
    terms = np.array([
        # ray 1, vertex 0 (added last), 1, 2 (added first): r deepest-first (b + b) + a; g first-hit-first would
        # give 1; b: 200 + 100 clamps to 255 before the -5 of vertex 0
        [a, b, -5.0], [b, b, 100.0], [b, a, 200.0],
        # ray 3: -0.0 alone gives +0 (+0 + -0); a NaN stays; 300 clamps
        [-0.0, nan, 300.0],
        # ray 4: the clamp is applied after each add (255 + -10, not 290 - 10 clamped); a NaN from the deepest stays
        [-10.0, 1.0, 0.5], [290.0, nan, 0.25],
    ], F)
    got = rtgpu.path_fold(offsets, terms)
    assert got.dtype == F and got.shape == (6, 3)
    want = np.array([
        [0.0, 0.0, 0.0],
        [F(F(b + b) + a), F(F(a + b) + b), 250.0],
        [0.0, 0.0, 0.0],
        [0.0, nan, 255.0],
        [245.0, nan, 0.75],
        [0.0, 0.0, 0.0],
    ], F)
    assert got[1, 0] == F(1.0 + 2.0 ** -23) and got[1, 1] == F(1.0), got[1]
    assert words(got, want), (got, want)
    assert not np.signbit(got[3, 0]) and not np.signbit(got[[0, 2, 5]]).any(), "+0 where nothing or -0.0 arrived"
    # no ray at all, and terms past offsets[n] (a capped export's unused tail) are ignored
    assert rtgpu.path_fold(np.zeros(1, np.uint32), np.zeros((0, 3), F)).shape == (0, 3)
    assert words(rtgpu.path_fold(offsets[:3], terms), want[:2])
    with pytest.raises(AssertionError):
        rtgpu.path_fold(np.array([0, 7], np.uint32), terms)  # offsets past the terms


def test_color_mul_by_hand():
    """init_color(c / 255 * coef): the clamps at 0 and 255, -0.0 and a NaN
    passing both compares, the quotient rounded before the product."""
    import rtgpu
    nan, inf = F(np.nan), F(np.inf)
    c = np.array([[255.0, 0.0, 127.5], [255.0, -0.0, 100.0], [10.0, nan, 255.0], [inf, 51.0, -inf], [200.0, 200.0, 200.0]], F)
    coef = np.array([1.0, -1.0, 2.0, 0.5, 0.0], F)
    got = rtgpu.color_mul(c, coef)
    third = F(F(F(F(100.0) / F(255.0)) * F(-1.0)) * F(255.0))
    assert third < 0
    want = np.array([
        [255.0, 0.0, F(F(F(127.5) / F(255.0)) * F(255.0))],
        [0.0, 0.0, 0.0],               # -255 and `third` clamp to 0; -0.0 / 255 * -1 = +0
        [F(F(F(F(10.0) / F(255.0)) * F(2.0)) * F(255.0)), nan, 255.0],   # 510 clamps to 255
        [255.0, F(F(F(F(51.0) / F(255.0)) * F(0.5)) * F(255.0)), 0.0],  # inf clamps to 255, -inf to 0
        [0.0, 0.0, 0.0],
    ], F)
    assert got.dtype == F and words(got, want), (got, want)
    # -0.0 passes `y < 0`: 0 / 255 * -1 * 255 = -0.0 stays -0.0
    neg = rtgpu.color_mul(np.array([[0.0, 0.0, 0.0]], F), F(-1.0))
    assert np.signbit(neg).all() and (neg == 0).all()
    # a scalar coef broadcasts; the quotient is rounded to float32 before the product
    x = F(77.0)
    one = rtgpu.color_mul(np.array([[x, x, x]], F), 0.3)
    assert one[0, 0] == F(F(F(x / F(255.0)) * F(0.3)) * F(255.0))
    assert rtgpu.color_mul(np.zeros((0, 3), F), 1.0).shape == (0, 3)


def test_bounce_dir_by_hand():
    """d - N * (2 * ((N.x d.x + N.y d.y) + N.z d.z)) in float32, N as given: a
    unit mirror, an unnormalised N, a dot product whose association shows, a
    zero N, a NaN."""
    import rtgpu
    d = np.array([[1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 1.0], [0.3, 0.4, 0.5], [1.0, 2.0, 3.0]], F)
    N = np.array([[0.0, 1.0, 0.0], [0.0, 2.0, 0.0], [1.0, 2.0 ** -24, 2.0 ** -24], [0.0, 0.0, 0.0], [np.nan, 0.0, 0.0]], F)
    got = rtgpu.bounce_dir(d, N)
    assert got.dtype == F and got.shape == (5, 3)
    assert words(got[0], F([1.0, 1.0, 0.0]))
    assert words(got[1], F([1.0, 7.0, 0.0]))  # N not normalised: -1 - 2 * (2 * -2)
    # (1 + 2^-24) + 2^-24 = 1 in float32 (left to right); 1 + (2^-24 + 2^-24) would be 1 + 2^-23
    s = F(2.0)
    assert words(got[2], F([F(1.0) - s * F(1.0), F(1.0) - F(s * F(2.0 ** -24)), F(1.0) - F(s * F(2.0 ** -24))]))
    assert words(got[3], d[3])
    assert np.isnan(got[4, 0]) and np.isnan(got[4, 1]) and np.isnan(got[4, 2])  # NaN * 0 = NaN in every component


def test_path_coefs_by_hand():
    """coef_0 = 1, coef_{v+1} = nr[obj_v] * coef_v in float32 along each path."""
    import rtgpu
    nr = np.array([0.9, 0.0, 0.3, 1.0], F)
    offsets = np.array([0, 0, 4, 5, 5, 7], np.uint32)
    rec = rtgpu.records_from_points(np.zeros((7, 3), F), np.ones((7, 3), F), [0, 0, 2, 1, 3, 3, 0], prim=rtgpu.RT_PATH_PRIM)
    got = rtgpu.path_coefs(offsets, rec, nr)
    c1 = F(F(0.9) * F(1.0))
    c2 = F(F(0.9) * c1)
    c3 = F(F(0.3) * c2)
    assert got.dtype == F and words(got, F([1.0, c1, c2, c3, 1.0, 1.0, 1.0]))
    assert rtgpu.path_coefs(np.zeros(3, np.uint32), rec[:0], nr).shape == (0,)
    assert rtgpu.RT_PATH_PRIM == 0x7fffffff and (rec["prim"] > 0).all()


# ---- csrc/rt_path_items.h on the CPU ----
def _build(tmp, name, flags):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags + [
        "-I" + os.path.join(REPO, "raytracing-gpu_amd", "csrc"),
        os.path.join(REPO, "tests", "native", "path_items.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """The stand-alone program, built once plain and once under the CPU
    AddressSanitizer + UBSan build; both are run as programs."""
    tmp = tmp_path_factory.mktemp("path_items")
    return {"plain": (_build(tmp, "path_items", []), None),
            "sanitized": (_build(tmp, "path_items_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]),
                          SAN)}


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_path_items(programs, which):
    exe, env = programs[which]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "path items ok" in r.stdout


def test_one_statement_of_the_arithmetic():
    """The kernels, the host layer and the native test include the header; the
    kernels index records and size their grids by it, the host sizes the
    scratch by it."""
    csrc = os.path.join(REPO, "raytracing-gpu_amd", "csrc")
    for path in (os.path.join(csrc, "rt_paths.cpp"), os.path.join(csrc, "rt_paths.hip"),
                 os.path.join(REPO, "tests", "native", "path_items.cpp")):
        assert '#include "rt_path_items.h"' in open(path).read(), path
    kernels = open(os.path.join(csrc, "rt_paths.hip")).read()
    assert "rt_path_rec_addr(" in kernels and "rt_path_chunks(" in kernels and "rt_path_blocks(" in kernels
    assert "p.hit_cap +" not in kernels and ">> 3" not in kernels, "no second statement of a record's address"
    host = open(os.path.join(csrc, "rt_paths.cpp")).read()
    assert "rt_path_scratch_words(" in host and "rt_path_blocks(" in host
    # the kernels are a translation unit of their own: the render's does not include them
    render = open(os.path.join(csrc, "rt_render.hip")).read()
    assert "rt_paths" not in render and "rt_path_items" not in render


# ---- where the entry points live ----
def _decls(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(rt_\w+)\s*\(", src, re.M)}


def test_path_entry_points_are_public_abi(built):
    """The entry points are declared in rt_hip.h (the drop-in boundary), not
    among the test hooks, exported by the library and bound by rtgpu; the
    header's RT_PATH_PRIM is rtgpu's."""
    import rtgpu
    pub, tst = _decls("rt_hip.h"), _decls("rt_hip_test.h")
    L = C.CDLL(rtgpu.LIB_PATH)
    bound = {p[0] for p in rtgpu._PROTOS}
    for name in ("rt_hip_path_records", "rt_hip_path_records_host"):
        assert name in pub and name not in tst, name
        assert hasattr(L, name), name
        assert name in bound, name
    for method in ("path_records", "path_records_device", "trace_paths"):
        assert callable(getattr(rtgpu.Context, method))
    for twin in ("path_fold", "color_mul", "bounce_dir", "path_coefs"):
        assert callable(getattr(rtgpu, twin))
    header = open(os.path.join(REPO, "include", "rt_hip.h")).read()
    m = re.search(r"#define\s+RT_PATH_PRIM\s+(0x[0-9a-fA-F]+)", header)
    assert m and int(m.group(1), 16) == rtgpu.RT_PATH_PRIM
