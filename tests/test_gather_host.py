"""The gather (include/rt_hip.h rt_hip_gather) without a GPU: the accumulation
rule rtgpu.gather_sum against a hand-written table that shows its order, the
slot arithmetic of csrc/rt_gather_items.h as a stand-alone program (plain and
under AddressSanitizer + UBSan), and where the entry points are declared."""
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


# ---- gather_sum: the rule, by hand ----
def test_gather_sum_by_hand():
    """Sequential float32 adds in ray order from +0, the reference's clamp at
    255 after each: values where (a + b) + c != a + (b + c) in float32, a -0.0
    first term, an inf with a -inf, a NaN, the clamp in mid-sum."""
    import rtgpu
    a, b, c = F(1.0), F(2.0 ** -24), F(2.0 ** -24)
    assert F(F(a + b) + c) == F(1.0) and F(a + F(b + c)) == F(1.0 + 2.0 ** -23), "the order shows in float32"
    inf, nan = F(np.inf), F(np.nan)
    # four records of k = 3 rays; channels r, g, b carry different cases
    colours = np.array([
        # record 0: r (a + b) + c;  g the same terms, small ones first;  b -0.0 first
        [a, b, -0.0], [b, c, 0.0], [c, a, 0.0],
        # record 1: r -0.0 thrice (+0 + -0 = +0);  g inf then -inf;  b -inf then inf
        [-0.0, inf, -inf], [-0.0, -inf, inf], [-0.0, 0.0, 0.0],
        # record 2: r the clamp in mid-sum (200 + 100 -> 255, then - 5);  g NaN stays;  b a sum of 255 exactly
        [200.0, 1.0, 100.0], [100.0, nan, 155.0], [-5.0, 300.0, 0.0],
        # record 3: r, g zeros;  b 255 + tiny stays 255
        [0.0, 0.0, 255.0], [0.0, -0.0, 1e-3], [0.0, 0.0, 0.0],
    ], F)
    got = rtgpu.gather_sum(colours, 3)
    assert got.dtype == F and got.shape == (4, 3)
    want = np.array([
        [F(F(a + b) + c), F(F(b + c) + a), 0.0],
        # inf is clamped to 255 before -inf arrives: 255 + -inf = -inf; -inf + inf = NaN
        [0.0, -inf, nan],
        [250.0, nan, 255.0],
        [0.0, 0.0, 255.0],
    ], F)
    assert got[0, 0] == F(1.0) and got[0, 1] == F(1.0 + 2.0 ** -23), got[0]
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (got, want)
    # +0.0 where only -0.0 arrived: the accumulator starts at +0
    assert not np.signbit(got[0, 2]) and not np.signbit(got[1, 0]) and not np.signbit(got[3, 1])
    # k = 1: the colour itself, clamped; the shape may be flat
    one = rtgpu.gather_sum(np.array([1.5, -2.0, 300.0, -0.0, nan, inf], F), 1)
    assert np.array_equal(one[0], F([1.5, -2.0, 255.0])) and one[1, 0] == 0 and not np.signbit(one[1, 0])
    assert np.isnan(one[1, 1]) and one[1, 2] == F(255.0)
    # not numpy's pairwise sum, not float64: 1 + 2^-24 * 4096 terms stays 1 sequentially
    many = np.zeros((4097, 3), F)
    many[0], many[1:] = 1.0, F(2.0 ** -24)
    assert (rtgpu.gather_sum(many, 4097) == F(1.0)).all()
    assert rtgpu.gather_sum(np.zeros((0, 3), F), 4).shape == (0, 3)
    with pytest.raises(AssertionError):
        rtgpu.gather_sum(np.zeros((7, 3), F), 3)


# ---- csrc/rt_gather_items.h on the CPU ----
def _build(tmp, name, flags):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags + [
        "-I" + os.path.join(REPO, "raytracing-gpu_amd", "csrc"),
        os.path.join(REPO, "tests", "native", "gather_items.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """The stand-alone program, built once plain and once under the CPU
    AddressSanitizer + UBSan build; both are run as programs."""
    tmp = tmp_path_factory.mktemp("gather_items")
    return {"plain": (_build(tmp, "gather_items", []), None),
            "sanitized": (_build(tmp, "gather_items_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]),
                          SAN)}


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_gather_items(programs, which):
    exe, env = programs[which]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "gather items ok" in r.stdout


def test_one_statement_of_the_slots():
    """The host layer, both kernels and the native test include the header; no
    one restates the slot arithmetic."""
    csrc = os.path.join(REPO, "raytracing-gpu_amd", "csrc")
    for path in (os.path.join(csrc, "rt_gather.cpp"), os.path.join(csrc, "rt_gather.h"),
                 os.path.join(REPO, "tests", "native", "gather_items.cpp")):
        assert '#include "rt_gather_items.h"' in open(path).read(), path
    kernels = open(os.path.join(csrc, "rt_gather.h")).read()
    assert "rt_gather_round_slot(" in kernels and "rt_gather_slot(" in kernels
    host = open(os.path.join(csrc, "rt_gather.cpp")).read()
    assert "rt_gather_path_groups(" in host and "rt_gather_item_count(" in host


# ---- where the entry points live ----
def _decls(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(rt_\w+)\s*\(", src, re.M)}


def test_gather_entry_points_are_public_abi(built):
    """The entry points are declared in rt_hip.h (the drop-in boundary), not
    among the test hooks, exported by the library and bound by rtgpu."""
    import rtgpu
    pub, tst = _decls("rt_hip.h"), _decls("rt_hip_test.h")
    L = C.CDLL(rtgpu.LIB_PATH)
    bound = {p[0] for p in rtgpu._PROTOS}
    for name in ("rt_hip_gather", "rt_hip_gather_host"):
        assert name in pub and name not in tst, name
        assert hasattr(L, name), name
        assert name in bound, name
    for method in ("gather", "gather_device"):
        assert callable(getattr(rtgpu.Context, method))
    assert callable(rtgpu.gather_sum)
