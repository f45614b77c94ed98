"""Occlusion batches (include/rt_hip.h rt_hip_occluded) without a GPU: the
batch arithmetic of csrc/rt_occl_items.h as a stand-alone program (plain and
under AddressSanitizer + UBSan), where the new entry points are declared, and
the hemisphere rays of the ambient-occlusion tool."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

OCCL_ENTRIES = ("rt_hip_occluded", "rt_hip_occluded_host")


# ---- csrc/rt_occl_items.h on the CPU ----
def _run_native(tmp_path, name, flags, env=None):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags + [
        "-I" + os.path.join(REPO, "raytracing-gpu_amd", "csrc"),
        os.path.join(REPO, "tests", "native", "occl_items.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "occl items ok" in r.stdout


def test_occl_items(tmp_path):
    _run_native(tmp_path, "occl_items", [])


def test_occl_items_sanitized(tmp_path):
    """The same program under the CPU AddressSanitizer + UBSan build."""
    _run_native(tmp_path, "occl_items_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"],
                {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})


# ---- where the entry points live ----
def _decls(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(rt_\w+)\s*\(", src, re.M)}


def test_occlusion_entry_points_are_public_abi(built):
    """The two functions are declared in rt_hip.h (the drop-in boundary), not
    among the test hooks, exported by the library and bound by rtgpu."""
    import rtgpu
    pub, tst = _decls("rt_hip.h"), _decls("rt_hip_test.h")
    L = C.CDLL(rtgpu.LIB_PATH)
    bound = {p[0] for p in rtgpu._PROTOS}
    for name in OCCL_ENTRIES:
        assert name in pub and name not in tst, name
        assert hasattr(L, name), name
        assert name in bound, name
    for method in ("occluded", "occluded_device"):
        assert callable(getattr(rtgpu.Context, method))
    assert callable(rtgpu.hemisphere_rays)


# ---- hemisphere_rays ----
def test_hemisphere_rays():
    import rtgpu
    rng = np.random.default_rng(16)
    P = rng.normal(size=(257, 3)) * 10.0
    N = rng.normal(size=(257, 3)) * rng.uniform(0.1, 5.0, (257, 1))  # any length
    N[:6] = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, -2], [-3, 0, 0], [0, 0.5, 0]], np.float64)
    for k in (1, 4, 7):
        o, d = rtgpu.hemisphere_rays(P, N, k, 2026)
        assert o.dtype == d.dtype == np.float32 and o.shape == d.shape == (257 * k, 3)
        assert np.array_equal(o, np.repeat(P.astype(np.float32), k, axis=0))  # a point's k rays are consecutive
        d64 = d.astype(np.float64)
        assert np.abs(np.linalg.norm(d64, axis=1) - 1.0).max() < 1e-6
        assert (np.einsum("ij,ij->i", d64, np.repeat(N, k, axis=0)) > 0).all()
        o2, d2 = rtgpu.hemisphere_rays(P, N, k, 2026)
        assert o.tobytes() == o2.tobytes() and d.tobytes() == d2.tobytes()
        _, d3 = rtgpu.hemisphere_rays(P, N, k, 2027)
        assert d.tobytes() != d3.tobytes()
    # cosine-weighted: the mean of dot(dir, unit N) is 2/3 (a uniform hemisphere's is 1/2)
    o, d = rtgpu.hemisphere_rays(P, N, 64, 5)
    un = np.repeat(N / np.linalg.norm(N, axis=1, keepdims=True), 64, axis=0)
    assert abs(np.einsum("ij,ij->i", d.astype(np.float64), un).mean() - 2.0 / 3.0) < 0.01
    # float32 inputs of a G-buffer, a zero normal gets +z
    o, d = rtgpu.hemisphere_rays(np.zeros((2, 3), np.float32), np.array([[0, 0, 0], [0, 1, 0]], np.float32), 3, 1)
    assert (d[:3, 2] > 0).all() and (d[3:, 1] > 0).all()
