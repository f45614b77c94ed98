"""Ambient occlusion from G-buffer records (include/rt_hip.h
rt_hip_ambient_occlusion) without a GPU: the ray rule of csrc/rt_ao_items.h as
a stand-alone program (plain and under AddressSanitizer + UBSan) against its
numpy float32 twin rtgpu.ao_rays_host word for word, the rule's properties,
where the entry points are declared, and ao_open_share."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO

AO_ENTRIES = ("rt_hip_ambient_occlusion", "rt_hip_ambient_occlusion_host", "rt_hip_ao_rays")
BASES = (0, 2 ** 32 - 100, 2 ** 40 + 5)  # (the second: the hash's low word wraps inside the batch)
SAN = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def edge_records(gpu_dtype):
    """Records at the rule's edges: misses, zero, NaN, inf, underflowing and
    overflowing normals (none shoots), scaled and tiny normals, the poles n.z =
    +-1, +-0 components, a NaN and an inf hit point (all shoot)."""
    nan, inf = np.nan, np.inf
    N = [(0, 0, 1), (0, 0, -1), (0, 0, 0), (-0.0, 0.0, -0.0), (nan, 0, 1), (0, nan, 0), (inf, 0, 0), (0, -inf, 1),
         (1e-30, 0, 0), (1e-30, 1e-30, -1e-30), (1e30, 0, 0), (1e30, 1e30, 1e30), (3, -4, 12), (0.001, 0.002, -0.002),
         (1e-20, 0, 0), (0, -1e-20, 1e-21), (1e18, -1e18, 0), (1, 0, -0.0), (0, 1, 0.0), (-1, -0.0, 0.0),
         (0.0, -0.0, 1.0), (-0.0, 0.0, -1.0), (1e-8, 0, -1), (0, 1e-8, 1), (0.6, 0, -0.8), (1, 1, 1), (-1, -1, -1),
         (0, 0, 1), (0, 0, 1), (0, 0, 1), (0, 1, 0)]
    s = np.zeros(len(N), gpu_dtype)
    s["N"] = np.array(N, np.float32)
    s["P"] = np.arange(3 * len(N), dtype=np.float32).reshape(-1, 3) * np.float32(0.37) - np.float32(5)
    s["prim"] = np.arange(len(N))
    s["dist"] = 1.0
    s["prim"][-4] = -1  # a miss with a fine normal
    s["P"][-3] = (nan, 0, 0)
    s["P"][-2] = (0, inf, 0)
    return s


def seeded_records(gpu_dtype, n, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros(n, gpu_dtype)
    N = rng.normal(size=(n, 3)) * np.exp(rng.uniform(-6.0, 6.0, (n, 1)))  # any length
    N[rng.random(n) < 0.1, 2] = 0.0
    N[rng.random(n) < 0.05, 0] = -0.0
    unit = rng.random(n) < 0.5  # a G-buffer's normals are mostly about unit length
    N[unit] /= np.maximum(np.linalg.norm(N[unit], axis=1, keepdims=True), 1e-30)
    s["N"] = N.astype(np.float32)
    s["P"] = (rng.normal(size=(n, 3)) * 100.0).astype(np.float32)
    s["prim"] = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 1 << 20, n))
    return s


def same_words(a, b):
    """Word for word as uint32; two NaNs agree whatever their bits."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---- csrc/rt_ao_items.h on the CPU ----
def _build(tmp, name, flags):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags + [
        "-I" + os.path.join(REPO, "raytracing-gpu_amd", "csrc"),
        os.path.join(REPO, "tests", "native", "ao_items.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def _run(exe, args=(), env=None):
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ao items ok" in r.stdout


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """The stand-alone program, built once plain and once under the CPU
    AddressSanitizer + UBSan build; both are run as programs."""
    tmp = tmp_path_factory.mktemp("ao_items")
    return {"plain": (_build(tmp, "ao_items", []), None),
            "sanitized": (_build(tmp, "ao_items_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]), SAN)}


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_ao_items(programs, which):
    exe, env = programs[which]
    _run(exe, env=env)


def _native_rays(exe, env, tmp_path, smp, k, table, seed, base):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<QQIIII", len(smp), base, k, len(table), seed, 0))
        f.write(smp.tobytes())
        f.write(np.ascontiguousarray(table, np.float32).tobytes())
    _run(exe, (fin, fout), env)
    raw = open(fout, "rb").read()
    nr = len(smp) * k
    assert len(raw) == 24 * nr + len(smp)
    o = np.frombuffer(raw, np.float32, 3 * nr).reshape(-1, 3)
    d = np.frombuffer(raw, np.float32, 3 * nr, 12 * nr).reshape(-1, 3)
    return o, d, np.frombuffer(raw, np.uint8, len(smp), 24 * nr).astype(bool)


@pytest.fixture(scope="module")
def records():
    import rtgpu
    return np.concatenate([edge_records(rtgpu.GSAMPLE), seeded_records(rtgpu.GSAMPLE, 3000, 18)])


@pytest.mark.parametrize("which", ["plain", "sanitized"])
@pytest.mark.parametrize("m", [1, 7, 37, 64])
def test_the_numpy_twin_equals_the_header(programs, records, tmp_path, which, m):
    """ao_rays_host == the header evaluated by the native program, word for
    word, for k in {1, 3, 64, 65} (m = 37 < k wraps the table) and the three
    bases; the edge rows shoot or not as the rule says."""
    import rtgpu
    exe, env = programs[which]
    table = rtgpu.ao_table(m, 5 + m)
    for k in (1, 3, 64, 65):
        for base in BASES:
            o, d, shot = _native_rays(exe, env, tmp_path, records, k, table, 20261020, base)
            ho, hd, hshot = rtgpu.ao_rays_host(records, k, table, 20261020, base=base)
            assert np.array_equal(shot, hshot), (k, m, base, np.flatnonzero(shot != hshot)[:5])
            assert same_words(o, ho), (k, m, base)
            bad = np.flatnonzero(~((d.view(np.uint32) == hd.view(np.uint32)) | (np.isnan(d) & np.isnan(hd))).all(axis=1))
            assert len(bad) == 0, (k, m, base, len(bad), bad[:5], d[bad[:2]], hd[bad[:2]])
    e = edge_records(rtgpu.GSAMPLE)
    want = np.ones(len(e), bool)
    want[2:12] = False  # zero, NaN, inf, underflow, overflow
    want[-4] = False    # the miss
    assert np.array_equal(hshot[:len(e)], want)
    assert 0.8 < hshot[len(e):].mean() < 0.95  # the seeded records: the misses do not shoot


# ---- properties of the rule ----
def test_rule_properties(records):
    import rtgpu
    smp = records
    table = rtgpu.ao_table(37, 1)
    assert table.dtype == np.float32 and table.shape == (37, 3) and (table[:, 2] > 0).all()
    assert np.abs(np.linalg.norm(table.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert rtgpu.ao_table(37, 1).tobytes() == table.tobytes() != rtgpu.ao_table(37, 2).tobytes()
    # cosine-weighted: the mean of z is 2/3
    assert abs(rtgpu.ao_table(4096, 3)[:, 2].astype(np.float64).mean() - 2.0 / 3.0) < 0.02
    o64, d64, shot = rtgpu.ao_rays_host(smp, 64, table, 9)
    # a sample's start and symmetry do not depend on k: the first rays of k = 64 are the rays of k = 5
    o5, d5, shot5 = rtgpu.ao_rays_host(smp, 5, table, 9)
    assert np.array_equal(shot, shot5)
    assert same_words(d64.reshape(len(smp), 64, 3)[:, :5], d5.reshape(len(smp), 5, 3))
    assert same_words(o64.reshape(len(smp), 64, 3)[:, :5], o5.reshape(len(smp), 5, 3))
    # ... and row t + m is row t again
    assert same_words(d64.reshape(len(smp), 64, 3)[:, 37:], d64.reshape(len(smp), 64, 3)[:, :27])
    # pieces with bases reproduce the whole; a wrong base does not
    for base in BASES:
        wo, wd, ws = rtgpu.ao_rays_host(smp, 3, table, 9, base=base)
        cuts = [0, 1, 99, 100, 101, 1000, len(smp)]
        parts = [rtgpu.ao_rays_host(smp[a:b], 3, table, 9, base=base + a) for a, b in zip(cuts, cuts[1:])]
        assert same_words(np.concatenate([p[1] for p in parts]), wd) and same_words(np.concatenate([p[0] for p in parts]), wo)
        assert np.array_equal(np.concatenate([p[2] for p in parts]), ws)
        assert not same_words(rtgpu.ao_rays_host(smp[100:], 3, table, 9, base=base + 99)[1], wd[300:])
    assert not same_words(rtgpu.ao_rays_host(smp, 3, table, 10)[1], rtgpu.ao_rays_host(smp, 3, table, 9)[1])
    # every direction lies on the normal's side and has unit length (unit table rows)
    # (normals whose squared length is a normal float: below that l itself is rounded coarsely)
    ln = np.linalg.norm(smp["N"].astype(np.float64), axis=1)
    fin = shot & (ln > 1e-15) & (ln < 1e15)
    d = d64.reshape(len(smp), 64, 3)[fin].astype(np.float64)
    n = smp["N"][fin].astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert (np.einsum("ikj,ij->ik", d, n) > 0).all()
    assert np.abs(np.linalg.norm(d, axis=2) - 1.0).max() < 1e-6
    # a record that does not shoot: zeros, the ray no batch traces
    assert not d64.reshape(len(smp), 64, 3)[~shot].any() and not o64.reshape(len(smp), 64, 3)[~shot].any()
    # the origin is P
    assert same_words(o64.reshape(len(smp), 64, 3)[shot][:, 7], smp["P"][shot])
    # the symmetries are used: all 8 low-bit patterns and every start row occur
    h = rtgpu.ao_hash(len(smp), 9)
    assert len(np.unique(h & 7)) == 8 and len(np.unique((h >> 3) % 37)) == 37


# ---- where the entry points live ----
def _decls(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(rt_\w+)\s*\(", src, re.M)}


def test_ao_entry_points_are_public_abi(built):
    """The entry points are declared in rt_hip.h (the drop-in boundary), not
    among the test hooks, exported by the library and bound by rtgpu."""
    import rtgpu
    pub, tst = _decls("rt_hip.h"), _decls("rt_hip_test.h")
    L = C.CDLL(rtgpu.LIB_PATH)
    bound = {p[0] for p in rtgpu._PROTOS}
    for name in AO_ENTRIES + ("rt_hip_ao_rays_host",):
        assert name in pub and name not in tst, name
        assert hasattr(L, name), name
        assert name in bound, name
    for method in ("ambient_occlusion", "ambient_occlusion_device", "ao_rays", "ao_rays_device"):
        assert callable(getattr(rtgpu.Context, method))
    for fn in ("ao_table", "ao_rays_host", "ao_open_share", "hemisphere_rays"):
        assert callable(getattr(rtgpu, fn))
    assert rtgpu.AO_KMAX == 1024 and "#define RT_AO_KMAX 1024" in open(os.path.join(REPO, "include", "rt_hip.h")).read()


# ---- ao_open_share ----
def test_ao_open_share():
    import rtgpu
    smp = np.zeros(6, rtgpu.GSAMPLE)
    smp["prim"] = [0, 1, -1, 2, 3, 4]
    smp["N"][:, 2] = [1, 1, 1, 0, 1, 1]  # (a miss and a zero normal: count 0 from the device, open)
    got = rtgpu.ao_open_share(np.array([0, 4, 0, 0, 1, 3], np.uint32), smp, 4)
    assert got.dtype == np.float64 and np.array_equal(got, [1.0, 0.0, 1.0, 1.0, 0.75, 0.25])
    assert np.array_equal(rtgpu.ao_open_share(np.array([65, 0], np.uint32), smp[:2], 65), [0.0, 1.0])
    with pytest.raises(AssertionError):
        rtgpu.ao_open_share(np.zeros(5, np.uint32), smp, 4)
