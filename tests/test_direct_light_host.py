"""Direct light for caller's records (include/rt_hip.h rt_hip_direct_light)
without a GPU: the tests' reference helper against the reference's own traced
colours, the numpy statement of the shadow rays and of the shading predicate,
csrc/rt_dlight_items.h as a stand-alone program (plain and under
AddressSanitizer + UBSan), and where the entry points are declared."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import direct_light_util as du
from conftest import REPO

F32 = np.float32
DL_ENTRIES = ("rt_hip_direct_light", "rt_hip_direct_light_host")
SAN = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


# ---- 1: the reference helper agrees with the reference's own images ----
@pytest.mark.parametrize("name", ["cube", "point-light", "dir-light-shadows"])
def test_reference_helper_gives_the_traced_colours(built, scene_dir, name):
    """For the first hits of the 32x18 camera rays on objects with nr == 0 the
    traced colour is color_add(0, color_mul(apply_light, 1.0)): the helper's
    apply_light per record gives the oracle's traced colour bit for bit."""
    import oracle as orc
    import rtgpu
    s = rtgpu.Scene.load_svati(os.path.join(scene_dir, name + ".svati"))
    s.set_size(32, 18)
    o, d = rtgpu.camera_rays(s.frame(), "pixel")
    rgb, first, _ = orc.trace_rays(s.ptr, o, d, first=True)
    nr = rtgpu.scene_materials(s.ptr)[:, 11]
    pick = np.flatnonzero((first["obj"] >= 0) & (nr[np.maximum(first["obj"], 0)] == 0))
    assert len(pick) > 100, (name, len(pick), "the scene has first hits on objects with nr == 0")
    rec = rtgpu.records_from_points(first["P"][pick], first["N"][pick], first["obj"][pick])
    assert rtgpu.direct_light_shades(rec, int(s.s.object_count)).all()
    local, mask = du.oracle_direct_light(s, rec)
    L, _ = du.oracle_lib()
    want = np.zeros_like(local)
    for k in range(len(rec)):
        c = L.oracle_color_add(orc.ColorS(0.0, 0.0, 0.0), L.oracle_color_mul(orc.ColorS(*map(float, local[k])), 1.0))
        want[k] = (c.r, c.g, c.b)
    bad = du.differing(want, rgb[pick])
    assert len(bad) == 0, (name, len(bad), bad[:5], want[bad[:3]], rgb[pick][bad[:3]])
    cast = rtgpu.casting_lights(s.lights())
    assert cast and (mask & ~np.uint32(sum(1 << li for li in cast))).max() == 0, "only casting lights have a bit"


def test_material_column_is_nr(built, scene_dir):
    """(column 11 of scene_materials is the reflectivity test 1 selects by)"""
    import rtgpu
    s = rtgpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    m = rtgpu.scene_materials(s.ptr)
    assert [float(m[k, 11]) for k in range(len(m))] == [float(s.s.objects[k].nr) for k in range(len(m))]


# ---- 2: shadow_rays_host and direct_light_shades ----
def test_shadow_rays_and_predicate_on_the_edge_block():
    import rtgpu
    rec, want = du.edge_block(rtgpu.GSAMPLE, 3)
    got = rtgpu.direct_light_shades(rec, 3)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert not rtgpu.direct_light_shades(rec, 0).any()
    assert rtgpu.direct_light_shades(rec, 2).sum() == want.sum() - 1  # the record of the last object
    lights = [(0, 1, 1, 1, 9, 9, 9), (1, 1, 1, 1, 0.5, -0.25, 1e30), (3, 1, 1, 1, 1, 1, 1), (2, .5, .5, .5, 3e38, -1, 2.5),
              (2, 1, 1, 1, 1, 2, 3), (1, 1, 1, 1, 0, -0.0, 0)]
    assert rtgpu.casting_lights(lights) == [1, 3, 4, 5]
    rays = rtgpu.shadow_rays_host(rec, lights)
    assert len(rays) == 4
    P = rec["P"]
    with np.errstate(all="ignore"):
        # cpu/light.c:53: vector3_scale(light.v, -1); cpu/light.c:78: vector3_sub(light.v, point.origin)
        d1 = np.tile(np.array([F32(0.5) * F32(-1), F32(-0.25) * F32(-1), F32(1e30) * F32(-1)], F32), (len(rec), 1))
        d3 = np.stack([F32(3e38) - P[:, 0], F32(-1) - P[:, 1], F32(2.5) - P[:, 2]], axis=1).astype(F32)
        d4 = np.stack([F32(1) - P[:, 0], F32(2) - P[:, 1], F32(3) - P[:, 2]], axis=1).astype(F32)
        d5 = np.tile(np.array([F32(0) * F32(-1), F32(-0.0) * F32(-1), F32(0) * F32(-1)], F32), (len(rec), 1))
    for (o, d), wd in zip(rays, (d1, d3, d4, d5)):
        assert o.dtype == d.dtype == F32 and o.tobytes() == P.tobytes()
        assert len(du.differing(d, wd)) == 0
        assert d.shape == (len(rec), 3)
    # the signs of zero are the products' and differences': -0.0 for 0 * -1, +0.0 for 1 - 1
    assert np.signbit(rays[3][1][0]).tolist() == [True, False, True]
    k = int(np.flatnonzero((P == (1, 2, 3)).all(axis=1))[0])
    assert rays[2][1][k].tobytes() == np.zeros(3, F32).tobytes()  # the light at P: direction +0 +0 +0
    # ctypes lights give the same rays
    arr = (rtgpu.Light * len(lights))()
    for l, (t, r, g, b, x, y, z) in zip(arr, lights):
        l.type, l.r, l.g, l.b, l.v.x, l.v.y, l.v.z = t, r, g, b, x, y, z
    for (o, d), (o2, d2) in zip(rays, rtgpu.shadow_rays_host(rec, arr)):
        assert o.tobytes() == o2.tobytes() and len(du.differing(d, d2)) == 0


def test_records_from_points():
    import rtgpu
    r = rtgpu.records_from_points([[1, 2, 3], [4, 5, 6]], [[0, 1, 0], [0, 0, 2]], [0, 1])
    assert r.dtype == rtgpu.GSAMPLE and r["prim"].tolist() == [0, 0] and r["obj"].tolist() == [0, 1]
    assert r["P"].tolist() == [[1, 2, 3], [4, 5, 6]] and r["N"].tolist() == [[0, 1, 0], [0, 0, 2]]
    assert rtgpu.records_from_points(np.zeros((3, 3)), np.ones((3, 3)), 2, prim=-1)["prim"].tolist() == [-1] * 3
    assert len(rtgpu.records_from_points(np.zeros((0, 3)), np.zeros((0, 3)), 0)) == 0


# ---- 3: csrc/rt_dlight_items.h on the CPU ----
def _build(tmp, name, flags):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags + [
        "-I" + os.path.join(REPO, "raytracing-gpu_amd", "csrc"),
        os.path.join(REPO, "tests", "native", "dlight_items.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def _run(exe, args=(), env=None):
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "dlight items ok" in r.stdout


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dlight_items")
    return {"plain": (_build(tmp, "dlight_items", []), None),
            "sanitized": (_build(tmp, "dlight_items_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]), SAN)}


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_dlight_items(programs, which):
    exe, env = programs[which]
    _run(exe, env=env)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_the_numpy_predicate_equals_the_header(programs, tmp_path, which):
    """direct_light_shades == rt_dl_shades evaluated by the native program on
    the edge block and on seeded records whose words are random bits (every
    class of float in P and N, any prim and obj)."""
    import rtgpu
    exe, env = programs[which]
    rng = np.random.default_rng(27)
    edge, want = du.edge_block(rtgpu.GSAMPLE, 5)
    rnd = rng.integers(0, 1 << 32, (4000, 10), dtype=np.uint64).astype(np.uint32)
    rnd[:, 1] = rng.integers(-2, 8, 4000).astype(np.int32).view(np.uint32)  # obj around [0, 5)
    rnd[1000:, 4:] = rng.normal(size=(3000, 6)).astype(F32).view(np.uint32)  # mostly finite
    rnd[2000:, 0] &= 0x7fffffff
    rec = np.concatenate([edge, rnd.view(rtgpu.GSAMPLE).reshape(-1)])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<QII", len(rec), 5, 0))
        f.write(rec.tobytes())
    _run(exe, (fin, fout), env)
    got = np.frombuffer(open(fout, "rb").read(), np.uint8).astype(bool)
    tw = rtgpu.direct_light_shades(rec, 5)
    assert np.array_equal(got, tw), np.flatnonzero(got != tw)[:5]
    assert np.array_equal(tw[:len(edge)], want)
    assert 0.2 < tw[len(edge):].mean() < 0.8, "some seeded records shade and some do not"


# ---- 4: where the entry points live ----
def _decls(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(rt_\w+)\s*\(", src, re.M)}


def test_direct_light_entry_points_are_public_abi(built):
    import rtgpu
    pub, tst = _decls("rt_hip.h"), _decls("rt_hip_test.h")
    L = C.CDLL(rtgpu.LIB_PATH)
    bound = {p[0] for p in rtgpu._PROTOS}
    for name in DL_ENTRIES:
        assert name in pub and name not in tst, name
        assert hasattr(L, name), name
        assert name in bound, name
    assert "rt_hip_lightbuf_box" in tst and "rt_hip_lightbuf_box" not in pub and hasattr(L, "rt_hip_lightbuf_box")
    for method in ("direct_light", "direct_light_device", "lightbuf_box"):
        assert callable(getattr(rtgpu.Context, method))
    for fn in ("records_from_points", "shadow_rays_host", "direct_light_shades", "casting_lights"):
        assert callable(getattr(rtgpu, fn))
