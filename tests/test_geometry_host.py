"""Moving geometry, the CPU side (include/rt_hip.h rt_hip_set_triangles): the
header the host flatten and the device update share (host/rt_zero_risk.h,
tests/native/zero_risk_twin.cpp, built plain and with AddressSanitizer +
UBSan), Scene.set_triangles_array against the oracle, object_range, and the
edit helpers of rtgpu.py against a value table computed once by scalar float32
arithmetic from their definitions.  No GPU: tests/test_geometry.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

HOST = os.path.join(REPO, "raytracing-gpu_amd", "host")
HOST_SRC = ["rt_error.c", "lex_prescan.c", "par_write.c", "scene_svati.c", "scene_obj.c", "vecmath.c", "ppm.c",
            "synth.c", "accel.c", "accel_probe.c"]


def _twin(tmp_path, name, flags, env=None):
    if not shutil.which("gcc") or not shutil.which("g++"):
        pytest.skip("gcc / g++ missing")
    inc = ["-I" + os.path.join(REPO, "include"), "-I" + HOST]
    common = ["-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra"] + flags
    objs = []
    for src in HOST_SRC:  # the host C side as the library builds it (C11), the twin as the device file includes the header (C++17)
        obj = str(tmp_path / (name + "_" + src[:-2] + ".o"))
        subprocess.run(["gcc", "-std=c11"] + common + inc + ["-c", os.path.join(HOST, src), "-o", obj], check=True)
        objs.append(obj)
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17"] + common + inc + [os.path.join(REPO, "tests", "native", "zero_risk_twin.cpp")]
                   + objs + ["-lm", "-lpthread", "-lz", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "zero risk twin ok" in r.stdout


def test_zero_risk_twin(tmp_path):
    """rt_tri_normal_can_vanish and origin_tri_dist2 on the fixed table, and
    rt_flatten flagging the same objects."""
    _twin(tmp_path, "zero_risk_twin", [])


def test_zero_risk_twin_sanitized(tmp_path):
    """The same program under the CPU AddressSanitizer + UBSan build."""
    _twin(tmp_path, "zero_risk_twin_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"],
          {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})


@pytest.fixture(scope="module")
def rt(built):
    import rtgpu
    return rtgpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_set_triangles_array_round_trips(rt, scene_dir):
    s = rt.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    t0 = s.triangles_array()
    assert t0.shape == (4812, 6, 3)
    rng = np.random.default_rng(7)
    # a range across an object boundary, in both accepted shapes
    first, n = rt.object_range(s, 1)
    lo, hi = first - 5, first + 9
    new = rng.standard_normal((hi - lo, 6, 3)).astype(np.float32)
    s.set_triangles_array(new, first=lo)
    t1 = s.triangles_array()
    assert np.array_equal(_bits(t1[lo:hi]), _bits(new))
    assert np.array_equal(_bits(t1[:lo]), _bits(t0[:lo])) and np.array_equal(_bits(t1[hi:]), _bits(t0[hi:]))
    s.set_triangles_array(t0.reshape(-1, 18))  # the whole scene, (n, 18)
    assert np.array_equal(_bits(s.triangles_array()), _bits(t0))
    s.set_triangles_array(np.zeros((0, 6, 3), np.float32), first=4812)  # an empty range at the end
    with pytest.raises(IndexError):
        s.set_triangles_array(new, first=4812 - len(new) + 1)
    with pytest.raises(ValueError):
        s.set_triangles_array(np.zeros((3, 17), np.float32))


def test_object_range_agrees_with_prim_object_triangle(rt, scene_dir):
    for name in ("spheres", "dir-light-shadows", "cube"):
        s = rt.Scene.load_svati(os.path.join(scene_dir, name + ".svati"))
        end = 0
        for k in range(int(s.s.object_count)):
            first, n = rt.object_range(s, k)
            assert first == end and n == int(s.s.objects[k].triangle_count)
            if n:
                assert rt.prim_object_triangle(s, first) == (k, 0)
                assert rt.prim_object_triangle(s, first + n - 1) == (k, n - 1)
            end = first + n
        assert end == s.triangle_count
        with pytest.raises(IndexError):
            rt.object_range(s, int(s.s.object_count))


def test_oracle_sees_the_edit_and_the_restore(rt, scene_dir):
    import oracle as orc
    s = rt.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(32, 18)
    ref0, cnt0 = orc.render(s.ptr, 32, 18, threads=4)
    t0 = s.triangles_array()
    first, n = rt.object_range(s, 3)
    ext = rt.vertex_extent(t0)
    s.set_triangles_array(rt.shift_triangles(t0[first:first + n], ext * np.array([0.125, 0.0625, -0.03125], np.float32)),
                          first)
    ref1, _ = orc.render(s.ptr, 32, 18, threads=4)
    assert not np.array_equal(_bits(ref1), _bits(ref0))
    s.set_triangles_array(t0[first:first + n], first)
    ref2, cnt2 = orc.render(s.ptr, 32, 18, threads=4)
    assert np.array_equal(_bits(ref2), _bits(ref0)) and cnt2 == cnt0


# Two triangles and what the edits make of them, computed once by scalar
# float32 arithmetic from the definitions (every operation rounded to float32,
# sums left to right): ext = the largest side of the vertex box; shift = every
# vertex + ext * (0.125, 0.0625, -0.03125); spin = ((v - m) @ R.T + m, n @ R.T)
# about the float32 mean m of the six vertices, R = [[c, 0, s], [0, 1, 0],
# [-s, 0, c]], c, s = float32(cos 0.3), float32(sin 0.3); scale = every vertex
# * (1.0625, 0.9375, 1.125).  Little-endian float32 words, (2, 6, 3).
TABLE_IN = [[[0.5, 1.25, -2.0], [3.0, 0.125, 0.75], [-1.5, 2.5, 4.0], [0.0, 0.6, 0.8], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]],
            [[10.0, -0.375, 6.5], [7.25, 8.0, -9.0], [0.1, 0.2, 0.3], [0.6, 0.0, 0.8], [0.0, 1.0, 0.0], [-0.8, 0.6, 0.0]]]
TABLE_EXT = 15.5
TABLE = {
    "shift": "00001c4000000e4000001fc000009e4000008c3f0000883e0000e03e00005e4000006140000000009a99193fcdcc4c3f0000803f"
             "00000000000000000000000000000000000080bf00003f410000183f0080c0400000134100800f4100c017c1666602409a99953f"
             "cccc3cbe9a99193f00000000cdcc4c3f000000000000803f00000000cdcc4cbf9a99193f00000000",
    "spin": "00806a3b0000a03ff3f68cbf2b184d400000003ea47e493f703009be00002040c418a7401517723e9a99193f26a7433fef90743f"
            "000000006d4e97be6d4e97be00000000ef9074bf8b753941fcffbfbeb1c586404a458c4000000041d1881cc1082f9a3ed0cc4c3e"
            "c56a9b3f22434f3f00000000d242163f000000000000803f0000000026a743bf9a99193f1517723e",
    "scale": "0000083f0000963f000010c000004c400000f03d0000583f0000ccbf0000164000009040000000009a99193fcdcc4c3f0000803f"
             "00000000000000000000000000000000000080bf00002a410000b4be0000ea400080f6400000f040000022c19a99d93d0000403e"
             "cdccac3e9a99193f00000000cdcc4c3f000000000000803f00000000cdcc4cbf9a99193f00000000",
}


def test_edit_helpers_reproduce_the_value_table(rt):
    t = np.array(TABLE_IN, np.float32)
    keep = t.copy()
    ext = rt.vertex_extent(t)
    assert ext.dtype == np.float32 and float(ext) == TABLE_EXT
    got = {"shift": rt.shift_triangles(t, ext * np.array([0.125, 0.0625, -0.03125], np.float32)),
           "spin": rt.spin_triangles(t, 0.3), "scale": rt.scale_triangles(t)}
    for name, a in got.items():
        want = np.frombuffer(bytes.fromhex(TABLE[name]), "<f4").reshape(2, 6, 3)
        assert a.dtype == np.float32 and a.shape == (2, 6, 3)
        assert np.array_equal(_bits(a), _bits(want)), f"{name}: {a.tolist()}"
    assert np.array_equal(_bits(t), _bits(keep)), "the helpers return new arrays"
    # (n, 18) rows are accepted too
    assert np.array_equal(_bits(rt.scale_triangles(t.reshape(2, 18))), _bits(got["scale"]))


# ---- the derived geometry, word for word (rt_flatten_image) ---------------------
# The host flatten against the numpy float32 reference of
# tests/geometry_words_util.py; the device side is tests/test_geometry_words.py.
import glob
import gzip

import geometry_words_util as gw

RT_EINVAL = -1
GOLDEN_SCENES = sorted(os.path.basename(p)[:-len(".svati.gz")]
                       for p in glob.glob(os.path.join(REPO, "tests", "golden", "scenes", "*.svati.gz")))
ADVERSARIAL = ["twins", "room", "slivers"]


def _flags_by_object(rec, counts):
    """Word 11 is 0 or 1 and the same over each object.  (Which objects: the
    predicate's truth table and rt_flatten's use of it are zero_risk_twin.cpp's.)"""
    flag = gw.bits(rec)[:, 11]
    assert set(np.unique(flag)) <= {0, 1}
    at = 0
    for c in counts:
        assert len(set(flag[at:at + c].tolist())) <= 1, f"object of prims [{at}, {at + c})"
        at += c
    return flag


def _check_host(rt, s, what):
    arrays = rt.flatten_arrays(s)
    counts = gw.object_counts(s)
    flag = _flags_by_object(arrays[0], counts)
    # (boxes by value: numpy's minimum / maximum leave the sign of a zero open)
    gw.check_against_reference(arrays, s.triangles_array(), counts, flag, what, box_bits=False)
    return arrays


@pytest.mark.parametrize("name", GOLDEN_SCENES)
def test_flatten_arrays_equal_the_numpy_reference(rt, scene_dir, name):
    assert len(GOLDEN_SCENES) >= 18
    s = rt.Scene.load_svati(os.path.join(scene_dir, name + ".svati"))
    assert s.triangle_count > 0
    _check_host(rt, s, name)


@pytest.mark.parametrize("name", ADVERSARIAL)
def test_flatten_arrays_equal_the_numpy_reference_adversarial(rt, tmp_path, name):
    import adversarial_util as adv
    case = next(c for c in adv.load_manifest() if c["scene"] == name and (c["width"], c["height"]) == (32, 18))
    s = rt.Scene.load_svati(adv.scene_path(case, tmp_path))
    _check_host(rt, s, name)


def test_flatten_arrays_equal_the_numpy_reference_edge_scene(rt, tmp_path):
    """The 1,900-prim scene of distinct words, then the tables of awkward
    normals and vertices written over its first 257 triangles."""
    tris = gw.distinct_triangles(1900, 20261020)
    s = gw.checked_scene(rt, tmp_path / "edge.svati", tris, gw.EDGE_COUNTS)
    rec, nrm, pbox, box = _check_host(rt, s, "edge scene")
    assert not gw.bits(rec)[:, 11].any(), "the generated normals stay away from the risk"
    # (no zero anywhere: these boxes are numpy's bit for bit)
    gw.check_against_reference((rec, nrm, pbox, box), s.triangles_array(), gw.EDGE_COUNTS, np.zeros(1900), "edge scene")
    t = s.triangles_array()
    t[:257, 3:], idx = gw.normal_table(257)
    s.set_triangles_array(t)
    rec, nrm, _, _ = _check_host(rt, s, "normals table")
    R = len(gw.NORMAL_ROWS)
    assert np.isnan(nrm[gw.ROW_ZERO]).all() and np.isnan(nrm[gw.ROW_UNDERFLOW, [1, 2, 4, 5, 7, 8]]).all()
    assert np.isinf(nrm[gw.ROW_UNDERFLOW, [0, 3, 6]]).all()
    assert (nrm[gw.ROW_OVERFLOW] == 0).all() and (gw.bits(nrm[gw.ROW_OVERFLOW, :3]) >> 31).tolist() == [0, 1, 0]
    assert idx[:R].tolist() == [[i] * 3 for i in range(R)]
    assert (gw.bits(rec)[:300, 11] == 1).all() and not gw.bits(rec)[300:, 11].any(), "the all-zeros rows flag object 0"
    t[:257, 3:] = gw.distinct_triangles(257, 7)[:, 3:]
    t[:257, :3] = gw.vertex_table(257)
    s.set_triangles_array(t)
    _check_host(rt, s, "vertex table")


def _single(rt, tmp_path, vertices):
    """One-triangle-per-row scenes: the vertex rows written over a scene of
    len(rows) clean triangles in one object."""
    v = np.asarray(vertices, gw.F32).reshape(-1, 3, 3)
    t = gw.distinct_triangles(len(v), 11)
    s = gw.checked_scene(rt, tmp_path / "zeros.svati", t, (len(v),))
    t = s.triangles_array()
    t[:, :3] = v
    s.set_triangles_array(t)
    return s


NEG0, POS0 = 0x80000000, 0x00000000


def test_box_zeros_have_one_sign_whatever_the_vertex_order(rt, tmp_path):
    """The sign of a zero in the vertex boxes and the scene box, pinned: of two
    zeros the minimum is -0 and the maximum +0 (host/rt_minmax.h), in all six
    vertex orders and both prim orders.  fminf / fmaxf, which the flatten used
    before, chose by operand position (glibc: fminf(-0, +0) = +0, fminf(+0, -0)
    = -0), so lo.x of (-0, +0, 5) was +0, of (+0, -0, 5) was -0, and the scene
    box kept the first zero it met; the device's v_min3_f32 / v_max3_f32 gave
    -0 / +0 throughout, so an updated context differed from a fresh one."""
    lo_rows = [[(c, 1.0, 2.0) for c in order] for order in gw.ZERO_LO]   # x = the triple, y = 1, z = 2
    hi_rows = [[(c, 1.0, 2.0) for c in order] for order in gw.ZERO_HI]
    s = _single(rt, tmp_path, lo_rows + hi_rows)
    _, _, pbox, box = rt.flatten_arrays(s)
    pb = gw.bits(pbox)
    assert (pb[:6, 0] == NEG0).all() and (pbox[:6, 3] == 5).all(), [hex(int(x)) for x in pb[:6, 0]]
    assert (pb[6:, 3] == POS0).all() and (pbox[6:, 0] == -5).all(), [hex(int(x)) for x in pb[6:, 3]]
    assert (gw.bits(box) == gw.bits(np.array([-5, 1, 2, 5, 1, 2], gw.F32))).all()
    # the scene box: two triangles whose lo.x / hi.y are the two zeros, in both prim orders
    a = [(NZ, NZ, 3.0), (NZ, NZ, 3.0), (NZ, NZ, 3.0)]
    b = [(PZ, PZ, 3.0), (PZ, PZ, 3.0), (PZ, PZ, 3.0)]
    for order in ([a, b], [b, a]):
        s = _single(rt, tmp_path, order)
        _, _, pbox, box = rt.flatten_arrays(s)
        assert gw.bits(box).tolist() == [NEG0, NEG0, gw.bits(gw.F32(3))[()], POS0, POS0, gw.bits(gw.F32(3))[()]]
        assert sorted(gw.bits(pbox)[:, 0].tolist()) == [POS0, NEG0]  # (each prim's own box keeps its own zero)


NZ, PZ = gw.NZ, gw.PZ


def test_word_hooks_refuse_null_arguments(rt, scene_dir):
    L = rt.lib()
    s = rt.Scene.load_svati(os.path.join(scene_dir, "cube.svati"))
    box = np.zeros(6, np.float32)
    assert L.rt_flatten_image(None, None, None, None, box.ctypes.data_as(C.c_void_p)) == RT_EINVAL
    assert L.rt_flatten_image(s.ptr, None, None, None, None) == RT_EINVAL
    assert L.rt_flatten_image(s.ptr, None, None, None, box.ctypes.data_as(C.c_void_p)) == 0  # a NULL output is skipped
    assert np.array_equal(gw.bits(box), gw.bits(rt.flatten_arrays(s)[3])) and box[0] < box[3]
    need = (C.c_size_t * 2)()
    assert L.rt_hip_geometry_image(None, None, None, None, box.ctypes.data_as(C.c_void_p)) == RT_EINVAL
    assert L.rt_hip_scene_image(None, None, 0, None, 0, need) == RT_EINVAL
