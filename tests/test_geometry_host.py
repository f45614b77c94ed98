"""Moving geometry, the CPU side (include/rt_hip.h rt_hip_set_triangles): the
header the host flatten and the device update share (host/rt_zero_risk.h,
tests/native/zero_risk_twin.cpp, built plain and with AddressSanitizer +
UBSan), Scene.set_triangles_array against the oracle, object_range, and the
edit helpers of rtgpu.py against a value table computed once by scalar float32
arithmetic from their definitions.  No GPU: tests/test_geometry.py."""
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
