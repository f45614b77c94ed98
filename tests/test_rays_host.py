"""Ray batches (include/rt_hip.h rt_hip_trace_rays, rt_hip_frame_rays) without
a GPU: the numpy restatement of the camera-ray generator and the sample fold
against the reference's own golden pixels, the quarter order, the batch
arithmetic of csrc/rt_ray_items.h as a stand-alone program (plain and under
AddressSanitizer + UBSan), and where the new entry points are declared."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import (REPO, golden_image, load_manifest_static, load_own_manifest, own_golden_image,
                      own_scene_path)

CASES = {f'{c["scene"]}_{c["width"]}x{c["height"]}': c for c in load_manifest_static()}
OWN = {f'{c["scene"]}_{c["width"]}x{c["height"]}': c for c in load_own_manifest()}  # our scenes, rendered by cpu/rt
RAY_ENTRIES = ("rt_hip_trace_rays", "rt_hip_trace_rays_host", "rt_hip_frame_rays")


# ---- the reference's trace() in Python over the oracle's exported pieces ----
class _Vec(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class _Ray(C.Structure):
    _fields_ = [("origin", _Vec), ("direction", _Vec)]


def _oracle():
    import oracle as orc
    L = orc.lib()
    L.oracle_collide.argtypes = [C.c_void_p, _Ray, C.POINTER(C.c_int)]
    L.oracle_collide.restype = _Ray
    L.oracle_apply_light.argtypes = [C.c_void_p, C.c_int, _Ray]
    L.oracle_apply_light.restype = orc.ColorS
    return L, orc


def _trace(L, orc, scene, nr, o, d, coef, counts):
    """cpu/raytracer.c:19-34 with the bounce of cpu/ray.c:16-25 in float32."""
    f32 = np.float32
    if float(coef) < 0.01:
        return orc.ColorS(0.0, 0.0, 0.0)
    counts[0] += 1
    oi = C.c_int(-1)
    hit = L.oracle_collide(scene, _Ray(_Vec(*o), _Vec(*d)), C.byref(oi))
    n = [f32(hit.direction.x), f32(hit.direction.y), f32(hit.direction.z)]
    if n[0] == 0 and n[1] == 0 and n[2] == 0:
        return orc.ColorS(0.0, 0.0, 0.0)
    local = L.oracle_apply_light(scene, oi.value, hit)
    dot = f32(f32(n[0] * d[0]) + f32(n[1] * d[1])) + f32(n[2] * d[2])  # v_dot: left to right, float
    k = f32(2) * dot
    nd = [f32(d[a] - f32(n[a] * k)) for a in range(3)]
    no = [f32(hit.origin.x), f32(hit.origin.y), f32(hit.origin.z)]
    refl = _trace(L, orc, scene, nr, no, nd, f32(nr[oi.value] * f32(coef)), counts)
    return L.oracle_color_add(refl, L.oracle_color_mul(local, f32(coef)))


def _pixels(case, count, seed):
    """A seeded sample of PPM pixels, the frame's corners always among them."""
    rng = np.random.default_rng(seed)
    W, H = case["width"], case["height"]
    pix = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)}
    while len(pix) < count:
        pix.add((int(rng.integers(H)), int(rng.integers(W))))
    return sorted(pix)


@pytest.mark.parametrize("name,count", [("cube_96x54", 48), ("spheres_96x54", 36), ("mirrors_32x18", 24)])
def test_camera_rays_and_fold_reproduce_golden_pixels(built, scene_dir, tmp_path, name, count):
    """camera_rays (pixel order: ray 4 (row W + col) + s, s in cpu sample order)
    traced by the reference's own recursion and folded by fold_samples gives
    the golden image's pixels bit for bit: the generator's pixel map, sample
    order and arithmetic and the fold, pinned with no GPU."""
    import rtgpu
    L, orc = _oracle()
    if name in OWN:
        case = OWN[name]
        s = rtgpu.Scene.load_svati(own_scene_path(case, tmp_path))
        gold = own_golden_image(case)
    else:
        case = CASES[name]
        s = rtgpu.Scene.load_svati(os.path.join(scene_dir, case["scene"] + ".svati"))
        gold = golden_image(case)
    s.set_size(case["width"], case["height"])
    o, d = rtgpu.camera_rays(s.frame(), "pixel")
    assert o.dtype == np.float32 and o.shape == d.shape == (4 * case["width"] * case["height"], 3)
    nr = rtgpu.scene_materials(s.ptr)[:, 11]
    scene = C.cast(s.ptr, C.c_void_p)
    pix = _pixels(case, count, 20261020)
    rgb = np.zeros((len(pix), 4, 3), np.float32)
    counts = [0]
    for k, (row, col) in enumerate(pix):
        for smp in range(4):
            i = 4 * (row * case["width"] + col) + smp
            c = _trace(L, orc, scene, nr, list(o[i]), list(d[i]), np.float32(1.0), counts)
            rgb[k, smp] = (c.r, c.g, c.b)
    got = rtgpu.fold_samples(rgb.reshape(-1, 3))
    want = np.stack([gold[r, c] for r, c in pix])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        [(p, g, w) for p, g, w in zip(pix, got, want) if not np.array_equal(g, w)][:4]
    assert counts[0] >= 4 * len(pix)


def test_fold_samples_is_the_reference_average(built):
    """fold_samples against oracle_color_add / oracle_color_mul on values
    that clamp, round and carry NaN."""
    import rtgpu
    L, orc = _oracle()
    rng = np.random.default_rng(7)
    rgb = (rng.random((64, 4, 3)) * 300.0 - 20.0).astype(np.float32)
    rgb[3, 1, 2] = np.nan
    rgb[5] = 255.0
    want = np.zeros((64, 3), np.float32)
    for k in range(64):
        acc = orc.ColorS(0.0, 0.0, 0.0)
        for smp in range(4):
            acc = L.oracle_color_add(acc, L.oracle_color_mul(orc.ColorS(*[float(x) for x in rgb[k, smp]]), 0.25))
        want[k] = (acc.r, acc.g, acc.b)
    got = rtgpu.fold_samples(rgb.reshape(-1, 3))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("W,H", [(4, 4), (8, 4), (12, 8), (100, 52), (256, 256)])
def test_quarter_order_is_a_bijection_of_quarters(W, H):
    """Every aligned 64 rays of the quarter order are one 4x4-pixel quarter x 4
    samples in rt_item_pixel's lane order (lane = 4 (4 r + c) + s), quarters in
    scanline order; perm and inv are inverse permutations."""
    import rtgpu
    perm, inv = rtgpu.quarter_order(W, H)
    n = 4 * W * H
    assert perm.shape == inv.shape == (n,)
    assert np.array_equal(np.sort(perm), np.arange(n))
    assert np.array_equal(perm[inv], np.arange(n)) and np.array_equal(inv[perm], np.arange(n))
    px, smp = perm >> 2, perm & 3
    row, col = px // W, px % W
    k = np.arange(n)
    assert np.array_equal((row // 4) * (W // 4) + col // 4, k // 64)
    assert np.array_equal(4 * (4 * (row % 4) + col % 4) + smp, k % 64)


def test_quarter_order_refuses_other_sizes():
    import rtgpu
    for W, H in ((96, 54), (6, 4), (0, 4)):
        with pytest.raises(ValueError):
            rtgpu.quarter_order(W, H)


def test_camera_rays_quarter_order_is_the_permuted_pixel_order(built, scene_dir):
    import rtgpu
    s = rtgpu.Scene.load_svati(os.path.join(scene_dir, "cube.svati"))
    s.set_size(100, 52)
    f = s.frame()
    o, d = rtgpu.camera_rays(f, "pixel")
    oq, dq = rtgpu.camera_rays(f, "quarter")
    perm, _ = rtgpu.quarter_order(100, 52)
    assert np.array_equal(oq.view(np.uint32), o[perm].view(np.uint32))
    assert np.array_equal(dq.view(np.uint32), d[perm].view(np.uint32))
    ln = np.linalg.norm(d.astype(np.float64), axis=1)
    assert np.all(np.abs(ln - 1.0) < 1e-6)


def test_equirect_and_ortho_rays_shapes():
    import rtgpu
    o, d = rtgpu.equirect_rays((1.0, 2.0, 3.0), 16, 8)
    assert o.shape == d.shape == (128, 3) and o.dtype == d.dtype == np.float32
    assert np.all(o == np.array([1.0, 2.0, 3.0], np.float32))
    assert np.all(np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0) < 1e-6)
    assert d[:16, 1].min() > 0 > d[-16:, 1].max()  # the top row looks up, the bottom row down
    assert len(np.unique(d, axis=0)) == 128
    o, d = rtgpu.ortho_rays((0.0, 0.0, -5.0), (2.0, 0.0, 0.0), (0.0, 3.0, 0.0), 4.0, 8, 4)
    assert o.shape == d.shape == (32, 3)
    assert np.all(d == np.array([0.0, 0.0, 1.0], np.float32))
    assert np.allclose(o[:, 0].min(), -1.75) and np.allclose(o[:, 0].max(), 1.75)
    assert np.allclose(o[0, 1], 0.75) and np.allclose(o[-1, 1], -0.75) and np.all(o[:, 2] == -5.0)


# ---- csrc/rt_ray_items.h on the CPU ----
def _run_native(tmp_path, name, flags, env=None):
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags + [
        "-I" + os.path.join(REPO, "raytracing-gpu_amd", "csrc"),
        os.path.join(REPO, "tests", "native", "ray_items.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ray items ok" in r.stdout


def test_ray_items(tmp_path):
    _run_native(tmp_path, "ray_items", [])


def test_ray_items_sanitized(tmp_path):
    """The same program under the CPU AddressSanitizer + UBSan build."""
    _run_native(tmp_path, "ray_items_asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"],
                {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})


# ---- where the entry points live ----
def _decls(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(rt_\w+)\s*\(", src, re.M)}


def test_ray_entry_points_are_public_abi(built):
    """The three functions are declared in rt_hip.h (the drop-in boundary), not
    among the test hooks, exported by the library and bound by rtgpu."""
    import rtgpu
    pub, tst = _decls("rt_hip.h"), _decls("rt_hip_test.h")
    L = C.CDLL(rtgpu.LIB_PATH)
    bound = {p[0] for p in rtgpu._PROTOS}
    for name in RAY_ENTRIES:
        assert name in pub and name not in tst, name
        assert hasattr(L, name), name
        assert name in bound, name
    src = open(os.path.join(REPO, "include", "rt_hip.h")).read()
    assert re.search(r"#define\s+RT_RAYS_PACKET\s+1u", src)
    assert rtgpu.RT_RAYS_PACKET == 1
    for method in ("trace_rays", "frame_rays"):
        assert callable(getattr(rtgpu.Context, method))

