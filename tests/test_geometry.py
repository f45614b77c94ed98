"""Moving geometry on the GPU (include/rt_hip.h rt_hip_set_triangles): new
triangles in a live context, everything that depends on them rebuilt on the
device (csrc/rt_geom.hip).  The defining property, checked after every update
by test_relight.py's rule: the updated context renders, counts and describes
itself exactly as a fresh context created on the edited rt_scene with the same
accel and settings, and the image is the oracle's at 0 ULP.

The edits (float32 throughout, rtgpu.py helpers; ext = the float32 largest
side of the scene's vertex box): shift(k) = object k plus ext * (0.125, 0.0625,
-0.03125); grow(k) = object k plus ext * (2, 0, 0), which triples the scene
box; spin(k) = object k turned by 0.3 about the y axis through its vertices'
mean; scale = every vertex times (1.0625, 0.9375, 1.125).
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import golden_image, load_own_manifest, own_scene_path

pytestmark = pytest.mark.gpu
OWN_CASES = load_own_manifest()
RT_EINVAL = -1
RT_EZERONORMAL = -9
ACCELS = ["flat", "octree_gpu"]
F32 = np.float32
INFO_TIMING = ("build_seconds", "lightbuf_seconds")


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ulp_diff(a, b):
    ai = a.view(np.int32).astype(np.int64)
    bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7FFFFFFF), ai)
    bi = np.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return np.abs(ai - bi)


def assert_bitexact(img, ref, what):
    """test_gpu.py's rule: 0 ULP in every channel."""
    d = _ulp_diff(np.ascontiguousarray(img), np.ascontiguousarray(ref))
    if d.max() != 0:
        bad = np.argwhere(d.reshape(-1, 3).max(axis=1) > 0)[:5].ravel()
        pytest.fail(f"{what}: {int((d > 0).sum())} channels differ, max {int(d.max())} ulp, "
                    f"first bad flat pixels {bad.tolist()}")


def _scene(gpu, scene_dir, tmp_path, name, W, H):
    if name == "mirrors":
        case = next(c for c in OWN_CASES if (c["width"], c["height"]) == (32, 18))
        s = gpu.Scene.load_svati(own_scene_path(case, tmp_path))
    elif name == "room":
        import adversarial_util as adv
        case = next(c for c in adv.load_manifest() if c["scene"] == "room" and (c["width"], c["height"]) == (W, H))
        s = gpu.Scene.load_svati(adv.scene_path(case, tmp_path))
    else:
        s = gpu.Scene.load_svati(os.path.join(scene_dir, name + ".svati"))
    s.set_size(W, H)
    return s


def _edit(gpu, s, kind, k=None, angle=0.3, base=None):
    """Applies the edit to the host rt_scene (what the oracle and a fresh
    context see) and returns (first, the new triangles) for the live context.
    base: the triangles the edit starts from (default: the scene's own)."""
    t = s.triangles_array() if base is None else base
    ext = gpu.vertex_extent(t)
    first, n = (0, len(t)) if kind == "scale" else gpu.object_range(s, k)
    part = t[first:first + n]
    if kind == "shift":
        new = gpu.shift_triangles(part, ext * np.array([0.125, 0.0625, -0.03125], F32))
    elif kind == "grow":
        new = gpu.shift_triangles(part, ext * np.array([2, 0, 0], F32))
    elif kind == "spin":
        new = gpu.spin_triangles(part, angle)
    else:
        new = gpu.scale_triangles(part)
    s.set_triangles_array(new, first)
    return first, new


def _info(ctx):
    return {k: v for k, v in ctx.info().items() if k not in INFO_TIMING}


def _matches_fresh(gpu, ctx, img, st, s, accel, what, setup=None, frame=None):
    """The `_check` rule of tests/test_relight.py, for an updated context: the
    bits equal render_image of a fresh context on the edited rt_scene (brought
    to the same settings by `setup`), every stats counter and every non-timing
    rt_accel_info field (device_bytes included) equal the fresh context's, the
    context validates, and the image is the oracle's at 0 ULP with its closest
    / shadow counts."""
    import oracle as orc
    f = frame or s.frame()
    fresh = gpu.Context(s, accel)
    if setup:
        setup(fresh)
    fimg, fst = fresh.render_image(f)
    finfo = _info(fresh)
    fresh.validate()
    fresh.close()
    assert np.array_equal(_bits(img), _bits(fimg)), \
        f"{what}: {int((_bits(img) != _bits(fimg)).sum())} channels differ from a fresh context's render"
    assert st == fst, f"{what}: stats {[(k, st[k], fst[k]) for k in st if st[k] != fst[k]]}"
    ctx.validate()
    info = _info(ctx)
    assert info == finfo, f"{what}: info {[(k, info[k], finfo[k]) for k in info if info[k] != finfo[k]]}"
    ref, cnt = orc.render(s.ptr, f.width, f.height, threads=4)
    if not np.array_equal(_bits(img), _bits(ref)):
        # The fresh context differs from the oracle identically (asserted
        # above): the README's known tested-not-proven reflection class (the
        # culling slack's reflection walk), not this feature.  Then the proven
        # reflection walk must give the oracle's bits, on the updated context.
        print(f"{what}: differs from the oracle as a fresh context does; asserting under exact reflections")
        ctx.set_exact_reflections(True)
        img2, st2 = ctx.render_image(f)
        ctx.set_exact_reflections(False)
        assert_bitexact(img2, ref, what + " vs oracle (exact reflections)")
        assert (st2["closest"], st2["shadow"]) == (cnt["closest"], cnt["shadow"])
    else:
        assert (st["closest"], st["shadow"]) == (cnt["closest"], cnt["shadow"]), what
    return fst


# ---- 1: the matrix ----------------------------------------------------------
MATRIX = [("spheres", 96, 54, "shift", 3), ("spheres", 96, 54, "spin", 0), ("spheres", 96, 54, "grow", 3),
          ("spheres", 96, 54, "scale", None),
          ("dir-light-shadows", 96, 54, "shift", 6), ("dir-light-shadows", 96, 54, "grow", 6),
          ("point-light", 96, 54, "shift", 6), ("point-light", 96, 54, "grow", 6),
          ("room", 32, 18, "spin", 0), ("room", 32, 18, "scale", None),
          ("mirrors", 32, 18, "shift", 1), ("mirrors", 32, 18, "scale", None),
          ("cube", 96, 54, "spin", 0), ("cube", 96, 54, "scale", None)]


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name,W,H,kind,k", MATRIX, ids=[f"{m[0]}-{m[3]}{'' if m[4] is None else m[4]}" for m in MATRIX])
def test_update_render_matches_fresh(gpu, scene_dir, tmp_path, name, W, H, kind, k, accel):
    s = _scene(gpu, scene_dir, tmp_path, name, W, H)
    f = s.frame()
    ctx = gpu.Context(s, accel)
    img0, _ = ctx.render_image(f)
    first, new = _edit(gpu, s, kind, k)
    ctx.set_triangles(new, first)
    assert ctx.geometry_updates() == 1
    img, st = ctx.render_image(f)
    assert not np.array_equal(_bits(img), _bits(img0)), "the edit changes the image"
    _matches_fresh(gpu, ctx, img, st, s, accel, f"{name} {kind} {accel}")


# ---- 2: range against whole, host against device pointer ---------------------
class DevMem:
    def __init__(self, gpu, nbytes):
        self.gpu, self.p = gpu, C.c_void_p()
        gpu._check(gpu.lib().rt_hip_malloc(0, nbytes, C.byref(self.p)), "rt_hip_malloc")

    @property
    def ptr(self):
        return self.p.value

    def upload(self, a):
        a = np.ascontiguousarray(a)
        self.gpu._check(self.gpu.lib().rt_hip_memcpy_h2d(self.p, a.ctypes.data_as(C.c_void_p), a.nbytes), "h2d")
        return self

    def download(self, shape, dtype):
        a = np.empty(shape, dtype)
        self.gpu._check(self.gpu.lib().rt_hip_memcpy_d2h(a.ctypes.data_as(C.c_void_p), self.p, a.nbytes), "d2h")
        return a

    def free(self):
        if self.p:
            self.gpu.lib().rt_hip_free(self.p)
            self.p = None


@pytest.mark.parametrize("accel", ACCELS)
def test_range_equals_whole_and_device_equals_host(gpu, scene_dir, tmp_path, accel):
    s = _scene(gpu, scene_dir, tmp_path, "spheres", 96, 54)
    f = s.frame()
    ctxs = [gpu.Context(s, accel) for _ in range(3)]
    first, new = _edit(gpu, s, "shift", 3)
    assert (first, len(new)) == gpu.object_range(s, 3)
    whole = s.triangles_array()
    assert len(whole) == 4812
    ctxs[0].set_triangles(new, first)           # the object's range, from the host
    ctxs[1].set_triangles(whole)                # all 4812 triangles of the edited scene
    mem = DevMem(gpu, new.nbytes).upload(new)   # the range again, from device memory
    ctxs[2].set_triangles_device(mem.ptr, first, len(new))
    mem.free()
    out = [(c.render_image(f), _info(c)) for c in ctxs]
    for (img, st), info in out[1:]:
        assert np.array_equal(_bits(img), _bits(out[0][0][0]))
        assert st == out[0][0][1] and info == out[0][1]
    _matches_fresh(gpu, ctxs[0], out[0][0][0], out[0][0][1], s, accel, f"range {accel}")


# ---- 3: back again ------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS)
def test_back_again_is_the_golden_image(gpu, scene_dir, tmp_path, manifest, accel):
    s = _scene(gpu, scene_dir, tmp_path, "spheres", 96, 54)
    f = s.frame()
    gold = golden_image(next(c for c in manifest if c["scene"] == "spheres" and (c["width"], c["height"]) == (96, 54)))
    t0 = s.triangles_array()
    ctx = gpu.Context(s, accel)
    info0 = _info(ctx)
    first, new = _edit(gpu, s, "shift", 3)
    ctx.set_triangles(new, first)
    img1, _ = ctx.render_image(f)
    assert not np.array_equal(_bits(img1), _bits(gold))
    ctx.set_triangles(t0[first:first + len(new)], first)
    img, _ = ctx.render_image(f)
    assert np.array_equal(_bits(img), _bits(gold))
    assert ctx.geometry_updates() == 2
    assert _info(ctx) == info0


# ---- 4: animation while streaming ---------------------------------------------
class Stream:
    """rt_hip_render + rt_hip_stats by hand, so that a spurious RT_EHITBUF
    shows (render_image would render again): stats() raises on any code."""

    def __init__(self, gpu, ctx, f):
        self.gpu, self.ctx = gpu, ctx
        self.tiles = DevMem(gpu, 4 * gpu.tile_buffer_floats(f.width, f.height, 1))
        self.rgb = DevMem(gpu, 12 * f.width * f.height)

    def frame(self, f):
        self.ctx.render(f, 0, 1, self.tiles.ptr)
        self.ctx.assemble(f, self.tiles.ptr, 1, self.rgb.ptr)
        st = self.ctx.stats()  # RT_OK, or it raises
        return self.rgb.download((f.height, f.width, 3), np.float32), st

    def free(self):
        self.tiles.free()
        self.rgb.free()


@pytest.mark.parametrize("pan", [False, True], ids=["same-camera", "panned"])
@pytest.mark.parametrize("accel", ACCELS)
def test_animation_while_streaming(gpu, scene_dir, tmp_path, accel, pan):
    # (32x18: every step is checked against a fresh context and the oracle)
    s = _scene(gpu, scene_dir, tmp_path, "spheres", 32, 18)
    t0 = s.triangles_array()
    ext = float(gpu.vertex_extent(t0))
    f = s.frame()
    u = np.array([f.u.x, f.u.y, f.u.z])
    eye = np.array([s.camera.position.x, s.camera.position.y, s.camera.position.z])
    ctx = gpu.Context(s, accel)
    ctx.set_overlap_lists(True)
    run = Stream(gpu, ctx, f)
    run.frame(f)
    run.frame(f)  # (the second frame of a camera builds its lists asynchronously, from the forecast)
    for step in range(1, 5):
        if pan:  # a camera of its own per step: the eye moved along the frame's u
            p = eye + u * (0.01 * ext * step)
            s.camera.position.x, s.camera.position.y, s.camera.position.z = float(p[0]), float(p[1]), float(p[2])
            f = s.frame()
        first, new = _edit(gpu, s, "spin", 0, angle=0.3 * step, base=t0)
        ctx.set_triangles(new, first)
        img, st = run.frame(f)
        img2, st2 = run.frame(f)  # the same frame again: lists from this geometry's forecast
        assert np.array_equal(_bits(img), _bits(img2)) and st == st2
        _matches_fresh(gpu, ctx, img, st, s, accel, f"step {step} {accel}", frame=f)
    assert ctx.geometry_updates() == 4
    run.free()


# ---- 5: kept state ------------------------------------------------------------
def _raises_einval(gpu, call):
    with pytest.raises(gpu.RtError) as e:
        call()
    assert e.value.code == RT_EINVAL
    return str(e.value)


@pytest.mark.parametrize("accel", ACCELS)
def test_kept_frame_is_forgotten_until_the_next_render(gpu, scene_dir, tmp_path, accel):
    s = _scene(gpu, scene_dir, tmp_path, "spheres", 96, 54)
    f = s.frame()
    ctx = gpu.Context(s, accel)
    ctx.set_gbuffer(True)
    run = Stream(gpu, ctx, f)
    gt = DevMem(gpu, 4 * gpu.gbuffer_tile_words(f.width, f.height, 1))
    run.frame(f)
    ctx.relight(f, 0, 1, run.tiles.ptr)  # a kept frame relights and hands out its G-buffer
    ctx.gbuffer(f, 0, 1, gt.ptr)
    ctx.stats()
    first, new = _edit(gpu, s, "shift", 3)
    ctx.set_triangles(new, first)
    _raises_einval(gpu, lambda: ctx.relight(f, 0, 1, run.tiles.ptr))
    _raises_einval(gpu, lambda: ctx.gbuffer(f, 0, 1, gt.ptr))
    gt.free()
    run.free()
    img, smp, st = ctx.render_image_gbuffer(f)
    rel, rst = ctx.relight_image(f)
    fresh = gpu.Context(s, accel)
    fresh.set_gbuffer(True)
    fimg, fsmp, fst = fresh.render_image_gbuffer(f)
    frel, frst = fresh.relight_image(f)
    fresh.close()
    assert np.array_equal(_bits(img), _bits(fimg)) and st == fst
    assert smp.tobytes() == fsmp.tobytes()
    assert np.array_equal(_bits(rel), _bits(frel)) and rst == frst
    assert np.array_equal(_bits(rel), _bits(img))


@pytest.mark.parametrize("accel", ACCELS)
def test_lights_and_materials_persist(gpu, scene_dir, tmp_path, accel):
    s = _scene(gpu, scene_dir, tmp_path, "spheres", 96, 54)
    f = s.frame()
    ctx = gpu.Context(s, accel)
    L = s.lights()
    k = next(i for i, l in enumerate(L) if l.type in (1, 2))
    L[k].v.x, L[k].v.y = L[k].v.x + 0.5, L[k].v.y - 0.25  # one light moved
    L[k].r = L[k].r * 0.5
    o = s.s.objects[0]
    o.kd.x, o.kd.y, o.kd.z = 0.7, o.kd.y * 0.5, 0.2
    o.ns = 17.5
    ctx.set_lights(L)
    ctx.set_materials(s)
    first, new = _edit(gpu, s, "shift", 3)
    ctx.set_triangles(new, first)
    img, st = ctx.render_image(f)
    _matches_fresh(gpu, ctx, img, st, s, accel, f"lights + materials + shift {accel}")


@pytest.mark.parametrize("accel", ACCELS)
def test_empty_update_is_a_no_op(gpu, scene_dir, tmp_path, accel):
    s = _scene(gpu, scene_dir, tmp_path, "spheres", 96, 54)
    f = s.frame()
    ctx = gpu.Context(s, accel)
    img, _ = ctx.render_image(f)
    info = _info(ctx)
    ctx.set_triangles(np.zeros((0, 6, 3), F32), first=7)
    ctx.set_triangles_device(0, 4812, 0)
    assert ctx.geometry_updates() == 0 and _info(ctx) == info
    rel, _ = ctx.relight_image(f)  # the kept frame still relights
    assert np.array_equal(_bits(rel), _bits(img))


# ---- 6: modes -----------------------------------------------------------------
MODES = {
    "exact-reflections": lambda c: c.set_exact_reflections(True),
    "slack-shadows": lambda c: c.set_exact_shadows(False),
    "no-light-buffers": lambda c: c.set_light_buffers(False),
}


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name,W,H,k", [("spheres", 96, 54, 3), ("mirrors", 32, 18, 1)])
def test_modes_survive_an_update(gpu, scene_dir, tmp_path, name, W, H, k, mode, accel):
    s = _scene(gpu, scene_dir, tmp_path, name, W, H)
    f = s.frame()
    ctx = gpu.Context(s, accel)
    MODES[mode](ctx)
    ctx.render_image(f)  # (what the mode builds lazily is built for the old geometry)
    first, new = _edit(gpu, s, "shift", k)
    ctx.set_triangles(new, first)
    img, st = ctx.render_image(f)
    _matches_fresh(gpu, ctx, img, st, s, accel, f"{name} {mode} {accel}", setup=MODES[mode])


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name,W,H,k", [("spheres", 96, 54, 3), ("mirrors", 32, 18, 1)])
def test_gbuffer_and_kept_visibility_after_an_update(gpu, scene_dir, tmp_path, name, W, H, k, accel):
    s = _scene(gpu, scene_dir, tmp_path, name, W, H)
    f = s.frame()
    ctx = gpu.Context(s, accel)
    ctx.set_keep_visibility(True)
    ctx.render_image_gbuffer(f)
    first, new = _edit(gpu, s, "shift", k)
    ctx.set_triangles(new, first)
    img, smp, st = ctx.render_image_gbuffer(f)
    fresh = gpu.Context(s, accel)
    fresh.set_keep_visibility(True)
    fimg, fsmp, fst = fresh.render_image_gbuffer(f)
    fresh.close()
    assert np.array_equal(_bits(img), _bits(fimg)) and st == fst
    assert smp.tobytes() == fsmp.tobytes(), "G-buffer records, prim included"
    assert (smp["prim"] >= 0).any() and smp["prim"].max() < s.triangle_count
    # a colour-only relight of the updated frame asks no query: the masks this
    # render kept are the new geometry's
    L = s.lights()
    j = next(i for i, l in enumerate(L) if l.type in (1, 2))
    L[j].r, L[j].g = L[j].r * 0.5, L[j].g * 0.25
    ctx.set_lights(L)
    rel, rst = ctx.relight_image(f)
    assert rst["shadow"] == 0 and rst["closest"] == st["closest"]
    fresh = gpu.Context(s, accel)  # (the scene's lights are edited now)
    fimg, _ = fresh.render_image(f)
    fresh.close()
    assert np.array_equal(_bits(rel), _bits(fimg)), "the relit frame is a fresh context's render"


# ---- 7: batches ---------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS)
def test_batches_after_an_update(gpu, scene_dir, tmp_path, accel):
    s = _scene(gpu, scene_dir, tmp_path, "spheres", 96, 54)
    ctx = gpu.Context(s, accel)
    ctx.render_image(s.frame())
    first, new = _edit(gpu, s, "shift", 3)
    ctx.set_triangles(new, first)
    fresh = gpu.Context(s, accel)
    tmax = F32(gpu.vertex_extent(s.triangles_array()) / F32(4))
    # the frame's own rays: 96x54 in pixel order (it has no quarter order:
    # 54 is no multiple of 4), and the quarter order of the same camera's
    # 96x52 frame, whose aligned groups of 64 are what a packet walks
    batches = [ctx.frame_rays(s.frame(), "pixel")]
    s.set_size(96, 52)
    batches.append(ctx.frame_rays(s.frame(), "quarter"))
    s.set_size(96, 54)
    for o, d in batches:
        fo, fd = o, d
        for packet in (False, True):
            rgb, smp, st = ctx.trace_rays(o, d, packet=packet, samples=True)
            frgb, fsmp, fst = fresh.trace_rays(fo, fd, packet=packet, samples=True)
            assert np.array_equal(_bits(rgb), _bits(frgb)) and smp.tobytes() == fsmp.tobytes() and st == fst
            occ, ost = ctx.occluded(o, d, tmax=tmax, packet=packet)
            focc, fost = fresh.occluded(fo, fd, tmax=tmax, packet=packet)
            assert np.array_equal(occ, focc) and ost == fost
            # (the eye is further than ext / 4 from most of the scene: unbounded too)
            occ, ost = ctx.occluded(o, d, packet=packet)
            focc, fost = fresh.occluded(fo, fd, packet=packet)
            assert np.array_equal(occ, focc) and ost == fost
            assert 0 < int(occ.sum()) < len(occ)
    fo, fd = fresh.frame_rays(s.frame(), "pixel")
    assert np.array_equal(_bits(fo), _bits(batches[0][0])) and np.array_equal(_bits(fd), _bits(batches[0][1]))
    fresh.close()


# ---- 8: the zero-normal risk flag ---------------------------------------------
def _zn_scene(gpu, tmp_path, two):
    """test_gpu.py::test_zero_normal_is_an_error's triangle with n1 = +z (it
    renders); `two`: a second such triangle beside it in the same object."""
    txt = "camera 32 32 0 0 -5 1 0 0 0 -1 0 60\na_light 1 1 1\n\nobject %d\nKa 1 1 1\n" % (6 if two else 3)
    txt += "v -2 2 0\nv 2 0 0\nv -2 0 0\nvn 0 0 1\nvn 0 0 1\nvn 0 0 1\n"
    if two:
        txt += "v -2 -1 0\nv 2 -3 0\nv -2 -3 0\nvn 0 0 1\nvn 0 0 1\nvn 0 0 1\n"
    sv = tmp_path / "zn.svati"
    sv.write_text(txt)
    return gpu.Scene.load_svati(str(sv))


def _risky(tri, on):
    t = np.array(tri, F32).reshape(1, 6, 3)
    t[0, 4] = (0, 0, -1 if on else 1)  # n1
    return t


def _renders_minus9(gpu, ctx, f):
    with pytest.raises(gpu.RtError) as e:
        ctx.render_image(f)
    assert e.value.code == RT_EZERONORMAL


@pytest.mark.parametrize("accel", ACCELS)
def test_zero_normal_risk_follows_the_normals(gpu, tmp_path, accel):
    s = _zn_scene(gpu, tmp_path, two=False)
    f = s.frame()
    ctx = gpu.Context(s, accel)
    t = s.triangles_array()
    assert np.array_equal(t[0, :3], np.array([[-2, 0, 0], [2, 0, 0], [-2, 2, 0]], F32))  # (LIFO order)
    img0, _ = ctx.render_image(f)
    ctx.set_triangles(_risky(t[0], True))
    _renders_minus9(gpu, ctx, f)
    ctx.set_triangles(_risky(t[0], False))
    img, st = ctx.render_image(f)
    assert np.array_equal(_bits(img), _bits(img0))
    _matches_fresh(gpu, ctx, img, st, s, accel, f"risk cleared {accel}")


@pytest.mark.parametrize("accel", ACCELS)
def test_zero_normal_risk_is_per_object(gpu, tmp_path, accel):
    """An object of two triangles, A risky and B clean: the flag depends on
    triangles outside the updated range."""
    s = _zn_scene(gpu, tmp_path, two=True)
    f = s.frame()
    t = s.triangles_array()
    assert len(t) == 2
    a = int(np.argmax(t[:, :3, 1].max(axis=1)))  # A: the triangle the zero line x = 0 crosses in view (y in [0, 2])
    b = 1 - a
    ctx = gpu.Context(s, accel)
    img0, _ = ctx.render_image(f)
    ctx.set_triangles(_risky(t[a], True), first=a)
    _renders_minus9(gpu, ctx, f)
    ctx.set_triangles(t[b:b + 1], first=b)  # only B's range, B clean: A keeps the object flagged
    _renders_minus9(gpu, ctx, f)
    ctx.set_triangles(_risky(t[a], False), first=a)  # A clean: every triangle of the object is
    img, st = ctx.render_image(f)
    assert np.array_equal(_bits(img), _bits(img0))
    _matches_fresh(gpu, ctx, img, st, s, accel, f"object risk cleared {accel}")


def _render_code(gpu, ctx, f):
    """rt_hip_render_image's return code and counters (filled whatever the code)."""
    img = np.empty((f.height, f.width, 3), F32)
    st = gpu.Stats()
    rc = gpu.lib().rt_hip_render_image(ctx.h, C.byref(f), img.ctypes.data_as(C.c_void_p), C.byref(st))
    return rc, st.as_dict(), img


@pytest.mark.parametrize("order", ["A-first", "B-first"])
def test_risk_flag_is_stamped_outside_the_updated_range(gpu, tmp_path, order):
    """The record flag itself (float 11), which only shadow rays read: object
    0 holds A, far outside every ray's reach, and B, which shadows a floor
    (object 1) from a point light.  No closest hit ever lands on A, so
    zero_normal stays 0; shadow_zero_risk counts the shadow rays that end on
    B exactly while A makes the object risky -- B's record is outside the
    updated range."""
    a_tri = "v 98 2 0\nv 102 0 0\nv 98 0 0\nvn 0 0 1\nvn 0 0 1\nvn 0 0 1\n"
    b_tri = "v -1 1 0\nv 1 -1 0\nv -1 -1 0\nvn 0 0 -1\nvn 0 0 -1\nvn 0 0 -1\n"
    floor = "v -4 4 2\nv 4 -4 2\nv -4 -4 2\nvn 0 0 -1\nvn 0 0 -1\nvn 0 0 -1\n" \
            "v 4 4 2\nv 4 -4 2\nv -4 4 2\nvn 0 0 -1\nvn 0 0 -1\nvn 0 0 -1\n"
    # (the parser stacks triangles LIFO: the last one written is prim 0 of its object)
    first_two = (b_tri + a_tri) if order == "A-first" else (a_tri + b_tri)
    sv = tmp_path / "flag.svati"
    sv.write_text("camera 32 32 0 0 -5 1 0 0 0 -1 0 60\na_light 0.2 0.2 0.2\np_light 1 1 1 0 0 -5\n\n"
                  "object 6\nKa 1 1 1\nKd 1 1 1\n" + first_two + "\nobject 6\nKa 1 1 1\nKd 1 1 1\n" + floor)
    s = gpu.Scene.load_svati(str(sv))
    f = s.frame()
    t = s.triangles_array()
    assert len(t) == 4 and gpu.object_range(s, 0) == (0, 2)
    a = int(np.argmax(t[:2, :3, 0].max(axis=1)))  # A: the one at x ~ 100
    assert (a == 0) == (order == "A-first")
    b = 1 - a
    ctx = gpu.Context(s, "octree_gpu")
    rc, st, img0 = _render_code(gpu, ctx, f)
    assert rc == 0 and st["shadow"] > 0 and st["shadow_zero_risk"] == 0 and st["zero_normal"] == 0
    ctx.set_triangles(_risky(t[a], True), first=a)
    rc, st, _ = _render_code(gpu, ctx, f)
    assert rc == RT_EZERONORMAL and st["zero_normal"] == 0 and st["shadow_zero_risk"] > 0
    risk = st["shadow_zero_risk"]
    ctx.set_triangles(t[b:b + 1], first=b)  # B alone, clean as ever: A keeps the flag on B's record
    rc, st, _ = _render_code(gpu, ctx, f)
    assert rc == RT_EZERONORMAL and st["zero_normal"] == 0 and st["shadow_zero_risk"] == risk
    s.set_triangles_array(_risky(t[a], True), a)  # a fresh context on the risky scene counts the same
    rc, fst, _ = _render_code(gpu, gpu.Context(s, "octree_gpu"), f)
    assert rc == RT_EZERONORMAL and fst == st
    s.set_triangles_array(t[a:a + 1], a)
    ctx.set_triangles(t[a:a + 1], first=a)
    rc, st, img = _render_code(gpu, ctx, f)
    assert rc == 0 and st["shadow_zero_risk"] == 0 and np.array_equal(_bits(img), _bits(img0))
    _matches_fresh(gpu, ctx, img, st, s, "octree_gpu", f"flag cleared {order}")


# ---- 9: errors ----------------------------------------------------------------
def test_refusals_change_nothing(gpu, scene_dir, tmp_path, manifest):
    s = _scene(gpu, scene_dir, tmp_path, "spheres", 96, 54)
    f = s.frame()
    gold = golden_image(next(c for c in manifest if c["scene"] == "spheres" and (c["width"], c["height"]) == (96, 54)))
    t = s.triangles_array()
    moved = gpu.shift_triangles(t, np.array([1, 2, 3], F32))
    host_tree = gpu.Context(s, "octree")
    msg = _raises_einval(gpu, lambda: host_tree.set_triangles(moved))
    assert "host" in msg
    _raises_einval(gpu, lambda: host_tree.set_triangles(moved[:0]))  # (a host tree refuses whatever the range)
    img, _ = host_tree.render_image(f)
    assert np.array_equal(_bits(img), _bits(gold)) and host_tree.geometry_updates() == 0
    for accel in ACCELS:
        ctx = gpu.Context(s, accel)
        info = _info(ctx)
        _raises_einval(gpu, lambda: ctx.set_triangles(moved[:10], first=4803))   # past the end
        _raises_einval(gpu, lambda: ctx.set_triangles(moved[:1], first=4812))
        _raises_einval(gpu, lambda: ctx.set_triangles_device(0, 0, 4812))         # NULL with count > 0
        with pytest.raises(gpu.RtError):
            gpu._check(gpu.lib().rt_hip_set_triangles(None, None, 0, 0), "null context")
        assert ctx.geometry_updates() == 0 and _info(ctx) == info
        img, _ = ctx.render_image(f)
        assert np.array_equal(_bits(img), _bits(gold)), accel
