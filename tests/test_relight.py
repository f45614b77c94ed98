"""Relighting on the GPU (include/rt_hip.h rt_hip_set_lights, rt_hip_set_materials,
rt_hip_set_keep_visibility, rt_hip_relight): the last render's kept hit
records shaded again under edited lights and materials.  Every relit image is
checked two ways: bit for bit against render_image of a fresh context created
on the edited scene, and by test_gpu.py's assert_bitexact rule (0 ULP) against
the oracle's render of the same edited rt_scene.  The shadow-query counts say
which path ran: none for a colour or material edit, one light's for a moved
light, the lights past the 32nd always.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from conftest import golden_image, load_manifest_static, load_own_manifest, own_golden_image, own_scene_path

pytestmark = pytest.mark.gpu
CASES = load_manifest_static()
OWN_CASES = load_own_manifest()
RT_EINVAL = -1
ACCELS = ["flat", "octree", "octree_gpu"]


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


def _load(gpu, scene_dir, name, W, H):
    s = gpu.Scene.load_svati(os.path.join(scene_dir, name + ".svati"))
    s.set_size(W, H)
    return s


def _mirrors(gpu, tmp_path):
    case = next(c for c in OWN_CASES if (c["width"], c["height"]) == (32, 18))
    return gpu.Scene.load_svati(own_scene_path(case, tmp_path)), case


def _casting(s):
    return sum(1 for l in s.lights() if l.type in (1, 2))


@contextlib.contextmanager
def _light_table(gpu, s, rows):
    """The scene with another light array (any length) for the block: the
    scene's own array is the library's, so it is swapped out and put back."""
    arr = (gpu.Light * len(rows))()
    for l, (t, r, g, b, x, y, z) in zip(arr, rows):
        l.type, l.r, l.g, l.b = int(t), r, g, b
        l.v.x, l.v.y, l.v.z = x, y, z
    # (the address, not the field: a ctypes pointer read from a structure is a
    # view of the field and would follow the swap)
    old_addr, old_n = C.cast(s.s.lights, C.c_void_p).value, int(s.s.light_count)
    s.s.lights = C.cast(arr, C.POINTER(gpu.Light))
    s.s.light_count = len(rows)
    try:
        yield arr
    finally:
        s.s.lights = C.cast(C.c_void_p(old_addr), C.POINTER(gpu.Light))
        s.s.light_count = old_n
        assert C.cast(s.s.lights, C.c_void_p).value == old_addr


def _rows(s):
    return [(l.type, l.r, l.g, l.b, l.v.x, l.v.y, l.v.z) for l in s.lights()]


def _fresh(gpu, s, accel, setup=None):
    ctx = gpu.Context(s, accel)
    if setup:
        setup(ctx)
    img, st = ctx.render_image(s.frame())
    ctx.close()
    return img, st


def _check(gpu, img, s, accel, what, setup=None, oracle=True):
    """img == a fresh context's render of the scene as it stands, bit for
    bit, and == the oracle's by assert_bitexact; returns the fresh stats."""
    fresh, fst = _fresh(gpu, s, accel, setup)
    assert np.array_equal(_bits(img), _bits(fresh)), \
        f"{what}: {int((_bits(img) != _bits(fresh)).sum())} channels differ from a fresh context's render"
    if oracle:
        import oracle as orc
        f = s.frame()
        ref, _ = orc.render(s.ptr, f.width, f.height, threads=4)
        assert_bitexact(img, ref, what + " vs oracle")
    return fst


def _edit_colours_and_materials(s):
    L = s.lights()
    k = next(i for i, l in enumerate(L) if l.type in (1, 2))
    L[k].r, L[k].g, L[k].b = L[k].r * 0.5, L[k].g * 0.5, L[k].b * 0.5
    a = next(i for i, l in enumerate(L) if l.type == 0)
    L[a].r, L[a].g, L[a].b = 0.4, 0.1, 0.25
    o = s.s.objects[0]
    o.kd.x, o.kd.y, o.kd.z = 0.7, o.kd.y * 0.5, 0.2
    o.ks.x, o.ks.y, o.ks.z = 0.3, 0.9, o.ks.z * 0.25
    o.ns = 17.5
    o.ka.x, o.ka.y, o.ka.z = 0.2, 0.6, 0.1


# ---- 1: colour-only and materials ----
@pytest.mark.parametrize("accel", ACCELS)
def test_colour_and_material_edits_ask_no_query(gpu, scene_dir, accel):
    s = _load(gpu, scene_dir, "spheres", 96, 54)
    f = s.frame()
    ncast = _casting(s)
    # keep-visibility on: the first relight already skips every query
    ctx = gpu.Context(s, accel)
    ctx.set_keep_visibility(True)
    img0, st0 = ctx.render_image(f)
    assert st0["shadow"] == st0["hit_records"] * ncast
    # keep-visibility off (the default): the first relight asks every query
    cold = gpu.Context(s, accel)
    cold.render_image(f)
    _edit_colours_and_materials(s)
    for c in (ctx, cold):
        c.set_lights(s.lights())
        c.set_materials(s)
    img, st = ctx.relight_image(f)
    fst = _check(gpu, img, s, accel, f"spheres/{accel} colours + materials, keep-visibility")
    assert not np.array_equal(_bits(img), _bits(img0))  # the edit is no no-op
    assert st["shadow"] == 0
    assert st["hit_records"] == st0["hit_records"] == fst["hit_records"]
    assert st["closest"] == st0["closest"] == fst["closest"]
    img, st = cold.relight_image(f)
    assert np.array_equal(_bits(img), _bits(_fresh(gpu, s, accel)[0]))
    assert st["shadow"] == fst["shadow"] == fst["hit_records"] * ncast
    L = s.lights()
    L[2].r, L[2].g, L[2].b = 0.1, 0.9, 0.5
    cold.set_lights(L)
    img, st = cold.relight_image(f)
    _check(gpu, img, s, accel, f"spheres/{accel} second colour edit")
    assert st["shadow"] == 0
    ctx.close()
    cold.close()


# ---- 2: one light moved ----
@pytest.mark.parametrize("accel", ACCELS)
def test_one_light_moved_asks_that_lights_queries(gpu, scene_dir, accel):
    s = _load(gpu, scene_dir, "spheres", 96, 54)
    f = s.frame()
    ctx = gpu.Context(s, accel)
    ctx.set_keep_visibility(True)
    img0, _ = ctx.render_image(f)
    s.lights()[5].v.x += 0.75
    ctx.set_lights(s.lights())
    img, st = ctx.relight_image(f)
    fst = _check(gpu, img, s, accel, f"spheres/{accel} light 5 moved")
    assert not np.array_equal(_bits(img), _bits(img0))
    assert fst["shadow"] == fst["hit_records"] * _casting(s)
    assert st["shadow"] == st["hit_records"] * 1
    assert st["hit_records"] == fst["hit_records"]
    ctx.close()


# ---- 3: table shape ----
@pytest.mark.parametrize("scene,accel", [("spheres", "octree"), ("cube", "octree_gpu"), ("point-light", "flat")])
def test_table_shape_edits(gpu, scene_dir, scene, accel):
    s = _load(gpu, scene_dir, scene, 96, 54)
    f = s.frame()
    ctx = gpu.Context(s, accel)
    ctx.set_keep_visibility(True)
    ctx.render_image(f)
    base = _rows(s)
    appended = base + [(2, 0.3, 0.2, 0.5, 1.0, 3.0, -2.0)]
    removed = appended[:2] + appended[3:] if len(appended) > 3 else appended[:1] + appended[2:]
    d = next((i for i, r in enumerate(removed) if r[0] == 1), None)
    turned = list(removed)
    if d is not None:  # the directional light becomes a point light at its vector
        turned[d] = (2,) + tuple(removed[d][1:])
    else:              # no directional light in this scene: a point light becomes directional
        p = next(i for i, r in enumerate(removed) if r[0] == 2)
        turned[p] = (1,) + tuple(removed[p][1:])
    for what, rows in (("append", appended), ("remove", removed), ("type change", turned), ("n = 0", []),
                       ("back", base)):
        with _light_table(gpu, s, rows) as arr:
            ctx.set_lights(arr)
            img, st = ctx.relight_image(f)
            _check(gpu, img, s, accel, f"{scene}/{accel} {what}")
            if not rows:
                assert st["shadow"] == 0
    ctx.close()


# ---- 4, 5: more than 32 lights ----
def _extended(s, kind):
    base = _rows(s)
    pts = [r for r in base if r[0] == 2]
    extra = []
    for k in range(34 - len(base)):
        t, r, g, b, x, y, z = pts[k % len(pts)]
        extra.append((kind, 0.03, 0.02, 0.04, x + 0.37 * (k + 1), y + 0.11 * k, z - 0.23 * (k + 1)))
    return base + extra


def test_34_lights_query_the_ones_past_the_32nd(gpu, scene_dir):
    s = _load(gpu, scene_dir, "spheres", 32, 18)
    f = s.frame()
    rows = _extended(s, 2)
    assert len(rows) == 34 and rows[32][0] == 2 and rows[33][0] == 2
    with _light_table(gpu, s, rows) as arr:
        ctx = gpu.Context(s, "octree")
        ctx.set_keep_visibility(True)
        _, st0 = ctx.render_image(f)
        assert st0["shadow"] == st0["hit_records"] * 33
        arr[1].r, arr[1].g, arr[1].b = 0.2, 0.5, 0.1
        ctx.set_lights(arr)
        img, st = ctx.relight_image(f)
        _check(gpu, img, s, "octree", "spheres 34 point lights, colour edit")
        assert st["shadow"] == st["hit_records"] * 2
        ctx.close()


def test_34_lights_extras_ambient_ask_no_query(gpu, scene_dir):
    s = _load(gpu, scene_dir, "spheres", 32, 18)
    f = s.frame()
    with _light_table(gpu, s, _extended(s, 0)) as arr:
        ctx = gpu.Context(s, "octree")
        ctx.set_keep_visibility(True)
        ctx.render_image(f)
        arr[1].r, arr[33].g = 0.2, 0.5
        ctx.set_lights(arr)
        img, st = ctx.relight_image(f)
        _check(gpu, img, s, "octree", "spheres 34 lights, extras ambient, colour edit")
        assert st["shadow"] == 0
        ctx.close()


# ---- 6: nr changed ----
def test_changed_reflectivity_is_refused(gpu, tmp_path):
    s, case = _mirrors(gpu, tmp_path)
    f = s.frame()
    ctx = gpu.Context(s, "octree")
    img0, _ = ctx.render_image(f)
    k = next(i for i in range(s.s.object_count) if s.s.objects[i].nr > 0.0)
    was = s.s.objects[k].nr
    s.s.objects[k].nr = was * 0.5
    s.s.objects[k].kd.x = 0.9
    with pytest.raises(gpu.RtError) as e:
        ctx.set_materials(s)
    assert e.value.code == RT_EINVAL
    img, _ = ctx.relight_image(f)  # nothing changed: not kd either
    assert np.array_equal(_bits(img), _bits(img0))
    assert np.array_equal(_bits(img), _bits(own_golden_image(case)))
    ctx.close()


# ---- 7: stale and revisited frames ----
def test_stale_and_revisited_frames(gpu, scene_dir):
    s = _load(gpu, scene_dir, "spheres", 96, 54)
    fa = s.frame()
    ctx = gpu.Context(s, "octree")
    ctx.render_image(fa)
    L = s.lights()
    L[3].r = 0.2
    ctx.set_lights(L)
    img, _ = ctx.relight_image(fa)
    _check(gpu, img, s, "octree", "frame A relit")
    s.s.camera.position.x += 0.5  # a panned view
    fb = s.frame()
    ctx.render_image(fb)
    with pytest.raises(gpu.RtError) as e:
        ctx.relight_image(fa)
    assert e.value.code == RT_EINVAL
    L[4].v.y += 0.5
    ctx.set_lights(L)
    img, _ = ctx.relight_image(fb)
    _check(gpu, img, s, "octree", "frame B relit")
    s.s.camera.position.x -= 0.5
    assert bytes(s.frame()) == bytes(fa)
    ctx.render_image(fa)
    L[4].v.y -= 0.25
    ctx.set_lights(L)
    img, _ = ctx.relight_image(fa)
    _check(gpu, img, s, "octree", "frame A rendered again and relit")
    ctx.close()


# ---- 8: invalidation ----
@pytest.mark.parametrize("setting", ["exact_shadows_off", "cull_slack"])
def test_settings_make_the_stored_decisions_stale(gpu, scene_dir, setting):
    s = _load(gpu, scene_dir, "point-light", 96, 54)
    f = s.frame()
    ctx = gpu.Context(s, "octree")
    ctx.set_keep_visibility(True)
    ctx.render_image(f)
    _, st = ctx.relight_image(f)
    assert st["shadow"] == 0  # every decision is current
    setup = (lambda c: c.set_exact_shadows(False)) if setting == "exact_shadows_off" else \
        (lambda c: c.set_cull_slack(128.0))
    setup(ctx)
    img, st = ctx.relight_image(f)
    fst = _check(gpu, img, s, "octree", f"point-light after {setting}", setup=setup)
    assert st["shadow"] == st["hit_records"] * _casting(s) == fst["shadow"]
    _, st = ctx.relight_image(f)
    assert st["shadow"] == 0
    ctx.close()


# ---- 9: ranks on one GPU ----
@pytest.mark.parametrize("W,H,nranks", [(100, 52, 3), (96, 54, 8)])
def test_ranks_relight_their_own_tiles(gpu, scene_dir, W, H, nranks):
    s = _load(gpu, scene_dir, "spheres", W, H)
    f = s.frame()
    L = gpu.lib()
    per = gpu.tile_buffer_floats(W, H, nranks)
    if nranks == 8:  # 96x54 in 32x32 blocks: 3 x 2 blocks on the diagonals 0..3, so ranks 4..7 have no tiles
        assert [gpu.rank_tile_count(W, H, r, nranks) == 0 for r in range(nranks)] == [False] * 4 + [True] * 4
    d, d_rgb = C.c_void_p(), C.c_void_p()
    assert L.rt_hip_malloc(0, per * nranks * 4, C.byref(d)) == 0
    assert L.rt_hip_malloc(0, W * H * 3 * 4, C.byref(d_rgb)) == 0
    zeros = np.zeros(per * nranks, np.float32)
    ctxs = [gpu.Context(s, "octree") for _ in range(nranks)]
    try:
        assert L.rt_hip_memcpy_h2d(d, zeros.ctypes.data_as(C.c_void_p), zeros.nbytes) == 0
        for r, c in enumerate(ctxs):
            c.render(f, r, nranks, d.value + 4 * per * r)
            c.stats()
        s.lights()[5].v.x += 0.75
        s.lights()[2].g = 0.3
        assert L.rt_hip_memcpy_h2d(d, zeros.ctypes.data_as(C.c_void_p), zeros.nbytes) == 0
        for r, c in enumerate(ctxs):
            c.set_lights(s.lights())
            c.relight(f, r, nranks, d.value + 4 * per * r)
            st = c.stats()
            assert st["shadow"] == st["hit_records"] * _casting(s)  # keep-visibility off: the first relight
        ctxs[0].assemble(f, d.value, nranks, d_rgb.value)
        ctxs[0].stats()
        img = np.empty((H, W, 3), np.float32)
        assert L.rt_hip_memcpy_d2h(img.ctypes.data_as(C.c_void_p), d_rgb, img.nbytes) == 0
        _check(gpu, img, s, "octree", f"spheres {W}x{H} over {nranks} ranks")
    finally:
        for c in ctxs:
            c.close()
        L.rt_hip_free(d)
        L.rt_hip_free(d_rgb)


# ---- 10, 11: idempotence, G-buffer ----
def test_relight_twice_and_gbuffer_untouched(gpu, scene_dir):
    s = _load(gpu, scene_dir, "cube", 96, 54)
    f = s.frame()
    L = gpu.lib()
    n = gpu.tile_buffer_floats(96, 54, 1)
    gw = gpu.gbuffer_tile_words(96, 54, 1)
    dt, dg = C.c_void_p(), C.c_void_p()
    assert L.rt_hip_malloc(0, n * 4, C.byref(dt)) == 0
    assert L.rt_hip_malloc(0, gw * 4, C.byref(dg)) == 0
    ctx = gpu.Context(s, "octree_gpu")
    ctx.set_gbuffer(True)

    def tiles():
        ctx.stats()
        out = np.empty(n, np.float32)
        assert L.rt_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), dt, out.nbytes) == 0
        return out

    def gbuf():
        ctx.gbuffer(f, 0, 1, dg.value)
        ctx.stats()
        out = np.empty(gw, np.uint32)
        assert L.rt_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), dg, out.nbytes) == 0
        return out

    try:
        ctx.render(f, 0, 1, dt.value)
        t0, g0 = tiles(), gbuf()
        s.lights()[1].v.x = -0.5
        s.lights()[0].r = 0.1
        ctx.set_lights(s.lights())
        ctx.relight(f, 0, 1, dt.value)
        t1, g1 = tiles(), gbuf()
        ctx.relight(f, 0, 1, dt.value)
        t2, g2 = tiles(), gbuf()
        assert not np.array_equal(_bits(t0), _bits(t1))
        assert np.array_equal(_bits(t1), _bits(t2))
        assert np.array_equal(g0, g1) and np.array_equal(g0, g2)
        fresh, _ = _fresh(gpu, s, "octree_gpu")
        assert np.array_equal(_bits(gpu.assemble_tiles_numpy(t1, 96, 54, 1)), _bits(fresh))
    finally:
        ctx.close()
        L.rt_hip_free(dt)
        L.rt_hip_free(dg)


# ---- 12: the default render untouched ----
@pytest.mark.parametrize("accel", ACCELS)
def test_keep_visibility_renders_the_golden(gpu, scene_dir, tmp_path, accel):
    case = next(c for c in CASES if (c["scene"], c["width"], c["height"]) == ("cube", 96, 54))
    s = _load(gpu, scene_dir, "cube", 96, 54)
    ctx = gpu.Context(s, accel)
    ctx.set_keep_visibility(True)
    img, st = ctx.render_image(s.frame())
    assert np.array_equal(_bits(img), _bits(golden_image(case)))
    assert st["closest"] == case["closest"] and st["shadow"] == case["shadow"]
    ctx.close()
    s, case = _mirrors(gpu, tmp_path)
    ctx = gpu.Context(s, accel)
    ctx.set_keep_visibility(True)
    img, st = ctx.render_image(s.frame())
    assert np.array_equal(_bits(img), _bits(own_golden_image(case)))
    assert st["closest"] == case["closest"] and st["shadow"] == case["shadow"]
    ctx.close()


# ---- 13: refusals ----
def test_refusals(gpu, scene_dir):
    s = _load(gpu, scene_dir, "cube", 96, 54)
    f = s.frame()
    L = gpu.lib()
    # the HIP runtime the product library brought into this process, by the path it is mapped from
    with open("/proc/self/maps") as maps:
        hip = C.CDLL(next(l.split()[-1] for l in maps if "libamdhip64.so" in l))
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    dt = C.c_void_p()
    assert L.rt_hip_malloc(0, gpu.tile_buffer_floats(96, 54, 1) * 4, C.byref(dt)) == 0
    ctx = gpu.Context(s, "octree")

    def refused(stream=None):
        with pytest.raises(gpu.RtError) as e:
            ctx.relight(f, 0, 1, dt.value, stream)
        assert e.value.code == RT_EINVAL

    try:
        refused()  # before any render
        ctx.render(f, 0, 1, dt.value)
        ctx.stats()
        other = C.c_void_p()
        assert hip.hipStreamCreate(C.byref(other)) == 0 and other.value
        try:
            refused(other.value)  # another stream
        finally:
            assert hip.hipStreamDestroy(other) == 0
        with pytest.raises(gpu.RtError) as e:
            ctx.relight(f, 1, 2, dt.value)  # another rank split
        assert e.value.code == RT_EINVAL
        ctx.set_policy(1)
        refused()
        ctx.set_policy(0)
        ctx.set_count_work(True)
        refused()
        ctx.set_count_work(False)
        ctx.relight(f, 0, 1, dt.value)  # none of the refusals changed anything
        ctx.stats()
        ctx.render_compat(s.camera)
        refused()  # the compatibility mode keeps no records
        objs = (gpu.Object * (s.s.object_count + 1))()
        with pytest.raises(gpu.RtError) as e:
            ctx.set_materials(objs)
        assert e.value.code == RT_EINVAL
    finally:
        ctx.close()
        L.rt_hip_free(dt)
