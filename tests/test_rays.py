"""Ray batches on the GPU (include/rt_hip.h rt_hip_trace_rays,
rt_hip_trace_rays_host, rt_hip_frame_rays; kernels csrc/rt_rays.h): a caller's
rays traced as the reference's trace(ray, 1.0), one colour and one hit record
per ray.

A frame's own camera rays through the ray API give the golden images and the
manifest's query counts (proven walks and brute force), the G-buffer's records
and, through the default slack walk, nothing the grazing class does not
explain; rays no pinhole makes agree between the proven octree walk and brute
force bit for bit; a ray cast answers what the closest-hit probe answers; the
packet flag changes no bit; the item scheme's edges, the hit buffers' growth
and the frames around a batch hold.  Shapes are the goldens' (96x54, 32x18)
and the smallest batches that cross an item, a stream or a grid boundary."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import (REPO, golden_image, load_manifest_static, load_own_manifest, own_golden_image,
                      own_scene_path)

pytestmark = pytest.mark.gpu

RT_EINVAL, RT_EHITBUF, RT_EINEXACT = -1, -10, -11
CASES = {f'{c["scene"]}_{c["width"]}x{c["height"]}': c for c in load_manifest_static()}
OWN = {f'{c["scene"]}_{c["width"]}x{c["height"]}': c for c in load_own_manifest()}
GOLDENS = ["cube_96x54", "spheres_96x54", "island_smooth_96x54", "car-on-road_96x54", "point-light_96x54",
           "dir-light-shadows_96x54", "mirrors_32x18"]
# (accel, exact reflections): brute force, and both octrees' proven walks
PROVEN = [("flat", False), ("octree", True), ("octree_gpu", True)]


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


def _load(gpu, scene_dir, tmp_path, name):
    """(scene at the case's size, case, golden image) of a reference or own golden."""
    if name in OWN:
        case = OWN[name]
        s = gpu.Scene.load_svati(own_scene_path(case, tmp_path))
        gold = own_golden_image(case)
    else:
        case = CASES[name]
        s = gpu.Scene.load_svati(os.path.join(scene_dir, case["scene"] + ".svati"))
        gold = golden_image(case)
    s.set_size(case["width"], case["height"])
    return s, case, gold


def _ctx(gpu, s, accel, exact=False):
    ctx = gpu.Context(s, accel)
    if exact:
        ctx.set_exact_reflections(True)
    return ctx


def _same(a, b):
    """Byte for byte (colours as float32, samples as GSAMPLE records)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _diff_rays(rgb_a, smp_a, rgb_b, smp_b):
    d = np.zeros(len(rgb_a), bool)
    d |= (rgb_a.view(np.uint32) != rgb_b.view(np.uint32)).any(axis=1)
    d |= (smp_a.view(np.uint32).reshape(len(smp_a), -1) != smp_b.view(np.uint32).reshape(len(smp_b), -1)).any(axis=1)
    return np.flatnonzero(d)


class Dev:
    """Device buffers through the C ABI's helpers, freed on close."""

    def __init__(self, gpu):
        self.L, self.bufs = gpu.lib(), []

    def malloc(self, nbytes):
        d = C.c_void_p()
        assert self.L.rt_hip_malloc(0, max(int(nbytes), 16), C.byref(d)) == 0
        self.bufs.append(d)
        return d.value

    def upload(self, a):
        a = np.ascontiguousarray(a)
        d = self.malloc(a.nbytes)
        assert self.L.rt_hip_memcpy_h2d(C.c_void_p(d), a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
        return d

    def host(self, d, shape, dtype):
        """(call after something that waits for the stream, e.g. stats())"""
        out = np.empty(shape, dtype)
        assert self.L.rt_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(d), out.nbytes) == 0
        return out

    def close(self):
        for d in self.bufs:
            self.L.rt_hip_free(d)
        self.bufs = []


# ---- 1, 2: a frame's rays give the frame ------------------------------------
@pytest.mark.parametrize("accel,exact", PROVEN, ids=[a for a, _ in PROVEN])
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_through_the_ray_api(gpu, scene_dir, tmp_path, name, accel, exact):
    """frame_rays -> trace_rays -> fold_samples is the golden image bit for bit,
    with the manifest's query counts, on brute force and both proven walks; the
    device generator equals camera_rays; the samples are the frame's G-buffer."""
    s, case, gold = _load(gpu, scene_dir, tmp_path, name)
    f = s.frame()
    ctx = _ctx(gpu, s, accel, exact)
    o, d = ctx.frame_rays(f, "pixel")
    ho, hd = gpu.camera_rays(f, "pixel")
    assert _same(o, ho) and _same(d, hd), "device generator vs camera_rays"
    rgb, smp, st = ctx.trace_rays(o, d, samples=True)
    img = gpu.fold_samples(rgb).reshape(gold.shape)
    bad = np.argwhere((img.view(np.uint32) != gold.view(np.uint32)).any(axis=2))
    assert len(bad) == 0, f"{len(bad)} pixels differ from the golden image, first {bad[:4].tolist()}"
    assert (st["closest"], st["shadow"]) == (case["closest"], case["shadow"])
    assert st["closest_unproven"] == 0 and st["depth_overflow"] == 0
    assert st["camera"] == len(o) and st["pixels"] == 0
    assert (st["cand_prims"], st["cand_entries"], st["cand_global"]) == (0, 0, 0)
    assert int(smp["queries"].sum()) == case["closest"]
    # the G-buffer of the same frame (rendered without exact reflections: the
    # capture refuses them), byte for byte
    _, gsmp, _ = gpu.Context(s, accel).render_image_gbuffer(f)
    assert _same(smp, gsmp.reshape(-1)), "ray samples vs the frame's G-buffer"
    # quarter order: the same rays permuted (96x54 has no quarter order)
    if f.width % 4 == 0 and f.height % 4 == 0:
        oq, dq = ctx.frame_rays(f, "quarter")
        perm, _ = gpu.quarter_order(f.width, f.height)
        assert _same(oq, o[perm]) and _same(dq, d[perm])


# ---- 3: the default (slack) walk ---------------------------------------------
def _first_difference_explained(gpu, walk, flat, tri, nr, o, d):
    """Follows one ray's path query by query with ray casts on both contexts;
    at the first query whose answers differ: is the ray the coplanar-grazing
    class on brute force's winner (tools/grazing.py)?"""
    from grazing import coplanar_grazing
    f32 = np.float32
    o, d, coef = np.asarray(o, f32), np.asarray(d, f32), f32(1.0)
    for _ in range(256):
        if float(coef) < 0.01:
            return False  # the paths agree to their end: the difference is not a query's
        _, sw, _ = walk.trace_rays(o[None], d[None], shade=False)
        _, sf, _ = flat.trace_rays(o[None], d[None], shade=False)
        if not _same(sw, sf):
            return sf["prim"][0] >= 0 and bool(coplanar_grazing(tri[sf["prim"][0]], o, d))
        n = sf["N"][0]
        if sf["prim"][0] < 0 or not n.any():
            return False
        k = f32(2) * (f32(f32(n[0] * d[0]) + f32(n[1] * d[1])) + f32(n[2] * d[2]))  # cpu/ray.c:16-25
        d = np.array([f32(d[a] - f32(n[a] * k)) for a in range(3)], f32)
        o = sf["P"][0].copy()
        coef = f32(nr[sf["obj"][0]] * coef)
    return False


@pytest.mark.parametrize("accel", ["octree", "octree_gpu"])
def test_default_walk_against_brute_force(gpu, scene_dir, tmp_path, accel):
    """The goldens' rays through the default slack walk (tested, not proven)
    against brute force on the same rays: every ray whose colour or sample
    differs is explained by the coplanar-grazing class at its first differing
    query.  A measurement of the walk's residual class; none unexplained."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    total = differ = 0
    for name in GOLDENS:
        s, case, _ = _load(gpu, scene_dir, tmp_path, name)
        o, d = gpu.camera_rays(s.frame(), "pixel")
        walk, flat = _ctx(gpu, s, accel), _ctx(gpu, s, "flat")
        rw, sw, stw = walk.trace_rays(o, d, samples=True)
        rf, sf, _ = flat.trace_rays(o, d, samples=True)
        assert stw["closest_unproven"] == 0
        bad = _diff_rays(rw, sw, rf, sf)
        total += len(o)
        differ += len(bad)
        if len(bad):
            tri, nr = s.triangles_array(), gpu.scene_materials(s.ptr)[:, 11]
            unexplained = [int(i) for i in bad[:64]
                           if not _first_difference_explained(gpu, walk, flat, tri, nr, o[i], d[i])]
            assert not unexplained and len(bad) <= 64, (name, len(bad), unexplained[:5])
    print(f"{accel} slack walk: {total} golden camera rays as a batch, {differ} differ from brute force, "
          f"all coplanar-grazing")


# ---- 4: rays no pinhole makes -------------------------------------------------
def _odd_rays(gpu, s, ctx):
    """A 128x64 panorama from the eye, a 64x64 orthographic view of the scene
    box along its diagonal and 4,096 seeded rays from inside and far outside the scene box with
    directions of length 0.25 .. 1.0625."""
    info = ctx.info()
    c, r = np.array(info["scene_center"], np.float64), float(info["scene_radius"])
    cam = s.camera
    eye = (cam.position.x, cam.position.y, cam.position.z)
    # the view looks along u x v = -(1, 1, 1) (a flat scene is not seen edge-on),
    # from a plane 3 radii before the box's centre
    u, v = np.array([1.0, 0.0, -1.0]), np.array([1.0, -2.0, 1.0])
    plane = c + 3.0 * r * np.ones(3) / np.sqrt(3.0)
    rng = np.random.default_rng(4096)
    n = 4096
    inside = c + (rng.random((n // 2, 3)) * 2.0 - 1.0) * r
    far_dir = rng.normal(size=(n // 2, 3))
    far_dir /= np.linalg.norm(far_dir, axis=1, keepdims=True)
    far = c + far_dir * r * rng.uniform(8.0, 1000.0, (n // 2, 1))
    org = np.concatenate([inside, far])
    target = c + (rng.random((n, 3)) * 2.0 - 1.0) * r  # every ray aims into the box
    dirs = target - org
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dirs *= rng.uniform(0.25, 1.0625, (n, 1))
    batches = {"equirect": gpu.equirect_rays(eye, 128, 64),
               "ortho": gpu.ortho_rays(plane, u, v, 2.5 * r, 64, 64),
               "random": (org.astype(np.float32), dirs.astype(np.float32))}
    ln = np.sqrt((batches["random"][1].astype(np.float64) ** 2).sum(axis=1))
    assert ln.min() >= 0.2499 and ln.max() <= 1.0625
    return batches


@pytest.mark.parametrize("scene", ["spheres", "car-on-road"])
def test_rays_no_pinhole_makes(gpu, scene_dir, scene):
    """Panorama, orthographic and random rays: the proven octree walk equals
    brute force bit for bit, colours and samples; directions of length 4 leave
    the proof's assumption -- RT_EINEXACT, counted, and still the same bits."""
    s = gpu.Scene.load_svati(os.path.join(scene_dir, scene + ".svati"))
    s.set_size(96, 54)
    flat, oct_ = _ctx(gpu, s, "flat"), _ctx(gpu, s, "octree_gpu", exact=True)
    for what, (o, d) in _odd_rays(gpu, s, oct_).items():
        rf, sf, stf = flat.trace_rays(o, d, samples=True)
        ro, so, sto = oct_.trace_rays(o, d, samples=True)
        assert (sf["prim"] >= 0).mean() > 0.02, (what, "the batch must hit the scene")
        assert _same(ro, rf) and _same(so, sf), (scene, what, _diff_rays(ro, so, rf, sf)[:5])
        assert sto["closest_unproven"] == 0 and oct_.last_rc == 0
        assert (sto["closest"], sto["shadow"], sto["camera"]) == (stf["closest"], stf["shadow"], len(o))
    o, d = _odd_rays(gpu, s, oct_)["random"]
    d4 = (d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True) * 4.0).astype(np.float32)
    rf, sf, _ = flat.trace_rays(o, d4, samples=True)
    oct_.inexact = True  # lets RT_EINEXACT through _check_render; the code is kept in last_rc
    ro, so, sto = oct_.trace_rays(o, d4, samples=True)
    assert oct_.last_rc == RT_EINEXACT and sto["closest_unproven"] > 0
    assert _same(ro, rf) and _same(so, sf)


# ---- 5: cast only --------------------------------------------------------------
@pytest.mark.parametrize("accel,exact", PROVEN, ids=[a for a, _ in PROVEN])
def test_ray_cast(gpu, scene_dir, accel, exact):
    """d_rgb = NULL: one closest-hit query per ray, no shade pass -- the full
    trace's first-hit fields with queries == 1, no shadow query, and the
    closest-hit probe's brute force answer."""
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(96, 54)
    ctx = _ctx(gpu, s, accel, exact)
    o, d = gpu.camera_rays(s.frame(), "pixel")
    _, full, _ = ctx.trace_rays(o, d, samples=True)
    rgb, cast, st = ctx.trace_rays(o, d, shade=False)
    assert rgb is None
    for k in ("prim", "obj", "dist", "P", "N"):
        assert _same(cast[k], full[k]), k
    assert (cast["queries"] == 1).all() and (full["queries"] >= 1).all()
    assert st["shadow"] == 0 and st["closest"] == len(o) == st["camera"] and st["hits"] == (cast["prim"] >= 0).sum()
    prim, dist = ctx.probe_closest(o, d, brute=True)
    assert np.array_equal(prim.view(np.int32), cast["prim"])
    hit = cast["prim"] >= 0
    assert hit.any() and not hit.all()
    assert np.array_equal(dist[hit].view(np.uint32), cast["dist"][hit].view(np.uint32))
    assert np.isinf(cast["dist"][~hit]).all()


# ---- 6: the packet flag ---------------------------------------------------------
@pytest.mark.parametrize("name", ["cube_256x256", "spheres_100x52"])
def test_packet_flag_changes_no_bit(gpu, scene_dir, tmp_path, name):
    """Quarter-ordered frame rays with and without RT_RAYS_PACKET: identical
    bytes, and the golden image after the inverse permutation."""
    s, case, gold = _load(gpu, scene_dir, tmp_path, name)
    f = s.frame()
    ctx = _ctx(gpu, s, "octree_gpu")
    o, d = ctx.frame_rays(f, "quarter")
    r0, s0, st0 = ctx.trace_rays(o, d, samples=True)
    r1, s1, st1 = ctx.trace_rays(o, d, samples=True, packet=True)
    assert _same(r0, r1) and _same(s0, s1), _diff_rays(r0, s0, r1, s1)[:5]
    assert (st0["closest"], st0["shadow"], st0["hits"]) == (st1["closest"], st1["shadow"], st1["hits"])
    assert st1["depth_overflow"] == 0
    _, inv = gpu.quarter_order(f.width, f.height)
    img = gpu.fold_samples(r1[inv]).reshape(gold.shape)
    assert np.array_equal(img.view(np.uint32), gold.view(np.uint32))


def test_packet_flag_on_incoherent_rays(gpu, scene_dir):
    """The flag is a promise about speed only: on a random batch it still gives
    the bits of the per-lane walk and of brute force."""
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(96, 54)
    ctx, flat = _ctx(gpu, s, "octree_gpu"), _ctx(gpu, s, "flat")
    o, d = _odd_rays(gpu, s, ctx)["random"]
    rf, sf, _ = flat.trace_rays(o, d, samples=True)
    r0, s0, _ = ctx.trace_rays(o, d, samples=True)
    r1, s1, st1 = ctx.trace_rays(o, d, samples=True, packet=True)
    assert st1["depth_overflow"] == 0
    assert _same(r0, r1) and _same(s0, s1)
    assert _same(r1, rf) and _same(s1, sf), _diff_rays(r1, s1, rf, sf)[:5]
    # ignored on FLAT and under exact reflections
    r2, s2, _ = flat.trace_rays(o, d, samples=True, packet=True)
    assert _same(r2, rf) and _same(s2, sf)
    ctx.set_exact_reflections(True)
    r3, s3, _ = ctx.trace_rays(o, d, samples=True, packet=True)
    assert _same(r3, rf) and _same(s3, sf)


# ---- 7: the item scheme's edges -------------------------------------------------
@pytest.fixture(scope="module")
def cube_pattern(gpu, scene_dir):
    """4,096 rays at the cube (12 triangles) and brute force's answer, shared."""
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "cube.svati"))
    s.set_size(32, 32)
    o, d = gpu.camera_rays(s.frame(), "pixel")
    assert len(o) == 4096
    rgb, smp, _ = gpu.Context(s, "flat").trace_rays(o, d, samples=True)
    assert 0.05 < (smp["prim"] >= 0).mean() < 0.95
    return s, o, d, rgb, smp


@pytest.mark.parametrize("accel", ["flat", "octree"])
def test_batch_sizes_at_item_edges(gpu, cube_pattern, accel):
    s, o, d, rgb, smp = cube_pattern
    ctx = _ctx(gpu, s, accel)
    for n in (0, 1, 63, 64, 65, 8 * 64 + 1):
        r, sm, st = ctx.trace_rays(o[:n], d[:n], samples=True, packet=(n == 65))
        assert r.shape == (n, 3) and sm.shape == (n,)
        assert _same(r, rgb[:n]) and _same(sm, smp[:n]), n
        assert st["camera"] == n and st["closest"] == int(smp["queries"][:n].sum())
    # more items than persistent waves: items pulled through the stream counters
    n = 64 * (ctx.info()["trace_grid"] + 9) + 1
    reps = -(-n // 4096)
    r, _, st = ctx.trace_rays(np.tile(o, (reps, 1))[:n], np.tile(d, (reps, 1))[:n])
    assert st["camera"] == n
    want = np.tile(rgb, (reps, 1))[:n]
    bad = np.flatnonzero((r.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (n, bad[:5])


@pytest.mark.parametrize("accel", ["flat", "octree"])
def test_invalid_rays_are_not_traced(gpu, cube_pattern, accel):
    """NaN origins, infinite and all-zero directions scattered in a batch:
    colour 0, a miss of 0 queries; every other ray is unchanged."""
    s, o, d, rgb, smp = cube_pattern
    o, d = o[:1000].copy(), d[:1000].copy()
    bad = np.array([0, 5, 63, 64, 65, 127, 500, 998, 999])
    o[bad[0::3], 1] = np.nan
    d[bad[1::3], 2] = np.inf
    d[bad[2::3]] = 0.0
    d[bad[2], 0] = -0.0
    ctx = _ctx(gpu, s, accel)
    for packet in (False, True):
        r, sm, st = ctx.trace_rays(o, d, samples=True, packet=packet)
        ok = np.ones(1000, bool)
        ok[bad] = False
        assert _same(r[ok], rgb[:1000][ok]) and _same(sm[ok], smp[:1000][ok])
        assert not r[bad].any()
        assert (sm["prim"][bad] == -1).all() and (sm["obj"][bad] == -1).all() and (sm["queries"][bad] == 0).all()
        assert np.isinf(sm["dist"][bad]).all() and not sm["P"][bad].any() and not sm["N"][bad].any()
        assert st["camera"] == 1000 - len(bad) and st["closest"] == int(smp["queries"][:1000][ok].sum())


# ---- 8: overflow and growth ----------------------------------------------------
def test_hit_buffer_overflow_and_growth(gpu, tmp_path):
    """mirrors 32x18: 2,304 rays make 101,376 records against a first sizing of
    two per ray.  The device call reports RT_EHITBUF through rt_hip_stats, the
    buffers grow, the second call gives the golden image; the host call hides
    the retry."""
    case = OWN["mirrors_32x18"]
    s = gpu.Scene.load_svati(own_scene_path(case, tmp_path))
    s.set_size(32, 18)
    gold = own_golden_image(case)
    o, d = gpu.camera_rays(s.frame(), "pixel")
    ctx = _ctx(gpu, s, "octree", exact=True)
    dev = Dev(gpu)
    d_o, d_d, d_rgb = dev.upload(o), dev.upload(d), dev.malloc(o.nbytes)
    ctx.trace_rays_device(d_o, d_d, len(o), d_rgb)
    with pytest.raises(gpu.RtError) as e:
        ctx.stats()
    assert e.value.code == RT_EHITBUF
    ctx.trace_rays_device(d_o, d_d, len(o), d_rgb)
    st = ctx.stats()
    img = gpu.fold_samples(dev.host(d_rgb, o.shape, np.float32)).reshape(gold.shape)
    dev.close()
    assert np.array_equal(img.view(np.uint32), gold.view(np.uint32))
    assert (st["closest"], st["shadow"], st["hit_records"]) == (case["closest"], case["shadow"], 101376)
    fresh = _ctx(gpu, s, "octree", exact=True)
    rgb, _, st2 = fresh.trace_rays(o, d)
    assert fresh.last_rc == 0 and st2["hit_records"] == 101376
    assert np.array_equal(gpu.fold_samples(rgb).reshape(gold.shape).view(np.uint32), gold.view(np.uint32))


# ---- 9: the neighbours stay intact ---------------------------------------------
def test_batch_invalidates_the_kept_frame(gpu, scene_dir):
    """A batch overwrites the hit records: relight and G-buffer of the frame
    before it are refused until the frame is rendered again, and then give
    what they gave."""
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(96, 54)
    f = s.frame()
    ctx = _ctx(gpu, s, "octree_gpu")
    ctx.set_gbuffer(True)
    ctx.set_keep_visibility(True)
    img, smp, st = ctx.render_image_gbuffer(f)
    lights = s.lights()
    for l in lights:
        l.r, l.g, l.b = 0.5 * l.r, 0.25 * l.g, 0.75 * l.b
    ctx.set_lights(lights)
    rel, _ = ctx.relight_image(f)
    assert not _same(rel, img)
    o, d = gpu.camera_rays(f, "pixel")
    ctx.trace_rays(o[:1000], d[:1000], samples=True)
    with pytest.raises(gpu.RtError) as e:
        ctx.relight_image(f)
    assert e.value.code == RT_EINVAL
    dev = Dev(gpu)
    with pytest.raises(gpu.RtError) as e:
        ctx.gbuffer(f, 0, 1, dev.malloc(4 * gpu.gbuffer_tile_words(f.width, f.height, 1)))
    assert e.value.code == RT_EINVAL
    dev.close()
    img2, smp2, st2 = ctx.render_image_gbuffer(f)
    rel2, _ = ctx.relight_image(f)
    assert _same(img2, rel) and _same(rel2, rel) and _same(smp2, smp)  # (the lights are the edited ones now)
    assert (st2["closest"], st2["shadow"]) == (st["closest"], st["shadow"])


@pytest.mark.parametrize("name,W,H", [("spheres", 96, 54), ("car-on-road", 98, 50)])
def test_batch_between_streamed_frames(gpu, scene_dir, name, W, H):
    """Three frames streamed with overlapped list builds, a batch enqueued on
    the same stream between each pair: the frames' images, the last frame's
    counters and the side-stream builds are those of the run without batches,
    and the batches' own results are brute force's."""
    from test_overlap_lists import STAT_KEYS, Run, _frames
    s = gpu.Scene.load_svati(os.path.join(scene_dir, name + ".svati"))
    s.set_size(W, H)
    out = {}
    for with_batches in (False, True):
        run = Run(gpu, s, "octree_gpu", True)
        frames = _frames(gpu, s, run.centre, n=3)
        o, d = gpu.camera_rays(frames[1], "pixel")
        o, d = o[:2048], d[:2048]
        dev = Dev(gpu)
        d_o, d_d = dev.upload(o), dev.upload(d)
        run.warm(frames[0])
        b0 = run.ctx.overlap_builds()
        rgbs, brgb = [], []
        for k, fr in enumerate(frames):
            if with_batches and k:
                brgb.append(dev.malloc(o.nbytes))
                run.ctx.trace_rays_device(d_o, d_d, len(o), brgb[-1], packet=(k == 2))
            rgbs.append(run.render(fr))
        st = run.ctx.stats()
        out[with_batches] = ([run.image(r, fr) for r, fr in zip(rgbs, frames)], {k: st[k] for k in STAT_KEYS},
                             run.ctx.overlap_builds() - b0, [dev.host(b, o.shape, np.float32) for b in brgb])
        dev.close()
        run.close()
    (img0, st0, builds0, _), (img1, st1, builds1, batches) = out[False], out[True]
    assert builds0 == builds1 and builds0 >= 2
    assert st0 == st1
    for a, b in zip(img0, img1):
        assert _same(a, b)
    ref, _, _ = _ctx(gpu, s, "flat").trace_rays(o, d)
    assert len(batches) == 2 and all(_same(b, ref) for b in batches)


def test_refusals_change_nothing(gpu, scene_dir):
    """RT_EINVAL for a non-default policy, the work-counting pass, no output,
    quarter order on 96x54, odd sizes and too many rays; the next render is
    the golden image."""
    case = CASES["cube_96x54"]
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "cube.svati"))
    s.set_size(96, 54)
    f = s.frame()
    ctx = _ctx(gpu, s, "octree")
    o, d = gpu.camera_rays(f, "pixel")
    o, d = o[:256], d[:256]

    def refused(call):
        with pytest.raises(gpu.RtError) as e:
            call()
        assert e.value.code == RT_EINVAL, e.value

    ctx.set_policy(1)
    refused(lambda: ctx.trace_rays(o, d))
    ctx.set_policy(0)
    ctx.set_count_work(True)
    refused(lambda: ctx.trace_rays(o, d))
    ctx.set_count_work(False)
    dev = Dev(gpu)
    d_o, d_d, d_rgb = dev.upload(o), dev.upload(d), dev.malloc(o.nbytes)
    refused(lambda: ctx.trace_rays_device(d_o, d_d, len(o)))  # neither colours nor samples
    refused(lambda: ctx.trace_rays_device(d_o, d_d, 0xfffffff9, d_rgb))  # past what a record index addresses
    refused(lambda: ctx.trace_rays_device(d_o, d_d, len(o), 0, d_rgb + 4))  # samples not 8-byte aligned
    ctx.trace_rays_device(d_o, d_d, 0, d_rgb)  # n = 0: RT_OK, nothing written
    dev.close()
    refused(lambda: ctx.frame_rays(f, "quarter"))
    odd = gpu.Frame()
    C.pointer(odd)[0] = f
    odd.width = 95
    refused(lambda: ctx.frame_rays(odd, "pixel"))
    img, st = ctx.render_image(f)
    assert np.array_equal(img.view(np.uint32), golden_image(case).view(np.uint32))
    assert (st["closest"], st["shadow"], st["pixels"]) == (case["closest"], case["shadow"], 96 * 54)
    assert st["camera"] == 4 * 96 * 54
    r, _, stb = ctx.trace_rays(o, d)
    assert stb["camera"] == 256 and stb["pixels"] == 0
    # the device-side frame check accounts a batch, and a cast, like a render
    ctx.frame_check()
    _, st = ctx.render_image(f)
    _, _, stb = ctx.trace_rays(o, d)
    _, _, stc = ctx.trace_rays(o, d, shade=False)
    flags, frames, closest, shadow = ctx.frame_check()
    assert (flags, frames) == (0, 3)
    assert closest == st["closest"] + stb["closest"] + stc["closest"] and stc["closest"] == 256
    assert shadow == st["shadow"] + stb["shadow"] and stc["shadow"] == 0
