"""The opt-in per-sample G-buffer (include/rt_hip.h rt_gsample) on the GPU:
every sample of whole small frames against the oracle's brute-force replay
(oracle/diag.c winner + oracle_collide's hit point and normal, bit for bit),
the colour image unchanged with the feature on, the octree's samples == brute
force over a whole frame, the rank tile buffers and their assembly, moving and
revisited cameras, and the combinations the capture refuses.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import (case_id, golden_image, load_manifest_static, load_own_manifest, own_golden_image,
                      own_scene_path)

pytestmark = pytest.mark.gpu
CASES = load_manifest_static()
OWN_CASES = load_own_manifest()
RT_EINVAL = -1
INF_BITS = 0x7F800000


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


def _case(scene, W, H):
    if scene == "mirrors":
        return next(c for c in OWN_CASES if (c["width"], c["height"]) == (W, H))
    return next(c for c in CASES if (c["scene"], c["width"], c["height"]) == (scene, W, H))


def _scene(gpu, case, scene_dir, tmp_path):
    if "svati" in case:
        return gpu.Scene.load_svati(own_scene_path(case, tmp_path))
    s = gpu.Scene.load_svati(os.path.join(scene_dir, case["scene"] + ".svati"))
    s.set_size(case["width"], case["height"])
    return s


def _gold(case):
    return own_golden_image(case) if "svati" in case else golden_image(case)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bytes(a, b, what):
    wa = np.ascontiguousarray(a).view(np.uint32).reshape(-1, 10)
    wb = np.ascontiguousarray(b).view(np.uint32).reshape(-1, 10)
    assert wa.shape == wb.shape, (what, wa.shape, wb.shape)
    bad = np.argwhere((wa != wb).any(axis=1)).ravel()
    assert len(bad) == 0, f"{what}: {len(bad)} samples differ, first (flat sample index) {bad[:5].tolist()}"


# ---- the reference: one replay per scene, shared by the three accels ----
class _V3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class _Ray(C.Structure):
    _fields_ = [("origin", _V3), ("direction", _V3)]


REF = np.dtype([("obj", np.int32), ("tri", np.int32), ("queries", np.int32), ("dist", np.uint32),
                ("P", np.uint32, 3), ("N", np.uint32, 3)])
_REF = {}
_COLLIDE = None


def _collide():
    global _COLLIDE
    if _COLLIDE is None:
        import oracle as orc
        orc.lib()
        L = C.CDLL(orc.LIB)  # a handle of our own: its prototypes are ours
        L.oracle_collide.argtypes = [C.c_void_p, _Ray, C.POINTER(C.c_int)]
        L.oracle_collide.restype = _Ray
        _COLLIDE = L.oracle_collide
    return _COLLIDE


def _reference(key, s, W, H):
    """(H, W, 4) REF records of the scene's frame from oracle.diag_pixel (the
    camera query's winner and float dist, the camera + reflection queries of
    each sample) and oracle_collide on the camera ray (P, N)."""
    if key in _REF:
        return _REF[key]
    import oracle as orc
    collide = _collide()
    ptr = C.cast(s.ptr, C.c_void_p)
    ref = np.zeros((H, W, 4), REF)
    ref["obj"] = ref["tri"] = -1
    ref["dist"] = INF_BITS
    cams = 0
    for row in range(H):
        for col in range(W):
            qs, _ = orc.diag_pixel(ptr, row, col, max_queries=4096)
            assert len(qs) < 4096
            for q in qs:
                if q["kind"] not in ("camera", "reflection"):
                    continue
                r = ref[row, col, q["sample"]]
                r["queries"] += 1
                if q["kind"] != "camera":
                    continue
                cams += 1
                if not q["result"]:
                    assert q["obj"] == -1 and q["tri"] == -1
                    continue
                r["obj"], r["tri"] = q["obj"], q["tri"]
                r["dist"] = np.float32(q["dist"]).view(np.uint32)
                oi = C.c_int(-1)
                hit = collide(ptr, _Ray(_V3(*q["o"]), _V3(*q["d"])), C.byref(oi))
                assert oi.value == q["obj"]
                r["P"] = np.array([hit.origin.x, hit.origin.y, hit.origin.z], np.float32).view(np.uint32)
                r["N"] = np.array([hit.direction.x, hit.direction.y, hit.direction.z], np.float32).view(np.uint32)
    assert cams == 4 * W * H  # every sample of an even-sized frame has a camera query
    _REF[key] = ref
    return ref


EVERY_SAMPLE = [("cube", 96, 54), ("island_smooth", 30, 34), ("mirrors", 32, 18)]


@pytest.mark.parametrize("accel", ["flat", "octree", "octree_gpu"])
@pytest.mark.parametrize("scene,W,H", EVERY_SAMPLE, ids=[f"{s}_{w}x{h}" for s, w, h in EVERY_SAMPLE])
def test_every_sample_matches_the_reference(gpu, scene_dir, tmp_path, scene, W, H, accel):
    """Every sample of every pixel, no exclusions: the winner's (object,
    triangle) and the bits of its new_dist == the oracle's camera query, the
    path's closest-hit queries == the camera + reflection queries the oracle
    lists, P and N of a hit == oracle_collide's bits, a miss is exactly
    (-1, -1, queries, +inf, 0, 0); zero_normal == depth_overflow == 0 and the
    query counts sum to the manifest's."""
    case = _case(scene, W, H)
    s = _scene(gpu, case, scene_dir, tmp_path)
    ref = _reference((scene, W, H), s, W, H)
    img, smp, st = gpu.Context(s, accel).render_image_gbuffer(s.frame())
    assert smp.shape == (H, W, 4) and smp.dtype == gpu.GSAMPLE
    assert st["zero_normal"] == 0 and st["depth_overflow"] == 0
    assert int(ref["queries"].sum()) == case["closest"] == st["closest"]
    what = f"{case_id(case)}/{accel}"
    hit = ref["obj"] >= 0
    if scene == "cube":
        assert 0 < hit.sum() < hit.size / 2  # most samples miss
    if scene == "island_smooth":
        assert hit.sum() > 0.9 * hit.size and W % 8 and H % 8  # nearly all hit; ragged tiles
    if scene == "mirrors":
        assert ref["queries"].max() == 44
    # prim -> (object, index in its triangle array), one lookup per distinct prim
    lut = {int(p): gpu.prim_object_triangle(s, int(p)) for p in np.unique(smp["prim"])}
    ot = np.array([lut[int(p)] for p in smp["prim"].ravel()], np.int32).reshape(H, W, 4, 2)
    for name, got, want in (("object of prim", ot[..., 0], ref["obj"]), ("triangle of prim", ot[..., 1], ref["tri"]),
                            ("obj", smp["obj"], ref["obj"]), ("queries", smp["queries"], ref["queries"]),
                            ("dist bits", _bits(smp["dist"]), ref["dist"]),
                            ("P bits", _bits(smp["P"]), ref["P"]), ("N bits", _bits(smp["N"]), ref["N"])):
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{what}: {name} differs at {len(bad)} places, first (row, col, sample, ..) {bad[:4].tolist()}"
    miss = smp[~hit]
    assert (miss["prim"] == -1).all() and (miss["obj"] == -1).all()
    assert (_bits(miss["dist"]) == INF_BITS).all()
    assert (_bits(miss["P"]) == 0).all() and (_bits(miss["N"]) == 0).all()
    cov = gpu.coverage(smp)
    assert cov.shape == (H, W) and cov.dtype == np.float32
    assert np.array_equal(cov, hit.sum(axis=2).astype(np.float32) / 4)


@pytest.mark.parametrize("accel", ["flat", "octree", "octree_gpu"])
@pytest.mark.parametrize("scene,W,H", [("cube", 96, 54), ("mirrors", 32, 18)])
def test_colour_unchanged_with_gbuffer_on(gpu, scene_dir, tmp_path, scene, W, H, accel):
    """The image of render_image_gbuffer is bit-exact to the golden, with the
    manifest's closest / shadow counts."""
    case = _case(scene, W, H)
    s = _scene(gpu, case, scene_dir, tmp_path)
    img, _, st = gpu.Context(s, accel).render_image_gbuffer(s.frame())
    assert np.array_equal(_bits(img), _bits(_gold(case))), f"{case_id(case)}/{accel}"
    assert (st["closest"], st["shadow"]) == (case["closest"], case["shadow"])


def test_octree_samples_equal_brute_force(gpu, scene_dir, tmp_path):
    """car-on-road 100x52: the octree contexts' samples == the FLAT context's,
    byte for byte."""
    case = _case("car-on-road", 100, 52)
    s = _scene(gpu, case, scene_dir, tmp_path)
    f = s.frame()
    img_f, smp_f, st_f = gpu.Context(s, "flat").render_image_gbuffer(f)
    assert np.array_equal(_bits(img_f), _bits(_gold(case)))
    assert 0 < (smp_f["prim"] >= 0).sum() < smp_f.size
    for accel in ("octree", "octree_gpu"):
        img, smp, st = gpu.Context(s, accel).render_image_gbuffer(f)
        _same_bytes(smp, smp_f, f"car-on-road 100x52 {accel} vs flat")
        assert st["closest"] == st_f["closest"] == int(smp["queries"].sum())


SENTINEL = 0xA5A5A5A5


def _per_rank_gbuffer(gpu, ctx, f, nranks):
    """render + gbuffer of every rank on this GPU into one gathered buffer
    (prefilled with SENTINEL), then the device assemble.  Returns (assembled
    (H, W, 4) samples, the gathered buffers (nranks, tiles_per_rank, 64, 40))."""
    W, H = f.width, f.height
    L = gpu.lib()
    per_c, per_g = gpu.tile_buffer_floats(W, H, nranks), gpu.gbuffer_tile_words(W, H, nranks)
    assert per_g == gpu.tiles_per_rank_host(W, H, nranks) * 64 * 4 * gpu.GB_WORDS
    dc, dg, ds = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.rt_hip_malloc(0, per_c * 4, C.byref(dc)) == 0
    assert L.rt_hip_malloc(0, per_g * nranks * 4, C.byref(dg)) == 0
    assert L.rt_hip_malloc(0, W * H * 160, C.byref(ds)) == 0
    host = np.full(per_g * nranks, SENTINEL, np.uint32)
    assert L.rt_hip_memcpy_h2d(dg, host.ctypes.data_as(C.c_void_p), host.nbytes) == 0
    try:
        for r in range(nranks):
            ctx.render(f, r, nranks, dc.value)
            ctx.gbuffer(f, r, nranks, dg.value + r * per_g * 4)
            ctx.stats()  # raises unless the frame is complete
        out = np.empty((H, W, 4), gpu.GSAMPLE)
        ctx.assemble_gbuffer(f, dg.value, nranks, ds.value)
        ctx.stats()  # sync
        assert L.rt_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), ds, out.nbytes) == 0
        assert L.rt_hip_memcpy_d2h(host.ctypes.data_as(C.c_void_p), dg, host.nbytes) == 0
    finally:
        for d in (dc, dg, ds):
            L.rt_hip_free(d)
    return out, host.reshape(nranks, -1, 64, 4 * gpu.GB_WORDS)


MISS_WORDS = np.array([0xFFFFFFFF, 0xFFFFFFFF, 0, INF_BITS, 0, 0, 0, 0, 0, 0], np.uint32)


@pytest.mark.parametrize("W,H,nranks", [(100, 52, 3), (96, 54, 8), (2, 2, 1), (6, 130, 1)])
def test_rank_tiles_and_assembly(gpu, scene_dir, W, H, nranks):
    """Per-rank render + gbuffer on one GPU, then assemble_gbuffer == the
    one-rank result (the FLAT context's render_image_gbuffer) byte for byte ==
    assemble_gbuffer_numpy of the downloaded tile buffers; padding slots are
    misses without a query, a rank without tiles (96x54 over 8: ranks 4 to 7)
    writes nothing, and no rank writes past its tiles."""
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "island_smooth.svati"))
    s.set_size(W, H)
    f = s.frame()
    _, one, _ = gpu.Context(s, "flat").render_image_gbuffer(f)
    ctx = gpu.Context(s, "octree")
    ctx.set_gbuffer(True)
    got, bufs = _per_rank_gbuffer(gpu, ctx, f, nranks)
    _same_bytes(got, one, f"island_smooth {W}x{H}: {nranks} ranks assembled on the device")
    host = gpu.assemble_gbuffer_numpy(bufs, W, H, nranks)
    assert host.shape == (H, W, 40)
    _same_bytes(host, one, f"island_smooth {W}x{H}: {nranks} ranks assembled on the host")
    counts = [gpu.rank_tile_count(W, H, r, nranks) for r in range(nranks)]
    if (W, H, nranks) == (96, 54, 8):
        assert [c > 0 for c in counts] == [True] * 4 + [False] * 4  # 3 x 2 blocks on diagonals 0..3
    for r in range(nranks):
        if counts[r] == 0:
            assert (bufs[r] == SENTINEL).all(), f"rank {r}/{nranks} owns no tile but wrote"
            continue
        pix = gpu.tile_pixels(W, H, r, nranks)
        pad = pix[..., 0] < 0
        assert (bufs[r, : len(pix)][pad].reshape(-1, 10) == MISS_WORDS).all(), f"rank {r}/{nranks}: padding slots"
        assert (bufs[r, len(pix):] == SENTINEL).all(), f"rank {r}/{nranks}: wrote past its tiles"


def _panned_frame(gpu, scene, du):
    cam = gpu.Camera()
    C.pointer(cam)[0] = scene.s.camera
    f0 = scene.frame()
    u = np.array([f0.u.x, f0.u.y, f0.u.z], np.float64)
    u /= np.linalg.norm(u)
    cam.position.x += float(u[0] * du)
    cam.position.y += float(u[1] * du)
    cam.position.z += float(u[2] * du)
    f = gpu.Frame()
    gpu._check(gpu.lib().rt_frame_from_camera(C.byref(cam), C.byref(f)), "frame")
    return f


def test_moving_and_revisited_cameras(gpu):
    """Frames A, B (panned), A on one octree context with the G-buffer on
    (the asynchronous, estimated-shape list builds of new and revisited
    cameras): each G-buffer and image == the FLAT context's for that frame,
    and the third image is bit-exact to the first."""
    s = gpu.Scene.synthetic(4, 4, 1200, seed=0x5EED, width=480, height=270)
    fa, fb = s.frame(), _panned_frame(gpu, s, 0.05)
    flat = gpu.Context(s, "flat")
    want = {"A": flat.render_image_gbuffer(fa), "B": flat.render_image_gbuffer(fb)}
    assert not np.array_equal(_bits(want["A"][1]["dist"]), _bits(want["B"][1]["dist"]))
    ctx = gpu.Context(s, "octree")
    ctx.set_gbuffer(True)
    imgs = []
    for k, name in enumerate(("A", "B", "A")):
        img, smp, st = ctx.render_image_gbuffer(fa if name == "A" else fb)
        if k == 0:
            assert st["cand_entries"] > 0  # the frame has camera candidate lists
        _same_bytes(smp, want[name][1], f"frame {k} ({name}) vs flat")
        assert np.array_equal(_bits(img), _bits(want[name][0])), f"frame {k} ({name}) image vs flat"
        assert (st["closest"], st["shadow"]) == (want[name][2]["closest"], want[name][2]["shadow"])
        imgs.append(img)
    assert np.array_equal(_bits(imgs[2]), _bits(imgs[0]))


def test_refusals(gpu, scene_dir):
    case = _case("cube", 96, 54)
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "cube.svati"))
    s.set_size(96, 54)
    f = s.frame()
    L = gpu.lib()
    dc, dg = C.c_void_p(), C.c_void_p()
    assert L.rt_hip_malloc(0, gpu.tile_buffer_floats(96, 54, 1) * 4, C.byref(dc)) == 0
    assert L.rt_hip_malloc(0, gpu.gbuffer_tile_words(96, 54, 1) * 4, C.byref(dg)) == 0

    def refused(call):
        with pytest.raises(gpu.RtError) as e:
            call()
        assert e.value.code == RT_EINVAL, e.value
    try:
        # never enabled
        ctx = gpu.Context(s, "octree")
        ctx.render(f, 0, 1, dc.value)
        ctx.stats()
        refused(lambda: ctx.gbuffer(f, 0, 1, dg.value))
        # another frame, another rank split
        ctx.set_gbuffer(True)
        refused(lambda: ctx.gbuffer(f, 0, 1, dg.value))  # the last render had it off
        ctx.render(f, 0, 1, dc.value)
        ctx.gbuffer(f, 0, 1, dg.value)
        ctx.stats()
        refused(lambda: ctx.gbuffer(_panned_frame(gpu, s, 0.05), 0, 1, dg.value))
        refused(lambda: ctx.gbuffer(f, 0, 2, dg.value))
        # policy `lane`, exact reflections, the work-counting pass
        ctx.set_policy(1)
        refused(lambda: ctx.render(f, 0, 1, dc.value))
        ctx.set_policy(0)
        ctx.set_exact_reflections(True)
        refused(lambda: ctx.render(f, 0, 1, dc.value))
        ctx.set_exact_reflections(False)
        ctx.set_count_work(True)
        refused(lambda: ctx.render(f, 0, 1, dc.value))
        ctx.set_count_work(False)
        # off again: the default render, bit-exact to the golden
        ctx.set_gbuffer(False)
        img, st = ctx.render_image(f)
        assert np.array_equal(_bits(img), _bits(golden_image(case)))
        assert (st["closest"], st["shadow"]) == (case["closest"], case["shadow"])
        refused(lambda: ctx.gbuffer(f, 0, 1, dg.value))
    finally:
        L.rt_hip_free(dc)
        L.rt_hip_free(dg)
