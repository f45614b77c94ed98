"""Occlusion batches on the GPU (include/rt_hip.h rt_hip_occluded): one byte
per ray, 1 if the reference's collide_dist (cpu/hit.c:93-109) is not 0 and <=
the ray's tmax.  The oracle decides; the cast, brute force, the packet flag, the
item scheme's edges, rays not traced, |d|, the kept frame and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import REPO
from test_rays import GOLDENS, PROVEN, Dev, _ctx, _load, _odd_rays

pytestmark = pytest.mark.gpu

RT_EINVAL, RT_EINEXACT = -1, -11
HEMI_SCENES = ["spheres", "island_smooth", "car-on-road", "point-light"]
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


class _Vec(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class _Ray(C.Structure):
    _fields_ = [("origin", _Vec), ("direction", _Vec)]


def _oracle_dists(scene, o, d):
    """collide_dist(scene, ray) of the oracle per ray -> float32 (n,)."""
    import oracle as orc
    L = orc.lib()
    L.oracle_collide_dist.argtypes = [C.c_void_p, _Ray]
    L.oracle_collide_dist.restype = C.c_float
    sp = C.cast(scene.ptr, C.c_void_p)
    return np.array([L.oracle_collide_dist(sp, _Ray(_Vec(*map(float, o[i])), _Vec(*map(float, d[i]))))
                     for i in range(len(o))], np.float32)


def _mixed(bytes_, what):
    """Non-vacuity: at least 5 % of a batch occluded and at least 5 % not."""
    share = float(np.asarray(bytes_, bool).mean())
    assert 0.05 <= share <= 0.95, (what, share)
    return share


_SHARED = {}


@pytest.fixture(scope="module")
def shared(gpu, scene_dir):
    """Per scene at 32x18, computed once: the camera rays, the first-hit
    samples of a FLAT cast, 4 hemisphere rays per hit, the scene radius and the
    oracle's collide_dist of the batch `hemi + every 4th camera ray`."""
    def get(name):
        if name not in _SHARED:
            s = gpu.Scene.load_svati(os.path.join(scene_dir, name + ".svati"))
            s.set_size(32, 18)
            flat = gpu.Context(s, "flat")
            o, d = gpu.camera_rays(s.frame(), "pixel")
            _, hits, _ = flat.trace_rays(o, d, shade=False)
            ok = (hits["prim"] >= 0) & hits["N"].any(axis=1)
            ho, hd = gpu.hemisphere_rays(hits["P"][ok], hits["N"][ok], 4, 20261020)
            bo, bd = np.concatenate([ho, o[::4]]), np.concatenate([hd, d[::4]])
            _SHARED[name] = dict(scene=s, o=o, d=d, hits=hits, hemi=(ho, hd), batch=(bo, bd),
                                 R=np.float32(flat.info()["scene_radius"]), D=_oracle_dists(s, bo, bd))
            flat.close()
        return _SHARED[name]
    return get


# ---- 1: the oracle decides -------------------------------------------------------
@pytest.mark.parametrize("accel,exact", PROVEN, ids=[a for a, _ in PROVEN])
@pytest.mark.parametrize("name", HEMI_SCENES)
def test_the_oracle_decides(gpu, shared, name, accel, exact):
    """byte = (D != 0 && D <= tmax) with D the oracle's collide_dist, for tmax
    unbounded, exactly D, one ulp below, one ulp above, R/4 and 0: brute force
    and both proven octree walks.  The three D-relative rounds are the point: a
    prefilter or a prune that loses a tie at the bound fails them."""
    sh = shared(name)
    (o, d), D, R = sh["batch"], sh["D"], sh["R"]
    nh = len(sh["hemi"][0])
    _mixed(D[:nh] != 0, (name, "hemi, unbounded"))
    _mixed((D[:nh] != 0) & (D[:nh] <= R / np.float32(4)), (name, "hemi, R/4"))
    _mixed(D != 0, (name, "batch, unbounded"))
    ctx = _ctx(gpu, sh["scene"], accel, exact)
    rounds = {"none": None, "D": D, "below": np.nextafter(D, np.float32(0)), "above": np.nextafter(D, INF),
              "R/4": np.full(len(D), R / np.float32(4), np.float32), "0": np.zeros(len(D), np.float32)}
    for what, tmax in rounds.items():
        got, st = ctx.occluded(o, d, tmax)
        want = (D != 0) & (D <= (INF if tmax is None else tmax))
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (name, accel, what, len(bad), bad[:5], D[bad[:5]])
        assert st["shadow_zero_risk"] == 0 and ctx.last_rc == 0 and st["closest_unproven"] == 0
        assert st["camera"] == len(o) and st["shadow"] == (len(o) if tmax is None else int((tmax > 0).sum()))
        assert (st["closest"], st["pixels"], st["hits"], st["hit_records"], st["cand_entries"]) == (0, 0, 0, 0, 0)
    assert not ctx.occluded(o, d, rounds["below"])[0].any() and ctx.occluded(o, d, D)[0].sum() == (D != 0).sum()


# ---- 2: cast consistency ---------------------------------------------------------
@pytest.fixture(scope="module")
def golden_rays(gpu, scene_dir, tmp_path_factory):
    """The goldens' camera rays (126,720 in all) and their scenes' radii, once."""
    tmp = tmp_path_factory.mktemp("own")
    out = {}
    for name in GOLDENS:
        s, _, _ = _load(gpu, scene_dir, tmp, name)
        o, d = gpu.camera_rays(s.frame(), "pixel")
        flat = gpu.Context(s, "flat")
        out[name] = dict(scene=s, o=o, d=d, R=np.float32(flat.info()["scene_radius"]))
        flat.close()
    assert sum(len(g["o"]) for g in out.values()) == 126720
    return out


@pytest.mark.parametrize("accel,exact", PROVEN, ids=[a for a, _ in PROVEN])
def test_cast_consistency(gpu, golden_rays, accel, exact):
    """occluded(o, d, tmax) == (prim >= 0 && dist <= tmax) of the same context's
    ray cast, for tmax unbounded, the cast's own dist, one ulp below it and a
    seeded value in (0, 2 dist)."""
    rng = np.random.default_rng(55)
    for name, g in golden_rays.items():
        ctx = _ctx(gpu, g["scene"], accel, exact)
        o, d = g["o"], g["d"]
        _, cast, _ = ctx.trace_rays(o, d, shade=False)
        hit, dist = cast["prim"] >= 0, cast["dist"]
        with np.errstate(invalid="ignore"):
            rnd = (dist * rng.uniform(1e-3, 2.0, len(o)).astype(np.float32)).astype(np.float32)
        for what, tmax in (("none", None), ("dist", dist), ("below", np.nextafter(dist, np.float32(0))), ("random", rnd)):
            got, st = ctx.occluded(o, d, tmax)
            want = hit & (dist <= (INF if tmax is None else tmax))
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (name, accel, what, len(bad), bad[:5])
            assert st["shadow_zero_risk"] == 0 and ctx.last_rc == 0
        if name.split("_96")[0] in ("cube", "spheres", "car-on-road", "point-light"):  # (the island fills its frame)
            _mixed(hit, (name, "camera rays"))
        ctx.close()


# ---- 3: the default slack walk against brute force ----------------------------------
@pytest.mark.parametrize("accel", ["octree", "octree_gpu"])
def test_default_bounded_walk_against_brute_force(gpu, golden_rays, shared, accel):
    """The per-lane bounded walk (tested, not proven) tests a subset of the
    records with the same exact test: no ray occluded that brute force calls
    free; a ray brute force calls occluded and the walk does not is the
    coplanar-grazing class on brute force's winner, at most 64 per scene."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from grazing import coplanar_grazing
    batches = [(n, g["scene"], g["o"], g["d"], g["R"]) for n, g in golden_rays.items()]
    batches += [(n + " hemi", shared(n)["scene"], *shared(n)["hemi"], shared(n)["R"]) for n in HEMI_SCENES]
    total = missed = 0
    for name, s, o, d, R in batches:
        walk, flat = _ctx(gpu, s, accel), _ctx(gpu, s, "flat")
        tri = None
        for tmax in (None, np.float32(R / np.float32(4))):
            gw, stw = walk.occluded(o, d, tmax)
            gf, _ = flat.occluded(o, d, tmax)
            assert stw["depth_overflow"] == 0 and walk.last_rc == 0
            extra = np.flatnonzero((gw == 1) & (gf == 0))
            assert len(extra) == 0, (name, accel, tmax, extra[:5])
            miss = np.flatnonzero((gw == 0) & (gf == 1))
            total += len(o)
            missed += len(miss)
            assert len(miss) <= 64, (name, accel, tmax, len(miss))
            if len(miss):
                tri = s.triangles_array() if tri is None else tri
                _, cast, _ = flat.trace_rays(o[miss], d[miss], shade=False)
                lim = INF if tmax is None else tmax
                unexplained = [int(i) for k, i in enumerate(miss)
                               if not (cast["prim"][k] >= 0 and cast["dist"][k] <= lim and
                                       coplanar_grazing(tri[cast["prim"][k]], o[i], d[i]))]
                assert not unexplained, (name, accel, tmax, unexplained[:5])
        walk.close()
        flat.close()
    print(f"{accel} bounded slack walk: {total} ray queries, {missed} occluded by brute force only, all coplanar-grazing")


# ---- 4: the packet flag changes no byte ----------------------------------------------
def _packet_batches(gpu, scene_dir, tmp_path):
    for name in ("cube_256x256", "spheres_100x52"):
        s, _, _ = _load(gpu, scene_dir, tmp_path, name)
        yield name, s, gpu.camera_rays(s.frame(), "quarter")
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(96, 54)
    ctx = gpu.Context(s, "flat")
    yield "spheres random", s, _odd_rays(gpu, s, ctx)["random"]
    ctx.close()


def test_packet_flag_changes_no_byte(gpu, scene_dir, tmp_path):
    """RT_RAYS_PACKET is a promise about the caller's order that only buys
    speed: quarter-ordered camera rays and a seeded incoherent batch, unbounded
    and with a seeded tmax per ray, give the same bytes with and without it, on
    the octree (where they are brute force's) and on FLAT (where it is ignored)."""
    rng = np.random.default_rng(64)
    for name, s, (o, d) in _packet_batches(gpu, scene_dir, tmp_path):
        flat, oct_ = _ctx(gpu, s, "flat"), _ctx(gpu, s, "octree_gpu")
        c = np.array(flat.info()["scene_center"], np.float32)
        # about the distance to the scene's middle: bounds on both sides of the hits
        tm = (np.linalg.norm(o - c, axis=1) * rng.uniform(0.0, 2.0, len(o))).astype(np.float32)
        for tmax in (None, tm):
            f0, _ = flat.occluded(o, d, tmax)
            f1, _ = flat.occluded(o, d, tmax, packet=True)
            o0, st0 = oct_.occluded(o, d, tmax)
            o1, st1 = oct_.occluded(o, d, tmax, packet=True)
            assert st1["depth_overflow"] == 0 and oct_.last_rc == 0
            assert np.array_equal(f0, f1), (name, "flat")
            assert np.array_equal(o0, o1), (name, "octree", np.flatnonzero(o0 != o1)[:5])
            assert np.array_equal(o1, f0), (name, "octree vs flat", np.flatnonzero(o1 != f0)[:5])
            assert (st0["camera"], st0["shadow"]) == (st1["camera"], st1["shadow"])
            if tmax is None:
                unbounded = int(f0.sum())
                _mixed(f0, name)
            else:
                assert 0 < f0.sum() < unbounded, (name, "the bounds cut some hits off and keep some")
        if name == "spheres random":  # ignored under exact reflections
            oct_.set_exact_reflections(True)
            e1, _ = oct_.occluded(o, d, tm, packet=True)
            assert np.array_equal(e1, flat.occluded(o, d, tm)[0])
        flat.close()
        oct_.close()


# ---- 5: item edges and untouched memory -------------------------------------------------
@pytest.fixture(scope="module")
def cube_rays(gpu, scene_dir):
    """513 rays spread over a 32x32 frame of the cube, a seeded tmax per ray and
    brute force's answers (unbounded, bounded), shared."""
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "cube.svati"))
    s.set_size(32, 32)
    o, d = gpu.camera_rays(s.frame(), "pixel")
    pick = (np.arange(513) * 7919) % len(o)
    o, d = o[pick].copy(), d[pick].copy()
    flat = gpu.Context(s, "flat")
    _, cast, _ = flat.trace_rays(o, d, shade=False)
    rng = np.random.default_rng(513)
    tm = np.where(cast["prim"] >= 0, cast["dist"] * rng.uniform(0.5, 1.5, 513), 1.0).astype(np.float32)
    a_none, a_tm = flat.occluded(o, d)[0], flat.occluded(o, d, tm)[0]
    flat.close()
    _mixed(a_none, "cube rays")
    assert 0 < a_tm.sum() < a_none.sum()
    return s, o, d, tm, a_none, a_tm


@pytest.mark.parametrize("accel", ["flat", "octree"])
def test_item_edges_and_untouched_memory(gpu, cube_rays, accel):
    """n around the 64-ray item's edges through the device entry point into a
    buffer 64 bytes longer, pre-filled with 0xAA: the first n bytes are the
    513-ray answer's prefix, every byte past n is untouched."""
    s, o, d, tm, a_none, a_tm = cube_rays
    ctx = _ctx(gpu, s, accel)
    full, _ = ctx.occluded(o, d)
    assert np.array_equal(full, a_none) and np.array_equal(ctx.occluded(o, d, tm)[0], a_tm)
    dev = Dev(gpu)
    d_o, d_d, d_t = dev.upload(o), dev.upload(d), dev.upload(tm)
    for n in (1, 63, 64, 65, 511, 513):
        for d_tmax, want in ((0, a_none), (d_t, a_tm)):
            d_out = dev.upload(np.full(n + 64, 0xAA, np.uint8))
            ctx.occluded_device(d_o, d_d, d_tmax, n, d_out, packet=(n == 65))
            st = ctx.stats()
            got = dev.host(d_out, n + 64, np.uint8)
            assert np.array_equal(got[:n], want[:n]), (accel, n)
            assert (got[n:] == 0xAA).all(), (accel, n, np.flatnonzero(got[n:] != 0xAA)[:5])
            assert st["camera"] == n and st["shadow"] == n
    ctx.occluded_device(0, 0, 0, 0, 0)  # n = 0: RT_OK, nothing written, nothing dereferenced
    dev.close()
    ctx.close()


# ---- 6: rays not traced ------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["flat", "octree"])
def test_rays_not_traced(gpu, cube_rays, accel):
    """Non-finite components, an all-zero direction and a NaN tmax are not
    traced; tmax of -1, 0 and -0.0 is traced without a query.  Byte 0 each, the
    valid rays' bytes unchanged, and the two counts in the stats."""
    s, o, d, tm, a_none, a_tm = cube_rays
    o, d, tm = o.copy(), d.copy(), tm.copy()
    occ = np.flatnonzero(a_tm)
    assert len(occ) >= 8
    untraced = np.unique(np.concatenate([[0, 5, 63, 64, 65, 127, 300, 511, 512], occ[:4]]))
    o[untraced[0::4], 1] = np.nan
    d[untraced[1::4], 2] = np.inf
    d[untraced[2::4]] = 0.0
    d[untraced[2::4][0], 0] = -0.0
    tm[untraced[3::4]] = np.nan
    unasked = np.setdiff1d(np.concatenate([[1, 62, 66, 128, 400, 510], occ[4:8]]), untraced)
    tm[unasked[0::3]] = -1.0
    tm[unasked[1::3]] = 0.0
    tm[unasked[2::3]] = -0.0
    ok = np.ones(513, bool)
    ok[untraced] = False
    ok[unasked] = False
    assert a_tm[untraced].any() and a_tm[unasked].any(), "some of the edited rays were occluded before"
    ctx = _ctx(gpu, s, accel)
    for packet in (False, True):
        got, st = ctx.occluded(o, d, tm, packet=packet)
        assert not got[~ok].any()
        assert np.array_equal(got[ok], a_tm[ok])
        assert st["camera"] == 513 - len(untraced) and st["shadow"] == 513 - len(untraced) - len(unasked)
    # without tmax the rays with a bad tmax are ordinary rays again
    got, st = ctx.occluded(o, d)
    geo = untraced[np.arange(len(untraced)) % 4 != 3]
    assert not got[geo].any() and st["camera"] == st["shadow"] == 513 - len(geo)
    rest = np.ones(513, bool)
    rest[geo] = False
    assert np.array_equal(got[rest], a_none[rest])
    ctx.close()


# ---- 7: |d| does not scale tmax ---------------------------------------------------------
def test_direction_length_does_not_scale_tmax(gpu, scene_dir):
    """tmax is a world distance: directions scaled by 0.25 and 1.0625 with the
    same tmax.  FLAT answers (prim >= 0 && dist <= tmax) of its own cast of the
    scaled rays; the proven octree walk and the default bounded walk equal
    FLAT.  |d| = 4 under exact reflections: RT_EINEXACT, counted, the same bytes."""
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(96, 54)
    flat, exact, walk = _ctx(gpu, s, "flat"), _ctx(gpu, s, "octree_gpu", exact=True), _ctx(gpu, s, "octree")
    o, d = gpu.camera_rays(s.frame(), "pixel")
    o, d = o[::5], d[::5]
    _, c1, _ = flat.trace_rays(o, d, shade=False)
    rng = np.random.default_rng(7)
    R = np.float32(flat.info()["scene_radius"])
    tm = np.where(c1["prim"] >= 0, c1["dist"] * rng.uniform(0.5, 1.5, len(o)), R).astype(np.float32)
    tm[::9] = c1["dist"][::9]  # ties (inf for a miss)
    answers = []
    for scale in (1.0, 0.25, 1.0625, 4.0):
        ds = (d * np.float32(scale)).astype(np.float32)
        _, cast, _ = flat.trace_rays(o, ds, shade=False)
        want = (cast["prim"] >= 0) & (cast["dist"] <= tm)
        got, _ = flat.occluded(o, ds, tm)
        assert np.array_equal(got, want), (scale, np.flatnonzero(got != want)[:5])
        _mixed(want, ("scaled", scale))
        answers.append(got)
        exact.inexact = scale > 1.0  # lets RT_EINEXACT through _check_render; the code is kept in last_rc
        ge, ste = exact.occluded(o, ds, tm)
        if scale == 4.0:
            assert exact.last_rc == RT_EINEXACT and ste["closest_unproven"] > 0
        elif scale > 1.0:  # unit directions times 1.0625 round to either side of the proof's |d| <= 1.0625
            assert exact.last_rc == (RT_EINEXACT if ste["closest_unproven"] else 0)
        else:
            assert exact.last_rc == 0 and ste["closest_unproven"] == 0
        if scale != 4.0:
            gw, _ = walk.occluded(o, ds, tm)
            assert np.array_equal(gw, got), ("default walk", scale, np.flatnonzero(gw != got)[:5])
            assert np.array_equal(walk.occluded(o, ds, tm, packet=True)[0], got), ("packet", scale)
        assert np.array_equal(ge, got), ("proven walk", scale, np.flatnonzero(ge != got)[:5])
    # the geometry is the same ray: away from the ties the answers agree across the scales
    away = np.ones(len(o), bool)
    away[::9] = False
    assert all((a[away] != answers[0][away]).mean() < 0.01 for a in answers[1:])


# ---- 8: the kept frame survives -------------------------------------------------------
def test_the_kept_frame_survives(gpu, scene_dir):
    """render (G-buffer and visibility kept) -> occlusion batch -> the G-buffer
    read through rt_hip_gbuffer is the render's, and a relight under edited
    lights gives the image and the stats of the same sequence without the batch."""
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(96, 54)
    f = s.frame()
    o, d = gpu.camera_rays(f, "pixel")
    # (rows, not the scene's own array: both runs render the scene as loaded)
    lights = [(l.type, 0.5 * l.r, 0.25 * l.g, 0.75 * l.b, l.v.x, l.v.y, l.v.z) for l in s.lights()]
    out = {}
    for with_batch in (False, True):
        ctx = _ctx(gpu, s, "octree_gpu")
        ctx.set_gbuffer(True)
        ctx.set_keep_visibility(True)
        img, smp, st = ctx.render_image_gbuffer(f)
        if with_batch:
            got, stb = ctx.occluded(o[:3000], d[:3000], np.float32(0.5) * np.float32(ctx.info()["scene_radius"]),
                                    packet=True)
            assert stb["camera"] == 3000 and stb["closest"] == 0 and stb["hit_records"] == 0
            want, _ = _ctx(gpu, s, "flat").occluded(o[:3000], d[:3000],
                                                     np.float32(0.5) * np.float32(ctx.info()["scene_radius"]))
            assert np.array_equal(got, want)
            # the G-buffer after the batch: the samples from before it
            dev = Dev(gpu)
            d_gt = dev.malloc(4 * gpu.gbuffer_tile_words(f.width, f.height, 1))
            d_gs = dev.malloc(smp.nbytes)
            ctx.gbuffer(f, 0, 1, d_gt)
            ctx.assemble_gbuffer(f, d_gt, 1, d_gs)
            ctx.stats()  # (waits for the stream)
            again = dev.host(d_gs, smp.shape, gpu.GSAMPLE)
            dev.close()
            assert again.tobytes() == smp.tobytes()
        ctx.set_lights(lights)
        rel, strel = ctx.relight_image(f)
        out[with_batch] = (img, smp, st, rel, strel)
        ctx.close()
    (img0, smp0, st0, rel0, strel0), (img1, smp1, st1, rel1, strel1) = out[False], out[True]
    assert img0.tobytes() == img1.tobytes() and smp0.tobytes() == smp1.tobytes() and st0 == st1
    assert rel0.tobytes() != img0.tobytes()
    assert rel0.tobytes() == rel1.tobytes()
    assert strel0 == strel1 and strel0["closest"] == st0["closest"] > 0


@pytest.mark.parametrize("name,W,H", [("spheres", 96, 54), ("car-on-road", 98, 50)])
def test_occlusion_batch_between_streamed_frames(gpu, scene_dir, name, W, H):
    """Three frames streamed with overlapped list builds, an occlusion batch
    enqueued on the same stream between each pair: the frames' images, the last
    frame's counters and the side-stream builds are those of the run without
    batches, and the batches' bytes are brute force's."""
    from test_overlap_lists import STAT_KEYS, Run, _frames
    s = gpu.Scene.load_svati(os.path.join(scene_dir, name + ".svati"))
    s.set_size(W, H)
    out = {}
    for with_batches in (False, True):
        run = Run(gpu, s, "octree_gpu", True)
        frames = _frames(gpu, s, run.centre, n=3)
        o, d = gpu.camera_rays(frames[1], "pixel")
        step = len(o) // 2048  # spread over the frame: sky and geometry
        o, d = o[::step][:2048].copy(), d[::step][:2048].copy()
        dev = Dev(gpu)
        d_o, d_d = dev.upload(o), dev.upload(d)
        run.warm(frames[0])
        b0 = run.ctx.overlap_builds()
        rgbs, bout = [], []
        for k, fr in enumerate(frames):
            if with_batches and k:
                bout.append(dev.malloc(len(o)))
                run.ctx.occluded_device(d_o, d_d, 0, len(o), bout[-1], packet=(k == 2))
            rgbs.append(run.render(fr))
        st = run.ctx.stats()
        out[with_batches] = ([run.image(r, fr) for r, fr in zip(rgbs, frames)], {k: st[k] for k in STAT_KEYS},
                             run.ctx.overlap_builds() - b0, [dev.host(b, len(o), np.uint8) for b in bout])
        dev.close()
        run.close()
    (img0, st0, builds0, _), (img1, st1, builds1, batches) = out[False], out[True]
    assert builds0 == builds1 and builds0 >= 2
    assert st0 == st1
    for a, b in zip(img0, img1):
        assert a.tobytes() == b.tobytes()
    ref, _ = _ctx(gpu, s, "flat").occluded(o, d)
    _mixed(ref, name)
    assert len(batches) == 2 and all(np.array_equal(b, ref) for b in batches)


# ---- 9: refusals change nothing -----------------------------------------------------------
def test_occlusion_refusals_change_nothing(gpu, cube_rays):
    """RT_EINVAL for NULL pointers, too many rays, a non-default policy and the
    work-counting pass; after each a valid batch gives the bytes it gave before."""
    s, o, d, tm, a_none, a_tm = cube_rays
    ctx = _ctx(gpu, s, "octree")
    dev = Dev(gpu)
    d_o, d_d, d_t, d_out = dev.upload(o), dev.upload(d), dev.upload(tm), dev.upload(np.full(513, 0xAA, np.uint8))

    def refused(call):
        with pytest.raises(gpu.RtError) as e:
            call()
        assert e.value.code == RT_EINVAL, e.value
        got, st = ctx.occluded(o, d, tm)
        assert np.array_equal(got, a_tm) and st["camera"] == 513

    refused(lambda: ctx.occluded_device(0, d_d, d_t, 513, d_out))
    refused(lambda: ctx.occluded_device(d_o, 0, d_t, 513, d_out))
    refused(lambda: ctx.occluded_device(d_o, d_d, d_t, 513, 0))
    refused(lambda: ctx.occluded_device(d_o, d_d, d_t, 0xfffffff9, d_out))  # nothing is dereferenced
    ctx.set_policy(1)
    refused_policy = None
    with pytest.raises(gpu.RtError) as e:
        ctx.occluded(o, d, tm)
    refused_policy = e.value.code
    ctx.set_policy(0)
    assert refused_policy == RT_EINVAL and np.array_equal(ctx.occluded(o, d, tm)[0], a_tm)
    ctx.set_count_work(True)
    with pytest.raises(gpu.RtError) as e:
        ctx.occluded_device(d_o, d_d, d_t, 513, d_out)
    ctx.set_count_work(False)
    assert e.value.code == RT_EINVAL and np.array_equal(ctx.occluded(o, d, tm)[0], a_tm)
    ctx.stats()
    assert (dev.host(d_out, 513, np.uint8) == 0xAA).all()  # no refused call wrote a byte
    dev.close()
    ctx.close()
