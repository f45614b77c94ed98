"""Ambient occlusion from G-buffer records on the GPU (include/rt_hip.h
rt_hip_ambient_occlusion): the device's rays equal the numpy twin's word for
word, a record's count is the sum of an occlusion batch's bytes on those rays,
the oracle decides, pieces with bases, the three sources of records, the kept
frame, streamed frames and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from test_ao_host import edge_records, same_words
from test_rays import PROVEN, Dev, _ctx

pytestmark = pytest.mark.gpu

RT_EINVAL = -1
SCENES = ["spheres", "island_smooth", "car-on-road", "point-light"]
INF = np.float32(np.inf)
SEED = 20261020
BASE = 2 ** 32 - 100  # the hash's low word wraps inside every batch here
FILL = 0xAB
KS = (1, 3, 4, 5, 64, 65, 100)  # (5: 60 busy lanes; 65, 100: two rounds)


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


_SHARED = {}


@pytest.fixture(scope="module")
def shared(gpu, scene_dir):
    """Per scene at 32x18, computed once and left unchanged: the 2,304
    first-hit records of a FLAT cast of the camera rays, the 37-row table, the
    k = 4 rays of the numpy twin and the oracle's collide_dist of them."""
    def get(name):
        if name not in _SHARED:
            s = gpu.Scene.load_svati(os.path.join(scene_dir, name + ".svati"))
            s.set_size(32, 18)
            flat = gpu.Context(s, "flat")
            o, d = gpu.camera_rays(s.frame(), "pixel")
            _, hits, _ = flat.trace_rays(o, d, shade=False)
            flat.close()
            assert len(hits) == 2304
            table = gpu.ao_table(37, SEED)
            ro, rd, shot = gpu.ao_rays_host(hits, 4, table, SEED)
            _SHARED[name] = dict(scene=s, cam=(o, d), hits=hits, table=table, rays=(ro, rd), shot=shot,
                                 D=_oracle_dists(s, ro, rd))
        return _SHARED[name]
    return get


@pytest.fixture(scope="module")
def records(gpu, shared):
    """The samples of `spheres` with the block of edge records appended."""
    return np.concatenate([shared("spheres")["hits"], edge_records(gpu.GSAMPLE)])


def _counts(bytes_, k):
    return np.asarray(bytes_, np.uint32).reshape(-1, k).sum(axis=1, dtype=np.uint32)


# ---- 1: rays word for word ------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 37])
def test_rays_word_for_word(gpu, shared, records, m):
    """rt_hip_ao_rays == ao_rays_host as uint32 for k in {1, 3, 4, 64, 65, 100}
    at a base whose low word wraps, the shot bytes included; memory past 3 n k
    floats and past n bytes, pre-filled, is untouched."""
    table = gpu.ao_table(m, 3 + m)
    n = len(records)
    assert records["prim"].min() < 0 <= records["prim"].max()
    ctx = _ctx(gpu, shared("spheres")["scene"], "flat")
    dev = Dev(gpu)
    d_s, d_t, d_sync = dev.upload(records), dev.upload(table), dev.malloc(4)
    for k in (1, 3, 4, 64, 65, 100):
        nr = n * k
        d_o = dev.upload(np.full(12 * nr + 64, FILL, np.uint8))
        d_d = dev.upload(np.full(12 * nr + 64, FILL, np.uint8))
        d_m = dev.upload(np.full(n + 64, FILL, np.uint8))
        ctx.ao_rays_device(d_s, n, k, d_t, m, SEED, d_o, d_d, d_m, base=BASE)
        # (a one-record batch on the same stream: its stats wait for the stream)
        ctx.ambient_occlusion_device(d_s, 1, 1, d_t, m, SEED, d_sync)
        ctx.stats()
        go, gd, gm = dev.host(d_o, 12 * nr + 64, np.uint8), dev.host(d_d, 12 * nr + 64, np.uint8), dev.host(d_m, n + 64, np.uint8)
        ho, hd, hshot = gpu.ao_rays_host(records, k, table, SEED, base=BASE)
        assert (go[12 * nr:] == FILL).all() and (gd[12 * nr:] == FILL).all() and (gm[n:] == FILL).all(), (k, m)
        assert np.array_equal(gm[:n], hshot.astype(np.uint8)), (k, m, np.flatnonzero(gm[:n] != hshot)[:5])
        assert same_words(go[:12 * nr].view(np.float32).reshape(-1, 3), ho), (k, m)
        god = gd[:12 * nr].view(np.float32).reshape(-1, 3)
        bad = np.flatnonzero(~((god.view(np.uint32) == hd.view(np.uint32)) | (np.isnan(god) & np.isnan(hd))).all(axis=1))
        assert len(bad) == 0, (k, m, len(bad), bad[:5], god[bad[:2]], hd[bad[:2]])
    # the host convenience is the same call
    o, d, shot = ctx.ao_rays(records, 3, table, SEED, base=BASE)
    ho, hd, hshot = gpu.ao_rays_host(records, 3, table, SEED, base=BASE)
    assert same_words(o, ho) and same_words(d, hd) and np.array_equal(shot, hshot)
    assert 0.05 < hshot.mean() < 0.95, "some records shoot and some do not"
    dev.close()
    ctx.close()


# ---- 2: counts equal an occlusion batch ------------------------------------------------------
@pytest.fixture(scope="module")
def dstar(gpu, shared, records):
    """A distance that is exactly one ray's: the median of a FLAT cast's hit
    distances over the k = 4 rays of `records`."""
    table = shared("spheres")["table"]
    o, d, _ = gpu.ao_rays_host(records, 4, table, SEED, base=BASE)
    flat = gpu.Context(shared("spheres")["scene"], "flat")
    _, cast, _ = flat.trace_rays(o, d, shade=False)
    flat.close()
    dist = np.sort(cast["dist"][cast["prim"] >= 0])
    assert len(dist) > 100
    return np.float32(dist[len(dist) // 2])


@pytest.mark.parametrize("accel", ["flat", "octree_gpu", "octree"])
def test_counts_equal_an_occlusion_batch(gpu, shared, records, dstar, accel):
    """ambient_occlusion == the per-sample sum of Context.occluded on the rays
    of test 1, no masking, with the batch's stats: every k, tmax in {none, D*,
    the float below, 0, -1, NaN}, the packet flag on and off, n around the
    item's edges into a pre-filled output (every word [0, n) written, none past)."""
    table = shared("spheres")["table"]
    m, N = len(table), len(records)
    ctx = _ctx(gpu, shared("spheres")["scene"], accel)
    dev = Dev(gpu)
    d_s, d_t = dev.upload(records), dev.upload(table)
    tmaxes = {"none": None, "D*": dstar, "below": np.nextafter(dstar, np.float32(0)), "0": np.float32(0),
              "-1": np.float32(-1), "nan": np.float32(np.nan)}
    seen = set()
    for k in KS:
        o, d, shot = gpu.ao_rays_host(records, k, table, SEED, base=BASE)
        spi = 64 // k if k <= 64 else 1
        for what, tmax in tmaxes.items():
            ref, rst = ctx.occluded(o, d, tmax)
            want = _counts(ref, k)
            if what in ("none", "D*"):
                assert 0 < want.sum() < shot.sum() * k, (accel, k, what, "some rays occluded and some not")
            if what == "below" and k >= 4:  # (D* is one of the first 4 rays' distances)
                assert want.sum() < _counts(ctx.occluded(o, d, dstar)[0], k).sum(), "the tie at D* is cut off"
            for packet in (False, True):
                got, st = ctx.ambient_occlusion(records, k, table, SEED, tmax=tmax, packet=packet, base=BASE)
                bad = np.flatnonzero(got != want)
                assert len(bad) == 0, (accel, k, what, packet, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
                assert st == rst, (accel, k, what, packet, st, rst)
                assert ctx.last_rc == 0
            assert rst["camera"] == (0 if what == "nan" else int((shot & np.isfinite(records["P"]).all(axis=1)).sum()) * k)
            assert rst["shadow"] == (rst["camera"] if what in ("none", "D*", "below") else 0)
            assert all(v == 0 for key, v in rst.items() if key not in ("camera", "shadow")), rst
        # n around the item's edges, through the device entry point
        ref_none, ref_d = _counts(ctx.occluded(o, d, None)[0], k), _counts(ctx.occluded(o, d, dstar)[0], k)
        for j, n in enumerate(sorted({0, 1, spi - 1, spi, spi + 1, 2304, N})):
            for tmax, want in ((None, ref_none), (dstar, ref_d)):
                d_out = dev.upload(np.full(n + 64, FILL * 0x01010101, np.uint32))
                ctx.ambient_occlusion_device(d_s if n else 0, n, k, d_t if n else 0, m, SEED, d_out if n else 0,
                                             tmax=tmax, packet=bool(j & 1), base=BASE)
                if n:
                    st = ctx.stats()
                    _, pst = ctx.occluded(o[:n * k], d[:n * k], tmax)
                    assert (st["camera"], st["shadow"]) == (pst["camera"], pst["shadow"]), (accel, k, n)
                got = dev.host(d_out, n + 64, np.uint32)
                assert np.array_equal(got[:n], want[:n]), (accel, k, n, np.flatnonzero(got[:n] != want[:n])[:5])
                assert (got[n:] == FILL * 0x01010101).all(), (accel, k, n)
                seen.add(n)
    assert {0, 1, 63, 64, 65, 20, 21, 22, 2304, N} <= seen
    dev.close()
    ctx.close()


# ---- 3: the oracle decides ----------------------------------------------------------------------
@pytest.mark.parametrize("accel,exact", PROVEN, ids=[a for a, _ in PROVEN])
@pytest.mark.parametrize("name", SCENES)
def test_the_oracle_decides(gpu, shared, name, accel, exact):
    """count = the number of a record's k = 4 rays with D != 0 && D <= tmax, D
    the oracle's collide_dist on the rays of ao_rays_host, for tmax unbounded,
    the median of the nonzero D (an actual distance: a tie at the bound), the
    float below it and 0: brute force and both proven octree walks."""
    sh = shared(name)
    D, hits, table = sh["D"], sh["hits"], sh["table"]
    live = np.repeat(sh["shot"], 4)
    assert live.sum() >= 1000, (name, "rays")
    share = float((D[live] != 0).mean())
    assert 0.05 <= share <= 0.95, (name, "unbounded", share)
    med = np.sort(D[D != 0])[int((D != 0).sum()) // 2]
    assert float(((D[live] != 0) & (D[live] <= med)).mean()) >= 0.02, (name, "median")
    ctx = _ctx(gpu, sh["scene"], accel, exact)
    for what, tmax in (("none", None), ("median", med), ("below", np.nextafter(med, np.float32(0))), ("0", np.float32(0))):
        want = _counts((D != 0) & (D <= (INF if tmax is None else tmax)), 4)
        got, st = ctx.ambient_occlusion(hits, 4, table, SEED, tmax=tmax)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (name, accel, what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
        assert st["shadow_zero_risk"] == 0 and st["closest_unproven"] == 0 and ctx.last_rc == 0
        assert st["camera"] == int(live.sum()) and st["shadow"] == (0 if what == "0" else st["camera"])
    assert _counts((D != 0) & (D <= med), 4).sum() > _counts((D != 0) & (D <= np.nextafter(med, np.float32(0))), 4).sum()
    ctx.close()


# ---- 4: pieces ----------------------------------------------------------------------------------
def test_pieces_with_bases_give_the_whole(gpu, shared, records):
    """The batch cut at ragged points, each piece with its base, gives the whole
    batch's words; a wrong base gives a different count vector."""
    table = shared("spheres")["table"]
    ctx = _ctx(gpu, shared("spheres")["scene"], "octree_gpu")
    whole, _ = ctx.ambient_occlusion(records, 4, table, SEED, base=BASE)
    assert 0 < whole.sum()
    dev = Dev(gpu)
    d_s, d_t = dev.upload(records), dev.upload(table)
    d_out = dev.upload(np.full(len(records) + 16, FILL * 0x01010101, np.uint32))
    cuts = [0, 1, 17, 99, 100, 101, 1000, 1003, len(records)]  # (the low word wraps between 99 and 100)
    for a, b in zip(cuts, cuts[1:]):
        ctx.ambient_occlusion_device(d_s + 40 * a, b - a, 4, d_t, len(table), SEED, d_out + 4 * a, base=BASE + a)
    ctx.stats()
    got = dev.host(d_out, len(records) + 16, np.uint32)
    assert np.array_equal(got[:len(records)], whole) and (got[len(records):] == FILL * 0x01010101).all()
    wrong, _ = ctx.ambient_occlusion(records[100:], 4, table, SEED, base=BASE + 99)
    assert not np.array_equal(wrong, whole[100:])
    dev.close()
    ctx.close()


# ---- 5: sources of records ------------------------------------------------------------------------
def test_sources_of_records(gpu, shared):
    """A tile buffer straight from rt_hip_gbuffer (device pointer, tile order),
    the assembled samples and a ray batch's records of the same camera rays:
    the assembled samples and the batch's records give the same words, which are
    the occlusion batch's on the twin's rays; the tile buffer gives them after
    reordering, under a table whose rays do not depend on a record's index
    (one row, the normal itself), and its padding slots count 0."""
    sh = shared("spheres")
    s, table = sh["scene"], sh["table"]
    f = s.frame()
    W, H = f.width, f.height
    ctx = _ctx(gpu, s, "octree_gpu")
    ctx.set_gbuffer(True)
    dev = Dev(gpu)
    ntile = gpu.gbuffer_tile_words(W, H, 1) // gpu.GB_WORDS
    d_c, d_g, d_a = dev.malloc(4 * gpu.tile_buffer_floats(W, H, 1)), dev.malloc(40 * ntile), dev.malloc(40 * 4 * W * H)
    ctx.render(f, 0, 1, d_c)
    ctx.gbuffer(f, 0, 1, d_g)
    ctx.assemble_gbuffer(f, d_g, 1, d_a)
    ctx.stats()
    smp = dev.host(d_a, 4 * W * H, gpu.GSAMPLE)
    normal = np.array([[0, 0, 1]], np.float32)
    d_t, d_n = dev.upload(table), dev.upload(normal)
    outs = {}
    for key, d_rec, n, d_tab, m in (("tiles", d_g, ntile, d_n, 1), ("assembled/normal", d_a, 4 * W * H, d_n, 1),
                                    ("assembled", d_a, 4 * W * H, d_t, len(table))):
        d_out = dev.upload(np.full(n, FILL * 0x01010101, np.uint32))
        ctx.ambient_occlusion_device(d_rec, n, 4, d_tab, m, SEED, d_out)
        ctx.stats()
        outs[key] = dev.host(d_out, n, np.uint32)
    # the ray batch's records of the same camera rays (the batch overwrites the kept frame: last)
    o, d = sh["cam"]
    d_o, d_d, d_r = dev.upload(o), dev.upload(d), dev.malloc(40 * len(o))
    ctx.trace_rays_device(d_o, d_d, len(o), 0, d_r)
    ctx.stats()
    d_out = dev.upload(np.full(len(o), FILL * 0x01010101, np.uint32))
    ctx.ambient_occlusion_device(d_r, len(o), 4, d_t, len(table), SEED, d_out)
    ctx.stats()
    outs["batch"] = dev.host(d_out, len(o), np.uint32)
    rec = dev.host(d_r, len(o), gpu.GSAMPLE)
    ro, rd, _ = gpu.ao_rays_host(smp, 4, table, SEED)
    want = _counts(ctx.occluded(ro, rd)[0], 4)
    assert 0 < want.sum() < 4 * len(smp)
    assert np.array_equal(outs["assembled"], want)
    # the rule reads prim, P and N: where the batch's records carry the frame's, the words are the frame's
    alike = (rec["prim"] == smp["prim"]) & (rec["P"].view(np.uint32) == smp["P"].view(np.uint32)).all(axis=1) & \
        (rec["N"].view(np.uint32) == smp["N"].view(np.uint32)).all(axis=1)
    assert alike.mean() > 0.99, alike.mean()
    assert np.array_equal(outs["batch"][alike], want[alike]), np.flatnonzero(outs["batch"] != want)[:5]
    bo, bd, _ = gpu.ao_rays_host(rec, 4, table, SEED)
    assert np.array_equal(outs["batch"], _counts(ctx.occluded(bo, bd)[0], 4))
    # along the normal every one of a record's 4 rays is the same ray: 0 or 4
    assert set(np.unique(outs["assembled/normal"])) == {0, 4}
    tiles = gpu.assemble_gbuffer_numpy(outs["tiles"], W, H, 1, words=4).reshape(-1)
    assert np.array_equal(tiles, outs["assembled/normal"])
    assert outs["tiles"].sum() == outs["assembled/normal"].sum(), "padding slots are misses: count 0"
    dev.close()
    ctx.close()


# ---- 6: the kept frame survives -----------------------------------------------------------------
def test_the_kept_frame_survives(gpu, scene_dir):
    """render (G-buffer and visibility kept) -> ambient occlusion -> the
    G-buffer read through rt_hip_gbuffer is the render's, and a relight under
    edited lights gives the image and the stats of the same sequence without it."""
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(96, 54)
    f = s.frame()
    table = gpu.ao_table(37, SEED)
    lights = [(l.type, 0.5 * l.r, 0.25 * l.g, 0.75 * l.b, l.v.x, l.v.y, l.v.z) for l in s.lights()]
    out = {}
    for with_ao in (False, True):
        ctx = _ctx(gpu, s, "octree_gpu")
        ctx.set_gbuffer(True)
        ctx.set_keep_visibility(True)
        img, smp, st = ctx.render_image_gbuffer(f)
        if with_ao:
            tmax = np.float32(0.5) * np.float32(ctx.info()["scene_radius"])
            part = smp.reshape(-1)[::6][:3000].copy()  # spread over the frame: sky and geometry
            got, sta = ctx.ambient_occlusion(part, 4, table, SEED, tmax=tmax, packet=True)
            ro, rd, shot = gpu.ao_rays_host(part, 4, table, SEED)
            assert sta["camera"] == 4 * int(shot.sum()) > 0 and sta["closest"] == 0 and sta["hit_records"] == 0
            flat = _ctx(gpu, s, "flat")
            assert np.array_equal(got, _counts(flat.occluded(ro, rd, tmax)[0], 4))
            flat.close()
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
        out[with_ao] = (img, smp, st, rel, strel)
        ctx.close()
    (img0, smp0, st0, rel0, strel0), (img1, smp1, st1, rel1, strel1) = out[False], out[True]
    assert img0.tobytes() == img1.tobytes() and smp0.tobytes() == smp1.tobytes() and st0 == st1
    assert rel0.tobytes() != img0.tobytes()
    assert rel0.tobytes() == rel1.tobytes()
    assert strel0 == strel1 and strel0["closest"] == st0["closest"] > 0


# ---- 7: between two streamed frames -----------------------------------------------------------------
def test_ambient_occlusion_between_streamed_frames(gpu, scene_dir, shared):
    """Three frames streamed with overlapped list builds, an ambient-occlusion
    call enqueued on the same stream between each pair: the frames' images, the
    last frame's counters and the side-stream builds are those of the run
    without, and the counts are brute force's."""
    from test_overlap_lists import STAT_KEYS, Run, _frames
    sh = shared("spheres")
    table, hits = sh["table"], sh["hits"]
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(96, 54)
    out = {}
    for with_ao in (False, True):
        run = Run(gpu, s, "octree_gpu", True)
        frames = _frames(gpu, s, run.centre, n=3)
        dev = Dev(gpu)
        d_s, d_t = dev.upload(hits), dev.upload(table)
        run.warm(frames[0])
        b0 = run.ctx.overlap_builds()
        rgbs, aout = [], []
        for k, fr in enumerate(frames):
            if with_ao and k:
                aout.append(dev.upload(np.full(len(hits), FILL * 0x01010101, np.uint32)))
                run.ctx.ambient_occlusion_device(d_s, len(hits), 4, d_t, len(table), SEED, aout[-1], packet=(k == 2))
            rgbs.append(run.render(fr))
        st = run.ctx.stats()
        out[with_ao] = ([run.image(r, fr) for r, fr in zip(rgbs, frames)], {k: st[k] for k in STAT_KEYS},
                        run.ctx.overlap_builds() - b0, [dev.host(b, len(hits), np.uint32) for b in aout])
        dev.close()
        run.close()
    (img0, st0, builds0, _), (img1, st1, builds1, counts) = out[False], out[True]
    assert builds0 == builds1 and builds0 >= 2
    assert st0 == st1
    for a, b in zip(img0, img1):
        assert a.tobytes() == b.tobytes()
    flat = _ctx(gpu, s, "flat")
    ref = _counts(flat.occluded(*sh["rays"])[0], 4)
    flat.close()
    assert 0 < ref.sum() and len(counts) == 2 and all(np.array_equal(c, ref) for c in counts)


# ---- 8: refusals change nothing -----------------------------------------------------------------------
def test_refusals_change_nothing(gpu, scene_dir, shared, records):
    """RT_EINVAL for each refusal of the contract; after each a valid call
    gives the counts it gave before and no refused call wrote a word.  After
    rt_hip_set_triangles the counts equal a fresh context's."""
    table = shared("spheres")["table"]
    m, n = len(table), len(records)
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(32, 18)
    ctx = _ctx(gpu, s, "octree_gpu")
    before, _ = ctx.ambient_occlusion(records, 4, table, SEED)
    dev = Dev(gpu)
    d_s, d_t = dev.upload(np.concatenate([records, records[:1]])), dev.upload(table)
    d_out = dev.upload(np.full(n, FILL * 0x01010101, np.uint32))
    d_o, d_d = dev.upload(np.full(12 * n * 4, FILL, np.uint8)), dev.upload(np.full(12 * n * 4, FILL, np.uint8))
    L = gpu.lib()

    def refused(call):
        with pytest.raises(gpu.RtError) as e:
            call()
        assert e.value.code == RT_EINVAL, e.value
        got, st = ctx.ambient_occlusion(records, 4, table, SEED)
        assert np.array_equal(got, before)

    ao = ctx.ambient_occlusion_device
    refused(lambda: ao(0, n, 4, d_t, m, SEED, d_out))
    refused(lambda: ao(d_s, n, 4, 0, m, SEED, d_out))
    refused(lambda: ao(d_s, n, 4, d_t, m, SEED, 0))
    refused(lambda: ao(d_s + 4, n, 4, d_t, m, SEED, d_out))  # not 8-byte aligned
    refused(lambda: ao(d_s, n, 0, d_t, m, SEED, d_out))
    refused(lambda: ao(d_s, n, gpu.AO_KMAX + 1, d_t, m, SEED, d_out))
    refused(lambda: ao(d_s, n, 4, d_t, 0, SEED, d_out))
    refused(lambda: ao(d_s, 0xfffffff8 // 4 + 1, 4, d_t, m, SEED, d_out))  # n k > RT_RAYS_MAX: nothing is dereferenced
    refused(lambda: ao(d_s, 0xfffffff8 // 1024 + 1, 1024, d_t, m, SEED, d_out))
    refused(lambda: gpu._check(L.rt_hip_ambient_occlusion(ctx.h, C.c_void_p(d_s), n, 0, 4, C.c_void_p(d_t), m, SEED,
                                                          C.c_float(np.inf), 2, C.c_void_p(d_out), None), "flags"))
    refused(lambda: gpu._check(L.rt_hip_ambient_occlusion(None, C.c_void_p(d_s), n, 0, 4, C.c_void_p(d_t), m, SEED,
                                                          C.c_float(np.inf), 0, C.c_void_p(d_out), None), "null context"))
    refused(lambda: ctx.ao_rays_device(d_s, n, 4, d_t, m, SEED, 0, d_d))
    refused(lambda: ctx.ao_rays_device(d_s + 4, n, 4, d_t, m, SEED, d_o, d_d))
    refused(lambda: ctx.ao_rays_device(d_s, n, 0, d_t, m, SEED, d_o, d_d))
    ctx.set_policy(1)
    with pytest.raises(gpu.RtError) as e:
        ctx.ambient_occlusion(records, 4, table, SEED)
    ctx.set_policy(0)
    assert e.value.code == RT_EINVAL and np.array_equal(ctx.ambient_occlusion(records, 4, table, SEED)[0], before)
    ctx.set_count_work(True)
    with pytest.raises(gpu.RtError) as e:
        ao(d_s, n, 4, d_t, m, SEED, d_out)
    ctx.set_count_work(False)
    assert e.value.code == RT_EINVAL and np.array_equal(ctx.ambient_occlusion(records, 4, table, SEED)[0], before)
    ao(0, 0, 4, 0, m, SEED, 0)  # n = 0: RT_OK, nothing written, nothing dereferenced
    ctx.stats()
    assert (dev.host(d_out, n, np.uint32) == FILL * 0x01010101).all()  # no refused call wrote a word
    assert (dev.host(d_o, 12 * n * 4, np.uint8) == FILL).all() and (dev.host(d_d, 12 * n * 4, np.uint8) == FILL).all()
    dev.close()
    # moved geometry: the live context's counts are a fresh context's
    first, count = gpu.object_range(s, 0)
    tris = s.triangles_array()
    moved = gpu.shift_triangles(tris[first:first + count], (0.0, 0.5 * float(gpu.vertex_extent(tris[first:first + count])), 0.0))
    ctx.set_triangles(moved, first)
    live, _ = ctx.ambient_occlusion(records, 4, table, SEED)
    s.set_triangles_array(moved, first)
    fresh_ctx = _ctx(gpu, s, "octree_gpu")
    fresh, _ = fresh_ctx.ambient_occlusion(records, 4, table, SEED)
    assert np.array_equal(live, fresh) and not np.array_equal(live, before)
    fresh_ctx.close()
    ctx.close()
