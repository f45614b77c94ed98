"""Traced light gathered over a record's hemisphere on the GPU (include/rt_hip.h
rt_hip_gather, rt_hip_gather_host; kernels csrc/rt_gather.h): per record the
sum, in ray order, of the colours rt_hip_trace_rays gives its k hemisphere
rays.  The contract is a composition of calls that exist, so every case
compares with that composition on the same context, word for word; the oracle
decides on the proven configurations.  All cases work on the 32 x 18 casts of
test_ao.py's `shared` fixture: 2,304 first-hit records per scene, the 37-row
table, SEED, and a base near 2^32 so the hash's low word wraps."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_own_manifest, own_scene_path
from test_ao import BASE, FILL, KS, SCENES, SEED, gpu, records, shared  # noqa: F401  (fixtures)
from test_ao_host import same_words
from test_rays import PROVEN, Dev, _ctx

pytestmark = pytest.mark.gpu

RT_EINVAL, RT_EHITBUF = -1, -10
OWN = {f'{c["scene"]}_{c["width"]}x{c["height"]}': c for c in load_own_manifest()}
GUARD = 64  # floats past 3 n that must keep their fill
FILLF = np.frombuffer(bytes([FILL] * 4), np.uint32)[0]


def _composition(gpu, ctx, recs, k, table, base=0, packet=False):
    """gather_sum(trace_rays(*ao_rays(...)), k) on `ctx`, and the batch's stats."""
    o, d, _ = ctx.ao_rays(recs, k, table, SEED, base=base)
    rgb, _, st = ctx.trace_rays(o, d, packet=packet)
    return gpu.gather_sum(rgb, k), st


def _bad(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return np.flatnonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all(axis=1))


def _gather_guarded(gpu, dev, ctx, d_s, n, k, d_t, m, packet=False, base=0):
    """rt_hip_gather into a pre-filled buffer -> (n, 3) float32; every word of
    [0, 3 n) written is not checkable from the fill alone (a sum may equal it),
    so the caller compares with the composition; none past 3 n is checked here."""
    d_out = dev.upload(np.full(3 * n + GUARD, FILLF, np.uint32))
    ctx.gather_device(d_s, n, k, d_t, m, SEED, d_out, packet=packet, base=base)
    ctx.stats()
    raw = dev.host(d_out, 3 * n + GUARD, np.uint32)
    assert (raw[3 * n:] == FILLF).all(), (n, k, "written past 3 n")
    return raw[:3 * n].view(np.float32).reshape(-1, 3)


# ---- 1: the composition, word for word ---------------------------------------------------------
@pytest.mark.parametrize("m", [1, 37])
@pytest.mark.parametrize("accel", ["flat", "octree_gpu", "octree"])
def test_the_composition_word_for_word(gpu, shared, records, accel, m):
    """Context.gather == gather_sum(trace_rays(*ao_rays(...)), k) on the same
    context as uint32 (two NaNs agree) for k in (1, 3, 4, 5, 64, 65, 100), with
    and without the packet flag; the device call into a guard-filled buffer
    writes the same words and none past 3 n; records that do not shoot give
    three +0.0."""
    table = gpu.ao_table(m, 3 + m)
    n = len(records)
    ctx = _ctx(gpu, shared("spheres")["scene"], accel)
    dev = Dev(gpu)
    d_s, d_t = dev.upload(records), dev.upload(table)
    _, _, shot = gpu.ao_rays_host(records, 4, table, SEED, base=BASE)
    assert 0.05 < shot.mean() < 0.95, "some records shoot and some do not"
    lit = 0
    for k in KS:
        want, wst = _composition(gpu, ctx, records, k, table, base=BASE)
        assert want.shape == (n, 3)
        lit += int((want != 0).any(axis=1).sum())
        for packet in (False, True):
            got, st = ctx.gather(records, k, table, SEED, packet=packet, base=BASE)
            bad = _bad(got, want)
            assert len(bad) == 0, (accel, k, m, packet, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
            assert ctx.last_rc == 0 and st["camera"] == wst["camera"] and st["closest"] == wst["closest"]
            dgot = _gather_guarded(gpu, dev, ctx, d_s, n, k, d_t, m, packet=packet, base=BASE)
            assert same_words(dgot, want), (accel, k, m, packet, _bad(dgot, want)[:5])
            assert (got[~shot].view(np.uint32) == 0).all(), (accel, k, m, packet, "a record that does not shoot: +0.0")
    assert lit > 100, "the gathers bring light back"
    dev.close()
    ctx.close()


# ---- 2: the oracle decides ---------------------------------------------------------------------
_ORACLE = {}


def _oracle_sums(gpu, sh, name):
    """gather_sum of the oracle's trace(ray, 1.0) on the twin's k = 4 rays (the
    fixture's, base 0), computed once per scene."""
    if name not in _ORACLE:
        import oracle as orc
        rgb, _, _ = orc.trace_rays(sh["scene"].ptr, *sh["rays"])
        _ORACLE[name] = gpu.gather_sum(rgb, 4)
    return _ORACLE[name]


@pytest.mark.parametrize("accel,exact", PROVEN, ids=[a for a, _ in PROVEN])
@pytest.mark.parametrize("name", SCENES)
def test_the_oracle_decides(gpu, shared, name, accel, exact):
    """gather_sum(oracle.trace_rays(scene, *ao_rays_host(...)), 4) against the
    device at 0 ULP on brute force and both proven walks.  (tests/test_rays.py
    grants no ULP allowance for batch colours against the oracle -- its goldens
    are compared bit for bit -- so none is taken here.)"""
    sh = shared(name)
    want = _oracle_sums(gpu, sh, name)
    assert int(sh["shot"].sum()) >= 250 and (want != 0).any(axis=1).sum() > 50, name
    ctx = _ctx(gpu, sh["scene"], accel, exact)
    got, st = ctx.gather(sh["hits"], 4, sh["table"], SEED)
    bad = _bad(got, want)
    assert len(bad) == 0, (name, accel, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert st["closest_unproven"] == 0 and st["depth_overflow"] == 0 and ctx.last_rc == 0
    assert st["camera"] == 4 * int(sh["shot"].sum()) and st["pixels"] == 0
    ctx.close()


# ---- 3: deep paths and the buffer growth -------------------------------------------------------
def test_deep_paths_and_buffer_growth(gpu, tmp_path):
    """mirrors 32x18 (paths 43 deep): the records of a cast of its camera rays,
    k = 4.  Seen on the device: the first rt_hip_gather of a fresh context
    overflows the first sizing of two records per path and rt_hip_stats reports
    RT_EHITBUF; after the growth the second call equals the composition, as the
    host wrapper's hidden second attempt does, and depth_overflow equals the
    batch's."""
    case = OWN["mirrors_32x18"]
    s = gpu.Scene.load_svati(own_scene_path(case, tmp_path))
    s.set_size(32, 18)
    o, d = gpu.camera_rays(s.frame(), "pixel")
    table = gpu.ao_table(37, SEED)
    ref = _ctx(gpu, s, "octree_gpu")
    _, hits, _ = ref.trace_rays(o, d, shade=False)
    want, wst = _composition(gpu, ref, hits, 4, table, base=BASE)
    ref.close()
    assert wst["hit_records"] > 2 * 4 * len(hits), "more than two records per path"
    ctx = _ctx(gpu, s, "octree_gpu")
    dev = Dev(gpu)
    d_s, d_t, d_rgb = dev.upload(hits), dev.upload(table), dev.malloc(12 * len(hits))
    ctx.gather_device(d_s, len(hits), 4, d_t, len(table), SEED, d_rgb, base=BASE)
    with pytest.raises(gpu.RtError) as e:
        ctx.stats()
    assert e.value.code == RT_EHITBUF
    ctx.gather_device(d_s, len(hits), 4, d_t, len(table), SEED, d_rgb, base=BASE)
    st = ctx.stats()
    got = dev.host(d_rgb, (len(hits), 3), np.float32)
    dev.close()
    ctx.close()
    assert same_words(got, want), _bad(got, want)[:5]
    assert st == wst, (st, wst)
    fresh = _ctx(gpu, s, "octree_gpu")
    got2, st2 = fresh.gather(hits, 4, table, SEED, base=BASE)
    assert fresh.last_rc == 0 and same_words(got2, want)
    assert st2["depth_overflow"] == wst["depth_overflow"] and st2["hit_records"] == wst["hit_records"]
    fresh.close()


# ---- 4: pieces with bases give the whole -------------------------------------------------------
def test_pieces_with_bases_give_the_whole(gpu, shared, records):
    """n cut at 1, 63, 64, 65 and the rest, each piece with its base, gives the
    whole batch's words (k = 3: 21 records an item; k = 100: two rounds); a
    wrong base gives other words."""
    table = shared("spheres")["table"]
    n = len(records)
    ctx = _ctx(gpu, shared("spheres")["scene"], "octree_gpu")
    dev = Dev(gpu)
    d_s, d_t = dev.upload(records), dev.upload(table)
    for k in (3, 100):
        whole, _ = ctx.gather(records, k, table, SEED, base=BASE)
        assert (whole != 0).any()
        d_out = dev.upload(np.full(3 * n + GUARD, FILLF, np.uint32))
        cuts = np.cumsum([0, 1, 63, 64, 65]).tolist() + [n]
        for a, b in zip(cuts, cuts[1:]):
            ctx.gather_device(d_s + 40 * a, b - a, k, d_t, len(table), SEED, d_out + 12 * a, base=BASE + a)
        ctx.stats()
        raw = dev.host(d_out, 3 * n + GUARD, np.uint32)
        assert (raw[3 * n:] == FILLF).all()
        assert same_words(raw[:3 * n].view(np.float32).reshape(-1, 3), whole), k
        wrong, _ = ctx.gather(records[100:], k, table, SEED, base=BASE + 99)
        assert not same_words(wrong, whole[100:])
    dev.close()
    ctx.close()


# ---- 5: sources of records ---------------------------------------------------------------------
def test_sources_of_records(gpu, shared):
    """A rank's tile buffer straight from rt_hip_gbuffer (padding slots
    included: misses, three +0.0), the assembled samples, a ray batch's records
    and records_from_points: the device call on each equals the host path on
    the same records."""
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
    tiles, smp = dev.host(d_g, ntile, gpu.GSAMPLE), dev.host(d_a, 4 * W * H, gpu.GSAMPLE)
    assert ntile > 4 * W * H, "the tile buffer has padding slots"
    o, d = sh["cam"]
    d_o, d_d, d_r = dev.upload(o), dev.upload(d), dev.malloc(40 * len(o))
    ctx.trace_rays_device(d_o, d_d, len(o), 0, d_r)
    ctx.stats()
    rec = dev.host(d_r, len(o), gpu.GSAMPLE)
    hit = sh["hits"][sh["hits"]["prim"] >= 0]
    pts = gpu.records_from_points(hit["P"] + np.float32(0.25) * hit["N"], hit["N"], hit["obj"])
    d_p, d_t = dev.upload(pts), dev.upload(table)
    for key, d_rec, host in (("tiles", d_g, tiles), ("assembled", d_a, smp), ("batch", d_r, rec), ("points", d_p, pts)):
        got = _gather_guarded(gpu, dev, ctx, d_rec, len(host), 4, d_t, len(table))
        want, _ = ctx.gather(host, 4, table, SEED)
        assert same_words(got, want), (key, _bad(got, want)[:5])
        assert (want != 0).any(), key
        assert (got[host["prim"] < 0].view(np.uint32) == 0).all(), key
    # the padding slots of the tile buffer are misses
    order = gpu.assemble_gbuffer_numpy(np.arange(ntile, dtype=np.uint32), W, H, 1, words=4).reshape(-1)
    pad = np.setdiff1d(np.arange(ntile), order)
    assert len(pad) == ntile - 4 * W * H and (tiles["prim"][pad] < 0).all()
    dev.close()
    ctx.close()


# ---- 6: stats and the context ------------------------------------------------------------------
def test_stats_are_the_batch_s(gpu, shared, records):
    """rt_hip_stats after a gather equals the stats after trace_rays on the same
    rays, field by field: k <= 64 and k > 64, with and without the packet flag,
    default and proven walks and brute force; the frame check accounts a gather
    like a batch."""
    table = shared("spheres")["table"]
    for accel, exact in (("flat", False), ("octree_gpu", False), ("octree_gpu", True)):
        ctx = _ctx(gpu, shared("spheres")["scene"], accel, exact)
        for k in ((4,) if exact else (4, 65)):  # (the proven walk is slow: its round loop is the same code)
            for packet in (False, True):
                _, wst = _composition(gpu, ctx, records, k, table, base=BASE, packet=packet)
                _, st = ctx.gather(records, k, table, SEED, packet=packet, base=BASE)
                assert st == wst, (accel, exact, k, packet, st, wst)
                assert st["pixels"] == 0 and (st["cand_prims"], st["cand_entries"], st["cand_global"]) == (0, 0, 0)
                assert st["camera"] > 0 and st["closest"] >= st["camera"] and st["hit_records"] > 0
        ctx.frame_check()
        _, st1 = ctx.gather(records, 4, table, SEED, base=BASE)
        _, st2 = ctx.gather(records, 5 if exact else 65, table, SEED, base=BASE)
        flags, frames, closest, shadow = ctx.frame_check()
        assert (flags, frames) == (0, 2)
        assert (closest, shadow) == (st1["closest"] + st2["closest"], st1["shadow"] + st2["shadow"])
        ctx.close()


def test_gather_invalidates_the_kept_frame(gpu, scene_dir, shared):
    """A gather overwrites the hit records: relight and G-buffer of the frame
    before it return RT_EINVAL until the frame is rendered again, and then give
    what they gave."""
    sh = shared("spheres")
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(96, 54)
    f = s.frame()
    ctx = _ctx(gpu, s, "octree_gpu")
    ctx.set_gbuffer(True)
    ctx.set_keep_visibility(True)
    img, smp, st = ctx.render_image_gbuffer(f)
    rel, _ = ctx.relight_image(f)
    ctx.gather(sh["hits"], 4, sh["table"], SEED)
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
    assert img2.tobytes() == img.tobytes() and smp2.tobytes() == smp.tobytes() and rel2.tobytes() == rel.tobytes()
    assert (st2["closest"], st2["shadow"]) == (st["closest"], st["shadow"])
    ctx.close()


def test_gather_between_streamed_frames(gpu, scene_dir, shared):
    """Three frames streamed with overlapped list builds, a gather enqueued on
    the same stream between each pair: the frames' images, the last frame's
    counters and the side-stream builds are those of the run without, and the
    gathers' sums are brute force's composition."""
    from test_overlap_lists import STAT_KEYS, Run, _frames
    sh = shared("spheres")
    table, hits = sh["table"], sh["hits"]
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(96, 54)
    out = {}
    for with_gather in (False, True):
        run = Run(gpu, s, "octree_gpu", True)
        frames = _frames(gpu, s, run.centre, n=3)
        dev = Dev(gpu)
        d_s, d_t = dev.upload(hits), dev.upload(table)
        run.warm(frames[0])
        b0 = run.ctx.overlap_builds()
        rgbs, gout = [], []
        for k, fr in enumerate(frames):
            if with_gather and k:
                gout.append(dev.upload(np.full(3 * len(hits), FILLF, np.uint32)))
                run.ctx.gather_device(d_s, len(hits), 4, d_t, len(table), SEED, gout[-1], packet=(k == 2))
            rgbs.append(run.render(fr))
        st = run.ctx.stats()
        out[with_gather] = ([run.image(r, fr) for r, fr in zip(rgbs, frames)], {k: st[k] for k in STAT_KEYS},
                            run.ctx.overlap_builds() - b0, [dev.host(b, (len(hits), 3), np.float32) for b in gout])
        dev.close()
        run.close()
    (img0, st0, builds0, _), (img1, st1, builds1, sums) = out[False], out[True]
    assert builds0 == builds1 and builds0 >= 2
    assert st0 == st1
    for a, b in zip(img0, img1):
        assert a.tobytes() == b.tobytes()
    flat = _ctx(gpu, s, "flat")
    ref, _ = _composition(gpu, flat, hits, 4, table)
    flat.close()
    assert (ref != 0).any() and len(sums) == 2 and all(same_words(g, ref) for g in sums)


def test_live_edits(gpu, scene_dir, shared):
    """After set_lights and set_materials, and after set_triangles with one
    object of `spheres` shifted, the live context's gather equals a fresh
    context's on the edited scene, and differs from the one before."""
    sh = shared("spheres")
    hits, table = sh["hits"], sh["table"]
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(32, 18)
    ctx = _ctx(gpu, s, "octree_gpu")
    before, _ = ctx.gather(hits, 4, table, SEED)

    def fresh_gather():
        fresh = _ctx(gpu, s, "octree_gpu")
        got, st = fresh.gather(hits, 4, table, SEED)
        fresh.close()
        return got, st

    for l in s.lights():
        l.r, l.g, l.b = 0.5 * l.r, 0.25 * l.g, 0.75 * l.b
    ctx.set_lights(s.lights())
    lights, lst = ctx.gather(hits, 4, table, SEED)
    want, wst = fresh_gather()
    assert same_words(lights, want) and lst == wst and not same_words(lights, before)
    objs = (gpu.Object * int(s.s.object_count)).from_address(C.addressof(s.s.objects.contents))
    for o in objs:
        o.kd.x, o.ks.y, o.ns = 0.5 * o.kd.x + 0.125, 0.75, 17.0
    ctx.set_materials(s)
    mats, mst = ctx.gather(hits, 4, table, SEED)
    want, wst = fresh_gather()
    assert same_words(mats, want) and mst == wst and not same_words(mats, lights)
    first, count = gpu.object_range(s, 0)
    tris = s.triangles_array()
    moved = gpu.shift_triangles(tris[first:first + count], (0.0, 0.5 * float(gpu.vertex_extent(tris[first:first + count])), 0.0))
    ctx.set_triangles(moved, first)
    s.set_triangles_array(moved, first)
    geo, gst = ctx.gather(hits, 4, table, SEED)
    want, wst = fresh_gather()
    assert same_words(geo, want) and gst == wst and not same_words(geo, mats)
    ctx.close()


# ---- 7: refusals change nothing ----------------------------------------------------------------
def test_refusals_change_nothing(gpu, scene_dir, shared, records):
    """RT_EINVAL for each refusal of the contract; no refused call writes a word,
    and after each the kept frame still relights to what it gave before."""
    table = shared("spheres")["table"]
    m, n = len(table), len(records)
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(32, 18)
    f = s.frame()
    ctx = _ctx(gpu, s, "octree_gpu")
    ctx.set_keep_visibility(True)
    ctx.render_image(f)
    rel, _ = ctx.relight_image(f)
    dev = Dev(gpu)
    d_s, d_t = dev.upload(np.concatenate([records, records[:1]])), dev.upload(table)
    d_out = dev.upload(np.full(3 * n, FILLF, np.uint32))
    L = gpu.lib()

    def refused(call):
        with pytest.raises(gpu.RtError) as e:
            call()
        assert e.value.code == RT_EINVAL, e.value
        again, _ = ctx.relight_image(f)
        assert again.tobytes() == rel.tobytes()

    g = ctx.gather_device
    refused(lambda: g(0, n, 4, d_t, m, SEED, d_out))
    refused(lambda: g(d_s, n, 4, 0, m, SEED, d_out))
    refused(lambda: g(d_s, n, 4, d_t, m, SEED, 0))
    refused(lambda: g(d_s + 4, n, 4, d_t, m, SEED, d_out))  # not 8-byte aligned
    refused(lambda: g(d_s, n, 0, d_t, m, SEED, d_out))
    refused(lambda: g(d_s, n, gpu.AO_KMAX + 1, d_t, m, SEED, d_out))
    refused(lambda: g(d_s, n, 4, d_t, 0, SEED, d_out))
    refused(lambda: g(d_s, 0xfffffff8 // 4 + 1, 4, d_t, m, SEED, d_out))  # n k > RT_RAYS_MAX: nothing is dereferenced
    refused(lambda: g(d_s, 0xfffffff8 // 1024 + 1, 1024, d_t, m, SEED, d_out))
    refused(lambda: g(0, 0xfffffff8 // 4 + 1, 4, 0, m, SEED, 0))
    refused(lambda: gpu._check(L.rt_hip_gather(ctx.h, C.c_void_p(d_s), n, 0, 4, C.c_void_p(d_t), m, SEED, 2,
                                               C.c_void_p(d_out), None), "flags"))
    refused(lambda: gpu._check(L.rt_hip_gather(None, C.c_void_p(d_s), n, 0, 4, C.c_void_p(d_t), m, SEED, 0,
                                               C.c_void_p(d_out), None), "null context"))
    ctx.set_policy(1)
    with pytest.raises(gpu.RtError) as e:
        ctx.gather(records, 4, table, SEED)
    assert e.value.code == RT_EINVAL
    with pytest.raises(gpu.RtError) as e:
        g(d_s, n, 4, d_t, m, SEED, d_out)
    ctx.set_policy(0)
    assert e.value.code == RT_EINVAL
    ctx.render_image(f)  # (rt_hip_set_policy itself drops the kept masks: the frame is rendered again)
    assert ctx.relight_image(f)[0].tobytes() == rel.tobytes()
    ctx.set_count_work(True)
    with pytest.raises(gpu.RtError) as e:
        g(d_s, n, 4, d_t, m, SEED, d_out)
    ctx.set_count_work(False)
    assert e.value.code == RT_EINVAL and ctx.relight_image(f)[0].tobytes() == rel.tobytes()
    g(0, 0, 4, 0, m, SEED, 0)  # n = 0: RT_OK, nothing written, nothing dereferenced
    assert ctx.relight_image(f)[0].tobytes() == rel.tobytes()
    got0, st0 = ctx.gather(records[:0], 4, table, SEED)
    assert got0.shape == (0, 3) and all(v == 0 for v in st0.values())
    ctx.stats()
    assert (dev.host(d_out, 3 * n, np.uint32) == FILLF).all()  # no refused call wrote a word
    # a valid call after all of it is the composition, and takes the kept frame
    got, _ = ctx.gather(records, 4, table, SEED, base=BASE)
    want, _ = _composition(gpu, ctx, records, 4, table, base=BASE)
    assert same_words(got, want)
    with pytest.raises(gpu.RtError) as e:
        ctx.relight_image(f)
    assert e.value.code == RT_EINVAL
    dev.close()
    ctx.close()
