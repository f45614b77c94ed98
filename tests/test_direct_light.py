"""Direct light for caller's surface records on the GPU (include/rt_hip.h
rt_hip_direct_light; kernel csrc/rt_dlight.h): apply_light of cpu/light.c:33-100
per rt_gsample record and the mask of its unshadowed casting lights.

The reference for every colour is the oracle's apply_light and for every mask
bit its collide_dist == 0 (tests/direct_light_util.py); colours are compared as
32-bit words, a NaN as any NaN, no tolerance, no record left out.  The expected
list of pow rounding pairs is empty, as test_pow_sweep measured none.  Shapes:
32x18 casts (2,304 records) and 96x54 frames."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import direct_light_util as du
from conftest import GOLDEN, load_own_manifest, own_scene_path
from test_rays import PROVEN, Dev, _ctx

pytestmark = pytest.mark.gpu

RT_EINVAL, RT_EINEXACT = -1, -11
F32 = np.float32
FILL = 0xAB
FILL32 = FILL * 0x01010101
SURFACES = ["cube", "spheres", "island_smooth", "car-on-road", "point-light", "dir-light-shadows", "mirrors"]
# brute force, both octrees at the default slack, both under the proven walk
CONTEXTS = [("flat", False), ("octree", False), ("octree_gpu", False), ("octree", True), ("octree_gpu", True)]
CTX_IDS = [a + ("_exact" if e else "") for a, e in CONTEXTS]
assert set(PROVEN) <= set(CONTEXTS)
LIGHT_CASES = json.load(open(os.path.join(GOLDEN, "lights", "manifest.json")))["cases"]


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


def _scene(gpu, scene_dir, tmp, name, w=32, h=18):
    if name == "mirrors":
        case = next(c for c in load_own_manifest() if c["scene"] == "mirrors")
        s = gpu.Scene.load_svati(own_scene_path(case, tmp))
    else:
        s = gpu.Scene.load_svati(os.path.join(scene_dir, name + ".svati"))
    s.set_size(w, h)
    return s


def _cast(gpu, s):
    """The first-hit records of the frame's camera rays, by brute force."""
    flat = gpu.Context(s, "flat")
    o, d = gpu.camera_rays(s.frame(), "pixel")
    _, hits, _ = flat.trace_rays(o, d, shade=False)
    flat.close()
    return hits


_SHARED = {}


@pytest.fixture(scope="module")
def shared(gpu, scene_dir, tmp_path_factory):
    """Per scene at 32x18, computed once and left unchanged: the 2,304 records
    of a FLAT cast, the oracle's colours and masks of them, and FLAT's bytes."""
    tmp = tmp_path_factory.mktemp("dl_scenes")

    def get(name):
        if name not in _SHARED:
            s = _scene(gpu, scene_dir, tmp, name)
            hits = _cast(gpu, s)
            assert len(hits) == 2304
            rgb, mask = du.oracle_direct_light(s, hits)
            flat = gpu.Context(s, "flat")
            frgb, fmask, fst = flat.direct_light(hits, lit=True)
            flat.close()
            _SHARED[name] = dict(scene=s, hits=hits, rgb=rgb, mask=mask, flat=(frgb, fmask, fst))
        return _SHARED[name]
    return get


def _radius(s):
    v = s.triangles_array()[:, :3].reshape(-1, 3)
    return 0.5 * float((v.max(axis=0) - v.min(axis=0)).max())


def _deferred_host(gpu, ctx, s, rec, lights=None):
    """(record, buffered light) pairs whose P lies outside the light's proof box."""
    shades = gpu.direct_light_shades(rec, int(s.s.object_count))
    P = rec["P"][shades]
    n = 0
    for li in gpu.casting_lights(s.lights() if lights is None else lights):
        box = ctx.lightbuf_box(li)
        if box is not None:
            n += int((~((P >= box[0]) & (P <= box[1])).all(axis=1)).sum())
    return n


def _stats_shape(st, rec_shading, ncast, what, long_rays=False):
    assert st["camera"] == rec_shading and st["shadow"] == rec_shading * ncast, (what, st)
    assert st["shadow_unproven"] == 0 and st["depth_overflow"] == 0, (what, st)
    assert long_rays or st["closest_unproven"] == 0, (what, st)
    others = {k: v for k, v in st.items()
              if k not in ("camera", "shadow", "shadow_deferred", "shadow_zero_risk", "closest_unproven")}
    assert all(v == 0 for v in others.values()), (what, others)


# ---- 1: oracle parity on surfaces ----------------------------------------------------------------
@pytest.mark.parametrize("accel,exact", CONTEXTS, ids=CTX_IDS)
@pytest.mark.parametrize("name", SURFACES)
def test_oracle_parity_on_surfaces(gpu, shared, name, accel, exact):
    """Every record of the 32x18 FLAT cast: colour words and masks against the
    oracle, and the context's bytes are FLAT's.  No query leaves a proof box."""
    sh = shared(name)
    s, hits = sh["scene"], sh["hits"]
    shades = gpu.direct_light_shades(hits, int(s.s.object_count))
    assert 100 < shades.sum(), (name, int(shades.sum()))
    ctx = _ctx(gpu, s, accel, exact)
    rgb, mask, st = ctx.direct_light(hits, lit=True)
    du.assert_same(rgb, mask, sh["rgb"], sh["mask"], f"{name} {accel} exact={exact}", records=hits)
    frgb, fmask, fst = sh["flat"]
    assert rgb.tobytes() == frgb.tobytes() and mask.tobytes() == fmask.tobytes(), (name, accel, "bytes differ from FLAT's")
    ncast = len(gpu.casting_lights(s.lights()))
    _stats_shape(st, int(shades.sum()), ncast, f"{name} {accel}")
    assert (st["camera"], st["shadow"]) == (fst["camera"], fst["shadow"])
    assert not rgb[~shades].any() and not mask[~shades].any()
    if accel != "flat":
        assert ctx.info()["lightbuf_failed"] == 0 and st["shadow_deferred"] == 0 == _deferred_host(gpu, ctx, s, hits)
        assert all(ctx.lightbuf_box(li) is not None for li in gpu.casting_lights(s.lights()))
    else:
        assert st["shadow_deferred"] == 0
    if name in ("point-light", "dir-light-shadows", "spheres"):
        full = sum(1 << li for li in gpu.casting_lights(s.lights()))
        m = mask[shades]
        assert (m != full).any() and (m != 0).any(), "some points are shadowed and some are lit"
    ctx.close()


# ---- 2: the frame identity -------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["flat", "octree_gpu"])
def test_frame_identity(gpu, scene_dir, tmp_path, accel):
    """On a 96x54 scene without reflections the direct light of the G-buffer's
    records, folded, is the rendered image bit for bit: from the assembled
    host records, and on the device from rt_hip_gbuffer's tile buffer (one
    rank, and one rank of 3) with the colours assembled on the host."""
    s = _scene(gpu, scene_dir, tmp_path, "point-light", 96, 54)
    assert (gpu.scene_materials(s.ptr)[:, 11] == 0).all(), "every material has nr == 0"
    f = s.frame()
    W, H = f.width, f.height
    ctx = gpu.Context(s, accel)
    ctx.set_gbuffer(True)
    img, smp, _ = ctx.render_image_gbuffer(f)
    rgb, _, st = ctx.direct_light(smp.reshape(-1))
    got = gpu.fold_samples(rgb).reshape(H, W, 3)
    bad = np.argwhere((got.view(np.uint32) != img.view(np.uint32)).any(axis=2))
    assert len(bad) == 0, (accel, len(bad), bad[:4].tolist())
    assert st["camera"] == int((smp["prim"] >= 0).sum()) > 1000
    dev = Dev(gpu)
    for nranks, rank in ((1, 0), (3, 1)):
        per_c, per_g = gpu.tile_buffer_floats(W, H, nranks), gpu.gbuffer_tile_words(W, H, nranks)
        n = per_g // gpu.GB_WORDS
        d_c, d_g = dev.malloc(4 * per_c), dev.malloc(4 * per_g)
        d_rgb = dev.upload(np.full(12 * n + 64, FILL, np.uint8))
        ctx.render(f, rank, nranks, d_c)
        ctx.gbuffer(f, rank, nranks, d_g)
        ctx.stats()
        ctx.direct_light_device(d_g, n, d_rgb)
        ctx.stats()
        raw = dev.host(d_rgb, 12 * n + 64, np.uint8)
        assert (raw[12 * n:] == FILL).all()
        tiles = gpu.fold_samples(raw[:12 * n].view(F32).reshape(-1, 3)).reshape(-1, 64, 3)
        want = gpu.tiles_from_image_numpy(img, rank, nranks)
        assert tiles.shape == want.shape and tiles.tobytes() == want.tobytes(), (accel, nranks, rank)
        if nranks == 1:
            back = gpu.assemble_tiles_numpy(tiles[None], W, H, 1)
            assert back.tobytes() == img.tobytes()
    dev.close()
    ctx.close()


# ---- 3: off the surfaces, off the box ---------------------------------------------------------------
def _off_surface_sets(s, hits):
    """name -> records: the cast's points moved along N, far points, random normals."""
    R = F32(_radius(s))
    hit = hits[hits["prim"] >= 0]
    sets = {}
    ln = np.linalg.norm(hit["N"].astype(np.float64), axis=1, keepdims=True)
    unit = (hit["N"] / np.maximum(ln, 1e-30)).astype(F32)
    for tag, k in (("1e-3 R", F32(1e-3)), ("R/4", F32(0.25)), ("4 R", F32(4.0))):
        r = hit.copy()
        r["P"] = (hit["P"] + unit * (k * R)).astype(F32)
        sets["along N by " + tag] = r
    far = hit[:: max(1, len(hit) // 96)][:96].copy()
    for a in range(3):
        for sg in (1, -1):
            r = far.copy()
            r["P"][:, a] = F32(sg) * F32(1e6) * R
            sets[f"1e6 R along {'+' if sg > 0 else '-'}{'xyz'[a]}"] = r
    rng = np.random.default_rng(20261021)
    r = hit.copy()
    r["N"] = (rng.normal(size=(len(hit), 3)) * np.exp(rng.uniform(-3, 3, (len(hit), 1)))).astype(F32)
    sets["random normals"] = r
    return sets


def _direct_light_rc(gpu, ctx, rec, packet):
    """direct_light through the device entry point and rt_hip_stats called
    bare -> (rgb, masks, stats, the stats call's return code): the outputs of a
    call whose stats report RT_EINEXACT are compared all the same."""
    n = len(rec)
    dev = Dev(gpu)
    d_s, d_rgb, d_lit = dev.upload(rec), dev.malloc(12 * n), dev.malloc(4 * n)
    ctx.direct_light_device(d_s, n, d_rgb, d_lit, packet=packet)
    st = gpu.Stats()
    rc = gpu.lib().rt_hip_stats(ctx.h, C.byref(st))
    rgb, mask = dev.host(d_rgb, (n, 3), F32), dev.host(d_lit, n, np.uint32)
    dev.close()
    return rgb, mask, st.as_dict(), rc


@pytest.mark.parametrize("accel,exact", CONTEXTS, ids=CTX_IDS)
@pytest.mark.parametrize("name", ["spheres", "point-light"])
def test_off_the_surfaces_off_the_box(gpu, shared, name, accel, exact):
    """Points no trace produces: the oracle decides on every context; the
    queries that leave a proof box are counted, no shadow query is unproven.
    The proven walk's bound covers directions up to RT_RF_DLMAX long
    (csrc/rt_reflect.h): a walked shadow ray with a longer one -- most point
    lights' -- is counted in closest_unproven and reported as RT_EINEXACT, as
    an occlusion batch of the same ray reports it, and is still the oracle's
    answer here."""
    sh = shared(name)
    s = sh["scene"]
    key = ("off", name)
    if key not in _SHARED:
        sets = _off_surface_sets(s, sh["hits"])
        _SHARED[key] = {k: (r,) + du.oracle_direct_light(s, r) for k, r in sets.items()}
    ctx = _ctx(gpu, s, accel, exact)
    ncast = len(gpu.casting_lights(s.lights()))
    far_deferred = 0
    for tag, (rec, wrgb, wmask) in _SHARED[key].items():
        for packet in (False, True):
            rgb, mask, st, rc = _direct_light_rc(gpu, ctx, rec, packet)
            du.assert_same(rgb, mask, wrgb, wmask, f"{name} {accel} exact={exact} {tag} packet={packet}", records=rec)
            _stats_shape(st, len(rec), ncast, (name, accel, tag), long_rays=exact)
            assert rc == (RT_EINEXACT if st["closest_unproven"] else 0), (name, accel, tag, rc, st)
            assert st["closest_unproven"] <= st["shadow_deferred"], "only the walked queries can be past the walk's bound"
            want_def = 0 if accel == "flat" else _deferred_host(gpu, ctx, s, rec)
            assert st["shadow_deferred"] == want_def, (name, accel, tag, st["shadow_deferred"], want_def)
        if tag.startswith("1e6 R"):
            far_deferred += st["shadow_deferred"]
            if accel != "flat":
                assert st["shadow_deferred"] == len(rec) * ncast, "every far point is off every box"
    assert (far_deferred > 0) == (accel != "flat")
    ctx.close()


# ---- 4: where a light is -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", LIGHT_CASES, ids=[c["row"].replace(" ", "_") for c in LIGHT_CASES])
def test_where_a_light_is(gpu, case, tmp_path):
    """Every fixture of tests/golden/lights at 32x18 -- zero, tiny, denormal
    and huge directions, point lights on the geometry, 1e6 to 3e38 away: the
    cast's records against the oracle on brute force and the device octree
    (buffers on and off: the zero, huge and far shadow rays through the walks
    too).  Pins that such rays are asked like any other, on every route."""
    import light_edges_util as lu
    s = gpu.Scene.load_svati(lu.scene_path(case, tmp_path))
    hits = _cast(gpu, s)
    shades = gpu.direct_light_shades(hits, int(s.s.object_count))
    assert shades.sum() > 500
    wrgb, wmask = du.oracle_direct_light(s, hits)
    ncast = len(gpu.casting_lights(s.lights()))
    assert ncast == 1
    flat = gpu.Context(s, "flat")
    frgb, fmask, fst = flat.direct_light(hits, lit=True)
    du.assert_same(frgb, fmask, wrgb, wmask, f"{case['row']} flat", records=hits)
    _stats_shape(fst, int(shades.sum()), ncast, case["row"])
    flat.close()
    ctx = gpu.Context(s, "octree_gpu")
    for buffers in (True, False):
        ctx.set_light_buffers(buffers)
        for packet in (False, True):
            rgb, mask, st = ctx.direct_light(hits, lit=True, packet=packet)
            what = f"{case['row']} octree_gpu buffers={buffers} packet={packet}"
            du.assert_same(rgb, mask, wrgb, wmask, what, records=hits)
            assert rgb.tobytes() == frgb.tobytes() and mask.tobytes() == fmask.tobytes(), what
            _stats_shape(st, int(shades.sum()), ncast, what)
    ctx.set_light_buffers(True)
    ctx.set_exact_reflections(True)
    rgb, mask, st = ctx.direct_light(hits, lit=True)
    assert rgb.tobytes() == frgb.tobytes() and mask.tobytes() == fmask.tobytes(), case["row"]
    ctx.close()


# ---- 5: without buffers ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["spheres", "point-light"])
def test_without_buffers(gpu, shared, name):
    sh = shared(name)
    s, hits = sh["scene"], sh["hits"]
    frgb, fmask, _ = sh["flat"]
    ctx = gpu.Context(s, "octree_gpu")

    def same(what):
        rgb, mask, st = ctx.direct_light(hits, lit=True)
        assert rgb.tobytes() == frgb.tobytes() and mask.tobytes() == fmask.tobytes(), (name, what)
        assert st["shadow_unproven"] == 0
        return st

    same("default")
    ctx.set_light_buffers(False)
    assert same("buffers off")["shadow_deferred"] == 0  # no light has a buffer to leave
    assert all(ctx.lightbuf_box(li) is None for li in gpu.casting_lights(s.lights()))
    ctx.set_light_buffers(True)
    same("buffers on again")
    ctx.set_lightbuf_entry_cap(1)
    assert ctx.info()["lightbuf_failed"] > 0
    assert same("entry cap 1")["shadow_deferred"] == 0
    ctx.set_lightbuf_entry_cap(0)
    assert ctx.info()["lightbuf_failed"] == 0
    ctx.set_exact_shadows(False)
    same("slack-grown buffers")
    ctx.set_exact_shadows(True)
    same("proven buffers again")
    ctx.close()


# ---- 6: live edits ----------------------------------------------------------------------------------------
def _light_rows(s):
    return [(int(l.type), l.r, l.g, l.b, l.v.x, l.v.y, l.v.z) for l in s.lights()]


@pytest.mark.parametrize("accel", ["flat", "octree_gpu"])
def test_live_edits(gpu, shared, tmp_path, accel):
    """After set_lights (a light moved, one recoloured, none, 33 with a
    shadowed point light at index 32), set_materials and set_triangles the
    live context answers as a fresh context on the edited scene and as the
    oracle on it."""
    sh = shared("point-light")
    s, hits = sh["scene"], sh["hits"]
    base = _light_rows(s)
    ctx = gpu.Context(s, accel)
    ctx.direct_light(hits)
    pt = next(k for k, r in enumerate(base) if r[0] == 2)
    moved = list(base)
    moved[pt] = base[pt][:4] + (base[pt][4] + 1.5, base[pt][5] + 0.5, base[pt][6] - 1.0)
    recol = list(base)
    recol[pt] = (2, 0.25, 1.0, 0.5) + base[pt][4:]
    # 33 lights: 31 ambient fillers of a small colour, the casting lights, and the scene's point light last, at index 32
    many = [r for k, r in enumerate(base) if k != pt]
    many = many + [(0, 0.002, 0.001, 0.003, 0, 0, 0)] * (32 - len(many)) + [base[pt]]
    assert len(many) == 33 and many[32][0] == 2
    every = gpu.direct_light_shades(hits, int(s.s.object_count))
    for tag, rows in (("moved", moved), ("recoloured", recol), ("none", []), ("many", many), ("back", base)):
        ctx.set_lights(rows)
        rgb, mask, st = ctx.direct_light(hits, lit=True)
        with du.light_table(gpu, s, rows):
            wrgb, wmask = du.oracle_direct_light(s, hits)
            fresh = gpu.Context(s, accel)
            qrgb, qmask, qst = fresh.direct_light(hits, lit=True)
            fresh.close()
            if tag == "many":  # the light at index 32 is shadowed at some points and not at others
                L = du.oracle_lib()[0]
                o32, d32 = gpu.shadow_rays_host(hits[every][::5], rows)[-1]
                sh32 = [L.oracle_collide_dist(C.cast(s.ptr, C.c_void_p), du.Ray(du._vec(o), du._vec(d))) != 0
                        for o, d in zip(o32, d32)]
                assert any(sh32) and not all(sh32)
        du.assert_same(rgb, mask, wrgb, wmask, f"{accel} lights {tag} against the oracle", records=hits)
        assert rgb.tobytes() == qrgb.tobytes() and mask.tobytes() == qmask.tobytes() and st == qst, (accel, tag)
        if tag == "none":
            assert not rgb.any() and not mask.any() and st["shadow"] == 0 and st["camera"] > 0
        if tag == "many":
            # the mask's bits are those of lights 0..31; the colour counts the light at index 32
            assert st["shadow"] == st["camera"] * len(gpu.casting_lights(rows))
            with du.light_table(gpu, s, many[:32]):
                only = gpu.Context(s, "flat")
                r31, m31, _ = only.direct_light(hits, lit=True)
                only.close()
            assert mask.tobytes() == m31.tobytes() and rgb.tobytes() != r31.tobytes()
            assert (mask >> 31).max() == 0 or many[31][0] in (1, 2)
    # materials
    objs = (gpu.Object * int(s.s.object_count)).from_address(C.addressof(s.s.objects.contents))
    keep = [(o.kd.x, o.ks.y, o.ns) for o in objs]
    for o in objs:
        o.kd.x, o.ks.y, o.ns = 0.5 * o.kd.x + 0.125, 0.75, 17.0
    ctx.set_materials(s)
    rgb, mask, _ = ctx.direct_light(hits, lit=True)
    wrgb, wmask = du.oracle_direct_light(s, hits)
    du.assert_same(rgb, mask, wrgb, wmask, f"{accel} materials edited", records=hits)
    assert rgb.tobytes() != sh["flat"][0].tobytes() and mask.tobytes() == sh["flat"][1].tobytes()
    for o, (a, b, c) in zip(objs, keep):
        o.kd.x, o.ks.y, o.ns = a, b, c
    ctx.set_materials(s)
    # geometry: one object moved
    first, count = gpu.object_range(s, 0)
    tris = s.triangles_array()
    old = tris[first:first + count].copy()
    new = gpu.shift_triangles(old, (0.0, 0.5 * float(gpu.vertex_extent(old)), 0.0))
    ctx.set_triangles(new, first)
    s.set_triangles_array(new, first)
    try:
        rgb, mask, st = ctx.direct_light(hits, lit=True)
        wrgb, wmask = du.oracle_direct_light(s, hits)
        du.assert_same(rgb, mask, wrgb, wmask, f"{accel} geometry moved", records=hits)
        fresh = gpu.Context(s, accel)
        qrgb, qmask, qst = fresh.direct_light(hits, lit=True)
        fresh.close()
        assert rgb.tobytes() == qrgb.tobytes() and mask.tobytes() == qmask.tobytes() and st == qst
        assert mask.tobytes() != sh["flat"][1].tobytes(), "the moved object changes some shadow"
    finally:
        s.set_triangles_array(old, first)
    ctx.close()


# ---- 7: batch edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["flat", "octree_gpu"])
def test_batch_edges(gpu, shared, accel):
    """n around the item's, the streams' and the grid's edges into pre-filled
    outputs; d_lit NULL and not; three pieces equal the whole; the packet flag
    changes no byte; the edge block gives exactly zero words."""
    sh = shared("point-light")
    s = sh["scene"]
    nobj = int(s.s.object_count)
    edge, eshades = du.edge_block(gpu.GSAMPLE, nobj)
    # the edge block's shading rows get points and normals of the scene's own
    src = sh["hits"][sh["hits"]["prim"] >= 0]
    edge["P"][eshades] = src["P"][:eshades.sum()]
    assert np.array_equal(gpu.direct_light_shades(edge, nobj), eshades)
    ctx = gpu.Context(s, accel)
    # more items than a persistent grid has waves (at most 32 per CU, 256 CUs): every stream's counter hands out
    # items after the waves' first, and the streams end at different counts (rt_ray_items.h: item k in stream k % 8)
    grid_items = 32 * 256 + 9
    big = np.concatenate([edge, np.tile(sh["hits"], 1 + (64 * grid_items) // len(sh["hits"]))])[:64 * grid_items + 1]
    whole_rgb, whole_mask, st = ctx.direct_light(big, lit=True)
    wrgb = np.concatenate([np.zeros((len(edge), 3), F32), np.tile(sh["flat"][0], (1 + len(big) // 2304, 1))])[:len(big)]
    wmask = np.concatenate([np.zeros(len(edge), np.uint32), np.tile(sh["flat"][1], 1 + len(big) // 2304)])[:len(big)]
    er, em = du.oracle_direct_light(s, edge)
    wrgb[:len(edge)], wmask[:len(edge)] = er, em
    assert whole_rgb.tobytes() == wrgb.tobytes() and whole_mask.tobytes() == wmask.tobytes()
    assert not whole_rgb[:len(edge)][~eshades].view(np.uint32).any() and not whole_mask[:len(edge)][~eshades].any()
    assert whole_rgb[:len(edge)][eshades].any()
    prgb, pmask, pst = ctx.direct_light(big, lit=True, packet=True)
    assert prgb.tobytes() == whole_rgb.tobytes() and pmask.tobytes() == whole_mask.tobytes() and pst == st
    dev = Dev(gpu)
    d_s = dev.upload(big)
    for j, n in enumerate((0, 1, 63, 64, 65, 8 * 64 + 1, 2304 + len(edge), len(big))):
        for with_lit in (True, False):
            d_rgb = dev.upload(np.full(12 * n + 64, FILL, np.uint8))
            d_lit = dev.upload(np.full(4 * n + 64, FILL, np.uint8))
            ctx.direct_light_device(d_s if n else 0, n, d_rgb if n else 0, d_lit if with_lit and n else 0, packet=bool(j & 1))
            if n:
                ctx.stats()
            g_rgb, g_lit = dev.host(d_rgb, 12 * n + 64, np.uint8), dev.host(d_lit, 4 * n + 64, np.uint8)
            assert (g_rgb[12 * n:] == FILL).all() and (g_lit[4 * n:] == FILL).all(), (accel, n)
            assert g_rgb[:12 * n].tobytes() == whole_rgb[:n].tobytes(), (accel, n, with_lit)
            if with_lit:
                assert g_lit[:4 * n].tobytes() == whole_mask[:n].tobytes(), (accel, n)
            else:
                assert (g_lit == FILL).all(), (accel, n, "d_lit NULL: no mask word written")
    # three pieces
    n = 2304 + len(edge)
    cuts = [0, 100, 100 + 64 * 9 + 1, n]
    parts = [ctx.direct_light(big[a:b], lit=True) for a, b in zip(cuts, cuts[1:])]
    assert np.concatenate([p[0] for p in parts]).tobytes() == whole_rgb[:n].tobytes()
    assert np.concatenate([p[1] for p in parts]).tobytes() == whole_mask[:n].tobytes()
    dev.close()
    ctx.close()


# ---- 8: the kept frame ----------------------------------------------------------------------------------------
def test_the_kept_frame_survives(gpu, scene_dir, shared):
    sh = shared("spheres")
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(96, 54)
    f = s.frame()
    lights = [(l.type, 0.5 * l.r, 0.25 * l.g, 0.75 * l.b, l.v.x, l.v.y, l.v.z) for l in s.lights()]
    out = {}
    for with_dl in (False, True):
        ctx = gpu.Context(s, "octree_gpu")
        ctx.set_gbuffer(True)
        ctx.set_keep_visibility(True)
        img, smp, st = ctx.render_image_gbuffer(f)
        assert ctx.frame_check()[1] == 1
        if with_dl:
            part = smp.reshape(-1)[::6][:3000].copy()
            part["P"][::5] += F32(1e6)  # some off every proof box
            rgb, mask, std = ctx.direct_light(part, lit=True, packet=True)
            shades = gpu.direct_light_shades(part, int(s.s.object_count))
            ncast = len(gpu.casting_lights(s.lights()))
            _stats_shape(std, int(shades.sum()), ncast, "between render and relight")
            assert std["shadow_deferred"] == _deferred_host(gpu, ctx, s, part) > 0
            assert std["closest"] == 0 and std["hit_records"] == 0 and std["pixels"] == 0
            flat = gpu.Context(s, "flat")
            frgb, fmask, _ = flat.direct_light(part, lit=True)
            flat.close()
            assert rgb.tobytes() == frgb.tobytes() and mask.tobytes() == fmask.tobytes()
            assert ctx.frame_check()[1] == 0, "the frame check counts renders only"
            dev = Dev(gpu)
            d_gt = dev.malloc(4 * gpu.gbuffer_tile_words(f.width, f.height, 1))
            d_gs = dev.malloc(smp.nbytes)
            ctx.gbuffer(f, 0, 1, d_gt)
            ctx.assemble_gbuffer(f, d_gt, 1, d_gs)
            ctx.stats()
            again = dev.host(d_gs, smp.shape, gpu.GSAMPLE)
            dev.close()
            assert again.tobytes() == smp.tobytes()
        ctx.set_lights(lights)
        rel, strel = ctx.relight_image(f)
        out[with_dl] = (img, smp, st, rel, strel)
        ctx.close()
    (img0, smp0, st0, rel0, strel0), (img1, smp1, st1, rel1, strel1) = out[False], out[True]
    assert img0.tobytes() == img1.tobytes() and smp0.tobytes() == smp1.tobytes() and st0 == st1
    assert rel0.tobytes() != img0.tobytes() and rel0.tobytes() == rel1.tobytes()
    assert strel0 == strel1 and strel0["closest"] == st0["closest"] > 0


def test_direct_light_between_streamed_frames(gpu, scene_dir, shared):
    """Three frames streamed with overlapped list builds, a direct-light call
    enqueued on the same stream between each pair: images, counters and
    side-stream builds are those of the run without."""
    from test_overlap_lists import STAT_KEYS, Run, _frames
    sh = shared("spheres")
    hits = sh["hits"]
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(96, 54)
    out = {}
    for with_dl in (False, True):
        run = Run(gpu, s, "octree_gpu", True)
        frames = _frames(gpu, s, run.centre, n=3)
        dev = Dev(gpu)
        d_s = dev.upload(hits)
        run.warm(frames[0])
        b0 = run.ctx.overlap_builds()
        rgbs, outs = [], []
        for k, fr in enumerate(frames):
            if with_dl and k:
                outs.append((dev.upload(np.full(12 * len(hits), FILL, np.uint8)), dev.upload(np.full(4 * len(hits), FILL, np.uint8))))
                run.ctx.direct_light_device(d_s, len(hits), outs[-1][0], outs[-1][1], packet=(k == 2))
            rgbs.append(run.render(fr))
        st = run.ctx.stats()
        out[with_dl] = ([run.image(r, fr) for r, fr in zip(rgbs, frames)], {k: st[k] for k in STAT_KEYS},
                        run.ctx.overlap_builds() - b0,
                        [(dev.host(a, 12 * len(hits), np.uint8), dev.host(b, 4 * len(hits), np.uint8)) for a, b in outs])
        dev.close()
        run.close()
    (img0, st0, builds0, _), (img1, st1, builds1, got) = out[False], out[True]
    assert builds0 == builds1 and builds0 >= 2 and st0 == st1
    for a, b in zip(img0, img1):
        assert a.tobytes() == b.tobytes()
    assert len(got) == 2
    for a, b in got:
        assert a.tobytes() == sh["flat"][0].tobytes() and b.tobytes() == sh["flat"][1].tobytes()


@pytest.mark.parametrize("accel", ["flat", "octree"])
def test_batch_kinds_share_one_path(gpu, shared, accel):
    """An occlusion batch, ambient occlusion with k = 3 and with k = 65 (the
    wide kernel) and a direct-light call share the context's batch stats
    block, grid table and last-batch bookkeeping.  Each runs twice on one
    context's own stream, in two orders, stats() read after every call: every
    output word and every stats dictionary is what the same call gives as the
    first and only call on a fresh context of the same kind.  Shapes: 130
    rays / records (three items, the last partial), 45 records at k = 3 (21
    samples an item: three items, the last partial), 3 records at k = 65."""
    sh = shared("spheres")
    s = sh["scene"]
    hit = sh["hits"][sh["hits"]["prim"] >= 0]
    assert len(hit) >= 130
    every = len(hit) // 130
    o, d = gpu.camera_rays(s.frame(), "pixel")
    o, d = o[::17][:130], d[::17][:130]
    tmax = np.where(np.arange(130) % 3 == 0, F32(np.inf), F32(2.0) * F32(_radius(s))).astype(F32)
    table = gpu.ao_table(16, 7)
    rec_dl, rec_ao, rec_wide = hit[::every][:130], hit[1::2 * every][:45], hit[2::40][:3]
    assert len(o) == len(rec_dl) == 130 and len(rec_ao) == 45 and len(rec_wide) == 3
    dev = Dev(gpu)
    d_o, d_d, d_t, d_tab = dev.upload(o), dev.upload(d), dev.upload(tmax), dev.upload(table)
    d_dl, d_ao, d_wide = dev.upload(rec_dl), dev.upload(rec_ao), dev.upload(rec_wide)

    def occl(ctx):
        d_out = dev.upload(np.full(130, FILL, np.uint8))
        ctx.occluded_device(d_o, d_d, d_t, 130, d_out)
        return ctx.stats(), [dev.host(d_out, 130, np.uint8)]

    def ao(ctx, d_rec, n, k):
        d_out = dev.upload(np.full(n, FILL32, np.uint32))
        ctx.ambient_occlusion_device(d_rec, n, k, d_tab, len(table), 5, d_out, tmax=_radius(s))
        return ctx.stats(), [dev.host(d_out, n, np.uint32)]

    def dl(ctx):
        d_rgb, d_lit = dev.upload(np.full(3 * 130, FILL32, np.uint32)), dev.upload(np.full(130, FILL32, np.uint32))
        ctx.direct_light_device(d_dl, 130, d_rgb, d_lit)
        return ctx.stats(), [dev.host(d_rgb, 3 * 130, np.uint32), dev.host(d_lit, 130, np.uint32)]

    calls = {"occluded": occl, "ao k=3": lambda c: ao(c, d_ao, 45, 3), "ao k=65": lambda c: ao(c, d_wide, 3, 65),
             "direct light": dl}
    alone = {}
    for what, call in calls.items():
        ctx = gpu.Context(s, accel)
        alone[what] = call(ctx)
        ctx.close()
    assert alone["occluded"][0]["shadow"] > 0 and alone["ao k=3"][0]["shadow"] > 0 and alone["ao k=65"][0]["shadow"] > 0
    assert alone["direct light"][0]["camera"] > 0 and alone["occluded"][1][0].max() == 1
    assert len({json.dumps(st, sort_keys=True) for st, _ in alone.values()}) >= 3, "a stale stats block would show"
    ctx = gpu.Context(s, accel)
    order = list(calls)
    for what in order + order[::-1]:
        st, outs = calls[what](ctx)
        assert st == alone[what][0], (accel, what, st, alone[what][0])
        for got, want in zip(outs, alone[what][1]):
            assert got.tobytes() == want.tobytes(), (accel, what)
    ctx.close()
    dev.close()


# ---- 9: refusals ----------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(gpu, shared):
    sh = shared("spheres")
    s, hits = sh["scene"], sh["hits"]
    n = len(hits)
    ctx = gpu.Context(s, "octree_gpu")
    before = ctx.direct_light(hits, lit=True)
    dev = Dev(gpu)
    d_s = dev.upload(np.concatenate([hits, hits[:1]]))
    d_rgb, d_lit = dev.upload(np.full(12 * n, FILL, np.uint8)), dev.upload(np.full(4 * n, FILL, np.uint8))
    L = gpu.lib()

    def refused(call):
        with pytest.raises(gpu.RtError) as e:
            call()
        assert e.value.code == RT_EINVAL, e.value
        got = ctx.direct_light(hits, lit=True)
        assert got[0].tobytes() == before[0].tobytes() and got[1].tobytes() == before[1].tobytes() and got[2] == before[2]

    dl = ctx.direct_light_device
    refused(lambda: dl(0, n, d_rgb, d_lit))
    refused(lambda: dl(d_s, n, 0, d_lit))
    refused(lambda: dl(d_s + 4, n, d_rgb, d_lit))  # not 8-byte aligned
    refused(lambda: dl(d_s, 0xfffffff8 + 1, d_rgb, d_lit))  # n > RT_RAYS_MAX: nothing is dereferenced
    refused(lambda: gpu._check(L.rt_hip_direct_light(ctx.h, C.c_void_p(d_s), n, 2, C.c_void_p(d_rgb), C.c_void_p(d_lit), None), "flags"))
    refused(lambda: gpu._check(L.rt_hip_direct_light(ctx.h, C.c_void_p(d_s), n, 3, C.c_void_p(d_rgb), None, None), "flags"))
    refused(lambda: gpu._check(L.rt_hip_direct_light(None, C.c_void_p(d_s), n, 0, C.c_void_p(d_rgb), None, None), "null context"))
    refused(lambda: gpu._check(L.rt_hip_direct_light_host(None, hits.ctypes.data_as(C.c_void_p), n, 0, None, None, None), "null"))
    ctx.set_policy(1)
    with pytest.raises(gpu.RtError) as e:
        dl(d_s, n, d_rgb, d_lit)
    ctx.set_policy(0)
    assert e.value.code == RT_EINVAL
    ctx.set_count_work(True)
    with pytest.raises(gpu.RtError) as e:
        dl(d_s, n, d_rgb, d_lit)
    ctx.set_count_work(False)
    assert e.value.code == RT_EINVAL
    # (a context left broken by a failed geometry update cannot be made from
    # outside: the refusal is the guard every entry point shares, RT_CTX_LIVE)
    dl(0, 0, 0, 0)  # n = 0: RT_OK, nothing written, nothing dereferenced
    ctx.stats()
    assert (dev.host(d_rgb, 12 * n, np.uint8) == FILL).all() and (dev.host(d_lit, 4 * n, np.uint8) == FILL).all()
    got = ctx.direct_light(hits, lit=True)
    assert got[0].tobytes() == before[0].tobytes() and got[1].tobytes() == before[1].tobytes()
    dev.close()
    ctx.close()
