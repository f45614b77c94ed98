"""Ties, axis-parallel rays, the two thresholds of cpu/hit.c and geometry
around the eye, on the GPU (fixtures: tests/golden/make_golden_adversarial.py;
ray sets: tests/adversarial_util.py).

Every other GPU test keeps the camera outside the geometry, sends no ray with
a zero direction component and holds no two coinciding triangles.  Here every
hit of `twins` is an exact tie, `room` surrounds eye, film and point light, and
`slivers` holds zero-area triangles, needles and triangles whose `a` crosses
1e-7.  The suite's rule holds throughout: bit-exact (0 ULP) against the
reference's goldens and the oracle, with the reference's query counts; the
default slack walk gets the existing allowance only (coplanar-grazing at the
first differing query, at most 64 rays per scene)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import adversarial_util as adv
from test_occlusion import _mixed
from test_rays import PROVEN, _ctx, _diff_rays, _first_difference_explained, _same

pytestmark = pytest.mark.gpu

CASES = adv.load_manifest()
BY_ID = {adv.case_id(c): c for c in CASES}
ACCELS = ["flat", "octree", "octree_gpu"]
OCTREES = ["octree", "octree_gpu"]
TRAV = [0, 1, 2, 3]  # test_gpu.py's traversal policies
INF = np.float32(np.inf)
sys.path.insert(0, os.path.join(adv.REPO, "tools"))


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


@pytest.fixture(scope="module")
def scenes(gpu, tmp_path_factory):
    """name -> (scene, case, golden image), loaded once."""
    tmp, out = tmp_path_factory.mktemp("adversarial"), {}

    def get(name):
        if name not in out:
            case = BY_ID[name]
            out[name] = (gpu.Scene.load_svati(adv.scene_path(case, tmp)), case, adv.golden(case))
        return out[name]
    return get


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_frame(img, st, gold, case, what):
    bad = np.argwhere((_bits(img) != _bits(gold)).any(axis=2))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ from the golden, first (row, col) {bad[:4].tolist()}"
    assert (st["closest"], st["shadow"]) == (case["closest"], case["shadow"]), what
    assert st["depth_overflow"] == 0 and st["zero_normal"] == 0 and st["shadow_zero_risk"] == 0, what


# ---- 1: frames ---------------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", list(BY_ID))
def test_frames_bitexact(gpu, scenes, name, accel):
    """render_image == the reference's golden with its query counts; on the
    octrees also with exact reflections (nothing unproven), under every
    traversal policy and with the camera refinement off."""
    s, case, gold = scenes(name)
    f = s.frame()
    ctx = gpu.Context(s, accel)
    img, st = ctx.render_image(f)
    _assert_frame(img, st, gold, case, f"{name}/{accel}")
    if accel == "flat":
        return
    ctx.set_exact_reflections(True)
    img, st = ctx.render_image(f)
    _assert_frame(img, st, gold, case, f"{name}/{accel}/exact reflections")
    assert st["closest_unproven"] == 0
    ctx.set_exact_reflections(False)
    for trav in TRAV[1:]:
        ctx.set_policy(trav)
        img, st = ctx.render_image(f)
        _assert_frame(img, st, gold, case, f"{name}/{accel}/policy {trav}")
    ctx.set_policy(0)
    ctx.set_camera_refine(False)
    img, st = ctx.render_image(f)
    _assert_frame(img, st, gold, case, f"{name}/{accel}/refinement off")


# ---- 2: winners, not only colours ---------------------------------------------------
_WINNERS = {}


def _winners(gpu, s, name):
    if name not in _WINNERS:
        o, d = gpu.camera_rays(s.frame(), "pixel")
        _WINNERS[name] = adv.oracle_collide(s, o, d)
    return _WINNERS[name]


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", ["twins_32x18", "room_32x18", "slivers_32x18"])
def test_gbuffer_winners(gpu, scenes, name, accel):
    """Every sample's obj, P and N == oracle_collide's on the frame's camera
    rays, bit for bit; on twins the winning triangle is the earlier object's."""
    s, case, gold = scenes(name)
    f = s.frame()
    obj, P, N = _winners(gpu, s, name)
    img, smp, st = gpu.Context(s, accel).render_image_gbuffer(f)
    _assert_frame(img, st, gold, case, f"{name}/{accel}/gbuffer")
    smp = smp.reshape(-1)
    for what, got, want in (("hit", smp["prim"] >= 0, obj >= 0), ("obj", smp["obj"], obj),
                            ("P bits", _bits(smp["P"]), _bits(P)), ("N bits", _bits(smp["N"]), _bits(N))):
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{name}/{accel}: {what} differs at {len(bad)} places, first (sample, ..) {bad[:4].tolist()}"
    assert (obj >= 0).any()
    if case["scene"] == "twins":
        owner = np.array([gpu.prim_object_triangle(s, int(p))[0] for p in smp["prim"]])
        hit = smp["prim"] >= 0
        assert (owner[hit] % 2 == 0).all(), f"a later twin won {int((owner[hit] % 2).sum())} samples"
        assert set(np.unique(owner[hit])) == {0, 2, 4}


# ---- 3, 4: ray batches ----------------------------------------------------------------
BATCHES = [("twins_32x18", k) for k in ("lattice+0", "lattice-0", "diagonal", "inside", "threshold")] + \
          [("slivers_96x54", "slivers")]
_BATCH = {}


@pytest.fixture(scope="module")
def batches(gpu, scenes):
    """(scene name, set) -> rays, the oracle's collide and collide_dist per ray
    and brute force's colours and samples, computed once."""
    def get(name, which):
        if (name, which) not in _BATCH:
            s, case, _ = scenes(name)
            o, d = adv.sliver_rays(s, case) if which == "slivers" else adv.twins_ray_sets()[which]
            assert len(o) <= 25000
            flat = gpu.Context(s, "flat")
            rgb, smp, st = flat.trace_rays(o, d, samples=True)
            assert st["depth_overflow"] == 0 and flat.last_rc == 0
            _BATCH[(name, which)] = dict(scene=s, o=o, d=d, ref=adv.oracle_collide(s, o, d), D=adv.oracle_dists(s, o, d),
                                         rgb=rgb, smp=smp, R=np.float32(flat.info()["scene_radius"]))
            flat.close()
        return _BATCH[(name, which)]
    return get


def _first_hits_match(smp, ref, what):
    obj, P, N = ref
    for field, got, want in (("hit", smp["prim"] >= 0, obj >= 0), ("obj", smp["obj"], obj),
                             ("P bits", _bits(smp["P"]), _bits(P)), ("N bits", _bits(smp["N"]), _bits(N))):
        bad = np.flatnonzero((got != want).reshape(len(obj), -1).any(axis=1))
        assert len(bad) == 0, f"{what}: {field} differs from oracle_collide on {len(bad)} rays, first {bad[:5].tolist()}"


@pytest.mark.parametrize("name,which", BATCHES, ids=[f"{n}-{w}" for n, w in BATCHES])
def test_ray_batches_first_hits_are_the_oracles(gpu, batches, name, which):
    """Brute force's first hit per ray == oracle_collide's (hit / miss, obj, P,
    N); both proven octree walks == brute force byte for byte, colours and
    samples, with nothing unproven."""
    b = batches(name, which)
    _first_hits_match(b["smp"], b["ref"], f"{name}/{which}/flat")
    hit = b["ref"][0] >= 0
    if which == "slivers":  # aimed at the slivers: some land on theirs, the others on what lies behind
        assert (b["ref"][0] == 0).any() and (b["ref"][0] > 0).any()
    else:
        assert hit.any() and not hit.all(), "the set must hit and miss"
    if which == "threshold":  # nine floats below the threshold miss, eight above it hit
        assert np.array_equal(hit.reshape(2, 4, 17), np.broadcast_to(np.arange(17) >= 9, (2, 4, 17)))
    if name.startswith("twins"):
        assert (b["ref"][0][hit] % 2 == 0).all()
    for accel, exact in PROVEN[1:]:
        ctx = _ctx(gpu, b["scene"], accel, exact)
        rgb, smp, st = ctx.trace_rays(b["o"], b["d"], samples=True)
        assert _same(rgb, b["rgb"]) and _same(smp, b["smp"]), \
            (name, which, accel, _diff_rays(rgb, smp, b["rgb"], b["smp"])[:5])
        assert st["closest_unproven"] == 0 and st["depth_overflow"] == 0 and ctx.last_rc == 0
        ctx.close()


@pytest.mark.parametrize("accel,packet", [("octree", False), ("octree_gpu", False), ("octree_gpu", True)])
def test_ray_batches_default_walk_against_brute_force(gpu, batches, accel, packet):
    """The default slack walk (and the packet walk of the first query) on the
    same sets against brute force: a differing ray is the coplanar-grazing
    class at its first differing query, at most 64 per scene.  Rays inside a
    triangle's plane (a == 0 exactly) are rejected by both and need no allowance."""
    figures = {}
    for name, which in BATCHES:
        b = batches(name, which)
        s = b["scene"]
        walk = _ctx(gpu, s, accel)
        rgb, smp, st = walk.trace_rays(b["o"], b["d"], samples=True, packet=packet)
        assert st["closest_unproven"] == 0 and st["depth_overflow"] == 0 and walk.last_rc == 0
        bad = _diff_rays(rgb, smp, b["rgb"], b["smp"])
        total, differ = figures.get(name, (0, 0))
        figures[name] = (total + len(b["o"]), differ + len(bad))
        if len(bad):
            flat = _ctx(gpu, s, "flat")
            tri, nr = s.triangles_array(), gpu.scene_materials(s.ptr)[:, 11]
            unexplained = [int(i) for i in bad[:64]
                           if not _first_difference_explained(gpu, walk, flat, tri, nr, b["o"][i], b["d"][i])]
            assert not unexplained, (name, which, len(bad), unexplained[:5])
            flat.close()
        walk.close()
    for name, (total, differ) in figures.items():
        assert differ <= 64, (name, differ)
        print(f"{name} {accel}{' packet' if packet else ''} slack walk: {total} rays, {differ} differ from brute force, "
              f"all coplanar-grazing")


@pytest.mark.parametrize("accel,exact", PROVEN, ids=[a for a, _ in PROVEN])
@pytest.mark.parametrize("name,which", BATCHES, ids=[f"{n}-{w}" for n, w in BATCHES])
def test_occlusion_the_oracle_decides(gpu, batches, name, which, accel, exact):
    """byte = (D != 0 && D <= tmax), D the oracle's collide_dist, for tmax
    unbounded, exactly D, one ulp below, one ulp above and R/4."""
    b = batches(name, which)
    o, d, D, R = b["o"], b["d"], b["D"], b["R"]
    if which.startswith("lattice") or which == "threshold":
        _mixed(D != 0, (name, which))
    ctx = _ctx(gpu, b["scene"], accel, exact)
    rounds = {"none": None, "D": D, "below": np.nextafter(D, np.float32(0)), "above": np.nextafter(D, INF),
              "R/4": np.full(len(D), R / np.float32(4), np.float32)}
    for what, tmax in rounds.items():
        got, st = ctx.occluded(o, d, tmax)
        want = (D != 0) & (D <= (INF if tmax is None else tmax))
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (name, which, accel, what, len(bad), bad[:5], D[bad[:5]])
        assert st["shadow_zero_risk"] == 0 and ctx.last_rc == 0 and st["closest_unproven"] == 0
    ctx.close()


def test_occlusion_packet_default_walk_against_brute_force(gpu, batches):
    """The bounded default walk with the packet flag against brute force:
    nothing occluded that brute force calls free; what it misses is the
    coplanar-grazing class on brute force's winner, at most 64 per scene."""
    from grazing import coplanar_grazing
    missed = {}
    for name, which in BATCHES:
        b = batches(name, which)
        s, o, d = b["scene"], b["o"], b["d"]
        walk, flat = _ctx(gpu, s, "octree_gpu"), _ctx(gpu, s, "flat")
        for tmax in (None, np.float32(b["R"] / np.float32(4))):
            gw, stw = walk.occluded(o, d, tmax, packet=True)
            gf, _ = flat.occluded(o, d, tmax)
            assert stw["depth_overflow"] == 0 and walk.last_rc == 0
            extra = np.flatnonzero((gw == 1) & (gf == 0))
            assert len(extra) == 0, (name, which, tmax, extra[:5])
            miss = np.flatnonzero((gw == 0) & (gf == 1))
            missed[name] = missed.get(name, 0) + len(miss)
            if len(miss):
                tri = s.triangles_array()
                _, cast, _ = flat.trace_rays(o[miss], d[miss], shade=False)
                lim = INF if tmax is None else tmax
                unexplained = [int(i) for k, i in enumerate(miss)
                               if not (cast["prim"][k] >= 0 and cast["dist"][k] <= lim and
                                       coplanar_grazing(tri[cast["prim"][k]], o[i], d[i]))]
                assert not unexplained, (name, which, tmax, unexplained[:5])
        walk.close()
        flat.close()
    for name, n in missed.items():
        assert n <= 64, (name, n)
        print(f"{name} octree_gpu packet bounded slack walk: {n} occluded by brute force only, all coplanar-grazing")


# ---- 5: shadows --------------------------------------------------------------------------
# (light buffers, exact shadows): proven buffers, the proven walk, slack-grown buffers
SHADOW_MODES = [("proven buffers", True, True), ("proven walk", False, True), ("slack buffers", True, False)]


@pytest.mark.parametrize("accel", OCTREES)
@pytest.mark.parametrize("name", ["twins_32x18", "room_32x18", "room_96x54"])
def test_shadow_queries_match_brute_force(gpu, scenes, name, accel):
    """Shadow rays of every light from the frame's first-hit points -- inside
    the room the point light's cone covers every direction -- through the
    light buffers (proven, slack) against brute force, and every shadow query
    of the frame (buffers, or the walk with the buffers off) against brute
    force on the same hit records: 0 differ in the proven modes.  The build
    succeeded or fell back loudly, and the frame is the golden either way."""
    s, case, gold = scenes(name)
    f = s.frame()
    o, d = gpu.camera_rays(f, "pixel")
    flat = gpu.Context(s, "flat")
    _, cast, _ = flat.trace_rays(o, d, shade=False)
    flat.close()
    org = np.ascontiguousarray(cast["P"][cast["prim"] >= 0])
    assert len(org) > 500
    lights = [i for i in range(int(s.s.light_count)) if int(s.s.lights[i].type) in (1, 2)]
    assert len(lights) == 2
    for mode, lbuf, exact in SHADOW_MODES:
        ctx = gpu.Context(s, accel)
        ctx.set_light_buffers(lbuf)
        ctx.set_exact_shadows(exact)
        info = ctx.info()
        if info["lightbuf_failed"]:
            assert info["lightbuf_fail_reason"], "a failed light-buffer build must say why"
            print(f"{name}/{accel}/{mode}: light buffers fell back: {info['lightbuf_fail_reason']}")
        img, st = ctx.render_image(f)
        if exact:
            _assert_frame(img, st, gold, case, f"{name}/{accel}/{mode}")
        v = ctx.verify_shadows(1)
        assert v["records"] > 500 and v["queries"] == 2 * v["records"], v
        print(f"{name}/{accel}/{mode}: {v}")
        if exact:
            assert v["records_differ"] == 0 and v["walk_lit_brute_shadowed"] == 0, (name, accel, mode, v)
        if lbuf and not info["lightbuf_failed"]:  # (the probe reads the buffers)
            assert info["lightbuf_entries"] + info["lightbuf_global"] > 0
            for li in lights:
                brute = ctx.probe_shadows(li, org, brute=True)
                got = ctx.probe_shadows(li, org, brute=False)
                differ = int((got != brute).sum())
                print(f"{name}/{accel}/{mode}: light {li}, {len(org)} shadow rays, {round(float(brute.mean()), 3)} "
                      f"shadowed, {differ} differ from brute force")
                if exact:
                    assert differ == 0, (name, accel, mode, li, differ, np.flatnonzero(got != brute)[:5])
                if name.startswith("room") and int(s.s.lights[li].type) == 2:
                    assert 0.05 < brute.mean() < 0.95  # the point light's rays: blocked and free
        ctx.close()


# ---- 6: lists on the device ------------------------------------------------------------------
def _render_rank(gpu, ctx, f, rank, nranks):
    L = gpu.lib()
    d = C.c_void_p()
    assert L.rt_hip_malloc(0, gpu.tile_buffer_floats(f.width, f.height, nranks) * 4, C.byref(d)) == 0
    try:
        ctx.render(f, rank, nranks, d.value)
        return ctx.stats()
    finally:
        L.rt_hip_free(d)


@pytest.mark.parametrize("accel", OCTREES)
@pytest.mark.parametrize("name", ["twins_96x54", "room_96x54", "slivers_96x54"])
def test_candidate_lists_match_host(gpu, scenes, name, accel):
    """The device-built camera candidate lists == the host re-derivation:
    every listed footprint bit for bit and every tile's list as a multiset, on
    one rank and on rank 1 of 3 -- with triangles across the eye plane, twins
    and zero-area triangles among them (those two are global: no footprint)."""
    s, case, _ = scenes(name)
    f = s.frame()
    ctx = gpu.Context(s, accel)
    for nranks, rank in ((1, 0), (3, 1)):
        _render_rank(gpu, ctx, f, rank, nranks)
        v = ctx.cand_verify(f, rank, nranks)
        assert v["listed"] > 0 and v["entries"] > 0, (nranks, rank, v)
        assert v["fp_mismatch"] == 0 and v["tile_mismatch"] == 0, (nranks, rank, v)
        assert v["filter_violation"] == 0, (nranks, rank, v)
        assert v["global"] == (2 if case["scene"] == "slivers" else 0), (nranks, rank, v)


# ---- 7: rank split and compatibility mode -------------------------------------------------------
@pytest.mark.parametrize("name", ["room_96x54", "twins_96x54"])
def test_three_ranks_gathered(gpu, scenes, name):
    """Rank-sharded renders + rank-major gather + assemble == the golden."""
    s, case, gold = scenes(name)
    f = s.frame()
    nranks = 3
    ctx = gpu.Context(s, "octree")
    per = gpu.tile_buffer_floats(f.width, f.height, nranks)
    L = gpu.lib()
    dg, drgb = C.c_void_p(), C.c_void_p()
    assert L.rt_hip_malloc(0, per * nranks * 4, C.byref(dg)) == 0
    assert L.rt_hip_malloc(0, f.width * f.height * 12, C.byref(drgb)) == 0
    tot = {"closest": 0, "shadow": 0}
    try:
        for r in range(nranks):
            ctx.render(f, r, nranks, dg.value + r * per * 4)
            st = ctx.stats()
            tot["closest"] += st["closest"]
            tot["shadow"] += st["shadow"]
        ctx.assemble(f, dg.value, nranks, drgb.value)
        img = np.empty((f.height, f.width, 3), np.float32)
        ctx.stats()  # sync
        assert L.rt_hip_memcpy_d2h(img.ctypes.data_as(C.c_void_p), drgb, img.nbytes) == 0
    finally:
        L.rt_hip_free(dg)
        L.rt_hip_free(drgb)
    bad = np.argwhere((_bits(img) != _bits(gold)).any(axis=2))
    assert len(bad) == 0, f"{name}: {len(bad)} pixels differ, first {bad[:4].tolist()}"
    assert (tot["closest"], tot["shadow"]) == (case["closest"], case["shadow"])


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", ["twins_32x18", "room_32x18"])
def test_compat_matches_oracle(gpu, scenes, name, accel):
    """rt_hip_render_compat == the oracle's restatement of gpu/rt, byte for
    byte, with its query counts."""
    import oracle as orc
    s, case, _ = scenes(name)
    W, H = case["width"], case["height"]
    img, st = gpu.Context(s, accel).render_compat(s.camera)
    ref, cnt = orc.render_gpu(s.ptr, W, H, threads=8)
    bad = np.argwhere((img != ref).any(axis=2))
    assert len(bad) == 0, f"{name} {accel}: {len(bad)} pixels differ, first {bad[:4].tolist()}"
    assert (st["closest"], st["shadow"]) == (cnt["closest"], cnt["shadow"])
    assert cnt["closest"] > W * H
