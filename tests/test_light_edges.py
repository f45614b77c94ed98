"""Where a light is, on the device: every row of tests/light_edges_util.py's
table -- axis-aligned, tied, tiny, denormal, huge and zero directions; point
lights on the scene's lattice, on a vertex, in a wall's plane, on a corner of
the triangle box, inside a closed box and 1e6 to 3e38 away -- through the
device build of the light buffers (count, sort, start table, global list),
the shade kernel's scan and the walks.

The conditions that keep these tests from passing by exercising nothing are
conditions on the inputs: shares are measured on the brute-force answer and
equal what the oracle's collide_dist gave when the fixtures were made
(tests/test_light_edges_host.py checks them without a GPU).  The lattice
frames are the reference's own (tests/golden/lights/).

Why the zero, tiny, denormal and huge directions terminate and stay in bounds
on every route is argued from the code in DESIGN.md §2 ("Where a light is").
Left out: non-finite lights (lb_derive_grid refuses them on the host,
tests/test_lightbuf_geom.py; nothing of them goes to a device) and the probe
through a buffer the light does not have (rt_hip_probe_shadows refuses it:
the zero direction, the buffers switched off, a capped build -- those routes
are walked by the frame tests and checked by verify_shadows)."""
import os
import sys

import numpy as np
import pytest

import light_edges_util as lu

pytestmark = pytest.mark.gpu
F32 = np.float32
MANIFEST = {c["row"]: c for c in lu.load_manifest()["cases"]}
ROW_IDS = [lu.row_slug(n) for n in lu.ROW_NAMES]
FAR = ["point 1e6 0 0", "point 1e6 1e6 1e6", "point 0 1e9 0", "point 3e38"]


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


def _same(got, want, what):
    lu.assert_same_words(got, want, what)


def _lattice(row, tmp_path, w=lu.W, h=lu.H):
    import rtgpu
    if (w, h) == (lu.W, lu.H):  # the committed text itself
        return rtgpu.Scene.load_svati(lu.scene_path(MANIFEST[row[0]], tmp_path))
    return lu.load_scene(tmp_path, lu.row_lights(row), w, h, name=f"{lu.row_slug(row[0])}_{w}")


def _surveyed(s, exact):
    """Host survey of every light that gets a buffer: (entries, global, [per light])."""
    import rtgpu
    per = []
    for li in range(int(s.s.light_count)):
        if int(s.s.lights[li].type) not in (1, 2):
            continue
        try:
            per.append(s.lightbuf_survey(li, exact, 1))
        except rtgpu.RtError:  # no grid: the light has no buffer
            per.append(None)
    return sum(h["entries"] for h in per if h), sum(h["global"] for h in per if h), per


def _check_verify(ctx, what):
    v = ctx.verify_shadows(1)
    assert v["records"] > 0 and v["queries"] > 0, (what, v)
    assert v["records_differ"] == 0 and v["walk_lit_brute_shadowed"] == 0, (what, v)


# ---- the probe ----------------------------------------------------------------------------------
@pytest.mark.parametrize("row", lu.ROWS, ids=ROW_IDS)
def test_probe_lattice(gpu, row, tmp_path):
    """The light buffer's answer equals brute force on every lattice origin and
    on its float neighbours, on the device-built and the host-built tree, with
    slack-grown and with proven footprints; brute force gives the oracle's
    count, and the row's share condition holds on it."""
    s = _lattice(row, tmp_path)
    o = lu.origins()
    want = MANIFEST[row[0]]["observed"]
    for accel in ("octree_gpu", "octree"):
        for exact in (False, True):
            ctx = gpu.Context(s, accel)
            ctx.set_exact_shadows(exact)
            what = f"{row[0]} {accel} exact={exact}"
            ref = ctx.probe_shadows(1, o, brute=True)
            share = lu.check_share(row, ref)
            print(what, "brute-force share", share)
            assert int(ref.sum()) == want["shadowed"] and len(o) == want["origins"], what
            if row[0] == "dir zero":  # no grid: nothing to probe through, the frame tests walk it
                with pytest.raises(gpu.RtError, match="no buffer"):
                    ctx.probe_shadows(1, o)
                assert ctx.info()["lightbuf_failed"] == 1 and "zero vector" in ctx.info()["lightbuf_fail_reason"]
                continue
            got = ctx.probe_shadows(1, o)
            bad = np.flatnonzero(got != ref)
            assert len(bad) == 0, (f"{what}: {len(bad)} of {len(o)} origins differ from brute force (buffer lit, "
                                   f"brute shadowed: {int((~got & ref).sum())}); first {o[bad[:3]].tolist()}")
            assert ctx.info()["lightbuf_failed"] == 0
            e, g, _ = _surveyed(s, exact)
            assert (ctx.info()["lightbuf_entries"], ctx.info()["lightbuf_global"]) == (e, g), what
            if accel == "octree_gpu" and not exact:
                ctx.set_light_buffers(False)  # no buffer to probe through: refused, not answered by something else
                with pytest.raises(gpu.RtError, match="no light buffers"):
                    ctx.probe_shadows(1, o)


def _synthetic(gpu, row, w=96, h=54):
    """The sphere field with the row's light in the slot of its type."""
    s = gpu.Scene.synthetic(3, 3, 9776, seed=0x5EED, width=w, height=h)
    tri = s.triangles_array()
    if lu.leaves_downwards(row):
        # the ground quad (prims 0 and 1) spans the field and takes every ray that leaves downwards: shrunk
        # to a quarter under the middle sphere, the spheres decide
        g = tri[:2].copy()
        assert (g[:, :3, 1] == 0).all() and (tri[2:, :3, 1] >= 0).all()
        c = np.array(lu.GROUND_C, F32)
        g[:, :3] = c + (g[:, :3] - c) * F32(lu.GROUND_SHRINK)
        s.set_triangles_array(g, 0)
        tri = s.triangles_array()
    v = tri[:, :3].reshape(-1, 3)
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    li = next(k for k in range(int(s.s.light_count)) if int(s.s.lights[k].type) == row[1])
    L = s.s.lights[li]
    L.v.x, L.v.y, L.v.z = lu.place(row, lo, hi)
    return s, tri, li, np.array([L.v.x, L.v.y, L.v.z], np.float64), lo, hi


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("row", [r for r in lu.ROWS if r[0] not in lu.FIELD_LEFT_OUT],
                         ids=[lu.row_slug(r[0]) for r in lu.ROWS if r[0] not in lu.FIELD_LEFT_OUT])
def test_probe_synthetic_grazing(gpu, row, exact):
    """Curved meshes, many cells, big footprints: shadow rays built to graze
    the sphere field's triangles under the row's light (tools/grazing.py; the
    origins of a direction of no usable length, or of a light too far to step
    towards, are made with the unit direction towards the light).  The near
    point rows keep their role on the field (light_edges_util.FIELD_POINTS),
    the two directions that leave downwards get a ground that does not take
    every ray, and every row's share condition is asserted on brute force:
    exactly 0, exactly 1 around the light inside the closed middle sphere,
    strictly between 1 % and 99 % otherwise.  Two rows are left out
    (light_edges_util.FIELD_LEFT_OUT says why)."""
    sys.path.insert(0, os.path.join(lu.REPO, "tools"))
    from grazing import grazing_origins
    s, tri, li, lv, lo, hi = _synthetic(gpu, row)
    c, R = 0.5 * (lo + hi), 0.5 * float((hi - lo).max())
    if row[1] == lu.DIRECTIONAL:
        n = float(np.linalg.norm(lv))
        o = grazing_origins(tri, 1, lv if 0.25 <= n <= 4.0 else lv / n, 2500, 20)
    elif np.linalg.norm(lv - c) > 100.0 * R:
        u = (lv - c) / np.linalg.norm(lv - c)
        o = grazing_origins(tri, 1, -u, 2500, 20)
    else:
        o = grazing_origins(tri, 2, lv, 2500, 20)
    assert len(o) > 10000, len(o)
    ctx = gpu.Context(s, "octree_gpu")
    ctx.set_exact_shadows(exact)
    got = ctx.probe_shadows(li, o)
    ref = ctx.probe_shadows(li, o, brute=True)
    share = float(ref.mean())
    print(row[0], "exact" if exact else "slack", len(o), "origins, brute-force share", share)
    if row[4] == lu.NOTHING:
        if row[1] == lu.POINT:  # t = distance / |d| stays below 1e-7 across the whole field
            assert 4.0 * R / np.linalg.norm(lv - c) < 1e-7
        assert share == 0.0, share
    elif row[4] == lu.ENCLOSED:  # every ray to a light inside a closed sphere crosses the sphere
        assert share == 1.0, share
    else:
        assert 0.01 < share < 0.99, share
    bad = np.flatnonzero(got != ref)
    assert len(bad) == 0, (f"{len(bad)} of {len(o)} grazing shadow rays differ from brute force "
                           f"(buffer lit, brute shadowed: {int((~got & ref).sum())}); first {bad[:5].tolist()}")
    assert ctx.info()["lightbuf_failed"] == 0


# ---- the frame ------------------------------------------------------------------------------------
ROUTES = [(0, True), (1, True), (2, True), (3, True), (0, False)]  # (policy, light buffers)


@pytest.mark.parametrize("row", lu.ROWS, ids=ROW_IDS)
def test_frame_routes(gpu, row, tmp_path):
    """Brute force renders the reference's frame word for word with its query
    counts; every route renders brute force's frame: policy 0 with buffers,
    policies 1, 2 and 3, buffers off, each with exact shadows on and off, the
    host-built tree, and the proven reflection walk.  Every shadow query of
    every frame equals brute force over all triangles (verify_shadows)."""
    case = MANIFEST[row[0]]
    s = _lattice(row, tmp_path)
    f = s.frame()
    img_f, st_f = gpu.Context(s, "flat").render_image(f)
    _same(img_f, lu.golden(case), f"{row[0]}: brute force against the reference's frame")
    assert (st_f["closest"], st_f["shadow"]) == (case["closest"], case["shadow"])

    def check(ctx, what):
        img, st = ctx.render_image(f)
        _same(img, img_f, f"{row[0]} {what} against brute force")
        assert (st["closest"], st["shadow"], st["depth_overflow"]) == (case["closest"], case["shadow"], 0), what
        _check_verify(ctx, f"{row[0]} {what}")
        return st

    ctx = gpu.Context(s, "octree_gpu")
    for exact in (False, True):
        ctx.set_exact_shadows(exact)
        for policy, lbuf in ROUTES:
            ctx.set_light_buffers(lbuf)
            ctx.set_policy(policy)
            st = check(ctx, f"policy {policy} buffers {lbuf} exact {exact}")
            if exact:  # the proven routes leave no query undecided
                assert st["shadow_unproven"] == 0, (policy, lbuf, st)
    ctx.set_policy(0)
    ctx.set_light_buffers(True)
    ctx.set_exact_reflections(True)
    assert check(ctx, "exact reflections")["closest_unproven"] == 0
    host = gpu.Context(s, "octree")
    for exact in (False, True):
        host.set_exact_shadows(exact)
        check(host, f"host tree exact {exact}")


@pytest.mark.parametrize("row", lu.ROWS, ids=ROW_IDS)
def test_frame_96x54(gpu, row, tmp_path):
    """The same at 96x54 (more than one tile row and column), the default
    route and the walk, against brute force."""
    s = _lattice(row, tmp_path, 96, 54)
    f = s.frame()
    img_f, st_f = gpu.Context(s, "flat").render_image(f)
    ctx = gpu.Context(s, "octree_gpu")
    for exact in (True, False):
        ctx.set_exact_shadows(exact)
        for lbuf in (True, False):
            ctx.set_light_buffers(lbuf)
            img, st = ctx.render_image(f)
            _same(img, img_f, f"{row[0]} 96x54 buffers {lbuf} exact {exact}")
            assert (st["closest"], st["shadow"], st["depth_overflow"]) == (st_f["closest"], st_f["shadow"], 0)
            _check_verify(ctx, f"{row[0]} 96x54 buffers {lbuf} exact {exact}")


# ---- far lights ------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("name", FAR)
def test_far_lights_build(gpu, name, exact, tmp_path):
    """The build is what the row intends: the device lists exactly the host
    survey's entries, and the scene falls into a few cells -- at least a
    quarter of the lattice scene's hit points look up one and the same cell
    and so do at least a quarter of the sphere field's centroids (the restated
    cell arithmetic, whose cube side tests/test_lightbuf_geom.py holds to the
    build's cell count; the survey's own max_count is the largest single
    footprint -- 1 to 3 cells with slack-grown footprints, up to 109 with
    proven ones -- not a cell's population, and is printed)."""
    row = lu.row(name)
    for s, li in ((_lattice(row, tmp_path), 1), _synthetic(gpu, row)[0:3:2]):
        ctx = gpu.Context(s, "octree_gpu")
        ctx.set_exact_shadows(exact)
        info = ctx.info()
        e, g, per = _surveyed(s, exact)
        assert info["lightbuf_failed"] == 0 and (info["lightbuf_entries"], info["lightbuf_global"]) == (e, g), (info, per)
        h = s.lightbuf_survey(li, exact, 1)
        print(name, "exact" if exact else "slack", s.triangle_count, "triangles:", h)
        assert h["entries"] + h["global"] + h["never"] >= h["surveyed"] == s.triangle_count
    share = lu.largest_cell_share(row[2], lu.origins(), MANIFEST[name]["triangles"])
    print(name, "largest cell's share of the lattice origins", share)
    assert share >= 0.25, share
    # the sphere field: its triangles' centroids as hit points, the cube map of its own triangle count
    s, tri, li, lv, _, _ = _synthetic(gpu, row)
    cen = tri[:, :3].astype(np.float64).mean(axis=1).astype(F32)
    share = lu.largest_cell_share(lv, cen, s.triangle_count)
    print(name, "largest cell's share of the sphere field's centroids", share)
    assert share >= 0.25, share


# ---- the mixed state: one light on its buffer, another on the walk, in one shade kernel ----------------
def _mixed_checks(gpu, s, ctx, f, img_f, st_f, what, buffered):
    img, st = ctx.render_image(f)
    _same(img, img_f, f"{what} against brute force")
    assert (st["closest"], st["shadow"], st["depth_overflow"]) == (st_f["closest"], st_f["shadow"], 0), what
    _check_verify(ctx, what)
    if buffered is not None:  # the light that kept its buffer still answers through it
        o = lu.origins()
        assert np.array_equal(ctx.probe_shadows(buffered, o), ctx.probe_shadows(buffered, o, brute=True)), what
    return img, st


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("scene", ["lattice", "synthetic"])
def test_mixed_zero_direction_beside_a_point_light(gpu, scene, exact, tmp_path):
    """A zero-length directional light has no grid; the point light beside it
    keeps its buffer: the render leaves the all-buffers route and the shade
    kernel answers one light through its buffer and the other by the walk."""
    if scene == "lattice":
        s = lu.load_scene(tmp_path, [lu.AMBIENT_LIGHT, lu.row_light(lu.row("dir zero")), lu.ORDINARY_POINT], 96, 54, "mixed")
        point = 2
    else:
        s, _, li, _, _, _ = _synthetic(gpu, lu.row("dir zero"))
        point = next(k for k in range(int(s.s.light_count)) if int(s.s.lights[k].type) == 2)
    f = s.frame()
    img_f, st_f = gpu.Context(s, "flat").render_image(f)
    ctx = gpu.Context(s, "octree_gpu")
    ctx.set_exact_shadows(exact)
    _mixed_checks(gpu, s, ctx, f, img_f, st_f, f"zero direction beside a point light, {scene}, exact {exact}",
                  point if scene == "lattice" else None)
    info = ctx.info()
    assert info["lightbuf_failed"] == 1 and info["lightbuf_entries"] > 0 and "zero vector" in info["lightbuf_fail_reason"]
    e, g, per = _surveyed(s, exact)
    assert (info["lightbuf_entries"], info["lightbuf_global"]) == (e, g) and sum(h is None for h in per) == 1
    ref = ctx.probe_shadows(point, lu.origins(), brute=True) if scene == "lattice" else None
    if ref is not None:
        assert 0.01 < ref.mean() < 0.99, ref.mean()


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("scene", ["lattice", "synthetic"])
def test_mixed_entry_cap_between_two_lights(gpu, scene, exact, tmp_path):
    """Ordinary lights, the entry cap strictly between the two lights'
    surveyed entry counts: exactly one build fails, the other light keeps its
    entries, and the image and the counts are unchanged."""
    if scene == "lattice":
        s = lu.load_scene(tmp_path, [lu.AMBIENT_LIGHT, lu.BASE_LIGHT, lu.ORDINARY_POINT], 96, 54, "cap")
    else:
        s = gpu.Scene.synthetic(3, 3, 9776, seed=0x5EED, width=96, height=54)
    f = s.frame()
    img_f, st_f = gpu.Context(s, "flat").render_image(f)
    _, _, per = _surveyed(s, exact)
    assert len(per) == 2 and all(per)
    small, big = sorted((h["entries"], k + 1) for k, h in enumerate(per))
    cap = (small[0] + big[0]) // 2
    assert small[0] < cap < big[0], (small, big)
    ctx = gpu.Context(s, "octree_gpu")
    ctx.set_exact_shadows(exact)
    what = f"entry cap {cap} between {small[0]} and {big[0]}, {scene}, exact {exact}"
    img, st = _mixed_checks(gpu, s, ctx, f, img_f, st_f, what + " (before)", None)
    assert ctx.info()["lightbuf_failed"] == 0 and ctx.info()["lightbuf_entries"] == small[0] + big[0]
    ctx.set_lightbuf_entry_cap(cap)
    info = ctx.info()
    assert info["lightbuf_failed"] == 1 and info["lightbuf_entries"] == small[0], (info, small, big)
    assert f"light {big[1]}" in info["lightbuf_fail_reason"] and "entries" in info["lightbuf_fail_reason"]
    img2, st2 = _mixed_checks(gpu, s, ctx, f, img_f, st_f, what, small[1] if scene == "lattice" else None)
    _same(img2, img, what + ": the image before the cap")
    assert (st2["closest"], st2["shadow"]) == (st["closest"], st["shadow"])
    with pytest.raises(gpu.RtError, match="no buffer"):  # not answered through a table that does not exist
        ctx.probe_shadows(big[1], lu.origins()[:64])
    ctx.set_lightbuf_entry_cap(0)
    assert ctx.info()["lightbuf_failed"] == 0 and ctx.info()["lightbuf_entries"] == small[0] + big[0]


# ---- live edits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True])
def test_live_edits_to_every_row(gpu, exact, tmp_path):
    """From a context rendered under the base lights -- an ambient light, a
    directional and a point light, each with a buffer -- set_lights with each
    row in the slot of its type and relight: a fresh context's render under
    those lights, bit for bit.  Only the changed light's buffer may be rebuilt:
    the device's entries and global prims are the base scene's survey of the
    light that stayed plus the row scene's survey of the light that changed (a
    buffer dropped, kept from another row or rebuilt from the wrong vector
    shows there).  Back under the base lights the first image returns."""
    base = [lu.AMBIENT_LIGHT, lu.BASE_LIGHT, lu.ORDINARY_POINT]
    s0 = lu.load_scene(tmp_path, base, name="base")
    f = s0.frame()
    ctx = gpu.Context(s0, "octree_gpu")
    ctx.set_exact_shadows(exact)
    img0, st0 = ctx.render_image(f)
    e0, g0, per0 = _surveyed(s0, exact)  # per0[0]: the directional light's, per0[1]: the point light's
    assert (ctx.info()["lightbuf_entries"], ctx.info()["lightbuf_global"]) == (e0, g0) and all(h["entries"] > 0 for h in per0)
    for k, row in enumerate(lu.ROWS):
        slot = 1 if row[1] == lu.DIRECTIONAL else 2
        lights = list(base)
        lights[slot] = lu.row_light(row)
        s = lu.load_scene(tmp_path, lights, name=f"edit{k}")
        fresh, st_fresh = gpu.Context(s, "flat").render_image(f)
        ctx.set_lights(lights)
        img, st = ctx.relight_image(f)
        _same(img, fresh, f"{row[0]}: relit against a fresh context, exact {exact}")
        _, _, per = _surveyed(s, exact)
        kept, changed = per0[2 - slot], per[slot - 1]
        want = (kept["entries"] + (changed["entries"] if changed else 0), kept["global"] + (changed["global"] if changed else 0))
        info = ctx.info()
        assert (info["lightbuf_entries"], info["lightbuf_global"]) == want, (row[0], info, kept, changed)
        assert per[2 - slot] == kept, row[0]  # (the survey of the light that stayed does not depend on the other)
        assert info["lightbuf_failed"] == (1 if row[0] == "dir zero" else 0) == (changed is None), row[0]
        ctx.set_lights(base)
        back, _ = ctx.relight_image(f)
        _same(back, img0, f"back under the base lights after {row[0]}")
        assert (ctx.info()["lightbuf_entries"], ctx.info()["lightbuf_global"], ctx.info()["lightbuf_failed"]) == (e0, g0, 0), row[0]
    again, st1 = ctx.render_image(f)
    _same(again, img0, "a render after all the edits")
    assert (st1["closest"], st1["shadow"]) == (st0["closest"], st0["shadow"])
