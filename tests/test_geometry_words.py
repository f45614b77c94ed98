"""The device-derived geometry, word for word (csrc/rt_geom.hip):
after rt_hip_set_triangles the context's prim-order records, normal rows,
vertex boxes, scene box and zero-risk flags -- and the tree rebuilt from them --
are those of a fresh context on the edited scene, compared here as 32-bit
words and not through what a small frame happens to see of them.

Expected values: the numpy float32 reference of tests/geometry_words_util.py
(its comparison rule: plain uint32 everywhere, two NaNs agree in the normal
rows alone), the host flatten (rtgpu.flatten_arrays; its flags are the host
predicate's, tests/native/zero_risk_twin.cpp), and a fresh context.  The host
side of the same comparison: tests/test_geometry_host.py.
"""
import time

import numpy as np
import pytest

import geometry_words_util as gw
from test_geometry import ACCELS, DevMem, _edit, _scene

pytestmark = pytest.mark.gpu
F32 = np.float32
BOX_BLOCKS_PRIMS = 1024 * 256  # RT_GEOM_BOX_BLOCKS workgroups of 256: above it k_box's lanes loop


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


@pytest.fixture(scope="module")
def pool():
    """Triangles whose every word is distinct, shared and never written: the
    edge scene's 1,900, then those the updates draw from."""
    t = gw.distinct_triangles(1900 + 5042 + 1024 + 1250, 20261020)
    t.setflags(write=False)
    return t


def _edge_scene(gpu, tmp_path, pool, counts=gw.EDGE_COUNTS):
    n = sum(counts)
    return gw.checked_scene(gpu, tmp_path / f"edge{n}.svati", pool[:n], counts)


def _host_flags(gpu, s):
    return gw.bits(gpu.flatten_arrays(s)[0])[:, 11]


def _check(gpu, ctx, s, accel, what, fresh=True, box_bits=None):
    """The context's arrays against the numpy reference of the (edited) host
    scene with the host's flags, and against a fresh context on that scene."""
    got = ctx.geometry_arrays()
    gw.check_against_reference(got, s.triangles_array(), gw.object_counts(s), _host_flags(gpu, s), what,
                               box_bits=box_bits)
    if fresh:
        f = gpu.Context(s, accel)
        gw.same_arrays(got, f.geometry_arrays(), what + ": against a fresh context")
        f.close()
    return got


# ---- a: the upload path ------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS + ["octree"])
def test_fresh_context_equals_the_host_flatten(gpu, tmp_path, pool, accel):
    s = _edge_scene(gpu, tmp_path, pool)
    ctx = gpu.Context(s, accel)
    host = gpu.flatten_arrays(s)
    if accel == "octree":  # a host tree keeps no vertex boxes, and says so
        with pytest.raises(gpu.RtError) as e:
            ctx.geometry_arrays()
        assert e.value.code == -1
        got = ctx.geometry_arrays(boxes=False)
        assert got[2] is None
    else:
        got = ctx.geometry_arrays()
        gw.same_words(got[2], host[2], "vertex boxes")
    gw.same_words(got[0], host[0], "records")
    gw.same_words(got[1], host[1], "normal rows")  # (uploaded, not derived: plain bits)
    gw.same_words(got[3], host[3], "scene box")
    tri, node = ctx.scene_image()
    assert tri.dtype == np.uint32 and node.dtype == np.uint32
    info = ctx.info()
    assert (len(tri), len(node)) == (info["tri_refs"], info["nodes"] if accel != "flat" else 0)
    if accel == "flat":
        gw.same_words(tri, gw.bits(host[0]), "flat: the scene image is the prim-order records")


# ---- b: ragged ranges ----------------------------------------------------------------
RANGES = [(0, 1), (0, 255), (0, 256), (0, 257), (1, 256), (255, 2), (256, 513), (300, 1), (301, 999), (1299, 601),
          (0, 1900), (1899, 1)]
FROM_DEVICE = [(1, 256), (255, 2), (1299, 601)]


@pytest.mark.parametrize("accel", ACCELS)
def test_ragged_ranges_touch_their_own_words_only(gpu, tmp_path, pool, accel):
    """One update per range, each with triangles no context has seen.  The
    whole arrays are compared, so a word written before or behind the range,
    or over words 9..11 of a record, shows wherever it lands."""
    s = _edge_scene(gpu, tmp_path, pool)
    ctx = gpu.Context(s, accel)
    at = 1900
    for k, (first, count) in enumerate(RANGES + FROM_DEVICE):
        new = pool[at:at + count]
        at += count
        before = ctx.geometry_arrays()
        s.set_triangles_array(new, first)
        if k < len(RANGES):
            ctx.set_triangles(new, first)
        else:
            mem = DevMem(gpu, new.nbytes).upload(new)
            ctx.set_triangles_device(mem.ptr, first, count)
            mem.free()
        what = f"[{first}, {first}+{count}) {'host' if k < len(RANGES) else 'device'} pointer, {accel}"
        got = _check(gpu, ctx, s, accel, what, box_bits=True)
        out = np.ones(1900, bool)
        out[first:first + count] = False
        for a, b, name in zip(got[:3], before[:3], ("records", "normal rows", "vertex boxes")):
            gw.same_words(a[out], b[out], f"{what}: {name} outside the range")
            cols = slice(0, 9) if name == "records" else slice(None)
            assert (gw.bits(a)[~out, cols] != gw.bits(b)[~out, cols]).any(axis=1).all(), \
                f"{what}: every prim's {name} inside the range are new"
        assert not gw.bits(got[0])[:, 11].any()
    assert ctx.geometry_updates() == len(RANGES) + len(FROM_DEVICE)
    ctx.validate()


# ---- c: the normals table ---------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("counts", [(257,), (1,) * 257], ids=["one-object", "an-object-each"])
def test_normals_that_are_not_unit_length(gpu, tmp_path, pool, accel, counts):
    """257 triangles (the table crosses a workgroup boundary) whose normals
    cycle through gw.NORMAL_ROWS.  Nothing is rendered: several of these are
    errors to the renderer.  With an object per triangle word 11 is the
    predicate's answer for that triangle's own rows."""
    s = _edge_scene(gpu, tmp_path, pool, counts)
    ctx = gpu.Context(s, accel)
    t = s.triangles_array()
    t[:, 3:], idx = gw.normal_table(257)
    s.set_triangles_array(t)
    ctx.set_triangles(t)
    rec, nrm, _, _ = _check(gpu, ctx, s, accel, f"normals table {accel}", box_bits=True)
    flag = gw.bits(rec)[:, 11]
    # what the rows are, so that the table cannot quietly stop being awkward
    assert np.isnan(nrm[gw.ROW_ZERO]).all() and np.isinf(nrm[gw.ROW_UNDERFLOW, [0, 3, 6]]).all()
    assert (nrm[gw.ROW_OVERFLOW] == 0).all() and (gw.bits(nrm[gw.ROW_OVERFLOW, :3]) >> 31).tolist() == [0, 1, 0]
    assert (nrm[5, [0, 1, 3, 4]] > 0.4).all(), "a denormal squared length still normalises"
    if len(counts) == 1:
        assert flag.all(), "the all-zeros rows flag their object"
    else:
        assert flag[gw.ROW_OVERFLOW] == 1, "all-zeros rows are flagged"
        has_nan = np.isnan(nrm).any(axis=1)
        assert has_nan.sum() > 50 and not flag[has_nan].any(), "NaN rows are never flagged"
        assert 0 < flag.sum() < 257


# ---- d: vertices -------------------------------------------------------------------------
def _signed_zero_report(name, upd, fresh):
    u, f = gw.bits(upd), gw.bits(fresh)
    rows = np.unique(np.argwhere(u != f)[:, 0])[:6]
    return f"{name}: updated / fresh bits differ in rows {rows.tolist()}: " \
           f"{[[hex(int(x)) for x in u[r]] for r in rows]} / {[[hex(int(x)) for x in f[r]] for r in rows]}"


@pytest.mark.parametrize("accel", ACCELS)
def test_awkward_vertices_and_the_sign_of_zero(gpu, tmp_path, pool, accel):
    """+-0 in every vertex order, denormal coordinates, +-1e30, identical
    vertices.  Records by bits; boxes by value against numpy (whose minimum /
    maximum leave the zero's sign open), by bits against a fresh context and
    the host flatten, and the zero's sign by the rule of host/rt_minmax.h."""
    s = _edge_scene(gpu, tmp_path, pool, (257,))
    ctx = gpu.Context(s, accel)
    t = s.triangles_array()
    t[:, :3] = gw.vertex_table(257)
    s.set_triangles_array(t)
    ctx.set_triangles(t)
    got = _check(gpu, ctx, s, accel, f"vertex table {accel}", fresh=False, box_bits=False)
    fresh = gpu.Context(s, accel)
    want = fresh.geometry_arrays()
    fresh.close()
    gw.same_words(got[0], want[0], "records against a fresh context")
    print("device vertex boxes of the six orders of (-0, +0, 5) then of (-5, -0, +0), x axis lo / hi:",
          [(hex(int(a)), hex(int(b))) for a, b in gw.bits(got[2])[:12, [0, 3]]])
    assert np.array_equal(gw.bits(got[2]), gw.bits(want[2])), _signed_zero_report("vertex boxes", got[2], want[2])
    assert np.array_equal(gw.bits(got[3]), gw.bits(want[3])), _signed_zero_report("scene box", got[3][None], want[3][None])
    gw.same_arrays(got, gpu.flatten_arrays(s), "against the host flatten")
    pb = gw.bits(got[2])
    assert (pb[:6, :3] == 0x80000000).all() and (pb[6:12, 3:] == 0).all(), "of two zeros lo is -0 and hi +0"
    # the scene box itself on a zero: x from the orders of (-0, +0, 5), y from those of (-5, -0, +0)
    t[:, :3] = gw.vertex_table(257, gw.ZERO_LO)
    t[:, :3, 1] = gw.vertex_table(257, gw.ZERO_HI)[:, :, 1]
    t[:, :3, 2] = pool[2000:2257, :3, 2]
    s.set_triangles_array(t)
    ctx.set_triangles(t)
    got = _check(gpu, ctx, s, accel, f"zero box {accel}", fresh=False, box_bits=False)
    fresh = gpu.Context(s, accel)
    want = fresh.geometry_arrays()
    tree = fresh.scene_image()
    fresh.close()
    print("device scene box lo.x, hi.y:", hex(int(gw.bits(got[3])[0])), hex(int(gw.bits(got[3])[4])))
    assert np.array_equal(gw.bits(got[2]), gw.bits(want[2])), _signed_zero_report("vertex boxes", got[2], want[2])
    assert np.array_equal(gw.bits(got[3]), gw.bits(want[3])), _signed_zero_report("scene box", got[3][None], want[3][None])
    assert (gw.bits(got[3])[[0, 4]] == [0x80000000, 0]).all() and got[3][3] == 5 and got[3][1] == -5
    for a, b, name in zip(ctx.scene_image(), tree, ("leaf-order records", "nodes")):
        gw.same_words(a, b, f"zero box {accel}: {name} against a fresh context")


# ---- e: the risk threshold on the device ----------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS)
def test_risk_threshold_in_device_arithmetic(gpu, tmp_path, pool, accel):
    normals, (pos, neg) = gw.risk_normals()
    n = len(normals)
    s = _edge_scene(gpu, tmp_path, pool, (1,) * n)
    ctx = gpu.Context(s, accel)
    t = s.triangles_array()
    t[:, 3:] = normals
    s.set_triangles_array(t)
    want = _host_flags(gpu, s)
    assert want[:9].tolist() == gw.K_ROWS_RISK
    for side in (pos, neg):  # both outcomes on each side of zero, or the table tests no threshold
        assert set(want[side].tolist()) == {0, 1} and want[side][8] == 1, want[side].tolist()
        assert (np.diff(want[side].astype(int)) <= 0).all(), "risky below the threshold, clean above"
    ctx.set_triangles(t)  # every case in one update
    rec = _check(gpu, ctx, s, accel, f"risk table {accel}", fresh=False, box_bits=True)[0]
    assert gw.bits(rec)[:, 11].tolist() == want.tolist()


@pytest.mark.parametrize("accel", ACCELS)
def test_risk_in_the_last_lane_of_a_ragged_workgroup(gpu, tmp_path, pool, accel):
    """Object 3 is prims [1300, 1900): 600 triangles, 88 in its last workgroup.
    A single risky triangle at its index 599 flags the whole object and no
    other; a one-triangle update that cleans it leaves no record flagged."""
    s = _edge_scene(gpu, tmp_path, pool)
    assert gpu.object_range(s, 3) == (1300, 600)
    ctx = gpu.Context(s, accel)
    clean = s.triangles_array()[1899:1900]
    risky = clean.copy()
    risky[0, 3:] = [(0, 0, 1), (0, 0, -1), (0, 0, 1)]
    s.set_triangles_array(risky, 1899)
    ctx.set_triangles(risky, 1899)
    rec = _check(gpu, ctx, s, accel, f"risky last lane {accel}", box_bits=True)[0]
    flag = gw.bits(rec)[:, 11]
    assert (flag[1300:] == 1).all() and not flag[:1300].any()
    s.set_triangles_array(clean, 1899)
    ctx.set_triangles(clean, 1899)
    rec = _check(gpu, ctx, s, accel, f"cleaned last lane {accel}", box_bits=True)[0]
    assert not gw.bits(rec)[:, 11].any()


# ---- f: the scene box above 262,144 prims ---------------------------------------------------
@pytest.fixture(scope="module", params=ACCELS)
def big(request, gpu):
    """Scene.synthetic_uv: 3 x 3 spheres of 82 stacks x 182 slices on their
    ground, 265,358 triangles (= 1036 x 256 + 142), cut down to its ambient
    light so that an update rebuilds no light buffer.  Measured on an MI355X:
    create 0.023 s (flat) / 0.032 s (octree_gpu); a one-triangle update 0.06 to
    0.09 ms for flatten + scene box + flags, and 4.3 to 7.1 ms for the tree."""
    s = gpu.Scene.synthetic_uv(3, 3, 82, 182, width=32, height=18)
    assert s.lights()[0].type == 0
    s.s.light_count = 1
    n = s.triangle_count
    assert n > BOX_BLOCKS_PRIMS and n % 256 != 0
    t0 = time.perf_counter()
    ctx = gpu.Context(s, request.param)
    print(f"{n} triangles, {request.param}: create {time.perf_counter() - t0:.3f} s")
    yield s, ctx, request.param
    ctx.close()


def test_scene_box_of_more_prims_than_the_first_pass_has_lanes(gpu, big):
    """Six one-triangle updates, each planting one extreme of the scene box at
    another prim -- the ends of the grid, both sides of the grid-stride loop's
    first wrap, the ragged end --, then the six put back."""
    s, ctx, accel = big
    t0 = s.triangles_array()
    n = len(t0)

    def np_box(t):
        v = t[:, :3].reshape(-1, 3)
        return np.concatenate([v.min(axis=0), v.max(axis=0)])

    box0 = ctx.geometry_arrays()[3]
    gw.same_words(box0, np_box(t0), "the fresh context's box")
    gw.same_words(box0, gpu.flatten_arrays(s)[3], "the host's box")
    ext = float((box0[3:] - box0[:3]).max())
    plant = [0, 255, BOX_BLOCKS_PRIMS - 1, BOX_BLOCKS_PRIMS, n - 1, n // 2 + 77]
    t = t0.copy()
    for k, p in enumerate(plant):  # k: lo.x, lo.y, lo.z, hi.x, hi.y, hi.z
        a = k % 3
        t[p, 1, a] = F32(box0[k] + (-1 if k < 3 else 1) * ext * (0.25 + 0.125 * k))
        s.set_triangles_array(t[p:p + 1], p)
        ctx.set_triangles(t[p:p + 1], p)
        box = ctx.geometry_arrays(boxes=False)[3]
        gw.same_words(box, np_box(t), f"{accel}: extreme {k} planted at prim {p}")
        assert box[k] == t[p, 1, a] and (gw.bits(box) != gw.bits(box0)).sum() == k + 1
        print(f"{accel}: update at prim {p}: flatten + box + flags, tree, light buffers {ctx.geometry_times()} s")
    ctx.validate()
    for k, p in reversed(list(enumerate(plant))):
        t[p] = t0[p]
        s.set_triangles_array(t[p:p + 1], p)
        ctx.set_triangles(t[p:p + 1], p)
        box = ctx.geometry_arrays(boxes=False)[3]
        gw.same_words(box, np_box(t), f"{accel}: extreme {k} at prim {p} put back")
    gw.same_words(box, box0, "the box shrinks back to its first bits")
    rec, nrm, pbox, _ = ctx.geometry_arrays()
    host = gpu.flatten_arrays(s)
    gw.same_words(rec, host[0], "records after the twelve updates")
    gw.same_normals(nrm, host[1], "normal rows after the twelve updates")
    gw.same_words(pbox, host[2], "vertex boxes after the twelve updates")


# ---- g: the rebuilt tree, word for word -------------------------------------------------------
TREE_EDITS = [("spheres", 96, 54, "shift", 3), ("spheres", 96, 54, "grow", 3), ("spheres", 96, 54, "spin", 0),
              ("spheres", 96, 54, "scale", None),
              ("room", 32, 18, "shift", 0), ("room", 32, 18, "grow", 0), ("room", 32, 18, "spin", 0),
              ("room", 32, 18, "scale", None)]


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name,W,H,kind,k", TREE_EDITS, ids=[f"{m[0]}-{m[3]}" for m in TREE_EDITS])
def test_rebuilt_tree_is_a_fresh_tree(gpu, scene_dir, tmp_path, name, W, H, kind, k, accel):
    """Nodes and leaf-order records as plain uint32 (flat: the prim-order
    records), against a fresh context after the edit and against the context's
    own first image after the original triangles are set back."""
    s = _scene(gpu, scene_dir, tmp_path, name, W, H)
    t0 = s.triangles_array()
    ctx = gpu.Context(s, accel)
    image0 = ctx.scene_image()
    assert (len(image0[1]) > 0) == (accel != "flat")
    first, new = _edit(gpu, s, kind, k)
    ctx.set_triangles(new, first)
    fresh = gpu.Context(s, accel)
    want = fresh.scene_image()
    gw.same_arrays(ctx.geometry_arrays(), fresh.geometry_arrays(), f"{name} {kind} {accel}")
    fresh.close()
    got = ctx.scene_image()
    for a, b, what in zip(got, want, ("leaf-order records", "nodes")):
        gw.same_words(a, b, f"{name} {kind} {accel}: {what} against a fresh context")
    assert not np.array_equal(got[0], image0[0]), "the edit changes the image"
    s.set_triangles_array(t0[first:first + len(new)], first)
    ctx.set_triangles(t0[first:first + len(new)], first)
    for a, b, what in zip(ctx.scene_image(), image0, ("leaf-order records", "nodes")):
        gw.same_words(a, b, f"{name} {kind} {accel}: {what} after setting the triangles back")
