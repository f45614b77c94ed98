"""The shading tables (csrc/rt_shade_rows.h): what the shade pass needs of a
light or a material and what cpu/light.c computes from the row alone -- the
channels over 255, a directional light's |d|, d / |d| and scale(v, -10) -- is
derived once per row on the device (shade_tables_kernel) wherever the raw rows
are uploaded, and the shade kernels read wave-uniform rows and light-buffer
descriptors by scalar loads.  Only where and how often the operations run
changed, so every image still equals the oracle's bit for bit; these tests aim
at what the tables add: a table left stale or derived from the wrong row after
rt_hip_set_lights / rt_hip_set_materials, rows past the first block of 32
lights, light lists with nothing to cast or a type the kernels skip, and the
other two users of lights_sum (recolour_kernel, oob_reshade_kernel).

Edits.  Light colours above 1, below 0 and exactly 0 go through chan()'s two
clamps before the division; a directional light turned into a point light and
back swaps which part of its row is meaningful; a directional v of 1e-3 and
1e3 times a unit vector moves |d| and the quotients d / |d| far from 1 (the
oracle keeps every pixel finite for both on all four scenes: checked on the
CPU, and asserted below).  Material channels above 1 and below 0 and the
exponents 0 and 1 do the same for the material rows.

The counting variant.  tests/golden/shade_tables_parent.json holds the work
counters of the commit before the tables (recorded with that commit's
library, two renders per case; the fields that differed between its own two
renders are listed there and none of the compared ones is among them)."""
import contextlib
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIELDS = ("closest", "shadow", "hits", "hit_records", "pixels", "shadow_tri_lanes", "closest_tri_lanes",
          "closest_node_lanes", "node_visits", "tri_tests", "shadow_zero_risk", "shadow_deferred")


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _load(gpu, scene_dir, name, W, H):
    s = gpu.Scene.load_svati(os.path.join(scene_dir, name + ".svati"))
    s.set_size(W, H)
    return s


@contextlib.contextmanager
def _light_table(gpu, s, rows):
    """The scene with another light array (any length) for the block: the
    scene's own array is the library's, so it is swapped out and put back."""
    arr = (gpu.Light * max(len(rows), 1))()
    for l, (t, r, g, b, x, y, z) in zip(arr, rows):
        l.type, l.r, l.g, l.b = int(t), r, g, b
        l.v.x, l.v.y, l.v.z = x, y, z
    old_addr, old_n = C.cast(s.s.lights, C.c_void_p).value, int(s.s.light_count)
    s.s.lights = C.cast(arr, C.POINTER(gpu.Light))
    s.s.light_count = len(rows)
    try:
        yield arr
    finally:
        s.s.lights = C.cast(C.c_void_p(old_addr), C.POINTER(gpu.Light))
        s.s.light_count = old_n


def _oracle(s):
    import oracle as orc
    f = s.frame()
    ref, cnt = orc.render(s.ptr, f.width, f.height, threads=4)
    ref = np.ascontiguousarray(ref).reshape(f.height, f.width, 3)
    assert np.isfinite(ref).all(), "the oracle's own image has a non-finite pixel: not a case to compare"
    return ref, cnt


def _same(img, ref, what):
    bad = np.argwhere((_bits(img).reshape(ref.shape) != _bits(ref)).any(axis=2))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first (row, col) {bad[:5].tolist()}"


def _check_scene_as_it_stands(gpu, s, accel, imgs, what):
    """Every image of `imgs` (name -> image) equals a fresh context's render of
    the scene as it stands and the oracle's, bit for bit."""
    ref, cnt = _oracle(s)
    ctx = gpu.Context(s, accel)
    fresh, st = ctx.render_image(s.frame())
    ctx.close()
    _same(fresh, ref, f"{what}: fresh context vs oracle")
    assert (st["closest"], st["shadow"]) == (cnt["closest"], cnt["shadow"])
    for name, img in imgs.items():
        _same(img, ref, f"{what}: {name} vs oracle")
    return st


# ---- tables follow edits ----
def _unit(l):
    v = np.array([l.v.x, l.v.y, l.v.z], np.float64)
    return v / np.linalg.norm(v)


def _set_v(l, v):
    l.v.x, l.v.y, l.v.z = (float(np.float32(x)) for x in v)


def _light_edits(s):
    """(name, edit) in order; each edit changes the scene's own light array."""
    L = s.lights()
    amb = next(i for i, l in enumerate(L) if l.type == 0)
    d = next((i for i, l in enumerate(L) if l.type == 1), None)
    k = d if d is not None else next(i for i, l in enumerate(L) if l.type == 2)
    unit = _unit(L[k])
    other = 2 if L[k].type == 1 else 1
    own = int(L[k].type)
    own_v = (L[k].v.x, L[k].v.y, L[k].v.z)

    def colours():  # above 1 (clamped by chan), below 0, exactly 0
        L[k].r, L[k].g, L[k].b = 1.75, -0.25, 0.0
        L[amb].r, L[amb].g, L[amb].b = 0.0, 2.5, -1.0

    def colours_back():
        L[k].r, L[k].g, L[k].b = 0.8, 0.6, 0.9
        L[amb].r, L[amb].g, L[amb].b = 0.3, 0.2, 0.25

    def turn():
        L[k].type = other

    def turn_back():
        L[k].type = own

    def directional(scale):
        def edit():
            L[k].type = 1
            _set_v(L[k], unit * scale)
        return edit

    def restore():
        L[k].type = own
        L[k].v.x, L[k].v.y, L[k].v.z = own_v

    return [("colours above 1, below 0 and 0", colours), ("colours back inside", colours_back),
            ("type turned", turn), ("type turned back", turn_back),
            ("directional, |v| = 1e-3", directional(1e-3)), ("directional, |v| = 1e3", directional(1e3)),
            ("light restored", restore)]


def _material_edits(s):
    o = s.s.objects[0]
    last = s.s.objects[s.s.object_count - 1]

    def channels():  # above 1, negative; exponent 0
        o.kd.x, o.kd.y = 1.6, -0.4
        o.ks.x, o.ks.z = -0.5, 3.0
        o.ka.y, o.ka.z = 1.25, -0.125
        o.ns = 0.0
        last.ns = 0.0

    def exponent_one():
        o.ns = 1.0
        last.ns = 1.0
        last.kd.z = 1.5

    return [("material channels above 1 and negative, exponent 0", channels), ("exponent 1", exponent_one)]


@pytest.mark.parametrize("scene", ["dir-light-shadows", "point-light", "sphere-spec", "car-on-road"])
def test_tables_follow_edits(gpu, scene_dir, scene):
    s = _load(gpu, scene_dir, scene, 96, 54)
    f = s.frame()
    ctx = gpu.Context(s, "octree")
    ctx.set_keep_visibility(True)
    img0, _ = ctx.render_image(f)
    _same(img0, _oracle(s)[0], f"{scene} unedited")
    seen = {_bits(img0).tobytes()}
    for what, edit in _light_edits(s) + _material_edits(s):
        edit()
        ctx.set_lights(s.lights())
        ctx.set_materials(s)
        relit, _ = ctx.relight_image(f)
        again, _ = ctx.render_image(f)
        _check_scene_as_it_stands(gpu, s, "octree", {"relight": relit, "render after the edit": again},
                                  f"{scene}, {what}")
        seen.add(_bits(relit).tobytes())
    assert len(seen) >= 5, "the edits are no no-ops"
    ctx.close()


# ---- block boundary, degenerate light lists ----
def _lights33():
    rows = [(0, 0.2, 0.25, 0.3, 0.0, 0.0, 0.0)]
    for k in range(32):  # alternating directional and point, dim enough not to saturate at once
        if k % 2 == 0:
            rows.append((1, 0.004 + 0.001 * k, 0.004, 0.006, 0.1 * (k - 16), -1.0, 0.5 + 0.05 * k))
        else:
            rows.append((2, 0.005, 0.003 + 0.001 * k, 0.007, -4.0 + 0.3 * k, 3.0 + 0.1 * k, 2.0 - 0.2 * k))
    return rows


def test_33_lights_second_block(gpu, scene_dir):
    """Light 32 lies in the second block (l0 = 32): its row is read at li >= 32
    and it has no stored lit bit, so a relight queries it again."""
    s = _load(gpu, scene_dir, "cube", 32, 18)
    f = s.frame()
    rows = _lights33()
    assert len(rows) == 33 and rows[32][0] == 2 and rows[31][0] == 1
    with _light_table(gpu, s, rows) as arr:
        ctx = gpu.Context(s, "octree")
        ctx.set_keep_visibility(True)
        img, st = ctx.render_image(f)
        fst = _check_scene_as_it_stands(gpu, s, "octree", {"render": img}, "cube, 33 lights")
        assert st["shadow"] == fst["shadow"] == st["hit_records"] * 32
        arr[32].r, arr[32].g, arr[32].b = 0.9, 0.1, 0.4  # the light of the second block, recoloured
        arr[31].v.x += 0.5                                # the last of the first block, moved
        ctx.set_lights(arr)
        relit, rst = ctx.relight_image(f)
        _check_scene_as_it_stands(gpu, s, "octree", {"relight": relit}, "cube, 33 lights, lights 31 and 32 edited")
        assert not np.array_equal(_bits(relit), _bits(img))
        assert rst["shadow"] == rst["hit_records"] * 2  # light 31 is dirty, light 32 has no stored bit
        ctx.close()


@pytest.mark.parametrize("rows", [
    [(0, 0.4, 0.3, 0.2, 0.0, 0.0, 0.0)],
    [(1, 0.6, 0.5, 0.4, 1.0, -1.0, 0.25), (7, 0.9, 0.9, 0.9, 0.0, 1.0, 0.0), (2, 0.5, 0.6, 0.7, -2.0, 3.0, 2.0)],
], ids=["ambient-only", "skipped-type-between-two"])
def test_degenerate_light_lists(gpu, scene_dir, rows):
    s = _load(gpu, scene_dir, "cube", 32, 18)
    f = s.frame()
    with _light_table(gpu, s, rows):
        ctx = gpu.Context(s, "octree")
        img, st = ctx.render_image(f)
        _check_scene_as_it_stands(gpu, s, "octree", {"render": img}, f"cube, lights {[r[0] for r in rows]}")
        assert st["shadow"] == st["hit_records"] * sum(1 for r in rows if r[0] in (1, 2))
        ctx.close()


# ---- the other users of lights_sum ----
def test_relight_recolours_and_requeries_one_light(gpu, scene_dir):
    """recolour_kernel (a colour-only edit: no query) and shade_kernel's
    relight form (one light moved and one recoloured: one light's queries)."""
    s = _load(gpu, scene_dir, "spheres", 32, 18)
    f = s.frame()
    ctx = gpu.Context(s, "octree")
    ctx.set_keep_visibility(True)
    img0, st0 = ctx.render_image(f)
    L = s.lights()
    L[2].r, L[2].g, L[2].b = 1.5, -0.5, 0.25
    L[0].g = 0.0
    ctx.set_lights(L)
    img1, st1 = ctx.relight_image(f)
    _check_scene_as_it_stands(gpu, s, "octree", {"recolour": img1}, "spheres, colour-only edit")
    assert st1["shadow"] == 0 and not np.array_equal(_bits(img1), _bits(img0))
    L[3].b = 0.125     # clean: its stored bits hold
    L[1].v.y -= 0.75   # dirty: the directional light turned
    ctx.set_lights(L)
    img2, st2 = ctx.relight_image(f)
    _check_scene_as_it_stands(gpu, s, "octree", {"partial relight": img2}, "spheres, one clean and one dirty light")
    assert st2["shadow"] == st2["hit_records"] and not np.array_equal(_bits(img2), _bits(img1))
    ctx.close()


OFFBOX = """camera 512 512 0.0 0.0 -10000000.0 1.0 0.0 0.0 0.0 -1.0 0.0 0.00013750987083133157

a_light 0.3 0.3 0.3
d_light 0.8 0.7 0.6 1.0 -1.0 1.0
p_light 0.5 0.5 0.5 3.0 4.0 -5.0

object 6
Ns 20.0
Kd 0.2 0.8 0.3
Ka 0.1 0.8 0.2
Ks 0.5 0.5 0.5

v -8.0 -8.0 3.0
v 8.0 -8.0 3.0
v 8.0 8.0 3.0
v -8.0 -8.0 3.0
v 8.0 8.0 3.0
v -8.0 8.0 5.0
""" + "vn 0.0 0.0 -1.0\n" * 6 + """
object 3
Ns 10.0
Kd 0.8 0.1 0.1
Ka 0.8 0.1 0.1
Ks 0.2 0.2 0.2

v -1.0 0.0 -2.0
v 1.0 0.0 -2.0
v 0.0 2.0 -2.0
""" + "vn 0.0 0.0 -1.0\n" * 3


def test_deferred_queries_reshade(gpu, tmp_path):
    """oob_reshade_kernel: the records whose queries the shade pass deferred
    are shaded again from the tables once brute force has decided them.  No
    golden scene defers a query at a test's size, so the frame is made for it:
    a camera 1e7 away (a float there has an ulp of 1) looking at a quad and a
    triangle 16 across through a field of view as narrow as they are.  The hit
    points o + nd (t |d|) land whole units off the surfaces, many of them more
    than the 1.2 units from the triangles' box that the light buffers' proof
    allows a shadow ray's origin (csrc/rt_lightbuf_host.cpp lb_fill)."""
    path = tmp_path / "offbox.svati"
    path.write_text(OFFBOX)
    s = gpu.Scene.load_svati(str(path))
    s.set_size(96, 54)
    f = s.frame()
    ctx = gpu.Context(s, "octree_gpu")
    ctx.set_exact_shadows(True)
    img, st = ctx.render_image(f)
    print("shadow_deferred", st["shadow_deferred"])
    assert st["shadow_deferred"] > 0, "the frame defers no query: it does not reach oob_reshade_kernel"
    flat, fst = gpu.Context(s, "flat").render_image(f)
    _same(img, np.ascontiguousarray(flat), "deferred queries vs brute force")
    _same(img, _oracle(s)[0], "deferred queries vs oracle")
    assert (st["closest"], st["shadow"]) == (fst["closest"], fst["shadow"])
    ctx.close()


# ---- the counting variant ----
@pytest.mark.parametrize("accel", ["octree", "octree_gpu"])
def test_counting_variant(gpu, scene_dir, accel):
    with open(os.path.join(GOLDEN, "shade_tables_parent.json")) as fh:
        rec = json.load(fh)["cases"][f"car-on-road_96x54/{accel}"]
    parent = rec["stats"]
    assert not set(FIELDS) & set(rec["differs_between_the_two_renders"])
    s = _load(gpu, scene_dir, "car-on-road", 96, 54)
    f = s.frame()
    plain, pst = gpu.Context(s, accel).render_image(f)
    ctx = gpu.Context(s, accel)
    ctx.set_count_work(True)
    img, st = ctx.render_image(f)
    ctx.close()
    assert np.array_equal(_bits(img), _bits(plain))
    print({k: (st[k], parent[k]) for k in FIELDS})
    assert (pst["closest"], pst["shadow"]) == (parent["closest"], parent["shadow"])
    for k in FIELDS:
        assert st[k] == parent[k], k
