"""Shading and fold arithmetic at its edges on the GPU, against the oracle.

tests/test_shading_edges_host.py pins the oracle to the reference's own frames
on the edge tables (exponents that are zero, negative, huge, infinite or NaN;
channels and light colours outside [0, 1]; reflectivities around (float)0.01;
lights behind, in the plane of, next to and on the surface they light) and
checks that the tables exercise what they claim.  Here the kernels are pinned
to the oracle on the same tables: colours word for word (a NaN as any NaN),
and the closest-hit and shadow query counts, which make the `coef < 0.01`
threshold sharp -- a wrong compare changes a count, not only a colour.

Routes.  Brute force (RT_ACCEL_FLAT), the device-built octree with its light
buffers (RT_ACCEL_OCTREE_GPU) with the packet flag off and on, a camera frame
of the committed fixtures, a relight after editing a live context
(recolour_kernel) and deferred shadow queries (oob_reshade_kernel) all sum the
lights through the one lights_sum; gpu/rt mode has its own float pow and uint8
colours.  Every route is compared with the oracle, and the GPU routes with
each other byte for byte.

The light on a hit point.  Its shadow ray's direction is (0, 0, 0) (1e-30 off:
a vector whose float length is 0).  The direction itself is finite, and only it
shapes an address: near_octant() compares its signs (0..7), inv_dir() clamps
1 / 0 to 1e30, lbuf_cells() looks no cell up when its largest component is 0
and clamps the cell otherwise, and the build lists a triangle that holds the
light in the light's global list (point_cone: the light is not outside the
triangle's ball).  normalize((0, 0, 0)) = NaN exists only inside hit_dist()
and the specular term: arithmetic.  Moller-Trumbore's a = e1 . (0 x e2) = 0
rejects every triangle as cpu/hit.c does, so the case runs on every route."""
import numpy as np
import pytest

import shading_edges_util as su

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


def _counts(st):
    return {"closest": st["closest"], "shadow": st["shadow"], "depth_overflow": st["depth_overflow"]}


def _want(cnt):
    return {"closest": cnt["closest"], "shadow": cnt["shadow"], "depth_overflow": 0}


def _same_bytes(a, b, what):
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what


class Routes:
    """The stage scene on brute force and on the device-built octree; trace():
    the same rays on flat, octree and octree + packet flag -- each equal to
    the oracle's colours (NaN as NaN) and counts, and to each other's bytes."""

    def __init__(self, gpu, s):
        self.gpu, self.s = gpu, s
        self.flat, self.oct = gpu.Context(s, "flat"), gpu.Context(s, "octree_gpu")

    def set_materials(self):
        self.flat.set_materials(self.s)
        self.oct.set_materials(self.s)

    def set_lights(self):
        self.flat.set_lights(self.s.lights())
        self.oct.set_lights(self.s.lights())

    def check(self, o, d, what):
        import oracle as orc
        want, _, cnt = orc.trace_rays(self.s.ptr, o, d)
        assert cnt["max_depth"] <= 4, what
        self.counts = cnt
        rf, _, stf = self.flat.trace_rays(o, d)
        su.assert_same_words(rf, want, f"{what}: flat against the oracle")
        assert _counts(stf) == _want(cnt), (what, "flat")
        ro, _, sto = self.oct.trace_rays(o, d)
        _same_bytes(ro, rf, f"{what}: octree against flat")
        assert _counts(sto) == _want(cnt), (what, "octree")
        rp, _, stp = self.oct.trace_rays(o, d, packet=True)
        _same_bytes(rp, rf, f"{what}: packet flag against flat")
        assert _counts(stp) == _want(cnt), (what, "packet")
        return rf, want

    def close(self):
        self.flat.close()
        self.oct.close()


# ---- a: the pow sweep ------------------------------------------------------------------------------
# Rays whose float colour differs between the device library's pow and glibc's, as (bits of (float)x,
# bits of Ns): measured on an MI355X over the sweep's 2,048 rays x 17 exponents -- none.
KNOWN_POW_MISMATCHES = []


def _chan(ls):
    return min(F32(ls) * F32(255), F32(255))


def _explain_pow_mismatch(x, ns, got, want):
    """A listed pair: the true value lies within 2^-50 (relative) of the
    midpoint of two neighbouring floats, and the two channels are chan() of
    those two floats: the results differ by exactly 1 ulp."""
    import oracle as orc
    true = orc.spec_pow_ld(float(x), float(F32(ns)))
    lo = F32(true)
    if np.longdouble(lo) > true:
        lo = np.nextafter(lo, F32(-np.inf))
    hi = np.nextafter(lo, F32(np.inf))
    mid = (np.longdouble(lo) + np.longdouble(hi)) / 2
    assert abs(true - mid) <= mid * np.longdouble(2.0) ** -50, (x, ns, true)
    assert {float(got), float(want)} == {float(_chan(lo)), float(_chan(hi))}, (x, ns, got, want, lo, hi)


def test_pow_sweep(gpu, tmp_path):
    """Ks = 1, Kd = Ka = 0, one white directional light from straight above,
    Nr = 0: the channel is chan(ls), ls = (float)pow(fmax(x, 0), Ns), for the
    2,048 rays of pow_rays() times every Ns of the table.  Bit equality;
    the README's contract allows 1 ulp where the two double pows round a value
    next to a float boundary differently, and only for pairs listed above."""
    import oracle as orc
    s = su.load_stage(tmp_path, su.POW_LIGHTS, [su.POW_MATERIAL] * 3)
    o, d = su.pow_rays()
    _, first, _ = orc.trace_rays(s.ptr, o, d, first=True)
    x = su.spec_x(first["N"])
    r = Routes(gpu, s)
    found = []
    for name, m in su.ns_rows():
        for k in range(3):
            su.set_material(s, k, dict(su.POW_MATERIAL, ns=m["ns"]))
        r.set_materials()
        want, _, cnt = orc.trace_rays(s.ptr, o, d)
        for ctx, route in ((r.flat, "flat"), (r.oct, "octree")):
            got, _, st = ctx.trace_rays(o, d)
            assert _counts(st) == _want(cnt), (name, route)
            bad = np.flatnonzero(su.words_differ(got, want).any(axis=1))
            for i in bad:
                pair = (int(F32(x[i]).view(np.uint32)), int(F32(m["ns"]).view(np.uint32)))
                found.append((route, name, pair, float(got[i, 0]), float(want[i, 0])))
                print("pow mismatch", found[-1])
                if pair in KNOWN_POW_MISMATCHES:
                    _explain_pow_mismatch(x[i], m["ns"], got[i, 0], want[i, 0])
    print(f"pow sweep: {len(o)} rays x {len(su.NS_VALUES)} exponents x 2 routes, {len(found)} mismatches")
    assert {p for _, _, p, _, _ in found} == set(KNOWN_POW_MISMATCHES), found[:8]
    r.close()


# ---- b: material edges ----------------------------------------------------------------------------
def test_material_edges(gpu, tmp_path):
    """Every row of the material table on the floor under the ambient +
    directional + point set, through set_materials and a re-trace (an Nr row:
    a context of its own, since reflectivity shapes the paths)."""
    o, d = su.stage_rays()
    s = su.load_stage(tmp_path, su.BASE_LIGHTS)
    shared = Routes(gpu, s)
    nans = clamps = 0
    for name, mats in su.material_cases():
        for k, m in enumerate(mats):
            su.set_material(s, k, m)
        if name.startswith("Nr="):
            r = Routes(gpu, s)
            got, _ = r.check(o, d, name)
            r.close()
            su.set_material(s, su.FLOOR, su.BENIGN)
        else:
            shared.set_materials()
            got, _ = shared.check(o, d, name)
        nans += int(np.isnan(got).any())
        clamps += int((got == 255).any())
    assert nans >= 5 and clamps >= 5  # (the host conditions say which rows)
    shared.close()


# ---- c: light edges ---------------------------------------------------------------------------------
def test_light_edges(gpu, tmp_path):
    """Every row of the light table over two benign and two edge materials,
    through set_lights and set_materials on live contexts.  The lights next to
    and on a hit point sit at the bits of a hit record's P."""
    o, d = su.stage_rays()
    s = su.load_stage(tmp_path, su.BASE_LIGHTS)
    r = Routes(gpu, s)
    _, smp, _ = r.oct.trace_rays(o[:su.N_EXACT], d[:su.N_EXACT], samples=True)
    p0 = tuple(float(c) for c in smp["P"][su.P0_RAY])
    assert p0 == su.P0 and smp["obj"][su.P0_RAY] == su.FLOOR
    last = None
    nans = 0
    for name, lights, mats in su.light_cases(p0):
        if lights is not last:  # a scene of the row's light count; the live contexts take the new table
            sl = su.load_stage(tmp_path, lights, mats, name="lights")
            r.s = sl
            r.set_lights()
            last = lights
        for k, m in enumerate(mats):
            su.set_material(sl, k, m)
        r.set_materials()
        got, _ = r.check(o, d, name)
        if name.startswith(su.ON_HIT):
            assert np.isnan(got[su.P0_RAY]).any(), "normalize((0, 0, 0)) did not reach the colour"
        nans += int(np.isnan(got).any())
    assert nans >= 8
    r.close()


# ---- d: the reflection threshold ----------------------------------------------------------------------
def test_reflection_threshold(gpu, tmp_path):
    """The Nr table and the pairs on the floor -> panel -> sky rays: colours
    and query counts.  (float)0.01 ends the path, one float above asks again."""
    o, d = su.bounce_rays()
    s = su.load_stage(tmp_path, su.BASE_LIGHTS)
    closest = {}
    for name, mats in su.nr_cases():
        for k, m in enumerate(mats):
            su.set_material(s, k, m)
        r = Routes(gpu, s)
        r.check(o, d, name)
        closest[name] = r.counts["closest"]
        r.close()
    assert closest["Nr=f0.01"] == len(o) and closest["Nr=f0.01+"] == 2 * len(o) and closest["Nr=inf"] == 3 * len(o)


# ---- e: the other routes ----------------------------------------------------------------------------------
CASES = su.load_manifest()["cases"]


@pytest.mark.parametrize("accel", ["flat", "octree", "octree_gpu"])
@pytest.mark.parametrize("case", CASES, ids=[c["scene"] for c in CASES])
def test_fixture_frames(gpu, tmp_path, case, accel):
    """A 32 x 18 camera frame of every committed fixture is the frame the
    reference rendered, with its query counts."""
    s = gpu.Scene.load_svati(su.scene_path(case, tmp_path))
    ctx = gpu.Context(s, accel)
    img, st = ctx.render_image(s.frame())
    ctx.close()
    su.assert_same_words(img, su.golden(case), f'{case["scene"]} on {accel} against the reference')
    assert _counts(st) == {"closest": case["closest"], "shadow": case["shadow"], "depth_overflow": 0}


def _relight_rows(table):
    if table == "materials":
        return [(name, su.BASE_LIGHTS, mats) for name, mats in su.material_cases() if not name.startswith("Nr=")]
    return [(name, lights, [su.BENIGN] * 3) for name, lights in su.light_rows()]


@pytest.mark.parametrize("table", ["materials", "lights"])
def test_relight_after_edits(gpu, tmp_path, table):
    """recolour_kernel: a benign frame is rendered once on the octree; then the
    live context is edited to every edge material row (but Nr's: reflectivity
    needs a new context) or every edge light row, and relit.  Each relit frame
    is the oracle's frame of the edited scene and, byte for byte, the frame a
    fresh brute-force context created with that table renders."""
    import oracle as orc
    s = su.load_stage(tmp_path, su.BASE_LIGHTS)
    f = s.frame()
    ctx = gpu.Context(s, "octree_gpu")
    ctx.set_keep_visibility(True)
    ctx.render_image(f)
    nans = 0
    for name, lights, mats in _relight_rows(table):
        e = su.load_stage(tmp_path, lights, mats, name="edited")
        ctx.set_lights(e.lights())
        ctx.set_materials(e)
        img, _ = ctx.relight_image(f)
        want, _ = orc.render(e.ptr, f.width, f.height)
        su.assert_same_words(img, want, f"{name}: relit against the oracle")
        fresh = gpu.Context(e, "flat")
        ref, _ = fresh.render_image(f)
        fresh.close()
        _same_bytes(img, ref, f"{name}: relit against a fresh context")
        nans += int(np.isnan(img).any())
    assert nans >= 4
    ctx.close()


def test_deferred_queries_reshade_at_the_edges(gpu, tmp_path):
    """oob_reshade_kernel: tests/test_shade_tables.py's frame that defers
    shadow queries, with Ns = -1 on the quad and a point light of colour
    (2, NaN, -1)."""
    import oracle as orc
    from test_shade_tables import OFFBOX
    path = tmp_path / "offbox.svati"
    path.write_text(OFFBOX)
    s = gpu.Scene.load_svati(str(path))
    s.set_size(96, 54)
    s.s.objects[0].ns = -1.0
    l = s.lights()[2]
    l.r, l.g, l.b = 2.0, su.NAN, -1.0
    f = s.frame()
    ctx = gpu.Context(s, "octree_gpu")
    ctx.set_exact_shadows(True)
    img, st = ctx.render_image(f)
    ctx.close()
    assert st["shadow_deferred"] > 0, "the frame defers no query: it does not reach oob_reshade_kernel"
    want, cnt = orc.render(s.ptr, f.width, f.height, threads=4)
    su.assert_same_words(img, want, "deferred queries against the oracle")
    assert np.isnan(want).any() and (want == 255).any()
    assert _counts(st) == _want(cnt)


# ---- f: gpu/rt mode ----------------------------------------------------------------------------------------
def test_compat_mode_finite_rows(gpu, tmp_path):
    """The finite rows of both tables at 24 x 16 through the compat render
    (rt_compat.h: float pow, uint8 colours, the nr > 0.01f bounce rule)
    against oracle.render_gpu."""
    import oracle as orc
    W, H = 24, 16

    def check(ctx, s, name):
        img, st = ctx.render_compat(s.camera)
        ref, cnt = orc.render_gpu(s.ptr, W, H, threads=8)
        bad = np.argwhere((img != ref).any(axis=2))
        assert len(bad) == 0, f"{name}: {len(bad)} pixels differ, first {bad[:4].tolist()}: " \
                              f"{img[tuple(bad[0])].tolist()} != {ref[tuple(bad[0])].tolist()}"
        assert (st["closest"], st["shadow"]) == (cnt["closest"], cnt["shadow"]), name

    s = su.load_stage(tmp_path, su.BASE_LIGHTS, w=W, h=H)
    shared = gpu.Context(s, "octree_gpu")
    n = 0
    for name, mats in su.material_cases():
        if not all(su.is_finite_material(m) for m in mats):
            continue
        for k, m in enumerate(mats):
            su.set_material(s, k, m)
        if name.startswith("Nr="):
            ctx = gpu.Context(s, "octree_gpu")
            check(ctx, s, name)
            ctx.close()
            su.set_material(s, su.FLOOR, su.BENIGN)
        else:
            shared.set_materials(s)
            check(shared, s, name)
        n += 1
    for name, lights in su.light_rows():
        if not su.lights_finite(lights):
            continue
        sl = su.load_stage(tmp_path, lights, w=W, h=H, name="lights")
        shared.set_materials(sl)
        shared.set_lights(sl.lights())
        check(shared, sl, name)
        n += 1
    shared.close()
    assert n >= 70
