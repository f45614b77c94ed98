"""Shared by tests/test_shading_edges_host.py, tests/test_shading_edges.py and
tests/golden/make_golden_shading.py: the stage (a floor, a tilted panel and a
dome of diverging normals under open sky), its ray sets, the tables of edge
materials and edge lights, the loader of tests/golden/shading/ and the
word-for-word comparison that takes NaN as NaN.  No GPU here.

What is computed after a hit -- cpu/light.c, cpu/colors.c and the `coef < 0.01`
of cpu/raytracer.c:21 -- is fed values no golden scene holds: exponents that
are zero, negative, huge, infinite or NaN, channels outside [0, 1], lights in
the plane of, next to and on the surface they light.  Non-finite values stay in
colours, Ka/Kd/Ks, Ns and Nr: they feed arithmetic, never an address.

The specular term of cpu/light.c:7-22 does not depend on the viewer: R is the
light's direction mirrored at N and V points at the light, so on a flat surface
under a directional light x = dot(R, V) is one number.  The dome makes it vary:
its vertex normals follow normalize(k (x - cx), 1, k z), so that under a light
from straight above x runs from exactly 1 (at the centre vertex, whose normal
is (0, 1, 0)) through 0 and below (at the rim, 68 degrees off)."""
import ctypes as C
import gzip
import json
import math
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
SHD = os.path.join(TESTS, "golden", "shading")
for _p in (os.path.join(REPO, "raytracing-gpu_amd"), os.path.join(REPO, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

F32 = np.float32
INF, NAN = float("inf"), float("nan")
ONE_DOWN = float(np.nextafter(F32(1), F32(0)))
ONE_UP = float(np.nextafter(F32(1), F32(2)))
T01 = float(F32(0.01))  # (float)0.01 = 0.00999999977648: below the double 0.01
T01_DOWN = float(np.nextafter(F32(0.01), F32(0)))
T01_UP = float(np.nextafter(F32(0.01), F32(1)))  # 0.0100000007078: above it
assert T01 < 0.01 < T01_UP


# ---- comparison -------------------------------------------------------------------
def words_differ(a, b):
    """Boolean array: where the float32 words of a and b differ, a NaN equal to
    any NaN (payload and sign are the platform's: x86 makes -qNaN where the
    GPU makes +qNaN)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))


def assert_same_words(got, want, what):
    bad = np.argwhere(words_differ(got, want))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {i}: "
                             f"{np.asarray(got)[i]!r} ({np.asarray(got, F32).view(np.uint32)[i]:#010x}) "
                             f"!= {np.asarray(want)[i]!r} ({np.asarray(want, F32).view(np.uint32)[i]:#010x})")


# ---- scene text -----------------------------------------------------------------------
def num(x):
    """A float32 as text that cpu/parser.c's %f reads back to the same bits
    (nan, inf, -inf, -0.0 and denormals included)."""
    x = float(F32(x))
    if math.isnan(x):
        return "nan"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return repr(x)


BENIGN = {"ka": (0.1, 0.1, 0.1), "kd": (0.6, 0.5, 0.4), "ks": (0.5, 0.5, 0.5), "ns": 12.0, "nr": 0.0}
SHINY = {"ka": (0.05, 0.1, 0.15), "kd": (0.3, 0.6, 0.2), "ks": (0.8, 0.7, 0.9), "ns": 96.078431, "nr": 0.0}


def material(**edit):
    m = dict(BENIGN)
    m.update(edit)
    return m


def _material_lines(m):
    return ["Ka " + " ".join(num(c) for c in m["ka"]), "Kd " + " ".join(num(c) for c in m["kd"]),
            "Ks " + " ".join(num(c) for c in m["ks"]), "Ns " + num(m["ns"]), "Nr " + num(m["nr"])]


def object_lines(m, tris):
    """tris = [((v0, v1, v2), (n0, n1, n2))] in file order."""
    lines = [f"object {3 * len(tris)}"] + _material_lines(m)
    for vs, _ in tris:
        lines += ["v " + " ".join(num(c) for c in v) for v in vs]
    for _, ns in tris:
        lines += ["vn " + " ".join(num(c) for c in n) for n in ns]
    return lines + [""]


AMBIENT, DIRECTIONAL, POINT, SPECULAR = 0, 1, 2, 3
_KEYWORD = {AMBIENT: "a_light", DIRECTIONAL: "d_light", POINT: "p_light"}


def light_lines(lights):
    """lights = [(type, r, g, b, x, y, z)]; a type the parser has no keyword
    for is written as an ambient placeholder (set it in memory afterwards)."""
    out = []
    for t, r, g, b, x, y, z in lights:
        if t in (DIRECTIONAL, POINT):
            out.append(f"{_KEYWORD[t]} {num(r)} {num(g)} {num(b)} {num(x)} {num(y)} {num(z)}")
        else:
            out.append(f"a_light {num(r)} {num(g)} {num(b)}")
    return out


def quad(a, b, c, d, n):
    """Two triangles a b c, a c d with one normal (or four, per corner)."""
    na, nb, nc, nd = n if isinstance(n[0], (tuple, list)) else (n, n, n, n)
    return [((a, b, c), (na, nb, nc)), ((a, c, d), (na, nc, nd))]


# ---- the stage ------------------------------------------------------------------------
# object 0: the floor, y = 0 on [0, 4] x [-4, 4], normal (0, 1, 0)
# object 1: the panel above the floor's +x edge, from (4, 0.5) up to (8.5, 9.5) in (x, y), normal (-2, 1, 0):
#           a ray that left the floor towards +x is sent up into the sky
# object 2: the dome, a flat 4 x 4 lattice of quads at y = 1 on [-3.5, -0.5] x [-1.5, 1.5] whose vertex
#           normals diverge: the interpolated N is shorter than 1 and turns by up to 68 degrees.  No floor
#           lies under it: a ray mirrored down from its underside leaves the scene (with a floor there,
#           a path whose coefficient is inf or NaN would bounce between the two)
FLOOR, PANEL, DOME = 0, 1, 2
DOME_C, DOME_Y, DOME_H, DOME_K = (-2.0, 0.0), 1.0, 1.5, 1.2
CAMERA = (-8.0, 6.0, 0.0, 0.0, 0.0, 1.0, 0.6, 0.8, 0.0, 50)  # position, u, v, fov: looks along (0.8, -0.6, 0)


def floor_tris():
    return quad((0, 0, -4), (4, 0, -4), (4, 0, 4), (0, 0, 4), (0, 1, 0))


def panel_tris():
    return quad((4, 0.5, -6), (4, 0.5, 6), (8.5, 9.5, 6), (8.5, 9.5, -6), (-2, 1, 0))


def dome_tris():
    def nrm(x, z):
        return (DOME_K * (x - DOME_C[0]), 1.0, DOME_K * (z - DOME_C[1]))
    tris, step = [], DOME_H / 2
    for i in range(4):
        for j in range(4):
            x0, z0 = DOME_C[0] - DOME_H + i * step, DOME_C[1] - DOME_H + j * step
            c = [(x0, z0), (x0 + step, z0), (x0 + step, z0 + step), (x0, z0 + step)]
            tris += quad(*[(x, DOME_Y, z) for x, z in c], [nrm(x, z) for x, z in c])
    return tris


def stage_text(lights, mats=None, w=32, h=18):
    """The stage as .svati text; mats: the three objects' materials."""
    mats = mats or [BENIGN, BENIGN, BENIGN]
    cam = f"camera {w} {h} " + " ".join(num(c) for c in CAMERA[:9]) + f" {CAMERA[9]}"
    lines = [cam] + light_lines(lights) + [""]
    for m, tris in zip(mats, (floor_tris(), panel_tris(), dome_tris())):
        lines += object_lines(m, tris)
    return "\n".join(lines)


def load_stage(tmpdir, lights, mats=None, w=32, h=18, name="stage"):
    """The stage as an rtgpu.Scene (the oracle reads the same rt_scene), the
    lights and materials set in memory so that what the parser cannot express
    (a light of type 3, or of a type nobody knows) arrives too."""
    import rtgpu
    path = os.path.join(str(tmpdir), name + ".svati")
    with open(path, "w") as f:
        f.write(stage_text(lights, mats, w, h))
    s = rtgpu.Scene.load_svati(path)
    set_lights(s, lights)
    for k, m in enumerate(mats or []):
        set_material(s, k, m)
    assert s.triangle_count == 36 and s.triangle_count < 64
    return s


def set_material(s, obj, m):
    o = s.s.objects[obj]
    for name in ("ka", "kd", "ks"):
        v = getattr(o, name)
        v.x, v.y, v.z = m[name]
    o.ns, o.nr = m["ns"], m["nr"]


def set_lights(s, lights):
    """Overwrites the scene's light array in place (same count)."""
    arr = s.lights()
    assert len(arr) == len(lights), (len(arr), len(lights))
    for l, (t, r, g, b, x, y, z) in zip(arr, lights):
        l.type, l.r, l.g, l.b = int(t), r, g, b
        l.v.x, l.v.y, l.v.z = x, y, z
    return arr


# ---- rays -------------------------------------------------------------------------------
def fan_rays(foot, base_y, heights, nphi, nr, rmax, scales=(1.0, 0.5, 0.75)):
    """From `height` above the point foot = (x, z) of the plane y = base_y to a
    polar lattice of targets of that plane, radius up to rmax: incidence from
    normal (r = 0) to grazing (atan(rmax / height)).  Unit directions times one
    of `scales` in turn: the reference uses a direction as given."""
    o, d = [], []
    for hi, h in enumerate(heights):
        fx, fz = foot[0] + 0.0625 * hi, foot[1] - 0.046875 * hi  # every height its own targets
        for a in range(nphi):
            phi = 2 * math.pi * (a + 0.25 + 0.125 * hi) / nphi
            for k in range(nr):
                r = rmax * k / (nr - 1)
                org = np.array([fx, base_y + h, fz])
                tgt = np.array([fx + r * math.cos(phi), base_y, fz + r * math.sin(phi)])
                dv = tgt - org
                dv *= scales[(a + k) % len(scales)] / np.linalg.norm(dv)
                o.append(org)
                d.append(dv)
    return np.array(o, F32), np.array(d, F32)


def down_rays(xs, zs, y, zero=0.0, scale=1.0):
    """Rays (zero, -scale, zero) from (x, y, z): every hit point on the floor or
    the dome is exact in float32 for x, z on a coarse binary lattice."""
    g = np.stack(np.meshgrid(xs, zs, indexing="ij"), -1).reshape(-1, 2)
    o = np.stack([g[:, 0], np.full(len(g), y), g[:, 1]], 1).astype(F32)
    d = np.tile(np.array([zero, -scale, zero], F32), (len(g), 1))
    return o, d


def _cat(sets):
    return np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])


EXACT_XS = np.arange(2, 10) * 0.25    # 0.5 .. 2.25: floor points clear of the dome and the panel
EXACT_ZS = -3.5 + np.arange(8) * 0.25  # -3.5 .. -1.75
N_EXACT = 64


def stage_rays():
    """The general set (materials, lights): 64 exact rays first (stage_rays()[:
    N_EXACT]: (+0, -1, +0) onto the floor lattice EXACT_XS x EXACT_ZS), the
    same with -0.0 and half length, fans over the floor from three heights and
    over the dome from two, and the bounce set."""
    sets = [down_rays(EXACT_XS, EXACT_ZS, 2.5), down_rays(EXACT_XS, EXACT_ZS, 2.5, -0.0, 0.5),
            fan_rays((2.0, 0.5), 0.0, (3.0, 0.75, 0.0625), 24, 24, 1.9),
            fan_rays((-2.25, 0.25), DOME_Y, (2.0, 0.125), 16, 15, 1.2), bounce_rays()]
    return _cat(sets)


def bounce_rays():
    """Floor -> panel -> sky: (0.8, -0.6, 0) from y = 1.5 onto the floor at x in
    [1.25, 3], mirrored to (0.8, 0.6, 0) into the panel, which sends it up."""
    o, d = [], []
    for i in range(8):
        for j in range(25):
            o.append((-0.75 + 0.25 * i, 1.5, -3.0 + 0.25 * j))
            d.append((0.8, -0.6, 0.0))
    return np.array(o, F32), np.array(d, F32)


POW_LIGHTS = [(DIRECTIONAL, 1.0, 1.0, 1.0, 0.0, -1.0, 0.0)]  # white, from straight above
POW_MATERIAL = {"ka": (0.0, 0.0, 0.0), "kd": (0.0, 0.0, 0.0), "ks": (1.0, 1.0, 1.0), "ns": 12.0, "nr": 0.0}


def pow_rays():
    """The pow sweep's 2,048 rays, all at the dome: fans from three heights
    (960), a 32 x 32 lattice of vertical rays within 0.1 of the centre vertex
    (x = dot(R, V) in (0.99, 1)) and an 8 x 8 lattice within 1e-4 of it, the
    vertex itself among them (x = 1)."""
    cx, cz = DOME_C
    fine = (np.arange(32) - 15.5) * (0.2 / 32)
    tiny = (np.arange(8) - 4) * 2.5e-5  # index 4: the centre vertex itself
    sets = [fan_rays((cx + 0.25, cz - 0.125), DOME_Y, (1.5, 0.25, 0.03125), 16, 20, 1.2),
            down_rays(cx + fine, cz + fine, 3.0), down_rays(cx + tiny, cz + tiny, 3.0)]
    return _cat(sets)


def spec_x(N, v=(0.0, -1.0, 0.0)):
    """x = dot(R, V) of cpu/light.c:11-19 for a directional light v at hit
    normals N (n, 3), operation for operation in float32 (the hit point drops
    out but for the rounding of (P - 10 v) - P, which the sweep's light, an
    axis vector, makes exact)."""
    N = np.asarray(N, F32)
    v = np.asarray(v, F32)

    def dot(a, b):
        return F32(a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]

    def normalize(a):
        s = F32(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
        ln = np.sqrt(s.astype(np.float64)).astype(F32)
        return a / ln[..., None]

    with np.errstate(all="ignore"):
        k = F32(2) * dot(N, v)
        R = normalize(v - k[..., None] * N)
        V = normalize(np.broadcast_to(F32(-10) * v, N.shape))
        return dot(R, V)


# ---- the material table: one varied word per row -------------------------------------------
NS_VALUES = [0.0, -0.0, 1.0, 0.5, 1.0 / 3.0, 2.0, 12.0, 96.078431, 1e3, 1e6, 3e38, -1.0, -0.5, 1e-45, INF, -INF, NAN]
CHANNEL_VALUES = [0.0, -0.0, 1.0, ONE_DOWN, ONE_UP, 1.0 / 255.0, 2.0, 1e30, -1.0, 1e-45, INF, -INF, NAN]
NR_VALUES = [0.0, -0.0, T01, T01_DOWN, T01_UP, 0.1, 1.0, 1.5, 100.0, -0.5, 1e-45, INF, NAN]


def tag(x):
    x = float(x)
    if x == T01:
        return "f0.01"
    if x == T01_DOWN:
        return "f0.01-"
    if x == T01_UP:
        return "f0.01+"
    if x == ONE_DOWN:
        return "1-"
    if x == ONE_UP:
        return "1+"
    return num(x)


def ns_rows():
    return [(f"Ns={tag(v)}", material(ns=v)) for v in NS_VALUES]


def channel_rows():
    rows = []
    for word in ("ks", "kd", "ka"):
        for i, v in enumerate(CHANNEL_VALUES):
            k = list(BENIGN[word])
            k[i % 3] = v  # the varied channel goes round r, g, b
            rows.append((f"{word.capitalize()}[{i % 3}]={tag(v)}", material(**{word: tuple(k)})))
    return rows


def nr_rows():
    return [(f"Nr={tag(v)}", material(nr=v)) for v in NR_VALUES]


def material_rows():
    return ns_rows() + channel_rows() + nr_rows()


def is_finite_material(m):
    return all(math.isfinite(float(F32(x))) for x in (*m["ka"], *m["kd"], *m["ks"], m["ns"], m["nr"]))


# (floor Nr, panel Nr): the product reaches the panel's reflection query on the
# second bounce -- at, below and above (float)0.01, and past it through
# values that are no reflectivity at all
NR_PAIRS = [(0.1, 0.1), (0.1, float(np.nextafter(F32(0.1), F32(0)))), (0.1, float(np.nextafter(F32(0.1), F32(1)))),
            (T01, 1.0), (T01_UP, 1.0), (T01_DOWN, 1.0), (1.0, T01), (1.0, T01_UP), (100.0, 1e-4), (100.0, 1.0001e-4),
            (-0.5, -0.5), (1e-45, INF), (INF, 0.0), (INF, -0.0), (NAN, 0.0), (0.5, NAN), (1.5, 1.5)]


# ---- the light table ------------------------------------------------------------------------
BASE_LIGHTS = [(AMBIENT, 0.2, 0.3, 0.4, 0.0, 0.0, 0.0), (DIRECTIONAL, 0.4, 0.35, 0.3, 0.25, -1.0, 0.5),
               (POINT, 0.3, 0.3, 0.25, -1.0, 5.0, 2.0)]
P0 = (float(EXACT_XS[3]), 0.0, float(EXACT_ZS[4]))  # the hit point of exact ray 3 * 8 + 4 (checked against the samples)
P0_RAY = 3 * 8 + 4
ON_HIT = "point on the hit point"


def light_rows(p0=P0):
    """[(name, lights)]: the base set with one more light, the row's.  p0: the
    exact hit point a light is put next to and on (the bits of a hit record)."""
    px, py, pz = (float(c) for c in p0)
    rows = [("ambient", (AMBIENT, 0.5, 0.25, 0.125, 0.0, 0.0, 0.0)),
            ("directional from above", (DIRECTIONAL, 0.5, 0.6, 0.7, -0.5, -1.0, 0.25)),
            ("directional from below", (DIRECTIONAL, 0.5, 0.6, 0.7, 0.25, 1.0, 0.5)),
            ("directional grazing +0", (DIRECTIONAL, 0.5, 0.6, 0.7, -1.0, 0.0, -1.0)),   # dot(L, N) = +0.0 on the floor
            ("directional grazing -0", (DIRECTIONAL, 0.5, 0.6, 0.7, 1.0, 0.0, 1.0)),     # L = (-1, -0.0, -1): -0.0
            ("point dot>0", (POINT, 0.5, 0.6, 0.7, 1.0, -3.0, 1.0)),    # below the floor: dot(-position, N) > 0
            ("point dot=+0", (POINT, 0.5, 0.6, 0.7, -6.0, 0.0, -5.0)),  # in the floor's plane, outside the floor
            ("point dot=-0", (POINT, 0.5, 0.6, 0.7, 6.0, 0.0, 5.0)),
            ("point dot<0", (POINT, 0.5, 0.6, 0.7, 1.0, 3.0, 1.0)),     # above: N flips for the diffuse term
            ("point 1e-3 off the hit point", (POINT, 0.5, 0.6, 0.7, px, py + 1e-3, pz)),
            ("point 1e-30 off the hit point", (POINT, 0.5, 0.6, 0.7, px, py + 1e-30, pz)),
            (ON_HIT, (POINT, 0.5, 0.6, 0.7, px, py, pz)),
            ("type 3", (SPECULAR, 0.5, 0.6, 0.7, 0.25, -1.0, 0.5)),
            ("unknown type", (7, 0.5, 0.6, 0.7, 0.25, -1.0, 0.5))]
    for i, v in enumerate(CHANNEL_VALUES):
        c = [0.5, 0.6, 0.7]
        c[i % 3] = v
        rows.append((f"directional colour[{i % 3}]={tag(v)}", (DIRECTIONAL, *c, -0.5, -1.0, 0.25)))
    for v in (-1.0, INF, NAN):
        rows.append((f"ambient colour={tag(v)}", (AMBIENT, v, 0.25, v, 0.0, 0.0, 0.0)))
    for v in (2.0, INF, NAN):
        rows.append((f"point colour={tag(v)}", (POINT, 0.5, v, v, 1.0, 3.0, 1.0)))
    out = [(name, BASE_LIGHTS + [l]) for name, l in rows]
    # 33 lights: the table's second block of 32 holds the edge light
    dim = [(DIRECTIONAL, 0.02, 0.03, 0.01, math.cos(k) * 0.5, -1.0, math.sin(k) * 0.5) for k in range(29)]
    out.append(("33 lights, edge colour last", BASE_LIGHTS + dim + [(DIRECTIONAL, INF, 1.0 / 255.0, -1.0, -0.5, -1.0, 0.25)]))
    out.append(("33 lights, on the hit point last", BASE_LIGHTS + dim + [(POINT, 0.5, NAN, 0.7, px, py, pz)]))
    return out


SKIPPED_LIGHTS = {"type 3": "cpu/light.c:94 skips the type", "unknown type": "cpu/light.c:94 skips the type"}
LIGHT_MATERIALS = [("benign", BENIGN), ("shiny", SHINY), ("Ns=0", material(ns=0.0)), ("Ns=-1", material(ns=-1.0))]


def lights_finite(lights):
    return all(math.isfinite(float(F32(x))) for l in lights for x in l[1:])


# ---- the committed fixtures (tests/golden/make_golden_shading.py) ----------------------------
def load_manifest():
    with open(os.path.join(SHD, "manifest.json")) as f:
        return json.load(f)


def scene_path(case, tmpdir):
    dst = os.path.join(str(tmpdir), case["svati"][:-3])
    with gzip.open(os.path.join(SHD, case["svati"]), "rb") as i, open(dst, "wb") as o:
        o.write(i.read())
    return dst


def golden(case):
    with gzip.open(os.path.join(SHD, case["file"]), "rb") as f:
        data = f.read()
    return np.frombuffer(data, dtype=np.float32).reshape(case["height"], case["width"], 3)


def patch_floor(n):
    """The floor as nx x nz patches (one object each, file order = row major),
    nx * nz >= n."""
    nx = int(math.ceil(math.sqrt(n)))
    nz = -(-n // nx)
    sx, sz = 4.0 / nx, 8.0 / nz
    out = []
    for k in range(n):
        i, j = k % nx, k // nx
        x0, z0 = i * sx, -4.0 + j * sz
        out.append(quad((x0, 0, z0), (x0 + sx, 0, z0), (x0 + sx, 0, z0 + sz), (x0, 0, z0 + sz), (0, 1, 0)))
    return out


def fixture_text(mats, lights, w=32, h=18, panel=BENIGN, dome=BENIGN):
    """A fixture scene: the stage with its floor cut into one patch per material."""
    cam = f"camera {w} {h} " + " ".join(num(c) for c in CAMERA[:9]) + f" {CAMERA[9]}"
    lines = [cam] + light_lines(lights) + [""]
    for m, tris in zip(mats, patch_floor(len(mats))):
        lines += object_lines(m, tris)
    lines += object_lines(panel, panel_tris()) + object_lines(dome, dome_tris())
    return "\n".join(lines)


def text_lights(lights):
    """The lights of a row the parser has a keyword for (a_light, d_light, p_light)."""
    return [l for l in lights if l[0] in _KEYWORD]


def fixture_scenes():
    """{name: (text, notes)} of tests/golden/shading/: every row of the
    material table on a patch of its own under the base lights, and light rows
    as text where text can say them."""
    mirror = material(nr=0.5)
    rows = dict(light_rows())
    four = [BENIGN, SHINY, material(ns=0.0), material(ns=-1.0)]
    scenes = {
        "ns": fixture_text([m for _, m in ns_rows()], BASE_LIGHTS),
        "channels": fixture_text([m for _, m in channel_rows()], BASE_LIGHTS),
        # the panel reflects too: the floor patch's Nr times 0.5 decides its next query
        "nr": fixture_text([m for _, m in nr_rows()] + [material(nr=a) for a, _ in NR_PAIRS], BASE_LIGHTS, panel=mirror),
        "lights-below-grazing": fixture_text([BENIGN, SHINY, material(ns=0.0), material(ns=-1.0)],
                                             BASE_LIGHTS + [rows[k][3] for k in ("directional from below", "directional grazing +0",
                                                                                 "directional grazing -0", "point dot=+0",
                                                                                 "point dot=-0", "point dot>0")]),
        # a NaN or an overflowing colour takes its channel over in every pixel: they get scenes of their own
        "lights-colours": fixture_text(four, BASE_LIGHTS + [rows[k][3] for k in rows if "colour" in k and not
                                                            any(t in k for t in ("=nan", "=inf", "e+30"))]),
        "lights-huge": fixture_text(four, BASE_LIGHTS + [rows[k][3] for k in rows if "colour" in k and
                                                         any(t in k for t in ("=inf", "e+30"))]),
        "lights-nan": fixture_text(four, BASE_LIGHTS + [rows[k][3] for k in rows if "colour" in k and "=nan" in k]),
        "lights-33": fixture_text([BENIGN, SHINY, material(ns=0.0), material(ns=-1.0)],
                                  text_lights(rows["33 lights, edge colour last"])),
    }
    return scenes


def fixture_materials(scene):
    """(patches, 11) float32: ka kd ks ns nr of a fixture scene's floor patches, in object order."""
    four = [BENIGN, SHINY, material(ns=0.0), material(ns=-1.0)]
    mats = {"ns": [m for _, m in ns_rows()], "channels": [m for _, m in channel_rows()],
            "nr": [m for _, m in nr_rows()] + [material(nr=a) for a, _ in NR_PAIRS]}.get(scene, four)
    return np.array([[*m["ka"], *m["kd"], *m["ks"], m["ns"], m["nr"]] for m in mats], F32)


# ---- the cases of tests/test_shading_edges.py ---------------------------------------------------
def material_cases():
    """[(name, [floor, panel, dome])]: "benign", then every row of the
    material table on the floor (panel and dome benign)."""
    return [("benign", [BENIGN, BENIGN, BENIGN])] + [(name, [m, BENIGN, BENIGN]) for name, m in material_rows()]


def light_cases(p0=P0):
    """[(name, lights, [floor, panel, dome])]: the base lights and every light
    row, each over the four materials of LIGHT_MATERIALS (on every object)."""
    return [(f"{row} | {mname}", lights, [m, m, m]) for row, lights in [("base", BASE_LIGHTS)] + light_rows(p0)
            for mname, m in LIGHT_MATERIALS]


def nr_cases():
    """[(name, [floor, panel, dome])] for the bounce rays: every Nr on the
    floor under a panel that reflects nothing, then the pairs."""
    return ([(name, [m, BENIGN, BENIGN]) for name, m in nr_rows()] +
            [(f"Nr pair {tag(a)} x {tag(b)}", [material(nr=a), material(nr=b), BENIGN]) for a, b in NR_PAIRS])


def oracle_runs(tmpdir, kind):
    """(name, (rgb, counts)) of every case of a kind through oracle.trace_rays."""
    import oracle as orc
    if kind == "lights":
        o, d = stage_rays()
        for k, (name, lights, mats) in enumerate(light_cases()):
            s = load_stage(tmpdir, lights, mats, name=f"l{k}")
            rgb, _, cnt = orc.trace_rays(s.ptr, o, d)
            yield name, (rgb, cnt)
        return
    o, d = stage_rays() if kind == "materials" else bounce_rays()
    s = load_stage(tmpdir, BASE_LIGHTS, name=kind)
    for name, mats in (material_cases() if kind == "materials" else nr_cases()):
        for k, m in enumerate(mats):
            set_material(s, k, m)
        rgb, _, cnt = orc.trace_rays(s.ptr, o, d)
        yield name, (rgb, cnt)


# rows that cannot change a word against the benign material (Ns 12, Nr 0), and why
_ENDS = "Nr * 1.0 < 0.01 ends the path before its next query, as Nr = 0 does (cpu/raytracer.c:21)"
UNCHANGING_MATERIALS = {"Ns=12.0": "the benign exponent itself", "Nr=0.0": "the benign reflectivity itself",
                        "Nr=-0.0": _ENDS, "Nr=f0.01": _ENDS, "Nr=f0.01-": _ENDS, "Nr=-0.5": _ENDS,
                        "Nr=1.401298464324817e-45": _ENDS}
