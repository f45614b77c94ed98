"""Shared by tests/test_light_edges_host.py, tests/test_light_edges.py,
tests/test_lightbuf_geom.py and tests/golden/make_golden_lights.py: the table of
edge lights (where a light is, not what colour it has), the lattice scene they
light, its hit points, a float32 restatement of the point query's face choice
and cell arithmetic (csrc/rt_lightbuf_cell.h), the loader of
tests/golden/lights/ and the conditions every row must meet.  No GPU here.

A light's position or direction shapes the light buffers' grids (lb_derive_grid,
csrc/rt_lightbuf_host.cpp), the cells a query looks up (lbuf_cells) and the
walks' slabs (rt_inv), not only arithmetic: axis-aligned directions put exact
zeros and -0.0 into the grid's axes, (1, 1, 0) ties the choice of the smallest
component, 1e-20 and 1e30 sit at the ends of the float range (the reference
rejects every triangle there: `a` below 1e-7, or t = distance / |d| below it),
and a light on the scene's integer lattice gives the cube map |x| == |y| and
sc = +-1 exactly, where its strict `>` compares and the clamp to n - 1 decide."""
import gzip
import json
import math
import os
import sys

import numpy as np

import shading_edges_util as su
from shading_edges_util import AMBIENT, DIRECTIONAL, POINT, assert_same_words, num, words_differ  # noqa: F401

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
LIGHTS = os.path.join(TESTS, "golden", "lights")
F32 = np.float32
W, H = 32, 18

# ---- the light table ------------------------------------------------------------------
# what the reference's test gives for the row's shadow rays (asserted on brute force and the oracle):
SHADOWS = "shadows"  # the share of shadowed origins lies strictly between 1 % and 99 %
NOTHING = "nothing"  # no triangle is ever accepted: the share is exactly 0
ENCLOSED = "enclosed"  # the light inside a closed box: every ray to it crosses the box, the share is exactly 1
BOX_C = (2.0, -2.0, 2.0)  # the centre of the closed box object

# (name, type, l.v, on the lattice, what the reference gives, the code it aims at)
ROWS = [
    ("dir 0 -1 0", DIRECTIONAL, (0.0, -1.0, 0.0), False, SHADOWS, "lb_derive_grid: w = (0, 1, 0), exact zeros in u and v"),
    ("dir 1 0 0", DIRECTIONAL, (1.0, 0.0, 0.0), False, SHADOWS, "lb_derive_grid: m = 1 by the first strict '<'; rt_inv's 1e30 on y and z"),
    ("dir 0 1 0 from below", DIRECTIONAL, (0.0, 1.0, 0.0), False, SHADOWS, "rays leave downwards through the floor's plane"),
    ("dir -0 0 1", DIRECTIONAL, (-0.0, 0.0, 1.0), False, SHADOWS, "-0.0 in l.v: +0.0 in the ray, near_octant and rt_inv's sign"),
    ("dir 1 1 0", DIRECTIONAL, (1.0, 1.0, 0.0), False, SHADOWS, "lb_derive_grid: |w.x| == |w.y|, the smallest is z"),
    ("dir 1 -1 1", DIRECTIONAL, (1.0, -1.0, 1.0), False, SHADOWS, "lb_derive_grid: a three-way tie of the smallest component"),
    ("dir 1 1e-8 0", DIRECTIONAL, (1.0, 1e-8, 0.0), False, SHADOWS, "a component that vanishes in float sums but not in the axes"),
    ("dir 0.5 -0.25 0", DIRECTIONAL, (0.5, -0.25, 0.0), False, SHADOWS, "in the plane of the wall z = 4: a == 0 exactly there"),
    ("dir 1e-20 0 0", DIRECTIONAL, (1e-20, 0.0, 0.0), False, NOTHING, "p.dlen = 1e-20: every |a| is below 1e-7 (proven mode: never)"),
    ("dir denormal", DIRECTIONAL, (3e-39, 3e-39, 0.0), False, NOTHING, "length(d) is 0 in float, > 0 in lb_derive_grid's double"),
    ("dir 1e30", DIRECTIONAL, (1e30, -1e30, 1e30), False, NOTHING, "|d|^2 overflows float: dlen = inf; t = distance / |d| < 1e-7"),
    ("dir zero", DIRECTIONAL, (0.0, 0.0, 0.0), False, NOTHING, "lb_derive_grid returns 1: no grid, the light's queries walk"),
    ("point lattice centre", POINT, (0.0, 0.0, 0.0), True, SHADOWS, "lbuf_cells: |x| == |y| face ties, sc = +-1 and 0"),
    ("point wall vertex", POINT, (4.0, 0.0, 0.0), True, SHADOWS, "a mesh vertex: the triangles around it go to the global list"),
    ("point wall plane", POINT, (4.0, 6.0, 0.0), True, SHADOWS, "in the plane x = 4 above the wall: band rows, a == 0 for the wall"),
    ("point box corner", POINT, (-8.0, -4.0, -8.0), True, SHADOWS, "a corner of the triangle box (and of the floor)"),
    ("point inside the closed box", POINT, BOX_C, True, ENCLOSED, "every ray from the box's faces crosses the opposite face"),
    ("point 1e6 0 0", POINT, (1e6, 0.0, 0.0), False, SHADOWS, "the scene in one or two cells; l.v - P keeps 4 bits of P below 1/16"),
    ("point 1e6 1e6 1e6", POINT, (1e6, 1e6, 1e6), False, SHADOWS, "far along the diagonal: three faces meet, lim about 1.7e6"),
    ("point 0 1e9 0", POINT, (0.0, 1e9, 0.0), False, NOTHING, "t = distance / 1e9 < 1e-7 for every triangle of the scene"),
    ("point 3e38", POINT, (3e38, 3e38, 3e38), False, NOTHING, "|x|^2 overflows: lim = inf; an exact three-way face tie"),
    ("point off the lattice", POINT, (4.0, 8.0, 12.000001), False, SHADOWS, "the control: one float step off a lattice point"),
]
ROW_NAMES = [r[0] for r in ROWS]
AMBIENT_LIGHT = (AMBIENT, 0.25, 0.25, 0.3, 0.0, 0.0, 0.0)
BASE_LIGHT = (DIRECTIONAL, 0.7, 0.65, 0.6, 0.25, -1.0, 0.5)  # general position: the live edits start from it
ORDINARY_POINT = (POINT, 0.6, 0.6, 0.5, -2.5, 3.25, -6.5)    # outside the walls, off the lattice


def row(name):
    return ROWS[ROW_NAMES.index(name)]


def row_light(r):
    return (r[1], 0.7, 0.65, 0.6, *r[2])


def row_lights(r):
    """The lights of a row's scene: one ambient light (no frame is black) and the row's."""
    return [AMBIENT_LIGHT, row_light(r)]


def row_slug(name):
    return name.replace(" ", "_").replace(".", "p")


# ---- the lattice scene ---------------------------------------------------------------------
# Every coordinate an integer or a quarter integer.  Walls x = -4, x = 4 and z = 4 of the box [-4, 4]^3 in
# unit quads with windows, a ceiling y = 4 that is a checkerboard of skylights (cpu/light.c's shadow rays
# have no far end: a closed room blocks every one), the side z = -4 open towards the camera, a closed box
# object [1, 3] x [-3, -1] x [1, 3] and a floor y = -4 on [-8, 8]^2, larger than the rest.
def lattice(origin, du, dv, nu, nv, normal, keep=lambda i, j: True):
    """nu x nv quads from `origin` along du, dv, the diagonals alternating."""
    o, du, dv = (np.array(x, np.float64) for x in (origin, du, dv))
    tris = []
    for i in range(nu):
        for j in range(nv):
            if not keep(i, j):
                continue
            a, b, c, d = o + i * du + j * dv, o + (i + 1) * du + j * dv, o + (i + 1) * du + (j + 1) * dv, \
                o + i * du + (j + 1) * dv
            quads = [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
            tris += [(tuple(map(tuple, q)), (normal, normal, normal)) for q in quads]
    return tris


def _window(i, j):
    return not (i % 3 == 1 and j % 3 == 1)


BOX_LO, BOX_HI = (1.0, -3.0, 1.0), (3.0, -1.0, 3.0)


def box_tris(lo=BOX_LO, hi=BOX_HI):
    lo, hi = np.array(lo), np.array(hi)
    tris = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for side, at in ((-1.0, lo[a]), (1.0, hi[a])):
            o, du, dv, n = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
            o[a], o[b], o[c] = at, lo[b], lo[c]
            du[b], dv[c], n[a] = hi[b] - lo[b], hi[c] - lo[c], side
            tris += lattice(o, du, dv, 1, 1, tuple(n))
    return tris


def scene_objects():
    """[(material, triangles)] in file order."""
    left = lattice((-4, -4, -4), (0, 1, 0), (0, 0, 1), 8, 8, (1, 0, 0), _window)
    right = lattice((4, -4, -4), (0, 1, 0), (0, 0, 1), 8, 8, (-1, 0, 0), _window)
    back = lattice((-4, -4, 4), (1, 0, 0), (0, 1, 0), 8, 8, (0, 0, -1), _window)
    ceiling = lattice((-4, 4, -4), (1, 0, 0), (0, 0, 1), 8, 8, (0, -1, 0), lambda i, j: (i + j) % 2 == 0)
    floor = lattice((-8, -4, -8), (4, 0, 0), (0, 0, 4), 4, 4, (0, 1, 0))
    return [(su.material(kd=(0.8, 0.3, 0.3)), left), (su.material(kd=(0.3, 0.8, 0.3)), right),
            (su.material(kd=(0.4, 0.4, 0.9), nr=0.3), back), (su.material(kd=(0.6, 0.6, 0.6)), ceiling),
            (su.material(kd=(0.9, 0.8, 0.2)), box_tris()), (su.material(kd=(0.7, 0.7, 0.7)), floor)]


CAMERA = "camera {w} {h} 0 1 -15 1 0 0 0 -1 0 50"  # in front of the open side, rays towards +z


def scene_text(lights, w=W, h=H):
    lines = [CAMERA.format(w=w, h=h)] + su.light_lines(lights) + [""]
    for m, tris in scene_objects():
        lines += su.object_lines(m, tris)
    return "\n".join(lines)


def load_scene(tmpdir, lights, w=W, h=H, name="lattice"):
    import rtgpu
    path = os.path.join(str(tmpdir), name + ".svati")
    with open(path, "w") as f:
        f.write(scene_text(lights, w, h))
    s = rtgpu.Scene.load_svati(path)
    assert 300 <= s.triangle_count <= 600, s.triangle_count
    return s


# ---- hit points -----------------------------------------------------------------------------------
def _grid(a, b, step=1.0):
    return np.arange(a, b + step / 2, step)


def lattice_points():
    """The integer lattice points of the walls, the ceiling and the floor
    (windows and skylights included: a hit point's bits, wherever a ray ends)."""
    g = _grid(-4, 4)
    pts = []
    for x in (-4.0, 4.0):
        pts += [(x, y, z) for y in g for z in g]
    pts += [(x, y, 4.0) for x in g for y in g]
    pts += [(x, 4.0, z) for x in g for z in g]
    pts += [(x, -4.0, z) for x in _grid(-8, 8) for z in _grid(-8, 8)]
    return np.unique(np.array(pts, F32), axis=0)


def box_face_points():
    """The quarter lattice strictly inside each face of the closed box object."""
    lo, hi = np.array(BOX_LO), np.array(BOX_HI)
    pts = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for at in (lo[a], hi[a]):
            for u in _grid(lo[b] + 0.25, hi[b] - 0.25, 0.25):
                for v in _grid(lo[c] + 0.25, hi[c] - 0.25, 0.25):
                    p = np.zeros(3)
                    p[a], p[b], p[c] = at, u, v
                    pts.append(p)
    return np.array(pts, F32)


def nudged(points):
    """The points, then each moved one float step down and up in x, y and z."""
    out = [points]
    for a in range(3):
        for to in (-np.inf, np.inf):
            q = points.copy()
            q[:, a] = np.nextafter(q[:, a], F32(to))
            out.append(q)
    return np.concatenate(out)


N_LATTICE = len(lattice_points())
N_FACE = len(box_face_points())


def origins():
    """probe_shadows' origins on the lattice scene: the lattice points (the
    first N_LATTICE), the box's face points (the next N_FACE), then both moved
    by one float step to either side in each coordinate."""
    return nudged(np.concatenate([lattice_points(), box_face_points()]))


def face_slice():
    return slice(N_LATTICE, N_LATTICE + N_FACE)


# ---- the point query's cells, restated (csrc/rt_lightbuf_cell.h:34-63) ----------------------------
def cube_side(nprim, mul=1):
    """n of lb_derive_grid for lb_fill's target of a scene of nprim triangles
    (times mul, as tests/native/lightbuf_geom.cpp multiplies it);
    tests/test_lightbuf_geom.py holds it to the cells the build derives."""
    target = min(max(2 * nprim, 4096), 1 << 25) * mul
    return min(max(int(math.ceil(math.sqrt(target / 6.0))), 1), 8192)


def point_cells(lv, o, n):
    """Float32, operation for operation: x = -(l.v - o), the face by strict '>'
    in the order x, y, z, sc = xj / m, tc = xk / m, (sc + 1) * half_n.  Test
    code only.  Returns per origin: an exact face tie (the largest |component|
    is reached twice), sc or tc exactly +-1, an exact integer cell coordinate
    (before the clamp to n - 1), sc or tc exactly 0."""
    o = np.asarray(o, F32)
    d = np.asarray(lv, F32)[None, :] - o  # shadow_dir: sub(l.v, P)
    x = -d
    ab = np.abs(x)
    a = np.zeros(len(o), np.int64)
    m = ab[:, 0].copy()
    for k in (1, 2):
        up = ab[:, k] > m
        a[up], m[up] = k, ab[up, k]
    idx = np.arange(len(o))
    xj, xk = x[idx, (a + 1) % 3], x[idx, (a + 2) % 3]
    ok = m > 0
    with np.errstate(all="ignore"):
        sc, tc = (xj / m).astype(F32), (xk / m).astype(F32)
        half_n = F32(0.5) * F32(n)
        cu, cv = ((sc + F32(1)) * half_n).astype(F32), ((tc + F32(1)) * half_n).astype(F32)
    tie = ok & ((ab == m[:, None]).sum(axis=1) >= 2)
    unit = ok & ((np.abs(sc) == 1) | (np.abs(tc) == 1))
    whole = ok & ((cu == np.floor(cu)) | (cv == np.floor(cv)))
    zero = ok & ((sc == 0) | (tc == 0))
    return tie, unit, whole, zero


def first_cells(lv, o, n):
    """cell[0] of lbuf_cells' point branch per origin (-1: none), by the same
    float32 operations: the face 2 a + (xa < 0), the coordinates clamped to n - 1."""
    o = np.asarray(o, F32)
    x = -(np.asarray(lv, F32)[None, :] - o)
    ab = np.abs(x)
    a = np.zeros(len(o), np.int64)
    m = ab[:, 0].copy()
    for k in (1, 2):
        up = ab[:, k] > m
        a[up], m[up] = k, ab[up, k]
    idx = np.arange(len(o))
    with np.errstate(all="ignore"):
        half_n = F32(0.5) * F32(n)
        ix = np.minimum((((x[idx, (a + 1) % 3] / m).astype(F32) + F32(1)) * half_n).astype(np.int64), n - 1)
        iy = np.minimum((((x[idx, (a + 2) % 3] / m).astype(F32) + F32(1)) * half_n).astype(np.int64), n - 1)
    f = 2 * a + (x[idx, a] < 0)
    return np.where(m > 0, (f * n + iy) * n + ix, -1)


def largest_cell_share(lv, o, nprim):
    """The share of the origins that look up the most popular first cell."""
    c = first_cells(lv, o, cube_side(nprim))
    _, counts = np.unique(c, return_counts=True)
    return float(counts.max()) / len(c)


def tie_counts(lv, o, nprim):
    tie, unit, whole, zero = point_cells(lv, o, cube_side(nprim))
    return {"face_ties": int(tie.sum()), "unit_sc_tc": int(unit.sum()), "whole_cells": int(whole.sum()),
            "zero_sc_tc": int(zero.sum())}


MIN_TIES = 64


# ---- what every row must meet (the oracle alone; no kernel is measured) ---------------------------
def oracle_shadowed(scene, li, o):
    """cpu/light.c:24-31 per origin through the oracle's collide_dist."""
    import adversarial_util as adv
    L = scene.s.lights[li]
    lv = np.array([L.v.x, L.v.y, L.v.z], F32)
    o = np.asarray(o, F32)
    d = np.tile(-lv, (len(o), 1)) if int(L.type) == DIRECTIONAL else lv[None, :] - o
    return adv.oracle_dists(scene, o, d.astype(F32)) != 0


def check_share(r, shadowed, face=None):
    """The row's condition on a brute-force (or oracle) answer over origins()."""
    share = float(np.mean(shadowed))
    if r[4] == NOTHING:
        assert share == 0.0, (r[0], share)
    elif r[4] == ENCLOSED:  # from the box's own faces too (t = 0 on the origin's face is no hit: the opposite one)
        inner = np.asarray(shadowed)[face_slice() if face is None else face]
        assert inner.all() and share == 1.0, (r[0], share, float(inner.mean()))
    else:
        assert 0.01 < share < 0.99, (r[0], share)
    return share


def check_conditions(r, scene):
    """The figures of a row from the oracle and the restated cell arithmetic;
    asserts what the row is meant to do.  scene: the row's rtgpu.Scene."""
    o = origins()
    sh = oracle_shadowed(scene, 1, o)
    out = {"origins": len(o), "shadowed": int(sh.sum()), "share": round(check_share(r, sh), 6)}
    if r[1] == POINT:
        out.update(tie_counts(r[2], o, scene.triangle_count))
        if r[3]:
            for k in ("face_ties", "unit_sc_tc", "whole_cells"):
                assert out[k] >= MIN_TIES, (r[0], k, out[k])
    return out


# ---- the committed fixtures (tests/golden/make_golden_lights.py) -----------------------------------
def load_manifest():
    with open(os.path.join(LIGHTS, "manifest.json")) as f:
        return json.load(f)


def scene_path(case, tmpdir):
    dst = os.path.join(str(tmpdir), case["svati"][:-3])
    with gzip.open(os.path.join(LIGHTS, case["svati"]), "rb") as i, open(dst, "wb") as f:
        f.write(i.read())
    return dst


def golden(case):
    with gzip.open(os.path.join(LIGHTS, case["file"]), "rb") as f:
        data = f.read()
    return np.frombuffer(data, dtype=np.float32).reshape(case["height"], case["width"], 3)


# ---- the synthetic sphere field (curved meshes, many cells, big footprints) -------------------------
# The near point rows on Scene.synthetic(3, 3, 9776, seed=0x5EED): nine spheres of radius 0.8 to 1.1 resting
# on a ground quad [-8.5, 8.5] x [-14, 3] at y = 0, their centres 3 apart around (0, ., -5.5).  A row keeps its
# role there, not its coordinates (moved affinely, the lattice centre is the centre of the middle sphere).
FIELD_POINTS = {
    "point lattice centre": (-1.5, 0.5, -7.0),         # among the geometry: in the gap between four spheres
    "point wall plane": (12.0, 0.0, -5.5),             # in the ground's plane, outside the ground
    "point box corner": (-8.5, 0.0, -14.0),            # a corner of the triangle box (and of the ground)
    "point inside the closed box": (0.0, 1.0, -5.5),   # inside the closed middle sphere: ENCLOSED there too
}
# Not on the sphere field, and why (tests/test_light_edges.py lists them):
FIELD_LEFT_OUT = {
    "dir zero": "no grid, so no buffer to probe through; the mixed-state test renders it on the sphere field",
    "point wall vertex": "a light on a mesh vertex: every ray towards it reaches the mesh at the light itself, so the "
                         "share is 1 but for rounding and the 1-99 % condition cannot hold; "
                         "test_gpu.py::test_light_buffer_point_light_near_surface puts a light on and just above a "
                         "sphere's vertex",
}
GROUND_SHRINK = 0.25  # for the directions that leave downwards, about GROUND_C: the whole ground takes every ray
GROUND_C = (0.0, 0.0, -5.5)


def leaves_downwards(r):
    return r[1] == DIRECTIONAL and r[2][1] > 1e-3


def place(r, lo, hi):
    """The row's vector for a scene whose triangle box is [lo, hi]: a
    direction as it is, a position moved from the table's [-4, 4]^3 (the near
    rows on the sphere field: FIELD_POINTS)."""
    if r[1] == DIRECTIONAL:
        return tuple(float(c) for c in r[2])
    if r[0] in FIELD_POINTS:
        return FIELD_POINTS[r[0]]
    c, R = 0.5 * (np.asarray(lo, np.float64) + hi), 0.5 * float(np.max(np.asarray(hi) - lo))
    return tuple(float(F32(max(-3e38, min(3e38, c[a] + r[2][a] * R / 4.0)))) for a in range(3))  # (3e38 stays finite)


# ---- the host contract program's second pass (tests/native/lightbuf_geom.cpp) ------------------------
GEOM_SCALE = 5.0  # the table's [-4, 4]^3 to the program's [-20, 20]^3


def geom_rows():
    """[(name, type, vector)] as the program holds them: positions scaled to its
    box, directions as they are (their length is what the row is about)."""
    out = []
    for name, t, v, _, _, _ in ROWS:
        out.append((name, t, tuple(float(F32(c)) for c in v) if t == DIRECTIONAL else
                    tuple(float(F32(max(-3e38, min(3e38, c * GEOM_SCALE)))) for c in v)))  # (3e38 stays finite)
    return out
