"""Shared by tests/test_adversarial_host.py, tests/test_adversarial.py and
tests/golden/make_golden_adversarial.py: the loader of tests/golden/adversarial/,
the oracle's collide / collide_dist per ray, the exact-in-float32 ray sets and
the conditions every adversarial fixture must meet (so that editing a fixture
cannot silently empty a test).  No GPU here."""
import ctypes as C
import gzip
import json
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)
ADV = os.path.join(TESTS, "golden", "adversarial")
for _p in (os.path.join(REPO, "raytracing-gpu_amd"), os.path.join(REPO, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

F32 = np.float32


# ---- fixtures -----------------------------------------------------------------
def load_manifest():
    with open(os.path.join(ADV, "manifest.json")) as f:
        return json.load(f)["cases"]


def case_id(case):
    return f'{case["scene"]}_{case["width"]}x{case["height"]}'


def scene_path(case, tmpdir):
    """The case's .svati, unpacked into tmpdir."""
    dst = os.path.join(str(tmpdir), case["svati"][:-3])
    with gzip.open(os.path.join(ADV, case["svati"]), "rb") as i, open(dst, "wb") as o:
        o.write(i.read())
    return dst


def golden(case):
    with gzip.open(os.path.join(ADV, case["file"]), "rb") as f:
        data = f.read()
    return np.frombuffer(data, dtype=np.float32).reshape(case["height"], case["width"], 3)


# ---- the oracle per ray ---------------------------------------------------------
class _Vec(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class _Ray(C.Structure):
    _fields_ = [("origin", _Vec), ("direction", _Vec)]


_L = None


def _oracle():
    global _L
    if _L is None:
        import oracle as orc
        orc.lib()
        L = C.CDLL(orc.LIB)  # a handle of our own: its prototypes are ours
        L.oracle_collide.argtypes = [C.c_void_p, _Ray, C.POINTER(C.c_int)]
        L.oracle_collide.restype = _Ray
        L.oracle_collide_dist.argtypes = [C.c_void_p, _Ray]
        L.oracle_collide_dist.restype = C.c_float
        _L = L
    return _L


def oracle_collide(scene, o, d):
    """collide() of cpu/hit.c:72-91 per ray -> (obj (n,) int32, -1 for a miss;
    P (n, 3) and N (n, 3) float32, zero for a miss)."""
    L, sp = _oracle(), C.cast(scene.ptr, C.c_void_p)
    n = len(o)
    obj, P, N = np.full(n, -1, np.int32), np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    for i in range(n):
        oi = C.c_int(-1)
        h = L.oracle_collide(sp, _Ray(_Vec(*map(float, o[i])), _Vec(*map(float, d[i]))), C.byref(oi))
        nrm = (h.direction.x, h.direction.y, h.direction.z)
        if nrm != (0.0, 0.0, 0.0):
            obj[i], P[i], N[i] = oi.value, (h.origin.x, h.origin.y, h.origin.z), nrm
    return obj, P, N


def oracle_dists(scene, o, d):
    """collide_dist() of cpu/hit.c:93-109 per ray -> float32 (n,), 0 = nothing."""
    L, sp = _oracle(), C.cast(scene.ptr, C.c_void_p)
    return np.array([L.oracle_collide_dist(sp, _Ray(_Vec(*map(float, o[i])), _Vec(*map(float, d[i]))))
                     for i in range(len(o))], F32)


# ---- ray sets (twins: wall in z = 2 on [-4, 4]^2, cube [-1, 1]^3, floor pair in y = -2) ----
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
DIAGONALS = [(0.5, 0.5, 0.0), (0.5, -0.5, 0.0), (0.5, 0.5, 0.5)]
QUARTER = np.arange(-20, 21, dtype=np.float64) * 0.25  # 41 values, -5 .. 5


def _axis_dir(axis, scale, zero):
    """scale * axis with `zero` (+0.0 or -0.0) in the two other components."""
    return np.array([scale * a if a else zero for a in axis], F32)


def lattice_rays(zero):
    """Axis-parallel rays over the twins scene: for each of +-x, +-y, +-z the
    unit vector and half of it, `zero` in the zero components, from the 41 x 41
    quarter lattice of [-5, 5]^2 in a plane 20 units outside the scene box
    [-4, 4]^2 x [-2, 2] (12 x 1681 rays)."""
    g = np.stack(np.meshgrid(QUARTER, QUARTER, indexing="ij"), -1).reshape(-1, 2)
    o, d = [], []
    for axis in AXES:
        a = int(np.flatnonzero(axis)[0])
        far = (24.0 if a < 2 else 22.0) * -axis[a]
        org = np.zeros((len(g), 3))
        org[:, a] = far
        org[:, [b for b in range(3) if b != a]] = g
        for scale in (1.0, 0.5):
            o.append(org.astype(F32))
            d.append(np.tile(_axis_dir(axis, scale, zero), (len(g), 1)))
    return np.concatenate(o), np.concatenate(d)


def diagonal_rays():
    """(0.5, 0.5, 0), (0.5, -0.5, 0) and (0.5, 0.5, 0.5) through every point of
    the quarter lattice of the plane x = 0, from 48 steps before it: through
    vertices, along quad diagonals and inside z = 2 and z = +-1 (3 x 1681 rays)."""
    g = np.stack(np.meshgrid(QUARTER, QUARTER, indexing="ij"), -1).reshape(-1, 2)
    p = np.concatenate([np.zeros((len(g), 1)), g], axis=1)
    o, d = [], []
    for dv in DIAGONALS:
        dv = np.array(dv)
        o.append((p - 48.0 * dv).astype(F32))
        d.append(np.tile(dv.astype(F32), (len(p), 1)))
    return np.concatenate(o), np.concatenate(d)


def inside_rays():
    """The same 24 axis directions and the three diagonals from the integer
    lattice of [-4, 4]^2 at z in {-2, -1, -0.5, 0, 1, 2}: origins inside the
    box and on the planes of the cube's faces, the wall and the floor pair
    (t = 0) (27 x 486 rays)."""
    xy = np.arange(-4, 5, dtype=np.float64)
    org = np.stack(np.meshgrid(xy, xy, [-2.0, -1.0, -0.5, 0.0, 1.0, 2.0], indexing="ij"), -1).reshape(-1, 3)
    o, d = [], []
    for axis in AXES:
        for scale in (1.0, 0.5):
            for zero in (0.0, -0.0):
                o.append(org.astype(F32))
                d.append(np.tile(_axis_dir(axis, scale, zero), (len(org), 1)))
    for dv in DIAGONALS:
        o.append(org.astype(F32))
        d.append(np.tile(np.array(dv, F32), (len(org), 1)))
    return np.concatenate(o), np.concatenate(d)


THRESHOLD_XY = [(2.5, 2.5), (-2.5, 2.25), (3.25, -2.5), (-3.75, -1.5)]


def threshold_z():
    """The 17 consecutive floats centred on float32(2.01)."""
    z = [F32(2.01)]
    for _ in range(8):
        z.insert(0, np.nextafter(z[0], F32(0)))
        z.append(np.nextafter(z[-1], F32(4)))
    return np.array(z, F32)


def threshold_rays():
    """From behind the twins' wall (z = 2) towards it, (0, 0, -1) and (0, 0,
    -0.5), the origin's z stepping through threshold_z(): new_dist passes
    cpu/hit.c's 0.01 from both sides (2 x 4 x 17 rays, away from the cube)."""
    o, d = [], []
    for dz in (-1.0, -0.5):
        for x, y in THRESHOLD_XY:
            for z in threshold_z():
                o.append((x, y, z))
                d.append((0.0, 0.0, dz))
    return np.array(o, F32), np.array(d, F32)


def sliver_rays(scene, case):
    """Unit rays aimed at the centroids of the slivers scene's needles and
    sweep triangles, from the eye and from 3 seeded origins each."""
    tri = scene.triangles_array()
    lo, hi = case["sweep_prims"]
    nl, nh = case["needle_prims"]
    cen = np.concatenate([tri[lo:hi, :3], tri[nl:nh, :3]]).astype(np.float64).mean(axis=1)
    cam = scene.camera
    eye = np.array([cam.position.x, cam.position.y, cam.position.z], np.float64)
    rng = np.random.default_rng(20261020)
    org = np.concatenate([np.tile(eye, (len(cen), 1))] +
                         [eye + rng.uniform(-3.0, 3.0, (len(cen), 3)) for _ in range(3)])
    tgt = np.tile(cen, (4, 1))
    dv = tgt - org
    dv /= np.linalg.norm(dv, axis=1, keepdims=True)
    return org.astype(F32), dv.astype(F32)


def twins_ray_sets():
    return {"lattice+0": lattice_rays(0.0), "lattice-0": lattice_rays(-0.0), "diagonal": diagonal_rays(),
            "inside": inside_rays(), "threshold": threshold_rays()}


# ---- what every fixture must meet -------------------------------------------------
TWIN_PAIRS = [(0, 1), (2, 3), (4, 5)]  # twins: object pairs holding the same triangles
ROOM_SPECIAL = {"straddles eye and film planes": 7, "between film and eye": 8, "behind the film": 9}


def check_conditions(case, s, gold):
    """The conditions of a committed case, from the reference's golden and the
    oracle alone.  s: the rtgpu.Scene of the case.  Returns a dict of figures."""
    import oracle as orc
    import rtgpu
    W, H = case["width"], case["height"]
    out = {}
    assert not np.isnan(gold).any(), "NaN in the golden"
    _, cnt = orc.render(s.ptr, W, H, threads=0)
    assert cnt["max_depth"] >= 1, cnt
    pr = rtgpu.accel_probe(s, "octree", 1, True)
    share = pr["shadow_hits"] / pr["shadow_queries"]
    assert 0.05 <= share <= 0.95, ("shadow-hit share", share)
    out["shadow_share"] = share
    o, d = rtgpu.camera_rays(s.frame(), "pixel")
    if case["scene"] == "twins":
        obj, _, _ = oracle_collide(s, o, d)
        tri = s.triangles_array()[:, :3]
        keys = [frozenset(map(tuple, t.tolist())) for t in tri]
        assert all(keys.count(k) == 2 for k in set(keys)), "every triangle exists twice"
        hit = obj >= 0
        assert hit.mean() >= 0.5, ("camera samples on a twinned triangle", hit.mean())
        assert (obj[hit] % 2 == 0).all(), "a later twin won"
        assert set(np.unique(obj[hit])) == {0, 2, 4}, np.unique(obj[hit])
        mats = rtgpu.scene_materials(s.ptr)
        assert mats[0, 11] > 0 and mats[2, 11] > 0 and mats[4, 11] == 0 and mats[5, 11] > 0
        out["hit_share"] = float(hit.mean())
    if case["scene"] == "room":
        assert rtgpu.accel_build_info(s, "octree")["max_depth"] >= 2
        wins = {k: 0 for k in ROOM_SPECIAL.values()}
        for row in range(H):
            for col in range(W):
                qs, _ = orc.diag_pixel(C.cast(s.ptr, C.c_void_p), row, col, max_queries=1024)
                for q in qs:
                    if q["kind"] in ("camera", "reflection") and q["obj"] in wins:
                        wins[q["obj"]] += 1
        assert all(v > 0 for v in wins.values()), ("special objects' wins", wins)
        out["special_wins"] = wins
        if W == 96:
            colours = len(np.unique(gold.reshape(-1, 3).view(np.uint32), axis=0))
            assert colours >= 100, colours
            out["colours"] = colours
    if case["scene"] == "slivers":
        lo, hi = case["sweep_prims"]
        tri = s.triangles_array()
        assert hi - lo == 80 and case["needle_prims"][1] - case["needle_prims"][0] == 19
        v = tri[lo:hi, :3].astype(np.float64)
        legs = np.sort(np.linalg.norm(v[:, [1, 2, 0]] - v, axis=2), axis=1)[:, :2]  # the two short edges
        # (float32 vertices near 1: the legs are exact to about 1e-7)
        assert np.allclose(legs[:, 0], legs[:, 1], rtol=1e-3) and legs.min() < 2.0 ** -10
        assert abs(legs.max() - 2.0 ** -6) < 1e-6
        rects = np.tile(np.array([0, 0, H, W], np.int32), (hi - lo, 1))
        acc = orc.camera_tri_accepts(s.ptr, tri[lo:hi], rects)
        assert (acc[:, 0] == 0).any(), "every sweep triangle is accepted by some camera sample"
        assert (acc[:, 0] > 0).any(), "no sweep triangle is accepted by any camera sample"
        out["sweep_accepted"] = int((acc[:, 0] > 0).sum())
        area = np.linalg.norm(np.cross(tri[:, 1, :].astype(np.float64) - tri[:, 0], tri[:, 2, :].astype(np.float64) - tri[:, 0]), axis=1)
        assert (area == 0).sum() == 2, "two zero-area triangles"
    return out
