"""Shared by tests/test_geometry_host.py and tests/test_geometry_words.py: an
independent numpy float32 reference of what the flatten derives from a scene's
triangles (host/accel.c rt_flatten, csrc/rt_geom.hip), the comparison rule,
seeded triangles whose every word is distinct, the scenes built from them and
the tables of awkward normals and vertices.  No GPU here.

The comparison rule: two float words agree if they are the same 32 bits.  In
the normal rows alone two NaNs agree whatever their bits: 0 / 0 is 0xFFC00000
on x86 and a NaN of the other sign on the GPU, nothing downstream tells them
apart, and host/rt_zero_risk.h answers 0 for any NaN."""
import itertools

import numpy as np

F32 = np.float32
FLT_MAX = F32(3.4028234663852886e38)
FLT_MIN = F32(1.17549435e-38)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- the reference -------------------------------------------------------------
def reference(tris, counts):
    """tris: (T, 6, 3) float32 (3 vertices, 3 normals), counts: the objects'
    triangle counts in order.  -> records' words 0..10 as uint32 (T, 11): v0,
    v1 - v0, v2 - v0, prim, object; normal rows (T, 9) float32: each normal
    over l = float32(sqrt(float64(s))), s = (x*x + y*y) + z*z in float32
    (host/vecmath.c:24-30, csrc/rt_device.h:34-41); vertex boxes (T, 6) and the
    scene box (6,) by np.minimum / np.maximum (whose zero's sign is
    unspecified: see same_boxes)."""
    t = np.ascontiguousarray(tris, dtype=F32).reshape(-1, 6, 3)
    T = len(t)
    assert sum(counts) == T
    v0, v1, v2 = t[:, 0], t[:, 1], t[:, 2]
    rec = np.empty((T, 11), np.uint32)
    with np.errstate(all="ignore"):
        rec[:, 0:3], rec[:, 3:6], rec[:, 6:9] = bits(v0), bits(v1 - v0), bits(v2 - v0)
        rec[:, 9] = np.arange(T, dtype=np.uint32)
        rec[:, 10] = np.repeat(np.arange(len(counts), dtype=np.uint32), counts)
        n = t[:, 3:6]
        s = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        assert s.dtype == F32
        l = np.sqrt(s.astype(np.float64)).astype(F32)
        nrm = (n / l[..., None]).astype(F32).reshape(T, 9)
    lo, hi = np.minimum(np.minimum(v0, v1), v2), np.maximum(np.maximum(v0, v1), v2)
    pbox = np.concatenate([lo, hi], axis=1)
    box = np.concatenate([lo.min(axis=0), hi.max(axis=0)]) if T else np.array([FLT_MAX] * 3 + [-FLT_MAX] * 3, F32)
    return rec, nrm, pbox, box


def object_counts(scene):
    s = scene.s
    return [int(s.objects[i].triangle_count) for i in range(int(s.object_count))]


def same_words(got, want, what):
    """Plain uint32 equality, with the first differing words in the message."""
    g, w = bits(got) if got.dtype != np.uint32 else got, bits(want) if want.dtype != np.uint32 else want
    assert g.shape == w.shape, f"{what}: shapes {g.shape} / {w.shape}"
    bad = np.argwhere(g != w)
    assert len(bad) == 0, (f"{what}: {len(bad)} words differ, first at {bad[:4].tolist()}: "
                           f"{[hex(int(g[tuple(i)])) for i in bad[:4]]} / {[hex(int(w[tuple(i)])) for i in bad[:4]]}")


def same_normals(got, want, what):
    """The rule for normal rows: the same bits, or both NaN."""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"{what}: shapes {g.shape} / {w.shape}"
    bad = np.argwhere((g != w) & ~(np.isnan(got) & np.isnan(want)))
    assert len(bad) == 0, (f"{what}: {len(bad)} normal words differ, first at {bad[:4].tolist()}: "
                           f"{[hex(int(g[tuple(i)])) for i in bad[:4]]} / {[hex(int(w[tuple(i)])) for i in bad[:4]]}")


def same_boxes(got, want, what):
    """By value (==): for boxes compared with numpy's minimum / maximum, which
    leave the sign of a zero open.  Finite input, so no NaN to excuse."""
    bad = np.argwhere(~(np.asarray(got) == np.asarray(want)))
    assert len(bad) == 0, f"{what}: {len(bad)} box values differ, first at {bad[:4].tolist()}"


def has_zero(a):
    return bool((np.asarray(a) == 0).any())


def check_against_reference(arrays, tris, counts, flags, what, box_bits=None):
    """arrays = (records (T, 12), normal rows, vertex boxes, scene box) of
    flatten_arrays / geometry_arrays against the reference of `tris`; flags:
    the expected word 11 per prim (uint32).  Boxes by bits unless a zero is
    among the expected values (box_bits overrides)."""
    rec, nrm, pbox, box = arrays
    wrec, wnrm, wpbox, wbox = reference(tris, counts)
    same_words(bits(rec)[:, :11], wrec, what + ": record words 0..10")
    same_words(bits(rec)[:, 11], np.asarray(flags, np.uint32), what + ": flag words")
    same_normals(nrm, wnrm, what + ": normal rows")
    if box_bits is None:
        box_bits = not has_zero(wpbox)
    if pbox is not None:
        (same_words if box_bits else same_boxes)(pbox, wpbox, what + ": vertex boxes")
    (same_words if box_bits else same_boxes)(box, wbox, what + ": scene box")


def same_arrays(got, want, what):
    """Two sets of arrays word for word (a context against the host flatten or
    against another context): bits everywhere, the NaN rule in the normal rows."""
    same_words(got[0], want[0], what + ": records")
    same_normals(got[1], want[1], what + ": normal rows")
    if got[2] is not None and want[2] is not None:
        same_words(got[2], want[2], what + ": vertex boxes")
    same_words(got[3], want[3], what + ": scene box")


# ---- seeded triangles, every word distinct -------------------------------------------
def distinct_triangles(n, seed):
    """(n, 6, 3) float32: small triangles (vertices within 0.25 of a centre in
    [-8, 8)^3, so that an octree over them stays small), normals of length 0.5 .. 2 within
    a cone about +z (the three unit normals of a triangle span a triangle at
    distance > 0.8 from the origin: far from the zero-normal risk, 1e-5), every
    one of the 18 n words a different finite float32."""
    rng = np.random.default_rng(seed)

    def draw(k):
        t = np.empty((k, 6, 3), F32)
        t[:, :3] = rng.uniform(-8, 8, (k, 1, 3)) + rng.uniform(-0.25, 0.25, (k, 3, 3))
        d = rng.uniform(-0.3, 0.3, (k, 3, 3))
        d[..., 2] += 1.0
        t[:, 3:] = d * rng.uniform(0.5, 2.0, (k, 3, 1))
        return t

    t = draw(n)
    for _ in range(64):
        flat = bits(t).reshape(-1)
        _, first = np.unique(flat, return_index=True)
        dup = np.ones(flat.size, bool)
        dup[first] = False
        rows = np.unique(np.flatnonzero(dup) // 18)
        if len(rows) == 0:
            break
        t[rows] = draw(len(rows))
    assert len(np.unique(bits(t))) == t.size and np.isfinite(t).all() and (t != 0).all()
    return t


def write_svati(path, tris, counts, width=32, height=18):
    """An ambient-light scene of the objects' triangles (9 significant digits:
    float32 round-trips).  The parser stacks an object's triangles LIFO, so
    the loaded order is read back from the scene, not assumed."""
    t = np.asarray(tris, F32).reshape(-1, 6, 3)
    assert sum(counts) == len(t)
    out = ["camera %d %d 0 0 -40 1 0 0 0 -1 0 60\na_light 1 1 1\n" % (width, height)]
    at = 0
    for c in counts:
        out.append("\nobject %d\nKa 1 1 1\n" % (3 * c))
        for tri in t[at:at + c]:
            out.extend("v %.9g %.9g %.9g\n" % tuple(float(x) for x in tri[k]) for k in range(3))
            out.extend("vn %.9g %.9g %.9g\n" % tuple(float(x) for x in tri[k]) for k in range(3, 6))
        at += c
    with open(path, "w") as f:
        f.write("".join(out))


EDGE_COUNTS = (300, 1, 999, 600)  # 1900 prims: no object boundary on a multiple of 256, one object of one triangle


def checked_scene(rt, path, tris, counts):
    """write_svati + load; the reference's own parser must read the same
    triangles and render the file (32x18) before anything else is done with it."""
    import oracle as orc
    write_svati(path, tris, counts)
    s = rt.Scene.load_svati(str(path))
    assert object_counts(s) == list(counts)
    got = s.triangles_array()
    # (the parser reverses an object's vertex and normal lines: the same words, another order)
    assert np.array_equal(np.sort(bits(got), axis=None), np.sort(bits(tris), axis=None)), \
        "the file does not round-trip the float32 words"
    osc = orc.OracleScene(str(path))
    assert np.array_equal(bits(rt.scene_triangles(osc.ptr)), bits(got)), "the reference parses the file differently"
    osc.set_size(32, 18)
    img, _ = orc.render(osc, 32, 18, threads=4)
    assert img.shape == (18, 32, 3) and not np.isnan(img).any()
    return s


# ---- the normals table ---------------------------------------------------------------
NORMAL_ROWS = [
    (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, -1, 0),            # unit vectors
    (3, 4, 0),
    (1e-20, 2e-20, 0),                                      # s is a denormal
    (1e-23, 0, 0),                                          # s underflows to 0: inf and NaN
    (1e20, -1e20, 1e19),                                    # s overflows: a row of signed zeros
    (0, 0, 0),                                              # NaN
    (1e-40, 1, 0),                                          # a denormal component
    (-0.0, 0.0, -1),
    (float(FLT_MAX), 0, 0),
    (float(FLT_MIN), float(FLT_MIN), 0),
]
ROW_UNDERFLOW, ROW_OVERFLOW, ROW_ZERO = 6, 7, 8


def normal_table(n):
    """(n, 3, 3) float32 and the (n, 3) row indices: triangle i < len(NORMAL_ROWS)
    has row i three times, the others cycle n0 / n1 / n2 through the rows at
    different rates (every (n0, n1) pair occurs within the first 13 + 169)."""
    R = len(NORMAL_ROWS)
    i = np.arange(n)
    j = i - R
    idx = np.where((i < R)[:, None], np.stack([i % R] * 3, 1), np.stack([j % R, (j // R) % R, (7 * j + j // R) % R], 1))
    return np.array(NORMAL_ROWS, F32)[idx], idx


# ---- the vertex table ----------------------------------------------------------------
NZ, PZ = -0.0, 0.0
ZERO_LO = list(itertools.permutations((NZ, PZ, 5.0)))    # the six vertex orders: lo is a zero
ZERO_HI = list(itertools.permutations((-5.0, NZ, PZ)))   # hi is a zero
COORD_TRIPLES = ZERO_LO + ZERO_HI + [
    (PZ, PZ, PZ), (NZ, NZ, NZ), (PZ, NZ, NZ), (NZ, PZ, PZ), (NZ, PZ, NZ), (PZ, NZ, PZ),
    (1e-40, -1e-40, 2e-40), (1e-40, 1e-40, NZ), (-1e-40, PZ, -2e-40),     # denormals
    (1e30, -1e30, 0.5), (-1e30, -1e30, 1e30), (1e30, 1e30, 1e30),
    (2.5, 2.5, 2.5),                                                       # three identical coordinates
]


def vertex_table(n, triples=None):
    """(n, 3, 3) float32 vertices [tri][vertex][axis]: axis a of triangle i
    takes the triple at a rate of its own, so every triple meets every axis;
    the first len(triples) triangles have the same triple on all three axes
    (among them three identical vertices)."""
    tr = np.array(COORD_TRIPLES if triples is None else triples, F32)
    K = len(tr)
    i = np.arange(n)
    j = i - K
    idx = np.where((i < K)[:, None], np.stack([i % K] * 3, 1), np.stack([j % K, (j // K) % K, (5 * j + j // K) % K], 1))
    return np.transpose(tr[idx], (0, 2, 1)).copy()  # [tri][axis][vertex] -> [tri][vertex][axis]


# ---- the risk threshold --------------------------------------------------------------
K_ROWS = [  # tests/native/zero_risk_twin.cpp kRows, as normals
    (0, 0, 1, 0, 0, 1, 0, 0, 1),
    (0, 0, 1, 0, 0, -1, 0, 0, 1),
    (0, 0, 1, 0, 0, -1, 0, 0, -1),
    (1, 0, 0.99e-5, -1, 0, 0.99e-5, 0, 1, 0.99e-5),
    (1, 0, 1.01e-5, -1, 0, 1.01e-5, 0, 1, 1.01e-5),
    (1, 0, -0.99e-5, -1, 0, -0.99e-5, 0, 1, -0.99e-5),
    (1, 0, -1.01e-5, -1, 0, -1.01e-5, 0, 1, -1.01e-5),
    (0, 0, 1, np.nan, np.nan, np.nan, 0, 0, -1),
    (0, 0, 1, 0, 0, -1, 0, np.nan, 1),
]
K_ROWS_RISK = [0, 1, 1, 1, 0, 1, 0, 0, 0]


def threshold_d():
    """The 17 consecutive float32 values centred on float32(1e-5)."""
    d = [F32(1e-5)]
    for _ in range(8):
        d.insert(0, np.nextafter(d[0], F32(0)))
        d.append(np.nextafter(d[-1], F32(1)))
    return np.array(d, F32)


def risk_normals():
    """(43, 3, 3) float32: K_ROWS, then normals (1, 0, d), (-1, 0, d), (0, 1, d)
    for d in threshold_d() and in -threshold_d(); with the index ranges of the
    two signs."""
    rows = [np.array(r, F32).reshape(3, 3) for r in K_ROWS]
    for sign in (1, -1):
        for d in threshold_d():
            rows.append(np.array([[1, 0, sign * d], [-1, 0, sign * d], [0, 1, sign * d]], F32))
    return np.stack(rows), (slice(9, 26), slice(26, 43))
