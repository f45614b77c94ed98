"""Shared by tests/test_direct_light_host.py and tests/test_direct_light.py:
the reference for rt_hip_direct_light -- the oracle's apply_light per record
and its collide_dist per (record, casting light) -- the block of edge records,
and the word-for-word comparison (a NaN as any NaN, no tolerance)."""
import contextlib
import ctypes as C

import numpy as np

F32 = np.float32


class Vec(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Ray(C.Structure):
    _fields_ = [("origin", Vec), ("direction", Vec)]


def oracle_lib():
    import oracle as orc
    L = orc.lib()
    L.oracle_apply_light.argtypes = [C.c_void_p, C.c_int, Ray]
    L.oracle_apply_light.restype = orc.ColorS
    L.oracle_collide_dist.argtypes = [C.c_void_p, Ray]
    L.oracle_collide_dist.restype = C.c_float
    return L, orc


def _vec(v):
    return Vec(float(v[0]), float(v[1]), float(v[2]))


def oracle_direct_light(scene, records, lights=None):
    """(rgb (n, 3) float32, uint32 (n,) masks) of the reference for GSAMPLE
    records on an rtgpu.Scene: oracle_apply_light(scene, obj, (P, N)) for every
    record that shades, and bit li < 32 set iff light li casts and
    oracle_collide_dist of its shadow ray (rtgpu.shadow_rays_host) is 0; zeros
    for a record that does not shade.  lights: the scene's own unless given (a
    context edited away from its scene needs an edited scene, not this)."""
    import rtgpu
    L, _ = oracle_lib()
    sp = C.cast(scene.ptr, C.c_void_p)
    r = np.ascontiguousarray(records, dtype=rtgpu.GSAMPLE).reshape(-1)
    shades = rtgpu.direct_light_shades(r, int(scene.s.object_count))
    rgb = np.zeros((len(r), 3), F32)
    mask = np.zeros(len(r), np.uint32)
    lights = scene.lights() if lights is None else lights
    rays = rtgpu.shadow_rays_host(r, lights)
    cast = rtgpu.casting_lights(lights)
    assert len(rays) == len(cast)
    for i in np.flatnonzero(shades):
        c = L.oracle_apply_light(sp, int(r["obj"][i]), Ray(_vec(r["P"][i]), _vec(r["N"][i])))
        rgb[i] = (c.r, c.g, c.b)
        m = 0
        for li, (o, d) in zip(cast, rays):
            if li < 32 and L.oracle_collide_dist(sp, Ray(_vec(o[i]), _vec(d[i]))) == 0:
                m |= 1 << li
        mask[i] = m
    return rgb, mask


@contextlib.contextmanager
def light_table(gpu, s, rows):
    """The scene with another light array (any length, rows of (type, r, g, b,
    x, y, z)) for the block: the scene's own array is the library's, so it is
    swapped out and put back."""
    arr = (gpu.Light * len(rows))()
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


def differing(a, b):
    """Rows of two (n, 3) float32 arrays that differ as 32-bit words; two NaNs
    agree whatever their bits (x86 makes -qNaN, the GPU +qNaN)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape, (a.shape, b.shape)
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return np.flatnonzero(~same.reshape(len(a), -1).all(axis=1))


def assert_same(got_rgb, got_mask, want_rgb, want_mask, what, scene=None, records=None):
    """Every record, no tolerance: the list of pairs that a pow rounding could
    excuse (oracle.spec_pow_ld, as test_pow_sweep lists them) is empty, so any
    differing word fails."""
    bad = differing(got_rgb, want_rgb)
    assert len(bad) == 0, (what, f"{len(bad)} of {len(got_rgb)} colours differ from the reference", bad[:5].tolist(),
                           got_rgb[bad[:3]].tolist(), want_rgb[bad[:3]].tolist(),
                           None if records is None else records[bad[:3]].tolist())
    if got_mask is not None:
        badm = np.flatnonzero(np.asarray(got_mask) != np.asarray(want_mask))
        assert len(badm) == 0, (what, f"{len(badm)} of {len(got_mask)} masks differ", badm[:5].tolist(),
                                [hex(int(x)) for x in np.asarray(got_mask)[badm[:5]]],
                                [hex(int(x)) for x in np.asarray(want_mask)[badm[:5]]])


def edge_block(dtype, nobj):
    """Records at the predicate's edges.  -> (records, shades): a miss, obj =
    -1 and obj = the object count, zero and -0.0 normals, an inf and a NaN in
    P and in N (none shades); a denormal N, a non-unit N, P = 0, the last
    object (all shade)."""
    nan, inf = np.nan, np.inf
    den = float(np.finfo(F32).smallest_subnormal)
    rows = [  # prim, obj, P, N, shades
        (-1, 0, (1, 2, 3), (0, 1, 0), False),
        (0, -1, (1, 2, 3), (0, 1, 0), False),
        (0, nobj, (1, 2, 3), (0, 1, 0), False),
        (0, 0, (1, 2, 3), (0, 0, 0), False),
        (0, 0, (1, 2, 3), (-0.0, 0.0, -0.0), False),
        (0, 0, (inf, 2, 3), (0, 1, 0), False),
        (0, 0, (1, nan, 3), (0, 1, 0), False),
        (0, 0, (1, 2, -inf), (0, 1, 0), False),
        (0, 0, (1, 2, 3), (inf, 1, 0), False),
        (0, 0, (1, 2, 3), (0, nan, 0), False),
        (0, 0, (1, 2, 3), (0, 1, -inf), False),
        (-2147483648, 0, (0, 0, 0), (0, 0, 0), False),
        (0, 0, (1, 2, 3), (den, 0, 0), True),
        (0, 0, (1, 2, 3), (0, -den, 0), True),
        (7, 0, (1, 2, 3), (3, -4, 12), True),
        (2147483647, nobj - 1, (0, 0, 0), (0, 0, 1), True),
        (0, 0, (-0.0, 0.0, -0.0), (0, -1, -0.0), True),
    ]
    r = np.zeros(len(rows), dtype)
    for k, (prim, obj, P, N, _) in enumerate(rows):
        r["prim"][k], r["obj"][k] = prim, obj
        r["P"][k], r["N"][k] = P, N
    r["dist"] = 1.0
    return r, np.array([row[4] for row in rows], bool)
