"""Host side of the per-sample G-buffer, no GPU: the word-generic tile
assembly's index map, the prim -> (object, triangle) map, and where the ABI
is declared."""
import os
import re

import numpy as np
import pytest

from conftest import REPO

GB_FUNCS = ("rt_hip_set_gbuffer", "rt_hip_gbuffer_tile_words", "rt_hip_gbuffer", "rt_hip_assemble_gbuffer",
            "rt_hip_render_image_gbuffer")


def _tiles_from_words(img, rank, nranks, rtgpu):
    """Word-generic inverse of assemble_gbuffer_numpy: rank `rank`'s tile
    buffer (tiles_per_rank x 64 x words, padding 0xffffffff) cut from an
    (H, W, words) image."""
    height, width, words = img.shape
    out = np.full((rtgpu.tiles_per_rank_host(width, height, nranks), 64, words), 0xFFFFFFFF, np.uint32)
    pix = rtgpu.tile_pixels(width, height, rank, nranks)
    ok = pix[..., 0] >= 0
    out[: len(pix)][ok] = img[pix[..., 0][ok], pix[..., 1][ok]]
    return out


@pytest.mark.parametrize("nranks", [1, 3, 8])
@pytest.mark.parametrize("W,H", [(30, 34), (100, 52), (6, 130), (2, 2), (96, 54)])
def test_assemble_gbuffer_numpy_round_trip(built, W, H, nranks):
    import rtgpu
    rng = np.random.default_rng(W * 1000 + H * 8 + nranks)
    for words in (40, 7):
        img = rng.integers(0, 2**32 - 1, (H, W, words), dtype=np.uint32)  # never the padding value
        gathered = np.stack([_tiles_from_words(img, r, nranks, rtgpu) for r in range(nranks)])
        back = rtgpu.assemble_gbuffer_numpy(gathered, W, H, nranks, words=words)
        assert back.shape == (H, W, words) and np.array_equal(back, img)
    assert rtgpu.gbuffer_tile_words(W, H, nranks) == rtgpu.tiles_per_rank_host(W, H, nranks) * 64 * 40
    # the G-buffer's words as records
    smp = rtgpu.assemble_gbuffer_numpy(np.zeros((nranks, gathered.shape[1], 64, 40), np.float32), W, H, nranks)
    assert np.ascontiguousarray(smp).view(rtgpu.GSAMPLE).shape == (H, W, 4)


def test_prim_object_triangle_matches_prefix_sums(built, scene_dir):
    import rtgpu
    s = rtgpu.Scene.load_svati(os.path.join(scene_dir, "car-on-road.svati"))
    counts = [int(s.s.objects[i].triangle_count) for i in range(s.s.object_count)]
    assert len(counts) > 1 and sum(counts) == len(s.triangles_array()) == s.triangle_count
    base = np.concatenate([[0], np.cumsum(counts)])
    tris = s.triangles_array()
    rng = np.random.default_rng(5)
    prims = set(rng.integers(0, sum(counts), 200).tolist()) | set(base[:-1].tolist()) | set((base[1:] - 1).tolist())
    for p in sorted(prims):
        if p < 0:
            continue
        o, t = rtgpu.prim_object_triangle(s, p)
        assert base[o] <= p < base[o + 1] and t == p - base[o]
        # the same triangle: the object's array at t == the concatenation at p
        obj = s.s.objects[o].triangles[t]
        assert (obj.vertex[0].x, obj.vertex[2].z, obj.normal[1].y) == \
            (tris[p, 0, 0], tris[p, 2, 2], tris[p, 4, 1])
    assert rtgpu.prim_object_triangle(s, -1) == (-1, -1)
    with pytest.raises(IndexError):
        rtgpu.prim_object_triangle(s, sum(counts))


def test_coverage_values():
    import rtgpu
    smp = np.zeros((1, 5, 4), rtgpu.GSAMPLE)
    smp["prim"] = -1
    for k in range(5):
        smp["prim"][0, k, :k] = 3
    assert rtgpu.coverage(smp).tolist() == [[0.0, 0.25, 0.5, 0.75, 1.0]]
    assert rtgpu.coverage(smp).dtype == np.float32


def test_gbuffer_abi_is_in_the_drop_in_header():
    def decls(h):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", h)).read(), flags=re.S)
        return {m.group(1) for m in re.finditer(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(rt_\w+)\s*\(", src, re.M)}
    pub, tst = decls("rt_hip.h"), decls("rt_hip_test.h")
    for fn in GB_FUNCS:
        assert fn in pub and fn not in tst, fn
    src = open(os.path.join(REPO, "include", "rt_hip.h")).read()
    assert re.search(r"#define\s+RT_GB_WORDS\s+10\b", src)
    assert "typedef struct rt_gsample { int prim, obj, queries; float dist, P[3], N[3]; } rt_gsample;" in src


def test_gbuffer_abi_is_exported_and_bound(built):
    import ctypes as C
    import rtgpu
    L = C.CDLL(rtgpu.LIB_PATH)
    bound = {p[0] for p in rtgpu._PROTOS}
    for fn in GB_FUNCS:
        assert hasattr(L, fn) and fn in bound, fn
    assert rtgpu.GSAMPLE.itemsize == 40 and rtgpu.GSAMPLE.names == ("prim", "obj", "queries", "dist", "P", "N")
