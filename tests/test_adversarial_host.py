"""The adversarial fixtures (tests/golden/make_golden_adversarial.py: twins,
room, slivers) without a GPU: the oracle renders each as the reference did,
the host octree and its walk model hold on them, the tile refinement of the
camera candidate lists drops nothing the reference accepts, the conditions
the fixtures were built to meet still hold in the committed files, and the
ray sets are what tests/test_adversarial.py says it sends."""
import hashlib

import numpy as np
import pytest

import adversarial_util as adv

CASES = adv.load_manifest()
BIG = [c for c in CASES if c["width"] == 96]


def _scene(case, tmp_path):
    import rtgpu
    return rtgpu.Scene.load_svati(adv.scene_path(case, tmp_path))


def test_manifest_lists_every_scene_at_both_sizes():
    assert sorted((c["scene"], c["width"], c["height"]) for c in CASES) == sorted(
        (s, w, h) for s in ("twins", "room", "slivers") for w, h in ((32, 18), (96, 54)))
    for c in CASES:  # the float images are the ones the manifest was written for
        assert hashlib.sha256(adv.golden(c).tobytes()).hexdigest() == c["f32_sha256"], adv.case_id(c)


@pytest.mark.parametrize("case", CASES, ids=[adv.case_id(c) for c in CASES])
def test_oracle_matches_reference(case, built, tmp_path):
    """The oracle's restatement renders every adversarial case bit for bit as
    the reference cpu/rt did, with its query counts."""
    import oracle as orc
    sc = orc.OracleScene(adv.scene_path(case, tmp_path))
    img, cnt = orc.render(sc, case["width"], case["height"], threads=0)
    gold = adv.golden(case)
    assert np.array_equal(img.view(np.uint32), gold.view(np.uint32)), \
        f"{int((img.view(np.uint32) != gold.view(np.uint32)).any(axis=2).sum())} pixels differ"
    assert cnt["closest"] == case["closest"] and cnt["shadow"] == case["shadow"]
    assert cnt["max_depth"] >= 1


@pytest.mark.parametrize("case", CASES, ids=[adv.case_id(c) for c in CASES])
def test_host_octree_and_walk_model(case, built, tmp_path):
    """Both accelerators validate; the host model of the device walk agrees
    with brute force on every camera sample's closest hit and shadow rays."""
    import rtgpu
    s = _scene(case, tmp_path)
    rtgpu.accel_validate(s, "octree")
    rtgpu.accel_validate(s, "flat")
    pr = rtgpu.accel_probe(s, "octree", 1, True)
    assert pr["mismatches"] == 0, pr
    assert pr["hits"] > 0 and pr["shadow_hits"] > 0, pr


@pytest.mark.parametrize("case", BIG, ids=[adv.case_id(c) for c in BIG])
def test_tile_refinement_drops_only_never_accepted_tiles(case, built, tmp_path):
    """test_exact.py's tile-refinement check on the 96x54 scenes: triangles
    around the eye, twins and slivers.  No dropped (triangle, tile) passes the
    oracle's a, u, v stages on any camera sample of the tile, some kept tile is
    really hit, and the survey partitions the triangles."""
    import oracle as orc
    import rtgpu
    s = _scene(case, tmp_path)
    r = rtgpu.cand_survey(s, 64.0, 1.0)
    assert r["safe"] + r["footprint"] + r["global"] == s.triangle_count
    assert sum(h[2] for h in r["hist"]) == r["entries"]
    rows, total = rtgpu.cand_refine_sample(s, stride=1, cap=1 << 20)
    assert len(rows) == total
    assert total > 0
    drop = rows[:, 3] == 0
    tris = s.triangles_array()
    rects = np.stack([rows[:, 2] * 8, rows[:, 1] * 8, np.full(len(rows), 8), np.full(len(rows), 8)], 1)
    acc = orc.camera_tri_accepts(s.ptr, tris[rows[:, 0]], rects)
    if drop.any():
        assert int(acc[drop, 1].max()) == 0, rows[drop][acc[drop, 1] > 0][:8]
    assert int((acc[~drop, 0] > 0).sum()) > 0  # real hits live in kept tiles


@pytest.mark.parametrize("case", CASES, ids=[adv.case_id(c) for c in CASES])
def test_zero_area_triangles_are_global_candidates(case, built, tmp_path):
    """slivers' two zero-area triangles have edges long enough for rounding to
    lift |a| past cpu/hit.c's 1e-7: no line has a bound, so classify() sends
    them to the global list.  (With |n| = 0 it once divided by it: NaN band
    coefficients, a footprint of 12 of the frame's 84 tiles, and a device
    footprint that the host re-derivation could never equal.)  Nothing else
    of the fixtures is global, and the survey still partitions the triangles."""
    import rtgpu
    s = _scene(case, tmp_path)
    r = rtgpu.cand_survey(s, 64.0, 1.0)
    assert r["global"] == (2 if case["scene"] == "slivers" else 0), r
    assert r["safe"] + r["footprint"] + r["global"] == s.triangle_count


@pytest.mark.parametrize("case", CASES, ids=[adv.case_id(c) for c in CASES])
def test_fixture_conditions_hold(case, built, tmp_path):
    """What the generator asserted, again from the committed files."""
    figures = adv.check_conditions(case, _scene(case, tmp_path), adv.golden(case))
    assert 0.05 <= figures["shadow_share"] <= 0.95


def _signs(d):
    """(components that are +0.0, components that are -0.0) per ray."""
    zero = d == 0
    neg = np.signbit(d)
    return (zero & ~neg).sum(axis=1), (zero & neg).sum(axis=1)


def test_ray_sets_are_what_they_say():
    sets = adv.twins_ray_sets()
    for name, (o, d) in sets.items():
        assert o.dtype == d.dtype == np.float32 and o.shape == d.shape and o.shape[1] == 3, name
        ln = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
        assert ln.min() >= 0.5 and ln.max() <= 1.0625, name
        # exact in float32: multiples of 1/4 (the threshold set's z apart)
        if name != "threshold":
            assert np.array_equal(o * 4, np.round(o * 4)) and np.array_equal(d * 2, np.round(d * 2)), name
    assert len(sets["lattice+0"][0]) == len(sets["lattice-0"][0]) == 12 * 1681
    pz, nz = _signs(sets["lattice+0"][1])
    assert (pz == 2).all() and (nz == 0).all()
    pz, nz = _signs(sets["lattice-0"][1])
    assert (pz == 0).all() and (nz == 2).all()
    assert np.array_equal(sets["lattice+0"][1], sets["lattice-0"][1])  # (0.0 == -0.0: the same rays but for the sign bit)
    o, d = sets["lattice+0"]
    assert len(np.unique(d, axis=0)) == 12
    assert (np.abs(o).max(axis=1) >= 22).all()  # 20 units outside [-4, 4]^2 x [-2, 2]
    assert len(sets["diagonal"][0]) == 3 * 1681
    pz, nz = _signs(sets["diagonal"][1])
    assert (nz == 0).all() and sorted(np.unique(pz)) == [0, 1]
    o, d = sets["inside"]
    assert len(o) == 27 * 486
    pz, nz = _signs(d)
    assert (pz == 2).sum() == (nz == 2).sum() == 12 * 486
    assert (np.abs(o[:, :2]).max(axis=1) <= 4).all() and (np.abs(o[:, 2]) <= 2).all()
    o, d = sets["threshold"]
    assert len(o) == 2 * 4 * 17
    z = adv.threshold_z()
    assert len(z) == 17 and z[8] == np.float32(2.01) and (np.diff(z.view(np.int32)) == 1).all()


def test_threshold_rays_pass_the_distance_threshold_from_both_sides(built, tmp_path):
    """cpu/hit.c's new_dist > 0.01 on the twins' wall: the floats up to
    2.00999999 miss, those from 2.01000023 upward hit, for both lengths of d;
    and the axis-parallel lattice rays hit and miss, every hit the earlier twin."""
    case = next(c for c in CASES if adv.case_id(c) == "twins_32x18")
    s = _scene(case, tmp_path)
    o, d = adv.threshold_rays()
    obj, P, _ = adv.oracle_collide(s, o, d)
    hit = (obj >= 0).reshape(2, 4, 17)
    assert hit.any() and not hit.all()
    z = adv.threshold_z()
    want = z.astype(np.float64) >= 2.0100002
    assert want.sum() == 8
    assert (hit == want).all(), hit.astype(int)
    assert (obj[obj >= 0] == 0).all()
    o, d = adv.lattice_rays(-0.0)
    k = 8 * 1681  # the unit +z rays: the 33 x 33 lattice points of the wall's square hit it or the cube
    assert (d[k:k + 1681] == np.array([0, 0, 1], np.float32)).all()
    obj, _, _ = adv.oracle_collide(s, o[k:k + 1681], d[k:k + 1681])
    assert (obj >= 0).sum() == 1089 and (obj[obj >= 0] % 2 == 0).all()


def test_sliver_rays(built, tmp_path):
    case = next(c for c in CASES if adv.case_id(c) == "slivers_96x54")
    s = _scene(case, tmp_path)
    o, d = adv.sliver_rays(s, case)
    assert o.shape == d.shape == (4 * 99, 3) and o.dtype == d.dtype == np.float32
    ln = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(ln - 1).max() < 1e-6
    obj, _, _ = adv.oracle_collide(s, o, d)
    assert (obj == 0).any() and (obj != 0).any()  # some land on their sliver, some pass it
