"""The light-placement fixtures (tests/golden/make_golden_lights.py) and the
table of tests/light_edges_util.py without a GPU.

First the oracle is pinned to the reference under every row: the frame the
reference's own cpu/ sources rendered is what oracle/rt_oracle.c renders, word
for word (a NaN as any NaN), with the reference's query counts -- whatever the
reference writes under a light of length 0, 1e-20 or 3e-39 is the expected
value.  Then the conditions that keep tests/test_light_edges.py from passing by
exercising nothing, from the oracle's collide_dist and the restated cell
arithmetic alone: they are conditions on the inputs, not measurements of any
kernel, and they equal what the manifest recorded when the fixtures were made."""
import hashlib

import numpy as np
import pytest

import light_edges_util as lu

MANIFEST = lu.load_manifest()
CASES = MANIFEST["cases"]
IDS = [lu.row_slug(c["row"]) for c in CASES]


def test_manifest_lists_every_row():
    assert [c["row"] for c in CASES] == lu.ROW_NAMES
    assert len(MANIFEST["notes"]) >= 2
    for c in CASES:
        g = lu.golden(c)
        assert hashlib.sha256(g.tobytes()).hexdigest() == c["f32_sha256"], c["row"]
        assert (c["width"], c["height"]) == (lu.W, lu.H)
        assert int(np.isnan(g).sum()) == c["nan_words"]
        assert (g != 0).any(), c["row"]  # the ambient light: no frame is black
        assert c["closest"] > 0 and c["shadow"] > 0


def test_table_is_what_the_issue_lists():
    """Every row is finite (so it is .svati text), named once, with the line
    that says which code it aims at."""
    assert len(set(lu.ROW_NAMES)) == len(lu.ROWS) == 22
    for name, t, v, on_lattice, gives, aims in lu.ROWS:
        assert t in (lu.DIRECTIONAL, lu.POINT) and len(v) == 3 and aims
        assert np.isfinite(np.asarray(v, np.float32)).all(), name
        assert gives in (lu.SHADOWS, lu.NOTHING, lu.ENCLOSED)
    dirs = [r[2] for r in lu.ROWS if r[1] == lu.DIRECTIONAL]
    assert (0.0, 0.0, 0.0) in dirs and any(np.signbit(v[0]) and v[0] == 0 for v in dirs)
    assert float(np.float32(3e-39)) != 0 and float(np.float32(3e-39)) < float(np.finfo(np.float32).tiny)
    step = np.nextafter(np.float32(12), np.float32(13))
    assert np.float32(lu.row("point off the lattice")[2][2]) == step  # the control: one float step off


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_committed_scene_is_the_generator_s(case, tmp_path):
    with open(lu.scene_path(case, tmp_path)) as f:
        assert f.read() == lu.scene_text(lu.row_lights(lu.row(case["row"])))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_matches_reference(case, built, tmp_path):
    """Word for word, NaN as NaN, and the query counts -- through the oracle's
    restated parser and through the product's loader, which must read -0.0,
    1e-20 and denormals as cpu/parser.c's %f does."""
    import oracle as orc
    import rtgpu
    path = lu.scene_path(case, tmp_path)
    gold = lu.golden(case)
    r = lu.row(case["row"])
    for what, scene in (("oracle parser", orc.OracleScene(path)), ("product loader", rtgpu.Scene.load_svati(path))):
        img, cnt = orc.render(scene.ptr, case["width"], case["height"], threads=0)
        lu.assert_same_words(img, gold, f'{case["row"]} ({what}) against the reference\'s frame')
        assert (cnt["closest"], cnt["shadow"]) == (case["closest"], case["shadow"]), what
    s = rtgpu.Scene.load_svati(path)
    assert s.triangle_count == case["triangles"] and int(s.s.light_count) == 2
    L = s.s.lights[1]
    got = np.array([L.v.x, L.v.y, L.v.z], np.float32)
    assert int(L.type) == r[1] and got.tobytes() == np.asarray(r[2], np.float32).tobytes(), (case["row"], got)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_row_conditions(case, built, tmp_path):
    """Shares strictly between 1 % and 99 % for the rows meant to shadow,
    exactly 0 where the reference accepts nothing, exactly 1 around the
    enclosed light (from the box's own faces too); at least 64 exact face
    ties, sc or tc of +-1 and whole cell coordinates for every point light on
    the lattice -- and all of it as the manifest recorded it."""
    import rtgpu
    s = rtgpu.Scene.load_svati(lu.scene_path(case, tmp_path))
    fig = lu.check_conditions(lu.row(case["row"]), s)
    print(case["row"], fig)
    assert fig == case["observed"], (fig, case["observed"])


def test_origins_are_what_the_tests_say():
    o = lu.origins()
    n = lu.N_LATTICE + lu.N_FACE
    assert o.dtype == np.float32 and len(o) == 7 * n and lu.N_LATTICE >= 500 and lu.N_FACE == 6 * 49
    base = o[:n]
    assert (base[:lu.N_LATTICE] == np.round(base[:lu.N_LATTICE])).all()  # exact integers
    assert (base * 4 == np.round(base * 4)).all()
    moved = o[n:].reshape(6, n, 3)
    for k in range(6):
        diff = moved[k] != base
        assert (diff.sum(axis=1) == 1).all() and diff[:, k // 2].all()
        to = np.float32(-np.inf if k % 2 == 0 else np.inf)
        assert np.array_equal(moved[k][:, k // 2], np.nextafter(base[:, k // 2], to))  # (from 0: a denormal)
    assert len(np.unique(o, axis=0)) == len(o)


def test_control_has_fewer_ties_than_its_lattice_point():
    """The restated cell arithmetic tells the lattice from one float step off it."""
    o = lu.origins()
    on = lu.tie_counts((4.0, 8.0, 12.0), o, 438)
    off = lu.tie_counts(lu.row("point off the lattice")[2], o, 438)
    assert on["face_ties"] >= lu.MIN_TIES > off["face_ties"], (on, off)
