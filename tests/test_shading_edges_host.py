"""The shading fixtures (tests/golden/make_golden_shading.py) and the tables of
tests/shading_edges_util.py without a GPU.

First the oracle is pinned to the reference where no golden had pinned it:
every fixture's frame, rendered by the reference's own cpu/ sources, is what
oracle/rt_oracle.c renders, word for word (a NaN channel NaN in both; sign and
payload are the platform's), with the reference's query counts.  Then the
conditions that keep tests/test_shading_edges.py from passing by exercising
nothing, from the oracle alone: they are conditions on the tables, not
measurements of any kernel."""
import hashlib

import numpy as np
import pytest

import adversarial_util as adv
import shading_edges_util as su

MANIFEST = su.load_manifest()
CASES = MANIFEST["cases"]
F32 = np.float32


def _id(c):
    return f'{c["scene"]}_{c["width"]}x{c["height"]}'


# ---- the oracle against the reference ---------------------------------------------------
def test_manifest_lists_every_scene():
    assert [c["scene"] for c in CASES] == list(su.fixture_scenes())
    assert len(MANIFEST["notes"]) >= 3  # what cpu/parser.c cannot say is written down
    for c in CASES:
        g = su.golden(c)
        assert hashlib.sha256(g.tobytes()).hexdigest() == c["f32_sha256"], _id(c)
        assert (c["width"], c["height"]) == (32, 18)
        assert int(np.isnan(g).sum()) == c["nan_words"]
    assert sum(c["nan_words"] for c in CASES) > 0 and sum(c["words_255"] for c in CASES) > 0


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_committed_scene_is_the_generator_s(case, tmp_path):
    """The committed text is what fixture_scenes() writes today: the tables
    cannot move away from the frames the reference rendered."""
    with open(su.scene_path(case, tmp_path)) as f:
        assert f.read() == su.fixture_scenes()[case["scene"]]


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_oracle_matches_reference(case, built, tmp_path):
    """Word for word, NaN as NaN, and the query counts -- through the oracle's
    restated parser and through the product's loader (the same rt_scene
    layout), which must read nan, inf and denormals as cpu/parser.c's %f does."""
    import oracle as orc
    import rtgpu
    path = su.scene_path(case, tmp_path)
    gold = su.golden(case)
    for what, scene in (("oracle parser", orc.OracleScene(path)), ("product loader", rtgpu.Scene.load_svati(path))):
        img, cnt = orc.render(scene.ptr, case["width"], case["height"], threads=0)
        su.assert_same_words(img, gold, f"{_id(case)} ({what}) against the reference's frame")
        assert (cnt["closest"], cnt["shadow"]) == (case["closest"], case["shadow"]), what
        assert cnt["max_depth"] <= 4


def test_loaders_agree_on_every_material_word(built, tmp_path):
    """The product's float lexer falls back to strtof for what it cannot
    decide: nan, inf, -inf, -0.0 and 1e-45 arrive as the reference's bits."""
    import rtgpu
    for case in CASES:
        s = rtgpu.Scene.load_svati(su.scene_path(case, tmp_path))  # (held: the scene owns what .ptr points to)
        mats = rtgpu.scene_materials(s.ptr)
        want = su.fixture_materials(case["scene"])
        got = np.ascontiguousarray(mats[:len(want), :11], F32)
        su.assert_same_words(got[:, :10], want[:, :10], case["scene"] + " ka kd ks ns")
        su.assert_same_words(mats[:len(want), 11], want[:, 10], case["scene"] + " nr")


# ---- the ray entry point --------------------------------------------------------------------
def test_trace_rays_is_the_frame(built, tmp_path):
    """oracle.trace_rays on a frame's own camera rays, folded, is oracle.render's
    frame with its counts: the new entry point reuses trace() unchanged."""
    import oracle as orc
    import rtgpu
    case = next(c for c in CASES if c["scene"] == "nr")
    s = rtgpu.Scene.load_svati(su.scene_path(case, tmp_path))
    o, d = rtgpu.camera_rays(s.frame(), "pixel")
    rgb, first, cnt = orc.trace_rays(s.ptr, o, d, first=True)
    img, want = orc.render(s.ptr, 32, 18)
    su.assert_same_words(rtgpu.fold_samples(rgb).reshape(img.shape), img, "folded rays against the frame")
    assert cnt == want and cnt["max_depth"] >= 2
    obj, P, N = adv.oracle_collide(s, o[:200], d[:200])
    assert np.array_equal(obj, first["obj"][:200])
    su.assert_same_words(first["P"][:200], P, "first hit P")
    su.assert_same_words(first["N"][:200], N, "first hit N")
    one, _, c1 = orc.trace_rays(s.ptr, o[:333], d[:333], threads=1)
    su.assert_same_words(one, rgb[:333], "one thread against many")
    empty, _, c0 = orc.trace_rays(s.ptr, o[:0], d[:0])
    assert empty.shape == (0, 3) and c0["closest"] == 0


def test_spec_pow_ld(built):
    import oracle as orc
    assert orc.spec_pow_ld(0.0, 0.0) == 1 and orc.spec_pow_ld(-3.0, 2.0) == 0 and abs(orc.spec_pow_ld(2.0, 0.5) ** 2 - 2) < 1e-18
    assert np.isinf(orc.spec_pow_ld(0.0, -1.0)) and np.isnan(orc.spec_pow_ld(0.5, float("nan")))
    assert np.finfo(np.longdouble).nmant >= 63  # more than a double holds


# ---- conditions: the pow sweep -----------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep(built, tmp_path_factory):
    import oracle as orc
    s = su.load_stage(tmp_path_factory.mktemp("sweep"), su.POW_LIGHTS, [su.POW_MATERIAL] * 3)
    o, d = su.pow_rays()
    _, first, cnt = orc.trace_rays(s.ptr, o, d, first=True)
    assert cnt["max_depth"] == 0 and cnt["shadow"] == (first["obj"] >= 0).sum()  # nothing in the light's way
    return s, o, d, first


def test_pow_sweep_spread(sweep):
    """x = dot(R, V) does not depend on Ns, so every Ns sees the same x: at
    least 1,000 distinct bit patterns, an exact 0 (after fmax), an exact 1 or
    above, at least 100 in (0.99, 1).  spec_x restates cpu/light.c:11-19; the
    oracle at Ns = 1, where the channel is x itself, says it restates it right."""
    import oracle as orc
    s, o, d, first = sweep
    hit = first["obj"] >= 0
    assert hit.sum() >= 2000 and (first["obj"] == su.DOME).sum() >= 2000
    x = su.spec_x(first["N"][hit])
    fig = {"rays": len(o), "distinct": len(np.unique(x.view(np.uint32))), "zero": int((np.maximum(x, 0) == 0).sum()),
           "one or above": int((x >= 1).sum()), "in (0.99, 1)": int(((x > 0.99) & (x < 1)).sum())}
    print(fig)
    assert fig["distinct"] >= 1000 and fig["zero"] >= 1 and fig["one or above"] >= 1 and fig["in (0.99, 1)"] >= 100
    ln = np.sqrt((first["N"][hit].astype(np.float64) ** 2).sum(axis=1))
    assert ln.min() < 0.9 and ln.max() == 1.0  # interpolated normals are not unit length
    for k in range(3):
        su.set_material(s, k, su.material(ka=(0, 0, 0), kd=(0, 0, 0), ks=(1, 1, 1), ns=1.0))
    rgb, _, _ = orc.trace_rays(s.ptr, o, d)
    want = np.minimum(np.maximum(x, F32(0)) * F32(255), F32(255))
    assert np.array_equal(rgb[hit, 0], want)


def test_pow_sweep_outcomes(sweep):
    """Across the sweep pow's float results include zero, a denormal, a value
    in (0, 1), exactly 1, a value above 1 and +inf; NaN too (the NaN exponent)."""
    _, _, _, first = sweep
    x = np.maximum(su.spec_x(first["N"][first["obj"] >= 0]), F32(0)).astype(np.float64)
    seen = set()
    tiny = float(np.finfo(F32).tiny)
    for ns in su.NS_VALUES:
        with np.errstate(all="ignore"):
            r = np.power(x, float(F32(ns))).astype(F32)
        seen |= {name for name, m in (("zero", r == 0), ("denormal", (r > 0) & (r < tiny)), ("in (0, 1)", (r >= tiny) & (r < 1)),
                                      ("one", r == 1), ("above one", (r > 1) & np.isfinite(r)), ("inf", np.isposinf(r)),
                                      ("nan", np.isnan(r))) if m.any()}
    assert seen == {"zero", "denormal", "in (0, 1)", "one", "above one", "inf", "nan"}, seen


# ---- conditions: material rows, light rows, the threshold ------------------------------------------
@pytest.fixture(scope="module")
def stage_runs(built, tmp_path_factory):
    """Every case of tests/test_shading_edges.py's material, light and Nr
    tables through the oracle: {name: (rgb, counts)}."""
    tmp = tmp_path_factory.mktemp("stage")
    return {kind: {name: run for name, run in su.oracle_runs(tmp, kind)} for kind in ("materials", "lights", "nr")}


def test_hit_point_is_exact(built, tmp_path):
    import oracle as orc
    s = su.load_stage(tmp_path, su.BASE_LIGHTS)
    o, d = su.stage_rays()
    _, first, _ = orc.trace_rays(s.ptr, o[:su.N_EXACT], d[:su.N_EXACT], first=True)
    assert (first["obj"] == su.FLOOR).all()
    assert np.array_equal(first["P"], np.stack([o[:su.N_EXACT, 0], np.zeros(su.N_EXACT, F32), o[:su.N_EXACT, 2]], 1))
    assert tuple(float(c) for c in first["P"][su.P0_RAY]) == su.P0
    z = d[su.N_EXACT:2 * su.N_EXACT]
    assert np.signbit(z[:, 0]).all() and np.signbit(z[:, 2]).all() and (z[:, [0, 2]] == 0).all()


def test_rows_change_the_output(stage_runs):
    """Every material row differs from the benign material in at least one
    output word, every light row from the base lights under at least one of
    the four materials, or is listed with the reason it cannot."""
    runs = stage_runs["materials"]
    assert list(runs) == ["benign"] + [name for name, _ in su.material_rows()]
    base = runs["benign"][0]
    same = {name for name, (rgb, _) in runs.items() if name != "benign" and not su.words_differ(rgb, base).any()}
    assert same == set(su.UNCHANGING_MATERIALS), sorted(same ^ set(su.UNCHANGING_MATERIALS))
    runs = stage_runs["lights"]
    rows = [name for name, _ in su.light_rows()]
    assert len(runs) == (1 + len(rows)) * len(su.LIGHT_MATERIALS)
    same = {row for row in rows if not any(su.words_differ(runs[f"{row} | {m}"][0], runs[f"base | {m}"][0]).any()
                                           for m, _ in su.LIGHT_MATERIALS)}
    assert same == set(su.SKIPPED_LIGHTS), sorted(same ^ set(su.SKIPPED_LIGHTS))
    # the edge materials matter under the edge lights: Ns = 0 and Ns = -1 differ from benign on every casting row
    for row in rows:
        if row not in su.SKIPPED_LIGHTS:
            assert su.words_differ(runs[f"{row} | Ns=0"][0], runs[f"{row} | benign"][0]).any(), row
            assert su.words_differ(runs[f"{row} | Ns=-1"][0], runs[f"{row} | benign"][0]).any(), row


def test_threshold_rows_differ_by_the_rays_that_hit(stage_runs):
    """(float)0.01 is below the double 0.01: the path ends.  One float above:
    every ray that hit the floor asks once more."""
    runs = stage_runs["nr"]
    nrays = len(su.bounce_rays()[0])
    at, up, down = (runs[f"Nr={t}"][1] for t in ("f0.01", "f0.01+", "f0.01-"))
    assert at["closest"] == down["closest"] == nrays and at["max_depth"] == 0
    assert up["closest"] - at["closest"] == nrays and up["max_depth"] == 1
    # the pairs: the product floor * panel decides the third query
    for (a, b) in su.NR_PAIRS:
        c = runs[f"Nr pair {su.tag(a)} x {su.tag(b)}"][1]
        with np.errstate(invalid="ignore"):  # inf * 0
            coef1 = F32(a) * F32(1)
            coef2 = F32(b) * coef1
        want = nrays * (1 + (not float(coef1) < 0.01) + (not float(coef1) < 0.01 and not float(coef2) < 0.01))
        assert c["closest"] == want, (a, b, c)
    depths = {runs[f"Nr pair {su.tag(a)} x {su.tag(b)}"][1]["max_depth"] for a, b in su.NR_PAIRS}
    assert depths == {0, 1, 2}


def test_no_path_is_deeper_than_four(stage_runs):
    for runs in stage_runs.values():
        for name, (_, cnt) in runs.items():
            assert cnt["max_depth"] <= 4, (name, cnt)
    assert max(c["max_depth"] for _, c in stage_runs["nr"].values()) >= 2


def test_nan_and_inf_coverage(stage_runs):
    """Per kind of row, one yields a NaN channel; one yields a channel that an
    infinity (not a large finite value) clamps to 255."""
    mats, lights, nr = stage_runs["materials"], stage_runs["lights"], stage_runs["nr"]

    def nan(runs, prefix):
        return any(np.isnan(rgb).any() for name, (rgb, _) in runs.items() if name.startswith(prefix))

    assert nan(mats, "Ns=") and nan(mats, "Ks[") and nan(mats, "Kd[") and nan(mats, "Ka[") and nan(nr, "Nr=")
    assert nan(lights, "directional colour") and nan(lights, "ambient colour") and nan(lights, "point colour")
    assert nan(lights, su.ON_HIT)  # normalize((0, 0, 0)) reaches the colour
    base = mats["benign"][0]
    assert not np.isnan(base).any()
    for runs, name, ref in ((mats, "Ns=-1.0", base),  # pow(0, -1) = inf, times Ks
                            (lights, "directional colour[1]=inf | benign", lights["base | benign"][0]),
                            (nr, "Nr=inf", nr["Nr=0.0"][0])):
        rgb = runs[name][0]
        assert ((rgb == 255) & (ref != 255)).any(), name
    # an infinite Ka / Kd / Ks channel is clamped where the colour is made (init_color): the frame of 1e30's
    for word in ("Ks", "Kd", "Ka"):
        assert not su.words_differ(mats[f"{word}[1]=inf"][0], mats[f"{word}[1]={su.tag(1e30)}"][0]).any(), word
        assert su.words_differ(mats[f"{word}[1]=inf"][0], mats[f"{word}[2]=-inf"][0]).any(), word
