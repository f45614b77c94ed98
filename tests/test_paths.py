"""A ray batch's paths written out on the GPU (include/rt_hip.h
rt_hip_path_records, rt_hip_path_records_host; kernels csrc/rt_paths.hip): a
CSR offset per ray and, per path vertex, an rt_gsample, its coef and its
shaded term.  The contract is a composition of things that exist: the terms
fold to the batch's own colours, vertex 0 is the batch's own sample record,
the records chain hop by hop through the first-hit query (on the same context,
and against the oracle on the proven configurations), the terms are the direct
light of the records times coef, and the consumers of records take the
exported buffer as it is.  All comparisons are 32-bit words, a NaN matching any
NaN, no tolerance.  The rays are the 32 x 18 camera rays of test_ao.py's
scenes and of mirrors_32x18 (paths 44 deep)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_own_manifest, own_scene_path
from test_ao import FILL, SCENES, SEED, gpu, shared  # noqa: F401  (fixtures)
from test_ao_host import same_words
from test_rays import PROVEN, Dev, _ctx

pytestmark = pytest.mark.gpu

RT_EINVAL, RT_EHITBUF = -1, -10
OWN = {f'{c["scene"]}_{c["width"]}x{c["height"]}': c for c in load_own_manifest()}
GUARD = 64  # words past an output that must keep their fill
FILLW = np.frombuffer(bytes([FILL] * 4), np.uint32)[0]
REFLECTIVE = ["spheres", "island_smooth", "car-on-road"]
ALL = SCENES + ["mirrors"]
F = np.float32


@pytest.fixture(scope="module")
def scenes(gpu, shared, tmp_path_factory):
    """name -> (scene at 32x18, (origins, dirs) of its 2,304 camera rays)."""
    cache = {}

    def get(name):
        if name not in cache:
            if name == "mirrors":
                s = gpu.Scene.load_svati(own_scene_path(OWN["mirrors_32x18"], tmp_path_factory.mktemp("mirrors")))
                s.set_size(32, 18)
                cache[name] = (s, gpu.camera_rays(s.frame(), "pixel"))
            else:
                cache[name] = (shared(name)["scene"], shared(name)["cam"])
        return cache[name]
    return get


def _nr(s):
    return s.materials_array()[:, 11]


def _words(a):
    """The 32-bit words of an array, a row per element (an empty array: no row)."""
    w = np.ascontiguousarray(a).view(np.uint32)
    return w.reshape(len(a), w.size // len(a)) if len(a) else w.reshape(0, 0)


def _same_records(a, b):
    """P, N and obj of two GSAMPLE arrays, word for word (a NaN matching a NaN)."""
    return (len(a) == len(b) and same_words(a["P"], b["P"]) and same_words(a["N"], b["N"])
            and np.array_equal(a["obj"], b["obj"]))


def _trace(ctx, o, d, **kw):
    """trace_rays + path_records -> dict(rgb, smp, st, off, rec, coef, terms, len)."""
    rgb, smp, st = ctx.trace_rays(o, d, **kw)
    off, rec, coef, terms = ctx.path_records()
    return dict(rgb=rgb, smp=smp, st=st, off=off, rec=rec, coef=coef, terms=terms,
                len=np.diff(off.astype(np.int64)))


def _check_csr(p, n):
    off = p["off"]
    assert off.dtype == np.uint32 and len(off) == n + 1 and off[0] == 0
    assert (p["len"] >= 0).all(), "offsets are monotone"
    assert int(off[n]) == p["st"]["hit_records"] == len(p["rec"]) == len(p["coef"]) == len(p["terms"])


_REF = {}


def _reference(gpu, scenes, name):
    """The paths of `name`'s camera rays on a FLAT context, computed once."""
    if name not in _REF:
        s, (o, d) = scenes(name)
        ctx = _ctx(gpu, s, "flat")
        _REF[name] = _trace(ctx, o, d, samples=True)
        ctx.close()
    return _REF[name]


# ---- 1: the fold ------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["flat", "octree_gpu", "octree"])
def test_terms_fold_to_the_batch_s_colours(gpu, scenes, accel):
    """path_fold(offsets, terms) == the d_rgb of the same batch, with and
    without the packet flag and d_samples, on every scene; offsets[0] == 0,
    monotone, offsets[n] == hit_records; misses, NaN rays and zero directions
    have no vertex."""
    deep = 0
    for name in ALL:
        s, (o, d) = scenes(name)
        o, d = o.copy(), d.copy()
        bad = np.array([0, 5, 63, 64, 65, 127, 500, 2302, 2303])
        o[bad[0::3], 1] = np.nan
        d[bad[1::3], 2] = np.inf
        d[bad[2::3]] = 0.0
        d[bad[2], 0] = -0.0
        n = len(o)
        ctx = _ctx(gpu, s, accel)
        for packet in (False, True):
            for samples in (False, True):
                p = _trace(ctx, o, d, packet=packet, samples=samples)
                _check_csr(p, n)
                got = gpu.path_fold(p["off"], p["terms"])
                assert same_words(got, p["rgb"]), (name, accel, packet, samples)
                assert (p["len"][bad] == 0).all(), "an untraced ray has no vertex"
                if samples:
                    assert p["st"]["zero_normal"] == 0
                    assert np.array_equal(p["len"] == 0, p["smp"]["prim"] < 0), "a miss, and only a miss, has no vertex"
        if name == "spheres":
            assert (p["len"] >= 2).sum() > 50, "spheres: rays with at least two vertices"
        if name == "point-light":
            assert p["len"].max() == 1, "point-light: nothing reflects"
        if name == "mirrors":
            assert p["len"].max() >= 40, "mirrors: a deep path"
        deep += int((p["len"] >= 2).sum())
        ctx.close()
    assert deep > 2000


# ---- 2: vertex 0 and the coefficients ---------------------------------------------------------
@pytest.mark.parametrize("accel", ["flat", "octree_gpu", "octree"])
def test_vertex_0_and_coefficients(gpu, scenes, accel):
    """P, N and obj of vertex 0 are the batch's own d_samples record; queries
    == v, prim == RT_PATH_PRIM, dist is +0; coef == path_coefs(offsets, records,
    nr)."""
    for name in ALL:
        s, (o, d) = scenes(name)
        ctx = _ctx(gpu, s, accel)
        p = _trace(ctx, o, d, samples=True)
        ctx.close()
        _check_csr(p, len(o))
        assert p["st"]["zero_normal"] == 0
        off, rec, ln = p["off"].astype(np.int64), p["rec"], p["len"]
        hit = ln > 0
        assert hit.sum() > 300, name
        assert _same_records(rec[off[:-1][hit]], p["smp"][hit]), (name, accel)
        v = np.arange(len(rec)) - np.repeat(off[:-1], ln)
        assert np.array_equal(rec["queries"], v), "queries == v"
        assert (rec["prim"] == gpu.RT_PATH_PRIM).all() and (rec["dist"].view(np.uint32) == 0).all()
        assert same_words(p["coef"], gpu.path_coefs(off, rec, _nr(s))), (name, accel)
        assert (p["coef"][off[:-1][hit]] == 1).all()
        if name in REFLECTIVE + ["mirrors"]:
            assert (p["coef"] < 1).any(), name


# ---- 3: hop by hop ----------------------------------------------------------------------------
def _hops(gpu, p, dirs):
    """The ray that leaves every vertex: (P_v, d_{v+1}), d_0 = the batch's
    direction, d_{v+1} = bounce_dir(d_v, N_v) -> (origins, dirs, has a successor)."""
    off, rec, ln = p["off"].astype(np.int64), p["rec"], p["len"]
    total = len(rec)
    out = np.zeros((total, 3), F)
    d_in = np.zeros((total, 3), F)
    d_in[off[:-1][ln > 0]] = dirs[ln > 0]
    for v in range(int(ln.max())):
        j = off[:-1][ln > v] + v
        out[j] = gpu.bounce_dir(d_in[j], rec["N"][j])
        nxt = off[:-1][ln > v + 1] + v + 1
        d_in[nxt] = out[nxt - 1]
    succ = np.ones(total, bool)
    succ[off[1:][ln > 0] - 1] = False
    return np.ascontiguousarray(rec["P"]), out, succ


def _check_chain(p, nr, first, succ, what):
    """first: P, N, obj of the first hit of every vertex's outgoing ray (obj <
    0: none).  With a successor it is the successor; without one the cast
    missed, or the next coefficient is below 0.01 as a double, or the winner's
    normal was zero: no vertex is missing, none is extra."""
    rec, coef = p["rec"], p["coef"]
    j = np.flatnonzero(succ)
    assert (first["obj"][j] >= 0).all(), (what, "a successor the cast does not find")
    assert _same_records(first[j], rec[j + 1]), (what, "the cast's hit is the next vertex")
    e = np.flatnonzero(~succ)
    nxt = (nr[rec["obj"][e]] * coef[e]).astype(F)
    missed = first["obj"][e] < 0
    cut = nxt.astype(np.float64) < 0.01
    zero = ~missed & ((first["N"][e].view(np.uint32) & 0x7fffffff) == 0).all(axis=1)
    assert (missed | cut | zero).all(), (what, "a path ends where the reference goes on", e[~(missed | cut | zero)][:5])
    return int(missed.sum()), int(cut.sum())


_ORACLE = {}


@pytest.mark.parametrize("accel,exact", PROVEN + [("octree_gpu", False)],
                         ids=[a for a, _ in PROVEN] + ["octree_gpu_default"])
def test_hop_by_hop(gpu, scenes, accel, exact):
    """A ray cast of all (P_v, d_{v+1}) on the same context gives vertex v + 1
    or a reason why there is none; on brute force and the two proven walks the
    oracle's first hits say the same at 0 ULP."""
    import oracle as orc
    missed = cut = 0
    for name in REFLECTIVE + ["mirrors"]:
        s, (o, d) = scenes(name)
        ctx = _ctx(gpu, s, accel, exact)
        p = _trace(ctx, o, d)
        assert p["st"]["zero_normal"] == 0
        po, pd, succ = _hops(gpu, p, d)
        assert succ.sum() > 50, name
        _, cast, _ = ctx.trace_rays(po, pd, shade=False)
        ctx.close()
        first = np.zeros(len(cast), orc.FIRST_HIT)
        first["obj"], first["P"], first["N"] = np.where(cast["prim"] >= 0, cast["obj"], -1), cast["P"], cast["N"]
        a, b = _check_chain(p, _nr(s), first, succ, (name, accel, "cast"))
        missed, cut = missed + a, cut + b
        if (accel, exact) in PROVEN:
            key = (name, po.tobytes(), pd.tobytes())
            if key not in _ORACLE:
                _ORACLE[key] = orc.trace_rays(s.ptr, po, pd, first=True)[1]
            _check_chain(p, _nr(s), _ORACLE[key], succ, (name, accel, "oracle"))
    assert missed > 100 and cut > 100, "paths end both ways"


# ---- 4: the terms ------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ["flat", "octree_gpu"])
def test_terms_are_direct_light_times_coef(gpu, scenes, accel):
    """terms == color_mul(direct_light(records), coef), every vertex of every
    scene."""
    lit = 0
    for name in ALL:
        s, (o, d) = scenes(name)
        ctx = _ctx(gpu, s, accel)
        p = _trace(ctx, o, d)
        assert p["st"]["zero_normal"] == 0
        direct, _, _ = ctx.direct_light(p["rec"])
        ctx.close()
        want = gpu.color_mul(direct, p["coef"])
        bad = np.flatnonzero((~((_words(want) == _words(p["terms"])) | (np.isnan(want) & np.isnan(p["terms"])))).any(axis=1))
        assert len(bad) == 0, (name, accel, len(bad), bad[:5], p["terms"][bad[:3]], want[bad[:3]])
        lit += int((want != 0).any(axis=1).sum())
    assert lit > 5000


# ---- 5: feeding the consumers ------------------------------------------------------------------
def test_consumers_take_the_exported_buffer(gpu, scenes):
    """ambient_occlusion and gather on the exported device buffer equal their
    host-path results on the downloaded records."""
    s, (o, d) = scenes("spheres")
    table = gpu.ao_table(37, SEED)
    ctx = _ctx(gpu, s, "octree_gpu")
    p = _trace(ctx, o, d)
    total, n = len(p["rec"]), len(o)
    dev = Dev(gpu)
    d_off, d_rec, d_t = dev.malloc(4 * (n + 1)), dev.malloc(40 * total), dev.upload(table)
    ctx.path_records_device(n, d_off, total, d_rec)
    d_cnt = dev.upload(np.full(total + GUARD, FILLW, np.uint32))
    ctx.ambient_occlusion_device(d_rec, total, 4, d_t, len(table), SEED, d_cnt)
    ctx.stats()
    assert _words(dev.host(d_rec, total, gpu.GSAMPLE)).tobytes() == _words(p["rec"]).tobytes()
    cnt = dev.host(d_cnt, total + GUARD, np.uint32)
    want, _ = ctx.ambient_occlusion(p["rec"], 4, table, SEED)
    assert np.array_equal(cnt[:total], want) and (cnt[total:] == FILLW).all() and want.any()
    deeper = p["rec"]["queries"] > 0
    assert deeper.sum() > 50 and want[deeper].any(), "what a mirror shows gets ambient occlusion"
    # the paths survived both occlusion batches; the gather takes them
    again = ctx.path_records()
    assert _words(again[1]).tobytes() == _words(p["rec"]).tobytes()
    d_sum = dev.upload(np.full(3 * total + GUARD, FILLW, np.uint32))
    ctx.gather_device(d_rec, total, 4, d_t, len(table), SEED, d_sum)
    ctx.stats()
    got = dev.host(d_sum, 3 * total + GUARD, np.uint32)
    wsum, _ = ctx.gather(p["rec"], 4, table, SEED)
    assert (got[3 * total:] == FILLW).all() and same_words(got[:3 * total].view(F).reshape(-1, 3), wsum)
    assert (wsum[deeper] != 0).any()
    dev.close()
    ctx.close()


# ---- 6: shapes ---------------------------------------------------------------------------------
def _slice_equal(p, ref, a, n):
    """The paths of rays [a, a + n) of `ref`."""
    lo, hi = int(ref["off"][a]), int(ref["off"][a + n])
    return (np.array_equal(p["off"], ref["off"][a:a + n + 1] - ref["off"][a])
            and _words(p["rec"]).tobytes() == _words(ref["rec"][lo:hi]).tobytes()
            and same_words(p["coef"], ref["coef"][lo:hi]) and same_words(p["terms"], ref["terms"][lo:hi]))


def test_batch_sizes_at_block_edges(gpu, scenes):
    """n in {1, 63, 64, 65, 255, 256, 257, 2304}: the paths of a batch of n of
    the fixture's rays are those rays' paths in the whole batch.  The small
    batches start at the first ray that bounces (the frame's first rows see
    the sky), so they hold paths of 0, 1 and more vertices."""
    ref = _reference(gpu, scenes, "spheres")
    s, (o, d) = scenes("spheres")
    a = min(int(np.flatnonzero(ref["len"] >= 2)[0]), len(o) - 257)
    assert ref["len"][a:a + 257].max() >= 2 and ref["len"][a:a + 257].sum() > 0
    ctx = _ctx(gpu, s, "flat")
    for n in (1, 63, 64, 65, 255, 256, 257, 2304):
        a_n = a if n < len(o) else 0
        p = _trace(ctx, o[a_n:a_n + n], d[a_n:a_n + n])
        _check_csr(p, n)
        assert _slice_equal(p, ref, a_n, n), n
    ctx.close()


def test_one_batch_past_a_chunk_of_block_totals(gpu, scenes):
    """262,145 rays -- one more than one step of the block-total scan covers
    (1,024 blocks of 256) -- made by repeating the fixture's: the repeated
    small result."""
    ref = _reference(gpu, scenes, "spheres")
    s, (o, d) = scenes("spheres")
    n = 1024 * 256 + 1
    reps = -(-n // len(o))
    ctx = _ctx(gpu, s, "flat")
    p = _trace(ctx, np.tile(o, (reps, 1))[:n], np.tile(d, (reps, 1))[:n])
    ctx.close()
    _check_csr(p, n)
    assert same_words(p["rgb"], np.tile(ref["rgb"], (reps, 1))[:n])
    ln = np.tile(ref["len"], reps)[:n]
    assert np.array_equal(p["len"], ln)
    whole, rest = divmod(n, len(o))
    k = int(ref["off"][rest])
    for key in ("rec", "coef", "terms"):
        small = ref[key]
        want = np.concatenate([small] * whole + [small[:k]])
        assert _words(p[key]).tobytes() == _words(want).tobytes(), key


def test_cap_and_count_only(gpu, scenes):
    """cap in {0, 1, total - 1, total} into buffers pre-filled with 0xAB and 64
    words of guard: below cap the whole export's words, nothing at or past cap
    changes, the offsets are complete every time; a count-only call."""
    ref = _reference(gpu, scenes, "spheres")
    s, (o, d) = scenes("spheres")
    n, total = len(o), len(ref["rec"])
    ctx = _ctx(gpu, s, "flat")
    ctx.trace_rays(o, d)
    dev = Dev(gpu)
    full = {"rec": _words(ref["rec"]).reshape(-1), "coef": _words(ref["coef"]).reshape(-1),
            "terms": _words(ref["terms"]).reshape(-1)}
    per = {"rec": 10, "coef": 1, "terms": 3}
    for cap in (0, 1, total - 1, total):
        d_off = dev.upload(np.full(n + 1 + GUARD, FILLW, np.uint32))
        bufs = {k: dev.upload(np.full(per[k] * total + GUARD, FILLW, np.uint32)) for k in per}
        ctx.path_records_device(n, d_off, cap, bufs["rec"], bufs["coef"], bufs["terms"])
        ctx.stats()
        off = dev.host(d_off, n + 1 + GUARD, np.uint32)
        assert np.array_equal(off[:n + 1], ref["off"]) and (off[n + 1:] == FILLW).all(), cap
        for k in per:
            got = dev.host(bufs[k], per[k] * total + GUARD, np.uint32)
            assert np.array_equal(got[:per[k] * cap], full[k][:per[k] * cap]), (cap, k)
            assert (got[per[k] * cap:] == FILLW).all(), (cap, k, "written at or past cap")
    # a count: no array, cap ignored; one array alone
    d_off = dev.upload(np.full(n + 1 + GUARD, FILLW, np.uint32))
    ctx.path_records_device(n, d_off, 12345)
    d_cf = dev.upload(np.full(total + GUARD, FILLW, np.uint32))
    ctx.path_records_device(n, d_off, total, 0, d_cf, 0)
    ctx.stats()
    off = dev.host(d_off, n + 1 + GUARD, np.uint32)
    assert np.array_equal(off[:n + 1], ref["off"]) and (off[n + 1:] == FILLW).all()
    cf = dev.host(d_cf, total + GUARD, np.uint32)
    assert np.array_equal(cf[:total], full["coef"]) and (cf[total:] == FILLW).all()
    only = ctx.path_records(records=False, coef=False, terms=False)
    assert np.array_equal(only[0], ref["off"]) and only[1:] == (None, None, None)
    dev.close()
    ctx.close()


# ---- 7: deep paths -----------------------------------------------------------------------------
def test_deep_paths_and_the_overflowing_batch(gpu, scenes):
    """mirrors: the first batch of a fresh context overflows the first sizing
    (RT_EHITBUF through rt_hip_stats); the export still folds to what that batch
    wrote to d_rgb.  After the retry the fold holds again, every path has its
    queries' vertices, and the longest is the oracle's max_depth + 1 (depth
    counts from 0, and the deepest call hit)."""
    import oracle as orc
    s, (o, d) = scenes("mirrors")
    n = len(o)
    ctx = _ctx(gpu, s, "octree_gpu", True)  # (the proven walk: the oracle's queries, by proof)
    dev = Dev(gpu)
    d_o, d_d, d_rgb, d_smp = dev.upload(o), dev.upload(d), dev.malloc(12 * n), dev.malloc(40 * n)
    ctx.trace_rays_device(d_o, d_d, n, d_rgb, d_smp)
    with pytest.raises(gpu.RtError) as e:
        ctx.stats()
    assert e.value.code == RT_EHITBUF
    rgb1 = dev.host(d_rgb, (n, 3), F)
    off, rec, coef, terms = ctx.path_records(n=n, cap=0, records=False, coef=False, terms=False)
    total1 = int(off[n])
    off1, rec1, coef1, terms1 = ctx.path_records(n=n, cap=total1)
    # (a path whose deepest record fell past the buffers is empty to the fold, and so to the export:
    # here that is nearly every path, 44 records deep against 2 a ray held)
    assert np.array_equal(off1, off) and len(terms1) == total1 < 2 * n
    assert same_words(gpu.path_fold(off1, terms1), rgb1), "the export is what the fold saw"
    ctx.trace_rays_device(d_o, d_d, n, d_rgb, d_smp)
    st = ctx.stats()
    rgb2, smp = dev.host(d_rgb, (n, 3), F), dev.host(d_smp, n, gpu.GSAMPLE)
    off2, rec2, coef2, terms2 = ctx.path_records(n=n, cap=st["hit_records"])
    dev.close()
    ctx.close()
    assert int(off2[n]) == st["hit_records"] == len(rec2) > total1
    assert same_words(gpu.path_fold(off2, terms2), rgb2)
    ln = np.diff(off2.astype(np.int64))
    # a path of q queries has q vertices (ended by the coefficient) or q - 1 (its last query missed)
    assert ((ln == smp["queries"]) | (ln == smp["queries"] - 1)).all()
    _, _, cnt = orc.trace_rays(s.ptr, o, d)
    assert int(smp["queries"].max()) == cnt["max_depth"] + 1
    longest = int(np.argmax(ln))
    last = int(off2[longest + 1]) - 1
    nxt = F(_nr(s)[rec2["obj"][last]] * coef2[last])
    assert float(nxt) < 0.01, "the longest path ends by its coefficient: its deepest query hit"
    assert ln.max() == cnt["max_depth"] + 1 >= 40


# ---- 8: survival and loss ----------------------------------------------------------------------
def _export_bytes(ctx):
    off, rec, coef, terms = ctx.path_records()
    return off.tobytes() + rec.tobytes() + coef.tobytes() + terms.tobytes()


def test_paths_survive_what_the_kept_frame_survives(gpu, scenes):
    """The export gives the same words after occluded, ambient_occlusion,
    ao_rays, direct_light, frame_rays, set_lights, set_materials and a second
    export."""
    s, (o, d) = scenes("spheres")
    table = gpu.ao_table(37, SEED)
    ctx = _ctx(gpu, s, "octree_gpu")
    p = _trace(ctx, o, d)
    want = _export_bytes(ctx)
    assert want == p["off"].tobytes() + p["rec"].tobytes() + p["coef"].tobytes() + p["terms"].tobytes()
    lights = s.lights()
    keep = [(l.r, l.g, l.b) for l in lights]
    steps = {
        "occluded": lambda: ctx.occluded(o, d),
        "ambient_occlusion": lambda: ctx.ambient_occlusion(p["rec"], 4, table, SEED),
        "ao_rays": lambda: ctx.ao_rays(p["rec"][:100], 4, table, SEED),
        "direct_light": lambda: ctx.direct_light(p["rec"]),
        "frame_rays": lambda: ctx.frame_rays(s.frame()),
        "stats": lambda: ctx.stats(),
        "second export": lambda: ctx.path_records(),
    }
    for what, step in steps.items():
        step()
        assert _export_bytes(ctx) == want, what
    try:
        for l in lights:
            l.r, l.g, l.b = 0.5 * l.r, 0.25 * l.g, 0.75 * l.b
        ctx.set_lights(lights)
        assert _export_bytes(ctx) == want, "set_lights: the terms stay the batch's own"
        ctx.set_materials(s)
        assert _export_bytes(ctx) == want, "set_materials"
        # and the edited lights do count for the next batch
        q = _trace(ctx, o, d)
        assert q["rec"].tobytes() == p["rec"].tobytes() and q["coef"].tobytes() == p["coef"].tobytes()
        assert q["terms"].tobytes() != p["terms"].tobytes()
    finally:
        for l, (r, g, b) in zip(lights, keep):
            l.r, l.g, l.b = r, g, b
    ctx.close()


def test_paths_are_gone_after_what_writes_hit_records(gpu, scene_dir, scenes):
    """RT_EINVAL before any batch and after a render, a ray cast, a gather and
    set_triangles, each naming the call; after the refusal the kept frame, where
    there is one, still relights.  After set_triangles plus a new batch the
    export equals a fresh context's."""
    _, (o, d) = scenes("spheres")
    s = gpu.Scene.load_svati(os.path.join(scene_dir, "spheres.svati"))
    s.set_size(32, 18)
    f = s.frame()
    table = gpu.ao_table(37, SEED)
    ctx = _ctx(gpu, s, "octree_gpu")
    ctx.set_keep_visibility(True)
    n = len(o)

    def refused(word):
        with pytest.raises(gpu.RtError) as e:
            ctx.path_records(n=n, cap=0)
        assert e.value.code == RT_EINVAL and word in str(e.value), e.value

    refused("no ray batch")
    p = _trace(ctx, o, d)
    ctx.render_image(f)
    rel, _ = ctx.relight_image(f)
    refused("rt_hip_render")
    assert ctx.relight_image(f)[0].tobytes() == rel.tobytes()
    ctx.trace_rays(o, d)
    ctx.trace_rays(o, d, shade=False)
    refused("ray cast")
    ctx.trace_rays(o, d)
    ctx.gather(p["rec"][:64], 4, table, SEED)
    refused("rt_hip_gather")
    ctx.trace_rays(o, d)
    ctx.render_compat(s.camera)
    refused("rt_hip_render_compat")
    ctx.trace_rays(o, d)
    first, count = gpu.object_range(s, 0)
    tris = s.triangles_array()
    moved = gpu.shift_triangles(tris[first:first + count], (0.0, 0.5 * float(gpu.vertex_extent(tris[first:first + count])), 0.0))
    ctx.set_triangles(moved, first)
    refused("rt_hip_set_triangles")
    s.set_triangles_array(moved, first)
    q = _trace(ctx, o, d)
    fresh = _ctx(gpu, s, "octree_gpu")
    w = _trace(fresh, o, d)
    fresh.close()
    for key in ("off", "rec", "coef", "terms", "rgb"):
        assert q[key].tobytes() == w[key].tobytes(), key
    assert q["rec"].tobytes() != p["rec"].tobytes()
    ctx.close()


def test_refusals_write_nothing(gpu, scenes):
    """RT_EINVAL for a wrong n, another stream, a misaligned record pointer,
    NULL offsets and a NULL context; no word is written, and the paths are
    still there."""
    s, (o, d) = scenes("spheres")
    ctx = _ctx(gpu, s, "octree_gpu")
    p = _trace(ctx, o, d)
    n, total = len(o), len(p["rec"])
    dev = Dev(gpu)
    d_off = dev.upload(np.full(n + 2, FILLW, np.uint32))
    d_rec = dev.upload(np.full(10 * total + 2, FILLW, np.uint32))
    d_cf = dev.upload(np.full(total, FILLW, np.uint32))
    d_tm = dev.upload(np.full(3 * total, FILLW, np.uint32))
    L = gpu.lib()

    def refused(call):
        with pytest.raises(gpu.RtError) as e:
            call()
        assert e.value.code == RT_EINVAL, e.value

    g = ctx.path_records_device
    refused(lambda: g(n - 1, d_off, total, d_rec, d_cf, d_tm))
    refused(lambda: g(n + 1, d_off, total, d_rec, d_cf, d_tm))
    refused(lambda: g(0, d_off, total, d_rec, d_cf, d_tm))
    refused(lambda: g(n, 0, total, d_rec, d_cf, d_tm))
    refused(lambda: g(n, d_off, total, d_rec + 4, d_cf, d_tm))  # not 8-byte aligned
    # (a stream handle that is not the batch's: the refusal compares it and never follows it)
    refused(lambda: g(n, d_off, total, d_rec, d_cf, d_tm, stream=d_off))
    refused(lambda: gpu._check(L.rt_hip_path_records(None, n, C.c_void_p(d_off), total, C.c_void_p(d_rec), None, None,
                                                     None), "null context"))
    host_off = np.full(n + 1, FILLW, np.uint32)
    refused(lambda: gpu._check(L.rt_hip_path_records_host(ctx.h, n - 1, host_off.ctypes.data_as(C.c_void_p), 0, None,
                                                          None, None), "wrong n"))
    assert (host_off == FILLW).all()
    ctx.stats()
    for buf, words in ((d_off, n + 2), (d_rec, 10 * total + 2), (d_cf, total), (d_tm, 3 * total)):
        assert (dev.host(buf, words, np.uint32) == FILLW).all(), "a refused call wrote a word"
    assert _export_bytes(ctx) == p["off"].tobytes() + p["rec"].tobytes() + p["coef"].tobytes() + p["terms"].tobytes()
    dev.close()
    ctx.close()
