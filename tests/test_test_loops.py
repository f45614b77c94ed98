"""The packet walk's test loops take their wave-wide verdicts straight from the
compares (consider_w of csrc/rt_isect.h, box_wants_w / stage_push_children and
staged_closest's re-test of csrc/rt_walk_wave.h, cand_range of
csrc/rt_query.h; the verdicts' arithmetic: rt_box_wants and rt_box_within of
host/rt_cull.h) and an octree fetch no longer carries the slot it can never
fill.  Only instruction sequences changed: every query pops the same nodes,
pushes the same children and passes the same records to the exact test.  On the
GPU that shows as

* work counters equal to the recording of the commit before the change
  (tests/golden/test_loops_parent.json) on scenes tests/test_packet_push.py
  does not pin: spheres 64x64 (mirror paths, deep stacks) and car-on-road
  100x52 (non-empty candidate lists), octree and octree_gpu, work-counting pass;
* images equal to the oracle's bit for bit under policy 0, policy 2 (every
  query staged) and policy 3 (directional-light shadows staged): one wave
  (cube 8x8), ragged quarters (cube 34x18) and a frame whose camera looks
  straight down the y axis from above the cube's centre (cube-down 16x16).

Counters.  closest, hits, pixels, closest_node_lanes, closest_tri_lanes,
node_visits, tri_tests and cand_entries are compared.  The parent was rendered
twice per case before recording; the fields that differed between its own two
renders are listed per case in the golden file ("differs_between_the_two_
renders") and none of the compared ones is among them.

The axis frame.  Every golden scene's camera already looks along -z (u = +x,
v = -y), so its centre column and row have a zero direction component each.
cube-down moves the camera to (0, 6, 0) looking along -y (u = +x, v = +z): the
centre pixel's ray has two zero components (rt_inv's +-1e30 clamp on both),
its origin's x and z are zeros lying between the cube's faces, and the rays of
the centre column and row run parallel to the faces' planes."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIELDS = ("closest", "hits", "pixels", "closest_node_lanes", "closest_tri_lanes", "node_visits", "tri_tests",
          "cand_entries")


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


@pytest.fixture(scope="module")
def scenes(scene_dir, tmp_path_factory):
    """Scene name -> .svati path: the golden scenes and cube-down."""
    d = tmp_path_factory.mktemp("test_loops")
    lines = open(os.path.join(scene_dir, "cube.svati")).read().split("\n")
    cam = next(i for i, ln in enumerate(lines) if ln.startswith("camera"))
    lines[cam] = "camera 512 512 0.0 6.0 0.0 1.0 0.0 0.0 0.0 0.0 1.0 70.0"
    down = d / "cube-down.svati"
    down.write_text("\n".join(lines))
    paths = {n: os.path.join(scene_dir, n + ".svati") for n in ("cube", "spheres", "car-on-road")}
    paths["cube-down"] = str(down)
    return paths


def _scene(gpu, scenes, name, W, H):
    s = gpu.Scene.load_svati(scenes[name])
    s.set_size(W, H)
    return s


COUNTED = [("spheres", 64, 64), ("car-on-road", 100, 52)]


@pytest.mark.parametrize("accel", ["octree", "octree_gpu"])
@pytest.mark.parametrize("scene,W,H", COUNTED, ids=[f"{n}_{w}x{h}" for n, w, h in COUNTED])
def test_work_counters_equal_the_parent(gpu, scenes, scene, W, H, accel):
    with open(os.path.join(GOLDEN, "test_loops_parent.json")) as fh:
        rec = json.load(fh)["cases"][f"{scene}_{W}x{H}/{accel}"]
    parent = rec["stats"]
    assert not set(FIELDS) & set(rec["differs_between_the_two_renders"])
    s = _scene(gpu, scenes, scene, W, H)
    ctx = gpu.Context(s, accel)
    ctx.set_count_work(True)
    _, st = ctx.render_image(s.frame())
    ctx.close()
    print({k: (st[k], parent[k]) for k in FIELDS})
    assert st["depth_overflow"] == 0
    for k in FIELDS:
        assert st[k] == parent[k], k


_ORACLE = {}


def _oracle(s, name, W, H):
    """The oracle's frame, rendered once per (scene, size)."""
    if (name, W, H) not in _ORACLE:
        import oracle as orc
        img, cnt = orc.render(s.ptr, W, H, threads=4)
        _ORACLE[name, W, H] = (np.ascontiguousarray(img).reshape(H, W, 3), cnt)
    return _ORACLE[name, W, H]


CASES = [("cube", 8, 8), ("cube", 34, 18), ("cube-down", 16, 16)]


@pytest.mark.parametrize("policy", [0, 2, 3])
@pytest.mark.parametrize("accel", ["octree", "octree_gpu"])
@pytest.mark.parametrize("scene,W,H", CASES, ids=[f"{n}_{w}x{h}" for n, w, h in CASES])
def test_images_match_the_oracle(gpu, scenes, scene, W, H, accel, policy):
    s = _scene(gpu, scenes, scene, W, H)
    ref, cnt = _oracle(s, scene, W, H)
    if scene == "cube-down":  # the frame shows the cube: the walk is exercised, not only the sky
        assert cnt["shadow"] > 0
    ctx = gpu.Context(s, accel)
    ctx.set_policy(policy)
    img, st = ctx.render_image(s.frame())
    ctx.close()
    bad = np.argwhere((np.ascontiguousarray(img).view(np.uint32) != ref.view(np.uint32)).any(axis=2))
    assert len(bad) == 0, \
        f"{scene} {W}x{H} {accel} policy {policy}: {len(bad)} pixels differ, first (row, col) {bad[:5].tolist()}"
    assert (st["closest"], st["shadow"]) == (cnt["closest"], cnt["shadow"])
    assert st["depth_overflow"] == 0
