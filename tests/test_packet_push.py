"""The packet walk pushes an interior node's wanted children in one vector
step (csrc/rt_push_plan.h, stage_push_children of csrc/rt_walk_wave.h) and the
wave stack holds what the serial far-to-near loop left there: the same records
and lane masks in the same slots.  Every walk is then the walk it was, which
shows on the GPU as

* work counters equal to the recording of the commit before the change
  (tests/golden/packet_push_parent.json): island_smooth 256x144, octree and
  octree_gpu, work-counting pass;
* images equal to the oracle's bit for bit under policy 0 (camera and coherent
  secondary rays through staged_closest), policy 2 (every query staged:
  stage_push_children<true> with the grown shadow boxes) and policy 3
  (directional-light shadows staged), at one wave (cube 8x8), ragged quarters
  (cube 34x18) and deep stacks of mirror paths (spheres 64x64).

Counters.  The closest-hit side's counts are sums over work items and each
item's walk is deterministic: closest, hits, pixels, closest_node_lanes,
closest_tri_lanes, node_visits - shadow_node_visits and tri_tests -
shadow_tri_tests were to be compared.  The parent was rendered twice before
recording, and shadow_tri_tests (with the clock counters) differed between
its two renders (octree 44,726 / 44,729, octree_gpu 45,203 / 45,412; the
golden file keeps both), so the difference tri_tests - shadow_tri_tests is
left out.  The trace kernel's own slots node_visits and tri_tests hold no
shadow query's work (flush_counts, csrc/rt_render.hip) and were equal in both
renders: they are compared themselves."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


def _scene(gpu, scene_dir, name, W, H):
    s = gpu.Scene.load_svati(os.path.join(scene_dir, name + ".svati"))
    s.set_size(W, H)
    return s


@pytest.mark.parametrize("accel", ["octree", "octree_gpu"])
def test_work_counters_equal_the_parent(gpu, scene_dir, accel):
    with open(os.path.join(GOLDEN, "packet_push_parent.json")) as fh:
        parent = json.load(fh)["stats"][accel]
    s = _scene(gpu, scene_dir, "island_smooth", 256, 144)
    ctx = gpu.Context(s, accel)
    ctx.set_count_work(True)
    _, st = ctx.render_image(s.frame())
    ctx.close()
    print({k: (st[k], parent[k]) for k in parent})
    assert st["depth_overflow"] == 0
    for k in ("closest", "hits", "pixels", "closest_node_lanes", "closest_tri_lanes", "node_visits", "tri_tests"):
        assert st[k] == parent[k], k
    assert st["node_visits"] - st["shadow_node_visits"] == parent["node_visits"] - parent["shadow_node_visits"]


_ORACLE = {}


def _oracle(s, name, W, H):
    """The oracle's frame, rendered once per (scene, size)."""
    if (name, W, H) not in _ORACLE:
        import oracle as orc
        img, cnt = orc.render(s.ptr, W, H, threads=4)
        _ORACLE[name, W, H] = (np.ascontiguousarray(img).reshape(H, W, 3), cnt)
    return _ORACLE[name, W, H]


CASES = [("cube", 8, 8), ("cube", 34, 18), ("spheres", 64, 64)]


@pytest.mark.parametrize("policy", [0, 2, 3])
@pytest.mark.parametrize("accel", ["octree", "octree_gpu"])
@pytest.mark.parametrize("scene,W,H", CASES, ids=[f"{n}_{w}x{h}" for n, w, h in CASES])
def test_images_match_the_oracle(gpu, scene_dir, scene, W, H, accel, policy):
    s = _scene(gpu, scene_dir, scene, W, H)
    ref, cnt = _oracle(s, scene, W, H)
    ctx = gpu.Context(s, accel)
    ctx.set_policy(policy)
    img, st = ctx.render_image(s.frame())
    ctx.close()
    bad = np.argwhere((np.ascontiguousarray(img).view(np.uint32) != ref.view(np.uint32)).any(axis=2))
    assert len(bad) == 0, \
        f"{scene} {W}x{H} {accel} policy {policy}: {len(bad)} pixels differ, first (row, col) {bad[:5].tolist()}"
    assert (st["closest"], st["shadow"]) == (cnt["closest"], cnt["shadow"])
    assert st["depth_overflow"] == 0
