"""Every counter rt_hip_stats reports, pinned to a recording: the own scene
mirrors at 96x54 (host octree: the trace and shade kernels, bounces) rendered
with the work-counting pass on, then relit after a colour-only light edit,
each integer field of Stats.as_dict() compared with
tests/golden/own/mirrors_96x54_stats.json.  The slots' numbers, the
shade-side set the relight zeroes and the slot -> rt_stats member table
(csrc/rt_counters.h) all show here: a slot moved or a member filled from
another slot changes a field.

The fixture was recorded at commit 985109c (the last one that spelled the
slots by number) by this file run as a program,
  python tests/test_counter_stats.py > tests/golden/own/mirrors_96x54_stats.json
twice.  The cycles_* fields are shader clocks and are left out.  The two
recordings differed in one more field, the counting render's shadow_tri_tests
(148180 and 149637): the shade kernel counts a triangle record once per wave,
and which 64 hit records share a wave follows the order the trace's waves
appended them in, which varies from run to run.  That field of the render is
left out too; every other field was equal.  A relight refuses the counting
pass, so it is switched off between the two calls; the relight's fields are
those of the plain shade kernel.
"""
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "own", "mirrors_96x54_stats.json")


# (call, field) pairs that vary between two runs of the same library (above)
UNSTABLE = {("render", "shadow_tri_tests")}


def record(rtgpu, svati):
    """{"render": ..., "relight": ...}: Stats.as_dict() without the clocks and UNSTABLE."""
    s = rtgpu.Scene.load_svati(svati)
    f = s.frame()
    ctx = rtgpu.Context(s, "octree")
    ctx.set_count_work(True)
    _, render = ctx.render_image(f)
    L = s.lights()
    k = next(i for i, l in enumerate(L) if l.type in (1, 2))
    L[k].r, L[k].g, L[k].b = L[k].r * 0.5, L[k].g * 0.25, L[k].b * 0.75
    ctx.set_lights(L)
    ctx.set_count_work(False)
    _, relight = ctx.relight_image(f)
    ctx.close()
    return {name: {k: v for k, v in st.items() if not k.startswith("cycles_") and (name, k) not in UNSTABLE}
            for name, st in (("render", render), ("relight", relight))}


@pytest.mark.gpu
def test_stats_match_the_recording(built, tmp_path):
    import rtgpu
    from conftest import load_own_manifest, own_scene_path
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    case = next(c for c in load_own_manifest() if (c["width"], c["height"]) == (96, 54))
    with open(FIXTURE) as f:
        want = json.load(f)
    got = record(rtgpu, own_scene_path(case, tmp_path))
    for call in ("render", "relight"):
        print(call, got[call])
        assert set(got[call]) == set(want[call])
        diff = {k: (got[call][k], want[call][k]) for k in want[call] if got[call][k] != want[call][k]}
        assert not diff, f"{call}: (got, recorded) {diff}"
    # the recording itself is of the frame the reference's golden counts
    assert want["render"]["closest"] == case["closest"] and want["render"]["shadow"] == case["shadow"]
    assert want["relight"]["shadow"] == case["shadow"] and want["render"]["shadow_tri_lanes"] > 0


if __name__ == "__main__":
    import gzip
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "raytracing-gpu_amd"))
    import rtgpu
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "mirrors.svati")
        with gzip.open(os.path.join(here, "golden", "own", "mirrors_96x54.svati.gz"), "rb") as i, \
                open(path, "wb") as o:
            o.write(i.read())
        json.dump(record(rtgpu, path), sys.stdout, indent=1, sort_keys=True)
        print()
