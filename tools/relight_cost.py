#!/usr/bin/env python3
"""Cost of relighting on one GPU (not part of the product): renders with
keep-visibility off and on (alternating, the context's own device events:
set_timing / frame_times / kernel_times), then relights of three edits --
colours only, one casting light moved, every casting light moved -- each
timed with device events on the render's stream, with the wall time of
rt_hip_set_lights for the edit, and each relit image compared bit for bit
with a fresh context's render of the edited scene.  Prints one JSON line.

    python3 tools/relight_cost.py [--grid 32 --tris 9776 --W 3840 --H 2160] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before the product library: both then share one HIP runtime

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-gpu_amd"))
import rtgpu  # noqa: E402

HBM_STREAM_TBPS = 6.3  # what a streaming kernel reaches on this chip (float4 copy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--tris", type=int, default=9776)
    ap.add_argument("--W", type=int, default=3840)
    ap.add_argument("--H", type=int, default=2160)
    ap.add_argument("--accel", default="octree_gpu")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=8, help="timed renders / relights of each kind")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    s = rtgpu.Scene.synthetic(a.grid, a.grid, a.tris, seed=0x5EED, width=a.W, height=a.H)
    f = s.frame()
    ctx = rtgpu.Context(s, a.accel)
    ctx.set_timing(True)
    L = rtgpu.lib()
    stream = torch.cuda.Stream(device=0)
    sh = stream.cuda_stream
    dt, drgb = C.c_void_p(), C.c_void_p()
    assert L.rt_hip_malloc(0, rtgpu.tile_buffer_floats(a.W, a.H, 1) * 4, C.byref(dt)) == 0
    assert L.rt_hip_malloc(0, a.W * a.H * 3 * 4, C.byref(drgb)) == 0
    med = statistics.median

    # ---- renders, keep-visibility off / on ----
    rt = {False: [], True: []}
    st = None
    for i in range(a.warmup + a.n):
        for on in (False, True):
            ctx.set_keep_visibility(on)
            ctx.render(f, 0, 1, dt.value, sh)
            st = ctx.stats()
            if i >= a.warmup:
                lists, kern = ctx.frame_times(1)[0]
                rt[on].append((lists + kern,) + tuple(ctx.kernel_times(1)[0]))
    records = st["hit_records"]
    lights = s.lights()
    casting = [i for i, l in enumerate(lights) if l.type in (1, 2)]

    def image():
        ctx.assemble(f, dt.value, 1, drgb.value, sh)
        ctx.stats()
        img = np.empty((a.H, a.W, 3), np.float32)
        assert L.rt_hip_memcpy_d2h(img.ctypes.data_as(C.c_void_p), drgb, img.nbytes) == 0
        return img

    # ---- relights: every repetition is a real edit (two states, alternating) ----
    def colour(k):
        lights[casting[0]].r = 0.5 if k & 1 else 1.0
        lights[0].g = 0.3 if k & 1 else 0.2

    def one(k):
        lights[casting[-1]].v.x += 0.75 if k & 1 else -0.75

    def every(k):
        for i in casting:
            lights[i].v.y += 0.5 if k & 1 else -0.5

    out = {
        "workload": f"synthetic {a.grid}x{a.grid} x {a.tris} tris, {a.W}x{a.H}, {a.accel}",
        "timed_each": a.n, "hit_records": records, "lights": len(lights), "casting_lights": len(casting),
    }
    for name, arr in (("off", rt[False]), ("on", rt[True])):
        out[f"render_ms_keep_{name}"] = [round(x[0], 4) for x in arr]
        out[f"render_ms_keep_{name}_median"] = round(med(x[0] for x in arr), 4)
        for j, ph in enumerate(("trace", "shade", "fold")):
            out[f"{ph}_ms_keep_{name}_median"] = round(med(x[1 + j] for x in arr), 4)
    out["shade_plus_fold_ms_median"] = round(med(x[2] + x[3] for x in rt[False]), 4)
    ctx.set_keep_visibility(True)
    ctx.render(f, 0, 1, dt.value, sh)
    ctx.stats()
    for name, edit in (("colour_only", colour), ("one_light_moved", one), ("all_lights_moved", every)):
        ms, wall, shadow = [], [], []
        for k in range(1, ((a.warmup + a.n) | 1) + 1):  # ends in the edited state (odd k)
            edit(k)
            t0 = time.perf_counter()
            ctx.set_lights(lights)
            t1 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.relight(f, 0, 1, dt.value, sh)
            e1.record(stream)
            rst = ctx.stats()
            e1.synchronize()
            if k > a.warmup:
                ms.append(e0.elapsed_time(e1))
                wall.append((t1 - t0) * 1e3)
                shadow.append(rst["shadow"])
        img = image()
        fresh_ctx = rtgpu.Context(s, a.accel)
        fimg, fst = fresh_ctx.render_image(f)
        fresh_ctx.close()
        out[name] = {
            "relight_ms": [round(x, 4) for x in ms], "relight_ms_median": round(med(ms), 4),
            "set_lights_wall_ms": [round(x, 3) for x in wall], "set_lights_wall_ms_median": round(med(wall), 3),
            "shadow_queries": shadow[-1], "fresh_shadow_queries": fst["shadow"],
            "shadow_deferred": rst["shadow_deferred"], "fresh_shadow_deferred": fst["shadow_deferred"],
            "equals_fresh_context_bit_for_bit": bool(np.array_equal(img.view(np.uint32), fimg.view(np.uint32))),
        }
    cms = out["colour_only"]["relight_ms_median"]
    moved = records * (36 + 16)
    # the colour-only relight is relight_zero + recolour_kernel + fold; the fold's time is the render's
    rec_ms = max(cms - out["fold_ms_keep_on_median"], 1e-6)
    out["recolour_bytes"] = moved
    out["recolour_ms_without_fold"] = round(rec_ms, 4)
    out["recolour_GBps"] = round(moved / rec_ms / 1e6, 1)
    out["recolour_GBps_of_whole_relight"] = round(moved / cms / 1e6, 1)
    out["recolour_byte_bound_ms"] = round(moved / (HBM_STREAM_TBPS * 1e9), 4)
    L.rt_hip_free(dt)
    L.rt_hip_free(drgb)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
