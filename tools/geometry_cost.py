#!/usr/bin/env python3
"""Cost of moving geometry on one GPU (not part of the product): on the C5
scene (Scene.synthetic()), one sphere moved from a device tensor.  Times, in
one process: rt_hip_create on the scene (wall); a full update (every triangle)
and a one-object update (wall around the synchronous call, and the call's own
split into flatten + box + flags, tree, light buffers: rt_hip_geometry_times);
then animation steps of update + render.  The last step's image is compared
bit for bit with a fresh context's render of the edited scene.  Prints one
JSON line.

    python3 tools/geometry_cost.py [--grid 32 --tris 9776 --W 3840 --H 2160] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--tris", type=int, default=9776)
    ap.add_argument("--W", type=int, default=3840)
    ap.add_argument("--H", type=int, default=2160)
    ap.add_argument("--accel", default="octree_gpu")
    ap.add_argument("--object", type=int, default=1, help="the object that moves")
    ap.add_argument("--n", type=int, default=3, help="timed updates of each kind, and creates")
    ap.add_argument("--steps", type=int, default=8, help="animation steps of update + render")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    s = rtgpu.Scene.synthetic(a.grid, a.grid, a.tris, seed=0x5EED, width=a.W, height=a.H)
    f = s.frame()
    L = rtgpu.lib()
    med = statistics.median
    ms = lambda xs: [round(1e3 * x, 3) for x in xs]  # noqa: E731

    # ---- rt_hip_create on the same scene, in this process ----
    create_wall, create_info = [], None
    ctx = None
    for _ in range(a.n):
        if ctx:
            ctx.close()
        t0 = time.perf_counter()
        ctx = rtgpu.Context(s, a.accel)
        create_wall.append(time.perf_counter() - t0)
        create_info = ctx.info()

    tris = s.triangles_array()
    ntri = len(tris)
    first, count = rtgpu.object_range(s, a.object)
    ext = rtgpu.vertex_extent(tris)
    d_all = torch.from_numpy(tris.reshape(ntri, 18)).cuda()          # the caller's vertices: a device tensor
    step = torch.tensor([float(ext) * 2.0 ** -10, 0.0, 0.0] * 3 + [0.0] * 9, dtype=torch.float32, device="cuda")

    def move():  # the object's vertices a little further along x (float32, on the device)
        d_all[first:first + count] += step
        torch.cuda.synchronize()

    def update(whole):
        move()
        t0 = time.perf_counter()
        if whole:
            ctx.set_triangles_device(d_all.data_ptr(), 0, ntri)
        else:
            ctx.set_triangles_device(d_all[first:].data_ptr(), first, count)
        return (time.perf_counter() - t0,) + ctx.geometry_times()

    out = {"workload": f"synthetic {a.grid}x{a.grid} x {a.tris} tris, {a.W}x{a.H}, {a.accel}",
           "triangles": ntri, "moved_object": a.object, "moved_triangles": count, "timed_each": a.n}
    out["create_wall_ms"] = ms(create_wall)
    out["create_wall_ms_median"] = round(1e3 * med(create_wall), 3)
    out["create_build_ms"] = round(1e3 * create_info["build_seconds"], 3)
    out["create_lightbuf_ms"] = round(1e3 * create_info["lightbuf_seconds"], 3)
    for name, whole in (("full_update", True), ("one_object_update", False)):
        update(whole)  # (the first update allocates its buffers)
        rows = [update(whole) for _ in range(a.n)]
        out[name] = {"wall_ms": ms(r[0] for r in rows), "wall_ms_median": round(1e3 * med(r[0] for r in rows), 3),
                     "flatten_box_flags_ms_median": round(1e3 * med(r[1] for r in rows), 3),
                     "tree_ms_median": round(1e3 * med(r[2] for r in rows), 3),
                     "light_buffers_ms_median": round(1e3 * med(r[3] for r in rows), 3)}
        out[name]["create_over_update"] = round(med(create_wall) / med(r[0] for r in rows), 3)

    # ---- animation: update + render, streamed ----
    dt, drgb = C.c_void_p(), C.c_void_p()
    assert L.rt_hip_malloc(0, rtgpu.tile_buffer_floats(a.W, a.H, 1) * 4, C.byref(dt)) == 0
    assert L.rt_hip_malloc(0, a.W * a.H * 3 * 4, C.byref(drgb)) == 0
    ctx.render(f, 0, 1, dt.value)
    ctx.stats()
    upd, ren = [], []
    for _ in range(a.steps):
        u = update(False)
        t0 = time.perf_counter()
        for attempt in range(3):  # (a new geometry's first frame may outgrow a buffer once: render again)
            ctx.render(f, 0, 1, dt.value)
            try:
                ctx.stats()
                break
            except rtgpu.RtError as e:
                if e.code != -10:
                    raise
        upd.append(u[0])
        ren.append(time.perf_counter() - t0)
    out["animation"] = {"steps": a.steps, "update_wall_ms": ms(upd), "render_wall_ms": ms(ren),
                        "update_wall_ms_median": round(1e3 * med(upd), 3),
                        "render_wall_ms_median": round(1e3 * med(ren), 3),
                        "step_wall_ms_median": round(1e3 * med(x + y for x, y in zip(upd, ren)), 3)}
    ctx.assemble(f, dt.value, 1, drgb.value)
    ctx.stats()
    img = np.empty((a.H, a.W, 3), np.float32)
    assert L.rt_hip_memcpy_d2h(img.ctypes.data_as(C.c_void_p), drgb, img.nbytes) == 0
    s.set_triangles_array(d_all.cpu().numpy())
    fresh = rtgpu.Context(s, a.accel)
    fimg, _ = fresh.render_image(f)
    same_info = {k: v for k, v in fresh.info().items() if "seconds" not in k} == \
                {k: v for k, v in ctx.info().items() if "seconds" not in k}
    fresh.close()
    out["equals_fresh_context_bit_for_bit"] = bool(np.array_equal(img.view(np.uint32), fimg.view(np.uint32)))
    out["info_equals_fresh_context"] = bool(same_info)
    out["geometry_updates"] = ctx.geometry_updates()
    L.rt_hip_free(dt)
    L.rt_hip_free(drgb)
    ctx.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
