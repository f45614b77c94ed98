#!/usr/bin/env python3
"""Cost of direct light for records on one GPU (not part of the product), in
one process: the frame is rendered with its G-buffer, the rank's G-buffer tile
buffer stays on the device (never copied to the host) and goes straight through
rt_hip_direct_light -- with and without the mask output, with and without
RT_RAYS_PACKET, the four variants alternating over --n rounds after --warmup,
each timed by device events around its launch on one stream -- and is set
against the shade pass's kernel time of the same frame in the same process
(Context.kernel_times): that pass asks the same queries of the same points
through the same buffers, for every hit record of the frame rather than the
first hits alone, plus the fold's bookkeeping; the time per query is printed
for both.

Prints one JSON line.  Run each invocation under a time limit of its own:

    timeout -k 10 300 python3 tools/direct_light_cost.py [--grid 32 --tris 9776 --W 3840 --H 2160] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-gpu_amd"))
import rtgpu  # noqa: E402


def _render_settled(ctx, frame, d_tiles):
    for attempt in range(3):  # (again after the hit buffers grew)
        ctx.render(frame, 0, 1, d_tiles)
        try:
            return ctx.stats()
        except rtgpu.RtError as e:
            if e.code != -10 or attempt == 2:
                raise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--tris", type=int, default=9776)
    ap.add_argument("--W", type=int, default=3840)
    ap.add_argument("--H", type=int, default=2160)
    ap.add_argument("--accel", default="octree_gpu")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=7, help="timed rounds of every variant")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    s = rtgpu.Scene.synthetic(a.grid, a.grid, a.tris, seed=0x5EED, width=a.W, height=a.H)
    f = s.frame()
    ctx = rtgpu.Context(s, a.accel)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    dev = torch.device("cuda", 0)

    def buf(n, dtype=torch.float32):
        return torch.empty(int(n), dtype=dtype, device=dev)

    words = rtgpu.gbuffer_tile_words(a.W, a.H, 1)
    n = words // rtgpu.GB_WORDS  # records of the tile buffer: 4 per pixel slot, padding slots included
    tiles = buf(rtgpu.tile_buffer_floats(a.W, a.H, 1))
    gt = buf(words, torch.int32)
    ctx.set_gbuffer(True)
    ctx.set_timing(True)
    _render_settled(ctx, f, tiles.data_ptr())
    shade_ms, st_frame = [], None
    for _ in range(a.warmup + a.n):  # the same frame's shade pass, by the render's own events
        ctx.render(f, 0, 1, tiles.data_ptr())
        st_frame = ctx.stats()
        shade_ms.append(ctx.kernel_times(1)[0])
    shade_ms = shade_ms[a.warmup:]
    ctx.gbuffer(f, 0, 1, gt.data_ptr())
    ctx.stats()
    rgb, lit = buf(3 * n), buf(n, torch.int32)

    def launch(with_lit, packet):
        return lambda: ctx.direct_light_device(gt.data_ptr(), n, rgb.data_ptr(), lit.data_ptr() if with_lit else 0,
                                               packet=packet, stream=sp)

    variants = {"rgb": launch(False, False), "rgb+lit": launch(True, False), "rgb packet": launch(False, True),
                "rgb+lit packet": launch(True, True)}
    ms = {name: [] for name in variants}
    stats = {}
    for rnd in range(a.warmup + a.n):
        for name, go in variants.items():  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            go()
            e1.record(stream)
            st = ctx.stats()
            e1.synchronize()
            if rnd >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
            stats[name] = {k: st[k] for k in ("camera", "shadow", "shadow_deferred", "shadow_unproven", "depth_overflow",
                                              "shadow_zero_risk")}
    nr = rtgpu.scene_materials(s.ptr)[:, 11]
    out = {"workload": f"synthetic {a.grid}x{a.grid} x {a.tris} tris, {a.W}x{a.H}, {a.accel}; the G-buffer tile buffer, "
                       f"{n} records, {int(s.s.light_count)} lights",
           "rounds": a.n, "warmup": a.warmup, "records": n, "variants": {},
           "frame": {"shadow": st_frame["shadow"], "hit_records": st_frame["hit_records"],
                     "trace_ms_median": round(statistics.median(x[0] for x in shade_ms), 4),
                     "shade_ms": [round(x[1], 4) for x in shade_ms],
                     "shade_ms_median": round(statistics.median(x[1] for x in shade_ms), 4)},
           "reflective_objects": int((nr != 0).sum())}
    for name in variants:
        m = statistics.median(ms[name])
        out["variants"][name] = {"ms": [round(x, 4) for x in ms[name]], "ms_median": round(m, 4),
                                 "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                                 "mrecords_per_s": round(stats[name]["camera"] / m / 1e3, 1), "stats": stats[name]}
    sm = out["frame"]["shade_ms_median"]
    out["ratios_to_the_shade_pass"] = {name: round(v["ms_median"] / sm, 3) for name, v in out["variants"].items()}
    # per query: the shade pass shades every hit record of the frame, the call the first hits only
    out["ns_per_query"] = {"shade pass": round(1e6 * sm / max(st_frame["shadow"], 1), 4),
                           **{name: round(1e6 * v["ms_median"] / max(v["stats"]["shadow"], 1), 4)
                              for name, v in out["variants"].items()}}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
