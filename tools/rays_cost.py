#!/usr/bin/env python3
"""Cost of ray batches on one GPU (not part of the product): on one context,
in one process, alternating --

    render        rt_hip_render of the frame (lists, packet walk, shade, fold)
    pixel         the frame's 4 W H camera rays as a batch, pixel order
    quarter       the same rays in quarter order
    quarter_pkt   quarter order with RT_RAYS_PACKET
    equirect      an --EW x --EH panorama from the eye
    cast          quarter order, cast only (samples, no colours)

each timed by device events around its launches on one stream, after --warmup
rounds (the first grows the hit buffers), --n rounds.  Prints one JSON line.

    python3 tools/rays_cost.py [--grid 32 --tris 9776 --W 3840 --H 2160] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-gpu_amd"))
import rtgpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--tris", type=int, default=9776)
    ap.add_argument("--W", type=int, default=3840)
    ap.add_argument("--H", type=int, default=2160)
    ap.add_argument("--EW", type=int, default=4096)
    ap.add_argument("--EH", type=int, default=2048)
    ap.add_argument("--accel", default="octree_gpu")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=7, help="timed rounds of every variant")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    s = rtgpu.Scene.synthetic(a.grid, a.grid, a.tris, seed=0x5EED, width=a.W, height=a.H)
    f = s.frame()
    ctx = rtgpu.Context(s, a.accel)
    L = rtgpu.lib()
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    dev = torch.device("cuda", 0)

    def buf(n, dtype=torch.float32):
        return torch.empty(int(n), dtype=dtype, device=dev)

    nf = 4 * a.W * a.H
    tiles = buf(rtgpu.tile_buffer_floats(a.W, a.H, 1))
    rays = {}
    for order, code in (("pixel", 0), ("quarter", 1)):
        o, d = buf(3 * nf), buf(3 * nf)
        rtgpu._check(L.rt_hip_frame_rays(ctx.h, C.byref(f), code, o.data_ptr(), d.data_ptr(), sp), "rt_hip_frame_rays")
        rays[order] = (o, d, nf)
    cam = s.camera
    eo, ed = rtgpu.equirect_rays((cam.position.x, cam.position.y, cam.position.z), a.EW, a.EH)
    rays["equirect"] = (torch.from_numpy(eo).to(dev).reshape(-1), torch.from_numpy(ed).to(dev).reshape(-1), len(eo))
    rgb = buf(3 * max(nf, len(eo)))
    smp = buf(rtgpu.GB_WORDS * nf, torch.int32)
    stream.synchronize()

    def batch(order, packet=False, cast=False):
        o, d, n = rays[order]
        return lambda: ctx.trace_rays_device(o.data_ptr(), d.data_ptr(), n, 0 if cast else rgb.data_ptr(),
                                             smp.data_ptr() if cast else 0, packet=packet, stream=sp), n

    variants = {
        "render": (lambda: ctx.render(f, 0, 1, tiles.data_ptr(), stream=sp), nf),
        "pixel": batch("pixel"),
        "quarter": batch("quarter"),
        "quarter_pkt": batch("quarter", packet=True),
        "equirect": batch("equirect"),
        "cast": batch("quarter", cast=True),
    }
    ms = {k: [] for k in variants}
    stats = {}
    for rnd in range(a.warmup + a.n):
        for name, (launch, n) in variants.items():  # alternating
            for attempt in range(3):  # (again after the hit buffers grew)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch()
                e1.record(stream)
                try:
                    st = ctx.stats()
                    break
                except rtgpu.RtError as e:
                    if e.code != -10 or attempt == 2 or rnd >= a.warmup:
                        raise
            e1.synchronize()
            if rnd >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
            stats[name] = {k: st[k] for k in ("closest", "shadow", "camera", "pixels", "hits", "hit_records")}
    med = statistics.median
    base = med(ms["render"])
    out = {"workload": f"synthetic {a.grid}x{a.grid} x {a.tris} tris, {a.W}x{a.H}, {a.accel}; "
                       f"equirect {a.EW}x{a.EH}", "rounds": a.n, "warmup": a.warmup, "variants": {}}
    for name, (_, n) in variants.items():
        m = med(ms[name])
        out["variants"][name] = {"rays": n, "ms": [round(x, 4) for x in ms[name]], "ms_median": round(m, 4),
                                 "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                                 "mrays_per_s": round(n / m / 1e3, 1), "x_render": round(m / base, 3),
                                 "stats": stats[name]}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
