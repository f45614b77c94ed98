#!/usr/bin/env python3
"""Cost of ambient occlusion from G-buffer records on one GPU (not part of the
product), in one process:

(a) the fused kernel (rt_hip_ambient_occlusion) against its yardstick, an
    occlusion batch (rt_hip_occluded) on the very rays, as dumped by
    rt_hip_ao_rays -- tmax none and scene radius / 64, the four variants
    alternating over --n rounds after --warmup, each timed by device events
    around its launches on one stream; the counts must equal the batch's
    summed bytes on every ray;
(b) the wall time of tools/ambient_occlusion.py's two paths (its ao_host and
    ao_device) on the same scene and size, with each path's own split.

Prints one JSON line.

    python3 tools/ao_cost.py [--grid 32 --tris 9776 --W 3840 --H 2160 --k 4] [--no-e2e] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-gpu_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import rtgpu  # noqa: E402
from ambient_occlusion import _render_settled, ao_device, ao_host  # noqa: E402

SEED = 20261020


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--tris", type=int, default=9776)
    ap.add_argument("--W", type=int, default=3840)
    ap.add_argument("--H", type=int, default=2160)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rows", type=int, default=64, help="rows of the direction table")
    ap.add_argument("--accel", default="octree_gpu")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=7, help="timed rounds of every variant")
    ap.add_argument("--no-e2e", action="store_true", help="skip (b)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    s = rtgpu.Scene.synthetic(a.grid, a.grid, a.tris, seed=0x5EED, width=a.W, height=a.H)
    f = s.frame()
    ctx = rtgpu.Context(s, a.accel)
    R = float(ctx.info()["scene_radius"])
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    dev = torch.device("cuda", 0)

    def buf(n, dtype=torch.float32):
        return torch.empty(int(n), dtype=dtype, device=dev)

    # the records: the frame's assembled G-buffer, in device memory
    n, k = 4 * a.W * a.H, a.k
    tiles = buf(rtgpu.tile_buffer_floats(a.W, a.H, 1))
    gt = buf(rtgpu.gbuffer_tile_words(a.W, a.H, 1), torch.int32)
    smp = buf(rtgpu.GB_WORDS * n, torch.int32)
    ctx.set_gbuffer(True)
    _render_settled(ctx, f, tiles.data_ptr())
    ctx.gbuffer(f, 0, 1, gt.data_ptr())
    ctx.assemble_gbuffer(f, gt.data_ptr(), 1, smp.data_ptr())
    ctx.stats()
    ctx.set_gbuffer(False)
    del tiles, gt
    table = torch.from_numpy(rtgpu.ao_table(a.rows, SEED)).to(dev)
    ro, rd, shot = buf(3 * n * k), buf(3 * n * k), buf(n, torch.uint8)
    ctx.ao_rays_device(smp.data_ptr(), n, k, table.data_ptr(), a.rows, SEED, ro.data_ptr(), rd.data_ptr(),
                       shot.data_ptr(), stream=sp)
    stream.synchronize()
    tm = torch.full((n * k,), R / 64.0, dtype=torch.float32, device=dev)
    counts, bytes_ = buf(n, torch.int32), buf(n * k, torch.uint8)

    def ao(tmax):
        return lambda: ctx.ambient_occlusion_device(smp.data_ptr(), n, k, table.data_ptr(), a.rows, SEED,
                                                    counts.data_ptr(), tmax=tmax, stream=sp)

    def batch(t):
        return lambda: ctx.occluded_device(ro.data_ptr(), rd.data_ptr(), t.data_ptr() if t is not None else 0, n * k,
                                           bytes_.data_ptr(), stream=sp)

    variants = {"ao": ao(None), "batch": batch(None), "ao_r64": ao(np.float32(R / 64.0)), "batch_r64": batch(tm)}
    ms = {name: [] for name in variants}
    stats, differ, share = {}, {}, {}
    for rnd in range(a.warmup + a.n):
        for name, launch in variants.items():  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            st = ctx.stats()
            e1.synchronize()
            if rnd >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
            stats[name] = {key: st[key] for key in ("camera", "shadow", "depth_overflow", "shadow_zero_risk")}
            if rnd == 0 and name.startswith("batch"):  # the counts against the summed bytes, every ray
                with torch.cuda.stream(stream):
                    sums = bytes_.view(n, k).sum(dim=1, dtype=torch.int32)
                    differ[name] = int((sums != counts).sum())
                    share[name] = float(bytes_.float().sum() / max(stats[name]["camera"], 1))
                stream.synchronize()
    out = {"workload": f"synthetic {a.grid}x{a.grid} x {a.tris} tris, {a.W}x{a.H}, {a.accel}; {n} records, "
                       f"{k} rays each from a {a.rows}-row table, scene radius {R:g}",
           "rounds": a.n, "warmup": a.warmup, "records": n, "records_shot": int(shot.sum()), "variants": {},
           "occluded_share_of_traced_rays": share, "records_whose_count_differs_from_the_batch": differ}
    for name in variants:
        m = statistics.median(ms[name])
        out["variants"][name] = {"ms": [round(x, 4) for x in ms[name]], "ms_median": round(m, 4),
                                 "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                                 "mrays_per_s": round(stats[name]["camera"] / m / 1e3, 1), "stats": stats[name]}
    v = out["variants"]
    out["ratios"] = {"ao / batch": round(v["ao"]["ms_median"] / v["batch"]["ms_median"], 3),
                     "ao_r64 / batch_r64": round(v["ao_r64"]["ms_median"] / v["batch_r64"]["ms_median"], 3)}
    del ro, rd, tm, bytes_, counts, smp, shot
    torch.cuda.empty_cache()
    if not a.no_e2e:
        e2e = {}
        for name, path in (("device", ao_device), ("default", ao_host)):
            t0 = time.perf_counter()
            open_share, rays_from, st, split = path(ctx, f, k, SEED, np.float32(R / 64.0))
            e2e[name] = {"wall_s": round(time.perf_counter() - t0, 3), "split_s": {key: round(x, 3) for key, x in split.items()},
                         "first_hits": int(rays_from), "queries": st["shadow"],
                         "mean_open_share": round(float(open_share.mean()), 5)}
            del open_share
        out["end_to_end"] = e2e
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
