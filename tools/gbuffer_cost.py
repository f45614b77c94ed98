#!/usr/bin/env python3
"""Cost of the opt-in G-buffer on one GPU (not part of the product): the
trace kernel with the capture off and on (alternating renders of one context,
device events: set_timing / kernel_times), and gbuffer_kernel (host clock
around `--reps` back-to-back launches ending in a synchronise, minus the
synchronise alone) with the bytes it moves.  Prints one JSON line.

    python3 tools/gbuffer_cost.py [--grid 32 --tris 9776 --W 3840 --H 2160] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=10, help="timed renders of each kind")
    ap.add_argument("--reps", type=int, default=10, help="gbuffer_kernel launches per timing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = rtgpu.Scene.synthetic(a.grid, a.grid, a.tris, seed=0x5EED, width=a.W, height=a.H)
    f = s.frame()
    ctx = rtgpu.Context(s, a.accel)
    ctx.set_timing(True)
    L = rtgpu.lib()
    dc, dg = C.c_void_p(), C.c_void_p()
    gwords = rtgpu.gbuffer_tile_words(a.W, a.H, 1)
    assert L.rt_hip_malloc(0, rtgpu.tile_buffer_floats(a.W, a.H, 1) * 4, C.byref(dc)) == 0
    assert L.rt_hip_malloc(0, gwords * 4, C.byref(dg)) == 0

    def render(on):
        ctx.set_gbuffer(on)
        ctx.render(f, 0, 1, dc.value)
        st = ctx.stats()
        return ctx.kernel_times(1)[0], st

    times = {False: [], True: []}
    for i in range(a.warmup + a.n):
        for on in (False, True):  # alternating, the capture's buffer allocated in the warm-up
            k, st = render(on)
            if i >= a.warmup:
                times[on].append(k)
    # gbuffer_kernel: the last render had the capture on
    ctx.gbuffer(f, 0, 1, dg.value)
    ctx.stats()
    gb = []
    for _ in range(5):
        t0 = time.perf_counter()
        ctx.stats()
        t1 = time.perf_counter()
        for _ in range(a.reps):
            ctx.gbuffer(f, 0, 1, dg.value)
        ctx.stats()
        t2 = time.perf_counter()
        gb.append(((t2 - t1) - (t1 - t0)) * 1e3 / a.reps)
    L.rt_hip_free(dc)
    L.rt_hip_free(dg)
    med = statistics.median
    tiles = rtgpu.tiles_per_rank(a.W, a.H, 1)
    samples = tiles * 64 * 4
    gb_ms = med(gb)
    written = gwords * 4                       # 40 B per sample of every tile slot
    read = samples * 16                        # the capture records
    # a hit sample also reads its 32 B hit record and its triangle's object
    # word; the stats count the hits of all bounces, so an upper bound
    hits_read = min(st["hits"], st["camera"]) * 36
    out = {
        "workload": f"synthetic {a.grid}x{a.grid} x {a.tris} tris, {a.W}x{a.H}, {a.accel}",
        "renders_each": a.n,
        "trace_ms_off": [round(k[0], 4) for k in times[False]],
        "trace_ms_on": [round(k[0], 4) for k in times[True]],
        "trace_ms_off_median": round(med(k[0] for k in times[False]), 4),
        "trace_ms_on_median": round(med(k[0] for k in times[True]), 4),
        "shade_ms_off_median": round(med(k[1] for k in times[False]), 4),
        "shade_ms_on_median": round(med(k[1] for k in times[True]), 4),
        "fold_ms_off_median": round(med(k[2] for k in times[False]), 4),
        "fold_ms_on_median": round(med(k[2] for k in times[True]), 4),
        "capture_bytes_written_by_trace": samples * 16,
        "gbuffer_kernel_ms": [round(x, 4) for x in gb],
        "gbuffer_kernel_ms_median": round(gb_ms, 4),
        "gbuffer_bytes_written": written,
        "gbuffer_bytes_read_capture": read,
        "gbuffer_bytes_read_records_upper_bound": hits_read,
        "gbuffer_write_GBps": round(written / gb_ms / 1e6, 1),
        "gbuffer_total_GBps_upper_bound": round((written + read + hits_read) / gb_ms / 1e6, 1),
    }
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
