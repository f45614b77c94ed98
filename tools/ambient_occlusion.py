#!/usr/bin/env python3
"""Ambient occlusion of a scene's camera view: render with the G-buffer, shoot
--k cosine-weighted hemisphere rays from every sample's first hit with a
distance bound, and write the per-pixel unoccluded share as a grey PNG (a
pixel's four samples averaged; samples that hit nothing count as open).

The default path goes through the host and the occlusion-batch API
(rt_hip_occluded): the G-buffer is downloaded, rtgpu.hemisphere_rays builds the
rays in numpy, the rays go up and one byte per ray comes down.  --device keeps
the samples on the device (rt_hip_render with the G-buffer, rt_hip_gbuffer,
rt_hip_assemble_gbuffer) and calls rt_hip_ambient_occlusion, which makes the
rays in the kernel from a --table-row table: only the counts are downloaded.
The two paths shoot different (equally distributed) rays.

    python3 tools/ambient_occlusion.py scene.svati out.png [--W 640 --H 360] [--k 16] [--tmax-radii 0.25] [--device]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-gpu_amd"))
import rtgpu  # noqa: E402


def ao_host(ctx, frame, k, seed, tmax):
    """The default path -> (open share per sample, first hits, stats, seconds
    per step: render + G-buffer download, ray generation, batch with copies)."""
    t0 = time.perf_counter()
    _, smp, _ = ctx.render_image_gbuffer(frame)
    smp = smp.reshape(-1)
    t1 = time.perf_counter()
    hit = (smp["prim"] >= 0) & smp["N"].any(axis=1)
    o, d = rtgpu.hemisphere_rays(smp["P"][hit], smp["N"][hit], k, seed)
    t2 = time.perf_counter()
    occ, st = ctx.occluded(o, d, tmax)
    open_share = np.ones(len(smp), np.float64)
    open_share[hit] = 1.0 - occ.reshape(-1, k).mean(axis=1)
    t3 = time.perf_counter()
    return open_share, int(hit.sum()), st, {"render_gbuffer_download": t1 - t0, "generation": t2 - t1,
                                            "batch_with_copies": t3 - t2}


def _render_settled(ctx, frame, d_tiles):
    for attempt in range(3):  # (again after the hit buffers grew)
        ctx.render(frame, 0, 1, d_tiles)
        try:
            return ctx.stats()
        except rtgpu.RtError as e:
            if e.code != -10 or attempt == 2:
                raise


def ao_device(ctx, frame, k, seed, tmax, rows=64):
    """--device -> (open share per sample, samples that shot, stats, seconds
    per step: render + G-buffer on the device, the fused kernel, the counts'
    download)."""
    L = rtgpu.lib()
    n = 4 * frame.width * frame.height
    table = rtgpu.ao_table(rows, seed)
    bufs = []

    def dev(nbytes):
        p = C.c_void_p()
        rtgpu._check(L.rt_hip_malloc(ctx.device, max(int(nbytes), 16), C.byref(p)), "rt_hip_malloc")
        bufs.append(p)
        return p.value
    try:
        t0 = time.perf_counter()
        d_c = dev(4 * rtgpu.tile_buffer_floats(frame.width, frame.height, 1))
        d_g = dev(4 * rtgpu.gbuffer_tile_words(frame.width, frame.height, 1))
        d_s, d_t, d_out = dev(4 * rtgpu.GB_WORDS * n), dev(table.nbytes), dev(4 * n)
        rtgpu._check(L.rt_hip_memcpy_h2d(C.c_void_p(d_t), table.ctypes.data_as(C.c_void_p), table.nbytes), "table")
        ctx.set_gbuffer(True)
        _render_settled(ctx, frame, d_c)
        ctx.gbuffer(frame, 0, 1, d_g)
        ctx.assemble_gbuffer(frame, d_g, 1, d_s)
        ctx.stats()
        ctx.set_gbuffer(False)
        t1 = time.perf_counter()
        ctx.ambient_occlusion_device(d_s, n, k, d_t, rows, seed, d_out, tmax=tmax)
        st = ctx.stats()
        t2 = time.perf_counter()
        counts = np.empty(n, np.uint32)
        rtgpu._check(L.rt_hip_memcpy_d2h(counts.ctypes.data_as(C.c_void_p), C.c_void_p(d_out), counts.nbytes), "counts")
        open_share = 1.0 - counts.astype(np.float64) / float(k)  # rtgpu.ao_open_share without the records
        t3 = time.perf_counter()
    finally:
        for p in bufs:
            L.rt_hip_free(p)
    return open_share, st["camera"] // k, st, {"render_gbuffer_on_device": t1 - t0, "kernel": t2 - t1,
                                               "counts_download": t3 - t2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out")
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--H", type=int, default=360)
    ap.add_argument("--k", type=int, default=16, help="hemisphere rays per first hit")
    ap.add_argument("--tmax-radii", type=float, default=0.25, help="the distance bound, in scene radii (0: none)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--accel", default="octree_gpu", choices=sorted(rtgpu.ACCEL))
    ap.add_argument("--device", action="store_true",
                    help="keep the samples on the device and make the rays in the kernel (rt_hip_ambient_occlusion)")
    ap.add_argument("--table-rows", type=int, default=64, help="--device: rows of the direction table")
    a = ap.parse_args()
    s = rtgpu.Scene.load_svati(a.scene)
    s.set_size(a.W, a.H)
    ctx = rtgpu.Context(s, a.accel if s.triangle_count else "flat")
    tmax = np.float32(a.tmax_radii * ctx.info()["scene_radius"]) if a.tmax_radii > 0 else None
    if a.device:
        open_share, shot, st, _ = ao_device(ctx, s.frame(), a.k, a.seed, tmax, a.table_rows)
    else:
        open_share, shot, st, _ = ao_host(ctx, s.frame(), a.k, a.seed, tmax)
    grey = np.rint(255.0 * open_share.reshape(a.H, a.W, 4).mean(axis=2)).astype(np.uint8)
    rgba = np.stack([grey, grey, grey, np.full_like(grey, 255)], axis=2)
    rtgpu.write_png(a.out, rgba)
    print(f"{a.out}: {a.W}x{a.H}, {shot} first hits x {a.k} rays, {st['shadow']} occlusion queries, "
          f"{100.0 * (1.0 - open_share).sum() / max(shot, 1):.1f} % occluded"
          + (f" within {float(tmax):g}" if tmax is not None else "") + (" (device)" if a.device else ""))


if __name__ == "__main__":
    main()
