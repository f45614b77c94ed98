#!/usr/bin/env python3
"""Ambient occlusion of a scene's camera view through the occlusion-batch API
(rt_hip_occluded): render with the G-buffer, shoot --k cosine-weighted
hemisphere rays from every sample's first hit with a distance bound, and write
the per-pixel unoccluded share as a grey PNG (a pixel's four samples averaged;
samples that hit nothing count as open).

    python3 tools/ambient_occlusion.py scene.svati out.png [--W 640 --H 360] [--k 16] [--tmax-radii 0.25]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-gpu_amd"))
import rtgpu  # noqa: E402


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
    a = ap.parse_args()
    s = rtgpu.Scene.load_svati(a.scene)
    s.set_size(a.W, a.H)
    ctx = rtgpu.Context(s, a.accel if s.triangle_count else "flat")
    _, smp, _ = ctx.render_image_gbuffer(s.frame())
    smp = smp.reshape(-1)
    hit = (smp["prim"] >= 0) & smp["N"].any(axis=1)
    o, d = rtgpu.hemisphere_rays(smp["P"][hit], smp["N"][hit], a.k, a.seed)
    tmax = np.float32(a.tmax_radii * ctx.info()["scene_radius"]) if a.tmax_radii > 0 else None
    occ, st = ctx.occluded(o, d, tmax)
    open_share = np.ones(len(smp), np.float64)
    open_share[hit] = 1.0 - occ.reshape(-1, a.k).mean(axis=1)
    grey = np.rint(255.0 * open_share.reshape(a.H, a.W, 4).mean(axis=2)).astype(np.uint8)
    rgba = np.stack([grey, grey, grey, np.full_like(grey, 255)], axis=2)
    rtgpu.write_png(a.out, rgba)
    print(f"{a.out}: {a.W}x{a.H}, {int(hit.sum())} first hits x {a.k} rays, {st['shadow']} occlusion queries, "
          f"{100.0 * occ.mean() if len(occ) else 0.0:.1f} % occluded"
          + (f" within {float(tmax):g}" if tmax is not None else ""))


if __name__ == "__main__":
    main()
