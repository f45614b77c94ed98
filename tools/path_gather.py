#!/usr/bin/env python3
"""A frame with one-bounce indirect light at every path vertex (not part of
the product): what a mirror shows is lit the way the surface in front of the
camera is.

The frame's camera rays are traced as a ray batch and the batch's paths are
exported (rt_hip_path_records): every bounce of every ray as a surface record
with its coef.  rt_hip_direct_light gives every vertex its direct light,
rt_hip_gather the light its --k hemisphere rays bring back; the gathered sum
over k times the object's diffuse colour kd is the vertex's indirect light.
The frame is

    sample = fold over the path, deepest first, of
             color_mul(color_add(direct_v, indirect_v), coef_v)

with the reference's colour algebra (rtgpu.path_fold, rtgpu.color_mul) and a
pixel's four samples folded by rtgpu.fold_samples.  With --k 0 the indirect
term is left out and the frame is the render's own, bit for bit.

    python3 tools/path_gather.py scene.svati out.png [--W 320 --H 180] [--k 16] [--rows 64]
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
    ap.add_argument("--W", type=int, default=320)
    ap.add_argument("--H", type=int, default=180)
    ap.add_argument("--k", type=int, default=16, help="hemisphere rays per path vertex (0: direct light only)")
    ap.add_argument("--rows", type=int, default=64, help="rows of the direction table")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--accel", default="octree_gpu", choices=sorted(rtgpu.ACCEL))
    a = ap.parse_args()
    f32 = np.float32
    s = rtgpu.Scene.load_svati(a.scene)
    s.set_size(a.W, a.H)
    frame = s.frame()
    ctx = rtgpu.Context(s, a.accel if s.triangle_count else "flat")
    o, d = ctx.frame_rays(frame, "pixel")
    rgb, off, rec, coef, terms, st = ctx.trace_paths(o, d)
    direct, _, _ = ctx.direct_light(rec)
    light = direct
    rays = 0
    if a.k > 0 and len(rec):
        table = rtgpu.ao_table(a.rows, a.seed)
        gathered, gst = ctx.gather(rec, a.k, table, a.seed)  # (takes the hit records: the paths are on the host by now)
        rays = gst["camera"]
        kd = s.materials_array()[:, 3:6][rec["obj"]]
        indirect = (gathered / f32(a.k) * kd).astype(f32)
        light = direct + indirect
        light = np.where(light > f32(255), f32(255), light).astype(f32)  # color_add's clamp
    vertex = rtgpu.color_mul(light, coef)
    samples = rtgpu.path_fold(off, vertex)
    if a.k <= 0:
        same = (samples.view(np.uint32) == rgb.view(np.uint32)) | (np.isnan(samples) & np.isnan(rgb))
        assert same.all(), "without the indirect term the composition is the batch's own colours"
    img = rtgpu.fold_samples(samples).reshape(a.H, a.W, 3)
    rgba = np.concatenate([np.rint(np.nan_to_num(img)).astype(np.uint8), np.full((a.H, a.W, 1), 255, np.uint8)], axis=2)
    rtgpu.write_png(a.out, rgba)
    ln = np.diff(off.astype(np.int64))
    print(f"{a.out}: {a.W}x{a.H}, {len(o)} camera rays, {len(rec)} path vertices ({int((ln > 1).sum())} rays bounce, "
          f"longest path {int(ln.max()) if len(ln) else 0}), {rays} gather rays; mean sample "
          f"{float(np.nan_to_num(rgb).mean()):.2f} -> {float(np.nan_to_num(samples).mean()):.2f}")


if __name__ == "__main__":
    main()
