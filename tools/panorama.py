#!/usr/bin/env python3
"""An equirectangular panorama of a scene from its camera's position, through
the ray-batch API (rt_hip_trace_rays): one ray per pixel, the reference's
trace(ray, 1.0) each, written as a P3 PPM.

    python3 tools/panorama.py scene.svati out.ppm [--W 1024 --H 512] [--accel octree_gpu]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-gpu_amd"))
import rtgpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out")
    ap.add_argument("--W", type=int, default=1024)
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--accel", default="octree_gpu", choices=sorted(rtgpu.ACCEL))
    a = ap.parse_args()
    s = rtgpu.Scene.load_svati(a.scene)
    cam = s.camera
    o, d = rtgpu.equirect_rays((cam.position.x, cam.position.y, cam.position.z), a.W, a.H)
    ctx = rtgpu.Context(s, a.accel if s.triangle_count else "flat")
    rgb, _, st = ctx.trace_rays(o, d)
    rtgpu.write_ppm(a.out, rgb.reshape(a.H, a.W, 3))
    print(f"{a.out}: {a.W}x{a.H}, {st['camera']} rays, {st['closest']} closest-hit and {st['shadow']} shadow queries")


if __name__ == "__main__":
    main()
