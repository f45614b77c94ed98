#!/usr/bin/env python3
"""A small example of direct light for caller's points (rt_hip_direct_light)
and of the light that arrives by way of other surfaces (rt_hip_gather): a
lattice of light probes in free space over a scene, six axis normals each,
shaded with one object's material and written as .npy.

    python3 tools/bake_probes.py scene.svati probes.npy [--n 8] [--obj 0] [--accel octree_gpu] [--bounce K]

probes.npy holds (n, n, n, 6, 3) float32: the colour (0..255 per channel) that
arrives at the probe for the normals +x -x +y -y +z -z, in lattice order x, y,
z over the scene's box.  <out>.lit.npy holds the unshadowed-light masks, (n, n,
n) uint32 (the mask does not depend on the normal).  With --bounce K,
<out>.bounce.npy holds (n, n, n, 6, 3) float32: per probe normal the raw sum of
the traced colours of K rays over its hemisphere (cosine-weighted table
directions; not divided by K, no weight -- the mean radiance estimate is sum /
K), and <out>.bounce.k.npy the K it was gathered with."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-gpu_amd"))
import rtgpu  # noqa: E402

NORMALS = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float32)


def probe_lattice(scene, n):
    """(n^3, 3) float32 points over the box of the scene's vertices."""
    v = scene.triangles_array()[:, :3].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    axes = [np.linspace(lo[a], hi[a], n, dtype=np.float32) for a in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)


def bake(ctx, points, obj):
    P = np.repeat(points, len(NORMALS), axis=0)
    N = np.tile(NORMALS, (len(points), 1))
    rgb, lit, st = ctx.direct_light(rtgpu.records_from_points(P, N, obj), packet=True, lit=True)
    return rgb.reshape(len(points), len(NORMALS), 3), lit.reshape(len(points), len(NORMALS))[:, 0], st


def bounce(ctx, points, obj, k, seed=20261021):
    """The raw sums of k traced hemisphere rays per (probe, normal)."""
    P = np.repeat(points, len(NORMALS), axis=0)
    N = np.tile(NORMALS, (len(points), 1))
    rgb, st = ctx.gather(rtgpu.records_from_points(P, N, obj), k, rtgpu.ao_table(max(64, k), seed), seed)
    return rgb.reshape(len(points), len(NORMALS), 3), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("out")
    ap.add_argument("--n", type=int, default=8, help="probes per axis")
    ap.add_argument("--obj", type=int, default=0, help="the object whose material shades the probes")
    ap.add_argument("--accel", default="octree_gpu")
    ap.add_argument("--bounce", type=int, default=0, metavar="K",
                    help="also gather K traced rays per probe normal (1..%d)" % rtgpu.AO_KMAX)
    a = ap.parse_args()
    s = rtgpu.Scene.load_obj(a.scene) if a.scene.endswith(".obj") else rtgpu.Scene.load_svati(a.scene)
    ctx = rtgpu.Context(s, a.accel)
    rgb, lit, st = bake(ctx, probe_lattice(s, a.n), a.obj)
    np.save(a.out, rgb.reshape(a.n, a.n, a.n, len(NORMALS), 3))
    np.save(os.path.splitext(a.out)[0] + ".lit.npy", lit.reshape(a.n, a.n, a.n))
    print(f"{a.n ** 3} probes x {len(NORMALS)} normals: {st['camera']} records shaded, {st['shadow']} shadow queries, "
          f"{st['shadow_deferred']} of them off a light buffer's proof box; mean colour {rgb.mean(axis=(0, 1)).round(2).tolist()}")
    if a.bounce:
        stem = os.path.splitext(a.out)[0]
        sums, sb = bounce(ctx, probe_lattice(s, a.n), a.obj, a.bounce)
        np.save(stem + ".bounce.npy", sums.reshape(a.n, a.n, a.n, len(NORMALS), 3))
        np.save(stem + ".bounce.k.npy", np.int32(a.bounce))
        print(f"bounce: {sb['camera']} rays traced ({a.bounce} per probe normal), {sb['closest']} closest-hit and "
              f"{sb['shadow']} shadow queries; mean of sum / K {(sums.mean(axis=(0, 1)) / a.bounce).round(2).tolist()}")


if __name__ == "__main__":
    main()
