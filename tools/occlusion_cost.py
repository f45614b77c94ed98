#!/usr/bin/env python3
"""Cost of occlusion batches on one GPU (not part of the product): on one
context, in one process, alternating --

    cast_cam      (a) the frame's 4 W H camera rays in quarter order, cast only
    occl_cam      (b) rt_hip_occluded of the same rays, unbounded
    occl_cam_pkt  (c) (b) with RT_RAYS_PACKET
    occl_hemi     (d) --k cosine-weighted hemisphere rays per first hit of (a), unbounded
    occl_hemi_r64 (e) (d) with tmax = scene radius / 64
    cast_hemi     (f) the cast of (d)'s rays

each timed by device events around its launches on one stream, after --warmup
rounds (the first grows the hit buffers), --n rounds.  The yardstick of an
any-hit batch is the existing cast on the same rays.  Prints one JSON line.

    python3 tools/occlusion_cost.py [--grid 32 --tris 9776 --W 3840 --H 2160] [--out FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-gpu_amd"))
import rtgpu  # noqa: E402


def hemisphere_rays_device(P, N, k, seed):
    """rtgpu.hemisphere_rays with torch on the device (float32 throughout)."""
    g = torch.Generator(device=P.device)
    g.manual_seed(seed)
    n = N / N.norm(dim=1, keepdim=True).clamp_min(1e-30)
    ax = torch.nn.functional.one_hot(n.abs().argmin(dim=1), 3).to(n.dtype)
    t = torch.linalg.cross(ax, n)
    t = t / t.norm(dim=1, keepdim=True)
    b = torch.linalg.cross(n, t)
    r = torch.rand((len(P), k), generator=g, device=P.device).sqrt() * 0.999
    phi = 2.0 * math.pi * torch.rand((len(P), k), generator=g, device=P.device)
    x, y, z = r * phi.cos(), r * phi.sin(), (1.0 - r * r).sqrt()
    d = x[..., None] * t[:, None] + y[..., None] * b[:, None] + z[..., None] * n[:, None]
    d = d / d.norm(dim=-1, keepdim=True)
    return P.repeat_interleave(k, dim=0).contiguous(), d.reshape(-1, 3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--tris", type=int, default=9776)
    ap.add_argument("--W", type=int, default=3840)
    ap.add_argument("--H", type=int, default=2160)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--accel", default="octree_gpu")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=7, help="timed rounds of every variant")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    s = rtgpu.Scene.synthetic(a.grid, a.grid, a.tris, seed=0x5EED, width=a.W, height=a.H)
    f = s.frame()
    ctx = rtgpu.Context(s, a.accel)
    R = float(ctx.info()["scene_radius"])
    L = rtgpu.lib()
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    dev = torch.device("cuda", 0)

    def buf(n, dtype=torch.float32):
        return torch.empty(int(n), dtype=dtype, device=dev)

    def settle(launch):
        for attempt in range(3):  # (again after the hit buffers grew)
            launch()
            try:
                return ctx.stats()
            except rtgpu.RtError as e:
                if e.code != -10 or attempt == 2:
                    raise

    nf = 4 * a.W * a.H
    co, cd = buf(3 * nf), buf(3 * nf)
    rtgpu._check(L.rt_hip_frame_rays(ctx.h, C.byref(f), 1, co.data_ptr(), cd.data_ptr(), sp), "rt_hip_frame_rays")
    csmp = buf(rtgpu.GB_WORDS * nf, torch.int32)
    settle(lambda: ctx.trace_rays_device(co.data_ptr(), cd.data_ptr(), nf, 0, csmp.data_ptr(), stream=sp))
    with torch.cuda.stream(stream):
        rec = csmp.view(nf, rtgpu.GB_WORDS)
        PN = rec[:, 4:10].view(torch.float32)
        hit = (rec[:, 0] >= 0) & (PN[:, 3:6] != 0).any(dim=1)
        ho, hd = hemisphere_rays_device(PN[hit][:, 0:3].contiguous(), PN[hit][:, 3:6].contiguous(), a.k, 20261020)
        nh = len(ho)
        tm = torch.full((nh,), R / 64.0, dtype=torch.float32, device=dev)
    hsmp = buf(rtgpu.GB_WORDS * nh, torch.int32)
    out_c, out_h = buf(nf, torch.uint8), buf(nh, torch.uint8)
    stream.synchronize()

    def cast(o, d, n, smp):
        return lambda: ctx.trace_rays_device(o.data_ptr(), d.data_ptr(), n, 0, smp.data_ptr(), stream=sp), n

    def occl(o, d, t, n, out, packet=False):
        return lambda: ctx.occluded_device(o.data_ptr(), d.data_ptr(), t.data_ptr() if t is not None else 0, n,
                                           out.data_ptr(), packet=packet, stream=sp), n

    variants = {
        "cast_cam": cast(co, cd, nf, csmp),
        "occl_cam": occl(co, cd, None, nf, out_c),
        "occl_cam_pkt": occl(co, cd, None, nf, out_c, packet=True),
        "occl_hemi": occl(ho, hd, None, nh, out_h),
        "occl_hemi_r64": occl(ho, hd, tm, nh, out_h),
        "cast_hemi": cast(ho, hd, nh, hsmp),
    }
    ms = {k: [] for k in variants}
    stats, share = {}, {}
    for rnd in range(a.warmup + a.n):
        for name, (launch, n) in variants.items():  # alternating
            for attempt in range(3):
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
            stats[name] = {k: st[k] for k in ("closest", "shadow", "camera", "hits", "hit_records", "depth_overflow")}
            if rnd == 0 and name.startswith("occl"):
                share[name] = float((out_c if "cam" in name else out_h).float().mean())
    # the bytes against the casts' answers on the same rays
    agree = {
        "occl_cam vs cast_cam": int(((csmp.view(nf, rtgpu.GB_WORDS)[:, 0] >= 0) != (out_c != 0)).sum()),
    }
    settle(variants["occl_hemi"][0])
    agree["occl_hemi vs cast_hemi"] = int(((hsmp.view(nh, rtgpu.GB_WORDS)[:, 0] >= 0) != (out_h != 0)).sum())
    med = statistics.median
    out = {"workload": f"synthetic {a.grid}x{a.grid} x {a.tris} tris, {a.W}x{a.H}, {a.accel}; "
                       f"{a.k} hemisphere rays per first hit, scene radius {R:g}",
           "rounds": a.n, "warmup": a.warmup, "variants": {}, "occluded_share": share,
           "rays_differing_from_the_cast": agree}
    for name, (_, n) in variants.items():
        m = med(ms[name])
        out["variants"][name] = {"rays": n, "ms": [round(x, 4) for x in ms[name]], "ms_median": round(m, 4),
                                 "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                                 "mrays_per_s": round(n / m / 1e3, 1), "stats": stats[name]}
    v = out["variants"]
    out["ratios"] = {"occl_cam / cast_cam": round(v["occl_cam"]["ms_median"] / v["cast_cam"]["ms_median"], 3),
                     "occl_cam_pkt / cast_cam": round(v["occl_cam_pkt"]["ms_median"] / v["cast_cam"]["ms_median"], 3),
                     "occl_hemi / cast_hemi": round(v["occl_hemi"]["ms_median"] / v["cast_hemi"]["ms_median"], 3),
                     "occl_hemi_r64 / occl_hemi": round(v["occl_hemi_r64"]["ms_median"] / v["occl_hemi"]["ms_median"], 3)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
