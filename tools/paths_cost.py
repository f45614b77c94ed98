#!/usr/bin/env python3
"""Cost of the path export (rt_hip_path_records) on one GPU (not part of the
product), on one context, in one process, alternating --

    batch    the frame's 4 W H camera rays in quarter order as a ray batch
    export   rt_hip_path_records of that batch: offsets, records, coef, terms
    count    the same call with no array (the two walks' first, the scans)
    copy     a device-to-device copy of the bytes the export reads and writes

each timed by device events around its launches on one stream, after one round
that allocates (a batch whose rt_hip_stats reports RT_EHITBUF is made again),
--n timed rounds.  The bytes of `copy`: per ray its `last` word twice and its
offset written twice and read once; per vertex the hit record (32 B), its link
twice (the two walks) and its term (16 B) read, 56 B written.  The export's
terms are folded in torch and compared with the batch's colours on every ray.
Prints one JSON line.

    python3 tools/paths_cost.py [--grid 32 --tris 9776 --W 3840 --H 2160] [--out FILE]
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

RT_EHITBUF = -10


def torch_path_fold(offsets, terms, n):
    """rtgpu.path_fold on the device: deepest first, the clamp after each add."""
    off = offsets.to(torch.int64)
    ln = off[1:] - off[:-1]
    acc = torch.zeros((n, 3), dtype=torch.float32, device=terms.device)
    for d in range(int(ln.max())):
        on = torch.nonzero(ln > d).reshape(-1)
        a = acc[on] + terms[off[on + 1] - 1 - d]
        acc[on] = torch.where(a > 255.0, torch.full_like(a, 255.0), a)
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--tris", type=int, default=9776)
    ap.add_argument("--W", type=int, default=3840)
    ap.add_argument("--H", type=int, default=2160)
    ap.add_argument("--accel", default="octree_gpu")
    ap.add_argument("--n", type=int, default=3, help="timed rounds of every variant")
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

    n = 4 * a.W * a.H
    o, d = buf(3 * n), buf(3 * n)
    rtgpu._check(L.rt_hip_frame_rays(ctx.h, C.byref(f), 1, o.data_ptr(), d.data_ptr(), sp), "rt_hip_frame_rays")
    rgb = buf(3 * n)
    off = buf(n + 1, torch.int32)

    def timed(launch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def batch():
        """The batch, timed; again (untimed result dropped) after the hit buffers grew."""
        for attempt in range(3):
            ms = timed(lambda: ctx.trace_rays_device(o.data_ptr(), d.data_ptr(), n, rgb.data_ptr(), stream=sp))
            try:
                return ms, ctx.stats()
            except rtgpu.RtError as e:
                if e.code != RT_EHITBUF or attempt == 2:
                    raise

    _, st = batch()  # allocates
    total = int(st["hit_records"])
    rec, coef, terms = buf(rtgpu.GB_WORDS * total, torch.int32), buf(total), buf(3 * total)
    nbytes = n * (2 * 4 + 3 * 4) + total * (32 + 2 * 4 + 16 + 56)
    # a copy of b bytes reads b and writes b: half the export's bytes, copied once
    src, dst = buf(nbytes // 2, torch.int8), buf(nbytes // 2, torch.int8)
    src.zero_()

    def export():
        ctx.path_records_device(n, off.data_ptr(), total, rec.data_ptr(), coef.data_ptr(), terms.data_ptr(), stream=sp)

    def count():
        ctx.path_records_device(n, off.data_ptr(), stream=sp)

    def copy():
        with torch.cuda.stream(stream):
            dst.copy_(src)

    timed(export), timed(count), timed(copy)  # (the scratch array's allocation)
    ms = {"batch": [], "export": [], "count": [], "copy": []}
    for _ in range(a.n):
        ms["batch"].append(batch()[0])
        ms["export"].append(timed(export))
        ms["count"].append(timed(count))
        ms["copy"].append(timed(copy))
    export()
    stream.synchronize()
    assert int(off[n]) == total, (int(off[n]), total)
    fold = torch_path_fold(off, terms.view(-1, 3), n)
    both_nan = torch.isnan(fold) & torch.isnan(rgb.view(-1, 3))
    differ = int(((fold.view(torch.int32) != rgb.view(-1, 3).view(torch.int32)) & ~both_nan).any(dim=1).sum())
    ln = (off[1:] - off[:-1]).to(torch.int64)
    med = statistics.median
    out = {"workload": f"synthetic {a.grid}x{a.grid} x {a.tris} tris, {a.W}x{a.H}, {a.accel}; the frame's {n} camera rays "
                       "in quarter order as a ray batch, its paths exported",
           "timed_rounds": a.n, "rays": n, "vertices": total, "rays_with_a_vertex": int((ln > 0).sum()),
           "longest_path": int(ln.max()), "bytes_read_and_written": nbytes, "rays_whose_fold_differs": differ,
           "variants": {k: {"ms": [round(x, 4) for x in v], "ms_median": round(med(v), 4)} for k, v in ms.items()}}
    out["export_over_batch"] = round(med(ms["export"]) / med(ms["batch"]), 3)
    out["export_over_copy"] = round(med(ms["export"]) / med(ms["copy"]), 3)
    out["export_gb_per_s"] = round(nbytes / med(ms["export"]) / 1e6, 1)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
