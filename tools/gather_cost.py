#!/usr/bin/env python3
"""Cost of the gather (rt_hip_gather) on one GPU (not part of the product), in
one process: the fused call against the composition it replaces, on the
records of a frame's assembled G-buffer, processed in pieces with `base` so the
hit-record buffers fit:

    gather        rt_hip_gather per piece
    composition   rt_hip_ao_rays (24 B a ray written), rt_hip_trace_rays on them
                  (read back, 12 B of colour a ray written) and the sequential
                  sum over k in torch (the colours read again), per piece

each with and without RT_RAYS_PACKET: one run that allocates (a piece whose
rt_hip_stats reports RT_EHITBUF is made again), then --n timed runs, the four
variants alternating, every piece timed by device events around its launches
on one stream and the pieces' times summed.  The sums must be equal on every
record.  Prints one JSON line.

    python3 tools/gather_cost.py [--grid 32 --tris 9776 --W 3840 --H 2160 --k 4 --piece 2097152] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracing-gpu_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import rtgpu  # noqa: E402
from ambient_occlusion import _render_settled  # noqa: E402

SEED = 20261020
RT_EHITBUF = -10


def torch_gather_sum(colours, k):
    """rtgpu.gather_sum on the device: sequential, in ray order, the clamp after each add."""
    c = colours.view(-1, k, 3)
    acc = torch.zeros((c.shape[0], 3), dtype=torch.float32, device=c.device)
    for r in range(k):
        acc = acc + c[:, r, :]
        acc = torch.where(acc > 255.0, torch.full_like(acc, 255.0), acc)
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--tris", type=int, default=9776)
    ap.add_argument("--W", type=int, default=3840)
    ap.add_argument("--H", type=int, default=2160)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rows", type=int, default=64, help="rows of the direction table")
    ap.add_argument("--piece", type=int, default=1 << 21, help="records of a piece")
    ap.add_argument("--accel", default="octree_gpu")
    ap.add_argument("--n", type=int, default=3, help="timed runs of every variant")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    s = rtgpu.Scene.synthetic(a.grid, a.grid, a.tris, seed=0x5EED, width=a.W, height=a.H)
    f = s.frame()
    ctx = rtgpu.Context(s, a.accel)
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
    pieces = [(lo, min(lo + a.piece, n)) for lo in range(0, n, a.piece)]
    most = max(hi - lo for lo, hi in pieces)
    ro, rd, col = buf(3 * most * k), buf(3 * most * k), buf(3 * most * k)
    out_g, out_c = buf(3 * n), buf(3 * n)
    rec = 4 * rtgpu.GB_WORDS  # bytes of a record

    def timed(steps):
        """The steps' launches between events on the stream -> ms per step; the
        stats afterwards (they wait).  RT_EHITBUF: the buffers grew, None."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(steps) + 1)]
        ev[0].record(stream)
        for j, step in enumerate(steps):
            step()
            ev[j + 1].record(stream)
        try:
            st = ctx.stats()
        except rtgpu.RtError as e:
            if e.code != RT_EHITBUF:
                raise
            return None, None
        ev[-1].synchronize()
        return [ev[j].elapsed_time(ev[j + 1]) for j in range(len(steps))], st

    def gather_piece(lo, hi, packet):
        return [lambda: ctx.gather_device(smp.data_ptr() + rec * lo, hi - lo, k, table.data_ptr(), a.rows, SEED,
                                          out_g.data_ptr() + 12 * lo, packet=packet, base=lo, stream=sp)]

    def composition_piece(lo, hi, packet):
        nr = (hi - lo) * k

        def rays():
            ctx.ao_rays_device(smp.data_ptr() + rec * lo, hi - lo, k, table.data_ptr(), a.rows, SEED, ro.data_ptr(),
                               rd.data_ptr(), base=lo, stream=sp)

        def trace():
            ctx.trace_rays_device(ro.data_ptr(), rd.data_ptr(), nr, col.data_ptr(), packet=packet, stream=sp)

        def total():
            with torch.cuda.stream(stream):
                out_c[3 * lo:3 * hi] = torch_gather_sum(col[:3 * nr], k).reshape(-1)

        return [rays, trace, total]

    variants = {"gather": (gather_piece, False), "gather_packet": (gather_piece, True),
                "composition": (composition_piece, False), "composition_packet": (composition_piece, True)}
    names = {"gather": ["gather"], "composition": ["ao_rays", "trace_rays", "torch_sum"]}
    runs = {name: [] for name in variants}
    stats, retried, differ = {}, {name: 0 for name in variants}, {}
    for rnd in range(1 + a.n):  # (round 0 allocates)
        for name, (piece, packet) in variants.items():  # alternating
            split = None
            total_st = {"camera": 0, "closest": 0, "shadow": 0, "hit_records": 0, "depth_overflow": 0}
            for lo, hi in pieces:
                ms, st = timed(piece(lo, hi, packet))
                if ms is None:  # the hit buffers grew: the piece again
                    retried[name] += 1
                    ms, st = timed(piece(lo, hi, packet))
                    assert ms is not None, "RT_EHITBUF twice"
                split = ms if split is None else [x + y for x, y in zip(split, ms)]
                for key in total_st:
                    total_st[key] += st[key]
            if rnd:
                runs[name].append(split)
            stats[name] = total_st
            if name.startswith("composition"):  # the sums against the gather's, every record
                stream.synchronize()
                g, c = out_g.view(torch.int32), out_c.view(torch.int32)
                both_nan = torch.isnan(out_g) & torch.isnan(out_c)
                differ[f"round {rnd} {name}"] = int((((g != c) & ~both_nan).view(-1, 3)).any(dim=1).sum())
    shot = int(stats["gather"]["camera"]) // k
    out = {"workload": f"synthetic {a.grid}x{a.grid} x {a.tris} tris, {a.W}x{a.H}, {a.accel}; {n} records of the "
                       f"frame's assembled G-buffer, {k} rays each from a {a.rows}-row table, in {len(pieces)} pieces of "
                       f"{a.piece} records with their bases",
           "timed_runs": a.n, "records": n, "records_traced": shot, "pieces": len(pieces), "piece_records": a.piece,
           "pieces_made_again_after_RT_EHITBUF": retried, "records_whose_sum_differs": differ,
           "lit_records": int((out_g.view(-1, 3) != 0).any(dim=1).sum()), "variants": {}}
    for name in variants:
        steps = names[name.split("_")[0]]
        tot = [sum(r) for r in runs[name]]
        out["variants"][name] = {
            "ms": [round(x, 3) for x in tot], "ms_median": round(statistics.median(tot), 3),
            "split_ms_median": {step: round(statistics.median(r[j] for r in runs[name]), 3) for j, step in enumerate(steps)},
            "mrays_per_s": round(stats[name]["camera"] / statistics.median(tot) / 1e3, 1), "stats": stats[name]}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
