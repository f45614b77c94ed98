#!/usr/bin/env python3
"""Golden fixtures for light placement at its edges, rendered by the
*reference* cpu/rt (build container only; TEST INFRASTRUCTURE, like
make_golden_shading.py).

Every other fixture keeps one directional light in general position and one
point light outside the geometry.  These are the lattice scene of
tests/light_edges_util.py -- walls with windows, a ceiling of skylights, a
closed box object and a larger floor, every coordinate an integer or a quarter
integer -- under each row of its light table: axis-aligned and tied
directions, directions of length 1e-20, 3e-39 (denormal), 1e30 and 0, point
lights on the lattice, on a vertex, in a wall's plane, on a corner of the
triangle box, inside the closed box and 1e6 to 3e38 away.  One scene per row:
an ambient light and the row's.

The scene text is generated here (our data), rendered by oracle/_ref/rt_probe
(the reference's cpu/ sources compiled unmodified by oracle/Makefile), and
stored as tests/golden/lights/<row>_<W>x<H>.svati.gz + .f32.gz + manifest.json
with the reference's query counts and the figures of
light_edges_util.check_conditions as they were when the fixtures were made.

    python tests/golden/make_golden_lights.py
"""
import gzip
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
PROBE = os.path.join(REPO, "oracle", "_ref", "rt_probe")
OUT = os.path.join(HERE, "lights")
sys.path.insert(0, os.path.dirname(HERE))
import light_edges_util as lu  # noqa: E402

NOTES = [
    "cpu/parser.c reads a light's vector with fscanf's %f, which takes -0.0, 1e-20 and denormals: every row is text.",
    "A directional light of length 0, 1e-20 or 3e-39 makes normalize() of cpu/light.c divide by (nearly) zero: "
    "whatever the reference writes there (NaN or unshadowed colours) is the expected value.",
    "A NaN channel is NaN in the frame; its sign and payload are the platform's and are not compared.",
]


def gz(path, data):
    with open(path, "wb") as raw:
        with gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0) as f:
            f.write(data)


def main():
    import oracle as orc
    import rtgpu
    os.makedirs(OUT, exist_ok=True)
    cases = []
    for r in lu.ROWS:
        name, slug = r[0], lu.row_slug(r[0])
        text = lu.scene_text(lu.row_lights(r))
        with tempfile.TemporaryDirectory() as td:
            sv = os.path.join(td, f"{slug}.svati")
            with open(sv, "w") as f:
                f.write(text)
            dump, ppm = os.path.join(td, "o.f32"), os.path.join(td, "o.ppm")
            p = subprocess.run(["bash", "-c", f"ulimit -s unlimited && exec {PROBE} {sv} {dump}"],
                               env=dict(os.environ, RT_PROBE_PPM=ppm), capture_output=True, text=True, check=True)
            m = re.search(r"closest_hit_queries=(\d+) shadow_queries=(\d+)", p.stderr)
            with open(dump, "rb") as f:
                assert f.readline() == f"RTF32 {lu.W} {lu.H}\n".encode()
                data = f.read()
            s = rtgpu.Scene.load_svati(sv)
            osc = orc.OracleScene(sv)
        sname, fname = f"{slug}_{lu.W}x{lu.H}.svati.gz", f"{slug}_{lu.W}x{lu.H}.f32.gz"
        gz(os.path.join(OUT, sname), text.encode())
        gz(os.path.join(OUT, fname), data)
        gold = np.frombuffer(data, np.float32).reshape(lu.H, lu.W, 3)
        case = {"row": name, "width": lu.W, "height": lu.H, "svati": sname, "file": fname,
                "closest": int(m.group(1)), "shadow": int(m.group(2)),
                "f32_sha256": hashlib.sha256(data).hexdigest(), "nan_words": int(np.isnan(gold).sum()),
                "triangles": s.triangle_count}
        for scene in (s.ptr, osc.ptr):  # the product's loader and the oracle's restated parser
            img, cnt = orc.render(scene, lu.W, lu.H, threads=0)
            bad = int(lu.words_differ(img, gold).sum())
            print(name, "oracle vs reference:", bad, "words differ;", cnt, case["closest"], case["shadow"])
        case["observed"] = lu.check_conditions(r, s)
        print(case)
        cases.append(case)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_lights.py (reference cpu/rt via oracle/_ref/rt_probe)",
                   "notes": NOTES, "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
