#!/usr/bin/env python3
"""Golden fixtures for the shading and fold arithmetic at its edges, rendered
by the *reference* cpu/rt (build container only; TEST INFRASTRUCTURE, like
make_golden_adversarial.py).

The reference's scenes and the adversarial ones keep Ns among five tame
exponents, every channel and light colour in [0, 1], Nr among six values and
every light off the surfaces.  These scenes are the stage of
tests/shading_edges_util.py -- a floor, a panel that sends reflections into the
sky, a dome of diverging normals -- with the floor cut into one patch per row
of the edge material table, or under edge lights:

  ns                    every Ns of the table (0, -0.0, fractions, 3e38, negative, 1e-45, inf, -inf, nan)
  channels              every Ka / Kd / Ks channel of the table (outside [0, 1], denormal, inf, nan)
  nr                    every Nr of the table under a panel of Nr 0.5 (the floats around (float)0.01 too)
  lights-below-grazing  directional light from below and at dot(L, N) = +0.0 and -0.0, point lights
                        in the floor's plane and below it
  lights-colours        light colours from the channel table that stay a channel's own affair
  lights-huge           the colours 1e30 and inf (their channel is 255 wherever the light reaches)
  lights-nan            the NaN colours (their channel is NaN wherever the light reaches)
  lights-33             33 lights, an edge colour in the table's second block

The scene text is generated here (our data), rendered by oracle/_ref/rt_probe
(the reference's cpu/ sources compiled unmodified by oracle/Makefile), and
stored as tests/golden/shading/<scene>_<W>x<H>.svati.gz + .f32.gz +
manifest.json.

    python tests/golden/make_golden_shading.py
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
OUT = os.path.join(HERE, "shading")
sys.path.insert(0, os.path.dirname(HERE))
import shading_edges_util as su  # noqa: E402

W, H = 32, 18

NOTES = [
    "cpu/parser.c and cpu/parse_obj.c read every number with fscanf's %f, which takes nan, inf, -inf, -0.0 and "
    "denormals (1e-45 becomes the smallest one): every value of the material and colour tables is text.",
    "The parser has keywords for ambient, directional and point lights only: a light of type 3 (SPECULAR) or of "
    "an unknown type cannot be written; cpu/light.c:94 skips both.  They exist in memory only "
    "(tests/test_shading_edges.py).",
    "A light next to or on a hit point needs the hit point's bits, which a camera ray does not give exactly: in "
    "memory only, on caller-supplied rays.",
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
    for name, text in su.fixture_scenes().items():
        with tempfile.TemporaryDirectory() as td:
            sv = os.path.join(td, f"{name}.svati")
            with open(sv, "w") as f:
                f.write(text)
            dump, ppm = os.path.join(td, "o.f32"), os.path.join(td, "o.ppm")
            p = subprocess.run(["bash", "-c", f"ulimit -s unlimited && exec {PROBE} {sv} {dump}"],
                               env=dict(os.environ, RT_PROBE_PPM=ppm), capture_output=True, text=True, check=True)
            m = re.search(r"closest_hit_queries=(\d+) shadow_queries=(\d+)", p.stderr)
            with open(dump, "rb") as f:
                assert f.readline() == f"RTF32 {W} {H}\n".encode()
                data = f.read()
            s = rtgpu.Scene.load_svati(sv)
            osc = orc.OracleScene(sv)
        sname, fname = f"{name}_{W}x{H}.svati.gz", f"{name}_{W}x{H}.f32.gz"
        gz(os.path.join(OUT, sname), text.encode())
        gz(os.path.join(OUT, fname), data)
        gold = np.frombuffer(data, np.float32).reshape(H, W, 3)
        case = {"scene": name, "width": W, "height": H, "svati": sname, "file": fname,
                "closest": int(m.group(1)), "shadow": int(m.group(2)),
                "f32_sha256": hashlib.sha256(data).hexdigest(),
                "nan_words": int(np.isnan(gold).sum()), "words_255": int((gold == 255).sum())}
        for scene in (s.ptr, osc):  # the product's loader and the oracle's restated parser
            img, cnt = orc.render(scene, W, H, threads=0)
            bad = int(su.words_differ(img, gold).sum())
            print(name, "oracle vs reference:", bad, "words differ;", cnt, case["closest"], case["shadow"])
        print(case, {"triangles": s.triangle_count, "lit": round(float((gold != 0).any(axis=2).mean()), 3)})
        cases.append(case)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_shading.py (reference cpu/rt via oracle/_ref/rt_probe)",
                   "notes": NOTES, "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
