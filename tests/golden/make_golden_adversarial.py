#!/usr/bin/env python3
"""Golden fixtures for adversarial scenes of our own, rendered by the
*reference* cpu/rt (build container only; TEST INFRASTRUCTURE, like
make_golden_own.py).

The reference's scenes, `mirrors` and the synthetic sphere field keep the
camera outside the geometry, send no ray with a zero direction component and
hold no two coinciding triangles.  Three scenes that do the opposite:

  twins    every triangle twice, in two objects (the second copy in reverse
           order), on integer coordinates: every hit is an exact tie that
           cpu/hit.c:59,82's strict '<' gives to the earlier object.
  room     eye, film plane and point light inside a closed, tessellated room
           with a mirror wall; triangles across the eye and film planes,
           between film and eye, and behind the film.
  slivers  zero-area triangles, needles 4 long and 2^-k wide, right triangles
           small and steep enough for Moller-Trumbore's `a` to cross 1e-7,
           under an 8000-unit ground triangle.

The scene text is generated here (our data), rendered by oracle/_ref/rt_probe
(the reference's cpu/ sources compiled unmodified by oracle/Makefile), and
stored as tests/golden/adversarial/<scene>_<W>x<H>.svati.gz + .f32.gz +
manifest.json.  Every case is checked against tests/adversarial_util.py's
check_conditions before it is listed.

    python tests/golden/make_golden_adversarial.py
"""
import gzip
import hashlib
import json
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
PROBE = os.path.join(REPO, "oracle", "_ref", "rt_probe")
OUT = os.path.join(HERE, "adversarial")
sys.path.insert(0, os.path.dirname(HERE))
import adversarial_util as adv  # noqa: E402

FOV = 50
SIZES = [(32, 18), (96, 54)]


def film_distance(w):
    """L of cpu/raytracer.c:82-86."""
    return w / (2 * math.tan(FOV * math.pi / 360))


def num(x):
    return repr(float(x))


def obj(material, tris):
    """One object: tris = [((v0, v1, v2), normal)], file order."""
    lines = [f"object {3 * len(tris)}"] + material
    for vs, _ in tris:
        lines += ["v " + " ".join(num(c) for c in v) for v in vs]
    for _, n in tris:
        lines += ["vn " + " ".join(num(c) for c in n)] * 3
    return lines + [""]


def mat(ka, kd, nr, ks=(0.3, 0.3, 0.3), ns=12):
    return ["Ka " + " ".join(map(num, ka)), "Kd " + " ".join(map(num, kd)), "Ks " + " ".join(map(num, ks)),
            f"Ns {ns}", f"Nr {num(nr)}"]


def lattice(origin, du, dv, nu, nv, normal, keep=lambda i, j: True):
    """nu x nv quads from `origin` along du, dv, the diagonals alternating;
    quad (i, j) is left out unless keep(i, j)."""
    o, du, dv = (np.array(x, np.float64) for x in (origin, du, dv))
    tris = []
    for i in range(nu):
        for j in range(nv):
            if not keep(i, j):
                continue
            a, b, c, d = o + i * du + j * dv, o + (i + 1) * du + j * dv, o + (i + 1) * du + (j + 1) * dv, \
                o + i * du + (j + 1) * dv
            quads = [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
            tris += [(tuple(map(tuple, q)), normal) for q in quads]
    return tris


def box(lo, hi):
    """The 12 triangles of an axis-aligned box, outward normals."""
    lo, hi = np.array(lo, np.float64), np.array(hi, np.float64)
    tris = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for side, at in ((-1.0, lo[a]), (1.0, hi[a])):
            o, du, dv, n = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
            o[a], o[b], o[c] = at, lo[b], lo[c]
            du[b], dv[c], n[a] = hi[b] - lo[b], hi[c] - lo[c], side
            tris += lattice(o, du, dv, 1, 1, tuple(n))
    return tris


def twins(w, h):
    # camera u = +x, v = -y: w = u x v = -z, the film at z = -9 - L, rays towards +z
    wall = lattice((-4, -4, 2), (1, 0, 0), (0, 1, 0), 8, 8, (0, 0, -1))
    cube = box((-1, -1, -1), (1, 1, 1))
    floor = lattice((-4, -2, -2), (8, 0, 0), (0, 0, 4), 1, 1, (0, 1, 0))
    objs = []
    objs += obj(mat((0.10, 0.02, 0.02), (0.8, 0.2, 0.2), 0.3), wall)
    objs += obj(mat((0.02, 0.02, 0.10), (0.1, 0.2, 0.9), 0.0), wall[::-1])
    objs += obj(mat((0.02, 0.10, 0.02), (0.2, 0.8, 0.2), 0.5), cube)
    objs += obj(mat((0.10, 0.10, 0.02), (0.9, 0.8, 0.1), 0.0), cube[::-1])
    # the third pair: the *later* object reflects, so a wrong winner changes the query counts
    objs += obj(mat((0.08, 0.02, 0.08), (0.7, 0.2, 0.7), 0.0), floor)
    objs += obj(mat((0.02, 0.08, 0.08), (0.1, 0.7, 0.7), 0.4), floor[::-1])
    return "\n".join([f"camera {w} {h} 0 0 -9 1 0 0 0 -1 0 {FOV}", "a_light 0.3 0.3 0.3",
                      "d_light 1 0.9 0.8 0.25 -0.5 1", "p_light 0.6 0.6 0.6 3 4 -6", ""] + objs), {}


def room(w, h):
    L = film_distance(w)
    R = 2.0 ** math.ceil(math.log2(4 * L))  # a power of two >= 4 L
    ex, ey, ez = 0.0, -0.75 * R, -0.5 * R   # the eye; the film plane is z = ez - L

    def q(x):
        return round(x * 16) / 16
    s = R / 4  # the walls' lattice step
    walls = [  # (origin, du, dv, inward normal, material)
        ((-R, -R, -R), (0, s, 0), (0, 0, s), (1, 0, 0), mat((0.10, 0.03, 0.03), (0.8, 0.3, 0.3), 0.0)),
        ((R, -R, -R), (0, s, 0), (0, 0, s), (-1, 0, 0), mat((0.03, 0.10, 0.03), (0.3, 0.8, 0.3), 0.0)),
        ((-R, -R, -R), (s, 0, 0), (0, 0, s), (0, 1, 0), mat((0.08, 0.08, 0.08), (0.7, 0.7, 0.7), 0.0)),
        ((-R, R, -R), (s, 0, 0), (0, 0, s), (0, -1, 0), mat((0.06, 0.06, 0.10), (0.5, 0.5, 0.9), 0.0)),
        ((-R, -R, -R), (s, 0, 0), (0, s, 0), (0, 0, 1), mat((0.10, 0.08, 0.02), (0.9, 0.7, 0.2), 0.0)),
        ((-R, -R, R), (s, 0, 0), (0, s, 0), (0, 0, -1), mat((0.04, 0.04, 0.04), (0.3, 0.3, 0.35), 0.6)),  # the mirror
    ]
    objs = []
    # cpu/light.c's shadow rays have no far end, so in a closed room every one of them is blocked: the
    # ceiling (wall 3) is a checkerboard of skylights, which leaves about half of them free
    for k, (o, du, dv, n, m) in enumerate(walls):
        objs += obj(m, lattice(o, du, dv, 8, 8, n, (lambda i, j: (i + j) % 2 == 0) if k == 3 else (lambda i, j: True)))
    objs += obj(mat((0.10, 0.02, 0.10), (0.8, 0.3, 0.8), 0.0), box((R / 4, -R, R / 2), (R / 2, -R / 2, 0.75 * R)))
    # object 7: across the eye plane z = ez and the film plane z = ez - L
    objs += obj(mat((0.12, 0.12, 0.0), (1.0, 1.0, 0.1), 0.0),
                [(((q(0.25 * L), q(ey + 0.05 * L), q(ez - 1.5 * L)), (q(0.35 * L), q(ey + 0.05 * L), q(ez + L)),
                   (q(0.25 * L), q(ey + 0.3 * L), q(ez + L))), (-1, 0, 0))])
    # object 8: wholly between film and eye, inside the converging camera rays
    objs += obj(mat((0.0, 0.12, 0.12), (0.1, 1.0, 1.0), 0.0),
                [(((q(-0.15 * L), q(ey - 0.1 * L), q(ez - 0.5 * L)), (q(-0.05 * L), q(ey - 0.1 * L), q(ez - 0.5 * L)),
                   (q(-0.1 * L), q(ey - 0.02 * L), q(ez - 0.6 * L))), (0, 0, -1))])
    # object 9: wholly behind the film; only reflection and shadow rays get there
    z3 = q(ez - 2 * L)
    objs += obj(mat((0.12, 0.0, 0.0), (1.0, 0.1, 0.1), 0.0),
                [(((-R / 4, ey - R / 8, z3), (R / 4, ey - R / 8, z3), (0.0, ey + R / 4, z3)), (0, 0, 1))])
    return "\n".join([f"camera {w} {h} {num(ex)} {num(ey)} {num(ez)} 1 0 0 0 -1 0 {FOV}", "a_light 0.4 0.4 0.4",
                      "d_light 0.8 0.8 0.7 0.25 -1 0.5",
                      f"p_light 0.7 0.7 0.6 {num(R / 4)} {num(-R / 4)} {num(R / 4)}", ""] + objs), {}


def slivers(w, h):
    L = film_distance(w)
    front = (0, 0, -1)
    zero = [(((-1, 1.5, 0), (-1, 1.5, 0), (1, 1.5, 0)), front),     # a repeated vertex
            (((-1, -1.5, 0), (0, -1.5, 0), (1, -1.5, 0)), front)]   # collinear
    needles = []
    for k in range(2, 21):  # 4 long, 2^-k wide; the wide ones overlap their neighbours in z = 0
        y = -1.0 + 0.125 * (k - 2)
        needles.append((((-2, y, 0), (2, y, 0), (-2, y + 2.0 ** -k, 0)), front))
    # the sweep: right triangles with legs 2^-(k/2+3), k = 6..15, 8 of each, seen at cos ~ 1/8, so that
    # a = e1 . (d x e2) ~ legs^2 / 8 runs from 3e-5 down through cpu/hit.c's 1e-7; each centroid on the
    # camera ray of a sample (ks, ls) of both frame sizes, at z = -1
    sweep = []
    t = 8.0 / L
    up = np.array([0.0, 0.125, math.sqrt(63.0) / 8.0])
    for j in range(80):
        leg = 2.0 ** -((6 + j // 8) / 2.0 + 3.0)
        ks, ls = -6.0 + 0.5 * (j % 24), (1.0, -1.5, 2.5, -3.0)[j // 24]
        cen = np.array([-ks * t, ls * t, -1.0])
        e1, e2 = leg * np.array([1.0, 0.0, 0.0]), leg * up
        a = cen - (e1 + e2) / 3.0
        b, c = (a + e1, a + e2) if j % 2 == 0 else (a + e2, a + e1)  # both signs of a
        sweep.append(((tuple(a), tuple(b), tuple(c)), front))
    ground = [(((-4000, -2, -4000), (4000, -2, -4000), (0, -2, 4000)), (0, 1, 0))]
    back = lattice((-2, -2, 1), (1, 0, 0), (0, 1, 0), 4, 4, front)
    objs = obj(mat((0.10, 0.06, 0.02), (0.9, 0.6, 0.2), 0.0), zero + needles + sweep)
    objs += obj(mat((0.05, 0.08, 0.05), (0.4, 0.7, 0.4), 0.2), ground)
    objs += obj(mat((0.04, 0.04, 0.10), (0.3, 0.3, 0.9), 0.0), back)
    # in memory an object's triangles are in reverse file order (cpu/parse_obj.c pops a stack)
    extra = {"sweep_prims": [0, 80], "needle_prims": [80, 99]}
    return "\n".join([f"camera {w} {h} 0 0 -9 1 0 0 0 -1 0 {FOV}", "a_light 0.3 0.3 0.3",
                      "d_light 1 0.9 0.8 1 -0.25 1", "p_light 0.6 0.6 0.6 4 -1 -6", ""] + objs), extra


SCENES = {"twins": twins, "room": room, "slivers": slivers}


def gz(path, data):
    with open(path, "wb") as raw:
        with gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0) as f:
            f.write(data)


def main():
    import oracle as orc
    import rtgpu
    os.makedirs(OUT, exist_ok=True)
    cases = []
    for name, gen in SCENES.items():
        for w, h in SIZES:
            text, extra = gen(w, h)
            with tempfile.TemporaryDirectory() as td:
                sv = os.path.join(td, f"{name}.svati")
                with open(sv, "w") as f:
                    f.write(text)
                dump, ppm = os.path.join(td, "o.f32"), os.path.join(td, "o.ppm")
                p = subprocess.run(["bash", "-c", f"ulimit -s unlimited && exec {PROBE} {sv} {dump}"],
                                   env=dict(os.environ, RT_PROBE_PPM=ppm), capture_output=True,
                                   text=True, check=True)
                m = re.search(r"closest_hit_queries=(\d+) shadow_queries=(\d+)", p.stderr)
                with open(dump, "rb") as f:
                    assert f.readline() == f"RTF32 {w} {h}\n".encode()
                    data = f.read()
                with open(ppm, "rb") as f:
                    ppm_md5 = hashlib.md5(f.read()).hexdigest()
                s = rtgpu.Scene.load_svati(sv)
            sname, fname = f"{name}_{w}x{h}.svati.gz", f"{name}_{w}x{h}.f32.gz"
            gz(os.path.join(OUT, sname), text.encode())
            gz(os.path.join(OUT, fname), data)
            case = {"scene": name, "width": w, "height": h, "svati": sname, "file": fname,
                    "closest": int(m.group(1)), "shadow": int(m.group(2)),
                    "f32_sha256": hashlib.sha256(data).hexdigest(), "ppm_md5": ppm_md5, **extra}
            gold = np.frombuffer(data, np.float32).reshape(h, w, 3)
            img, cnt = orc.render(s.ptr, w, h, threads=0)
            assert np.array_equal(img.view(np.uint32), gold.view(np.uint32)), "the oracle differs from the reference"
            assert (cnt["closest"], cnt["shadow"]) == (case["closest"], case["shadow"])
            figures = adv.check_conditions(case, s, gold)
            hit = float((gold.reshape(-1, 3) != 0).any(axis=1).mean())
            print(case, {"triangles": s.triangle_count, "lit pixels": round(hit, 3),
                         "octree depth": rtgpu.accel_build_info(s, "octree")["max_depth"], **figures})
            cases.append(case)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_adversarial.py (reference cpu/rt via oracle/_ref/rt_probe)",
                   "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
