"""The next frame's candidate lists built on the context's second stream,
beside the previous frame's shade pass (csrc/rt_overlap.h,
rt_hip_set_overlap_lists): the images, the counters and whatever is read
between two renders are what the same sequence gives with every build on the
caller's stream.

Six frames, each with its own camera (panned the way bench.py's fresh-camera
loop pans them, so a stale list would show), enqueued without a wait in
between; then the same frames again with stats() after each.  The shapes are
the smallest that still have several tile rows, big and small footprints and
a refined entry: golden scenes at 96x54 and the ragged 98x50, spheres 64x64,
both octrees."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_image

pytestmark = pytest.mark.gpu

NFRAMES = 6
STAT_KEYS = ("closest", "shadow", "hits", "cand_entries", "depth_overflow")
CASES = [("spheres", 96, 54), ("car-on-road", 98, 50), ("spheres", 64, 64)]
IDS = [f"{n}_{w}x{h}" for n, w, h in CASES]


@pytest.fixture(scope="module")
def gpu(built):
    import rtgpu
    if rtgpu.device_count() == 0:
        pytest.fail("gpu tests need a gfx950 device")
    return rtgpu


def _scene(gpu, scene_dir, name, W, H):
    s = gpu.Scene.load_svati(f"{scene_dir}/{name}.svati")
    s.set_size(W, H)
    return s


def _frames(gpu, s, centre, n=NFRAMES, pan=2.0):
    """The scene's own frame, then n - 1 more with the eye moved along the
    frame's u by `pan` pixels (at the scene centre's depth) per frame."""
    f0 = s.frame()
    cam0 = gpu.Camera()
    C.pointer(cam0)[0] = s.s.camera
    eye = np.array([cam0.position.x, cam0.position.y, cam0.position.z])
    film = np.linalg.norm(np.array([f0.C.x, f0.C.y, f0.C.z]) - eye)
    depth = max(float(np.linalg.norm(np.array(centre) - eye)), 1e-3)
    u = np.array([f0.u.x, f0.u.y, f0.u.z])
    out = [f0]
    for k in range(1, n):
        cam = gpu.Camera()
        C.pointer(cam)[0] = cam0
        p = eye + u * (pan * depth / film * k)
        cam.position.x, cam.position.y, cam.position.z = float(p[0]), float(p[1]), float(p[2])
        fr = gpu.Frame()
        gpu._check(gpu.lib().rt_frame_from_camera(C.byref(cam), C.byref(fr)), "frame")
        out.append(fr)
    return out


class Run:
    """One context on its own stream; every frame renders into device buffers
    of its own, so nothing has to be waited for between two frames."""

    def __init__(self, gpu, s, accel, overlap, nranks=1, setup=None):
        self.gpu, self.L, self.nranks = gpu, gpu.lib(), nranks
        self.ctx = gpu.Context(s, accel)
        self.ctx.set_overlap_lists(overlap)
        if setup:
            setup(self.ctx)
        self.centre = self.ctx.info()["scene_center"]
        self.bufs = []

    def malloc(self, nbytes):
        d = C.c_void_p()
        assert self.L.rt_hip_malloc(0, nbytes, C.byref(d)) == 0
        self.bufs.append(d)
        return d

    def host(self, d, n, dtype=np.uint32):
        """n words of d (call after something that waits for the stream)."""
        out = np.empty(n, dtype)
        assert self.L.rt_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), d, out.nbytes) == 0
        return out

    def warm(self, frame):
        """The first frame of a size: its hit buffers and list sizes (a build
        with a read-back, on the caller's stream)."""
        per = self.gpu.tile_buffer_floats(frame.width, frame.height, self.nranks)
        tiles = self.malloc(4 * per)
        for r in range(self.nranks):
            for attempt in range(3):
                self.ctx.render(frame, r, self.nranks, tiles.value)
                try:
                    self.ctx.stats()
                    break
                except self.gpu.RtError as e:
                    if e.code != -10 or attempt == 2:
                        raise

    def render(self, frame):
        """Enqueues the frame (every rank in turn) and its assemble; the
        device image, not waited for."""
        per = self.gpu.tile_buffer_floats(frame.width, frame.height, self.nranks)
        tiles = self.malloc(4 * per * self.nranks)
        rgb = self.malloc(12 * frame.width * frame.height)
        for r in range(self.nranks):
            self.ctx.render(frame, r, self.nranks, tiles.value + 4 * per * r)
        self.ctx.assemble(frame, tiles.value, self.nranks, rgb.value)
        return rgb

    def image(self, rgb, frame):
        return self.host(rgb, frame.width * frame.height * 3).reshape(frame.height, frame.width, 3)

    def close(self):
        """Destroys the context (which waits for its work), then the buffers."""
        self.ctx.close()
        for d in self.bufs:
            self.L.rt_hip_free(d)
        self.bufs = []


def _sequence(gpu, s, accel, overlap, between=None, at=3, nranks=1, setup=None, frames_of=None):
    """(images, last stats, frame-check sums, side builds, what `between`
    returned) of the six frames enqueued back to back, `between` run before
    frame `at`."""
    run = Run(gpu, s, accel, overlap, nranks, setup)
    frames = _frames(gpu, s, run.centre)
    if frames_of:
        frames = frames_of(run, frames)
    run.warm(frames[0])
    run.ctx.frame_check()
    b0 = run.ctx.overlap_builds()
    rgbs, extra = [], None
    for k, fr in enumerate(frames):
        if between and k == at:
            extra = between(run, frames, k)
        rgbs.append(run.render(fr))
    check = run.ctx.frame_check()  # (waits for the stream)
    last = run.ctx.stats() if nranks == 1 else None
    imgs = [run.image(rgb, fr) for rgb, fr in zip(rgbs, frames)]
    builds = run.ctx.overlap_builds() - b0
    return run, frames, imgs, last, check, builds, extra


@pytest.mark.parametrize("accel", ["octree", "octree_gpu"])
@pytest.mark.parametrize("scene,W,H", CASES, ids=IDS)
def test_six_panned_frames_equal_the_serial_build(gpu, scene_dir, manifest, scene, W, H, accel):
    s = _scene(gpu, scene_dir, scene, W, H)
    off, frames, img_off, last_off, chk_off, builds_off, _ = _sequence(gpu, s, accel, False)
    on, _, img_on, last_on, chk_on, builds_on, _ = _sequence(gpu, s, accel, True)
    print("side builds", builds_on, builds_off, "frame check", chk_on, chk_off)
    assert builds_off == 0 and builds_on >= 4
    assert chk_on == chk_off and chk_on[0] == 0 and chk_on[1] == NFRAMES
    for k in range(NFRAMES):
        assert np.array_equal(img_on[k], img_off[k]), f"frame {k}"
    for k in range(1, NFRAMES):  # each camera its own image: a stale list would show
        assert not np.array_equal(img_on[k], img_on[0]), f"frame {k} equals frame 0"
    assert {k: last_on[k] for k in STAT_KEYS} == {k: last_off[k] for k in STAT_KEYS}
    gold = [c for c in manifest if c["scene"] == scene and (c["width"], c["height"]) == (W, H)]
    if gold:
        assert np.array_equal(img_on[0], golden_image(gold[0]).view(np.uint32))
        assert (last_on["depth_overflow"], chk_on[0]) == (0, 0)
    # the same frames again, the counters read after each (the builds still
    # go to the side stream: the fork is by events, not by the caller's pace)
    per_on, per_off = [], []
    for run, per in ((on, per_on), (off, per_off)):
        for fr in frames:
            run.render(fr)
            st = run.ctx.stats()
            per.append({k: st[k] for k in STAT_KEYS})
    assert per_on == per_off
    assert per_on[-1] == {k: last_on[k] for k in STAT_KEYS}
    assert on.ctx.overlap_builds() >= 2 * NFRAMES - 2 and off.ctx.overlap_builds() == 0
    on.close()
    off.close()


def _b_stats(run, frames, k):
    st = run.ctx.stats()
    return {key: st[key] for key in STAT_KEYS}


def _b_frame_check(run, frames, k):
    return run.ctx.frame_check()


def _b_relight(run, frames, k):
    fr = frames[k - 1]
    tiles = run.malloc(4 * run.gpu.tile_buffer_floats(fr.width, fr.height, 1))
    rgb = run.malloc(12 * fr.width * fr.height)
    run.ctx.relight(fr, 0, 1, tiles.value)
    run.ctx.assemble(fr, tiles.value, 1, rgb.value)
    return rgb, fr.width * fr.height * 3  # read after the whole sequence


def _b_gbuffer(run, frames, k):
    fr = frames[k - 1]
    words = run.gpu.gbuffer_tile_words(fr.width, fr.height, 1)
    buf = run.malloc(4 * words)
    run.ctx.gbuffer(fr, 0, 1, buf.value)
    return buf, words


def _b_tile_entries(run, frames, k):
    return [int(x) for x in run.ctx.cand_tile_entries(16)]


def _b_light_edit(run, frames, k):
    lights = run.scene.lights()
    rows = [(l.type, l.r * 0.5, l.g, l.b, l.v.x, l.v.y + 0.25, l.v.z) for l in lights]
    run.ctx.set_lights(rows)
    return len(rows)


BETWEEN = {"stats": _b_stats, "frame_check": _b_frame_check, "relight": _b_relight, "gbuffer": _b_gbuffer,
           "tile_entries": _b_tile_entries, "light_edit": _b_light_edit}


@pytest.mark.parametrize("what", sorted(BETWEEN))
def test_a_reader_or_an_edit_between_two_renders(gpu, scene_dir, what):
    """stats(), the frame check, a relight of the last frame, a G-buffer read,
    rt_hip_cand_tile_entries or a light edit between frames 2 and 3."""
    s = _scene(gpu, scene_dir, "spheres", 96, 54)
    setup = (lambda ctx: ctx.set_gbuffer(True)) if what == "gbuffer" else None

    def between(run, frames, k):
        run.scene = s
        return BETWEEN[what](run, frames, k)

    res = {}
    for overlap in (False, True):
        run, frames, imgs, last, chk, builds, extra = _sequence(gpu, s, "octree_gpu", overlap, between, 3,
                                                                setup=setup)
        if isinstance(extra, tuple) and isinstance(extra[0], C.c_void_p):
            extra = run.host(*extra)
        res[overlap] = (imgs, {k: last[k] for k in STAT_KEYS}, chk, extra)
        print(what, "overlap", overlap, "side builds", builds, "frame check", chk)
        assert builds >= 3 if overlap else builds == 0
        run.close()
    (img_off, last_off, chk_off, x_off), (img_on, last_on, chk_on, x_on) = res[False], res[True]
    for k in range(NFRAMES):
        assert np.array_equal(img_on[k], img_off[k]), f"frame {k}"
    assert last_on == last_off and chk_on == chk_off and chk_on[0] == 0
    if isinstance(x_on, np.ndarray):
        assert np.array_equal(x_on, x_off)
        if what == "relight":  # the same lights: frame 2 again
            assert np.array_equal(x_on.reshape(img_on[2].shape), img_on[2])
    else:
        assert x_on == x_off


def test_a_change_of_frame_size_builds_on_the_callers_stream(gpu, scene_dir):
    """Frames 3..5 at 98x50 after 96x54: the first frame of the new size reads
    its sizes back on the caller's stream, the later ones overlap again."""
    s = _scene(gpu, scene_dir, "spheres", 96, 54)
    s2 = _scene(gpu, scene_dir, "spheres", 98, 50)

    def frames_of(run, frames):
        return frames[:3] + _frames(gpu, s2, run.centre)[3:]

    out = {}
    for overlap in (False, True):
        run, frames, imgs, last, chk, builds, _ = _sequence(gpu, s, "octree_gpu", overlap, frames_of=frames_of)
        out[overlap] = (imgs, {k: last[k] for k in STAT_KEYS}, chk)
        print("overlap", overlap, "side builds", builds, "frame check", chk)
        assert 3 <= builds < NFRAMES if overlap else builds == 0
        run.close()
    for k in range(NFRAMES):
        assert np.array_equal(out[True][0][k], out[False][0][k]), f"frame {k}"
    assert out[True][1:] == out[False][1:]
    assert (out[True][0][5].shape[1], out[True][0][5].shape[0]) == (98, 50)


def test_three_ranks_rendered_in_turn_on_one_context(gpu, scene_dir, manifest):
    """Rank after rank of a 3-rank split on one context: every build is
    another rank's than the last (read back, on the caller's stream), with the
    overlap on or off, and the frames are the one-rank frames."""
    s = _scene(gpu, scene_dir, "spheres", 96, 54)
    one = _sequence(gpu, s, "octree_gpu", False)
    imgs = {}
    for overlap in (False, True):
        run, frames, imgs[overlap], _, chk, builds, _ = _sequence(gpu, s, "octree_gpu", overlap, nranks=3)
        print("overlap", overlap, "side builds", builds, "frame check", chk)
        assert chk[0] == 0
        run.close()
    for k in range(NFRAMES):
        assert np.array_equal(imgs[True][k], imgs[False][k]), f"frame {k}"
        assert np.array_equal(imgs[True][k], one[2][k]), f"frame {k} against one rank"
    gold = [c for c in manifest if c["scene"] == "spheres" and (c["width"], c["height"]) == (96, 54)][0]
    assert np.array_equal(imgs[True][0], golden_image(gold).view(np.uint32))
    one[0].close()


def test_a_context_destroyed_right_after_the_last_enqueue(gpu, scene_dir):
    s = _scene(gpu, scene_dir, "spheres", 96, 54)
    ref = _sequence(gpu, s, "octree_gpu", False)
    run = Run(gpu, s, "octree_gpu", True)
    frames = _frames(gpu, s, run.centre)
    run.warm(frames[0])
    rgbs = [run.render(fr) for fr in frames]
    assert run.ctx.overlap_builds() >= 4
    run.ctx.close()  # nothing waited for: the destroy waits for the side stream's build
    for k, (rgb, fr) in enumerate(zip(rgbs, frames)):
        assert np.array_equal(run.image(rgb, fr), ref[2][k]), f"frame {k}"
    run.close()
    ref[0].close()
