"""rtgpu -- Python view of the C ABI in include/rt_scene.h and include/rt_hip.h.

A thin ctypes binding used by bench.py and the tests; the product is the
shared library lib/librtgpu.so (host C + gfx950 HIP kernels).  There is no
Python or CPU fallback: if the library or a gfx950 device is missing every
render call raises RtError.

Mirrors the reference interface for the path: `raytrace(input, output)`
(cpu/headers/raytracer.h:4) is `raytrace()`, the scene model of
cpu/headers/scene.h:7-55 is `Scene` (same C layout), the per-render query
counters are those of SURVEY.md §8d.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.environ.get("RTGPU_LIB") or os.path.join(LIB_DIR, "librtgpu.so")

RT_ACCEL_FLAT = 0
RT_ACCEL_OCTREE = 1
RT_ACCEL_OCTREE_GPU = 2
ACCEL = {"flat": RT_ACCEL_FLAT, "octree": RT_ACCEL_OCTREE, "octree_gpu": RT_ACCEL_OCTREE_GPU}


class RtError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what}: rt error {code}")
        self.code = code


# ---- C layouts (include/rt_scene.h, identical to cpu/headers/scene.h) ----
class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Triangle(C.Structure):
    _fields_ = [("vertex", Vec3 * 3), ("normal", Vec3 * 3)]


class Object(C.Structure):
    _fields_ = [("triangles", C.POINTER(Triangle)), ("triangle_count", C.c_uint),
                ("ka", Vec3), ("kd", Vec3), ("ks", Vec3),
                ("ns", C.c_float), ("ni", C.c_float), ("nr", C.c_float), ("d", C.c_float)]


class Light(C.Structure):
    _fields_ = [("type", C.c_int), ("r", C.c_float), ("g", C.c_float), ("b", C.c_float),
                ("v", Vec3)]


class Camera(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("position", Vec3), ("u", Vec3),
                ("v", Vec3), ("fov", C.c_float)]


class SceneStruct(C.Structure):
    _fields_ = [("objects", C.POINTER(Object)), ("object_count", C.c_size_t),
                ("lights", C.POINTER(Light)), ("light_count", C.c_size_t),
                ("camera", Camera)]


class ProbeResult(C.Structure):
    _fields_ = [("queries", C.c_ulonglong), ("hits", C.c_ulonglong),
                ("node_visits", C.c_ulonglong), ("tri_tests", C.c_ulonglong),
                ("max_stack", C.c_ulonglong), ("mismatches", C.c_ulonglong),
                ("shadow_queries", C.c_ulonglong), ("shadow_hits", C.c_ulonglong),
                ("shadow_node_visits", C.c_ulonglong), ("shadow_tri_tests", C.c_ulonglong)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class Frame(C.Structure):
    _fields_ = [("u", Vec3), ("v", Vec3), ("C", Vec3), ("position", Vec3),
                ("width", C.c_int), ("height", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("closest", C.c_ulonglong), ("shadow", C.c_ulonglong), ("camera", C.c_ulonglong),
                ("node_visits", C.c_ulonglong), ("tri_tests", C.c_ulonglong),
                ("depth_overflow", C.c_ulonglong), ("zero_normal", C.c_ulonglong),
                ("pixels", C.c_ulonglong), ("hits", C.c_ulonglong),
                ("cand_prims", C.c_ulonglong), ("cand_entries", C.c_ulonglong),
                ("cand_global", C.c_ulonglong),
                ("closest_node_lanes", C.c_ulonglong), ("closest_tri_lanes", C.c_ulonglong),
                ("shadow_node_lanes", C.c_ulonglong), ("shadow_tri_lanes", C.c_ulonglong),
                ("cycles_camera", C.c_ulonglong), ("cycles_cand", C.c_ulonglong),
                ("cycles_secondary", C.c_ulonglong), ("cycles_shadow", C.c_ulonglong),
                ("cycles_shadow_directional", C.c_ulonglong), ("stack_spills", C.c_ulonglong),
                ("shadow_zero_risk", C.c_ulonglong), ("hit_records", C.c_ulonglong),
                ("shadow_node_visits", C.c_ulonglong), ("shadow_tri_tests", C.c_ulonglong),
                ("shadow_unproven", C.c_ulonglong), ("shadow_deferred", C.c_ulonglong),
                ("closest_unproven", C.c_ulonglong)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class AccelInfo(C.Structure):
    _fields_ = [("triangles", C.c_ulonglong), ("tri_refs", C.c_ulonglong),
                ("nodes", C.c_ulonglong), ("leaves", C.c_ulonglong), ("max_depth", C.c_ulonglong),
                ("tri_record_bytes", C.c_ulonglong), ("node_record_bytes", C.c_ulonglong),
                ("device_bytes", C.c_ulonglong), ("build_seconds", C.c_double),
                ("max_leaf", C.c_ulonglong), ("shadow_global", C.c_ulonglong),
                ("shadow_mu_max", C.c_double), ("lightbuf_entries", C.c_ulonglong),
                ("lightbuf_global", C.c_ulonglong), ("lightbuf_seconds", C.c_double),
                ("lightbuf_never", C.c_ulonglong), ("lightbuf_band", C.c_ulonglong),
                ("lightbuf_failed", C.c_ulonglong), ("lightbuf_fail_reason", C.c_char * 96),
                ("trace_grid", C.c_int), ("shade_grid", C.c_int),
                ("scene_center", C.c_float * 3), ("scene_radius", C.c_float)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["lightbuf_fail_reason"] = d["lightbuf_fail_reason"].decode(errors="replace")
        d["scene_center"] = list(d["scene_center"])
        return d


# (name, restype, argtypes) for every entry point of include/*.h
_PROTOS = [
    ("rt_strerror", C.c_char_p, [C.c_int]),
    ("rt_last_error", C.c_char_p, []),
    ("rt_scene_load_svati", C.c_int, [C.c_char_p, C.POINTER(C.POINTER(SceneStruct))]),
    ("rt_scene_load_obj", C.c_int, [C.c_char_p, C.POINTER(C.POINTER(SceneStruct))]),
    ("rt_scene_append_obj", C.c_int, [C.POINTER(SceneStruct), C.c_char_p]),
    ("rt_scene_write_svati", C.c_int, [C.POINTER(SceneStruct), C.c_char_p]),
    ("rt_scene_write_obj", C.c_int, [C.POINTER(SceneStruct), C.c_char_p]),
    ("rt_scene_synthetic", C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.c_ulonglong, C.c_int,
                                     C.c_int, C.POINTER(C.POINTER(SceneStruct))]),
    ("rt_scene_synthetic_uv", C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_ulonglong,
                                        C.c_int, C.c_int, C.POINTER(C.POINTER(SceneStruct))]),
    ("rt_scene_triangle_count", C.c_size_t, [C.POINTER(SceneStruct)]),
    ("rt_scene_free", None, [C.POINTER(SceneStruct)]),
    ("rt_ppm_write", C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_void_p]),
    ("rt_png_write_rgba", C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_void_p]),
    ("rt_frame_from_camera", C.c_int, [C.POINTER(Camera), C.POINTER(Frame)]),
    ("rt_accel_build_info", C.c_int, [C.POINTER(SceneStruct), C.c_int, C.POINTER(AccelInfo)]),
    ("rt_accel_validate", C.c_int, [C.POINTER(SceneStruct), C.c_int]),
    ("rt_accel_probe", C.c_int, [C.POINTER(SceneStruct), C.c_int, C.c_int, C.c_int,
                                 C.POINTER(ProbeResult)]),
    ("rt_hip_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("rt_hip_create", C.c_int, [C.c_int, C.POINTER(SceneStruct), C.c_int, C.POINTER(C.c_void_p)]),
    ("rt_hip_accel_info", C.c_int, [C.c_void_p, C.POINTER(AccelInfo)]),
    ("rt_hip_accel_validate", C.c_int, [C.c_void_p]),
    ("rt_flatten_image", C.c_int, [C.POINTER(SceneStruct), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rt_hip_geometry_image", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rt_hip_scene_image", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.POINTER(C.c_size_t)]),
    ("rt_hip_destroy", None, [C.c_void_p]),
    ("rt_hip_tiles_per_rank", C.c_int, [C.c_int, C.c_int, C.c_int]),
    ("rt_hip_tile_buffer_floats", C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    ("rt_tile_map_check", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]),
    ("rt_hip_render", C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int, C.c_int, C.c_void_p,
                                C.c_void_p]),
    ("rt_hip_stats", C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    ("rt_hip_frame_check", C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint),
                                     C.POINTER(C.c_ulonglong)]),
    ("rt_hip_set_count_work", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_hip_set_cull_slack", C.c_int, [C.c_void_p, C.c_float]),
    ("rt_hip_set_camera_slack", C.c_int, [C.c_void_p, C.c_float]),
    ("rt_hip_cand_verify", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ("rt_hip_cand_verify_compat", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rt_hip_cand_tile_entries", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("rt_hip_set_cand_item_cap", C.c_int, [C.c_void_p, C.c_uint]),
    ("rt_hip_set_overlap_lists", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_hip_overlap_builds", C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    ("rt_hip_verify_shadows", C.c_int, [C.c_void_p, C.c_uint, C.POINTER(C.c_ulonglong)]),
    ("rt_hip_verify_shadows_from", C.c_int, [C.c_void_p, C.c_uint, C.c_uint, C.POINTER(C.c_ulonglong)]),
    ("rt_hip_set_exact_camera", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_hip_set_policy", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_hip_set_exact_shadows", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_hip_set_exact_reflections", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_hip_set_light_buffers", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_hip_set_lightbuf_entry_cap", C.c_int, [C.c_void_p, C.c_ulonglong]),
    ("rt_lightbuf_survey", C.c_int, [C.c_void_p, C.c_uint, C.c_int, C.c_uint, C.c_void_p]),
    ("rt_hip_probe_shadows", C.c_int, [C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    ("rt_hip_probe_closest", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                       C.c_void_p]),
    ("rt_hip_tile_cycles", C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_size_t]),
    ("rt_hip_tile_phase_cycles", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong),
                                           C.c_size_t]),
    ("rt_hip_set_timing", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_hip_frame_times", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float),
                                     C.POINTER(C.c_float)]),
    ("rt_hip_frame_kernel_times", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float),
                                            C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("rt_hip_set_camera_bound_scale", C.c_int, [C.c_void_p, C.c_double]),
    ("rt_hip_set_camera_refine", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_cand_refine_sample", C.c_int, [C.POINTER(SceneStruct), C.c_float, C.c_double, C.c_uint, C.c_int,
                                        C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("rt_cand_survey", C.c_int, [C.POINTER(SceneStruct), C.c_float, C.c_double, C.c_int, C.c_int,
                                 C.POINTER(C.c_ulonglong)]),
    ("rt_hip_assemble", C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_void_p, C.c_int, C.c_void_p,
                                  C.c_void_p]),
    ("rt_hip_cand_produce", C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int, C.c_int, C.POINTER(C.c_uint),
                                      C.POINTER(C.c_uint), C.c_void_p]),
    ("rt_hip_cand_exchange_local", C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(Frame)]),
    ("rt_hip_cand_send_buffer", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("rt_hip_cand_consume", C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                      C.c_uint, C.c_void_p]),
    ("rt_hip_render_image", C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_void_p,
                                      C.POINTER(Stats)]),
    ("rt_hip_set_lights", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("rt_hip_set_materials", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("rt_hip_set_keep_visibility", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_hip_set_triangles", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]),
    ("rt_hip_set_triangles_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]),
    ("rt_hip_geometry_updates", C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    ("rt_hip_geometry_times", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("rt_hip_relight", C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("rt_hip_relight_image", C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_void_p, C.POINTER(Stats)]),
    ("rt_hip_set_gbuffer", C.c_int, [C.c_void_p, C.c_int]),
    ("rt_hip_gbuffer_tile_words", C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    ("rt_hip_gbuffer", C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("rt_hip_assemble_gbuffer", C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p]),
    ("rt_hip_render_image_gbuffer", C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_void_p, C.c_void_p,
                                              C.POINTER(Stats)]),
    ("rt_hip_trace_rays", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    ("rt_hip_trace_rays_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p,
                                         C.c_void_p, C.POINTER(Stats)]),
    ("rt_hip_frame_rays", C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rt_hip_frame_rays_host", C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int, C.c_void_p, C.c_void_p]),
    ("rt_hip_occluded", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p,
                                  C.c_void_p]),
    ("rt_hip_occluded_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint,
                                       C.c_void_p, C.POINTER(Stats)]),
    ("rt_hip_ambient_occlusion", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_ulonglong, C.c_uint, C.c_void_p,
                                           C.c_uint, C.c_uint, C.c_float, C.c_uint, C.c_void_p, C.c_void_p]),
    ("rt_hip_ambient_occlusion_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_ulonglong, C.c_uint,
                                                C.c_void_p, C.c_uint, C.c_uint, C.c_float, C.c_uint, C.c_void_p,
                                                C.POINTER(Stats)]),
    ("rt_hip_ao_rays", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_ulonglong, C.c_uint, C.c_void_p, C.c_uint,
                                 C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rt_hip_ao_rays_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_ulonglong, C.c_uint, C.c_void_p,
                                      C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rt_hip_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_ulonglong, C.c_uint, C.c_void_p, C.c_uint,
                                C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]),
    ("rt_hip_gather_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_ulonglong, C.c_uint, C.c_void_p,
                                     C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.POINTER(Stats)]),
    ("rt_hip_path_records", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    ("rt_hip_path_records_host", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    ("rt_hip_direct_light", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    ("rt_hip_direct_light_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_void_p,
                                           C.POINTER(Stats)]),
    ("rt_hip_lightbuf_box", C.c_int, [C.c_void_p, C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_float),
                                      C.POINTER(C.c_float)]),
    ("rt_hip_malloc", C.c_int, [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("rt_hip_free", C.c_int, [C.c_void_p]),
    ("rt_hip_memcpy_d2h", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("rt_hip_memcpy_h2d", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("rt_hip_memcpy_d2d", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("rt_raytrace", C.c_int, [C.c_char_p, C.c_char_p]),
    ("rt_hip_render_compat", C.c_int, [C.c_void_p, C.POINTER(Camera), C.c_void_p,
                                       C.POINTER(Stats)]),
    ("rt_raytrace_gpu", C.c_int, [C.c_char_p, C.c_char_p, C.c_int]),
    ("rt_raytrace_multi", C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(Stats),
                                    C.POINTER(C.c_double)]),
    ("rt_raytrace_multi_dev", C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.c_int,
                                        C.POINTER(Stats), C.POINTER(C.c_double)]),
]

_lib = None


def build():
    """Compile lib/librtgpu.so and lib/rt for gfx950 (make -C raytracing-gpu_amd)."""
    subprocess.run(["make", "-s", "-j8", "-C", HERE], check=True)


def lib():
    """The loaded product library; raises if it was never built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RtError(-6, f"{LIB_PATH} missing: run raytracing-gpu_amd/rtgpu.build() "
                              "(make -C raytracing-gpu_amd)")
        L = C.CDLL(LIB_PATH)
        for name, res, args in _PROTOS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        L = lib()
        raise RtError(rc, f"{what}: {L.rt_strerror(rc).decode()} ({L.rt_last_error().decode()})")


class Scene:
    """Owns an rt_scene* (layout of cpu/headers/scene.h)."""

    def __init__(self, ptr):
        self.ptr = ptr

    @classmethod
    def load_svati(cls, path):
        p = C.POINTER(SceneStruct)()
        _check(lib().rt_scene_load_svati(os.fsencode(path), C.byref(p)), f"load {path}")
        return cls(p)

    @classmethod
    def load_obj(cls, path):
        p = C.POINTER(SceneStruct)()
        _check(lib().rt_scene_load_obj(os.fsencode(path), C.byref(p)), f"load {path}")
        return cls(p)

    @classmethod
    def synthetic(cls, gx=32, gy=32, tris_per_sphere=9766, seed=0x5EED, width=3840, height=2160):
        p = C.POINTER(SceneStruct)()
        _check(lib().rt_scene_synthetic(gx, gy, tris_per_sphere, seed, width, height, C.byref(p)),
               "synthetic scene")
        return cls(p)

    @classmethod
    def synthetic_uv(cls, gx, gy, stacks, slices, seed=0x5EED, width=3840, height=2160):
        """Explicit tessellation (round 1's C5 was 258 stacks x 19 slices)."""
        p = C.POINTER(SceneStruct)()
        _check(lib().rt_scene_synthetic_uv(gx, gy, stacks, slices, seed, width, height,
                                           C.byref(p)), "synthetic scene")
        return cls(p)

    @property
    def s(self):
        return self.ptr.contents

    @property
    def camera(self):
        return self.s.camera

    def set_size(self, width, height):
        """Same effect as rewriting the camera line's width/height."""
        self.s.camera.width = width
        self.s.camera.height = height

    @property
    def triangle_count(self):
        return int(lib().rt_scene_triangle_count(self.ptr))

    def write_svati(self, path):
        _check(lib().rt_scene_write_svati(self.ptr, os.fsencode(path)), f"write {path}")

    def write_obj(self, path):
        _check(lib().rt_scene_write_obj(self.ptr, os.fsencode(path)), f"write {path}")

    def triangles_array(self):
        """All triangles as a (T, 6, 3) float32 array (vertices then normals)."""
        return scene_triangles(self.ptr)

    def set_triangles_array(self, array, first=0):
        """Write an (n, 6, 3) or (n, 18) float32 array (the layout of
        triangles_array()) over the triangles [first, first + n) of the host
        rt_scene, in prim order: the oracle and a fresh Context then see the
        edited scene (Context.set_triangles edits a live context)."""
        a = _triangle_rows(array)
        first = int(first)
        if first < 0 or first + len(a) > self.triangle_count:
            raise IndexError(f"triangles [{first}, {first + len(a)}) of {self.triangle_count}")
        s, base, done = self.s, 0, 0
        for i in range(s.object_count):
            o = s.objects[i]
            n = int(o.triangle_count)
            lo, hi = max(first, base), min(first + len(a), base + n)
            if lo < hi:
                dst = C.addressof(o.triangles.contents) + 72 * (lo - base)
                C.memmove(dst, a[lo - first:hi - first].ctypes.data, 72 * (hi - lo))
                done += hi - lo
            base += n
        assert done == len(a)

    def materials_array(self):
        return scene_materials(self.ptr)

    def lights(self):
        """The scene's own light array as a ctypes (Light * light_count) view:
        edits change the scene (what an oracle given the same rt_scene renders,
        and what Context.set_lights(scene.lights()) uploads)."""
        n = int(self.s.light_count)
        if n == 0:
            return (Light * 0)()
        return (Light * n).from_address(C.addressof(self.s.lights.contents))

    def lightbuf_survey(self, light, exact=False, stride=1):
        """Host-only count of light `light`'s buffer (rt_lightbuf_survey)."""
        out = (C.c_ulonglong * 12)()
        _check(lib().rt_lightbuf_survey(self.ptr, int(light), 1 if exact else 0, int(stride), out),
               "lightbuf_survey")
        keys = ("entries", "never", "global", "band", "big", "surveyed", "band_entries", "max_count",
                "max_prim", "entries_gt1024", "entries_65_1024", "prims_gt64")
        return dict(zip(keys, (int(x) for x in out)))

    def frame(self):
        f = Frame()
        cam = Camera()
        C.pointer(cam)[0] = self.s.camera
        _check(lib().rt_frame_from_camera(C.byref(cam), C.byref(f)), "frame")
        return f

    def close(self):
        if self.ptr:
            lib().rt_scene_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _as_scene_ptr(ptr):
    if isinstance(ptr, C.c_void_p):
        return C.cast(ptr, C.POINTER(SceneStruct))
    return ptr


def scene_triangles(ptr):
    """Triangles of any scene with the cpu/headers/scene.h layout (product or
    oracle), as a (T, 6, 3) float32 array: 3 vertices then 3 normals."""
    s = _as_scene_ptr(ptr).contents
    out = []
    for i in range(s.object_count):
        o = s.objects[i]
        n = o.triangle_count
        if n:
            buf = (C.c_float * (18 * n)).from_address(C.addressof(o.triangles.contents))
            out.append(np.frombuffer(buf, dtype=np.float32).reshape(n, 6, 3).copy())
    return np.concatenate(out) if out else np.zeros((0, 6, 3), np.float32)


def _triangle_rows(array):
    """(n, 18) contiguous float32 rows of an (n, 6, 3) or (n, 18) array."""
    a = np.ascontiguousarray(array, dtype=np.float32)
    if a.ndim == 3 and a.shape[1:] == (6, 3):
        a = a.reshape(len(a), 18)
    if a.ndim != 2 or a.shape[1] != 18:
        raise ValueError(f"triangles are (n, 6, 3) or (n, 18) float32, not {a.shape}")
    return a


# ---- moving geometry (include/rt_hip.h rt_hip_set_triangles) ----
def object_range(scene, k):
    """(first, count) of object k's triangles in prim order (object, then the
    object's triangle index): the range rt_hip_set_triangles takes."""
    s = _as_scene_ptr(scene.ptr if isinstance(scene, Scene) else scene).contents
    if not 0 <= int(k) < s.object_count:
        raise IndexError(f"object {k} of {s.object_count}")
    first = sum(int(s.objects[i].triangle_count) for i in range(int(k)))
    return first, int(s.objects[int(k)].triangle_count)


def vertex_extent(tris):
    """The float32 largest side of the vertex box of (n, 6, 3) triangles."""
    v = np.asarray(tris, np.float32).reshape(-1, 6, 3)[:, :3].reshape(-1, 3)
    return np.float32((v.max(axis=0) - v.min(axis=0)).max())


def shift_triangles(tris, delta):
    """Every vertex plus float32 `delta` (3 values), in float32; normals stay.
    -> a new (n, 6, 3) float32 array."""
    t = np.array(tris, np.float32).reshape(-1, 6, 3)
    t[:, :3] = t[:, :3] + np.asarray(delta, np.float32)
    return t


def _rot_y(v, c, s):
    """v @ R.T for R = [[c, 0, s], [0, 1, 0], [-s, 0, c]] in float32, each
    component the products summed left to right (x R_i0 + y R_i1) + z R_i2."""
    f32 = np.float32
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([(x * c + y * f32(0)) + z * s, (x * f32(0) + y * f32(1)) + z * f32(0),
                     (x * -s + y * f32(0)) + z * c], axis=-1).astype(f32)


def spin_triangles(tris, angle=0.3):
    """The triangles turned by `angle` about the y axis through the float32
    mean m of their vertices (the vertex rows summed in order, in float32,
    divided by their count): vertices become (v - m) @ R.T + m, normals n @ R.T,
    R = [[c, 0, s], [0, 1, 0], [-s, 0, c]], c, s = float32(cos angle),
    float32(sin angle); float32 throughout.  -> a new (n, 6, 3) float32 array."""
    f32 = np.float32
    t = np.array(tris, f32).reshape(-1, 6, 3)
    c, s = f32(np.cos(angle)), f32(np.sin(angle))
    v = t[:, :3].reshape(-1, 3)
    m = (np.cumsum(v, axis=0, dtype=f32)[-1] / f32(len(v))).astype(f32) if len(v) else np.zeros(3, f32)
    t[:, :3] = _rot_y(t[:, :3] - m, c, s) + m
    t[:, 3:] = _rot_y(t[:, 3:], c, s)
    return t


def scale_triangles(tris, factors=(1.0625, 0.9375, 1.125)):
    """Every vertex times float32 `factors` (per axis), in float32; normals
    stay.  -> a new (n, 6, 3) float32 array."""
    t = np.array(tris, np.float32).reshape(-1, 6, 3)
    t[:, :3] = t[:, :3] * np.asarray(factors, np.float32)
    return t


def scene_materials(ptr):
    """(objects, 13) float32: ka kd ks ns ni nr d per object."""
    s = _as_scene_ptr(ptr).contents
    rows = []
    for i in range(s.object_count):
        o = s.objects[i]
        rows.append([o.ka.x, o.ka.y, o.ka.z, o.kd.x, o.kd.y, o.kd.z, o.ks.x, o.ks.y, o.ks.z,
                     o.ns, o.ni, o.nr, o.d])
    return np.array(rows, np.float32).reshape(-1, 13)


def _geometry_buffers(n):
    """(records (n, 12), normal rows (n, 9), vertex boxes (n, 6), scene box (6,)) float32, to be filled."""
    return [np.zeros(shape, np.float32) for shape in ((n, 12), (n, 9), (n, 6), (6,))]


def flatten_arrays(scene):
    """What the host flatten derives from the scene's triangles, in prim order
    (rt_flatten_image, no device): the records (T, 12) -- v0, e1, e2, then the
    prim, object and flag words as float32 bit patterns --, the normalised
    normal rows (T, 9), the vertex boxes (T, 6) and the scene box (6,)."""
    out = _geometry_buffers(scene.triangle_count)
    _check(lib().rt_flatten_image(scene.ptr, *(a.ctypes.data_as(C.c_void_p) for a in out)), "rt_flatten_image")
    return tuple(out)


def accel_build_info(scene, accel="octree"):
    i = AccelInfo()
    a = ACCEL[accel] if isinstance(accel, str) else accel
    _check(lib().rt_accel_build_info(scene.ptr, a, C.byref(i)), "accel_build_info")
    return i.as_dict()


def accel_validate(scene, accel="octree"):
    a = ACCEL[accel] if isinstance(accel, str) else accel
    _check(lib().rt_accel_validate(scene.ptr, a), "accel_validate")


def accel_probe(scene, accel="octree", stride=97, check=True):
    r = ProbeResult()
    a = ACCEL[accel] if isinstance(accel, str) else accel
    _check(lib().rt_accel_probe(scene.ptr, a, stride, 1 if check else 0, C.byref(r)), "probe")
    return r.as_dict()


def cand_survey(scene, eps_ulps=64.0, bound_scale=1.0, threads=8, leaves=False):
    """Host-only: {safe, footprint, global, entries} of the camera candidate
    lists of the scene's frame (csrc/rt_cand_geom.h classify + raster, run by csrc/rt_cand_host.cpp)."""
    out = (C.c_ulonglong * 88)()
    _check(lib().rt_cand_survey(scene.ptr, eps_ulps, bound_scale, threads, 1 if leaves else 0, out),
           "cand_survey")
    r = dict(zip(("safe", "footprint", "global", "entries"), (int(x) for x in out[:4])))
    # the entries the device lists hold with the per-tile refinement (big
    # footprints refined, csrc/rt_cand_geom.h tile_keep); the big footprints'
    # entries before and after it
    r["refined"] = int(out[68])
    r["big_entries"], r["big_kept"] = int(out[69]), int(out[70])
    # the float fast path (quick_class) and what the f64 classification makes
    # of the prims it lists
    r["quick"] = dict(zip(("listed", "listed_safe_leaf", "listed_safe_other", "listed_no_tiles",
                           "listed_global", "safe", "away", "listed_safe_reach", "listed_safe_steep",
                           "safe_violations"), (int(x) for x in out[71:81])))
    r["hist"] = [(1 << k, int(out[4 + k]), int(out[20 + k])) for k in range(16) if out[4 + k]]
    # footprint prims by how far their T_D box reaches beyond the triangle, in
    # units of the walk's slack: (lower edge 2^(k-8), prims, entries)
    r["growth_hist"] = [(2.0 ** (k - 8) if k else 0.0, int(out[36 + k]), int(out[52 + k]))
                        for k in range(16) if out[36 + k]]
    return r


def cand_refine_sample(scene, stride=1, cap=1 << 20, eps_ulps=64.0, bound_scale=1.0, compat=False):
    """Host-only: every stride-th entry of the refined candidate footprints
    as rows (prim, tile x, tile y, kept) -- csrc/rt_cand_geom.h tile_keep -- and
    the number sampled (compat: the gpu/rt mode's 3x frame)."""
    import numpy as np
    out = np.zeros((cap, 4), np.uint32)
    n, total = C.c_size_t(0), C.c_size_t(0)
    _check(lib().rt_cand_refine_sample(scene.ptr, eps_ulps, bound_scale, stride, 1 if compat else 0,
                                       out.ctypes.data, cap, C.byref(n), C.byref(total)), "cand_refine_sample")
    return out[:n.value], total.value


def device_count():
    n = C.c_int(0)
    rc = lib().rt_hip_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def tiles_per_rank(width, height, nranks):
    return int(lib().rt_hip_tiles_per_rank(width, height, nranks))


def tile_buffer_floats(width, height, nranks):
    return int(lib().rt_hip_tile_buffer_floats(width, height, nranks))


# ---- per-sample G-buffer (include/rt_hip.h rt_gsample) ----
GB_WORDS = 10
GSAMPLE = np.dtype([("prim", np.int32), ("obj", np.int32), ("queries", np.int32), ("dist", np.float32),
                    ("P", np.float32, 3), ("N", np.float32, 3)])
assert GSAMPLE.itemsize == 4 * GB_WORDS


def gbuffer_tile_words(width, height, nranks):
    """32-bit words of one rank's G-buffer tile buffer (rt_hip_gbuffer_tile_words)."""
    return int(lib().rt_hip_gbuffer_tile_words(width, height, nranks))


def prim_object_triangle(scene, prim):
    """(object index, index into that object's triangle array) of the global
    triangle index `prim` of a G-buffer sample (objects in file order, each
    object's triangles in array order); prim = -1 (miss) gives (-1, -1)."""
    prim = int(prim)
    if prim < 0:
        return -1, -1
    s = _as_scene_ptr(scene.ptr if isinstance(scene, Scene) else scene).contents
    base = 0
    for i in range(s.object_count):
        n = int(s.objects[i].triangle_count)
        if prim < base + n:
            return i, prim - base
        base += n
    raise IndexError(f"prim {prim} of {base} triangles")


def coverage(samples):
    """(H, W) float32 alpha in {0, 1/4, 1/2, 3/4, 1}: the share of each pixel's
    four samples whose camera ray hit geometry."""
    return ((samples["prim"] >= 0).sum(axis=-1) * 0.25).astype(np.float32)


# ---- ray batches (include/rt_hip.h rt_hip_trace_rays, rt_hip_frame_rays) ----
RT_RAYS_PACKET = 1
RAY_ORDER = {"pixel": 0, "quarter": 1}


def quarter_order(width, height):
    """(perm, inv) of rt_hip_frame_rays' quarter order (csrc/rt_ray_items.h
    rt_quarter_order_ray): perm[k] = the pixel-order index 4 (row W + col) + s
    of quarter-order ray k, inv its inverse.  Each aligned 64 rays are one
    4x4-pixel quarter (quarters in scanline order), lane = 4 (4 r + c) + s
    (csrc/rt_tiles.h rt_item_pixel).  width, height: multiples of 4."""
    if width <= 0 or height <= 0 or width % 4 or height % 4:
        raise ValueError(f"quarter order needs multiples of 4, not {width}x{height}")
    k = np.arange(4 * width * height, dtype=np.int64)
    quarter, lane = k // 64, k % 64
    px, smp = lane >> 2, lane & 3
    row = 4 * (quarter // (width // 4)) + (px >> 2)
    col = 4 * (quarter % (width // 4)) + (px & 3)
    perm = 4 * (row * width + col) + smp
    inv = np.empty_like(perm)
    inv[perm] = k
    return perm, inv


def camera_rays(frame, order="pixel"):
    """The 4 W H camera rays of `frame` as (origins, dirs), (n, 3) float32 each,
    bit for bit what rt_hip_frame_rays writes: the float arithmetic of
    cpu/raytracer.c:55-60 (csrc/rt_render.hip camera_ray) -- sample s of PPM
    pixel (row, col) has k = i + 0.5 (s >> 1), l = j + 0.5 (s & 1) with
    i = W - col - W/2, j = H - row - H/2, its origin (C + u k) + v l on the
    film and its direction normalize(position - origin).  order: "pixel" (ray
    4 (row W + col) + s) or "quarter" (quarter_order)."""
    W, H = int(frame.width), int(frame.height)
    f32 = np.float32
    idx = np.arange(4 * W * H, dtype=np.int64)
    if RAY_ORDER[order] if isinstance(order, str) else order:
        idx = quarter_order(W, H)[0]
    px, smp = idx >> 2, idx & 3
    row, col = px // W, px % W
    k = (W - col - W // 2).astype(f32) + f32(0.5) * (smp >> 1).astype(f32)
    l = (H - row - H // 2).astype(f32) + f32(0.5) * (smp & 1).astype(f32)

    def v3(v):
        return [f32(v.x), f32(v.y), f32(v.z)]
    u, v, c, pos = v3(frame.u), v3(frame.v), v3(frame.C), v3(frame.position)
    o = [(c[a] + k * u[a]) + l * v[a] for a in range(3)]
    d = [pos[a] - o[a] for a in range(3)]
    s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]  # float sum, f64 sqrt rounded to float (vector3_length)
    ln = np.sqrt(s.astype(np.float64)).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = [x / ln for x in d]
    return np.stack(o, axis=1).astype(f32), np.stack(d, axis=1).astype(f32)


def fold_samples(rgb):
    """Pixels from sample colours: every 4 consecutive rows of rgb ((4 n, 3)
    float32, a pixel's samples in cpu order) give acc = color_add(acc,
    color_mul(s, 0.25)) from acc = 0 (cpu/raytracer.c:55-68, cpu/colors.c) in
    float32 -> (n, 3)."""
    f32 = np.float32
    s = np.ascontiguousarray(rgb, dtype=f32).reshape(-1, 4, 3)
    acc = np.zeros((len(s), 3), f32)
    for j in range(4):
        y = (s[:, j] / f32(255.0) * f32(0.25)) * f32(255.0)  # color_mul -> init_color
        y = np.where(y > f32(255.0), f32(255.0), y)
        y = np.where(y < f32(0.0), f32(0.0), y)
        acc = acc + y  # color_add
        acc = np.where(acc > f32(255.0), f32(255.0), acc)
    return acc.astype(f32)


def equirect_rays(position, width, height):
    """An equirectangular panorama's rays from `position`: pixel (row, col)
    looks along longitude 2 pi (col + 0.5) / width - pi (0 = +x, towards +z)
    and latitude pi / 2 - pi (row + 0.5) / height (+y up), unit directions.
    Host numpy only -> (origins, dirs), (width * height, 3) float32 each, row-major."""
    rows, cols = np.mgrid[0:height, 0:width]
    lon = 2.0 * np.pi * (cols + 0.5) / width - np.pi
    lat = 0.5 * np.pi - np.pi * (rows + 0.5) / height
    d = np.stack([np.cos(lat) * np.cos(lon), np.sin(lat), np.cos(lat) * np.sin(lon)], axis=-1)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3).astype(np.float32)
    o = np.broadcast_to(np.asarray(position, np.float32), d.shape).copy()
    return o, d


def ortho_rays(position, u, v, extent, width, height):
    """An orthographic view's rays: a width x height grid of parallel rays
    along normalize(u x v), their origins on the plane through `position`
    spanned by the unit vectors of u (to the right) and v (up), the grid
    `extent` wide and extent * height / width high, pixel centres, row 0 on
    top.  Host numpy only -> (origins, dirs), (width * height, 3) float32 each."""
    u = np.asarray(u, np.float64) / np.linalg.norm(u)
    v = np.asarray(v, np.float64) / np.linalg.norm(v)
    w = np.cross(u, v)
    w /= np.linalg.norm(w)
    rows, cols = np.mgrid[0:height, 0:width]
    x = ((cols + 0.5) / width - 0.5) * extent
    y = (0.5 - (rows + 0.5) / height) * extent * height / width
    o = np.asarray(position, np.float64) + x[..., None] * u + y[..., None] * v
    o = o.reshape(-1, 3).astype(np.float32)
    d = np.broadcast_to(w.astype(np.float32), o.shape).copy()
    return o, d


def hemisphere_rays(P, N, k, seed):
    """Ambient-occlusion rays from a G-buffer: k cosine-weighted directions
    about the normal of every surface point, origins at the points.  P, N:
    (m, 3) points and normals (any length; a zero normal gets +z).  Host numpy
    only, seeded -> (origins, dirs), (m k, 3) float32 each, a point's k rays
    consecutive; the directions have unit length and dot(dir, N) > 0."""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    n = np.ascontiguousarray(N, dtype=np.float64).reshape(-1, 3).copy()
    assert len(P) == len(n) and k >= 1
    ln = np.linalg.norm(n, axis=1)
    n[ln == 0] = (0.0, 0.0, 1.0)
    n /= np.where(ln == 0, 1.0, ln)[:, None]
    # an orthonormal frame (t, b, n): t from the axis n leans on least
    ax = np.eye(3)[np.argmin(np.abs(n), axis=1)]
    t = np.cross(ax, n)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    rng = np.random.default_rng(seed)
    # cosine-weighted: a uniform point of the unit disc, lifted; the radius is
    # kept off 1 so that the lifted direction stays clear of the tangent plane
    r = np.sqrt(rng.random((len(P), k))) * 0.999
    phi = 2.0 * np.pi * rng.random((len(P), k))
    x, y = r * np.cos(phi), r * np.sin(phi)
    z = np.sqrt(1.0 - r * r)
    d = x[..., None] * t[:, None] + y[..., None] * b[:, None] + z[..., None] * n[:, None]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.repeat(P, k, axis=0)
    return o.astype(np.float32), d.reshape(-1, 3).astype(np.float32)


AO_KMAX = 1024  # RT_AO_KMAX


def ao_table(m, seed):
    """m local directions for Context.ambient_occlusion: cosine-weighted about
    +z, unit length, z > 0 (the radius is kept off 1, as hemisphere_rays does)
    -> (m, 3) float32, seeded."""
    rng = np.random.default_rng(seed)
    r = np.sqrt(rng.random(m)) * 0.999
    phi = 2.0 * np.pi * rng.random(m)
    t = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - r * r)], axis=1)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    return t.astype(np.float32)


def _ao_mix32(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def ao_hash(n, seed, base=0):
    """The hash of samples base .. base + n - 1 (csrc/rt_ao_items.h rt_ao_hash) -> uint32 (n,)."""
    g = np.uint64(base) + np.arange(n, dtype=np.uint64)
    lo, hi = (g & np.uint64(0xffffffff)).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32)
    return _ao_mix32(lo ^ _ao_mix32(hi + np.uint32(seed & 0xffffffff)))


def ao_rays_host(samples, k, table, seed, base=0):
    """The numpy float32 twin of csrc/rt_ao_items.h: the k rays of every
    GSAMPLE record, bit for bit what the device generates (every step one
    correctly rounded float32 operation in the header's order) -> (origins,
    dirs) (n k, 3) float32 in ray order i k + r, zeros for a record that does
    not shoot, and the shot mask, bool (n,)."""
    smp = np.ascontiguousarray(samples, dtype=GSAMPLE).reshape(-1)
    tab = np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 3)
    n, m = len(smp), len(tab)
    assert 1 <= k <= AO_KMAX and m >= 1
    f = np.float32
    N, P = smp["N"].astype(f), smp["P"].astype(f)
    with np.errstate(all="ignore"):
        s = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
        l = np.sqrt(s.astype(np.float64)).astype(f)
        shot = (smp["prim"] >= 0) & (l > 0) & (l < np.inf)
        nx, ny, nz = N[:, 0] / l, N[:, 1] / l, N[:, 2] / l
        sg = np.copysign(f(1), nz)
        a = f(-1) / (sg + nz)
        b = nx * ny * a
        T = np.stack([f(1) + sg * nx * nx * a, sg * b, -sg * nx], axis=1)
        B = np.stack([b, sg + ny * ny * a, -ny], axis=1)
        nn = np.stack([nx, ny, nz], axis=1)
        h = ao_hash(n, seed, base)
        rows = ((h >> np.uint32(3)) % np.uint32(m))[:, None].astype(np.uint64) + np.arange(k, dtype=np.uint64)[None, :]
        row = tab[(rows % np.uint64(m)).astype(np.int64)]  # (n, k, 3)
        swap = ((h & np.uint32(1)) != 0)[:, None]
        x = np.where(swap, row[..., 1], row[..., 0])
        y = np.where(swap, row[..., 0], row[..., 1])
        x = np.where(((h & np.uint32(2)) != 0)[:, None], -x, x)
        y = np.where(((h & np.uint32(4)) != 0)[:, None], -y, y)
        z = row[..., 2]
        d = (x[..., None] * T[:, None, :] + y[..., None] * B[:, None, :]) + z[..., None] * nn[:, None, :]
    d = np.where(shot[:, None, None], d, f(0)).astype(f)
    o = np.where(shot[:, None, None], np.broadcast_to(P[:, None, :], d.shape), f(0)).astype(f)
    return o.reshape(-1, 3), d.reshape(-1, 3), shot


def ao_open_share(counts, samples, k):
    """The unoccluded share per sample from Context.ambient_occlusion's
    counts: 1 - count / k; a sample that did not shoot counts as open."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1)
    assert len(c) == len(np.asarray(samples).reshape(-1)) and k >= 1
    return 1.0 - c / float(k)


def gather_sum(colours, k):
    """The numpy float32 twin of a gather's accumulation (include/rt_hip.h
    rt_hip_gather): the colours of n k rays, (n k, 3) in ray order i k + r ->
    (n, 3) float32, acc = color_add(acc, colour) from (+0, +0, +0) over r = 0 ..
    k - 1: one float32 add per channel per ray, then the reference's clamp `if
    (x > 255) x = 255` (cpu/colors.c), sequentially in ray order -- no pairwise or
    tree sum, no division by k, no weight."""
    f = np.float32
    c = np.ascontiguousarray(colours, dtype=f).reshape(-1, 3)
    k = int(k)
    assert k >= 1 and len(c) % k == 0
    c = c.reshape(-1, k, 3)
    acc = np.zeros((len(c), 3), f)
    with np.errstate(all="ignore"):
        for r in range(k):
            acc = (acc + c[:, r, :]).astype(f)
            acc = np.where(acc > f(255), f(255), acc)
    return acc


# ---- a ray batch's paths (include/rt_hip.h rt_hip_path_records) ----
RT_PATH_PRIM = 0x7fffffff


def _color_add(acc, c):
    """color_add of cpu/colors.c in float32: one add per channel, then `if (x >
    255) x = 255` (a NaN passes the compare)."""
    f = np.float32
    acc = (acc + c).astype(f)
    return np.where(acc > f(255), f(255), acc)


def path_fold(offsets, terms):
    """The numpy float32 twin of a ray batch's fold over exported paths
    (Context.path_records): offsets (n + 1,), terms (total, 3) -> (n, 3)
    float32, per ray acc = color_add(acc, term_v) from (+0, +0, +0) over its
    vertices deepest first (v = len - 1 .. 0), as cpu/raytracer.c:29-30 sums
    from the deepest call outwards.  An empty path gives +0 +0 +0."""
    f = np.float32
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    t = np.ascontiguousarray(terms, dtype=f).reshape(-1, 3)
    n = len(off) - 1
    assert n >= 0 and (n == 0 or (np.diff(off) >= 0).all()) and off[0] == 0 and off[-1] <= len(t)
    ln = np.diff(off)
    acc = np.zeros((n, 3), f)
    with np.errstate(all="ignore"):
        for d in range(int(ln.max()) if n else 0):
            on = np.nonzero(ln > d)[0]
            acc[on] = _color_add(acc[on], t[off[on + 1] - 1 - d])
    return acc


def color_mul(c, coef):
    """color_mul of cpu/colors.c in float32: init_color(c / 255 * coef) per
    channel -- the quotient, the product, times 255, then `if (y > 255) y =
    255; if (y < 0) y = 0` (a NaN and -0.0 pass both compares).  c (n, 3),
    coef scalar or (n,) -> (n, 3) float32."""
    f = np.float32
    c = np.ascontiguousarray(c, dtype=f).reshape(-1, 3)
    k = np.broadcast_to(np.asarray(coef, dtype=f).reshape(-1, 1), (len(c), 1))
    with np.errstate(all="ignore"):
        y = (((c / f(255)).astype(f) * k).astype(f) * f(255)).astype(f)
        y = np.where(y > f(255), f(255), y)
        y = np.where(y < f(0), f(0), y)
    return y.astype(f)


def bounce_dir(d, N):
    """ray_bounce of cpu/ray.c:16-25 in float32, in the device's operation
    order (csrc/rt_device.h bounce_dir): d - N * (2 * ((N.x d.x + N.y d.y) + N.z
    d.z)), N used as given.  (n, 3), (n, 3) -> (n, 3) float32."""
    f = np.float32
    d = np.ascontiguousarray(d, dtype=f).reshape(-1, 3)
    N = np.ascontiguousarray(N, dtype=f).reshape(-1, 3)
    with np.errstate(all="ignore"):
        p = (N * d).astype(f)
        dot = ((p[:, 0] + p[:, 1]).astype(f) + p[:, 2]).astype(f)
        s = (f(2) * dot).astype(f)
        return (d - (s[:, None] * N).astype(f)).astype(f)


def path_coefs(offsets, records, nr):
    """The coefficients of exported paths from their records alone: coef_0 = 1,
    coef_{v+1} = nr[obj_v] * coef_v in float32 (cpu/raytracer.c:29), nr = the
    objects' reflection coefficients (Scene.materials_array()[:, 11]) ->
    float32 (total,)."""
    f = np.float32
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    r = np.ascontiguousarray(records, dtype=GSAMPLE).reshape(-1)
    nr = np.asarray(nr, dtype=f).reshape(-1)
    ln = np.diff(off)
    out = np.zeros(len(r), f)
    with np.errstate(all="ignore"):
        for v in range(int(ln.max()) if len(ln) else 0):
            j = off[:-1][ln > v] + v
            out[j] = f(1) if v == 0 else (nr[r["obj"][j - 1]] * out[j - 1]).astype(f)
    return out


# ---- direct light for caller's records (include/rt_hip.h rt_hip_direct_light) ----
def records_from_points(P, N, obj, prim=0):
    """GSAMPLE records for Context.direct_light from caller points: (n, 3)
    positions and normals (used as given, not normalised), an object index
    (scalar or (n,): whose material shades the point) and a prim (>= 0: a hit;
    the direct light reads only its sign).  queries = 0, dist = 0."""
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
    N = np.ascontiguousarray(N, dtype=np.float32).reshape(-1, 3)
    assert len(P) == len(N)
    r = np.zeros(len(P), GSAMPLE)
    r["P"], r["N"] = P, N
    r["obj"] = np.broadcast_to(np.asarray(obj, dtype=np.int32), (len(P),))
    r["prim"] = np.broadcast_to(np.asarray(prim, dtype=np.int32), (len(P),))
    return r


def direct_light_shades(records, nobjects):
    """Which GSAMPLE records Context.direct_light shades (csrc/rt_dlight_items.h
    rt_dl_shades): a hit (prim >= 0) of an object 0 <= obj < nobjects whose P
    and N are finite and whose N is not zero by vector3_is_zero (-0.0 is zero,
    a denormal is not) -> bool (n,).  Every other record gets 0 0 0 and mask 0."""
    r = np.ascontiguousarray(records, dtype=GSAMPLE).reshape(-1)
    pb, nb = r["P"].view(np.uint32), r["N"].view(np.uint32)
    fin = ((pb & 0x7f800000) != 0x7f800000).all(axis=1) & ((nb & 0x7f800000) != 0x7f800000).all(axis=1)
    zero = ((nb[:, 0] | nb[:, 1] | nb[:, 2]) & 0x7fffffff) == 0
    return (r["prim"] >= 0) & (r["obj"] >= 0) & (r["obj"] < int(nobjects)) & fin & ~zero


def _light_rows(lights):
    """(type, (x, y, z) float32) per light of a ctypes Light array or a
    sequence of (type, r, g, b, x, y, z)."""
    rows = []
    for l in lights:
        if isinstance(l, Light):
            rows.append((int(l.type), np.array([l.v.x, l.v.y, l.v.z], np.float32)))
        else:
            rows.append((int(l[0]), np.array(l[4:7], np.float32)))
    return rows


def shadow_rays_host(records, lights):
    """The shadow rays Context.direct_light decides, in float32 numpy: per
    casting light (type 1 directional, 2 point) of `lights`, in their order
    (casting_lights gives their indices), a tuple (origins, dirs) of (n, 3)
    float32 arrays in the operation order of cpu/light.c:53,78 -- origin P, direction
    vector3_scale(l.v, -1) for a directional light, vector3_sub(l.v, P) for a
    point light; neither is normalised."""
    r = np.ascontiguousarray(records, dtype=GSAMPLE).reshape(-1)
    P = np.ascontiguousarray(r["P"], dtype=np.float32)
    out = []
    for t, v in _light_rows(lights):
        if t == 1:
            d = np.broadcast_to(v * np.float32(-1.0), P.shape).astype(np.float32)
        elif t == 2:
            with np.errstate(all="ignore"):
                d = (v[None, :] - P).astype(np.float32)
        else:
            continue
        out.append((P.copy(), np.ascontiguousarray(d)))
    return out


def casting_lights(lights):
    """Indices of the lights that cast a shadow ray (directional and point)."""
    return [li for li, (t, _) in enumerate(_light_rows(lights)) if t in (1, 2)]


class Context:
    """One device image of a scene (rt_hip_create); renders through the C ABI."""

    RT_EINEXACT = -11
    _batch_n = _batch_records = 0  # the last trace_rays with colours: its rays and rt_stats.hit_records

    def __init__(self, scene: Scene, accel="octree", device=0):
        self.device = device
        self.accel = ACCEL[accel] if isinstance(accel, str) else accel
        self.inexact = False  # a parity-breaking tuning knob was set (A/B runs)
        h = C.c_void_p()
        _check(lib().rt_hip_create(device, scene.ptr, self.accel, C.byref(h)), "rt_hip_create")
        self.h = h

    def _check_render(self, rc, what):
        """RT_EINEXACT is expected after a parity-breaking knob was set."""
        if rc == self.RT_EINEXACT and self.inexact:
            return
        _check(rc, what)

    def info(self):
        i = AccelInfo()
        _check(lib().rt_hip_accel_info(self.h, C.byref(i)), "accel_info")
        return i.as_dict()

    def validate(self):
        """Invariants of the device scene image (rt_hip_accel_validate)."""
        _check(lib().rt_hip_accel_validate(self.h), "accel_validate")

    def geometry_arrays(self, boxes=True):
        """The context's own records, normal rows, vertex boxes and scene box
        as they stand on the device, in flatten_arrays' layout
        (rt_hip_geometry_image).  boxes=False: None for the vertex boxes (a
        host-tree context keeps none)."""
        out = _geometry_buffers(int(self.info()["triangles"]))
        ptr = [a.ctypes.data_as(C.c_void_p) for a in out]
        if not boxes:
            ptr[2], out[2] = None, None
        _check(lib().rt_hip_geometry_image(self.h, *ptr), "rt_hip_geometry_image")
        return tuple(out)

    def scene_image(self):
        """(triangle records (nrec, 12), nodes (nodes, 8)) of the scene image
        the kernels walk, as uint32 words (rt_hip_scene_image): leaf-order
        records and the octree's nodes, or the prim-order records and no node
        on a flat context."""
        need = (C.c_size_t * 2)()
        _check(lib().rt_hip_scene_image(self.h, None, 0, None, 0, need), "rt_hip_scene_image")
        tri, node = np.zeros(int(need[0]), np.uint32), np.zeros(int(need[1]), np.uint32)
        _check(lib().rt_hip_scene_image(self.h, tri.ctypes.data_as(C.c_void_p) if tri.size else None, tri.size,
                                        node.ctypes.data_as(C.c_void_p) if node.size else None, node.size, need),
               "rt_hip_scene_image")
        return tri.reshape(-1, 12), node.reshape(-1, 8)

    def set_count_work(self, on=True):
        _check(lib().rt_hip_set_count_work(self.h, 1 if on else 0), "count_work")

    def set_exact_camera(self, on=True):
        _check(lib().rt_hip_set_exact_camera(self.h, 1 if on else 0), "exact_camera")
        if not on:
            self.inexact = True

    def set_timing(self, on=True):
        """HIP events around the candidate lists and the render kernel of
        every render (rt_hip_set_timing); read them with frame_times()."""
        _check(lib().rt_hip_set_timing(self.h, 1 if on else 0), "timing")

    def frame_times(self, n=1):
        """[(lists_ms, render_kernel_ms)] of the last n timed renders, oldest first."""
        a, b = (C.c_float * n)(), (C.c_float * n)()
        _check(lib().rt_hip_frame_times(self.h, n, a, b), "frame_times")
        return list(zip(a, b))

    def kernel_times(self, n=1):
        """[(trace_ms, shade_ms, fold_ms)] of the last n timed renders, oldest first."""
        a, b, c = (C.c_float * n)(), (C.c_float * n)(), (C.c_float * n)()
        _check(lib().rt_hip_frame_kernel_times(self.h, n, a, b, c), "frame_kernel_times")
        return list(zip(a, b, c))

    def tile_cycles(self, n):
        """Per-tile shader clocks of the last instrumented render (numpy uint64)."""
        out = np.zeros(n, dtype=np.uint64)
        _check(lib().rt_hip_tile_cycles(self.h, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), n),
               "tile_cycles")
        return out

    def tile_phase_cycles(self, phase, n):
        """Per-item phase clocks (rt_hip_tile_phase_cycles; numpy uint64)."""
        out = np.zeros(n, dtype=np.uint64)
        _check(lib().rt_hip_tile_phase_cycles(self.h, phase,
                                              out.ctypes.data_as(C.POINTER(C.c_ulonglong)), n),
               "tile_phase_cycles")
        return out

    def set_light_buffers(self, on=True):
        """Light buffers for the default shadow queries (rt_hip_set_light_buffers)."""
        _check(lib().rt_hip_set_light_buffers(self.h, 1 if on else 0), "light_buffers")

    def set_lightbuf_entry_cap(self, cap):
        """Test hook: light-buffer builds of more than `cap` entries fail (0: no cap);
        the buffers are rebuilt now (rt_hip_set_lightbuf_entry_cap)."""
        _check(lib().rt_hip_set_lightbuf_entry_cap(self.h, int(cap)), "lightbuf_entry_cap")

    def probe_shadows(self, light, origins, brute=False):
        """Shadow rays of light `light` from (n, 3) origins: shadowed flags
        through the light buffer, or brute force (rt_hip_probe_shadows)."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(o), np.uint8)
        _check(lib().rt_hip_probe_shadows(self.h, int(light), o.ctypes.data_as(C.c_void_p), len(o),
                                          1 if brute else 0, out.ctypes.data_as(C.c_void_p)),
               "probe_shadows")
        return out.astype(bool)

    def probe_closest(self, origins, dirs, brute=False):
        """Closest hits of (n, 3) rays queried as reflection rays (the per-lane
        octree walk) or by brute force (rt_hip_probe_closest): (prim, dist)
        arrays, prim = 0xffffffff for no hit."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        assert len(o) == len(d)
        prim = np.zeros(len(o), np.uint32)
        dist = np.zeros(len(o), np.float32)
        _check(lib().rt_hip_probe_closest(self.h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                          len(o), 1 if brute else 0, prim.ctypes.data_as(C.c_void_p),
                                          dist.ctypes.data_as(C.c_void_p)), "probe_closest")
        return prim, dist

    def set_exact_shadows(self, on=True):
        """Shadow rays exact by proof (rt_hip_set_exact_shadows; default on):
        proven light buffers, the proven walk where a light's queries walk.
        Off: slack-grown buffers, measured against brute force, not proven."""
        _check(lib().rt_hip_set_exact_shadows(self.h, 1 if on else 0), "exact_shadows")

    def set_exact_reflections(self, on=True):
        """Reflection rays exact by proof (rt_hip_set_exact_reflections):
        the reflection walk grows every node's box by the float test's error
        region for the ray (csrc/rt_reflect.hip); the closest-hit probe uses
        the same walk.  Off (the default): the culling slack, tested."""
        _check(lib().rt_hip_set_exact_reflections(self.h, 1 if on else 0), "exact_reflections")

    def set_policy(self, policy):
        """Octree traversal policy (rt_hip_set_policy): 0 default, 1 per-lane,
        2 staged packet, 3 default + staged directional shadows."""
        _check(lib().rt_hip_set_policy(self.h, int(policy)), "policy")

    def set_camera_refine(self, on=True):
        """Per-tile refinement of the big candidate footprints (default on)."""
        _check(lib().rt_hip_set_camera_refine(self.h, 1 if on else 0), "camera_refine")

    def set_camera_bound_scale(self, scale):
        _check(lib().rt_hip_set_camera_bound_scale(self.h, float(scale)), "bound_scale")
        if scale < 1.0:
            self.inexact = True

    def set_cull_slack(self, ulps):
        _check(lib().rt_hip_set_cull_slack(self.h, float(ulps)), "cull_slack")
        if ulps < 64.0:
            self.inexact = True

    def cand_verify(self, frame, rank=0, nranks=1):
        """Host re-derivation of the last render's candidate lists:
        {listed, entries, fp_mismatch, tile_mismatch, global}."""
        out = (C.c_ulonglong * 7)()
        _check(lib().rt_hip_cand_verify(self.h, C.byref(frame), rank, nranks, out), "cand_verify")
        return dict(zip(("listed", "entries", "fp_mismatch", "tile_mismatch", "global",
                         "filter_violation", "filtered"), (int(x) for x in out)))

    def cand_verify_compat(self, camera):
        """cand_verify for the last rt_hip_render_compat of `camera`."""
        out = (C.c_ulonglong * 7)()
        _check(lib().rt_hip_cand_verify_compat(self.h, C.byref(camera), out), "cand_verify_compat")
        return dict(zip(("listed", "entries", "fp_mismatch", "tile_mismatch", "global",
                         "filter_violation", "filtered"), (int(x) for x in out)))

    def verify_shadows(self, stride=1, first=0):
        """Shadow outcomes of the last render's hit records (every stride-th
        per region, from the first-th): the walk vs brute force
        (rt_hip_verify_shadows_from)."""
        out = (C.c_ulonglong * 4)()
        _check(lib().rt_hip_verify_shadows_from(self.h, stride, first, out), "verify_shadows")
        return dict(zip(("records", "queries", "records_differ", "walk_lit_brute_shadowed"),
                        (int(x) for x in out)))

    def cand_tile_entries(self, ntiles):
        """Candidate-list entries per rank-local tile of the last render."""
        out = np.zeros(ntiles, np.uint32)
        _check(lib().rt_hip_cand_tile_entries(self.h, out.ctypes.data_as(C.c_void_p), ntiles),
               "cand_tile_entries")
        return out

    def set_cand_item_cap(self, cap):
        """Test hook: cap the big footprints' emission work items (0: one
        wave per footprint, the fallback path)."""
        _check(lib().rt_hip_set_cand_item_cap(self.h, int(cap)), "cand_item_cap")

    def set_overlap_lists(self, on=True):
        """The next frame's list build beside the last frame's shade pass
        (rt_hip_set_overlap_lists, default on; off for A/B runs)."""
        _check(lib().rt_hip_set_overlap_lists(self.h, 1 if on else 0), "overlap_lists")

    def overlap_builds(self):
        """List builds of this context that ran on its second stream."""
        n = C.c_ulonglong()
        _check(lib().rt_hip_overlap_builds(self.h, C.byref(n)), "overlap_builds")
        return int(n.value)

    def set_camera_slack(self, ulps):
        _check(lib().rt_hip_set_camera_slack(self.h, float(ulps)), "camera_slack")

    def render(self, frame, rank, nranks, d_tiles, stream=None):
        _check(lib().rt_hip_render(self.h, C.byref(frame), rank, nranks, C.c_void_p(d_tiles),
                                   C.c_void_p(stream) if stream else None), "rt_hip_render")

    def stats(self):
        st = Stats()
        self._check_render(lib().rt_hip_stats(self.h, C.byref(st)), "rt_hip_stats")
        return st.as_dict()

    # rt_hip_frame_check flag bits (csrc/rt_counters.h RT_FRAME_*)
    FRAME_FLAGS = {1: "hit records past the buffer (RT_EHITBUF)", 2: "bounce limit / stack overflow (RT_EDEPTH)",
                   4: "zero interpolated normal (RT_EZERONORMAL)",
                   8: "unproven or undecided exact shadow / reflection queries (RT_EINEXACT)",
                   16: "asynchronous list build overflow (RT_EHITBUF)"}

    def frame_check(self):
        """(flags, frames, closest, shadow): the per-frame completeness checks
        of every render since the last call, ORed (0 = every frame complete,
        FRAME_FLAGS names the bits), the renders checked and their summed
        closest-hit / shadow queries (rt_hip_frame_check); all reset."""
        fl, n, q = C.c_uint(), C.c_uint(), (C.c_ulonglong * 2)()
        _check(lib().rt_hip_frame_check(self.h, C.byref(fl), C.byref(n), q), "rt_hip_frame_check")
        return int(fl.value), int(n.value), int(q[0]), int(q[1])

    def cand_produce(self, frame, rank, nranks, stream=None):
        """Triangle-parallel lists, step 1 (rt_hip_cand_produce): this rank's
        slice of the prims over the whole frame, routed by destination rank.
        Returns (counts per destination rank, this slice's global prims)."""
        counts = (C.c_uint * nranks)()
        ng = C.c_uint()
        _check(lib().rt_hip_cand_produce(self.h, C.byref(frame), rank, nranks, counts, C.byref(ng),
                                         C.c_void_p(stream) if stream else None), "rt_hip_cand_produce")
        return [int(x) for x in counts], int(ng.value)

    def cand_send_buffer(self):
        """(device pointer, entries) of the last produce's routed entries
        (3 x uint32 each, destination-rank order)."""
        ptr, n = C.c_void_p(), C.c_size_t()
        _check(lib().rt_hip_cand_send_buffer(self.h, C.byref(ptr), C.byref(n)), "rt_hip_cand_send_buffer")
        return ptr.value or 0, int(n.value)

    def cand_consume(self, frame, rank, nranks, d_entries, n, nglobal, stream=None):
        """Step 4: this rank's lists from the n received entries; the next
        render of (frame, rank, nranks) uses them (rt_hip_cand_consume)."""
        _check(lib().rt_hip_cand_consume(self.h, C.byref(frame), rank, nranks, C.c_void_p(d_entries), n, nglobal,
                                         C.c_void_p(stream) if stream else None), "rt_hip_cand_consume")

    def assemble(self, frame, d_gathered, nranks, d_rgb, stream=None):
        _check(lib().rt_hip_assemble(self.h, C.byref(frame), C.c_void_p(d_gathered), nranks,
                                     C.c_void_p(d_rgb), C.c_void_p(stream) if stream else None),
               "rt_hip_assemble")

    def render_image(self, frame):
        """Whole frame on this device -> (H, W, 3) float32 in PPM order, stats."""
        img = np.empty((frame.height, frame.width, 3), np.float32)
        st = Stats()
        self._check_render(lib().rt_hip_render_image(self.h, C.byref(frame),
                                                     img.ctypes.data_as(C.c_void_p), C.byref(st)),
                           "rt_hip_render_image")
        return img, st.as_dict()

    def set_lights(self, lights):
        """Replace the light table (rt_hip_set_lights): a ctypes Light array
        (e.g. Scene.lights()) or a sequence of (type, r, g, b, x, y, z).  Only
        the buffers of lights whose (type, position) changed are rebuilt."""
        if not isinstance(lights, C.Array):
            rows = list(lights)
            arr = (Light * len(rows))()
            for l, (t, r, g, b, x, y, z) in zip(arr, rows):
                l.type, l.r, l.g, l.b = int(t), r, g, b
                l.v.x, l.v.y, l.v.z = x, y, z
            lights = arr
        _check(lib().rt_hip_set_lights(self.h, C.cast(lights, C.c_void_p), len(lights)), "rt_hip_set_lights")

    def set_materials(self, scene_or_objects):
        """ka, kd, ks, ns of every object (rt_hip_set_materials) from a Scene
        or a ctypes Object array; nr must be what the context was created with."""
        if isinstance(scene_or_objects, Scene):
            s = scene_or_objects.s
            ptr, n = C.cast(s.objects, C.c_void_p), int(s.object_count)
        else:
            ptr, n = C.cast(scene_or_objects, C.c_void_p), len(scene_or_objects)
        _check(lib().rt_hip_set_materials(self.h, ptr, n), "rt_hip_set_materials")

    def set_triangles(self, array, first=0):
        """Replace the triangles [first, first + n) of the live context, in
        prim order, by an (n, 6, 3) or (n, 18) float32 host array (the layout
        of Scene.triangles_array(); rt_hip_set_triangles_host): everything that
        depends on them is rebuilt on the device before this returns."""
        a = _triangle_rows(array)
        _check(lib().rt_hip_set_triangles_host(self.h, a.ctypes.data_as(C.c_void_p) if len(a) else None,
                                               int(first), len(a)), "rt_hip_set_triangles_host")

    def set_triangles_device(self, ptr, first, count):
        """set_triangles from device memory of the context's device: `count`
        records of 18 floats at `ptr` (a torch tensor's data_ptr();
        rt_hip_set_triangles), read on the context's stream."""
        _check(lib().rt_hip_set_triangles(self.h, C.c_void_p(ptr) if ptr else None, int(first), int(count)),
               "rt_hip_set_triangles")

    def geometry_updates(self):
        """Successful geometry updates of this context so far."""
        n = C.c_ulonglong()
        _check(lib().rt_hip_geometry_updates(self.h, C.byref(n)), "rt_hip_geometry_updates")
        return int(n.value)

    def geometry_times(self):
        """(flatten + box + flags, tree, light buffers) wall seconds of the
        last successful geometry update (rt_hip_geometry_times)."""
        t = (C.c_double * 3)()
        _check(lib().rt_hip_geometry_times(self.h, t), "rt_hip_geometry_times")
        return tuple(float(x) for x in t)

    def set_keep_visibility(self, on=True):
        """Renders keep each hit record's unshadowed-light mask, so the first
        relight can already skip shadow queries (rt_hip_set_keep_visibility)."""
        _check(lib().rt_hip_set_keep_visibility(self.h, 1 if on else 0), "rt_hip_set_keep_visibility")

    def relight(self, frame, rank, nranks, d_tiles, stream=None):
        """The last render's kept hit records shaded again under the current
        lights and materials, folded into d_tiles (rt_hip_relight)."""
        _check(lib().rt_hip_relight(self.h, C.byref(frame), rank, nranks, C.c_void_p(d_tiles),
                                    C.c_void_p(stream) if stream else None), "rt_hip_relight")

    def relight_image(self, frame):
        """relight() of the whole frame after render_image(frame) -> (H, W, 3)
        float32 in PPM order, stats (rt_hip_relight_image)."""
        img = np.empty((frame.height, frame.width, 3), np.float32)
        st = Stats()
        self._check_render(lib().rt_hip_relight_image(self.h, C.byref(frame), img.ctypes.data_as(C.c_void_p),
                                                      C.byref(st)), "rt_hip_relight_image")
        return img, st.as_dict()

    def set_gbuffer(self, on=True):
        """Renders capture the per-sample G-buffer (rt_hip_set_gbuffer); read
        it with gbuffer() after each render."""
        _check(lib().rt_hip_set_gbuffer(self.h, 1 if on else 0), "rt_hip_set_gbuffer")

    def gbuffer(self, frame, rank, nranks, d_tiles, stream=None):
        """The last render's G-buffer tile buffer (rt_hip_gbuffer): d_tiles =
        device memory of gbuffer_tile_words() words."""
        _check(lib().rt_hip_gbuffer(self.h, C.byref(frame), rank, nranks, C.c_void_p(d_tiles),
                                    C.c_void_p(stream) if stream else None), "rt_hip_gbuffer")

    def assemble_gbuffer(self, frame, d_gathered, nranks, d_samples, stream=None):
        """Gathered G-buffer tile buffers -> H*W*4 records in PPM order."""
        _check(lib().rt_hip_assemble_gbuffer(self.h, C.byref(frame), C.c_void_p(d_gathered), nranks,
                                             C.c_void_p(d_samples), C.c_void_p(stream) if stream else None),
               "rt_hip_assemble_gbuffer")

    def render_image_gbuffer(self, frame):
        """Whole frame on this device -> (H, W, 3) float32 image, (H, W, 4)
        GSAMPLE records (a pixel's four samples in cpu order), stats."""
        img = np.empty((frame.height, frame.width, 3), np.float32)
        smp = np.empty((frame.height, frame.width, 4), GSAMPLE)
        st = Stats()
        self._check_render(lib().rt_hip_render_image_gbuffer(self.h, C.byref(frame),
                                                             img.ctypes.data_as(C.c_void_p),
                                                             smp.ctypes.data_as(C.c_void_p), C.byref(st)),
                           "rt_hip_render_image_gbuffer")
        return img, smp, st.as_dict()

    def _keep_rc(self, rc):
        self.last_rc = rc
        return rc

    def trace_rays_device(self, d_origins, d_dirs, n, d_rgb=0, d_samples=0, packet=False, stream=None):
        """rt_hip_trace_rays on device pointers (asynchronous): d_rgb receives
        3 n floats, d_samples n GSAMPLE records; 0 leaves either out (d_rgb
        = 0: a ray cast)."""
        _check(lib().rt_hip_trace_rays(self.h, C.c_void_p(d_origins), C.c_void_p(d_dirs), int(n),
                                       RT_RAYS_PACKET if packet else 0, C.c_void_p(d_rgb) if d_rgb else None,
                                       C.c_void_p(d_samples) if d_samples else None,
                                       C.c_void_p(stream) if stream else None), "rt_hip_trace_rays")

    def trace_rays(self, origins, dirs, packet=False, samples=False, shade=True):
        """trace(ray, 1.0) of cpu/raytracer.c:19-34 for (n, 3) float32 rays
        (rt_hip_trace_rays_host; directions used as given) -> (rgb (n, 3)
        float32 or None, GSAMPLE records (n,) of the first hits or None,
        stats).  shade=False: a ray cast (samples only, one query per ray).
        packet: each aligned 64 rays walk their first query as one packet --
        the same bits, faster for coherent groups."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        assert len(o) == len(d)
        samples = samples or not shade
        rgb = np.zeros((len(o), 3), np.float32) if shade else None
        smp = np.zeros(len(o), GSAMPLE) if samples else None
        st = Stats()
        self.last_rc = 0  # the call's return code (RT_EINEXACT passes _check_render after a parity-breaking knob)
        rc = self._keep_rc(lib().rt_hip_trace_rays_host(
            self.h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), len(o),
            RT_RAYS_PACKET if packet else 0, rgb.ctypes.data_as(C.c_void_p) if shade else None,
            smp.ctypes.data_as(C.c_void_p) if samples else None, C.byref(st)))
        if shade and len(o):  # what path_records sizes its arrays by
            self._batch_n, self._batch_records = len(o), int(st.hit_records)
        self._check_render(rc, "rt_hip_trace_rays_host")
        return rgb, smp, st.as_dict()

    def frame_rays(self, frame, order="pixel"):
        """The frame's 4 W H camera rays from the device generator
        (rt_hip_frame_rays) -> (origins, dirs), (n, 3) float32 each; order
        "pixel" or "quarter" (camera_rays is the numpy restatement)."""
        n = 4 * frame.width * frame.height
        o, d = np.empty((max(n, 0), 3), np.float32), np.empty((max(n, 0), 3), np.float32)
        _check(lib().rt_hip_frame_rays_host(self.h, C.byref(frame), RAY_ORDER[order] if isinstance(order, str) else order,
                                            o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)),
               "rt_hip_frame_rays")
        return o, d

    def occluded_device(self, d_origins, d_dirs, d_tmax, n, d_out, packet=False, stream=None):
        """rt_hip_occluded on device pointers (asynchronous): d_out receives n
        bytes, 1 where something lies within d_tmax[i] (world distance) along
        ray i; d_tmax = 0 (NULL): no bound."""
        _check(lib().rt_hip_occluded(self.h, C.c_void_p(d_origins) if d_origins else None,
                                     C.c_void_p(d_dirs) if d_dirs else None, C.c_void_p(d_tmax) if d_tmax else None,
                                     int(n), RT_RAYS_PACKET if packet else 0, C.c_void_p(d_out) if d_out else None,
                                     C.c_void_p(stream) if stream else None), "rt_hip_occluded")

    def occluded(self, origins, dirs, tmax=None, packet=False):
        """Is anything in the way of (n, 3) float32 rays, up to tmax
        (rt_hip_occluded_host)?  byte i = collide_dist(ray i) != 0 and <=
        tmax[i] (cpu/hit.c:93-109); tmax: None (no bound: has_direct_hit), a
        scalar or (n,) world distances, independent of |dir| -> (uint8 (n,),
        stats).  packet: each aligned 64 rays walk as one packet -- the same
        bytes, faster for coherent groups."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        assert len(o) == len(d)
        t = None
        if tmax is not None:
            t = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, dtype=np.float32), (len(o),)))
        out = np.zeros(len(o), np.uint8)
        st = Stats()
        self.last_rc = 0  # the call's return code (RT_EINEXACT passes _check_render after a parity-breaking knob)
        self._check_render(self._keep_rc(lib().rt_hip_occluded_host(
            self.h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
            t.ctypes.data_as(C.c_void_p) if t is not None else None, len(o), RT_RAYS_PACKET if packet else 0,
            out.ctypes.data_as(C.c_void_p), C.byref(st))), "rt_hip_occluded_host")
        return out, st.as_dict()

    def ambient_occlusion_device(self, d_samples, n, k, d_table, m, seed, d_out, tmax=None, packet=False, base=0,
                                 stream=None):
        """rt_hip_ambient_occlusion on device pointers (asynchronous): d_samples
        = n GSAMPLE records (a tile buffer, assembled samples, a ray batch's
        records), d_table = m rows of 3 floats, d_out receives n uint32 counts."""
        _check(lib().rt_hip_ambient_occlusion(
            self.h, C.c_void_p(d_samples) if d_samples else None, int(n), int(base), int(k),
            C.c_void_p(d_table) if d_table else None, int(m), int(seed) & 0xffffffff,
            float(np.inf if tmax is None else tmax), RT_RAYS_PACKET if packet else 0,
            C.c_void_p(d_out) if d_out else None, C.c_void_p(stream) if stream else None), "rt_hip_ambient_occlusion")

    def ambient_occlusion(self, samples, k, table, seed, tmax=None, packet=False, base=0):
        """How many of each GSAMPLE record's k hemisphere rays are occluded
        within tmax (None: no bound)?  The rays are ao_rays_host's, made on the
        device (rt_hip_ambient_occlusion_host) -> (uint32 (n,), stats: those
        of the occlusion batch of the same rays)."""
        smp = np.ascontiguousarray(samples, dtype=GSAMPLE).reshape(-1)
        tab = np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(smp), np.uint32)
        st = Stats()
        self.last_rc = 0  # the call's return code (RT_EINEXACT passes _check_render after a parity-breaking knob)
        self._check_render(self._keep_rc(lib().rt_hip_ambient_occlusion_host(
            self.h, smp.ctypes.data_as(C.c_void_p), len(smp), int(base), int(k), tab.ctypes.data_as(C.c_void_p),
            len(tab), int(seed) & 0xffffffff, float(np.inf if tmax is None else tmax),
            RT_RAYS_PACKET if packet else 0, out.ctypes.data_as(C.c_void_p), C.byref(st))),
            "rt_hip_ambient_occlusion_host")
        return out, st.as_dict()

    def gather_device(self, d_samples, n, k, d_table, m, seed, d_rgb, packet=False, base=0, stream=None):
        """rt_hip_gather on device pointers (asynchronous): d_samples = n
        GSAMPLE records (a tile buffer, assembled samples, a ray batch's
        records, caller points), d_table = m rows of 3 floats, d_rgb receives
        3 n floats: per record the sum of its k hemisphere rays' traced colours."""
        _check(lib().rt_hip_gather(
            self.h, C.c_void_p(d_samples) if d_samples else None, int(n), int(base), int(k),
            C.c_void_p(d_table) if d_table else None, int(m), int(seed) & 0xffffffff,
            RT_RAYS_PACKET if packet else 0, C.c_void_p(d_rgb) if d_rgb else None,
            C.c_void_p(stream) if stream else None), "rt_hip_gather")

    def gather(self, samples, k, table, seed, packet=False, base=0):
        """The light each GSAMPLE record's k hemisphere rays bring back: the
        rays are ao_rays_host's, made on the device, each traced as
        trace_rays traces it, their colours summed per record by gather_sum's
        rule (rt_hip_gather_host) -> (rgb (n, 3) float32: raw sums, not divided
        by k, stats: those of the ray batch of the same rays)."""
        smp = np.ascontiguousarray(samples, dtype=GSAMPLE).reshape(-1)
        tab = np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 3)
        rgb = np.zeros((len(smp), 3), np.float32)
        st = Stats()
        self.last_rc = 0  # the call's return code (RT_EINEXACT passes _check_render after a parity-breaking knob)
        self._check_render(self._keep_rc(lib().rt_hip_gather_host(
            self.h, smp.ctypes.data_as(C.c_void_p), len(smp), int(base), int(k), tab.ctypes.data_as(C.c_void_p),
            len(tab), int(seed) & 0xffffffff, RT_RAYS_PACKET if packet else 0, rgb.ctypes.data_as(C.c_void_p),
            C.byref(st))), "rt_hip_gather_host")
        return rgb, st.as_dict()

    def path_records_device(self, n, d_offsets, cap=0, d_records=0, d_coef=0, d_terms=0, stream=None):
        """rt_hip_path_records on device pointers (asynchronous, on the
        batch's stream): the paths of the last ray batch with colours, n its
        rays.  d_offsets receives n + 1 uint32; below `cap` vertices d_records
        receives GSAMPLE records, d_coef one float and d_terms three floats per
        vertex; 0 leaves any of the three out (all three: a count)."""
        _check(lib().rt_hip_path_records(
            self.h, int(n), C.c_void_p(d_offsets) if d_offsets else None, int(cap),
            C.c_void_p(d_records) if d_records else None, C.c_void_p(d_coef) if d_coef else None,
            C.c_void_p(d_terms) if d_terms else None, C.c_void_p(stream) if stream else None),
            "rt_hip_path_records")

    def path_records(self, records=True, coef=True, terms=True, n=None, cap=None):
        """The paths of the last ray batch with colours (rt_hip_path_records_host)
        -> (offsets (n + 1,) uint32, GSAMPLE records (total,), coef (total,)
        float32, terms (total, 3) float32; None for what was not asked).  n and
        cap default to the rays and rt_stats.hit_records of the last
        trace_rays / trace_paths of this object; the arrays are checked against
        offsets[n] and cut to it (an overflowing batch counts more records than
        its paths hold).  cap given: at most cap vertices, as the C call."""
        if n is None:
            n = self._batch_n
        fit = cap is None
        if fit:
            cap = self._batch_records
        n, cap = int(n), int(cap)
        off = np.zeros(n + 1, np.uint32)
        for _ in range(2):
            rec = np.zeros(cap, GSAMPLE) if records else None
            cf = np.zeros(cap, np.float32) if coef else None
            tm = np.zeros((cap, 3), np.float32) if terms else None
            _check(lib().rt_hip_path_records_host(
                self.h, n, off.ctypes.data_as(C.c_void_p), cap,
                rec.ctypes.data_as(C.c_void_p) if records else None, cf.ctypes.data_as(C.c_void_p) if coef else None,
                tm.ctypes.data_as(C.c_void_p) if terms else None), "rt_hip_path_records_host")
            total = int(off[n])
            if not fit or total <= cap or not (records or coef or terms):
                break
            cap = total  # (the export reads only: the same words again, all of them)
        k = min(total, cap)
        cut = lambda a: None if a is None else a[:k]
        return off, cut(rec), cut(cf), cut(tm)

    def trace_paths(self, origins, dirs, packet=False):
        """trace_rays and the batch's paths in one go -> (rgb (n, 3) float32,
        offsets (n + 1,) uint32, GSAMPLE records (total,), coef (total,), terms
        (total, 3), stats): path_fold(offsets, terms) is rgb."""
        rgb, _, st = self.trace_rays(origins, dirs, packet=packet)
        off, rec, cf, tm = self.path_records()
        return rgb, off, rec, cf, tm, st

    def direct_light_device(self, d_samples, n, d_rgb, d_lit=0, packet=False, stream=None):
        """rt_hip_direct_light on device pointers (asynchronous): d_samples = n
        GSAMPLE records (a tile buffer, assembled samples, a ray batch's
        records, caller points), d_rgb receives 3 n floats, d_lit (0: none) n
        uint32 unshadowed-light masks."""
        _check(lib().rt_hip_direct_light(self.h, C.c_void_p(d_samples) if d_samples else None, int(n),
                                         RT_RAYS_PACKET if packet else 0, C.c_void_p(d_rgb) if d_rgb else None,
                                         C.c_void_p(d_lit) if d_lit else None,
                                         C.c_void_p(stream) if stream else None), "rt_hip_direct_light")

    def direct_light(self, samples, packet=False, lit=False):
        """apply_light of cpu/light.c:33-100 at each GSAMPLE record's (P, N)
        with its object's material, under the context's current lights
        (rt_hip_direct_light_host) -> (rgb (n, 3) float32, uint32 (n,) masks of
        the unshadowed casting lights 0..31 or None, stats).  Records that do
        not shade (direct_light_shades) get 0 0 0 and mask 0."""
        smp = np.ascontiguousarray(samples, dtype=GSAMPLE).reshape(-1)
        rgb = np.zeros((len(smp), 3), np.float32)
        mask = np.zeros(len(smp), np.uint32) if lit else None
        st = Stats()
        self.last_rc = 0  # the call's return code (RT_EINEXACT passes _check_render after a parity-breaking knob)
        self._check_render(self._keep_rc(lib().rt_hip_direct_light_host(
            self.h, smp.ctypes.data_as(C.c_void_p), len(smp), RT_RAYS_PACKET if packet else 0,
            rgb.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p) if lit else None, C.byref(st))),
            "rt_hip_direct_light_host")
        return rgb, mask, st.as_dict()

    def lightbuf_box(self, light):
        """The proof box (lo, hi), float32 (3,) each, of light `light`'s
        buffer (rt_hip_lightbuf_box), or None when the light has none."""
        has = C.c_int(0)
        lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
        _check(lib().rt_hip_lightbuf_box(self.h, int(light), C.byref(has), lo, hi), "rt_hip_lightbuf_box")
        return (np.array(lo[:], np.float32), np.array(hi[:], np.float32)) if has.value else None

    def ao_rays_device(self, d_samples, n, k, d_table, m, seed, d_origins, d_dirs, d_shot=0, base=0, stream=None):
        """rt_hip_ao_rays on device pointers (asynchronous)."""
        _check(lib().rt_hip_ao_rays(self.h, C.c_void_p(d_samples) if d_samples else None, int(n), int(base), int(k),
                                    C.c_void_p(d_table) if d_table else None, int(m), int(seed) & 0xffffffff,
                                    C.c_void_p(d_origins) if d_origins else None,
                                    C.c_void_p(d_dirs) if d_dirs else None, C.c_void_p(d_shot) if d_shot else None,
                                    C.c_void_p(stream) if stream else None), "rt_hip_ao_rays")

    def ao_rays(self, samples, k, table, seed, base=0):
        """The rays the device generates for GSAMPLE records (rt_hip_ao_rays)
        -> (origins, dirs) (n k, 3) float32 and the shot mask: ao_rays_host's."""
        smp = np.ascontiguousarray(samples, dtype=GSAMPLE).reshape(-1)
        tab = np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 3)
        n, nr = len(smp), len(smp) * int(k)
        o, d, shot = np.zeros((nr, 3), np.float32), np.zeros((nr, 3), np.float32), np.zeros(n, np.uint8)
        _check(lib().rt_hip_ao_rays_host(self.h, smp.ctypes.data_as(C.c_void_p), n, int(base), int(k),
                                         tab.ctypes.data_as(C.c_void_p), len(tab), int(seed) & 0xffffffff,
                                         o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                         shot.ctypes.data_as(C.c_void_p)), "rt_hip_ao_rays_host")
        return o, d, shot.astype(bool)

    def render_compat(self, camera):
        """gpu/rt compatibility mode (rt_hip_render_compat) -> (H, W, 4)
        uint8 RGBA in gpu/rt's PNG row order, stats."""
        img = np.empty((camera.height, camera.width, 4), np.uint8)
        st = Stats()
        cam = Camera()
        C.pointer(cam)[0] = camera
        self._check_render(lib().rt_hip_render_compat(self.h, C.byref(cam), img.ctypes.data_as(C.c_void_p),
                                                      C.byref(st)), "rt_hip_render_compat")
        return img, st.as_dict()

    def close(self):
        if self.h:
            lib().rt_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cand_exchange_local(contexts, frame):
    """Triangle-parallel lists of an len(contexts)-rank frame in this process
    (rt_hip_cand_exchange_local): contexts[r] produces rank r's slice, the
    blocks move by device memcpy, every rank consumes its own; each context's
    next render(frame, r, n) uses them.  The exchange rt_raytrace_multi makes
    over RCCL from 4 GPUs up, drivable with every context on one GPU."""
    arr = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
    _check(lib().rt_hip_cand_exchange_local(arr, len(contexts), C.byref(frame)), "rt_hip_cand_exchange_local")


def exchange_cand_entries(dist, send, counts, nglobal):
    """Step 3 of the triangle-parallel lists (include/rt_hip.h
    rt_hip_cand_produce): the all-to-all of the routed entries over
    torch.distributed (RCCL for device tensors, gloo for host tensors).
    send: (sum(counts), 3) int32 tensor in destination-rank order; counts:
    entries for each rank; nglobal: this rank's global prims.  Returns (the
    (n, 3) int32 entries this rank receives, in source-rank order, and the
    producers' global prims summed).  Two collectives: the (count, globals)
    pairs, then the entries."""
    import torch
    w = len(counts)
    meta = torch.tensor([[int(c), int(nglobal)] for c in counts], dtype=torch.int64,
                        device=send.device).reshape(-1)
    rmeta = torch.empty_like(meta)
    dist.all_to_all_single(rmeta, meta)
    rm = rmeta.view(w, 2).tolist()
    rc = [int(a) for a, _ in rm]
    recv = torch.empty((sum(rc), 3), dtype=torch.int32, device=send.device)
    dist.all_to_all_single(recv, send[: sum(counts)], output_split_sizes=rc,
                           input_split_sizes=[int(c) for c in counts])
    return recv, sum(int(b) for _, b in rm)


def write_ppm(path, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w, _ = rgb.shape
    _check(lib().rt_ppm_write(os.fsencode(path), w, h, rgb.ctypes.data_as(C.c_void_p)), "ppm")


def write_png(path, rgba):
    """8-bit RGBA PNG (rt_png_write_rgba); rgba = (H, W, 4) uint8."""
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w, _ = rgba.shape
    _check(lib().rt_png_write_rgba(os.fsencode(path), w, h, rgba.ctypes.data_as(C.c_void_p)), "png")


def raytrace_gpu(input_path, output_path, accel=None):
    """Drop-in for gpu/rt's main (gpu/rt.cpp:56-97): PNG in compatibility mode."""
    a = -1 if accel is None else (ACCEL[accel] if isinstance(accel, str) else accel)
    _check(lib().rt_raytrace_gpu(os.fsencode(input_path), os.fsencode(output_path), a),
           "rt_raytrace_gpu")


def raytrace_devices(input_path, output_path, devices, accel=None):
    """rt_raytrace_multi_dev: rank g on device devices[g] (a device shared by
    several ranks: memcpy transport in place of RCCL); (stats, render_ms)."""
    st = Stats()
    ms = C.c_double(0)
    a = -1 if accel is None else (ACCEL[accel] if isinstance(accel, str) else accel)
    devs = (C.c_int * len(devices))(*devices)
    _check(lib().rt_raytrace_multi_dev(os.fsencode(input_path), os.fsencode(output_path), len(devices), devs, a,
                                       C.byref(st), C.byref(ms)), "rt_raytrace_multi_dev")
    return st.as_dict(), ms.value


def raytrace(input_path, output_path, gpus=1, accel=None):
    """Drop-in for raytrace() (cpu/raytracer.c:79-136); returns (stats, render_ms)."""
    st = Stats()
    ms = C.c_double(0)
    a = -1 if accel is None else (ACCEL[accel] if isinstance(accel, str) else accel)
    _check(lib().rt_raytrace_multi(os.fsencode(input_path), os.fsencode(output_path), gpus, a,
                                   C.byref(st), C.byref(ms)), "rt_raytrace")
    return st.as_dict(), ms.value


# ---- tile map (host mirror of csrc/rt_tiles.h) ----
def block_side(nranks):
    """Tiles per block side: 4 when the frame is split, 1 (plain scanline
    tiles) for one rank.  Block (bx, by) belongs to rank (bx + by) % nranks;
    a rank's buffer holds its blocks in scanline order."""
    return 4 if nranks > 1 else 1


def _blocks(width, height, nranks):
    tb = block_side(nranks)
    tx, ty = (width + 7) // 8, (height + 7) // 8
    return tb, -(-tx // tb), -(-ty // tb)


def _rank_block_grid(width, height, nranks):
    """(blocks_y, blocks_x) arrays: each block's rank and rank-local index."""
    tb, bx, by = _blocks(width, height, nranks)
    x = np.arange(bx)[None, :]
    y = np.arange(by)[:, None]
    rank = (x + y) % nranks
    local = np.zeros((by, bx), np.int64)
    for r in range(nranks):
        m = (rank == r).ravel()
        local.ravel()[m] = np.arange(int(m.sum()))
    return rank, local


def rank_tile_count(width, height, rank, nranks):
    """Tiles (whole blocks, edge padding included) rank `rank` renders."""
    tb = block_side(nranks)
    rk, _ = _rank_block_grid(width, height, nranks)
    return int((rk == rank).sum()) * tb * tb


def tiles_per_rank_host(width, height, nranks):
    """The most tiles any rank holds (the tile buffers' stride)."""
    return max(rank_tile_count(width, height, r, nranks) for r in range(nranks))


def tile_xy(t, rank, nranks, width, height):
    """(tx, ty) of rank-local tiles t (numpy arrays) of rank `rank`."""
    tb = block_side(nranks)
    rk, _ = _rank_block_grid(width, height, nranks)
    ys, xs = np.nonzero(rk == rank)  # scanline order = the rank's block order
    t = np.asarray(t)
    j, k = t // (tb * tb), t % (tb * tb)
    return xs[j] * tb + k % tb, ys[j] * tb + k // tb


def tile_local(tx, ty, nranks, width, height):
    """(rank, local index) of tiles (tx, ty) (numpy arrays)."""
    tb = block_side(nranks)
    rk, loc = _rank_block_grid(width, height, nranks)
    tx, ty = np.asarray(tx), np.asarray(ty)
    bx, by = tx // tb, ty // tb
    return rk[by, bx], loc[by, bx] * (tb * tb) + (ty % tb) * tb + tx % tb


def tile_pixels(width, height, rank, nranks):
    """(tiles, 64, 2) PPM (row, col) of the rank's tile-buffer slots, -1 where
    the slot is padding (past the frame's edge)."""
    n = rank_tile_count(width, height, rank, nranks)
    tx, ty = tile_xy(np.arange(n), rank, nranks, width, height)
    lane = np.arange(64)
    r = ty[:, None] * 8 + (lane // 8)[None, :]
    c = tx[:, None] * 8 + (lane % 8)[None, :]
    bad = (r >= height) | (c >= width)
    return np.stack([np.where(bad, -1, r), np.where(bad, -1, c)], axis=2)


def assemble_tiles_numpy(gathered, width, height, nranks):
    """Host mirror of the assemble kernel's index map (for CPU tests of the
    tiling / gather layout): gathered = nranks x tiles_per_rank x 64 x 3."""
    tpr = tiles_per_rank_host(width, height, nranks)
    g = np.asarray(gathered, np.float32).reshape(nranks, tpr, 64, 3)
    rows, cols = np.mgrid[0:height, 0:width]
    rk, loc = tile_local(cols // 8, rows // 8, nranks, width, height)
    lane = (rows % 8) * 8 + (cols % 8)
    return g[rk, loc, lane]


def assemble_gbuffer_numpy(gathered, width, height, nranks, words=4 * GB_WORDS):
    """assemble_tiles_numpy for tile buffers of `words` 32-bit words per pixel
    slot (the assemble_words kernel's index map): gathered = nranks x
    tiles_per_rank x 64 x words of any 4-byte dtype -> (H, W, words) uint32;
    view the G-buffer's 40 words as GSAMPLE for (H, W, 4) records."""
    tpr = tiles_per_rank_host(width, height, nranks)
    g = np.ascontiguousarray(gathered).view(np.uint32).reshape(nranks, tpr, 64, words)
    rows, cols = np.mgrid[0:height, 0:width]
    rk, loc = tile_local(cols // 8, rows // 8, nranks, width, height)
    lane = (rows % 8) * 8 + (cols % 8)
    return g[rk, loc, lane]


def tiles_from_image_numpy(img, rank, nranks):
    """Host mirror of what rank `rank` renders: its tile buffer
    (tiles_per_rank x 64 x 3, zero-padded) cut from a full (H, W, 3) image."""
    img = np.asarray(img, np.float32)
    height, width, _ = img.shape
    tpr = tiles_per_rank_host(width, height, nranks)
    out = np.zeros((tpr, 64, 3), np.float32)
    pix = tile_pixels(width, height, rank, nranks)
    ok = pix[..., 0] >= 0
    out[: len(pix)][ok] = img[pix[..., 0][ok], pix[..., 1][ok]]
    return out
