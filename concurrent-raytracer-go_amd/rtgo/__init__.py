"""rtgo — Python mirror of the reference's renderer interface over librtgo.so.

The reference's seam is the Go method set of ``*renderer.ParallelRenderer``
(internal/renderer/renderer.go:54-126, settings.go:3-36) plus
``scene.LoadFromFile`` (internal/scene/scene.go:45-57).  This module exposes
the same names (snake_case) on top of the C ABI in include/rt_api.h; the
compute path is the gfx950 kernel inside librtgo.so.  There is no CPU
fallback: rendering without a GPU raises ``RenderError``.

The library is loaded lazily.  When PyTorch is already imported its HIP
runtime (same soname, libamdhip64.so.7) is the one librtgo binds to, so
torch device pointers and streams can be passed to ``Context``.
"""
from __future__ import annotations

import ctypes
import json
import os
import time
from datetime import datetime, timezone

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RTGO_LIB selects an alternative build of the same library (the RT_WG_TIMING
# instrumented build of scripts/wg_timing.py); the library itself reads no
# environment variable
LIB_PATH = os.environ.get("RTGO_LIB") or os.path.join(os.path.dirname(_HERE), "build", "librtgo.so")

RT_OK = 0
RT_E_TIMEOUT = -6  # a multi-rank frame did not finish in time (rt_renderer_set_watchdog)
RT_OBJ_SPHERE, RT_OBJ_CUBE = 0, 1
MATERIAL_KINDS = {
    "lambertian": 0,
    "metal": 1,
    "shiny": 2,
    "perfectmirror": 3,
    "glass": 4,
    "dielectric": 5,
    "diffuselight": 6,
}
RT_LAYOUT_IMAGE, RT_LAYOUT_PACKED_TILES = 0, 1
RT_PATH_AUTO, RT_PATH_MEGAKERNEL = 0, 1
RT_PARTITION_AUTO, RT_PARTITION_STRIDED, RT_PARTITION_BALANCED = 0, 1, 2
SKIES = {"none": 0, "default": 1, "white": 2, "sunset": 3, "night": 4}  # RT_SKY_*
RT_CAMERA_REFERENCE, RT_CAMERA_LOOKAT = 0, 1  # rt_settings.camera
CAMERAS = {"reference": RT_CAMERA_REFERENCE, "lookat": RT_CAMERA_LOOKAT}
RT_COMM_ID_BYTES = 128
RT_MAX_FRAMES = 32  # frames per launch (rt_context_render_frames_async)
# wavefront kernel classes (RT_WF_*, rt_context_kernel_seconds)
WF_KERNELS = ["extend", "shade1", "occlude_hard", "cone", "softgen", "cone_rays", "occlude_soft", "shade", "regen", "resolve"]


class RenderError(RuntimeError):
    """A librtgo call failed (message from rt_last_error)."""


# --------------------------------------------------------------- C structs
class Material(ctypes.Structure):
    _fields_ = [
        ("kind", ctypes.c_int32),
        ("_pad", ctypes.c_int32),
        ("color", ctypes.c_double * 3),
        ("roughness", ctypes.c_double),
        ("metallic", ctypes.c_double),
        ("specular", ctypes.c_double),
        ("refraction_index", ctypes.c_double),
    ]


class Object(ctypes.Structure):
    _fields_ = [
        ("type", ctypes.c_int32),
        ("_pad", ctypes.c_int32),
        ("position", ctypes.c_double * 3),
        ("size", ctypes.c_double * 3),
        ("radius", ctypes.c_double),
        ("material", Material),
    ]


class Light(ctypes.Structure):
    _fields_ = [
        ("position", ctypes.c_double * 3),
        ("color", ctypes.c_double * 3),
        ("intensity", ctypes.c_double),
    ]


class Camera(ctypes.Structure):
    _fields_ = [
        ("position", ctypes.c_double * 3),
        ("look_at", ctypes.c_double * 3),
        ("up", ctypes.c_double * 3),
        ("fov", ctypes.c_double),
        ("aspect_ratio", ctypes.c_double),
    ]


class SceneView(ctypes.Structure):
    _fields_ = [
        ("camera", Camera),
        ("objects", ctypes.POINTER(Object)),
        ("num_objects", ctypes.c_int32),
        ("_pad0", ctypes.c_int32),
        ("lights", ctypes.POINTER(Light)),
        ("num_lights", ctypes.c_int32),
        ("_pad1", ctypes.c_int32),
    ]


class Settings(ctypes.Structure):
    _fields_ = [
        ("samples", ctypes.c_int32),
        ("max_depth", ctypes.c_int32),
        ("anti_aliasing", ctypes.c_int32),
        ("recursive_reflections", ctypes.c_int32),
        ("soft_shadows", ctypes.c_int32),
        ("depth_of_field", ctypes.c_int32),
        ("num_workers", ctypes.c_int32),
        ("num_devices", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("sky", ctypes.c_int32),
        ("camera", ctypes.c_int32),
    ]


class Tuning(ctypes.Structure):
    """rt_tuning: how the same work is cut and ordered (never the image)."""

    _fields_ = [
        ("path", ctypes.c_int32),
        ("pilot", ctypes.c_int32),
        ("frustum", ctypes.c_int32),
        ("stage", ctypes.c_int32),
        ("block_work", ctypes.c_double),
        ("block_samples", ctypes.c_int32),
        ("bvh_bins", ctypes.c_int32),
        ("bvh_leaf", ctypes.c_int32),
        ("wf_paths", ctypes.c_int32),
        ("wf_chunk", ctypes.c_int64),
        ("wf_lds_nodes", ctypes.c_int32),
        ("wf_trav_block", ctypes.c_int32),
        ("wf_trav_wgs", ctypes.c_int32),
        ("pilot_depth", ctypes.c_int32),
        ("split_samples", ctypes.c_int32),
        ("measure", ctypes.c_int32),
        ("split_depth", ctypes.c_int32),
        ("partition", ctypes.c_int32),
        ("wf_list_tries", ctypes.c_int32),
        ("tail_helpers", ctypes.c_int32),
        ("tail_paths", ctypes.c_int32),
        ("tail_depth", ctypes.c_int32),
        ("tail_every", ctypes.c_int32),
        ("tail_at", ctypes.c_int32),
        ("stream", ctypes.c_int32),
        ("stream_chunk", ctypes.c_int32),
        ("stream_max_mb", ctypes.c_double),
        ("stream_order", ctypes.c_int32),
        ("_stream_pad", ctypes.c_int32),
    ]


class Stats(ctypes.Structure):
    _fields_ = [
        ("render_seconds", ctypes.c_double),
        ("kernel_seconds", ctypes.c_double),
        ("rays_per_second", ctypes.c_double),
        ("pixels_per_second", ctypes.c_double),
        ("objects", ctypes.c_int32),
        ("lights", ctypes.c_int32),
        ("create_seconds", ctypes.c_double),
        ("scene_seconds", ctypes.c_double),
        ("bvh_build_seconds", ctypes.c_double),
        ("launch_seconds", ctypes.c_double),
        ("download_seconds", ctypes.c_double),
        ("destroy_seconds", ctypes.c_double),
    ]


class ContextStats(ctypes.Structure):
    """rt_context_stats (rt_context_get_stats)."""

    _fields_ = [(n, ctypes.c_int64) for n in ("schedules_built", "measuring_frames", "frames", "launches",
                                             "batched_launches", "blocks", "split_pixels", "tail_exported",
                                             "tail_errors", "stream_launches", "stream_live_pixels")]


COUNT_FIELDS = [
    "camera_rays",
    "bounce_rays",
    "shadow_rays",
    "sphere_tests",
    "triangle_tests",
    "box_tests",
    "shade_events",
    "light_evals",
    "rng_draws",
]


class Adaptive(ctypes.Structure):
    """rt_adaptive: the stop rule of an adaptive progression."""

    _fields_ = [
        ("tolerance", ctypes.c_int32),
        ("patience", ctypes.c_int32),
        ("min_samples", ctypes.c_int32),
        ("_pad", ctypes.c_int32),
    ]


class AovBuffers(ctypes.Structure):
    """rt_aov_buffers: the device pointers of a feature-buffer pass (None / 0: not written)."""

    _fields_ = [
        ("d_albedo", ctypes.c_void_p),
        ("d_normal", ctypes.c_void_p),
        ("d_depth", ctypes.c_void_p),
        ("d_coverage", ctypes.c_void_p),
        ("d_object", ctypes.c_void_p),
    ]


AOV_NAMES = ["albedo", "normal", "depth", "coverage", "object"]


class AovSpec(ctypes.Structure):
    """rt_aov_spec: the parameters of the specular-through feature pass (default_aov_spec())."""

    _fields_ = [
        ("max_bounces", ctypes.c_int32),
        ("_pad", ctypes.c_int32),
        ("max_roughness", ctypes.c_double),
    ]


class AovSpecBuffers(ctypes.Structure):
    """rt_aov_spec_buffers: the device pointers of a specular-through feature pass (None / 0: not written)."""

    _fields_ = [
        ("d_albedo", ctypes.c_void_p),
        ("d_normal", ctypes.c_void_p),
        ("d_depth", ctypes.c_void_p),
        ("d_coverage", ctypes.c_void_p),
        ("d_object", ctypes.c_void_p),
        ("d_specular", ctypes.c_void_p),
        ("d_bounces", ctypes.c_void_p),
    ]


AOV_SPEC_NAMES = AOV_NAMES + ["specular", "bounces"]


class Denoise(ctypes.Structure):
    """rt_denoise: the parameters of the à-trous denoiser (default_denoise())."""

    _fields_ = [
        ("levels", ctypes.c_int32),
        ("normal_power", ctypes.c_int32),
        ("sigma_color", ctypes.c_double),
        ("sigma_depth", ctypes.c_double),
        ("demodulate", ctypes.c_int32),
        ("_pad", ctypes.c_int32),
    ]


class DenoiseInputs(ctypes.Structure):
    """rt_denoise_inputs: color, normal and depth are required; albedo and object may be None / 0."""

    _fields_ = [
        ("color", ctypes.c_void_p),
        ("normal", ctypes.c_void_p),
        ("depth", ctypes.c_void_p),
        ("albedo", ctypes.c_void_p),
        ("object", ctypes.c_void_p),
    ]


class Temporal(ctypes.Structure):
    """rt_temporal: the parameters of temporal accumulation (default_temporal())."""

    _fields_ = [
        ("max_history", ctypes.c_double),
        ("depth_tol", ctypes.c_double),
        ("normal_min", ctypes.c_double),
        ("min_weight", ctypes.c_double),
    ]


class TemporalFrame(ctypes.Structure):
    """rt_temporal_frame: one frame's buffers (color and depth required; object and normal may be None / 0;
    count is read in the previous frame only) and the 12 doubles of rt_camera_frame for its camera."""

    _fields_ = [
        ("color", ctypes.c_void_p),
        ("depth", ctypes.c_void_p),
        ("object", ctypes.c_void_p),
        ("normal", ctypes.c_void_p),
        ("count", ctypes.c_void_p),
        ("frame", ctypes.c_double * 12),
    ]


class Motion(ctypes.Structure):
    """rt_motion: the per-object translations of rt_temporal_motion_async: ``motion`` points
    to num_objects rows of 3 doubles (a device pointer for the _async call)."""

    _fields_ = [
        ("motion", ctypes.c_void_p),
        ("num_objects", ctypes.c_int32),
        ("_pad", ctypes.c_int32),
    ]


class HistoryClip(ctypes.Structure):
    """rt_history_clip: the parameters of history rectification (default_history_clip())."""

    _fields_ = [
        ("radius", ctypes.c_int32),
        ("min_taps", ctypes.c_int32),
        ("gamma", ctypes.c_double),
        ("min_half", ctypes.c_double),
    ]


class Matte(ctypes.Structure):
    """rt_matte: the parameters of the matte pass (default_matte())."""

    _fields_ = [
        ("ranks", ctypes.c_int32),
        ("level", ctypes.c_int32),
    ]


class MatteBuffers(ctypes.Structure):
    """rt_matte_buffers: the device pointers of a matte pass (None / 0: not written); d_id and d_count are
    ``ranks`` planes of W*H int32, d_rest one."""

    _fields_ = [
        ("d_id", ctypes.c_void_p),
        ("d_count", ctypes.c_void_p),
        ("d_rest", ctypes.c_void_p),
    ]


class MatteResolve(ctypes.Structure):
    """rt_matte_resolve: the parameters of the edge resolve (default_matte_resolve())."""

    _fields_ = [
        ("radius", ctypes.c_int32),
        ("_pad", ctypes.c_int32),
        ("background", ctypes.c_double * 3),
    ]


class MatteResolveInputs(ctypes.Structure):
    """rt_matte_resolve_inputs: color, object, id and count are required; rest may be None / 0."""

    _fields_ = [
        ("color", ctypes.c_void_p),
        ("object", ctypes.c_void_p),
        ("id", ctypes.c_void_p),
        ("count", ctypes.c_void_p),
        ("rest", ctypes.c_void_p),
        ("ranks", ctypes.c_int32),
        ("samples", ctypes.c_int32),
    ]


RT_MATTE_SLOTS, RT_MATTE_MAX_RANKS = 16, 8
RT_MATTE_OBJECT, RT_MATTE_FACE = 0, 1
MATTE_LEVELS = {"object": RT_MATTE_OBJECT, "face": RT_MATTE_FACE}


class Variance(ctypes.Structure):
    """rt_variance: the parameters of the variance pass (default_variance())."""

    _fields_ = [
        ("min_history", ctypes.c_double),
        ("sigma_depth", ctypes.c_double),
        ("normal_power", ctypes.c_int32),
        ("_pad", ctypes.c_int32),
    ]


class VarianceInputs(ctypes.Structure):
    """rt_variance_inputs: color, normal and depth are required; albedo and object may be None / 0;
    moments and count are given both or neither."""

    _fields_ = [
        ("color", ctypes.c_void_p),
        ("normal", ctypes.c_void_p),
        ("depth", ctypes.c_void_p),
        ("albedo", ctypes.c_void_p),
        ("object", ctypes.c_void_p),
        ("moments", ctypes.c_void_p),
        ("count", ctypes.c_void_p),
    ]


class DenoiseVar(ctypes.Structure):
    """rt_denoise_var: the parameters of the variance-guided filter (default_denoise_var())."""

    _fields_ = [
        ("levels", ctypes.c_int32),
        ("normal_power", ctypes.c_int32),
        ("sigma_lum", ctypes.c_double),
        ("sigma_depth", ctypes.c_double),
        ("demodulate", ctypes.c_int32),
        ("prefilter", ctypes.c_int32),
    ]


class Counts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in COUNT_FIELDS] + [("culled", ctypes.c_uint64 * 9),
                                                               ("soft_occlusion", ctypes.c_uint64 * 9),
                                                               ("extend", ctypes.c_uint64 * 9),
                                                               ("hard_occlusion", ctypes.c_uint64 * 9)]

    def as_dict(self):
        """The nine counts (the reference's: every camera sample walked)."""
        return {n: int(getattr(self, n)) for n in COUNT_FIELDS}

    def culled_dict(self):
        """The part of each count the product never executes (culled pixels' camera samples)."""
        return {n: int(self.culled[i]) for i, n in enumerate(COUNT_FIELDS)}

    def soft_occlusion_dict(self):
        """The wavefront soft-shadow traversal kernel's share of the counts."""
        return {n: int(self.soft_occlusion[i]) for i, n in enumerate(COUNT_FIELDS)}

    def extend_dict(self):
        """The wavefront closest-hit traversal kernel's share of the counts."""
        return {n: int(self.extend[i]) for i, n in enumerate(COUNT_FIELDS)}

    def hard_occlusion_dict(self):
        """The wavefront hard-ray traversal kernel's share of the counts."""
        return {n: int(self.hard_occlusion[i]) for i, n in enumerate(COUNT_FIELDS)}

    def executed_dict(self):
        """Executed work: count - culled."""
        return {n: int(getattr(self, n)) - int(self.culled[i]) for i, n in enumerate(COUNT_FIELDS)}


# the symbols include/rt_api.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = [
    "rt_settings_default",
    "rt_abi_version",
    "rt_last_error",
    "rt_scene_load_json",
    "rt_scene_parse_json",
    "rt_scene_view",
    "rt_scene_warnings",
    "rt_scene_free",
    "rt_scene_print_hittables",
    "rt_render",
    "rt_validate",
    "rt_camera_frame",
    "rt_renderer_create",
    "rt_renderer_render",
    "rt_renderer_destroy",
    "rt_renderer_set_tuning",
    "rt_tuning_default",
    "rt_context_set_tuning",
    "rt_context_create",
    "rt_context_destroy",
    "rt_context_set_scene",
    "rt_num_tiles",
    "rt_tiles_for_rank",
    "rt_max_local_tiles",
    "rt_packed_bytes",
    "rt_packed_rgba_offset",
    "rt_context_render_async",
    "rt_unpack_tiles_async",
    "rt_comm_unique_id",
    "rt_comm_create",
    "rt_comm_destroy",
    "rt_comm_gather_tiles_async",
    "rt_context_last_kernel_seconds",
    "rt_context_set_debug_buffer",
    "rt_tonemap_rgba",
    "rt_write_png",
    "rt_write_ppm",
    "rt_partition_create",
    "rt_partition_balanced",
    "rt_partition_destroy",
    "rt_partition_world",
    "rt_partition_owner",
    "rt_partition_local_tiles",
    "rt_partition_tile",
    "rt_partition_max_local",
    "rt_partition_packed_bytes",
    "rt_partition_rgba_offset",
    "rt_partition_work",
    "rt_context_set_partition",
    "rt_unpack_partition_async",
    "rt_comm_gather_bytes_async",
    "rt_renderer_rank_seconds",
    "rt_renderer_num_ranks",
    "rt_debug_xlane_faults",
    "rt_context_tail_debug",
    "rt_context_profile",
    "rt_context_kernel_seconds",
    "rt_context_render_frames_async",
    "rt_unpack_partition_frames_async",
    "rt_release_cached_memory",
    "rt_renderer_set_watchdog",
    "rt_renderer_test_stall",
    "rt_context_get_stats",
    "rt_context_progressive_begin",
    "rt_context_progressive_add_async",
    "rt_context_progressive_samples",
    "rt_context_progressive_end",
    "rt_rgba_delta_async",
    "rt_context_progressive_set_adaptive",
    "rt_context_progressive_counts_async",
    "rt_context_progressive_state",
    "rt_adaptive_step",
    "rt_scene_cone_rows",
    "rt_context_render_cameras_async",
    "rt_camera_orbit",
    "rt_stream_decode",
    "rt_soft_screen",
    "rt_context_render_aov_async",
    "rt_aov_spec_default",
    "rt_aov_spec_follows",
    "rt_context_render_aov_spec_async",
    "rt_denoise_default",
    "rt_denoise_workspace_bytes",
    "rt_denoise_async",
    "rt_denoise_host",
    "rt_temporal_default",
    "rt_temporal_async",
    "rt_temporal_host",
    "rt_temporal_moments_async",
    "rt_temporal_moments_host",
    "rt_variance_default",
    "rt_variance_async",
    "rt_variance_host",
    "rt_denoise_var_default",
    "rt_denoise_var_workspace_bytes",
    "rt_denoise_var_async",
    "rt_denoise_var_host",
    "rt_temporal_motion_async",
    "rt_temporal_motion_host",
    "rt_scene_motion",
    "rt_history_clip_default",
    "rt_temporal_clip_async",
    "rt_temporal_clip_host",
    "rt_matte_default",
    "rt_context_render_matte_async",
    "rt_matte_resolve_default",
    "rt_matte_resolve_async",
    "rt_matte_resolve_host",
]

_lib = None


def lib():
    """Load librtgo.so (once) and declare the C signatures."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RenderError(
            f"{LIB_PATH} is missing: build it with `make -C concurrent-raytracer-go_amd` "
            "(or __graft_entry__.build())"
        )
    # One HIP runtime per process: torch bundles libamdhip64.so (soname
    # libamdhip64.so.7) and loads it by a path the dynamic loader cannot
    # match against an already-loaded /opt/rocm copy, so torch must come
    # first; librtgo's DT_NEEDED libamdhip64.so.7 then binds to torch's copy.
    if os.environ.get("RTGO_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_size_t
    sig = {
        "rt_settings_default": (None, [ctypes.POINTER(Settings)]),
        "rt_abi_version": (i32, []),
        "rt_last_error": (ctypes.c_char_p, []),
        "rt_scene_load_json": (ctypes.c_int, [ctypes.c_char_p, i32, ctypes.POINTER(vp)]),
        "rt_scene_parse_json": (ctypes.c_int, [ctypes.c_char_p, sz, i32, ctypes.POINTER(vp)]),
        "rt_scene_view": (ctypes.POINTER(SceneView), [vp]),
        "rt_scene_warnings": (i32, [vp]),
        "rt_scene_free": (None, [vp]),
        "rt_scene_print_hittables": (ctypes.c_int, [vp]),
        "rt_render": (
            ctypes.c_int,
            [ctypes.POINTER(SceneView), i32, i32, ctypes.POINTER(Settings), vp, vp, ctypes.POINTER(Stats)],
        ),
        "rt_validate": (ctypes.c_int, [ctypes.POINTER(SceneView), i32, i32, ctypes.POINTER(Settings)]),
        "rt_renderer_create": (ctypes.c_int, [ctypes.POINTER(i32), i32, ctypes.POINTER(vp)]),
        "rt_renderer_render": (
            ctypes.c_int,
            [vp, ctypes.POINTER(SceneView), i32, i32, ctypes.POINTER(Settings), vp, vp, ctypes.POINTER(Stats)],
        ),
        "rt_renderer_destroy": (None, [vp]),
        "rt_renderer_set_tuning": (ctypes.c_int, [vp, ctypes.POINTER(Tuning)]),
        "rt_tuning_default": (None, [ctypes.POINTER(Tuning)]),
        "rt_context_set_tuning": (ctypes.c_int, [vp, ctypes.POINTER(Tuning)]),
        "rt_max_local_tiles": (i32, [i32, i32, i32]),
        "rt_packed_bytes": (sz, [i32, i32, i32]),
        "rt_packed_rgba_offset": (sz, [i32, i32, i32]),
        "rt_comm_unique_id": (ctypes.c_int, [vp]),
        "rt_comm_create": (ctypes.c_int, [vp, i32, i32, i32, ctypes.POINTER(vp)]),
        "rt_comm_destroy": (None, [vp]),
        "rt_comm_gather_tiles_async": (ctypes.c_int, [vp, i32, i32, vp, vp, vp]),
        "rt_context_create": (ctypes.c_int, [i32, ctypes.POINTER(vp)]),
        "rt_context_destroy": (None, [vp]),
        "rt_context_set_scene": (ctypes.c_int, [vp, ctypes.POINTER(SceneView), i32]),
        "rt_num_tiles": (i32, [i32, i32]),
        "rt_tiles_for_rank": (i32, [i32, i32, i32, i32]),
        "rt_context_render_async": (
            ctypes.c_int,
            [vp, i32, i32, ctypes.POINTER(Settings), i32, i32, i32, vp, vp, vp, ctypes.POINTER(Counts)],
        ),
        "rt_unpack_tiles_async": (ctypes.c_int, [i32, i32, i32, vp, vp, vp, vp]),
        "rt_context_last_kernel_seconds": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double)]),
        "rt_context_set_debug_buffer": (ctypes.c_int, [vp, vp]),
        "rt_tonemap_rgba": (None, [vp, i32, vp]),
        "rt_write_png": (ctypes.c_int, [ctypes.c_char_p, vp, i32, i32]),
        "rt_write_ppm": (ctypes.c_int, [ctypes.c_char_p, vp, i32, i32]),
        "rt_partition_create": (ctypes.c_int, [i32, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(vp)]),
        "rt_partition_balanced": (ctypes.c_int, [vp, i32, i32, ctypes.POINTER(Settings), i32, ctypes.POINTER(vp)]),
        "rt_partition_destroy": (None, [vp]),
        "rt_partition_world": (i32, [vp]),
        "rt_partition_owner": (i32, [vp, i32]),
        "rt_partition_local_tiles": (i32, [vp, i32]),
        "rt_partition_tile": (i32, [vp, i32, i32]),
        "rt_partition_max_local": (i32, [vp]),
        "rt_partition_packed_bytes": (sz, [vp]),
        "rt_partition_rgba_offset": (sz, [vp]),
        "rt_partition_work": (ctypes.c_double, [vp, i32]),
        "rt_context_set_partition": (ctypes.c_int, [vp, vp]),
        "rt_unpack_partition_async": (ctypes.c_int, [vp, vp, vp, vp, vp]),
        "rt_comm_gather_bytes_async": (ctypes.c_int, [vp, sz, vp, vp, vp]),
        "rt_renderer_rank_seconds": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double), ctypes.c_int32]),
        "rt_renderer_num_ranks": (ctypes.c_int32, [vp]),
        "rt_debug_xlane_faults": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)]),
        "rt_context_tail_debug": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_uint64)]),
        "rt_context_profile": (ctypes.c_int, [vp, i32]),
        "rt_context_render_frames_async": (
            ctypes.c_int,
            [vp, i32, i32, ctypes.POINTER(Settings), i32, ctypes.POINTER(ctypes.c_uint64), i32, i32, i32,
             ctypes.POINTER(vp), ctypes.POINTER(vp), vp],
        ),
        "rt_unpack_partition_frames_async": (ctypes.c_int, [vp, i32, vp, vp, vp, vp]),
        "rt_release_cached_memory": (ctypes.c_int, []),
        "rt_renderer_set_watchdog": (ctypes.c_int, [vp, ctypes.c_double]),
        "rt_renderer_test_stall": (ctypes.c_int, [vp, i32, ctypes.c_double]),
        "rt_context_get_stats": (ctypes.c_int, [vp, ctypes.POINTER(ContextStats)]),
        "rt_context_kernel_seconds": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double),
                                                     ctypes.POINTER(ctypes.c_int64)]),
        "rt_context_progressive_begin": (ctypes.c_int, [vp, i32, i32, ctypes.POINTER(Settings), i32, i32, i32]),
        "rt_context_progressive_add_async": (ctypes.c_int, [vp, i32, vp, vp, vp]),
        "rt_context_progressive_samples": (ctypes.c_int64, [vp]),
        "rt_context_progressive_end": (ctypes.c_int, [vp]),
        "rt_rgba_delta_async": (ctypes.c_int, [vp, vp, sz, vp, vp]),
        "rt_context_progressive_set_adaptive": (ctypes.c_int, [vp, ctypes.POINTER(Adaptive)]),
        "rt_context_progressive_counts_async": (ctypes.c_int, [vp, vp, vp]),
        "rt_context_progressive_state": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int64)]),
        "rt_adaptive_step": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8), i32, i32,
                                             i32, ctypes.POINTER(Adaptive), ctypes.POINTER(i32)]),
        "rt_camera_frame": (ctypes.c_int, [ctypes.POINTER(Camera), i32, i32, i32, ctypes.POINTER(ctypes.c_double)]),
        "rt_scene_cone_rows": (ctypes.c_int, [ctypes.POINTER(SceneView), i32, ctypes.POINTER(ctypes.c_uint64), sz]),
        "rt_context_render_cameras_async": (
            ctypes.c_int,
            [vp, i32, i32, ctypes.POINTER(Settings), i32, ctypes.POINTER(Camera), ctypes.POINTER(ctypes.c_uint64), i32,
             i32, i32, ctypes.POINTER(vp), ctypes.POINTER(vp), vp],
        ),
        "rt_camera_orbit": (ctypes.c_int, [ctypes.POINTER(Camera), i32, ctypes.c_double, ctypes.POINTER(Camera)]),
        "rt_stream_decode": (ctypes.c_int, [i32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                             ctypes.POINTER(ctypes.c_uint32), sz, ctypes.POINTER(ctypes.c_uint32)]),
        "rt_soft_screen": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double)] * 7 + [sz, ctypes.POINTER(i32)]),
        "rt_context_render_aov_async": (ctypes.c_int, [vp, i32, i32, ctypes.POINTER(Settings), ctypes.POINTER(Camera),
                                                       ctypes.POINTER(AovBuffers), vp]),
        "rt_aov_spec_default": (None, [ctypes.POINTER(AovSpec)]),
        "rt_aov_spec_follows": (ctypes.c_int, [ctypes.POINTER(Material), ctypes.POINTER(AovSpec)]),
        "rt_context_render_aov_spec_async": (ctypes.c_int, [vp, i32, i32, ctypes.POINTER(Settings),
                                                            ctypes.POINTER(Camera), ctypes.POINTER(AovSpec),
                                                            ctypes.POINTER(AovSpecBuffers), vp]),
        "rt_denoise_default": (None, [ctypes.POINTER(Denoise)]),
        "rt_denoise_workspace_bytes": (sz, [i32, i32]),
        "rt_denoise_async": (ctypes.c_int, [ctypes.POINTER(Denoise), i32, i32, ctypes.POINTER(DenoiseInputs), vp, vp,
                                             vp, sz, vp]),
        "rt_denoise_host": (ctypes.c_int, [ctypes.POINTER(Denoise), i32, i32, ctypes.POINTER(DenoiseInputs), vp, vp]),
        "rt_temporal_default": (None, [ctypes.POINTER(Temporal)]),
        "rt_temporal_async": (ctypes.c_int, [ctypes.POINTER(Temporal), i32, i32, ctypes.POINTER(TemporalFrame),
                                              ctypes.POINTER(TemporalFrame), vp, vp, vp, vp]),
        "rt_temporal_host": (ctypes.c_int, [ctypes.POINTER(Temporal), i32, i32, ctypes.POINTER(TemporalFrame),
                                             ctypes.POINTER(TemporalFrame), vp, vp, vp]),
        "rt_temporal_moments_async": (ctypes.c_int, [ctypes.POINTER(Temporal), i32, i32, ctypes.POINTER(TemporalFrame),
                                                      ctypes.POINTER(TemporalFrame), vp, vp, vp, vp, vp, vp, vp]),
        "rt_temporal_moments_host": (ctypes.c_int, [ctypes.POINTER(Temporal), i32, i32, ctypes.POINTER(TemporalFrame),
                                                     ctypes.POINTER(TemporalFrame), vp, vp, vp, vp, vp, vp]),
        "rt_variance_default": (None, [ctypes.POINTER(Variance)]),
        "rt_variance_async": (ctypes.c_int, [ctypes.POINTER(Variance), i32, i32, ctypes.POINTER(VarianceInputs), vp, vp]),
        "rt_variance_host": (ctypes.c_int, [ctypes.POINTER(Variance), i32, i32, ctypes.POINTER(VarianceInputs), vp]),
        "rt_denoise_var_default": (None, [ctypes.POINTER(DenoiseVar)]),
        "rt_denoise_var_workspace_bytes": (sz, [i32, i32]),
        "rt_denoise_var_async": (ctypes.c_int, [ctypes.POINTER(DenoiseVar), i32, i32, ctypes.POINTER(DenoiseInputs), vp,
                                                 vp, vp, vp, vp, sz, vp]),
        "rt_denoise_var_host": (ctypes.c_int, [ctypes.POINTER(DenoiseVar), i32, i32, ctypes.POINTER(DenoiseInputs), vp,
                                                vp, vp, vp]),
        "rt_temporal_motion_async": (ctypes.c_int, [ctypes.POINTER(Temporal), i32, i32, ctypes.POINTER(TemporalFrame),
                                                     ctypes.POINTER(TemporalFrame), ctypes.POINTER(Motion), vp, vp, vp,
                                                     vp, vp, vp, vp]),
        "rt_temporal_motion_host": (ctypes.c_int, [ctypes.POINTER(Temporal), i32, i32, ctypes.POINTER(TemporalFrame),
                                                    ctypes.POINTER(TemporalFrame), ctypes.POINTER(Motion), vp, vp, vp,
                                                    vp, vp, vp]),
        "rt_scene_motion": (ctypes.c_int, [ctypes.POINTER(SceneView), ctypes.POINTER(SceneView),
                                            ctypes.POINTER(ctypes.c_double), sz]),
        "rt_history_clip_default": (None, [ctypes.POINTER(HistoryClip)]),
        "rt_temporal_clip_async": (ctypes.c_int, [ctypes.POINTER(Temporal), i32, i32, ctypes.POINTER(TemporalFrame),
                                                   ctypes.POINTER(TemporalFrame), ctypes.POINTER(Motion),
                                                   ctypes.POINTER(HistoryClip), vp, vp, vp, vp, vp, vp, vp, vp]),
        "rt_temporal_clip_host": (ctypes.c_int, [ctypes.POINTER(Temporal), i32, i32, ctypes.POINTER(TemporalFrame),
                                                  ctypes.POINTER(TemporalFrame), ctypes.POINTER(Motion),
                                                  ctypes.POINTER(HistoryClip), vp, vp, vp, vp, vp, vp, vp]),
        "rt_matte_default": (None, [ctypes.POINTER(Matte)]),
        "rt_context_render_matte_async": (ctypes.c_int, [vp, i32, i32, ctypes.POINTER(Settings), ctypes.POINTER(Camera),
                                                         ctypes.POINTER(Matte), ctypes.POINTER(MatteBuffers), vp]),
        "rt_matte_resolve_default": (None, [ctypes.POINTER(MatteResolve)]),
        "rt_matte_resolve_async": (ctypes.c_int, [ctypes.POINTER(MatteResolve), i32, i32,
                                                   ctypes.POINTER(MatteResolveInputs), vp, vp, vp]),
        "rt_matte_resolve_host": (ctypes.c_int, [ctypes.POINTER(MatteResolve), i32, i32,
                                                  ctypes.POINTER(MatteResolveInputs), vp, vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def _check(rc):
    if rc != RT_OK:
        msg = lib().rt_last_error()
        raise RenderError(f"librtgo error {rc}: {msg.decode() if msg else ''}")


def default_settings() -> Settings:
    s = Settings()
    lib().rt_settings_default(ctypes.byref(s))
    return s


def default_tuning(**over) -> Tuning:
    t = Tuning()
    lib().rt_tuning_default(ctypes.byref(t))
    for k, v in over.items():
        setattr(t, k, v)
    return t


# --------------------------------------------------------------- scene
class Scene:
    """A loaded scene (scene.Scene, internal/scene/scene.go:12-16)."""

    def __init__(self, handle=None, objects=None, lights=None, camera=None):
        self._handle = handle
        if handle is not None:
            self._view = lib().rt_scene_view(handle).contents
        else:
            self._objects = (Object * max(1, len(objects)))(*objects)
            self._lights = (Light * max(1, len(lights)))(*lights)
            v = SceneView()
            v.camera = camera
            v.objects = ctypes.cast(self._objects, ctypes.POINTER(Object))
            v.num_objects = len(objects)
            v.lights = ctypes.cast(self._lights, ctypes.POINTER(Light))
            v.num_lights = len(lights)
            self._view = v

    @classmethod
    def load_from_file(cls, path: str) -> "Scene":
        """scene.LoadFromFile (scene.go:45-57)."""
        h = ctypes.c_void_p()
        _check(lib().rt_scene_load_json(path.encode(), 0, ctypes.byref(h)))
        return cls(handle=h)

    @classmethod
    def from_json_text(cls, text: str) -> "Scene":
        h = ctypes.c_void_p()
        b = text.encode()
        _check(lib().rt_scene_parse_json(b, len(b), 0, ctypes.byref(h)))
        return cls(handle=h)

    @classmethod
    def from_python(cls, camera: dict, objects: list, lights: list) -> "Scene":
        """Build a scene from already-decoded values (loader defaults applied)."""
        cam = Camera()
        cam.position[:] = camera.get("position", (0, 0, 0))
        cam.look_at[:] = camera.get("lookAt", (0, 0, 0))
        cam.up[:] = camera.get("up", (0, 0, 0))
        cam.fov = camera.get("fov", 0.0)
        cam.aspect_ratio = camera.get("aspectRatio", 0.0)
        objs = []
        for o in objects:
            ob = Object()
            ob.type = RT_OBJ_SPHERE if o["type"] == "sphere" else RT_OBJ_CUBE
            ob.position[:] = o.get("position", (0, 0, 0))
            ob.size[:] = o.get("size", (0, 0, 0))
            ob.radius = o.get("radius", 0.0)
            # the fields each material kind reads, with scene.go:104-148's defaults
            m = o["material"]
            t = m["type"] if m["type"] in MATERIAL_KINDS else "lambertian"
            ob.material.kind = MATERIAL_KINDS[t]
            if t != "dielectric":
                ob.material.color[:] = m.get("color", (0, 0, 0))
            if t in ("metal", "shiny", "perfectmirror"):
                ob.material.roughness = m.get("roughness", 0.0)
            if t in ("metal", "shiny"):
                ob.material.metallic = m.get("metallic", 1.0 if t == "metal" else 0.0)
                ob.material.specular = m.get("specular", 1.0)
            if t in ("glass", "dielectric"):
                ob.material.refraction_index = m.get("refractionIndex", 1.5)
            objs.append(ob)
        ls = []
        for l in lights:
            li = Light()
            li.position[:] = l["position"]
            li.color[:] = l.get("color", (0, 0, 0))
            li.intensity = l.get("intensity", 0.0)
            ls.append(li)
        return cls(objects=objs, lights=ls, camera=cam)

    @property
    def view(self) -> SceneView:
        return self._view

    @property
    def num_objects(self) -> int:
        return self._view.num_objects

    @property
    def warnings(self) -> int:
        return lib().rt_scene_warnings(self._handle) if self._handle is not None else 0

    def translated(self, offsets) -> "Scene":
        """A copy of the scene with object k moved by offsets[k] (a (num_objects, 3) array):
        position + offset in binary64, everything else as it is."""
        n = self.num_objects
        off = np.asarray(offsets, np.float64)
        if off.shape != (n, 3) or not np.isfinite(off).all():
            raise RenderError(f"Scene.translated: offsets are a finite ({n}, 3) array, one row per object")
        objs = []
        for k in range(n):
            ob = Object.from_buffer_copy(self._view.objects[k])
            for j in range(3):
                ob.position[j] = ob.position[j] + float(off[k, j])
            objs.append(ob)
        lights = [Light.from_buffer_copy(self._view.lights[k]) for k in range(self._view.num_lights)]
        return Scene(objects=objs, lights=lights, camera=Camera.from_buffer_copy(self._view.camera))

    def relit(self, light_offsets) -> "Scene":
        """A copy of the scene with light i moved by light_offsets[i] (a (num_lights, 3) array; DESIGN.md
        §4.18): position + offset in binary64, everything else as it is."""
        n = int(self._view.num_lights)
        off = np.asarray(light_offsets, np.float64)
        if off.shape != (n, 3) or not np.isfinite(off).all():
            raise RenderError(f"Scene.relit: light_offsets are a finite ({n}, 3) array, one row per light")
        objs = [Object.from_buffer_copy(self._view.objects[k]) for k in range(self.num_objects)]
        lights = []
        for i in range(n):
            lt = Light.from_buffer_copy(self._view.lights[i])
            for j in range(3):
                lt.position[j] = lt.position[j] + float(off[i, j])
            lights.append(lt)
        return Scene(objects=objs, lights=lights, camera=Camera.from_buffer_copy(self._view.camera))

    def print_hittables(self):
        if self._handle is not None:
            lib().rt_scene_print_hittables(self._handle)

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and _lib is not None:
            _lib.rt_scene_free(h)
            self._handle = None


# --------------------------------------------------------------- renderer
class ParallelRenderer:
    """renderer.ParallelRenderer (renderer.go:20-29) backed by the GPU kernel."""

    FEATURES = [
        "Improved metallic reflections with Fresnel effect",
        "Shiny materials with configurable roughness and specular",
        "Enhanced light source reflections",
        "Better specular highlights for metallic surfaces",
    ]

    def __init__(self, num_workers: int = 1, num_devices: int = 1, devices=None):
        """devices: the device of each rank (default 0..num_devices-1; a
        device may repeat: its ranks share it)."""
        self.settings = default_settings()  # NewParallelRenderer defaults, renderer.go:54-65
        self.settings.num_workers = num_workers
        self.settings.num_devices = len(devices) if devices else num_devices
        self.devices = list(devices) if devices else None
        self.benchmark_data: dict = {}
        self.last_linear = None
        self.last_stats = None
        self._r = None  # the rt_renderer (made by the first render, kept like the Go object)
        self._tuning = None
        self.last_samples = None  # samples per pixel of the last render_progressive
        self._prog_ctx = None  # its Context (made by the first call, kept)
        self.last_sample_counts = None  # per-pixel samples of the last render_progressive (H x W)
        self.last_progressive_state = None  # Context.progressive_state() at its end
        self.last_denoised_linear = None  # the filter's linear output of the last denoised render (H x W x 3)
        self.last_temporal_linear = None  # render_sequence(temporal=...): the accumulated frames (n x H x W x 3)
        self.last_history = None  # ... and each pixel's history length (n x H x W)
        self.last_variance = None  # variance=...: the variance pass's output (n x H x W, or H x W of render_denoised)
        self.last_clipped = None  # render_sequence(clip=...): 1 where the history was clipped (n x H x W)
        self.last_resolved_linear = None  # matte=...: the edge-resolved image

    def set_tuning(self, tuning: Tuning):
        self._tuning = tuning
        if self._r is not None:
            _check(lib().rt_renderer_set_tuning(self._r, ctypes.byref(tuning)))

    def _renderer(self):
        if self._r is None:
            h = ctypes.c_void_p()
            if self.devices:
                devs = (ctypes.c_int32 * len(self.devices))(*self.devices)
                _check(lib().rt_renderer_create(devs, len(self.devices), ctypes.byref(h)))
            else:
                _check(lib().rt_renderer_create(None, max(1, self.settings.num_devices), ctypes.byref(h)))
            self._r = h
            if self._tuning is not None:
                _check(lib().rt_renderer_set_tuning(self._r, ctypes.byref(self._tuning)))
        return self._r

    def close(self):
        if self._r is not None and _lib is not None:
            _lib.rt_renderer_destroy(self._r)
        self._r = None
        if getattr(self, "_prog_ctx", None) is not None and _lib is not None:
            self._prog_ctx.close()
        self._prog_ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_watchdog(self, seconds: float):
        """rt_renderer_set_watchdog: bound a multi-rank Render's wait (RT_E_TIMEOUT after `seconds`)."""
        _check(lib().rt_renderer_set_watchdog(self._renderer(), float(seconds)))

    def test_stall(self, rank: int, ms: float):
        """rt_renderer_test_stall (test hook): the next multi-rank frame's rank first sleeps `ms` on the GPU."""
        _check(lib().rt_renderer_test_stall(self._renderer(), rank, float(ms)))

    # settings.go:3-25
    def set_samples(self, samples: int):
        self.settings.samples = samples

    def set_max_depth(self, max_depth: int):
        self.settings.max_depth = max_depth

    def set_anti_aliasing(self, on: bool):
        self.settings.anti_aliasing = int(on)

    def set_recursive_reflections(self, on: bool):
        self.settings.recursive_reflections = int(on)

    def set_soft_shadows(self, on: bool):
        self.settings.soft_shadows = int(on)

    def set_depth_of_field(self, on: bool):
        self.settings.depth_of_field = int(on)

    def set_seed(self, seed: int):
        self.settings.seed = seed

    def set_sky(self, sky: str):
        """Opt-in sky on miss (atmosphere.go presets); "none" = black, the reference."""
        self.settings.sky = SKIES[sky]

    def set_camera(self, model: str):
        """Camera model: "reference" (getRay's fixed -Z, 90-degree view, the default) or
        "lookat" (opt-in: the scene's own position, lookAt, up and fov; rt_camera_frame)."""
        self.settings.camera = CAMERAS[model]

    def get_stats(self) -> dict:  # settings.go:27-36
        s = self.settings
        return {
            "workers": s.num_workers,
            "samples": s.samples,
            "maxDepth": s.max_depth,
            "antiAliasing": bool(s.anti_aliasing),
            "recursiveReflections": bool(s.recursive_reflections),
            "softShadows": bool(s.soft_shadows),
            "depthOfField": bool(s.depth_of_field),
        }

    def render(self, scene: Scene, width: int, height: int, keep_linear: bool = True) -> np.ndarray:
        """Render (renderer.go:67-126): returns an (H, W, 4) uint8 RGBA image.

        The mean linear radiance (before tone mapping) is kept in
        ``self.last_linear`` as an (H, W, 3) float32 array; keep_linear=False
        skips it (None), as Go's Render returns the RGBA image only.
        """
        _check(lib().rt_validate(ctypes.byref(scene.view), width, height, ctypes.byref(self.settings)))
        lin = np.zeros((height, width, 3), np.float32) if keep_linear else None
        rgba = np.zeros((height, width, 4), np.uint8)
        st = Stats()
        _check(
            lib().rt_renderer_render(
                self._renderer(),
                ctypes.byref(scene.view),
                width,
                height,
                ctypes.byref(self.settings),
                lin.ctypes.data if lin is not None else None,
                rgba.ctypes.data,
                ctypes.byref(st),
            )
        )
        self.last_linear = lin
        self.last_stats = st
        self.benchmark_data = {
            "scene_name": "demo_scene",
            "resolution": f"{width}x{height}",
            "render_time_seconds": st.render_seconds,
            "samples": self.settings.samples,
            "max_depth": self.settings.max_depth,
            "num_workers": self.settings.num_workers,
            "objects": st.objects,
            "lights": st.lights,
            "timestamp": datetime.now(timezone.utc).isoformat(),
            "features": list(self.FEATURES),
            "kernel_time_seconds": st.kernel_seconds,
            "pixels_per_second": st.pixels_per_second,
            "rays_per_second": st.rays_per_second,
        }
        return rgba

    def render_progressive(self, scene: Scene, width: int, height: int, pass_samples: int, time_budget=None,
                           until_changed_pixels=None, on_pass=None, adaptive=None, denoise=None, guide="first",
                           specular=None, matte=None) -> np.ndarray:
        """Render the frame ``pass_samples`` samples at a time, on one device.

        ``self.settings.samples`` is the cap; the last pass is clipped to it.
        After each pass ``on_pass(samples_done, rgba, changed_pixels)`` is
        called with the (H, W, 4) uint8 image of the samples so far and the
        number of pixels that differ from the previous pass's image (None for
        the first pass).  Stops after the first pass at which the cap is
        reached, the wall time since the call began is >= ``time_budget``
        (seconds), or ``changed_pixels <= until_changed_pixels``.  The image
        after n samples is that of ``render`` with samples = n, byte for byte.
        Returns the last image; ``last_linear`` holds its linear radiance and
        ``last_samples`` the samples rendered.

        ``adaptive``: None, or a dict with ``tolerance`` and
        optionally ``patience`` (1) and ``min_samples`` (0): every pixel stops
        on its own (Context.progressive_set_adaptive), and the progression
        also stops once no pixel is active.  Pixel p of the image is then that
        of ``render`` with samples = ``last_sample_counts[p]``.  In every mode
        ``last_sample_counts`` (H x W uint32) and ``last_progressive_state``
        (Context.progressive_state) are set.

        ``denoise``: None, or the filter's parameters (a Denoise, a dict of its fields,
        True for the defaults).  The first-hit feature buffers are rendered once before the first pass,
        with min(cap, pass_samples) samples; every pass's image is then denoised, ``on_pass`` receives the
        denoised preview and the denoised last image is returned, its linear radiance in
        ``last_denoised_linear``.  ``changed_pixels`` and every stop rule still read the raw images, and
        ``last_linear`` and ``last_sample_counts`` stay those of the raw progression.
        ``guide`` ("first" or "specular", with ``specular`` the pass's parameters; §4.16) picks the feature
        pass as in ``render_denoised``.

        ``matte`` (only with ``denoise``; True, a number of matte samples or a dict as in
        ``render_denoised``): the matte is rendered once before the first pass, every pass's denoised image
        goes through the edge resolve as the last step, ``on_pass`` receives and the call returns the
        resolved image, and ``last_resolved_linear`` holds the last one's linear radiance.
        """
        t0 = time.perf_counter()
        if (len(self.devices) if self.devices else max(1, self.settings.num_devices)) > 1:
            raise RenderError("render_progressive renders on one device (multi-GPU progressions are not supported)")
        cap = int(self.settings.samples)
        if pass_samples < 1 or cap < 1:
            raise RenderError("render_progressive: pass_samples and settings.samples must be >= 1")
        _check(lib().rt_validate(ctypes.byref(scene.view), width, height, ctypes.byref(self.settings)))
        dn = _as_denoise(denoise) if denoise is not None else None
        spec = _as_guide(guide, specular)
        if spec is not None and dn is None:
            raise RenderError('render_progressive: guide="specular" guides the denoiser and needs denoise')
        mopt = _as_matte_option(matte, "render_progressive")
        if mopt is not None and dn is None:
            raise RenderError("render_progressive: matte resolves the denoised preview and needs denoise")
        import torch

        dev = self.devices[0] if self.devices else 0
        if self._prog_ctx is None:  # (a context of its own, kept like the rt_renderer)
            self._prog_ctx = Context(dev)
        ctx = self._prog_ctx
        if self._tuning is not None:
            ctx.set_tuning(self._tuning)
        ctx.set_scene(scene)
        npix = width * height
        with torch.cuda.device(dev):
            lin = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
            bufs = [torch.zeros(npix * 4, dtype=torch.uint8, device="cuda") for _ in range(2)]
            delta = torch.zeros(2, dtype=torch.int32, device="cuda")
            counts = torch.zeros(npix, dtype=torch.int32, device="cuda")
            if dn is not None:  # the feature buffers, once: the first pass's samples of the same frame
                feat, work, nbytes, out_lin, out_rgba = self._denoise_buffers(npix, width, height)
                fst = Settings.from_buffer_copy(self.settings)
                fst.samples = min(cap, int(pass_samples))
                self._guide_pass(ctx, width, height, fst, feat, None, spec)
                if mopt is not None:
                    mt = self._matte_pass(ctx, width, height, fst, mopt,
                                          feat["object"].data_ptr() if spec is None else None)
            ctx.progressive_begin(width, height, self.settings)
            if adaptive is not None:
                ctx.progressive_set_adaptive(adaptive["tolerance"], adaptive.get("patience", 1),
                                             adaptive.get("min_samples", 0))
            done, k, img, state = 0, 0, None, None
            try:
                while True:
                    n = min(int(pass_samples), cap - done)
                    cur, prev = bufs[k & 1], bufs[(k & 1) ^ 1]
                    ctx.progressive_add(n, lin.data_ptr(), cur.data_ptr(), 0)
                    if k > 0:  # how much the preview still moved in this pass
                        rgba_delta_async(prev.data_ptr(), cur.data_ptr(), npix, delta.data_ptr(), 0)
                    if dn is not None:  # (reads the raw image, writes buffers of its own)
                        denoise_async(width, height, lin.data_ptr(), feat["normal"].data_ptr(),
                                      feat["depth"].data_ptr(), feat["albedo"].data_ptr(), feat["object"].data_ptr(),
                                      out_lin.data_ptr(), out_rgba.data_ptr(), work.data_ptr(), nbytes, dn, 0)
                        if mopt is not None:
                            self._matte_apply(width, height, mopt, mt, out_lin.data_ptr())
                    torch.cuda.synchronize()
                    done += n
                    shown = mt["rgba"] if mopt is not None else (out_rgba if dn is not None else cur)
                    img = shown.cpu().numpy().reshape(height, width, 4)
                    changed = int(delta[0].item()) & 0xFFFFFFFF if k > 0 else None
                    if on_pass is not None:
                        on_pass(done, img, changed)
                    k += 1
                    if adaptive is not None:
                        state = ctx.progressive_state()
                        if state["active"] == 0:
                            break
                    if done >= cap:
                        break
                    if time_budget is not None and time.perf_counter() - t0 >= time_budget:
                        break
                    if until_changed_pixels is not None and changed is not None and changed <= until_changed_pixels:
                        break
                state = ctx.progressive_state()
                ctx.progressive_counts(counts.data_ptr(), 0)
                torch.cuda.synchronize()
            finally:
                ctx.progressive_end()
            self.last_linear = lin.cpu().numpy().reshape(height, width, 3)
            if dn is not None:
                self.last_denoised_linear = out_lin.cpu().numpy().reshape(height, width, 3)
            if mopt is not None:
                self.last_resolved_linear = mt["linear"].cpu().numpy().reshape(height, width, 3)
            self.last_sample_counts = counts.cpu().numpy().view(np.uint32).reshape(height, width)
        self.last_progressive_state = state
        self.last_samples = done
        self.benchmark_data = {
            "scene_name": "demo_scene",
            "resolution": f"{width}x{height}",
            "render_time_seconds": time.perf_counter() - t0,
            "samples": done,
            "max_depth": self.settings.max_depth,
            "num_workers": self.settings.num_workers,
            "timestamp": datetime.now(timezone.utc).isoformat(),
            "features": list(self.FEATURES),
            "passes": k,
            "mean_samples_per_pixel": state["samples"] / max(1, state["pixels"]),
        }
        return img

    def render_sequence(self, scene: Scene, width: int, height: int, cameras, seeds=None, temporal=None,
                        denoise=None, variance=None, guide="first", specular=None, offsets=None, clip=None,
                        light_offsets=None, matte=None) -> np.ndarray:
        """The scene from each of ``cameras`` (Camera structs or scene-file camera dicts; any number):
        an (n, H, W, 4) uint8 array, frame f that of ``render`` with the scene's camera replaced by
        cameras[f] and seed seeds[f] (None: the renderer's seed), byte for byte.
        On one device, with a context of its own, in launches of at most RT_MAX_FRAMES frames
        (Context.render_cameras_async).  ``last_linear`` becomes (n, H, W, 3) float32.

        temporal (True, a dict of Temporal's fields or a Temporal): the frames render as
        above, each gets a feature pass with its own camera, seed and samples, and they are accumulated in
        order on the device (rt_temporal_async: frame f's history is frame f - 1's result; the feature
        buffers ping-pong).  The returned frames are the ACCUMULATED ones; ``last_linear`` stays the raw
        renders, ``last_temporal_linear`` is (n, H, W, 3) float32 and ``last_history`` (n, H, W) float32
        (each pixel's history length).  With seeds None, frame f then takes seed settings.seed + f: the same
        seed for every frame would repeat the same screen-locked noise, which accumulation cannot remove.

        denoise (True, a dict or a Denoise; §4.13; only together with ``temporal``, as the CLI's --denoise
        with --orbit): frame f's returned image is rt_denoise_async of its accumulated colour with its own
        features; what is fed back to the next frame is the unfiltered accumulation.
        ``last_denoised_linear`` is (n, H, W, 3).  A call without ``temporal`` / ``denoise`` sets the
        attributes of what it did not compute to None.

        variance (True, or a dict of DenoiseVar's and Variance's fields; §4.15; only together with
        ``temporal`` and instead of ``denoise``, as the CLI's --denoise-variance): the accumulation also
        carries the luminance moments (rt_temporal_moments_async, the unfiltered accumulation and moments
        are fed back), rt_variance_async turns them into each frame's variance and frame f's returned image
        is rt_denoise_var_async of its accumulated colour.  ``last_variance`` is (n, H, W) float32,
        ``last_denoised_linear`` (n, H, W, 3).

        guide ("first" or "specular", with ``specular`` the pass's parameters; §4.16; only together with
        ``denoise`` or ``variance``): "specular" guides the SPATIAL filter (rt_denoise_async, or
        rt_variance_async and rt_denoise_var_async) by the specular-through buffers of each frame.  The
        accumulation keeps the first-hit buffers: reprojection needs the geometric depth and the camera.

        offsets (an (n, num_objects, 3) array; §4.17): frame f is the scene with object k moved by
        offsets[f][k] (Scene.translated), byte for byte ``render`` of that moved scene with cameras[f] and
        seeds[f].  The frames then render one by one, each after rt_context_set_scene of its own scene, and
        the feature passes use the same scene.  With ``temporal`` the accumulation is
        rt_temporal_motion_async with scene_motion(frame f - 1's scene, frame f's) as its table, so that a
        moving object keeps its history; ``denoise``, ``variance`` and ``guide`` compose as above.  Without
        ``offsets`` the method and its launches are what they were.

        clip ("default" / True, a dict of HistoryClip's fields or a HistoryClip; §4.18; only together with
        ``temporal``, with or without ``offsets``): the accumulation is rt_temporal_clip_async, which clips
        each pixel's reprojected history to what the current frame's neighbourhood allows, demodulated by the
        frame's albedo.  ``last_clipped`` is (n, H, W) float32, 1 where a channel was clipped.  It composes
        with ``denoise``, ``variance`` and ``guide``.  With clip None nothing changes.

        light_offsets (an (n, num_lights, 3) array; §4.18): frame f is the scene with light i moved by
        light_offsets[f][i] (Scene.relit), rendered one by one as with ``offsets``, with which it composes.
        Lights are not part of the motion table: a moving light is what ``clip`` is for.

        matte (True, a number of matte samples or a dict as in ``render_denoised``; §4.19; only together with
        ``temporal``): each frame gets an object-level matte with its own camera, seed and scene, and the
        frame that is SHOWN -- the filtered one with ``denoise`` or ``variance``, else the accumulated one --
        goes through rt_matte_resolve_async as the last step.  The resolved frame is returned but never fed
        back: the history stays the unfiltered accumulation.  ``last_resolved_linear`` is (n, H, W, 3)
        float32.  With matte None nothing changes."""
        t0 = time.perf_counter()
        mopt = _as_matte_option(matte, "render_sequence")
        if mopt is not None and (temporal is None or temporal is False):
            raise RenderError("render_sequence: matte resolves the accumulated frames and needs temporal")
        hc = None if clip is None or clip is False else _as_history_clip(clip)
        if hc is not None and (temporal is None or temporal is False):
            raise RenderError("render_sequence: clip rectifies the accumulated history and needs temporal")
        spec = _as_guide(guide, specular)
        tp = None if temporal is None or temporal is False else _as_temporal(temporal)
        dn = None if denoise is None or denoise is False else _as_denoise(denoise)
        vg = None if variance is None or variance is False else _as_variance(variance)
        if dn is not None and tp is None:
            raise RenderError("render_sequence: denoise filters the accumulated frames and needs temporal")
        if vg is not None and tp is None:
            raise RenderError("render_sequence: variance is estimated from the accumulated frames and needs temporal")
        if vg is not None and dn is not None:
            raise RenderError("render_sequence: variance and denoise are two filters for the same frames: give one")
        if spec is not None and dn is None and vg is None:
            raise RenderError('render_sequence: guide="specular" guides the spatial filter and needs denoise or variance')
        if tp is not None and int(self.settings.samples) < 1:
            raise RenderError("render_sequence: temporal needs settings.samples >= 1")
        if (len(self.devices) if self.devices else max(1, self.settings.num_devices)) > 1:
            raise RenderError("render_sequence renders on one device (sequences over several GPUs are not supported)")
        cams = [_as_camera(c) for c in cameras]
        n = len(cams)
        if n < 1:
            raise RenderError("render_sequence: at least one camera is needed")
        if seeds is not None and len(seeds) != n:
            raise RenderError(f"render_sequence: {len(seeds)} seeds for {n} cameras")
        if seeds is None and tp is not None:
            seeds = [(int(self.settings.seed) + f) & (2 ** 64 - 1) for f in range(n)]
        scenes = None
        if light_offsets is not None:
            loff = np.asarray(light_offsets, np.float64)
            if loff.shape != (n, int(scene.view.num_lights), 3) or not np.isfinite(loff).all():
                raise RenderError(f"render_sequence: light_offsets have shape {loff.shape}, expected a finite "
                                  f"({n}, {int(scene.view.num_lights)}, 3) array: one row per frame and light")
        if offsets is not None:
            off = np.asarray(offsets, np.float64)
            if off.shape != (n, scene.num_objects, 3):
                raise RenderError(f"render_sequence: offsets have shape {off.shape}, expected "
                                  f"({n}, {scene.num_objects}, 3): one row per frame and object")
        if light_offsets is not None and offsets is None:
            off = np.zeros((n, scene.num_objects, 3), np.float64)
        if offsets is not None or light_offsets is not None:
            scenes = [scene.translated(off[f]) for f in range(n)]
            if light_offsets is not None:
                scenes = [scenes[f].relit(loff[f]) for f in range(n)]
            tables = [np.zeros((max(1, scene.num_objects), 3), np.float64)]  # (frame 0 starts the history)
            tables += [scene_motion(scenes[f - 1], scenes[f]) if scene.num_objects > 0 else tables[0]
                       for f in range(1, n)]
            if tp is not None and scene.num_objects < 1:
                raise RenderError("render_sequence: offsets with temporal need a scene with objects")
        for s in (scenes if scenes is not None else [scene]):
            _check(lib().rt_validate(ctypes.byref(s.view), width, height, ctypes.byref(self.settings)))
        import torch

        dev = self.devices[0] if self.devices else 0
        if self._prog_ctx is None:  # (the context render_progressive uses, kept like the rt_renderer)
            self._prog_ctx = Context(dev)
        ctx = self._prog_ctx
        if self._tuning is not None:
            ctx.set_tuning(self._tuning)
        if scenes is None:
            ctx.set_scene(scene)
        npix = width * height
        with torch.cuda.device(dev):
            lin = torch.zeros((n, npix * 3), dtype=torch.float32, device="cuda")
            rgba = torch.zeros((n, npix * 4), dtype=torch.uint8, device="cuda")
            for f in range(n) if scenes is not None else ():  # moved frames: one scene and one launch each
                ctx.set_scene(scenes[f])
                ctx.render_cameras_async(width, height, self.settings, [cams[f]], [lin[f].data_ptr()],
                                         [rgba[f].data_ptr()], seeds=None if seeds is None else [int(seeds[f])],
                                         stream=0)
            for f0 in range(0, n, RT_MAX_FRAMES) if scenes is None else ():
                f1 = min(n, f0 + RT_MAX_FRAMES)
                ctx.render_cameras_async(width, height, self.settings, cams[f0:f1],
                                         [lin[f].data_ptr() for f in range(f0, f1)],
                                         [rgba[f].data_ptr() for f in range(f0, f1)],
                                         seeds=None if seeds is None else [int(s) for s in seeds[f0:f1]], stream=0)
            if tp is not None:
                # per frame: its features, the accumulation into its own slot (frame f - 1's slot is the
                # history, so no output is ever the buffer the taps read), the filter over the result
                feat = [{k: torch.zeros(npix * (3 if k in ("albedo", "normal") else 1),
                                        dtype=torch.int32 if k == "object" else torch.float32, device="cuda")
                         for k in ("albedo", "normal", "depth", "object")} for _ in range(2)]
                acc = torch.zeros((n, npix * 3), dtype=torch.float32, device="cuda")
                cnt = torch.zeros((n, npix), dtype=torch.float32, device="cuda")
                if dn is not None:
                    nbytes = denoise_workspace_bytes(width, height)
                    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
                    dlin = torch.zeros((n, npix * 3), dtype=torch.float32, device="cuda")
                if vg is not None:
                    nbytes = denoise_var_workspace_bytes(width, height)
                    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
                    dlin = torch.zeros((n, npix * 3), dtype=torch.float32, device="cuda")
                    mom = torch.zeros((n, npix * 2), dtype=torch.float32, device="cuda")
                    var = torch.zeros((n, npix), dtype=torch.float32, device="cuda")
                if hc is not None:
                    clp = torch.zeros((n, npix), dtype=torch.float32, device="cuda")
                if spec is not None:  # the spatial filter's guide; the accumulation keeps the first hits
                    sg = {k: torch.zeros_like(v) for k, v in feat[0].items()}
                fst = Settings.from_buffer_copy(self.settings)
                if mopt is not None:  # one matte's buffers, reused frame by frame on the one stream
                    mid, mcn = (torch.zeros(mopt[1] * npix, dtype=torch.int32, device="cuda") for _ in range(2))
                    mre = torch.zeros(npix, dtype=torch.int32, device="cuda")
                    rlin = torch.zeros((n, npix * 3), dtype=torch.float32, device="cuda")
                    mst = Settings.from_buffer_copy(self.settings)
                    mst.samples = mopt[0]
                prev = None
                if scenes is not None:
                    mot = [torch.from_numpy(t).to("cuda") for t in tables]
                for f in range(n):
                    ft = feat[f & 1]
                    fst.seed = int(seeds[f]) & (2 ** 64 - 1)
                    if scenes is not None:
                        ctx.set_scene(scenes[f])
                    if spec is not None:
                        self._guide_pass(ctx, width, height, fst, sg, cams[f], spec)
                    gd = sg if spec is not None else ft
                    ctx.render_aov_async(width, height, fst,
                                         AovBuffers(ft["albedo"].data_ptr(), ft["normal"].data_ptr(),
                                                    ft["depth"].data_ptr(), None, ft["object"].data_ptr()),
                                         camera=cams[f], stream=0)
                    cur = temporal_frame(camera_frame(cams[f], int(self.settings.camera), width, height),
                                         lin[f].data_ptr(), ft["depth"].data_ptr(), ft["object"].data_ptr(),
                                         ft["normal"].data_ptr())
                    if hc is not None:  # (the same outputs as the branches below, by rt_temporal_clip_async)
                        temporal_clip_async(width, height, cur, prev, acc[f].data_ptr(), cnt[f].data_ptr(),
                                            None if vg is not None else rgba[f].data_ptr(), tp, 0, clip=hc,
                                            d_motion=mot[f].data_ptr() if scenes is not None else None,
                                            num_objects=mot[f].shape[0] if scenes is not None else 0,
                                            d_cur_albedo=ft["albedo"].data_ptr(),
                                            d_prev_moments=(mom[f - 1].data_ptr()
                                                            if vg is not None and prev is not None else None),
                                            d_out_moments=mom[f].data_ptr() if vg is not None else None,
                                            d_out_clipped=clp[f].data_ptr())
                    if vg is not None:
                        if hc is not None:
                            pass
                        elif scenes is not None:
                            temporal_motion_async(width, height, cur, prev, mot[f].data_ptr(), mot[f].shape[0],
                                                  acc[f].data_ptr(), cnt[f].data_ptr(), None, tp, 0,
                                                  d_cur_albedo=ft["albedo"].data_ptr(),
                                                  d_prev_moments=mom[f - 1].data_ptr() if prev is not None else None,
                                                  d_out_moments=mom[f].data_ptr())
                        else:
                            temporal_moments_async(width, height, cur, prev, ft["albedo"].data_ptr(),
                                                   mom[f - 1].data_ptr() if prev is not None else None,
                                                   acc[f].data_ptr(), cnt[f].data_ptr(), mom[f].data_ptr(), None, tp, 0)
                        variance_async(width, height, acc[f].data_ptr(), gd["normal"].data_ptr(),
                                       gd["depth"].data_ptr(), gd["albedo"].data_ptr(), gd["object"].data_ptr(),
                                       mom[f].data_ptr(), cnt[f].data_ptr(), var[f].data_ptr(), vg[0], 0)
                        denoise_var_async(width, height, acc[f].data_ptr(), gd["normal"].data_ptr(),
                                          gd["depth"].data_ptr(), var[f].data_ptr(), gd["albedo"].data_ptr(),
                                          gd["object"].data_ptr(), dlin[f].data_ptr(), rgba[f].data_ptr(), None,
                                          work.data_ptr(), nbytes, vg[1], 0)
                    elif hc is not None:
                        pass
                    elif scenes is not None:
                        temporal_motion_async(width, height, cur, prev, mot[f].data_ptr(), mot[f].shape[0],
                                              acc[f].data_ptr(), cnt[f].data_ptr(), rgba[f].data_ptr(), tp, 0)
                    else:
                        temporal_async(width, height, cur, prev, acc[f].data_ptr(), cnt[f].data_ptr(),
                                       rgba[f].data_ptr(), tp, 0)
                    prev = temporal_frame(cur.frame, acc[f].data_ptr(), ft["depth"].data_ptr(),
                                          ft["object"].data_ptr(), ft["normal"].data_ptr(), cnt[f].data_ptr())
                    if dn is not None:
                        denoise_async(width, height, acc[f].data_ptr(), gd["normal"].data_ptr(), gd["depth"].data_ptr(),
                                      gd["albedo"].data_ptr(), gd["object"].data_ptr(), dlin[f].data_ptr(),
                                      rgba[f].data_ptr(), work.data_ptr(), nbytes, dn, 0)
                    if mopt is not None:  # the shown frame's last step; nothing of it is fed back
                        mst.seed = fst.seed
                        ctx.render_matte_async(width, height, mst,
                                               MatteBuffers(mid.data_ptr(), mcn.data_ptr(), mre.data_ptr()),
                                               params=default_matte(ranks=mopt[1]), camera=cams[f], stream=0)
                        shown = dlin[f] if dn is not None or vg is not None else acc[f]
                        matte_resolve_async(width, height, shown.data_ptr(), ft["object"].data_ptr(), mid.data_ptr(),
                                            mcn.data_ptr(), mre.data_ptr(), mopt[1], mopt[0], rlin[f].data_ptr(),
                                            rgba[f].data_ptr(), mopt[2], 0)
            torch.cuda.synchronize()
            self.last_resolved_linear = rlin.cpu().numpy().reshape(n, height, width, 3) if mopt is not None else None
            self.last_linear = lin.cpu().numpy().reshape(n, height, width, 3)
            self.last_temporal_linear = acc.cpu().numpy().reshape(n, height, width, 3) if tp is not None else None
            self.last_history = cnt.cpu().numpy().reshape(n, height, width) if tp is not None else None
            self.last_denoised_linear = (dlin.cpu().numpy().reshape(n, height, width, 3)
                                         if dn is not None or vg is not None else None)
            self.last_variance = var.cpu().numpy().reshape(n, height, width) if vg is not None else None
            self.last_clipped = clp.cpu().numpy().reshape(n, height, width) if hc is not None else None
            img = rgba.cpu().numpy().reshape(n, height, width, 4)
        self.benchmark_data = {
            "scene_name": "demo_scene",
            "resolution": f"{width}x{height}",
            "render_time_seconds": time.perf_counter() - t0,
            "samples": self.settings.samples,
            "max_depth": self.settings.max_depth,
            "num_workers": self.settings.num_workers,
            "timestamp": datetime.now(timezone.utc).isoformat(),
            "features": list(self.FEATURES),
            "frames": n,
        }
        return img

    def render_aov(self, scene: Scene, width: int, height: int, camera=None, specular=None) -> dict:
        """The first-hit feature buffers of the frame (rt_context_render_aov_async) with the
        renderer's samples, seed and camera model, as numpy arrays: ``albedo`` and ``normal`` (H, W, 3)
        float32, ``depth`` and ``coverage`` (H, W) float32, ``object`` (H, W) int32 (-1: nothing hit; depth
        +Inf there).  camera: a Camera or a scene-file camera dict (with ``position``) in place of the
        scene's.  Runs on the renderer's first device whatever ``num_devices`` is.

        specular ("default", a dict of AovSpec's fields or an AovSpec; None: the first-hit pass): the
        specular-through feature buffers instead (rt_context_render_aov_spec_async), the
        five arrays taken behind the scene's mirrors plus ``specular`` and ``bounces`` (H, W) float32."""
        if int(width) < 1 or int(height) < 1:
            raise RenderError(f"render_aov: invalid image size {width}x{height}")
        spec = None if specular is None else _as_aov_spec(specular)
        names = AOV_NAMES if spec is None else AOV_SPEC_NAMES
        if int(self.settings.samples) < 1:
            raise RenderError("render_aov: settings.samples must be >= 1")
        if isinstance(camera, dict) and "position" not in camera:
            raise RenderError("render_aov: a camera dict needs a position")
        if camera is not None and not isinstance(camera, (dict, Camera, Scene)):
            raise RenderError("render_aov: camera is a Camera, a Scene, a camera dict or None")
        view = SceneView.from_buffer_copy(scene.view)  # (validated with the camera the pass shoots from)
        if camera is not None:
            view.camera = _as_camera(camera)
        _check(lib().rt_validate(ctypes.byref(view), width, height, ctypes.byref(self.settings)))
        import torch

        dev = self.devices[0] if self.devices else 0
        if self._prog_ctx is None:  # (the context render_progressive uses, kept like the rt_renderer)
            self._prog_ctx = Context(dev)
        ctx = self._prog_ctx
        if self._tuning is not None:
            ctx.set_tuning(self._tuning)
        ctx.set_scene(scene)
        npix = width * height
        with torch.cuda.device(dev):
            bufs = {n: torch.zeros(npix * (3 if n in ("albedo", "normal") else 1),
                                   dtype=torch.int32 if n == "object" else torch.float32, device="cuda")
                    for n in names}
            if spec is None:
                out = AovBuffers(*[bufs[n].data_ptr() for n in names])
                ctx.render_aov_async(width, height, self.settings, out, camera=camera, stream=0)
            else:
                out = AovSpecBuffers(*[bufs[n].data_ptr() for n in names])
                ctx.render_aov_spec_async(width, height, self.settings, out, spec=spec, camera=camera, stream=0)
            torch.cuda.synchronize()
            return {n: bufs[n].cpu().numpy().reshape((height, width, 3) if n in ("albedo", "normal")
                                                     else (height, width)) for n in names}

    def render_matte(self, scene: Scene, width: int, height: int, samples: int = 16, ranks: int = 4,
                     level="object", camera=None) -> dict:
        """The matte layers of the frame (rt_context_render_matte_async) with ``samples``
        camera rays per pixel and the renderer's seed and camera model, as numpy arrays: ``id`` and
        ``count`` (K, H, W) int32 (K = ranks; -1 and 0 for an empty rank), ``rest`` (H, W) int32 and
        ``coverage`` (K, H, W) float32 = count / samples.  level: "object" (the key is the object's index)
        or "face" (object * 16 + the triangle's ordinal in its cube).  camera as in ``render_aov``.  Runs on
        the renderer's first device."""
        if int(width) < 1 or int(height) < 1:
            raise RenderError(f"render_matte: invalid image size {width}x{height}")
        if int(samples) < 1 or not 1 <= int(ranks) <= RT_MATTE_MAX_RANKS:
            raise RenderError(f"render_matte: samples must be >= 1 and ranks in 1..{RT_MATTE_MAX_RANKS}")
        if isinstance(camera, dict) and "position" not in camera:
            raise RenderError("render_matte: a camera dict needs a position")
        if camera is not None and not isinstance(camera, (dict, Camera, Scene)):
            raise RenderError("render_matte: camera is a Camera, a Scene, a camera dict or None")
        m = default_matte(ranks=int(ranks), level=level)
        st = Settings.from_buffer_copy(self.settings)
        st.samples = int(samples)
        view = SceneView.from_buffer_copy(scene.view)
        if camera is not None:
            view.camera = _as_camera(camera)
        _check(lib().rt_validate(ctypes.byref(view), width, height, ctypes.byref(st)))
        import torch

        dev = self.devices[0] if self.devices else 0
        if self._prog_ctx is None:  # (the context render_progressive and render_aov use, kept)
            self._prog_ctx = Context(dev)
        ctx = self._prog_ctx
        if self._tuning is not None:
            ctx.set_tuning(self._tuning)
        ctx.set_scene(scene)
        npix, k = width * height, int(m.ranks)
        with torch.cuda.device(dev):
            ids = torch.zeros(max(k, 1) * npix, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(max(k, 1) * npix, dtype=torch.int32, device="cuda")
            rest = torch.zeros(npix, dtype=torch.int32, device="cuda")
            ctx.render_matte_async(width, height, st, MatteBuffers(ids.data_ptr(), cnt.data_ptr(), rest.data_ptr()),
                                   params=m, camera=camera, stream=0)
            torch.cuda.synchronize()
            count = cnt.cpu().numpy().reshape(k, height, width)
            return {"id": ids.cpu().numpy().reshape(k, height, width), "count": count,
                    "rest": rest.cpu().numpy().reshape(height, width),
                    "coverage": (count.astype(np.float64) / float(samples)).astype(np.float32)}

    @staticmethod
    def _matte_pass(ctx, width, height, settings, opt, d_object=None, camera=None):
        """What the edge resolve of a ``matte=`` option reads beside the image, on the current
        device: an object-level matte of the frame with opt's samples and ranks, and the frame's first-hit
        ids (d_object; None: a first-hit pass with the frame's settings makes them).  A dict of tensors, its
        own output buffers ``linear`` and ``rgba`` included."""
        import torch

        samples, ranks, _ = opt
        npix = width * height
        m = {n: torch.zeros((1 if n == "rest" else ranks) * npix, dtype=torch.int32, device="cuda")
             for n in ("id", "count", "rest")}
        if d_object is None:
            m["object"] = torch.zeros(npix, dtype=torch.int32, device="cuda")
            ctx.render_aov_async(width, height, settings, AovBuffers(None, None, None, None, m["object"].data_ptr()),
                                 camera=camera, stream=0)
            d_object = m["object"].data_ptr()
        m["d_object"] = d_object
        st = Settings.from_buffer_copy(settings)
        st.samples = samples
        ctx.render_matte_async(width, height, st,
                               MatteBuffers(m["id"].data_ptr(), m["count"].data_ptr(), m["rest"].data_ptr()),
                               params=default_matte(ranks=ranks), camera=camera, stream=0)
        m["linear"] = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
        m["rgba"] = torch.zeros(npix * 4, dtype=torch.uint8, device="cuda")
        return m

    @staticmethod
    def _matte_apply(width, height, opt, m, d_color):
        """rt_matte_resolve_async of the image at d_color with the buffers of ``_matte_pass``, into its
        ``linear`` and ``rgba``."""
        samples, ranks, rs = opt
        matte_resolve_async(width, height, d_color, m["d_object"], m["id"].data_ptr(), m["count"].data_ptr(),
                            m["rest"].data_ptr(), ranks, samples, m["linear"].data_ptr(), m["rgba"].data_ptr(), rs, 0)

    @staticmethod
    def _guide_pass(ctx, width, height, settings, feat, camera=None, spec=None):
        """The albedo, normal, depth and object a filter is guided by into the tensors of ``feat``: the
        first-hit pass (spec None) or the specular-through pass (an AovSpec, §4.16)."""
        ptr = [feat["albedo"].data_ptr(), feat["normal"].data_ptr(), feat["depth"].data_ptr(), None,
               feat["object"].data_ptr()]
        if spec is None:
            ctx.render_aov_async(width, height, settings, AovBuffers(*ptr), camera=camera, stream=0)
        else:
            ctx.render_aov_spec_async(width, height, settings, AovSpecBuffers(*ptr, None, None), spec=spec,
                                      camera=camera, stream=0)

    @staticmethod
    def _denoise_buffers(npix: int, width: int, height: int):
        """Device buffers of a denoised frame: the four feature buffers the filter reads, its workspace
        and its two outputs (torch tensors on the current device)."""
        import torch

        feat = {n: torch.zeros(npix * (3 if n in ("albedo", "normal") else 1),
                               dtype=torch.int32 if n == "object" else torch.float32, device="cuda")
                for n in ("albedo", "normal", "depth", "object")}
        nbytes = denoise_workspace_bytes(width, height)
        work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        out_lin = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
        out_rgba = torch.zeros(npix * 4, dtype=torch.uint8, device="cuda")
        return feat, work, nbytes, out_lin, out_rgba

    def render_denoised(self, scene: Scene, width: int, height: int, params=None, camera=None,
                        variance=None, guide="first", specular=None, matte=None) -> np.ndarray:
        """Render, then denoise: the frame of ``render`` (the renderer's settings; camera as
        in ``render_aov``), its first-hit feature buffers with the same samples, seed and camera model, and
        rt_denoise_async over both, on the renderer's first device.  params: a Denoise, a dict of its fields
        or None (default_denoise()).  Returns the denoised (H, W, 4) uint8 image; ``last_linear`` is the raw
        render's linear radiance as after ``render``, ``last_denoised_linear`` the filter's.

        variance (True, or a dict of DenoiseVar's and Variance's fields; §4.15; instead of ``params``): the
        filter is rt_denoise_var_async, steered by rt_variance_async of the render.  A single frame has no
        moments, so the variance is the spatial estimate; ``last_variance`` is (H, W) float32.

        guide ("first" or "specular"; §4.16): "specular" guides the filter by the specular-through albedo,
        normal, depth and object (``specular``: the pass's parameters as in ``render_aov``), so that it
        stops at the edges of what a mirror shows; "first" is the first-hit guide.

        matte (True, a number of matte samples, or a dict with any of samples, ranks, radius, background;
        §4.19): the filtered frame goes through the edge resolve as the last step -- an object-level matte of
        the frame (16 samples, 4 ranks by default) and rt_matte_resolve_async -- and the resolved image is
        returned; ``last_resolved_linear`` holds its linear radiance and ``last_denoised_linear`` stays the
        filter's.  Without it nothing changes."""
        spec = _as_guide(guide, specular)
        mopt = _as_matte_option(matte, "render_denoised")
        if int(width) < 1 or int(height) < 1:
            raise RenderError(f"render_denoised: invalid image size {width}x{height}")
        if int(self.settings.samples) < 1:
            raise RenderError("render_denoised: settings.samples must be >= 1")
        if isinstance(camera, dict) and "position" not in camera:
            raise RenderError("render_denoised: a camera dict needs a position")
        if camera is not None and not isinstance(camera, (dict, Camera, Scene)):
            raise RenderError("render_denoised: camera is a Camera, a Scene, a camera dict or None")
        vg = None if variance is None or variance is False else _as_variance(variance)
        if vg is not None and params is not None:
            raise RenderError("render_denoised: variance and params are two filters for the same frame: give one")
        dn = _as_denoise(params)
        view = SceneView.from_buffer_copy(scene.view)  # (validated with the camera the frame is shot from)
        if camera is not None:
            view.camera = _as_camera(camera)
        _check(lib().rt_validate(ctypes.byref(view), width, height, ctypes.byref(self.settings)))
        import torch

        dev = self.devices[0] if self.devices else 0
        if self._prog_ctx is None:  # (the context render_progressive and render_aov use, kept)
            self._prog_ctx = Context(dev)
        ctx = self._prog_ctx
        if self._tuning is not None:
            ctx.set_tuning(self._tuning)
        ctx.set_scene(scene)
        npix = width * height
        with torch.cuda.device(dev):
            lin = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
            feat, work, nbytes, out_lin, out_rgba = self._denoise_buffers(npix, width, height)
            if camera is None:
                ctx.render_async(width, height, self.settings, lin.data_ptr(), 0, 0)
            else:
                ctx.render_cameras_async(width, height, self.settings, [camera], [lin.data_ptr()], stream=0)
            self._guide_pass(ctx, width, height, self.settings, feat, camera, spec)
            if vg is not None:
                nbytes = denoise_var_workspace_bytes(width, height)
                work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
                var = torch.zeros(npix, dtype=torch.float32, device="cuda")
                variance_async(width, height, lin.data_ptr(), feat["normal"].data_ptr(), feat["depth"].data_ptr(),
                               feat["albedo"].data_ptr(), feat["object"].data_ptr(), None, None, var.data_ptr(),
                               vg[0], 0)
                denoise_var_async(width, height, lin.data_ptr(), feat["normal"].data_ptr(), feat["depth"].data_ptr(),
                                  var.data_ptr(), feat["albedo"].data_ptr(), feat["object"].data_ptr(),
                                  out_lin.data_ptr(), out_rgba.data_ptr(), None, work.data_ptr(), nbytes, vg[1], 0)
            else:
                denoise_async(width, height, lin.data_ptr(), feat["normal"].data_ptr(), feat["depth"].data_ptr(),
                              feat["albedo"].data_ptr(), feat["object"].data_ptr(), out_lin.data_ptr(),
                              out_rgba.data_ptr(), work.data_ptr(), nbytes, dn, 0)
            if mopt is not None:  # (the first-hit ids: the guide's own unless it looked through the mirrors)
                mt = self._matte_pass(ctx, width, height, self.settings, mopt,
                                      feat["object"].data_ptr() if spec is None else None, camera)
                self._matte_apply(width, height, mopt, mt, out_lin.data_ptr())
            torch.cuda.synchronize()
            self.last_variance = var.cpu().numpy().reshape(height, width) if vg is not None else None
            self.last_linear = lin.cpu().numpy().reshape(height, width, 3)
            self.last_denoised_linear = out_lin.cpu().numpy().reshape(height, width, 3)
            if mopt is not None:
                self.last_resolved_linear = mt["linear"].cpu().numpy().reshape(height, width, 3)
                return mt["rgba"].cpu().numpy().reshape(height, width, 4)
            return out_rgba.cpu().numpy().reshape(height, width, 4)

    def rank_seconds(self) -> list:
        """Device seconds of each rank's render launches in the last render (load balance)."""
        r = self._renderer()
        n = lib().rt_renderer_num_ranks(r)  # (the renderer's own count, not the mutable settings)
        out = (ctypes.c_double * max(1, n))()
        _check(lib().rt_renderer_rank_seconds(r, out, n))
        return list(out)

    def save_image(self, img: np.ndarray, filename: str):
        """SaveImage (renderer.go:438-451); '.ppm' writes a P3 PPM."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w = img.shape[:2]
        f = lib().rt_write_ppm if filename.endswith(".ppm") else lib().rt_write_png
        _check(f(filename.encode(), img.ctypes.data, w, h))

    def save_benchmark_data(self, path: str):
        """SaveBenchmarkData (renderer.go:473-485)."""
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(path, "w") as f:
            json.dump(self.benchmark_data, f, indent=2)


# --------------------------------------------------------------- device API
class Context:
    """A scene resident on one device (rt_context_*)."""

    def __init__(self, device: int = 0):
        self._h = ctypes.c_void_p()
        _check(lib().rt_context_create(device, ctypes.byref(self._h)))

    def set_scene(self, scene: Scene, force_bvh: int = 0):
        self._scene = scene  # keep alive
        _check(lib().rt_context_set_scene(self._h, ctypes.byref(scene.view), force_bvh))

    def set_tuning(self, tuning: Tuning):
        _check(lib().rt_context_set_tuning(self._h, ctypes.byref(tuning)))

    def render_async(self, width, height, settings: Settings, d_linear: int, d_rgba: int, stream: int = 0,
                     rank: int = 0, world: int = 1, layout: int = RT_LAYOUT_IMAGE):
        _check(
            lib().rt_context_render_async(
                self._h, width, height, ctypes.byref(settings), rank, world, layout,
                ctypes.c_void_p(d_linear), ctypes.c_void_p(d_rgba), ctypes.c_void_p(stream), None,
            )
        )

    def count(self, width, height, settings: Settings, d_linear: int, d_rgba: int, stream: int = 0,
              rank: int = 0, world: int = 1, layout: int = RT_LAYOUT_IMAGE, full: bool = False):
        """The counting variant: the reference's nine counts (dict); full=True
        returns the Counts struct (with the culled part, Counts.culled_dict)."""
        c = Counts()
        _check(
            lib().rt_context_render_async(
                self._h, width, height, ctypes.byref(settings), rank, world, layout,
                ctypes.c_void_p(d_linear), ctypes.c_void_p(d_rgba), ctypes.c_void_p(stream), ctypes.byref(c),
            )
        )
        return c if full else c.as_dict()

    def render_frames_async(self, width, height, settings: Settings, seeds, d_linear, d_rgba=None, stream: int = 0,
                            rank: int = 0, world: int = 1, layout: int = RT_LAYOUT_IMAGE):
        """rt_context_render_frames_async: len(seeds) frames of one schedule in one launch;
        d_linear / d_rgba: per-frame device pointers (d_rgba None: no RGBA8)."""
        n = len(seeds)
        sd = (ctypes.c_uint64 * n)(*seeds)
        lp = (ctypes.c_void_p * n)(*d_linear)
        rp = (ctypes.c_void_p * n)(*d_rgba) if d_rgba is not None else None
        _check(lib().rt_context_render_frames_async(self._h, width, height, ctypes.byref(settings), n, sd, rank, world,
                                                     layout, lp, rp, ctypes.c_void_p(stream)))

    def render_cameras_async(self, width, height, settings: Settings, cameras, d_linear, d_rgba=None, seeds=None,
                             stream: int = 0, rank: int = 0, world: int = 1, layout: int = RT_LAYOUT_IMAGE):
        """rt_context_render_cameras_async: len(cameras) frames of the scene, frame f seen from cameras[f]
        (Camera structs or scene-file camera dicts) with seed seeds[f] (None: settings.seed), in one
        streamed launch where a batched launch would stream, else frame by frame;
        d_linear / d_rgba: per-frame device pointers (d_rgba None: no RGBA8)."""
        n = len(cameras)
        cams = (Camera * max(1, n))(*[_as_camera(c) for c in cameras])
        sd = (ctypes.c_uint64 * n)(*seeds) if seeds is not None else None
        lp = (ctypes.c_void_p * max(1, n))(*d_linear)
        rp = (ctypes.c_void_p * max(1, n))(*d_rgba) if d_rgba is not None else None
        _check(lib().rt_context_render_cameras_async(self._h, width, height, ctypes.byref(settings), n, cams, sd, rank,
                                                      world, layout, lp, rp, ctypes.c_void_p(stream)))

    def render_aov_async(self, width, height, settings: Settings, out: AovBuffers, camera=None, stream: int = 0):
        """rt_context_render_aov_async: the first-hit feature buffers of the whole frame
        into the device buffers of ``out`` (an AovBuffers; a pointer of None / 0 is not written): albedo and
        normal W*H*3 float32, depth and coverage W*H float32, object W*H int32.  camera: a Camera, a Scene or
        a scene-file camera dict; None: the scene's.  No image is rendered and no state of the context changes."""
        cam = ctypes.byref(_as_camera(camera)) if camera is not None else None
        _check(lib().rt_context_render_aov_async(self._h, width, height, ctypes.byref(settings), cam, ctypes.byref(out),
                                                  ctypes.c_void_p(stream)))

    def render_aov_spec_async(self, width, height, settings: Settings, out: AovSpecBuffers, spec=None, camera=None,
                              stream: int = 0):
        """rt_context_render_aov_spec_async: the specular-through feature buffers of the whole frame (DESIGN.md
        §4.16) into the device buffers of ``out`` (an AovSpecBuffers; a pointer of None / 0 is not written):
        the five of ``render_aov_async`` taken behind the scene's mirrors, and specular and bounces W*H
        float32.  spec: an AovSpec, a dict of its fields, None or "default" (default_aov_spec()).  camera as
        in ``render_aov_async``.  No image is rendered and no state of the context changes."""
        sp = _as_aov_spec(spec)
        cam = ctypes.byref(_as_camera(camera)) if camera is not None else None
        _check(lib().rt_context_render_aov_spec_async(self._h, width, height, ctypes.byref(settings), cam,
                                                       ctypes.byref(sp), ctypes.byref(out), ctypes.c_void_p(stream)))

    def render_matte_async(self, width, height, settings: Settings, out: MatteBuffers, params=None, camera=None,
                           stream: int = 0):
        """rt_context_render_matte_async: the matte layers of the whole frame into the device
        pointers of ``out`` (int32; d_id and d_count ``ranks`` planes of W*H, d_rest one); ``settings.samples``
        is the number of matte samples.  params: a Matte, a dict of its fields or None (default_matte());
        camera as in ``render_aov_async``.  No image is rendered and no state of the context changes."""
        m = _as_one(params, Matte, default_matte, "matte")
        cam = ctypes.byref(_as_camera(camera)) if camera is not None else None
        _check(lib().rt_context_render_matte_async(self._h, width, height, ctypes.byref(settings), cam, ctypes.byref(m),
                                                   ctypes.byref(out), ctypes.c_void_p(stream)))

    def progressive_begin(self, width, height, settings: Settings, rank: int = 0, world: int = 1,
                          layout: int = RT_LAYOUT_IMAGE):
        """rt_context_progressive_begin: start a progression of this frame; settings.samples is the cap."""
        _check(lib().rt_context_progressive_begin(self._h, width, height, ctypes.byref(settings), rank, world, layout))

    def progressive_add(self, nsamples: int, d_linear: int, d_rgba: int, stream: int = 0):
        """rt_context_progressive_add_async: the next nsamples samples of every pixel, then the
        image of the mean over all samples so far into d_linear / d_rgba (either may be 0)."""
        _check(lib().rt_context_progressive_add_async(self._h, nsamples, ctypes.c_void_p(d_linear),
                                                       ctypes.c_void_p(d_rgba), ctypes.c_void_p(stream)))

    def progressive_set_adaptive(self, tolerance, patience: int = 1, min_samples: int = 0):
        """rt_context_progressive_set_adaptive: after progressive_begin and before the first add, every
        pixel stops on its own once its displayed RGBA8 moved by at most `tolerance` for `patience` adds in
        a row and it has at least `min_samples` samples.  tolerance=None switches it off again."""
        if tolerance is None:
            _check(lib().rt_context_progressive_set_adaptive(self._h, None))
            return
        a = Adaptive(int(tolerance), int(patience), int(min_samples), 0)
        _check(lib().rt_context_progressive_set_adaptive(self._h, ctypes.byref(a)))

    def progressive_counts(self, d_counts: int, stream: int = 0):
        """rt_context_progressive_counts_async: the per-pixel sample counts (uint32) in the progression's
        layout into the device buffer d_counts."""
        _check(lib().rt_context_progressive_counts_async(self._h, ctypes.c_void_p(d_counts), ctypes.c_void_p(stream)))

    def progressive_state(self) -> dict:
        """rt_context_progressive_state (waits for the last add): in-image pixels of the rank's tiles, those
        still active, the sum of their sample counts, adds so far."""
        out = (ctypes.c_int64 * 4)()
        _check(lib().rt_context_progressive_state(self._h, out))
        return {"pixels": int(out[0]), "active": int(out[1]), "samples": int(out[2]), "adds": int(out[3])}

    def progressive_samples(self) -> int:
        """Samples per pixel the progression has rendered; -1: no progression."""
        return int(lib().rt_context_progressive_samples(self._h))

    def progressive_end(self):
        _check(lib().rt_context_progressive_end(self._h))

    def set_partition(self, partition):
        """Render the tiles of `partition` (a Partition, or None: strided)."""
        self._partition = partition  # (copied by the library; kept for symmetry)
        _check(lib().rt_context_set_partition(self._h, partition._h if partition is not None else None))

    def balanced_partition(self, width, height, settings: Settings, world: int) -> "Partition":
        """rt_partition_balanced: a pilot-estimated, work-balanced tile partition."""
        h = ctypes.c_void_p()
        _check(lib().rt_partition_balanced(self._h, width, height, ctypes.byref(settings), world, ctypes.byref(h)))
        return Partition(_handle=h)

    def set_debug_buffer(self, d_buf: int):
        _check(lib().rt_context_set_debug_buffer(self._h, ctypes.c_void_p(d_buf)))

    def profile(self, on: bool = True):
        """Per-kernel HIP-event timing of the wavefront path (resets the totals)."""
        _check(lib().rt_context_profile(self._h, 1 if on else 0))

    def kernel_seconds(self) -> dict:
        """{kernel class: (total seconds, launches)} since profile(True)."""
        s = (ctypes.c_double * len(WF_KERNELS))()
        n = (ctypes.c_int64 * len(WF_KERNELS))()
        _check(lib().rt_context_kernel_seconds(self._h, s, n))
        return {k: (s[i], int(n[i])) for i, k in enumerate(WF_KERNELS)}

    def tail_debug(self) -> dict:
        """rt_context_tail_debug: tail-helper counters since the layout (ticks at 100 MHz)."""
        out = (ctypes.c_uint64 * 6)()
        _check(lib().rt_context_tail_debug(self._h, out))
        return dict(zip(("exported", "paths_done", "solo_ticks", "export_ticks", "helper_ticks", "err"), out))

    def stats(self) -> dict:
        """rt_context_get_stats: schedules built, measuring frames, frames, launches, batched launches;
        the last schedule's work blocks and split pixels."""
        s = ContextStats()
        _check(lib().rt_context_get_stats(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in ContextStats._fields_}

    def last_kernel_seconds(self) -> float:
        s = ctypes.c_double()
        _check(lib().rt_context_last_kernel_seconds(self._h, ctypes.byref(s)))
        return s.value

    def close(self):
        if self._h:
            lib().rt_context_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def num_tiles(width: int, height: int) -> int:
    return lib().rt_num_tiles(width, height)


def tiles_for_rank(width: int, height: int, rank: int, world: int) -> int:
    return lib().rt_tiles_for_rank(width, height, rank, world)


def _as_camera(camera) -> Camera:
    """A Camera from a Camera, a Scene (its camera) or a scene file's camera dict."""
    if isinstance(camera, Scene):
        return camera.view.camera
    if isinstance(camera, dict):
        cam = Camera()
        cam.position[:] = camera.get("position", (0, 0, 0))
        cam.look_at[:] = camera.get("lookAt", (0, 0, 0))
        cam.up[:] = camera.get("up", (0, 0, 0))
        cam.fov = camera.get("fov", 0.0)
        cam.aspect_ratio = camera.get("aspectRatio", 0.0)
        return cam
    return camera


def _camera_dict(cam: Camera) -> dict:
    return {"position": list(cam.position), "lookAt": list(cam.look_at), "up": list(cam.up), "fov": cam.fov,
            "aspectRatio": cam.aspect_ratio}


def camera_orbit(camera, n: int, degrees: float = 360.0) -> list:
    """rt_camera_orbit: n views on a circle around the camera's lookAt, about its up axis, `degrees`
    in all (view k is turned by degrees * k / n; view 0 is the camera itself, bit for bit), as a
    list of scene-file camera dicts.  camera: a Camera, a Scene or a camera dict.  Host only."""
    n = int(n)
    cam = _as_camera(camera)
    out = (Camera * max(1, n))()
    _check(lib().rt_camera_orbit(ctypes.byref(cam), n, float(degrees), out))
    return [_camera_dict(out[k]) for k in range(n)]


def camera_frame(camera, model, width: int, height: int) -> np.ndarray:
    """rt_camera_frame: the viewport frame of `camera` (a Camera, a Scene, or a scene file's
    camera dict) under `model` (RT_CAMERA_* or its name) for a width x height image, as 12
    float64: origin, lower_left, horizontal, vertical."""
    camera = _as_camera(camera)
    out = np.zeros(12, np.float64)
    _check(lib().rt_camera_frame(ctypes.byref(camera), CAMERAS.get(model, model), width, height,
                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return out


def cone_rows(scene: Scene, force_bvh: int = 0) -> np.ndarray:
    """rt_scene_cone_rows: (num_lights, num_objects) uint64 -- per light and hittable, the spheres
    (bit b: the scene's b-th sphere) a shadow cone of a hit on that hittable can hold (host only)."""
    nl, no = int(scene.view.num_lights), int(scene.view.num_objects)
    out = np.zeros(max(nl * no, 1), np.uint64)
    _check(lib().rt_scene_cone_rows(ctypes.byref(scene.view), force_bvh,
                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), out.size))
    return out[: nl * no].reshape(nl, no)


def stream_decode(order: int, frames: int, nlive: int, spp: int, entries) -> np.ndarray:
    """rt_stream_decode: (n, 3) uint32 -- the (frame, live pixel, sample) of each queue entry of a
    streamed launch, decoded by the stream kernel's own function (host only)."""
    e = np.ascontiguousarray(entries, np.uint32)
    out = np.zeros((max(e.size, 1), 3), np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    _check(lib().rt_stream_decode(order, frames, nlive, spp, e.ctypes.data_as(u32p), e.size, out.ctypes.data_as(u32p)))
    return out[: e.size]


SOFT_UNDECIDED, SOFT_MISS, SOFT_HIT = 0, 1, 2


def soft_screen(centers, r2, origins, dirs, il, tmin, tmax) -> np.ndarray:
    """rt_soft_screen: (n,) int32 -- per case SOFT_MISS / SOFT_HIT where the stream kernels' screen of a soft
    shadow ray is sure, SOFT_UNDECIDED where the exact test decides (host only; the kernels' own function).
    centers, origins, dirs (unnormalised): (n, 3); r2, il (the caller's 1 / |dir|), tmin, tmax: (n,) or scalars."""
    c, o, u = (np.ascontiguousarray(a, np.float64).reshape(-1, 3) for a in (centers, origins, dirs))
    n = c.shape[0]
    assert o.shape[0] == n and u.shape[0] == n, (c.shape, o.shape, u.shape)
    s = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), (n,))) for a in (r2, il, tmin, tmax)]
    out = np.zeros(max(n, 1), np.int32)
    dp = ctypes.POINTER(ctypes.c_double)
    _check(lib().rt_soft_screen(c.ctypes.data_as(dp), s[0].ctypes.data_as(dp), o.ctypes.data_as(dp), u.ctypes.data_as(dp),
                                s[1].ctypes.data_as(dp), s[2].ctypes.data_as(dp), s[3].ctypes.data_as(dp), n,
                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    return out[:n]


def render(scene: Scene, width: int, height: int, settings: Settings):
    """One-shot rt_render: (rgba (H,W,4) u8, linear (H,W,3) f32, Stats)."""
    lin = np.zeros((height, width, 3), np.float32)
    rgba = np.zeros((height, width, 4), np.uint8)
    st = Stats()
    _check(lib().rt_render(ctypes.byref(scene.view), width, height, ctypes.byref(settings), lin.ctypes.data,
                           rgba.ctypes.data, ctypes.byref(st)))
    return rgba, lin, st


def adaptive_step(old_rgba, new_rgba, had_image, count: int, streak: int, tolerance: int, patience: int = 1,
                  min_samples: int = 0):
    """rt_adaptive_step: the stop rule of an adaptive progression for one pixel on the host (no device):
    (stop, new_streak) from its displayed RGBA before and after an add (four bytes each), whether it had an
    image before the add, its sample count including the add and its streak before it."""
    o = (ctypes.c_uint8 * 4)(*[int(v) for v in old_rgba])
    n = (ctypes.c_uint8 * 4)(*[int(v) for v in new_rgba])
    a = Adaptive(int(tolerance), int(patience), int(min_samples), 0)
    ns = ctypes.c_int32(0)
    rc = lib().rt_adaptive_step(o, n, 1 if had_image else 0, int(count), int(streak), ctypes.byref(a), ctypes.byref(ns))
    if rc < 0:
        _check(rc)
    return bool(rc), int(ns.value)


def rgba_delta_async(d_a: int, d_b: int, npix: int, d_out: int, stream: int = 0):
    """rt_rgba_delta_async: two RGBA8 device images of npix pixels -> the device words d_out[0]
    (pixels that differ) and d_out[1] (the largest byte difference); zeroes d_out first."""
    _check(lib().rt_rgba_delta_async(ctypes.c_void_p(d_a), ctypes.c_void_p(d_b), npix, ctypes.c_void_p(d_out),
                                     ctypes.c_void_p(stream)))


def default_aov_spec(**over) -> AovSpec:
    """rt_aov_spec_default (max_bounces 4, max_roughness 0.1), with the given fields replaced."""
    sp = AovSpec()
    lib().rt_aov_spec_default(ctypes.byref(sp))
    for k, v in over.items():
        if k not in ("max_bounces", "max_roughness"):
            raise RenderError(f"default_aov_spec: no such field {k}")
        setattr(sp, k, v)
    return sp


def _as_aov_spec(spec) -> AovSpec:
    """None, True or "default": the defaults; an AovSpec as it is; a dict: default_aov_spec(**dict)."""
    if spec is None or spec is True or spec == "default":
        return default_aov_spec()
    if isinstance(spec, AovSpec):
        return spec
    if isinstance(spec, dict):
        return default_aov_spec(**spec)
    raise RenderError('specular parameters are an AovSpec, a dict of its fields, "default" or None')


def aov_spec_follows(material, spec=None) -> bool:
    """rt_aov_spec_follows: whether the specular-through feature pass follows the reflection of ``material``
    (a Material, or a scene-file material dict) under ``spec`` (as in ``_as_aov_spec``).  No device needed."""
    if isinstance(material, dict):
        material = Scene.from_json_text(json.dumps({
            "camera": {"position": [0, 0, 1]}, "lights": [],
            "objects": [{"type": "sphere", "position": [0, 0, 0], "radius": 1, "material": material}],
        })).view.objects[0].material
    sp = _as_aov_spec(spec)
    rc = lib().rt_aov_spec_follows(ctypes.byref(material), ctypes.byref(sp))
    _check(min(rc, 0))
    return rc == 1


def _as_guide(guide, specular):
    """The AovSpec of a ``guide=`` / ``specular=`` pair, or None for the first-hit guide."""
    if guide not in ("first", "specular"):
        raise RenderError('guide is "first" or "specular"')
    if guide == "first":
        if specular is not None:
            raise RenderError('specular parameters need guide="specular"')
        return None
    return _as_aov_spec(specular)


def default_denoise(**over) -> Denoise:
    """rt_denoise_default (levels 4, normal_power 32, sigma_color 0.5, sigma_depth 0.05, demodulate 1),
    with the given fields replaced."""
    d = Denoise()
    lib().rt_denoise_default(ctypes.byref(d))
    for k, v in over.items():
        if k not in ("levels", "normal_power", "sigma_color", "sigma_depth", "demodulate"):
            raise RenderError(f"default_denoise: no such field {k}")
        setattr(d, k, v)
    return d


def _as_denoise(params) -> Denoise:
    """None: the defaults; a Denoise as it is; a dict: default_denoise(**dict)."""
    if params is None or params is True:
        return default_denoise()
    if isinstance(params, Denoise):
        return params
    if isinstance(params, dict):
        return default_denoise(**params)
    raise RenderError("denoise parameters are a Denoise, a dict of its fields or None")


def denoise_workspace_bytes(width: int, height: int) -> int:
    """rt_denoise_workspace_bytes: the device bytes rt_denoise_async needs for a width x height image."""
    return int(lib().rt_denoise_workspace_bytes(width, height))


def denoise_async(width: int, height: int, d_color: int, d_normal: int, d_depth: int, d_albedo=None, d_object=None,
                  d_out_linear=None, d_out_rgba=None, d_workspace=None, workspace_bytes: int = 0, params=None,
                  stream: int = 0):
    """rt_denoise_async: every argument a device pointer (an int; None: not given);
    asynchronous on ``stream``.  d_out_linear may be d_color (in place)."""
    p = _as_denoise(params)
    inp = DenoiseInputs(d_color, d_normal, d_depth, d_albedo, d_object)
    _check(lib().rt_denoise_async(ctypes.byref(p), width, height, ctypes.byref(inp), ctypes.c_void_p(d_out_linear),
                                  ctypes.c_void_p(d_out_rgba), ctypes.c_void_p(d_workspace), workspace_bytes,
                                  ctypes.c_void_p(stream)))


def denoise_host(color, normal, depth, albedo=None, object=None, params=None):
    """rt_denoise_host: the denoiser on numpy arrays, without a device.  color, normal (and albedo) are
    (H, W, 3) float32, depth (H, W) float32, object (H, W) int32.  Returns (linear (H, W, 3) float32,
    rgba (H, W, 4) uint8)."""
    color = np.ascontiguousarray(color, np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise RenderError("denoise_host: color is an (H, W, 3) array")
    h, w = color.shape[:2]

    def arr(a, dtype, shape, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype)
        if a.shape != shape:
            raise RenderError(f"denoise_host: {name} has shape {a.shape}, expected {shape}")
        return a

    normal = arr(normal, np.float32, (h, w, 3), "normal")
    depth = arr(depth, np.float32, (h, w), "depth")
    albedo = arr(albedo, np.float32, (h, w, 3), "albedo")
    obj = arr(object, np.int32, (h, w), "object")
    p = _as_denoise(params)
    inp = DenoiseInputs(*[a.ctypes.data if a is not None else None for a in (color, normal, depth, albedo, obj)])
    lin = np.zeros((h, w, 3), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    _check(lib().rt_denoise_host(ctypes.byref(p), w, h, ctypes.byref(inp), lin.ctypes.data, rgba.ctypes.data))
    return lin, rgba


def default_temporal(**over) -> Temporal:
    """rt_temporal_default (max_history 32, depth_tol 0.05, normal_min 0.9, min_weight 0.25), with the
    given fields replaced."""
    t = Temporal()
    lib().rt_temporal_default(ctypes.byref(t))
    for k, v in over.items():
        if k not in ("max_history", "depth_tol", "normal_min", "min_weight"):
            raise RenderError(f"default_temporal: no such field {k}")
        setattr(t, k, v)
    return t


def _as_temporal(params) -> Temporal:
    """None or True: the defaults; a Temporal as it is; a dict: default_temporal(**dict)."""
    if params is None or params is True:
        return default_temporal()
    if isinstance(params, Temporal):
        return params
    if isinstance(params, dict):
        return default_temporal(**params)
    raise RenderError("temporal parameters are a Temporal, a dict of its fields, True or None")


def temporal_frame(frame, color, depth, object=None, normal=None, count=None) -> TemporalFrame:
    """An rt_temporal_frame from pointers (ints; None: not given) and the 12 doubles of camera_frame."""
    f = np.ascontiguousarray(frame, np.float64).ravel()
    if f.size != 12:
        raise RenderError("temporal: a frame is the 12 doubles of camera_frame")
    return TemporalFrame(color, depth, object, normal, count, (ctypes.c_double * 12)(*[float(v) for v in f]))


def temporal_async(width: int, height: int, cur: TemporalFrame, prev, d_out_color: int, d_out_count: int,
                   d_out_rgba=None, params=None, stream: int = 0):
    """rt_temporal_async: cur and prev (None: start a history) are TemporalFrames of
    device pointers (temporal_frame()); the outputs are device pointers, d_out_rgba may be None;
    asynchronous on ``stream``.  d_out_color / d_out_count must not be prev's color / count."""
    p = _as_temporal(params)
    _check(lib().rt_temporal_async(ctypes.byref(p), width, height, ctypes.byref(cur),
                                   ctypes.byref(prev) if prev is not None else None, ctypes.c_void_p(d_out_color),
                                   ctypes.c_void_p(d_out_count), ctypes.c_void_p(d_out_rgba), ctypes.c_void_p(stream)))


def temporal_host(cur: dict, prev=None, params=None):
    """rt_temporal_host: temporal accumulation on numpy arrays, without a device.  cur and prev (None:
    start a history) are dicts with ``color`` (H, W, 3) float32, ``depth`` (H, W) float32, ``frame`` (the
    12 doubles of camera_frame), optionally ``object`` (H, W) int32 and ``normal`` (H, W, 3) float32 (each
    in both frames or in neither), and in prev ``count`` (H, W) float32 -- the previous call's results.
    Returns (color (H, W, 3) float32, count (H, W) float32, rgba (H, W, 4) uint8)."""
    color = np.ascontiguousarray(cur["color"], np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise RenderError("temporal_host: color is an (H, W, 3) array")
    h, w = color.shape[:2]
    keep = []

    def frame_of(d, name):
        def arr(k, dtype, shape):
            a = d.get(k)
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype)
            if a.shape != shape:
                raise RenderError(f"temporal_host: {name}.{k} has shape {a.shape}, expected {shape}")
            keep.append(a)
            return a.ctypes.data

        return temporal_frame(d["frame"], arr("color", np.float32, (h, w, 3)), arr("depth", np.float32, (h, w)),
                              arr("object", np.int32, (h, w)), arr("normal", np.float32, (h, w, 3)),
                              arr("count", np.float32, (h, w)))

    fc = frame_of(cur, "cur")
    fp = frame_of(prev, "prev") if prev is not None else None
    p = _as_temporal(params)
    out = np.zeros((h, w, 3), np.float32)
    cnt = np.zeros((h, w), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    _check(lib().rt_temporal_host(ctypes.byref(p), w, h, ctypes.byref(fc), ctypes.byref(fp) if fp is not None else None,
                                  out.ctypes.data, cnt.ctypes.data, rgba.ctypes.data))
    return out, cnt, rgba


_VARIANCE_FIELDS = ("min_history", "normal_power", "sigma_depth")
_DENOISE_VAR_FIELDS = ("levels", "normal_power", "sigma_lum", "sigma_depth", "demodulate", "prefilter")


def default_variance(**over) -> Variance:
    """rt_variance_default (min_history 4, normal_power 32, sigma_depth 0.05), with the given fields replaced."""
    v = Variance()
    lib().rt_variance_default(ctypes.byref(v))
    for k, val in over.items():
        if k not in _VARIANCE_FIELDS:
            raise RenderError(f"default_variance: no such field {k}")
        setattr(v, k, val)
    return v


def default_denoise_var(**over) -> DenoiseVar:
    """rt_denoise_var_default (levels 4, normal_power 32, sigma_lum 2, sigma_depth 0.05, demodulate 1,
    prefilter 1), with the given fields replaced."""
    d = DenoiseVar()
    lib().rt_denoise_var_default(ctypes.byref(d))
    for k, val in over.items():
        if k not in _DENOISE_VAR_FIELDS:
            raise RenderError(f"default_denoise_var: no such field {k}")
        setattr(d, k, val)
    return d


def _as_one(params, cls, default, what):
    if params is None or params is True:
        return default()
    if isinstance(params, cls):
        return params
    if isinstance(params, dict):
        return default(**params)
    raise RenderError(f"{what} parameters are a {cls.__name__}, a dict of its fields or None")


def _as_variance(params):
    """The (Variance, DenoiseVar) of a ``variance=`` argument.  True: the defaults; a dict: each field goes
    to the struct that has it (normal_power and sigma_depth to both); a (Variance, DenoiseVar) pair as it is."""
    if params is True:
        return default_variance(), default_denoise_var()
    if isinstance(params, tuple) and len(params) == 2 and isinstance(params[0], Variance) \
            and isinstance(params[1], DenoiseVar):
        return params
    if isinstance(params, dict):
        for k in params:
            if k not in _VARIANCE_FIELDS and k not in _DENOISE_VAR_FIELDS:
                raise RenderError(f"variance: no such field {k}")
        return (default_variance(**{k: v for k, v in params.items() if k in _VARIANCE_FIELDS}),
                default_denoise_var(**{k: v for k, v in params.items() if k in _DENOISE_VAR_FIELDS}))
    raise RenderError("variance is True, a dict of DenoiseVar's and Variance's fields or a (Variance, DenoiseVar) pair")


def temporal_moments_async(width: int, height: int, cur: TemporalFrame, prev, d_cur_albedo, d_prev_moments,
                           d_out_color: int, d_out_count: int, d_out_moments: int, d_out_rgba=None, params=None,
                           stream: int = 0):
    """rt_temporal_moments_async: temporal_async with the current frame's albedo (None:
    not given), the previous call's moments (given exactly when prev is) and the moments' output, all
    device pointers.  The three outputs must not be prev's color / count / moments."""
    p = _as_temporal(params)
    _check(lib().rt_temporal_moments_async(ctypes.byref(p), width, height, ctypes.byref(cur),
                                           ctypes.byref(prev) if prev is not None else None,
                                           ctypes.c_void_p(d_cur_albedo), ctypes.c_void_p(d_prev_moments),
                                           ctypes.c_void_p(d_out_color), ctypes.c_void_p(d_out_count),
                                           ctypes.c_void_p(d_out_moments), ctypes.c_void_p(d_out_rgba),
                                           ctypes.c_void_p(stream)))


def _host_arrays(what, h, w, keep, **arrays):
    """Contiguous arrays of the expected (dtype, shape), kept alive in ``keep``; returns their addresses."""
    out = {}
    for name, (a, dtype, shape) in arrays.items():
        if a is None:
            out[name] = None
            continue
        a = np.ascontiguousarray(a, dtype)
        if a.shape != shape:
            raise RenderError(f"{what}: {name} has shape {a.shape}, expected {shape}")
        keep.append(a)
        out[name] = a.ctypes.data
    return out


def temporal_moments_host(cur: dict, prev=None, params=None):
    """rt_temporal_moments_host: temporal_host with the luminance moments.  cur may also hold ``albedo``
    (H, W, 3) float32, prev must also hold ``moments`` (H, W, 2) float32 -- the previous call's.  Returns
    (color, count, moments (H, W, 2) float32, rgba)."""
    color = np.ascontiguousarray(cur["color"], np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise RenderError("temporal_moments_host: color is an (H, W, 3) array")
    h, w = color.shape[:2]
    keep = []

    def frame_of(d, name):
        a = _host_arrays(f"temporal_moments_host: {name}", h, w, keep,
                         color=(d.get("color"), np.float32, (h, w, 3)), depth=(d.get("depth"), np.float32, (h, w)),
                         object=(d.get("object"), np.int32, (h, w)), normal=(d.get("normal"), np.float32, (h, w, 3)),
                         count=(d.get("count"), np.float32, (h, w)), albedo=(d.get("albedo"), np.float32, (h, w, 3)),
                         moments=(d.get("moments"), np.float32, (h, w, 2)))
        return temporal_frame(d["frame"], a["color"], a["depth"], a["object"], a["normal"], a["count"]), a

    fc, ac = frame_of(cur, "cur")
    fp, ap = frame_of(prev, "prev") if prev is not None else (None, {"moments": None})
    p = _as_temporal(params)
    out = np.zeros((h, w, 3), np.float32)
    cnt = np.zeros((h, w), np.float32)
    mom = np.zeros((h, w, 2), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    _check(lib().rt_temporal_moments_host(ctypes.byref(p), w, h, ctypes.byref(fc),
                                          ctypes.byref(fp) if fp is not None else None, ac["albedo"], ap["moments"],
                                          out.ctypes.data, cnt.ctypes.data, mom.ctypes.data, rgba.ctypes.data))
    return out, cnt, mom, rgba


def scene_motion(prev: "Scene", cur: "Scene") -> np.ndarray:
    """rt_scene_motion: the (num_objects, 3) float64 table of each object's translation from
    ``prev`` to ``cur``.  Refused when the scenes differ in anything but their objects' positions (lights and
    cameras are not compared) or a position is not finite."""
    n = max(0, int(cur.num_objects))
    out = np.zeros((n, 3), np.float64)
    rc = lib().rt_scene_motion(ctypes.byref(prev.view), ctypes.byref(cur.view),
                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out.size)
    if rc < 0:
        _check(rc)
    return out


def temporal_motion_async(width: int, height: int, cur: TemporalFrame, prev, d_motion: int, num_objects: int,
                          d_out_color: int, d_out_count: int, d_out_rgba=None, params=None, stream: int = 0,
                          d_cur_albedo=None, d_prev_moments=None, d_out_moments=None):
    """rt_temporal_motion_async: temporal_async (with d_out_moments: temporal_moments_async)
    for objects that moved.  d_motion is a device pointer to num_objects rows of 3 doubles, row k the
    translation of object k from the previous frame to the current one; both frames must carry ``object``."""
    p = _as_temporal(params)
    m = Motion(d_motion, num_objects, 0)
    _check(lib().rt_temporal_motion_async(ctypes.byref(p), width, height, ctypes.byref(cur),
                                          ctypes.byref(prev) if prev is not None else None, ctypes.byref(m),
                                          ctypes.c_void_p(d_cur_albedo), ctypes.c_void_p(d_prev_moments),
                                          ctypes.c_void_p(d_out_color), ctypes.c_void_p(d_out_count),
                                          ctypes.c_void_p(d_out_moments), ctypes.c_void_p(d_out_rgba),
                                          ctypes.c_void_p(stream)))


def temporal_motion_host(cur: dict, prev=None, motion=None, params=None, moments: bool = False):
    """rt_temporal_motion_host: temporal_host (moments=True: temporal_moments_host, with ``albedo`` in cur and
    ``moments`` in prev) with ``motion``, an (num_objects, 3) float64 table.  Returns (color, count, rgba),
    or (color, count, moments, rgba)."""
    what = "temporal_motion_host"
    color = np.ascontiguousarray(cur["color"], np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise RenderError(f"{what}: color is an (H, W, 3) array")
    table = np.ascontiguousarray(motion, np.float64) if motion is not None else None
    if table is None or table.ndim != 2 or table.shape[1] != 3:
        raise RenderError(f"{what}: motion is a (num_objects, 3) array")
    h, w = color.shape[:2]
    keep = []

    def frame_of(d, name):
        a = _host_arrays(f"{what}: {name}", h, w, keep,
                         color=(d.get("color"), np.float32, (h, w, 3)), depth=(d.get("depth"), np.float32, (h, w)),
                         object=(d.get("object"), np.int32, (h, w)), normal=(d.get("normal"), np.float32, (h, w, 3)),
                         count=(d.get("count"), np.float32, (h, w)), albedo=(d.get("albedo"), np.float32, (h, w, 3)),
                         moments=(d.get("moments"), np.float32, (h, w, 2)))
        return temporal_frame(d["frame"], a["color"], a["depth"], a["object"], a["normal"], a["count"]), a

    fc, ac = frame_of(cur, "cur")
    fp, ap = frame_of(prev, "prev") if prev is not None else (None, {"moments": None})
    p = _as_temporal(params)
    m = Motion(table.ctypes.data, table.shape[0], 0)
    out = np.zeros((h, w, 3), np.float32)
    cnt = np.zeros((h, w), np.float32)
    mom = np.zeros((h, w, 2), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    _check(lib().rt_temporal_motion_host(ctypes.byref(p), w, h, ctypes.byref(fc),
                                         ctypes.byref(fp) if fp is not None else None, ctypes.byref(m),
                                         ac["albedo"] if moments else None, ap["moments"] if moments else None,
                                         out.ctypes.data, cnt.ctypes.data, mom.ctypes.data if moments else None,
                                         rgba.ctypes.data))
    return (out, cnt, mom, rgba) if moments else (out, cnt, rgba)


_HISTORY_CLIP_FIELDS = ("radius", "min_taps", "gamma", "min_half")


def default_history_clip(**over) -> HistoryClip:
    """rt_history_clip_default (radius 1, min_taps 5, gamma 1, min_half 0), with the given
    fields replaced."""
    c = HistoryClip()
    lib().rt_history_clip_default(ctypes.byref(c))
    for k, val in over.items():
        if k not in _HISTORY_CLIP_FIELDS:
            raise RenderError(f"default_history_clip: no such field {k}")
        setattr(c, k, val)
    return c


def _as_history_clip(params) -> HistoryClip:
    if isinstance(params, str) and params == "default":
        return default_history_clip()
    return _as_one(params, HistoryClip, default_history_clip, "clip")


def temporal_clip_async(width: int, height: int, cur: TemporalFrame, prev, d_out_color: int, d_out_count: int,
                        d_out_rgba=None, params=None, stream: int = 0, clip=None, d_motion=None, num_objects: int = 0,
                        d_cur_albedo=None, d_prev_moments=None, d_out_moments=None, d_out_clipped=None):
    """rt_temporal_clip_async: temporal_motion_async (d_motion None: temporal_async, or with
    d_out_moments temporal_moments_async) whose reprojected history is clipped to mean +- gamma * sigma of the
    current frame's neighbourhood.  clip: a HistoryClip, a dict of its fields or None (the defaults);
    d_cur_albedo demodulates the window and may be given without moments; d_out_clipped (W*H floats, 1 where
    a channel was clipped) is optional."""
    p = _as_temporal(params)
    c = _as_history_clip(clip)
    m = Motion(d_motion, num_objects, 0) if d_motion is not None else None
    _check(lib().rt_temporal_clip_async(ctypes.byref(p), width, height, ctypes.byref(cur),
                                        ctypes.byref(prev) if prev is not None else None,
                                        ctypes.byref(m) if m is not None else None, ctypes.byref(c),
                                        ctypes.c_void_p(d_cur_albedo), ctypes.c_void_p(d_prev_moments),
                                        ctypes.c_void_p(d_out_color), ctypes.c_void_p(d_out_count),
                                        ctypes.c_void_p(d_out_moments), ctypes.c_void_p(d_out_clipped),
                                        ctypes.c_void_p(d_out_rgba), ctypes.c_void_p(stream)))


def temporal_clip_host(cur: dict, prev=None, motion=None, params=None, moments: bool = False, clip=None):
    """rt_temporal_clip_host: temporal_motion_host (motion None: temporal_host / temporal_moments_host) with
    history rectification.  cur may hold ``albedo`` with and without moments.  Returns (color, count, clipped
    (H, W) float32, rgba), or (color, count, moments, clipped, rgba)."""
    what = "temporal_clip_host"
    color = np.ascontiguousarray(cur["color"], np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise RenderError(f"{what}: color is an (H, W, 3) array")
    table = np.ascontiguousarray(motion, np.float64) if motion is not None else None
    if table is not None and (table.ndim != 2 or table.shape[1] != 3):
        raise RenderError(f"{what}: motion is a (num_objects, 3) array or None")
    h, w = color.shape[:2]
    keep = []

    def frame_of(d, name):
        a = _host_arrays(f"{what}: {name}", h, w, keep,
                         color=(d.get("color"), np.float32, (h, w, 3)), depth=(d.get("depth"), np.float32, (h, w)),
                         object=(d.get("object"), np.int32, (h, w)), normal=(d.get("normal"), np.float32, (h, w, 3)),
                         count=(d.get("count"), np.float32, (h, w)), albedo=(d.get("albedo"), np.float32, (h, w, 3)),
                         moments=(d.get("moments"), np.float32, (h, w, 2)))
        return temporal_frame(d["frame"], a["color"], a["depth"], a["object"], a["normal"], a["count"]), a

    fc, ac = frame_of(cur, "cur")
    fp, ap = frame_of(prev, "prev") if prev is not None else (None, {"moments": None})
    p = _as_temporal(params)
    c = _as_history_clip(clip)
    m = Motion(table.ctypes.data, table.shape[0], 0) if table is not None else None
    out = np.zeros((h, w, 3), np.float32)
    cnt = np.zeros((h, w), np.float32)
    mom = np.zeros((h, w, 2), np.float32)
    clp = np.zeros((h, w), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    _check(lib().rt_temporal_clip_host(ctypes.byref(p), w, h, ctypes.byref(fc),
                                       ctypes.byref(fp) if fp is not None else None,
                                       ctypes.byref(m) if m is not None else None, ctypes.byref(c), ac["albedo"],
                                       ap["moments"] if moments else None, out.ctypes.data, cnt.ctypes.data,
                                       mom.ctypes.data if moments else None, clp.ctypes.data, rgba.ctypes.data))
    return (out, cnt, mom, clp, rgba) if moments else (out, cnt, clp, rgba)


def default_matte(**over) -> Matte:
    """rt_matte_default (ranks 4, level RT_MATTE_OBJECT), with the given fields replaced;
    level may be "object" or "face"."""
    m = Matte()
    lib().rt_matte_default(ctypes.byref(m))
    for k, v in over.items():
        if k not in ("ranks", "level"):
            raise RenderError(f"default_matte: no such field {k}")
        if k == "level" and isinstance(v, str):
            if v not in MATTE_LEVELS:
                raise RenderError(f"default_matte: level is one of {sorted(MATTE_LEVELS)}")
            v = MATTE_LEVELS[v]
        setattr(m, k, v)
    return m


def default_matte_resolve(**over) -> MatteResolve:
    """rt_matte_resolve_default (radius 2, background 0), with the given fields replaced."""
    r = MatteResolve()
    lib().rt_matte_resolve_default(ctypes.byref(r))
    for k, v in over.items():
        if k not in ("radius", "background"):
            raise RenderError(f"default_matte_resolve: no such field {k}")
        if k == "background":
            v = (ctypes.c_double * 3)(*[float(c) for c in v])
        setattr(r, k, v)
    return r


def matte_resolve_async(width: int, height: int, d_color: int, d_object: int, d_id: int, d_count: int, d_rest,
                        ranks: int, samples: int, d_out_linear=None, d_out_rgba=None, params=None, stream: int = 0):
    """rt_matte_resolve_async: every pointer a device pointer (an int; None: not given);
    asynchronous on ``stream``.  d_id and d_count are ``ranks`` planes of an object-level matte of
    ``samples`` samples, d_rest its rest plane or None; d_out_linear must not be d_color."""
    p = _as_one(params, MatteResolve, default_matte_resolve, "matte resolve")
    inp = MatteResolveInputs(d_color, d_object, d_id, d_count, d_rest, ranks, samples)
    _check(lib().rt_matte_resolve_async(ctypes.byref(p), width, height, ctypes.byref(inp),
                                        ctypes.c_void_p(d_out_linear), ctypes.c_void_p(d_out_rgba),
                                        ctypes.c_void_p(stream)))


def matte_resolve_host(color, object, id, count, rest=None, samples: int = 16, params=None):
    """rt_matte_resolve_host: the edge resolve on numpy arrays, without a device.  color is (H, W, 3)
    float32, object (H, W) int32, id and count (K, H, W) int32, rest (H, W) int32 or None.  Returns
    (linear (H, W, 3) float32, rgba (H, W, 4) uint8)."""
    what = "matte_resolve_host"
    color = np.ascontiguousarray(color, np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise RenderError(f"{what}: color is an (H, W, 3) array")
    h, w = color.shape[:2]
    count = np.ascontiguousarray(count, np.int32)
    if count.ndim != 3:
        raise RenderError(f"{what}: count is a (K, H, W) array")
    k = count.shape[0]
    keep = []
    a = _host_arrays(what, h, w, keep, object=(object, np.int32, (h, w)), id=(id, np.int32, (k, h, w)),
                     count=(count, np.int32, (k, h, w)), rest=(rest, np.int32, (h, w)))
    p = _as_one(params, MatteResolve, default_matte_resolve, "matte resolve")
    inp = MatteResolveInputs(color.ctypes.data, a["object"], a["id"], a["count"], a["rest"], k, int(samples))
    lin = np.zeros((h, w, 3), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    _check(lib().rt_matte_resolve_host(ctypes.byref(p), w, h, ctypes.byref(inp), lin.ctypes.data, rgba.ctypes.data))
    return lin, rgba


def matte_mask(matte: dict, key: int) -> np.ndarray:
    """The (H, W) float32 coverage of one key in a matte of ``ParallelRenderer.render_matte``: the sum over
    the ranks of ``coverage`` where ``id`` is the key (a key dropped from a pixel's ranks counts as 0 there)."""
    ids, cov = np.asarray(matte["id"]), np.asarray(matte["coverage"], np.float32)
    return np.where(ids == int(key), cov, np.float32(0)).sum(axis=0, dtype=np.float32)


def _as_matte_option(matte, what):
    """The (samples, ranks, MatteResolve) of a ``matte=`` option: True (16 samples, 4 ranks, the default
    resolve), an int number of samples, or a dict with any of samples, ranks, radius, background."""
    if matte is None or matte is False:
        return None
    opt = {}
    if matte is True:
        pass
    elif isinstance(matte, int):
        opt["samples"] = matte
    elif isinstance(matte, dict):
        opt = dict(matte)
    else:
        raise RenderError(f"{what}: matte is True, a number of samples or a dict")
    for k in opt:
        if k not in ("samples", "ranks", "radius", "background"):
            raise RenderError(f"{what}: matte has no field {k}")
    samples, ranks = int(opt.get("samples", 16)), int(opt.get("ranks", 4))
    if samples < 1 or not 1 <= ranks <= RT_MATTE_MAX_RANKS:
        raise RenderError(f"{what}: matte needs samples >= 1 and ranks in 1..{RT_MATTE_MAX_RANKS}")
    return samples, ranks, default_matte_resolve(**{k: opt[k] for k in ("radius", "background") if k in opt})


def variance_async(width: int, height: int, d_color: int, d_normal: int, d_depth: int, d_albedo=None, d_object=None,
                   d_moments=None, d_count=None, d_out_var: int = None, params=None, stream: int = 0):
    """rt_variance_async: every argument a device pointer (an int; None: not given);
    d_moments and d_count both or neither; asynchronous on ``stream``."""
    p = _as_one(params, Variance, default_variance, "variance")
    inp = VarianceInputs(d_color, d_normal, d_depth, d_albedo, d_object, d_moments, d_count)
    _check(lib().rt_variance_async(ctypes.byref(p), width, height, ctypes.byref(inp), ctypes.c_void_p(d_out_var),
                                   ctypes.c_void_p(stream)))


def variance_host(color, normal, depth, albedo=None, object=None, moments=None, count=None, params=None):
    """rt_variance_host: the variance pass on numpy arrays, without a device.  moments is (H, W, 2) float32,
    count (H, W) float32.  Returns the variance, (H, W) float32."""
    color = np.ascontiguousarray(color, np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise RenderError("variance_host: color is an (H, W, 3) array")
    h, w = color.shape[:2]
    keep = []
    a = _host_arrays("variance_host", h, w, keep, color=(color, np.float32, (h, w, 3)),
                     normal=(normal, np.float32, (h, w, 3)), depth=(depth, np.float32, (h, w)),
                     albedo=(albedo, np.float32, (h, w, 3)), object=(object, np.int32, (h, w)),
                     moments=(moments, np.float32, (h, w, 2)), count=(count, np.float32, (h, w)))
    p = _as_one(params, Variance, default_variance, "variance")
    inp = VarianceInputs(*[a[k] for k in ("color", "normal", "depth", "albedo", "object", "moments", "count")])
    out = np.zeros((h, w), np.float32)
    _check(lib().rt_variance_host(ctypes.byref(p), w, h, ctypes.byref(inp), out.ctypes.data))
    return out


def denoise_var_workspace_bytes(width: int, height: int) -> int:
    """rt_denoise_var_workspace_bytes: the device bytes rt_denoise_var_async needs for a width x height image."""
    return int(lib().rt_denoise_var_workspace_bytes(width, height))


def denoise_var_async(width: int, height: int, d_color: int, d_normal: int, d_depth: int, d_variance: int,
                      d_albedo=None, d_object=None, d_out_linear=None, d_out_rgba=None, d_out_variance=None,
                      d_workspace=None, workspace_bytes: int = 0, params=None, stream: int = 0):
    """rt_denoise_var_async: every argument a device pointer (an int; None: not given);
    asynchronous on ``stream``."""
    p = _as_one(params, DenoiseVar, default_denoise_var, "denoise_var")
    inp = DenoiseInputs(d_color, d_normal, d_depth, d_albedo, d_object)
    _check(lib().rt_denoise_var_async(ctypes.byref(p), width, height, ctypes.byref(inp), ctypes.c_void_p(d_variance),
                                      ctypes.c_void_p(d_out_linear), ctypes.c_void_p(d_out_rgba),
                                      ctypes.c_void_p(d_out_variance), ctypes.c_void_p(d_workspace), workspace_bytes,
                                      ctypes.c_void_p(stream)))


def denoise_var_host(color, normal, depth, variance, albedo=None, object=None, params=None):
    """rt_denoise_var_host: the variance-guided filter on numpy arrays, without a device.  variance is
    (H, W) float32.  Returns (linear (H, W, 3) float32, rgba (H, W, 4) uint8, variance (H, W) float32)."""
    color = np.ascontiguousarray(color, np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise RenderError("denoise_var_host: color is an (H, W, 3) array")
    h, w = color.shape[:2]
    keep = []
    a = _host_arrays("denoise_var_host", h, w, keep, color=(color, np.float32, (h, w, 3)),
                     normal=(normal, np.float32, (h, w, 3)), depth=(depth, np.float32, (h, w)),
                     albedo=(albedo, np.float32, (h, w, 3)), object=(object, np.int32, (h, w)),
                     variance=(variance, np.float32, (h, w)))
    p = _as_one(params, DenoiseVar, default_denoise_var, "denoise_var")
    inp = DenoiseInputs(*[a[k] for k in ("color", "normal", "depth", "albedo", "object")])
    lin = np.zeros((h, w, 3), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    var = np.zeros((h, w), np.float32)
    _check(lib().rt_denoise_var_host(ctypes.byref(p), w, h, ctypes.byref(inp), a["variance"], lin.ctypes.data,
                                     rgba.ctypes.data, var.ctypes.data))
    return lin, rgba, var


def max_local_tiles(width: int, height: int, world: int) -> int:
    return lib().rt_max_local_tiles(width, height, world)


def packed_bytes(width: int, height: int, world: int) -> int:
    """Bytes of one rank's packed share: float3 + RGBA8 per pixel of rank 0's tiles."""
    return lib().rt_packed_bytes(width, height, world)


def packed_rgba_offset(width: int, height: int, world: int) -> int:
    return lib().rt_packed_rgba_offset(width, height, world)


def unpack_tiles_async(width, height, world, d_gathered, d_linear, d_rgba, stream=0):
    """Scatter gathered shares [world][packed_bytes] into W*H images."""
    _check(
        lib().rt_unpack_tiles_async(
            width, height, world, ctypes.c_void_p(d_gathered), ctypes.c_void_p(d_linear), ctypes.c_void_p(d_rgba),
            ctypes.c_void_p(stream),
        )
    )


class Partition:
    """rt_partition: which rank renders each 32x32 tile (include/rt_api.h)."""

    def __init__(self, width=0, height=0, world=1, owner=None, _handle=None):
        if _handle is not None:
            self._h = _handle
            return
        self._h = ctypes.c_void_p()
        arr = None
        if owner is not None:
            owner = list(owner)
            arr = (ctypes.c_int32 * len(owner))(*owner)
        _check(lib().rt_partition_create(width, height, world, arr, ctypes.byref(self._h)))

    @property
    def world(self) -> int:
        return lib().rt_partition_world(self._h)

    def owner(self, tile: int) -> int:
        return lib().rt_partition_owner(self._h, tile)

    def owners(self, width: int, height: int) -> np.ndarray:
        return np.array([self.owner(t) for t in range(num_tiles(width, height))], np.int32)

    def local_tiles(self, rank: int) -> int:
        return lib().rt_partition_local_tiles(self._h, rank)

    def tiles(self, rank: int) -> list:
        return [lib().rt_partition_tile(self._h, rank, k) for k in range(self.local_tiles(rank))]

    @property
    def max_local(self) -> int:
        return lib().rt_partition_max_local(self._h)

    @property
    def packed_bytes(self) -> int:
        return lib().rt_partition_packed_bytes(self._h)

    @property
    def rgba_offset(self) -> int:
        return lib().rt_partition_rgba_offset(self._h)

    def work(self, rank: int) -> float:
        return lib().rt_partition_work(self._h, rank)

    def unpack_async(self, d_gathered, d_linear, d_rgba, stream=0):
        _check(lib().rt_unpack_partition_async(self._h, ctypes.c_void_p(d_gathered), ctypes.c_void_p(d_linear),
                                               ctypes.c_void_p(d_rgba), ctypes.c_void_p(stream)))

    def unpack_frames_async(self, nframes, d_gathered, d_linear, d_rgba, stream=0):
        """[world][nframes][packed bytes] -> [nframes][W*H] images."""
        _check(lib().rt_unpack_partition_frames_async(self._h, nframes, ctypes.c_void_p(d_gathered),
                                                      ctypes.c_void_p(d_linear), ctypes.c_void_p(d_rgba),
                                                      ctypes.c_void_p(stream)))

    def close(self):
        if self._h and _lib is not None:
            _lib.rt_partition_destroy(self._h)
        self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """rt_comm: the RCCL communicator of one process per GPU (rank 0 makes
    the id with ``unique_id()``; the caller broadcasts it)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (ctypes.c_uint8 * RT_COMM_ID_BYTES)()
        _check(lib().rt_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, uid: bytes, world: int, rank: int, device: int):
        buf = (ctypes.c_uint8 * RT_COMM_ID_BYTES)(*uid)
        self._h = ctypes.c_void_p()
        _check(lib().rt_comm_create(buf, world, rank, device, ctypes.byref(self._h)))

    def gather_bytes_async(self, share_bytes, d_share, d_gathered, stream=0):
        _check(lib().rt_comm_gather_bytes_async(self._h, share_bytes, ctypes.c_void_p(d_share),
                                                ctypes.c_void_p(d_gathered), ctypes.c_void_p(stream)))

    def gather_tiles_async(self, width, height, d_share, d_gathered, stream=0):
        _check(lib().rt_comm_gather_tiles_async(self._h, width, height, ctypes.c_void_p(d_share),
                                                ctypes.c_void_p(d_gathered), ctypes.c_void_p(stream)))

    def close(self):
        if self._h:
            lib().rt_comm_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
