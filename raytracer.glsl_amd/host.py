"""Host-side Python binding of the C ABI (include/rtgl_amd.h) plus a headless mirror of the
reference's Renderer/Window frame loop.  Used by tests/, bench.py and __graft_entry__.py.

There is no CPU fallback: if librtgl_amd.so is missing or no HIP device is present, everything here
raises.  (The C++ facade with the reference's class names lives in include/rtgl/.)
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import numpy as np

from .scenes import FrameParams, GlibcRand, Scene

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTGL_AMD_LIB") or os.path.join(PKG_DIR, "librtgl_amd.so")   # override: A/B of experimental builds
CSRC_DIR = os.path.join(PKG_DIR, "csrc")

KERNEL_MEGA, KERNEL_WAVEFRONT = 0, 1
# first-hit planes (option "aov", include/rtgl_amd.h): one bit per plane
AOV_ALBEDO, AOV_NORMAL, AOV_POSITION, AOV_IDS = 1, 2, 4, 8
AOV_ALL = AOV_ALBEDO | AOV_NORMAL | AOV_POSITION | AOV_IDS
# rtgl_denoise (include/rtgl_amd.h): flag bits and the documented defaults
DENOISE_DEMODULATE = 1
DENOISE_DEFAULTS = dict(passes=5, sigma_color=16.0, sigma_normal=0.3, sigma_position=0.05, demodulate=True)
# rtgl_denoise_guided
DENOISE_GUIDED_DEFAULTS = dict(passes=5, sigma_lum=4.0, sigma_normal=0.3, sigma_position=0.05, firefly_ratio=1.0, demodulate=True)
# rtgl_temporal_accumulate
TEMPORAL_DEFAULTS = dict(max_history=32.0, sigma_normal=0.3, sigma_position=0.05)
# rtgl_temporal_clip
TEMPORAL_CLIP_DEFAULTS = dict(sigma_scale=2.0, clip_history=3.0, sigma_normal=0.3, sigma_position=0.05)
# rtgl_tonemap (source: 0 image, 1 denoised, 2 temporal history; op: 0 linear, 1 Reinhard with white point, 2 ACES fit)
TONEMAP_DEFAULTS = dict(source=0, op=1, auto=True, exposure=1.0, key=0.18, white=4.0, adapt=1.0, exposure_min=2.0 ** -16, exposure_max=2.0 ** 16,
                        low_permille=100, high_permille=20)
TONEMAP_AUTO_EXPOSURE = 1
# rtgl_error_estimate
ERROR_DEFAULTS = dict(threshold=0.05, floor=0.01, quantile_permille=950, first_frames=1, keep_snapshot=False)
ERROR_KEEP_SNAPSHOT = 1
ERROR_TILE_DTYPE = np.dtype([("sum", np.float32), ("mse", np.float32), ("count", np.uint32), ("converged", np.uint32)])
# adaptive sampling (rtgl_adaptive_*)
ADAPTIVE_DEFAULTS = dict(threshold=0.05, floor=0.01, min_samples=16, max_samples=1024)
ADAPTIVE_TILE_DTYPE = np.dtype([("sum", np.float32), ("mse", np.float32), ("count", np.uint32), ("converged", np.uint32), ("samples", np.uint32),
                                ("samples_snapshot", np.uint32), ("reserved", np.uint32, (2,))])
# robust accumulation (rtgl_robust_*)
ROBUST_DEFAULTS = dict(buckets=8, gain=1.0, dest=0)
ROBUST_DEST_BUFFER, ROBUST_DEST_IMAGE = 0, 1
# rtgl_robust_error_estimate
ROBUST_ERROR_DEFAULTS = dict(threshold=0.05, floor=0.01, gain=1.0, quantile_permille=950)
# rtgl_robust_denoise
ROBUST_DENOISE_DEFAULTS = dict(passes=5, sigma_lum=4.0, sigma_normal=0.3, sigma_position=0.05, gain=1.0, demodulate=True)
# a robust adaptive session (rtgl_robust_adaptive_*)
ROBUST_ADAPTIVE_DEFAULTS = dict(buckets=8, threshold=0.05, floor=0.01, gain=1.0, min_samples=32, max_samples=1024)

# every symbol include/rtgl_amd.h declares
ABI_SYMBOLS = [
    "rtgl_create", "rtgl_create_tiled", "rtgl_destroy", "rtgl_last_error",
    "rtgl_upload_spheres", "rtgl_upload_materials", "rtgl_upload_meshes", "rtgl_upload_vertices",
    "rtgl_upload_nodes", "rtgl_upload_envmap", "rtgl_set_frame_params", "rtgl_render_frame",
    "rtgl_synchronize", "rtgl_read_image_f32", "rtgl_read_image_u8", "rtgl_write_image_f32",
    "rtgl_clear_image", "rtgl_local_rows", "rtgl_local_row_to_global", "rtgl_device_image",
    "rtgl_bind_device_image", "rtgl_set_stream", "rtgl_get_counters", "rtgl_read_rng_state",
    "rtgl_set_option", "rtgl_get_option", "rtgl_last_frame_ms", "rtgl_last_frame_timing",
    "rtgl_accumulated_timing", "rtgl_timing_reset", "rtgl_create_multi", "rtgl_device_count", "rtgl_gather_tiles",
    "rtgl_read_aov", "rtgl_device_aov", "rtgl_guides_frame",
    "rtgl_denoise_defaults", "rtgl_denoise", "rtgl_read_denoised_f32", "rtgl_device_denoised",
    "rtgl_denoise_guided_defaults", "rtgl_denoise_guided", "rtgl_read_denoise_variance_f32", "rtgl_device_denoise_variance",
    "rtgl_temporal_defaults", "rtgl_temporal_accumulate", "rtgl_temporal_reset", "rtgl_read_temporal_f32", "rtgl_device_temporal",
    "rtgl_read_temporal_moments_f32", "rtgl_device_temporal_moments",
    "rtgl_temporal_clip_defaults", "rtgl_temporal_clip",
    "rtgl_tonemap_defaults", "rtgl_tonemap", "rtgl_tonemap_reset", "rtgl_read_display_u8", "rtgl_device_display",
    "rtgl_read_tonemap_exposure", "rtgl_read_tonemap_histogram",
    "rtgl_error_defaults", "rtgl_error_estimate", "rtgl_error_reset", "rtgl_read_error_summary", "rtgl_read_error_tiles",
    "rtgl_device_error_tiles",
    "rtgl_adaptive_defaults", "rtgl_adaptive_begin", "rtgl_adaptive_frame", "rtgl_adaptive_update", "rtgl_adaptive_set_mask",
    "rtgl_adaptive_get_mask", "rtgl_read_adaptive_tiles", "rtgl_device_adaptive_tiles",
    "rtgl_robust_defaults", "rtgl_robust_begin", "rtgl_robust_accumulate", "rtgl_robust_resolve", "rtgl_robust_end", "rtgl_robust_frames",
    "rtgl_read_robust_f32", "rtgl_read_robust_bucket_f32",
    "rtgl_robust_error_defaults", "rtgl_robust_error_estimate", "rtgl_read_robust_error_summary", "rtgl_read_robust_error_tiles",
    "rtgl_device_robust_error_tiles",
    "rtgl_robust_denoise_defaults", "rtgl_robust_denoise",
    "rtgl_robust_adaptive_defaults", "rtgl_robust_adaptive_begin", "rtgl_robust_adaptive_frame", "rtgl_robust_adaptive_accumulate",
    "rtgl_robust_adaptive_update", "rtgl_robust_adaptive_set_mask", "rtgl_robust_adaptive_get_mask", "rtgl_robust_adaptive_resolve",
    "rtgl_robust_adaptive_end", "rtgl_read_robust_adaptive_f32", "rtgl_read_robust_adaptive_bucket_f32", "rtgl_read_robust_adaptive_tiles",
    "rtgl_device_robust_adaptive_tiles",
]


class RtglError(RuntimeError):
    pass


class CFrameParams(C.Structure):
    """rtgl_frame_params"""
    _fields_ = [("frames", C.c_int32), ("samples", C.c_uint32), ("max_bounce", C.c_uint32), ("time", C.c_float),
                ("background", C.c_float * 3), ("reset_flag", C.c_int32), ("use_envmap", C.c_int32),
                ("use_dof", C.c_int32), ("random", C.c_int32), ("camera_position", C.c_float * 3),
                ("camera_fov", C.c_float), ("camera_aperture", C.c_float), ("camera_focal_length", C.c_float),
                ("camera_forward", C.c_float * 3), ("camera_up", C.c_float * 3), ("camera_right", C.c_float * 3)]


class CCounters(C.Structure):
    """rtgl_counters"""
    _fields_ = [("paths", C.c_uint64), ("segments", C.c_uint64), ("triangle_tests", C.c_uint64),
                ("candidates", C.c_uint64), ("env_lookups", C.c_uint64), ("culled_tests", C.c_uint64), ("reserved", C.c_uint64 * 2)]


class CFrameTiming(C.Structure):
    """rtgl_frame_timing"""
    _fields_ = [("frame_ms", C.c_float), ("intersect_ms", C.c_float), ("intersect_launches", C.c_uint32), ("reserved", C.c_uint32)]


class CDenoiseParams(C.Structure):
    """rtgl_denoise_params"""
    _fields_ = [("passes", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class CDenoiseGuidedParams(C.Structure):
    """rtgl_denoise_guided_params"""
    _fields_ = [("passes", C.c_uint32), ("sigma_lum", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float),
                ("firefly_ratio", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class CTemporalParams(C.Structure):
    """rtgl_temporal_params"""
    _fields_ = [("max_history", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class CTemporalClipParams(C.Structure):
    """rtgl_temporal_clip_params"""
    _fields_ = [("sigma_scale", C.c_float), ("clip_history", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class CTonemapParams(C.Structure):
    """rtgl_tonemap_params"""
    _fields_ = [("source", C.c_uint32), ("op", C.c_uint32), ("flags", C.c_uint32), ("exposure", C.c_float), ("key", C.c_float),
                ("white", C.c_float), ("adapt", C.c_float), ("exposure_min", C.c_float), ("exposure_max", C.c_float),
                ("low_permille", C.c_uint32), ("high_permille", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class CErrorParams(C.Structure):
    """rtgl_error_params"""
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("quantile_permille", C.c_uint32), ("first_frames", C.c_int32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class CErrorSummary(C.Structure):
    """rtgl_error_summary"""
    _fields_ = [("valid", C.c_uint32), ("converged", C.c_uint32), ("frames_now", C.c_int32), ("frames_snapshot", C.c_int32),
                ("tiles_valid", C.c_uint32), ("tiles_converged", C.c_uint32), ("pixels_ignored", C.c_uint32), ("scale", C.c_float),
                ("mse", C.c_float), ("max_tile_mse", C.c_float), ("reserved", C.c_uint32 * 6)]


class CAdaptiveParams(C.Structure):
    """rtgl_adaptive_params"""
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class CAdaptiveSummary(C.Structure):
    """rtgl_adaptive_summary"""
    _fields_ = [("tiles_total", C.c_uint32), ("tiles_active", C.c_uint32), ("tiles_converged", C.c_uint32), ("tiles_capped", C.c_uint32),
                ("blocks_active", C.c_uint32), ("samples_min", C.c_uint32), ("samples_max", C.c_uint32), ("converged", C.c_uint32),
                ("samples_total", C.c_uint64), ("max_tile_mse", C.c_float), ("reserved", C.c_uint32 * 5)]


class CRobustParams(C.Structure):
    """rtgl_robust_params"""
    _fields_ = [("buckets", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 6)]


class CRobustResolveParams(C.Structure):
    """rtgl_robust_resolve_params"""
    _fields_ = [("gain", C.c_float), ("dest", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class CRobustErrorParams(C.Structure):
    """rtgl_robust_error_params"""
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("gain", C.c_float), ("quantile_permille", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class CRobustDenoiseParams(C.Structure):
    """rtgl_robust_denoise_params"""
    _fields_ = [("passes", C.c_uint32), ("sigma_lum", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float), ("gain", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class CRobustAdaptiveParams(C.Structure):
    """rtgl_robust_adaptive_params"""
    _fields_ = [("buckets", C.c_uint32), ("threshold", C.c_float), ("floor", C.c_float), ("gain", C.c_float), ("min_samples", C.c_uint32),
                ("max_samples", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


def build_library(force: bool = False) -> str:
    """hipcc-compile the HIP kernels + C ABI for gfx950 into librtgl_amd.so (in-tree)."""
    srcs = [os.path.join(CSRC_DIR, f) for f in os.listdir(CSRC_DIR) if f.endswith((".hip", ".hpp", ".h"))]
    srcs.append(os.path.join(PKG_DIR, "..", "include", "rtgl_amd.h"))
    stale = not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        # -B: `force` really recompiles (a library newer than its sources would otherwise make `make all` a no-op and a
        # stale binary could travel to the GPU box)
        subprocess.check_call(["make", "-s", "-C", CSRC_DIR] + (["-B"] if force else []) + ["all"])
    return LIB_PATH


_lib = None


def load_library() -> C.CDLL:
    """dlopen the product library; raises if it has not been built (no fallback of any kind)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtglError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc) first; there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, u32, i = C.c_void_p, C.c_uint32, C.c_int
    L.rtgl_create.argtypes = [C.POINTER(vp), i, i, i]
    L.rtgl_create_tiled.argtypes = [C.POINTER(vp), i, i, i, i, i, i]
    L.rtgl_create_multi.argtypes = [C.POINTER(vp), i, i, C.POINTER(i), i, i]
    L.rtgl_device_count.argtypes = [vp]
    L.rtgl_gather_tiles.argtypes = [vp]
    L.rtgl_destroy.argtypes = [vp]; L.rtgl_destroy.restype = None
    L.rtgl_last_error.argtypes = [vp]; L.rtgl_last_error.restype = C.c_char_p
    for name in ("rtgl_upload_spheres", "rtgl_upload_materials", "rtgl_upload_meshes", "rtgl_upload_vertices", "rtgl_upload_nodes"):
        getattr(L, name).argtypes = [vp, vp, u32]
    L.rtgl_upload_envmap.argtypes = [vp, vp, i, i, i, i]
    L.rtgl_set_frame_params.argtypes = [vp, C.POINTER(CFrameParams)]
    for name in ("rtgl_render_frame", "rtgl_guides_frame", "rtgl_synchronize", "rtgl_clear_image", "rtgl_local_rows"):
        getattr(L, name).argtypes = [vp]
    L.rtgl_read_image_f32.argtypes = [vp, vp]
    L.rtgl_read_image_u8.argtypes = [vp, vp, i]
    L.rtgl_write_image_f32.argtypes = [vp, vp]
    L.rtgl_local_row_to_global.argtypes = [vp, i]
    L.rtgl_device_image.argtypes = [vp]; L.rtgl_device_image.restype = vp
    L.rtgl_bind_device_image.argtypes = [vp, vp]
    L.rtgl_set_stream.argtypes = [vp, vp]
    L.rtgl_get_counters.argtypes = [vp, C.POINTER(CCounters)]
    L.rtgl_read_rng_state.argtypes = [vp, vp]
    L.rtgl_read_aov.argtypes = [vp, i, vp]
    L.rtgl_device_aov.argtypes = [vp, i]; L.rtgl_device_aov.restype = vp
    L.rtgl_denoise_defaults.argtypes = [C.POINTER(CDenoiseParams)]
    L.rtgl_denoise.argtypes = [vp, C.POINTER(CDenoiseParams)]
    L.rtgl_read_denoised_f32.argtypes = [vp, vp]
    L.rtgl_device_denoised.argtypes = [vp]; L.rtgl_device_denoised.restype = vp
    L.rtgl_denoise_guided_defaults.argtypes = [C.POINTER(CDenoiseGuidedParams)]
    L.rtgl_denoise_guided.argtypes = [vp, C.POINTER(CDenoiseGuidedParams)]
    L.rtgl_read_denoise_variance_f32.argtypes = [vp, vp]
    L.rtgl_device_denoise_variance.argtypes = [vp]; L.rtgl_device_denoise_variance.restype = vp
    L.rtgl_temporal_defaults.argtypes = [C.POINTER(CTemporalParams)]
    L.rtgl_temporal_accumulate.argtypes = [vp, C.POINTER(CTemporalParams)]
    L.rtgl_temporal_reset.argtypes = [vp]
    L.rtgl_read_temporal_f32.argtypes = [vp, vp]
    L.rtgl_device_temporal.argtypes = [vp]; L.rtgl_device_temporal.restype = vp
    L.rtgl_read_temporal_moments_f32.argtypes = [vp, vp]
    L.rtgl_device_temporal_moments.argtypes = [vp]; L.rtgl_device_temporal_moments.restype = vp
    L.rtgl_temporal_clip_defaults.argtypes = [C.POINTER(CTemporalClipParams)]
    L.rtgl_temporal_clip.argtypes = [vp, C.POINTER(CTemporalClipParams)]
    L.rtgl_tonemap_defaults.argtypes = [C.POINTER(CTonemapParams)]
    L.rtgl_tonemap.argtypes = [vp, C.POINTER(CTonemapParams)]
    L.rtgl_tonemap_reset.argtypes = [vp]
    L.rtgl_read_display_u8.argtypes = [vp, vp, i]
    L.rtgl_device_display.argtypes = [vp]; L.rtgl_device_display.restype = vp
    L.rtgl_read_tonemap_exposure.argtypes = [vp, C.POINTER(C.c_float)]
    L.rtgl_read_tonemap_histogram.argtypes = [vp, vp, C.POINTER(u32)]
    L.rtgl_error_defaults.argtypes = [C.POINTER(CErrorParams)]
    L.rtgl_error_estimate.argtypes = [vp, C.POINTER(CErrorParams)]
    L.rtgl_error_reset.argtypes = [vp]
    L.rtgl_read_error_summary.argtypes = [vp, C.POINTER(CErrorSummary)]
    L.rtgl_read_error_tiles.argtypes = [vp, vp, C.POINTER(u32), C.POINTER(u32)]
    L.rtgl_device_error_tiles.argtypes = [vp]; L.rtgl_device_error_tiles.restype = vp
    L.rtgl_adaptive_defaults.argtypes = [C.POINTER(CAdaptiveParams)]
    L.rtgl_adaptive_begin.argtypes = [vp, C.POINTER(CAdaptiveParams)]
    L.rtgl_adaptive_frame.argtypes = [vp]
    L.rtgl_adaptive_update.argtypes = [vp, C.POINTER(CAdaptiveSummary)]
    L.rtgl_adaptive_set_mask.argtypes = [vp, vp]
    L.rtgl_adaptive_get_mask.argtypes = [vp, vp]
    L.rtgl_read_adaptive_tiles.argtypes = [vp, vp, C.POINTER(u32), C.POINTER(u32)]
    L.rtgl_device_adaptive_tiles.argtypes = [vp]; L.rtgl_device_adaptive_tiles.restype = vp
    L.rtgl_robust_defaults.argtypes = [C.POINTER(CRobustParams), C.POINTER(CRobustResolveParams)]
    L.rtgl_robust_begin.argtypes = [vp, C.POINTER(CRobustParams)]
    L.rtgl_robust_accumulate.argtypes = [vp]
    L.rtgl_robust_resolve.argtypes = [vp, C.POINTER(CRobustResolveParams)]
    L.rtgl_robust_end.argtypes = [vp]
    L.rtgl_robust_frames.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.rtgl_read_robust_f32.argtypes = [vp, vp]
    L.rtgl_read_robust_bucket_f32.argtypes = [vp, u32, vp]
    L.rtgl_robust_error_defaults.argtypes = [C.POINTER(CRobustErrorParams)]
    L.rtgl_robust_error_estimate.argtypes = [vp, C.POINTER(CRobustErrorParams)]
    L.rtgl_read_robust_error_summary.argtypes = [vp, C.POINTER(CErrorSummary)]
    L.rtgl_read_robust_error_tiles.argtypes = [vp, vp, C.POINTER(u32), C.POINTER(u32)]
    L.rtgl_device_robust_error_tiles.argtypes = [vp]; L.rtgl_device_robust_error_tiles.restype = vp
    L.rtgl_robust_denoise_defaults.argtypes = [C.POINTER(CRobustDenoiseParams)]
    L.rtgl_robust_denoise.argtypes = [vp, C.POINTER(CRobustDenoiseParams)]
    L.rtgl_robust_adaptive_defaults.argtypes = [C.POINTER(CRobustAdaptiveParams)]
    L.rtgl_robust_adaptive_begin.argtypes = [vp, C.POINTER(CRobustAdaptiveParams)]
    L.rtgl_robust_adaptive_frame.argtypes = [vp]
    L.rtgl_robust_adaptive_accumulate.argtypes = [vp]
    L.rtgl_robust_adaptive_update.argtypes = [vp, C.POINTER(CAdaptiveSummary)]
    L.rtgl_robust_adaptive_set_mask.argtypes = [vp, vp]
    L.rtgl_robust_adaptive_get_mask.argtypes = [vp, vp]
    L.rtgl_robust_adaptive_resolve.argtypes = [vp, C.POINTER(CRobustResolveParams)]
    L.rtgl_robust_adaptive_end.argtypes = [vp]
    L.rtgl_read_robust_adaptive_f32.argtypes = [vp, vp]
    L.rtgl_read_robust_adaptive_bucket_f32.argtypes = [vp, u32, vp]
    L.rtgl_read_robust_adaptive_tiles.argtypes = [vp, vp, C.POINTER(u32), C.POINTER(u32)]
    L.rtgl_device_robust_adaptive_tiles.argtypes = [vp]; L.rtgl_device_robust_adaptive_tiles.restype = vp
    L.rtgl_set_option.argtypes = [vp, C.c_char_p, i]
    L.rtgl_get_option.argtypes = [vp, C.c_char_p, C.POINTER(i)]
    L.rtgl_last_frame_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rtgl_last_frame_timing.argtypes = [vp, C.POINTER(CFrameTiming)]
    L.rtgl_accumulated_timing.argtypes = [vp, C.POINTER(CFrameTiming), C.POINTER(C.c_uint32)]
    L.rtgl_timing_reset.argtypes = [vp]
    _lib = L
    return L


def to_c_params(p: FrameParams) -> CFrameParams:
    cp = CFrameParams()
    cp.frames, cp.samples, cp.max_bounce, cp.time = int(p.frames), int(p.samples), int(p.max_bounce), float(p.time)
    cp.background[:] = [float(x) for x in p.background]
    cp.reset_flag, cp.use_envmap, cp.use_dof, cp.random = int(p.reset_flag), int(p.use_envmap), int(p.use_dof), int(p.random)
    cp.camera_position[:] = [float(x) for x in p.camera_position]
    cp.camera_fov, cp.camera_aperture, cp.camera_focal_length = float(p.camera_fov), float(p.camera_aperture), float(p.camera_focal_length)
    cp.camera_forward[:] = [float(x) for x in p.camera_forward]
    cp.camera_up[:] = [float(x) for x in p.camera_up]
    cp.camera_right[:] = [float(x) for x in p.camera_right]
    return cp


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class Context:
    """One rtgl_context.  rank/world/strip_rows select row-strip tiling for multi-GPU runs."""

    def __init__(self, width: int, height: int, device: int = 0, rank: int = 0, world: int = 1, strip_rows: int = 16, devices=None):
        """devices=[ordinals]: one single-process multi-device context (rtgl_create_multi) instead of a (rank, world) tile."""
        self.lib = load_library()
        self.width, self.height = int(width), int(height)
        self.rank, self.world, self.strip_rows = rank, world, strip_rows
        h = C.c_void_p()
        if devices is not None:
            self.rank, self.world = 0, 1
            arr = (C.c_int * len(devices))(*devices)
            rc = self.lib.rtgl_create_multi(C.byref(h), width, height, arr, len(devices), strip_rows)
        else:
            rc = self.lib.rtgl_create_tiled(C.byref(h), width, height, device, rank, world, strip_rows)
        if rc != 0:
            raise RtglError(f"rtgl_create failed ({rc}): {self.lib.rtgl_last_error(None).decode()}")
        self.h = h
        self.local_rows = self.lib.rtgl_local_rows(self.h)

    def _chk(self, rc):
        if rc != 0:
            raise RtglError(f"rtgl call failed ({rc}): {self.lib.rtgl_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.rtgl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- scene
    def upload_spheres(self, a):
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 8); self._chk(self.lib.rtgl_upload_spheres(self.h, _ptr(a), a.shape[0]))

    def upload_materials(self, a):
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 8); self._chk(self.lib.rtgl_upload_materials(self.h, _ptr(a), a.shape[0]))

    def upload_meshes(self, a):
        a = np.ascontiguousarray(a, np.uint32).reshape(-1, 4); self._chk(self.lib.rtgl_upload_meshes(self.h, _ptr(a), a.shape[0]))

    def upload_vertices(self, a):
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 4); self._chk(self.lib.rtgl_upload_vertices(self.h, _ptr(a), a.shape[0]))

    def upload_nodes(self, a):
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 12); self._chk(self.lib.rtgl_upload_nodes(self.h, _ptr(a), a.shape[0]))

    def upload_envmap(self, env):
        if env is None:
            return
        e = np.ascontiguousarray(env, np.uint8)
        self._chk(self.lib.rtgl_upload_envmap(self.h, _ptr(e), e.shape[0], e.shape[2], e.shape[1], e.shape[3]))

    def upload_scene(self, s: Scene):
        self.upload_spheres(s.spheres); self.upload_materials(s.materials); self.upload_meshes(s.meshes)
        self.upload_vertices(s.vertices); self.upload_nodes(s.nodes); self.upload_envmap(s.env)

    # --- frames
    def set_params(self, p: FrameParams):
        cp = to_c_params(p)
        self._chk(self.lib.rtgl_set_frame_params(self.h, C.byref(cp)))

    def render(self, p: FrameParams | None = None, sync: bool = True):
        if p is not None:
            self.set_params(p)
        self._chk(self.lib.rtgl_render_frame(self.h))
        if sync:
            self._chk(self.lib.rtgl_synchronize(self.h))

    def guides_frame(self, p: FrameParams | None = None, sync: bool = True):
        """One guide pass (rtgl_guides_frame): the camera rays' first hits folded into the enabled first-hit planes, and nothing else."""
        if p is not None:
            self.set_params(p)
        self._chk(self.lib.rtgl_guides_frame(self.h))
        if sync:
            self._chk(self.lib.rtgl_synchronize(self.h))

    def synchronize(self):
        self._chk(self.lib.rtgl_synchronize(self.h))

    def last_frame_ms(self) -> float:
        ms = C.c_float()
        self._chk(self.lib.rtgl_last_frame_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def last_frame_timing(self) -> dict:
        t = CFrameTiming()
        self._chk(self.lib.rtgl_last_frame_timing(self.h, C.byref(t)))
        return dict(frame_ms=float(t.frame_ms), intersect_ms=float(t.intersect_ms), intersect_launches=int(t.intersect_launches))

    def accumulated_timing(self) -> dict:
        t, n = CFrameTiming(), C.c_uint32()
        self._chk(self.lib.rtgl_accumulated_timing(self.h, C.byref(t), C.byref(n)))
        return dict(frames=int(n.value), frame_ms=float(t.frame_ms), intersect_ms=float(t.intersect_ms), intersect_launches=int(t.intersect_launches))

    def timing_reset(self):
        self._chk(self.lib.rtgl_timing_reset(self.h))

    # --- image
    def read_image(self) -> np.ndarray:
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._chk(self.lib.rtgl_read_image_f32(self.h, _ptr(out)))
        return out

    def read_image_u8(self, flip: bool = False) -> np.ndarray:
        out = np.zeros((self.local_rows, self.width, 4), np.uint8)
        self._chk(self.lib.rtgl_read_image_u8(self.h, _ptr(out), int(flip)))
        return out

    def write_image(self, img: np.ndarray):
        img = np.ascontiguousarray(img, np.float32)
        assert img.shape == (self.local_rows, self.width, 4)
        self._chk(self.lib.rtgl_write_image_f32(self.h, _ptr(img)))

    def clear_image(self):
        self._chk(self.lib.rtgl_clear_image(self.h))

    def global_rows(self) -> np.ndarray:
        return np.array([self.lib.rtgl_local_row_to_global(self.h, r) for r in range(self.local_rows)], np.int64)

    def device_image_ptr(self) -> int:
        return int(self.lib.rtgl_device_image(self.h) or 0)

    def bind_device_image(self, ptr: int):
        self._chk(self.lib.rtgl_bind_device_image(self.h, C.c_void_p(ptr)))

    def set_stream(self, stream_handle: int):
        self._chk(self.lib.rtgl_set_stream(self.h, C.c_void_p(stream_handle)))

    # --- diagnostics
    def set_option(self, key: str, value: int):
        self._chk(self.lib.rtgl_set_option(self.h, key.encode(), int(value)))

    def get_option(self, key: str) -> int:
        v = C.c_int()
        self._chk(self.lib.rtgl_get_option(self.h, key.encode(), C.byref(v)))
        return int(v.value)

    def counters(self) -> dict:
        c = CCounters()
        self._chk(self.lib.rtgl_get_counters(self.h, C.byref(c)))
        return {k: int(getattr(c, k)) for k in ("paths", "segments", "triangle_tests", "candidates", "env_lookups", "culled_tests")}

    def read_rng_state(self) -> np.ndarray:
        out = np.zeros((self.local_rows, self.width, 4), np.uint32)
        self._chk(self.lib.rtgl_read_rng_state(self.h, _ptr(out)))
        return out

    # --- first-hit planes
    def set_aov(self, mask: int):
        """Enable the planes of `mask` (AOV_* bits; 0 frees them): allocated zeroed, their running mean restarts."""
        self.set_option("aov", mask)

    def read_aov(self, plane: int) -> np.ndarray:
        """One plane (a single AOV_* bit) as (local_rows, width, 4): int32 for AOV_IDS, float32 otherwise."""
        out = np.zeros((self.local_rows, self.width, 4), np.int32 if plane == AOV_IDS else np.float32)
        self._chk(self.lib.rtgl_read_aov(self.h, int(plane), _ptr(out)))
        return out

    def device_aov_ptr(self, plane: int) -> int:
        """Device pointer of one plane (0: see the context's last error)."""
        return int(self.lib.rtgl_device_aov(self.h, int(plane)) or 0)

    # --- denoiser
    def denoise(self, passes=None, sigma_color=None, sigma_normal=None, sigma_position=None, demodulate=None):
        """Enqueue the a-trous filter over the image as it stands (rtgl_denoise; does not wait).  An argument left at None keeps the
        library's default (DENOISE_DEFAULTS); a sigma <= 0 switches its term off."""
        p = CDenoiseParams()
        self._chk(self.lib.rtgl_denoise_defaults(C.byref(p)))
        if passes is not None:
            p.passes = int(passes)
        if sigma_color is not None:
            p.sigma_color = float(sigma_color)
        if sigma_normal is not None:
            p.sigma_normal = float(sigma_normal)
        if sigma_position is not None:
            p.sigma_position = float(sigma_position)
        if demodulate is not None:
            p.flags = (p.flags & ~DENOISE_DEMODULATE) | (DENOISE_DEMODULATE if demodulate else 0)
        self._chk(self.lib.rtgl_denoise(self.h, C.byref(p)))

    def read_denoised(self) -> np.ndarray:
        """The denoised buffer of the last denoise() as (local_rows, width, 4) float32, laid out like read_image()."""
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._chk(self.lib.rtgl_read_denoised_f32(self.h, _ptr(out)))
        return out

    def device_denoised_ptr(self) -> int:
        """Device pointer of the denoised buffer (0 before the first successful denoise(): see the context's last error)."""
        return int(self.lib.rtgl_device_denoised(self.h) or 0)

    def denoise_guided(self, passes=None, sigma_lum=None, sigma_normal=None, sigma_position=None, firefly_ratio=None, demodulate=None):
        """Enqueue the variance-guided filter over the image as it stands (rtgl_denoise_guided; does not wait).  It writes the buffer
        read_denoised() returns and the variance buffer.  An argument left at None keeps the library's default (DENOISE_GUIDED_DEFAULTS);
        sigma_normal, sigma_position or firefly_ratio <= 0 switches that term or the clamp off."""
        p = CDenoiseGuidedParams()
        self._chk(self.lib.rtgl_denoise_guided_defaults(C.byref(p)))
        if passes is not None:
            p.passes = int(passes)
        for name, value in (("sigma_lum", sigma_lum), ("sigma_normal", sigma_normal), ("sigma_position", sigma_position), ("firefly_ratio", firefly_ratio)):
            if value is not None:
                setattr(p, name, float(value))
        if demodulate is not None:
            p.flags = (p.flags & ~DENOISE_DEMODULATE) | (DENOISE_DEMODULATE if demodulate else 0)
        self._chk(self.lib.rtgl_denoise_guided(self.h, C.byref(p)))

    def read_denoise_variance(self) -> np.ndarray:
        """{mu, v0, variance after the last pass, s0} per pixel of the last denoise_guided(), (local_rows, width, 4) float32."""
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._chk(self.lib.rtgl_read_denoise_variance_f32(self.h, _ptr(out)))
        return out

    def device_denoise_variance_ptr(self) -> int:
        """Device pointer of the variance buffer (0 before the first successful denoise_guided(): see the context's last error)."""
        return int(self.lib.rtgl_device_denoise_variance(self.h) or 0)

    # --- temporal accumulation
    def temporal_accumulate(self, max_history=None, sigma_normal=None, sigma_position=None):
        """Enqueue one step of the reprojected history (rtgl_temporal_accumulate; does not wait): the previous call's history carried
        through the previous camera into the view of the current frame parameters and blended with the image as it stands.  An argument
        left at None keeps the library's default (TEMPORAL_DEFAULTS); a sigma <= 0 switches its test off."""
        p = CTemporalParams()
        self._chk(self.lib.rtgl_temporal_defaults(C.byref(p)))
        for name, value in (("max_history", max_history), ("sigma_normal", sigma_normal), ("sigma_position", sigma_position)):
            if value is not None:
                setattr(p, name, float(value))
        self._chk(self.lib.rtgl_temporal_accumulate(self.h, C.byref(p)))

    def temporal_reset(self):
        """The next temporal_accumulate() starts without history."""
        self._chk(self.lib.rtgl_temporal_reset(self.h))

    def read_temporal(self) -> np.ndarray:
        """The history the last temporal_accumulate() wrote as (local_rows, width, 4) float32: rgb and the history length n."""
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._chk(self.lib.rtgl_read_temporal_f32(self.h, _ptr(out)))
        return out

    def device_temporal_ptr(self) -> int:
        """Device pointer of the history buffer the LATEST temporal_accumulate() wrote (two buffers take turns: ask after each call;
        0 before the first successful call: see the context's last error)."""
        return int(self.lib.rtgl_device_temporal(self.h) or 0)

    def read_temporal_moments(self) -> np.ndarray:
        """The luminance moments {m1, m2, v, n} the last temporal_accumulate() stored (option "temporal_moments" 1 or 2) as
        (local_rows, width, 4) float32."""
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._chk(self.lib.rtgl_read_temporal_moments_f32(self.h, _ptr(out)))
        return out

    def device_temporal_moments_ptr(self) -> int:
        """Device pointer of the moments buffer the LATEST temporal_accumulate() wrote (two buffers take turns with the history's; 0 unless
        that call stored moments: see the context's last error)."""
        return int(self.lib.rtgl_device_temporal_moments(self.h) or 0)

    def temporal_clip(self, sigma_scale=None, clip_history=None, sigma_normal=None, sigma_position=None):
        """Enqueue the clamp of the latest history into the current frame's neighbourhood colour box (rtgl_temporal_clip; does not wait;
        call it after temporal_accumulate()): where a pixel is clamped its history length is cut to clip_history.  An argument left at None
        keeps the library's default (TEMPORAL_CLIP_DEFAULTS); a sigma <= 0 switches its term of the geometric weight off."""
        p = CTemporalClipParams()
        self._chk(self.lib.rtgl_temporal_clip_defaults(C.byref(p)))
        for name, value in (("sigma_scale", sigma_scale), ("clip_history", clip_history), ("sigma_normal", sigma_normal), ("sigma_position", sigma_position)):
            if value is not None:
                setattr(p, name, float(value))
        self._chk(self.lib.rtgl_temporal_clip(self.h, C.byref(p)))

    # --- display transform
    def tonemap(self, source=None, op=None, auto=None, exposure=None, key=None, white=None, adapt=None, exposure_min=None, exposure_max=None,
                low_permille=None, high_permille=None):
        """Enqueue the display transform (rtgl_tonemap; does not wait): the image (source 0), the denoised buffer (1) or the temporal
        history (2) exposed, tone-mapped (op 0 linear, 1 Reinhard with white point, 2 ACES fit) and sRGB-encoded into the RGBA8 display
        buffer.  auto: the exposure is solved on the device from a luminance histogram; otherwise `exposure` is used as given.  An
        argument left at None keeps the library's default (TONEMAP_DEFAULTS)."""
        p = CTonemapParams()
        self._chk(self.lib.rtgl_tonemap_defaults(C.byref(p)))
        for name, value in (("source", source), ("op", op), ("low_permille", low_permille), ("high_permille", high_permille)):
            if value is not None:
                setattr(p, name, int(value))
        for name, value in (("exposure", exposure), ("key", key), ("white", white), ("adapt", adapt), ("exposure_min", exposure_min), ("exposure_max", exposure_max)):
            if value is not None:
                setattr(p, name, float(value))
        if auto is not None:
            p.flags = (p.flags & ~TONEMAP_AUTO_EXPOSURE) | (TONEMAP_AUTO_EXPOSURE if auto else 0)
        self._chk(self.lib.rtgl_tonemap(self.h, C.byref(p)))

    def tonemap_reset(self):
        """The next tonemap() takes its target exposure at once, whatever `adapt`."""
        self._chk(self.lib.rtgl_tonemap_reset(self.h))

    def read_display(self, flip: bool = False) -> np.ndarray:
        """The display buffer the last tonemap() wrote as (local_rows, width, 4) uint8, row 0 = bottom unless flip."""
        out = np.zeros((self.local_rows, self.width, 4), np.uint8)
        self._chk(self.lib.rtgl_read_display_u8(self.h, _ptr(out), int(flip)))
        return out

    def device_display_ptr(self) -> int:
        """Device pointer of the RGBA8 display buffer (0 before the first successful tonemap(): see the context's last error)."""
        return int(self.lib.rtgl_device_display(self.h) or 0)

    def read_tonemap_exposure(self) -> np.float32:
        """The exposure the last tonemap() applied."""
        e = C.c_float()
        self._chk(self.lib.rtgl_read_tonemap_exposure(self.h, C.byref(e)))
        return np.float32(e.value)

    def read_tonemap_histogram(self):
        """(bins uint32[256], ignored) of the last tonemap() with auto exposure: eight bins per binade of luminance from 2^-16 to 2^16,
        and the pixels whose luminance is not > 0."""
        hist, ignored = np.zeros(256, np.uint32), C.c_uint32()
        self._chk(self.lib.rtgl_read_tonemap_histogram(self.h, _ptr(hist), C.byref(ignored)))
        return hist, int(ignored.value)

    # --- error estimate
    def error_estimate(self, threshold=None, floor=None, quantile_permille=None, first_frames=None, keep_snapshot=None):
        """Enqueue the error estimate of the accumulation image (rtgl_error_estimate; does not wait): the relative MSE of the luminance
        per 16 x 16 tile and for the picture, from the image and the snapshot the previous call left, and whether `quantile_permille` of
        the tiles are at or below `threshold` (a relative RMSE).  first_frames: the `frames` of the first frame after the image was last
        zero.  keep_snapshot: leave an existing snapshot as it is.  The first call (and the first after anything that restarts the
        accumulation) only takes the snapshot: its summary has valid = 0.  None keeps the library's default (ERROR_DEFAULTS)."""
        p = CErrorParams()
        self._chk(self.lib.rtgl_error_defaults(C.byref(p)))
        for name, value in (("threshold", threshold), ("floor", floor)):
            if value is not None:
                setattr(p, name, float(value))
        for name, value in (("quantile_permille", quantile_permille), ("first_frames", first_frames)):
            if value is not None:
                setattr(p, name, int(value))
        if keep_snapshot is not None:
            p.flags = (p.flags & ~ERROR_KEEP_SNAPSHOT) | (ERROR_KEEP_SNAPSHOT if keep_snapshot else 0)
        self._chk(self.lib.rtgl_error_estimate(self.h, C.byref(p)))

    def error_reset(self):
        """Drop the snapshot: the next error_estimate() takes a new one."""
        self._chk(self.lib.rtgl_error_reset(self.h))

    @staticmethod
    def _summary_dict(s: CErrorSummary) -> dict:
        out = {k: int(getattr(s, k)) for k in ("valid", "converged", "frames_now", "frames_snapshot", "tiles_valid", "tiles_converged", "pixels_ignored")}
        raw = np.frombuffer(bytes(s), np.float32)                      # (the bits, not a round trip through a Python float)
        out.update(scale=raw[7], mse=raw[8], max_tile_mse=raw[9])
        return out

    def read_error_summary(self) -> dict:
        """The summary of the last error_estimate() (synchronises): valid, converged, frames_now, frames_snapshot, tiles_valid,
        tiles_converged, pixels_ignored as int, scale, mse, max_tile_mse as np.float32."""
        s = CErrorSummary()
        self._chk(self.lib.rtgl_read_error_summary(self.h, C.byref(s)))
        return self._summary_dict(s)

    def read_error_tiles(self) -> np.ndarray:
        """The tile records of the last error_estimate() as a structured array (ty, tx) of ERROR_TILE_DTYPE; tile row 0 = image row 0."""
        tx, ty = (self.width + 15) // 16, (self.height + 15) // 16
        out = np.zeros((ty, tx), ERROR_TILE_DTYPE)
        nx, ny = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.rtgl_read_error_tiles(self.h, _ptr(out), C.byref(nx), C.byref(ny)))
        assert (int(nx.value), int(ny.value)) == (tx, ty)
        return out

    def device_error_tiles_ptr(self) -> int:
        """Device pointer of the tile records (0 before the first successful error_estimate(): see the context's last error)."""
        return int(self.lib.rtgl_device_error_tiles(self.h) or 0)

    # --- masked tiles: what adaptive_* and robust_adaptive_* share; `fn` is the library function of the caller's kind
    def _tiles_shape(self):
        return (self.height + 15) // 16, (self.width + 15) // 16

    def _tile_update(self, fn) -> dict:
        s = CAdaptiveSummary()
        self._chk(fn(self.h, C.byref(s)))
        out = {k: int(getattr(s, k)) for k in ("tiles_total", "tiles_active", "tiles_converged", "tiles_capped", "blocks_active", "samples_min",
                                               "samples_max", "converged", "samples_total")}
        out["max_tile_mse"] = np.frombuffer(bytes(s), np.float32)[10]      # (the bits, not a round trip through a Python float)
        return out

    def _tile_set_mask(self, fn, tiles):
        t = np.ascontiguousarray(np.asarray(tiles) != 0, np.uint8)
        assert t.shape == self._tiles_shape()
        self._chk(fn(self.h, _ptr(t)))

    def _tile_get_mask(self, fn) -> np.ndarray:
        out = np.zeros(self._tiles_shape(), np.uint8)
        self._chk(fn(self.h, _ptr(out)))
        return out

    def _tile_records(self, fn) -> np.ndarray:
        out = np.zeros(self._tiles_shape(), ADAPTIVE_TILE_DTYPE)
        nx, ny = C.c_uint32(), C.c_uint32()
        self._chk(fn(self.h, _ptr(out), C.byref(nx), C.byref(ny)))
        assert (int(ny.value), int(nx.value)) == out.shape
        return out

    # --- adaptive sampling
    def adaptive_begin(self, threshold=None, floor=None, min_samples=None, max_samples=None):
        """Open a session of masked frames (rtgl_adaptive_begin): the image is cleared, every tile is active and has no sample.  None keeps
        the library's default (ADAPTIVE_DEFAULTS)."""
        p = CAdaptiveParams()
        self._chk(self.lib.rtgl_adaptive_defaults(C.byref(p)))
        for name, value in (("threshold", threshold), ("floor", floor)):
            if value is not None:
                setattr(p, name, float(value))
        for name, value in (("min_samples", min_samples), ("max_samples", max_samples)):
            if value is not None:
                setattr(p, name, int(value))
        self._chk(self.lib.rtgl_adaptive_begin(self.h, C.byref(p)))

    def adaptive_frame(self, p: FrameParams | None = None, sync: bool = True):
        """One frame of one sample over the active tiles (rtgl_adaptive_frame), with the parameters `p` if given."""
        if p is not None:
            self.set_params(p)
        self._chk(self.lib.rtgl_adaptive_frame(self.h))
        if sync:
            self._chk(self.lib.rtgl_synchronize(self.h))

    def adaptive_update(self) -> dict:
        """Estimate the tiles that were sampled since their snapshot, set the mask from the records (rtgl_adaptive_update; synchronises)
        and return the summary: ints, and max_tile_mse as np.float32."""
        return self._tile_update(self.lib.rtgl_adaptive_update)

    def adaptive_set_mask(self, tiles):
        """An explicit mask (ty, tx), non-zero = active, until the next adaptive_update()."""
        self._tile_set_mask(self.lib.rtgl_adaptive_set_mask, tiles)

    def adaptive_get_mask(self) -> np.ndarray:
        return self._tile_get_mask(self.lib.rtgl_adaptive_get_mask)

    def read_adaptive_tiles(self) -> np.ndarray:
        """The tile records as a structured array (ty, tx) of ADAPTIVE_TILE_DTYPE; tile row 0 = image row 0."""
        return self._tile_records(self.lib.rtgl_read_adaptive_tiles)

    def device_adaptive_tiles_ptr(self) -> int:
        """Device pointer of the tile records (0 before the first adaptive_begin(): see the context's last error)."""
        return int(self.lib.rtgl_device_adaptive_tiles(self.h) or 0)

    # --- robust accumulation
    def robust_begin(self, buckets=None):
        """Open a session of robust accumulation (rtgl_robust_begin): `buckets` zeroed bucket planes of this context's rows and no frame
        yet.  None keeps the library's default (ROBUST_DEFAULTS)."""
        p = CRobustParams()
        self._chk(self.lib.rtgl_robust_defaults(C.byref(p), None))
        if buckets is not None:
            p.buckets = int(buckets)
        self._chk(self.lib.rtgl_robust_begin(self.h, C.byref(p)))

    def robust_accumulate(self):
        """Fold the image as it stands, taken as one sample, into the next bucket (rtgl_robust_accumulate)."""
        self._chk(self.lib.rtgl_robust_accumulate(self.h))

    def _resolve(self, fn, gain, dest):      # (robust_resolve and robust_adaptive_resolve)
        p = CRobustResolveParams()
        self._chk(self.lib.rtgl_robust_defaults(None, C.byref(p)))
        if gain is not None:
            p.gain = float(gain)
        if dest is not None:
            p.dest = int(dest)
        self._chk(fn(self.h, C.byref(p)))

    def robust_resolve(self, gain=None, dest=None):
        """The trimmed mean of the buckets (rtgl_robust_resolve) into the output plane (dest ROBUST_DEST_BUFFER: read_robust()) or into
        the accumulation image (ROBUST_DEST_IMAGE).  None keeps the library's default."""
        self._resolve(self.lib.rtgl_robust_resolve, gain, dest)

    def robust_end(self):
        self._chk(self.lib.rtgl_robust_end(self.h))

    def robust_frames(self):
        """(frames folded since robust_begin(), buckets)"""
        n, k = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.rtgl_robust_frames(self.h, C.byref(n), C.byref(k)))
        return int(n.value), int(k.value)

    def read_robust(self) -> np.ndarray:
        """The output plane of the latest robust_resolve() with dest ROBUST_DEST_BUFFER: this context's rows, RGB and the Gini coefficient."""
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._chk(self.lib.rtgl_read_robust_f32(self.h, _ptr(out)))
        return out

    def read_robust_bucket(self, j: int) -> np.ndarray:
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._chk(self.lib.rtgl_read_robust_bucket_f32(self.h, int(j), _ptr(out)))
        return out

    # --- robust error estimate
    def robust_error_estimate(self, threshold=None, floor=None, gain=None, quantile_permille=None):
        """Enqueue the error estimate of the open robust session (rtgl_robust_error_estimate; does not wait): the relative MSE of the
        luminance of the picture robust_resolve(gain=gain) makes, per 16 x 16 tile and for the picture, from the spread of the buckets, and
        whether `quantile_permille` of the tiles are at or below `threshold` (a relative RMSE).  Needs at least as many frames as buckets.
        None keeps the library's default (ROBUST_ERROR_DEFAULTS)."""
        p = CRobustErrorParams()
        self._chk(self.lib.rtgl_robust_error_defaults(C.byref(p)))
        for name, value in (("threshold", threshold), ("floor", floor), ("gain", gain)):
            if value is not None:
                setattr(p, name, float(value))
        if quantile_permille is not None:
            p.quantile_permille = int(quantile_permille)
        self._chk(self.lib.rtgl_robust_error_estimate(self.h, C.byref(p)))

    def read_robust_error_summary(self) -> dict:
        """The summary of the session's last robust_error_estimate() (synchronises), with the fields of read_error_summary():
        frames_now is the session's frame count, frames_snapshot 0 and scale 1."""
        s = CErrorSummary()
        self._chk(self.lib.rtgl_read_robust_error_summary(self.h, C.byref(s)))
        return self._summary_dict(s)

    def read_robust_error_tiles(self) -> np.ndarray:
        """The tile records of the session's last robust_error_estimate() as a structured array (ty, tx) of ERROR_TILE_DTYPE."""
        out = np.zeros(self._tiles_shape(), ERROR_TILE_DTYPE)
        nx, ny = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.rtgl_read_robust_error_tiles(self.h, _ptr(out), C.byref(nx), C.byref(ny)))
        assert (int(ny.value), int(nx.value)) == out.shape
        return out

    def device_robust_error_tiles_ptr(self) -> int:
        """Device pointer of those records (0 before the session's first successful robust_error_estimate(): see the context's last error)."""
        return int(self.lib.rtgl_device_robust_error_tiles(self.h) or 0)

    # --- a robust adaptive session
    def robust_adaptive_begin(self, buckets=None, threshold=None, floor=None, gain=None, min_samples=None, max_samples=None):
        """Open a robust adaptive session (rtgl_robust_adaptive_begin): zeroed bucket planes, every tile active and without a sample; the
        image is not touched.  None keeps the library's default (ROBUST_ADAPTIVE_DEFAULTS)."""
        p = CRobustAdaptiveParams()
        self._chk(self.lib.rtgl_robust_adaptive_defaults(C.byref(p)))
        for name, value in (("threshold", threshold), ("floor", floor), ("gain", gain)):
            if value is not None:
                setattr(p, name, float(value))
        for name, value in (("buckets", buckets), ("min_samples", min_samples), ("max_samples", max_samples)):
            if value is not None:
                setattr(p, name, int(value))
        self._chk(self.lib.rtgl_robust_adaptive_begin(self.h, C.byref(p)))

    def robust_adaptive_frame(self, p: FrameParams | None = None, sync: bool = True):
        """One frame of one sample over the active tiles, folded into the bucket of each tile's next sample (rtgl_robust_adaptive_frame),
        with the parameters `p` if given."""
        if p is not None:
            self.set_params(p)
        self._chk(self.lib.rtgl_robust_adaptive_frame(self.h))
        if sync:
            self._chk(self.lib.rtgl_synchronize(self.h))

    def robust_adaptive_accumulate(self):
        """The fold with the image as it stands as the sample of every active tile (rtgl_robust_adaptive_accumulate)."""
        self._chk(self.lib.rtgl_robust_adaptive_accumulate(self.h))

    def robust_adaptive_update(self) -> dict:
        """Estimate the tiles whose count has moved, set the mask from the records (rtgl_robust_adaptive_update; synchronises) and return
        the summary as adaptive_update() does."""
        return self._tile_update(self.lib.rtgl_robust_adaptive_update)

    def robust_adaptive_set_mask(self, tiles):
        """An explicit mask (ty, tx), non-zero = active, until the next robust_adaptive_update()."""
        self._tile_set_mask(self.lib.rtgl_robust_adaptive_set_mask, tiles)

    def robust_adaptive_get_mask(self) -> np.ndarray:
        return self._tile_get_mask(self.lib.rtgl_robust_adaptive_get_mask)

    def robust_adaptive_resolve(self, gain=None, dest=None):
        """The trimmed mean of the buckets with every pixel's N taken from its tile (rtgl_robust_adaptive_resolve) into the session's output
        plane (dest ROBUST_DEST_BUFFER: read_robust_adaptive()) or into the accumulation image (ROBUST_DEST_IMAGE)."""
        self._resolve(self.lib.rtgl_robust_adaptive_resolve, gain, dest)

    def robust_adaptive_end(self):
        self._chk(self.lib.rtgl_robust_adaptive_end(self.h))

    def read_robust_adaptive(self) -> np.ndarray:
        """The output plane of the latest robust_adaptive_resolve() with dest ROBUST_DEST_BUFFER: RGB and the Gini coefficient."""
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._chk(self.lib.rtgl_read_robust_adaptive_f32(self.h, _ptr(out)))
        return out

    def read_robust_adaptive_bucket(self, j: int) -> np.ndarray:
        out = np.zeros((self.local_rows, self.width, 4), np.float32)
        self._chk(self.lib.rtgl_read_robust_adaptive_bucket_f32(self.h, int(j), _ptr(out)))
        return out

    def read_robust_adaptive_tiles(self) -> np.ndarray:
        """The session's tile records as a structured array (ty, tx) of ADAPTIVE_TILE_DTYPE; tile row 0 = image row 0."""
        return self._tile_records(self.lib.rtgl_read_robust_adaptive_tiles)

    def device_robust_adaptive_tiles_ptr(self) -> int:
        """Device pointer of those records (0 without a session: see the context's last error)."""
        return int(self.lib.rtgl_device_robust_adaptive_tiles(self.h) or 0)

    # --- robust denoise
    def robust_denoise(self, passes=None, sigma_lum=None, sigma_normal=None, sigma_position=None, gain=None, demodulate=None):
        """Enqueue the resolve of the open robust session and the variance-guided filter over it in one call (rtgl_robust_denoise; does
        not wait): the luminance tolerance of every pixel comes from the spread of its own buckets.  It writes the buffer read_denoised()
        returns and the variance buffer {lum(c0), v0, variance after the last pass, buckets kept}; the session, the image and the
        first-hit planes are only read.  Needs at least as many frames as buckets.  An argument left at None keeps the library's default
        (ROBUST_DENOISE_DEFAULTS); sigma_normal or sigma_position <= 0 switches that term off."""
        p = CRobustDenoiseParams()
        self._chk(self.lib.rtgl_robust_denoise_defaults(C.byref(p)))
        if passes is not None:
            p.passes = int(passes)
        for name, value in (("sigma_lum", sigma_lum), ("sigma_normal", sigma_normal), ("sigma_position", sigma_position), ("gain", gain)):
            if value is not None:
                setattr(p, name, float(value))
        if demodulate is not None:
            p.flags = (p.flags & ~DENOISE_DEMODULATE) | (DENOISE_DEMODULATE if demodulate else 0)
        self._chk(self.lib.rtgl_robust_denoise(self.h, C.byref(p)))


class FrameLoop:
    """Pure host logic of the reference's Window::run + Renderer::render frame bookkeeping (no GPU):
    m_frames is incremented BEFORE render (src/window.cpp:42), u_random = rand() once per frame after
    srand(0) (src/main.cpp:207, src/renderer.cpp:102), a reset uploads the stale frame count with
    u_reset_flag = 1 and then zeroes the count (src/renderer.cpp:98,123-127)."""

    def __init__(self, params: FrameParams | None = None, seed: int = 0):
        self.params = params or FrameParams()
        self.m_frames = 0
        self.m_reset = False
        self._rand = GlibcRand(seed)

    def reset_buffer(self):
        self.m_reset = True

    def next_frame(self) -> FrameParams:
        self.m_frames += 1
        p = self.params.replace(frames=self.m_frames, random=self._rand.rand(), reset_flag=int(self.m_reset))
        if self.m_reset:
            self.m_reset = False
            self.m_frames = 0
        return p

    def session_frame(self, reset_flag: int = 0) -> FrameParams:
        """The uniforms of one frame of an adaptive or robust session (renderer.h's adaptive_frame() / robust_frame()): one rand(), like
        every frame, but frames = 0, the frame count is not advanced and a pending reset stays pending for the next next_frame()."""
        return self.params.replace(frames=0, reset_flag=reset_flag, random=self._rand.rand())


class HeadlessRenderer(FrameLoop):
    """FrameLoop driving a Context: the Python twin of include/rtgl/renderer.h's Renderer."""

    def __init__(self, width: int, height: int, device: int = 0, seed: int = 0, aov: int = 0, **tiling):
        super().__init__(seed=seed)
        self.ctx = Context(width, height, device, **tiling)
        if aov:
            self.set_aov(aov)

    def set_aov(self, mask: int):
        self.ctx.set_aov(mask)

    def read_aov(self, plane: int) -> np.ndarray:
        return self.ctx.read_aov(plane)

    def denoise(self, **params):
        self.ctx.denoise(**params)

    def denoise_guided(self, **params):
        self.ctx.denoise_guided(**params)

    def read_denoise_variance(self) -> np.ndarray:
        return self.ctx.read_denoise_variance()

    def read_denoised(self) -> np.ndarray:
        return self.ctx.read_denoised()

    def device_denoised_ptr(self) -> int:
        return self.ctx.device_denoised_ptr()

    def temporal_accumulate(self, **params):
        self.ctx.temporal_accumulate(**params)

    def temporal_reset(self):
        self.ctx.temporal_reset()

    def temporal_clip(self, **params):
        self.ctx.temporal_clip(**params)

    def tonemap(self, **params):
        self.ctx.tonemap(**params)

    def read_display(self, flip: bool = False) -> np.ndarray:
        return self.ctx.read_display(flip)

    def error_estimate(self, **params):
        self.ctx.error_estimate(**params)

    def read_error_summary(self) -> dict:
        return self.ctx.read_error_summary()

    def render_until(self, threshold: float, max_frames: int, check_every: int = 16, **params):
        """Render until the picture is this clean: frames as render_frame() makes them, an error_estimate(threshold=threshold, **params)
        after every `check_every` of them (and after the last one), stopping at the first converged summary or after `max_frames`
        frames.  Returns (frames rendered by this call, the latest summary).  The frames are counted the reference's way: first_frames
        is 1 unless given."""
        if max_frames < 1 or check_every < 1:
            raise ValueError("render_until: max_frames and check_every must be >= 1")
        done, summary = 0, None
        while done < max_frames:
            for _ in range(min(check_every, max_frames - done)):
                self.render_frame(sync=False)
                done += 1
            self.ctx.error_estimate(threshold=threshold, **params)
            summary = self.ctx.read_error_summary()
            if summary["valid"] and summary["converged"]:
                break
        return done, summary

    def render_adaptive(self, threshold: float, max_samples: int, min_samples: int = 16, check_every: int = 16, floor=None):
        """Render until every tile is at or below `threshold` (a relative RMSE) or holds `max_samples` samples: a session of masked
        frames (adaptive_begin), with the uniforms render_frame() would use (frames and reset_flag are ignored; one rand() per frame, the
        frame count is not advanced and a pending reset_buffer() stays pending, as in renderer.h), an adaptive_update() after every
        `check_every` of them, until no tile is active.  Returns (frames rendered, the latest summary)."""
        if check_every < 1:
            raise ValueError("render_adaptive: check_every must be >= 1")
        self.ctx.adaptive_begin(threshold=threshold, floor=floor, min_samples=min_samples, max_samples=max_samples)
        done, summary = 0, self.ctx.adaptive_update()
        while not summary["converged"]:
            for _ in range(check_every):
                self.ctx.adaptive_frame(self.session_frame(), sync=False)
                done += 1
            summary = self.ctx.adaptive_update()
        return done, summary

    def render_robust(self, frames: int, buckets: int = 8, gain: float = 1.0, to_image: bool = False) -> np.ndarray:
        """`frames` one-sample frames (the uniforms render_frame() would use, with frames = 0 and reset_flag = 1; one rand() per frame, the
        frame count is not advanced and a pending reset_buffer() stays pending, as in renderer.h) folded into `buckets` bucket means
        (robust_begin, robust_accumulate), then the trimmed mean of the buckets (robust_resolve).  Returns the resolved picture: RGB and
        the Gini coefficient, or with to_image the accumulation image, which then holds it.  The session stays open."""
        if frames < 1:
            raise ValueError("render_robust: frames must be >= 1")
        self.ctx.robust_begin(buckets=buckets)
        for _ in range(frames):
            self.ctx.render(self.session_frame(reset_flag=1), sync=False)
            self.ctx.robust_accumulate()
        self.ctx.robust_resolve(gain=gain, dest=ROBUST_DEST_IMAGE if to_image else ROBUST_DEST_BUFFER)
        return self.ctx.read_image() if to_image else self.ctx.read_robust()

    def robust_error_estimate(self, **params):
        self.ctx.robust_error_estimate(**params)

    def read_robust_error_summary(self) -> dict:
        return self.ctx.read_robust_error_summary()

    def robust_denoise(self, **params):
        self.ctx.robust_denoise(**params)

    def render_robust_until(self, threshold: float, max_frames: int, check_every: int = 16, buckets: int = 8, gain: float = 1.0, to_image: bool = False, **params):
        """Render a robust session until its resolved picture is this clean: session frames as render_robust() makes them, a
        robust_error_estimate(threshold=threshold, gain=gain, **params) after every `check_every` of them once the session holds at
        least `buckets` frames (and after the last one), stopping at the first converged summary or after `max_frames` frames; then the
        resolve with the same gain.  Returns (frames rendered, the latest summary or None if no estimate was possible, the resolved
        picture as render_robust() returns it).  The session stays open."""
        if max_frames < 1 or check_every < 1:
            raise ValueError("render_robust_until: max_frames and check_every must be >= 1")
        self.ctx.robust_begin(buckets=buckets)
        done, summary = 0, None
        while done < max_frames:
            for _ in range(min(check_every, max_frames - done)):
                self.ctx.render(self.session_frame(reset_flag=1), sync=False)
                self.ctx.robust_accumulate()
                done += 1
            if done >= buckets:
                self.ctx.robust_error_estimate(threshold=threshold, gain=gain, **params)
                summary = self.ctx.read_robust_error_summary()
                if summary["valid"] and summary["converged"]:
                    break
        self.ctx.robust_resolve(gain=gain, dest=ROBUST_DEST_IMAGE if to_image else ROBUST_DEST_BUFFER)
        return done, summary, (self.ctx.read_image() if to_image else self.ctx.read_robust())

    def render_robust_adaptive(self, threshold: float, max_samples: int, min_samples=None, check_every: int = 16, buckets: int = 8,
                               gain: float = 1.0, to_image: bool = False, floor=None):
        """Render until the picture robust_adaptive_resolve(gain=gain) makes is at or below `threshold` (a relative RMSE) in every tile, or
        the tile holds `max_samples` samples: a robust adaptive session (robust_adaptive_begin) of masked frames with the uniforms of
        session_frame(), a robust_adaptive_update() after every `check_every` of them, until no tile is active; then the resolve.  Returns
        (frames rendered, the latest summary, the resolved picture as render_robust() returns it).  The session stays open."""
        if check_every < 1:
            raise ValueError("render_robust_adaptive: check_every must be >= 1")
        self.ctx.robust_adaptive_begin(buckets=buckets, threshold=threshold, floor=floor, gain=gain, min_samples=min_samples, max_samples=max_samples)
        done, summary = 0, self.ctx.robust_adaptive_update()
        while not summary["converged"]:
            for _ in range(check_every):
                self.ctx.robust_adaptive_frame(self.session_frame(), sync=False)
                done += 1
            summary = self.ctx.robust_adaptive_update()
        self.ctx.robust_adaptive_resolve(gain=gain, dest=ROBUST_DEST_IMAGE if to_image else ROBUST_DEST_BUFFER)
        return done, summary, (self.ctx.read_image() if to_image else self.ctx.read_robust_adaptive())

    def read_temporal(self) -> np.ndarray:
        return self.ctx.read_temporal()

    def device_temporal_ptr(self) -> int:
        return self.ctx.device_temporal_ptr()

    def read_temporal_moments(self) -> np.ndarray:
        return self.ctx.read_temporal_moments()

    def device_temporal_moments_ptr(self) -> int:
        return self.ctx.device_temporal_moments_ptr()

    def set_scene(self, scene: Scene):
        self.ctx.upload_scene(scene)

    def render_frame(self, sync: bool = True) -> FrameParams:
        p = self.next_frame()
        self.ctx.render(p, sync=sync)
        return p

    def render_guides(self, passes: int = 1) -> list:
        """`passes` guide passes (Context.guides_frame) with the uniforms of session_frame(): one rand() per pass, like every frame, the
        frame count is not advanced and a pending reset_buffer() stays pending, as in renderer.h.  Returns the parameters of the passes,
        in order.  The planes then hold the mean of these passes and of whatever they held since their last restart."""
        if passes < 1:
            raise ValueError("render_guides: passes must be >= 1")
        used = []
        for _ in range(passes):
            used.append(self.session_frame())
            self.ctx.guides_frame(used[-1], sync=False)
        self.ctx.synchronize()
        return used

    def run(self, frames: int):
        for _ in range(frames):
            self.render_frame(sync=False)
        self.ctx.synchronize()
