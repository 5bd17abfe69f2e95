"""2019global_amd — MI355X-native (gfx950) per-pixel radiance path for preon7/2019global.

Host-side mirror of the reference's render API over the C-ABI in ``include/gi.h`` (``libgi.so``):

  reference (C++ header-only)                         here
  ---------------------------------------------------  ------------------------------------------
  Camera(pos, lookAt, focal)        camera.h:8-10      Camera(pos, look_at, focal)
  Octree(min, max) / push_back(e)   octree.h:14,20   Octree(min, max) / push_back(e)
  ImpSphere / ImpTriangle / ExpQuad entities.h:45,138,581  same names and constructor arguments
  Material(color[, shader]), .specular_power           Material(color, shader, specular_power)
  RayTracer(camera, light)          raytracer.h:18     RayTracer(camera, light)
    .setScene(octree) / .run(w, h) / .start() / .stop() / .running() / .getImage()

``RayTracer.run`` renders on the GPU through ``gi_render`` and returns when the frame is done (or
``stop()`` was called from another thread); ``getImage()`` returns the RGB888 frame the reference's
``Image`` would hold.  There is no CPU fallback: without ``libgi.so`` or a gfx950 device every
render raises ``GIError``.

Lower-level handles for benchmarks and multi-GPU: ``DeviceScene`` (a scene resident in HBM) with
``render_device`` into caller-owned device buffers on a HIP stream; ``MultiScene`` (several GPUs of
one process, RCCL gather; ``RayTracer`` uses it when ``GI_DEVICES`` lists more than one device);
``Octree.intersect`` (the reference's public candidate query, on the host).  ``DeviceScene.intersect`` /
``occluded`` answer batches of rays; ``DeviceScene.render_aov`` returns a frame's first-hit feature
buffers (distance, normal, albedo, primitive, entity, texture coordinate) and ``camera_rays`` its pixel
rays as ray records, each with a ``_device`` form on a HIP stream.  ``denoise`` filters a noisy frame over
those buffers (an edge-avoiding a-trous filter: a preview of the first progressive passes), with
``denoise_device`` on a HIP stream into caller-owned buffers.  ``DeviceScene.frame_moments`` returns the
per-pixel sample mean, variance of the mean and per-sample radiance of the scene's retained Mode X frame, and
``denoise_var`` is the filter with its colour stop per pixel from that variance (``_device`` forms alike).
``temporal`` / ``temporal_device`` reproject the previous frame's accumulated colour and variance onto a frame's
first hits and blend them with it: the samples a moving camera would otherwise throw away.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Optional, Sequence

import numpy as np

from . import scenes as _scenes

__all__ = [
    "GIError", "lib", "Camera", "Material", "Octree", "ImpSphere", "ImpTriangle", "ExpQuad",
    "ExpSphere", "ExpCube", "ExpCone", "ExpRectangle", "ExpBox",
    "RayTracer", "DeviceScene", "MODE_R", "MODE_X", "STAT_RAYS", "STAT_NODES", "STAT_PRIMS",
    "STAT_PIXELS", "TILE", "MultiScene", "devices_from_env", "obj_entities", "RAY_DOUBLES",
    "AOV_OUTPUTS", "camera_rays", "camera_rays_device",
    "PathId", "RadianceParams", "SampleParams", "PATH_ID_DTYPE", "SAMPLE_JITTER",
    "sample_rays", "sample_rays_device", "resolve_samples", "resolve_samples_device",
    "DenoiseParams", "DENOISE_ALBEDO_STOP", "denoise", "denoise_scratch_bytes", "denoise_device",
    "MOMENTS_OUTPUTS", "DenoiseVarParams", "DENOISE_VAR_OUTPUTS", "DENOISE_VAR_SIGMA_V", "DENOISE_VAR_FLOOR",
    "denoise_var", "denoise_var_scratch_bytes", "denoise_var_device",
    "TemporalParams", "TemporalFrame", "TemporalOut", "TEMPORAL_PRIM_STOP", "TEMPORAL_OUTPUTS", "TEMPORAL_PLANES",
    "temporal", "temporal_device",
    "AdaptiveParams", "AdaptiveOut", "ADAPTIVE_RELATIVE", "ADAPTIVE_OUTPUTS",
]

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GI_LIB") or os.path.join(HERE, "libgi.so")   # GI_LIB: A/B builds

MODE_R, MODE_X = 0, 1
FLAG_STATS = 1
FLAG_R_DFS = 2   # Mode R: reverse-DFS over the whole reference octree (A/B against the default)
FLAG_TIME = 4    # HIP events around the dominant kernel; read with DeviceScene.kernel_ms()
FLAG_X_NO_SHADOW = 8   # Mode X, tests only: no shadow rays (reduces depth-1 Mode X to the reference's shading)
FLAG_X_WF = 16   # Mode X: the wavefront form (one launch per bounce over compacted path queues, gi_wf.hip)
FLAG_X_MEGA = 32   # Mode X: the persistent path-state kernel k_mode_x
FLAG_X_SEG = 64   # Mode X: the segment-synchronous persistent form k_seg (no form flag: chosen per launch)
FLAG_X_ALL_LEAVES = 128   # Mode X, tests only: shadow queries visit every leaf of the flat table (DeviceScene.shadow_leaves)
KAT_X_TREE, KAT_X_HBM = 1, 2   # gi_kat_x_query's flags
X_FORMS = ("k_mode_x", "k_wf_bounce", "k_seg")   # gi_scene_x_form's values
R_KERNELS = ("k_mode_r", "k_rf_walk", "k_mode_r_batch")   # gi_scene_r_kernel's (1: the flat phases)
STAT_RAYS, STAT_NODES, STAT_PRIMS, STAT_PIXELS, STAT_X_PATH_MAX = 0, 1, 2, 3, 4
STAT_X_ITERS, STAT_X_TRAV, STAT_X_HANDLE, STAT_X_HLANES, STAT_X_HCLOSE, STAT_X_HSHADOW = 5, 6, 7, 8, 9, 10
STAT_X_CYC_TRAV, STAT_X_CYC_HIT, STAT_X_CYC_NEXT, STAT_X_CYC_ALL = 11, 12, 13, 14
STAT_X_RESOLVED = 15
STAT_X_IT_NODE, STAT_X_LN_NODE, STAT_X_IT_LEAF, STAT_X_LN_LEAF = 16, 17, 18, 19
STAT_X_IT_RS, STAT_X_LN_RS, STAT_X_IT_ST, STAT_X_LN_ST = 20, 21, 22, 23
STAT_R_PAIRS, STAT_R_OVF_TILES = 24, 25
STATS_N = 26
TILE = 8
ABI_VERSION = 21
RAY_DOUBLES = 8   # a ray record of the batched queries: o[3], d[3], tmax, reserved (gi.h GI_RAY_DOUBLES)
# the feature buffers of DeviceScene.render_aov (gi.h gi_aov, in its field order): name -> (dtype, trailing shape)
AOV_OUTPUTS = ("t", "normal", "albedo", "prim", "entity", "uv")
_AOV_KINDS = {"t": (np.float64, ()), "normal": (np.float64, (3,)), "albedo": (np.float64, (3,)),
              "prim": (np.int32, ()), "entity": (np.int32, ()), "uv": (np.int32, (2,))}


class GIError(RuntimeError):
    pass


# ---- C structures (include/gi.h) -------------------------------------------------------------
class EntityDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("has_material", ctypes.c_int32), ("args", ctypes.c_double * 11),
                ("mat_color", ctypes.c_double * 3), ("mat_shader", ctypes.c_double * 3),
                ("mat_specular_power", ctypes.c_double), ("mat_reflectivity", ctypes.c_double)]


class SceneDesc(ctypes.Structure):
    _fields_ = [("octree_min", ctypes.c_double * 3), ("octree_max", ctypes.c_double * 3),
                ("n_entities", ctypes.c_int32), ("entities", ctypes.POINTER(EntityDesc))]


class CameraDesc(ctypes.Structure):
    _fields_ = [("pos", ctypes.c_double * 3), ("up", ctypes.c_double * 3), ("forward", ctypes.c_double * 3),
                ("focal", ctypes.c_double)]


class Opts(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("spp", ctypes.c_int32), ("depth", ctypes.c_int32),
                ("shard_count", ctypes.c_int32), ("shard_index", ctypes.c_int32), ("band_rows", ctypes.c_int32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32), ("seed", ctypes.c_uint64),
                ("stats", ctypes.c_void_p), ("sample_begin", ctypes.c_int32), ("sample_end", ctypes.c_int32)]


class SceneInfo(ctypes.Structure):
    _fields_ = [("n_entities", ctypes.c_int32), ("n_nodes", ctypes.c_int32), ("n_leaves", ctypes.c_int32),
                ("max_depth", ctypes.c_int32), ("n_reachable", ctypes.c_int32), ("n_dropped", ctypes.c_int32),
                ("x_nodes", ctypes.c_int32), ("x_prims", ctypes.c_int32), ("device_bytes", ctypes.c_int64),
                ("x_node_bytes", ctypes.c_int32), ("x_lds_resident", ctypes.c_int32),
                ("x_flat_leaves", ctypes.c_int32), ("x_fan_leaves", ctypes.c_int32)]


class Hit(ctypes.Structure):
    _fields_ = [("entity", ctypes.c_int32), ("u", ctypes.c_int32), ("v", ctypes.c_int32),
                ("point", ctypes.c_double * 3), ("normal", ctypes.c_double * 3)]


class AovFrame(ctypes.Structure):
    _fields_ = [("w", ctypes.c_int32), ("h", ctypes.c_int32), ("x0", ctypes.c_int32), ("y0", ctypes.c_int32),
                ("x1", ctypes.c_int32), ("y1", ctypes.c_int32)]


class Aov(ctypes.Structure):
    _fields_ = [("t", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("albedo", ctypes.c_void_p),
                ("prim", ctypes.c_void_p), ("entity", ctypes.c_void_p), ("uv", ctypes.c_void_p)]


DENOISE_ALBEDO_STOP = 1   # gi.h GI_DENOISE_ALBEDO_STOP
DENOISE_OUTPUTS = ("rgb", "rgb8")


class DenoiseParams(ctypes.Structure):
    _fields_ = [("levels", ctypes.c_int32), ("normal_pow_log2", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_int32), ("sigma_c", ctypes.c_double), ("sigma_p", ctypes.c_double)]


class DenoiseIO(ctypes.Structure):
    _fields_ = [("rgb", ctypes.c_void_p), ("t", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("albedo", ctypes.c_void_p),
                ("out_rgb", ctypes.c_void_p), ("out_rgb8", ctypes.c_void_p)]


MOMENTS_OUTPUTS = ("mean", "var", "samples")   # gi.h gi_moments, in its field order


class Moments(ctypes.Structure):
    _fields_ = [("mean", ctypes.c_void_p), ("var", ctypes.c_void_p), ("samples", ctypes.c_void_p)]


DENOISE_VAR_OUTPUTS = ("rgb", "var", "rgb8")
# denoise_var's defaults, chosen by a sweep over the first passes of the Cornell box (DESIGN.md §9 "Denoiser")
DENOISE_VAR_SIGMA_V = 1.0
DENOISE_VAR_FLOOR = 1e-6


class DenoiseVarParams(ctypes.Structure):
    _fields_ = [("levels", ctypes.c_int32), ("normal_pow_log2", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_int32), ("sigma_v", ctypes.c_double), ("sigma_p", ctypes.c_double),
                ("var_floor", ctypes.c_double)]


class DenoiseVarIO(ctypes.Structure):
    _fields_ = [("rgb", ctypes.c_void_p), ("var", ctypes.c_void_p), ("t", ctypes.c_void_p), ("normal", ctypes.c_void_p),
                ("albedo", ctypes.c_void_p), ("out_rgb", ctypes.c_void_p), ("out_var", ctypes.c_void_p),
                ("out_rgb8", ctypes.c_void_p)]


TEMPORAL_PRIM_STOP = 1   # gi.h GI_TEMPORAL_PRIM_STOP
TEMPORAL_OUTPUTS = ("rgb", "var", "len")   # gi.h gi_temporal_out, in its field order
TEMPORAL_PLANES = ("rgb", "var", "t", "normal", "prim", "len")   # gi.h gi_temporal_frame, in its field order


class TemporalParams(ctypes.Structure):
    _fields_ = [("max_history", ctypes.c_int32), ("flags", ctypes.c_uint32), ("alpha_min", ctypes.c_double),
                ("cos_min", ctypes.c_double), ("sigma_p", ctypes.c_double)]


class TemporalFrame(ctypes.Structure):
    _fields_ = [("rgb", ctypes.c_void_p), ("var", ctypes.c_void_p), ("t", ctypes.c_void_p), ("normal", ctypes.c_void_p),
                ("prim", ctypes.c_void_p), ("len", ctypes.c_void_p)]


class TemporalOut(ctypes.Structure):
    _fields_ = [("rgb", ctypes.c_void_p), ("var", ctypes.c_void_p), ("len", ctypes.c_void_p)]


ADAPTIVE_RELATIVE = 1   # gi.h GI_ADAPTIVE_RELATIVE
ADAPTIVE_OUTPUTS = ("rgb", "rgb8", "mean", "var", "n")   # gi.h gi_adaptive_out, in its field order
_ADAPTIVE_KINDS = {"rgb": (np.float64, (3,)), "rgb8": (np.uint8, (3,)), "mean": (np.float64, (3,)),
                   "var": (np.float64, (3,)), "n": (np.int32, ())}


class AdaptiveParams(ctypes.Structure):
    _fields_ = [("min_samples", ctypes.c_int32), ("flags", ctypes.c_uint32), ("tol", ctypes.c_double),
                ("y_floor", ctypes.c_double)]


class AdaptiveOut(ctypes.Structure):
    _fields_ = [("rgb", ctypes.c_void_p), ("rgb8", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("var", ctypes.c_void_p),
                ("n", ctypes.c_void_p)]


SAMPLE_JITTER = 1   # gi.h GI_SAMPLE_JITTER
# a gi_path_id record as a numpy dtype: the stream (a render's pixel index y w + x) and the sample of a path
PATH_ID_DTYPE = np.dtype([("stream", "<u8"), ("sample", "<u4"), ("reserved", "<u4")])


class PathId(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_uint64), ("sample", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class RadianceParams(ctypes.Structure):
    _fields_ = [("depth", ctypes.c_int32), ("flags", ctypes.c_uint32), ("seed", ctypes.c_uint64)]


class SampleParams(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("sample_begin", ctypes.c_int32), ("sample_end", ctypes.c_int32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32), ("aperture", ctypes.c_double),
                ("focus", ctypes.c_double)]


TILE_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8),
                           ctypes.POINTER(ctypes.c_double))

EXPORTS = ["gi_abi_version", "gi_last_error", "gi_camera_init", "gi_scene_create", "gi_scene_destroy",
           "gi_scene_get_info", "gi_render", "gi_render_device", "gi_shard_tiles", "gi_unshard_device",
           "gi_trace_ray", "gi_kat_expbox", "gi_kat_r_prims", "gi_kat_r_entities", "gi_kat_x_query", "gi_kat_x_variant", "gi_kat_x_texel", "gi_scene_kernel_ms", "gi_scene_x_form", "gi_scene_seg_ring", "gi_scene_shadow_leaves", "gi_scene_r_kernel", "gi_octree_create", "gi_octree_destroy",
           "gi_octree_intersect", "gi_multi_create", "gi_multi_destroy", "gi_multi_info", "gi_multi_render", "gi_device_count",
           "gi_device_list", "gi_build_id", "gi_obj_parse", "gi_intersect", "gi_occluded", "gi_intersect_device",
           "gi_occluded_device", "gi_render_aov", "gi_render_aov_device", "gi_camera_rays", "gi_camera_rays_device",
           "gi_denoise_scratch_bytes", "gi_denoise_device", "gi_denoise",
           "gi_frame_samples_info", "gi_frame_moments_device", "gi_frame_moments",
           "gi_denoise_var_scratch_bytes", "gi_denoise_var_device", "gi_denoise_var",
           "gi_temporal_device", "gi_temporal",
           "gi_render_adaptive_device", "gi_render_adaptive", "gi_adaptive_info",
           "gi_radiance_device", "gi_radiance", "gi_sample_rays_device", "gi_sample_rays",
           "gi_resolve_samples_device", "gi_resolve_samples"]

_lib = None
_lock = threading.Lock()


def lib():
    """Load libgi.so (built in-tree by ``2019global_amd/build.py``).  torch, when importable, is
    imported first so that libgi binds to the same HIP runtime instance torch uses."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise GIError(f"{LIB_PATH} is missing: run `python 2019global_amd/build.py` (no CPU fallback)")
        try:
            import torch  # noqa: F401  (one HIP runtime per process)
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        vp, i32, dp = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
        L.gi_abi_version.restype = i32
        L.gi_last_error.restype = ctypes.c_char_p
        L.gi_camera_init.argtypes = [dp, dp, ctypes.c_double, ctypes.POINTER(CameraDesc)]
        L.gi_scene_create.argtypes = [ctypes.POINTER(SceneDesc), ctypes.POINTER(vp)]
        L.gi_scene_destroy.argtypes = [vp]
        L.gi_scene_destroy.restype = None
        L.gi_scene_get_info.argtypes = [vp, ctypes.POINTER(SceneInfo)]
        L.gi_render.argtypes = [vp, ctypes.POINTER(CameraDesc), dp, i32, i32, ctypes.POINTER(Opts), dp,
                                ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int), TILE_CB, vp]
        L.gi_render_device.argtypes = [vp, ctypes.POINTER(CameraDesc), dp, i32, i32, ctypes.POINTER(Opts), vp, vp, vp]
        L.gi_shard_tiles.argtypes = [i32, i32, i32]
        L.gi_shard_tiles.restype = ctypes.c_int64
        L.gi_unshard_device.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
        L.gi_trace_ray.argtypes = [vp, dp, dp, dp, ctypes.POINTER(Hit), dp]
        L.gi_kat_expbox.argtypes = [i32, dp, ctypes.POINTER(ctypes.c_int32)]
        ip = ctypes.POINTER(ctypes.c_int32)
        L.gi_kat_r_prims.argtypes = [i32, i32, dp, ip, dp]
        L.gi_kat_r_entities.argtypes = [vp, i32, dp, ip, dp]
        L.gi_kat_x_query.argtypes = [vp, i32, dp, dp, i32, ip, dp, ip, ip, ip, dp, ip, dp]
        L.gi_kat_x_variant.argtypes = [vp, i32, ip]
        L.gi_kat_x_texel.argtypes = [vp, i32, dp, i32, dp, ip]
        i64 = ctypes.c_int64
        L.gi_intersect.argtypes = [vp, i64, dp, dp, ip, ip, dp]
        L.gi_occluded.argtypes = [vp, i64, dp, ip]
        L.gi_intersect_device.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp]
        L.gi_occluded_device.argtypes = [vp, i64, vp, vp, vp]
        L.gi_render_aov.argtypes = [vp, ctypes.POINTER(CameraDesc), ctypes.POINTER(AovFrame), ctypes.POINTER(Aov)]
        L.gi_render_aov_device.argtypes = [vp, ctypes.POINTER(CameraDesc), ctypes.POINTER(AovFrame), ctypes.POINTER(Aov), vp]
        L.gi_camera_rays.argtypes = [ctypes.POINTER(CameraDesc), ctypes.POINTER(AovFrame), dp]
        L.gi_camera_rays_device.argtypes = [ctypes.POINTER(CameraDesc), ctypes.POINTER(AovFrame), vp, vp]
        L.gi_denoise_scratch_bytes.argtypes = [ctypes.POINTER(AovFrame), ctypes.POINTER(DenoiseParams)]
        L.gi_denoise_scratch_bytes.restype = ctypes.c_int64
        L.gi_denoise_device.argtypes = [ctypes.POINTER(CameraDesc), ctypes.POINTER(AovFrame), ctypes.POINTER(DenoiseParams),
                                        ctypes.POINTER(DenoiseIO), vp, ctypes.c_int64, vp]
        L.gi_denoise.argtypes = [ctypes.POINTER(CameraDesc), ctypes.POINTER(AovFrame), ctypes.POINTER(DenoiseParams),
                                 ctypes.POINTER(DenoiseIO)]
        L.gi_frame_samples_info.argtypes = [vp, ip, ip, ip, ip]
        L.gi_frame_moments_device.argtypes = [vp, ctypes.POINTER(AovFrame), ctypes.POINTER(Moments), vp]
        L.gi_frame_moments.argtypes = [vp, ctypes.POINTER(AovFrame), ctypes.POINTER(Moments)]
        L.gi_denoise_var_scratch_bytes.argtypes = [ctypes.POINTER(AovFrame), ctypes.POINTER(DenoiseVarParams)]
        L.gi_denoise_var_scratch_bytes.restype = ctypes.c_int64
        L.gi_denoise_var_device.argtypes = [ctypes.POINTER(CameraDesc), ctypes.POINTER(AovFrame), ctypes.POINTER(DenoiseVarParams),
                                            ctypes.POINTER(DenoiseVarIO), vp, ctypes.c_int64, vp]
        L.gi_denoise_var.argtypes = [ctypes.POINTER(CameraDesc), ctypes.POINTER(AovFrame), ctypes.POINTER(DenoiseVarParams),
                                     ctypes.POINTER(DenoiseVarIO)]
        tp_args = [ctypes.POINTER(CameraDesc), ctypes.POINTER(CameraDesc), ctypes.POINTER(AovFrame), ctypes.POINTER(TemporalParams),
                   ctypes.POINTER(TemporalFrame), ctypes.POINTER(TemporalFrame), ctypes.POINTER(TemporalOut)]
        L.gi_temporal_device.argtypes = tp_args + [vp]
        L.gi_temporal.argtypes = tp_args
        ad_args = [vp, ctypes.POINTER(CameraDesc), dp, i32, i32, ctypes.POINTER(Opts), ctypes.POINTER(AdaptiveParams),
                   ctypes.POINTER(AdaptiveOut)]
        L.gi_render_adaptive_device.argtypes = ad_args + [vp]
        L.gi_render_adaptive.argtypes = ad_args
        L.gi_adaptive_info.argtypes = [vp, ip, ip, ip, ctypes.POINTER(ctypes.c_int64)]
        L.gi_radiance_device.argtypes = [vp, i64, vp, vp, dp, ctypes.POINTER(RadianceParams), vp, vp]
        L.gi_radiance.argtypes = [vp, i64, dp, vp, dp, ctypes.POINTER(RadianceParams), dp]
        L.gi_sample_rays_device.argtypes = [ctypes.POINTER(CameraDesc), ctypes.POINTER(AovFrame), ctypes.POINTER(SampleParams),
                                            vp, vp, vp]
        L.gi_sample_rays.argtypes = [ctypes.POINTER(CameraDesc), ctypes.POINTER(AovFrame), ctypes.POINTER(SampleParams), vp, vp]
        L.gi_resolve_samples_device.argtypes = [i64, ctypes.c_int32, vp, vp, vp, vp]
        L.gi_resolve_samples.argtypes = [i64, ctypes.c_int32, dp, vp, vp]
        L.gi_scene_kernel_ms.argtypes =[vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)]
        L.gi_scene_x_form.argtypes = [vp, ctypes.POINTER(Opts), ctypes.POINTER(ctypes.c_int32)]
        L.gi_scene_seg_ring.argtypes = [vp, ctypes.POINTER(Opts), ctypes.POINTER(ctypes.c_int32)]
        L.gi_scene_shadow_leaves.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        L.gi_scene_r_kernel.argtypes = [vp, ctypes.POINTER(Opts), ctypes.POINTER(ctypes.c_int32)]
        L.gi_octree_create.argtypes = [ctypes.POINTER(SceneDesc), ctypes.POINTER(vp)]
        L.gi_octree_destroy.argtypes = [vp]
        L.gi_octree_destroy.restype = None
        L.gi_octree_intersect.argtypes = [vp, dp, dp, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64,
                                          ctypes.POINTER(ctypes.c_int64)]
        L.gi_multi_create.argtypes = [ctypes.POINTER(SceneDesc), i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(vp)]
        L.gi_multi_destroy.argtypes = [vp]
        L.gi_multi_destroy.restype = None
        L.gi_multi_info.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                    ctypes.POINTER(ctypes.c_int)]
        L.gi_multi_render.argtypes = [vp, ctypes.POINTER(CameraDesc), dp, i32, i32, ctypes.POINTER(Opts), dp,
                                      ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int), TILE_CB, vp]
        L.gi_device_list.argtypes = [ctypes.POINTER(ctypes.c_int32), i32]
        L.gi_build_id.restype = ctypes.c_char_p
        L.gi_obj_parse.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.POINTER(EntityDesc),
                                   ctypes.POINTER(EntityDesc), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
        if L.gi_abi_version() != ABI_VERSION:
            raise GIError(f"libgi ABI {L.gi_abi_version()} != {ABI_VERSION}")
        _lib = L
        return L


def build_id() -> str:
    """Source hash the loaded libgi was compiled from (build.py source_hash)."""
    return lib().gi_build_id().decode()


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise GIError(f"{what} failed ({rc}): {lib().gi_last_error().decode()}")


def _check_rays(rays) -> int:
    """The ray count of a host ray array for DeviceScene.intersect / occluded; ValueError unless it is a
    C-contiguous float64 array of shape (n, RAY_DOUBLES).  Checked before the library is touched."""
    if not isinstance(rays, np.ndarray) or rays.dtype != np.float64 or rays.ndim != 2 or rays.shape[1] != RAY_DOUBLES or \
            not rays.flags.c_contiguous:
        raise ValueError(f"rays: a C-contiguous float64 array of shape (n, {RAY_DOUBLES}) -- o[3], d[3], tmax, reserved")
    return int(rays.shape[0])


def _check_ids(ids, n):
    """The path ids of a host radiance call: None, or a C-contiguous array of PATH_ID_DTYPE and shape (n,).
    ValueError otherwise.  Checked before the library is touched."""
    if ids is None:
        return None
    if not isinstance(ids, np.ndarray) or ids.dtype != PATH_ID_DTYPE or ids.shape != (n,) or not ids.flags.c_contiguous:
        raise ValueError("ids: None or a C-contiguous array of PATH_ID_DTYPE (stream, sample, reserved), one per ray")
    return ids


def _sample_params(seed, samples, jitter, aperture, focus) -> SampleParams:
    """The gi_sample_params of a call: samples = (begin, end) or a count (0, count).  ValueError for a sample
    range that is not two integers 0 <= begin <= end, and for an aperture or focus that is not a number."""
    def whole(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if whole(samples):
        samples = (0, samples)
    samples = tuple(samples) if isinstance(samples, (tuple, list)) else ()
    if len(samples) != 2 or not all(whole(v) for v in samples) or not 0 <= samples[0] <= samples[1] < 2 ** 31:
        raise ValueError("samples: a count, or (begin, end) with 0 <= begin <= end")
    return SampleParams(int(seed), int(samples[0]), int(samples[1]), SAMPLE_JITTER if jitter else 0, 0, float(aperture),
                        float(focus))


def _check_rows(rows):
    """(n_pix, ns) of host radiance rows for resolve_samples; ValueError unless rows is a C-contiguous float64
    array of shape (n_pix, ns, 3) with ns >= 1.  Checked before the library is touched."""
    if not isinstance(rows, np.ndarray) or rows.dtype != np.float64 or rows.ndim != 3 or rows.shape[2] != 3 or \
            rows.shape[1] < 1 or not rows.flags.c_contiguous:
        raise ValueError("rows: a C-contiguous float64 array of shape (n_pix, ns, 3), ns >= 1")
    return int(rows.shape[0]), int(rows.shape[1])


def _aov_frame(w, h, window) -> AovFrame:
    """The gi_aov_frame of a w x h frame and its window (x0, y0, x1, y1), None: the whole frame.  ValueError
    unless w, h > 0 and 0 <= x0 <= x1 <= w, 0 <= y0 <= y1 <= h (an empty window is allowed).  Checked
    before the library is touched."""
    def whole(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if not (whole(w) and whole(h)) or w <= 0 or h <= 0 or w >= 2 ** 31 or h >= 2 ** 31:
        raise ValueError("frame: w and h are positive integers")
    if window is None:
        window = (0, 0, w, h)
    window = tuple(window)
    if len(window) != 4 or not all(whole(v) for v in window):
        raise ValueError("window: four integers (x0, y0, x1, y1)")
    x0, y0, x1, y1 = (int(v) for v in window)
    if not (0 <= x0 <= x1 <= w and 0 <= y0 <= y1 <= h):
        raise ValueError(f"window {window}: reversed or not inside the {w} x {h} frame")
    return AovFrame(int(w), int(h), x0, y0, x1, y1)


def _d3(v) -> ctypes.Array:
    return (ctypes.c_double * 3)(*[float(x) for x in v])


# ---- reference-shaped API ---------------------------------------------------------------------
class Material:
    """Material(color[, shader]) (material.h:13-20); specular_power (material.h:29).
    reflectivity: Mode X only (no reference counterpart) -- probability that a bounce is a mirror
    reflection instead of a diffuse sample; 0 = the reference's diffuse-only material."""

    def __init__(self, color, shader=(0.1, 0.7, 1.0), specular_power: float = 5.0, reflectivity: float = 0.0):
        self.color = tuple(float(c) for c in color)
        self.shader_parameters = tuple(float(c) for c in shader)
        self.specular_power = float(specular_power)
        self.reflectivity = float(reflectivity)


class _Entity:
    kind = 0

    def __init__(self, args: Sequence[float], material: Optional[Material]):
        self._args = tuple(float(a) for a in args)
        self._material = material   # explicit override (entity->material = ...)

    @property
    def material(self) -> Optional[Material]:
        return self._material

    @material.setter
    def material(self, m: Material) -> None:
        self._material = m

    def _desc(self, d: EntityDesc) -> None:
        d.kind = self.kind
        for i, a in enumerate(self._args):
            d.args[i] = a
        m = self._material
        d.has_material = 1 if m is not None else 0
        if m is not None:
            for i in range(3):
                d.mat_color[i] = m.color[i]
                d.mat_shader[i] = m.shader_parameters[i]
            d.mat_specular_power = m.specular_power
            d.mat_reflectivity = m.reflectivity


class ImpSphere(_Entity):
    """ImpSphere(pos, float radius, color) (entities.h:45)."""
    kind = _scenes.IMP_SPHERE

    def __init__(self, pos, radius, color):
        super().__init__((*pos, radius, *color), None)


class ImpTriangle(_Entity):
    """ImpTriangle(p1, p2, p3) (entities.h:138); default material red (entities.h:21)."""
    kind = _scenes.IMP_TRIANGLE

    def __init__(self, p1, p2, p3):
        super().__init__((*p1, *p2, *p3), None)


class ExpQuad(_Entity):
    """ExpQuad(pos, float width, float length, float alpha, color) (entities.h:581)."""
    kind = _scenes.EXP_QUAD

    def __init__(self, pos, width, length, alpha, color):
        super().__init__((*pos, width, length, alpha, *color), None)


class ExpSphere(_Entity):
    """ExpSphere(pos, float radius, color) (entities.h:461): 10x10 stack/sector triangle mesh."""
    kind = _scenes.EXP_SPHERE

    def __init__(self, pos, radius, color):
        super().__init__((*pos, radius, *color), None)


class ExpCube(_Entity):
    """ExpCube(pos, float width, float length, float height, color) (entities.h:652)."""
    kind = _scenes.EXP_CUBE

    def __init__(self, pos, width, length, height, color):
        super().__init__((*pos, width, length, height, *color), None)


class ExpCone(_Entity):
    """ExpCone(pos, dir, float height, float radius, color) (entities.h:823).  As in the reference,
    dir is kept but the mesh always points along (-1, 0, -10) (:825)."""
    kind = _scenes.EXP_CONE

    def __init__(self, pos, dir, height, radius, color):
        super().__init__((*pos, *dir, height, radius, *color), None)


class ExpRectangle(_Entity):
    """ExpRectangle(p1, p2, p3) (entities.h:310); requires (p1-p3).(p2-p3) == 0 (:312)."""
    kind = _scenes.EXP_RECTANGLE

    def __init__(self, p1, p2, p3):
        super().__init__((*p1, *p2, *p3), None)


class ExpBox(_Entity):
    """ExpBox(min, max) (entities.h:381); getTextureCoord is (0, 0)."""
    kind = _scenes.EXP_BOX

    def __init__(self, mn, mx):
        super().__init__((*mn, *mx), None)


def obj_entities(text, material: Optional[Material] = None) -> list:
    """A Wavefront OBJ mesh (text or bytes) as ImpTriangle entities (entities.h:138), one per
    triangle of each face's fan in file order, through libgi's gi_obj_parse (no device needed);
    push them onto an Octree like hand-built entities.  `material` is set on every triangle (None:
    the reference's default ImpTriangle material)."""
    L = lib()
    data = text.encode() if isinstance(text, str) else bytes(text)
    tmpl = None
    if material is not None:
        tmpl = EntityDesc()
        t = _Entity((), material)
        t._desc(tmpl)
    n = ctypes.c_int64()
    _check(L.gi_obj_parse(data, len(data), tmpl, None, 0, ctypes.byref(n)), "gi_obj_parse")
    arr = (EntityDesc * max(1, n.value))()
    _check(L.gi_obj_parse(data, len(data), tmpl, arr, n.value, ctypes.byref(n)), "gi_obj_parse")
    out = []
    for i in range(n.value):
        d = arr[i]
        e = ImpTriangle(tuple(d.args[0:3]), tuple(d.args[3:6]), tuple(d.args[6:9]))
        if material is not None:
            e.material = Material(material.color, material.shader_parameters, material.specular_power,
                                  material.reflectivity)
        out.append(e)
    return out


class Octree:
    """Octree(min, max) + push_back (octree.h:14-43).  The tree itself is built by libgi from the
    push order (gi_scene_create), exactly as the reference builds it."""

    def __init__(self, min=(-20, -20, -20), max=(20, 20, 20)):
        self.min = tuple(float(v) for v in min)
        self.max = tuple(float(v) for v in max)
        self.entities = []
        self.generation = 0       # bumped by push_back: a RayTracer re-uploads a changed scene
        self._host = None         # gi_octree for intersect(), rebuilt when the generation changes
        self._host_gen = -1

    def push_back(self, e: _Entity) -> None:
        self.entities.append(e)
        self.generation += 1

    def intersect(self, origin, direction) -> list:
        """Octree::intersect(Ray(origin, dir)) (octree.h:46-68 -> Node::intersect :132-155): the
        candidate list -- entities in DFS order over children 0..7, duplicates kept -- from libgi's
        host copy of the reference octree (gi_octree_intersect; no device needed).  `direction` is
        normalised first, as the reference's Ray constructor does (ray.h:6)."""
        L = lib()
        if self._host is None or self._host_gen != self.generation:
            self._close_host()
            d, keep = self._scene_desc()
            h = ctypes.c_void_p()
            _check(L.gi_octree_create(ctypes.byref(d), ctypes.byref(h)), "gi_octree_create")
            del keep
            self._host, self._host_gen = h, self.generation
        dv = np.asarray(direction, np.float64)
        dv = dv * (1.0 / np.sqrt((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]))   # glm::normalize
        n = ctypes.c_int64()
        _check(L.gi_octree_intersect(self._host, _d3(origin), _d3(dv), None, 0, ctypes.byref(n)), "gi_octree_intersect")
        out = (ctypes.c_int32 * max(1, n.value))()
        _check(L.gi_octree_intersect(self._host, _d3(origin), _d3(dv), out, n.value, ctypes.byref(n)),
               "gi_octree_intersect")
        return [self.entities[i] for i in out[:n.value]]

    def _close_host(self):
        if self._host is not None and self._host.value:
            lib().gi_octree_destroy(self._host)
        self._host = None

    def __del__(self):
        try:
            self._close_host()
        except Exception:
            pass

    @classmethod
    def from_scene(cls, s: "_scenes.Scene") -> "Octree":
        o = cls(s.octree_min, s.octree_max)
        for e in s.entities:
            ent = _Entity(e.args, None if e.material is None else
                          Material(e.material.color, e.material.shader, e.material.specular_power,
                                   e.material.reflectivity))
            ent.kind = e.kind
            o.push_back(ent)
        return o

    def _scene_desc(self):
        n = len(self.entities)
        arr = (EntityDesc * max(n, 1))()
        for i, e in enumerate(self.entities):
            e._desc(arr[i])
        d = SceneDesc()
        d.octree_min = _d3(self.min)
        d.octree_max = _d3(self.max)
        d.n_entities = n
        d.entities = ctypes.cast(arr, ctypes.POINTER(EntityDesc))
        return d, arr


class Camera:
    """Camera(pos, lookAt, focal) (camera.h:8-10): up = (0,0,1), forward = normalize(lookAt - pos)."""

    def __init__(self, pos, lookAt=(0.0, 0.0, 0.0), focal: float = 0.04):
        self._c = CameraDesc()
        _check(lib().gi_camera_init(_d3(pos), _d3(lookAt), float(focal), ctypes.byref(self._c)), "gi_camera_init")

    @property
    def pos(self):
        return tuple(self._c.pos)

    @property
    def up(self):
        return tuple(self._c.up)

    @property
    def forward(self):
        return tuple(self._c.forward)

    @property
    def focalDist(self):
        return self._c.focal


class DeviceScene:
    """A scene resident in HBM on the current HIP device (gi_scene_create)."""

    def __init__(self, octree: Octree):
        L = lib()
        d, keep = octree._scene_desc()
        h = ctypes.c_void_p()
        _check(L.gi_scene_create(ctypes.byref(d), ctypes.byref(h)), "gi_scene_create")
        self._h = h
        del keep

    @classmethod
    def from_scene(cls, s: "_scenes.Scene") -> "DeviceScene":
        return cls(Octree.from_scene(s))

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            lib().gi_scene_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        i = SceneInfo()
        _check(lib().gi_scene_get_info(self._h, ctypes.byref(i)), "gi_scene_get_info")
        return {f: getattr(i, f) for f, _ in SceneInfo._fields_}

    @staticmethod
    def opts(mode=MODE_R, spp=1, depth=1, seed=0, shard_count=1, shard_index=0, band_rows=0, stats_ptr=0,
             flags=0, samples=None) -> Opts:
        """samples=(begin, end): a progressive pass of Mode X samples [begin, end) (gi.h gi_opts)."""
        o = Opts()
        o.mode, o.spp, o.depth, o.seed = mode, spp, depth, seed
        o.shard_count, o.shard_index, o.band_rows = shard_count, shard_index, band_rows
        o.flags = (FLAG_STATS if stats_ptr else 0) | flags
        o.stats = stats_ptr or None
        if samples is not None:
            o.sample_begin, o.sample_end = samples
        return o

    def render(self, cam: Camera, light, w: int, h: int, mode=MODE_R, spp=1, depth=1, seed=0, band_rows=0,
               cancel: Optional[ctypes.c_int] = None, callback=None, out=None, flags=0, samples=None):
        """Host-buffer render (gi_render).  Returns (rgb float64 [h,w,3], rgb8 uint8 [h,w,3]).
        out=(rgb, rgb8): caller-owned C-contiguous arrays to fill instead (either may be None:
        that output is not copied back).  samples=(begin, end): one progressive Mode X pass."""
        if out is None:
            rgb, rgb8 = np.zeros((h, w, 3), np.float64), np.zeros((h, w, 3), np.uint8)
        else:
            rgb, rgb8 = out
        for a, dt in ((rgb, np.float64), (rgb8, np.uint8)):
            if a is not None and (a.dtype != dt or a.size != w * h * 3 or not a.flags.c_contiguous):
                raise ValueError("render: out arrays must be C-contiguous [h, w, 3] float64 / uint8")
        cb = TILE_CB(callback) if callback is not None else TILE_CB()
        o = self.opts(mode, spp, depth, seed, band_rows=band_rows, flags=flags, samples=samples)
        _check(lib().gi_render(self._h, ctypes.byref(cam._c), _d3(light), w, h, ctypes.byref(o),
                               rgb.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if rgb is not None else None,
                               rgb8.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if rgb8 is not None else None,
                               ctypes.byref(cancel) if cancel is not None else None, cb, None), "gi_render")
        return rgb, rgb8

    def render_device(self, cam: Camera, light, w: int, h: int, d_rgb: int, d_rgb8: int = 0, stream: int = 0,
                      mode=MODE_R, spp=1, depth=1, seed=0, shard_count=1, shard_index=0, stats_ptr=0,
                      flags=0, samples=None) -> None:
        """Asynchronous render into device buffers (gi_render_device); pointers are ints."""
        o = self.opts(mode, spp, depth, seed, shard_count, shard_index, stats_ptr=stats_ptr, flags=flags,
                      samples=samples)
        _check(lib().gi_render_device(self._h, ctypes.byref(cam._c), _d3(light), w, h, ctypes.byref(o),
                                      d_rgb or None, d_rgb8 or None, stream or None), "gi_render_device")

    def x_form(self, mode=MODE_X, spp=1, depth=1, flags=0) -> str:
        """The Mode X form a render with these options would run: "k_mode_x" (persistent path-state
        kernel), "k_wf_bounce" (wavefront, one launch per bounce) or "k_seg" (segment-synchronous) --
        gi_scene_x_form."""
        o = self.opts(mode, spp, depth, 0, flags=flags)
        f = ctypes.c_int32()
        _check(lib().gi_scene_x_form(self._h, ctypes.byref(o), ctypes.byref(f)), "gi_scene_x_form")
        return X_FORMS[f.value]

    def seg_ring(self, mode=MODE_X, spp=1, depth=1, flags=0) -> bool:
        """Whether a render with these options would run k_seg with its per-wave ring of prepared
        primary rays (chosen per scene by LDS room; GI_SEG_RING=0 forces it off) -- gi_scene_seg_ring."""
        o = self.opts(mode, spp, depth, 0, flags=flags)
        f = ctypes.c_int32()
        _check(lib().gi_scene_seg_ring(self._h, ctypes.byref(o), ctypes.byref(f)), "gi_scene_seg_ring")
        return bool(f.value)

    def shadow_leaves(self, light, cam_pos):
        """(boundary mask, live mask) over the scene's flat leaf table for a Mode X render with this light
        from this camera position: bit k of the first is set when leaf k lies in a plane with the whole
        scene on one side, bit k of the second when the render's shadow queries visit leaf k (the light
        could be occluded by it) -- gi_scene_shadow_leaves.  (0, 0) without the flat query."""
        b, m = ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().gi_scene_shadow_leaves(self._h, _d3(light), _d3(cam_pos), ctypes.byref(b), ctypes.byref(m)),
               "gi_scene_shadow_leaves")
        return b.value, m.value

    def r_kernel(self, flags=0) -> str:
        """The Mode R kernel a render would run: "k_mode_r" (one lane per pixel), "k_rf_walk" (the flat
        phases k_rf_*, their overflowed tiles by k_mode_r_batch) or "k_mode_r_batch" (the whole frame)
        -- gi_scene_r_kernel."""
        o = self.opts(MODE_R, 1, 1, 0, flags=flags)
        k = ctypes.c_int32()
        _check(lib().gi_scene_r_kernel(self._h, ctypes.byref(o), ctypes.byref(k)), "gi_scene_r_kernel")
        return R_KERNELS[k.value]

    def kernel_ms(self):
        """(average ms, launches) of the dominant kernel over the renders issued with FLAG_TIME since
        the previous call (gi_scene_kernel_ms; waits for the last one, then resets)."""
        ms, n = ctypes.c_float(), ctypes.c_int64()
        _check(lib().gi_scene_kernel_ms(self._h, ctypes.byref(ms), ctypes.byref(n)), "gi_scene_kernel_ms")
        return float(ms.value), int(n.value)

    def trace_ray(self, origin, direction, light):
        hit = Hit()
        rgb = (ctypes.c_double * 3)()
        _check(lib().gi_trace_ray(self._h, _d3(origin), _d3(direction), _d3(light), ctypes.byref(hit), rgb),
               "gi_trace_ray")
        return hit, tuple(rgb)

    # ---- batched ray queries (gi.h "batched ray queries") ------------------------------------------
    INTERSECT_OUTPUTS = ("t", "prim", "entity", "normal")

    def intersect(self, rays: np.ndarray, want=INTERSECT_OUTPUTS) -> dict:
        """Closest hits of host rays (gi_intersect): rays is a C-contiguous float64 array of shape
        (n, RAY_DOUBLES) -- o[3], d[3] (used as given), tmax (may be inf), reserved.  Returns the
        outputs named in want: "t" (n,) float64, "prim" and "entity" (n,) int32, "normal" (n, 3)
        float64; a miss is t = inf, prim = entity = -1, normal = 0.  ValueError for any other input."""
        n = _check_rays(rays)
        want = tuple(want)
        if not want or any(k not in self.INTERSECT_OUTPUTS for k in want) or len(set(want)) != len(want):
            raise ValueError(f"intersect: want is a non-empty selection of {self.INTERSECT_OUTPUTS}")
        m = max(n, 1)   # (a zero-length call still hands the library valid pointers)
        bufs = {"t": np.empty(m, np.float64), "prim": np.empty(m, np.int32), "entity": np.empty(m, np.int32),
                "normal": np.empty((m, 3), np.float64)}
        ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
        ptr = {k: (bufs[k].ctypes.data_as(dp if bufs[k].dtype == np.float64 else ip) if k in want else None)
               for k in self.INTERSECT_OUTPUTS}
        _check(lib().gi_intersect(self._h, n, rays.ctypes.data_as(dp), ptr["t"], ptr["prim"], ptr["entity"], ptr["normal"]),
               "gi_intersect")
        return {k: bufs[k][:n] for k in want}

    def occluded(self, rays: np.ndarray) -> np.ndarray:
        """Any hit of host rays (gi_occluded; rays as for intersect): (n,) int32, 1 where some primitive
        lies at t in (1e-7, tmax), else 0."""
        n = _check_rays(rays)
        out = np.empty(max(n, 1), np.int32)
        _check(lib().gi_occluded(self._h, n, rays.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "gi_occluded")
        return out[:n]

    def intersect_device(self, n: int, d_rays: int, d_t: int = 0, d_prim: int = 0, d_entity: int = 0, d_normal: int = 0,
                         stream: int = 0) -> None:
        """Asynchronous closest hits of n device-resident rays into device buffers (gi_intersect_device);
        pointers are ints, an output of 0 is not written."""
        _check(lib().gi_intersect_device(self._h, int(n), d_rays or None, d_t or None, d_prim or None, d_entity or None,
                                         d_normal or None, stream or None), "gi_intersect_device")

    def occluded_device(self, n: int, d_rays: int, d_occluded: int, stream: int = 0) -> None:
        """Asynchronous any-hit answers (int32, 1 / 0) of n device-resident rays (gi_occluded_device)."""
        _check(lib().gi_occluded_device(self._h, int(n), d_rays or None, d_occluded or None, stream or None),
               "gi_occluded_device")

    # ---- radiance along caller-supplied rays (gi.h "radiance") ---------------------------------------
    def radiance(self, rays: np.ndarray, light, depth: int, ids=None, seed: int = 0, flags: int = 0) -> np.ndarray:
        """The radiance arriving along host rays (gi_radiance): one Mode X path sample per record of rays
        ((n, RAY_DOUBLES) float64; d is normalised by the library, tmax is ignored), its random numbers those of
        ids[i] = (stream, sample) -- a PATH_ID_DTYPE array, None: (i, 0) -- under seed.  Returns (n, 3) float64,
        unclamped: over sample_rays' records, the rows a render of that frame writes.  flags: FLAG_X_NO_SHADOW
        only.  ValueError for any other array."""
        n = _check_rays(rays)
        ids = _check_ids(ids, n)
        out = np.empty((max(n, 1), 3), np.float64)
        p = RadianceParams(int(depth), int(flags), int(seed))
        dp = ctypes.POINTER(ctypes.c_double)
        _check(lib().gi_radiance(self._h, n, rays.ctypes.data_as(dp) if n else ctypes.cast(_scratch_ptr(), dp),
                                 ids.ctypes.data if ids is not None and n else None, _d3(light), ctypes.byref(p),
                                 out.ctypes.data_as(dp)), "gi_radiance")
        return out[:n]

    def radiance_device(self, n: int, d_rays: int, d_rgb: int, light, depth: int, d_ids: int = 0, seed: int = 0,
                        flags: int = 0, stream: int = 0) -> None:
        """Asynchronous radiance of n device-resident rays into a device buffer of n x 3 float64
        (gi_radiance_device); pointers are ints, d_ids = 0: stream = i, sample = 0."""
        p = RadianceParams(int(depth), int(flags), int(seed))
        _check(lib().gi_radiance_device(self._h, int(n), d_rays or None, d_ids or None, _d3(light), ctypes.byref(p),
                                        d_rgb or None, stream or None), "gi_radiance_device")

    # ---- first-hit feature buffers (gi.h "feature buffers") ------------------------------------------
    def render_aov(self, cam: "Camera", w: int, h: int, window=None, want=AOV_OUTPUTS) -> dict:
        """What each pixel of the window (x0, y0, x1, y1) of a w x h frame shows (gi_render_aov; None: the
        whole frame): the outputs named in want as arrays shaped (rows, cols[, 3 | 2]) -- "t" float64
        (distance from the camera; inf: no hit), "normal" and "albedo" float64 x 3, "prim" and "entity"
        int32 (-1: no hit), "uv" int32 x 2.  ValueError for an unknown, repeated or empty want and a
        window that is reversed or not inside the frame."""
        want = tuple(want)
        if not want or any(k not in AOV_OUTPUTS for k in want) or len(set(want)) != len(want):
            raise ValueError(f"render_aov: want is a non-empty selection of {AOV_OUTPUTS}")
        f = _aov_frame(w, h, window)
        rows, cols = f.y1 - f.y0, f.x1 - f.x0
        bufs = {k: np.empty((rows, cols) + _AOV_KINDS[k][1], _AOV_KINDS[k][0]) for k in want}
        a = Aov(**{k: bufs[k].ctypes.data if bufs[k].size else _scratch_ptr() for k in want})
        _check(lib().gi_render_aov(self._h, ctypes.byref(cam._c), ctypes.byref(f), ctypes.byref(a)), "gi_render_aov")
        return bufs

    def render_aov_device(self, cam: "Camera", w: int, h: int, window=None, d_t: int = 0, d_normal: int = 0,
                          d_albedo: int = 0, d_prim: int = 0, d_entity: int = 0, d_uv: int = 0, stream: int = 0) -> None:
        """Asynchronous feature buffers into device planes (gi_render_aov_device); pointers are ints, an
        output of 0 is not written."""
        f = _aov_frame(w, h, window)
        a = Aov(d_t or None, d_normal or None, d_albedo or None, d_prim or None, d_entity or None, d_uv or None)
        _check(lib().gi_render_aov_device(self._h, ctypes.byref(cam._c), ctypes.byref(f), ctypes.byref(a), stream or None),
               "gi_render_aov_device")

    # ---- sample moments of the retained frame (gi.h "sample moments") ---------------------------------
    def frame_samples_info(self) -> dict:
        """The retained frame -- the scene's last render, if it was a whole Mode X frame with spp > 1 on one shard:
        {"w", "h", "n" (samples rendered so far), "spp"} (gi_frame_samples_info); GIError without one."""
        v = [ctypes.c_int32() for _ in range(4)]
        _check(lib().gi_frame_samples_info(self._h, *(ctypes.byref(x) for x in v)), "gi_frame_samples_info")
        return dict(zip(("w", "h", "n", "spp"), (int(x.value) for x in v)))

    def frame_moments(self, w: int, h: int, window=None, want=("mean", "var")) -> dict:
        """Per-pixel sample moments of the retained w x h frame over the window (x0, y0, x1, y1) (None: the whole
        frame), gi_frame_moments: the outputs named in want, float64 -- "mean" (rows, cols, 3), min(mean, 1) being
        the delivered frame; "var" (rows, cols, 3), the sample variance of the mean; "samples" (rows, cols, n, 3),
        the per-sample radiance itself.  ValueError for an unknown, repeated or empty want or a bad window."""
        want = tuple(want)
        if not want or any(k not in MOMENTS_OUTPUTS for k in want) or len(set(want)) != len(want):
            raise ValueError(f"frame_moments: want is a non-empty selection of {MOMENTS_OUTPUTS}")
        f = _aov_frame(w, h, window)
        rows, cols = f.y1 - f.y0, f.x1 - f.x0
        n = self.frame_samples_info()["n"] if "samples" in want else 0
        bufs = {k: np.empty((rows, cols, n, 3) if k == "samples" else (rows, cols, 3), np.float64) for k in want}
        m = Moments(**{k: bufs[k].ctypes.data if bufs[k].size else _scratch_ptr() for k in want})
        _check(lib().gi_frame_moments(self._h, ctypes.byref(f), ctypes.byref(m)), "gi_frame_moments")
        return bufs

    def frame_moments_device(self, w: int, h: int, window=None, d_mean: int = 0, d_var: int = 0, d_samples: int = 0,
                             stream: int = 0) -> None:
        """Asynchronous frame_moments into device planes (gi_frame_moments_device), ordered on the device with the
        scene's renders; pointers are ints, an output of 0 is not written."""
        f = _aov_frame(w, h, window)
        m = Moments(d_mean or None, d_var or None, d_samples or None)
        _check(lib().gi_frame_moments_device(self._h, ctypes.byref(f), ctypes.byref(m), stream or None), "gi_frame_moments_device")

    # ---- adaptive sampling (gi.h "adaptive sampling") --------------------------------------------------
    @staticmethod
    def _adaptive_params(min_samples, tol, relative, y_floor) -> AdaptiveParams:
        return AdaptiveParams(min_samples, ADAPTIVE_RELATIVE if relative else 0, tol, y_floor)

    def render_adaptive(self, cam: Camera, light, w: int, h: int, samples, spp: int, depth: int = 1, seed=0, tol: float = 0.01,
                        min_samples: int = 4, relative: bool = False, y_floor: float = 0.0, flags=0, stats_ptr=0,
                        want=("rgb", "n")) -> dict:
        """One pass, Mode X samples [begin, end) = samples, of an adaptive frame of at most spp samples per pixel
        (gi_render_adaptive): traces the pixels still active, then stops those whose variance of the mean, summed
        over the channels, is at most tol^2 (relative: (tol max(r + g + b, y_floor))^2) once they have min_samples.
        Returns the planes named in want, over the whole frame: "rgb" (h, w, 3) float64 and "rgb8" uint8, the
        delivered frame; "mean" and "var" (h, w, 3), the unclamped mean and the one-pass variance of the mean;
        "n" (h, w) int32, the samples each pixel has received.  ValueError for an unknown, repeated or empty want."""
        want = tuple(want)
        if not want or any(k not in ADAPTIVE_OUTPUTS for k in want) or len(set(want)) != len(want):
            raise ValueError(f"render_adaptive: want is a non-empty selection of {ADAPTIVE_OUTPUTS}")
        bufs = {k: np.empty((h, w) + _ADAPTIVE_KINDS[k][1], _ADAPTIVE_KINDS[k][0]) for k in want}
        o = self.opts(MODE_X, spp, depth, seed, stats_ptr=stats_ptr, flags=flags, samples=samples)
        p = self._adaptive_params(min_samples, tol, relative, y_floor)
        a = AdaptiveOut(**{k: bufs[k].ctypes.data for k in want})
        _check(lib().gi_render_adaptive(self._h, ctypes.byref(cam._c), _d3(light), w, h, ctypes.byref(o), ctypes.byref(p),
                                        ctypes.byref(a)), "gi_render_adaptive")
        return bufs

    def render_adaptive_device(self, cam: Camera, light, w: int, h: int, samples, spp: int, depth: int = 1, seed=0,
                               tol: float = 0.01, min_samples: int = 4, relative: bool = False, y_floor: float = 0.0, flags=0,
                               stats_ptr=0, d_rgb: int = 0, d_rgb8: int = 0, d_mean: int = 0, d_var: int = 0, d_n: int = 0,
                               stream: int = 0) -> None:
        """Asynchronous render_adaptive into device planes (gi_render_adaptive_device): no allocation per call beyond
        the scene's scratch, no copy, no host synchronisation -- a schedule of passes can be queued without reading
        anything back; pointers are ints, an output of 0 is not written."""
        o = self.opts(MODE_X, spp, depth, seed, stats_ptr=stats_ptr, flags=flags, samples=samples)
        p = self._adaptive_params(min_samples, tol, relative, y_floor)
        a = AdaptiveOut(d_rgb or None, d_rgb8 or None, d_mean or None, d_var or None, d_n or None)
        _check(lib().gi_render_adaptive_device(self._h, ctypes.byref(cam._c), _d3(light), w, h, ctypes.byref(o),
                                               ctypes.byref(p), ctypes.byref(a), stream or None), "gi_render_adaptive_device")

    def adaptive_info(self) -> dict:
        """The adaptive frame: {"w", "h", "samples_done" (the last pass's end), "active" (pixels still traced)}
        (gi_adaptive_info: waits for the last pass); GIError without one."""
        v = [ctypes.c_int32() for _ in range(3)]
        act = ctypes.c_int64()
        _check(lib().gi_adaptive_info(self._h, *(ctypes.byref(x) for x in v), ctypes.byref(act)), "gi_adaptive_info")
        return {"w": int(v[0].value), "h": int(v[1].value), "samples_done": int(v[2].value), "active": int(act.value)}

    def kat_r_entities(self, rays: np.ndarray) -> dict:
        """Every ray (o, dir; 6 doubles, dir normalised on the device) against every entity through the
        Mode R kernels' entity test (gi_kat_r_entities; a test hook): hit (n, E) int32 and pn (n, E, 6)."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        n, ne = rays.shape[0], self.info()["n_entities"]
        hit = np.zeros((n, ne), np.int32)
        pn = np.zeros((n, ne, 6))
        _check(lib().gi_kat_r_entities(self._h, n, rays.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                       hit.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                       pn.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "gi_kat_r_entities")
        return dict(hit=hit, pn=pn)

    def kat_x_variant(self, flags: int = 0) -> dict:
        """The kernel variant kat_x_query runs with these flags (flags 0: k_seg's for this scene):
        {"LDS", "W4", "SH", "TRI", "CN", "FLAT"} -> bool (gi_kat_x_variant)."""
        out = (ctypes.c_int32 * 6)()
        _check(lib().gi_kat_x_variant(self._h, int(flags), out), "gi_kat_x_variant")
        return dict(zip(("LDS", "W4", "SH", "TRI", "CN", "FLAT"), (bool(v) for v in out)))

    def kat_x_query(self, recs: np.ndarray, cam_pos, flags: int = 0) -> dict:
        """Ray-level Mode X queries on the device (gi_kat_x_query; a test hook): records (o, d, light,
        d2) of 12 doubles -> prim1, t1, occl, skip_s, prim2, t2, skip2 per ray and the scalar skip_cos
        (None for no rays).  flags: KAT_X_TREE walks the tree where the flat leaf table would apply,
        KAT_X_HBM runs the HBM-resident variant on a scene staged in LDS."""
        recs = np.ascontiguousarray(recs, np.float64).reshape(-1, 12)
        n = recs.shape[0]
        out = dict(prim1=np.zeros(n, np.int32), t1=np.zeros(n), occl=np.zeros(n, np.int32), skip_s=np.zeros(n, np.int32),
                   prim2=np.zeros(n, np.int32), t2=np.zeros(n), skip2=np.zeros(n, np.int32))
        sc = ctypes.c_double(float("nan"))
        ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
        _check(lib().gi_kat_x_query(self._h, n, recs.ctypes.data_as(dp), _d3(cam_pos), int(flags),
                                    out["prim1"].ctypes.data_as(ip), out["t1"].ctypes.data_as(dp),
                                    out["occl"].ctypes.data_as(ip), out["skip_s"].ctypes.data_as(ip),
                                    out["prim2"].ctypes.data_as(ip), out["t2"].ctypes.data_as(dp),
                                    out["skip2"].ctypes.data_as(ip), ctypes.byref(sc)), "gi_kat_x_query")
        out["skip_cos"] = sc.value if n else None
        return out

    def kat_x_texel(self, ents, points, exact: bool = False):
        """The texel Mode X's segment kernels shade a hit with (gi_kat_x_texel; a test hook): entity
        indices (n) and points (n, 3) -> (texel (n, 3) float64, how (n) int32).  exact=False runs the
        shading helper (how: 1 its fp32 filter decided, 2 the exact code, 0 a triangle of truncated
        colour (1, 1, 1)), exact=True the exact texture-coordinate code alone (how: 2)."""
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        n = pts.shape[0]
        recs = np.empty((n, 4), np.float64)
        recs[:, 0] = np.asarray(ents, np.float64).reshape(n)
        recs[:, 1:] = pts
        tex, how = np.zeros((n, 3)), np.zeros(n, np.int32)
        ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
        _check(lib().gi_kat_x_texel(self._h, n, recs.ctypes.data_as(dp), 1 if exact else 0, tex.ctypes.data_as(dp),
                                    how.ctypes.data_as(ip)), "gi_kat_x_texel")
        return tex, how


_scratch = None


def _scratch_ptr() -> int:
    """A valid non-null host address for an output of zero elements (an empty window)."""
    global _scratch
    if _scratch is None:
        _scratch = np.zeros(8)
    return _scratch.ctypes.data


def camera_rays(cam: "Camera", w: int, h: int, window=None) -> np.ndarray:
    """The pixel rays of the window (x0, y0, x1, y1) of a w x h frame (None: the whole frame) as ray
    records for DeviceScene.intersect / occluded (gi_camera_rays): (rows * cols, RAY_DOUBLES) float64,
    row-major over the window -- o = the camera position, d the normalised primary direction the renders
    and render_aov trace, tmax = inf, reserved = 0."""
    f = _aov_frame(w, h, window)
    rays = np.empty(((f.y1 - f.y0) * (f.x1 - f.x0), RAY_DOUBLES), np.float64)
    p = rays.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if rays.size else \
        ctypes.cast(_scratch_ptr(), ctypes.POINTER(ctypes.c_double))
    _check(lib().gi_camera_rays(ctypes.byref(cam._c), ctypes.byref(f), p), "gi_camera_rays")
    return rays


def camera_rays_device(cam: "Camera", w: int, h: int, d_rays: int, window=None, stream: int = 0) -> None:
    """Asynchronous camera_rays into a device buffer of rows * cols records, 16-byte aligned, on the current
    device (gi_camera_rays_device); the pointer is an int."""
    f = _aov_frame(w, h, window)
    _check(lib().gi_camera_rays_device(ctypes.byref(cam._c), ctypes.byref(f), d_rays or None, stream or None),
           "gi_camera_rays_device")


def sample_rays(cam: "Camera", w: int, h: int, samples=1, window=None, seed: int = 0, jitter: bool = True,
                aperture: float = 0.0, focus: float = 1.0):
    """The rays a Mode X render traces for the samples (a count, or (begin, end)) of every pixel of the window of a
    w x h frame, through a thin lens of radius aperture focused at distance focus when aperture > 0
    (gi_sample_rays): (rays, ids), (rows * cols * ns, RAY_DOUBLES) float64 and (rows * cols * ns,) PATH_ID_DTYPE,
    laid out [window pixel, row-major][sample] -- DeviceScene.radiance's inputs.  d is not normalised."""
    f = _aov_frame(w, h, window)
    p = _sample_params(seed, samples, jitter, aperture, focus)
    n = (f.y1 - f.y0) * (f.x1 - f.x0) * (p.sample_end - p.sample_begin)
    rays, ids = np.empty((n, RAY_DOUBLES), np.float64), np.empty(n, PATH_ID_DTYPE)
    _check(lib().gi_sample_rays(ctypes.byref(cam._c), ctypes.byref(f), ctypes.byref(p),
                                rays.ctypes.data if n else _scratch_ptr(), ids.ctypes.data if n else _scratch_ptr()),
           "gi_sample_rays")
    return rays, ids


def sample_rays_device(cam: "Camera", w: int, h: int, d_rays: int, d_ids: int, samples=1, window=None, seed: int = 0,
                       jitter: bool = True, aperture: float = 0.0, focus: float = 1.0, stream: int = 0) -> None:
    """Asynchronous sample_rays into device buffers of rows * cols * ns records (rays 16-byte aligned) on the
    current device (gi_sample_rays_device); pointers are ints, an output of 0 is not written."""
    f = _aov_frame(w, h, window)
    p = _sample_params(seed, samples, jitter, aperture, focus)
    _check(lib().gi_sample_rays_device(ctypes.byref(cam._c), ctypes.byref(f), ctypes.byref(p), d_rays or None,
                                       d_ids or None, stream or None), "gi_sample_rays_device")


def resolve_samples(rows: np.ndarray, want=("rgb", "rgb8")) -> dict:
    """Per-sample radiance rows (n_pix, ns, 3) to pixels as the renders resolve theirs (gi_resolve_samples): "rgb"
    (n_pix, 3) float64, the mean of the rows summed in sample order, clamped at 1; "rgb8" (n_pix, 3) uint8."""
    n_pix, ns = _check_rows(rows)
    want = tuple(want)
    if not want or any(k not in ("rgb", "rgb8") for k in want) or len(set(want)) != len(want):
        raise ValueError('resolve_samples: want is a non-empty selection of ("rgb", "rgb8")')
    bufs = {"rgb": np.empty((max(n_pix, 1), 3), np.float64), "rgb8": np.empty((max(n_pix, 1), 3), np.uint8)}
    dp = ctypes.POINTER(ctypes.c_double)
    _check(lib().gi_resolve_samples(n_pix, ns, rows.ctypes.data_as(dp) if n_pix else ctypes.cast(_scratch_ptr(), dp),
                                    bufs["rgb"].ctypes.data if "rgb" in want else None,
                                    bufs["rgb8"].ctypes.data if "rgb8" in want else None), "gi_resolve_samples")
    return {k: bufs[k][:n_pix] for k in want}


def resolve_samples_device(n_pix: int, ns: int, d_rows: int, d_rgb: int = 0, d_rgb8: int = 0, stream: int = 0) -> None:
    """Asynchronous resolve_samples of device rows [n_pix][ns][3] into device pixels (gi_resolve_samples_device);
    pointers are ints, an output of 0 is not written."""
    _check(lib().gi_resolve_samples_device(int(n_pix), int(ns), d_rows or None, d_rgb or None, d_rgb8 or None,
                                           stream or None), "gi_resolve_samples_device")


def _denoise_params(levels, sigma_c, sigma_p, normal_pow_log2, albedo_stop) -> DenoiseParams:
    return DenoiseParams(int(levels), int(normal_pow_log2), DENOISE_ALBEDO_STOP if albedo_stop else 0, 0, float(sigma_c),
                         float(sigma_p))


def denoise_scratch_bytes(w: int, h: int, window=None, levels: int = 4, sigma_c: float = 0.25, sigma_p: float = 0.01,
                          normal_pow_log2: int = 5, albedo_stop: bool = True) -> int:
    """The bytes of device scratch denoise_device needs for this window and these parameters
    (gi_denoise_scratch_bytes; host code, no device)."""
    f = _aov_frame(w, h, window)
    p = _denoise_params(levels, sigma_c, sigma_p, normal_pow_log2, albedo_stop)
    n = lib().gi_denoise_scratch_bytes(ctypes.byref(f), ctypes.byref(p))
    if n < 0:
        _check(int(n), "gi_denoise_scratch_bytes")
    return int(n)


def denoise(cam: "Camera", w: int, h: int, rgb, t, normal, albedo=None, window=None, levels: int = 4, sigma_c: float = 0.25,
            sigma_p: float = 0.01, normal_pow_log2: int = 5, albedo_stop: bool = True, want=DENOISE_OUTPUTS) -> dict:
    """The edge-avoiding a-trous filter of gi.h "denoiser" over the window (x0, y0, x1, y1) of a w x h frame
    (None: the whole frame), from host arrays (gi_denoise): rgb (rows, cols, 3), and render_aov's t (rows, cols),
    normal and albedo (rows, cols, 3) for the same camera and window, float64; albedo may be None without
    albedo_stop.  sigma_c: about 0.5 / sqrt(samples accumulated so far).  Returns the outputs named in want:
    "rgb" (rows, cols, 3) float64, "rgb8" (rows, cols, 3) uint8.  ValueError for a wrong shape or want."""
    want = tuple(want)
    if not want or any(k not in DENOISE_OUTPUTS for k in want) or len(set(want)) != len(want):
        raise ValueError(f"denoise: want is a non-empty selection of {DENOISE_OUTPUTS}")
    f = _aov_frame(w, h, window)
    rows, cols = f.y1 - f.y0, f.x1 - f.x0
    if albedo is None and albedo_stop:
        raise ValueError("denoise: albedo_stop needs the albedo plane")

    def plane(name, a, tail):
        a = np.ascontiguousarray(a, np.float64)
        if a.size != rows * cols * (tail[0] if tail else 1):
            raise ValueError(f"denoise: {name} must hold {(rows, cols) + tail} float64")
        return a
    ins = {"rgb": plane("rgb", rgb, (3,)), "t": plane("t", t, ()), "normal": plane("normal", normal, (3,))}
    if albedo is not None:
        ins["albedo"] = plane("albedo", albedo, (3,))
    bufs = {"rgb": np.empty((rows, cols, 3), np.float64), "rgb8": np.empty((rows, cols, 3), np.uint8)}
    io = DenoiseIO(**{k: (a.ctypes.data if a.size else _scratch_ptr()) for k, a in ins.items()},
                   # (an empty window: valid addresses, the outputs' apart from the inputs' -- out_rgb is not rgb)
                   **{"out_" + k: (bufs[k].ctypes.data if bufs[k].size else _scratch_ptr() + 32) for k in want})
    p = _denoise_params(levels, sigma_c, sigma_p, normal_pow_log2, albedo_stop)
    _check(lib().gi_denoise(ctypes.byref(cam._c), ctypes.byref(f), ctypes.byref(p), ctypes.byref(io)), "gi_denoise")
    return {k: bufs[k] for k in want}


def denoise_device(cam: "Camera", w: int, h: int, d_rgb: int, d_t: int, d_normal: int, d_albedo: int, d_scratch: int,
                   scratch_bytes: int, d_out_rgb: int = 0, d_out_rgb8: int = 0, window=None, levels: int = 4,
                   sigma_c: float = 0.25, sigma_p: float = 0.01, normal_pow_log2: int = 5, albedo_stop: bool = True,
                   stream: int = 0) -> None:
    """Asynchronous denoise of device planes into device outputs on the current device (gi_denoise_device);
    pointers are ints, an output of 0 is not written.  d_scratch: scratch_bytes >= denoise_scratch_bytes(...)
    bytes of device memory, 16-byte aligned, the call's own until its launches have run."""
    f = _aov_frame(w, h, window)
    io = DenoiseIO(d_rgb or None, d_t or None, d_normal or None, d_albedo or None, d_out_rgb or None, d_out_rgb8 or None)
    p = _denoise_params(levels, sigma_c, sigma_p, normal_pow_log2, albedo_stop)
    _check(lib().gi_denoise_device(ctypes.byref(cam._c), ctypes.byref(f), ctypes.byref(p), ctypes.byref(io), d_scratch or None,
                                   int(scratch_bytes), stream or None), "gi_denoise_device")


def _denoise_var_params(levels, sigma_v, sigma_p, var_floor, normal_pow_log2, albedo_stop) -> DenoiseVarParams:
    return DenoiseVarParams(int(levels), int(normal_pow_log2), DENOISE_ALBEDO_STOP if albedo_stop else 0, 0, float(sigma_v),
                            float(sigma_p), float(var_floor))


def denoise_var_scratch_bytes(w: int, h: int, window=None, levels: int = 4, sigma_v: float = DENOISE_VAR_SIGMA_V,
                              sigma_p: float = 0.01, var_floor: float = DENOISE_VAR_FLOOR, normal_pow_log2: int = 5,
                              albedo_stop: bool = True) -> int:
    """The bytes of device scratch denoise_var_device needs for this window and these parameters
    (gi_denoise_var_scratch_bytes; host code, no device)."""
    f = _aov_frame(w, h, window)
    p = _denoise_var_params(levels, sigma_v, sigma_p, var_floor, normal_pow_log2, albedo_stop)
    n = lib().gi_denoise_var_scratch_bytes(ctypes.byref(f), ctypes.byref(p))
    if n < 0:
        _check(int(n), "gi_denoise_var_scratch_bytes")
    return int(n)


def denoise_var(cam: "Camera", w: int, h: int, rgb, var, t, normal, albedo=None, window=None, levels: int = 4,
                sigma_v: float = DENOISE_VAR_SIGMA_V, sigma_p: float = 0.01, var_floor: float = DENOISE_VAR_FLOOR,
                normal_pow_log2: int = 5, albedo_stop: bool = True, want=DENOISE_VAR_OUTPUTS) -> dict:
    """The variance-guided filter of gi.h "variance-guided denoiser" from host arrays (gi_denoise_var): denoise's
    planes plus var (rows, cols, 3), the variance of the mean (DeviceScene.frame_moments' "var", with its "mean" as
    rgb); the colour stop of a pixel is sigma_v^2 times its prefiltered variance plus var_floor.  Returns the
    outputs named in want: "rgb" and "var" (rows, cols, 3) float64, "rgb8" (rows, cols, 3) uint8.  ValueError for a
    wrong shape or want."""
    want = tuple(want)
    if not want or any(k not in DENOISE_VAR_OUTPUTS for k in want) or len(set(want)) != len(want):
        raise ValueError(f"denoise_var: want is a non-empty selection of {DENOISE_VAR_OUTPUTS}")
    f = _aov_frame(w, h, window)
    rows, cols = f.y1 - f.y0, f.x1 - f.x0
    if albedo is None and albedo_stop:
        raise ValueError("denoise_var: albedo_stop needs the albedo plane")

    def plane(name, a, tail):
        a = np.ascontiguousarray(a, np.float64)
        if a.size != rows * cols * (tail[0] if tail else 1):
            raise ValueError(f"denoise_var: {name} must hold {(rows, cols) + tail} float64")
        return a
    ins = {"rgb": plane("rgb", rgb, (3,)), "var": plane("var", var, (3,)), "t": plane("t", t, ()),
           "normal": plane("normal", normal, (3,))}
    if albedo is not None:
        ins["albedo"] = plane("albedo", albedo, (3,))
    bufs = {"rgb": np.empty((rows, cols, 3), np.float64), "var": np.empty((rows, cols, 3), np.float64),
            "rgb8": np.empty((rows, cols, 3), np.uint8)}
    io = DenoiseVarIO(**{k: (a.ctypes.data if a.size else _scratch_ptr()) for k, a in ins.items()},
                      # (an empty window: valid addresses, the outputs' apart from the inputs')
                      **{"out_" + k: (bufs[k].ctypes.data if bufs[k].size else _scratch_ptr() + 32) for k in want})
    p = _denoise_var_params(levels, sigma_v, sigma_p, var_floor, normal_pow_log2, albedo_stop)
    _check(lib().gi_denoise_var(ctypes.byref(cam._c), ctypes.byref(f), ctypes.byref(p), ctypes.byref(io)), "gi_denoise_var")
    return {k: bufs[k] for k in want}


def denoise_var_device(cam: "Camera", w: int, h: int, d_rgb: int, d_var: int, d_t: int, d_normal: int, d_albedo: int,
                       d_scratch: int, scratch_bytes: int, d_out_rgb: int = 0, d_out_var: int = 0, d_out_rgb8: int = 0,
                       window=None, levels: int = 4, sigma_v: float = DENOISE_VAR_SIGMA_V, sigma_p: float = 0.01,
                       var_floor: float = DENOISE_VAR_FLOOR, normal_pow_log2: int = 5, albedo_stop: bool = True,
                       stream: int = 0) -> None:
    """Asynchronous denoise_var of device planes into device outputs on the current device (gi_denoise_var_device);
    pointers are ints, an output of 0 is not written.  d_scratch: scratch_bytes >= denoise_var_scratch_bytes(...)
    bytes of device memory, 16-byte aligned, the call's own until its launches have run."""
    f = _aov_frame(w, h, window)
    io = DenoiseVarIO(d_rgb or None, d_var or None, d_t or None, d_normal or None, d_albedo or None, d_out_rgb or None,
                      d_out_var or None, d_out_rgb8 or None)
    p = _denoise_var_params(levels, sigma_v, sigma_p, var_floor, normal_pow_log2, albedo_stop)
    _check(lib().gi_denoise_var_device(ctypes.byref(cam._c), ctypes.byref(f), ctypes.byref(p), ctypes.byref(io), d_scratch or None,
                                       int(scratch_bytes), stream or None), "gi_denoise_var_device")


def _temporal_params(max_history, alpha_min, cos_min, sigma_p, prim_stop) -> TemporalParams:
    return TemporalParams(int(max_history), TEMPORAL_PRIM_STOP if prim_stop else 0, float(alpha_min), float(cos_min), float(sigma_p))


# temporal's defaults are starting values (README.md "Temporal accumulation": what they do on the Cornell box)
def temporal(cam: "Camera", prev_cam: Optional["Camera"], w: int, h: int, cur: dict, hist: Optional[dict] = None, window=None,
             max_history: int = 32, alpha_min: float = 0.0, cos_min: float = 0.9, sigma_p: float = 0.01, prim_stop: bool = True,
             want=TEMPORAL_OUTPUTS) -> dict:
    """The temporal accumulation of gi.h "temporal accumulation" over the window (x0, y0, x1, y1) of a w x h frame
    (None: the whole frame), from host arrays (gi_temporal).  cur: the current frame's planes by name -- "rgb"
    (rows, cols, 3) float64 (frame_moments' "mean", or the frame), "t" (rows, cols) and "normal" (rows, cols, 3)
    float64 of render_aov for cam, "prim" (rows, cols) int32 with prim_stop, "var" (rows, cols, 3) float64 where the
    variance is carried.  hist: the previous frame's planes for prev_cam -- the accumulated "rgb" (and "var"), that
    frame's "t", "normal" (and "prim"), and "len" (rows, cols) int32, the samples accumulated per pixel; None (prev_cam
    may be None too): the first frame, every valid pixel resets.  Returns the outputs named in want: "rgb" and "var"
    (rows, cols, 3) float64, "len" (rows, cols) int32 -- with this frame's t, normal and prim the next call's hist.
    ValueError for a wrong shape, a missing plane or a wrong want."""
    want = tuple(want)
    if not want or any(k not in TEMPORAL_OUTPUTS for k in want) or len(set(want)) != len(want):
        raise ValueError(f"temporal: want is a non-empty selection of {TEMPORAL_OUTPUTS}")
    f = _aov_frame(w, h, window)
    rows, cols = f.y1 - f.y0, f.x1 - f.x0
    if hist is not None and prev_cam is None:
        raise ValueError("temporal: a history needs prev_cam")
    kinds = {"rgb": (np.float64, (3,)), "var": (np.float64, (3,)), "t": (np.float64, ()), "normal": (np.float64, (3,)),
             "prim": (np.int32, ()), "len": (np.int32, ())}

    def planes(side, d, need):
        missing = [k for k in need if d.get(k) is None]
        if missing:
            raise ValueError(f"temporal: {side} lacks {missing}")
        got = {}
        for k in need:
            dt, tail = kinds[k]
            a = np.ascontiguousarray(d[k], dt)
            if a.size != rows * cols * (tail[0] if tail else 1):
                raise ValueError(f"temporal: {side}[{k!r}] must hold {(rows, cols) + tail} {np.dtype(dt).name}")
            got[k] = a
        return got
    need = ["rgb", "t", "normal"] + (["prim"] if prim_stop else []) + (["var"] if "var" in want else [])
    c = planes("cur", cur, need)
    hh = planes("hist", hist, need + ["len"]) if hist is not None else None
    bufs = {"rgb": np.empty((rows, cols, 3), np.float64), "var": np.empty((rows, cols, 3), np.float64),
            "len": np.empty((rows, cols), np.int32)}

    def frame_of(d):   # (an empty window: valid addresses, apart from the outputs')
        return TemporalFrame(**{k: (a.ctypes.data if a.size else _scratch_ptr()) for k, a in d.items()})
    fc, fh = frame_of(c), (frame_of(hh) if hh is not None else None)
    out = TemporalOut(**{k: (bufs[k].ctypes.data if bufs[k].size else _scratch_ptr() + 32) for k in want})
    p = _temporal_params(max_history, alpha_min, cos_min, sigma_p, prim_stop)
    _check(lib().gi_temporal(ctypes.byref(cam._c), ctypes.byref(prev_cam._c) if prev_cam is not None else None, ctypes.byref(f),
                             ctypes.byref(p), ctypes.byref(fc), ctypes.byref(fh) if fh is not None else None, ctypes.byref(out)),
           "gi_temporal")
    return {k: bufs[k] for k in want}


def temporal_device(cam: "Camera", prev_cam: Optional["Camera"], w: int, h: int, d_cur: dict, d_hist: Optional[dict] = None,
                    d_out_rgb: int = 0, d_out_var: int = 0, d_out_len: int = 0, window=None, max_history: int = 32,
                    alpha_min: float = 0.0, cos_min: float = 0.9, sigma_p: float = 0.01, prim_stop: bool = True,
                    stream: int = 0) -> None:
    """Asynchronous temporal of device planes into device outputs on the current device (gi_temporal_device); d_cur and
    d_hist map the names of TEMPORAL_PLANES to device pointers (ints; a missing name or 0: null), d_hist None: the
    first frame; an output of 0 is not written.  No scratch."""
    f = _aov_frame(w, h, window)

    def frame_of(d):
        if any(k not in TEMPORAL_PLANES for k in d):
            raise ValueError(f"temporal_device: the planes are named {TEMPORAL_PLANES}")
        return TemporalFrame(**{k: (int(v) or None) for k, v in d.items() if v})
    fc, fh = frame_of(d_cur), (frame_of(d_hist) if d_hist is not None else None)
    out = TemporalOut(d_out_rgb or None, d_out_var or None, d_out_len or None)
    p = _temporal_params(max_history, alpha_min, cos_min, sigma_p, prim_stop)
    _check(lib().gi_temporal_device(ctypes.byref(cam._c), ctypes.byref(prev_cam._c) if prev_cam is not None else None, ctypes.byref(f),
                                    ctypes.byref(p), ctypes.byref(fc), ctypes.byref(fh) if fh is not None else None, ctypes.byref(out),
                                    stream or None), "gi_temporal_device")


def devices_from_env(default=None):
    """GI_DEVICES="0,1,2,3" (device per shard; repeats allowed) or "all"; None when unset."""
    v = os.environ.get("GI_DEVICES")
    if not v:
        return default
    if v.strip() == "all":
        import torch
        return list(range(torch.cuda.device_count()))
    return [int(t) for t in v.split(",") if t.strip()]


class MultiScene:
    """RayTracer::run over several GPUs of this process (gi_multi_*): a scene replica per device,
    8x8 tiles dealt round-robin over the shards, packed tiles gathered to devices[0] by RCCL
    send/recv over xGMI, bit-identical to a one-device render."""

    def __init__(self, octree: Octree, devices: Sequence[int]):
        L = lib()
        d, keep = octree._scene_desc()
        devs = (ctypes.c_int * len(devices))(*[int(x) for x in devices])
        h = ctypes.c_void_p()
        _check(L.gi_multi_create(ctypes.byref(d), len(devices), devs, ctypes.byref(h)), "gi_multi_create")
        self._h = h
        del keep

    @classmethod
    def from_scene(cls, s: "_scenes.Scene", devices: Sequence[int]) -> "MultiScene":
        return cls(Octree.from_scene(s), devices)

    def info(self) -> dict:
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(lib().gi_multi_info(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "gi_multi_info")
        return {"shards": a.value, "devices": b.value, "rccl": bool(c.value)}

    def render(self, cam: Camera, light, w: int, h: int, mode=MODE_R, spp=1, depth=1, seed=0, band_rows=0,
               cancel: Optional[ctypes.c_int] = None, callback=None, out=None):
        """gi_multi_render into host arrays; out=(rgb, rgb8) as DeviceScene.render (either may be None)."""
        if out is None:
            rgb, rgb8 = np.zeros((h, w, 3), np.float64), np.zeros((h, w, 3), np.uint8)
        else:
            rgb, rgb8 = out
        for a, dt in ((rgb, np.float64), (rgb8, np.uint8)):
            if a is not None and (a.dtype != dt or a.size != w * h * 3 or not a.flags.c_contiguous):
                raise ValueError("render: out arrays must be C-contiguous [h, w, 3] float64 / uint8")
        cb = TILE_CB(callback) if callback is not None else TILE_CB()
        o = DeviceScene.opts(mode, spp, depth, seed, band_rows=band_rows)
        _check(lib().gi_multi_render(self._h, ctypes.byref(cam._c), _d3(light), w, h, ctypes.byref(o),
                                     rgb.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if rgb is not None else None,
                                     rgb8.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if rgb8 is not None else None,
                                     ctypes.byref(cancel) if cancel is not None else None, cb, None), "gi_multi_render")
        return rgb, rgb8

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            lib().gi_multi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kat_expbox(recs: np.ndarray) -> np.ndarray:
    """Device ExpBox node test over (min, max, origin, dir) records (gi_kat_expbox)."""
    recs = np.ascontiguousarray(recs, np.float64)
    out = np.zeros(recs.shape[0], np.int32)
    _check(lib().gi_kat_expbox(recs.shape[0], recs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "gi_kat_expbox")
    return out


KAT_R_TRI, KAT_R_SPHERE, KAT_R_BOX, KAT_R_BOX4 = 0, 1, 2, 3
_KAT_R_WIDTH = {KAT_R_TRI: 15, KAT_R_SPHERE: 10, KAT_R_BOX: 12, KAT_R_BOX4: 12}


def kat_r_prims(kind: int, recs: np.ndarray) -> dict:
    """Mode R's primitive tests on the device, record by record (gi_kat_r_prims; a test hook): triangles
    (p1 p2 p3 o dir), spheres (pos radius o dir), boxes (min max o dir) by one lane or by the grouped
    node test.  hit (n,) int32; pn (n, 6) point and normal for triangles and spheres, None for boxes."""
    recs = np.ascontiguousarray(recs, np.float64).reshape(-1, _KAT_R_WIDTH[kind])
    n = recs.shape[0]
    hit = np.zeros(n, np.int32)
    pn = np.zeros((n, 6)) if kind in (KAT_R_TRI, KAT_R_SPHERE) else None
    _check(lib().gi_kat_r_prims(int(kind), n, recs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                hit.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                pn.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if pn is not None else None),
           "gi_kat_r_prims")
    return dict(hit=hit, pn=pn)


def shard_tiles(w: int, h: int, shard_count: int) -> int:
    return int(lib().gi_shard_tiles(w, h, shard_count))


def unshard_device(w, h, shard_count, d_packed, d_packed8, d_rgb, d_rgb8, stream=0) -> None:
    _check(lib().gi_unshard_device(w, h, shard_count, d_packed or None, d_packed8 or None, d_rgb or None,
                                   d_rgb8 or None, stream or None), "gi_unshard_device")


class Image:
    """What the reference's Image (image.h:7-29) holds after run(): RGB888 pixels."""

    def __init__(self, rgb8: np.ndarray, rgb: Optional[np.ndarray] = None):
        self.rgb8 = rgb8
        self.radiance = rgb

    def width(self) -> int:
        return self.rgb8.shape[1]

    def height(self) -> int:
        return self.rgb8.shape[0]

    def getPixel(self, x: int, y: int):
        p = self.rgb8[y, x]
        return (p[0] / 255.0, p[1] / 255.0, p[2] / 255.0)


class RayTracer:
    """RayTracer(camera, light) (raytracer.h:15-101) backed by the gfx950 kernels."""

    def __init__(self, camera: Camera, light):
        self._camera = camera
        self._light = tuple(float(v) for v in light)
        self._image = Image(np.zeros((0, 0, 3), np.uint8))
        self._scene: Optional[Octree] = None
        self._dev: Optional[DeviceScene] = None
        self._cancel = ctypes.c_int(1)   # _running = false (raytracer.h:96)
        self.band_rows = 64              # progressive granularity (reference: per pixel)

    def setScene(self, scene: Octree) -> None:
        self._scene = scene
        self._dev = None   # rebuilt lazily on the next run()
        self._dev_gen = -1

    def running(self) -> bool:
        return self._cancel.value == 0

    def stop(self) -> None:
        self._cancel.value = 1

    def start(self) -> None:
        self._cancel.value = 0

    def getImage(self) -> Image:
        return self._image

    def run(self, w: int, h: int) -> None:
        self._image = Image(np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3)))   # raytracer.h:25
        if self._scene is None:
            raise GIError("setScene() was not called")
        # the reference reads the live octree on every run (raytracer.h:45): re-upload after push_back
        if self._dev is None or getattr(self, "_dev_gen", -1) != self._scene.generation:
            devs = devices_from_env()
            self._dev = MultiScene(self._scene, devs) if devs and len(devs) > 1 else DeviceScene(self._scene)
            self._dev_gen = self._scene.generation
        img = self._image

        def on_band(_user, y0, rows, p8, pf):
            n = w * rows * 3
            img.rgb8[y0:y0 + rows] = np.ctypeslib.as_array(p8, shape=(n,)).reshape(rows, w, 3)
            img.radiance[y0:y0 + rows] = np.ctypeslib.as_array(pf, shape=(n,)).reshape(rows, w, 3)

        rgb = np.zeros((h, w, 3))
        rgb8 = np.zeros((h, w, 3), np.uint8)
        o = DeviceScene.opts(MODE_R, band_rows=self.band_rows)
        cb = TILE_CB(on_band)
        fn = lib().gi_multi_render if isinstance(self._dev, MultiScene) else lib().gi_render
        rc = fn(self._dev._h, ctypes.byref(self._camera._c), _d3(self._light), w, h, ctypes.byref(o),
                             rgb.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                             rgb8.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(self._cancel), cb, None)
        if rc not in (0, -4):   # -4: stopped, partial frame like the reference's loop exit
            _check(rc, "gi_render")
