"""ada-ray-tracer_amd -- host-side binding of libart_hip.so (MI355X / gfx950 render backend).

The product is the C ABI in include/art_hip.h; this module is the thin ctypes layer the tests, bench.py
and the multi-GPU harness use, plus a mirror of the reference's host interface
(Ray_Tracer.Init_Render / Resize_Viewport / Render_Pass / GetSPP / Finished, ray_tracer.ads:40-48)
so that callers read like test.adb:32-75.

The directory name contains a hyphen, so import it through ``__graft_entry__.load_package()`` (which
registers it as ``ada_ray_tracer_amd``).  There is no CPU fallback: every call needs the HIP library
and a GPU and raises ``ArtError`` otherwise.
"""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from . import radiance      # art_radiance_rays_device: ArtRadianceParams and Backend.radiance_rays_torch
from . import aov_rays      # art_aovs_rays_device, art_camera_rays_device: their structs, Backend.aovs_rays_torch and camera_rays_torch
from . import display       # art_auto_exposure_device, art_display_device: their structs and constants, Backend.exposure_state, auto_exposure_torch, display_torch
from . import upsample      # art_upsample_device: its structs and Backend.upsample_torch
from . import firefly       # art_firefly_device: its struct, its defaults and Backend.firefly_torch
from . import bloom         # art_bloom_device: its struct, its defaults and Backend.bloom_torch
from . import temporal_upsample      # art_temporal_upsample_device: its structs, Backend.temporal_upsample_torch, jitter_sequence, jittered_camera

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("ART_LIB", os.path.join(PKG_DIR, "libart_hip.so"))   # ART_LIB: A/B builds of the same source
# the C++ mirror of the Ada host layer (host/); ART_ASAN=1: its AddressSanitizer + UBSan build (tests/run_sanitizers.sh, CPU only)
HOST_LIB_PATH = os.path.join(PKG_DIR, "libart_host_asan.so" if os.environ.get("ART_ASAN", "") not in ("", "0") else "libart_host.so")

f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)
u32p = C.POINTER(C.c_uint32)

MAT_NULL, MAT_LIGHT, MAT_LAMBERT, MAT_MIRROR, MAT_GLASS, MAT_PHONG = range(6)
LIGHT_RECT, LIGHT_SPHERE = 0, 1
MESH_REFERENCE_BF, MESH_CLOSEST = 0, 1
RT_DEBUG, RT_WHITTED, PT_STUPID, PT_SHADOW, PT_MIS = range(5)
LAYOUT_ADA_XY, LAYOUT_ROW_MAJOR = 0, 1
TRACE_COOP, TRACE_SIMPLE = 0, 1
BVH_HOST_SAH, BVH_GPU_LBVH, BVH_GPU_PLOC, BVH_GPU_SAH = 0, 1, 2, 3     # option "bvh_builder"
DEFAULT_BVH_BUILDER = BVH_GPU_SAH


class ArtError(RuntimeError):
    pass


class ArtMaterial(C.Structure):
    _fields_ = [("type", C.c_int32), ("light", C.c_int32), ("p", C.c_float * 8)]


class ArtLight(C.Structure):
    _fields_ = [("shape", C.c_int32), ("mat", C.c_int32),
                ("boxMin", C.c_float * 3), ("boxMax", C.c_float * 3), ("normal", C.c_float * 3),
                ("center", C.c_float * 3), ("radius", C.c_float),
                ("intensity", C.c_float * 3), ("surfaceArea", C.c_float)]


class ArtSphere(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("r", C.c_float), ("mat", C.c_int32)]


class ArtMesh(C.Structure):
    _fields_ = [("mode", C.c_int32), ("nverts", C.c_int32), ("ntris", C.c_int32),
                ("pos", f32p), ("nrm", f32p), ("uv", f32p), ("idx", i32p), ("matid", i32p),
                ("bbmin", C.c_float * 3), ("bbmax", C.c_float * 3)]


class ArtInstance(C.Structure):
    _fields_ = [("mesh", C.c_int32), ("m", C.c_float * 12)]


class ArtSceneDesc(C.Structure):
    _fields_ = [("n_spheres", C.c_int32), ("spheres", C.POINTER(ArtSphere)),
                ("has_cornell", C.c_int32),
                ("cb_min", C.c_float * 3), ("cb_max", C.c_float * 3),
                ("cb_mat", C.c_int32 * 6), ("cb_nrm", (C.c_float * 3) * 6),
                ("n_lights", C.c_int32), ("lights", C.POINTER(ArtLight)),
                ("n_materials", C.c_int32), ("materials", C.POINTER(ArtMaterial)),
                ("n_meshes", C.c_int32), ("meshes", C.POINTER(ArtMesh)),
                ("cam_pos", C.c_float * 3), ("cam_matrix", C.c_float * 16),
                ("n_instances", C.c_int32), ("instances", C.POINTER(ArtInstance))]


class ArtPassParams(C.Structure):
    _fields_ = [("render_type", C.c_int32), ("aa_on", C.c_int32), ("max_depth", C.c_int32), ("vthreads", C.c_int32),
                ("background", C.c_float * 3), ("seed", C.c_uint64), ("layout", C.c_int32)]


class ArtStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("samples", C.c_uint64), ("trace_ms", C.c_double), ("pass_ms", C.c_double),
                ("trace_launches", C.c_uint64), ("box_tests", C.c_uint64), ("tri_tests", C.c_uint64),
                ("node_visits", C.c_uint64), ("leaf_visits", C.c_uint64), ("traced_rays", C.c_uint64),
                ("node_phase_iters", C.c_uint64), ("leaf_phase_iters", C.c_uint64), ("wave_iters", C.c_uint64), ("lost_paths", C.c_uint64)]


class ArtStageStats(C.Structure):
    _fields_ = [("shade_ms", C.c_double), ("raygen_ms", C.c_double), ("fold_ms", C.c_double), ("shade_launches", C.c_uint64), ("batches", C.c_uint64),
                ("items_in", C.c_uint64 * 16), ("items_out", C.c_uint64 * 16)]


class ArtReduceInfo(C.Structure):
    _fields_ = [("devices", C.c_int32), ("rccl_ranks", C.c_int32), ("path", C.c_int32), ("reduces", C.c_int32),
                ("reduce_ms", C.c_double), ("device_pass_ms", C.c_double * 8),
                ("device_busy_ms", C.c_double * 8), ("device_idle_ms", C.c_double * 8), ("device_start_skew_ms", C.c_double * 8),
                ("passes", C.c_int32), ("passes_overlapped", C.c_int32)]


class ArtHit(C.Structure):
    _fields_ = [("t", C.c_float), ("is_hit", C.c_int32), ("prim_type", C.c_int32), ("prim_index", C.c_int32),
                ("mat_id", C.c_int32), ("mat", C.c_int32), ("normal", C.c_float * 3), ("u", C.c_float), ("v", C.c_float)]


class ArtAovBuffers(C.Structure):
    _fields_ = [("albedo3f", C.c_void_p), ("normal3f", C.c_void_p), ("depth", C.c_void_p), ("alpha", C.c_void_p),
                ("prim_type", C.c_void_p), ("prim_index", C.c_void_p), ("mat", C.c_void_p)]


class ArtMotionSource(C.Structure):
    _fields_ = [("cur_pos3f", C.c_void_p), ("prev_pos3f", C.c_void_p), ("nverts", C.c_int64), ("prev_m12f", C.c_void_p), ("n_instances", C.c_int64)]


class ArtDenoiseParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("demodulate", C.c_int32),
                ("normal_log2", C.c_int32), ("variant", C.c_int32), ("scale", C.c_float), ("sigma_color", C.c_float), ("sigma_depth", C.c_float)]


class ArtSvgfParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("demodulate", C.c_int32),
                ("normal_log2", C.c_int32), ("n_colours", C.c_int32), ("scale", C.c_float), ("sigma_color", C.c_float), ("sigma_depth", C.c_float)]


class ArtTemporalCamera(C.Structure):
    _fields_ = [("cam_pos", C.c_float * 3), ("cam_matrix", C.c_float * 16), ("width", C.c_int32), ("height", C.c_int32)]


class ArtTemporalParams(C.Structure):
    _fields_ = [("cur", ArtTemporalCamera), ("prev", ArtTemporalCamera), ("n_colours", C.c_int32), ("max_history", C.c_int32),
                ("scale", C.c_float), ("depth_tol", C.c_float), ("normal_min", C.c_float)]


class ArtSvgfSpatialParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("radius", C.c_int32), ("normal_log2", C.c_int32), ("min_history", C.c_float),
                ("sigma_depth", C.c_float)]


class ArtAdaptiveParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("aa_on", C.c_int32), ("min_colours", C.c_int32), ("max_samples", C.c_int32),
                ("threshold", C.c_float), ("lum_floor", C.c_float)]


# Backend.render_aovs_torch: plane -> (field of ArtAovBuffers, floats or ints per pixel, integer plane)
AOV_PLANES = collections.OrderedDict([("albedo", ("albedo3f", 3, False)), ("normal", ("normal3f", 3, False)), ("depth", ("depth", 1, False)),
                                      ("alpha", ("alpha", 1, False)), ("prim_type", ("prim_type", 1, True)), ("prim_index", ("prim_index", 1, True)),
                                      ("mat", ("mat", 1, True))])


class ArtBvhInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("n_tris", C.c_int32), ("max_stack", C.c_int32), ("node_width", C.c_int32),
                ("build_ms", C.c_double)]


class ArtRefitInfo(C.Structure):
    _fields_ = [("refits", C.c_uint64), ("refit_ms", C.c_double), ("plan_ms", C.c_double), ("bad_vertices", C.c_uint64)]


class ArtRebuildInfo(C.Structure):
    _fields_ = [("rebuilds", C.c_uint64), ("gather_ms", C.c_double), ("build_ms", C.c_double), ("host_ms", C.c_double)]


class ArtTreeCost(C.Structure):
    _fields_ = [("root_area", C.c_double), ("node_visits", C.c_double), ("leaf_visits", C.c_double), ("tri_tests", C.c_double)]


class ArtMoveInfo(C.Structure):
    _fields_ = [("moves", C.c_uint64), ("move_ms", C.c_double), ("plan_ms", C.c_double), ("bad_matrices", C.c_uint64), ("repads", C.c_uint64)]


class ArtMeshRefitInfo(C.Structure):
    _fields_ = [("refits", C.c_uint64), ("refit_ms", C.c_double), ("plan_ms", C.c_double), ("bad_vertices", C.c_uint64), ("repads", C.c_uint64)]


class ArtInstanceRebuildInfo(C.Structure):
    _fields_ = [("rebuilds", C.c_uint64), ("gather_ms", C.c_double), ("build_ms", C.c_double), ("host_ms", C.c_double)]


class ArtMeshRebuildInfo(C.Structure):
    _fields_ = [("rebuilds", C.c_uint64), ("gather_ms", C.c_double), ("build_ms", C.c_double), ("host_ms", C.c_double)]


class ArtTwoLevelInfo(C.Structure):
    _fields_ = [("n_inst", C.c_int32), ("n_entry", C.c_int32), ("n_mesh", C.c_int32), ("n_tlas_nodes", C.c_int32), ("n_blas_nodes", C.c_int32),
                ("n_records", C.c_int32), ("inst_shift", C.c_int32), ("updated", C.c_int32),
                ("mesh_pad_rel", C.c_float), ("mesh_pad_min", C.c_float), ("scene_extent", C.c_float), ("tlas_pad_rel", C.c_float),
                ("tlas_pad_abs", C.c_float), ("reserved_", C.c_int32)]


TWO_LEVEL_ARRAYS = ("inst", "tlas_nodes", "tlas_tris", "blas_nodes", "blas_tris", "qnodes", "mesh_pad", "mesh_box", "mesh_base", "node_mesh")


class ArtTwoLevelBuffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in TWO_LEVEL_ARRAYS] + [("cap", C.c_int64 * 10)]


def two_level_arrays(call):
    """call(info pointer, buffers pointer or None) -> rc is art_export_two_level or a function with its arguments: the sizes first, then
    the arrays.  Returns (dict of numpy arrays and of the info's scalars, rc): rc != 0 means the call failed and the dict is None."""
    info = ArtTwoLevelInfo()
    rc = call(C.byref(info), None)
    if rc:
        return None, rc
    i = info
    shapes = dict(inst=((i.n_entry, 32), np.uint32), tlas_nodes=((i.n_tlas_nodes, 32), np.float32), tlas_tris=((i.n_entry, 12), np.float32),
                  blas_nodes=((i.n_blas_nodes, 32), np.float32), blas_tris=((i.n_records, 12), np.float32),
                  qnodes=((i.n_tlas_nodes + i.n_blas_nodes, 16), np.uint32), mesh_pad=((i.n_mesh,), np.float32), mesh_box=((i.n_mesh, 6), np.float32),
                  mesh_base=((i.n_mesh, 3), np.int32), node_mesh=((i.n_blas_nodes,), np.int32))
    out = {name: np.zeros(*shapes[name]) for name in TWO_LEVEL_ARRAYS}
    buf = ArtTwoLevelBuffers()
    for k, name in enumerate(TWO_LEVEL_ARRAYS):
        setattr(buf, name, out[name].ctypes.data); buf.cap[k] = out[name].size
    rc = call(C.byref(info), C.byref(buf))
    if rc:
        return None, rc
    for name in ("n_inst", "inst_shift", "updated"):
        out[name] = int(getattr(info, name))
    for name in ("mesh_pad_rel", "mesh_pad_min", "scene_extent", "tlas_pad_rel", "tlas_pad_abs"):
        out[name] = np.float32(getattr(info, name))
    return out, 0


# Backend.denoise_svgf_torch's defaults: the best setting of profiles/svgf/quality.json (the sweep of profiles/svgf/quality.py)
SVGF_ITERATIONS = 1
SVGF_SIGMA_COLOR = 2.0


# Backend.temporal_torch's defaults: the best setting of profiles/temporal/quality.json (the sweep of profiles/temporal/quality.py)
TEMPORAL_MAX_HISTORY = 64
TEMPORAL_DEPTH_TOL = 0.2
TEMPORAL_NORMAL_MIN = 0.5
# Backend.svgf_spatial_variance_torch's defaults: the best setting of profiles/svgf_spatial/quality.json (the sweep of profiles/svgf_spatial/quality.py)
SVGF_SPATIAL_RADIUS = 1
SVGF_SPATIAL_MIN_HISTORY = 8.0
SVGF_SPATIAL_SIGMA_DEPTH = 0.0
# Backend.render_adaptive's and adaptive_estimate_torch's defaults: the best setting of profiles/adaptive/quality.json (the sweep of profiles/adaptive/quality.py)
ADAPTIVE_THRESHOLD = 0.1
ADAPTIVE_LUM_FLOOR = 1.0
ADAPTIVE_MIN_COLOURS = 16


class HitCpp(C.Structure):
    _fields_ = [("primIndex", C.c_int32), ("geomIndex", C.c_int32), ("instIndex", C.c_int32), ("t", C.c_float),
                ("normal", C.c_float * 3), ("texCoord", C.c_float * 2)]


EXPORTED_SYMBOLS = [
    "art_init", "art_init_devices", "art_device_count", "art_reduce", "art_get_reduce_info", "art_set_stream", "art_upload_scene", "art_resize", "art_set_shard", "art_render_pass",
    "art_debug_hit_pass", "art_bind_accum", "art_bind_moments", "art_accum_device", "art_download", "art_synchronize", "art_trace_rays",
    "art_trace_rays_device", "art_occluded_rays_device", "art_aovs_rays_device", "art_camera_rays_device", "art_render_aovs_device", "art_render_aovs_motion_device", "art_denoise_device", "art_denoise_svgf_device", "art_denoise_svgf_var_device", "art_temporal_device", "art_temporal_motion_device", "art_temporal_history_bytes", "art_svgf_spatial_variance_device", "art_set_camera",
    "art_exposure_state_bytes", "art_auto_exposure_device", "art_display_device", "art_upsample_device", "art_temporal_upsample_device", "art_firefly_device", "art_bloom_device",
    "art_compact_mask_device", "art_render_pass_masked", "art_adaptive_estimate_device", "art_radiance_rays_device",
    "art_refit_device", "art_get_refit_info",
    "art_rebuild_device", "art_get_rebuild_info", "art_get_tree_cost", "art_move_instances_device", "art_get_move_info",
    "art_refit_mesh_device", "art_get_mesh_refit_info",
    "art_rebuild_instance_tree_device", "art_get_instance_rebuild_info", "art_get_instance_tree_cost",
    "art_rebuild_mesh_tree_device", "art_get_mesh_rebuild_info", "art_get_mesh_tree_cost",
    "art_export_bvh", "art_export_two_level", "art_get_stats", "art_get_stage_stats", "art_get_camera_rays_traced", "art_set_option", "art_last_error", "art_shutdown",
    "gcore_init_and_clear", "gcore_destroy", "gcore_add_mesh_3f", "gcore_instance_meshes", "gcore_commit_scene",
    "gcore_closest_hit", "gcore_closest_hit_n", "gcore_set_two_level", "gcore_set_single_ray_on_gpu",
]


def build_library(force=False):
    """hipcc cross-compiles libart_hip.so for gfx950 (works without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", PKG_DIR, "clean"])
    subprocess.check_call(["make", "-s", "-j4", "-C", PKG_DIR])
    return LIB_PATH


_lib = None


def load_library():
    """dlopen the in-tree libart_hip.so.  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ArtError("libart_hip.so is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); there is no fallback path")
    L = C.CDLL(LIB_PATH)
    L.art_last_error.restype = C.c_char_p
    L.art_accum_device.restype = C.c_void_p
    L.art_set_stream.argtypes = [C.c_void_p]
    L.art_init_devices.argtypes = [C.c_int32, i32p]
    L.art_upload_scene.argtypes = [C.POINTER(ArtSceneDesc)]
    L.art_resize.argtypes = [C.c_int32, C.c_int32]
    L.art_set_shard.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.art_render_pass.argtypes = [C.POINTER(ArtPassParams), f32p, u32p, i32p]
    L.art_debug_hit_pass.argtypes = [C.POINTER(ArtPassParams), f32p, u32p, i32p, i32p, i32p]
    L.art_bind_accum.argtypes = [C.c_void_p]
    L.art_bind_moments.argtypes = [C.c_void_p]
    L.art_download.argtypes = [f32p, u32p, C.c_int32, C.c_int32]
    L.art_trace_rays.argtypes = [f32p, f32p, f32p, C.c_int64, C.POINTER(ArtHit), C.c_int32, C.POINTER(ArtStats)]
    L.art_trace_rays_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    L.art_occluded_rays_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.art_render_aovs_device.argtypes = [C.POINTER(ArtPassParams), C.POINTER(ArtAovBuffers), C.c_void_p]
    L.art_aovs_rays_device.argtypes = [C.POINTER(aov_rays.ArtAovRaysParams)] + [C.c_void_p] * 4 + [C.c_int64, C.POINTER(aov_rays.ArtAovRayBuffers), C.c_void_p]
    L.art_camera_rays_device.argtypes = [C.POINTER(ArtPassParams), C.c_void_p, C.c_void_p, C.c_void_p]
    L.art_render_aovs_motion_device.argtypes = [C.POINTER(ArtPassParams), C.POINTER(ArtAovBuffers), C.POINTER(ArtMotionSource), C.c_void_p, C.c_void_p]
    L.art_denoise_device.argtypes = [C.POINTER(ArtDenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.art_denoise_svgf_device.argtypes = [C.POINTER(ArtSvgfParams)] + [C.c_void_p] * 8
    L.art_set_camera.argtypes = [C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 16)]
    L.art_denoise_svgf_var_device.argtypes = [C.POINTER(ArtSvgfParams)] + [C.c_void_p] * 8
    L.art_temporal_device.argtypes = [C.POINTER(ArtTemporalParams)] + [C.c_void_p] * 11
    L.art_temporal_motion_device.argtypes = [C.POINTER(ArtTemporalParams)] + [C.c_void_p] * 12
    L.art_svgf_spatial_variance_device.argtypes = [C.POINTER(ArtSvgfSpatialParams)] + [C.c_void_p] * 4
    L.art_exposure_state_bytes.argtypes = []
    L.art_exposure_state_bytes.restype = C.c_int64
    L.art_auto_exposure_device.argtypes = [C.POINTER(display.ArtExposureParams)] + [C.c_void_p] * 3
    L.art_display_device.argtypes = [C.POINTER(display.ArtDisplayParams)] + [C.c_void_p] * 5
    L.art_upsample_device.argtypes = [C.POINTER(upsample.ArtUpsampleParams), C.c_void_p, C.POINTER(upsample.ArtUpsampleGuides), C.POINTER(upsample.ArtUpsampleGuides),
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    L.art_firefly_device.argtypes = [C.POINTER(firefly.ArtFireflyParams)] + [C.c_void_p] * 7
    L.art_bloom_device.argtypes = [C.POINTER(bloom.ArtBloomParams)] + [C.c_void_p] * 5
    L.art_temporal_upsample_device.argtypes = [C.POINTER(temporal_upsample.params_struct()), C.c_void_p, C.c_void_p, C.POINTER(temporal_upsample.ArtTemporalUpsampleGuides),
                                               C.POINTER(temporal_upsample.ArtTemporalUpsampleGuides)] + [C.c_void_p] * 7
    L.art_temporal_history_bytes.argtypes = [C.c_int32, C.c_int32]
    L.art_temporal_history_bytes.restype = C.c_int64
    L.art_compact_mask_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.art_render_pass_masked.argtypes = [C.POINTER(ArtPassParams), C.c_void_p, C.c_void_p, i32p, C.POINTER(C.c_int64)]
    L.art_adaptive_estimate_device.argtypes = [C.POINTER(ArtAdaptiveParams)] + [C.c_void_p] * 8
    L.art_radiance_rays_device.argtypes = [C.POINTER(radiance.ArtRadianceParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.art_refit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.art_get_refit_info.argtypes = [C.POINTER(ArtRefitInfo)]
    L.art_rebuild_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.art_get_rebuild_info.argtypes = [C.POINTER(ArtRebuildInfo)]
    L.art_get_tree_cost.argtypes = [C.POINTER(ArtTreeCost)]
    L.art_move_instances_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.art_get_move_info.argtypes = [C.POINTER(ArtMoveInfo)]
    L.art_refit_mesh_device.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.art_get_mesh_refit_info.argtypes = [C.POINTER(ArtMeshRefitInfo)]
    L.art_rebuild_instance_tree_device.argtypes = [C.c_void_p]
    L.art_get_instance_rebuild_info.argtypes = [C.POINTER(ArtInstanceRebuildInfo)]
    L.art_get_instance_tree_cost.argtypes = [C.POINTER(ArtTreeCost)]
    L.art_rebuild_mesh_tree_device.argtypes = [C.c_int32, C.c_void_p]
    L.art_get_mesh_rebuild_info.argtypes = [C.POINTER(ArtMeshRebuildInfo)]
    L.art_get_mesh_tree_cost.argtypes = [C.c_int32, C.POINTER(ArtTreeCost)]
    L.art_export_bvh.argtypes = [f32p, C.c_int64, f32p, C.c_int64, C.POINTER(ArtBvhInfo)]
    L.art_export_two_level.argtypes = [C.POINTER(ArtTwoLevelInfo), C.POINTER(ArtTwoLevelBuffers)]
    L.art_get_stats.argtypes = [C.POINTER(ArtStats)]
    L.art_get_reduce_info.argtypes = [C.POINTER(ArtReduceInfo)]
    L.art_get_stage_stats.argtypes = [C.POINTER(ArtStageStats)]
    L.art_get_camera_rays_traced.argtypes = [C.POINTER(C.c_uint64)]
    L.art_set_option.argtypes = [C.c_char_p, C.c_int64]
    L.gcore_add_mesh_3f.argtypes = [f32p, C.c_int, i32p, C.c_int]
    L.gcore_add_mesh_3f.restype = C.c_int
    L.gcore_instance_meshes.argtypes = [C.c_int, f32p, C.c_int]
    L.gcore_closest_hit.argtypes = [f32p, f32p, C.c_float, C.c_float, C.POINTER(HitCpp)]
    L.gcore_closest_hit.restype = C.c_bool
    L.gcore_closest_hit_n.argtypes = [C.c_int, f32p, f32p, f32p, f32p, C.POINTER(HitCpp), C.POINTER(C.c_ubyte)]
    L.gcore_closest_hit_n.restype = C.c_int
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise ArtError(load_library().art_last_error().decode())


def _fp(a):
    return None if a is None else a.ctypes.data_as(f32p)


def _ip(a):
    return None if a is None else a.ctypes.data_as(i32p)


def _up(a):
    return None if a is None else a.ctypes.data_as(u32p)


RayHits = collections.namedtuple("RayHits", "t is_hit prim_type prim_index mat_id mat normal uv raw")
RayHits.__doc__ = """Backend.trace_rays_torch: views of ONE [N, 11] int32 tensor (`raw`) whose bytes are the ArtHit array.
t, normal [N, 3], uv [N, 2]: float32; is_hit, prim_type, prim_index, mat_id, mat: int32."""

HIP_STREAM_LEGACY = 1      # hipStreamLegacy: torch's default stream is the null stream (handle 0), and NULL means the library's stream to the C ABI


def _ptr(x):
    return None if x is None else x.data_ptr()


def _stream(torch, device):
    """torch's current stream of `device`: what the torch-facing calls enqueue on, without waiting for it"""
    return torch.cuda.current_stream(device)


def _handle(stream):
    """a torch.cuda.Stream as the C ABI takes it"""
    return stream.cuda_stream or HIP_STREAM_LEGACY


# One argument of a torch-facing call: label is what a refusal opens with ("denoise_torch: albedo"), dtype the name of a torch dtype
# (None: any), rule an exact shape, a least number of elements, or (predicate, sentence) where the sentence's {} is the shape as it
# came (None: any shape); an optional plane may be None.
_Plane = collections.namedtuple("_Plane", "label x dtype rule optional", defaults=(None, None, False))


def _expected(*shape):
    """the exact shape in the words of the older wrappers (the ray queries, the vertex updates)"""
    return (lambda x: tuple(x.shape) == shape, "shape {}, expected %s" % (shape,))


def _check_planes(torch, planes, contiguous="refuse", kind="", tail=""):
    """THE check of what a plane is -- a torch tensor, its dtype, its shape, its layout, in that order, plane after plane -- for
    every torch-facing call.  contiguous: "refuse" a strided tensor (`tail` ends that sentence), "make" it contiguous as the older
    wrappers do, or None (not looked at).  kind: what else the argument may be, ahead of "a torch tensor is required".  Where a
    plane is (_check_devices) is not looked at.  Returns the tensors, None for an absent optional plane."""
    checked = []
    for p in planes:
        x, rule = p.x, p.rule
        if x is None and p.optional:
            checked.append(None)
            continue
        if torch is None or not isinstance(x, torch.Tensor):
            raise ArtError("%s: %sa torch tensor is required, not %s" % (p.label, kind, type(x).__name__))
        if p.dtype is not None and x.dtype != getattr(torch, p.dtype):
            raise ArtError("%s: dtype must be %s, not %s" % (p.label, getattr(torch, p.dtype), x.dtype))
        if isinstance(rule, int):
            rule = (lambda x, n=rule: x.numel() >= n, "the tensor holds {numel} elements, the frame needs %d" % rule)
        elif rule is not None and not callable(rule[0]):
            rule = (lambda x, shape=tuple(rule): tuple(x.shape) == shape, "shape must be %s, not {}" % list(rule))
        if rule is not None and not rule[0](x):
            raise ArtError("%s: %s" % (p.label, rule[1].format(tuple(x.shape), numel=x.numel())))
        if contiguous == "make":
            x = x.contiguous()
        elif contiguous == "refuse" and not x.is_contiguous():
            raise ArtError("%s: the tensor must be contiguous%s" % (p.label, tail))
        checked.append(x)
    return checked


def _check_devices(planes, device=None, where=" on the library's device"):
    """THE check of where the planes are: every one that is there on a GPU, and on `device` where one is given (the device of the
    call's first tensor, which names it; `where` stands in while that is not a GPU, or with no device given)."""
    for p in planes:
        if p.x is not None and (p.x.device.type != "cuda" or (device is not None and p.x.device != device)):
            raise ArtError("%s: must be a GPU tensor%s, not on %s"
                           % (p.label, " on %s" % device if device is not None and device.type == "cuda" else where, p.x.device))


def _frame_plane(torch, label, x, dtype, rule, optional=False, kind="", tail=""):
    """A plane the library reads or writes from its first element on (bind_accum, bind_moments, the adaptive calls), in the order of
    refusals those calls have: what it is, where it is, dtype and layout, its size last.  Returns its device address (None for an
    absent optional plane)."""
    if x is None and optional:
        return None
    _check_planes(torch, [_Plane(label, x)], None, kind)
    _check_devices([_Plane(label, x)])
    _check_planes(torch, [_Plane(label, x, dtype)], tail=tail)
    _check_planes(torch, [_Plane(label, x, dtype, rule)])
    return x.data_ptr()


def _colour_frame(torch, call, color):
    """color is what names the frame of the image-space calls: a tensor shaped [H, W, 3], ahead of every other check -> (H, W)"""
    _check_planes(torch, [_Plane(call + ": color", color, None, (lambda x: x.dim() == 3 and x.shape[2] == 3 and x.numel() != 0,
                                                                  "shape must be [H, W, 3], not {}"))], None)
    return int(color.shape[0]), int(color.shape[1])


def _image_plane(call, h, w, name, x, per, dtype="float32", optional=True):
    """a plane of an H x W frame with `per` words per pixel; per = 2 is the moments, which may be flat and longer (bind_moments' tensor)"""
    rule = (h, w, 3) if per == 3 else (h, w)
    if per == 2:
        rule = (lambda x: x.numel() >= 2 * h * w, "shape must hold at least %d elements ([H, W, 2]), not {}" % (2 * h * w))
    return _Plane("%s: %s" % (call, name), x, dtype, rule, optional)


def _only_aov_planes(call, keywords):
    """the dict of render_aovs_torch may be given whole as keyword arguments: what a filter does not read of it is ignored"""
    for name in keywords:
        if name not in AOV_PLANES:
            raise TypeError("%s: unexpected keyword argument %r" % (call, name))


def _known_planes(call, want):
    want = tuple(want)
    for name in want:
        if name not in AOV_PLANES:
            raise ValueError("%s: unknown plane %r (known: %s)" % (call, name, ", ".join(AOV_PLANES)))
    return want


class SceneDesc:
    """Flattened scene held in numpy arrays (keeps them alive) + the ArtSceneDesc view of them."""

    def __init__(self, spheres=(), lights=(), materials=(), meshes=(), cornell=None,
                 cam_pos=(0.0, 2.55, 12.5), cam_matrix=None, instances=()):
        """instances: [(mesh index, 12 floats: object -> world 3x4 row-major)] -- then `meshes` are object-space prototypes (ArtSceneDesc::n_instances)"""
        self._kw = dict(spheres=spheres, lights=lights, materials=materials, cornell=cornell, cam_pos=cam_pos, cam_matrix=cam_matrix)      # (for flattened_copy)
        self.spheres = (ArtSphere * max(1, len(spheres)))()
        for i, (pos, r, mat) in enumerate(spheres):
            self.spheres[i].pos = (C.c_float * 3)(*pos); self.spheres[i].r = r; self.spheres[i].mat = mat
        self.lights = (ArtLight * max(1, len(lights)))()
        for i, l in enumerate(lights):
            L = self.lights[i]
            L.shape = l["shape"]; L.mat = l["mat"]
            for k in ("boxMin", "boxMax", "normal", "center", "intensity"):
                setattr(L, k, (C.c_float * 3)(*l.get(k, (0.0, 0.0, 0.0))))
            L.radius = l.get("radius", 0.0); L.surfaceArea = l["surfaceArea"]
        self.materials = (ArtMaterial * max(1, len(materials)))()
        for i, m in enumerate(materials):
            M = self.materials[i]
            M.type = m["type"]; M.light = m.get("light", 0)
            p = list(m.get("p", ())) + [0.0] * 8
            M.p = (C.c_float * 8)(*p[:8])
        self._mesh_arrays = []
        self.meshes = (ArtMesh * max(1, len(meshes)))()
        for i, m in enumerate(meshes):
            pos = np.ascontiguousarray(m["pos"], np.float32).reshape(-1, 3)
            nrm = np.ascontiguousarray(m["nrm"], np.float32).reshape(-1, 3)
            idx = np.ascontiguousarray(m["idx"], np.int32).reshape(-1, 3)
            uv = np.ascontiguousarray(m.get("uv", np.zeros((pos.shape[0], 2))), np.float32).reshape(-1, 2)
            matid = np.ascontiguousarray(m.get("matid", np.zeros(idx.shape[0])), np.int32)
            self._mesh_arrays.append((pos, nrm, idx, uv, matid))
            M = self.meshes[i]
            M.mode = m["mode"]; M.nverts = pos.shape[0]; M.ntris = idx.shape[0]
            M.pos = _fp(pos); M.nrm = _fp(nrm); M.uv = _fp(uv); M.idx = _ip(idx); M.matid = _ip(matid)
            bbmin = m.get("bbmin", pos.min(0)); bbmax = m.get("bbmax", pos.max(0))
            M.bbmin = (C.c_float * 3)(*[float(v) for v in bbmin]); M.bbmax = (C.c_float * 3)(*[float(v) for v in bbmax])
        d = ArtSceneDesc()
        d.n_spheres = len(spheres); d.spheres = self.spheres
        d.n_lights = len(lights); d.lights = self.lights
        d.n_materials = len(materials); d.materials = self.materials
        d.n_meshes = len(meshes); d.meshes = self.meshes
        if cornell is not None:
            d.has_cornell = 1
            d.cb_min = (C.c_float * 3)(*cornell["min"]); d.cb_max = (C.c_float * 3)(*cornell["max"])
            d.cb_mat = (C.c_int32 * 6)(*cornell["mat"])
            for k in range(6):
                d.cb_nrm[k] = (C.c_float * 3)(*cornell["nrm"][k])
        d.cam_pos = (C.c_float * 3)(*cam_pos)
        cm = np.eye(4, dtype=np.float32).ravel() if cam_matrix is None else np.asarray(cam_matrix, np.float32).ravel()
        d.cam_matrix = (C.c_float * 16)(*[float(v) for v in cm])
        self.instances = (ArtInstance * max(1, len(instances)))()
        for i, (mesh, m) in enumerate(instances):
            self.instances[i].mesh = int(mesh); self.instances[i].m = (C.c_float * 12)(*[float(v) for v in np.asarray(m, np.float32).ravel()[:12]])
        d.n_instances = len(instances); d.instances = self.instances
        self.desc = d


class Backend(radiance.RadianceQueries, display.DisplayCalls, aov_rays.AovRayCalls, upsample.UpsampleCalls, temporal_upsample.TemporalUpsampleCalls, firefly.FireflyCalls, bloom.BloomCalls):
    """One process-wide backend instance (the C library is a singleton, like g_data / ray_tracer.ads globals)."""

    def __init__(self, device=-1, devices=None):
        """device: one GPU (art_init).  devices: a list of ordinals, or a count n for 0..n-1 -> one process drives them all
        (art_init_devices): pixel tiles sharded inside the library, RCCL reduce to the first device."""
        self.lib = load_library()
        if devices is None:
            _check(self.lib.art_init(device))
        elif isinstance(devices, int):
            _check(self.lib.art_init_devices(devices, None))
        else:
            arr = (C.c_int32 * len(devices))(*devices)
            _check(self.lib.art_init_devices(len(devices), arr))
        self._accum_tensor = None                     # the tensor bind_accum holds while it is bound
        self._moments_tensor = None                   # the same for bind_moments

    def reduce(self):
        _check(self.lib.art_reduce())

    def set_stream(self, hip_stream):
        _check(self.lib.art_set_stream(hip_stream))

    def set_option(self, name, value):
        _check(self.lib.art_set_option(name.encode(), int(value)))

    def upload_scene(self, scene):
        desc = getattr(scene, "desc", scene)          # SceneDesc / scenes.HostSceneDesc, or a raw ArtSceneDesc
        _check(self.lib.art_upload_scene(C.byref(desc)))

    def resize(self, width, height):
        t = self._accum_tensor
        if t is not None and t.numel() < 3 * width * height:
            raise ArtError("resize: the bound accum tensor holds %d elements, a %d x %d frame needs %d" % (t.numel(), width, height, 3 * width * height))
        m = getattr(self, "_moments_tensor", None)
        if m is not None and m.numel() < 2 * width * height:
            raise ArtError("resize: the bound moments tensor holds %d elements, a %d x %d frame needs %d" % (m.numel(), width, height, 2 * width * height))
        self.width, self.height = width, height
        _check(self.lib.art_resize(width, height))

    def set_shard(self, rank, nranks, tile=32):
        _check(self.lib.art_set_shard(rank, nranks, tile))

    @staticmethod
    def pass_params(render_type=PT_MIS, aa_on=True, max_depth=8, vthreads=1, seed=1, background=(0.0, 0.0, 0.0),
                    layout=LAYOUT_ROW_MAJOR):
        p = ArtPassParams()
        p.render_type, p.aa_on, p.max_depth, p.vthreads = render_type, int(aa_on), max_depth, vthreads
        p.background = (C.c_float * 3)(*background); p.seed = seed; p.layout = layout
        return p

    def _frame_shape(self, layout):
        return (self.height, self.width) if layout == LAYOUT_ROW_MAJOR else (self.width, self.height)

    def _get(self, entry, struct, *first):
        """a struct the library fills in: art_get_...(first..., &struct)"""
        x = struct()
        _check(getattr(self.lib, entry)(*first, C.byref(x)))
        return x

    def _need_device(self):
        _check(self.lib.art_trace_rays_device(None, None, None, None, 0, None, TRACE_COOP, None))     # n = 0: "is there a device?"

    def render_pass(self, params, spp, want_accum=True, want_screen=False):
        """Returns (accum or None, screen or None, new spp).  Arrays are [H,W,..] for ROW_MAJOR, [W,H,..] for ADA_XY."""
        shape = self._frame_shape(params.layout)
        accum = np.zeros(shape + (3,), np.float32) if want_accum else None
        screen = np.zeros(shape, np.uint32) if want_screen else None
        s = C.c_int32(spp)
        _check(self.lib.art_render_pass(C.byref(params), _fp(accum), _up(screen), C.byref(s)))
        return accum, screen, s.value

    def render_pass_device(self, params, spp):
        s = C.c_int32(spp)
        _check(self.lib.art_render_pass(C.byref(params), None, None, C.byref(s)))
        return s.value

    def debug_hit_pass(self, params):
        shape = self._frame_shape(params.layout)
        accum = np.zeros(shape + (3,), np.float32); screen = np.zeros(shape, np.uint32)
        prim = np.zeros(shape, np.int32); mat = np.zeros(shape, np.int32); ptype = np.zeros(shape, np.int32)
        _check(self.lib.art_debug_hit_pass(C.byref(params), _fp(accum), _up(screen), _ip(prim), _ip(mat), _ip(ptype)))
        return accum, screen, prim, mat, ptype

    def download(self, spp, layout=LAYOUT_ROW_MAJOR, want_screen=True):
        shape = self._frame_shape(layout)
        accum = np.zeros(shape + (3,), np.float32)
        screen = np.zeros(shape, np.uint32) if want_screen else None
        _check(self.lib.art_download(_fp(accum), _up(screen), layout, spp))
        return accum, screen

    def bind_accum(self, accum):
        """Render into caller-owned device memory (art_bind_accum; the contract is in include/art_hip.h): row-major float3, zeroed by the
        next resize, added to by every pass.  accum: None (back to the library's buffer), an integer device address (the caller keeps
        the memory alive and large enough), or a contiguous float32 torch tensor on the library's GPU.  A tensor is checked before any
        C call, held here until the next bind_accum so that it cannot be collected while bound, and resize() refuses a frame it is
        too small for."""
        self._bind("accum", accum, 3)

    def bind_moments(self, moments):
        """Let the render passes keep the luminance moments {S1, S2} of every pixel in caller-owned device memory (art_bind_moments; the
        contract is in include/art_hip.h): row-major float2, zeroed by the next resize, added to by every pass.  moments: None (no
        moments, the default), an integer device address, or a contiguous float32 torch tensor on the library's GPU with at least
        2 * W * H elements for the frame the next resize() sets.  Checked before any C call, held until the next bind_moments and
        guarded by resize(), which refuses a frame the tensor is too small for, exactly as bind_accum's tensor."""
        self._bind("moments", moments, 2)

    def _bind(self, what, x, per):
        """bind_accum / bind_moments: art_bind_<what>(x), holding the tensor x came as in _<what>_tensor"""
        held = None
        if x is not None and not isinstance(x, int):
            held = x
            x = _frame_plane(sys.modules.get("torch"), "bind_" + what, x, "float32", (lambda t: t.numel() != 0, "the tensor is empty"),
                             kind="None, an integer device address or ",
                             tail=" (the library writes row-major float%d from its first element on)" % per)
        _check(getattr(self.lib, "art_bind_" + what)(x))       # (a refused pointer keeps the previous binding, and the tensor held for it)
        setattr(self, "_%s_tensor" % what, held)

    def synchronize(self):
        _check(self.lib.art_synchronize())

    def stage_stats(self):
        """the wavefront stages around the trace kernel: GPU ms per kind of kernel, items read / kept per bounce (device 0, cumulative)"""
        return self._get("art_get_stage_stats", ArtStageStats)

    def camera_rays_traced(self):
        """camera rays the render passes generated and traced since resize(): with option camera_dedup (default) each distinct ray of a
        batch once, else one per sample; stats().rays counts one camera query per sample either way"""
        n = C.c_uint64(0)
        _check(self.lib.art_get_camera_rays_traced(C.byref(n)))
        return n.value

    def reduce_info(self):
        """what the multi-device path did: ranks of the RCCL communicator, GPU time of the reduces, GPU time of every device's passes"""
        return self._get("art_get_reduce_info", ArtReduceInfo)

    def trace_rays(self, origins, dirs, tfar=None, kernel=TRACE_COOP, want_stats=False):
        o = np.ascontiguousarray(origins, np.float32); d = np.ascontiguousarray(dirs, np.float32)
        n = o.shape[0]
        out = (ArtHit * n)()
        st = ArtStats()
        tf = None if tfar is None else np.ascontiguousarray(tfar, np.float32)
        _check(self.lib.art_trace_rays(_fp(o), _fp(d), _fp(tf), n, out, kernel, C.byref(st) if want_stats else None))
        return (out, st) if want_stats else out

    def _query(self, origins, dirs, tnear, tfar):
        """Validated, contiguous inputs of a device query, and the HIP stream it runs on (torch's current stream of their device):
        float32, [N, 3] rays, [N] intervals."""
        import torch
        if not isinstance(origins, torch.Tensor) or origins.dim() != 2:
            raise ArtError("origins: a [N, 3] float32 tensor is required")
        n = origins.shape[0]
        planes = [_Plane("origins", origins, "float32", _expected(n, 3)), _Plane("dirs", dirs, "float32", _expected(n, 3)),
                  _Plane("tnear", tnear, "float32", _expected(n), True), _Plane("tfar", tfar, "float32", _expected(n), True)]
        o, d, tn, tf = _check_planes(torch, planes, "make")
        self._need_device()
        _check_devices(planes, o.device)
        return torch, o, d, tn, tf, n, _handle(_stream(torch, o.device))

    def trace_rays_torch(self, origins, dirs, tnear=None, tfar=None, kernel=TRACE_COOP):
        """Closest hit of N rays held in torch tensors on the GPU (origins, dirs [N, 3] float32; tnear, tfar [N] or None), enqueued on
        torch.cuda.current_stream() without waiting for it.  Returns RayHits on the same device (art_trace_rays_device)."""
        torch, o, d, tn, tf, n, stream = self._query(origins, dirs, tnear, tfar)
        raw = torch.empty((n, 11), dtype=torch.int32, device=o.device)
        _check(self.lib.art_trace_rays_device(_ptr(o), _ptr(d), _ptr(tn), _ptr(tf), n, raw.data_ptr() if n else None, kernel, stream))
        f = raw.view(torch.float32)
        return RayHits(f[:, 0], raw[:, 1], raw[:, 2], raw[:, 3], raw[:, 4], raw[:, 5], f[:, 6:9], f[:, 9:11], raw)

    def occluded_torch(self, origins, dirs, tnear=None, tfar=None):
        """Occlusion of N rays held in torch tensors on the GPU: a bool [N] tensor, equal to trace_rays_torch(...).is_hit != 0 on the same
        rays and intervals (art_occluded_rays_device)."""
        torch, o, d, tn, tf, n, stream = self._query(origins, dirs, tnear, tfar)
        out = torch.empty((n,), dtype=torch.bool, device=o.device)
        _check(self.lib.art_occluded_rays_device(_ptr(o), _ptr(d), _ptr(tn), _ptr(tf), n, out.data_ptr() if n else None, stream))
        return out

    def _aov_outputs(self, torch, want, motion=False):
        """The planes of `want` for the frame of resize(), and "motion" if asked, allocated by torch on its current device: (dict,
        the ArtAovBuffers that points at the planes of `want`, the device)"""
        self._need_device()
        dev = torch.device("cuda", torch.cuda.current_device())
        h, w = getattr(self, "height", 0), getattr(self, "width", 0)
        out, buf = {}, ArtAovBuffers()
        for name in want:
            field, per, integer = AOV_PLANES[name]
            out[name] = torch.empty((h, w, 3) if per == 3 else (h, w), dtype=torch.int32 if integer else torch.float32, device=dev)
            setattr(buf, field, out[name].data_ptr() or None)
        if motion:
            out["motion"] = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        return out, buf, dev

    def render_aovs_torch(self, params, want=tuple(AOV_PLANES)):
        """First-hit feature buffers of the frame (art_render_aovs_device): a dict of torch tensors on the library's GPU, one per name in
        `want` -- albedo, normal [H, W, 3] float32; depth, alpha [H, W] float32; prim_type, prim_index, mat [H, W] int32 -- allocated by
        torch and enqueued on torch.cuda.current_stream() without waiting for it.  Of `params` only aa_on and background are read: with
        aa_on a float plane is the mean of the pixel's four camera rays, the ids are those of ray 0.  An unknown name raises ValueError
        before any call."""
        want = _known_planes("render_aovs_torch", want)
        import torch
        out, buf, dev = self._aov_outputs(torch, want)
        _check(self.lib.art_render_aovs_device(C.byref(params), C.byref(buf), _handle(_stream(torch, dev))))
        return out

    def render_aovs_torch_motion(self, params, want=tuple(AOV_PLANES), cur_pos=None, prev_pos=None, prev_matrices=None):
        """render_aovs_torch plus the motion plane (art_render_aovs_motion_device; include/art_hip.h states the arithmetic): the same
        dict with "motion", float32 [H, W, 3] -- where each pixel's surface point was one update ago minus where it is -- from one
        trace of the camera rays.  Flat scene: cur_pos = the vertices in force (what refit_torch was last given), prev_pos = those one
        update earlier, float32 [nverts, 3] GPU tensors, both or neither.  Instanced scene: prev_matrices = the matrices one update
        earlier, float32 [n_instances, 12] (or [n, 3, 4]).  All None: the plane is zero.  `want` may be empty.  Every tensor is checked
        before any C call; what the library refuses (a wrong count, arrays of the other kind of scene) raises ArtError."""
        call = "render_aovs_torch_motion"
        want = _known_planes(call, want)
        import torch
        src = ArtMotionSource()
        for name, x, last in (("cur_pos", cur_pos, 3), ("prev_pos", prev_pos, 3), ("prev_matrices", prev_matrices, 12)):
            rows = (lambda x, last=last: x.dim() >= 2 and x.numel() != 0 and x.numel() == x.shape[0] * last, "shape must be [n, %d], not {}" % last)
            plane = [_Plane("%s: %s" % (call, name), x, "float32", rows, True)]
            _check_planes(torch, plane)                     # (plane after plane: all of one before any of the next)
            _check_devices(plane, where="")
        if (cur_pos is None) != (prev_pos is None):
            raise ArtError("render_aovs_torch_motion: cur_pos and prev_pos must both be given or both be None")
        if cur_pos is not None:
            if cur_pos.shape[0] != prev_pos.shape[0]:
                raise ArtError("render_aovs_torch_motion: cur_pos and prev_pos differ in length")
            src.cur_pos3f, src.prev_pos3f, src.nverts = cur_pos.data_ptr(), prev_pos.data_ptr(), int(cur_pos.shape[0])
        if prev_matrices is not None:
            src.prev_m12f, src.n_instances = prev_matrices.data_ptr(), int(prev_matrices.shape[0])
        out, buf, dev = self._aov_outputs(torch, want, motion=True)
        _check(self.lib.art_render_aovs_motion_device(C.byref(params), C.byref(buf), C.byref(src), out["motion"].data_ptr() or None,
                                                      _handle(_stream(torch, dev))))
        return out

    def denoise_torch(self, color, albedo=None, normal=None, depth=None, iterations=5, scale=1.0, sigma_color=4.0, sigma_depth=1.0,
                      normal_log2=7, demodulate=True, out=None, variant=0, **other_planes):
        """Edge-avoiding a-trous filter of `color` guided by the feature buffers (art_denoise_device; include/art_hip.h states the
        arithmetic).  color, albedo, normal: float32 [H, W, 3]; depth: float32 [H, W]; all contiguous and on one GPU, the library's; a
        guide that is None is not used.  Returns `out`, float32 [H, W, 3] on the same device (torch.empty when None; `out is color`
        filters in place).  Enqueued on torch.cuda.current_stream() without waiting for it.  Every tensor is checked before any C
        call.  A tensor bound with bind_accum is accepted as it is (scale = 1 / spp), and so is the dict of render_aovs_torch as
        keyword arguments: its planes that the filter does not read (alpha, prim_type, prim_index, mat) are ignored.  The defaults
        of iterations, the sigmas and normal_log2 are starting values taken from the literature (Dammertz et al. 2010, SVGF), not
        tuned on this renderer."""
        call = "denoise_torch"
        _only_aov_planes(call, other_planes)
        torch = sys.modules.get("torch")
        h, w = _colour_frame(torch, call, color)
        for name, x, per in (("color", color, 3), ("albedo", albedo, 3), ("normal", normal, 3), ("depth", depth, 1), ("out", out, 3)):
            plane = [_image_plane(call, h, w, name, x, per)]
            _check_planes(torch, plane)                     # (plane after plane: all of one before any of the next)
            _check_devices(plane, color.device)
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.float32, device=color.device)
        p = ArtDenoiseParams(w, h, int(iterations), 1 if demodulate else 0, int(normal_log2), int(variant), float(scale), float(sigma_color), float(sigma_depth))
        _check(self.lib.art_denoise_device(C.byref(p), _ptr(color), _ptr(albedo), _ptr(normal), _ptr(depth), _ptr(out),
                                           _handle(_stream(torch, color.device))))
        return out

    def denoise_svgf_torch(self, color, moments=None, n_colours=0, albedo=None, normal=None, depth=None, iterations=SVGF_ITERATIONS, scale=1.0,
                           sigma_color=SVGF_SIGMA_COLOR, sigma_depth=1.0, normal_log2=7, demodulate=True, out=None, variance_out=None, variance=None, **other_planes):
        """The variance-guided variant of denoise_torch (art_denoise_svgf_device; include/art_hip.h states the arithmetic): the colour
        stop is measured in standard deviations of the pixel's own estimate, which come from `moments`, float32 with 2 * H * W
        elements ([H, W, 2] or flat: the tensor of bind_moments as it is) and `n_colours`, the colours behind them (spp / 4 with
        anti-aliasing, else spp).  color, the guides, out and the stream are denoise_torch's; variance_out: float32 [H, W] or None,
        receives the variance of the filtered luminance.  A tensor bound with bind_accum is accepted as it is when it is viewed as
        [H, W, 3], and so is the dict of render_aovs_torch as keyword arguments.  Every tensor is checked before any C call.  The
        defaults of iterations and sigma_color are the best setting of the sweep in profiles/svgf/quality.json.
        variance: float32 [H, W], given INSTEAD of moments and n_colours (art_denoise_svgf_var_device): the variance of each pixel's
        luminance estimate in the units of color before scale -- temporal_torch's second result, with scale = 1."""
        call = "denoise_svgf_torch"
        _only_aov_planes(call, other_planes)
        torch = sys.modules.get("torch")
        h, w = _colour_frame(torch, call, color)
        if variance is not None and (moments is not None or n_colours):
            raise ArtError("denoise_svgf_torch: give moments (with n_colours) or variance, not both")
        spread = ("variance", variance, 1) if variance is not None else ("moments", moments, 2)
        planes = [_image_plane(call, h, w, name, x, per, optional=name != "moments")
                  for name, x, per in (("color", color, 3), spread, ("albedo", albedo, 3), ("normal", normal, 3), ("depth", depth, 1), ("out", out, 3),
                                       ("variance_out", variance_out, 1))]
        _check_planes(torch, planes)
        _check_devices(planes, color.device)               # (the devices last: a wrong kind of argument is named before a wrong place)
        if variance is None and int(n_colours) < 2:
            raise ArtError("denoise_svgf_torch: n_colours must be at least 2 (a variance needs two colours), not %s" % (n_colours,))
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.float32, device=color.device)
        p = ArtSvgfParams(w, h, int(iterations), 1 if demodulate else 0, int(normal_log2), int(n_colours), float(scale), float(sigma_color), float(sigma_depth))
        entry = self.lib.art_denoise_svgf_device if variance is None else self.lib.art_denoise_svgf_var_device
        _check(entry(C.byref(p), _ptr(color), _ptr(spread[1]), _ptr(albedo), _ptr(normal), _ptr(depth), _ptr(out), _ptr(variance_out),
                     _handle(_stream(torch, color.device))))
        return out

    @staticmethod
    def temporal_camera(cam, width, height):
        """(cam_pos [3], cam_matrix [16] or [4, 4]) and the frame's size -> ArtTemporalCamera"""
        pos, mat = cam
        pos = [float(v) for v in np.asarray(pos, np.float32).reshape(-1)]
        mat = [float(v) for v in np.asarray(mat, np.float32).reshape(-1)]
        if len(pos) != 3 or len(mat) != 16:
            raise ArtError("temporal_torch: a camera is (cam_pos of 3 floats, cam_matrix of 16 floats, row-major)")
        return ArtTemporalCamera((C.c_float * 3)(*pos), (C.c_float * 16)(*mat), int(width), int(height))

    def temporal_torch(self, cur, history, cam_cur, cam_prev, n_colours, max_history=TEMPORAL_MAX_HISTORY, depth_tol=TEMPORAL_DEPTH_TOL,
                       normal_min=TEMPORAL_NORMAL_MIN, scale=1.0, id_plane="prim_index", motion=None):
        """Temporal reprojection and accumulation (art_temporal_device; include/art_hip.h states the arithmetic).  cur: a dict -- the one
        of render_aovs_torch plus "color" (float32 [H, W, 3]; the tensor of bind_accum viewed so is accepted as it is, scale = 1 / spp)
        and "moments" (float32 with 2 * H * W elements: the tensor of bind_moments as it is); of the guides "normal" [H, W, 3], "depth"
        [H, W] and cur[id_plane] (int32 [H, W]) are read where present, every other entry is ignored.  history: the fourth result of
        the previous call, or None for the first frame (cam_prev is then not read and may be None); its frame size is its own.
        cam_cur, cam_prev: (cam_pos, cam_matrix).  n_colours: the colours behind color and moments.  Returns (out [H, W, 3], variance
        [H, W], length [H, W], new_history [3, H, W, 4]), float32 tensors on color's device, enqueued on torch.cuda.current_stream()
        without waiting for it.  Every tensor is checked before any C call.  The defaults of max_history, depth_tol and normal_min are
        the best setting of the sweep in profiles/temporal/quality.json.
        motion: float32 [H, W, 3] or None -- the "motion" plane of render_aovs_torch_motion for this frame; given, the call is
        art_temporal_motion_device, which follows surfaces that moved (cur["motion"] is NOT read: the plane is named explicitly)."""
        call = "temporal_torch"
        torch = sys.modules.get("torch")
        if not isinstance(cur, dict):
            raise ArtError("temporal_torch: cur: a dict of planes is required, not %s" % type(cur).__name__)
        color = cur.get("color")
        h, w = _colour_frame(torch, call, color)
        moments, normal, depth, ids = [cur.get(name) if name else None for name in ("moments", "normal", "depth", id_plane)]
        whole = (lambda x: x.dim() == 4 and x.shape[0] == 3 and x.shape[3] == 4 and x.numel() != 0, "shape must be [3, H', W', 4], not {}")
        planes = [_image_plane(call, h, w, "color", color, 3), _image_plane(call, h, w, "moments", moments, 2, optional=False),
                  _image_plane(call, h, w, "normal", normal, 3), _image_plane(call, h, w, "depth", depth, 1),
                  _image_plane(call, h, w, id_plane, ids, 1, "int32"), _Plane(call + ": history", history, "float32", whole, True),
                  _image_plane(call, h, w, "motion", motion, 3)]
        _check_planes(torch, planes)
        if history is not None and cam_prev is None:
            raise ArtError("temporal_torch: cam_prev: a history needs the camera it was rendered with")
        for name, cam in (("cam_cur", cam_cur), ("cam_prev", cam_prev if history is not None else None)):
            if cam is not None and not (isinstance(cam, (tuple, list)) and len(cam) == 2):
                raise ArtError("temporal_torch: %s: a camera is (cam_pos, cam_matrix)" % name)
        if cam_cur is None:
            raise ArtError("temporal_torch: cam_cur: a camera is (cam_pos, cam_matrix)")
        dev = color.device
        _check_devices(planes, dev)                         # (after the cameras: what an argument is, is named before where it is)
        if int(n_colours) < 1:
            raise ArtError("temporal_torch: n_colours must be at least 1, not %s" % (n_colours,))
        p = ArtTemporalParams()
        p.cur = self.temporal_camera(cam_cur, w, h)
        if history is not None:
            p.prev = self.temporal_camera(cam_prev, int(history.shape[2]), int(history.shape[1]))
        p.n_colours, p.max_history = int(n_colours), int(max_history)
        p.scale, p.depth_tol, p.normal_min = float(scale), float(depth_tol), float(normal_min)
        out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        var = torch.empty((h, w), dtype=torch.float32, device=dev)
        length = torch.empty((h, w), dtype=torch.float32, device=dev)
        new = torch.empty((3, h, w, 4), dtype=torch.float32, device=dev)
        entry, moved = (self.lib.art_temporal_device, ()) if motion is None else (self.lib.art_temporal_motion_device, (_ptr(motion),))
        _check(entry(C.byref(p), _ptr(color), _ptr(moments), _ptr(normal), _ptr(depth), _ptr(ids), *moved, _ptr(history), _ptr(new), _ptr(out),
                     _ptr(var), _ptr(length), _handle(_stream(torch, dev))))
        return out, var, length, new

    def svgf_spatial_variance_torch(self, hist, variance, width, height, radius=SVGF_SPATIAL_RADIUS, min_history=SVGF_SPATIAL_MIN_HISTORY,
                                    sigma_depth=SVGF_SPATIAL_SIGMA_DEPTH, normal_log2=7, out=None):
        """SVGF's spatial variance estimate (art_svgf_spatial_variance_device; include/art_hip.h states the arithmetic): where a pixel's
        history is shorter than min_history colours, or its variance is not finite, the variance comes from the luminance moments pooled
        over the (2 * radius + 1)^2 window of the history; every other pixel keeps its word.  hist: temporal_torch's fourth result,
        float32 [3, H, W, 4]; variance: its second, float32 [H, W]; width, height: the frame's size, which both must have.  out: float32
        [H, W] or None (a new tensor); it may be `variance` itself.  Returns out, enqueued on torch.cuda.current_stream() without waiting
        for it; it goes into denoise_svgf_torch(variance=...).  Every tensor is checked before any C call.  The defaults of radius,
        min_history and sigma_depth are the best setting of the sweep in profiles/svgf_spatial/quality.json."""
        torch = sys.modules.get("torch")
        call = "svgf_spatial_variance_torch"
        w, h = int(width), int(height)
        if w < 1 or h < 1:
            raise ArtError("%s: width and height must be at least 1, not %d x %d" % (call, w, h))
        planes = [_Plane(call + ": hist", hist, "float32", (3, h, w, 4)), _Plane(call + ": variance", variance, "float32", (h, w)),
                  _Plane(call + ": out", out, "float32", (h, w), True)]
        _check_planes(torch, planes)
        _check_devices(planes, hist.device)
        if out is None:
            out = torch.empty((h, w), dtype=torch.float32, device=hist.device)
        p = ArtSvgfSpatialParams(w, h, int(radius), int(normal_log2), float(min_history), float(sigma_depth))
        _check(self.lib.art_svgf_spatial_variance_device(C.byref(p), hist.data_ptr(), variance.data_ptr(), out.data_ptr(),
                                                         _handle(_stream(torch, hist.device))))
        return out

    def _mask_tensor(self, torch, call, mask):
        if torch is not None and isinstance(mask, torch.Tensor) and mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)                   # (a bool tensor is one byte per element, 0 or 1)
        return mask, _frame_plane(torch, call + ": mask", mask, "uint8", self.width * self.height)

    def compact_mask_torch(self, mask):
        """The selected pixels of this rank's list, in list order (art_compact_mask_device; include/art_hip.h): mask is a uint8 or bool GPU
        tensor with H * W elements ([H, W] or flat), non-zero = selected.  Returns (pixels, count): a uint32-valued int32 tensor of H * W
        words whose first `count` hold the global pixel indices y * W + x, and count as a one-element int32 tensor -- both stay on the GPU,
        enqueued on torch.cuda.current_stream() without waiting for it."""
        torch = sys.modules.get("torch")
        mask, mp = self._mask_tensor(torch, "compact_mask_torch", mask)
        n = self.width * self.height
        pixels = torch.empty(n, dtype=torch.int32, device=mask.device)
        count = torch.empty(1, dtype=torch.int32, device=mask.device)
        _check(self.lib.art_compact_mask_device(mp, pixels.data_ptr(), n, count.data_ptr(), _handle(_stream(torch, mask.device))))
        return pixels, count

    def render_pass_masked(self, params, spp, mask, counts=None):
        """One render pass over the pixels mask selects (art_render_pass_masked; include/art_hip.h): bit for bit the full pass at that spp
        restricted to them; spp advances by the pass's samples whatever the mask holds.  mask: uint8 or bool GPU tensor with H * W
        elements; counts: None or an int32 GPU tensor with H * W elements (uint32 words), to whose selected pixels the pass's samples are
        added.  Tensors are checked before any C call.  The host waits once for the list's length and at the end, as render_pass does.
        Returns (new spp, pixels rendered)."""
        torch = sys.modules.get("torch")
        mask, mp = self._mask_tensor(torch, "render_pass_masked", mask)
        cp = _frame_plane(torch, "render_pass_masked: counts", counts, "int32", self.width * self.height, optional=True)
        s = C.c_int32(spp); k = C.c_int64(0)
        _check(self.lib.art_render_pass_masked(C.byref(params), mp, cp, C.byref(s), C.byref(k)))
        return s.value, k.value

    def adaptive_estimate_torch(self, accum, moments, counts, aa_on, threshold=None, lum_floor=None, min_colours=None, max_samples=1 << 30,
                                want=("mean", "variance", "error", "mask")):
        """Per pixel the mean colour, the variance of the mean's luminance, the relative error and the next mask
        (art_adaptive_estimate_device; include/art_hip.h states the arithmetic).  accum: float32 with 3 * H * W elements (the tensor of
        bind_accum as it is), moments: float32 with 2 * H * W (bind_moments), counts: int32 with H * W (uint32 words: the samples behind
        each pixel), all on the GPU, for the frame of resize().  Returns a dict of the planes named in `want`: mean [H, W, 3] float32,
        variance and error [H, W] float32, mask [H, W] uint8, enqueued on torch.cuda.current_stream() without waiting for it.  The
        defaults of threshold, lum_floor and min_colours are the best setting of the sweep in profiles/adaptive/quality.json."""
        torch = sys.modules.get("torch")
        call = "adaptive_estimate_torch"
        w, h = self.width, self.height
        ap = _frame_plane(torch, call + ": accum", accum, "float32", 3 * w * h)
        mp = _frame_plane(torch, call + ": moments", moments, "float32", 2 * w * h)
        cp = _frame_plane(torch, call + ": counts", counts, "int32", w * h)
        for name in want:
            if name not in ("mean", "variance", "error", "mask"):
                raise ArtError("%s: want: unknown plane %r" % (call, name))
        if not want:
            raise ArtError("%s: want: at least one plane" % call)
        dev = accum.device
        out = {}
        if "mean" in want:
            out["mean"] = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        for name in ("variance", "error"):
            if name in want:
                out[name] = torch.empty((h, w), dtype=torch.float32, device=dev)
        if "mask" in want:
            out["mask"] = torch.empty((h, w), dtype=torch.uint8, device=dev)
        p = ArtAdaptiveParams(w, h, 1 if aa_on else 0, int(ADAPTIVE_MIN_COLOURS if min_colours is None else min_colours), int(max_samples),
                              float(ADAPTIVE_THRESHOLD if threshold is None else threshold), float(ADAPTIVE_LUM_FLOOR if lum_floor is None else lum_floor))
        _check(self.lib.art_adaptive_estimate_device(C.byref(p), ap, mp, cp, *[_ptr(out.get(name)) for name in ("mean", "variance", "error", "mask")],
                                                     _handle(_stream(torch, dev))))
        return out

    def render_adaptive(self, params, budget_samples, step_vthreads, threshold=None, lum_floor=None, min_colours=None, max_samples=1 << 30,
                        first_vthreads=None, max_passes=1 << 20):
        """The plain adaptive loop on the frame of resize(): one full pass of first_vthreads (default step_vthreads) virtual threads, then
        estimate and masked pass of step_vthreads until the mask is empty, the next pass would take the total past budget_samples
        (camera samples over the whole frame), or max_passes is reached.  Binds an accum, a moments and a counts tensor of its own for the
        run (resize() zeroes the first two) and unbinds them at the end; single device, the whole frame (no set_shard).  Returns a dict: accum
        [H, W, 3] and moments [H, W, 2] float32, counts [H, W] int32, spp, passes and samples (the total), and mean [H, W, 3] =
        accum / counts from the estimate kernel."""
        import torch
        w, h = self.width, self.height
        per = 4 if params.aa_on else 1
        dev = torch.device("cuda", torch.cuda.current_device())
        accum = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        moments = torch.zeros((h, w, 2), dtype=torch.float32, device=dev)
        counts = torch.zeros((h, w), dtype=torch.int32, device=dev)
        step = ArtPassParams.from_buffer_copy(params); step.vthreads = int(step_vthreads)
        first = ArtPassParams.from_buffer_copy(params); first.vthreads = int(first_vthreads or step_vthreads)
        self.bind_accum(accum); self.bind_moments(moments)
        try:
            self.resize(w, h)
            spp = self.render_pass_device(first, 0)
            counts += spp
            passes, used = 1, spp * w * h
            kw = dict(threshold=threshold, lum_floor=lum_floor, min_colours=min_colours, max_samples=max_samples)
            while passes < max_passes:
                mask = self.adaptive_estimate_torch(accum, moments, counts, params.aa_on, want=("mask",), **kw)["mask"]
                k = int(mask.count_nonzero())
                if k == 0 or used + k * step.vthreads * per > budget_samples:
                    break
                spp, rendered = self.render_pass_masked(step, spp, mask, counts)
                used += rendered * step.vthreads * per
                passes += 1
            mean = self.adaptive_estimate_torch(accum, moments, counts, params.aa_on, want=("mean",), **kw)["mean"]
            torch.cuda.synchronize()
        finally:
            self.bind_moments(None); self.bind_accum(None)
        return dict(accum=accum, moments=moments, counts=counts, spp=spp, passes=passes, samples=used, mean=mean)

    def _vertex_tensors(self, pos, nrm):
        """Validated, contiguous vertex tensors of refit_torch / rebuild_torch, and torch's current stream of their device."""
        import torch
        if not isinstance(pos, torch.Tensor) or pos.dim() != 2:
            raise ArtError("pos: a [nverts, 3] float32 tensor is required")
        n = pos.shape[0]
        planes = [_Plane("pos", pos, "float32", _expected(n, 3)), _Plane("nrm", nrm, "float32", _expected(n, 3), True)]
        p, q = _check_planes(torch, planes, "make")
        self._need_device()
        _check_devices(planes, p.device)
        return torch, p, q, n, _stream(torch, p.device)

    @staticmethod
    def _refuse_bad_vertices(torch, call, p, q, stream):
        """check=True of the refits, before any launch; the ONE host synchronisation with the stream that it costs is here"""
        with torch.cuda.stream(stream):
            bad = (~(p.abs() <= 1e18)).any(dim=1).sum()
            badn = torch.zeros_like(bad) if q is None else (~torch.isfinite(q)).any(dim=1).sum()
            counts = torch.stack([bad, badn]).tolist()                     # the one host synchronisation
        if counts[0] or counts[1]:
            raise ValueError("%s: %d vertex position(s) not finite or beyond 1e18 in magnitude, %d normal(s) not finite" % (call, *counts))

    def set_camera(self, cam_pos, cam_matrix=None):
        """Replace the camera of the uploaded scene without a rebuild (art_set_camera): cam_pos 3 floats, cam_matrix 16 floats row-major
        or [4, 4] (None: the identity).  Stream-ordered on the library's stream: passes enqueued before see the old camera, later ones
        the new; the result is a fresh upload's with that camera, bit for bit."""
        pos = [float(v) for v in np.asarray(cam_pos, np.float32).reshape(-1)]
        mat = [float(v) for v in (np.eye(4, dtype=np.float32) if cam_matrix is None else np.asarray(cam_matrix, np.float32)).reshape(-1)]
        if len(pos) != 3 or len(mat) != 16:
            raise ArtError("set_camera: cam_pos takes 3 floats and cam_matrix 16")
        _check(self.lib.art_set_camera(C.byref((C.c_float * 3)(*pos)), C.byref((C.c_float * 16)(*mat))))

    def refit_torch(self, pos, nrm=None, check=True):
        """Move the vertices of the scene's CLOSEST mesh and refit its tree in place (art_refit_device): pos, nrm float32 [nverts, 3] tensors on
        the library's GPU, in the vertex order of the uploaded mesh; nrm None keeps the normals.  Enqueued on torch.cuda.current_stream()
        without waiting for it: work enqueued before sees the old geometry, work enqueued after the new.  The tree keeps its topology.
        check=True raises ValueError before any launch when a coordinate is not finite or beyond 1e18 in magnitude (or a normal is not
        finite); that check costs ONE host synchronisation with the stream.  check=False skips it: boxes holding a bad vertex are then
        emptied on the GPU and the next synchronize fails with the count."""
        torch, p, q, n, stream = self._vertex_tensors(pos, nrm)
        if check and n:
            self._refuse_bad_vertices(torch, "refit_torch", p, q, stream)
        _check(self.lib.art_refit_device(p.data_ptr(), _ptr(q), n, _handle(stream)))

    def refit_info(self):
        """ArtRefitInfo: refits, refit_ms (GPU time of device 0's refit kernels), plan_ms, bad_vertices -- cumulative since the upload (waits)"""
        return self._get("art_get_refit_info", ArtRefitInfo)

    def rebuild_torch(self, pos, nrm=None):
        """Build a new tree for the scene's CLOSEST mesh at new vertex positions, on the GPU (art_rebuild_device): the tree the next
        upload_scene of the moved mesh would build under the options as they stand.  pos, nrm as for refit_torch; enqueued on
        torch.cuda.current_stream(), but unlike a refit the call returns only when the tree is committed (the builders read counts
        back).  A bad vertex (not finite, beyond 1e18) fails the call with the count and leaves the scene unchanged."""
        torch, p, q, n, stream = self._vertex_tensors(pos, nrm)
        _check(self.lib.art_rebuild_device(p.data_ptr(), _ptr(q), n, _handle(stream)))

    def rebuild_info(self):
        """ArtRebuildInfo: rebuilds, gather_ms, build_ms (GPU time on device 0), host_ms (host time inside the calls) -- cumulative since the upload"""
        return self._get("art_get_rebuild_info", ArtRebuildInfo)

    def tree_cost(self):
        """ArtTreeCost of the tree in HBM (device 0; waits): root_area and the surface-area expectation of node visits, leaf visits and
        triangle tests per line through the root.  Compare a refitted tree's figure with a rebuilt one's to decide when to rebuild."""
        return self._get("art_get_tree_cost", ArtTreeCost)

    def move_instances_torch(self, m, check=True):
        """Move the instances of an instanced scene (art_move_instances_device): m is a float32 tensor [n_instances, 3, 4] or
        [n_instances, 12] on the library's GPU, instance i's object -> world matrix in the order of the uploaded instance list.  Enqueued
        on torch.cuda.current_stream() without waiting for it: work enqueued before sees the old placement, work enqueued after the new
        one.  The picture is the one of upload_scene at the new matrices; the instance tree keeps its topology.  check=True raises
        ValueError before any launch when an element is not finite; that check costs ONE host synchronisation with the stream.
        check=False skips it: a bad matrix (also a singular one, which check=True does not look for) empties its instance on the GPU
        and the next synchronize fails with the count."""
        import torch
        plane = _Plane("m", m, "float32", (lambda m: (m.dim() == 3 and tuple(m.shape[1:]) == (3, 4)) or (m.dim() == 2 and m.shape[1] == 12),
                                           "shape {}, expected [n_instances, 3, 4] or [n_instances, 12]"))
        m, = _check_planes(torch, [plane], "make")
        n = m.shape[0]
        self._need_device()
        _check_devices([plane])
        stream = _stream(torch, m.device)
        if check and n:
            with torch.cuda.stream(stream):
                bad = int((~torch.isfinite(m.reshape(n, 12))).any(dim=1).sum().item())      # the one host synchronisation
            if bad:
                raise ValueError("move_instances_torch: %d matrix(es) with an element that is not finite" % bad)
        _check(self.lib.art_move_instances_device(m.data_ptr(), n, _handle(stream)))

    def move_info(self):
        """ArtMoveInfo: moves, move_ms (GPU time of device 0's move kernels), plan_ms, bad_matrices, repads (meshes whose boxes a move
        had to widen) -- cumulative since the upload (waits)"""
        return self._get("art_get_move_info", ArtMoveInfo)

    def refit_mesh_torch(self, mesh, pos, nrm=None, check=True):
        """Deform mesh number `mesh` of an instanced scene (art_refit_mesh_device): pos, nrm float32 [nverts, 3] tensors on the library's
        GPU, object space, in the vertex order of that uploaded mesh; nrm None keeps the normals.  Enqueued on torch.cuda.current_stream()
        without waiting for it: work enqueued before sees the old shape, work enqueued after the new.  The picture is the one of
        upload_scene with that mesh's vertices replaced, at the matrices in force; the trees keep their topology.  check=True raises
        ValueError before any launch when a coordinate is not finite or beyond 1e18 in magnitude (or a normal is not finite); that check
        costs ONE host synchronisation with the stream.  check=False skips it: boxes and entry points holding a bad vertex are then
        emptied on the GPU and the next synchronize fails with the count."""
        torch, p, q, n, stream = self._vertex_tensors(pos, nrm)
        if check and n:
            self._refuse_bad_vertices(torch, "refit_mesh_torch", p, q, stream)
        _check(self.lib.art_refit_mesh_device(int(mesh), p.data_ptr(), _ptr(q), n, _handle(stream)))

    def mesh_refit_info(self):
        """ArtMeshRefitInfo: refits, refit_ms (GPU time of device 0's kernels), plan_ms, bad_vertices, repads (meshes whose boxes a mesh
        refit had to widen) -- cumulative since the upload (waits)"""
        return self._get("art_get_mesh_refit_info", ArtMeshRefitInfo)

    @staticmethod
    def _rebuild_stream(stream):
        """the stream a rebuild waits for: the caller's, else torch's current stream if torch is loaded and the GPU is in use, else the library's"""
        if stream is not None:
            return _handle(stream)
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
            return _handle(torch.cuda.current_stream())
        return None

    def rebuild_instances(self, stream=None):
        """Build the instance tree of the uploaded instanced scene again, on the GPU, from the entry points' world boxes as the last
        move or mesh refit left them (art_rebuild_instance_tree_device): the entry points and the meshes stay, the tree over them is the
        one upload_scene would build at the matrices in force.  stream: a torch.cuda.Stream whose work runs first (None: torch's current
        stream if torch is loaded and the GPU is in use, else the library's).  Unlike a move the call returns only when the tree is
        committed.  Bad matrices or bad vertices in force fail the call with their count and leave the scene unchanged."""
        _check(self.lib.art_rebuild_instance_tree_device(self._rebuild_stream(stream)))

    def instance_rebuild_info(self):
        """ArtInstanceRebuildInfo: rebuilds, gather_ms, build_ms (GPU time on device 0), host_ms (host time inside the calls) -- cumulative since the upload"""
        return self._get("art_get_instance_rebuild_info", ArtInstanceRebuildInfo)

    def instance_tree_cost(self):
        """ArtTreeCost of the instance tree in HBM (device 0; waits): root_area and the surface-area expectation of node visits and of
        entry points entered (leaf_visits = tri_tests) per line through the root.  Compare the figure of a moved tree with a rebuilt
        one's to decide when to call rebuild_instances."""
        return self._get("art_get_instance_tree_cost", ArtTreeCost)

    def rebuild_mesh(self, mesh, stream=None):
        """Build the tree of mesh number `mesh` of the uploaded instanced scene again, on the GPU, from its triangle records as the
        last refit_mesh_torch left them (art_rebuild_mesh_tree_device): the tree is the one upload_scene would build for the deformed
        mesh at the pad in force; indices, shading, matrices, entry points and the instance tree stay, the meshes behind it move.
        stream: as for rebuild_instances.  The call returns only when the tree is committed.  Bad matrices or bad vertices in force, and
        an instance of the mesh that the build opened (inst_open), fail the call and leave the scene unchanged."""
        _check(self.lib.art_rebuild_mesh_tree_device(int(mesh), self._rebuild_stream(stream)))

    def mesh_rebuild_info(self):
        """ArtMeshRebuildInfo: rebuilds, gather_ms, build_ms (GPU time on device 0), host_ms (host time inside the calls) -- cumulative since the upload"""
        return self._get("art_get_mesh_rebuild_info", ArtMeshRebuildInfo)

    def mesh_tree_cost(self, mesh):
        """ArtTreeCost of mesh number `mesh`'s tree in HBM, in object space (device 0; waits).  Compare the figure of a refitted tree with
        the one at the last build to decide when to call rebuild_mesh."""
        return self._get("art_get_mesh_tree_cost", ArtTreeCost, int(mesh))

    def bvh_info(self):
        info = ArtBvhInfo()
        _check(self.lib.art_export_bvh(None, 0, None, 0, C.byref(info)))
        return info

    def export_bvh(self):
        info = ArtBvhInfo()
        _check(self.lib.art_export_bvh(None, 0, None, 0, C.byref(info)))
        nodes = np.zeros(info.n_nodes * 8 * info.node_width, np.float32); tris = np.zeros(info.n_tris * 12, np.float32)
        _check(self.lib.art_export_bvh(_fp(nodes), nodes.size, _fp(tris), tris.size, C.byref(info)))
        return nodes, tris, info

    def export_two_level(self):
        """The two-level tree of the uploaded instanced scene as it lies in device 0's HBM (art_export_two_level; waits): a dict of numpy
        arrays -- inst [n_entry, 32] uint32 (DevInstance words), tlas_nodes [., 32], tlas_tris [n_entry, 12], blas_nodes [., 32], blas_tris
        [., 12] float32, qnodes [., 16] uint32 (the instance tree's nodes first), mesh_pad [n_mesh], mesh_box [n_mesh, 6] float32, mesh_base
        [n_mesh, 3], node_mesh int32 -- and the scalars n_inst, inst_shift, updated, mesh_pad_rel, mesh_pad_min, scene_extent, tlas_pad_rel,
        tlas_pad_abs."""
        out, rc = two_level_arrays(self.lib.art_export_two_level)
        _check(rc)
        return out

    def stats(self):
        return self._get("art_get_stats", ArtStats)

    def shutdown(self):
        self.lib.art_shutdown()
        self._accum_tensor = None


class RayTracer:
    """Mirror of package Ray_Tracer (ray_tracer.ads:18-48) on top of the backend.

    width/height/Threads_Num/Anti_Aliasing_On/Max_Trace_Depth/Background_Color are the package variables of
    ray_tracer.ads:20-27; Render_Pass forwards to art_render_pass instead of waking Path_Trace_Thread tasks."""

    def __init__(self, backend, scene):
        self.backend = backend
        backend.upload_scene(scene)
        self.width, self.height = 1024, 768          # ray_tracer.ads:20-21
        self.Threads_Num = 14 * 2                     # ray_tracer.ads:23
        self.Anti_Aliasing_On = True                  # ray_tracer.ads:24
        self.Max_Trace_Depth = 8                      # ray_tracer.ads:25
        self.Background_Color = (0.0, 0.0, 0.0)       # ray_tracer.ads:27
        self.seed = 1
        self.g_rend_type = PT_MIS
        self.g_finish = False
        self.g_spp = 0
        self.screen_buffer = None                     # ScreenBufferData(x, y): [width, height] u32
        self.g_accBuff = None                         # AccumBuff(x, y): [width, height, 3] f32

    def Init_Render(self, a_rendType):                # ray_tracer.adb:197-200
        self.g_rend_type = a_rendType

    def Resize_Viewport(self, size_x, size_y):        # ray_tracer.adb:297-320
        self.width, self.height = size_x, size_y
        self.backend.resize(size_x, size_y)
        self.g_spp = 0

    def GetSPP(self):                                 # ray_tracer.adb:322-325
        return self.g_spp

    def Finished(self):                               # ray_tracer.adb:202-205
        return self.g_finish

    def Render_Pass(self):                            # ray_tracer.adb:240-293
        p = Backend.pass_params(self.g_rend_type, self.Anti_Aliasing_On, self.Max_Trace_Depth, self.Threads_Num, self.seed,
                                self.Background_Color, LAYOUT_ADA_XY)
        if self.g_rend_type in (RT_DEBUG, RT_WHITTED):
            self.g_accBuff, self.screen_buffer, _, _, _ = self.backend.debug_hit_pass(p)
            self.g_finish = True
            return
        self.g_accBuff, self.screen_buffer, self.g_spp = self.backend.render_pass(p, self.g_spp, True, True)


def save_bmp(path, image_u32_rowmajor):
    """Bitmap.SaveBMP (bitmap.adb:31-85): 14+40 byte headers, then per pixel the bytes (bits 16-23, 8-15, 0-7), no row padding."""
    img = np.ascontiguousarray(image_u32_rowmajor, np.uint32)
    h, w = img.shape
    hdr = np.zeros(54, np.uint8)
    hdr[0:2] = (0x42, 0x4D)
    hdr[2:6] = np.frombuffer(np.uint32(54 + w * h * 3).tobytes(), np.uint8)
    hdr[10:14] = np.frombuffer(np.uint32(54).tobytes(), np.uint8)
    hdr[14:18] = np.frombuffer(np.uint32(40).tobytes(), np.uint8)
    hdr[18:22] = np.frombuffer(np.uint32(w).tobytes(), np.uint8)
    hdr[22:26] = np.frombuffer(np.uint32(h).tobytes(), np.uint8)
    hdr[26:28] = (1, 0); hdr[28:30] = (24, 0)
    px = np.stack([(img >> 16) & 255, (img >> 8) & 255, img & 255], -1).astype(np.uint8)
    data = hdr.tobytes() + px.tobytes()
    if path is not None:
        with open(path, "wb") as f:
            f.write(data)
    return data
