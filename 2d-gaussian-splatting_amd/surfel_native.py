"""ctypes loader for libsurfel_hip.so — the C-ABI boundary declared in include/surfel_hip.h.

There is NO fallback: if the HIP library is missing or cannot be loaded this module raises, so a
GPU box can never silently run some other path.  torch is imported first so that the HIP runtime
already mapped by PyTorch-ROCm (same SONAME libamdhip64.so.7) is the one our library binds to; torch
here is plumbing only (device memory through its caching allocator, current stream).

Adding a side module: check its tensors with device_tensor / rows below ("no CPU path: CPU tensors raise" is stated there, once),
and take a mesh with surfel_mesh.mesh_arrays; an `out=` buffer goes through uint8_buffer, a writer behind the renderer is built from
surfel_frames.
"""
import ctypes as C
import math
import os
import threading

import torch  # (must precede the CDLL below, see module doc)

_HERE = os.path.dirname(os.path.abspath(__file__))
# SURFEL_LIB: diagnostics only (e.g. the -DSURFEL_IEEE_MATH twin built by `python build.py --ieee`)
LIB_PATH = os.environ.get("SURFEL_LIB") or os.path.join(_HERE, "lib", "libsurfel_hip.so")

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
HOOK_FN = C.CFUNCTYPE(None, C.c_void_p)


class DevPtr:
    """Parameter type of a DEVICE pointer: a torch tensor passes as its data_ptr() and must live on a HIP device (a host address
    must never reach a kernel), None as NULL, anything else (c_void_p, int, byref) as c_void_p takes it."""

    @classmethod
    def from_param(cls, v):
        if isinstance(v, torch.Tensor):
            if not v.is_cuda:
                raise RuntimeError("libsurfel_hip: tensors must live on a HIP device (got %s)" % v.device)
            return C.c_void_p(v.data_ptr())
        return None if v is None else C.c_void_p.from_param(v)


class Stream:
    """Parameter type of `void* stream` (a hipStream_t), always the last parameter: call() fills it in."""
    from_param = C.c_void_p.from_param


class TsdfVolume(C.Structure):
    """surfel_tsdf_volume of include/surfel_mesh.h"""
    _fields_ = [("origin", C.c_int * 3), ("dims", C.c_int * 3), ("voxel_size", C.c_float), ("sdf_trunc", C.c_float), ("budget_bytes", C.c_int64),
                ("table", C.c_void_p), ("scratch", C.c_void_p), ("nblocks", C.c_int64), ("keys", C.c_void_p), ("stamp", C.c_void_p),
                ("list", C.c_void_p), ("tsdf_rgb", C.c_void_p), ("weight", C.c_void_p), ("info", C.c_void_p), ("vbase", C.c_void_p),
                ("tbase", C.c_void_p), ("pool_scratch", C.c_void_p), ("views", C.c_int64), ("nverts", C.c_int64), ("ntris", C.c_int64)]


class UnboundedVolume(C.Structure):
    """surfel_unbounded_volume of include/surfel_mesh_unbounded.h"""
    _fields_ = [("M", C.c_int), ("slab", C.c_int), ("R", C.c_float), ("center", C.c_float * 3), ("radius", C.c_float), ("voxel_size", C.c_float),
                ("budget_bytes", C.c_int64), ("tsdf", C.c_void_p), ("info", C.c_void_p), ("vbase", C.c_void_p), ("tbase", C.c_void_p),
                ("scan_scratch", C.c_void_p), ("slab_base", C.c_void_p), ("nslabs", C.c_int64), ("nverts", C.c_int64), ("ntris", C.c_int64)]


class UnboundedView(C.Structure):
    """surfel_unbounded_view of include/surfel_mesh_unbounded.h (64 B; an array of them is copied to the device)"""
    _fields_ = [("proj", C.c_float * 12), ("H", C.c_int32), ("W", C.c_int32), ("offset", C.c_int64)]


class EvalGrid(C.Structure):
    """surfel_eval_grid of include/surfel_eval.h"""
    _fields_ = [("origin", C.c_float * 3), ("cell", C.c_float), ("dims", C.c_int * 3), ("budget_bytes", C.c_int64), ("n", C.c_int64),
                ("sorted", C.c_void_p), ("order", C.c_void_p), ("ranges", C.c_void_p)]


class JpegDecDesc(C.Structure):
    """surfel_jpegdec_desc of include/surfel_jpegdec.h (a host structure: what surfel_jpegdec.parse found in the file's segments)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32),
                ("restart_interval", C.c_int32), ("ecs_offset", C.c_int64), ("ecs_bytes", C.c_int64),
                ("tq", C.c_uint8 * 4), ("td", C.c_uint8 * 4), ("ta", C.c_uint8 * 4), ("qt", (C.c_uint16 * 64) * 4),
                ("bits", (C.c_uint8 * 16) * 4), ("huffval", (C.c_uint8 * 256) * 4)]


class RepairPlan(C.Structure):
    """surfel_repair_plan of include/surfel_repair.h (a host structure; its arrays are device memory from the caller's allocator)"""
    _fields_ = [(k, C.c_int64) for k in ("V", "F", "max_hole_edges", "survivors", "split", "border", "loops", "fill_triangles", "fill_vertices")] + \
               [(k, C.c_void_p) for k in ("triangles", "triangle_source", "split_source", "half_edge", "loop", "position", "lengths", "fill_vertex",
                                          "fill_offset", "triangle_offset", "centroid_offset")]


# ---- every exported function: name ->(restype, parameter types ...), grouped by the header that declares it.  d = device pointer,
# s = the stream, u = any other void*, a = allocator callback; host pointers keep their POINTER(...) type.
_i, _i64, _f, _f64, _d, _s, _u, _a = C.c_int, C.c_int64, C.c_float, C.c_double, DevPtr, Stream, C.c_void_p, ALLOC_FN
_fp, _ip, _i64p, _f64p = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double)
_vol, _uvol, _grid, _jdesc = C.POINTER(TsdfVolume), C.POINTER(UnboundedVolume), C.POINTER(EvalGrid), C.POINTER(JpegDecDesc)
_rplan = C.POINTER(RepairPlan)
_adam = (_i, _d, _d, _d, _d, _d, _fp, _f, _f, _f, _i, _f, _i, _i, _d, _d)      # surfel_adam_step up to gcol_all
SIGNATURES = {
    "surfel_hip.h": {
        "surfel_abi_version": (_i,),
        "surfel_last_error": (C.c_char_p,),
        "surfel_rasterize_forward": (_i64, _a, _u, _a, _u, _a, _u, _i, _i, _i, _d, _i, _i, _d, _d, _d, _d, _d, _f, _d, _d, _d, _d, _d, _f, _f, _i,
                                     _d, _d, _d, _i, _s),
        "surfel_rasterize_backward": (_i, _a, _u, _i, _i, _i, _i64, _d, _i, _i, _d, _d, _d, _d, _f, _d, _d, _d, _d, _d, _f, _f, _d, _d, _d, _d,
                                      _d, _d, _d, _d, _d, _d, _d, _d, _d, _d, _d, _i, _s),
        "surfel_mark_visible": (_i, _i, _d, _d, _d, _d, _s),
        "surfel_knn_dist2": (_i, _a, _u, _i, _d, _d, _s),
        "surfel_set_option": (_i, C.c_char_p, _i),
        "surfel_set_backward_hook": (_i, HOOK_FN, _u),
        "surfel_forward_count": (_i64,),
    },
    "surfel_contrib.h": {
        "surfel_rasterize_contribution": (_i, _i, _i64, _i, _i, _d, _d, _d, C.c_uint32, _d, _d, _d, _d, _d, _d, _d, _i, _s),
    },
    "surfel_select.h": {
        "surfel_rasterize_label_votes": (_i, _i, _i64, _i, _i, _d, _d, _d, _d, _i, _d, _i, _s),
    },
    "surfel_debug.h": {
        "surfel_last_stage_ms": (_i, _fp, _i),
        "surfel_last_stage_ids": (_i, _ip, _i),
        "surfel_collect_stage_ms": (_i, _fp, _ip, _i),
        "surfel_stage_name": (C.c_char_p, _i),
        "surfel_debug_sort_pairs": (_i, _a, _u, _d, _d, _i64, _i, _i, _s),
        "surfel_debug_tile_depth_sort": (_i, _i, _i64, _d, _d, _d, _d, _i, _s),
        "surfel_debug_tile_depth_sort_classes": (_i, _ip, _i),
        "surfel_debug_set_tile_radix_min": (_i, _i),
        "surfel_debug_set_blend_stats": (_i, _d),
        "surfel_debug_last_binning": (_i,),
        "surfel_debug_capacity_evictions": (_i,),
        "surfel_debug_image_layout": (_i, _i, _i, _i64p),
        "surfel_debug_box_probe": (_i, _d, _i64, _fp, _s),
        "surfel_debug_latency_probe": (_i, _d, _i64, _i, _fp, _s),
    },
    "surfel_train.h": {
        "surfel_l1_ssim_forward": (_i, _i, _i, _i, _d, _d, _d, _d, _s),
        "surfel_l1_ssim_backward": (_i, _i, _i, _i, _d, _d, _d, _f, _f, _d, _d, _d, _s),
        "surfel_l1_ssim_forward_w": (_i, _i, _i, _i, _i, _d, _d, _d, _d, _s),
        "surfel_l1_ssim_backward_w": (_i, _i, _i, _i, _i, _d, _d, _d, _f, _f, _d, _d, _d, _s),
        "surfel_render_post_forward": (_i, _i, _i, _d, _d, _f, _d, _d, _s),
        "surfel_render_post_backward": (_i, _i, _i, _d, _d, _f, _d, _f, _f, _d, _d, _s),
        "surfel_train_loss_forward": (_i, _i, _i, _d, _d, _d, _d, _d, _d, _f, _d, _s),
        "surfel_train_loss_backward": (_i, _i, _i, _d, _d, _d, _f, _f, _d, _d, _f, _f, _f, _d, _d, _d, _d, _d, _f, _f, _f, _d, _d, _s),
        "surfel_reduce_partials": (_i, _d, _i, _i, _i, _f, _d, _s),
        "surfel_loss_finalize": (_i, _d, _i, _i, _d, _i, _i, _f, _f, _f, _d, _d, _s),
        "surfel_activate": (_i, _i, _d, _d, _s),
        "surfel_adam_step": (_i,) + _adam + (_i, _s),
        "surfel_train_update": (_i,) + _adam + (_d, _d, _d, _d, _d, _s),
        "surfel_sh_grad_gather": (_i, _i, _i, _i, _d, _d, _d, _d, _s),
        "surfel_densify_stats": (_i, _i, _d, _d, _d, _d, _d, _s),
    },
    "surfel_mesh.h": {
        "surfel_tsdf_table_bytes": (_i64, _vol),
        "surfel_tsdf_block_bytes": (_i64,),
        "surfel_mesh_prepare_view": (_i, _i, _i, _d, _d, _d, _f, _d, _d, _s),
        "surfel_tsdf_init": (_i, _vol, _a, _u, _s),
        "surfel_tsdf_mark": (_i, _vol, _i, _i, _d, _d, _s),
        "surfel_tsdf_allocate": (_i64, _vol, _a, _u, _s),
        "surfel_tsdf_integrate": (_i, _vol, _i, _i, _d, _d, _d, _s),
        "surfel_tsdf_count": (_i, _vol, _s),
        "surfel_tsdf_extract": (_i, _vol, _d, _d, _d, _s),
        "surfel_mesh_clusters": (_i, _a, _u, _i64, _i64, _d, _d, _d, _s),
        "surfel_mesh_filter": (_i, _a, _u, _i64, _i64, _d, _d, _d, _d, _d, _i, _d, _d, _d, _i64p, _s),
    },
    "surfel_mesh_unbounded.h": {
        "surfel_unbounded_bytes": (_i64, _uvol),
        "surfel_unbounded_init": (_i, _uvol, _a, _u, _s),
        "surfel_unbounded_fuse": (_i, _uvol, _i, _d, _d, _d, _s),
        "surfel_unbounded_count": (_i, _uvol, _s),
        "surfel_unbounded_extract": (_i, _uvol, _d, _d, _s),
        "surfel_unbounded_color": (_i, _i64, _d, _i, _d, _d, _d, _f, _d, _s),
    },
    "surfel_eval.h": {
        "surfel_eval_sample_count": (_i64, _a, _u, _i64, _i64, _d, _d, _f64, _i64, _d, _s),
        "surfel_eval_sample_emit": (_i, _i64, _i64, _d, _d, _f64, _d, _i64, _d, _s),
        "surfel_eval_grid_build": (_i, _a, _u, _grid, _i64, _d, _d, _s),
        "surfel_eval_thin": (_i, _a, _u, _grid, _f, _d, _ip, _s),
        "surfel_eval_obs_mask": (_i, _i64, _d, _fp, _f, _f64, _d, _ip, _d, _d, _s),
        "surfel_eval_above_plane": (_i, _i64, _d, _f64p, _d, _s),
        "surfel_eval_nearest": (_i, _a, _u, _grid, _i64, _d, _f, _d, _d, _s),
        "surfel_eval_mean_below": (_i, _a, _u, _i64, _d, _f, _d, _s),
        "surfel_eval_dilate_masks": (_i, _a, _u, _i, _i, _i, _d, _i, _d, _s),
        "surfel_eval_cull_vertices": (_i, _i64, _d, _i, _d, _i, _i, _d, _d, _s),
    },
    "surfel_eval_tnt.h": {
        "surfel_tnt_mesh_cloud": (_i, _i64, _i64, _d, _d, _d, _s),
        "surfel_tnt_transform": (_i, _i64, _d, _f64p, _d, _s),
        "surfel_tnt_crop": (_i, _i64, _d, _i, _f64, _f64, _i, _d, _d, _s),
        "surfel_tnt_voxel_down_sample": (_i64, _a, _u, _i64, _d, _f64, _f64p, _i64, _d, _d, _d, _s),
        "surfel_tnt_corr_sums": (_i, _a, _u, _i64, _d, _d, _i64, _d, _d, _s),
        "surfel_tnt_histogram": (_i, _i64, _d, _i, _d, _f64, _d, _s),
    },
    "surfel_metrics.h": {
        "surfel_lpips_workspace_bytes": (_i64, _i, _i, _i64),
        "surfel_lpips_prepare": (_i, _i, _i, _d, _d, _d, _s),
        "surfel_lpips_conv3x3": (_i, _i, _i, _i, _i, _d, _d, _d, _d, _s),
        "surfel_lpips_pool": (_i, _i, _i, _i, _d, _d, _s),
        "surfel_lpips_tap": (_i, _i, _i, _i, _d, _d, _d, _s),
        "surfel_sq_err_partials": (_i, _i64, _d, _d, _d, _s),
    },
    "surfel_scene.h": {
        "surfel_scene_resample_table": (_i, _i, _i, _ip, _ip, _i64),
        "surfel_scene_resample_h": (_i, _i, _i, _i, _i, _i, _d, _d, _d, _d, _d, _d, _s),
        "surfel_scene_resample_v": (_i, _i, _i, _i, _i, _i, _d, _d, _d, _d, _d, _d, _s),
        "surfel_scene_to_float": (_i, _i, _i, _i, _d, _d, _d, _s),
        "surfel_scene_composite": (_i, _i, _i, _i, _d, _d, _s),
    },
    "surfel_vis.h": {
        "surfel_vis_quantize": (_i, _i, _i, _i, _d, _f, _f, _d, _s),
        "surfel_vis_order_stats": (_i, _i64, _d, _i, _i64p, _d, _d, _i64, _s),
        "surfel_vis_depth_turbo": (_i, _i, _i, _d, _f64, _f64, _d, _s),
    },
    "surfel_view.h": {
        "surfel_view_scalar": (_i, _i, _i, _d, _d, _d, _i64, _s),
        "surfel_view_gradient": (_i, _i, _i, _d, _f, _f, _d, _d, _i64, _s),
    },
    "surfel_cull.h": {
        "surfel_cull_mesh_depth": (_i64, _a, _u, _i64, _i64, _d, _d, _i, _d, _d, _i, _i, _i, _f, _f, _i, _d, _fp, _s),
        "surfel_cull_visibility": (_i, _i64, _d, _i, _d, _d, _i, _i, _i, _d, _f, _d, _s),
    },
    "surfel_meshview.h": {
        "surfel_meshview_visibility": (_i64, _a, _u, _i64, _i64, _d, _d, _i, _d, _d, _i, _i, _i, _f, _f, _i, _d, _fp, _s),
        "surfel_meshview_vertex_normals": (_i, _i64, _i64, _d, _d, _d, _d, _s),
        "surfel_meshview_shade": (_i, _i64, _i64, _d, _d, _d, _d, _i, _d, _d, _i, _i, _i, _i, _d, _i, _f, _f, _f, _d, _s),
    },
    "surfel_simplify.h": {
        "surfel_simplify_bounds": (_i, _a, _u, _i64, _d, _fp, _s),                       # bounds, origin, counts, stage_ms: HOST pointers
        "surfel_simplify_clusters": (_i64, _a, _u, _i64, _d, _fp, _fp, _f, _d, _s),
        "surfel_simplify_count": (_i64, _a, _u, _i64, _i64, _d, _d, _fp, _fp, _f, _i64p, _s),
        "surfel_simplify_mesh": (_i, _a, _u, _i64, _i64, _d, _d, _d, _fp, _fp, _f, _f64, _d, _d, _d, _d, _d, _i64p, _fp, _s),
    },
    "surfel_texture.h": {
        "surfel_texture_classify": (_i, _a, _u, _i64, _i64, _d, _d, _f, _d, _i64p, _s),      # counts, table: HOST pointers
        "surfel_texture_layout": (_i64, _a, _u, _i64, _i64, _d, _d, _d, _i64p, _i, _ip, _d, _d, _s),
        "surfel_texture_bake": (_i, _i64, _i64, _d, _d, _ip, _d, _i, _i, _i, _d, _d, _i, _i, _i, _d, _d, _f, _f, _i, _i, _d, _s),
        "surfel_texture_resolve": (_i, _i64, _i64, _d, _d, _d, _ip, _d, _i, _i, _d, _i, _f, _f, _f, _d, _d, _s),
        "surfel_texture_shade": (_i, _i64, _i64, _d, _d, _d, _d, _i, _i, _i, _d, _d, _i, _i, _i, _i, _d, _f, _f, _f, _d, _s),
    },
    "surfel_smooth.h": {
        "surfel_smooth_adjacency": (_i64, _a, _u, _i64, _i64, _d, _d, _d, _d, _d, _d, _i64p, _s),      # counts, factors: HOST pointers
        "surfel_smooth_steps": (_i, _i64, _d, _d, _d, _d, _i, _i, _f64p, _d, _d, _d, _s),
    },
    "surfel_repair.h": {
        "surfel_repair_analyze": (_i, _a, _u, _i64, _i64, _d, _d, _i64, _rplan, _i64p, _fp, _s),      # plan, counts, stage_ms: HOST pointers
        "surfel_repair_emit": (_i, _rplan, _d, _d, _d, _d, _d, _d, _d, _d, _s),
        "surfel_repair_loops": (_i, _rplan, _d, _d, _d, _d, _s),
    },
    "surfel_jpeg.h": {
        "surfel_jpeg_capacity": (_i64, _i, _i),
        "surfel_jpeg_scratch_bytes": (_i64, _i, _i),
        "surfel_jpeg_encode": (_i, _i, _i, _d, _i, _d, _i64, _d, _d, _i64, _s),
    },
    "surfel_png.h": {
        "surfel_png_capacity": (_i64, _i, _i, _i),
        "surfel_png_scratch_bytes": (_i64, _i, _i, _i),
        "surfel_png_encode": (_i, _i, _i, _i, _d, _d, _i64, _d, _d, _i64, _s),
    },
    "surfel_jpegdec.h": {
        "surfel_jpegdec_scratch_bytes": (_i64, _jdesc, _i),
        "surfel_jpegdec_decode": (_i, _jdesc, _d, _i64, _d, _d, _i64, _i, _i, _i, _d, _s),
    },
    "surfel_undistort.h": {
        "surfel_scene_undistort": (_i, _i, _i, _i, _i, _i, _f64p, _f64p, _d, _d, _s),
    },
    "surfel_log.h": {
        "surfel_log_append": (_i, _d, _d, _i, _i, _i, _d, _f, _f, _s),
        "surfel_log_panel": (_i, _i, _i, _i, _d, _d, _d, _i64, _s),
        "surfel_log_crc32c": (C.c_uint32, _u, _i64),                       # the framing entries take HOST pointers
        "surfel_log_frame": (_i64, _u, _i64, _u),
        "surfel_log_steps_capacity": (_i64, _i64),
        "surfel_log_encode_steps": (_i64, _u, _i64, _f, _f64, _u, _i64),
    },
}
EXPORTS = [name for h in ("surfel_hip.h", "surfel_debug.h", "surfel_train.h") for name in SIGNATURES[h]]
CONTRIB_EXPORTS = list(SIGNATURES["surfel_contrib.h"])
SELECT_EXPORTS = list(SIGNATURES["surfel_select.h"])
MESH_EXPORTS = list(SIGNATURES["surfel_mesh.h"])
UNBOUNDED_EXPORTS = list(SIGNATURES["surfel_mesh_unbounded.h"])
EVAL_EXPORTS = list(SIGNATURES["surfel_eval.h"])
TNT_EXPORTS = list(SIGNATURES["surfel_eval_tnt.h"])
METRICS_EXPORTS = list(SIGNATURES["surfel_metrics.h"])
SCENE_EXPORTS = list(SIGNATURES["surfel_scene.h"])
VIS_EXPORTS = list(SIGNATURES["surfel_vis.h"])
VIEW_EXPORTS = list(SIGNATURES["surfel_view.h"])
CULL_EXPORTS = list(SIGNATURES["surfel_cull.h"])
MESHVIEW_EXPORTS = list(SIGNATURES["surfel_meshview.h"])
SIMPLIFY_EXPORTS = list(SIGNATURES["surfel_simplify.h"])
TEXTURE_EXPORTS = list(SIGNATURES["surfel_texture.h"])
SMOOTH_EXPORTS = list(SIGNATURES["surfel_smooth.h"])
REPAIR_EXPORTS = list(SIGNATURES["surfel_repair.h"])
JPEG_EXPORTS = list(SIGNATURES["surfel_jpeg.h"])
PNG_EXPORTS = list(SIGNATURES["surfel_png.h"])
JPEGDEC_EXPORTS = list(SIGNATURES["surfel_jpegdec.h"])
UNDISTORT_EXPORTS = list(SIGNATURES["surfel_undistort.h"])
LOG_EXPORTS = list(SIGNATURES["surfel_log.h"])
_SIG = {name: sig for group in SIGNATURES.values() for name, sig in group.items()}


# error codes and the per-call option overrides carried in the upper bits of the `debug` argument (include/surfel_hip.h, its order)
E_INVALID = -1
E_LIMIT = -4
E_OVERFLOW = -5
OPT_NO_CULL = 1 << 8
OPT_BWD_QUAD = 1 << 11
OPT_BWD_ROWS = 1 << 12
OPT_PBWD_COOP = 1 << 13
OPT_PBWD_THREAD = 1 << 14
OPT_BWD_SCAN = 1 << 15         # scan walk (lanes = instances); deterministic, not bit-identical to rows / quad
OPT_EXACT_BINNING = 1 << 16    # forward: size the binning buffers exactly (host wait for the instance count) for this call
OPT_TILE_CUTS = 1 << 17        # backward: tile cuts instead of zero gradient records (default: R >= 2^21); bit-identical
OPT_ZERO_RECORDS = 1 << 18     # backward: zero gradient records behind a tile's saturation point (default: R < 2^21)
OPT_LAZY_COUNT = 1 << 21       # forward: do not wait for the instance count; forward_count() collects it (include/surfel_hip.h)
OPT_BWD_GATHER = 1 << 22       # backward: ignore the forward's tile stream, gather by surfel id (bit-identical)
OPT_NO_STREAM = 1 << 23        # forward: no backward follows (inference / no_grad): leave no tile stream behind
OPT_PBWD_NO_JAC = 1 << 24      # backward: read the SH block again instead of the forward's d(colour)/d(direction) rows (same result to rounding)


def opt_tile_order(mode):
    """per-call "tile_order" (0 auto, 1 XCD-contiguous, 2 longest lists first) in the debug word (SURFEL_OPT_TILE_ORDER)"""
    return ((int(mode) + 1) & 3) << 19


def opt_tile_sort(mode):
    return ((mode + 1) & 3) << 9


_lib = None
_lock = threading.Lock()


def load():
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libsurfel_hip.so not found at %s — build it with `python 2d-gaussian-splatting_amd/build.py` "
                "(hipcc --offload-arch=gfx950). There is no CPU / PyTorch fallback for the rasterizer." % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (restype, *argtypes) in _SIG.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        if lib.surfel_abi_version() != 1:
            raise ImportError("libsurfel_hip.so ABI version mismatch")
        # SURFEL_OPTIONS="name=value,..." -> surfel_set_option (A/B runs of an unmodified caller, e.g. bench.py)
        for kv in filter(None, os.environ.get("SURFEL_OPTIONS", "").split(",")):
            name, _, value = kv.partition("=")
            if lib.surfel_set_option(name.strip().encode(), int(value)) != 0:
                raise ValueError("SURFEL_OPTIONS: unknown option %r" % name)
        _lib = lib
    return _lib


class LimitError(RuntimeError):
    """SURFEL_E_LIMIT: a size exceeds an internal limit or the caller's byte budget (raise the budget or coarsen the input)."""


class CapacityOverflow(RuntimeError):
    """a lazily counted frame held more tile instances than its capacity: render it again (OPT_EXACT_BINNING)"""


_ERRORS = {E_LIMIT: LimitError, E_OVERFLOW: CapacityOverflow}
_STREAMED = frozenset(name for name, sig in _SIG.items() if sig[-1] is Stream)


def call(device, name, *args):
    """The one path from Python into the library: `name`(*args) with `device` current and, where the function's last parameter is
    the stream, that device's current stream appended.  device=None: a call that touches no device (no device guard, a NULL
    stream).  Tensors pass as they are (DevPtr).  Returns the return code when it is >= 0; a negative one raises LimitError
    (SURFEL_E_LIMIT), CapacityOverflow (SURFEL_E_OVERFLOW) or RuntimeError, each with the code and the library's message.  The
    function is looked up on the loaded library at every call, so a proxy put in its place (scripts/host_split.py) sees them all."""
    fn = getattr(load(), name)
    if name in _STREAMED:
        args += (None if device is None else current_stream_ptr(device),)
    try:
        if device is None:
            rc = fn(*args)
        else:
            with torch.cuda.device(device):
                rc = fn(*args)
    except C.ArgumentError as e:      # ctypes' wrapper around what a parameter type refused (DevPtr: a host tensor)
        raise RuntimeError("%s: %s" % (name, e)) from None
    if rc < 0:
        raise _ERRORS.get(rc, RuntimeError)("%s failed (%d): %s" % (name, rc, last_error()))
    return rc


_hook_keepalive = None


def set_backward_hook(fn):
    """surfel_set_backward_hook: fn() is called inside every rasterizer backward once dL/dcolour is final on the stream (None
    removes the hook).  The ctypes thunk is kept alive here for as long as the hook is installed."""
    global _hook_keepalive
    thunk = HOOK_FN() if fn is None else HOOK_FN(lambda user: fn())
    call(None, "surfel_set_backward_hook", thunk, None)
    _hook_keepalive = None if fn is None else thunk


def forward_count():
    """surfel_forward_count: exact instance count of this thread's last forward; raises CapacityOverflow for a lazily counted frame
    whose lists were truncated."""
    return int(call(None, "surfel_forward_count"))


def last_error():
    return load().surfel_last_error().decode()


def bucket_bytes(n):
    """Size actually requested from torch for an n-byte scratch buffer.  The R-sized buffers (binning state, the 80 B/instance
    gradient records: ~10 GB at 1.3e8 instances) change by a few per cent from frame to frame; the caching allocator cannot grow
    a cached block, so every new maximum cost a fresh hipMalloc of the whole buffer (290 ms at 10 GB, measured) while the slightly
    smaller block stayed cached — reserved memory ratcheted up by the buffer size each time.  Sizes of 64 MiB and more are
    therefore rounded up to the next multiple of 1/16 .. 1/8 of themselves (a power of two), so a fluctuating size settles in one or
    two blocks; smaller requests are left to the allocator's own 2 MiB rounding."""
    n = int(n)
    if n < (1 << 26):
        return max(n, 1)
    step = 1 << (n.bit_length() - 4)
    return (n + step - 1) // step * step


class TorchAllocator:
    """Allocator callback backed by torch's caching allocator (uint8 tensors kept alive in `held`).
    The ctypes callback closes over the `held` list only — not over `self` — so there is no reference cycle and the
    buffers go back to the caching allocator as soon as the last reference dies (with a cycle they waited for the
    cyclic GC, which at 10 M surfels grew the footprint by ~13 GB per step)."""

    def __init__(self, device):
        held = []

        def _alloc(user, nbytes):
            try:
                t = torch.empty(bucket_bytes(nbytes), dtype=torch.uint8, device=device)
            except Exception:  # out of memory -> NULL -> SURFEL_E_ALLOC
                return None
            held.append(t)
            return t.data_ptr()

        self.device = device
        self.held = held
        self.cb = ALLOC_FN(_alloc)

    def last(self):
        return self.held[-1]

    def view(self, pointer, dtype, shape):
        """The held buffer that starts at `pointer` (an address the library reported), viewed as `shape` elements of `dtype`."""
        for t in self.held:
            if t.data_ptr() == pointer:
                return t[:math.prod(shape) * dtype.itemsize].view(dtype).view(*shape)
        raise KeyError(pointer)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------ argument checks of the side modules
# (`who` is the calling module's name, the prefix of every message)
def device_tensor(who, t, what=None):
    """t, or "no CPU path: CPU tensors raise": RuntimeError for anything but a tensor on a HIP device.  what: the argument's name in
    the message, for the modules that name it"""
    if not torch.is_tensor(t) or not t.is_cuda:
        got = t.device if torch.is_tensor(t) else type(t).__name__
        raise RuntimeError("%s: tensors must live on a HIP device (%sgot %s)" % (who, "" if what is None else what + ": ", got))
    return t


def view_buffers(who, buffers, device, P, holder):
    """(b, W, H) of the view a pass runs behind: `buffers` is surfel_render.rasterize_buffers' dict, or a render package that carries
    it under "buffers".  ValueError when a key is missing or the view's surfel count is not P, RuntimeError unless `device` (where the
    pass accumulates; holder: what it accumulates in, for the messages) and the three buffers are on a HIP device."""
    b = buffers.get("buffers", buffers)
    for k in ("geom", "binning", "image", "num_rendered", "width", "height"):
        if k not in b:
            raise ValueError("%s: the view's buffers lack %r" % (who, k))
    if device.type != "cuda":
        raise RuntimeError("%s: tensors must live on a HIP device (the %s are on %s)" % (who, holder, device))
    for k in ("geom", "binning", "image"):
        device_tensor(who, b[k], k)
    if "P" in b and int(b["P"]) != P:
        raise ValueError("%s: the view rendered %d surfels, the %s hold %d" % (who, int(b["P"]), holder, P))
    return b, int(b["width"]), int(b["height"])


def uint8_buffer(who, t, n, device, what="out", at_least=False):
    """The buffer for `n` output bytes: a new uint8 [n] on `device` when the caller supplied none (t is None), otherwise t — ValueError
    unless it is a contiguous uint8 tensor of n elements (any shape) or, with at_least, a one-dimensional one of n elements or more
    (the encoders' out and scratch)"""
    if t is None:
        return torch.empty(n, dtype=torch.uint8, device=device)
    if t.dtype != torch.uint8 or not t.is_contiguous() or ((t.dim() != 1 or t.numel() < n) if at_least else t.numel() != n):
        raise ValueError("%s: %s must be a contiguous uint8 tensor of %s%d elements" % (who, what, "at least " if at_least else "", n))
    return t


def file_bytes(buf, size):
    """The file an encoder left on the device as bytes: waits for the int64 [1] device tensor `size`, then copies exactly that many
    bytes of `buf`"""
    return buf[:int(size.item())].cpu().numpy().tobytes()


def rows(who, t, what, dtype, shape="[N, 3]"):
    """t as a contiguous [N, 3] device tensor of `dtype`, detached; ValueError for another shape.  shape: how the message writes [N, 3]"""
    t = device_tensor(who, t, what)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("%s: %s must be %s, got %s" % (who, what, shape, list(t.shape)))
    return t.detach().to(dtype).contiguous()


def counts_dict(names, carray):
    """{name: int} of a ctypes array of counts the library filled"""
    return {k: int(v) for k, v in zip(names, carray)}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream_ptr(device):
    # (torch.cuda.current_stream() builds a Stream object per call: ~7 us of the ~400 us a training iteration costs on the host)
    if _raw_stream is not None and device.index is not None:
        return C.c_void_p(_raw_stream(device.index))
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class ManualCtx:
    """Stand-in for the autograd context when a caller drives forward() / backward() of the library's autograd Functions itself
    (surfel_trainer: the iteration's chain is fixed — rasterizer -> loss -> loss backward -> rasterizer backward — and the autograd
    engine, its worker-thread hand-over and the parameter gates cost more host time than all the launches together)."""
    manual = True
    needs_input_grad = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        pass

    def set_materialize_grads(self, value):
        pass


def stage_times():
    """[(stage_name, ms)] of the last debug-mode forward/backward on this thread."""
    lib = load()
    ms = (C.c_float * 16)()
    ids = (C.c_int * 16)()
    n = lib.surfel_last_stage_ms(ms, 16)
    lib.surfel_last_stage_ids(ids, 16)
    return [(lib.surfel_stage_name(ids[k]).decode(), float(ms[k])) for k in range(n)]


def collect_stage_times():
    """{stage_name: (total_ms, launches)} for all debug==2 calls since the previous collect (synchronises)."""
    lib = load()
    ms = (C.c_float * 16)()
    cnt = (C.c_int * 16)()
    n = lib.surfel_collect_stage_ms(ms, cnt, 16)
    return {lib.surfel_stage_name(k).decode(): (float(ms[k]), int(cnt[k])) for k in range(n) if cnt[k] > 0}
