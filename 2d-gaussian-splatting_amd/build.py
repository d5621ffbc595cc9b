"""Build libsurfel_hip.so (gfx950) in-tree with hipcc.  Usage: python build.py [--force]

The .so is git-ignored but travels to the GPU box with the gpurun snapshot.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "lib", "libsurfel_hip.so")
SOURCES = ["surfel_preprocess.hip", "surfel_forward.hip", "surfel_backward.hip", "surfel_backward_scan.hip", "surfel_contrib.hip", "surfel_select.hip", "surfel_sort.hip", "surfel_api.hip", "knn.hip", "box_probe.hip",
           "train_loss.hip", "train_post.hip", "train_fused.hip", "train_optim.hip", "train_api.hip",
           "device_scan.hip", "mesh_tsdf.hip", "mesh_unbounded.hip", "eval_geometry.hip", "eval_tnt.hip", "metrics_lpips.hip", "scene_image.hip", "frame_vis.hip", "view_image.hip", "mesh_cull.hip", "mesh_view.hip", "frame_jpeg.hip", "frame_png.hip", "scene_jpeg.hip", "scene_undistort.hip", "train_log.hip", "log_events.cpp", "mesh_simplify.hip", "mesh_texture.hip", "mesh_smooth.hip", "mesh_repair.hip"]
# blend kernels: packed-f32 VALU (SLP) costs ~1.6x a scalar op on gfx950 plus the v_movs that pair the operands
# surfel_backward.hip spells every fused multiply-add out (FMA macro) and is compiled with contraction off, so its kernel variants
# round identically per (pixel, surfel) pair
EXTRA = {"surfel_forward.hip": ["-fno-slp-vectorize"], "surfel_backward.hip": ["-fno-slp-vectorize", "-ffp-contract=off"],
         "surfel_backward_scan.hip": ["-fno-slp-vectorize", "-ffp-contract=off"],
         # surfel_contrib.hip walks as blend_fwd does and must round w = alpha * T and the transmittance as it does: the forward's flags
         "surfel_contrib.hip": ["-fno-slp-vectorize"],
         # surfel_select.hip walks as surfel_contrib.hip does, for the same reason: the forward's flags
         "surfel_select.hip": ["-fno-slp-vectorize"],
         # mesh_tsdf.hip: no contraction, so the allocation pass rounds as its fp32 restatement (tests/mesh_oracle.py)
         "mesh_tsdf.hip": ["-ffp-contract=off"],
         # eval_geometry.hip: no contraction, so the sampling decisions (fp64) and the thinning's pair test (fp32) round as their
         # restatements (tests/eval_oracle.py)
         "eval_geometry.hip": ["-ffp-contract=off"],
         # eval_tnt.hip: no contraction, so the fp64 decisions (crop, voxel cell, histogram bin) round as their restatements
         # (tests/tnt_oracle.py)
         "eval_tnt.hip": ["-ffp-contract=off"],
         # scene_image.hip: no contraction, so the fp64 resampling weights (host) and the fp64 composite (device) round as their
         # restatements (tests/scene_oracle.py)
         "scene_image.hip": ["-ffp-contract=off"],
         # frame_vis.hip: no contraction, so v * scale + bias (fp32) and the fp64 depth normalisation round as their restatements
         # (tests/path_oracle.py)
         "frame_vis.hip": ["-ffp-contract=off"],
         # view_image.hip: no contraction, so the Sobel sums and the normalisation (fp32) round as their restatement (tests/view_oracle.py)
         "view_image.hip": ["-ffp-contract=off"],
         # mesh_cull.hip: no contraction, so the visibility kernel's fp32 chain rounds as its restatement (tests/cull_oracle.py); the
         # rasteriser writes its fused multiply-adds out
         "mesh_cull.hip": ["-ffp-contract=off"],
         # mesh_view.hip: no contraction, so the vertex-normal and shading kernels (fp32) round as their restatement
         # (tests/meshview_oracle.py); the rasteriser it shares with mesh_cull.hip (mesh_raster.h) writes its fused multiply-adds out
         "mesh_view.hip": ["-ffp-contract=off"],
         # frame_jpeg.hip: no contraction, so the colour conversion, the DCT sums and the quantiser's division (fp32) round as their
         # restatement (tests/video_oracle.py) and the JPEG file comes out byte for byte
         "frame_jpeg.hip": ["-ffp-contract=off"],
         # scene_undistort.hip: no contraction, so the fp64 distortion formula and the bilinear blend round as their restatement
         # (tests/undistort_oracle.py)
         "scene_undistort.hip": ["-ffp-contract=off"],
         # train_log.hip: no contraction, so the fp64 running means (two products and a sum) and the panels' fp32 chains round as their
         # restatement (tests/log_oracle.py)
         "train_log.hip": ["-ffp-contract=off"],
         # mesh_simplify.hip: no contraction, so the fp32 cell index and the fp64 quadric sums and solve round as their restatement
         # (tests/simplify_oracle.py) and the simplified mesh comes out bit for bit
         "mesh_simplify.hip": ["-ffp-contract=off"],
         # mesh_texture.hip: no contraction, so the layout, baking, resolve and textured shading (fp32) round as their restatement
         # (tests/texture_oracle.py) and the atlas comes out bit for bit
         "mesh_texture.hip": ["-ffp-contract=off"],
         # mesh_smooth.hip: no contraction, so a filter step's fp64 mean and blend (a product, then a sum) round as their restatement
         # (tests/smooth_oracle.py) and the smoothed vertices come out bit for bit
         "mesh_smooth.hip": ["-ffp-contract=off"],
         # mesh_repair.hip: no contraction, so a fill centroid's fp64 sum and division round as their restatement
         # (tests/repair_oracle.py) and the repaired vertices come out bit for bit
         "mesh_repair.hip": ["-ffp-contract=off"]}
HEADERS = ["surfel_common.h", "surfel_kernels.h", "surfel_tile_walk.h", "surfel_contrib_kernel.h", os.path.join("..", "..", "include", "surfel_contrib.h"), "surfel_select_kernel.h", os.path.join("..", "..", "include", "surfel_select.h"), "surfel_blend_bwd.h", "train_kernels.h", "train_loss_body.h", "train_post_body.h", os.path.join("..", "..", "include", "surfel_hip.h"), os.path.join("..", "..", "include", "surfel_debug.h"),
           os.path.join("..", "..", "include", "surfel_train.h"), "mesh_mc_table.h", "mesh_mc.h", "block_ops.h", "side_util.h", "carve.h", "mesh_topology.h", os.path.join("..", "..", "include", "surfel_mesh.h"),
           os.path.join("..", "..", "include", "surfel_mesh_unbounded.h"), os.path.join("..", "..", "include", "surfel_eval.h"),
           os.path.join("..", "..", "include", "surfel_eval_tnt.h"), os.path.join("..", "..", "include", "surfel_metrics.h"),
           os.path.join("..", "..", "include", "surfel_scene.h"), "vis_turbo_table.h", os.path.join("..", "..", "include", "surfel_vis.h"),
           "vis_pixels.h", os.path.join("..", "..", "include", "surfel_view.h"), os.path.join("..", "..", "include", "surfel_cull.h"),
           "jpeg_tables.h", os.path.join("..", "..", "include", "surfel_jpeg.h"), os.path.join("..", "..", "include", "surfel_png.h"),
           os.path.join("..", "..", "include", "surfel_jpegdec.h"), os.path.join("..", "..", "include", "surfel_undistort.h"),
           "log_jet_table.h", os.path.join("..", "..", "include", "surfel_log.h"), "mesh_raster.h", "mesh_sample.h",
           os.path.join("..", "..", "include", "surfel_meshview.h"), os.path.join("..", "..", "include", "surfel_simplify.h"),
           os.path.join("..", "..", "include", "surfel_texture.h"), os.path.join("..", "..", "include", "surfel_smooth.h"),
           os.path.join("..", "..", "include", "surfel_repair.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-Wall", "-Wno-unused-result"]


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def build_variant(tag, defines, verbose=False):
    """Diagnostic twin lib/libsurfel_hip_<tag>.so with extra -D flags (e.g. -DSCAN_TIMING); loaded only through SURFEL_LIB."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    bdir = os.path.join(HERE, "build_" + tag)
    os.makedirs(bdir, exist_ok=True)
    os.makedirs(os.path.join(HERE, "lib"), exist_ok=True)
    lib = os.path.join(HERE, "lib", "libsurfel_hip_%s.so" % tag)
    objs = []
    for src in SOURCES:
        obj = os.path.join(bdir, src + ".o")
        objs.append(obj)
        cmd = [hipcc] + FLAGS + list(defines) + EXTRA.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs)
    return lib


def build(force=False, verbose=False, ieee=False):
    """ieee=True: the diagnostic twin lib/libsurfel_hip_ieee.so (-DSURFEL_IEEE_MATH: IEEE division and libm expf in the blend kernels);
    never loaded by the product (surfel_native loads it only when SURFEL_LIB points at it)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(os.path.join(HERE, "lib"), exist_ok=True)
    bdir = os.path.join(HERE, "build_ieee" if ieee else "build")
    os.makedirs(bdir, exist_ok=True)
    LIB = os.path.join(HERE, "lib", "libsurfel_hip_ieee.so" if ieee else "libsurfel_hip.so")
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs = []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        obj = os.path.join(bdir, src + ".o")
        objs.append(obj)
        if force or _stale(obj, [sp] + hdrs):
            cmd = [hipcc] + FLAGS + (["-DSURFEL_IEEE_MATH"] if ieee else []) + EXTRA.get(src, []) + ["-c", sp, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
    if force or _stale(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    if "--variant" in sys.argv:      # python build.py --variant TAG -DFOO -DBAR=1
        k = sys.argv.index("--variant")
        print(build_variant(sys.argv[k + 1], sys.argv[k + 2:], verbose=False))
        sys.exit(0)
    print(build(force="--force" in sys.argv, verbose=True, ieee="--ieee" in sys.argv))
