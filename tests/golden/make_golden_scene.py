"""Generate tests/golden/ref_scene.npz by IMPORTING the reference's own readers and running them on the captures of
tests/scene_scenes.py.  Runs only in the build container (needs /root/reference and Pillow); the .npz (arrays and JSON only) is committed.

Run: the reference's readColmapSceneInfo, readNerfSyntheticInfo, cameraList_from_camInfos and camera_to_JSON, with --eval on and off,
-r in {-1, 1, 2, 20} and the white background on and off (Blender).

Stand-ins, as in make_golden_train.py: torch.Tensor.cuda is the identity; `plyfile` is a small shim over surfel_io.  One more:
Pillow >= 12 refuses the reference's `Image.fromarray(int8 array, "RGB")` (scene/dataset_readers.py:210); the shim hands the same bytes
over as uint8, which is what older Pillow did with them.

Recorded: per camera R, T, FoVx / FoVy, width / height (of the CameraInfo), colmap id; per eval setting the order of both splits,
translate, radius and the cameras.json entries; per -r value every camera's original_image as the u8 array it is 1/255 of (checked here)
and its mask; the points of the point cloud (Blender: their number, the first 64 and column sums — 100 000 random points).
Images do not depend on --eval and are stored once; -r -1 is stored only where it differs from -r 1 (it does not for these sizes: checked).

Usage:  python tests/golden/make_golden_scene.py
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
for p in (REPO, os.path.join(REPO, "2d-gaussian-splatting_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import surfel_io          # noqa: E402
import scene_scenes as S  # noqa: E402

BLENDER_SEED = 0


class _PlyElement:
    def __init__(self, data):
        self.data = data

    @staticmethod
    def describe(data, name):
        assert name == "vertex"
        return _PlyElement(data)


class _PlyData:
    def __init__(self, elements):
        self.elements = elements

    def write(self, path):
        surfel_io.write_ply_records(path, self.elements[0].data)

    @staticmethod
    def read(path):
        return {"vertex": surfel_io.read_ply(path)}


for name in ["plyfile", "cv2", "matplotlib", "matplotlib.pyplot", "simple_knn", "simple_knn._C", "diff_surfel_rasterization"]:
    sys.modules[name] = types.ModuleType(name)
sys.modules["plyfile"].PlyData = _PlyData
sys.modules["plyfile"].PlyElement = _PlyElement
sys.modules["simple_knn._C"].distCUDA2 = lambda x: None
sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
torch.Tensor.cuda = lambda self, *a, **k: self

sys.path.insert(0, REF)
from scene import dataset_readers as DR                                      # noqa: E402
from utils.camera_utils import cameraList_from_camInfos, camera_to_JSON      # noqa: E402
from PIL import Image as _Image                                               # noqa: E402


class _ImageShim:
    """PIL.Image for scene/dataset_readers.py: fromarray takes an int8 array as the uint8 bytes it holds"""
    open = staticmethod(_Image.open)

    @staticmethod
    def fromarray(a, mode=None):
        if a.dtype == np.int8:
            a = a.view(np.uint8)
        return _Image.fromarray(a, mode) if a.ndim != 3 else _Image.fromarray(a)


DR.Image = _ImageShim


def u8_of(t):
    """the u8 array a [C, H, W] float tensor is 1/255 of, as [H, W, C]"""
    a = t.numpy()
    u8 = np.round(a * 255.0).astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32) / np.float32(255.0), a)
    return np.ascontiguousarray(u8.transpose(1, 2, 0))


def record_infos(out, tag, infos):
    out[tag + "/R"] = np.stack([np.asarray(c.R, np.float64) for c in infos])
    out[tag + "/T"] = np.stack([np.asarray(c.T, np.float64) for c in infos])
    out[tag + "/fov"] = np.array([[c.FovX, c.FovY] for c in infos], np.float64)
    out[tag + "/wh"] = np.array([[c.width, c.height] for c in infos], np.int64)
    out[tag + "/uid"] = np.array([c.uid for c in infos], np.int64)
    out[tag + "/names"] = np.array([c.image_name for c in infos])


def record_split(out, tag, info):
    out[tag + "/translate"] = np.asarray(info.nerf_normalization["translate"], np.float64)
    out[tag + "/radius"] = np.float64(info.nerf_normalization["radius"])
    out[tag + "/cameras_json"] = json.dumps([camera_to_JSON(i, c) for i, c in enumerate(list(info.test_cameras) + list(info.train_cameras))])


def record_images(out, tag, infos, keys, resolutions):
    by_r = {}
    for r in resolutions:
        args = types.SimpleNamespace(resolution=r, data_device="cpu")
        cams = cameraList_from_camInfos(infos, 1.0, args)
        by_r[r] = [(u8_of(c.original_image), None if c.gt_alpha_mask is None else u8_of(c.gt_alpha_mask)) for c in cams]
        for c, info in zip(cams, infos):
            assert np.array_equal(c.R, info.R) and np.array_equal(c.T, info.T) and c.FoVx == info.FovX and c.FoVy == info.FovY
    for a, b in zip(by_r[-1], by_r[1]):      # no image here is wider than 1600: -r -1 loads what -r 1 loads
        assert np.array_equal(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1]))
    for r in resolutions:
        if r == -1:
            continue
        for key, (img, mask) in zip(keys, by_r[r]):
            out["%s/r%d/%s/image" % (tag, r, key)] = img
            if mask is not None:
                out["%s/r%d/%s/mask" % (tag, r, key)] = mask


def main():
    out = {}
    resolutions = (-1, 1, 2, 20)
    with tempfile.TemporaryDirectory() as tmp:
        # ---------------------------------------------------------------- COLMAP
        root = os.path.join(tmp, "colmap")
        S.write_colmap(root, "bin")
        for ev in (False, True):
            info = DR.readColmapSceneInfo(root, "images", ev)
            tag = "colmap/eval%d" % ev
            out[tag + "/train"] = np.array([c.image_name for c in info.train_cameras])
            out[tag + "/test"] = np.array([c.image_name for c in info.test_cameras])
            record_split(out, tag, info)
            if not ev:
                record_infos(out, "colmap/cams", info.train_cameras)
                record_images(out, "colmap", info.train_cameras, [c.image_name for c in info.train_cameras], resolutions)
                out["colmap/points"] = np.asarray(info.point_cloud.points)
                out["colmap/colors_u8"] = np.round(np.asarray(info.point_cloud.colors) * 255.0).astype(np.uint8)
                assert np.array_equal(out["colmap/colors_u8"] / 255.0, info.point_cloud.colors) and not np.any(info.point_cloud.normals)
        # ---------------------------------------------------------------- Blender
        root = os.path.join(tmp, "blender")
        S.write_blender(root)
        for white in (False, True):
            for ev in (False, True):
                np.random.seed(BLENDER_SEED)
                info = DR.readNerfSyntheticInfo(root, white, ev)
                tag = "blender/eval%d" % ev
                everyone = list(info.train_cameras) + list(info.test_cameras)      # train frames, then test frames, either way
                if not white:
                    out[tag + "/n_train"] = np.int64(len(info.train_cameras))
                    record_split(out, tag, info)
                if not ev:
                    if not white:
                        record_infos(out, "blender/cams", everyone)
                        pts = np.asarray(info.point_cloud.points)
                        out["blender/points_n"] = np.int64(pts.shape[0])
                        out["blender/points_head"] = pts[:64]
                        out["blender/points_sum"] = pts.astype(np.float64).sum(0)
                        out["blender/colors_head"] = np.round(np.asarray(info.point_cloud.colors)[:64] * 255.0).astype(np.uint8)
                    record_images(out, "blender/white%d" % white, everyone, ["%d" % i for i in range(len(everyone))], resolutions)
        # the resolution rule itself, through the reference's loadCam on blank images (sizes only)
        widths = [53, 55, 1600, 1601, 1610, 1617, 1619, 1626, 3200, 5187]
        for r in (-1, 1, 2, 4, 8, 20, 777):
            sizes = []
            for w in widths:
                ci = DR.CameraInfo(uid=0, R=np.eye(3), T=np.zeros(3), FovY=1.0, FovX=1.0, image=_Image.new("L", (w, 701)), image_path="", image_name="",
                                   width=w, height=701)
                cam = cameraList_from_camInfos([ci], 1.0, types.SimpleNamespace(resolution=r, data_device="cpu"))[0]
                sizes.append((cam.image_width, cam.image_height))
            out["rule/r%d" % r] = np.array(sizes, np.int64)
        out["rule/widths"] = np.array(widths, np.int64)
    path = os.path.join(HERE, "ref_scene.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
