"""Captures on MI355X (SCENE.md): COLMAP and Blender (NeRF-synthetic) folders -> surfel_render.Camera lists + an initial GaussianModel,
with the reference's conventions (scene/__init__.py, scene/dataset_readers.py, scene/colmap_loader.py, utils/camera_utils.py) and the
model-folder layout (`input.ply`, `cameras.json`, `point_cloud/iteration_N`) that surfel_mesh.py and surfel_metrics.py read.

The host decodes (PIL) and parses; everything after the decode is HIP (include/surfel_scene.h): the decoded u8 HWC image is uploaded once,
resampled with Pillow's 8-bit BICUBIC arithmetic (bit for bit what `pil_image.resize(resolution)` returns), composited over the
background (Blender), and converted to planar fp32 with the alpha channel split off as the mask.  There is no host fallback: a CPU
tensor or device is refused by the library's boundary.  With decode="device" the JPEG files are decoded in HIP too (JPEGDEC.md): the
threads read and parse them, the file's bytes are what is uploaded, and a file the decoder does not take goes to PIL as before.
With undistort=True a COLMAP capture whose cameras are SIMPLE_RADIAL, RADIAL, OPENCV or FULL_OPENCV is undistorted on the way in
(UNDISTORT.md, surfel_undistort.py): the reader hands out the undistorted pinhole cameras, and every decoded image passes through the
undistortion kernel before anything else is done to it.
"""
import collections
import ctypes as C
import json
import math
import os
import random
import struct
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple

import numpy as np
import torch

import surfel_io
import surfel_native as _n
import surfel_undistort
from surfel_render import Camera, world2view

MAX_WORKERS = 8
LLFFHOLD = 8


# ------------------------------------------------------------------------------------------------ image path (HIP)
def resample_tables(in_size, out_size):
    """(ksize, bounds [out, 2] int32, coeffs [ksize, out] int32) of one axis: surfel_scene_resample_table (host, no device)."""
    ksize = _n.call(None, "surfel_scene_resample_table", int(in_size), int(out_size), None, None, 0)
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((ksize, out_size), np.int32)
    ip = C.POINTER(C.c_int)
    _n.call(None, "surfel_scene_resample_table", int(in_size), int(out_size), bounds.ctypes.data_as(ip), coeffs.ctypes.data_as(ip), coeffs.size)
    return ksize, bounds, coeffs


_TABLES = collections.OrderedDict()      # (in, out, device) -> (ksize, bounds, coeffs) on the device; a capture has one or two image sizes


def _device_tables(in_size, out_size, device):
    key = (int(in_size), int(out_size), str(device))
    hit = _TABLES.get(key)
    if hit is None:
        ksize, bounds, coeffs = resample_tables(in_size, out_size)
        hit = _TABLES[key] = (ksize, torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device))
        while len(_TABLES) > 16:
            _TABLES.popitem(last=False)
    return hit


def target_resolution(orig_w, orig_h, resolution, resolution_scale=1.0):
    """(width, height) an image is loaded at for the -r value (utils/camera_utils.py:22-39, in the same double operations: a 1601-wide
    image comes out 1599 wide at -r -1)."""
    if resolution in (1, 2, 4, 8):
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


def decode(pil_image):
    """The u8 [H, W, C] array (C = 1, 3, 4) of a PIL image of mode L, RGB or RGBA: the modes whose channels the reference resamples as
    8-bit planes.  Palette, 1-bit, 16-bit, float and LA images are refused (PIL resamples them by other rules)."""
    if isinstance(pil_image, np.ndarray):
        a = pil_image
    else:
        if pil_image.mode not in ("L", "RGB", "RGBA"):
            raise ValueError("image mode %r is not supported: convert it to L, RGB or RGBA (8 bits per channel)" % pil_image.mode)
        a = np.array(pil_image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError("expected an 8-bit image, got %s %s" % (a.dtype, a.shape))
    if a.ndim == 2:
        a = a[:, :, None]
    if a.shape[2] not in (1, 3, 4):
        raise ValueError("expected 1, 3 or 4 channels, got %d" % a.shape[2])
    return np.ascontiguousarray(a)


def _on_device(t):
    """the library's refusal (surfel_native.DevPtr), before a stream of a device that has none is asked for"""
    if t.device.type != "cuda":
        raise RuntimeError("libsurfel_hip: tensors must live on a HIP device (got %s)" % t.device)
    return t.contiguous()


def _u8_on_device(image, device):
    if torch.is_tensor(image):
        if image.dtype != torch.uint8 or image.dim() != 3:
            raise ValueError("expected a uint8 [H, W, C] tensor")
        return _on_device(image)
    return _on_device(torch.from_numpy(decode(image)).to(device))


def resample_h(src, W2):
    """u8 [H, W, C] on the device -> u8 [H, W2, C] (the intermediate Pillow rounds to between its two passes)"""
    src = _on_device(src)
    H, W, Cn = (int(v) for v in src.shape)
    ksize, bounds, coeffs = _device_tables(W, W2, src.device)
    out = torch.empty((H, W2, Cn), dtype=torch.uint8, device=src.device)
    _n.call(src.device, "surfel_scene_resample_h", H, W, Cn, W2, ksize, src, bounds, coeffs, out, None, None)
    return out


def load_image(image, resolution, device="cuda"):
    """image: a PIL image (L, RGB, RGBA), a u8 HWC array, or a u8 [H, W, C] tensor already on the device; resolution = (width, height).
    One upload of the decoded bytes, then the horizontal pass, the vertical pass and the conversion, the last of them writing
    (image [min(C, 3), H2, W2] fp32 = u8 / 255, mask [1, H2, W2] or None).  A pass is skipped when its axis keeps its size."""
    src = _u8_on_device(image, device)
    H, W, Cn = (int(v) for v in src.shape)
    W2, H2 = int(resolution[0]), int(resolution[1])
    dev = src.device
    planes = torch.empty((min(Cn, 3), H2, W2), dtype=torch.float32, device=dev)
    mask = torch.empty((1, H2, W2), dtype=torch.float32, device=dev) if Cn == 4 else None
    if W2 != W and H2 != H:
        src, W = resample_h(src, W2), W2
    if H2 != H:
        ksize, bounds, coeffs = _device_tables(H, H2, dev)
        _n.call(dev, "surfel_scene_resample_v", H, W, Cn, H2, ksize, src, bounds, coeffs, None, planes, mask)
    elif W2 != W:
        ksize, bounds, coeffs = _device_tables(W, W2, dev)
        _n.call(dev, "surfel_scene_resample_h", H, W, Cn, W2, ksize, src, bounds, coeffs, None, planes, mask)
    else:
        _n.call(dev, "surfel_scene_to_float", H, W, Cn, src, planes, mask)
    return planes, mask


def composite(rgba, white_background):
    """u8 [H, W, 4] on the device -> u8 [H, W, 3] over black or white (scene/dataset_readers.py:204-210: fp64, truncated)"""
    if rgba.dim() != 3 or rgba.shape[2] != 4 or rgba.dtype != torch.uint8:
        raise ValueError("expected a uint8 [H, W, 4] tensor")
    rgba = _on_device(rgba)
    out = torch.empty((rgba.shape[0], rgba.shape[1], 3), dtype=torch.uint8, device=rgba.device)
    _n.call(rgba.device, "surfel_scene_composite", int(rgba.shape[0]), int(rgba.shape[1]), int(bool(white_background)), rgba, out)
    return out


# ------------------------------------------------------------------------------------------------ records
class CameraInfo(NamedTuple):
    uid: int
    R: np.ndarray            # camera-to-world rotation
    T: np.ndarray            # world-to-camera translation
    FovY: float
    FovX: float
    image_path: str
    image_name: str
    width: int
    height: int
    composite: bool = False  # Blender: RGBA over the background before anything else
    distortion: np.ndarray = None   # undistort=True on a distorted COLMAP camera: q[12] of UNDISTORT.md; width, height and FoV above are the undistorted ones
    pinhole: tuple = None           # ... and the undistorted camera (fx, fy, cx2, cy2) the image is resampled into
    source_size: tuple = None       # ... and the (width, height) the COLMAP camera, and so the file, must have


class PointCloud(NamedTuple):
    points: np.ndarray
    colors: np.ndarray
    normals: np.ndarray


class SceneInfo(NamedTuple):
    point_cloud: PointCloud
    train_cameras: list
    test_cameras: list
    nerf_normalization: dict
    ply_path: str


def focal2fov(focal, pixels):
    return 2 * math.atan(pixels / (2 * focal))


def fov2focal(fov, pixels):
    return pixels / (2 * math.tan(fov / 2))


def qvec2rotmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * y ** 2 - 2 * z ** 2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x ** 2 - 2 * z ** 2, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x ** 2 - 2 * y ** 2]])


def nerfpp_norm(cam_infos):
    """{"translate", "radius"} of scene/dataset_readers.py:40-64: minus the mean camera centre, and 1.1 x the largest distance of a centre
    from it — on the fp32 world-to-view matrices, as there, so the numbers agree to the last digit."""
    centers = [np.linalg.inv(world2view(c.R, c.T))[:3, 3:4] for c in cam_infos]
    centers = np.hstack(centers)
    center = np.mean(centers, axis=1, keepdims=True)
    diagonal = np.max(np.linalg.norm(centers - center, axis=0, keepdims=True))
    return {"translate": -center.flatten(), "radius": diagonal * 1.1}


def camera_to_json(id, cam):
    """One cameras.json entry (utils/camera_utils.py:64-84): position / rotation = camera-to-world, fx / fy in pixels of width / height."""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = cam.R.transpose()
    Rt[:3, 3] = cam.T
    Rt[3, 3] = 1.0
    c2w = np.linalg.inv(Rt)
    return {"id": id, "img_name": cam.image_name, "width": cam.width, "height": cam.height, "position": c2w[:3, 3].tolist(),
            "rotation": [row.tolist() for row in c2w[:3, :3]], "fy": fov2focal(cam.FovY, cam.height), "fx": fov2focal(cam.FovX, cam.width)}


# ------------------------------------------------------------------------------------------------ COLMAP models
# model id -> (name, number of parameters); downstream accepts the two undistorted pinhole models, and with undistort=True those of
# surfel_undistort.MODELS
COLMAP_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8),
                 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}

ColmapCamera = collections.namedtuple("ColmapCamera", "id model width height params")
ColmapImage = collections.namedtuple("ColmapImage", "id qvec tvec camera_id name")


def _unpack(f, fmt):
    size = struct.calcsize(fmt)
    data = f.read(size)
    if len(data) != size:
        raise ValueError("truncated COLMAP file %s" % f.name)
    return struct.unpack(fmt, data)


def read_cameras_bin(path):
    cams = {}
    with open(path, "rb") as f:
        for _ in range(_unpack(f, "<Q")[0]):
            cid, model_id, w, h = _unpack(f, "<iiQQ")
            if model_id not in COLMAP_MODELS:
                raise ValueError("%s: unknown camera model id %d" % (path, model_id))
            name, npar = COLMAP_MODELS[model_id]
            cams[cid] = ColmapCamera(cid, name, int(w), int(h), np.array(_unpack(f, "<%dd" % npar)))
    return cams


def read_images_bin(path):
    images = {}
    with open(path, "rb") as f:
        for _ in range(_unpack(f, "<Q")[0]):
            rec = _unpack(f, "<i7di")
            name = bytearray()
            while True:
                ch = f.read(1)
                if ch in (b"\x00", b""):
                    break
                name += ch
            npts = _unpack(f, "<Q")[0]
            f.seek(24 * npts, 1)          # the 2-D observations (x, y, point3D id) are not used
            images[rec[0]] = ColmapImage(rec[0], np.array(rec[1:5]), np.array(rec[5:8]), rec[8], name.decode("utf-8"))
    return images


def read_points3d_bin(path):
    with open(path, "rb") as f:
        n = _unpack(f, "<Q")[0]
        xyz, rgb = np.empty((n, 3)), np.empty((n, 3))
        for i in range(n):
            rec = _unpack(f, "<Q3d3Bd")
            xyz[i], rgb[i] = rec[1:4], rec[4:7]
            f.seek(8 * _unpack(f, "<Q")[0], 1)      # the track
    return xyz, rgb


def _data_lines(path):
    with open(path, "r") as f:
        for line in f:
            line = line.strip()
            if line and not line.startswith("#"):
                yield line


def read_cameras_txt(path):
    cams = {}
    for line in _data_lines(path):
        e = line.split()
        cams[int(e[0])] = ColmapCamera(int(e[0]), e[1], int(e[2]), int(e[3]), np.array([float(v) for v in e[4:]]))
    return cams


def read_images_txt(path):
    images = {}
    with open(path, "r") as f:
        while True:
            line = f.readline()
            if not line:
                break
            line = line.strip()
            if line and not line.startswith("#"):
                e = line.split()
                images[int(e[0])] = ColmapImage(int(e[0]), np.array([float(v) for v in e[1:5]]), np.array([float(v) for v in e[5:8]]), int(e[8]), e[9])
                f.readline()              # the image's 2-D observations
    return images


def read_points3d_txt(path):
    rows = [line.split() for line in _data_lines(path)]
    xyz = np.array([[float(v) for v in e[1:4]] for e in rows]).reshape(-1, 3)
    rgb = np.array([[float(int(v)) for v in e[4:7]] for e in rows]).reshape(-1, 3)
    return xyz, rgb


def store_points_ply(path, xyz, rgb):
    """points3D.ply as the reference stores it: float x y z, zero normals, uchar red green blue"""
    rec = np.zeros(xyz.shape[0], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                        ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for k, n in enumerate(("x", "y", "z")):
        rec[n] = xyz[:, k]
    for k, n in enumerate(("red", "green", "blue")):
        rec[n] = rgb[:, k]
    surfel_io.write_ply_records(path, rec)


def fetch_points_ply(path):
    v = surfel_io.read_ply(path)
    return PointCloud(points=np.vstack([v["x"], v["y"], v["z"]]).T, colors=np.vstack([v["red"], v["green"], v["blue"]]).T / 255.0,
                      normals=np.vstack([v["nx"], v["ny"], v["nz"]]).T)


def _image_size(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.size


def _has_model(sparse):
    return any(os.path.exists(os.path.join(sparse, name)) for name in ("cameras.bin", "cameras.txt"))


def read_colmap_scene(path, images="images", eval=False, llffhold=LLFFHOLD, undistort=False):
    """scene/dataset_readers.py:132-177: sparse/0/{cameras,images,points3D}.bin (else .txt), cameras sorted by image name, every
    llffhold-th of them held out under eval, points3D converted to points3D.ply on first open.
    undistort=True (UNDISTORT.md): a camera of a model in surfel_undistort.MODELS yields the undistorted pinhole camera's width, height
    and FoV, with the distortion carried along for load_cameras; pinhole cameras are untouched.  The model is sparse/0, else
    distorted/sparse/0, and the images are the `images` folder, else input/ (convert.py's layout before its undistortion step)."""
    sparse = os.path.join(path, "sparse/0")
    if undistort and not _has_model(sparse) and _has_model(os.path.join(path, "distorted/sparse/0")):
        sparse = os.path.join(path, "distorted/sparse/0")
    if os.path.exists(os.path.join(sparse, "images.bin")) and os.path.exists(os.path.join(sparse, "cameras.bin")):
        extr, intr = read_images_bin(os.path.join(sparse, "images.bin")), read_cameras_bin(os.path.join(sparse, "cameras.bin"))
    else:
        extr, intr = read_images_txt(os.path.join(sparse, "images.txt")), read_cameras_txt(os.path.join(sparse, "cameras.txt"))
    folder = os.path.join(path, "images" if images is None else images)
    if undistort and not os.path.isdir(folder):
        folder = os.path.join(path, "input")
    infos = []
    undistorted = {}      # COLMAP camera id -> (q, (W2, H2, fx, fy, cx2, cy2)): the rule runs once per camera
    for im in extr.values():
        cam = intr[im.camera_id]
        width, height, extra = cam.width, cam.height, {}
        if cam.model == "SIMPLE_PINHOLE":
            fx = fy = cam.params[0]
        elif cam.model == "PINHOLE":
            fx, fy = cam.params[0], cam.params[1]
        elif not undistort:
            raise ValueError("COLMAP camera model %s is not supported: only undistorted captures (PINHOLE or SIMPLE_PINHOLE) are; run "
                             "COLMAP's image_undistorter first, or pass undistort=True (--undistort, UNDISTORT.md)" % cam.model)
        elif cam.model not in surfel_undistort.MODELS:
            raise ValueError("COLMAP camera model %s is not supported, with or without undistort: only %s can be undistorted here (the "
                             "fisheye, FOV and thin-prism models need atan)" % (cam.model, ", ".join(surfel_undistort.MODELS)))
        else:
            if cam.id not in undistorted:
                q = surfel_undistort.distortion_params(cam.model, cam.params)
                undistorted[cam.id] = (q, surfel_undistort.undistorted_camera(q, cam.width, cam.height))
            q, (width, height, fx, fy, cx2, cy2) = undistorted[cam.id]
            extra = dict(distortion=q, pinhole=(fx, fy, cx2, cy2), source_size=(cam.width, cam.height))
        image_path = os.path.join(folder, os.path.basename(im.name))
        infos.append(CameraInfo(uid=cam.id, R=np.transpose(qvec2rotmat(im.qvec)), T=np.array(im.tvec), FovY=focal2fov(fy, height),
                                FovX=focal2fov(fx, width), image_path=image_path, image_name=os.path.basename(image_path).split(".")[0],
                                width=width, height=height, **extra))
    infos = sorted(infos, key=lambda c: c.image_name)
    train = [c for i, c in enumerate(infos) if not eval or i % llffhold != 0]
    test = [c for i, c in enumerate(infos) if eval and i % llffhold == 0]
    ply_path = os.path.join(sparse, "points3D.ply")
    if not os.path.exists(ply_path):
        if os.path.exists(os.path.join(sparse, "points3D.bin")):
            xyz, rgb = read_points3d_bin(os.path.join(sparse, "points3D.bin"))
        else:
            xyz, rgb = read_points3d_txt(os.path.join(sparse, "points3D.txt"))
        store_points_ply(ply_path, xyz, rgb)
    return SceneInfo(fetch_points_ply(ply_path), train, test, nerfpp_norm(train), ply_path)


# ------------------------------------------------------------------------------------------------ Blender (NeRF-synthetic)
def read_transforms(path, transforms_file, extension=".png"):
    """scene/dataset_readers.py:179-219 without the pixels: the image is composited on the device when it is loaded."""
    with open(os.path.join(path, transforms_file)) as f:
        contents = json.load(f)
    fovx = contents["camera_angle_x"]
    infos = []
    for idx, frame in enumerate(contents["frames"]):
        image_path = os.path.join(path, frame["file_path"] + extension)
        c2w = np.array(frame["transform_matrix"], dtype=np.float64)
        c2w[:3, 1:3] *= -1                 # OpenGL / Blender axes (y up, z back) -> COLMAP's (y down, z forward)
        w2c = np.linalg.inv(c2w)
        w, h = _image_size(image_path)
        infos.append(CameraInfo(uid=idx, R=np.transpose(w2c[:3, :3]), T=w2c[:3, 3], FovY=focal2fov(fov2focal(fovx, w), h), FovX=fovx,
                                image_path=image_path, image_name=os.path.splitext(os.path.basename(image_path))[0], width=w, height=h,
                                composite=True))
    return infos


def read_blender_scene(path, white_background=False, eval=False, seed=0, num_pts=100_000):
    """scene/dataset_readers.py:221-255.  The random initial points come from numpy's legacy generator seeded with `seed` (the reference
    draws them from the process-wide one)."""
    train = read_transforms(path, "transforms_train.json")
    test = read_transforms(path, "transforms_test.json")
    if not eval:
        train, test = train + test, []
    ply_path = os.path.join(path, "points3d.ply")
    if not os.path.exists(ply_path):
        rng = np.random.RandomState(seed)
        xyz = rng.random_sample((num_pts, 3)) * 2.6 - 1.3
        shs = rng.random_sample((num_pts, 3)) / 255.0
        store_points_ply(ply_path, xyz, (shs * 0.28209479177387814 + 0.5) * 255)
    return SceneInfo(fetch_points_ply(ply_path), train, test, nerfpp_norm(train), ply_path)


def read_scene_info(source_path, images="images", white_background=False, eval=False, seed=0, undistort=False):
    """Scene-type detection of scene/__init__.py:43-49; with undistort=True distorted/sparse alone also makes a COLMAP capture."""
    if os.path.exists(os.path.join(source_path, "sparse")) or (undistort and os.path.exists(os.path.join(source_path, "distorted", "sparse"))):
        return read_colmap_scene(source_path, images, eval, undistort=undistort)
    if os.path.exists(os.path.join(source_path, "transforms_train.json")):
        return read_blender_scene(source_path, white_background, eval, seed=seed)
    raise ValueError("could not recognize the scene type of %s: neither sparse/ (COLMAP) nor transforms_train.json (Blender)" % source_path)


# ------------------------------------------------------------------------------------------------ Scene
def search_max_iteration(folder):
    return max(int(name.split("_")[-1]) for name in os.listdir(folder))


def _decode_file(info):
    from PIL import Image
    with Image.open(info.image_path) as im:
        return decode(im.convert("RGBA") if info.composite else im)


def _pillow_bytes(data):
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return decode(im)


def _read_file(info):
    """decode="device": ("device", file bytes, descriptor) for a JPEG file the device decoder takes (surfel_jpegdec.parse: no entropy
    decoding here), ("fallback", pixels) for a JPEG file it does not take, ("host", pixels) for everything else."""
    import surfel_jpegdec
    if info.composite or os.path.splitext(info.image_path)[1].lower() not in (".jpg", ".jpeg"):
        return ("host", _decode_file(info))
    with open(info.image_path, "rb") as f:
        data = f.read()
    desc = surfel_jpegdec.parse(data)
    if desc is None:
        return ("fallback", _pillow_bytes(data))
    return ("device", data, desc)


def _decoded(infos, workers, decode_file=_decode_file):
    """decoded images in camera order; at most 2 x workers of them are in flight"""
    workers = max(1, min(int(workers), MAX_WORKERS))
    with ThreadPoolExecutor(workers) as pool:
        pending = collections.deque()
        it = iter(infos)
        for info in it:
            pending.append(pool.submit(decode_file, info))
            if len(pending) >= 2 * workers:
                break
        while pending:
            yield pending.popleft().result()
            for info in it:
                pending.append(pool.submit(decode_file, info))
                break


_warned_large = False


def load_cameras(infos, resolution=-1, white_background=False, data_device="cuda", workers=4, decode="host", *, decode_options=None):
    """surfel_render.Camera list of utils/camera_utils.py:41-62 (cameraList_from_camInfos): the decode runs on `workers` threads, the
    device work on the calling thread in camera order.  decode="device" (JPEGDEC.md): the threads only read and parse .jpg / .jpeg
    files, and the calling thread uploads each file and decodes it on the device (surfel_jpegdec.decode_jpeg); a file the decoder does not take, or reports as not converged or damaged, is decoded by Pillow as with
    decode="host".  An info that carries a distortion (read_colmap_scene(undistort=True)) has its decoded image undistorted on the device
    first (surfel_undistort.undistort); the -r rule and the size warning then see the undistorted size.  The cameras do not depend on
    `decode` or `workers`.  decode_options (keyword only, for the tests: Scene and the
    CLIs do not pass it): decode_jpeg's subseq_bits / max_rounds, to make the subsequences short or the rounds run out."""
    global _warned_large
    if decode not in ("host", "device"):
        raise ValueError("decode must be 'host' or 'device', got %r" % (decode,))
    cams = []
    fallbacks = 0
    for id, (info, item) in enumerate(zip(infos, _decoded(infos, workers, _read_file if decode == "device" else _decode_file))):
        u8 = item
        if decode == "device":
            u8 = item[1]
            fallbacks += item[0] == "fallback"
            if item[0] == "device":
                import surfel_jpegdec
                try:
                    u8 = surfel_jpegdec.decode_jpeg(item[1], data_device, desc=item[2], **(decode_options or {}))
                except surfel_jpegdec.JpegNotDecoded:
                    u8, fallbacks = _pillow_bytes(item[1]), fallbacks + 1
        if info.distortion is not None:
            if (int(u8.shape[1]), int(u8.shape[0])) != tuple(info.source_size):
                raise ValueError("%s is %d x %d, but its COLMAP camera (%d) is %d x %d: the images are not the ones the model was built on"
                                 % (info.image_path, u8.shape[1], u8.shape[0], info.uid, info.source_size[0], info.source_size[1]))
            u8 = u8 if torch.is_tensor(u8) else torch.from_numpy(u8).to(data_device)
            u8 = surfel_undistort.undistort(u8, info.distortion, info.pinhole, (info.width, info.height))
        h, w = u8.shape[:2]
        if resolution == -1 and w > 1600 and not _warned_large:
            print("[ INFO ] Encountered quite large input images (>1.6K pixels width), rescaling to 1.6K.\n "
                  "If this is not desired, please explicitly specify '--resolution/-r' as 1")
            _warned_large = True
        src = u8 if torch.is_tensor(u8) else torch.from_numpy(u8).to(data_device)
        if info.composite:
            src = composite(src, white_background)
        image, mask = load_image(src, target_resolution(w, h, resolution), data_device)
        cams.append(Camera(colmap_id=info.uid, R=info.R, T=info.T, FoVx=info.FovX, FoVy=info.FovY, image=image, gt_alpha_mask=mask,
                           image_name=info.image_name, uid=id, data_device=data_device))
    if fallbacks:
        print("[ INFO ] %d of %d images: JPEG files outside the device decoder's scope (or reported not converged / damaged), decoded by Pillow"
              % (fallbacks, len(cams)))
    return cams


class Scene:
    """scene/__init__.py:21-92 for one resolution scale.  On a fresh run writes input.ply and cameras.json (test cameras first, then train,
    ids by position) into model_path; load_iteration (-1: the latest) loads point_cloud/iteration_N instead of initialising from the
    capture's points.  Results do not depend on `workers`.  undistort=True: a distorted COLMAP capture is undistorted while it is loaded
    (UNDISTORT.md), and cameras.json carries the undistorted sizes and focal lengths."""

    def __init__(self, source_path, model_path, images="images", resolution=-1, white_background=False, eval=False, data_device="cuda",
                 load_iteration=None, shuffle=True, seed=0, workers=4, gaussians=None, sh_degree=3, decode="host", undistort=False):
        from surfel_model import GaussianModel
        self.model_path = model_path
        self.loaded_iter = None
        if load_iteration:
            self.loaded_iter = search_max_iteration(os.path.join(model_path, "point_cloud")) if load_iteration == -1 else load_iteration
        info = read_scene_info(source_path, images, white_background, eval, seed, undistort=undistort)
        train, test = list(info.train_cameras), list(info.test_cameras)
        if not self.loaded_iter:
            os.makedirs(model_path, exist_ok=True)
            with open(info.ply_path, "rb") as src, open(os.path.join(model_path, "input.ply"), "wb") as dst:
                dst.write(src.read())
            with open(os.path.join(model_path, "cameras.json"), "w") as f:
                json.dump([camera_to_json(id, cam) for id, cam in enumerate(test + train)], f)
        if shuffle:
            rng = random.Random(seed)
            rng.shuffle(train)
            rng.shuffle(test)
        self.cameras_extent = float(info.nerf_normalization["radius"])
        self.train_cameras = load_cameras(train, resolution, white_background, data_device, workers, decode)
        self.test_cameras = load_cameras(test, resolution, white_background, data_device, workers, decode)
        self.gaussians = gaussians if gaussians is not None else GaussianModel(sh_degree, device=torch.device(data_device))
        if self.loaded_iter:
            self.gaussians.load_ply(os.path.join(model_path, "point_cloud", "iteration_%d" % self.loaded_iter, "point_cloud.ply"))
        else:
            self.gaussians.create_from_pcd(info.point_cloud, self.cameras_extent)

    def save(self, iteration):
        self.gaussians.save_ply(os.path.join(self.model_path, "point_cloud/iteration_%d" % iteration, "point_cloud.ply"))

    def getTrainCameras(self, scale=1.0):
        return self.train_cameras

    def getTestCameras(self, scale=1.0):
        return self.test_cameras
