"""Deterministic writers of tiny captures for the scene tests: a COLMAP model (binary or text) with its images, and a Blender
(NeRF-synthetic) folder.  numpy + PIL only; every byte follows from the seeds, and the images are PNG so every machine decodes the same."""
import json
import math
import os
import struct

import numpy as np

COLMAP_NAMES = ["view_07", "view_02", "view_09", "view_00", "view_05", "view_03", "view_08", "view_01", "view_04"]      # file order != name order
COLMAP_CAMERAS = {1: ("SIMPLE_PINHOLE", 53, 37, (61.25,)), 2: ("PINHOLE", 48, 36, (52.5, 51.75))}      # id -> model, width, height, focal(s)
BLENDER_SIZE = (40, 30)          # width, height
BLENDER_ANGLE_X = 0.6911112070083618


def noise_image(seed, h, w, c):
    """seeded noise with saturated 0 / 255 stripes (the worst case for the resampler's clipping)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
    a[::7] = 255
    a[3::7] = 0
    a[:, 2::9] = 0
    a[:, 5::9] = 255
    if c == 4:
        a[:, :, 3] = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        a[: h // 3, :, 3] = 255
        a[-(h // 4):, :, 3] = 0
    return a


def save_png(path, a):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a).save(path, "PNG")


def look_at_w2c(eye, target=(0.0, 0.0, 0.0), up=(0.0, -1.0, 0.0)):
    """world-to-camera rotation (rows = camera axes x right, y down, z forward) and translation"""
    eye = np.asarray(eye, np.float64)
    z = np.asarray(target, np.float64) - eye
    z /= np.linalg.norm(z)
    x = np.cross(-np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ eye


def rotmat_to_qvec(R):
    """unit quaternion (w, x, y, z), w >= 0, of a rotation matrix"""
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q = np.array(q)
    q /= np.linalg.norm(q)
    return -q if q[0] < 0 else q


def colmap_records(seed=11):
    """images [(id, qvec, tvec, camera id, file name, [(x, y, point id)])] in file order, points [(id, xyz, rgb, error, [(image, idx)])]"""
    rng = np.random.default_rng(seed)
    images = []
    for k, name in enumerate(COLMAP_NAMES):
        ang = 2 * math.pi * k / len(COLMAP_NAMES) + 0.1
        eye = (3.0 * math.cos(ang), 0.4 * math.sin(3 * ang) - 0.3, 3.0 * math.sin(ang) + 0.2 * k / 9)
        R, t = look_at_w2c(eye, target=(0.1, -0.05, 0.0))
        obs = [(float(rng.uniform(0, 50)), float(rng.uniform(0, 30)), int(rng.integers(-1, 200))) for _ in range(int(rng.integers(0, 5)))]
        images.append((10 + 3 * k, rotmat_to_qvec(R), t, 1 + k % 2, name + ".png", obs))
    points = []
    for p in range(200):
        track = [(int(images[int(rng.integers(0, 9))][0]), int(rng.integers(0, 4))) for _ in range(int(rng.integers(2, 6)))]
        points.append((7 + 2 * p, rng.normal(size=3) * 0.6, rng.integers(0, 256, size=3), float(rng.uniform(0.1, 2.0)), track))
    return images, points


def write_colmap(root, fmt="bin", seed=11):
    """root/images/*.png (camera 1: RGB, camera 2: RGBA) and root/sparse/0/{cameras,images,points3D}.<fmt>; returns (images, points)"""
    images, points = colmap_records(seed)
    sparse = os.path.join(root, "sparse", "0")
    os.makedirs(sparse, exist_ok=True)
    for k, im in enumerate(images):
        _, w, h, _ = COLMAP_CAMERAS[im[3]]
        save_png(os.path.join(root, "images", im[4]), noise_image(100 + k, h, w, 3 if im[3] == 1 else 4))
    model_ids = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1}
    if fmt == "bin":
        with open(os.path.join(sparse, "cameras.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(COLMAP_CAMERAS)))
            for cid, (model, w, h, params) in COLMAP_CAMERAS.items():
                full = params + (w / 2.0, h / 2.0)
                f.write(struct.pack("<iiQQ", cid, model_ids[model], w, h) + struct.pack("<%dd" % len(full), *full))
        with open(os.path.join(sparse, "images.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(images)))
            for iid, q, t, cid, name, obs in images:
                f.write(struct.pack("<i7di", iid, *q, *t, cid) + name.encode() + b"\x00" + struct.pack("<Q", len(obs)))
                for x, y, pid in obs:
                    f.write(struct.pack("<ddq", x, y, pid))
        with open(os.path.join(sparse, "points3D.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(points)))
            for pid, xyz, rgb, err, track in points:
                f.write(struct.pack("<Q3d3Bd", pid, *xyz, *[int(v) for v in rgb], err) + struct.pack("<Q", len(track)))
                for a, b in track:
                    f.write(struct.pack("<ii", a, b))
    else:
        with open(os.path.join(sparse, "cameras.txt"), "w") as f:
            f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
            for cid, (model, w, h, params) in COLMAP_CAMERAS.items():
                f.write("%d %s %d %d %s\n" % (cid, model, w, h, " ".join(repr(float(v)) for v in params + (w / 2.0, h / 2.0))))
        with open(os.path.join(sparse, "images.txt"), "w") as f:
            f.write("# Image list with two lines of data per image:\n")
            for iid, q, t, cid, name, obs in images:
                f.write("%d %s %d %s\n" % (iid, " ".join(repr(float(v)) for v in list(q) + list(t)), cid, name))
                f.write(" ".join("%r %r %d" % o for o in obs) + "\n")
        with open(os.path.join(sparse, "points3D.txt"), "w") as f:
            f.write("# 3D point list with one line of data per point:\n")
            for pid, xyz, rgb, err, track in points:
                f.write("%d %s %d %d %d %r %s\n" % (pid, " ".join(repr(float(v)) for v in xyz), rgb[0], rgb[1], rgb[2], err,
                                                   " ".join("%d %d" % t for t in track)))
    return images, points


def write_blender(root, seed=23):
    """root/{train,test}/r_N.png (RGBA) + transforms_train.json (4 frames) + transforms_test.json (2 frames)"""
    w, h = BLENDER_SIZE
    k = 0
    for split, count in (("train", 4), ("test", 2)):
        frames = []
        for i in range(count):
            ang = 2 * math.pi * k / 6 + 0.25
            eye = np.array([4.0 * math.cos(ang), 4.0 * math.sin(ang), 1.0 + 0.3 * k])
            z = eye / np.linalg.norm(eye)                 # Blender cameras look down -z
            x = np.cross([0.0, 0.0, 1.0], z)
            x /= np.linalg.norm(x)
            y = np.cross(z, x)
            c2w = np.eye(4)
            c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, eye
            frames.append({"file_path": "./%s/r_%d" % (split, i), "rotation": 0.012566370614359171, "transform_matrix": c2w.tolist()})
            save_png(os.path.join(root, split, "r_%d.png" % i), noise_image(seed + k, h, w, 4))
            k += 1
        with open(os.path.join(root, "transforms_%s.json" % split), "w") as f:
            json.dump({"camera_angle_x": BLENDER_ANGLE_X, "frames": frames}, f, indent=1)
    return root
