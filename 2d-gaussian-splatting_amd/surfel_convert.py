"""python surfel_convert.py -s CAPTURE [--quality 95]: the undistortion step of the reference's `convert.py --skip_matching`, without
COLMAP (UNDISTORT.md).

Reads CAPTURE/input/ and CAPTURE/distorted/sparse/0 (what COLMAP's mapper left there), undistorts every image on the device
(surfel_undistort), and writes CAPTURE/images/NAME — .png through surfel_png.png_bytes, .jpg / .jpeg through surfel_video.jpeg_bytes —
and CAPTURE/sparse/0/{cameras,images,points3D}.bin: PINHOLE cameras, the same poses with no 2-D observations, the points copied.  The
result is a capture the default reader (surfel_scene.read_colmap_scene) loads.  Out of scope: --resize pyramids (the -r rule
resamples on load, and ImageMagick's filter cannot be matched here), feature matching and mapping, blank_pixels > 0, and a re-centred
principal point.
"""
import argparse
import os
import struct
import sys

import torch

import surfel_scene
import surfel_undistort


def _write_cameras_bin(path, cams):
    """cams: [(id, width, height, (fx, fy, cx, cy))], all written as PINHOLE (model id 1)"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cams)))
        for cid, w, h, params in cams:
            f.write(struct.pack("<iiQQ4d", cid, 1, w, h, *params))


def _write_images_bin(path, images):
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(images)))
        for im in images:
            f.write(struct.pack("<i7di", im.id, *im.qvec, *im.tvec, im.camera_id) + im.name.encode("utf-8") + b"\x00" + struct.pack("<Q", 0))


def _copy_points(src_dir, dst_path):
    """points3D.bin byte for byte; a text model's points are packed into the binary layout (id, xyz, rgb, error, track)"""
    if os.path.exists(os.path.join(src_dir, "points3D.bin")):
        with open(os.path.join(src_dir, "points3D.bin"), "rb") as f, open(dst_path, "wb") as g:
            g.write(f.read())
        return
    rows = [line.split() for line in surfel_scene._data_lines(os.path.join(src_dir, "points3D.txt"))]
    with open(dst_path, "wb") as g:
        g.write(struct.pack("<Q", len(rows)))
        for e in rows:
            track = [int(v) for v in e[8:]]
            g.write(struct.pack("<Q3d3Bd", int(e[0]), *[float(v) for v in e[1:4]], *[int(v) for v in e[4:7]], float(e[7])))
            g.write(struct.pack("<Q", len(track) // 2) + struct.pack("<%di" % len(track), *track))


def _encode(u8, ext, quality):
    if ext == ".png":
        import surfel_png
        if u8.shape[2] == 4:
            raise ValueError("an RGBA image cannot be written: the PNG encoder takes 1 or 3 channels")
        return surfel_png.png_bytes(u8)
    import surfel_video
    if u8.shape[2] != 3:
        raise ValueError("a %d-channel image cannot be written as JPEG: the encoder takes RGB" % u8.shape[2])
    return surfel_video.jpeg_bytes(u8, quality)


def convert(source_path, quality=95, device="cuda", say=print):
    """-> number of images written"""
    from PIL import Image
    src_sparse = os.path.join(source_path, "distorted", "sparse", "0")
    src_images = os.path.join(source_path, "input")
    if os.path.exists(os.path.join(src_sparse, "cameras.bin")) and os.path.exists(os.path.join(src_sparse, "images.bin")):
        extr, intr = surfel_scene.read_images_bin(os.path.join(src_sparse, "images.bin")), surfel_scene.read_cameras_bin(os.path.join(src_sparse, "cameras.bin"))
    else:
        extr, intr = surfel_scene.read_images_txt(os.path.join(src_sparse, "images.txt")), surfel_scene.read_cameras_txt(os.path.join(src_sparse, "cameras.txt"))
    for im in extr.values():
        ext = os.path.splitext(im.name)[1].lower()
        if ext not in (".png", ".jpg", ".jpeg"):
            raise ValueError("%s: only .png, .jpg and .jpeg images can be written" % im.name)
    cams = {}      # id -> (q or None, (W2, H2, fx, fy, cx2, cy2))
    for cid, cam in intr.items():
        if cam.model == "SIMPLE_PINHOLE":
            cams[cid] = (None, (cam.width, cam.height, cam.params[0], cam.params[0], cam.params[1], cam.params[2]))
        elif cam.model == "PINHOLE":
            cams[cid] = (None, (cam.width, cam.height) + tuple(cam.params))
        else:
            q = surfel_undistort.distortion_params(cam.model, cam.params)
            cams[cid] = (q, surfel_undistort.undistorted_camera(q, cam.width, cam.height))
    dst_sparse, dst_images = os.path.join(source_path, "sparse", "0"), os.path.join(source_path, "images")
    os.makedirs(dst_sparse, exist_ok=True)
    os.makedirs(dst_images, exist_ok=True)
    for im in extr.values():
        q, (W2, H2, fx, fy, cx2, cy2) = cams[im.camera_id]
        name = os.path.basename(im.name)
        path = os.path.join(src_images, name)
        if q is None:      # a pinhole camera's image is already what the trainer takes
            with open(path, "rb") as f, open(os.path.join(dst_images, name), "wb") as g:
                g.write(f.read())
            continue
        with Image.open(path) as pil:
            u8 = surfel_scene.decode(pil)
        cam = intr[im.camera_id]
        if (u8.shape[1], u8.shape[0]) != (cam.width, cam.height):
            raise ValueError("%s is %d x %d, but its COLMAP camera (%d) is %d x %d" % (path, u8.shape[1], u8.shape[0], cam.id, cam.width, cam.height))
        out = surfel_undistort.undistort(torch.from_numpy(u8).to(device), q, (fx, fy, cx2, cy2), (W2, H2))
        try:
            data = _encode(out, os.path.splitext(name)[1].lower(), quality)
        except ValueError as e:
            raise ValueError("%s: %s" % (path, e)) from None
        with open(os.path.join(dst_images, name), "wb") as g:
            g.write(data)
    _write_cameras_bin(os.path.join(dst_sparse, "cameras.bin"), [(cid, c[1][0], c[1][1], c[1][2:]) for cid, c in cams.items()])
    _write_images_bin(os.path.join(dst_sparse, "images.bin"), list(extr.values()))
    _copy_points(src_sparse, os.path.join(dst_sparse, "points3D.bin"))
    say("%d images and %d cameras undistorted into %s" % (len(extr), len(cams), source_path))
    return len(extr)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Undistort a COLMAP capture (input/ + distorted/sparse/0 -> images/ + sparse/0): convert.py --skip_matching "
                                             "without COLMAP; see UNDISTORT.md for what is out of scope")
    ap.add_argument("--source_path", "-s", required=True, type=str)
    ap.add_argument("--quality", default=95, type=int, help="JPEG quality of the .jpg / .jpeg images written, 1 .. 100")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args(argv)
    convert(os.path.abspath(args.source_path), args.quality, say=(lambda *a: None) if args.quiet else print)
    return 0


if __name__ == "__main__":
    sys.exit(main())
