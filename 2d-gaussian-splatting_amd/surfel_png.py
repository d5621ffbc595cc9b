"""PNG frames on MI355X — the encoder behind the per-frame exports (the reference's save_img_u8 / export_image write PNG and its
metrics read PNG).  PNG.md states the rules.

The frames never leave the device as pixels: a PNG encoder in HIP (surfel_png_encode of libsurfel_hip.so, include/surfel_png.h) turns
each uint8 [H, W, 1 | 3] frame into a complete PNG file in device memory, and only those bytes travel to the host.  No host encoder is
involved.
"""
import threading

import torch

import surfel_native as _n

_n.load()


def capacity(H, W, C):
    """surfel_png_capacity: an upper bound of the file size of an H x W x C frame"""
    return int(_n.call(None, "surfel_png_capacity", int(H), int(W), int(C)))


def scratch_bytes(H, W, C):
    """surfel_png_scratch_bytes"""
    return int(_n.call(None, "surfel_png_scratch_bytes", int(H), int(W), int(C)))


def _frame(img):
    img = _n.device_tensor("surfel_png", img)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] not in (1, 3):
        raise ValueError("surfel_png: a uint8 [H, W, 1 or 3] frame expected, got %s %s" % (img.dtype, tuple(img.shape)))
    return img.detach().contiguous()


# one scratch buffer per (device, stream) and frame shape: the encoder's launches are ordered on that stream, so consecutive frames of a
# loop may share it; a frame loop allocates nothing after its first frame
_cache = {}
_cache_lock = threading.Lock()
_CACHE_ENTRIES = 8


def _cached_scratch(device, shape, nbytes):
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, shape)
    with _cache_lock:
        buf = _cache.get(key)
        if buf is None:
            while len(_cache) >= _CACHE_ENTRIES:
                _cache.pop(next(iter(_cache)))
            buf = _cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return buf


def encode_png(img, out=None, scratch=None, size=None):
    """uint8 [H, W, 1 | 3] on the device -> (buffer, size): a uint8 device tensor whose first int(size) bytes are the PNG file, and the
    int64 [1] device tensor that holds that length (surfel_png_encode).  Nothing waits for the device.
    out: a contiguous uint8 device tensor of at least capacity(H, W, C) elements to write into (any byte alignment); no byte at or
    beyond the file's length is touched.  scratch: a contiguous uint8 device tensor of at least scratch_bytes(H, W, C) elements (8-byte
    aligned); by default one cached buffer per stream and shape.  size: an int64 [1] device tensor to reuse."""
    t = _frame(img)
    H, W, Cn = (int(v) for v in t.shape)
    cap, nscratch = capacity(H, W, Cn), scratch_bytes(H, W, Cn)
    out = _n.uint8_buffer("encode_png", out, cap, t.device, at_least=True)
    if scratch is None:
        scratch = _cached_scratch(t.device, (H, W, Cn), nscratch)
    else:
        _n.uint8_buffer("encode_png", scratch, nscratch, t.device, "scratch", at_least=True)
    if size is None:
        size = torch.empty(1, dtype=torch.int64, device=t.device)
    _n.call(t.device, "surfel_png_encode", H, W, Cn, t, out, out.numel(), size, scratch, scratch.numel())
    return out, size


def png_bytes(img):
    """The PNG file of a device frame as bytes: encode_png, then wait and copy exactly that many bytes."""
    buf, size = encode_png(img)
    return _n.file_bytes(buf, size)
