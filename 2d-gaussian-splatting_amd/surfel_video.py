"""Trajectory videos on MI355X — the part of the reference's `create_videos` (utils/render_utils.py:203-268) that turns the colour /
depth / normal frame sequences into video files.  VIDEO.md states the rules.

The frames never leave the device as pixels: a baseline JPEG encoder in HIP (surfel_jpeg_encode of libsurfel_hip.so,
include/surfel_jpeg.h) turns each 8-bit RGB frame into a JFIF file in device memory, and only those bytes — about a tenth of the raw
frame — travel to the host, where VideoWriter appends them as the chunks of a Motion-JPEG AVI 1.0 file.  No host encoder is involved.
"""
import queue
import struct
import threading

import torch

import surfel_frames as _f
import surfel_native as _n

_n.load()


def capacity(H, W):
    """surfel_jpeg_capacity: an upper bound of the file size of an H x W frame at any quality"""
    return int(_n.call(None, "surfel_jpeg_capacity", int(H), int(W)))


def scratch_bytes(H, W):
    """surfel_jpeg_scratch_bytes"""
    return int(_n.call(None, "surfel_jpeg_scratch_bytes", int(H), int(W)))


def _frame(img):
    img = _n.device_tensor("surfel_video", img)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("surfel_video: a uint8 [H, W, 3] frame expected, got %s %s" % (img.dtype, tuple(img.shape)))
    return img.detach().contiguous()


def encode_jpeg(img, quality=95, out=None, size=None):
    """uint8 [H, W, 3] RGB on the device -> (buffer, size): a uint8 device tensor whose first int(size) bytes are the JFIF file, and the
    int64 [1] device tensor that holds that length (surfel_jpeg_encode).  Nothing waits for the device.
    out: a contiguous uint8 device tensor of at least capacity(H, W) elements to write into (any byte alignment); no byte at or beyond
    the file's length is touched.  size: an int64 [1] device tensor to reuse."""
    t = _frame(img)
    H, W = int(t.shape[0]), int(t.shape[1])
    cap, nscratch = capacity(H, W), scratch_bytes(H, W)
    out = _n.uint8_buffer("encode_jpeg", out, cap, t.device, at_least=True)
    if size is None:
        size = torch.empty(1, dtype=torch.int64, device=t.device)
    scratch = torch.empty(nscratch, dtype=torch.uint8, device=t.device)
    _n.call(t.device, "surfel_jpeg_encode", H, W, t, int(quality), out, out.numel(), size, scratch, nscratch)
    return out, size


def jpeg_bytes(img, quality=95):
    """The JFIF file of a device frame as bytes: encode_jpeg, then wait and copy exactly that many bytes."""
    buf, size = encode_jpeg(img, quality)
    return _n.file_bytes(buf, size)


# ------------------------------------------------------------------------------------------------ Motion-JPEG AVI
_HDRL_BYTES = 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))      # 'hdrl' + avih + LIST strl (strh, strf)
_MOVI_FOURCC = 12 + 8 + _HDRL_BYTES + 8                         # file offset of the 'movi' fourcc


class VideoWriter:
    """Writes a Motion-JPEG AVI 1.0 file behind the renderer.  add_frame(uint8 [H, W, 3] device tensor) encodes the frame on the device
    into one of `ring` device buffers, copies the size word to pinned memory without blocking and records an event; one writer thread
    waits for the event, copies exactly that many bytes into pinned memory on a side stream and appends them as a `00dc` chunk, so frames
    reach the file in submission order.  add_frame blocks only when the whole ring is in flight.  add_jpeg(bytes) queues a finished
    JFIF file from the host the same way.  close() writes the index, patches the headers and re-raises the first exception the thread
    met; a file that would pass 2 GiB is refused at the frame that would (OpenDML is out of scope) and keeps the frames before it."""

    MAX_BYTES = 2 ** 31 - 1

    def __init__(self, path, H, W, fps=60, quality=95, ring=4):
        self.H, self.W, self.fps, self.quality = int(H), int(W), int(fps), int(quality)
        if self.H < 1 or self.W < 1 or self.fps < 1 or self.fps != fps or not 1 <= self.quality <= 100:
            raise ValueError("VideoWriter: H, W >= 1, an integer fps >= 1 and a quality in 1 .. 100 expected")
        self.ring = max(1, int(ring))
        self.path = path
        self.frames = 0                         # chunks in the file
        self.submitted = 0
        self._largest = 0
        self._file = open(path, "wb")
        self._file.write(self._headers(0, 0, 0))
        self._pos = _MOVI_FOURCC + 4
        self._index = []                        # (offset relative to the 'movi' fourcc, size)
        self._device = None                     # the device side (surfel_frames.EncodedStream), made by the first add_frame
        self._ring = _f.SlotRing(self.ring)
        self._queue = queue.Queue()
        self._thread = threading.Thread(target=self._run, name="video-writer", daemon=True)
        self._thread.start()

    wait_s = property(lambda self: self._ring.wait_s, doc="time add_frame() spent waiting for a free buffer")

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self._finish()
        return False

    # ---- the container
    def _headers(self, frames, movi_bytes, riff_bytes):
        rate = self._largest * self.fps
        avih = struct.pack("<14I", int(round(1e6 / self.fps)), min(rate, 0xFFFFFFFF), 0, 0x10, frames, 0, 1, self._largest, self.W, self.H, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, 1, self.fps, 0, frames, self._largest, 0xFFFFFFFF, 0, 0, 0,
                           min(self.W, 0xFFFF), min(self.H, 0xFFFF))
        strf = struct.pack("<IiiHH4sIiiII", 40, self.W, self.H, 1, 24, b"MJPG", self.W * self.H * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", 56) + strh + b"strf" + struct.pack("<I", 40) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", 56) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        assert len(hdrl) == _HDRL_BYTES
        return (b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl +
                b"LIST" + struct.pack("<I", movi_bytes) + b"movi")

    def _append(self, data):
        """one `00dc` chunk (thread side)"""
        n = len(data)
        end = self._pos + 8 + n + (n & 1) + 8 + 16 * (len(self._index) + 1)      # the file's length with this chunk and the index
        if end > self.MAX_BYTES:
            raise RuntimeError("VideoWriter: frame %d (%d bytes) would take %s past 2 GiB; the file keeps the %d frames before it "
                               "(AVI 1.0 holds no more; OpenDML is not written)" % (len(self._index), n, self.path, len(self._index)))
        self._file.write(b"00dc" + struct.pack("<I", n))
        self._file.write(data)
        if n & 1:
            self._file.write(b"\0")
        self._index.append((self._pos - _MOVI_FOURCC, n))
        self._pos += 8 + n + (n & 1)
        self._largest = max(self._largest, n)
        self.frames = len(self._index)

    # ---- the thread
    def _run(self):
        while True:
            item = self._queue.get()
            if item is None:
                return
            kind, payload, event = item
            try:
                if self._ring.error is None:
                    self._append(payload if kind == "bytes" else self._device.fetch(payload, event))
            except BaseException as e:
                self._ring.park(e)
            finally:
                if kind == "slot":
                    self._ring.release(payload)

    # ---- the caller's side
    def add_frame(self, img):
        t = _frame(img)
        if tuple(t.shape) != (self.H, self.W, 3):
            raise ValueError("VideoWriter.add_frame: a [%d, %d, 3] frame expected, got %s" % (self.H, self.W, tuple(t.shape)))
        if self._thread is None:
            raise RuntimeError("VideoWriter.add_frame after close()")
        if self._device is None:
            self._capacity = capacity(self.H, self.W)
            self._device = _f.EncodedStream(t.device, self.ring)
        slot = self._ring.acquire()
        try:
            event = self._device.encode(slot, self._capacity, lambda out, size: encode_jpeg(t, self.quality, out=out, size=size))
        except BaseException:
            self._ring.release(slot)
            raise
        self.submitted += 1
        self._queue.put(("slot", slot, event))

    def add_jpeg(self, data):
        """a finished JFIF file from the host (bytes), in order with the frames of add_frame"""
        if self._thread is None:
            raise RuntimeError("VideoWriter.add_jpeg after close()")
        self.submitted += 1
        self._queue.put(("bytes", bytes(data), None))

    def _finish(self):
        thread, self._thread = self._thread, None
        if thread is None:
            return
        self._queue.put(None)
        thread.join()
        f, self._file = self._file, None
        try:
            f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
            for off, n in self._index:
                f.write(b"00dc" + struct.pack("<III", 0x10, off, n))
            total = f.tell()
            f.seek(0)
            f.write(self._headers(len(self._index), self._pos - _MOVI_FOURCC, total - 8))
        finally:
            f.close()
            self._device = None

    def close(self):
        self._finish()
        self._ring.reraise()
