"""Training log on MI355X (LOG.md): the reference's TensorBoard log (train.py:115-119, 184-248 — prepare_output_and_logger and
training_report) as TensorBoard event files, written without the tensorboard package and without a host wait in the step.

- Step scalars: one small launch per step (surfel_log_append of include/surfel_log.h) turns the step's six device scalars into one
  32-byte record of a device ring; the running means of train.py:97-98 live on the device.  Every `block` steps the block's records are
  copied into pinned memory on the training stream, without blocking, and a writer thread waits for that copy, lets the library's host
  code frame the Events (surfel_log_encode_steps: ctypes releases the interpreter lock for the call) and appends them to the file.
- Panels: surfel_log_panel converts a map to 8-bit pixels on the device as TensorBoard's image summary would, and
  surfel_png.encode_png compresses them there: only PNG bytes reach the host.
- Reading back: read_events() and `python surfel_log.py MODEL_DIR [--csv] [--images DIR]` give the curves as CSV and the panels as PNG
  files to a user without TensorBoard; both checksums of every record are verified.

There is no host fallback for the device parts: a CPU tensor is refused.
"""
import ctypes as C
import os
import queue
import socket
import struct
import threading
import time

import numpy as np
import torch

import surfel_native as _n

RECORD_BYTES, STATE_BYTES, PANEL_SCRATCH_BYTES = 32, 32, 64      # include/surfel_log.h
RECORD_DTYPE = np.dtype([("iteration", "<i4"), ("points", "<i4"), ("reg_loss", "<f4"), ("total_loss", "<f4"), ("ema_dist", "<f4"),
                         ("ema_normal", "<f4"), ("raw_total", "<f4"), ("seq", "<u4")])
MODES = {"rgb": 0, "gray": 1, "normal": 2, "turbo_max": 3, "jet_minmax": 4}
STEP_TAGS = ("train_loss_patches/dist_loss", "train_loss_patches/normal_loss", "train_loss_patches/reg_loss",
             "train_loss_patches/total_loss", "iter_time", "total_points")
FILE_VERSION = "brain.Event:2"
PANEL_VIEWS = 5                     # training_report logs the panels of the first five views of a split (train.py:214)
# (panel, render_pkg key, mode) in the order training_report writes them (train.py:216-233)
PANELS = (("depth", "surf_depth", "turbo_max"), ("render", "render", "rgb"), ("rend_normal", "rend_normal", "normal"),
          ("surf_normal", "surf_normal", "normal"), ("rend_alpha", "rend_alpha", "gray"), ("rend_dist", "rend_dist", "jet_minmax"))


# ------------------------------------------------------------------------------------------------ wire format (host, rare events)
def _varint(v):
    v = int(v)
    if v < 0:
        raise ValueError("varint: negative value")
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def _field_bytes(number, data):
    return _varint(number << 3 | 2) + _varint(len(data)) + bytes(data)


def value_scalar(tag, x):
    """Summary.Value { tag, simple_value }"""
    return _field_bytes(1, tag.encode()) + b"\x15" + struct.pack("<f", float(x))


def value_image(tag, height, width, png):
    """Summary.Value { tag, image { height, width, colorspace 3, encoded_image_string } }"""
    img = b"\x08" + _varint(height) + b"\x10" + _varint(width) + b"\x18\x03" + _field_bytes(4, png)
    return _field_bytes(1, tag.encode()) + _field_bytes(4, img)


def event(wall_time, step=0, values=(), file_version=None):
    """A serialised Event: fields in ascending number, a zero step omitted"""
    out = b"\x09" + struct.pack("<d", float(wall_time))
    if int(step):
        out += b"\x10" + _varint(step)
    if file_version is not None:
        out += _field_bytes(3, file_version.encode())
    if values:
        out += _field_bytes(5, b"".join(_field_bytes(1, v) for v in values))
    return out


def crc32c(data):
    data = bytes(data)
    return int(_n.call(None, "surfel_log_crc32c", data, len(data)))


def masked_crc(data):
    c = crc32c(data)
    return ((c >> 15 | c << 17) + 0xa282ead8) & 0xffffffff


def frame(payload):
    """The TFRecord of one payload (surfel_log_frame)"""
    payload = bytes(payload)
    out = C.create_string_buffer(len(payload) + 16)
    n = _n.call(None, "surfel_log_frame", payload, len(payload), out)
    return out.raw[:n]


def encode_steps(records, iter_time_ms, wall_time):
    """records: RECORD_DTYPE array (host) -> the bytes of their step Events (surfel_log_encode_steps)"""
    rec = np.ascontiguousarray(records, RECORD_DTYPE)
    cap = int(_n.call(None, "surfel_log_steps_capacity", len(rec)))
    out = C.create_string_buffer(max(cap, 1))
    n = _n.call(None, "surfel_log_encode_steps", rec.ctypes.data_as(C.c_void_p), len(rec), float(iter_time_ms), float(wall_time), out, cap)
    return out.raw[:n]


# ------------------------------------------------------------------------------------------------ the device parts
def append(state, ring, iteration, points, scalars, lambda_normal, lambda_dist):
    """surfel_log_append: one record into ring (uint8 [capacity * 32]) behind whatever the current stream holds"""
    _n.device_tensor("surfel_log", scalars, "scalars")
    if scalars.dtype != torch.float32 or scalars.numel() < 6 or not scalars.is_contiguous():
        raise ValueError("surfel_log.append: six contiguous float32 scalars expected")
    _n.call(scalars.device, "surfel_log_append", state, ring, ring.numel() // RECORD_BYTES, int(iteration), int(points), scalars,
            float(lambda_normal), float(lambda_dist))


def panel(mode, planes, out=None, scratch=None):
    """float32 [C, H, W] (or [H, W]) on the device -> uint8 [H, W, 3] as TensorBoard's image summary shows it (surfel_log_panel).
    mode: "rgb" and "normal" take three planes, "gray", "turbo_max" and "jet_minmax" one.  Nothing waits for the device."""
    if mode not in MODES:
        raise ValueError("surfel_log.panel: mode must be one of %s" % ", ".join(MODES))
    t = _n.device_tensor("surfel_log", planes, "planes").detach()
    if t.dtype != torch.float32:
        raise ValueError("surfel_log.panel: float32 planes expected, got %s" % t.dtype)
    if t.dim() == 2:
        t = t[None]
    need = 3 if mode in ("rgb", "normal") else 1
    if t.dim() != 3 or t.shape[0] != need:
        raise ValueError("surfel_log.panel: mode %s takes [%d, H, W] planes, got %s" % (mode, need, tuple(planes.shape)))
    t = t.contiguous()
    H, W = int(t.shape[1]), int(t.shape[2])
    out = _n.uint8_buffer("surfel_log.panel", out, H * W * 3, t.device)
    if scratch is None:
        scratch = torch.empty(PANEL_SCRATCH_BYTES, dtype=torch.uint8, device=t.device)
    _n.call(t.device, "surfel_log_panel", MODES[mode], H, W, t, out, scratch, scratch.numel())
    return out.view(H, W, 3)


# ------------------------------------------------------------------------------------------------ the writer
class EventFile:
    """The file itself, host only: events.out.tfevents.<time>.<host>.<pid>.0 in logdir, whose first record is the Event
    file_version "brain.Event:2".  write_steps / write_event append framed records; nothing here touches a device."""

    def __init__(self, logdir):
        _n.load()
        os.makedirs(logdir, exist_ok=True)
        self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s.%d.0" % (int(time.time()), socket.gethostname(), os.getpid()))
        self._file = open(self.path, "wb")
        self.bytes_written = 0
        self.write(frame(event(time.time(), file_version=FILE_VERSION)))

    def write(self, data):
        self._file.write(data)
        self.bytes_written += len(data)

    def write_steps(self, records, iter_time_ms, wall_time):
        self.write(encode_steps(records, iter_time_ms, wall_time))

    def write_event(self, payload):
        self.write(frame(payload))

    def close(self):
        self._file.close()


class EventWriter:
    """events.out.tfevents.<time>.<host>.<pid>.0 in logdir, first record file_version "brain.Event:2".

    append(iteration, points, scalars, lambda_normal, lambda_dist) is one launch on the current stream.  Every `block` appends the
    block's records are copied into one of `slots` pinned blocks (non-blocking, same stream) and a timing event is recorded behind the
    copy; the writer thread waits for that event, frames the block and appends it to the file.  The training thread waits only when
    every pinned block is still unwritten: then it waits for the oldest and counts one in `stalls`.  add(step, values) queues a rare
    Event (panels, report scalars) behind the steps already queued, so the file stays in order.  close() flushes the partial block,
    joins the thread and re-raises what it met.
    iter_time (a departure, LOG.md): the time between two block-boundary events divided by the block's steps, the same for every
    step of a block: the whole step as the device saw it, not forward + backward.  A boundary is the event behind a block's copy, or
    mark(): the writer's creation marks one, a caller that queues other work between two steps brackets it with flush() and mark()
    (report does), and a training loop that does not start at once after creating the writer calls mark() in front of its first step."""

    def __init__(self, logdir, block=256, slots=4, device=None):
        self.block, self.slots = max(1, int(block)), max(1, int(slots))
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError("surfel_log: the log ring lives on a HIP device (got %s)" % self.device)
        self.capacity = 2 * self.block      # at most `block` records are ever unflushed, and the copy is stream-ordered before a slot's next append
        with torch.cuda.device(self.device):
            self._state = torch.zeros(STATE_BYTES, dtype=torch.uint8, device=self.device)
            self._ring = torch.zeros(self.capacity * RECORD_BYTES, dtype=torch.uint8, device=self.device)
        self._pinned = [torch.zeros(self.block * RECORD_BYTES, dtype=torch.uint8).pin_memory() for _ in range(self.slots)]
        self._out = [C.create_string_buffer(int(_n.call(None, "surfel_log_steps_capacity", self.block))) for _ in range(self.slots)]
        self._free = queue.Queue()
        for k in range(self.slots):
            self._free.put(k)
        self._work = queue.Queue()
        self._error = None
        self.steps = self._flushed = 0
        self.stalls = 0
        self._closed = False
        self.mark()
        self._file = EventFile(logdir)      # last of what can fail: no file is left behind by a writer that could not get its buffers
        self.path = self._file.path
        self._thread = threading.Thread(target=self._run, name="event-writer", daemon=True)
        self._thread.start()

    @property
    def bytes_written(self):
        return self._file.bytes_written

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close(reraise=exc_type is None)
        return False

    # ---- training thread
    def append(self, iteration, points, scalars, lambda_normal, lambda_dist):
        if self._closed:
            raise RuntimeError("EventWriter.append after close()")
        append(self._state, self._ring, iteration, points, scalars, lambda_normal, lambda_dist)
        self.steps += 1
        if self.steps - self._flushed == self.block:
            self.flush()

    def mark(self):
        """a block boundary here: the time of the next block's steps starts behind what the current stream holds now"""
        with torch.cuda.device(self.device):
            self._last_event = torch.cuda.Event(enable_timing=True)
            self._last_event.record()

    def flush(self):
        """close the partial block now (a no-op without unflushed steps): its copy and its boundary event are queued on the current stream"""
        count = self.steps - self._flushed
        if count == 0:
            return
        try:
            slot = self._free.get_nowait()
        except queue.Empty:
            self.stalls += 1
            slot = self._free.get()
        first, nbytes, size = (self._flushed % self.capacity) * RECORD_BYTES, count * RECORD_BYTES, self.capacity * RECORD_BYTES
        head = min(nbytes, size - first)      # (a partial block flushed by add() shifts the later ones: a block may straddle the wrap)
        with torch.cuda.device(self.device):
            self._pinned[slot][:head].copy_(self._ring[first:first + head], non_blocking=True)
            if head < nbytes:
                self._pinned[slot][head:nbytes].copy_(self._ring[:nbytes - head], non_blocking=True)
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
        self._work.put(("steps", slot, count, self._last_event, ev, time.time()))
        self._last_event = ev
        self._flushed = self.steps

    def add(self, step, values, wall_time=None):
        """queue one Event of serialised Summary.Values (value_scalar, value_image) behind everything queued so far"""
        if self._closed:
            raise RuntimeError("EventWriter.add after close()")
        self.flush()      # the steps before this Event come first in the file
        self._work.put(("raw", event(time.time() if wall_time is None else wall_time, step, list(values))))

    def close(self, reraise=True):
        if not self._closed:
            self._closed = True
            try:
                self.flush()
            finally:
                self._work.put(None)
                self._thread.join()
                self._file.close()
        if reraise and self._error is not None:
            err, self._error = self._error, None
            raise err

    # ---- writer thread
    def _run(self):
        while True:
            item = self._work.get()
            if item is None:
                return
            try:
                if item[0] == "steps":
                    _, slot, count, ev0, ev1, wall = item
                    try:
                        if self._error is None:
                            ev1.synchronize()
                            ms = ev0.elapsed_time(ev1) / count
                            out = self._out[slot]
                            n = _n.call(None, "surfel_log_encode_steps", C.c_void_p(self._pinned[slot].data_ptr()), count, ms, wall, out, len(out))
                            self._file.write(memoryview(out)[:n])
                    finally:
                        self._free.put(slot)
                elif self._error is None:
                    self._file.write_event(item[1])
            except BaseException as e:      # noqa: BLE001 — parked for close(); the queue keeps draining so that nobody waits for ever
                if self._error is None:
                    self._error = e


def report(trainer, writer, name, cams, first):
    """training_report's part for one split (train.py:206-248) at the trainer's iteration: the panels of the first five views — depth,
    render, rend_normal, surf_normal, rend_alpha, rend_dist, and ground_truth when `first` (the first test iteration) — as one Event
    per view, tags <name>_view_<image_name>/<panel>, and the scalars <name>/loss_viewpoint - l1_loss and - psnr, the numbers of
    Trainer.evaluate(cams), which are returned as (psnr, l1).  The partial block is flushed in front of the renders and a boundary is
    marked behind them, so the report's device time is in no step's iter_time."""
    import surfel_png
    from surfel_render import render
    if not cams:
        return None
    it = trainer.iteration
    writer.flush()
    with torch.no_grad():
        for cam in cams[:PANEL_VIEWS]:
            pkg = render(cam, trainer.model, trainer.pipe, trainer.background)
            maps = [(label, pkg[key], mode) for label, key, mode in PANELS]
            if first:
                maps.append(("ground_truth", cam.original_image, "rgb"))
            encoded = []
            for label, planes, mode in maps:
                pix = panel(mode, planes.float())
                buf, size = surfel_png.encode_png(pix, out=torch.empty(surfel_png.capacity(*pix.shape), dtype=torch.uint8, device=pix.device))
                encoded.append((label, pix.shape, buf, size))
            values = []
            for label, shape, buf, size in encoded:      # (the launches of all panels are queued before the first wait)
                values.append(value_image("%s_view_%s/%s" % (name, cam.image_name, label), int(shape[0]), int(shape[1]), _n.file_bytes(buf, size)))
            writer.add(it, values)
    ps, l1 = trainer.evaluate(cams)
    writer.add(it, [value_scalar(name + "/loss_viewpoint - l1_loss", l1), value_scalar(name + "/loss_viewpoint - psnr", ps)])
    writer.mark()
    return ps, l1


# ------------------------------------------------------------------------------------------------ reading back
class CorruptRecord(ValueError):
    """a record whose length or payload checksum does not match, or a truncated file; .index is the record's index in the file"""

    def __init__(self, index, what):
        ValueError.__init__(self, "record %d: %s" % (index, what))
        self.index = index


def _read_varint(b, p):
    v = shift = 0
    while True:
        if p >= len(b):
            raise ValueError("truncated varint")
        c = b[p]
        p += 1
        v |= (c & 127) << shift
        if c < 128:
            return v, p
        shift += 7


def _fields(b):
    """[(number, wire type, value)] of a serialised message: varints as int, 64- and 32-bit fields and strings as bytes"""
    out, p = [], 0
    while p < len(b):
        key, p = _read_varint(b, p)
        number, wt = key >> 3, key & 7
        if wt == 0:
            v, p = _read_varint(b, p)
        elif wt == 1:
            v, p = b[p:p + 8], p + 8
        elif wt == 5:
            v, p = b[p:p + 4], p + 4
        elif wt == 2:
            n, p = _read_varint(b, p)
            v, p = b[p:p + n], p + n
        else:
            raise ValueError("wire type %d" % wt)
        if p > len(b):
            raise ValueError("truncated field %d" % number)
        out.append((number, wt, v))
    return out


def parse_event(payload):
    """{"wall_time", "step", "file_version", "values": [{"tag", "simple_value"} or {"tag", "image": {height, width, colorspace, png}}]}"""
    ev = {"wall_time": 0.0, "step": 0, "file_version": None, "values": []}
    for number, wt, v in _fields(payload):
        if number == 1 and wt == 1:
            ev["wall_time"] = struct.unpack("<d", v)[0]
        elif number == 2 and wt == 0:
            ev["step"] = v
        elif number == 3 and wt == 2:
            ev["file_version"] = v.decode()
        elif number == 5 and wt == 2:
            for n2, w2, val in _fields(v):
                if n2 != 1 or w2 != 2:
                    continue
                d = {"tag": ""}
                for n3, w3, x in _fields(val):
                    if n3 == 1 and w3 == 2:
                        d["tag"] = x.decode()
                    elif n3 == 2 and w3 == 5:
                        d["simple_value"] = struct.unpack("<f", x)[0]
                    elif n3 == 4 and w3 == 2:
                        img = {"height": 0, "width": 0, "colorspace": 0, "png": b""}
                        for n4, w4, y in _fields(x):
                            if w4 == 0 and n4 in (1, 2, 3):
                                img[("height", "width", "colorspace")[n4 - 1]] = y
                            elif n4 == 4 and w4 == 2:
                                img["png"] = bytes(y)
                        d["image"] = img
                ev["values"].append(d)
    return ev


def read_records(path):
    """the payloads of an event file, both checksums of every record verified (CorruptRecord names the record)"""
    data = open(path, "rb").read()
    out, p = [], 0
    while p < len(data):
        k = len(out)
        if p + 12 > len(data):
            raise CorruptRecord(k, "truncated header")
        n, = struct.unpack_from("<Q", data, p)
        if struct.unpack_from("<I", data, p + 8)[0] != masked_crc(data[p:p + 8]):
            raise CorruptRecord(k, "length checksum mismatch")
        if p + 12 + n + 4 > len(data):
            raise CorruptRecord(k, "truncated payload")
        payload = data[p + 12:p + 12 + n]
        if struct.unpack_from("<I", data, p + 12 + n)[0] != masked_crc(payload):
            raise CorruptRecord(k, "payload checksum mismatch")
        out.append(payload)
        p += 16 + n
    return out


def read_events(path):
    """[parse_event(...)] of every record of an event file"""
    return [parse_event(p) for p in read_records(path)]


def event_files(model_dir):
    return sorted(os.path.join(model_dir, f) for f in os.listdir(model_dir) if f.startswith("events.out.tfevents."))


def scalar_rows(events):
    """(sorted tags, {step: {tag: value}}) of the scalar values"""
    rows, tags = {}, set()
    for ev in events:
        for v in ev["values"]:
            if "simple_value" in v:
                rows.setdefault(ev["step"], {})[v["tag"]] = v["simple_value"]
                tags.add(v["tag"])
    return sorted(tags), rows


def main(argv=None):
    """python surfel_log.py MODEL_DIR [--csv] [--images DIR]: a summary of the folder's event files; --csv prints step,<tag>,... rows of
    the scalars; --images DIR writes every panel as DIR/<step>/<tag with / as __>.png"""
    import argparse
    import sys
    ap = argparse.ArgumentParser(description="Read the TensorBoard event files a --tensorboard training run left in MODEL_DIR")
    ap.add_argument("model_dir")
    ap.add_argument("--csv", action="store_true", help="print the scalar curves as CSV")
    ap.add_argument("--images", metavar="DIR", default=None, help="write the image panels as PNG files into DIR")
    args = ap.parse_args(argv)
    files = event_files(args.model_dir)
    if not files:
        print("no event files in %s" % args.model_dir, file=sys.stderr)
        return 1
    events = [ev for f in files for ev in read_events(f)]
    tags, rows = scalar_rows(events)
    if args.csv:
        print(",".join(["step"] + tags))
        for step in sorted(rows):
            print(",".join([str(step)] + ["%.9g" % rows[step][t] if t in rows[step] else "" for t in tags]))
    images = 0
    for ev in events:
        for v in ev["values"]:
            if "image" in v:
                images += 1
                if args.images:
                    folder = os.path.join(args.images, "%06d" % ev["step"])
                    os.makedirs(folder, exist_ok=True)
                    with open(os.path.join(folder, v["tag"].replace("/", "__") + ".png"), "wb") as f:
                        f.write(v["image"]["png"])
    if not args.csv:
        print("%d file(s), %d events, %d steps with scalars, %d scalar tags, %d images" % (len(files), len(events), len(rows), len(tags), images))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
