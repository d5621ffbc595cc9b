"""What the frame writers share (surfel_path.FrameWriter, surfel_video.VideoWriter, surfel_view.Viewer): a ring of slots that bounds the
frames in flight and keeps the first exception of the threads behind it, the device side of a stream of files encoded on the device,
and the read-back of a device tensor through pinned memory."""
import threading
import time

import torch


class SlotRing:
    """`ring` slots, numbered from 0.  acquire() blocks only when all of them are out and adds the time it waited to wait_s.
    park(e) keeps the first exception the threads behind the writer met; reraise() raises it, once (the writer's close())."""

    def __init__(self, ring):
        self.ring = ring
        self.wait_s = 0.0
        self.error = None
        self._free = threading.Semaphore(ring)
        self._idle = list(range(ring))
        self._lock = threading.Lock()

    def acquire(self):
        t0 = time.perf_counter()
        self._free.acquire()
        self.wait_s += time.perf_counter() - t0
        with self._lock:
            return self._idle.pop()

    def release(self, slot):
        with self._lock:
            self._idle.append(slot)
        self._free.release()

    def park(self, e):
        with self._lock:
            if self.error is None:
                self.error = e

    def reraise(self):
        e, self.error = self.error, None
        if e is not None:
            raise e


def to_pinned(src, pinned, stream=None):
    """(pinned, view): the bytes of the flat uint8 device tensor `src` as a memoryview of the pinned uint8 host tensor `pinned`, which is
    replaced by one of src.numel() bytes when it is None or shorter.  A non-blocking copy on `stream` (None: the current one) and a wait
    for the event behind it."""
    n = src.numel()
    if pinned is None or pinned.numel() < n:
        pinned = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    with torch.cuda.device(src.device), torch.cuda.stream(stream):
        pinned[:n].copy_(src, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
    done.synchronize()
    return pinned, memoryview(pinned.numpy())[:n]


class EncodedStream:
    """The device side of a writer whose files are encoded on the device, for `ring` slots on one device: a side stream, and per slot an
    output buffer and a pinned staging buffer (both grown on demand), the file's int64 size on the device and its copy in pinned memory."""

    def __init__(self, device, ring):
        self.device = device
        with torch.cuda.device(device):
            self.stream = torch.cuda.Stream(device=device)
            self.sizes = torch.zeros(ring, dtype=torch.int64, device=device)
            self.host_size = torch.zeros(ring, dtype=torch.int64).pin_memory()
        self.buffers = [None] * ring
        self.staging = [None] * ring

    def encode(self, slot, capacity, fn):
        """fn(out=, size=) writes a file of at most `capacity` bytes into the slot's buffer on the current stream; the size word follows
        to pinned memory without blocking.  Returns the event behind both."""
        with torch.cuda.device(self.device):
            if self.buffers[slot] is None or self.buffers[slot].numel() < capacity:
                self.buffers[slot] = torch.empty(capacity, dtype=torch.uint8, device=self.device)
            size = self.sizes[slot:slot + 1]
            fn(out=self.buffers[slot], size=size)
            self.host_size[slot:slot + 1].copy_(size, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
        return event

    def fetch(self, slot, event):
        """the finished file of a slot as a memoryview of pinned memory (thread side): waits for the event, reads the size and copies
        exactly that many bytes on the side stream"""
        event.synchronize()
        n = int(self.host_size[slot])
        self.staging[slot], view = to_pinned(self.buffers[slot][:n], self.staging[slot], self.stream)
        return view
