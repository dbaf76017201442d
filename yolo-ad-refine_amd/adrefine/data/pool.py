"""The HBM-resident image pool: dataset images are decoded on the host once, resized on the GPU by adr_resize_u8
(csrc/adr_resize.hip: BaseDataset.load_image's cv2.resize, data/base.py:168-172) and stay in device memory, where
adr_augment_u8 / adr_letterbox_u8 read them as their sources. A training batch then moves only descriptors and
tables over PCIe (render / render_letterbox in augment.py).

  DevicePool   one uint8 device tensor, 256-byte-aligned blocks, exact-size free list
  DeviceImage  the handle of one HWC BGR uint8 image in a pool; stands where a numpy source image stands in an
               ImagePlan (shape, dtype, ndim, size)
  queue/flush  images are queued with a loader (a callable returning the decoded HWC BGR uint8 image); flush decodes
               what is pending in a small thread pool, packs it into pinned staging, copies it and runs one
               adr_resize_u8 launch per staging round on the project's stream. Every GPU call is made by the thread
               that calls flush(); prepare() (decode only) may run on another thread."""
from __future__ import annotations

import ctypes
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .augment import LB_AREA2, LB_COPY, LB_LINEAR, resize_linear_tables

__all__ = ["DevicePool", "DeviceImage", "PoolFull", "ResizeDesc", "resize_mode", "resize_prefix"]

ALIGN = 256


class PoolFull(MemoryError):
    """DevicePool.alloc: no free block of the size and not enough untouched capacity left."""


class ResizeDesc(ctypes.Structure):
    """adr_resize_desc (include/adr.h)."""
    _fields_ = [("src_off", ctypes.c_int64), ("dst_off", ctypes.c_int64)] + [(n, ctypes.c_int) for n in (
        "sw", "sh", "nw", "nh", "mode", "tab_off")]


def resize_mode(sw, sh, nw, nh):
    """The path cv2.resize(INTER_LINEAR) takes (as render_letterbox chooses it)."""
    if (sw, sh) == (nw, nh):
        return LB_COPY
    if (sw, sh) == (2 * nw, 2 * nh):
        return LB_AREA2
    return LB_LINEAR


def resize_prefix(sizes):
    """adr_resize_u8's block prefix for destination sizes [(nw, nh), ...]: the first block of each image."""
    blocks = [(((nh * nw * 3 + 3) // 4) + 255) // 256 for nw, nh in sizes]
    return np.concatenate([[0], np.cumsum(blocks)[:-1]]).astype(np.int32)


def _round_up(n, a=ALIGN):
    return (n + a - 1) // a * a


class DeviceImage:
    """One HWC BGR uint8 image of h x w pixels at byte offset `off` of `pool` (compact: row stride w * 3)."""

    dtype = np.dtype(np.uint8)
    ndim = 3

    def __init__(self, pool, off, h, w):
        self.pool, self.off, self.h, self.w = pool, off, int(h), int(w)

    @property
    def shape(self):
        return (self.h, self.w, 3)

    @property
    def size(self):
        return self.h * self.w * 3

    def numpy(self):
        """The image as a host array (flushes the pool; a device-to-host copy, for tests and debugging)."""
        if self.off is None:
            raise ValueError("DeviceImage: the image was released")
        self.pool.flush()
        return self.pool.tensor[self.off:self.off + self.size].cpu().numpy().reshape(self.shape)

    def __repr__(self):
        return f"DeviceImage({self.h} x {self.w} at {self.off})"


class DevicePool:
    """capacity_bytes of device memory for images. alloc / free hand out 256-byte-aligned blocks; a freed block is
    reused by the next alloc of the same (rounded) size (`slot_bytes`: one size for all). `staging_bytes` bounds the pinned host buffers (two of
    them, used alternately) and the device staging buffer; `workers` host threads decode."""

    def __init__(self, device, capacity_bytes, staging_bytes=256 << 20, workers=8, slot_bytes=None):
        self.device = torch.device(device)
        self.capacity = _round_up(int(capacity_bytes))
        self.tensor = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
        self.staging_bytes = int(staging_bytes)
        self.workers = max(1, min(int(workers), 16))
        # slot_bytes: every request up to it takes a block of exactly that size, so that any freed block serves any
        # later image (a pool that images of many shapes enter and leave; exact sizes would never be reused)
        self.slot_bytes = None if slot_bytes is None else _round_up(int(slot_bytes))
        self._top = 0
        self._free = {}  # rounded size -> [offsets]
        self._size = {}  # live offset -> rounded size
        self._pending = []  # [handle, loader, (h0, w0) or None, decoded array or None]
        self._lock = threading.RLock()
        self._decode_lock = threading.Lock()
        self._exec = None
        self._pinned = []  # up to two [tensor, event or None]
        self._dev_stage = None
        self.rounds = 0  # copy + launch rounds so far (one flush may take several)
        self.launches = 0

    # ---- blocks ----
    def alloc(self, nbytes):
        n = _round_up(max(int(nbytes), 1))
        if self.slot_bytes is not None and n <= self.slot_bytes:
            n = self.slot_bytes
        with self._lock:
            free = self._free.get(n)
            if free:
                off = free.pop()
            elif self._top + n <= self.capacity:
                off = self._top
                self._top += n
            else:
                raise PoolFull(f"DevicePool: no room for {n} bytes ({self._top} of {self.capacity} handed out, "
                               f"{sum(len(v) for v in self._free.values())} free blocks of other sizes)")
            self._size[off] = n
            return off

    def free(self, off):
        with self._lock:
            n = self._size.pop(off)  # KeyError: not a live block
            self._free.setdefault(n, []).append(off)

    @property
    def used_bytes(self):
        with self._lock:
            return sum(self._size.values())

    # ---- images ----
    def image(self, h, w):
        """A new image handle of h x w pixels (its pixels arrive with queue + flush)."""
        return DeviceImage(self, self.alloc(h * w * 3), h, w)

    def release(self, im):
        """Give the image's block back. Work already enqueued on the stream that reads it stays correct: a later
        resize into the block is ordered behind it on the same stream."""
        with self._lock:
            if any(p[0] is im for p in self._pending):
                self._pending = [p for p in self._pending if p[0] is not im]
            self.free(im.off)
            im.off = None

    def queue(self, im, loader, src_hw=None):
        """Fill `im` at the next flush with cv2.resize(loader(), (im.w, im.h)). loader() returns the decoded HWC BGR
        uint8 image; src_hw, when given, is the (h0, w0) it must have."""
        if im.pool is not self or im.off is None:
            raise ValueError("DevicePool.queue: not a live image of this pool")
        with self._lock:
            self._pending.append([im, loader, None if src_hw is None else (int(src_hw[0]), int(src_hw[1])), None])

    def _executor(self):
        if self._exec is None:
            self._exec = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="adr-decode")
        return self._exec

    @staticmethod
    def _decode(entry):
        im, loader, src_hw, _ = entry
        a = loader()
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("DevicePool: a loader must return an HWC BGR uint8 image")
        if src_hw is not None and tuple(a.shape[:2]) != src_hw:
            raise ValueError(f"DevicePool: decoded image is {a.shape[:2]}, expected {src_hw} (stale label cache?)")
        return np.ascontiguousarray(a)

    def prepare(self, limit_bytes=None):
        """Decode pending images on the host (no GPU call; any thread). Without src_hw the size of an image is
        only known once it is decoded, so limit_bytes bounds what is known."""
        with self._decode_lock:
            with self._lock:
                todo, total = [], 0
                for e in self._pending:
                    if e[3] is None:
                        n = e[2][0] * e[2][1] * 3 if e[2] is not None else 0
                        if limit_bytes is not None and todo and total + n > limit_bytes:
                            break
                        todo.append(e)
                        total += n
            if not todo:
                return 0
            if len(todo) == 1 or self.workers == 1:
                arrays = [self._decode(e) for e in todo]
            else:
                arrays = list(self._executor().map(self._decode, todo))
            for e, a in zip(todo, arrays):
                e[3] = a
            return len(todo)

    def _pinned_buffer(self, nbytes):
        """A pinned host buffer of at least nbytes that no copy is still reading: the two buffers alternate, and one
        is taken again only after the event recorded behind the copy that read it has completed."""
        if len(self._pinned) < 2:
            self._pinned.append([None, None])
            slot = self._pinned[-1]
        else:
            slot = self._pinned[self.rounds % 2]
        if slot[1] is not None:
            slot[1].synchronize()
            slot[1] = None
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(max(nbytes, min(self.staging_bytes, 1 << 20)), dtype=torch.uint8).pin_memory()
        return slot

    def flush(self):
        """Decode what is pending, copy it and resize it into the pool: one pinned copy + one adr_resize_u8 launch
        per staging round, on kernels.stream(), all from the calling thread. Returns the number of images."""
        with self._lock:
            if not self._pending:
                return 0
        from ..kernels import stream
        from ..native import lib
        if ctypes.sizeof(ResizeDesc) != lib.adr_resize_desc_size():
            raise RuntimeError("adr_resize_desc layout mismatch between adrefine and libadr_hip")
        done = 0
        while True:
            self.prepare(self.staging_bytes)
            with self._lock:
                batch, total = [], 0
                for e in self._pending:
                    if e[3] is None:
                        break
                    if batch and total + e[3].size > self.staging_bytes:
                        break
                    batch.append(e)
                    total += e[3].size
                if not batch:
                    if self._pending:
                        continue
                    return done
                del self._pending[:len(batch)]
            self._round(batch, total, lib, stream())
            done += len(batch)

    def _round(self, batch, total, lib, strm):
        B = len(batch)
        slot = self._pinned_buffer(total)
        host = slot[0].numpy()
        descs = (ResizeDesc * B)()
        tabs, ntab, off = [], 0, 0
        for b, (im, _, _, a) in enumerate(batch):
            sh, sw = a.shape[:2]
            host[off:off + a.size] = a.reshape(-1)
            d = descs[b]
            d.src_off, d.dst_off, d.sw, d.sh, d.nw, d.nh = off, im.off, sw, sh, im.w, im.h
            d.mode = resize_mode(sw, sh, im.w, im.h)
            if d.mode == LB_LINEAR:
                tab = np.concatenate(resize_linear_tables(sw, im.w) + resize_linear_tables(sh, im.h))
                d.tab_off = ntab
                tabs.append(tab)
                ntab += tab.size
            off += a.size
            batch[b][3] = None
        if self._dev_stage is None or self._dev_stage.numel() < total:
            self._dev_stage = torch.empty(max(total, min(self.staging_bytes, 1 << 20)), dtype=torch.uint8,
                                          device=self.device)
        with torch.cuda.device(self.device):
            self._dev_stage[:total].copy_(slot[0][:total], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            slot[1] = ev
            meta = np.concatenate([np.frombuffer(bytearray(descs), dtype=np.uint8).view(np.int32),
                                   resize_prefix([(im.w, im.h) for im, _, _, _ in batch])] +
                                  (tabs if tabs else [np.zeros(1, np.int32)]))
            md = torch.from_numpy(meta).to(self.device, non_blocking=True)
            nd = ctypes.sizeof(ResizeDesc) * B
            lib.adr_resize_u8(ctypes.c_void_p(self._dev_stage.data_ptr()), total, ctypes.c_void_p(md.data_ptr()),
                              ctypes.cast(descs, ctypes.c_void_p), ctypes.c_void_p(md.data_ptr() + nd), B,
                              ctypes.c_void_p(md.data_ptr() + nd + 4 * B), ntab,
                              ctypes.c_void_p(self.tensor.data_ptr()), self.capacity, strm)
        self._keep = md  # lives until the next round's launch is enqueued behind this one (stream order)
        self.rounds += 1
        self.launches += 1

    def close(self):
        if self._exec is not None:
            self._exec.shutdown(wait=True)
            self._exec = None
