"""build_yolo_dataset / build_dataloader (reference data/build.py:84-103, 127-145) without worker processes: a forked
or spawned child would import adrefine and might open the GPU. The loader is a plain iterable; the host side of a
batch (the transforms: RNG draws, label arithmetic, plans; and the image decodes) can run up to `prefetch` batches
ahead on ONE background thread, which never touches the GPU; the pool flush (copy + adr_resize_u8) and collate_fn
(the render launch) run on the thread that iterates. At most prefetch + 1 batches are ever begun and not yet rendered:
the thread is admitted to the next batch only when the batch prefetch + 1 places back has been rendered and its retired
images freed (dataset.end_batch), however slow the iterating thread is; a cache=None pool is sized for exactly that
(YOLODataset.pool_slots, `inflight`). The batches do not depend on `prefetch`: the single thread
builds the samples in the same order with the same global `random` / `np.random` streams (the iterating thread must
not draw from them while an epoch is under way)."""
from __future__ import annotations

import queue
import threading

import torch

from .dataset import YOLODataset

__all__ = ["build_yolo_dataset", "build_dataloader", "DataLoader", "SEED"]

SEED = 6148914691236517205  # build.py:134


def build_yolo_dataset(cfg, img_path, batch, data, mode="train", rect=False, stride=32, **kw):
    """build.py:84-103; **kw: YOLODataset's own arguments (device, pool, cache_gb, inflight, workers)."""
    return YOLODataset(img_path=img_path, imgsz=cfg.imgsz, batch_size=batch, augment=mode == "train", hyp=cfg,
                       rect=getattr(cfg, "rect", False) or rect, cache=getattr(cfg, "cache", None) or None,
                       single_cls=getattr(cfg, "single_cls", False) or False, stride=int(stride),
                       pad=0.0 if mode == "train" else 0.5, prefix=f"{mode}: ", task=getattr(cfg, "task", "detect"),
                       classes=getattr(cfg, "classes", None), data=data,
                       fraction=getattr(cfg, "fraction", 1.0) if mode == "train" else 1.0, **kw)


class DataLoader:
    """An epoch per iteration: index order -> batches of `batch` (the last short one kept) -> dataset[i] per index
    -> pool.flush() -> dataset.collate_fn. reset() drops a running epoch's iterator (after close_mosaic);
    set_epoch(e) is the DistributedSampler's."""

    def __init__(self, dataset, batch, shuffle=True, rank=-1, world_size=1, prefetch=1, sampler=None):
        self.dataset = dataset
        self.batch = max(1, min(int(batch), len(dataset)))
        self.shuffle = bool(shuffle) and not getattr(dataset, "rect", False)
        self.prefetch = max(0, int(prefetch))
        self.generator = torch.Generator()
        self.generator.manual_seed(SEED + rank)
        self.sampler = sampler  # any iterable of indices: overrides the order (a fixed order: tests, replays)
        if sampler is None and rank >= 0:
            self.sampler = torch.utils.data.DistributedSampler(dataset, num_replicas=world_size, rank=rank,
                                                               shuffle=self.shuffle)
        if getattr(dataset, "cache", "gpu") is None and self.prefetch + 1 > getattr(dataset, "inflight", 1 << 30):
            raise ValueError(f"build_dataloader: prefetch={self.prefetch} needs a dataset built with inflight >= "
                             f"{self.prefetch + 1} (its pool is sized for {dataset.inflight} batches in flight)")
        self._n = len(self.sampler) if self.sampler is not None else len(dataset)
        self._stop = None

    def __len__(self):
        return (self._n + self.batch - 1) // self.batch

    def set_epoch(self, epoch):
        if hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(epoch)

    def indices(self):
        """The epoch's index order: the sampler's, torch.randperm(n, generator) when shuffling, else 0..n-1."""
        if self.sampler is not None:
            return [int(i) for i in self.sampler]
        if self.shuffle:
            return torch.randperm(len(self.dataset), generator=self.generator).tolist()
        return list(range(len(self.dataset)))

    def reset(self):
        """Stop the running epoch's background thread; the next iter() starts a new epoch."""
        if self._stop is not None:
            self._stop.set()
            self._stop = None

    def _collate(self, samples):
        return self.dataset.collate_fn(samples)

    def _build(self, seq, idx):
        ds = self.dataset
        if hasattr(ds, "begin_batch"):
            ds.begin_batch(seq)
        return [ds[i] for i in idx]

    def _admit(self, seq, permits, stop):
        """Block the background thread until batch `seq` may be begun: a permit is free once a batch has been rendered
        and ended. False: the epoch was stopped."""
        while not stop.is_set():
            if permits.acquire(timeout=0.05):
                return True
        return False

    def _finish(self, seq, samples):
        pool = getattr(self.dataset, "pool", None)
        if pool is not None:
            pool.flush()
        out = self._collate(samples)
        if hasattr(self.dataset, "end_batch"):
            self.dataset.end_batch(seq)
        return out

    def __iter__(self):
        self.reset()
        order = self.indices()
        chunks = [order[i:i + self.batch] for i in range(0, len(order), self.batch)]
        # the dataset's begin_batch / end_batch key: batches built so far, over all epochs and loaders of the dataset
        seq0 = getattr(self.dataset, "batches_built", 0)
        try:
            self.dataset.batches_built = seq0 + len(chunks)
        except AttributeError:
            pass
        if self.prefetch == 0:
            for k, idx in enumerate(chunks):
                yield self._finish(seq0 + k, self._build(seq0 + k, idx))
            return
        stop, q = threading.Event(), queue.Queue(maxsize=self.prefetch)
        permits = threading.Semaphore(self.prefetch + 1)  # batches begun and not ended
        self._stop = stop

        def put(item):
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.05)
                    return True
                except queue.Full:
                    pass
            return False

        def work():  # host only: transforms and decodes
            try:
                pool = getattr(self.dataset, "pool", None)
                for k, idx in enumerate(chunks):
                    if not self._admit(seq0 + k, permits, stop):
                        return
                    samples = self._build(seq0 + k, idx)
                    if pool is not None and hasattr(pool, "prepare"):
                        pool.prepare()
                    if not put((seq0 + k, samples, None)):
                        return
                put(None)
            except BaseException as e:  # noqa: BLE001 - handed to the iterating thread
                put((None, None, e))

        t = threading.Thread(target=work, name="adr-loader", daemon=True)
        t.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                seq, samples, err = item
                if err is not None:
                    raise err
                out = self._finish(seq, samples)
                permits.release()
                yield out
        finally:
            stop.set()
            t.join()
            if self._stop is stop:
                self._stop = None


def build_dataloader(dataset, batch, shuffle=True, rank=-1, world_size=1, prefetch=1, sampler=None):
    """build.py:127-145: the order is torch.randperm(n, generator) of a generator seeded 6148914691236517205 + rank
    (each epoch draws the next permutation from it); rank >= 0: torch's DistributedSampler(num_replicas=world_size,
    rank=rank, shuffle=shuffle), which needs no process group when both are given. shuffle is off for rect datasets.
    prefetch=0: everything inline. sampler (not in the reference's signature): any iterable of indices to use as the
    order instead, e.g. to replay a recorded one."""
    return DataLoader(dataset, batch, shuffle, rank, world_size, prefetch, sampler)
