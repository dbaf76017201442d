"""YOLODataset for detection (reference data/base.py BaseDataset + data/dataset.py:30-260 YOLODataset +
data/utils.py img2label_paths / exif_size / verify_image_label): an images/ + labels/ directory read into the
reference's label records, with the images resident in device memory.

What differs from the reference, on purpose:
  * load_image decodes nothing. (h0, w0) comes from the verified label record; the image is a DeviceImage handle of a
    data/pool.py DevicePool, queued there with a loader, decoded on the host (a sibling .npy first, as the reference
    does; otherwise PIL: exif_transpose, RGB, reversed to BGR) and resized by adr_resize_u8 at the pool's next flush
    (render / render_letterbox flush). PNG / BMP decode exactly; JPEG goes through PIL's libjpeg, which is PARITY
    UNPINNED against OpenCV's decoder. (cv2.imread applies the EXIF orientation too, and verify_image_label's shape
    is exif_size's: the two agree for the orientations exif_size swaps.)
  * cache="gpu" is the deterministic counterpart of cache="ram": every image is loaded in index order at construction
    and stays resident. cache=None keeps training images until the mosaic buffer evicts them and validation images
    until the batch after theirs has been rendered. "ram" / "disk" raise.
  * the label cache is the project's own <labels parent>/<name>.adrcache.npz (arrays only); the reference's pickled
    .cache is neither read nor written.
The `buffer` bookkeeping of base.py:176-185 is kept literally, so Mosaic.get_indexes draws what the reference draws.
Segments and keypoints raise NotImplementedError (data/instance.py is boxes only)."""
from __future__ import annotations

import glob
import hashlib
import math
import os
import threading
import warnings
from copy import deepcopy
from pathlib import Path

import numpy as np

from .augment import build_transforms, close_mosaic, collate_fn
from .instance import Instances

__all__ = ["YOLODataset", "IMG_FORMATS", "img2label_paths", "get_hash", "exif_size", "verify_image_label",
           "load_bgr"]

IMG_FORMATS = {"bmp", "dng", "jpeg", "jpg", "mpo", "png", "tif", "tiff", "webp", "pfm"}  # data/utils.py:38
CACHE_VERSION = 1


def img2label_paths(img_paths):
    """data/utils.py:44-47."""
    sa, sb = f"{os.sep}images{os.sep}", f"{os.sep}labels{os.sep}"
    return [sb.join(x.rsplit(sa, 1)).rsplit(".", 1)[0] + ".txt" for x in img_paths]


def get_hash(paths):
    """data/utils.py:50-55: sha256 of the summed file sizes and of the paths."""
    size = sum(os.path.getsize(p) for p in paths if os.path.exists(p))
    h = hashlib.sha256(str(size).encode())
    h.update("".join(paths).encode())
    return h.hexdigest()


def exif_size(img):
    """data/utils.py:58-70: the EXIF-corrected PIL size (JPEG only)."""
    s = img.size
    if img.format == "JPEG":
        try:
            exif = img.getexif()
            if exif and exif.get(274, None) in {6, 8}:
                s = s[1], s[0]
        except Exception:  # noqa: BLE001 - as the reference: any EXIF failure leaves the size as it is
            pass
    return s


def verify_image_label(im_file, lb_file, num_cls):
    """data/utils.py:98-167 for detection: (im_file, lb (n, 5) float32, (h, w), nm, nf, ne, nc, msg); a corrupt pair
    gives im_file None and nc 1."""
    from PIL import Image, ImageOps
    nm, nf, ne, nc, msg = 0, 0, 0, 0, ""
    try:
        im = Image.open(im_file)
        im.verify()
        shape = exif_size(im)
        shape = (shape[1], shape[0])  # hw
        assert (shape[0] > 9) & (shape[1] > 9), f"image size {shape} <10 pixels"
        assert im.format.lower() in IMG_FORMATS, f"invalid image format {im.format}"
        if im.format.lower() in {"jpg", "jpeg"}:
            with open(im_file, "rb") as f:
                f.seek(-2, 2)
                if f.read() != b"\xff\xd9":  # corrupt JPEG
                    ImageOps.exif_transpose(Image.open(im_file)).save(im_file, "JPEG", subsampling=0, quality=100)
                    msg = f"WARNING {im_file}: corrupt JPEG restored and saved"
        if os.path.isfile(lb_file):
            nf = 1
            with open(lb_file) as f:
                lb = [x.split() for x in f.read().strip().splitlines() if len(x)]
            if any(len(x) > 6 for x in lb):
                raise NotImplementedError(f"{lb_file}: segment / keypoint label rows (detection boxes only)")
            lb = np.array(lb, dtype=np.float32)
            nl = len(lb)
            if nl:
                assert lb.shape[1] == 5, f"labels require 5 columns, {lb.shape[1]} columns detected"
                points = lb[:, 1:]
                assert points.max() <= 1, f"non-normalized or out of bounds coordinates {points[points > 1]}"
                assert lb.min() >= 0, f"negative label values {lb[lb < 0]}"
                max_cls = lb[:, 0].max()
                assert max_cls <= num_cls, (f"Label class {int(max_cls)} exceeds dataset class count {num_cls}. "
                                            f"Possible class labels are 0-{num_cls - 1}")
                _, i = np.unique(lb, axis=0, return_index=True)
                if len(i) < nl:  # duplicate rows: the survivors come in np.unique's (sorted) order, as in the reference
                    lb = lb[i]
                    msg = f"WARNING {im_file}: {nl - len(i)} duplicate labels removed"
            else:
                ne = 1
                lb = np.zeros((0, 5), dtype=np.float32)
        else:
            nm = 1
            lb = np.zeros((0, 5), dtype=np.float32)
        return im_file, lb[:, :5], shape, nm, nf, ne, nc, msg
    except NotImplementedError:
        raise
    except Exception as e:  # noqa: BLE001 - as the reference: any failure marks the pair corrupt
        return None, None, None, nm, nf, ne, 1, f"WARNING {im_file}: ignoring corrupt image/label: {e}"


def load_bgr(im_file):
    """The decoded HWC BGR uint8 image: a sibling .npy when there is one (base.py:155-161), otherwise PIL with the EXIF
    orientation applied (what cv2.imread does). JPEG: PARITY UNPINNED against OpenCV's decoder."""
    fn = Path(im_file).with_suffix(".npy")
    if fn.exists():
        try:
            return np.ascontiguousarray(np.load(fn))
        except Exception as e:  # noqa: BLE001
            warnings.warn(f"ignoring corrupt *.npy image file {fn}: {e}", stacklevel=2)
    from PIL import Image, ImageOps
    try:
        with Image.open(im_file) as im:
            rgb = np.asarray(ImageOps.exif_transpose(im).convert("RGB"))
    except Exception as e:  # noqa: BLE001
        raise FileNotFoundError(f"Image Not Found {im_file}") from e
    return np.ascontiguousarray(rgb[:, :, ::-1])


class YOLODataset:
    """The reference's constructor arguments and attributes (im_files, labels, ni, buffer, max_buffer_length,
    batch_shapes, batch, transforms, imgsz, augment, rect). `pool`: an image pool to use instead of a DevicePool made
    here (anything with image(h, w) / queue(im, loader, src_hw) / release(im) / flush(); tests inject a host
    stand-in); `inflight`: how many batches may be under construction or unrendered at once when the pool is sized
    here (the loader's prefetch + 1)."""

    def __init__(self, img_path, imgsz=640, cache=False, augment=True, hyp=None, prefix="", rect=False, batch_size=16,
                 stride=32, pad=0.5, single_cls=False, classes=None, fraction=1.0, data=None, task="detect",
                 device="cuda", pool=None, cache_gb=None, inflight=2, workers=8):
        if task != "detect":
            raise NotImplementedError(f"YOLODataset: task {task!r} (detection only)")
        if hyp is None:
            raise ValueError("YOLODataset: hyp (the augmentation hyper-parameters) is required")
        self.use_segments = self.use_keypoints = self.use_obb = False
        self.data = data if data is not None else {}
        self.img_path, self.imgsz, self.augment, self.single_cls = img_path, imgsz, augment, single_cls
        self.prefix, self.fraction = prefix, fraction
        self.im_files = self.get_img_files(self.img_path)
        self.labels = self.get_labels()
        self.update_labels(include_class=classes)
        self.ni = len(self.labels)
        self._shapes = [tuple(int(v) for v in lb["shape"]) for lb in self.labels]  # hw; set_rectangle pops "shape"
        self.rect, self.batch_size, self.stride, self.pad = rect, batch_size, stride, pad
        if self.rect:
            assert self.batch_size is not None
            self.set_rectangle()
        self.buffer = []
        self.max_buffer_length = min((self.ni, self.batch_size * 8, 1000)) if self.augment else 0
        self.ims, self.im_hw0, self.im_hw = [None] * self.ni, [None] * self.ni, [None] * self.ni
        self.npy_files = [Path(f).with_suffix(".npy") for f in self.im_files]
        self._src_hw = [None] * self.ni
        self.cache = cache.lower() if isinstance(cache, str) else "ram" if cache is True else None
        if self.cache in ("ram", "disk"):
            raise NotImplementedError(f"YOLODataset: cache={self.cache!r}; images are cached in device memory: "
                                      'cache="gpu"')
        if self.cache not in (None, "gpu"):
            raise ValueError(f"YOLODataset: cache={cache!r}")
        self.inflight = max(1, int(inflight))
        self._hyp = hyp  # pool_slots reads mixup
        self._retired, self._seq, self._rlock = [], 0, threading.Lock()
        self.batches_built = 0  # the loaders' batch counter (begin_batch / end_batch)
        self.pool = pool
        if self.cache == "gpu" and pool is None and not self.check_cache_gpu(device, cache_gb):
            self.cache = None
        if self.pool is None:
            from .pool import ALIGN, DevicePool
            if self.cache == "gpu":
                self.pool = DevicePool(device, self._resident_bytes(), workers=workers)
            else:  # images come and go: uniform slots of imgsz * imgsz * 3 bytes, so that every freed one is reusable
                per = (imgsz * imgsz * 3 + ALIGN - 1) // ALIGN * ALIGN
                self.pool = DevicePool(device, self.pool_slots() * per, workers=workers, slot_bytes=per)
        if self.cache == "gpu":
            self.cache_images()
        self.transforms = self.build_transforms(hyp=hyp)

    # ---- files and labels ----
    def get_img_files(self, img_path):
        """base.py:106-130."""
        try:
            f = []
            for p in img_path if isinstance(img_path, list) else [img_path]:
                p = Path(p)
                if p.is_dir():
                    f += glob.glob(str(p / "**" / "*.*"), recursive=True)
                elif p.is_file():
                    with open(p) as t:
                        t = t.read().strip().splitlines()
                        parent = str(p.parent) + os.sep
                        f += [x.replace("./", parent) if x.startswith("./") else x for x in t]
                else:
                    raise FileNotFoundError(f"{self.prefix}{p} does not exist")
            im_files = sorted(x.replace("/", os.sep) for x in f if x.split(".")[-1].lower() in IMG_FORMATS)
            assert im_files, f"{self.prefix}No images found in {img_path}"
        except Exception as e:
            raise FileNotFoundError(f"{self.prefix}Error loading data from {img_path}") from e
        if self.fraction < 1:
            im_files = im_files[: round(len(im_files) * self.fraction)]
        return im_files

    def cache_path(self):
        return Path(self.label_files[0]).parent.with_suffix(".adrcache.npz")

    def cache_labels(self, path):
        """dataset.py:66-131, sequential, saved as plain arrays."""
        num_cls = len(self.data["names"]) if "names" in self.data else 1 << 30
        labels, msgs, nm, nf, ne, nc = [], [], 0, 0, 0, 0
        for im_file, lb_file in zip(self.im_files, self.label_files):
            f, lb, shape, a, b, c, d, msg = verify_image_label(im_file, lb_file, num_cls)
            nm, nf, ne, nc = nm + a, nf + b, ne + c, nc + d
            if f:
                labels.append({"im_file": f, "shape": shape, "cls": lb[:, 0:1], "bboxes": lb[:, 1:],
                               "normalized": True, "bbox_format": "xywh"})
            if msg:
                msgs.append(msg)
                warnings.warn(f"{self.prefix}{msg}", stacklevel=2)
        if nf == 0:
            warnings.warn(f"{self.prefix}WARNING No labels found in {path}", stacklevel=2)
        counts = np.array([len(lb["cls"]) for lb in labels], dtype=np.int64)
        rows = [np.concatenate([lb["cls"], lb["bboxes"]], 1) for lb in labels]
        try:
            np.savez(path, version=CACHE_VERSION, hash=get_hash(self.label_files + self.im_files),
                     im_files=np.array([lb["im_file"] for lb in labels], dtype=str),
                     shapes=np.array([lb["shape"] for lb in labels], dtype=np.int64).reshape(-1, 2), counts=counts,
                     rows=np.concatenate(rows, 0) if rows else np.zeros((0, 5), np.float32),
                     results=np.array([nf, nm, ne, nc, len(self.im_files)]), msgs=np.array(msgs, dtype=str))
        except OSError as e:
            warnings.warn(f"{self.prefix}label cache {path} not saved: {e}", stacklevel=2)
        return labels

    def load_label_cache(self, path):
        """The label records of a cache file whose hash matches the files as they are now, or None."""
        try:
            with np.load(path, allow_pickle=False) as z:
                if int(z["version"]) != CACHE_VERSION or str(z["hash"]) != get_hash(self.label_files + self.im_files):
                    return None
                files, shapes, counts, rows = z["im_files"], z["shapes"], z["counts"], z["rows"]
        except (OSError, KeyError, ValueError):
            return None
        labels, at = [], 0
        for f, s, n in zip(files, shapes, counts):
            lb = rows[at:at + int(n)]
            at += int(n)
            labels.append({"im_file": str(f), "shape": (int(s[0]), int(s[1])), "cls": lb[:, 0:1], "bboxes": lb[:, 1:],
                           "normalized": True, "bbox_format": "xywh"})
        return labels

    def get_labels(self):
        """dataset.py:133-172."""
        self.label_files = img2label_paths(self.im_files)
        path = self.cache_path()
        labels = self.load_label_cache(path)
        self.label_cache_hit = labels is not None
        if labels is None:
            labels = self.cache_labels(path)
        if not labels:
            warnings.warn(f"WARNING No images found in {path}, training may not work correctly", stacklevel=2)
        self.im_files = [lb["im_file"] for lb in labels]
        if sum(len(lb["cls"]) for lb in labels) == 0:
            warnings.warn(f"WARNING No labels found in {path}, training may not work correctly", stacklevel=2)
        return labels

    def update_labels(self, include_class):
        """base.py:132-149."""
        include_class_array = np.array(include_class).reshape(1, -1)
        for i in range(len(self.labels)):
            if include_class is not None:
                cls = self.labels[i]["cls"]
                j = (cls == include_class_array).any(1)
                self.labels[i]["cls"] = cls[j]
                self.labels[i]["bboxes"] = self.labels[i]["bboxes"][j]
            if self.single_cls:
                self.labels[i]["cls"][:, 0] = 0

    def set_rectangle(self):
        """base.py:261-284."""
        bi = np.floor(np.arange(self.ni) / self.batch_size).astype(int)
        nb = bi[-1] + 1
        s = np.array([x.pop("shape") for x in self.labels])
        ar = s[:, 0] / s[:, 1]
        irect = ar.argsort()
        self.im_files = [self.im_files[i] for i in irect]
        self.labels = [self.labels[i] for i in irect]
        self._shapes = [self._shapes[i] for i in irect]
        ar = ar[irect]
        shapes = [[1, 1]] * nb
        for i in range(nb):
            ari = ar[bi == i]
            mini, maxi = ari.min(), ari.max()
            if maxi < 1:
                shapes[i] = [maxi, 1]
            elif mini > 1:
                shapes[i] = [1, 1 / mini]
        self.batch_shapes = np.ceil(np.array(shapes) * self.imgsz / self.stride + self.pad).astype(int) * self.stride
        self.batch = bi

    # ---- images ----
    def pool_slots(self):
        """Images a cache=None pool must hold. Training: the buffer + the batches in flight, whose evicted images wait
        for their render. Only a load_image call that finds its image absent evicts, one image at most, and a sample
        makes one such call (its own index; the mosaic's other three come out of the buffer, resident by
        construction), or two with MixUp (hyp.mixup > 0: the second sample's random.randint index as well, whose
        mosaic again draws from the buffer): at most one, or two, evictions per sample. Validation: one batch more,
        since an image stays until the batch after its own has been rendered. `inflight` batches at most are begun
        and not yet ended: the loader admits a new batch only then (build.py DataLoader._admit)."""
        batches = self.inflight + (0 if self.augment else 1)
        loads = 2 if self.augment and not self.rect and getattr(self._hyp, "mixup", 0.0) > 0 else 1
        return self.max_buffer_length + batches * self.batch_size * loads

    def source_hw(self, i):
        """(h0, w0) of what load_bgr will return for image i: the sibling .npy's when there is one (the reference
        takes im.shape of whatever it loaded, base.py:155-167), otherwise the verified label record's."""
        if self._src_hw[i] is None:
            hw, fn = self._shapes[i], self.npy_files[i]
            if fn.exists():
                try:
                    hw = tuple(int(v) for v in np.load(fn, mmap_mode="r").shape[:2])
                except Exception:  # noqa: BLE001 - load_bgr falls back to the image file in the same way
                    pass
            self._src_hw[i] = hw
        return self._src_hw[i]

    def resized_hw(self, i):
        """(h, w) load_image leaves image i at (base.py:168-172)."""
        h0, w0 = self.source_hw(i)
        r = self.imgsz / max(h0, w0)
        if r != 1:
            return min(math.ceil(h0 * r), self.imgsz), min(math.ceil(w0 * r), self.imgsz)
        return h0, w0

    def _resident_bytes(self):
        from .pool import ALIGN
        return sum((h * w * 3 + ALIGN - 1) // ALIGN * ALIGN for h, w in map(self.resized_hw, range(self.ni)))

    def check_cache_gpu(self, device, cache_gb=None):
        """The counterpart of check_cache_ram: the exact size of the resident set against cache_gb (default: half of
        the device's free memory)."""
        import torch
        need = self._resident_bytes()
        budget = cache_gb * (1 << 30) if cache_gb is not None else torch.cuda.mem_get_info(device)[0] // 2
        if need > budget:
            warnings.warn(f"{self.prefix}{need / 2**30:.2f}GB of device memory required to cache the images but the "
                          f"budget is {budget / 2**30:.2f}GB, not caching images", stacklevel=2)
            return False
        return True

    def cache_images(self):
        """Every image loaded in index order (cache="gpu"); one flush resizes them all."""
        for i in range(self.ni):
            self.ims[i], self.im_hw0[i], self.im_hw[i] = self.load_image(i)
        self.pool.flush()

    def load_image(self, i, rect_mode=True):
        """base.py:151-187 with the image a queued DeviceImage: (image, (h0, w0), (h, w))."""
        im, f = self.ims[i], self.im_files[i]
        if im is None:
            if not rect_mode:
                raise NotImplementedError("load_image(rect_mode=False)")
            h0, w0 = self.source_hw(i)
            h, w = self.resized_hw(i)
            im = self.pool.image(h, w)
            self.pool.queue(im, lambda f=f: load_bgr(f), (h0, w0))
            if self.augment:
                self.ims[i], self.im_hw0[i], self.im_hw[i] = im, (h0, w0), (h, w)
                self.buffer.append(i)
                if 1 < len(self.buffer) >= self.max_buffer_length:  # prevent empty buffer
                    j = self.buffer.pop(0)
                    if self.cache != "gpu":
                        self._retire(self.ims[j], 0)
                        self.ims[j], self.im_hw0[j], self.im_hw[j] = None, None, None
            elif self.cache != "gpu":
                self._retire(im, 1)  # a validation image lives until the batch after its own has been rendered
            return im, (h0, w0), (h, w)
        return self.ims[i], self.im_hw0[i], self.im_hw[i]

    # An image that leaves (evicted from the buffer, or a validation image) may still be a tile of a sample that has
    # not been rendered, so its block goes back to the pool only once that batch has: begin_batch(k) names the batch
    # under construction, end_batch(k) (after batch k's render was enqueued) frees what was retired up to it. Stream
    # order then makes the reuse safe: the next resize into the block runs behind the render that read it. This does not
# depend on how many source images a sample has (four for a mosaic, up to eight for a MixUp of two mosaics, any of
# which a later load of the same sample may evict): a sample of batch k holds only images that were resident while it
# was built, so each of them is retired, if at all, under a batch number >= k, and batches end in order, after
# their render.
    def _retire(self, im, delay):
        with self._rlock:
            self._retired.append((self._seq + delay, im))

    def begin_batch(self, k):
        """Batch k is about to be built. Between begin_batch(k) and end_batch(k) the images it retires stay allocated,
        so a caller keeps at most `inflight` batches begun and not ended (the pool is sized for that)."""
        self._seq = k

    def end_batch(self, k):
        with self._rlock:
            gone = [im for s, im in self._retired if s <= k]
            self._retired = [(s, im) for s, im in self._retired if s > k]
        for im in gone:
            self.pool.release(im)
        return len(gone)

    # ---- samples ----
    def get_image_and_label(self, index):
        """base.py:290-301 + update_labels_info (dataset.py:204-227)."""
        label = deepcopy(self.labels[index])
        label.pop("shape", None)
        label["img"], label["ori_shape"], label["resized_shape"] = self.load_image(index)
        label["ratio_pad"] = (label["resized_shape"][0] / label["ori_shape"][0],
                              label["resized_shape"][1] / label["ori_shape"][1])
        if self.rect:
            label["rect_shape"] = self.batch_shapes[self.batch[index]]
        return self.update_labels_info(label)

    def update_labels_info(self, label):
        bboxes = label.pop("bboxes")
        bbox_format = label.pop("bbox_format")
        normalized = label.pop("normalized")
        segments = np.zeros((0, 1000, 2), dtype=np.float32)
        label["instances"] = Instances(bboxes, segments, None, bbox_format=bbox_format, normalized=normalized)
        return label

    def __getitem__(self, index):
        return self.transforms(self.get_image_and_label(index))

    def __len__(self):
        return len(self.labels)

    def build_transforms(self, hyp=None):
        return build_transforms(self, self.imgsz, hyp, self.augment)

    def close_mosaic(self, hyp):
        return close_mosaic(self, hyp)

    @staticmethod
    def collate_fn(batch, device="cuda"):
        return collate_fn(batch, device)
