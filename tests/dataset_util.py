"""Shared pieces of the YOLODataset tests (test infrastructure): the tiny dataset of tests/golden/dataset_tiny.npz
written back to a directory (scripts/gen_dataset_golden.py writes the very same tree for the reference), the seeded
passes' parameters, and a host stand-in for data/pool.py's DevicePool."""
import random
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
IMGSZ = 64
NAMES = {0: "a", 1: "b", 2: "c"}
# image name -> (w0, h0); sorted by name = the dataset's order. im8 is read from its .npy sibling (its PNG holds
# zeros); im9 is the corrupt pair (a coordinate > 1) that must be skipped.
SIZES = {"im1": (23, 17), "im2": (128, 96), "im3": (150, 97), "im4": (64, 40), "im5": (41, 131), "im6": (64, 64),
         "im7": (10, 10), "im8": (99, 33), "im9": (20, 30)}
NPY_ONLY = "im8"
LABEL_TEXTS = {
    "im1": "0 0.5 0.5 0.4 0.6\n1 0.3 0.3 0.2 0.2\n",
    "im2": "2 0.6 0.4 0.5 0.3\n0 0.25 0.75 0.3 0.4\n2 0.6 0.4 0.5 0.3\n1 0.5 0.5 0.9 0.9\n",  # a duplicated row
    "im3": "1 0.4 0.6 0.5 0.5\n0 0.8 0.2 0.3 0.3\n2 0.2 0.2 0.25 0.3\n",
    "im4": "",                                                                              # empty file
    "im5": None,                                                                            # missing file
    "im6": "0 0.5 0.5 0.8 0.8\n2 0.3 0.7 0.3 0.4\n",
    "im7": "1 0.5 0.5 0.6 0.6\n",
    "im8": "2 0.5 0.5 0.5 0.7\n0 0.2 0.4 0.3 0.5\n",
    "im9": "0 0.5 1.2 0.4 0.6\n",                                                          # corrupt: skipped
}
TRAIN = dict(seed=11, batch_size=1, order=[0, 1, 2, 3, 4, 5, 6, 7, 0, 3, 1, 6], collate=4)
RESIDENT_N = 4  # the resident (cache) training pass records the first 4 samples of TRAIN: one batch
CLOSE = dict(seed=12, order=[2, 5, 7, 4])
RECT = dict(batch_size=3, stride=32, pad=0.5)
CLASSES = [0, 2]
# adr_resize_u8 descriptors (src_off, dst_off, sw, sh, nw, nh, mode, tab_off) of a valid launch and its buffer sizes:
# the CPU tests reject one-rule violations of them, the GPU test launches them
RESIZE_GOOD = [(0, 0, 8, 8, 8, 8, 0, 0), (192, 256, 8, 8, 4, 4, 2, 0), (384, 512, 8, 8, 5, 3, 1, 0)]
RESIZE_SRC_BYTES, RESIZE_DST_BYTES, RESIZE_NTAB = 576, 768, 24


def hyp():
    sys.path.insert(0, str(ROOT / "oracle"))
    from recipe import AUG_HYPS
    return SimpleNamespace(**AUG_HYPS["default"], mask_ratio=4, overlap_mask=True, deterministic=True)


def make_image(name):
    """Seeded BGR uint8 image: smooth gradients plus rectangles, so that interpolation matters."""
    w, h = SIZES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rs.uniform(0, 6, 3)
    img = 127.5 + 70 * np.sin(xx[..., None] * 0.17 + yy[..., None] * 0.11 + ph) + 35 * np.cos(yy[..., None] * 0.23 - ph)
    for _ in range(3):
        x0, y0 = rs.randint(0, w - 2), rs.randint(0, h - 2)
        x1, y1 = x0 + 1 + rs.randint(0, max(1, w // 2)), y0 + 1 + rs.randint(0, max(1, h // 2))
        img[y0:y1, x0:x1] = rs.uniform(0, 255, 3)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def write_tree(root, images):
    """root/images/<name>.png + root/labels/<name>.txt from {name: BGR image}; returns root/images."""
    from PIL import Image
    (root / "images").mkdir(parents=True)
    (root / "labels").mkdir()
    for name, bgr in images.items():
        if name == NPY_ONLY:
            np.save(root / "images" / f"{name}.npy", bgr)
            bgr = np.zeros_like(bgr)
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(root / "images" / f"{name}.png")
        if LABEL_TEXTS[name] is not None:
            (root / "labels" / f"{name}.txt").write_text(LABEL_TEXTS[name])
    return root / "images"


def fixture_images(g):
    return {name: g[f"native_{name}"] for name in SIZES}


def seed(s):
    random.seed(s)
    np.random.seed(s)


class HostPool:
    """DevicePool's interface on the host: an image is a numpy array, filled at queue() with `resized(loader())`
    (default: the cv2.resize restatement of tests/letterbox_util.py). Counts what the dataset allocates and frees."""

    def __init__(self, lookup=None):
        self.lookup = lookup  # (h, w) -> array: the fixture's reference-resized images instead of a resize here
        self.live, self.allocs, self.frees, self.flushes = {}, 0, 0, 0

    def image(self, h, w):
        a = np.zeros((h, w, 3), np.uint8)
        self.live[id(a)] = a
        self.allocs += 1
        return a

    def queue(self, im, loader, src_hw=None):
        src = loader()
        assert src_hw is None or tuple(src.shape[:2]) == tuple(src_hw)
        if self.lookup is not None:
            im[...] = self.lookup(src, im.shape[:2])
        else:
            import letterbox_util as U
            im[...] = src if src.shape == im.shape else U.resize(src, (im.shape[1], im.shape[0]))

    def release(self, im):
        del self.live[id(im)]
        self.frees += 1

    def flush(self):
        self.flushes += 1
        return 0
