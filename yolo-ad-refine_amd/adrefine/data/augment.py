"""The v8 training augmentation chain (reference data/augment.py v8_transforms :2273-2335) with its pixel work on
the GPU.

The transforms keep the reference's classes, constructor arguments, RNG calls (python `random` / `np.random`, same
order, same count) and label arithmetic (numpy, bit-identical boxes through adrefine.data.instance). What they do
NOT do is touch pixels: `labels["img"]` is an ImagePlan — the recipe of the image (mosaic tiles over source images,
the warpAffine or warpPerspective matrix, MixUp's second layer and ratio, the HSV LUTs, the flips, the channel order)
— and `collate_fn` renders the whole batch with one launch of adr_augment_u8, or of adr_augment_mix_u8 when a sample of it is mixed
(csrc/adr_augment.hip), straight into the uint8 (B, 3, H, W) tensor the trainer reads
(FusedTrainer takes uint8 batches, /255 in the stem). The 2s x 2s mosaic canvas, the warped and the HSV images of
the reference never exist.

Covered (detection, the default hyp of cfg/default.yaml and any degrees / translate / scale / shear / flip / HSV
gains): Mosaic (n=4), CopyPaste (p=0 or no segments), RandomPerspective (perspective 0: warpAffine; perspective > 0:
warpPerspective, the float32 3x3 inverted in double on the host as cv::invert does, the per-pixel division in the
kernel), MixUp (any p: the second sample through the same pre_transform, np.random.beta(32, 32), labels concatenated, the float64 blend
(img1 * r + img2 * (1 - r)).astype(np.uint8) evaluated per pixel by the kernel, two products and a sum without FMA,
truncated), Albumentations (absent package: no-op, as in the reference without albumentations installed), RandomHSV,
RandomFlip, Format; LetterBox (every constructor argument; rect_shape, ratio_pad and the label update), as
RandomPerspective's pre_transform when mosaic is off (mosaic p < 1, close_mosaic), as the validation transform
(build_transforms with augment off) and on raw images of any size (render_letterbox, FusedPredictor.predict_images).
A LetterBox that only pads (the shape already equals new_unpad: every dataset-fed image, since
BaseDataset.load_image leaves the long side at imgsz) is a canvas with one tile and goes through adr_augment_u8 with
the rest of the chain; a LetterBox that resizes is rendered by adr_letterbox_u8 (csrc/adr_letterbox.hip: cv2.resize
INTER_LINEAR in OpenCV's fixed point + constant border + RGB / CHW). Not covered (raise): a LetterBox resize followed
by warp / HSV / flip in one plan (cannot arise from a dataset), CopyPaste with p > 0, mosaic9,
segments / keypoints. Source images come in resized as BaseDataset.load_image leaves them (data/base.py:151-190): host arrays (uploaded with the batch), or DeviceImages of one data/pool.py DevicePool,
decoded on the host once, resized by adr_resize_u8 and resident in HBM (data/dataset.py YOLODataset): then a batch
uploads descriptors and tables only."""
from __future__ import annotations

import copy
import ctypes
import math
import random

import numpy as np
import torch

from .instance import Instances

__all__ = ["ImagePlan", "Compose", "Mosaic", "CopyPaste", "RandomPerspective", "MixUp", "Albumentations", "RandomHSV",
           "RandomFlip", "LetterBox", "Format", "v8_transforms", "build_transforms", "close_mosaic", "collate_fn",
           "render", "render_letterbox", "warp_affine_tables", "warp_perspective_matrix", "resize_linear_tables"]


class ImagePlan:
    """A deferred uint8 BGR HWC image (see the module docstring). Stages must come in the chain's order:
    canvas (source / mosaic / letterbox) -> warp -> mix -> hsv -> flips -> channel order. A letterbox that resizes is
    a stage of its own (`resize`), followed by the channel order only. The mix stage (MixUp) holds a second layer: a
    plan of the same size with a canvas and at most a warp. The warp is M (warpAffine) or P (warpPerspective), never
    both; every stage rule treats them alike."""

    def __init__(self, src: np.ndarray):
        if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3:
            raise ValueError("ImagePlan: sources are HWC BGR uint8 images")
        h, w = src.shape[:2]
        self.tiles = [(src, 0, 0, w, h, 0, 0)]  # (source, x1a, y1a, x2a, y2a, x1b, y1b) on the canvas
        self.canvas = (w, h)
        self.size = (w, h)  # current (w, h)
        self.resize = None  # (nw, nh, left, top): LetterBox's cv2.resize of the canvas to (nw, nh), placed at (left, top)
        self.ratio_pad = None  # LetterBox: ((ratio_w, ratio_h), (left, top))
        self.M = None  # 2x3 float32 warpAffine matrix (canvas -> output)
        self.P = None  # 3x3 float32 warpPerspective matrix (canvas -> output); at most one of M and P
        self.mix = None  # MixUp: (second layer ImagePlan, r, 1 - r), both ratios float64 from the host
        self.lut = None  # (3, 256) uint8
        self.flip_ud = self.flip_lr = False
        self.rgb = False

    @property
    def shape(self):
        return (self.size[1], self.size[0], 3)

    def _stage(self, ok, what):
        if self.resize is not None:
            raise NotImplementedError(f"ImagePlan: {what} after a LetterBox that resizes (cv2.resize is not fused into "
                                      "the later stages; images from a dataset are already at new_unpad: pad only)")
        if not ok or (self.mix is not None and what not in ("hsv", "flip")):
            raise NotImplementedError(f"ImagePlan: {what} out of the supported chain order")

    def _layer_only(self):
        """Canvas and at most a warp: what a layer of a mix may be."""
        return self.lut is None and not (self.flip_ud or self.flip_lr) and self.resize is None and self.mix is None

    def layers(self):
        """The plans whose tiles the image reads: itself, and the second layer of a mix."""
        return (self,) if self.mix is None else (self, self.mix[0])

    def mixup(self, second, r):
        """(img1 * r + img2 * (1 - r)).astype(np.uint8) (MixUp._mix_transform, augment.py:943-945) with this plan as
        img1: uint8 arrays times a float64, so two float64 products and a float64 sum, truncated. 1 - r is taken here,
        in float64, once."""
        self._stage(self._layer_only(), "mix")
        second._stage(second._layer_only(), "mix")
        if second.size != self.size:
            raise NotImplementedError(f"ImagePlan: mix of images of sizes {self.size} and {second.size}")
        r = float(r)
        self.mix = (second, r, 1 - r)

    def letterbox(self, new_unpad, left, top, right, bottom):
        """The plan of cv2.copyMakeBorder(cv2.resize(image, new_unpad) if its size differs, top, bottom, left, right,
        114) (LetterBox, augment.py:1583-1589) — a new plan; this one is unchanged."""
        self._stage(self.M is None and self.P is None and self.lut is None and not (self.flip_ud or self.flip_lr),
                    "letterbox")
        q = copy.copy(self)
        w, h = self.size
        nw, nh = (int(v) for v in new_unpad)
        if (w, h) == (nw, nh):  # pad only: the canvas grows, its tiles move
            q.tiles = [(s, x1a + left, y1a + top, x2a + left, y2a + top, x1b, y1b)
                       for s, x1a, y1a, x2a, y2a, x1b, y1b in self.tiles]
            q.canvas = q.size = (w + left + right, h + top + bottom)
        else:
            src = self.tiles[0][0] if len(self.tiles) == 1 else None
            if src is None or self.tiles[0][1:] != (0, 0, src.shape[1], src.shape[0], 0, 0) or self.canvas != (w, h):
                raise NotImplementedError("ImagePlan: a LetterBox resize of anything but one whole source image")
            if nw <= 0 or nh <= 0:
                raise ValueError(f"LetterBox: empty resized image {nw} x {nh}")
            q.tiles = list(self.tiles)
            q.resize = (nw, nh, left, top)
            q.size = (nw + left + right, nh + top + bottom)
        return q


def _is_device(src):
    """A source image resident in a DevicePool (data/pool.py DeviceImage) instead of a host array."""
    return hasattr(src, "pool") and hasattr(src, "off")


def _plan(img):
    if isinstance(img, ImagePlan):
        return img
    return ImagePlan(img if _is_device(img) else np.ascontiguousarray(img))


def _source_pool(plans, what):
    """The DevicePool every tile source of the batch (of both layers of a mixed image) lives in, or None when all of
    them are host arrays."""
    srcs = [t[0] for p in plans for q in p.layers() for t in q.tiles]
    dev = [s for s in srcs if _is_device(s)]
    if not dev:
        return None
    if len(dev) != len(srcs):
        raise ValueError(f"{what}: the batch mixes host and device-resident source images")
    pool = dev[0].pool
    if any(s.pool is not pool for s in dev):
        raise ValueError(f"{what}: the batch's device-resident source images come from two pools")
    if any(s.off is None for s in dev):
        raise ValueError(f"{what}: a source image was released from its pool")
    return pool


def _same_device(a, b):
    """torch.device("cuda") names the current device: equal to any index of its type."""
    return a.type == b.type and (a.index is None or b.index is None or a.index == b.index)


class Compose:
    """augment.py:146-316 (call, append, insert)."""

    def __init__(self, transforms):
        self.transforms = transforms if isinstance(transforms, list) else [transforms]

    def __call__(self, data):
        for t in self.transforms:
            data = t(data)
        return data

    def append(self, transform):
        self.transforms.append(transform)

    def insert(self, index, transform):
        self.transforms.insert(index, transform)


class BaseMixTransform:
    """augment.py:318-435."""

    def __init__(self, dataset, pre_transform=None, p=0.0):
        self.dataset, self.pre_transform, self.p = dataset, pre_transform, p

    def __call__(self, labels):
        if random.uniform(0, 1) > self.p:
            return labels
        indexes = self.get_indexes()
        if isinstance(indexes, int):
            indexes = [indexes]
        mix_labels = [self.dataset.get_image_and_label(i) for i in indexes]
        if self.pre_transform is not None:
            for i, data in enumerate(mix_labels):
                mix_labels[i] = self.pre_transform(data)
        labels["mix_labels"] = mix_labels
        if "texts" in labels:
            raise NotImplementedError("multi-modal texts")
        labels = self._mix_transform(labels)
        labels.pop("mix_labels", None)
        return labels


class Mosaic(BaseMixTransform):
    """augment.py:489-865, the 2x2 mosaic (_mosaic4 :657-713, _update_labels :788-812, _cat_labels :814-864)."""

    def __init__(self, dataset, imgsz=640, p=1.0, n=4):
        assert 0 <= p <= 1.0 and n in {4, 9}
        if n != 4:
            raise NotImplementedError("Mosaic n=9 (only the 2x2 mosaic of v8_transforms)")
        super().__init__(dataset=dataset, p=p)
        self.imgsz = imgsz
        self.border = (-imgsz // 2, -imgsz // 2)
        self.n = n

    def get_indexes(self, buffer=True):
        if buffer:
            return random.choices(list(self.dataset.buffer), k=self.n - 1)
        return [random.randint(0, len(self.dataset) - 1) for _ in range(self.n - 1)]

    def _mix_transform(self, labels):
        assert labels.get("rect_shape", None) is None, "rect and mosaic are mutually exclusive."
        assert len(labels.get("mix_labels", [])), "There are no other images for mosaic augment."
        return self._mosaic4(labels)

    def _mosaic4(self, labels):
        mosaic_labels = []
        s = self.imgsz
        yc, xc = (int(random.uniform(-x, 2 * s + x)) for x in self.border)
        plan = None
        for i in range(4):
            patch = labels if i == 0 else labels["mix_labels"][i - 1]
            src = _plan(patch["img"])
            if len(src.tiles) != 1 or src.M is not None or src.P is not None or src.lut is not None \
                    or src.resize is not None or src.mix is not None:
                raise NotImplementedError("Mosaic tiles must be untransformed source images")
            img = src.tiles[0][0]
            h, w = patch.pop("resized_shape")
            if i == 0:
                plan = ImagePlan(img)
                plan.tiles, plan.canvas, plan.size = [], (2 * s, 2 * s), (2 * s, 2 * s)
                x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
                x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h
            elif i == 1:
                x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
                x1b, y1b, x2b, y2b = 0, h - (y2a - y1a), min(w, x2a - x1a), h
            elif i == 2:
                x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
                x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, min(y2a - y1a, h)
            else:
                x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
                x1b, y1b, x2b, y2b = 0, 0, min(w, x2a - x1a), min(y2a - y1a, h)
            # img4[y1a:y2a, x1a:x2a] = img[y1b:y2b, x1b:x2b]: numpy slice semantics (empty when reversed)
            if x2a > x1a and y2a > y1a and x2b > x1b and y2b > y1b:
                plan.tiles.append((img, x1a, y1a, x2a, y2a, x1b, y1b))
            padw, padh = x1a - x1b, y1a - y1b
            patch["img"] = img  # _update_labels reads its shape
            ins = patch["instances"]
            nh, nw = img.shape[:2]
            ins.convert_bbox(format="xyxy")
            ins.denormalize(nw, nh)
            ins.add_padding(padw, padh)
            mosaic_labels.append(patch)
        final = self._cat_labels(mosaic_labels)
        final["img"] = plan
        return final

    def _cat_labels(self, mosaic_labels):
        if len(mosaic_labels) == 0:
            return {}
        imgsz = self.imgsz * 2
        final = {
            "im_file": mosaic_labels[0]["im_file"],
            "ori_shape": mosaic_labels[0]["ori_shape"],
            "resized_shape": (imgsz, imgsz),
            "cls": np.concatenate([m["cls"] for m in mosaic_labels], 0),
            "instances": Instances.concatenate([m["instances"] for m in mosaic_labels], axis=0),
            "mosaic_border": self.border,
        }
        final["instances"].clip(imgsz, imgsz)
        good = final["instances"].remove_zero_area_boxes()
        final["cls"] = final["cls"][good]
        return final


class CopyPaste(BaseMixTransform):
    """augment.py:1631-1729: a no-op without segments or with p = 0 (the detection default)."""

    def __init__(self, dataset=None, pre_transform=None, p=0.5, mode="flip"):
        super().__init__(dataset=dataset, pre_transform=pre_transform, p=p)
        self.mode = mode

    def __call__(self, labels):
        if len(labels["instances"].segments) == 0 or self.p == 0:
            return labels
        raise NotImplementedError("CopyPaste with segments")


class MixUp(BaseMixTransform):
    """augment.py:866-949: the second sample goes through pre_transform (its own mosaic / letterbox and warp draws),
    np.random.beta gives the ratio, the labels are concatenated; the blend becomes the plan's mix stage."""

    def __init__(self, dataset, pre_transform=None, p=0.0):
        super().__init__(dataset=dataset, pre_transform=pre_transform, p=p)

    def get_indexes(self):
        return random.randint(0, len(self.dataset) - 1)

    def _mix_transform(self, labels):
        r = np.random.beta(32.0, 32.0)  # mixup ratio, alpha=beta=32.0
        labels2 = labels["mix_labels"][0]
        img = _plan(labels["img"])
        img.mixup(_plan(labels2["img"]), r)
        labels["img"] = img
        labels["instances"] = Instances.concatenate([labels["instances"], labels2["instances"]], axis=0)
        labels["cls"] = np.concatenate([labels["cls"], labels2["cls"]], 0)
        return labels


class Albumentations:
    """augment.py:1732-1918 without the albumentations package: `transform is None`, so no draw and no change."""

    def __init__(self, p=1.0):
        self.p, self.transform = p, None

    def __call__(self, labels):
        return labels


class RandomPerspective:
    """augment.py:951-1298: perspective 0 plans cv2.warpAffine (plan.M = M[:2]), perspective != 0 plans
    cv2.warpPerspective (plan.P = M, the whole float32 3x3); the draws and the box arithmetic are the same either
    way, as in the reference."""

    def __init__(self, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0, border=(0, 0),
                 pre_transform=None):
        self.degrees, self.translate, self.scale, self.shear = degrees, translate, scale, shear
        self.perspective, self.border, self.pre_transform = perspective, border, pre_transform

    def affine_transform(self, img, border):
        """augment.py:1016-1077: the same float32 matrices, multiplied in the same order."""
        C = np.eye(3, dtype=np.float32)
        C[0, 2] = -img.shape[1] / 2
        C[1, 2] = -img.shape[0] / 2
        P = np.eye(3, dtype=np.float32)
        P[2, 0] = random.uniform(-self.perspective, self.perspective)
        P[2, 1] = random.uniform(-self.perspective, self.perspective)
        R = np.eye(3, dtype=np.float32)
        a = random.uniform(-self.degrees, self.degrees)
        s = random.uniform(1 - self.scale, 1 + self.scale)
        R[:2] = rotation_matrix_2d(a, s)
        S = np.eye(3, dtype=np.float32)
        S[0, 1] = math.tan(random.uniform(-self.shear, self.shear) * math.pi / 180)
        S[1, 0] = math.tan(random.uniform(-self.shear, self.shear) * math.pi / 180)
        T = np.eye(3, dtype=np.float32)
        T[0, 2] = random.uniform(0.5 - self.translate, 0.5 + self.translate) * self.size[0]
        T[1, 2] = random.uniform(0.5 - self.translate, 0.5 + self.translate) * self.size[1]
        M = T @ S @ R @ P @ C
        if (border[0] != 0) or (border[1] != 0) or (M != np.eye(3)).any():
            img._stage(img.M is None and img.P is None and img.lut is None and not (img.flip_ud or img.flip_lr),
                       "warp")
            if self.perspective:
                img.P = M.copy()  # cv2.warpPerspective(img, M): the whole matrix, its third row included
            else:
                img.M = M[:2].copy()
            img.size = tuple(self.size)
        return img, M, s

    def apply_bboxes(self, bboxes, M):
        n = len(bboxes)
        if n == 0:
            return bboxes
        xy = np.ones((n * 4, 3), dtype=bboxes.dtype)
        xy[:, :2] = bboxes[:, [0, 1, 2, 3, 0, 3, 2, 1]].reshape(n * 4, 2)
        xy = xy @ M.T
        xy = (xy[:, :2] / xy[:, 2:3] if self.perspective else xy[:, :2]).reshape(n, 8)
        x = xy[:, [0, 2, 4, 6]]
        y = xy[:, [1, 3, 5, 7]]
        return np.concatenate((x.min(1), y.min(1), x.max(1), y.max(1)), dtype=bboxes.dtype).reshape(4, n).T

    def __call__(self, labels):
        if self.pre_transform and "mosaic_border" not in labels:
            labels = self.pre_transform(labels)
        labels.pop("ratio_pad", None)
        img = _plan(labels["img"])
        cls = labels["cls"]
        instances = labels.pop("instances")
        instances.convert_bbox(format="xyxy")
        instances.denormalize(*img.shape[:2][::-1])
        border = labels.pop("mosaic_border", self.border)
        self.size = img.shape[1] + border[1] * 2, img.shape[0] + border[0] * 2
        img, M, scale = self.affine_transform(img, border)
        bboxes = self.apply_bboxes(instances.bboxes, M)
        new_instances = Instances(bboxes, None, None, bbox_format="xyxy", normalized=False)
        new_instances.clip(*self.size)
        instances.scale(scale_w=scale, scale_h=scale, bbox_only=True)
        i = self.box_candidates(box1=instances.bboxes.T, box2=new_instances.bboxes.T, area_thr=0.10)
        labels["instances"] = new_instances[i]
        labels["cls"] = cls[i]
        labels["img"] = img
        labels["resized_shape"] = img.shape[:2]
        return labels

    @staticmethod
    def box_candidates(box1, box2, wh_thr=2, ar_thr=100, area_thr=0.1, eps=1e-16):
        w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
        w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
        ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
        return (w2 > wh_thr) & (h2 > wh_thr) & (w2 * h2 / (w1 * h1 + eps) > area_thr) & (ar < ar_thr)


def rotation_matrix_2d(angle, scale):
    """cv2.getRotationMatrix2D(center=(0, 0), angle, scale) in double (imgwarp.cpp: angle *= CV_PI/180)."""
    a = angle * (math.pi / 180)
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    return np.array([[alpha, beta, 0.0], [-beta, alpha, 0.0]], dtype=np.float64)


class RandomHSV:
    """augment.py:1301-1378: the gains and LUTs as the reference computes them; pixels on the GPU."""

    def __init__(self, hgain=0.5, sgain=0.5, vgain=0.5):
        self.hgain, self.sgain, self.vgain = hgain, sgain, vgain

    def __call__(self, labels):
        img = _plan(labels["img"])
        if self.hgain or self.sgain or self.vgain:
            r = np.random.uniform(-1, 1, 3) * [self.hgain, self.sgain, self.vgain] + 1
            x = np.arange(0, 256, dtype=r.dtype)
            lut_hue = ((x * r[0]) % 180).astype(np.uint8)
            lut_sat = np.clip(x * r[1], 0, 255).astype(np.uint8)
            lut_val = np.clip(x * r[2], 0, 255).astype(np.uint8)
            img._stage(img.lut is None and not (img.flip_ud or img.flip_lr), "hsv")
            img.lut = np.stack([lut_hue, lut_sat, lut_val])
        labels["img"] = img
        return labels


class RandomFlip:
    """augment.py:1381-1472 (boxes; no keypoints)."""

    def __init__(self, p=0.5, direction="horizontal", flip_idx=None):
        assert direction in {"horizontal", "vertical"} and 0 <= p <= 1.0
        self.p, self.direction, self.flip_idx = p, direction, flip_idx

    def __call__(self, labels):
        img = _plan(labels["img"])
        instances = labels.pop("instances")
        instances.convert_bbox(format="xywh")
        h, w = img.shape[:2]
        h = 1 if instances.normalized else h
        w = 1 if instances.normalized else w
        if self.direction == "vertical" and random.random() < self.p:
            img._stage(True, "flip")
            img.flip_ud = not img.flip_ud
            instances.flipud(h)
        if self.direction == "horizontal" and random.random() < self.p:
            img._stage(True, "flip")
            img.flip_lr = not img.flip_lr
            instances.fliplr(w)
        labels["img"] = img
        labels["instances"] = instances
        return labels


class LetterBox:
    """augment.py:1475-1640: the reference's arithmetic in the reference's order; the image becomes an ImagePlan
    (pad only: a canvas with the image at (left, top); otherwise a resize stage for adr_letterbox_u8)."""

    def __init__(self, new_shape=(640, 640), auto=False, scaleFill=False, scaleup=True, center=True, stride=32):
        self.new_shape = new_shape
        self.auto = auto
        self.scaleFill = scaleFill
        self.scaleup = scaleup
        self.stride = stride
        self.center = center

    def __call__(self, labels=None, image=None):
        """labels -> labels with labels["img"] the letterboxed plan; image= alone -> the plan
        (plan.ratio_pad = ((ratio_w, ratio_h), (left, top)))."""
        if labels is None:
            labels = {}
        img = _plan(labels.get("img") if image is None else image)
        shape = img.shape[:2]  # current shape [height, width]
        new_shape = labels.pop("rect_shape", self.new_shape)
        if isinstance(new_shape, int):
            new_shape = (new_shape, new_shape)
        r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
        if not self.scaleup:
            r = min(r, 1.0)
        ratio = r, r
        new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
        dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
        if self.auto:
            dw, dh = np.mod(dw, self.stride), np.mod(dh, self.stride)
        elif self.scaleFill:
            dw, dh = 0.0, 0.0
            new_unpad = (new_shape[1], new_shape[0])
            ratio = new_shape[1] / shape[1], new_shape[0] / shape[0]
        if self.center:
            dw /= 2
            dh /= 2
        top, bottom = int(round(dh - 0.1)) if self.center else 0, int(round(dh + 0.1))
        left, right = int(round(dw - 0.1)) if self.center else 0, int(round(dw + 0.1))
        out = img.letterbox(new_unpad, left, top, right, bottom)
        out.ratio_pad = (ratio, (left, top))
        if labels.get("ratio_pad"):
            labels["ratio_pad"] = (labels["ratio_pad"], (left, top))  # for evaluation
        if len(labels):
            labels["img"] = img  # _update_labels denormalises with the shape before the letterbox
            labels = self._update_labels(labels, ratio, dw, dh)
            labels["img"] = out
            labels["resized_shape"] = new_shape
            return labels
        return out

    def _update_labels(self, labels, ratio, padw, padh):
        labels["instances"].convert_bbox(format="xyxy")
        labels["instances"].denormalize(*labels["img"].shape[:2][::-1])
        labels["instances"].scale(*ratio)
        labels["instances"].add_padding(padw, padh)
        return labels


class Format:
    """augment.py:1920-2100 for detection (xywh, normalised, batch_idx); the image stays a plan until collate."""

    def __init__(self, bbox_format="xywh", normalize=True, return_mask=False, return_keypoint=False,
                 return_obb=False, mask_ratio=4, mask_overlap=True, batch_idx=True, bgr=0.0):
        if return_mask or return_keypoint or return_obb:
            raise NotImplementedError("Format: detection boxes only")
        self.bbox_format, self.normalize, self.batch_idx, self.bgr = bbox_format, normalize, batch_idx, bgr

    def __call__(self, labels):
        img = _plan(labels.pop("img"))
        h, w = img.shape[:2]
        cls = labels.pop("cls")
        instances = labels.pop("instances")
        instances.convert_bbox(format=self.bbox_format)
        instances.denormalize(w, h)
        nl = len(instances)
        img.rgb = random.uniform(0, 1) > self.bgr  # _format_img: img[::-1] (BGR -> RGB) unless bgr wins
        labels["img"] = img
        labels["cls"] = torch.from_numpy(cls) if nl else torch.zeros(nl)
        labels["bboxes"] = torch.from_numpy(instances.bboxes) if nl else torch.zeros((nl, 4))
        if self.normalize:
            labels["bboxes"][:, [0, 2]] /= w
            labels["bboxes"][:, [1, 3]] /= h
        if self.batch_idx:
            labels["batch_idx"] = torch.zeros(nl)
        return labels


def v8_transforms(dataset, imgsz, hyp, stretch=False):
    """augment.py:2273-2335 (detection: no keypoints, copy_paste_mode 'flip' or p = 0)."""
    mosaic = Mosaic(dataset, imgsz=imgsz, p=hyp.mosaic)
    affine = RandomPerspective(degrees=hyp.degrees, translate=hyp.translate, scale=hyp.scale, shear=hyp.shear,
                               perspective=hyp.perspective,
                               pre_transform=None if stretch else LetterBox(new_shape=(imgsz, imgsz)))
    pre_transform = Compose([mosaic, affine])
    if hyp.copy_paste_mode == "flip":
        pre_transform.insert(1, CopyPaste(p=hyp.copy_paste, mode=hyp.copy_paste_mode))
    else:
        pre_transform.append(CopyPaste(dataset, pre_transform=None, p=hyp.copy_paste, mode=hyp.copy_paste_mode))
    return Compose([
        pre_transform,
        MixUp(dataset, pre_transform=pre_transform, p=hyp.mixup),
        Albumentations(p=1.0),
        RandomHSV(hgain=hyp.hsv_h, sgain=hyp.hsv_s, vgain=hyp.hsv_v),
        RandomFlip(direction="vertical", p=hyp.flipud),
        RandomFlip(direction="horizontal", p=hyp.fliplr, flip_idx=None),
    ])


def build_transforms(dataset, imgsz, hyp, augment=True):
    """YOLODataset.build_transforms (data/dataset.py:174-195) for detection: the training chain, or the validation
    LetterBox(scaleup=False), followed by Format."""
    if augment:
        rect = getattr(dataset, "rect", False)
        hyp.mosaic = hyp.mosaic if augment and not rect else 0.0
        hyp.mixup = hyp.mixup if augment and not rect else 0.0
        transforms = v8_transforms(dataset, imgsz, hyp)
    else:
        transforms = Compose([LetterBox(new_shape=(imgsz, imgsz), scaleup=False)])
    transforms.append(Format(bbox_format="xywh", normalize=True, return_mask=getattr(dataset, "use_segments", False),
                             return_keypoint=getattr(dataset, "use_keypoints", False),
                             return_obb=getattr(dataset, "use_obb", False), batch_idx=True,
                             mask_ratio=getattr(hyp, "mask_ratio", 4), mask_overlap=getattr(hyp, "overlap_mask", True),
                             bgr=hyp.bgr if augment else 0.0))
    return transforms


def close_mosaic(dataset, hyp):
    """YOLODataset.close_mosaic (data/dataset.py:197-202; the trainer calls it for the last `close_mosaic` epochs,
    engine/trainer.py:749-751): mosaic, copy_paste and mixup off, dataset.transforms rebuilt."""
    hyp.mosaic = 0.0
    hyp.copy_paste = 0.0
    hyp.mixup = 0.0
    dataset.transforms = build_transforms(dataset, dataset.imgsz, hyp, getattr(dataset, "augment", True))
    return dataset.transforms


def resize_linear_tables(s, n):
    """cv::resize's 8-bit INTER_LINEAR coefficients of one axis, source length s -> n (imgproc/resize.cpp, restated:
    PARITY UNPINNED against real OpenCV): scale = 1 / (n / s) in double, f = (float)((d + 0.5) * scale - 0.5),
    i = floor(f), f -= i; i < 0 -> (0, 0), i >= s - 1 -> (s - 1, 0); (short)cvRound((1.f - f) * 2048) and
    (short)cvRound(f * 2048) (INTER_RESIZE_COEF_BITS 11, round half to even). Returns (i, c0, c1) int32 arrays."""
    scale = 1.0 / (n / s)
    f = ((np.arange(n, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    i = np.floor(f).astype(np.int64)
    f = f - i.astype(np.float32)
    lo, hi = i < 0, i >= s - 1
    f[lo | hi] = 0
    i[lo] = 0
    i[hi] = s - 1
    one, coef = np.float32(1.0), np.float32(2048.0)
    c0 = np.clip(np.rint((one - f) * coef), -32768, 32767)
    c1 = np.clip(np.rint(f * coef), -32768, 32767)
    return i.astype(np.int32), c0.astype(np.int32), c1.astype(np.int32)


def warp_affine_tables(M, dsize):
    """cv::warpAffine's fixed-point source coordinates (INTER_LINEAR; imgwarp.cpp WarpAffineInvoker): the 2x3 matrix
    in double, inverted as warpAffine does, then adelta[x] = cvRound(M0*x*1024), bdelta[x] = cvRound(M3*x*1024),
    X0[y] = cvRound((M1*y + M2)*1024) + 16, Y0[y] = cvRound((M4*y + M5)*1024) + 16 (AB_BITS 10, round_delta 16);
    the kernel takes X = (X0 + adelta) >> 5 (INTER_BITS 5)."""
    m = np.asarray(M, dtype=np.float64).reshape(6).copy()
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0], m[4] = A11, A22
    m[1] *= -D
    m[3] *= -D
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    W, H = dsize
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    return (np.rint(m[0] * xs * 1024).astype(np.int64), np.rint(m[3] * xs * 1024).astype(np.int64),
            np.rint((m[1] * ys + m[2]) * 1024).astype(np.int64) + 16,
            np.rint((m[4] * ys + m[5]) * 1024).astype(np.int64) + 16)


def warp_perspective_matrix(P):
    """The nine coefficients cv::warpPerspective iterates with (imgwarp.cpp, restated: PARITY UNPINNED against real
    OpenCV): the float32 3x3 matrix converted to double and inverted by cv::invert's closed 3x3 form (determinant by
    the first row, d = 1 / det, the adjugate's entries times d; a zero determinant gives the zero matrix), every
    product and difference rounded on its own (Python floats: no FMA). Returns a float64 array of 9."""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (float(v) for v in np.asarray(P, dtype=np.float32).reshape(9))
    det = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20)
    if det == 0:
        return np.zeros(9, dtype=np.float64)
    d = 1.0 / det
    return np.array([(m11 * m22 - m12 * m21) * d, (m02 * m21 - m01 * m22) * d, (m01 * m12 - m02 * m11) * d,
                     (m12 * m20 - m10 * m22) * d, (m00 * m22 - m02 * m20) * d, (m02 * m10 - m00 * m12) * d,
                     (m10 * m21 - m11 * m20) * d, (m01 * m20 - m00 * m21) * d, (m00 * m11 - m01 * m10) * d],
                    dtype=np.float64)


class _Tile(ctypes.Structure):
    _fields_ = [("off", ctypes.c_int64)] + [(n, ctypes.c_int) for n in ("sw", "x1a", "y1a", "x2a", "y2a", "x1b", "y1b")]


class AugDesc(ctypes.Structure):
    """adr_aug_desc (include/adr.h)."""
    _fields_ = [("tile", _Tile * 4)] + [(n, ctypes.c_int) for n in (
        "ntile", "cw", "ch", "warp", "tab_off", "lut_off", "flip_ud", "flip_lr", "rgb", "pad_")]


class AugMix(ctypes.Structure):
    """adr_augment_mix_u8's per-image record (include/adr.h)."""
    _fields_ = [("second", ctypes.c_int), ("pad_", ctypes.c_int), ("r", ctypes.c_double),
                ("one_minus_r", ctypes.c_double)]


def render(plans, device="cuda", out=None):
    """Run adr_augment_u8 for a list of ImagePlans of one output size, or adr_augment_mix_u8 when one of them has a
    mix stage: returns the uint8 (B, 3, H, W) batch."""
    from ..native import lib
    from ..kernels import stream

    if ctypes.sizeof(AugDesc) != lib.adr_augment_desc_size():
        raise RuntimeError("adr_aug_desc layout mismatch between adrefine and libadr_hip")
    B = len(plans)
    W, H = plans[0].size
    if any(p.size != (W, H) for p in plans):
        raise ValueError("render: every image of a batch must have the same size")
    if any(p.resize is not None for p in plans):
        raise ValueError("render: a LetterBox resize is rendered by render_letterbox (adr_letterbox_u8)")
    mixed = [b for b, p in enumerate(plans) if p.mix is not None]
    if mixed and ctypes.sizeof(AugMix) != lib.adr_augment_mix_desc_size():
        raise RuntimeError("adr_augment_mix_u8's mix record layout mismatch between adrefine and libadr_hip")
    for b in mixed:
        q = plans[b].mix[0]
        if q.size != (W, H) or not q._layer_only():
            raise ValueError(f"render: image {b}'s second layer is not a canvas / warp plan of the batch's size")
    resident = _source_pool(plans, "render")  # sources already in HBM: no pixels are uploaded
    if resident is not None:
        if out is not None and not _same_device(out.device, resident.device):
            raise ValueError("render: out is not on the device of the source images' pool")
        resident.flush()
        device = resident.device
    srcs, index = [], {}
    descs = (AugDesc * (B + len(mixed)))()  # the images' own descriptors, then the second layers'
    mix = (AugMix * B)()
    tabs, luts = [], []
    off = ntab = 0

    def layer(d, p):  # canvas and warp of one layer; a source shared by layers or images is uploaded once
        nonlocal off, ntab
        if len(p.tiles) > 4:
            raise ValueError("render: at most four tiles per image")
        d.ntile = len(p.tiles)
        for k, (src, x1a, y1a, x2a, y2a, x1b, y1b) in enumerate(p.tiles):
            key = id(src)
            if key not in index:
                if resident is not None:
                    index[key] = src.off
                else:
                    index[key] = off
                    srcs.append(np.ascontiguousarray(src).reshape(-1))
                    off += src.size
            t = d.tile[k]
            t.off, t.sw = index[key], src.shape[1]
            t.x1a, t.y1a, t.x2a, t.y2a, t.x1b, t.y1b = x1a, y1a, x2a, y2a, x1b, y1b
        d.cw, d.ch = p.canvas
        if p.M is not None and p.P is not None:
            raise ValueError("render: a plan has a warpAffine and a warpPerspective matrix")
        d.warp = int(p.M is not None)
        if p.M is not None:
            tab = np.concatenate(warp_affine_tables(p.M, (W, H)))
            if np.abs(tab).max() >= 2 ** 31:
                raise ValueError("render: warp coordinates out of int32 range")
            d.tab_off = ntab
            tabs.append(tab.astype(np.int32))
            ntab += tab.size
        elif p.P is not None:  # warp 2: nine doubles inside the int tables, at an even (8-byte aligned) offset
            t = warp_perspective_matrix(p.P)
            if not np.isfinite(t).all():
                raise ValueError("render: the inverse of a warpPerspective matrix is not finite")
            if ntab & 1:
                tabs.append(np.zeros(1, np.int32))
                ntab += 1
            d.warp, d.tab_off = 2, ntab
            tabs.append(t.view(np.int32))
            ntab += 18
        d.lut_off = -1

    for b, p in enumerate(plans):
        d = descs[b]
        layer(d, p)
        d.lut_off = -1 if p.lut is None else 768 * len(luts)
        if p.lut is not None:
            luts.append(p.lut.reshape(-1))
        d.flip_ud, d.flip_lr, d.rgb = int(p.flip_ud), int(p.flip_lr), int(p.rgb)
        mix[b].second = -1
    for k, b in enumerate(mixed):
        q, r, one_minus_r = plans[b].mix
        layer(descs[B + k], q)
        mix[b].second, mix[b].r, mix[b].one_minus_r = B + k, r, one_minus_r
    if resident is not None:
        pool = resident.tensor
    else:
        pool = torch.from_numpy(np.concatenate(srcs)).to(device, non_blocking=True)
    dd = torch.frombuffer(bytearray(descs), dtype=torch.uint8).to(device, non_blocking=True)
    tb = torch.from_numpy(np.concatenate(tabs) if tabs else np.zeros(1, np.int32)).to(device, non_blocking=True)
    lt = torch.from_numpy(np.concatenate(luts) if luts else np.zeros(1, np.uint8)).to(device, non_blocking=True)
    if out is None:
        out = torch.empty(B, 3, H, W, dtype=torch.uint8, device=device)
    if not mixed:  # the launch a batch without MixUp has always taken
        lib.adr_augment_u8(ctypes.c_void_p(pool.data_ptr()), ctypes.c_void_p(dd.data_ptr()), B,
                           ctypes.c_void_p(tb.data_ptr()), ctypes.c_void_p(lt.data_ptr()),
                           ctypes.c_void_p(out.data_ptr()), H, W, stream())
        out._adr_keep = (pool, dd, tb, lt)  # the inputs live until the launch has read them (stream order)
        return out
    mm = torch.frombuffer(bytearray(mix), dtype=torch.uint8).to(device, non_blocking=True)
    lib.adr_augment_mix_u8(ctypes.c_void_p(pool.data_ptr()), ctypes.c_void_p(dd.data_ptr()), len(descs),
                           ctypes.c_void_p(mm.data_ptr()), ctypes.cast(mix, ctypes.c_void_p), B,
                           ctypes.c_void_p(tb.data_ptr()), ctypes.c_void_p(lt.data_ptr()),
                           ctypes.c_void_p(out.data_ptr()), H, W, stream())
    out._adr_keep = (pool, dd, mm, tb, lt)
    return out


class LetterboxDesc(ctypes.Structure):
    """adr_letterbox_desc (include/adr.h)."""
    _fields_ = [("off", ctypes.c_int64)] + [(n, ctypes.c_int) for n in (
        "sw", "sh", "nw", "nh", "left", "top", "mode", "tab_off", "rgb", "pad_")]


LB_COPY, LB_LINEAR, LB_AREA2 = 0, 1, 2


def _letterbox_geometry(p):
    """(src, nw, nh, left, top) of a plan adr_letterbox_u8 can render; src None: nothing but the 114 fill."""
    if p.M is not None or p.P is not None or p.lut is not None or p.flip_ud or p.flip_lr or len(p.tiles) > 1 or p.mix is not None:
        raise ValueError("render_letterbox: the plan has mosaic / warp / mix / HSV / flip stages (render() takes "
                         "those)")
    if not p.tiles:
        return None, 0, 0, 0, 0
    src, x1a, y1a, x2a, y2a, x1b, y1b = p.tiles[0]
    sh, sw = src.shape[:2]
    if (x1b, y1b, x2a - x1a, y2a - y1a) != (0, 0, sw, sh):
        raise ValueError("render_letterbox: the plan's tile is not one whole source image")
    if p.resize is not None:
        return (src,) + tuple(p.resize)
    return src, sw, sh, x1a, y1a  # pad only


def render_letterbox(plans_or_images, new_shape=None, device="cuda", out=None, rgb=True, **letterbox_args):
    """Run adr_letterbox_u8 for a list of letterbox ImagePlans and / or HWC BGR uint8 images (letterboxed here with
    LetterBox(new_shape, **letterbox_args), planes in RGB order when `rgb`; a plan keeps its own channel order).
    Returns (uint8 (B, 3, H, W) batch, [((ratio_w, ratio_h), (left, top)) per image]). `out`: an existing uint8
    (B', 3, H, W) device tensor, B' >= the number of images, written in place; the slots beyond the images are
    filled with 114."""
    from ..native import lib
    from ..kernels import stream

    if ctypes.sizeof(LetterboxDesc) != lib.adr_letterbox_desc_size():
        raise RuntimeError("adr_letterbox_desc layout mismatch between adrefine and libadr_hip")
    plans, lb = [], None
    for im in plans_or_images:
        if not isinstance(im, ImagePlan):
            if new_shape is None:
                raise ValueError("render_letterbox: images need new_shape")
            lb = lb or LetterBox(new_shape, **letterbox_args)
            im = lb(image=im)
            im.rgb = bool(rgb)
        plans.append(im)
    if not plans:
        raise ValueError("render_letterbox: no images")
    W, H = plans[0].size
    if any(p.size != (W, H) for p in plans):
        raise ValueError("render_letterbox: every image of a batch must have the same letterboxed size")
    if out is not None:
        if out.dtype != torch.uint8 or not out.is_contiguous() or tuple(out.shape[1:]) != (3, H, W) \
                or out.shape[0] < len(plans):
            raise ValueError(f"render_letterbox: out {tuple(out.shape)} does not take {len(plans)} images of "
                             f"(3, {H}, {W}) uint8")
        device = out.device
    resident = _source_pool(plans, "render_letterbox")  # sources already in HBM: no pixels are uploaded
    if resident is not None:
        resident.flush()
        if out is None:
            device = resident.device
        elif not _same_device(out.device, resident.device):
            raise ValueError("render_letterbox: out is not on the device of the source images' pool")
    B = len(plans) if out is None else out.shape[0]
    descs = (LetterboxDesc * B)()
    srcs, index, tabs, info = [], {}, [], []
    off = ntab = 0
    for b, p in enumerate(plans):
        src, nw, nh, left, top = _letterbox_geometry(p)
        info.append(p.ratio_pad if p.ratio_pad is not None else ((1.0, 1.0), (left, top)))
        d = descs[b]
        if src is None:
            continue  # nw == 0: fill
        if nw > W - left or nh > H - top or left < 0 or top < 0:
            raise ValueError(f"render_letterbox: image {b} ({nw} x {nh} at {left}, {top}) outside {W} x {H}")
        key = id(src)
        if key not in index:
            if resident is not None:
                index[key] = src.off
            else:
                index[key] = off
                srcs.append(np.ascontiguousarray(src).reshape(-1))
                off += src.size
        sh, sw = src.shape[:2]
        d.off, d.sw, d.sh, d.nw, d.nh, d.left, d.top, d.rgb = index[key], sw, sh, nw, nh, left, top, int(p.rgb)
        if (sw, sh) == (nw, nh):
            d.mode = LB_COPY
        elif (sw, sh) == (2 * nw, 2 * nh):
            d.mode = LB_AREA2  # cv::resize: INTER_LINEAR with an exact 2x shrink takes the INTER_AREA fast path
        else:
            d.mode, d.tab_off = LB_LINEAR, ntab
            tab = np.concatenate(resize_linear_tables(sw, nw) + resize_linear_tables(sh, nh))
            tabs.append(tab)
            ntab += tab.size
    if resident is not None:
        pool, pool_bytes = resident.tensor, resident.capacity
    else:
        pool_np = np.concatenate(srcs) if srcs else np.zeros(1, np.uint8)
        pool, pool_bytes = torch.from_numpy(pool_np).to(device, non_blocking=True), pool_np.size
    dd = torch.frombuffer(bytearray(descs), dtype=torch.uint8).to(device, non_blocking=True)
    tb = torch.from_numpy(np.concatenate(tabs) if tabs else np.zeros(1, np.int32)).to(device, non_blocking=True)
    if out is None:
        out = torch.empty(B, 3, H, W, dtype=torch.uint8, device=device)
    lib.adr_letterbox_u8(ctypes.c_void_p(pool.data_ptr()), pool_bytes, ctypes.c_void_p(dd.data_ptr()),
                         ctypes.cast(descs, ctypes.c_void_p), B, ctypes.c_void_p(tb.data_ptr()), ntab,
                         ctypes.c_void_p(out.data_ptr()), H, W, stream())
    out._adr_keep = (pool, dd, tb)  # the inputs live until the launch has read them (stream order)
    return out, info


def collate_fn(batch, device="cuda"):
    """YOLODataset.collate_fn (data/dataset.py:230-246) with the images rendered on the GPU: one launch of
    adr_augment_u8, or of adr_letterbox_u8 for plans whose LetterBox resizes (one of each for a mixed batch)."""
    plans = [b["img"] for b in batch]
    lb = [i for i, p in enumerate(plans) if p.resize is not None]
    if not lb:
        img = render(plans, device)
    elif len(lb) == len(plans):
        img = render_letterbox(plans, device=device)[0]
    else:
        rest = [i for i in range(len(plans)) if plans[i].resize is None]
        if any(p.size != plans[0].size for p in plans):
            raise ValueError("collate_fn: every image of a batch must have the same size")
        W, H = plans[0].size
        img = torch.empty(len(plans), 3, H, W, dtype=torch.uint8, device=device)
        img[lb] = render_letterbox([plans[i] for i in lb], device=device)[0]
        img[rest] = render([plans[i] for i in rest], device)
    new = {"img": img}
    for k in ("cls", "bboxes"):
        new[k] = torch.cat([b[k] for b in batch], 0)
    new["batch_idx"] = torch.cat([b["batch_idx"] + i for i, b in enumerate(batch)], 0)
    # per-image metadata the validator needs (scale_boxes back to the source image), as per-image lists like the
    # reference's collate of non-tensor values; only when every sample carries the key
    for k in ("im_file", "ori_shape", "resized_shape", "ratio_pad"):
        if all(k in b for b in batch):
            new[k] = [b[k] for b in batch]
    return new
