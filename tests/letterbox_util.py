"""Shared pieces of the LetterBox parity tests (test infrastructure).

The numpy restatement of the two OpenCV calls LetterBox makes (reference data/augment.py:1583-1589) — cv2.resize
(8U, 3 channels, INTER_LINEAR) and cv2.copyMakeBorder (BORDER_CONSTANT) — from OpenCV 4.x's published algorithm
(imgproc/resize.cpp). OpenCV is not installed: like oracle/stubs/cv2 these restatements are PARITY UNPINNED against
real OpenCV; they ARE the definition of parity for adr_letterbox_u8 and for the fixtures
scripts/gen_letterbox_golden.py makes by running the reference's own LetterBox / scale_boxes code on them.

  resize INTER_LINEAR 8U: scale = 1 / (n / s) in double per axis; f = (float)((d + 0.5) * scale - 0.5), i = floor(f),
      f -= i; i < 0 -> i = 0, f = 0; i >= s - 1 -> i = s - 1, f = 0; coefficients (short)cvRound((1.f - f) * 2048),
      (short)cvRound(f * 2048) (INTER_RESIZE_COEF_BITS 11). Horizontal D = S[i] * a0 + S[min(i + 1, s - 1)] * a1;
      vertical dst = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2.
      An exact 2x shrink in both axes takes the INTER_AREA fast path: (s00 + s01 + s10 + s11 + 2) >> 2.

Also: a numpy executor of letterbox ImagePlans, the case list (each case the smallest that reaches one way to go
wrong) and the seeded inputs of the cases and of the close-mosaic chain."""
import random
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
INTER_LINEAR = 1
BORDER_CONSTANT = 0


def _axis(s, n):
    scale = 1.0 / (n / s)
    f = ((np.arange(n, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    i = np.floor(f).astype(np.int64)
    f = (f - i.astype(np.float32)).astype(np.float32)
    for d in range(n):
        if i[d] < 0:
            i[d], f[d] = 0, 0
        if i[d] >= s - 1:
            i[d], f[d] = s - 1, 0
    c0 = np.clip(np.rint((np.float32(1) - f) * np.float32(2048)), -32768, 32767).astype(np.int64)
    c1 = np.clip(np.rint(f * np.float32(2048)), -32768, 32767).astype(np.int64)
    return i, c0, c1


def resize(img, dsize, interpolation=INTER_LINEAR, **kw):
    """cv2.resize(img, (w, h), interpolation=cv2.INTER_LINEAR) for 8U HWC images."""
    if interpolation != INTER_LINEAR or img.dtype != np.uint8 or img.ndim != 3:
        raise NotImplementedError("cv2.resize restatement: 8U HWC INTER_LINEAR only")
    nw, nh = dsize
    sh, sw = img.shape[:2]
    S = img.astype(np.int64)
    if sw == 2 * nw and sh == 2 * nh:
        return ((S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, a0, a1 = _axis(sw, nw)
    sy, b0, b1 = _axis(sh, nh)
    D = S[:, sx] * a0[None, :, None] + S[:, np.minimum(sx + 1, sw - 1)] * a1[None, :, None]  # (sh, nw, 3)
    D0, D1 = D[sy], D[np.minimum(sy + 1, sh - 1)]
    out = (((b0[:, None, None] * (D0 >> 4)) >> 16) + ((b1[:, None, None] * (D1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def copyMakeBorder(img, top, bottom, left, right, borderType=BORDER_CONSTANT, value=(0, 0, 0)):  # noqa: N802
    if borderType != BORDER_CONSTANT:
        raise NotImplementedError("cv2.copyMakeBorder restatement: BORDER_CONSTANT only")
    h, w = img.shape[:2]
    out = np.empty((h + top + bottom, w + left + right, 3), dtype=img.dtype)
    out[...] = np.asarray(value[:3], dtype=img.dtype)
    out[top:top + h, left:left + w] = img
    return out


def execute_letterbox(p):
    """The HWC BGR image a letterbox ImagePlan stands for (no warp / HSV / flip stages)."""
    assert p.M is None and p.lut is None and not (p.flip_ud or p.flip_lr)
    W, H = p.size
    if p.resize is None:
        out = np.full((H, W, 3), 114, dtype=np.uint8)
        for src, x1a, y1a, x2a, y2a, x1b, y1b in p.tiles:
            out[y1a:y2a, x1a:x2a] = src[y1b:y1b + (y2a - y1a), x1b:x1b + (x2a - x1a)]
        return out
    nw, nh, left, top = p.resize
    img = resize(p.tiles[0][0], (nw, nh))
    return copyMakeBorder(img, top, H - top - nh, left, W - left - nw, BORDER_CONSTANT, value=(114, 114, 114))


def execute_chw(p):
    """The (3, H, W) planes render_letterbox writes for the plan."""
    img = execute_letterbox(p).transpose(2, 0, 1)
    return np.ascontiguousarray(img[::-1] if p.rgb else img)


# name, source (h, w), LetterBox arguments, rect_shape put into the labels (or None)
CASES = [
    ("up", (30, 40), dict(new_shape=(96, 96)), None),                      # upscale 40x30 -> 96
    ("down", (113, 150), dict(new_shape=(96, 96)), None),                  # non-integer downscale
    ("area2x", (128, 192), dict(new_shape=(96, 96)), None),                # exact 2x: the area fast path
    ("narrow", (50, 2), dict(new_shape=(96, 96)), None),                   # 2-pixel-wide source: both sx clamps
    ("odd_resize", (50, 75), dict(new_shape=(96, 128)), None),             # odd dh with a resize: top != bottom
    ("odd_pad", (51, 77), dict(new_shape=(96, 128), scaleup=False), None),  # odd dw and dh (pad only)
    ("corner", (113, 150), dict(new_shape=(96, 96), center=False), None),  # center=False
    ("noscaleup", (40, 56), dict(new_shape=(96, 96), scaleup=False), None),  # small source: pad only
    ("fill", (60, 100), dict(new_shape=(96, 128), scaleFill=True), None),  # different x and y ratios
    ("auto", (100, 300), dict(new_shape=(96, 128), auto=True, stride=32), None),  # minimum rectangle: 64 x 128
    ("w90", (70, 111), dict(new_shape=(64, 90)), None),                    # W % 4 != 0: the scalar store path
    ("rect", (80, 100), dict(new_shape=(96, 96)), (64, 96)),               # rect_shape in the labels wins
]


def case_inputs(idx):
    """Seeded inputs of case idx: BGR uint8 source (smooth gradient + noise), cls (k, 1), normalised xywh boxes
    (k, 4) float32, and detections (6, 6) float32 [x1, y1, x2, y2, conf, cls] in letterboxed coordinates, some of
    them outside the image so that the clip acts."""
    h, w = CASES[idx][1]
    rs = np.random.RandomState(100 + idx)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rs.uniform(0, 6, 3)
    base = 127.5 + 80 * np.sin(xx[..., None] * 0.21 + yy[..., None] * 0.13 + ph) + 30 * np.cos(yy[..., None] * 0.3)
    img = np.clip(np.rint(base + rs.uniform(-30, 30, (h, w, 3))), 0, 255).astype(np.uint8)
    k = 1 + idx % 4
    ctr = 0.1 + 0.8 * rs.uniform(size=(k, 2))
    wh = np.minimum(0.05 + 0.45 * rs.uniform(size=(k, 2)), 2 * np.minimum(ctr, 1 - ctr))
    bboxes = np.concatenate([ctr, wh], 1).astype(np.float32)
    cls = rs.randint(0, 80, (k, 1)).astype(np.float32)
    xy = rs.uniform(-20, 120, (6, 2))
    det = np.concatenate([xy, xy + rs.uniform(1, 60, (6, 2)), rs.uniform(0, 1, (6, 1)),
                          rs.randint(0, 80, (6, 1))], 1).astype(np.float32)
    return img, cls, bboxes, det


def case_labels(idx, instances_cls):
    """The labels dict of case idx as a dataset hands it to the transform (data/base.py:290-301)."""
    img, cls, bboxes, _ = case_inputs(idx)
    h, w = img.shape[:2]
    labels = {"im_file": f"case{idx}.jpg", "ori_shape": (h, w), "resized_shape": (h, w), "ratio_pad": (1.0, 1.0),
              "img": img, "cls": cls,
              "instances": instances_cls(bboxes, np.zeros((0, 1000, 2), dtype=np.float32), None, bbox_format="xywh",
                                         normalized=True)}
    if CASES[idx][3] is not None:
        labels["rect_shape"] = CASES[idx][3]
    return labels


# the close-mosaic chain fixture: v8_transforms with the default hyp but mosaic = 0 (what close_mosaic leaves),
# + Format + collate_fn, on recipe.synthetic_aug_items(8, 256)
CLOSE_MOSAIC = dict(name="aug_closemosaic_256", imgsz=256, seed=5, order=[0, 1, 2, 3])


def close_mosaic_hyp():
    sys.path.insert(0, str(ROOT / "oracle"))
    from recipe import AUG_HYPS
    return SimpleNamespace(**dict(AUG_HYPS["default"], mosaic=0.0))


def seed_chain(seed):
    random.seed(seed)
    np.random.seed(seed)
