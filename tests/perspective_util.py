"""Shared pieces of the warpPerspective parity tests (test infrastructure).

A numpy float64 restatement of cv2.warpPerspective (8U, 3 channels, INTER_LINEAR, BORDER_CONSTANT) from OpenCV 4.x's
published algorithm (imgproc/imgwarp.cpp: cv::warpPerspective, WarpPerspectiveInvoker, remap's fixed-point bilinear).
OpenCV is not installed: like oracle/stubs/cv2 and tests/letterbox_util.py this restatement is PARITY UNPINNED against
real OpenCV; it IS the definition of parity for the perspective branch of adr_augment_u8 / adr_augment_mix_u8 and for
the fixtures scripts/gen_perspective_golden.py makes by running the reference's own chain and dataset on it.

  matrix:      the float32 3x3 M in double, inverted by cv::invert's closed 3x3 form (determinant by the first row,
               d = 1 / det, adjugate entries times d; det == 0: the zero matrix), products and differences rounded
               one by one.
  coordinates: the output is walked in blocks bw0 = min(1024 / min(16, H), W) wide. With bx the block's first column
               and x1 = x - bx: X0 = (t0*bx + t1*y) + t2, Y0 = (t3*bx + t4*y) + t5, W0 = (t6*bx + t7*y) + t8;
               W = W0 + t6*x1, W = W ? 32 / W : 0; fX = max(INT_MIN, min(INT_MAX, (X0 + t0*x1) * W)), fY likewise;
               X = cvRound(fX) (round half to even), sx = saturate_cast<short>(X >> 5), fx = X & 31.
  remap:       as oracle/stubs/cv2's warpAffine: weights (32-fx)(32-fy)*32 etc. (INTER_REMAP_COEF_BITS 15),
               (sum + 2^14) >> 15, taps outside the source take borderValue.

Also: the hyps, seeds and orders of the two fixtures, our chain on the same seeds, a numpy executor of plans with P
(tests/aug_util.execute_plan / tests/mixup_util's blend for everything else), and the hand-built cases of
tests/test_gpu_perspective.py."""
import copy
import random
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import aug_util as A
import dataset_util as D

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
from recipe import AUG_HYPS, synthetic_aug_items  # noqa: E402

INTER_LINEAR = 1
INT_MIN, INT_MAX = -2147483648.0, 2147483647.0


def invert3x3(M):
    """cv::invert (DECOMP_LU) of a 3x3 double matrix: the closed form, flat (9,) float64."""
    m = np.asarray(M, dtype=np.float32).astype(np.float64).reshape(3, 3)
    det = m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) \
        + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0])
    t = np.zeros(9, dtype=np.float64)
    if det != 0:
        d = np.float64(1.0) / det
        t[0] = (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) * d
        t[1] = (m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]) * d
        t[2] = (m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]) * d
        t[3] = (m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]) * d
        t[4] = (m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]) * d
        t[5] = (m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]) * d
        t[6] = (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]) * d
        t[7] = (m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]) * d
        t[8] = (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]) * d
    return t


def perspective_coords(M, dsize):
    """(sx, sy, fx, fy, paths) of every output pixel, (H, W) int64 arrays; paths: boolean masks of the pixels whose
    denominator is exactly zero ("w0"), whose fX or fY was clamped to the int range ("int") and whose sx or sy was
    clamped to the short range ("short")."""
    t = invert3x3(M)
    W, H = dsize
    bh0 = min(16, H)
    bw0 = min(1024 // bh0, W)
    xs = np.arange(W, dtype=np.int64)
    bx = ((xs // bw0) * bw0).astype(np.float64)[None, :]
    x1 = (xs - (xs // bw0) * bw0).astype(np.float64)[None, :]
    ys = np.arange(H, dtype=np.float64)[:, None]
    X0 = (t[0] * bx + t[1] * ys) + t[2]
    Y0 = (t[3] * bx + t[4] * ys) + t[5]
    W0 = (t[6] * bx + t[7] * ys) + t[8]
    den = W0 + t[6] * x1
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        w = np.where(den != 0, np.float64(32.0) / np.where(den != 0, den, 1.0), 0.0)
        rawX, rawY = (X0 + t[0] * x1) * w, (Y0 + t[3] * x1) * w
        fX = np.where(rawX < INT_MAX, rawX, INT_MAX)  # std::min(INT_MAX, v), then std::max(INT_MIN, .)
        fX = np.where(INT_MIN < fX, fX, INT_MIN)
        fY = np.where(rawY < INT_MAX, rawY, INT_MAX)
        fY = np.where(INT_MIN < fY, fY, INT_MIN)
    X, Y = np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    paths = {"w0": den == 0, "int": (fX != rawX) | (fY != rawY), "short": (sx != X >> 5) | (sy != Y >> 5)}
    return sx, sy, X & 31, Y & 31, paths


def remap_linear(img, sx, sy, fx, fy, borderValue):
    """cv::remap's 8U fixed-point bilinear with BORDER_CONSTANT at integer coordinates (sx, sy) and 1/32 fractions."""
    Hs, Ws = img.shape[:2]
    cval = np.asarray(borderValue[:3], dtype=np.int64)
    acc = np.zeros(sx.shape + (3,), dtype=np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            wgt = ((32 - fx) if dx == 0 else fx) * ((32 - fy) if dy == 0 else fy) * 32
            yy, xx = sy + dy, sx + dx
            ok = (yy >= 0) & (yy < Hs) & (xx >= 0) & (xx < Ws)
            v = img[np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)].astype(np.int64)
            acc += np.where(ok[..., None], v, cval) * wgt[..., None]
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def warpPerspective(img, M, dsize, borderValue=(0, 0, 0), **kw):  # noqa: N802 (OpenCV naming)
    """cv2.warpPerspective(img, M, dsize=(w, h), borderValue=...) for 8U HWC images."""
    if kw.get("flags", INTER_LINEAR) != INTER_LINEAR or img.dtype != np.uint8 or img.ndim != 3 \
            or kw.get("borderMode", 0) != 0:
        raise NotImplementedError("cv2.warpPerspective restatement: 8U 3-channel INTER_LINEAR BORDER_CONSTANT only")
    sx, sy, fx, fy, _ = perspective_coords(M, dsize)
    return remap_linear(img, sx, sy, fx, fy, borderValue)


# tests/golden/aug_persp_256.npz: v8_transforms + Format + collate_fn on recipe.synthetic_aug_items(8, 256). `seed` is
# the first seed from seed0 on at which the generator's conditions hold (it searches and records it; the tests read
# the fixture's)
AUG = dict(name="aug_persp_256", hyp="rot", perspective=0.001, mixup=0.5, imgsz=256, order=[4, 5, 6, 7, 0, 2],
           seed0=31)
# tests/golden/dataset_persp_tiny.npz: the reference's YOLODataset on dataset_util's tiny tree at imgsz 64 with
# perspective 0.001. "mosaic": mosaic 1.0; "letterbox": mosaic 0.0, LetterBox is RandomPerspective's pre_transform
DATASET = {
    "mosaic": dict(seed=31, hyp=dict(perspective=0.001), order=[0, 1, 2, 3, 4, 5, 6, 7], batch_size=1, collate=4),
    "letterbox": dict(seed=32, hyp=dict(perspective=0.001, mosaic=0.0), order=[2, 5, 7, 4], batch_size=1, collate=4),
}


def aug_hyp(perspective=AUG["perspective"], mixup=AUG["mixup"]):
    return SimpleNamespace(**dict(AUG_HYPS[AUG["hyp"]], perspective=perspective, mixup=mixup))


def dataset_hyp(tag):
    h = D.hyp()
    for k, v in DATASET[tag]["hyp"].items():
        setattr(h, k, v)
    return h


def run_chain(seed, **hyp):
    """Our v8_transforms + Format on the fixture's items, hyp and order, seeded as the generator seeds the reference."""
    from adrefine.data.augment import Format, v8_transforms
    from adrefine.data.instance import Instances
    hyp = aug_hyp(**hyp)
    ds = A.SynthDS(synthetic_aug_items(8, AUG["imgsz"]), AUG["imgsz"], Instances)
    T = v8_transforms(ds, AUG["imgsz"], hyp)
    T.append(Format(bbox_format="xywh", normalize=True, batch_idx=True, bgr=hyp.bgr))
    random.seed(seed)
    np.random.seed(seed)
    return [T(ds.get_image_and_label(i)) for i in AUG["order"]]


def execute_layer(p):
    """HWC BGR uint8: the canvas of a layer and its warp, affine (oracle/stubs/cv2) or perspective (here)."""
    assert p.M is None or p.P is None
    cw, ch = p.canvas
    img = np.full((ch, cw, 3), 114, dtype=np.uint8)
    for src, x1a, y1a, x2a, y2a, x1b, y1b in p.tiles:
        img[y1a:y2a, x1a:x2a] = np.asarray(src)[y1b:y1b + (y2a - y1a), x1b:x1b + (x2a - x1a)]
    if p.M is not None:
        img = A.cv2_oracle.warpAffine(img, p.M, dsize=p.size, borderValue=(114, 114, 114))
    if p.P is not None:
        assert p.P.shape == (3, 3) and p.P.dtype == np.float32
        img = warpPerspective(img, p.P, dsize=p.size, borderValue=(114, 114, 114))
    return img


def execute_plan(p):
    """The (3, H, W) planes a plan stands for. The layers (with P or not) are materialised here, the float64 blend as
    tests/mixup_util.py does it; LUT, flips and channel order are tests/aug_util.execute_plan's, run on a plan whose
    canvas is the materialised image."""
    img = execute_layer(p)
    if p.mix is not None:
        q, r, one_minus_r = p.mix
        assert isinstance(r, float) and isinstance(one_minus_r, float) and one_minus_r == 1 - r
        img = (img * r + execute_layer(q) * one_minus_r).astype(np.uint8)
    rest = copy.copy(p)
    h, w = img.shape[:2]
    rest.tiles, rest.canvas, rest.M, rest.P, rest.mix = [(img, 0, 0, w, h, 0, 0)], (w, h), None, None, None
    return A.execute_plan(rest)


def src_image(rs, h, w):
    """Seeded BGR uint8 source: a smooth gradient plus noise, so that a one-step coordinate error shows."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rs.uniform(0, 6, 3)
    base = 127.5 + 80 * np.sin(xx[..., None] * 0.23 + yy[..., None] * 0.17 + ph)
    return np.clip(np.rint(base + rs.uniform(-40, 40, (h, w, 3))), 0, 255).astype(np.uint8)


def gentle_matrix(rs, cw, ch, W, H, persp):
    """T @ S @ R @ P @ C in float32 as RandomPerspective builds it, with rotation, scale, shear and P[2, :2] drawn
    from rs (|P[2, k]| <= persp): the canvas centre goes to the output centre."""
    C, P, R, S, T = (np.eye(3, dtype=np.float32) for _ in range(5))
    C[0, 2], C[1, 2] = -cw / 2, -ch / 2
    P[2, 0], P[2, 1] = rs.uniform(-persp, persp, 2)
    a, s = np.deg2rad(rs.uniform(-12, 12)), rs.uniform(0.7, 1.3) * min(W / cw, H / ch)
    R[:2, :2] = [[np.cos(a) * s, np.sin(a) * s], [-np.sin(a) * s, np.cos(a) * s]]
    S[0, 1], S[1, 0] = np.tan(np.deg2rad(rs.uniform(-4, 4, 2)))
    T[0, 2], T[1, 2] = rs.uniform(0.4, 0.6) * W, rs.uniform(0.4, 0.6) * H
    return T @ S @ R @ P @ C


# A matrix whose computed inverse is exact: rows (1, 0, 0), (0, 1, 0), (-1/64, 2^-30, 1/2). The denominator
# 1/2 - x/64 + y * 2^-30 changes sign at column 32 of a 96-wide output: it is exactly zero at (32, 0), a tiny non-zero
# number in the rest of column 32 (the quotient leaves the int range, then the short range), ordinary elsewhere.
STRONG = np.array([[1, 0, 0], [0, 1, 0], [1 / 32, -2.0 ** -29, 2]], dtype=np.float32)


def mosaic_plan(rs, W, H, warp=None):
    """A 2W x 2H canvas of four tiles around its centre that leave border on every side; `warp` sets P (a 3x3
    matrix) or M (2x3), the output is W x H."""
    from adrefine.data.augment import ImagePlan
    p = ImagePlan(src_image(rs, 8, 8))
    xc, yc = W + 3, H - 2
    p.tiles = []
    for x1, y1, x2, y2 in ((xc - W // 2, yc - H // 2, xc, yc), (xc, yc - H // 2 - 1, xc + W // 2 + 2, yc),
                           (xc - W // 2 + 3, yc, xc, yc + H // 2), (xc, yc, xc + W // 2 - 1, yc + H // 2 + 1)):
        p.tiles.append((src_image(rs, y2 - y1 + 3, x2 - x1 + 2), x1, y1, x2, y2, 2, 3))
    p.canvas = (2 * W, 2 * H)
    set_warp(p, warp, (W, H))
    return p


def single_plan(rs, cw, ch, W, H, warp=None):
    """One whole source image cw x ch as the canvas."""
    from adrefine.data.augment import ImagePlan
    p = ImagePlan(src_image(rs, ch, cw))
    set_warp(p, warp, (W, H))
    return p


def set_warp(p, warp, size):
    if warp is not None:
        warp = np.asarray(warp, dtype=np.float32)
        if warp.shape == (3, 3):
            p.P = warp
        else:
            p.M = warp
        p.size = tuple(size)
