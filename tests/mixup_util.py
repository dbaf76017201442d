"""Shared pieces of the MixUp parity tests (test infrastructure): the hyps, seeds and orders of the two fixtures
scripts/gen_mixup_golden.py makes by running the reference's own chain and dataset, our chain on the same seeds, and a
numpy executor of a plan with a mix stage: each layer through the cv2 restatement of oracle/stubs/cv2 (as
aug_util.execute_plan does), the float64 blend as numpy evaluates the reference's expression, then LUT, flips and
channel order."""
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

# tests/golden/aug_mixup_256.npz: v8_transforms + Format + collate_fn on recipe.synthetic_aug_items(8, 256). `seed` is
# the first seed from SEED0 on at which at least two samples are mixed, at least one is not, and truncation shows
# (the generator searches and records it; the tests read the fixture's)
AUG = dict(name="aug_mixup_256", hyp="rot", mixup=0.5, imgsz=256, order=[4, 5, 6, 7, 0, 2], seed0=21)
# tests/golden/dataset_mixup_tiny.npz: the reference's YOLODataset on dataset_util's tiny tree at imgsz 64.
# "mix": every sample mixed, both layers mosaics; "half": mosaic 0.5, so letterboxed layers meet mosaic layers
DATASET = {
    "mix": dict(seed=21, hyp=dict(mixup=1.0), order=D.TRAIN["order"], batch_size=1, collate=4),
    "half": dict(seed=22, hyp=dict(mosaic=0.5, mixup=1.0), order=[3, 0, 6, 2, 7, 5, 1, 4], batch_size=1, collate=4),
}


def aug_hyp(mixup=AUG["mixup"]):
    return SimpleNamespace(**dict(AUG_HYPS[AUG["hyp"]], mixup=mixup))


def dataset_hyp(tag):
    h = D.hyp()
    for k, v in DATASET[tag]["hyp"].items():
        setattr(h, k, v)
    return h


def run_chain(seed, mixup=AUG["mixup"]):
    """Our v8_transforms + Format on the fixture's items, hyp and order, seeded as the generator seeds the reference."""
    from adrefine.data.augment import Format, v8_transforms
    from adrefine.data.instance import Instances
    hyp = aug_hyp(mixup)
    ds = A.SynthDS(synthetic_aug_items(8, AUG["imgsz"]), AUG["imgsz"], Instances)
    T = v8_transforms(ds, AUG["imgsz"], hyp)
    T.append(Format(bbox_format="xywh", normalize=True, batch_idx=True, bgr=hyp.bgr))
    random.seed(seed)
    np.random.seed(seed)
    return [T(ds.get_image_and_label(i)) for i in AUG["order"]]


def execute_layer(p):
    """HWC BGR uint8: the canvas of a layer and its warp."""
    cw, ch = p.canvas
    img = np.full((ch, cw, 3), 114, dtype=np.uint8)
    for src, x1a, y1a, x2a, y2a, x1b, y1b in p.tiles:
        img[y1a:y2a, x1a:x2a] = np.asarray(src)[y1b:y1b + (y2a - y1a), x1b:x1b + (x2a - x1a)]
    if p.M is not None:
        img = A.cv2_oracle.warpAffine(img, p.M, dsize=p.size, borderValue=(114, 114, 114))
    return img


def execute_plan(p):
    """The (3, H, W) planes a plan stands for, a mix stage included."""
    img = execute_layer(p)
    if p.mix is not None:
        q, r, one_minus_r = p.mix
        assert isinstance(r, float) and isinstance(one_minus_r, float) and one_minus_r == 1 - r
        img = (img * r + execute_layer(q) * one_minus_r).astype(np.uint8)
    if p.lut is not None:
        hsv = A.cv2_oracle.bgr2hsv_u8(img)
        hsv = np.stack([p.lut[k][hsv[..., k]] for k in range(3)], -1)
        img = A.cv2_oracle.hsv2bgr_u8(hsv)
    if p.flip_ud:
        img = img[::-1]
    if p.flip_lr:
        img = img[:, ::-1]
    img = img.transpose(2, 0, 1)
    return np.ascontiguousarray(img[::-1] if p.rgb else img)


def border_ratio(want, seed=0):
    """A MixUp ratio drawn as the chain draws it (np.random.beta(32, 32) of a seeded generator) for which the blend of
    two 114 border pixels, 114 * r + 114 * (1 - r) in float64, truncates to `want` (113 or 114)."""
    rs = np.random.RandomState(seed)
    for _ in range(100000):
        r = float(rs.beta(32.0, 32.0))
        if int(np.float64(114) * r + np.float64(114) * (1 - r)) == want:
            return r
    raise AssertionError(f"no ratio found whose 114 blend truncates to {want}")
