"""Generate the warpPerspective fixtures by running the REFERENCE's own code — build container only (like
oracle/gen_golden.py it refuses to run without the reference checkout). CPU only.

Run:  python scripts/gen_perspective_golden.py

The reference is imported as scripts/gen_mixup_golden.py imports it (oracle/stubs for the packages absent from the
image; cv2.resize / cv2.copyMakeBorder set to the numpy restatements of tests/letterbox_util.py, cv2.imread to a PIL
decode; warpAffine / cvtColor are oracle/stubs/cv2's). cv2.warpPerspective is set at run time to the numpy restatement
of tests/perspective_util.py (PARITY UNPINNED against real OpenCV, as the others are). RandomPerspective's own
arithmetic (the P[2, 0] / P[2, 1] draws in their place in the RNG order, the float32 product T @ S @ R @ P @ C, the
xy / w branch of apply_bboxes, the box filter) is the reference's. Three of its methods and cv2.warpPerspective are
wrapped at run time to OBSERVE it (what warpAffine(M[:2]) would have given, what the affine branch of apply_bboxes
would have given for the boxes that were kept, which samples were mixed); the wrappers call the original and change
nothing.

Writes (data only; hyps, seed ranges and orders in tests/perspective_util.py):
  tests/golden/aug_persp_256.npz      v8_transforms (hyp "rot" + perspective 0.001, mixup 0.5) + Format +
                                      YOLODataset.collate_fn on recipe.synthetic_aug_items(8, 256): img, cls, bboxes,
                                      batch_idx, seed, order, mixed (per sample). The seed is the first from
                                      perspective_util.AUG["seed0"] on at which some image differs from
                                      warpAffine(M[:2])'s, some kept box differs from the affine branch's, at least
                                      one sample is mixed and one is not, and the file is no larger than the largest
                                      existing aug_*.npz.
  tests/golden/dataset_persp_tiny.npz the reference's YOLODataset on the tiny tree of tests/dataset_util.py at imgsz
                                      64 with perspective 0.001: a seeded pass with mosaic 1.0 and one with mosaic 0.0
                                      (LetterBox is RandomPerspective's pre_transform); the same conditions on images
                                      and boxes asserted for each pass; no larger than dataset_tiny.npz."""
from __future__ import annotations

import io
import os
import sys
import tempfile
import zipfile
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
REPO = Path(__file__).resolve().parents[1]
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO / "oracle"))
sys.path.insert(0, str(REPO / "tests"))
import dataset_util as D  # noqa: E402
import letterbox_util as U  # noqa: E402


def _import_reference():
    if not REF.is_dir():
        raise SystemExit("gen_perspective_golden: the reference checkout is not present — fixtures are generated in "
                         "the build container")
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.dont_write_bytecode = True
    os.environ.setdefault("YOLO_CONFIG_DIR", "/tmp/adr_yolo_cfg")
    sys.path.insert(0, str(REPO / "oracle" / "stubs"))
    sys.path.insert(1, str(REF))
    import cv2
    from PIL import Image
    import perspective_util as P
    cv2.resize = U.resize
    cv2.copyMakeBorder = U.copyMakeBorder
    cv2.INTER_LINEAR, cv2.BORDER_CONSTANT = U.INTER_LINEAR, U.BORDER_CONSTANT
    cv2.imread = lambda f, *a: np.ascontiguousarray(np.asarray(Image.open(f).convert("RGB"))[:, :, ::-1])
    cv2.warpPerspective = P.warpPerspective
    import ultralytics  # noqa: F401
    from ultralytics.data import augment
    from ultralytics.data.dataset import YOLODataset
    from ultralytics.utils.instance import Instances
    return cv2, augment, YOLODataset, Instances


class _Watch:
    """Observes cv2.warpPerspective, RandomPerspective.apply_bboxes / box_candidates and MixUp._mix_transform of the
    reference; the originals do all the work."""

    def __init__(self, cv2, augment):
        self.cv2, self.augment = cv2, augment
        RP = augment.RandomPerspective
        self._warp, self._boxes, self._cand = cv2.warpPerspective, RP.apply_bboxes, RP.box_candidates
        self._mixup = augment.MixUp._mix_transform
        self.reset()
        watch = self

        def warp(img, M, dsize=None, borderValue=(0, 0, 0), **kw):
            out = watch._warp(img, M, dsize=dsize, borderValue=borderValue, **kw)
            assert M.shape == (3, 3) and M.dtype == np.float32
            affine = cv2.warpAffine(img, M[:2], dsize=dsize, borderValue=borderValue)
            watch.warps += 1
            watch.pixels += int((out != affine).any(-1).sum())
            return out

        def boxes(this, bboxes, M):
            out = watch._boxes(this, bboxes, M)
            persp, this.perspective = this.perspective, 0.0
            try:
                affine = watch._boxes(this, bboxes, M)
            finally:
                this.perspective = persp
            watch.last = (out, affine, this.size)
            return out

        def cand(this, box1, box2, **kw):
            i = watch._cand(this, box1, box2, **kw)
            out, affine, (w, h) = watch.last
            if len(out):
                hi = np.array([w, h, w, h], dtype=out.dtype)
                a, b = np.clip(out, 0, hi)[i], np.clip(affine, 0, hi)[i]
                assert np.array_equal(a, box2.T[i])  # the kept boxes are the perspective branch's
                watch.kept += int(i.sum())
                watch.kept_differ += int((a != b).any(1).sum())
            return i

        def mixup(this, labels):
            watch.mixes += 1
            return watch._mixup(this, labels)

        cv2.warpPerspective, RP.apply_bboxes, RP.box_candidates = warp, boxes, cand
        augment.MixUp._mix_transform = mixup

    def reset(self):
        self.warps = self.pixels = self.kept = self.kept_differ = self.mixes = 0
        self.last = None

    def close(self):
        RP = self.augment.RandomPerspective
        self.cv2.warpPerspective, RP.apply_bboxes, RP.box_candidates = self._warp, self._boxes, self._cand
        self.augment.MixUp._mix_transform = self._mixup


def _packed(d):
    """An .npz with LZMA members (np.load reads them through zipfile like deflated ones), as bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_LZMA) as z:
        for k, v in d.items():
            with z.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)
    return buf.getvalue()


def aug_persp(augment, YOLODataset, Instances, watch):
    import aug_util as A
    import perspective_util as P
    cfg = P.AUG
    limit = max(f.stat().st_size for f in OUT.glob("aug_*.npz") if f.stem != cfg["name"])
    items = P.synthetic_aug_items(8, cfg["imgsz"])
    for seed in range(cfg["seed0"], cfg["seed0"] + 200):
        hyp = P.aug_hyp()
        ds = A.SynthDS(items, cfg["imgsz"], Instances)
        T = augment.v8_transforms(ds, cfg["imgsz"], hyp)
        T.append(augment.Format(bbox_format="xywh", normalize=True, return_mask=False, return_keypoint=False,
                                return_obb=False, batch_idx=True, mask_ratio=4, mask_overlap=True, bgr=hyp.bgr))
        U.seed_chain(seed)
        watch.reset()
        samples, mixed = [], []
        for i in cfg["order"]:
            n = watch.mixes
            samples.append(T(ds.get_image_and_label(i)))
            mixed.append(watch.mixes > n)
        if not (watch.pixels and watch.kept_differ and any(mixed) and not all(mixed)):
            continue
        assert watch.warps == len(samples) + sum(mixed)
        batch = YOLODataset.collate_fn(samples)
        blob = _packed(dict(
            img=batch["img"].numpy(), cls=batch["cls"].numpy(), bboxes=batch["bboxes"].numpy(),
            batch_idx=batch["batch_idx"].numpy(), seed=seed, imgsz=cfg["imgsz"], order=np.array(cfg["order"]),
            mixed=np.array(mixed)))
        if len(blob) <= limit:
            break
    else:
        raise SystemExit("gen_perspective_golden: no seed met the fixture's conditions")
    (OUT / f"{cfg['name']}.npz").write_bytes(blob)
    print(cfg["name"], "seed", seed, "mixed", mixed, "pixels that differ from warpAffine(M[:2])", watch.pixels,
          "kept boxes", watch.kept, "of which differ from the affine branch", watch.kept_differ, len(blob), "bytes")


def _batch(d, tag, batch):
    d[f"{tag}_img"] = batch["img"].numpy()
    for k in ("bboxes", "cls", "batch_idx"):
        d[f"{tag}_{k}"] = batch[k].numpy()


def dataset_persp(YOLODataset, watch):
    import perspective_util as P
    images = {name: D.make_image(name) for name in D.SIZES}
    d = {}
    with tempfile.TemporaryDirectory() as tmp:
        img_dir = str(D.write_tree(Path(tmp) / "tiny", images))
        for tag, cfg in P.DATASET.items():
            ds = YOLODataset(img_path=img_dir, imgsz=D.IMGSZ, cache=False, hyp=P.dataset_hyp(tag),
                             data={"names": D.NAMES}, task="detect", augment=True, rect=False,
                             batch_size=cfg["batch_size"], pad=0.0)
            assert ds.max_buffer_length == 8
            D.seed(cfg["seed"])
            watch.reset()
            samples = [ds[i] for i in cfg["order"]]
            assert watch.warps == len(samples) and watch.pixels and watch.kept_differ and not watch.mixes, \
                (tag, watch.warps, watch.pixels, watch.kept_differ)
            mosaic = ds.transforms.transforms[0].transforms[0]
            assert mosaic.p == (0.0 if tag == "letterbox" else 1.0)
            d[f"{tag}_seed"] = np.array(cfg["seed"])
            d[f"{tag}_buffer"] = np.array(list(ds.buffer), dtype=np.int64)
            for k in range(0, len(samples), cfg["collate"]):
                _batch(d, f"{tag}_b{k // cfg['collate']}", YOLODataset.collate_fn(samples[k:k + cfg["collate"]]))
            print(tag, "pixels that differ from warpAffine(M[:2])", watch.pixels, "kept boxes", watch.kept,
                  "of which differ from the affine branch", watch.kept_differ)
    blob = _packed(d)
    assert len(blob) <= (OUT / "dataset_tiny.npz").stat().st_size, len(blob)
    (OUT / "dataset_persp_tiny.npz").write_bytes(blob)
    print("dataset_persp_tiny.npz", len(blob), "bytes,", len(d), "arrays")


def main():
    cv2, augment, YOLODataset, Instances = _import_reference()
    OUT.mkdir(parents=True, exist_ok=True)
    watch = _Watch(cv2, augment)
    try:
        aug_persp(augment, YOLODataset, Instances, watch)
        dataset_persp(YOLODataset, watch)
    finally:
        watch.close()


if __name__ == "__main__":
    main()
