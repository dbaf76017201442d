"""Generate the MixUp fixtures by running the REFERENCE's own code — build container only (like oracle/gen_golden.py it
refuses to run without the reference checkout). CPU only.

Run:  python scripts/gen_mixup_golden.py

The reference is imported as scripts/gen_dataset_golden.py imports it (oracle/stubs for the packages absent from the
image; cv2.resize / cv2.copyMakeBorder set to the numpy restatements of tests/letterbox_util.py, cv2.imread to a PIL
decode; warpAffine / cvtColor are oracle/stubs/cv2's: PARITY UNPINNED against real OpenCV). MixUp's own arithmetic
(np.random.beta, the float64 blend and its truncation, the label concatenation) and the order of every RNG draw are
the reference's. Two of its methods are wrapped at run time to OBSERVE it (which samples were mixed, what the blend's
inputs were, how many layers were mosaics); the wrappers call the original and change nothing.

Writes (data only; hyps, seeds and orders in tests/mixup_util.py):
  tests/golden/aug_mixup_256.npz      v8_transforms (hyp "rot", mixup 0.5) + Format + YOLODataset.collate_fn on
                                      recipe.synthetic_aug_items(8, 256): img, cls, bboxes, batch_idx, seed, order,
                                      mixed (per sample), ratio (per sample, nan when not mixed). The seed is the first
                                      from mixup_util.AUG["seed0"] on at which >= 2 samples are mixed, >= 1 is not, and
                                      some blended pixel differs from the rounded (untruncated) blend.
  tests/golden/dataset_mixup_tiny.npz the reference's YOLODataset on the tiny tree of tests/dataset_util.py at imgsz
                                      64: a seeded pass with mixup 1.0 (buffer after every sample, collated batches),
                                      and one with mosaic 0.5, mixup 1.0 in which a letterboxed layer meets a mosaic
                                      layer (asserted)."""
from __future__ import annotations

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
        raise SystemExit("gen_mixup_golden: the reference checkout is not present — fixtures are generated in the "
                         "build container")
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.dont_write_bytecode = True
    os.environ.setdefault("YOLO_CONFIG_DIR", "/tmp/adr_yolo_cfg")
    sys.path.insert(0, str(REPO / "oracle" / "stubs"))
    sys.path.insert(1, str(REF))
    import cv2
    from PIL import Image
    cv2.resize = U.resize
    cv2.copyMakeBorder = U.copyMakeBorder
    cv2.INTER_LINEAR, cv2.BORDER_CONSTANT = U.INTER_LINEAR, U.BORDER_CONSTANT
    cv2.imread = lambda f, *a: np.ascontiguousarray(np.asarray(Image.open(f).convert("RGB"))[:, :, ::-1])
    import ultralytics  # noqa: F401
    from ultralytics.data import augment
    from ultralytics.data.dataset import YOLODataset
    from ultralytics.utils.instance import Instances
    return augment, YOLODataset, Instances


class _Watch:
    """Observes MixUp._mix_transform and Mosaic._mix_transform of the reference (calls counted, the blend's inputs
    and output kept); the original methods do all the work."""

    def __init__(self, augment):
        self.augment = augment
        self.mix, self.mosaics = [], 0
        self._mixup, self._mosaic = augment.MixUp._mix_transform, augment.Mosaic._mix_transform
        watch = self

        def mixup(this, labels):
            a, b = labels["img"], labels["mix_labels"][0]["img"]
            state = np.random.get_state()
            r = np.random.beta(32.0, 32.0)  # the draw the original is about to make
            np.random.set_state(state)
            out = watch._mixup(this, labels)
            watch.mix.append((a, b, r, out["img"].copy()))  # RandomHSV later writes into the blended array
            return out

        def mosaic(this, labels):
            watch.mosaics += 1
            return watch._mosaic(this, labels)

        augment.MixUp._mix_transform, augment.Mosaic._mix_transform = mixup, mosaic

    def close(self):
        self.augment.MixUp._mix_transform, self.augment.Mosaic._mix_transform = self._mixup, self._mosaic


def _save(path, d):
    """An .npz with LZMA members (np.load reads them through zipfile like deflated ones): smaller than
    np.savez_compressed's deflate on these images."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
        for k, v in d.items():
            with z.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def aug_mixup(augment, YOLODataset, Instances, watch):
    import aug_util as A
    import mixup_util as X
    from recipe import synthetic_aug_items
    cfg = X.AUG
    items = synthetic_aug_items(8, cfg["imgsz"])
    for seed in range(cfg["seed0"], cfg["seed0"] + 200):
        hyp = X.aug_hyp()
        ds = A.SynthDS(items, cfg["imgsz"], Instances)
        T = augment.v8_transforms(ds, cfg["imgsz"], hyp)
        T.append(augment.Format(bbox_format="xywh", normalize=True, return_mask=False, return_keypoint=False,
                                return_obb=False, batch_idx=True, mask_ratio=4, mask_overlap=True, bgr=hyp.bgr))
        U.seed_chain(seed)
        samples, mixed, ratio, visible = [], [], [], 0
        for i in cfg["order"]:
            n = len(watch.mix)
            samples.append(T(ds.get_image_and_label(i)))
            mixed.append(len(watch.mix) > n)
            ratio.append(watch.mix[-1][2] if mixed[-1] else np.nan)
            if mixed[-1]:
                a, b, r, out = watch.mix[-1]
                assert out.dtype == np.uint8 and (a * r).dtype == np.float64
                blend = a * r + b * (1 - r)
                assert np.array_equal(out, blend.astype(np.uint8))
                visible += int((out != np.rint(blend)).sum())
        if sum(mixed) >= 2 and not all(mixed) and visible:
            break
    else:
        raise SystemExit("gen_mixup_golden: no seed met the fixture's conditions")
    batch = YOLODataset.collate_fn(samples)
    _save(OUT / f"{cfg['name']}.npz", dict(
        img=batch["img"].numpy(), cls=batch["cls"].numpy(), bboxes=batch["bboxes"].numpy(),
        batch_idx=batch["batch_idx"].numpy(), seed=seed, imgsz=cfg["imgsz"], order=np.array(cfg["order"]),
        mixed=np.array(mixed), ratio=np.array(ratio, dtype=np.float64)))
    print(cfg["name"], "seed", seed, "mixed", mixed, "pixels where truncation shows", visible,
          (OUT / f"{cfg['name']}.npz").stat().st_size, "bytes")


def _batch(d, tag, batch):
    d[f"{tag}_img"] = batch["img"].numpy()
    for k in ("bboxes", "cls", "batch_idx"):
        d[f"{tag}_{k}"] = batch[k].numpy()


def dataset_mixup(YOLODataset, watch):
    import mixup_util as X
    images = {name: D.make_image(name) for name in D.SIZES}
    d = {}
    with tempfile.TemporaryDirectory() as tmp:
        img_dir = str(D.write_tree(Path(tmp) / "tiny", images))
        for tag, cfg in X.DATASET.items():
            ds = YOLODataset(img_path=img_dir, imgsz=D.IMGSZ, cache=False, hyp=X.dataset_hyp(tag),
                             data={"names": D.NAMES}, task="detect", augment=True, rect=False,
                             batch_size=cfg["batch_size"], pad=0.0)
            assert ds.max_buffer_length == 8
            D.seed(cfg["seed"])
            samples, buffers, mosaics = [], [], []
            for i in cfg["order"]:
                n, m = len(watch.mix), watch.mosaics
                samples.append(ds[i])
                assert len(watch.mix) == n + 1  # mixup 1.0: every sample is mixed
                buffers.append(list(ds.buffer))
                mosaics.append(watch.mosaics - m)
            if tag == "mix":
                assert set(mosaics) == {2}
            else:  # a letterboxed layer met a mosaic layer, and the other combinations occur too or not: recorded
                assert 1 in mosaics, mosaics
            d[f"{tag}_buffers"] = np.array([b + [-1] * (8 - len(b)) for b in buffers], dtype=np.int64)
            d[f"{tag}_mosaics"] = np.array(mosaics, dtype=np.int64)
            d[f"{tag}_seed"] = np.array(cfg["seed"])
            for k in range(0, len(samples), cfg["collate"]):
                _batch(d, f"{tag}_b{k // cfg['collate']}", YOLODataset.collate_fn(samples[k:k + cfg["collate"]]))
            print(tag, "mosaic layers per sample", mosaics, "last buffer", buffers[-1])
    _save(OUT / "dataset_mixup_tiny.npz", d)
    print("dataset_mixup_tiny.npz", (OUT / "dataset_mixup_tiny.npz").stat().st_size, "bytes,", len(d), "arrays")


def main():
    augment, YOLODataset, Instances = _import_reference()
    OUT.mkdir(parents=True, exist_ok=True)
    watch = _Watch(augment)
    try:
        aug_mixup(augment, YOLODataset, Instances, watch)
        dataset_mixup(YOLODataset, watch)
    finally:
        watch.close()


if __name__ == "__main__":
    main()
