"""Generate the LetterBox fixtures by running the REFERENCE's own code — build container only (like
oracle/gen_golden.py it refuses to run without the reference checkout).

Run:  python scripts/gen_letterbox_golden.py

The reference is imported the way oracle/gen_golden.py `_import_reference` does (oracle/stubs for the packages
absent from the image). The two OpenCV calls LetterBox makes are not in oracle/stubs/cv2; they are set on the
imported stub module at run time to the numpy restatements of tests/letterbox_util.py (cv2.resize INTER_LINEAR 8U,
cv2.copyMakeBorder constant), so the fixtures pin the reference's arithmetic around them (ratio, new_unpad, the
+-0.1 rounding of the pads, the label update, scale_boxes / clip_boxes) while OpenCV's internals are PARITY UNPINNED.

Writes (data only):
  tests/golden/letterbox_cases.npz      per case of letterbox_util.CASES: the reference LetterBox output image from
                                        labels (and, checked equal, from image= alone), ratio_pad, resized_shape,
                                        updated boxes / cls, scale_boxes results (ratio_pad None and given) and
                                        clip_boxes
  tests/golden/aug_closemosaic_256.npz  v8_transforms (default hyp, mosaic = 0) + Format + YOLODataset.collate_fn
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

REF = Path("/root/reference")
REPO = Path(__file__).resolve().parents[1]
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO / "oracle"))
sys.path.insert(0, str(REPO / "tests"))
import letterbox_util as U  # noqa: E402


def _import_reference():
    if not REF.is_dir():
        raise SystemExit("gen_letterbox_golden: the reference checkout is not present — fixtures are generated in "
                         "the build container")
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.dont_write_bytecode = True
    os.environ.setdefault("YOLO_CONFIG_DIR", "/tmp/adr_yolo_cfg")
    sys.path.insert(0, str(REPO / "oracle" / "stubs"))
    sys.path.insert(1, str(REF))
    import cv2
    cv2.resize = U.resize
    cv2.copyMakeBorder = U.copyMakeBorder
    cv2.INTER_LINEAR, cv2.BORDER_CONSTANT = U.INTER_LINEAR, U.BORDER_CONSTANT
    import ultralytics  # noqa: F401
    from ultralytics.data import augment
    from ultralytics.data.dataset import YOLODataset
    from ultralytics.utils import ops as uops
    from ultralytics.utils.instance import Instances
    return augment, YOLODataset, uops, Instances


def letterbox_cases(augment, uops, Instances):
    d = {"names": np.array([c[0] for c in U.CASES])}
    for i, (name, _, kw, _) in enumerate(U.CASES):
        src, _, _, det = U.case_inputs(i)
        labels = augment.LetterBox(**kw)(U.case_labels(i, Instances))
        img = labels["img"]
        new_shape = U.CASES[i][3] or kw["new_shape"]
        if U.CASES[i][3] is None:  # image= alone gives the same pixels (rect_shape only exists in labels)
            assert np.array_equal(augment.LetterBox(**kw)(image=src), img)
        (ratio0, (left, top)) = labels["ratio_pad"]
        ins = labels["instances"]
        assert ins._bboxes.format == "xyxy" and not ins.normalized
        d[f"{name}_img"] = img
        d[f"{name}_bboxes"] = ins.bboxes
        d[f"{name}_cls"] = labels["cls"]
        d[f"{name}_pad"] = np.array([left, top], dtype=np.int64)
        d[f"{name}_ratio_in"] = np.array(ratio0, dtype=np.float64)
        d[f"{name}_resized_shape"] = np.array(labels["resized_shape"], dtype=np.int64)
        # detections in letterboxed coordinates back to the source image, as detect/predict.py does (ratio_pad None),
        # as the validator does (ratio_pad given), and the clip alone
        h0, w0 = src.shape[:2]
        t = torch.from_numpy(det)
        d[f"{name}_scaled"] = uops.scale_boxes(img.shape[:2], t.clone(), (h0, w0)).numpy()
        rp = ((new_shape[0] / h0 * 0.97, new_shape[1] / w0 * 0.97), (left, top))
        d[f"{name}_rp"] = np.array([rp[0][0], rp[0][1], left, top], dtype=np.float64)
        d[f"{name}_scaled_rp"] = uops.scale_boxes(img.shape[:2], t.clone(), (h0, w0), ratio_pad=rp).numpy()
        d[f"{name}_scaled_xywh"] = uops.scale_boxes(img.shape[:2], t.clone(), (h0, w0), xywh=True).numpy()
        d[f"{name}_clipped"] = uops.clip_boxes(t.clone(), (h0, w0)).numpy()
        print(name, img.shape, (left, top), ins.bboxes.shape)
    np.savez_compressed(OUT / "letterbox_cases.npz", **d)


def close_mosaic_chain(augment, YOLODataset, Instances):
    from recipe import synthetic_aug_items
    cfg = U.CLOSE_MOSAIC

    class _DS:
        def __init__(self, items, imgsz):
            self.items, self.imgsz = items, imgsz
            self.buffer = list(range(len(items)))
            self.data = {"flip_idx": []}
            self.use_keypoints = False

        def __len__(self):
            return len(self.items)

        def get_image_and_label(self, i):
            it = self.items[i]
            h, w = it["img"].shape[:2]
            return {"im_file": f"syn{i}.jpg", "ori_shape": (h, w), "resized_shape": (h, w), "ratio_pad": (1.0, 1.0),
                    "img": it["img"].copy(), "cls": it["cls"].copy(),
                    "instances": Instances(it["bboxes"].copy(), np.zeros((0, 1000, 2), dtype=np.float32), None,
                                           bbox_format="xywh", normalized=True)}

    hyp = U.close_mosaic_hyp()
    ds = _DS(synthetic_aug_items(8, cfg["imgsz"]), cfg["imgsz"])
    T = augment.v8_transforms(ds, cfg["imgsz"], hyp)
    T.append(augment.Format(bbox_format="xywh", normalize=True, return_mask=False, return_keypoint=False,
                            return_obb=False, batch_idx=True, mask_ratio=4, mask_overlap=True, bgr=hyp.bgr))
    U.seed_chain(cfg["seed"])
    batch = YOLODataset.collate_fn([T(ds.get_image_and_label(i)) for i in cfg["order"]])
    np.savez_compressed(OUT / f"{cfg['name']}.npz", img=batch["img"].numpy(), cls=batch["cls"].numpy(),
                        bboxes=batch["bboxes"].numpy(), batch_idx=batch["batch_idx"].numpy(), seed=cfg["seed"],
                        imgsz=cfg["imgsz"], order=np.array(cfg["order"]))
    print(cfg["name"], tuple(batch["img"].shape), tuple(batch["bboxes"].shape))


def main():
    augment, YOLODataset, uops, Instances = _import_reference()
    OUT.mkdir(parents=True, exist_ok=True)
    letterbox_cases(augment, uops, Instances)
    close_mosaic_chain(augment, YOLODataset, Instances)


if __name__ == "__main__":
    main()
