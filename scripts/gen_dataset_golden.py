"""Generate the YOLODataset fixture by running the REFERENCE's own dataset code — build container only (like
oracle/gen_golden.py it refuses to run without the reference checkout). CPU only.

Run:  python scripts/gen_dataset_golden.py

The reference is imported as scripts/gen_letterbox_golden.py imports it (oracle/stubs for the packages absent from
the image). The cv2 stub has no resize / imread: cv2.resize and cv2.copyMakeBorder are set to the numpy restatements
of tests/letterbox_util.py (PARITY UNPINNED against real OpenCV) and cv2.imread to a PIL decode (RGB reversed to BGR;
the tree holds lossless PNGs, and one image is read from its .npy sibling by the reference itself). The reference's
own YOLODataset CONSTRUCTOR runs (get_img_files, the label verification and its .cache in the temporary directory,
update_labels, set_rectangle, build_transforms), not unbound methods on a stand-in. The tiny dataset (tests/
dataset_util.py: seeded images, label texts) is written to a temporary directory; every pass runs at imgsz 64.

Writes tests/golden/dataset_tiny.npz (data only): the native images, the label texts, im_files order, the verified
labels (plain, and with classes=[0, 2] + single_cls), load_image's outputs, set_rectangle's order and batch_shapes,
a seeded training pass (buffer after every sample, collated batches), the same pass with every image resident (the
reference's cache="ram" filled in index order), a close-mosaic pass, a rect and a square
validation pass. Every load_image output is asserted to lie within 1 grey level of
round(F.interpolate(bilinear, align_corners=False)) of its source, except on the exact-2x (area path) image: that
anchors the fixture outside the restatement."""
from __future__ import annotations

import os
import sys
import tempfile
import zipfile
from pathlib import Path

import numpy as np
import torch

REF = Path("/root/reference")
REPO = Path(__file__).resolve().parents[1]
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO / "oracle"))
sys.path.insert(0, str(REPO / "tests"))
import dataset_util as D  # noqa: E402
import letterbox_util as U  # noqa: E402


def _import_reference():
    if not REF.is_dir():
        raise SystemExit("gen_dataset_golden: the reference checkout is not present — fixtures are generated in "
                         "the build container")
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
    from ultralytics.data.dataset import YOLODataset
    return YOLODataset


def _labels(ds, d, tag):
    for i, lb in enumerate(ds.labels):
        d[f"{tag}_cls_{i}"] = lb["cls"]
        d[f"{tag}_bboxes_{i}"] = lb["bboxes"]
        assert lb["normalized"] is True and lb["bbox_format"] == "xywh" and len(lb["segments"]) == 0
        if "shape" in lb:
            d[f"{tag}_shape_{i}"] = np.array(lb["shape"], dtype=np.int64)


def _batch(d, tag, batch):
    d[f"{tag}_img"] = batch["img"].numpy()
    for k in ("bboxes", "cls", "batch_idx"):
        d[f"{tag}_{k}"] = batch[k].numpy()
    if "ratio_pad" in batch:
        d[f"{tag}_im_file"] = np.array([Path(f).name for f in batch["im_file"]])
        d[f"{tag}_ori_shape"] = np.array(batch["ori_shape"], dtype=np.int64)
        d[f"{tag}_resized_shape"] = np.array([tuple(int(v) for v in s) for s in batch["resized_shape"]], dtype=np.int64)
        d[f"{tag}_ratio_pad"] = np.array([[rp[0][0], rp[0][1], rp[1][0], rp[1][1]] for rp in batch["ratio_pad"]],
                                         dtype=np.float64)


def main():
    YOLODataset = _import_reference()
    images = {name: D.make_image(name) for name in D.SIZES}
    d = {f"native_{name}": im for name, im in images.items()}
    d["names"] = np.array(list(D.SIZES))
    d["label_texts"] = np.array(["<missing>" if D.LABEL_TEXTS[n] is None else D.LABEL_TEXTS[n] for n in D.SIZES])
    data = {"names": D.NAMES}
    with tempfile.TemporaryDirectory() as tmp:
        img_dir = str(D.write_tree(Path(tmp) / "tiny", images))

        def make(**kw):
            kw = dict(dict(img_path=img_dir, imgsz=D.IMGSZ, cache=False, hyp=D.hyp(), data=data, task="detect"), **kw)
            return YOLODataset(**kw)

        # files, labels, load_image (augment off: no buffer)
        ds = make(augment=False, rect=False, batch_size=4)
        d["im_files"] = np.array([Path(f).name for f in ds.im_files])
        assert len(ds.im_files) == 8 and "im9.png" not in set(d["im_files"])
        _labels(ds, d, "labels")
        anchors = 0
        for i in range(ds.ni):
            im, hw0, hw = ds.load_image(i)
            d[f"load_img_{i}"], d[f"load_hw0_{i}"], d[f"load_hw_{i}"] = im, np.array(hw0), np.array(hw)
            name = Path(ds.im_files[i]).stem
            src = images[name]
            assert tuple(hw0) == src.shape[:2] and im.shape[:2] == tuple(hw)
            if src.shape[0] == 2 * hw[0] and src.shape[1] == 2 * hw[1]:
                continue  # INTER_LINEAR's area fast path: not bilinear point sampling
            t = torch.from_numpy(src.astype(np.float32)).permute(2, 0, 1)[None]
            want = torch.nn.functional.interpolate(t, size=tuple(hw), mode="bilinear", align_corners=False)
            want = want[0].permute(1, 2, 0).round().numpy()
            assert np.abs(want - im.astype(np.float32)).max() <= 1, (name, np.abs(want - im).max())
            anchors += 1
        assert anchors == 7
        dsq = ds
        # update_labels: classes + single_cls
        _labels(make(augment=False, rect=False, batch_size=4, classes=D.CLASSES, single_cls=True), d, "labels_sel")
        # set_rectangle
        dr = make(augment=False, rect=True, **D.RECT)
        d["rect_im_files"] = np.array([Path(f).name for f in dr.im_files])
        d["rect_batch_shapes"], d["rect_batch"] = np.asarray(dr.batch_shapes, dtype=np.int64), np.asarray(dr.batch)
        # seeded training pass: batch_size 1 -> max_buffer_length = min(ni, 8, 1000) = 8: the buffer evicts
        cfg = D.TRAIN
        hyp = D.hyp()
        dt = make(augment=True, rect=False, batch_size=cfg["batch_size"], pad=0.0, hyp=hyp)
        assert dt.max_buffer_length == 8
        D.seed(cfg["seed"])
        samples, buffers = [], []
        for i in cfg["order"]:
            samples.append(dt[i])
            buffers.append(list(dt.buffer))
        assert any(len(b) < 8 for b in buffers) and buffers[-1][0] != 0  # the buffer filled up and evicted
        d["train_buffers"] = np.array([b + [-1] * (8 - len(b)) for b in buffers], dtype=np.int64)
        for k in range(0, len(samples), cfg["collate"]):
            _batch(d, f"train_b{k // cfg['collate']}", YOLODataset.collate_fn(samples[k:k + cfg["collate"]]))
        # close-mosaic pass on the same dataset (its buffer goes on)
        dt.close_mosaic(hyp)
        D.seed(D.CLOSE["seed"])
        samples = [dt[i] for i in D.CLOSE["order"]]
        d["close_buffer"] = np.array(list(dt.buffer), dtype=np.int64)
        _batch(d, "close_b0", YOLODataset.collate_fn(samples))
        # the training pass with every image resident (the reference's cache="ram", loaded here in index order by
        # the statements of its cache_images loop: its ThreadPool's order is not deterministic): load_image then
        # never appends to the buffer again
        dc = make(augment=True, rect=False, batch_size=cfg["batch_size"], pad=0.0, hyp=D.hyp())
        dc.cache = "ram"
        for i in range(dc.ni):
            dc.ims[i], dc.im_hw0[i], dc.im_hw[i] = dc.load_image(i)
        d["trainres_buffer"] = np.array(list(dc.buffer), dtype=np.int64)
        D.seed(cfg["seed"])
        samples = [dc[i] for i in cfg["order"][:D.RESIDENT_N]]  # one batch keeps the file small
        assert list(dc.buffer) == d["trainres_buffer"].tolist() == [1, 2, 3, 4, 5, 6, 7]
        for k in range(0, len(samples), cfg["collate"]):
            _batch(d, f"trainres_b{k // cfg['collate']}", YOLODataset.collate_fn(samples[k:k + cfg["collate"]]))
        # validation: rect (one shape per batch) and square
        for tag, dv, bs in (("valrect", dr, D.RECT["batch_size"]), ("valsq", dsq, 4)):
            for b, k in enumerate(range(0, dv.ni, bs)):
                _batch(d, f"{tag}_b{b}", YOLODataset.collate_fn([dv[i] for i in range(k, min(k + bs, dv.ni))]))
    OUT.mkdir(parents=True, exist_ok=True)
    # an .npz is a zip of .npy members; LZMA members (np.load reads them through zipfile like deflated ones) are a
    # third smaller on these smooth images than np.savez_compressed's deflate
    with zipfile.ZipFile(OUT / "dataset_tiny.npz", "w", compression=zipfile.ZIP_LZMA) as z:
        for k, v in d.items():
            with z.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)
    print("dataset_tiny.npz", (OUT / "dataset_tiny.npz").stat().st_size, "bytes,", len(d), "arrays")


if __name__ == "__main__":
    main()
