"""Generate the validation-loss fixture by running the REFERENCE's own eval forward and model.loss(batch, preds) —
build container only (like scripts/gen_val_golden.py it refuses to run without the reference checkout; set
ADR_REFERENCE to its path, default: `reference` next to this repository).

Run:  python scripts/gen_valloss_golden.py

What the reference's validator does per batch while training (engine/validator.py:176-184): preds = model(img) in
eval mode, self.loss += model.loss(batch, preds)[1]; after the loop self.loss.cpu() / len(dataloader) (:204). Here,
on the CPU in fp32 through oracle/stubs, for the 701 yaml (`n701`) and the stock yolo11n (`y11n`), both with nc = 16
and the recipe weights of the net fixtures (oracle/recipe.recipe_state_dict). yolo11n runs at 64 x 96 (H x W). The
701 model cannot: its multi-scale token mixer pools the P5 map to (H // 4, W // 4) (nn/modules/block.py:2452), which
is empty below 128 pixels, and its EDFFN reflect-pads the P5 map to a multiple of 8 (block.py:2404), which needs a
side of at least 5 — the reference raises at both. So the 701 batches are 160 x 192 (P5 5 x 6), its smallest
non-square shape:

  three batches of two uint8 images; batch 0 has labels in both images, batch 1 an image without labels, batch 2 no
  labels at all.

Writes (data only) tests/golden/val_loss.npz:
  inputs   nc, <tag>_imgsz (H, W), <tag>_b<k>_img uint8 (2, 3, H, W); b<k>_batch_idx, b<k>_cls (n, 1),
           b<k>_bboxes (n, 4) normalised xywh (shared by both models)
  outputs  <tag>_items (3, 3) the per-batch loss_items, <tag>_mean (3,) = sum over batches / 3 in fp32 in batch order
and tests/golden/results_csv.txt: the header and one value line as the reference's BaseTrainer.save_metrics formats
them (engine/trainer.py:652-659), from the metrics dict of a detection run with fixed sample values (the `time`
column, which save_metrics takes from the wall clock, is pinned by fixing time.time during the call), followed by the
values that produced the line.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
REF = Path(os.environ.get("ADR_REFERENCE", REPO.parent / "reference"))
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO / "oracle"))
from recipe import recipe_state_dict  # noqa: E402

IMGSZ = {"n701": (160, 192), "y11n": (64, 96)}
NC = 16
NB, B = 3, 2
# the sample row of results_csv.txt: values with more than six significant digits, small and large magnitudes
CSV_SAMPLE = {"train/box_loss": 1.23457, "train/cls_loss": 0.98765, "train/dfl_loss": 10.5, "metrics/precision(B)": 0.5,
              "metrics/recall(B)": 0.33333, "metrics/mAP50(B)": 0.41234, "metrics/mAP50-95(B)": 1e-05,
              "val/box_loss": 2.0, "val/cls_loss": 3.14159, "val/dfl_loss": 0.0, "lr/pg0": 0.0700123456,
              "lr/pg1": 0.000333333333, "lr/pg2": 1.2345678e-05}
CSV_EPOCH, CSV_TIME = 6, 1234.56789


def _import_reference():
    if not REF.is_dir():
        raise SystemExit("gen_valloss_golden: the reference checkout is not present — fixtures are generated in the "
                         "build container")
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.dont_write_bytecode = True
    os.environ.setdefault("YOLO_CONFIG_DIR", "/tmp/adr_yolo_cfg")
    sys.path.insert(0, str(REPO / "oracle" / "stubs"))
    sys.path.insert(1, str(REF))
    import ultralytics  # noqa: F401
    from ultralytics.engine.trainer import BaseTrainer
    from ultralytics.nn import tasks
    return tasks, BaseTrainer


def images(tag):
    """Seeded uint8 images: 8 x 8 blocks of uniform noise (compressible, and with edges for the network)."""
    rng = np.random.default_rng(40 + len(tag) + ord(tag[0]))
    H, W = IMGSZ[tag]
    return [np.repeat(np.repeat(rng.integers(0, 256, (B, 3, H // 8, W // 8), dtype=np.uint8), 8, 2), 8, 3)
            for _ in range(NB)]


def batches():
    """The labels of both models' batches (normalised, so they fit either image size)."""
    rng = np.random.default_rng(31)
    out = []
    counts = [(3, 2), (4, 0), (0, 0)]
    for k in range(NB):
        bi, cl, bx = [], [], []
        for j, n in enumerate(counts[k]):
            ctr = rng.uniform(0.2, 0.8, (n, 2))
            wh = rng.uniform(0.15, 0.55, (n, 2))
            bi.append(np.full(n, j, np.float32))
            cl.append(rng.integers(0, NC, n).astype(np.float32))
            bx.append(np.concatenate([ctr, wh], 1).astype(np.float32))
        out.append({"batch_idx": np.concatenate(bi), "cls": np.concatenate(cl).reshape(-1, 1),
                    "bboxes": np.concatenate(bx).reshape(-1, 4)})
    return out


def run_model(tasks, cfg, bts, imgs):
    model = tasks.DetectionModel(str(cfg), nc=NC, verbose=False)
    for mm in model.modules():
        if isinstance(mm, torch.nn.Dropout):
            mm.p = 0.0
    sd = model.state_dict()
    model.load_state_dict(recipe_state_dict([(k, v.shape) for k, v in sd.items()]), strict=True)
    model.args = type("H", (), {"box": 7.5, "cls": 0.5, "dfl": 1.5})()
    model.eval()
    total, items = None, []
    for b, img in zip(bts, imgs):
        batch = {"img": torch.from_numpy(img).float() / 255, "batch_idx": torch.from_numpy(b["batch_idx"]),
                 "cls": torch.from_numpy(b["cls"]), "bboxes": torch.from_numpy(b["bboxes"])}
        with torch.no_grad():
            preds = model(batch["img"])
            it = model.loss(batch, preds)[1]
        items.append(it.float().numpy().copy())
        total = it.clone() if total is None else total + it
    return np.stack(items), (total.cpu() / len(bts)).numpy()


def csv_lines(BaseTrainer, tmp):
    import time
    t = BaseTrainer.__new__(BaseTrainer)
    Path(tmp).mkdir(parents=True, exist_ok=True)
    t.csv = Path(tmp) / "results.csv"
    if t.csv.exists():
        t.csv.unlink()
    t.epoch = CSV_EPOCH
    t.train_time_start = 0.0
    real = time.time
    time.time = lambda: CSV_TIME
    try:
        t.save_metrics(metrics=dict(CSV_SAMPLE))
    finally:
        time.time = real
    lines = t.csv.read_text().splitlines()
    assert len(lines) == 2
    return lines


def main():
    tasks, BaseTrainer = _import_reference()
    OUT.mkdir(parents=True, exist_ok=True)
    bts = batches()
    d = {"nc": np.array(NC), "nbatches": np.array(NB)}
    for k, b in enumerate(bts):
        for key, v in b.items():
            d[f"b{k}_{key}"] = v
    for tag, cfg in (("n701", REPO / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"),
                     ("y11n", REPO / "tests" / "configs" / "yolo11n.yaml")):
        imgs = images(tag)
        d[f"{tag}_imgsz"] = np.array(IMGSZ[tag], dtype=np.int64)
        for k, im in enumerate(imgs):
            d[f"{tag}_b{k}_img"] = im
        items, mean = run_model(tasks, cfg, bts, imgs)
        d[f"{tag}_items"], d[f"{tag}_mean"] = items.astype(np.float32), mean.astype(np.float32)
        print(tag, "items", items.tolist(), "mean", mean.tolist())
    np.savez_compressed(OUT / "val_loss.npz", **d)
    print("wrote", OUT / "val_loss.npz", (OUT / "val_loss.npz").stat().st_size, "bytes")
    header, row = csv_lines(BaseTrainer, "/tmp/adr_valloss_golden")
    vals = [f"epoch={CSV_EPOCH}", f"time={CSV_TIME!r}"] + [f"{k}={v!r}" for k, v in CSV_SAMPLE.items()]
    (OUT / "results_csv.txt").write_text("\n".join([header, row, *vals]) + "\n")
    print(header)
    print(row)


if __name__ == "__main__":
    main()
