"""Generate the batched-validator fixture by running the REFERENCE's own DetectionValidator bookkeeping — build
container only (like oracle/gen_golden.py and scripts/gen_letterbox_golden.py it refuses to run without the
reference checkout; set ADR_REFERENCE to its path, default: `reference` next to this repository).

Run:  python scripts/gen_val_golden.py

The reference's DetectionValidator is built with __new__ plus the attributes its methods read (as
oracle/gen_golden.py does for BaseValidator); its own init_metrics, update_metrics (plots=True, so the confusion
matrix runs) and get_stats process synthetic batches. Only the plotting switch of the metrics object is turned off
after init_metrics (ap_per_class would draw curves).

Writes (data only) tests/golden/val_batched.npz, for the runs `mc` (nc = 5, three batches) and `sc` (single_cls,
nc = 1, one batch), with <run>_<batch>_ prefixes:
  inputs   det (B, 300, 6) padded detections in letterbox space, counts, cls, bboxes (normalised xywh), batch_idx,
           ori_shape (B, 2), ratio_pad (B, 4: ratio_h, ratio_w, left, top); imgsz
  outputs  gt_xyxy (labels in native space, from _prepare_batch), per run: tp, conf, pred_cls, target_cls, cm,
           nt_per_class, nt_per_image, seen, results_keys / results_vals (results_dict), fitness, p, r, ap,
           ap_class_index

The script asserts that no two confusion-matrix candidate pairs (conf > 0.25, IoU > 0.45) of one image have equal
IoU: such ties are decided by numpy's unstable sort in the reference (parity unpinned) and must not be in the
fixture. It also asserts that the numpy restatement in tests/val_util.py reproduces everything it writes.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
REF = Path(os.environ.get("ADR_REFERENCE", REPO.parent / "reference"))
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO / "tests"))
import val_util as V  # noqa: E402

IMGSZ = (64, 96)  # network input (H, W)
ROWS = 300
F = np.float32


def _import_reference():
    if not REF.is_dir():
        raise SystemExit("gen_val_golden: the reference checkout is not present — fixtures are generated in the "
                         "build container")
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.dont_write_bytecode = True
    os.environ.setdefault("YOLO_CONFIG_DIR", "/tmp/adr_yolo_cfg")
    sys.path.insert(0, str(REPO / "oracle" / "stubs"))
    sys.path.insert(1, str(REF))
    import ultralytics  # noqa: F401
    from ultralytics.models.yolo.detect.val import DetectionValidator
    from ultralytics.utils.metrics import DetMetrics
    return DetectionValidator, DetMetrics


def letterbox_ratio_pad(ori):
    """ratio_pad as the val LetterBox leaves it (data/augment.py:1475-1640, scaleup, center): ((r, r), (left, top))."""
    h0, w0 = ori
    r = min(IMGSZ[0] / h0, IMGSZ[1] / w0)
    nw, nh = int(round(w0 * r)), int(round(h0 * r))
    dw, dh = (IMGSZ[1] - nw) / 2, (IMGSZ[0] - nh) / 2
    return ((r, r), (int(round(dw - 0.1)), int(round(dh - 0.1))))


def to_letterbox(native, rp):
    """native xyxy -> letterbox-space xyxy (fp64; the inputs of the fixture are whatever this gives, as fp32)."""
    g, (px, py) = rp[0][0], rp[1]
    return np.asarray(native, dtype=np.float64) * g + np.array([px, py, px, py], dtype=np.float64)


def norm_xywh(lb_xyxy):
    b = np.asarray(lb_xyxy, dtype=np.float64).reshape(-1, 4)
    H, W = IMGSZ
    return np.stack([(b[:, 0] + b[:, 2]) / 2 / W, (b[:, 1] + b[:, 3]) / 2 / H, (b[:, 2] - b[:, 0]) / W,
                     (b[:, 3] - b[:, 1]) / H], 1).astype(F)


def random_image(rng, ori, n_lab, n_match, n_fp, nc, conf_lo=0.02):
    """Labels in native space (some reach over the border, so the clip acts), detections = jittered labels + false
    positives (some in the letterbox padding), sorted by confidence as NMS returns them."""
    h0, w0 = ori
    rp = letterbox_ratio_pad(ori)
    wh = np.stack([rng.uniform(0.06, 0.5, n_lab) * w0, rng.uniform(0.06, 0.5, n_lab) * h0], 1)
    ctr = np.stack([rng.uniform(-0.02, 1.02, n_lab) * w0, rng.uniform(-0.02, 1.02, n_lab) * h0], 1)
    gt = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1)
    gcls = rng.integers(0, nc, n_lab).astype(F)
    rows = []
    for k in rng.integers(0, max(n_lab, 1), n_match) if n_lab else []:
        j = gt[k] + rng.normal(0, 0.07, 4) * np.r_[wh[k], wh[k]]
        c = gcls[k] if rng.random() < 0.85 else float(rng.integers(0, nc))
        rows.append([*j, rng.uniform(conf_lo, 1.0), c])
    for _ in range(n_fp):
        c0 = np.array([rng.uniform(-0.1, 1.0) * w0, rng.uniform(-0.1, 1.0) * h0])
        rows.append([*c0, *(c0 + np.array([rng.uniform(0.05, 0.4) * w0, rng.uniform(0.05, 0.4) * h0])),
                     rng.uniform(0.001, 0.6), float(rng.integers(0, nc))])
    det = np.array(rows, dtype=np.float64).reshape(-1, 6)
    det = det[np.argsort(-det[:, 4], kind="stable")]
    det[:, :4] = to_letterbox(det[:, :4], rp)
    return dict(ori=ori, rp=rp, cls=gcls, bboxes=norm_xywh(to_letterbox(gt, rp)), det=det.astype(F))


def crafted_image(nc):
    """ori (50, 96): gain 1, pads (0, 7); x coordinates multiples of 3 and integer y are exact through the normalised
    labels (k / 32 * 96, k / 64 * 64), so the IoUs below are exact in fp32.
      tie    L0 (0,10,24,30), L1 (6,10,30,30) class 1; d0 (3,10,27,30) has IoU 420/540 with both -> takes L1 (larger
             index) and, as the lower index, keeps it; d1 (9,10,33,30), best L1 too, is not correct; L0 stays free.
             Both have conf <= 0.25: they are not confusion-matrix candidates (their pairs tie).
      on 0.5 LA (48,10,72,30) class 0, dA (48,10,72,20): IoU 240/480 = 0.5 exactly -> TP at 0.5 only
      below  LB (48,32,72,48) class nc-1, dB (48,32,72,39.999): IoU just under 0.5
      on cm  LC (75,10,96,30), dC (75,10,96,19): IoU 189/420 rounds to float32(0.45) -> not > cm_iou
      above  LD (75,32,96,48), dD (75,32,96,39.3) of another class: IoU 0.456 -> an off-diagonal matrix entry, no TP
    """
    ori = (50, 96)
    rp = letterbox_ratio_pad(ori)
    assert rp == ((1.0, 1.0), (0, 7)), rp
    gt = np.array([[0, 10, 24, 30], [6, 10, 30, 30], [48, 10, 72, 30], [48, 32, 72, 48], [75, 10, 96, 30],
                   [75, 32, 96, 48]], dtype=np.float64)
    gcls = np.array([1, 1, 0, nc - 1, 2, 2], dtype=F)
    det = np.array([[48, 10, 72, 20, 0.9, 0], [75, 10, 96, 19, 0.8, 2], [75, 32, 96, 39.3, 0.7, 3],
                    [48, 32, 72, 39.999, 0.6, nc - 1], [3, 10, 27, 30, 0.2, 1], [9, 10, 33, 30, 0.1, 1]],
                   dtype=np.float64)
    det[:, :4] = to_letterbox(det[:, :4], rp)
    return dict(ori=ori, rp=rp, cls=gcls, bboxes=norm_xywh(to_letterbox(gt, rp)), det=det.astype(F))


def far_image(rng, nc):
    """Labels on the left, confident detections on the right: no pair above cm_iou, so the reference's `if n:`
    leaves the detections out of the matrix and every label goes to the background row."""
    ori = (100, 120)
    rp = letterbox_ratio_pad(ori)
    gt = np.array([[5, 10, 30, 40], [10, 50, 45, 90], [2, 60, 20, 99]], dtype=np.float64)
    det = np.array([[80, 10, 110, 40, 0.9, 0], [70, 50, 119, 95, 0.7, nc - 1], [85, 20, 100, 80, 0.5, 1]],
                   dtype=np.float64)
    det[:, :4] = to_letterbox(det[:, :4], rp)
    return dict(ori=ori, rp=rp, cls=np.array([0, nc - 1, 2], dtype=F), bboxes=norm_xywh(to_letterbox(gt, rp)),
                det=det.astype(F))


def build_batches(nc, single=False):
    rng = np.random.default_rng(20 if single else 7)
    if single:
        imgs = [random_image(rng, (80, 60), 9, 14, 10, 1), random_image(rng, (64, 96), 0, 0, 5, 1),
                random_image(rng, (100, 120), 6, 0, 0, 1), random_image(rng, (40, 90), 12, 30, 35, 1)]
        for im in imgs:  # a multi-class model's classes: single_cls zeroes the column
            im["det"][:, 5] = rng.integers(0, 5, len(im["det"]))
        return [imgs]
    b0 = [random_image(rng, (100, 120), 8, 12, 25, nc),        # 37 detections
          random_image(rng, (40, 90), 5, 0, 0, nc),            # labels, no detections
          random_image(rng, (77, 51), 0, 0, 9, nc),            # detections, no labels
          random_image(rng, (64, 96), 0, 0, 0, nc),            # neither
          crafted_image(nc)]
    b1 = [random_image(rng, (200, 300), 260, 180, 120, nc),    # more labels than one LDS chunk (256); 300 detections
          random_image(rng, (33, 47), 3, 40, 25, nc),          # 65 detections
          far_image(rng, nc),
          random_image(rng, (128, 96), 20, 70, 60, nc)]        # 130 detections
    b2 = [random_image(rng, (50, 96), 4, 6, 2, nc), random_image(rng, (90, 90), 7, 10, 9, nc),
          random_image(rng, (64, 96), 2, 0, 0, nc), random_image(rng, (64, 48), 6, 9, 4, nc)]
    b1[0]["det"] = b1[0]["det"][:ROWS]
    return [b0, b1, b2]


def collate(imgs):
    B = len(imgs)
    det = np.zeros((B, ROWS, 6), dtype=F)
    counts = np.zeros(B, dtype=np.int32)
    for i, im in enumerate(imgs):
        n = len(im["det"])
        assert n <= ROWS
        det[i, :n] = im["det"]
        counts[i] = n
    return dict(det=det, counts=counts, cls=np.concatenate([im["cls"] for im in imgs]).astype(F),
                bboxes=np.concatenate([im["bboxes"] for im in imgs]).astype(F).reshape(-1, 4),
                batch_idx=np.concatenate([np.full(len(im["cls"]), i, dtype=F) for i, im in enumerate(imgs)]),
                ori_shape=np.array([im["ori"] for im in imgs], dtype=np.int64),
                ratio_pad=np.array([[*im["rp"][0], *im["rp"][1]] for im in imgs], dtype=np.float64),
                rp=[im["rp"] for im in imgs], ori=[im["ori"] for im in imgs])


def run_reference(DetectionValidator, DetMetrics, batches, nc, single):
    v = DetectionValidator.__new__(DetectionValidator)
    v.args = SimpleNamespace(conf=0.001, iou=0.7, single_cls=single, plots=True, save_json=False, save_txt=False,
                             save_hybrid=False, half=False, val=True, split="val", task="detect", max_det=ROWS,
                             agnostic_nms=False, verbose=False)
    v.device = torch.device("cpu")
    v.training = False
    v.data = {}
    v.save_dir = Path("/tmp/adr_val_golden")
    v.on_plot = None
    v.iouv = torch.linspace(0.5, 0.95, 10)
    v.niou = v.iouv.numel()
    v.lb = []
    v.metrics = DetMetrics(save_dir=v.save_dir, on_plot=None)
    v.init_metrics(SimpleNamespace(names={i: f"c{i}" for i in range(nc)}))
    v.metrics.plot = False
    gts = []
    for cb in batches:
        batch = {"img": torch.zeros(len(cb["counts"]), 3, *IMGSZ), "batch_idx": torch.from_numpy(cb["batch_idx"]),
                 "cls": torch.from_numpy(cb["cls"]).view(-1, 1), "bboxes": torch.from_numpy(cb["bboxes"]),
                 "ori_shape": cb["ori"], "ratio_pad": cb["rp"], "im_file": [f"i{k}.jpg" for k in range(len(cb["ori"]))]}
        preds = [torch.from_numpy(cb["det"][i, :n].copy()) for i, n in enumerate(cb["counts"])]
        gt = np.zeros((len(cb["cls"]), 4), dtype=F)
        for si in range(len(preds)):
            pb = v._prepare_batch(si, batch)
            gt[cb["batch_idx"] == si] = pb["bbox"].numpy().reshape(-1, 4)
        gts.append(gt)
        v.update_metrics(preds, batch)
    stats = {k: torch.cat(x, 0).cpu().numpy() for k, x in v.stats.items()}
    res = v.get_stats()
    return v, stats, res, gts


def main():
    DetectionValidator, DetMetrics = _import_reference()
    OUT.mkdir(parents=True, exist_ok=True)
    d = {"imgsz": np.array(IMGSZ, dtype=np.int64)}
    for run, nc, single in (("mc", 5, False), ("sc", 1, True)):
        batches = [collate(b) for b in build_batches(nc, single)]
        v, stats, res, gts = run_reference(DetectionValidator, DetMetrics, batches, nc, single)
        # the tie condition on the inputs, and the restatement against the reference
        cm = np.zeros((nc + 1, nc + 1), dtype=np.int64)
        ntc, nti, tp = np.zeros(nc, np.int64), np.zeros(nc, np.int64), []
        for bi, (cb, gt) in enumerate(zip(batches, gts)):
            tab = [V.table_row(o, r) for o, r in zip(cb["ori"], cb["rp"])]
            mine = V.run_batch(cb["det"], cb["counts"], cb["cls"], cb["bboxes"], cb["batch_idx"], tab, IMGSZ, nc,
                               single_cls=single)
            assert np.array_equal(mine["gt_xyxy"], gt), (run, bi)
            for i, n in enumerate(cb["counts"]):
                g = gt[cb["batch_idx"] == i]
                iou = V.box_iou(g, mine["predn"][i][:, :4])
                cand = V.cm_candidates(iou, mine["predn"][i][:, 4], 0.25, 0.45)
                assert len(np.unique(cand)) == len(cand), f"{run} batch {bi} image {i}: tied confusion-matrix pairs"
                if n or len(g):
                    tp.append(mine["correct"][i, :n].astype(bool))
            cm += mine["cm"]
            ntc += mine["nt_per_class"]
            nti += mine["nt_per_image"]
            for k in ("det", "counts", "cls", "bboxes", "batch_idx", "ori_shape", "ratio_pad"):
                d[f"{run}_{bi}_{k}"] = cb[k]
            d[f"{run}_{bi}_gt_xyxy"] = gt
        assert np.array_equal(np.concatenate(tp, 0), stats["tp"]), run
        assert np.array_equal(cm, v.confusion_matrix.matrix.astype(np.int64)), run
        assert np.array_equal(ntc, v.nt_per_class) and np.array_equal(nti, v.nt_per_image), run
        m = v.metrics.box
        d.update({f"{run}_nbatches": np.array(len(batches)), f"{run}_nc": np.array(nc),
                  f"{run}_tp": stats["tp"], f"{run}_conf": stats["conf"], f"{run}_pred_cls": stats["pred_cls"],
                  f"{run}_target_cls": stats["target_cls"], f"{run}_cm": v.confusion_matrix.matrix,
                  f"{run}_cm_tp": v.confusion_matrix.tp_fp()[0], f"{run}_cm_fp": v.confusion_matrix.tp_fp()[1],
                  f"{run}_nt_per_class": v.nt_per_class.astype(np.int64),
                  f"{run}_nt_per_image": v.nt_per_image.astype(np.int64), f"{run}_seen": np.array(v.seen),
                  f"{run}_results_keys": np.array(list(res.keys())),
                  f"{run}_results_vals": np.array([float(x) for x in res.values()], dtype=np.float64),
                  f"{run}_fitness": np.array(float(v.metrics.fitness), dtype=np.float64),
                  f"{run}_p": np.asarray(m.p, dtype=np.float64), f"{run}_r": np.asarray(m.r, dtype=np.float64),
                  f"{run}_ap": np.asarray(m.all_ap, dtype=np.float64).reshape(-1, 10),
                  f"{run}_ap_class_index": np.asarray(m.ap_class_index, dtype=np.int64)})
        print(run, "images", v.seen, "dets", len(stats["tp"]), "tp@.5", int(stats["tp"][:, 0].sum()), "labels",
              int(v.nt_per_class.sum()), "cm sum", int(v.confusion_matrix.matrix.sum()), res)
    np.savez_compressed(OUT / "val_batched.npz", **d)
    print("wrote", OUT / "val_batched.npz", (OUT / "val_batched.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
