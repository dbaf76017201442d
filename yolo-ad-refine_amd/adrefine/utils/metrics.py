"""Validator metrics tail — drop-in for the reference's detection validation bookkeeping:
models/yolo/detect/val.py:125-229 (update_metrics, _process_batch, get_stats), engine/validator.py:221-261
(match_predictions), utils/metrics.py:52-72 (box_iou), :1054-1059 (smooth), :1112-1141 (compute_ap),
:1144-1231 (ap_per_class), :1234-1360 (Metric: mp, mr, map50, map, fitness).

The per-image work runs on the device: the IoU matrix (adr_box_iou) and the TP matching at the ten IoU thresholds
(adr_match_predictions: each detection's best same-class label, then per label and threshold the lowest-index
detection claiming it). The dataset-level AP integration runs once on the host over the concatenated statistics, from
the definitions below (own formulation, pinned by tests/golden/metrics_val.npz which the reference itself produced).
Boxes are compared in the network's input space (the reference's scale_boxes to the original image is the identity
for unpadded, unresized inputs; callers with letterboxed images scale both sides first).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import kernels as K
from ..native import lib

IOUV = np.linspace(0.5, 0.95, 10)  # the validator's mAP@0.5:0.95 thresholds (val.py:36)
_PR_POINTS = 1000  # resolution of the confidence-indexed precision / recall curves (metrics.py:1191)
_AP_POINTS = 101   # COCO interpolation points (metrics.py:1135)


def box_iou(box1: torch.Tensor, box2: torch.Tensor, eps=1e-7) -> torch.Tensor:
    """(N, 4) x (M, 4) xyxy -> (N, M) IoU on the device (adr_box_iou; utils/metrics.py:52-72)."""
    if not box1.is_cuda:
        raise RuntimeError("box_iou: device tensors required (HIP kernel, no CPU fallback)")
    a = box1.float().contiguous()
    b = box2.float().contiguous()
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
    lib.adr_box_iou(K.fptr(a), a.shape[0], K.fptr(b), b.shape[0], float(eps), K.fptr(out), K.stream())
    return out


_THR = {}


def match_predictions(pred_classes, true_classes, iou, iouv=IOUV):
    """engine/validator.py:221-261 (greedy): (P, T) bool of correct detections, computed by adr_match_predictions from
    the (G, P) IoU matrix of one image. Thresholds are applied in float32, as the reference's comparison of a float32
    IoU array with Python floats is.

    Limits, by design: P <= 2048 detections per image (the kernel keeps each detection's best label in LDS). The
    detections come from adr_nms, which caps max_det at 300, so this path never approaches it; a larger P raises.
    Exact IoU ties between labels go to the larger label index — what the reference's reversed ascending argsort
    gives on small inputs; numpy's sort is not stable on large ones, so tie handling there is parity unpinned (a
    documented deviation)."""
    dev = iou.device
    G, P = iou.shape
    T = len(iouv)
    if G == 0 or P == 0:
        return np.zeros((P, T), dtype=bool)
    key = (str(dev), tuple(np.asarray(iouv, dtype=np.float64).tolist()))
    thr = _THR.get(key)
    if thr is None:
        thr = torch.tensor(np.asarray(iouv, dtype=np.float32), device=dev)
        _THR[key] = thr
    io = iou.float().contiguous()
    gc = true_classes.to(dev).float().contiguous()
    pc = pred_classes.to(dev).float().contiguous()
    out = torch.empty(P, T, dtype=torch.uint8, device=dev)
    lib.adr_match_predictions(K.fptr(io), G, P, K.fptr(gc), K.fptr(pc), K.fptr(thr), T, K.fptr(out), K.stream())
    return out.cpu().numpy().astype(bool)


def box_filter(y, frac):
    """metrics.py:1054-1059: moving average over an odd window of about 2*frac of the curve, the ends extended with
    the edge values."""
    width = round(len(y) * frac * 2) // 2 + 1
    ext = np.pad(y, width // 2, mode="edge")
    return np.convolve(ext, np.full(width, 1.0 / width), mode="valid")


def interpolated_ap(recall, precision):
    """metrics.py:1112-1141. Area under the precision envelope (the running maximum of precision taken from the
    high-recall end), sampled at 101 equally spaced recall levels and integrated with the trapezoid rule. The curve is
    anchored at (recall 0, precision 1) and (recall 1, precision 0)."""
    r = np.concatenate(([0.0], recall, [1.0]))
    envelope = np.maximum.accumulate(np.concatenate(([1.0], precision, [0.0]))[::-1])[::-1]
    grid = np.linspace(0, 1, _AP_POINTS)
    v = np.interp(grid, r, envelope)
    return float(np.sum(np.diff(grid) * (v[1:] + v[:-1])) / 2.0)


def ap_per_class(tp, conf, pred_cls, target_cls, eps=1e-16):
    """metrics.py:1144-1231 (no plotting). tp (n, T) bool, conf (n,), pred_cls (n,), target_cls (m,). Returns
    (tp, fp, p, r, f1, ap, classes, p_curve, r_curve, f1_curve, x) with the reference's meaning: p / r / f1 per class
    at the single confidence that maximises the smoothed class-mean F1, ap (classes, T)."""
    rank = np.argsort(-conf)  # confidence order, same sort rule as the reference
    hits, score, klass = tp[rank], conf[rank], pred_cls[rank]
    classes, n_labels = np.unique(target_cls, return_counts=True)
    n_cls, T = classes.shape[0], tp.shape[1]
    xs = np.linspace(0, 1, _PR_POINTS)
    ap = np.zeros((n_cls, T))
    p_curve = np.zeros((n_cls, _PR_POINTS))
    r_curve = np.zeros((n_cls, _PR_POINTS))
    for k in range(n_cls):
        sel = klass == classes[k]
        n_det = int(sel.sum())
        if n_det == 0 or n_labels[k] == 0:
            continue
        true_pos = np.cumsum(hits[sel], axis=0)  # (n_det, T) integer running counts
        seen = np.arange(1, n_det + 1)[:, None]    # detections so far = TP + FP
        recall = true_pos / (n_labels[k] + eps)
        precision = true_pos / seen
        neg_score = -score[sel]  # ascending abscissa for np.interp
        r_curve[k] = np.interp(-xs, neg_score, recall[:, 0], left=0)
        p_curve[k] = np.interp(-xs, neg_score, precision[:, 0], left=1)
        for t in range(T):
            ap[k, t] = interpolated_ap(recall[:, t], precision[:, t])
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    at = int(box_filter(f1_curve.mean(0), 0.1).argmax())
    p, r, f1 = p_curve[:, at], r_curve[:, at], f1_curve[:, at]
    n_tp = (r * n_labels).round()
    n_fp = (n_tp / (p + eps) - n_tp).round()
    return n_tp, n_fp, p, r, f1, ap, classes.astype(int), p_curve, r_curve, f1_curve, xs


class ConfusionMatrix:
    """The detection validator's confusion matrix (metrics.py:900-1000, task='detect', no plotting): `matrix` is
    the reference's float64 (nc + 1, nc + 1) array, rows = predicted class (last: background), columns = true class.
    The counts are accumulated on the device by adr_val_match (int32) and read when `matrix` is."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45, counts=None):
        self.nc = nc
        self.conf = 0.25 if conf in {None, 0.001} else conf  # metrics.py:917
        self.iou_thres = iou_thres
        self.counts = counts if counts is not None else np.zeros((nc + 1, nc + 1), dtype=np.int64)

    @property
    def matrix(self):
        c = self.counts
        return (c.cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)).astype(np.float64)

    def tp_fp(self):
        """metrics.py:995-1000: true and false positives per class, the background class removed."""
        m = self.matrix
        tp = m.diagonal()
        fp = m.sum(1) - tp
        return tp[:-1], fp[:-1]


class DetectionStats:
    """The detection validator's statistics (val.py:125-190, get_stats :192-201) and box Metric
    (metrics.py:1234-1360): update(preds, batch) per batch, results() at the end."""

    KEYS = ("tp", "conf", "pred_cls", "target_cls", "target_img")

    def __init__(self, nc=80):
        self.nc = nc
        self.stats = {k: [] for k in self.KEYS}
        self.seen = 0
        self._dev = None      # update_batched: device accumulators (confusion matrix, label tallies, thresholds)
        self._pending = []    # update_batched: per batch (det, counts, correct) on the device until results()
        self.confusion_matrix = None
        self.last_gt_xyxy = None

    def update(self, preds, batch_idx, cls, bboxes_xyxy):
        """preds: per image (n, 6) [x1, y1, x2, y2, conf, cls] device tensors (adr_nms output); labels: the batch's
        batch_idx (N,), cls (N,), xyxy boxes in input pixels (N, 4)."""
        T = len(IOUV)
        for si, pred in enumerate(preds):
            self.seen += 1
            sel = batch_idx == si
            tcls, tbox = cls[sel], bboxes_xyxy[sel]
            tcls_np = tcls.cpu().numpy()
            n = len(pred)
            if n == 0 and not len(tcls):
                continue  # an image with neither detections nor labels adds nothing (val.py:140-145)
            row = {"target_cls": tcls_np, "target_img": np.unique(tcls_np)}
            if n == 0:
                row.update(tp=np.zeros((0, T), dtype=bool), conf=np.zeros(0), pred_cls=np.zeros(0))
            else:
                row["conf"] = pred[:, 4].cpu().numpy()
                row["pred_cls"] = pred[:, 5].cpu().numpy()
                row["tp"] = (match_predictions(pred[:, 5], tcls, box_iou(tbox.to(pred.device), pred[:, :4]))
                             if len(tcls) else np.zeros((n, T), dtype=bool))
            for k in self.KEYS:
                self.stats[k].append(row[k])

    def update_batched(self, out, n, batch, imgsz=None, cm_conf=None, cm_iou=0.45, single_cls=False,
                       confusion=True):
        """One batch in one launch (adr_scale_boxes + adr_val_match), in native image space as the reference's
        validator (val.py:104-161), with NO host synchronisation: the statistics stay on the device until results().

        out (B, rows, 6), n (B,) int32: the padded NMS output in the network's input space, as
        FusedPredictor.run_padded returns it (it is copied; the caller's tensors are not changed). batch: the
        collated labels `cls`, `bboxes` (normalised xywh) and `batch_idx` — host tensors, so that the per-image
        offsets need no device read — and the per-image lists `ori_shape` [(h0, w0)] and `ratio_pad`
        [((ratio_h, ratio_w), (left, top))]; imgsz (H, W) defaults to batch['img'].shape[2:]. cm_conf None or 0.001
        means 0.25 (metrics.py:917). single_cls zeroes the detections' class column (val.py:149-150)."""
        dev = out.device
        if not out.is_cuda:
            raise RuntimeError("update_batched: device tensors required (HIP kernel, no CPU fallback)")
        B, rows = out.shape[0], out.shape[1]
        H, W = (int(v) for v in (imgsz if imgsz is not None else batch["img"].shape[2:]))
        T = len(IOUV)
        if self._dev is None:
            self._dev = {"cm": torch.zeros(self.nc + 1, self.nc + 1, dtype=torch.int32, device=dev),
                         "ntc": torch.zeros(self.nc, dtype=torch.int32, device=dev),
                         "nti": torch.zeros(self.nc, dtype=torch.int32, device=dev),
                         "thr": torch.tensor(np.asarray(IOUV, dtype=np.float32), device=dev)}
            self.confusion_matrix = ConfusionMatrix(self.nc, conf=cm_conf, iou_thres=cm_iou, counts=self._dev["cm"])
        cm = self.confusion_matrix
        # host side: labels sorted by image, CSR offsets, the scale table; one pinned staging buffer, async upload
        bi = torch.as_tensor(batch["batch_idx"]).reshape(-1).cpu().long()
        cls = torch.as_tensor(batch["cls"]).reshape(-1).cpu().float()
        box = torch.as_tensor(batch["bboxes"]).reshape(-1, 4).cpu().float()
        N = int(bi.numel())
        if N and bool((bi[1:] < bi[:-1]).any()):
            order = torch.argsort(bi, stable=True)
            bi, cls, box = bi[order], cls[order], box[order]
        if N and (int(bi.min()) < 0 or int(bi.max()) >= B):
            raise ValueError("update_batched: batch_idx outside the batch")
        off = np.zeros(B + 1, dtype=np.int32)
        np.cumsum(np.bincount(bi.numpy(), minlength=B), out=off[1:])
        rows_tab = [(rp[0][0], rp[1][0], rp[1][1], shp[1], shp[0])
                    for shp, rp in zip(batch["ori_shape"], batch["ratio_pad"])]
        if len(rows_tab) != B:
            raise ValueError(f"update_batched: {len(rows_tab)} ori_shape / ratio_pad entries for a batch of {B}")
        stage = torch.empty(5 * B + 5 * N, dtype=torch.float32).pin_memory()
        stage[:5 * B] = torch.tensor(rows_tab, dtype=torch.float32).reshape(-1)
        stage[5 * B:5 * B + N] = cls
        stage[5 * B + N:] = box.reshape(-1)
        off_t = torch.from_numpy(off).pin_memory()
        dstage = stage.to(dev, non_blocking=True)
        doff = off_t.to(dev, non_blocking=True)
        tab, dcls, dbox = dstage[:5 * B], dstage[5 * B:5 * B + N], dstage[5 * B + N:]
        det = out.detach().float().clone()
        cnt = n.detach().to(torch.int32).clone()
        if single_cls:
            det[..., 5] = 0
        gt = torch.empty(max(N, 1), 4, dtype=torch.float32, device=dev)
        correct = torch.empty(B, rows, T, dtype=torch.uint8, device=dev)
        st = K.stream()
        lib.adr_scale_boxes(K.fptr(det), K.fptr(cnt), K.fptr(tab), B, rows, 6, 0, st)
        lib.adr_val_match(K.fptr(det), K.fptr(cnt), B, rows, K.fptr(dcls), K.fptr(dbox), K.fptr(doff),
                          off.ctypes.data, N, K.fptr(tab), H, W, K.fptr(self._dev["thr"]), T, float(cm.conf),
                          float(cm.iou_thres), self.nc, K.fptr(gt), K.fptr(correct),
                          K.fptr(self._dev["cm"]) if confusion else None, K.fptr(self._dev["ntc"]),
                          K.fptr(self._dev["nti"]), st)
        self._pending.append((det, cnt, correct, cls.numpy().copy(), off, (stage, off_t)))
        self.last_gt_xyxy = gt[:N]
        self.seen += B

    def _flush_batched(self):
        """Move the pending batches' statistics to the host (the only synchronisation of the batched path) and file
        them per image under the same keys as update()."""
        if not self._pending:
            return
        counts = torch.cat([p[1] for p in self._pending]).cpu().numpy()
        if (counts < 0).any():
            raise RuntimeError("adr_nms reported a grid-barrier timeout for a validated batch; statistics invalid")
        T = len(IOUV)
        i0 = 0
        for det, cnt, correct, tcls, off, _ in self._pending:
            cc = det[..., 4:6].cpu().numpy()
            tp = correct.cpu().numpy().astype(bool)
            for b in range(det.shape[0]):
                k = int(min(counts[i0 + b], det.shape[1]))
                t = tcls[off[b]:off[b + 1]]
                if k == 0 and not len(t):
                    continue  # val.py:140-145
                row = {"target_cls": t, "target_img": np.unique(t), "tp": tp[b, :k].reshape(k, T),
                       "conf": cc[b, :k, 0], "pred_cls": cc[b, :k, 1]}
                for key in self.KEYS:
                    self.stats[key].append(row[key])
            i0 += det.shape[0]
        self._pending = []

    def results(self):
        self._flush_batched()
        s = {k: np.concatenate(v, 0) if v else np.zeros(0) for k, v in self.stats.items()}
        p = r = np.zeros(0)
        ap, idx = np.zeros((0, len(IOUV))), np.zeros(0, int)
        if len(s["tp"]) and s["tp"].any():
            _, _, p, r, _, ap, idx, *_ = ap_per_class(s["tp"], s["conf"], s["pred_cls"], s["target_cls"])
        mean = [float(v.mean()) if len(v) else 0.0 for v in (p, r, ap[:, 0] if len(ap) else ap, ap)]
        fitness = 0.9 * mean[2] + 0.1 * mean[3]  # Metric.fitness weights (0, 0, 0.9, 0.1)
        res = {"p": p, "r": r, "ap": ap, "ap_class_index": idx, "metrics/precision(B)": mean[0],
               "metrics/recall(B)": mean[1], "metrics/mAP50(B)": mean[2], "metrics/mAP50-95(B)": mean[3],
               "fitness": fitness}
        if self._dev is not None:  # the batched path ran: the validator's tallies (val.py:182-183) and matrix
            res.update(nt_per_class=self._dev["ntc"].cpu().numpy().astype(np.int64),
                       nt_per_image=self._dev["nti"].cpu().numpy().astype(np.int64), seen=self.seen,
                       confusion_matrix=self.confusion_matrix)
        return res
