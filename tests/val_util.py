"""Numpy restatement of adr_val_match (csrc/adr_val.hip), stages a to d, in the reference's fp32 arithmetic and order
(models/yolo/detect/val.py:104-161, engine/validator.py:221-261, utils/metrics.py:52-72 and :932-989). The fixtures
of tests/golden/val_batched.npz, which the reference's own validator produced (scripts/gen_val_golden.py), pin it;
the GPU tests compare the kernel against both."""
import numpy as np

F = np.float32
IOUV = np.linspace(0.5, 0.95, 10)


def table_row(ori_shape, ratio_pad):
    """adr_scale_boxes' row {gain, padx, pady, w0, h0} of one image (ops.py:112-114 with ratio_pad given)."""
    return [ratio_pad[0][0], ratio_pad[1][0], ratio_pad[1][1], ori_shape[1], ori_shape[0]]


def scale_clip(xyxy, row):
    """(v - pad) / gain in fp32, clipped to the source image (ops.py:116-123, 315-334)."""
    gain, px, py, w0, h0 = (F(v) for v in row)
    out = np.asarray(xyxy, dtype=F).copy()
    pad = np.array([px, py, px, py], dtype=F)
    hi = np.array([w0, h0, w0, h0], dtype=F)
    out[:, :4] = np.minimum(np.maximum((out[:, :4] - pad) / gain, F(0)), hi)
    return out


def labels_native(bboxes, imgsz, row):
    """Stage a: normalised xywh -> xyxy -> * (W, H, W, H) -> scale_boxes (val.py:113-114)."""
    b = np.asarray(bboxes, dtype=F).reshape(-1, 4)
    H, W = imgsz
    half = b[:, 2:] / F(2)
    xyxy = np.concatenate([b[:, :2] - half, b[:, :2] + half], 1) * np.array([W, H, W, H], dtype=F)
    return scale_clip(xyxy, row)


def box_iou(a, b, eps=1e-7):
    """(G, 4) x (P, 4) -> (G, P), utils/metrics.py:52-72 in fp32."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    wh = np.maximum(np.minimum(a[:, None, 2:], b[None, :, 2:]) - np.maximum(a[:, None, :2], b[None, :, :2]), F(0))
    inter = wh[..., 0] * wh[..., 1]
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (area_a[:, None] + area_b[None, :] - inter + F(eps))


def thresholds(iouv=IOUV):
    return np.asarray(iouv, dtype=F)


def match_tp(iou, gt_cls, det_cls, thr):
    """Stage b: each detection's best same-class label (ties: larger label index); at thr[t] the label goes to the
    lowest-index detection whose best it is with IoU >= thr[t]."""
    G, P = iou.shape
    out = np.zeros((P, len(thr)), dtype=bool)
    if G == 0 or P == 0:
        return out
    masked = np.where(np.asarray(gt_cls)[:, None] == np.asarray(det_cls)[None, :], iou, F(0))
    bg = G - 1 - np.argmax(masked[::-1], axis=0)  # the last maximum
    bv = masked[bg, np.arange(P)]
    for t, th in enumerate(thr):
        taken = set()
        for p in range(P):
            if bv[p] >= th and bg[p] not in taken:
                out[p, t] = True
                taken.add(bg[p])
    return out


def cm_candidates(iou, conf, cm_conf, cm_iou):
    """IoUs of the confusion matrix's candidate pairs of one image (kept detections, iou > cm_iou)."""
    keep = np.asarray(conf, dtype=F) > F(cm_conf)
    sub = iou[:, keep]
    return sub[sub > F(cm_iou)]


def cm_update(cm, iou, conf, det_cls, gt_cls, nc, cm_conf=0.25, cm_iou=0.45):
    """Stage c on one image with labels (an image without labels adds nothing; without detections iou is (G, 0))."""
    G, P = iou.shape
    if G == 0:
        return
    clamp = lambda c: min(max(int(c), 0), nc)  # noqa: E731
    best_g = np.full(P, -1)
    best_v = np.zeros(P, dtype=F)
    kept = np.asarray(conf, dtype=F) > F(cm_conf) if P else np.zeros(0, bool)
    for p in range(P):
        if not kept[p]:
            continue
        for g in range(G):
            if iou[g, p] > F(cm_iou) and iou[g, p] >= best_v[p]:  # ties: the larger label index
                best_v[p], best_g[p] = iou[g, p], g
    winner = {}
    for p in range(P):  # ties: the lower detection index
        g = best_g[p]
        if g >= 0 and (g not in winner or best_v[p] > best_v[winner[g]]):
            winner[g] = p
    for g in range(G):
        if g in winner:
            cm[clamp(det_cls[winner[g]]), clamp(gt_cls[g])] += 1
        else:
            cm[nc, clamp(gt_cls[g])] += 1
    if winner:
        won = set(winner.values())
        for p in range(P):
            if kept[p] and p not in won:
                cm[clamp(det_cls[p]), nc] += 1


def run_batch(det, counts, cls, bboxes, batch_idx, rows_tab, imgsz, nc, thr=None, cm_conf=0.25, cm_iou=0.45,
              det_native=False, single_cls=False):
    """All four stages on one batch. det (B, rows, 6) padded, in letterbox space unless det_native. Returns a dict:
    gt_xyxy (N, 4), correct (B, rows, T) uint8, cm, nt_per_class, nt_per_image (this batch's contribution), and the
    per-image native detections."""
    thr = thresholds() if thr is None else thr
    det = np.asarray(det, dtype=F)
    B, rows = det.shape[:2]
    cls = np.asarray(cls, dtype=F).reshape(-1)
    bboxes = np.asarray(bboxes, dtype=F).reshape(-1, 4)
    batch_idx = np.asarray(batch_idx).reshape(-1)
    out = {"gt_xyxy": np.zeros((len(cls), 4), dtype=F), "correct": np.zeros((B, rows, len(thr)), dtype=np.uint8),
           "cm": np.zeros((nc + 1, nc + 1), dtype=np.int64), "nt_per_class": np.zeros(nc, dtype=np.int64),
           "nt_per_image": np.zeros(nc, dtype=np.int64), "predn": []}
    for b in range(B):
        sel = np.nonzero(batch_idx == b)[0]
        gt = labels_native(bboxes[sel], imgsz, rows_tab[b])
        out["gt_xyxy"][sel] = gt
        n = int(counts[b])
        d = det[b, :n].copy()
        if single_cls:
            d[:, 5] = 0
        if not det_native:
            d = scale_clip(d, rows_tab[b])
        out["predn"].append(d)
        gc = cls[sel]
        ci = gc.astype(np.int64)
        ci = ci[(ci >= 0) & (ci < nc)]
        out["nt_per_class"] += np.bincount(ci, minlength=nc)
        out["nt_per_image"] += np.bincount(np.unique(ci), minlength=nc)
        iou = box_iou(gt, d[:, :4])
        out["correct"][b, :n] = match_tp(iou, gc, d[:, 5], thr)
        cm_update(out["cm"], iou, d[:, 4], d[:, 5], gc, nc, cm_conf, cm_iou)
    return out


def fixture_batches(g, run):
    """The batches of one run ('mc' or 'sc') of tests/golden/val_batched.npz as dicts, with the per-image lists
    ori_shape [(h0, w0)] and ratio_pad [((ratio_h, ratio_w), (left, top))] the way collate_fn delivers them."""
    out = []
    for bi in range(int(g[f"{run}_nbatches"])):
        b = {k: g[f"{run}_{bi}_{k}"] for k in ("det", "counts", "cls", "bboxes", "batch_idx", "gt_xyxy")}
        b["ori_shape"] = [tuple(int(v) for v in o) for o in g[f"{run}_{bi}_ori_shape"]]
        b["ratio_pad"] = [((float(r[0]), float(r[1])), (float(r[2]), float(r[3]))) for r in g[f"{run}_{bi}_ratio_pad"]]
        b["table"] = [table_row(o, r) for o, r in zip(b["ori_shape"], b["ratio_pad"])]
        out.append(b)
    return out


def stats_rows(correct, counts, n_labels):
    """tp rows in the validator's order: images with neither detections nor labels add nothing (val.py:140-145)."""
    rows = [correct[i, :int(n)].astype(bool) for i, n in enumerate(counts) if int(n) or n_labels[i]]
    return np.concatenate(rows, 0) if rows else np.zeros((0, correct.shape[2]), dtype=bool)
