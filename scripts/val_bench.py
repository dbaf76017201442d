"""Measure the validator's per-batch bookkeeping after NMS (no ratio is promised; the one requirement is that the
batched path is not slower than the per-image path it replaces, in the same run on the same device).

  python scripts/val_bench.py [--out profiles/val_bench.json]      (run it under `timeout`)

Input: data/synthetic.head_output at batch 32, 8400 anchors, 80 classes -> adr_nms at the validator's settings (conf
0.001, IoU 0.7, multi-label, 300 per image), about 10 labels per image. Timed per batch, medians of `reps` runs after
warm-up, each as host wall clock around call + stream synchronise (the per-image path synchronises inside, so wall
clock is the comparable figure) and as HIP-event time on the stream:
  (i)   per_image_update   DetectionStats.update on the list of per-image detections (one adr_box_iou + one
                           adr_match_predictions launch and several host reads per image), counts read first
  (ii)  update_batched     adr_scale_boxes + adr_val_match + the host staging of one batch, no host read
  (iii) val_match_kernel   adr_val_match alone, inputs resident
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "yolo-ad-refine_amd"))

B, NA, NC, S = 32, 8400, 80, 640


def timed(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    ev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(e0.elapsed_time(e1))
    return {"wall_median_ms": statistics.median(wall), "wall_min_ms": min(wall), "wall_max_ms": max(wall),
            "event_median_ms": statistics.median(ev), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "val_bench.json"))
    args = ap.parse_args()
    from adrefine import kernels as K
    from adrefine.data.synthetic import head_output, labels
    from adrefine.native import lib
    from adrefine.utils.metrics import IOUV, DetectionStats
    from adrefine.utils.ops import non_max_suppression_padded

    y = head_output(B, NA, NC, S).cuda()
    out, n = non_max_suppression_padded(y, 0.001, 0.7, multi_label=True, max_det=300)
    lab = labels(B, NC, seed=3, mean_n=10.0)
    cls, box, bi = lab["cls"].reshape(-1), lab["bboxes"], lab["batch_idx"]
    xyxy = torch.cat([box[:, :2] - box[:, 2:] / 2, box[:, :2] + box[:, 2:] / 2], 1) * S
    batch = {"cls": cls, "bboxes": box, "batch_idx": bi, "ori_shape": [(S, S)] * B,
             "ratio_pad": [((1.0, 1.0), (0, 0))] * B}
    counts = n.tolist()
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "anchors": NA, "nc": NC, "labels": int(len(cls)),
           "detections": int(sum(counts))}

    def per_image():
        k = n.tolist()
        preds = [out[i, :k[i]] for i in range(B)]
        DetectionStats(NC).update(preds, bi, cls, xyxy)

    st = DetectionStats(NC)

    def batched():
        st.update_batched(out, n, batch, imgsz=(S, S))
        st._pending.clear()  # keep the timed loop from accumulating device buffers

    res["per_image_update"] = timed(per_image)
    res["update_batched"] = timed(batched)

    # the kernel alone, inputs resident
    N = len(cls)
    off = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(np.bincount(bi.numpy().astype(int), minlength=B), out=off[1:])
    det = out.clone()
    tab = torch.tensor([[1.0, 0, 0, S, S]] * B, dtype=torch.float32).cuda()
    d = {"cls": cls.cuda(), "box": box.cuda().contiguous(), "off": torch.from_numpy(off).cuda(),
         "thr": torch.tensor(np.asarray(IOUV, dtype=np.float32)).cuda(),
         "gt": torch.empty(N, 4, device="cuda"), "correct": torch.empty(B, 300, 10, dtype=torch.uint8, device="cuda"),
         "cm": torch.zeros(NC + 1, NC + 1, dtype=torch.int32, device="cuda"),
         "ntc": torch.zeros(NC, dtype=torch.int32, device="cuda"),
         "nti": torch.zeros(NC, dtype=torch.int32, device="cuda")}
    res["val_match_kernel"] = timed(lambda: lib.adr_val_match(
        K.fptr(det), K.fptr(n), B, 300, K.fptr(d["cls"]), K.fptr(d["box"]), K.fptr(d["off"]), off.ctypes.data, N,
        K.fptr(tab), S, S, K.fptr(d["thr"]), 10, 0.25, 0.45, NC, K.fptr(d["gt"]), K.fptr(d["correct"]),
        K.fptr(d["cm"]), K.fptr(d["ntc"]), K.fptr(d["nti"]), K.stream()))
    res["ratio_per_image_over_batched_wall"] = (res["per_image_update"]["wall_median_ms"] /
                                                res["update_batched"]["wall_median_ms"])
    res["batched_not_slower"] = bool(res["update_batched"]["wall_median_ms"] <=
                                     res["per_image_update"]["wall_median_ms"])
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
