"""Measure adr_nms on both sides of 16 384 predictions per image: non_max_suppression_padded on seeded synthetic head
outputs (oracle/recipe.py synthetic_predictions), HIP events around each call, 20 calls after 5 warm-ups. No number is
promised for the large rows (the path above 16 384 is plain launches with a sort that spills to global memory; it is
recorded, not tuned); the one requirement is that the 8 400-prediction row, the persistent single-launch kernel, does
not move when the large path changes.

  python scripts/nms_bench.py [--out profiles/nms_large.json] [--rows small,large_nc1,large_nc80]   (run it under `timeout`)

A library without the large path (ADR_LIB=... selects another build) raises on the large rows; the row then records
the error instead of a time."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "yolo-ad-refine_amd"))
sys.path.insert(0, str(ROOT / "oracle"))

ROWS = {
    # name: (B, A, nc, img, conf, multi_label)
    "small": (32, 8400, 80, 640, 0.25, False),
    "large_nc1": (16, 33600, 1, 1280, 0.001, True),
    "large_nc80": (16, 33600, 80, 1280, 0.25, False),
}
WARM, REPS, IOU = 5, 20, 0.7


def timed(fn):
    ev = []
    for k in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= WARM:
            ev.append(e0.elapsed_time(e1))
    return {"event_median_ms": statistics.median(ev), "event_min_ms": min(ev), "event_max_ms": max(ev), "reps": len(ev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "nms_large.json"))
    ap.add_argument("--rows", default=",".join(ROWS))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "nms_bench needs the GPU"
    from recipe import synthetic_predictions

    from adrefine.native import lib
    from adrefine.utils.ops import non_max_suppression_padded

    res = {"device": torch.cuda.get_device_name(0), "warmup": WARM, "iou": IOU, "rows": {}}
    for name in args.rows.split(","):
        B, A, nc, img, conf, multi = ROWS[name]
        row = {"B": B, "A": A, "nc": nc, "conf": conf, "multi_label": multi,
               "workspace_bytes": int(lib.adr_nms_workspace(B, nc, A, int(multi and nc > 1), 300))}
        pred = synthetic_predictions(B, A, nc, img, seed=A + nc).cuda()
        try:
            out, n = non_max_suppression_padded(pred, conf, IOU, multi_label=multi)
            counts = n.tolist()
            assert min(counts) >= 0, "grid barrier timed out"
            row["detections"] = sum(counts)
            row.update(timed(lambda: non_max_suppression_padded(pred, conf, IOU, multi_label=multi)))
            row["images_per_s"] = B / (row["event_median_ms"] * 1e-3)
        except RuntimeError as e:
            row["error"] = str(e).splitlines()[0][:200]
        res["rows"][name] = row
        del pred
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
