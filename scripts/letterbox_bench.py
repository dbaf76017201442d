"""Measure the LetterBox path (no speed is promised; the feature has no predecessor to compare with).

  python scripts/letterbox_bench.py [--out profiles/letterbox_bench.json]      (run it under `timeout`)

1. render_letterbox of 32 synthetic 1920x1080 BGR sources -> 640x640: HIP-event time of the whole call (host tables
   + pool / descriptor / table upload + kernel) and of the kernel alone (inputs already on the device), and the
   kernel's GB/s over (source bytes + 3*H*W written per image) as a fraction of the 8 TB/s HBM peak.
2. FusedPredictor (701-n, bf16, batch 32, 640x640, one hipGraph): predict_images on the 32 raw sources against
   predict on the pre-letterboxed uint8 batch.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "yolo-ad-refine_amd"))
sys.path.insert(0, str(ROOT / "oracle"))

B, SH, SW, S = 32, 1080, 1920, 640
HBM_PEAK = 8.0e12


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "letterbox_bench.json"))
    args = ap.parse_args()
    from adrefine.data import augment as A
    from adrefine.engine.predictor import FusedPredictor
    from adrefine.kernels import stream
    from adrefine.native import lib
    from adrefine.nn.tasks import DetectionModel
    from recipe import recipe_state_dict

    rs = np.random.RandomState(0)
    imgs = [rs.randint(0, 256, (SH, SW, 3), dtype=np.uint8) for _ in range(B)]
    out = torch.empty(B, 3, S, S, dtype=torch.uint8, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "source": [SH, SW], "imgsz": S}
    res["render_with_upload"] = timed(lambda: A.render_letterbox(imgs, (S, S), out=out))

    # the kernel alone: the same launch with its inputs resident
    A.render_letterbox(imgs, (S, S), out=out)
    pool, dd, tb = out._adr_keep
    lbx = A.LetterBox((S, S))
    descs = (A.LetterboxDesc * B)()
    ntab = 0
    for b, im in enumerate(imgs):
        nw, nh, left, top = lbx(image=im).resize
        d = descs[b]
        d.off, d.sw, d.sh, d.nw, d.nh, d.left, d.top, d.mode, d.tab_off, d.rgb = (
            b * im.size, SW, SH, nw, nh, left, top, A.LB_LINEAR, ntab, 1)
        ntab += 3 * (nw + nh)
    assert bytes(descs) == bytes(dd.cpu().numpy()) and ntab == tb.numel()
    ref = out.clone()
    res["kernel"] = timed(lambda: lib.adr_letterbox_u8(
        ctypes.c_void_p(pool.data_ptr()), pool.numel(), ctypes.c_void_p(dd.data_ptr()),
        ctypes.cast(descs, ctypes.c_void_p), B, ctypes.c_void_p(tb.data_ptr()), ntab, ctypes.c_void_p(out.data_ptr()),
        S, S, stream()), reps=20)
    assert torch.equal(out, ref)
    nbytes = B * (SH * SW * 3 + 3 * S * S)
    gbs = nbytes / (res["kernel"]["median_ms"] * 1e-3) / 1e9
    res["kernel"].update(bytes=nbytes, GBps=gbs, fraction_of_8TBps=gbs * 1e9 / HBM_PEAK,
                         note="bytes = every source byte once + 3*H*W written; a 3x downscale's taps touch about "
                              "4/9 of the source pixels, so the traffic the kernel needs is lower than this count")

    m = DetectionModel(str(ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"),
                       compute_dtype=torch.bfloat16)
    m.load_state_dict(recipe_state_dict([(k, v.shape) for k, v in m.state_dict().items()]), strict=True)
    m = m.cuda().eval()
    p = FusedPredictor(m)
    pre = ref.clone()
    p.capture(pre)
    res["predict_preletterboxed"] = timed(lambda: p.predict(pre))
    res["predict_images"] = timed(lambda: p.predict_images(imgs))
    for k in ("predict_preletterboxed", "predict_images"):
        res[k]["images_per_s"] = B / (res[k]["median_ms"] * 1e-3)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
