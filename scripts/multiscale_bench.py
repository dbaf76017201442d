"""Measure multi-scale training (FusedTrainer(multi_scale=True); no speed is promised, the feature has no predecessor).

  python scripts/multiscale_bench.py [--out profiles/multiscale.json]      (run it under `timeout`)

701-n, bf16, batch 64, imgsz 640 — the benchmark's workload — at the three sizes that bound the draw: the smallest
(320), imgsz itself (640, the 1:1 draw: the uint8 batch, no resample) and the largest (960). Per size:

1. the step: eager ms/step, the time capture(batch, size=...) takes (host clock, the call ends in a device
   synchronise), and replay ms/step of the captured graphs. Steps are timed with HIP events around STEPS steps after
   WARM warm-up steps of that shape; the draws come from a fixed source, so every timed step has the shape named.
2. the resample alone: adr_multiscale_u8 into a resident output against torch's own
   F.interpolate(img.float() / 255, bilinear) on the device, alternating, HIP events per call; the kernel's GB/s over
   (source bytes + 4 * output elements) as a fraction of the 8 TB/s HBM peak (it is bound by the stores), and the
   largest difference between the two results.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "yolo-ad-refine_amd"))
sys.path.insert(0, str(ROOT / "oracle"))

B, IMGSZ, STRIDE = 64, 640, 32
WARM, STEPS = 5, 50  # a timed window of 0.5-2 s per figure
HBM_PEAK = 8.0e12


class Fixed:
    """A `random`-like source whose every randrange is `value` (multi_scale_shape rounds it down to the stride)."""

    def __init__(self):
        self.value = IMGSZ

    def randrange(self, a, b):
        assert a <= self.value < b, (a, self.value, b)
        return self.value


def steps_ms(tr, batch, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        tr.step(batch)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def calls_ms(fns, warm=5, reps=200):
    """Median / min / max ms of each fn, the fns alternating call by call."""
    for _ in range(warm):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [{"median_ms": statistics.median(m), "min_ms": min(m), "max_ms": max(m), "reps": reps} for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "multiscale.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "multiscale_bench.py measures on the GPU"
    from adrefine import kernels as K
    from adrefine.engine.trainer import FusedTrainer
    from adrefine.native import lib
    from adrefine.nn.tasks import DetectionModel
    from recipe import recipe_state_dict, synthetic_labels

    sizes = [IMGSZ // 2 // STRIDE * STRIDE, IMGSZ, int(IMGSZ * 1.5) // STRIDE * STRIDE]
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (B, 3, IMGSZ, IMGSZ), generator=g, dtype=torch.uint8).cuda()
    batch = {"img": img, **synthetic_labels(B, 80, seed=1)}
    res = {"device": torch.cuda.get_device_name(0), "model": "yolo11-701-YOLO-AD-Refine n, bf16", "batch": B,
           "imgsz": IMGSZ, "sizes": sizes, "warmup_steps": WARM, "timed_steps": STEPS, "step": {}, "resample": {}}

    # the resample alone, against torch on the device
    for s in sizes:
        if s == IMGSZ:
            continue
        out = torch.empty(B, 3, s, s, dtype=torch.float32, device="cuda")
        ref = [None]

        def kernel():
            lib.adr_multiscale_u8(K.fptr(img), B, IMGSZ, IMGSZ, K.fptr(out), s, s, K.stream())

        def torch_ops():
            ref[0] = F.interpolate(img.float() / 255, size=(s, s), mode="bilinear", align_corners=False)

        k, t = calls_ms([kernel, torch_ops])
        nbytes = B * 3 * (IMGSZ * IMGSZ + 4 * s * s)
        gbs = nbytes / (k["median_ms"] * 1e-3) / 1e9
        k.update(bytes=nbytes, GBps=gbs, fraction_of_8TBps=gbs * 1e9 / HBM_PEAK)
        res["resample"][str(s)] = {"adr_multiscale_u8": k, "torch_float_div_interpolate": t,
                                   "speedup": t["median_ms"] / k["median_ms"],
                                   "max_abs_diff": float((out - ref[0]).abs().max())}
        del out, ref

    m = DetectionModel(str(ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"),
                       compute_dtype=torch.bfloat16)
    m.load_state_dict(recipe_state_dict([(k, v.shape) for k, v in m.state_dict().items()]), strict=True)
    rng = Fixed()
    tr = FusedTrainer(m.cuda(), nbs=B, batch_size=B, multi_scale=True, imgsz=IMGSZ, rng=rng, graph_shapes=1)
    for s in sizes:
        rng.value = s
        for _ in range(WARM):
            tr.step(batch)
        eager = steps_ms(tr, batch, STEPS)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.capture(batch, size=(s, s))
        capture_s = time.perf_counter() - t0
        assert tr._key[0] == (B, 3, s, s) and not tr._other
        for _ in range(WARM):
            tr.step(batch)
        replay = steps_ms(tr, batch, STEPS)
        res["step"][str(s)] = {"eager_ms_per_step": eager, "replay_ms_per_step": replay,
                               "eager_over_replay": eager / replay, "capture_s": capture_s,
                               "input": "uint8, no resample" if s == IMGSZ else "adr_multiscale_u8 fp32"}
    res["peak_hbm_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
