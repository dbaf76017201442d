"""Optimizer-tail timing: the captured optimizer graph (g_opt: gradient norm + clip + update + EMA + zero_grad) and
the whole captured training step of YOLO-AD-Refine-n at bs 64 / 640^2 (bf16 compute, synthetic uint8 batch, as
bench.py's flagship run), for SGD and for AdamW. HIP events around single replays, medians after warm-up replays.

    python scripts/opt_bench.py --label this-tree --commit <sha> --out profiles/opt_bench.json

Runs on any tree that has FusedTrainer: one without the `optimizer` argument (the parent of the Adam change) is
measured for SGD only, so the same script gives the parent's SGD tail for comparison. Results are merged into
--out under --label. Needs a GPU; there is no CPU fallback."""
from __future__ import annotations

import argparse
import inspect
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT / "yolo-ad-refine_amd"), str(ROOT / "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
CFG = ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"


def _events(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)  # us
    ts.sort()
    return {"median_us": round(statistics.median(ts), 2), "p10_us": round(ts[len(ts) // 10], 2),
            "p90_us": round(ts[(9 * len(ts)) // 10], 2), "reps": reps, "warmup": warmup}


def measure(name, bs, img, reps, warmup):
    import torch

    from adrefine.data.synthetic import train_batch
    from adrefine.engine.trainer import FusedTrainer
    from adrefine.nn.tasks import DetectionModel
    torch.manual_seed(0)
    model = DetectionModel(str(CFG), compute_dtype=torch.bfloat16).cuda()
    kw = {} if name == "SGD" else {"optimizer": name, "lr0": 0.000119, "momentum": 0.9}
    tr = FusedTrainer(model, batch_size=bs, world_size=1, **kw)
    batch, _ = train_batch(bs, img, seed=0, device=torch.device("cuda"), u8=True)
    for _ in range(3):
        tr.step(batch)
    tr.capture(batch)
    tr.step(batch)
    torch.cuda.synchronize()
    g_opt = tr.graphs[1]
    # the tail alone: replaying it on a zeroed arena is the same memory traffic (every stream is read and written
    # whatever the gradient values); the hyper vector stays at the last step's values
    tail = _events(g_opt.replay, reps, warmup)
    step = _events(lambda: tr.step(batch), max(reps // 5, 20), max(warmup // 5, 5))
    nupd = sum(t.numel() for _, t, _, isp in tr.entries if isp and getattr(t, "_adr_used", False))
    ntot = sum(t.numel() for _, t, _, _ in tr.entries)
    streams = 10 if name != "SGD" else 8
    return {"tail": tail, "step": step, "nchunks": tr.nchunks, "updated_elements": nupd, "ema_elements": ntot,
            # algorithmic bytes of the update kernel: p, g, moment(s), ema read and written for updated entries,
            # p read and ema read + written for EMA-only ones; plus the norm pass's read of g
            "alg_bytes": 4 * (streams * nupd + 3 * (ntot - nupd) + nupd)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True)
    ap.add_argument("--commit", default=None, help="commit the measured tree was built from")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "opt_bench.json"))
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--img", type=int, default=640)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "opt_bench.py needs a GPU"
    from adrefine.engine.trainer import FusedTrainer
    names = ["SGD"] + (["AdamW"] if "optimizer" in inspect.signature(FusedTrainer.__init__).parameters else [])
    res = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "bs": args.bs, "img": args.img,
           "dtype": "bf16", "timer": "HIP events around one replay / one captured step, median"}
    for name in names:
        res[name] = measure(name, args.bs, args.img, args.reps, args.warmup)
        print(name, json.dumps(res[name]), flush=True)
    if "AdamW" in res:
        res["adamw_over_sgd_tail"] = round(res["AdamW"]["tail"]["median_us"] / res["SGD"]["tail"]["median_us"], 3)
        res["adamw_over_sgd_step"] = round(res["AdamW"]["step"]["median_us"] / res["SGD"]["step"]["median_us"], 4)
    out = Path(args.out)
    doc = json.loads(out.read_text()) if out.exists() else {}
    doc.setdefault("runs", {}).setdefault(args.label, []).append(res)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
