"""Measure the dataset path: adr_resize_u8, the construction of a device-resident dataset, the per-batch render from
resident sources against the same plans rendered from host numpy sources (the path before the pool), and the loader's
throughput beside a training step. No number is promised; the one requirement is (c): the resident path is not slower
than the host-source path of the same run on the same device.

  python scripts/dataset_bench.py [--out profiles/dataset_bench.json] [--n 512] [--mixup P] [--perspective P]
  (run it under `timeout`)

--mixup P (default 0: the rows as they have always been measured) sets hyp.mixup: a sample is then mixed with
probability P (two layers, adr_augment_mix_u8). With P > 0 the result does not replace the file: it is stored in it
under the key "mixup_P", next to the existing rows. --perspective P (default 0) sets hyp.perspective: every image is
then warped by cv2.warpPerspective's arithmetic (AugDesc.warp == 2) instead of warpAffine's tables; the result is stored
under the key "perspective_P" in the same way (with both, under "mixup_P_perspective_P").

Input: a synthetic directory of --n PNGs around 1280 x 720 (five sizes) with 1-8 labels each, written to a temporary
directory; imgsz 640, batch 64, the default hyp. Medians of 20 batches after 3 warm-ups, HIP events and host wall
clock around call + synchronise, as scripts/val_bench.py."""
from __future__ import annotations

import argparse
import copy
import json
import random
import statistics
import sys
import tempfile
import time
import warnings
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "yolo-ad-refine_amd"))
sys.path.insert(0, str(ROOT / "oracle"))

IMGSZ, BS = 640, 64
SIZES = [(1280, 720), (1280, 853), (960, 1280), (1024, 768), (1280, 960)]  # (w, h)
HBM_PEAK = 8.0e12


def write_dataset(root, n):
    from PIL import Image
    (root / "images").mkdir(parents=True)
    (root / "labels").mkdir()
    rs = np.random.RandomState(0)
    for i in range(n):
        w, h = SIZES[i % len(SIZES)]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        ph = rs.uniform(0, 6, 3).astype(np.float32)
        img = 127.5 + 80 * np.sin(xx[..., None] * 0.02 + yy[..., None] * 0.013 + ph) + rs.uniform(-8, 8, (h, w, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(root / "images" / f"{i:05d}.png", compress_level=1)
        k = rs.randint(1, 9)
        ctr = 0.1 + 0.8 * rs.uniform(size=(k, 2))
        wh = np.minimum(0.05 + 0.45 * rs.uniform(size=(k, 2)), 2 * np.minimum(ctr, 1 - ctr))
        rows = np.concatenate([rs.randint(0, 80, (k, 1)), ctr, wh], 1)
        (root / "labels" / f"{i:05d}.txt").write_text("".join("%d %.6f %.6f %.6f %.6f\n" % tuple(r) for r in rows))
    return str(root / "images")


def timed(fns, warm=3):
    """fns: one callable per batch; the first `warm` are warm-up."""
    ev, wall = [], []
    for k, fn in enumerate(fns):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= warm:
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
    return {"wall_median_ms": statistics.median(wall), "wall_min_ms": min(wall), "wall_max_ms": max(wall),
            "event_median_ms": statistics.median(ev), "reps": len(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dataset_bench.json"))
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--no-train", action="store_true", help="skip (d)")
    ap.add_argument("--mixup", type=float, default=0.0, help="hyp.mixup; > 0: stored under the key mixup_P")
    ap.add_argument("--perspective", type=float, default=0.0,
                    help="hyp.perspective; > 0: stored under the key perspective_P")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dataset_bench needs the GPU"
    from recipe import AUG_HYPS

    from adrefine.data.augment import render
    from adrefine.data.build import build_dataloader
    from adrefine.data.dataset import YOLODataset, load_bgr
    from adrefine.data.pool import DevicePool

    hyp = lambda: SimpleNamespace(**dict(AUG_HYPS["default"], mixup=args.mixup,  # noqa: E731
                                         perspective=args.perspective), mask_ratio=4, overlap_mask=True)
    res = {"imgsz": IMGSZ, "batch": BS, "images": args.n, "device": torch.cuda.get_device_name(0)}
    if args.mixup > 0:
        res["mixup"] = args.mixup
    if args.perspective > 0:
        res["perspective"] = args.perspective
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        tree = write_dataset(Path(tmp) / "syn", args.n)
        res["write_png_s"] = time.perf_counter() - t0
        data = {"names": {i: str(i) for i in range(80)}}

        def make(**kw):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return YOLODataset(tree, imgsz=IMGSZ, hyp=hyp(), data=data, batch_size=BS, **kw)

        # (b) construction of cache="gpu": label scan, then decode / copy + kernel
        t0 = time.perf_counter()
        ds = make(cache=None, augment=True)  # writes the label cache; its pool is small
        res["label_scan_s"] = time.perf_counter() - t0
        del ds
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds = make(cache="gpu", augment=True, pool=None)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        # the same work, split: decode alone, then the copy + launch rounds of already decoded images
        pool = DevicePool("cuda", ds._resident_bytes())
        for i in range(ds.ni):
            h, w = ds.resized_hw(i)
            pool.queue(pool.image(h, w), lambda f=ds.im_files[i]: load_bgr(f), ds.source_hw(i))
        t0 = time.perf_counter()
        pool.prepare()
        decode = time.perf_counter() - t0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        pool.flush()
        e1.record()
        torch.cuda.synchronize()
        res["construct_cache_gpu"] = {"total_s": total, "decode_s": decode, "pack_copy_kernel_wall_s":
                                      time.perf_counter() - t0, "copy_kernel_event_ms": e0.elapsed_time(e1),
                                      "rounds": pool.rounds, "resident_bytes": ds._resident_bytes()}
        # (a) adr_resize_u8 alone: one batch's 256 sources, staged on the device
        srcs = [load_bgr(ds.im_files[i]) for i in range(min(256, ds.ni))]
        p2 = DevicePool("cuda", sum((s.size + 255) // 256 * 256 for s in srcs), staging_bytes=4 << 30)

        def one_resize():
            ims = []
            for i, s in enumerate(srcs):
                h, w = ds.resized_hw(i)
                im = p2.image(h, w)
                p2.queue(im, lambda s=s: s, s.shape[:2])
                ims.append(im)
            p2.prepare()
            return ims

        ker = []
        # one flush stages the sources; the launch it made is then repeated on the staged bytes (same arguments)
        from adrefine import native
        calls = []
        native.CALL_HOOK = lambda name, fn, a: calls.append((fn, a)) or fn(*a)
        ims = one_resize()
        p2.flush()
        native.CALL_HOOK = None
        torch.cuda.synchronize()
        fn, a = calls[-1]
        moved = sum(s.size for s in srcs) + sum(im.size for im in ims)
        for k in range(23):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert fn(*a) == 0
            e1.record()
            torch.cuda.synchronize()
            if k >= 3:
                ker.append(e0.elapsed_time(e1))
        ms = statistics.median(ker)
        res["resize_kernel"] = {"sources": len(srcs), "event_median_ms": ms, "bytes_read_plus_written": moved,
                                "bytes_per_s": moved / (ms * 1e-3), "fraction_of_8TBps": moved / (ms * 1e-3) / HBM_PEAK}
        # (c) the same plans from resident and from host sources
        host = {id(ds.ims[i]): ds.ims[i].numpy().copy() for i in range(ds.ni)}
        random.seed(0)
        np.random.seed(0)
        plans = [[ds[random.randrange(ds.ni)]["img"] for _ in range(BS)] for _ in range(23)]

        def on_host(ps):
            out = []
            for p in ps:
                q = copy.copy(p)
                q.tiles = [(host[id(t[0])],) + tuple(t[1:]) for t in p.tiles]
                if p.mix is not None:
                    q.mix = (on_host([p.mix[0]])[0],) + p.mix[1:]
                out.append(q)
            return out

        hplans = [on_host(ps) for ps in plans]
        same = torch.equal(render(plans[0]), render(hplans[0], "cuda"))
        r_dev = timed([lambda ps=ps: render(ps) for ps in plans])
        r_host = timed([lambda ps=ps: render(ps, "cuda") for ps in hplans])
        r_dev2 = timed([lambda ps=ps: render(ps) for ps in plans])
        if args.perspective > 0:
            res["perspective_layers_per_batch"] = statistics.mean(
                sum(q.P is not None for p in ps for q in p.layers()) for ps in plans)
        if args.mixup > 0:
            res["mixed_samples_per_batch"] = statistics.mean(sum(p.mix is not None for p in ps) for ps in plans)
        res["render_batch"] = {"resident": r_dev, "host_sources": r_host, "resident_again": r_dev2, "identical": same,
                               "resident_not_slower": min(r_dev["wall_median_ms"], r_dev2["wall_median_ms"]) <=
                               r_host["wall_median_ms"]}
        # (d) loader throughput beside a training step
        if not args.no_train:
            from adrefine.engine.trainer import FusedTrainer
            from adrefine.nn.tasks import DetectionModel
            m = DetectionModel(str(ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"),
                               compute_dtype=torch.bfloat16)
            tr = FusedTrainer(m.cuda(), batch_size=BS, nbs=BS)
            first = next(iter(build_dataloader(ds, BS, prefetch=0)))
            for _ in range(3):
                tr.step(first)
            res["train_step_alone"] = timed([lambda: tr.step(first) for _ in range(13)])
            for prefetch in (0, 1):
                ld = build_dataloader(ds, BS, prefetch=prefetch)
                for _ in ld:  # warm epoch
                    pass
                torch.cuda.synchronize()
                t0, nimg = time.perf_counter(), 0
                for _ in range(2):
                    for batch in ld:
                        tr.step(batch)
                        nimg += batch["img"].shape[0]
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                res[f"loader_with_step_prefetch{prefetch}"] = {"images_per_s": nimg / dt, "ms_per_batch": dt / (nimg / BS) * 1e3}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    key = "_".join(f"{k}_{v:g}" for k, v in (("mixup", args.mixup), ("perspective", args.perspective)) if v > 0)
    if key and Path(args.out).exists():  # beside the default-hyp rows, which stay as they were measured
        res = dict(json.loads(Path(args.out).read_text()), **{key: res})
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
