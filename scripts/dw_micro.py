"""Time the depthwise conv kernels per site shape of the train step, old against new, with HIP events around R
back-to-back calls after a warm-up (bf16, through the C ABI):
  forward and data gradient: dw_img_kernel (ADR_DW_RUN=0) against the row-run dw_run_kernel;
  backward: data gradient + weight gradient (with the bias rows) as two launches against adr_dwconv_bwd_fused.

  python scripts/dw_micro.py            the default sites (the n-scale step at bs 64, 640^2)
  python scripts/dw_micro.py --sites    first run one training forward of the detector and print every depthwise
                                        site's (N, H, W, C, k, x channel stride), then time those shapes
"""
import argparse
import ctypes
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "yolo-ad-refine_amd"))
from adrefine import kernels as K  # noqa: E402
from adrefine.native import lib  # noqa: E402

# (N, H, W, C, k, channel stride): C2PTSSA PFF 3x3 and 7x7, EDFFN 3x3
DEFAULT_SITES = [(64, 20, 20, 128, 3, 128), (64, 20, 20, 128, 7, 128), (64, 20, 20, 512, 3, 512)]


def model_sites(img, bs):
    from adrefine.nn.tasks import DetectionModel
    cfg = ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"
    m = DetectionModel(str(cfg), compute_dtype=torch.bfloat16).cuda().train()
    seen, orig = [], K.dwconv

    def spy(x, w, b, k):
        n, c, h, wd = x.shape
        seen.append((n, h, wd, c, k, K.nhwc(x)[2]))
        return orig(x, w, b, k)

    K.dwconv = spy
    try:
        m(torch.rand(bs, 3, img, img, device="cuda"))
    finally:
        K.dwconv = orig
    torch.cuda.synchronize()
    for i, s in enumerate(seen):
        print("site %2d: N=%d H=%d W=%d C=%d k=%d xcs=%d" % ((i,) + s), flush=True)
    uniq = []
    for s in seen:
        if s not in uniq:
            uniq.append(s)
    return uniq


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps  # us per call


def site_times(N, H, W, C, k, cs, reps):
    x = torch.randn(N, H, W, cs, device="cuda").to(torch.bfloat16)
    dy = torch.randn(N, H, W, cs, device="cuda").to(torch.bfloat16)
    y = torch.empty_like(x)
    w = torch.randn(C, 1, k, k, device="cuda") * 0.1
    b = torch.zeros(C, device="cuda")
    wsb = lib.adr_dwconv_wgrad_workspace(N, H, W, C, k)
    ws = torch.empty(wsb // 4 + 1, dtype=torch.float32, device="cuda")
    bp = torch.empty(N * 2 * C, dtype=torch.float32, device="cuda")
    ch = ctypes.c_int(0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = K.stream()

    def fwd():
        lib.adr_dwconv_fwd(K.BF16, p(x), cs, K.fptr(w), K.fptr(b), p(y), cs, N, H, W, C, k, st)

    def dgrad():
        lib.adr_dwconv_bwd(K.BF16, p(x), cs, p(dy), cs, K.fptr(w), p(y), cs, None, N, H, W, C, k, 0, 0, K.fptr(ws), wsb,
                           st)

    def wgrad():
        lib.adr_dwconv_wgrad_partials_bias(K.BF16, p(x), cs, p(dy), cs, N, H, W, C, k, K.fptr(ws), wsb, K.fptr(bp),
                                           ctypes.byref(ch), st)

    def two():
        dgrad()
        wgrad()

    def fused():
        lib.adr_dwconv_bwd_fused(K.BF16, p(x), cs, p(dy), cs, K.fptr(w), p(y), cs, None, N, H, W, C, k, 0, 0,
                                 K.fptr(ws), wsb, K.fptr(bp), ctypes.byref(ch), st)

    r = {}
    os.environ["ADR_DW_RUN"] = os.environ["ADR_DW_FUSED"] = "0"
    r["fwd_old"], r["dgrad_old"], r["wgrad"], r["bwd_old"] = (timed(f, reps) for f in (fwd, dgrad, wgrad, two))
    os.environ["ADR_DW_RUN"] = os.environ["ADR_DW_FUSED"] = "1"
    r["fwd_new"], r["dgrad_new"] = timed(fwd, reps), timed(dgrad, reps)
    ok = lib.adr_dwconv_bwd_fused_supported(K.BF16, H, W, C, k, cs, cs, cs)
    r["bwd_new"] = timed(fused, reps) if ok else float("nan")
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", action="store_true")
    ap.add_argument("--img", type=int, default=640)
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    sites = model_sites(a.img, a.bs) if a.sites else DEFAULT_SITES
    print("| N | HxW | C | k | xcs | fwd old | fwd new | dgrad old | dgrad new | wgrad | dgrad+wgrad old | fused bwd |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for (N, H, W, C, k, cs) in sites:
        r = site_times(N, H, W, C, k, cs, a.reps)
        print("| %d | %dx%d | %d | %d | %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f |" % (
            N, H, W, C, k, cs, r["fwd_old"], r["fwd_new"], r["dgrad_old"], r["dgrad_new"], r["wgrad"], r["bwd_old"],
            r["bwd_new"]), flush=True)


if __name__ == "__main__":
    main()
