"""Test-time augmentation plan — the host arithmetic of the reference's DetectionModel._predict_augment
(nn/tasks.py:357-394) restated with Python floats: the three views of scale_img (utils/torch_utils.py:439-448) and
the anchor columns _clip_augmented (tasks.py:385-394) keeps of each.

The plan is pure host data. The pixels are rendered by adr_tta_views and the three decoded outputs are de-scaled,
de-flipped, clipped and concatenated by adr_tta_merge (csrc/adr_tta.hip); tta_views / tta_merge below bind them.
"""
from __future__ import annotations

import math
from collections import namedtuple

SCALES = (1, 0.83, 0.67)   # tasks.py:363
FLIPS = (None, 3, None)    # tasks.py:364 (3: left-right)
PAD_VALUE = 0.447          # torch_utils.py:448 (the imagenet mean)
MAX_ANCHORS = 16384        # adr_nms takes A <= 16384 predictions per image

# scale, flip: the view's entry of SCALES / FLIPS; (rh, rw): the resized size; (ph, pw): the padded size the network
# sees; anchors: its prediction count A_v; [keep0, keep1): the columns of it that are kept; out_off: where they start
# in the concatenated output
TtaView = namedtuple("TtaView", "scale flip rh rw ph pw anchors keep0 keep1 out_off")
TtaPlan = namedtuple("TtaPlan", "H W views a_total")


def tta_plan(H, W, gs=32, nl=3):
    """The three views of an (H, W) batch for a head of `nl` levels at strides gs / 2^(nl-1) ... gs, `gs` the
    largest stride. Raises NotImplementedError when the concatenated prediction count exceeds what adr_nms takes."""
    H, W, gs, nl = int(H), int(W), int(gs), int(nl)
    if H <= 0 or W <= 0 or gs <= 0 or nl <= 0 or gs % 2 ** (nl - 1):
        raise ValueError(f"tta_plan: image size {H}x{W}, stride {gs}, {nl} levels")
    strides = [gs // 2 ** (nl - 1 - i) for i in range(nl)]
    g = sum(4 ** x for x in range(nl))  # tasks.py:388
    e = 1  # tasks.py:389
    views, off = [], 0
    for v, (s, f) in enumerate(zip(SCALES, FLIPS)):
        if s == 1.0:  # torch_utils.py:441-442
            rh, rw, ph, pw = H, W, H, W
        else:
            rh, rw = int(H * s), int(W * s)  # :444
            ph, pw = (math.ceil(x * s / gs) * gs for x in (H, W))  # :447
        a = sum(-(-ph // st) * -(-pw // st) for st in strides)  # (the stride-2 convs round up)
        k0, k1 = 0, a
        if v == 0:  # tasks.py:390-391
            k1 = a - (a // g) * sum(4 ** x for x in range(e))
        if v == len(SCALES) - 1:  # :392-393
            k0 = (a // g) * sum(4 ** (nl - 1 - x) for x in range(e))
        views.append(TtaView(s, f, rh, rw, ph, pw, a, k0, k1, off))
        off += k1 - k0
    if off > MAX_ANCHORS:
        raise NotImplementedError(
            f"augment=True at {H}x{W} concatenates {off} predictions per image; adr_nms takes at most {MAX_ANCHORS} "
            f"(the limit falls just above 640x640)")
    return TtaPlan(H, W, tuple(views), off)


_TABLES = {}  # (device, B, plan) -> (host records, device records, per-view element offsets, total elements)


def _view_tables(plan, B, dev):
    """The adr_tta_view records of the plan's non-identity views, on the host and on the device. Built once per
    (device, batch, plan): a captured graph replays the launch that reads them, so they are never re-uploaded."""
    import numpy as np
    import torch

    from ..native import lib
    key = (str(dev), B, plan)
    hit = _TABLES.get(key)
    if hit is None:
        dt = np.dtype([("out_off", "<i8"), ("rh", "<i4"), ("rw", "<i4"), ("ph", "<i4"), ("pw", "<i4"),
                       ("flip", "<i4"), ("pad", "<i4")])
        if dt.itemsize != lib.adr_tta_view_size():
            raise RuntimeError("tta: adr_tta_view layout mismatch")
        rows, offs, o = [], [], 0
        for v in plan.views[1:]:
            if v.flip not in (None, 3):
                raise NotImplementedError("tta: only left-right flips (3) are rendered")
            rows.append((o, v.rh, v.rw, v.ph, v.pw, int(v.flip == 3), 0))
            offs.append(o)
            o += B * 3 * v.ph * v.pw
        host = np.array(rows, dtype=dt)
        hit = _TABLES[key] = (host, torch.from_numpy(host.view(np.uint8).copy()).to(dev), tuple(offs), o)
    return hit


def tta_views(x, plan):
    """[x, view 1, view 2]: the network inputs of the plan's views of x (B, 3, H, W), uint8 or fp32 — the identity
    view is x itself, the others fp32 NCHW batches rendered by one adr_tta_views launch into one buffer."""
    import ctypes

    import torch

    from .. import kernels as K
    from ..native import lib
    if not x.is_cuda:
        raise RuntimeError("adrefine: HIP kernels need device tensors (no CPU fallback)")
    if x.dim() != 4 or x.shape[1] != 3 or tuple(x.shape[2:]) != (plan.H, plan.W):
        raise ValueError(f"tta_views: batch {tuple(x.shape)} for a plan of {plan.H}x{plan.W}")
    if plan.views[0].scale != 1 or plan.views[0].flip is not None:
        raise NotImplementedError("tta: the first view is the batch itself")
    u8 = x.dtype == torch.uint8
    src = x if u8 else x.float()
    if not src.is_contiguous():
        src = src.contiguous()
    B = x.shape[0]
    host, dev_tab, offs, total = _view_tables(plan, B, x.device)
    buf = torch.empty(total, dtype=torch.float32, device=x.device)
    lib.adr_tta_views(int(u8), K.fptr(src), B, plan.H, plan.W, K.fptr(dev_tab), ctypes.c_void_p(host.ctypes.data),
                      len(offs), K.fptr(buf), total, K.stream())
    out = [x]
    for v, o in zip(plan.views[1:], offs):
        out.append(buf[o:o + B * 3 * v.ph * v.pw].view(B, 3, v.ph, v.pw))
    return out


def tta_merge(ys, plan):
    """The three decoded outputs y_v (B, 4 + nc, A_v) fp32 -> (B, 4 + nc, A_total): boxes de-scaled, the flipped
    view's x mirrored, the tails clipped, concatenated along the anchor axis (one adr_tta_merge launch)."""
    import ctypes

    import torch

    from .. import kernels as K
    from ..native import lib
    if len(ys) != 3 or len(plan.views) != 3:
        raise ValueError("tta_merge: three views")
    B, rows = ys[0].shape[0], ys[0].shape[1]
    for y, v in zip(ys, plan.views):
        if not y.is_cuda or y.dtype != torch.float32 or not y.is_contiguous() or tuple(y.shape) != (B, rows, v.anchors):
            raise ValueError(f"tta_merge: output {tuple(y.shape)} {y.dtype} for a view of {v.anchors} anchors "
                             f"(fp32, contiguous, on the device)")
    i3, f3 = ctypes.c_int * 3, ctypes.c_float * 3
    out = torch.empty(B, rows, plan.a_total, dtype=torch.float32, device=ys[0].device)
    lib.adr_tta_merge(K.fptr(ys[0]), K.fptr(ys[1]), K.fptr(ys[2]), i3(*[v.anchors for v in plan.views]),
                      i3(*[v.keep0 for v in plan.views]), i3(*[v.keep1 for v in plan.views]),
                      f3(*[v.scale for v in plan.views]), i3(*[int(v.flip == 3) for v in plan.views]),
                      float(plan.W), K.fptr(out), B, rows, plan.a_total, K.stream())
    return out
