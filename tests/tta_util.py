"""Shared pieces of the test-time-augmentation tests (test infrastructure): plain-torch restatements of the
reference's scale_img (utils/torch_utils.py:439-448), DetectionModel._descale_pred and _clip_augmented
(nn/tasks.py:374-394), and the inputs of the fixtures scripts/gen_tta_golden.py writes. The script asserts that these
restatements equal the reference's own functions bit for bit; on CPU tensors they ARE the definition of parity for
adr_tta_views and adr_tta_merge."""
import math
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
SCALES = (1, 0.83, 0.67)
FLIPS = (None, 3, None)
VIEWS_SHAPE = (2, 3, 40, 56)  # tta_views.npz
VIEWS_SEED = 31
EDGE_SHAPE = (1, 3, 33, 47)   # one row and one column more than a multiple of 2: the last taps clamp
EDGE_SEED = 32
# whole-network fixtures: name -> yaml (under tests/configs), class count, batch, size, image seed. nc is 16, not the
# yamls' 80 (DetectionModel(cfg, nc=16)): the augmented output has 1.9 x the columns of a plain one and is stored
# next to it, and with 84 rows either file would be twice the size a committed file may have
NETS = {
    "tta_net701_256x320": dict(cfg="yolo11-701-YOLO-AD-Refine.yaml", nc=16, B=2, H=256, W=320, seed=0),
    "tta_y11n_320": dict(cfg="yolo11n.yaml", nc=16, B=1, H=320, W=320, seed=0),
}


def u8_images(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8))


def rect_images(B, H, W, seed):
    """recipe.synthetic_images cut to a rectangle."""
    sys.path.insert(0, str(ROOT / "oracle"))
    from recipe import synthetic_images
    return synthetic_images(B, max(H, W), seed=seed)[:, :, :H, :W].contiguous()


def scale_img(img, ratio=1.0, same_shape=False, gs=32):
    """torch_utils.py:439-448."""
    if ratio == 1.0:
        return img
    h, w = img.shape[2:]
    s = (int(h * ratio), int(w * ratio))
    img = F.interpolate(img, size=s, mode="bilinear", align_corners=False)
    if not same_shape:
        h, w = (math.ceil(x * ratio / gs) * gs for x in (h, w))
    return F.pad(img, [0, w - s[1], 0, h - s[0]], value=0.447)


def view(x, v, gs=32):
    """The network input of view v (tasks.py:367)."""
    return scale_img(x.flip(FLIPS[v]) if FLIPS[v] else x, SCALES[v], gs=gs)


def descale_pred(p, flips, scale, img_size, dim=1):
    """tasks.py:374-383 (p is modified in place, as there)."""
    p[:, :4] /= scale
    x, y, wh, cls = p.split((1, 1, 2, p.shape[dim] - 4), dim)
    if flips == 2:
        y = img_size[0] - y
    elif flips == 3:
        x = img_size[1] - x
    return torch.cat((x, y, wh, cls), dim)


def clip_augmented(y, nl=3):
    """tasks.py:385-394."""
    g = sum(4 ** x for x in range(nl))
    e = 1
    i = (y[0].shape[-1] // g) * sum(4 ** x for x in range(e))
    y[0] = y[0][..., :-i]
    i = (y[-1].shape[-1] // g) * sum(4 ** (nl - 1 - x) for x in range(e))
    y[-1] = y[-1][..., i:]
    return y


def merge(ys, img_size, nl=3):
    """tasks.py:369-372 on the three per-view outputs (CPU tensors; left unchanged)."""
    y = [descale_pred(yi.clone(), fi, si, img_size) for yi, si, fi in zip(ys, SCALES, FLIPS)]
    return torch.cat(clip_augmented(y, nl), -1)


def segments(plan):
    """[(first output column, length, scale)] of the plan's views."""
    return [(v.out_off, v.keep1 - v.keep0, v.scale) for v in plan.views]
