"""Generate the test-time-augmentation fixtures by running the REFERENCE's own code — build container only (like
oracle/gen_golden.py it refuses to run without the reference checkout). CPU only.

Run:  python scripts/gen_tta_golden.py

The reference is imported as oracle/gen_golden.py imports it (oracle/stubs for the packages absent from the image;
the AYHead's deformable convolution is the stub's restatement, so the 701 fixture is `unpinned_3rdparty` like every
whole-network fixture of that yaml). Shapes, seeds and yaml names are tests/tta_util.py's.

Writes (data only):
  tests/golden/tta_views.npz          the reference's scale_img (utils/torch_utils.py:439-448) on x.flip(3) at 0.83
                                      and on x at 0.67 (nn/tasks.py:367), for the seeded uint8 batch of
                                      tta_util.VIEWS_SHAPE divided by 255: u8, v1, v2. Asserted here: the restatements
                                      of tests/tta_util.py (scale_img, descale_pred, clip_augmented) equal the
                                      reference's functions bit for bit.
  tests/golden/tta_net701_256x320.npz the reference DetectionModel of the 701 yaml, recipe weights, eval mode:
                                      y_aug = model(x, augment=True)[0] and y = model(x)[0] on recipe.synthetic_images
                                      cut to B=2, 256 x 320 (MLCA couples the images of a batch), with img_seed.
  tests/golden/tta_y11n_320.npz       the same for yolo11n at B=1, 320 x 320.
  tests/golden/TTA_MANIFEST.json      what each of the three holds and the reference lines it comes from, in the
                                      entry form of MANIFEST.json (which oracle/gen_golden.py owns and this script
                                      leaves alone)."""
from __future__ import annotations

import json
import os
import sys
import zipfile
from pathlib import Path

import numpy as np
import torch

REF = Path("/root/reference")
REPO = Path(__file__).resolve().parents[1]
OUT = REPO / "tests" / "golden"
MAX_BYTES = 1 << 20
sys.path.insert(0, str(REPO / "oracle"))
sys.path.insert(0, str(REPO / "tests"))
import tta_util as T  # noqa: E402
from recipe import recipe_state_dict  # noqa: E402


def _import_reference():
    if not REF.is_dir():
        raise SystemExit("gen_tta_golden: the reference checkout is not present — fixtures are generated in the "
                         "build container")
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.dont_write_bytecode = True
    os.environ.setdefault("YOLO_CONFIG_DIR", "/tmp/adr_yolo_cfg")
    sys.path.insert(0, str(REPO / "oracle" / "stubs"))
    sys.path.insert(1, str(REF))
    import ultralytics  # noqa: F401
    from ultralytics.nn import tasks
    from ultralytics.utils import torch_utils
    return tasks, torch_utils


def _save(path, d):
    """An .npz with LZMA members (np.load reads them through zipfile like deflated ones)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
        for k, v in d.items():
            with z.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)
    size = path.stat().st_size
    print(path.name, size, "bytes")
    if size > MAX_BYTES:
        raise SystemExit(f"gen_tta_golden: {path.name} is {size} bytes, over the {MAX_BYTES} limit of a committed file")


def views(tasks, torch_utils):
    u8 = T.u8_images(T.VIEWS_SHAPE, T.VIEWS_SEED)
    x = u8.float() / 255
    v1 = torch_utils.scale_img(x.flip(3), 0.83, gs=32)
    v2 = torch_utils.scale_img(x, 0.67, gs=32)
    assert torch.equal(T.view(x, 0), x) and torch.equal(T.view(x, 1), v1) and torch.equal(T.view(x, 2), v2)
    for shape, seed in ((T.VIEWS_SHAPE, T.VIEWS_SEED), (T.EDGE_SHAPE, T.EDGE_SEED)):  # the restatement == the reference
        xe = T.u8_images(shape, seed).float() / 255
        for s, f in zip(T.SCALES, T.FLIPS):
            xf = xe.flip(f) if f else xe
            assert torch.equal(T.scale_img(xf, s), torch_utils.scale_img(xf, s))
    g = torch.Generator().manual_seed(5)
    ys = [torch.rand(2, 7, a, generator=g) * 300 for a in (1680, 1323, 882)]
    ref = [tasks.DetectionModel._descale_pred(y.clone(), f, s, (256, 320)) for y, s, f in zip(ys, T.SCALES, T.FLIPS)]
    mine = [T.descale_pred(y.clone(), f, s, (256, 320)) for y, s, f in zip(ys, T.SCALES, T.FLIPS)]
    assert all(torch.equal(a, b) for a, b in zip(ref, mine))
    holder = type("M", (), {"model": [type("H", (), {"nl": 3})()]})()
    clipped = tasks.DetectionModel._clip_augmented(holder, list(ref))
    assert torch.equal(torch.cat(clipped, -1), T.merge(ys, (256, 320)))
    _save(OUT / "tta_views.npz", dict(u8=u8.numpy(), v1=v1.numpy(), v2=v2.numpy()))
    return {"tta_views": dict(what="scale_img of x.flip(3) at 0.83 and of x at 0.67 on a seeded (2, 3, 40, 56) batch",
                              reference="utils/torch_utils.py:439-448, nn/tasks.py:363-367", unpinned_3rdparty=False)}


def nets(tasks):
    notes = {}
    for name, c in T.NETS.items():
        torch.manual_seed(0)
        ref_yaml = REF / "z-yaml" / c["cfg"]
        model = tasks.DetectionModel(str(ref_yaml if ref_yaml.is_file() else REPO / "tests" / "configs" / c["cfg"]),
                                     nc=c.get("nc"), verbose=False)
        sd = model.state_dict()
        model.load_state_dict(recipe_state_dict([(k, v.shape) for k, v in sd.items()]), strict=True)
        model.eval()
        x = T.rect_images(c["B"], c["H"], c["W"], c["seed"])
        with torch.no_grad():
            y = model(x)[0]
            y_aug, none = model(x, augment=True)
        assert none is None
        a0 = y.shape[-1]
        assert torch.equal(y_aug[..., :a0 - a0 // 21], y[..., :a0 - a0 // 21])
        _save(OUT / f"{name}.npz", dict(img_seed=np.array(c["seed"]), y_aug=y_aug.numpy(), y=y.numpy()))
        notes[name] = dict(what=f"{c['cfg']} eval model(x, augment=True)[0] and model(x)[0], bs{c['B']} "
                                f"{c['H']}x{c['W']} (recipe weights)",
                           reference="nn/tasks.py:357-394, utils/torch_utils.py:439-448",
                           unpinned_3rdparty="701" in c["cfg"])
    return notes


def main():
    tasks, torch_utils = _import_reference()
    OUT.mkdir(parents=True, exist_ok=True)
    torch.set_num_threads(8)
    notes = views(tasks, torch_utils)
    notes.update(nets(tasks))
    # MANIFEST.json is oracle/gen_golden.py's; these fixtures are listed in a manifest of their own, same entry form
    (OUT / "TTA_MANIFEST.json").write_text(json.dumps(
        {"generator": "scripts/gen_tta_golden.py", "torch": torch.__version__, "fixtures": notes}, indent=1) + "\n")


if __name__ == "__main__":
    main()
