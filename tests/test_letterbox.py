"""LetterBox, the close-mosaic chain and scale_boxes / clip_boxes on the host (CPU) against fixtures made by running
the reference's own code (scripts/gen_letterbox_golden.py; its cv2.resize / cv2.copyMakeBorder on the numpy
restatement in tests/letterbox_util.py, so OpenCV's internals are PARITY UNPINNED, the reference's arithmetic around
them is pinned).

The image fixtures come from the same restatement the plans are executed with, so one test anchors the restatement
itself to an independent bilinear resize (torch F.interpolate)."""
from pathlib import Path

import numpy as np
import pytest
import torch

import letterbox_util as U

GOLD = Path(__file__).resolve().parent / "golden"
IDS = [c[0] for c in U.CASES]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "letterbox_cases.npz", allow_pickle=False)


@pytest.mark.parametrize("idx", range(len(U.CASES)), ids=IDS)
def test_letterbox_plan_and_labels_vs_reference(idx, gold):
    from adrefine.data.augment import ImagePlan, LetterBox
    from adrefine.data.instance import Instances
    name, _, kw, rect = U.CASES[idx]
    labels = LetterBox(**kw)(U.case_labels(idx, Instances))
    plan = labels["img"]
    assert isinstance(plan, ImagePlan)
    img = U.execute_letterbox(plan)
    assert img.shape == gold[f"{name}_img"].shape and np.array_equal(img, gold[f"{name}_img"])
    (ratio_in, (left, top)) = labels["ratio_pad"]
    assert [left, top] == gold[f"{name}_pad"].tolist() and np.array_equal(np.array(ratio_in), gold[f"{name}_ratio_in"])
    assert list(labels["resized_shape"]) == gold[f"{name}_resized_shape"].tolist()
    ins = labels["instances"]
    assert ins.format == "xyxy" and not ins.normalized
    assert ins.bboxes.dtype == gold[f"{name}_bboxes"].dtype and np.array_equal(ins.bboxes, gold[f"{name}_bboxes"])
    assert np.array_equal(labels["cls"], gold[f"{name}_cls"])
    assert plan.ratio_pad[1] == (left, top)
    pad_only = name in ("odd_pad", "noscaleup")
    assert (plan.resize is None) == pad_only
    if rect is None:  # image= alone returns the plan of the same pixels
        alone = LetterBox(**kw)(image=U.case_inputs(idx)[0])
        assert isinstance(alone, ImagePlan) and np.array_equal(U.execute_letterbox(alone), gold[f"{name}_img"])


def test_letterbox_cases_reach_their_paths(gold):
    """The case list reaches what it is there for: left != right and top != bottom, the clamps, the area path."""
    from adrefine.data.augment import LetterBox, resize_linear_tables
    p = LetterBox(**U.CASES[IDS.index("odd_pad")][2])(image=U.case_inputs(IDS.index("odd_pad"))[0])
    (x1, y1, x2, y2) = p.tiles[0][1:5]
    assert (x1, p.size[0] - x2) == (25, 26) and (y1, p.size[1] - y2) == (22, 23)
    p = LetterBox(**U.CASES[IDS.index("odd_resize")][2])(image=U.case_inputs(IDS.index("odd_resize"))[0])
    nw, nh, left, top = p.resize
    assert top == 5 and p.size[1] - top - nh == 6
    sx, a0, a1 = resize_linear_tables(2, 4)  # the 2-pixel-wide source: both clamps, and the package's tables
    i, c0, c1 = U._axis(2, 4)
    assert sx.tolist() == [0, 0, 0, 1] and a1[0] == 0 and a1[3] == 0 and 0 < a1[1] < a1[2] < 2048
    assert np.array_equal(sx, i) and np.array_equal(a0, c0) and np.array_equal(a1, c1)
    p = LetterBox(**U.CASES[IDS.index("area2x")][2])(image=U.case_inputs(IDS.index("area2x"))[0])
    assert p.resize[:2] == (96, 64) and p.tiles[0][0].shape[:2] == (128, 192)
    assert gold["w90_img"].shape[1] % 4 != 0 and gold["auto_img"].shape[:2] == (64, 128)


@pytest.mark.parametrize("idx", range(len(U.CASES)), ids=IDS)
def test_resize_restatement_vs_float_bilinear(idx):
    """The non-circular anchor: the restated fixed-point resize is within 1 grey level of round(bilinear) computed in
    floating point by torch (align_corners=False: the same sampling geometry (d + 0.5) * scale - 0.5 with edge
    clamping; the 2x area path is bilinear at fx = fy = 1/2). Bound: the fixed-point budget — coefficients quantised
    to 2^-11 (|error| <= 255 * 2 * 2^-12 per pass), two truncating shifts (>> 4 of the row sums, >> 16 of each
    product: < 1/4 + 2/4 of a final unit before the + 2 >> 2 rounding) — less than one grey level in total, so the
    rounded results differ by at most 1."""
    from adrefine.data.augment import LetterBox
    src = U.case_inputs(idx)[0]
    p = LetterBox(**U.CASES[idx][2])(image=src)
    if p.resize is None:
        nw, nh = src.shape[1], src.shape[0]
    else:
        nw, nh = p.resize[:2]
    ours = U.resize(src, (nw, nh)) if p.resize is not None else src
    t = torch.from_numpy(src).permute(2, 0, 1)[None].double()
    ref = torch.nn.functional.interpolate(t, size=(nh, nw), mode="bilinear", align_corners=False)
    ref = ref.round().clamp(0, 255)[0].permute(1, 2, 0).numpy()
    diff = np.abs(ours.astype(np.int64) - ref.astype(np.int64))
    print(U.CASES[idx][0], "max |restated - round(bilinear)| =", int(diff.max()), "mean", float(diff.mean()))
    assert ours.shape == ref.shape and diff.max() <= 1


def test_close_mosaic_chain_vs_reference():
    """build_transforms + close_mosaic (mosaic off: RandomPerspective runs its LetterBox pre_transform) on the
    fixture's items and seeds: labels bit-exact, every plan (a padded canvas -> warp -> HSV -> flip) executes to the
    fixture image exactly."""
    from aug_util import SynthDS, execute_plan
    from adrefine.data.augment import LetterBox, build_transforms
    from adrefine.data.instance import Instances
    from recipe import synthetic_aug_items
    out = run_close_mosaic()
    cfg = U.CLOSE_MOSAIC
    g = np.load(GOLD / f"{cfg['name']}.npz", allow_pickle=False)
    cls = torch.cat([o["cls"] for o in out]).numpy()
    bboxes = torch.cat([o["bboxes"] for o in out]).numpy()
    bidx = torch.cat([o["batch_idx"] + i for i, o in enumerate(out)]).numpy()
    assert np.array_equal(cls, g["cls"]) and np.array_equal(bidx, g["batch_idx"])
    assert bboxes.dtype == g["bboxes"].dtype and np.array_equal(bboxes, g["bboxes"])
    for i, o in enumerate(out):
        assert o["img"].resize is None  # dataset-fed: pad only, rendered by adr_augment_u8
        img = execute_plan(o["img"])
        assert img.shape == g["img"][i].shape and np.array_equal(img, g["img"][i]), i
    # the validation transform (augment off) is LetterBox(scaleup=False) + Format, and runs
    ds = SynthDS(synthetic_aug_items(8, cfg["imgsz"]), cfg["imgsz"], Instances)
    T = build_transforms(ds, cfg["imgsz"], U.close_mosaic_hyp(), augment=False)
    assert isinstance(T.transforms[0], LetterBox) and not T.transforms[0].scaleup
    o = T(ds.get_image_and_label(1))
    assert o["img"].shape == (256, 256, 3) and o["img"].rgb and o["bboxes"].shape[1] == 4


def run_close_mosaic():
    """Our chain as a trainer reaches it: build_transforms with the default hyp, then close_mosaic, + the seeds."""
    from types import SimpleNamespace

    from aug_util import SynthDS
    from adrefine.data.augment import build_transforms, close_mosaic
    from adrefine.data.instance import Instances
    from recipe import AUG_HYPS, synthetic_aug_items
    cfg = U.CLOSE_MOSAIC
    hyp = SimpleNamespace(**AUG_HYPS["default"])
    ds = SynthDS(synthetic_aug_items(8, cfg["imgsz"]), cfg["imgsz"], Instances)
    ds.augment = True
    ds.transforms = build_transforms(ds, cfg["imgsz"], hyp, augment=True)
    close_mosaic(ds, hyp)
    assert hyp.mosaic == 0.0 and hyp.mixup == 0.0 and hyp.copy_paste == 0.0
    U.seed_chain(cfg["seed"])
    return [ds.transforms(ds.get_image_and_label(i)) for i in cfg["order"]]


def test_resize_then_warp_is_a_scope_guard():
    """A LetterBox that resizes followed by a warp / HSV in one plan is not implemented and says so."""
    from adrefine.data.augment import LetterBox, RandomHSV
    from adrefine.data.instance import Instances
    labels = LetterBox(new_shape=(96, 96))(U.case_labels(0, Instances))
    with pytest.raises(NotImplementedError, match="LetterBox that resizes"):
        RandomHSV()(labels)


@pytest.mark.parametrize("idx", range(len(U.CASES)), ids=IDS)
def test_scale_boxes_cpu_vs_reference(idx, gold):
    from adrefine.utils.ops import clip_boxes, scale_boxes
    name = U.CASES[idx][0]
    src, _, _, det = U.case_inputs(idx)
    h0, w0 = src.shape[:2]
    shape1 = gold[f"{name}_img"].shape[:2]
    t = torch.from_numpy(det)
    assert np.array_equal(scale_boxes(shape1, t.clone(), (h0, w0)).numpy(), gold[f"{name}_scaled"])
    r = gold[f"{name}_rp"]
    rp = ((float(r[0]), float(r[1])), (int(r[2]), int(r[3])))
    assert np.array_equal(scale_boxes(shape1, t.clone(), (h0, w0), ratio_pad=rp).numpy(), gold[f"{name}_scaled_rp"])
    assert np.array_equal(scale_boxes(shape1, t.clone(), (h0, w0), xywh=True).numpy(), gold[f"{name}_scaled_xywh"])
    assert np.array_equal(clip_boxes(t.clone(), (h0, w0)).numpy(), gold[f"{name}_clipped"])
    assert np.array_equal(clip_boxes(det.copy(), (h0, w0)), gold[f"{name}_clipped"])  # the numpy branch
    assert not np.array_equal(gold[f"{name}_scaled"], det)
