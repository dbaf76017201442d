"""GPU: adr_letterbox_u8 and adr_scale_boxes (csrc/adr_letterbox.hip) against the fixtures the reference's own
LetterBox / scale_boxes code made (scripts/gen_letterbox_golden.py; OpenCV's resize restated in
tests/letterbox_util.py: PARITY UNPINNED), the close-mosaic chain through collate_fn, and
FusedPredictor.predict_images end to end."""
from pathlib import Path

import numpy as np
import pytest
import torch

import letterbox_util as U
from conftest import ROOT
from gpu_util import load_recipe_into

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
CFG = ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"
IDS = [c[0] for c in U.CASES]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "letterbox_cases.npz", allow_pickle=False)


def _groups(gold):
    """Case indices by output shape (H, W): each group is one launch."""
    by = {}
    for i, name in enumerate(IDS):
        by.setdefault(gold[f"{name}_img"].shape[:2], []).append(i)
    return by


def test_letterbox_kernel_renders_every_case(gold):
    """Cases of equal output shape are one launch (mixed source sizes and resize modes) with one fill slot at the
    end; every image equals the reference's LetterBox output exactly, in BGR and in RGB plane order."""
    from adrefine.data.augment import LetterBox, render_letterbox
    from adrefine.data.instance import Instances
    seen = set()
    for (H, W), idxs in _groups(gold).items():
        for rgb in (True, False):
            plans = []
            for i in idxs:
                p = LetterBox(**U.CASES[i][2])(U.case_labels(i, Instances))["img"]
                p.rgb = rgb
                plans.append(p)
                seen.add("copy" if p.resize is None else "area" if p.tiles[0][0].shape[1] == 2 * p.resize[0]
                         else "linear")
            out = torch.zeros(len(idxs) + 1, 3, H, W, dtype=torch.uint8, device="cuda")
            got, info = render_letterbox(plans, out=out)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr() and len(info) == len(idxs)
            img = out.cpu().numpy()
            for k, i in enumerate(idxs):
                want = gold[f"{IDS[i]}_img"].transpose(2, 0, 1)
                want = want[::-1] if rgb else want
                bad = np.argwhere(img[k] != want)
                assert len(bad) == 0, (IDS[i], rgb, len(bad), bad[:5].tolist())
                assert info[k][1] == tuple(gold[f"{IDS[i]}_pad"].tolist())
            assert (img[-1] == 114).all()  # the empty slot
    assert seen == {"copy", "area", "linear"}
    assert any(W % 4 for _, W in _groups(gold)) and any(W % 4 == 0 for _, W in _groups(gold))


def test_letterbox_from_raw_images(gold):
    """render_letterbox on raw images with LetterBox arguments: a new tensor, RGB planes."""
    from adrefine.data.augment import render_letterbox
    idxs = [i for i in _groups(gold)[(96, 96)] if U.CASES[i][2] == dict(new_shape=(96, 96)) and U.CASES[i][3] is None]
    assert len(idxs) >= 3
    out, info = render_letterbox([U.case_inputs(i)[0] for i in idxs], (96, 96), "cuda")
    torch.cuda.synchronize()
    for k, i in enumerate(idxs):
        assert np.array_equal(out[k].cpu().numpy(), gold[f"{IDS[i]}_img"].transpose(2, 0, 1)[::-1]), IDS[i]


def test_letterbox_entry_rejects_bad_geometry():
    """The entry validates the host copy of the descriptors before launching."""
    from adrefine.data.augment import ImagePlan, render_letterbox
    p = ImagePlan(np.zeros((8, 8, 3), np.uint8))
    p.resize, p.size = (200, 200, 0, 0), (96, 96)
    with pytest.raises(ValueError, match="outside"):
        render_letterbox([p], device="cuda")


def test_collate_close_mosaic_vs_reference():
    from adrefine.data.augment import collate_fn
    from test_letterbox import run_close_mosaic
    g = np.load(GOLD / f"{U.CLOSE_MOSAIC['name']}.npz", allow_pickle=False)
    batch = collate_fn(run_close_mosaic())
    torch.cuda.synchronize()
    img = batch["img"].cpu().numpy()
    assert img.dtype == np.uint8 and img.shape == g["img"].shape
    bad = np.argwhere(img != g["img"])
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    assert np.array_equal(batch["bboxes"].numpy(), g["bboxes"]) and np.array_equal(batch["cls"].numpy(), g["cls"])
    assert np.array_equal(batch["batch_idx"].numpy(), g["batch_idx"])


def test_collate_routes_resize_plans(gold):
    """The validation transform on images that are not at imgsz: plans with a resize, and a mixed batch (one pad
    only), go through collate_fn."""
    from adrefine.data.augment import Compose, Format, LetterBox, collate_fn
    from adrefine.data.instance import Instances
    idxs = [IDS.index(n) for n in ("up", "noscaleup", "down")]
    out = []
    for i in idxs:
        T = Compose([LetterBox(**U.CASES[i][2]), Format()])
        out.append(T(U.case_labels(i, Instances)))
    assert [o["img"].resize is None for o in out] == [False, True, False]
    batch = collate_fn(out)
    torch.cuda.synchronize()
    for k, i in enumerate(idxs):
        want = gold[f"{IDS[i]}_img"].transpose(2, 0, 1)[::-1]
        assert np.array_equal(batch["img"][k].cpu().numpy(), want), IDS[i]


def test_scale_boxes_device_vs_reference(gold):
    """adr_scale_boxes on the padded layout (B, max_det, 6) with per-image counts: rows below the count equal the
    reference's scale_boxes exactly, rows at or beyond it are untouched; and ops.scale_boxes / clip_boxes on device
    tensors (contiguous and the pred[:, :4] row view)."""
    from adrefine.kernels import fptr, stream
    from adrefine.native import lib
    from adrefine.utils.ops import clip_boxes, scale_boxes, scale_boxes_table, scale_gain_pad
    B, R = len(IDS), 8
    boxes = torch.full((B, R, 6), -7.25)
    counts, rows = [], []
    for i, name in enumerate(IDS):
        det = torch.from_numpy(U.case_inputs(i)[3])
        n = 6 - i % 3
        boxes[i, :6] = det
        counts.append(n)
        h0, w0 = U.CASES[i][1]
        gain, pad = scale_gain_pad(gold[f"{name}_img"].shape[:2], (h0, w0))
        rows.append((gain, pad[0], pad[1], w0, h0))
    before = boxes.clone()
    d = boxes.cuda()
    cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    tab = scale_boxes_table(rows, "cuda")
    lib.adr_scale_boxes(fptr(d), fptr(cnt), fptr(tab), B, R, 6, 0, stream())
    got = d.cpu()
    for i, name in enumerate(IDS):
        n = counts[i]
        assert np.array_equal(got[i, :n].numpy(), gold[f"{name}_scaled"][:n]), name
        assert torch.equal(got[i, n:], before[i, n:]), name
    for i, name in enumerate(IDS):
        det = torch.from_numpy(U.case_inputs(i)[3])
        h0, w0 = U.CASES[i][1]
        shape1 = gold[f"{name}_img"].shape[:2]
        r = gold[f"{name}_rp"]
        rp = ((float(r[0]), float(r[1])), (int(r[2]), int(r[3])))
        assert np.array_equal(scale_boxes(shape1, det.cuda(), (h0, w0)).cpu().numpy(), gold[f"{name}_scaled"])
        assert np.array_equal(scale_boxes(shape1, det.cuda(), (h0, w0), ratio_pad=rp).cpu().numpy(),
                              gold[f"{name}_scaled_rp"])
        assert np.array_equal(scale_boxes(shape1, det.cuda(), (h0, w0), xywh=True).cpu().numpy(),
                              gold[f"{name}_scaled_xywh"])
        assert np.array_equal(clip_boxes(det.cuda(), (h0, w0)).cpu().numpy(), gold[f"{name}_clipped"])
        full = det.cuda()
        scale_boxes(shape1, full[:, :4], (h0, w0))  # the row view the reference's postprocess passes
        assert np.array_equal(full.cpu().numpy(), gold[f"{name}_scaled"])


def test_predict_images_end_to_end():
    """predict_images on 3 images of different sizes (graph captured at batch 4, the model and size of
    test_predictor_matches_model_plus_nms) equals the reference path exactly: numpy-executor letterbox -> uint8
    batch -> predict() -> CPU scale_boxes. A second call with other images returns theirs (the static input is
    rewritten in place); the slot beyond len(imgs) yields nothing; eager (no graph) agrees."""
    from adrefine.data.augment import LetterBox
    from adrefine.data.synthetic import images_u8
    from adrefine.engine.predictor import FusedPredictor
    from adrefine.nn.tasks import DetectionModel
    from adrefine.utils.ops import scale_boxes
    m = DetectionModel(str(CFG), compute_dtype=torch.float32)
    load_recipe_into(m)
    m = m.cuda().eval()
    S = 320
    p = FusedPredictor(m, conf=0.001, iou=0.7, multi_label=True)
    ref_p = FusedPredictor(m, conf=0.001, iou=0.7, multi_label=True)
    p.capture(images_u8(4, S, seed=3).cuda())

    def sources(seed, shapes):
        big = images_u8(len(shapes), 512, seed=seed).numpy().transpose(0, 2, 3, 1)
        return [np.ascontiguousarray(big[k, :h, :w]) for k, (h, w) in enumerate(shapes)]

    def reference(imgs):
        batch = np.full((4, 3, S, S), 114, dtype=np.uint8)
        for k, im in enumerate(imgs):
            plan = LetterBox((S, S), auto=False)(image=im)
            plan.rgb = True
            batch[k] = U.execute_chw(plan)
        dets = ref_p.predict(torch.from_numpy(batch).cuda())
        return [scale_boxes((S, S), d.cpu(), im.shape[:2]) for d, im in zip(dets, imgs)]

    total = 0
    for seed, shapes in ((21, [(240, 400), (512, 300), (150, 150)]), (22, [(333, 211), (480, 512)])):
        imgs = sources(seed, shapes)
        got = p.predict_images(imgs)
        want = reference(imgs)
        assert len(got) == len(imgs)
        for a, b in zip(got, want):
            assert a.shape == b.shape and torch.equal(a.cpu(), b)
            total += len(b)
        if seed == 21:  # no graph: the batch is the images (four, as the reference path's batch)
            imgs4 = imgs + [imgs[0][:100, :90].copy()]
            eager = FusedPredictor(m, conf=0.001, iou=0.7, multi_label=True).predict_images(imgs4, imgsz=S)
            for a, b in zip(eager, reference(imgs4)):
                assert a.shape == b.shape and torch.equal(a.cpu(), b)
    assert total > 0
    with pytest.raises(ValueError):
        p.predict_images([imgs[0]] * 5)
