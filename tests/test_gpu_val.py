"""GPU: adr_val_match (csrc/adr_val.hip), DetectionStats.update_batched and engine/validator.DetectionValidator against
the fixture the reference's own validator produced (tests/golden/val_batched.npz) and the numpy restatement
(tests/val_util.py); save_last_and_best on a device trainer."""
import numpy as np
import pytest
import torch

import val_util as V
from conftest import ROOT, golden
from gpu_util import load_recipe_into

pytestmark = pytest.mark.gpu
CFG = ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"
RUNS = ("mc", "sc")


@pytest.fixture(scope="module")
def gold():
    return golden("val_batched")


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _native_det(b):
    """The batch's padded detections mapped to native space by adr_scale_boxes, as update_batched does."""
    from adrefine import kernels as K
    from adrefine.native import lib
    det, cnt = _dev(b["det"], torch.float32), _dev(b["counts"], torch.int32)
    tab = torch.tensor(b["table"], dtype=torch.float32).cuda()
    lib.adr_scale_boxes(K.fptr(det), K.fptr(cnt), K.fptr(tab), det.shape[0], det.shape[1], 6, 0, K.stream())
    return det, cnt, tab


def _val_match(b, imgsz, nc, acc, single=False, with_cm=True):
    """One adr_val_match call on a fixture batch; acc = (cm, ntc, nti) device accumulators."""
    from adrefine import kernels as K
    from adrefine.native import lib
    det, cnt, tab = _native_det(b)
    if single:
        det[..., 5] = 0
    B, rows = det.shape[:2]
    N = len(b["cls"])
    off = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(np.bincount(b["batch_idx"].astype(int), minlength=B), out=off[1:])
    cls, box, doff = _dev(b["cls"], torch.float32), _dev(b["bboxes"], torch.float32), _dev(off, torch.int32)
    thr = _dev(V.thresholds(), torch.float32)
    gt = torch.full((max(N, 1), 4), -7.0, device="cuda")
    correct = torch.full((B, rows, 10), 9, dtype=torch.uint8, device="cuda")  # every row must be written
    lib.adr_val_match(K.fptr(det), K.fptr(cnt), B, rows, K.fptr(cls), K.fptr(box), K.fptr(doff), off.ctypes.data, N,
                      K.fptr(tab), int(imgsz[0]), int(imgsz[1]), K.fptr(thr), 10, 0.25, 0.45, nc, K.fptr(gt),
                      K.fptr(correct), K.fptr(acc[0]) if with_cm else None, K.fptr(acc[1]), K.fptr(acc[2]),
                      K.stream())
    torch.cuda.synchronize()
    return gt[:N].cpu().numpy(), correct.cpu().numpy()


def _acc(nc):
    return (torch.zeros(nc + 1, nc + 1, dtype=torch.int32, device="cuda"),
            torch.zeros(nc, dtype=torch.int32, device="cuda"), torch.zeros(nc, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("run", RUNS)
def test_val_match_vs_reference_fixture(gold, run):
    """gt_xyxy bit for bit, correct exact with zero rows past the count, confusion matrix and both tallies exact."""
    nc, imgsz = int(gold[f"{run}_nc"]), tuple(gold["imgsz"])
    acc = _acc(nc)
    tp = []
    for b in V.fixture_batches(gold, run):
        gt, correct = _val_match(b, imgsz, nc, acc, single=run == "sc")
        assert np.array_equal(gt.view(np.uint32), b["gt_xyxy"].view(np.uint32))
        want = V.run_batch(b["det"], b["counts"], b["cls"], b["bboxes"], b["batch_idx"], b["table"], imgsz, nc,
                           single_cls=run == "sc")
        assert np.array_equal(correct, want["correct"])
        for i, n in enumerate(b["counts"]):
            assert not correct[i, int(n):].any()
        tp.append(V.stats_rows(correct, b["counts"], np.bincount(b["batch_idx"].astype(int), minlength=len(b["counts"]))))
    assert np.array_equal(np.concatenate(tp, 0), gold[f"{run}_tp"])
    assert np.array_equal(acc[0].cpu().numpy(), gold[f"{run}_cm"].astype(np.int32))
    assert np.array_equal(acc[1].cpu().numpy(), gold[f"{run}_nt_per_class"])
    assert np.array_equal(acc[2].cpu().numpy(), gold[f"{run}_nt_per_image"])


def test_val_match_accumulates_and_cm_is_optional(gold):
    nc, imgsz = int(gold["mc_nc"]), tuple(gold["imgsz"])
    b = V.fixture_batches(gold, "mc")[1]
    one, two, none = _acc(nc), _acc(nc), _acc(nc)
    _, c1 = _val_match(b, imgsz, nc, one)
    _val_match(b, imgsz, nc, two)
    _val_match(b, imgsz, nc, two)
    for x, y in zip(one, two):
        assert x.sum() > 0 and torch.equal(2 * x, y)
    _, c0 = _val_match(b, imgsz, nc, none, with_cm=False)
    assert np.array_equal(c0, c1) and int(none[0].abs().sum()) == 0
    assert torch.equal(none[1], one[1]) and torch.equal(none[2], one[2])


def _batched_stats(gold, run):
    from adrefine.utils.metrics import DetectionStats
    st = DetectionStats(nc=int(gold[f"{run}_nc"]))
    for b in V.fixture_batches(gold, run):
        batch = {"cls": torch.from_numpy(b["cls"]).view(-1, 1), "bboxes": torch.from_numpy(b["bboxes"]),
                 "batch_idx": torch.from_numpy(b["batch_idx"]), "ori_shape": b["ori_shape"], "ratio_pad": b["ratio_pad"]}
        det, cnt = _dev(b["det"], torch.float32), _dev(b["counts"], torch.int32)
        keep = det.clone()
        st.update_batched(det, cnt, batch, imgsz=tuple(gold["imgsz"]), cm_conf=0.001, single_cls=run == "sc")
        assert torch.equal(det, keep)  # the caller's tensors are not changed
        assert np.array_equal(st.last_gt_xyxy.cpu().numpy(), b["gt_xyxy"])
    return st


@pytest.mark.parametrize("run", RUNS)
def test_update_batched_results_vs_reference(gold, run):
    st = _batched_stats(gold, run)
    assert not st.stats["tp"] and len(st._pending) == int(gold[f"{run}_nbatches"])  # nothing read back yet
    r = st.results()
    assert np.array_equal(np.concatenate(st.stats["tp"], 0), gold[f"{run}_tp"])
    assert np.array_equal(np.concatenate(st.stats["conf"]), gold[f"{run}_conf"])
    assert np.array_equal(r["ap_class_index"], gold[f"{run}_ap_class_index"])
    for k in ("p", "r", "ap"):
        np.testing.assert_allclose(r[k], gold[f"{run}_{k}"], rtol=0, atol=1e-12)
    for k, v in zip(gold[f"{run}_results_keys"], gold[f"{run}_results_vals"]):
        assert abs(r[str(k)] - v) < 1e-12, k
    assert abs(r["fitness"] - float(gold[f"{run}_fitness"])) < 1e-12
    assert r["seen"] == int(gold[f"{run}_seen"])
    assert np.array_equal(r["nt_per_class"], gold[f"{run}_nt_per_class"])
    assert np.array_equal(r["nt_per_image"], gold[f"{run}_nt_per_image"])
    cm = r["confusion_matrix"]
    assert cm.matrix.dtype == np.float64 and np.array_equal(cm.matrix, gold[f"{run}_cm"])
    assert np.array_equal(cm.tp_fp()[0], gold[f"{run}_cm_tp"]) and np.array_equal(cm.tp_fp()[1], gold[f"{run}_cm_fp"])


def test_update_batched_equals_update_on_metrics_fixture():
    """On metrics_val.npz with an identity table (gain 1, no pad, no effective clip) the batched path gives the tp and
    results() of DetectionStats.update. Both get the same boxes: the labels as normalised xywh for the batched path and
    their fp32 round trip as xyxy for update; detections clamped at 0 (the only clip an identity table applies)."""
    from adrefine.utils.metrics import DetectionStats
    g = golden("metrics_val")
    p, lb = g["preds"].copy(), g["labels"]
    p[:, 1:5] = np.maximum(p[:, 1:5], 0)
    nimg, S = int(max(p[:, 0].max(), lb[:, 0].max())) + 1, 640
    xyxy = lb[:, 2:6].astype(np.float64)
    xywh = np.stack([(xyxy[:, 0] + xyxy[:, 2]) / 2 / S, (xyxy[:, 1] + xyxy[:, 3]) / 2 / S,
                     (xyxy[:, 2] - xyxy[:, 0]) / S, (xyxy[:, 3] - xyxy[:, 1]) / S], 1).astype(np.float32)
    ident = [1.0, 0.0, 0.0, 1e9, 1e9]
    same = V.labels_native(xywh, (S, S), ident)
    assert np.abs(same - lb[:, 2:6]).max() < 1e-3
    preds = [torch.from_numpy(p[p[:, 0] == i, 1:]).cuda() for i in range(nimg)]
    a = DetectionStats(nc=80)
    a.update(preds, torch.from_numpy(lb[:, 0]), torch.from_numpy(lb[:, 1]), torch.from_numpy(same))
    det = torch.zeros(nimg, 300, 6, device="cuda")
    for i, q in enumerate(preds):
        det[i, :len(q)] = q
    cnt = torch.tensor([len(q) for q in preds], dtype=torch.int32, device="cuda")
    b = DetectionStats(nc=80)
    b.update_batched(det, cnt, {"cls": torch.from_numpy(lb[:, 1]), "bboxes": torch.from_numpy(xywh),
                                "batch_idx": torch.from_numpy(lb[:, 0]), "ori_shape": [(1e9, 1e9)] * nimg,
                                "ratio_pad": [((1.0, 1.0), (0.0, 0.0))] * nimg}, imgsz=(S, S))
    ra, rb = a.results(), b.results()
    assert np.array_equal(np.concatenate(a.stats["tp"], 0), np.concatenate(b.stats["tp"], 0))
    assert np.concatenate(a.stats["tp"], 0).any()
    for k in ("p", "r", "ap", "ap_class_index"):
        assert np.array_equal(ra[k], rb[k]), k
    for k in ("metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "fitness"):
        assert ra[k] == rb[k], k
    assert set(ra) | {"nt_per_class", "nt_per_image", "seen", "confusion_matrix"} == set(rb)


def _model():
    from adrefine.nn.tasks import DetectionModel
    m = DetectionModel(str(CFG), compute_dtype=torch.float32)
    load_recipe_into(m)
    return m.cuda().eval()


def _val_batches():
    """Two collated val batches (4 and 3 images, the second smaller than the captured one) at 320 x 320 with
    letterbox-like ratio_pad rows."""
    from adrefine.data.synthetic import images_u8, labels
    out = []
    for k, B in enumerate((4, 3)):
        lab = labels(B, 80, seed=5 + k)
        oris = [(300, 400), (640, 480), (320, 320), (200, 333)][:B]
        rps = []
        for h0, w0 in oris:
            r = min(320 / h0, 320 / w0)
            rps.append(((r, r), (int(round((320 - round(w0 * r)) / 2 - 0.1)), int(round((320 - round(h0 * r)) / 2 - 0.1)))))
        out.append({"img": images_u8(B, 320, seed=20 + k).cuda(), **lab, "ori_shape": oris, "ratio_pad": rps})
    return out


def test_detection_validator_end_to_end():
    """DetectionValidator on two batches == predict() per batch -> CPU scale_boxes -> numpy restatement; load_ema after a
    trainer step changes the predictor's outputs."""
    from adrefine.engine.predictor import FusedPredictor
    from adrefine.engine.trainer import FusedTrainer
    from adrefine.engine.validator import DetectionValidator
    from adrefine.utils.metrics import ap_per_class
    from adrefine.utils.ops import scale_boxes
    m = _model()
    batches = _val_batches()
    v = DetectionValidator(m, nc=80)
    res = v(batches)
    assert v.predictor.graph is not None and tuple(v.predictor.static_in.shape) == (4, 3, 320, 320)
    # the same statistics by hand
    p = FusedPredictor(m, conf=0.001, iou=0.7, multi_label=True)
    cm = np.zeros((81, 81), dtype=np.int64)
    ntc, nti, tp, conf, pcls, tcls = np.zeros(80, np.int64), np.zeros(80, np.int64), [], [], [], []
    first = None
    for bt in batches:
        preds = p.predict(bt["img"])
        first = preds if first is None else first
        B = len(preds)
        det = np.zeros((B, 300, 6), dtype=np.float32)
        for i, q in enumerate(preds):
            q = q.cpu()
            scale_boxes((320, 320), q[:, :4], bt["ori_shape"][i], ratio_pad=bt["ratio_pad"][i])
            det[i, :len(q)] = q.numpy()
        counts = [len(q) for q in preds]
        tab = [V.table_row(o, r) for o, r in zip(bt["ori_shape"], bt["ratio_pad"])]
        w = V.run_batch(det, counts, bt["cls"].numpy(), bt["bboxes"].numpy(), bt["batch_idx"].numpy(), tab, (320, 320),
                        80, det_native=True)
        nl = np.bincount(bt["batch_idx"].numpy().astype(int), minlength=B)
        tp.append(V.stats_rows(w["correct"], counts, nl))
        conf += [d[:, 4] for d in w["predn"]]
        pcls += [d[:, 5] for d in w["predn"]]
        tcls.append(bt["cls"].numpy().reshape(-1))
        cm += w["cm"]
        ntc += w["nt_per_class"]
        nti += w["nt_per_image"]
    tp, conf, pcls, tcls = (np.concatenate(x, 0) for x in (tp, conf, pcls, tcls))
    assert len(tp) > 0
    assert np.array_equal(np.concatenate(v.stats.stats["tp"], 0), tp)
    assert np.array_equal(np.concatenate(v.stats.stats["conf"]), conf)
    assert np.array_equal(np.concatenate(v.stats.stats["pred_cls"]), pcls)
    assert np.array_equal(res["confusion_matrix"].matrix, cm.astype(np.float64))
    assert np.array_equal(res["nt_per_class"], ntc) and np.array_equal(res["nt_per_image"], nti) and res["seen"] == 7
    if tp.any():
        ap = ap_per_class(tp, conf, pcls, tcls)[5]
        assert abs(res["metrics/mAP50-95(B)"] - ap.mean()) < 1e-12
    assert abs(res["fitness"] - (0.9 * res["metrics/mAP50(B)"] + 0.1 * res["metrics/mAP50-95(B)"])) < 1e-12
    assert set(res["speed"]) == {"preprocess", "inference", "postprocess"} and res["speed"]["inference"] > 0
    # the EMA of a trainer that took a step (on its own copy of the network) differs from the recipe weights
    from adrefine.data.synthetic import labels
    from adrefine.nn.tasks import DetectionModel
    mt = DetectionModel(str(CFG), compute_dtype=torch.float32)
    load_recipe_into(mt)
    tr = FusedTrainer(mt.cuda(), nbs=4, batch_size=4, ema_decay=0.5, ema_tau=1)
    tr.step({"img": batches[0]["img"].float() / 255, **labels(4, 80, seed=9)})
    v.load_ema(tr)
    ema = tr.ema_state_dict()
    k0 = next(k for k, t in m.state_dict().items() if t.dtype.is_floating_point and t.numel() > 16)
    assert torch.equal(m.state_dict()[k0], ema[k0])
    after = v.predictor.predict(batches[0]["img"])
    assert any(a.shape != b.shape or not torch.equal(a, b) for a, b in zip(after, first))


def test_save_last_and_best_device_trainer(tmp_path):
    """best.pt only on fitness >= best; the stored best round-trips through load_checkpoint (device trainer)."""
    from adrefine.engine import checkpoint as C
    from adrefine.engine.trainer import FusedTrainer
    tr = FusedTrainer(_model().train(), nbs=4, batch_size=4)
    best = C.save_last_and_best(tr, tmp_path, 0, 0.25, None)
    best = C.save_last_and_best(tr, tmp_path, 1, 0.125, best)
    assert best == 0.25 and C.load_checkpoint(tmp_path / "best.pt")["epoch"] == 0
    assert C.load_checkpoint(tmp_path / "last.pt")["best_fitness"] == 0.25
    best = C.save_last_and_best(tr, tmp_path, 2, 0.25, best)
    ck = C.load_checkpoint(tmp_path / "best.pt")
    assert ck["epoch"] == 2 and ck["best_fitness"] == 0.25
