"""GPU: validation losses — FusedPredictor(keep_feats=True) keeps the eval forward's level maps, and
DetectionValidator(compute_loss=True) turns them into val/box_loss, val/cls_loss, val/dfl_loss, against a hand loop
and against the reference's numbers (tests/golden/val_loss.npz, scripts/gen_valloss_golden.py)."""
import functools

import pytest
import torch

from conftest import ROOT, golden
from gpu_util import assert_close, load_recipe_into

pytestmark = pytest.mark.gpu

CFGS = {"n701": "yolo11-701-YOLO-AD-Refine.yaml", "y11n": "yolo11n.yaml"}
LOSS_KEYS = ("val/box_loss", "val/cls_loss", "val/dfl_loss")


def _model(tag, nc):
    from adrefine.nn.tasks import DetectionModel
    m = DetectionModel(str(ROOT / "tests" / "configs" / CFGS[tag]), nc=nc, compute_dtype=torch.float32)
    for mm in m.modules():
        if isinstance(mm, torch.nn.Dropout):
            mm.p = 0.0
    load_recipe_into(m)
    return m.cuda().eval()


def _batches(tag):
    g = golden("val_loss")
    H, W = (int(v) for v in g[f"{tag}_imgsz"])
    out = []
    for k in range(int(g["nbatches"])):
        B = g[f"{tag}_b{k}_img"].shape[0]
        out.append({"img": torch.from_numpy(g[f"{tag}_b{k}_img"]).cuda(),
                    **{key: torch.from_numpy(g[f"b{k}_{key}"]) for key in ("batch_idx", "cls", "bboxes")},
                    "ori_shape": [(H, W)] * B, "ratio_pad": [((1.0, 1.0), (0, 0))] * B})
    return out, int(g["nc"])


@functools.lru_cache(maxsize=None)
def _validated(tag):
    """(results with compute_loss, results without, hand-loop mean) — computed once per model."""
    from adrefine.engine.validator import DetectionValidator
    batches, nc = _batches(tag)
    model = _model(tag, nc)
    with_loss = DetectionValidator(model, nc, compute_loss=True)(batches)
    plain = DetectionValidator(model, nc)(batches)
    # the hand loop: the criterion WITH gradients on model(img), summed in fp32 in batch order, / number of batches
    crit = model.init_criterion()
    total = torch.zeros(3, dtype=torch.float32, device="cuda")
    for b in batches:
        preds = model(b["img"])
        assert all(f.requires_grad for f in preds[1])
        loss, items = crit(preds, b)
        assert loss.grad_fn is not None
        total += items
    hand = (total.cpu() / len(batches))
    return with_loss, plain, hand


@pytest.mark.parametrize("tag", ["y11n", "n701"])
def test_keep_feats_maps_and_detections(tag):
    from adrefine.engine.predictor import FusedPredictor
    batches, nc = _batches(tag)
    model = _model(tag, nc)
    img = batches[0]["img"]
    with torch.no_grad():
        want = [f.clone() for f in model(img)[1]]
    base = FusedPredictor(model, conf=0.001, multi_label=True)
    out0, n0 = (t.clone() for t in base.run_padded(img))
    keep = FusedPredictor(model, conf=0.001, multi_label=True, keep_feats=True)
    out, n, feats = keep.run_padded(img)  # eager
    assert len(feats) == 3 and all(torch.equal(a, b) for a, b in zip(feats, want))
    assert torch.equal(out, out0) and torch.equal(n, n0)
    keep.capture(img)
    other = batches[1]["img"]
    keep.run_padded(other)
    out, n, feats = keep.run_padded(img)  # replayed; the static maps are rewritten in place
    assert all(f is s for f, s in zip(feats, keep.static_feats))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(feats, want))
    assert torch.equal(out, out0) and torch.equal(n, n0)
    assert base.feats is None and base.static_feats is None


@pytest.mark.parametrize("tag", ["y11n", "n701"])
def test_validator_losses_equal_hand_loop(tag):
    with_loss, _, hand = _validated(tag)
    got = torch.tensor([with_loss[k] for k in LOSS_KEYS], dtype=torch.float32)
    print(f"[val-loss] {tag}: validator {got.tolist()} hand loop {hand.tolist()}")
    assert torch.equal(got, hand)


@pytest.mark.parametrize("tag", ["y11n", "n701"])
def test_validator_losses_vs_reference(tag):
    """fp32 against the reference's CPU fp32 values, at the tolerance
    tests/test_gpu_loss.py::test_network_train_step_loss_and_grads applies to loss items (rtol 1e-4, atol 1e-5)."""
    with_loss, _, _ = _validated(tag)
    g = golden("val_loss")
    got = torch.tensor([with_loss[k] for k in LOSS_KEYS], dtype=torch.float32)
    ref = torch.from_numpy(g[f"{tag}_mean"])
    rel = ((got - ref).abs() / ref.abs().clamp_min(1e-30)).tolist()
    print(f"[val-loss] {tag}: validator {got.tolist()} reference {ref.tolist()} rel {rel}")
    assert_close(got, g[f"{tag}_mean"], rtol=1e-4, atol=1e-5, what="val losses")


@pytest.mark.parametrize("tag", ["y11n", "n701"])
def test_other_results_unchanged(tag):
    with_loss, plain, _ = _validated(tag)
    assert set(with_loss) - set(plain) == set(LOSS_KEYS)
    for k, v in plain.items():
        if k == "speed":  # timings differ run to run; the loss has a slot of its own, the others keep their meaning
            assert set(with_loss[k]) - set(v) == {"loss"} and with_loss[k]["loss"] > 0
            continue
        w = with_loss[k]
        if hasattr(v, "matrix"):
            assert (v.matrix == w.matrix).all()
        elif hasattr(v, "shape"):
            assert v.shape == w.shape and (v == w).all(), k
        else:
            assert v == w, k


def test_incompatible_flags():
    from adrefine.engine.predictor import FusedPredictor
    from adrefine.engine.validator import DetectionValidator
    with pytest.raises(ValueError):
        DetectionValidator(torch.nn.Identity(), 16, augment=True, compute_loss=True)
    with pytest.raises(ValueError):
        FusedPredictor(torch.nn.Identity(), augment=True, keep_feats=True)
