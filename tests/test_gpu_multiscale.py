"""Multi-scale training (FusedTrainer(multi_scale=True), reference models/yolo/detect/train.py:57-74): the fused
uint8 -> resized fp32 kernel adr_multiscale_u8 against torch, its argument checks, and the trainer's steps against
twins fed the resized batch by hand — eagerly, at a 1:1 draw, and through graphs captured per image shape.

Kernel criterion. r32 / r64 are F.interpolate(u8 / 255, bilinear, align_corners=False) by torch on the CPU in fp32 and
fp64 from the same uint8 data, k the kernel's output: max|k - r64| <= max|r32 - r64| + 2^-22. Values lie in [0, 1];
the slack is eight half-ulp roundings at 1.0 (the kernel's seven arithmetic roundings and the /255), the first term
torch-fp32's own distance from fp64 on that input. Bit equality with CPU torch is not asked (it divides by 255, the
device multiplies by fp32(1/255)). The same bound holds for max|k - d| against torch's F.interpolate on the device.

Trainer criterion. The multi_scale trainer and a multi_scale=False twin fed multi_scale_resize(img, shape) and the
same labels run the same code on the same bits; the baseline is run twice and the spread between its two runs is what
the multi_scale trainer may differ by — no more. On the MI355X that spread is ZERO at these shapes (192, 288 and 256
at batch 2; printed by the fixture), so the assertions below are bitwise equality."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from gpu_util import load_recipe_into
from recipe import synthetic_images, synthetic_labels

pytestmark = pytest.mark.gpu
CFG = ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"

# (source H x W) -> (oh x ow)
CASES = [((64, 64), (32, 32)),    # exact 2:1, every weight 0.5
         ((64, 64), (96, 96)),    # upsampling, border clamp on both edges
         ((40, 72), (64, 96)),    # non-square, both axes differ
         ((64, 64), (33, 64)),    # oh a multiple of nothing
         ((64, 64), (33, 50)),    # ow % 4 == 2: every other row starts off a 16-byte boundary (head and tail stores)
         ((37, 53), (35, 67)),    # ow odd: all four row alignments
         ((24, 300), (5, 331)),   # more than 64 column groups per row: two blocks along x; oh % 4 != 0
         ((37, 53), (3, 1)),      # one output column
         ((1, 1), (4, 4))]        # degenerate clamp


def _inputs(H, W):
    """B = 2 (a wrong batch stride shows): random bytes, and a horizontal ramp in image 0 / a vertical one in image 1."""
    g = torch.Generator().manual_seed(H * 1000 + W)
    rnd = torch.randint(0, 256, (2, 3, H, W), generator=g, dtype=torch.uint8)
    hr = torch.linspace(0, 255, W).round().to(torch.uint8).view(1, 1, W).expand(3, H, W)
    vr = torch.linspace(0, 255, H).round().to(torch.uint8).view(1, H, 1).expand(3, H, W)
    return {"random": rnd, "ramps": torch.stack((hr, vr)).contiguous()}


def _interp(x, size):
    return F.interpolate(x / 255, size=size, mode="bilinear", align_corners=False)


@pytest.mark.parametrize("src,dst", CASES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in CASES])
def test_kernel_matches_torch(src, dst):
    from adrefine import kernels as K
    for what, u8 in _inputs(*src).items():
        r32, r64 = _interp(u8.float(), dst), _interp(u8.double(), dst)
        dev = u8.cuda()
        k = K.multi_scale_resize(dev, dst)
        d = _interp(dev.float(), dst)
        torch.cuda.synchronize()
        assert k.shape == (2, 3, *dst) and k.dtype == torch.float32 and k.is_contiguous()
        k, d = k.cpu(), d.cpu()
        bound = float((r32.double() - r64).abs().max()) + 2.0 ** -22
        ek = float((k.double() - r64).abs().max())
        ed = float((k - d).abs().max())
        print(f"{src}->{dst} {what}: |k - r64| {ek:.3e}, |k - device torch| {ed:.3e}, bound {bound:.3e}")
        assert ek <= bound, (what, ek, bound)
        assert ed <= bound, (what, ed, bound)


@pytest.mark.parametrize("ow", [48, 50])
@pytest.mark.parametrize("mis", [1, 2, 3])
def test_kernel_output_off_a_16_byte_boundary(mis, ow):
    """The entry writes through an output pointer that is 4- but not 16-byte aligned: the same bits as into an
    aligned buffer, and not one element before or after the batch."""
    from adrefine import kernels as K
    from adrefine.native import lib
    u8 = _inputs(40, 72)["random"].cuda()
    want = K.multi_scale_resize(u8, (33, ow))
    n = want.numel()
    buf = torch.full((n + 8,), 7.0, device="cuda")
    lib.adr_multiscale_u8(K.fptr(u8), 2, 40, 72, K.fptr(buf[mis:]), 33, ow, K.stream())
    torch.cuda.synchronize()
    assert torch.equal(buf[mis:mis + n].view_as(want), want)
    assert bool((buf[:mis] == 7.0).all()) and bool((buf[mis + n:] == 7.0).all())


def test_entry_checks_arguments():
    from adrefine import kernels as K
    from adrefine.native import lib
    img = torch.zeros(1, 3, 4, 4, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, 3, 8, 8, device="cuda")
    i, o = K.fptr(img), K.fptr(out)
    for args in ((None, 1, 4, 4, o, 8, 8), (i, 1, 4, 4, None, 8, 8), (i, 1, 4, 4, o, 0, 8), (i, 1, 4, 4, o, 8, 0),
                 (i, 0, 4, 4, o, 8, 8), (i, 1, 0, 4, o, 8, 8), (i, 1, 4, -1, o, 8, 8)):
        with pytest.raises(RuntimeError, match="adr_multiscale_u8"):
            lib.adr_multiscale_u8(*args, K.stream())
    assert not out.any()
    with pytest.raises(RuntimeError, match="uint8"):
        K.multi_scale_resize(img.float(), (8, 8))


# ---- trainer -------------------------------------------------------------------------------------------------

IMGSZ = 256
# randrange results -> // 32 * 32: 192 (down), 288 (up), 256 (1:1), 192, 288
DRAWS = [200, 300, 256, 210, 319]
SHAPES = [(192, 192), (288, 288), None, (192, 192), (288, 288)]


class _Draws:
    """A `random`-like source of fixed randrange results; records the bounds it was asked for."""

    def __init__(self, vals):
        self.vals, self.calls = list(vals), []

    def randrange(self, a, b):
        self.calls.append((a, b))
        return self.vals.pop(0)


def _trainer(**kw):
    from adrefine.engine.trainer import FusedTrainer
    from adrefine.nn.tasks import DetectionModel
    m = DetectionModel(str(CFG))
    load_recipe_into(m)
    return FusedTrainer(m.cuda(), nbs=2, batch_size=2, **kw)


def _batch(seed):
    img = (synthetic_images(2, IMGSZ, seed=seed) * 255).round().to(torch.uint8)
    return {"img": img.cuda(), **synthetic_labels(2, 80, seed=seed + 1)}


def _batches():
    return [_batch(s) for s in (0, 5, 9, 5, 0)]


def _resized(batch, shape):
    """What a multi_scale=False twin is fed for a draw of `shape`: the kernel's fp32 image and the same labels."""
    from adrefine import kernels as K
    if shape is None:
        return batch
    return {**batch, "img": K.multi_scale_resize(batch["img"], shape)}


def _names(tr):
    """One parameter that receives a gradient per optimizer group."""
    from adrefine.engine.trainer import param_groups
    return [next(n for n, p in g if getattr(p, "_adr_used", False)) for g in param_groups(tr.model)]


def _snap(tr, items, names):
    sd, ema = dict(tr.model.named_parameters()), tr.ema_state_dict()
    return {"items": items.clone(), "p": {n: sd[n].detach().clone() for n in names},
            "ema": {n: ema[n].clone() for n in names}}


def _watch(tr):
    """Record (dtype, shape, gt) of every batch the trainer's eager forward/backward is given."""
    seen, fb = [], tr.forward_backward

    def forward_backward(batch, after_stage=None):
        seen.append((batch["img"].dtype, tuple(batch["img"].shape), batch.get("gt")))
        return fb(batch, after_stage)

    tr.forward_backward = forward_backward
    return seen


def _final(tr):
    return ({k: v.detach().clone() for k, v in tr.model.state_dict().items() if v.dtype.is_floating_point},
            {k: v.clone() for k, v in tr.ema_state_dict().items()})


def _maxdiff(a, b):
    return max(float((a[k] - b[k]).abs().max()) for k in a)


@pytest.fixture(scope="module")
def runs():
    """Five steps (draws 192, 288, 1:1, 192, 288) of: the baseline twice (multi_scale=False, fed the resized batch by
    hand), the eager multi_scale trainer, and a multi_scale trainer that captures 288 x 288 after its first step."""
    batches = _batches()
    out = {}
    for tag in ("base1", "base2"):
        tr = _trainer()
        snaps, names = [], None
        for b, shape in zip(batches, SHAPES):
            items = tr.step(_resized(b, shape))
            names = names or _names(tr)
            snaps.append(_snap(tr, items, names))
        torch.cuda.synchronize()
        out[tag] = {"snaps": snaps, "final": _final(tr)}
    for tag in ("eager", "graph"):
        rng = _Draws(DRAWS)
        tr = _trainer(multi_scale=True, imgsz=IMGSZ, rng=rng)
        seen = _watch(tr)
        snaps, eager_calls, keys = [], [], []
        for i, b in enumerate(batches):
            n0 = len(seen)
            items = tr.step(b)
            eager_calls.append(len(seen) - n0)
            keys.append(tr._key)
            snaps.append(_snap(tr, items, _names(tr)))
            if tag == "graph" and i == 0:
                tr.capture(batches[1], size=(288, 288))
                seen.clear()
        torch.cuda.synchronize()
        out[tag] = {"snaps": snaps, "final": _final(tr), "seen": list(seen), "eager_calls": eager_calls, "keys": keys,
                    "rng": rng, "shapes": [k[0] for k in list(tr._other) + [tr._key] if k is not None]}
    spread = []
    for s1, s2 in zip(out["base1"]["snaps"], out["base2"]["snaps"]):
        spread.append({"items": float((s1["items"] - s2["items"]).abs().max()), "p": _maxdiff(s1["p"], s2["p"]),
                       "ema": _maxdiff(s1["ema"], s2["ema"])})
    out["spread"] = spread
    print("baseline run-to-run spread per step:", spread)
    return out


def test_trainer_eager_matches_resized_twin(runs):
    """Steps 0 (192, down) and 1 (288, up), and the later 192 / 288 steps: loss items, one parameter per group and
    their EMA entries differ from the hand-fed baseline by no more than the baseline's own two runs differ (zero on
    the MI355X: bitwise). The draws ask for randrange(imgsz * 0.5, imgsz * 1.5 + stride), once per step."""
    e, b = runs["eager"], runs["base1"]
    assert e["rng"].calls == [(128, 416)] * 5 and not e["rng"].vals
    assert e["eager_calls"] == [1] * 5
    for i in (0, 1, 3, 4):
        se, sb, sp = e["snaps"][i], b["snaps"][i], runs["spread"][i]
        d = {"items": float((se["items"] - sb["items"]).abs().max()), "p": _maxdiff(se["p"], sb["p"]),
             "ema": _maxdiff(se["ema"], sb["ema"])}
        print(f"step {i}: multi_scale vs baseline {d}, baseline spread {sp}")
        for k in d:
            assert d[k] <= sp[k], (i, k, d[k], sp[k])
    assert len(e["snaps"][0]["p"]) == 3
    assert not torch.equal(e["snaps"][0]["items"], e["snaps"][1]["items"])


def test_trainer_builds_gt_at_the_new_size(runs):
    """The prepared gt is the normalised boxes times (ow, oh) of the RESIZED image: rows [cls, x1, y1, x2, y2]."""
    seen = runs["eager"]["seen"]
    for (dtype, shape, gt), b, want in zip(seen, _batches(), SHAPES):
        oh, ow = want or (IMGSZ, IMGSZ)
        assert shape == (2, 3, oh, ow)
        assert dtype == (torch.uint8 if want is None else torch.float32)
        xywh = b["bboxes"].numpy().astype(np.float32) * np.array([ow, oh, ow, oh], dtype=np.float32)
        rows = np.concatenate((b["cls"].numpy().reshape(-1, 1).astype(np.float32), xywh[:, :2] - xywh[:, 2:] / 2,
                               xywh[:, :2] + xywh[:, 2:] / 2), 1)
        gt = gt.cpu().numpy()
        bi = b["batch_idx"].numpy().astype(np.int64)
        for j in range(2):
            mine = rows[bi == j]
            assert np.array_equal(gt[j, :len(mine)], mine) and not gt[j, len(mine):].any()


def test_one_to_one_draw_keeps_the_uint8_path(runs):
    """Draw 256 at imgsz 256: no resample, the model is given the uint8 batch, the step is the baseline's."""
    e, b, sp = runs["eager"], runs["base1"], runs["spread"][2]
    assert e["seen"][2][0] == torch.uint8 and e["seen"][2][1] == (2, 3, IMGSZ, IMGSZ)
    se, sb = e["snaps"][2], b["snaps"][2]
    assert float((se["items"] - sb["items"]).abs().max()) <= sp["items"]
    assert _maxdiff(se["p"], sb["p"]) <= sp["p"] and _maxdiff(se["ema"], sb["ema"]) <= sp["ema"]


def test_graph_replays_captured_shape_and_runs_others_eagerly(runs):
    """capture(batch, size=(288, 288)) after one eager step: the steps that draw 288 replay (no eager forward), the
    steps that draw 192 or 1:1 have no captured set and run eagerly; every step matches the eager multi_scale twin
    under tests/test_gpu_graph.py's criterion (10 x the eager-eager spread + 2e-4)."""
    g, e = runs["graph"], runs["eager"]
    assert g["eager_calls"] == [1, 0, 1, 1, 0]
    assert g["keys"][1:] == [((2, 3, 288, 288), torch.float32)] * 4 and g["shapes"] == [(2, 3, 288, 288)]
    assert g["rng"].calls == [(128, 416)] * 5  # capture(size=...) draws nothing
    for i, (sg, se) in enumerate(zip(g["snaps"], e["snaps"])):
        a, b = se["items"], sg["items"]
        d = float((a - b).abs().max())
        print(f"step {i}: graph-trainer vs eager items {d:.3e}")
        assert d <= 10 * runs["spread"][i]["items"] + 2e-4 * float(a.abs().max()), (i, a, b)
    spread = _maxdiff(runs["base1"]["final"][0], runs["base2"]["final"][0])
    d = _maxdiff(e["final"][0], g["final"][0])
    de = _maxdiff(e["final"][1], g["final"][1])
    print(f"eager-eager max |dparam| {spread:.3e}, eager-graph {d:.3e}, EMA {de:.3e}")
    assert d <= 10 * spread + 2e-4 and de <= 10 * spread + 2e-4


def test_graph_shapes_evicts_least_recently_used():
    """graph_shapes=1: capturing 192 x 192 evicts the 288 x 288 set; a later 288 draw runs eagerly, a 192 draw
    replays. With graph_shapes=2 both stay."""
    b = _batch(0)
    k288, k192 = ((2, 3, 288, 288), torch.float32), ((2, 3, 192, 192), torch.float32)
    for keep in (1, 2):
        tr = _trainer(multi_scale=True, imgsz=IMGSZ, rng=_Draws([256, 300, 200]), graph_shapes=keep)
        seen = _watch(tr)
        tr.step(b)
        tr.capture(b, size=(288, 288))
        assert tr._key == k288 and not tr._other
        tr.capture(b, size=(192, 192))
        assert tr._key == k192 and list(tr._other) == ([] if keep == 1 else [k288])
        seen.clear()
        tr.step(b)  # 288
        assert len(seen) == (1 if keep == 1 else 0) and tr._key == (k192 if keep == 1 else k288)
        tr.step(b)  # 192
        assert len(seen) == (1 if keep == 1 else 0) and tr._key == k192
        torch.cuda.synchronize()


def test_prebuilt_gt_with_multi_scale_raises():
    from adrefine.utils.loss import preprocess_targets
    b = _batch(0)
    gt = preprocess_targets(b["batch_idx"], b["cls"], b["bboxes"], 2, (IMGSZ, IMGSZ))
    rng = _Draws([200])
    tr = _trainer(multi_scale=True, imgsz=IMGSZ, rng=rng)
    with pytest.raises(ValueError, match="gt"):
        tr.step({"img": b["img"], "gt": gt})
    assert rng.calls == [] and tr.ni == 0
