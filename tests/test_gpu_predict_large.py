"""GPU: the inference engine above adr_nms's former limit. yolo11n at 896 x 896 is the smallest square input over it:
12 544 + 3 136 + 784 = 16 464 predictions per image, so the NMS takes its plain-launch path with the spilling sort —
eagerly, captured into the predictor's hipGraph, and under predict_images."""
import numpy as np
import pytest
import torch

from conftest import ROOT
from gpu_util import load_recipe_into

pytestmark = pytest.mark.gpu
S = 896
ARGS = dict(conf=0.001, iou=0.7, multi_label=True)


@pytest.fixture(scope="module")
def model():
    from adrefine.nn.tasks import DetectionModel
    m = DetectionModel(str(ROOT / "tests" / "configs" / "yolo11n.yaml"))
    load_recipe_into(m)
    return m.cuda().eval()


def test_predictor_896_eager_graph_and_plain_nms(model):
    """predict(uint8) eager == captured and replayed twice == non_max_suppression_padded(model(uint8 / 255)), exactly."""
    from adrefine.data.synthetic import images_u8
    from adrefine.engine.predictor import FusedPredictor
    from adrefine.utils.ops import non_max_suppression_padded
    x = images_u8(1, S, seed=5).cuda()
    with torch.no_grad():
        y, _ = model(x.float() / 255)
    assert y.shape[-1] == 16464
    out, n = non_max_suppression_padded(y, ARGS["conf"], ARGS["iou"], multi_label=True)
    ref = [out[i, :k].clone() for i, k in enumerate(n.tolist())]
    assert sum(len(r) for r in ref) > 0
    p = FusedPredictor(model, **ARGS)
    eager = p.predict(x)
    p.capture(x)
    first = p.predict(x)
    second = p.predict(x)
    for got in (eager, first, second):
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            assert a.shape == b.shape and torch.equal(a, b)


def test_predict_images_896(model):
    """One 700 x 500 BGR image at imgsz 896: the boxes lie inside the source image and equal scale_boxes applied to
    the padded result of the letterboxed batch."""
    from adrefine.data.augment import render_letterbox
    from adrefine.data.synthetic import images_u8
    from adrefine.engine.predictor import FusedPredictor
    from adrefine.utils.ops import scale_boxes
    h0, w0 = 500, 700
    img = np.ascontiguousarray(images_u8(1, 704, seed=9).numpy().transpose(0, 2, 3, 1)[0, :h0, :w0])
    p = FusedPredictor(model, **ARGS)
    got = p.predict_images([img], imgsz=S)
    assert len(got) == 1 and len(got[0]) > 0
    batch, _ = render_letterbox([img], (S, S), device="cuda", rgb=True, auto=False)
    out, n = p.run_padded(batch)
    want = out[0, :int(n[0])].clone()
    scale_boxes((S, S), want[:, :4], (h0, w0))
    assert got[0].shape == want.shape and torch.equal(got[0], want)
    b = got[0][:, :4]
    assert float(b.min()) >= 0 and float(b[:, [0, 2]].max()) <= w0 and float(b[:, [1, 3]].max()) <= h0
