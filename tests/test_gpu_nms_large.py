"""Batched NMS above 16 384 predictions per image (inputs over 864 x 864): adr_nms runs its stages as six plain
launches whose per-(image, class) sort spills from LDS to global memory. The bar is the one of test_gpu_nms.py:
bit-exact against the reference's non_max_suppression (oracle.adr_oracle), the same rows in the same order.

Every case first checks its precondition on the CPU: the candidate scores of each image are pairwise distinct.
The reference cuts to max_nms with an unstable argsort, so only then is its order pinned."""
import numpy as np
import pytest
import torch

from conftest import ROOT
from gpu_util import load_recipe_into
from oracle import adr_oracle as O
from oracle.recipe import synthetic_predictions

pytestmark = pytest.mark.gpu


def _ops():
    from adrefine.utils import ops
    return ops


def _check(out, ref):
    assert len(out) == len(ref)
    for i, (o, r) in enumerate(zip(out, ref)):
        o = o.cpu().numpy()
        r = r.numpy() if isinstance(r, torch.Tensor) else r
        assert o.shape == r.shape, (i, o.shape, r.shape)
        assert np.array_equal(o, r), f"image {i}: first mismatch row {np.argwhere((o != r).any(1))[:1].ravel()}"


def _candidate_counts(pred, conf, multi, classes=None):
    """Candidates per image as the reference forms them; asserts that their scores are pairwise distinct."""
    counts = []
    for x in pred:
        cls = x[4:]  # (nc, na)
        if multi and cls.shape[0] > 1:
            keep = cls > conf
            if classes is not None:
                m = torch.zeros(cls.shape[0], dtype=torch.bool)
                m[list(classes)] = True
                keep &= m[:, None]
            s = cls[keep]
        else:
            s, j = cls.max(0)
            keep = s > conf
            if classes is not None:
                keep &= (j[:, None] == torch.tensor(list(classes))).any(1)
            s = s[keep]
        assert torch.unique(s).numel() == s.numel(), "tied candidate scores: the reference's order is not pinned"
        counts.append(int(s.numel()))
    return counts


CASES = [
    # (bs, na, nc, img, conf, iou, multi, extra kwargs)
    (2, 16385, 1, 896, 0.0, 0.7, False, {}),                       # first A over the LDS limit; fits the LDS sort
    (1, 16464, 80, 896, 0.25, 0.7, False, {}),                     # a real 896^2 grid, 80 small buckets
    (2, 33600, 1, 1280, 1e-6, 0.5, False, {}),                     # one bucket over 16 384, no select
    (2, 33600, 1, 1280, 1e-6, 0.5, False, {"max_nms": 18000}),     # select, then an 18 000-key bucket
    (1, 33600, 2, 1280, 1e-6, 0.6, True, {"max_nms": 40000}),      # two buckets over 16 384
    (1, 33600, 2, 1280, 1e-6, 0.6, True, {}),                      # over 16 384 before the max_nms cut, under it after
    (1, 33600, 2, 1280, 1e-6, 0.45, False, {"agnostic": True}),    # one group holds every candidate
    (1, 33600, 3, 1280, 1e-6, 0.7, False, {"classes": [1], "max_det": 40}),  # class filter and max_det
]


@pytest.mark.parametrize("bs,na,nc,img,conf,iou,multi,kw", CASES)
def test_nms_large_oracle(bs, na, nc, img, conf, iou, multi, kw):
    pred = synthetic_predictions(bs, na, nc, img, seed=na + nc)
    counts = _candidate_counts(pred, conf, multi, kw.get("classes"))
    assert max(counts) > 0
    ref = O.non_max_suppression(pred.clone(), conf, iou, multi_label=multi, **kw)
    out = _ops().non_max_suppression(pred.cuda(), conf, iou, multi_label=multi, **kw)
    print(f"candidates per image {counts}, kept {[len(r) for r in ref]}")
    _check(out, ref)


def test_small_shapes_unchanged():
    """adr_nms_workspace for shapes up to 16 384 predictions returns what it returned before the large path existed.
    The constants were read from the parent commit's library: adr_nms_workspace is host arithmetic and runs without a
    GPU, so `lib.adr_nms_workspace(8, 80, 8400, multi, 300)` was called on a build of that commit."""
    from adrefine.native import lib
    assert int(lib.adr_nms_workspace(8, 80, 8400, 0, 300)) == 47569152
    assert int(lib.adr_nms_workspace(8, 80, 8400, 1, 300)) == 65377024


def test_large_after_captured_small_graph():
    """A FusedPredictor graph captured on the small workspace keeps working after large-A calls replaced that
    workspace with a bigger one: the superseded buffer stays allocated, so the replay writes into memory that is
    still its own and returns what it returned before.

    The (1, 33600, 1) call alone does not outgrow the graph's workspace (0.8 MB against the 2.1 MB that yolo11n's
    80 classes x 2100 anchors take multi-label), so a (1, 33600, 80) multi-label call follows it, which does
    (65 MB); the test asserts that the workspace was replaced."""
    from adrefine.data.synthetic import images_u8
    from adrefine.engine.predictor import FusedPredictor
    from adrefine.nn.tasks import DetectionModel
    ops = _ops()
    m = DetectionModel(str(ROOT / "tests" / "configs" / "yolo11n.yaml"))
    load_recipe_into(m)
    m = m.cuda().eval()
    x = images_u8(1, 320, seed=3).cuda()
    dev = x.device
    if dev in ops._WS:  # start from no workspace; the one earlier tests grew stays referenced
        ops._WS_SUPERSEDED.setdefault(dev, []).append(ops._WS.pop(dev))
    p = FusedPredictor(m, conf=0.001, iou=0.7, multi_label=True)
    p.predict(x)  # eager: the workspace is allocated on the current stream
    p.capture(x)
    before = [t.clone() for t in p.predict(x)]
    assert sum(len(t) for t in before) > 0
    small = ops._WS[dev]
    pred = synthetic_predictions(1, 33600, 1, 1280, seed=33601).cuda()
    out, n = ops.non_max_suppression_padded(pred, 1e-6, 0.5)
    assert int(n[0]) > 0
    pred = synthetic_predictions(1, 33600, 80, 1280, seed=33680).cuda()
    out, n = ops.non_max_suppression_padded(pred, 0.25, 0.7, multi_label=True)
    assert int(n[0]) > 0
    big = ops._WS[dev]
    assert big.numel() > small.numel() and big.data_ptr() != small.data_ptr()
    assert any(t is small for t in ops._WS_SUPERSEDED[x.device])
    junk = torch.full((small.numel(),), 255, dtype=torch.uint8, device=x.device)  # what a freed block would be reused for
    after = p.predict(x)
    assert len(after) == len(before)
    for a, b in zip(after, before):
        assert torch.equal(a, b)
    assert bool((junk == 255).all())
