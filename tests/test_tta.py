"""CPU: the test-time-augmentation host plan (adrefine/utils/tta.py) against the worked values of the reference's
Python-float arithmetic, and the plain-torch restatements of tests/tta_util.py against the fixtures the reference
produced (scripts/gen_tta_golden.py)."""
import numpy as np
import pytest
import torch

import tta_util as T
from conftest import golden

# (H, W) -> padded view sizes, kept columns per view, A_total
TABLE = {
    (640, 640): (((640, 640), (544, 544), (448, 448)), (8000, 6069, 980), 15049),
    (320, 320): (((320, 320), (288, 288), (224, 224)), (2000, 1701, 245), 3946),
    (256, 320): (((256, 320), (224, 288), (192, 224)), (1600, 1323, 210), 3133),
}


@pytest.mark.parametrize("hw", list(TABLE))
def test_plan_reproduces_the_reference_arithmetic(hw):
    from adrefine.utils.tta import tta_plan
    sizes, kept, total = TABLE[hw]
    p = tta_plan(*hw)
    assert (p.H, p.W) == hw and p.a_total == total
    assert tuple((v.ph, v.pw) for v in p.views) == sizes
    assert tuple(v.keep1 - v.keep0 for v in p.views) == kept
    assert tuple(v.scale for v in p.views) == T.SCALES and tuple(v.flip for v in p.views) == T.FLIPS
    off = 0
    for i, v in enumerate(p.views):
        assert v.out_off == off and 0 <= v.keep0 < v.keep1 <= v.anchors
        assert v.anchors == sum((v.ph // s) * (v.pw // s) for s in (8, 16, 32))
        assert (v.rh, v.rw) == (hw if i == 0 else (int(hw[0] * v.scale), int(hw[1] * v.scale)))
        assert v.rh <= v.ph and v.rw <= v.pw and v.ph % 32 == 0 and v.pw % 32 == 0
        off += v.keep1 - v.keep0
    # view 0 drops its tail, the last view its head, the middle one nothing (tasks.py:385-394)
    assert p.views[0].keep0 == 0 and p.views[0].keep1 == p.views[0].anchors - p.views[0].anchors // 21
    assert (p.views[1].keep0, p.views[1].keep1) == (0, p.views[1].anchors)
    assert p.views[2].keep0 == (p.views[2].anchors // 21) * 16 and p.views[2].keep1 == p.views[2].anchors
    # the same numbers from the torch restatement run on empty-ish tensors
    ys = [torch.zeros(1, 5, v.anchors) for v in p.views]
    assert T.merge(ys, hw).shape[-1] == total


def test_plan_raises_above_the_nms_limit():
    from adrefine.utils.tta import MAX_ANCHORS, tta_plan
    assert MAX_ANCHORS == 16384
    with pytest.raises(NotImplementedError, match="16384"):
        tta_plan(672, 672)
    assert tta_plan(640, 640).a_total <= MAX_ANCHORS


def test_view_restatements_equal_the_reference_fixture():
    g = golden("tta_views")
    u8 = torch.from_numpy(g["u8"])
    assert tuple(u8.shape) == T.VIEWS_SHAPE and torch.equal(u8, T.u8_images(T.VIEWS_SHAPE, T.VIEWS_SEED))
    x = u8.float() / 255
    for v in (1, 2):
        mine, ref = T.view(x, v).numpy(), g[f"v{v}"]
        assert mine.shape == ref.shape and np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), v
    from adrefine.utils.tta import tta_plan
    p = tta_plan(*T.VIEWS_SHAPE[2:])
    for v in (1, 2):
        assert g[f"v{v}"].shape[2:] == (p.views[v].ph, p.views[v].pw)
        assert np.all(g[f"v{v}"][:, :, p.views[v].rh:, :] == np.float32(0.447))
        assert np.all(g[f"v{v}"][:, :, :, p.views[v].rw:] == np.float32(0.447))


@pytest.mark.parametrize("name", list(T.NETS))
def test_net_fixture_segment_layout(name):
    """The fixture's augmented output has the plan's layout, its first segment is the plain output's kept columns
    exactly, and the restatements applied to three per-view outputs (the stored plain one and two seeded stand-ins of
    the views' shapes) give that layout and that first segment."""
    from adrefine.utils.tta import tta_plan
    c, g = T.NETS[name], golden(name)
    y_aug, y = torch.from_numpy(g["y_aug"]), torch.from_numpy(g["y"])
    p = tta_plan(c["H"], c["W"])
    rows = 4 + c["nc"]
    assert tuple(y_aug.shape) == (c["B"], rows, p.a_total) and tuple(y.shape) == (c["B"], rows, p.views[0].anchors)
    a0 = p.views[0].anchors
    assert p.views[0].keep1 == a0 - a0 // 21
    assert torch.equal(y_aug[..., :a0 - a0 // 21], y[..., :a0 - a0 // 21])
    gen = torch.Generator().manual_seed(3)
    ys = [y] + [torch.rand(c["B"], rows, v.anchors, generator=gen) * 100 for v in p.views[1:]]
    cat = T.merge(ys, (c["H"], c["W"]))
    assert cat.shape == y_aug.shape
    for (off, n, s), v, yi in zip(T.segments(p), p.views, ys):
        seg = cat[..., off:off + n]
        assert torch.equal(seg[:, 4:], yi[:, 4:, v.keep0:v.keep1])
        box = yi[:, :4, v.keep0:v.keep1] / s
        if v.flip == 3:
            box[:, 0] = c["W"] - box[:, 0]
        assert torch.equal(seg[:, :4], box)
    assert torch.equal(cat[..., :p.views[0].keep1], y_aug[..., :p.views[0].keep1])
    # the de-scaled, de-flipped boxes of the other views land in and around the base image
    for (off, n, s), v in list(zip(T.segments(p), p.views))[1:]:
        cx, cy = y_aug[:, 0, off:off + n], y_aug[:, 1, off:off + n]
        assert float(cx.min()) > -c["W"] and float(cx.max()) < 2 * c["W"]
        assert float(cy.min()) > -c["H"] and float(cy.max()) < 2 * c["H"]
