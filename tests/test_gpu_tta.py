"""GPU: test-time augmentation — adr_tta_views and adr_tta_merge (csrc/adr_tta.hip) against the reference-generated
fixtures and the torch restatements of tests/tta_util.py; DetectionModel.predict(augment=True) against the reference's
model(x, augment=True); FusedPredictor / DetectionValidator with augment=True, eager and as one hipGraph."""
import warnings

import numpy as np
import pytest
import torch

import dataset_util as D
import tta_util as T
from conftest import ROOT, golden
from gpu_util import assert_close, load_recipe_into
from recipe import synthetic_predictions

pytestmark = pytest.mark.gpu
_MODELS = {}


def _model(cfg="yolo11-701-YOLO-AD-Refine.yaml", nc=16, dtype=torch.float32):
    """Recipe-weight eval models, built once per (yaml, nc, compute dtype)."""
    from adrefine.nn.tasks import DetectionModel
    key = (cfg, nc, dtype)
    if key not in _MODELS:
        m = DetectionModel(str(ROOT / "tests" / "configs" / cfg), nc=nc, compute_dtype=dtype)
        load_recipe_into(m)
        _MODELS[key] = m.cuda()
    return _MODELS[key].eval()


def _views_bound(H, W):
    # a few ulps of the blend at values <= 1, plus one ulp of the source coordinate in each axis (should ATen's CPU
    # build contract scale * (dst + 0.5) - 0.5 where adr_tta.hip does not) times a pixel difference <= 1
    return 2.0 ** -21 + max(H, W) * 2.0 ** -22


def _check_views(u8, refs, what):
    from adrefine.utils.tta import tta_plan, tta_views
    B, _, H, W = u8.shape
    plan = tta_plan(H, W)
    for src, tag in ((u8.cuda(), "uint8"), ((u8.float() / 255).cuda(), "fp32")):
        out = tta_views(src, plan)
        assert out[0] is src and len(out) == 3
        for v, ref in zip((1, 2), refs):
            pv, got = plan.views[v], out[v].cpu()
            assert got.dtype == torch.float32 and got.shape == ref.shape == (B, 3, pv.ph, pv.pw)
            pad = np.float32(0.447)
            assert torch.all(got[:, :, pv.rh:, :] == pad) and torch.all(got[:, :, :, pv.rw:] == pad)
            err = float((got[:, :, :pv.rh, :pv.rw].double() - ref[:, :, :pv.rh, :pv.rw].double()).abs().max())
            print(f"{what} view {v} from {tag}: max|err| {err:.3e} (bound {_views_bound(H, W):.3e})")
            assert err <= _views_bound(H, W), (what, v, tag, err)


def test_views_against_the_reference_fixture():
    g = golden("tta_views")
    _check_views(torch.from_numpy(g["u8"]), [torch.from_numpy(g["v1"]), torch.from_numpy(g["v2"])], "tta_views.npz")


def test_views_last_row_and_column_clamp():
    """(1, 3, 33, 47): the last source row and column are the i1 == i0 taps, and the padded width (64 / 32) is not
    the resized width (39 / 31). Reference: the torch restatement on the CPU."""
    u8 = T.u8_images(T.EDGE_SHAPE, T.EDGE_SEED)
    x = u8.float() / 255
    _check_views(u8, [T.view(x, 1), T.view(x, 2)], "edge")


@pytest.mark.parametrize("nc", [3, 1])
def test_merge_bit_exact(nc):
    from adrefine.utils.tta import tta_merge, tta_plan
    plan = tta_plan(256, 320)
    ys = [synthetic_predictions(2, v.anchors, nc, 320, seed=7 + i) for i, v in enumerate(plan.views)]
    ref = T.merge(ys, (256, 320))
    out = tta_merge([y.cuda() for y in ys], plan).cpu()
    assert out.shape == ref.shape == (2, 4 + nc, 3133)
    assert np.array_equal(out.numpy().view(np.uint32), ref.numpy().view(np.uint32))
    a0 = plan.views[0]
    assert torch.equal(out[..., :a0.keep1], ys[0][..., :a0.keep1])  # scale 1: the input's own bits


@pytest.mark.parametrize("flag", [True, False])
def test_ela_rectangular_map(flag):
    """ELA_HSFPN on a 28 x 36 map (P3 of the 224 x 288 view): the build took square maps only, which stack both axis
    means into one batch. Forward, input gradient and parameter gradients in fp32 against the same gate written with
    torch modules on the CPU (block.py:1408-1424: axis means -> shared Conv1d(7) -> GroupNorm(16) -> sigmoid ->
    product), within gpu_util.TOL, the bound of every single-module fp32 test."""
    from adrefine.nn.modules.block import ELA_HSFPN
    from gpu_util import TOL
    m = ELA_HSFPN(128, flag)
    load_recipe_into(m)
    ref = torch.nn.Sequential(torch.nn.Conv1d(128, 128, 7, padding=3), torch.nn.GroupNorm(16, 128), torch.nn.Sigmoid())
    ref.load_state_dict({k.split(".", 1)[1]: v for k, v in m.state_dict().items()})
    gen = torch.Generator().manual_seed(11)
    x0, gy = torch.randn(2, 128, 28, 36, generator=gen), torch.randn(2, 128, 28, 36, generator=gen)
    xr = x0.clone().requires_grad_(True)
    a_h, a_w = ref(xr.mean(3)).unsqueeze(3), ref(xr.mean(2)).unsqueeze(2)
    yr = xr * a_h * a_w if flag else (a_h * a_w).expand_as(xr)
    yr.backward(gy)
    m = m.cuda().train()
    x = x0.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = m(x)
    y.backward(gy.cuda())
    tol = TOL[torch.float32]
    assert_close(y, yr, what="out", **tol)
    assert_close(x.grad, xr.grad, what="dx", **tol)
    for (k, p), q in zip(m.conv1x1.named_parameters(), ref.parameters()):
        assert_close(p.grad, q.grad, what=k, **tol)


@pytest.mark.parametrize("name", list(T.NETS))
def test_predict_augment_against_the_reference(name):
    """model.predict(x, augment=True) in fp32 == the reference's model(x, augment=True), segment by segment: boxes
    within test_gpu_net.py's bound widened by the division by the view's scale, scores within its bound. On a model
    that ignores `augment` the output has A_0 columns, not A_total."""
    from adrefine.utils.tta import tta_plan
    c, g = T.NETS[name], golden(name)
    m = _model(c["cfg"], c["nc"])
    x = T.rect_images(c["B"], c["H"], c["W"], int(g["img_seed"])).cuda()
    with torch.no_grad():
        y, none = m.predict(x, augment=True)
    plan = tta_plan(c["H"], c["W"])
    ref = torch.from_numpy(g["y_aug"])
    assert none is None and tuple(y.shape) == (c["B"], 4 + c["nc"], plan.a_total) == tuple(ref.shape)
    for off, n, s in T.segments(plan):
        a, b = y[..., off:off + n], ref[..., off:off + n]
        assert_close(a[:, :4], b[:, :4], rtol=1e-4, atol=1e-3 / s, what=f"{name} boxes of scale {s}")
        assert_close(a[:, 4:], b[:, 4:], rtol=1e-4, atol=1e-4, what=f"{name} scores of scale {s}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_predict_augment_structure(dtype):
    from adrefine.utils.tta import tta_plan
    m = _model(dtype=dtype)
    x = T.rect_images(2, 256, 320, 4).cuda()
    with torch.no_grad():
        y = m.predict(x)[0]
        ya, none = m.predict(x, augment=True)
        again = m.predict(x, augment=False)[0]
    k = tta_plan(256, 320).views[0].keep1
    assert none is None and ya.dtype == torch.float32 and ya.shape[-1] == 3133 and bool(torch.isfinite(ya).all())
    assert torch.equal(ya[..., :k], y[..., :k]) and torch.equal(again, y)
    try:
        with pytest.raises(RuntimeError, match="augment"):
            m.train().predict(x, augment=True)
    finally:
        m.eval()


def test_predictor_augment_graph_equals_eager():
    from adrefine.data.synthetic import images_u8
    from adrefine.engine.predictor import FusedPredictor
    from adrefine.utils.ops import non_max_suppression_padded
    m = _model()
    x = images_u8(2, 320, seed=3)[:, :, :256].contiguous().cuda()
    x2 = images_u8(2, 320, seed=4)[:, :, :256].contiguous().cuda()
    args = dict(conf=0.001, iou=0.7, multi_label=True)
    p = FusedPredictor(m, augment=True, **args)
    eager = [t.clone() for t in p.run_padded(x)]
    eager2 = [t.clone() for t in p.run_padded(x2)]
    p.capture(x)
    graph = [t.clone() for t in p.run_padded(x)]
    graph2 = [t.clone() for t in p.run_padded(x2)]  # the views are re-rendered inside the graph
    with torch.no_grad():
        y = m.predict(x.float() / 255, augment=True)[0]
        ref = non_max_suppression_padded(y, 0.001, 0.7, None, False, True, 300)
    plain = FusedPredictor(m, **args).run_padded(x)
    for a, b, c in zip(eager, graph, ref):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b in zip(eager2, graph2):
        assert torch.equal(a, b)
    assert int(eager[1].sum()) > 0 and not torch.equal(eager[0], eager2[0])
    assert not (torch.equal(plain[0], eager[0]) and torch.equal(plain[1], eager[1]))  # the switch does something
    # raw images of two sizes through the captured graph: boxes come back inside each source image
    rs = np.random.RandomState(5)
    imgs = [rs.randint(0, 256, (180, 240, 3)).astype(np.uint8), rs.randint(0, 256, (300, 200, 3)).astype(np.uint8)]
    dets = p.predict_images(imgs)
    assert len(dets) == 2
    for d, im in zip(dets, imgs):
        h0, w0 = im.shape[:2]
        assert d.shape[1] == 6 and bool((d[:, :4] >= 0).all())
        assert bool((d[:, [0, 2]] <= w0).all()) and bool((d[:, [1, 3]] <= h0).all())


def test_validator_augment(tmp_path):
    """DetectionValidator(augment=True) on the tiny dataset (its images tiled up to 320): the tallies of the plain run,
    and the metrics of a hand loop of run_padded + update_batched over the same batches."""
    from types import SimpleNamespace

    from adrefine.data.build import build_dataloader, build_yolo_dataset
    from adrefine.engine.predictor import FusedPredictor
    from adrefine.engine.validator import RESULT_KEYS, DetectionValidator
    from adrefine.utils.metrics import DetectionStats
    g = golden("dataset_tiny")
    imgs = {n: np.tile(g[f"native_{n}"], (4, 4, 1)) for n in list(D.SIZES)[:8]}
    tree = str(D.write_tree(tmp_path / "big", imgs))
    nc = 16
    cfg = SimpleNamespace(**vars(D.hyp()), imgsz=320, rect=False, cache="gpu", single_cls=False, task="detect",
                          classes=None, fraction=1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        val = build_yolo_dataset(cfg, tree, 4, {"names": {i: str(i) for i in range(nc)}}, mode="val")
    batches = list(build_dataloader(val, 4, shuffle=False, prefetch=0))
    assert len(batches) == 2
    m = _model()
    res = DetectionValidator(m, nc=nc, augment=True)(batches)
    base = DetectionValidator(m, nc=nc)(batches)
    assert set(RESULT_KEYS) <= set(res) and all(np.isfinite(res[k]) for k in RESULT_KEYS)
    assert res["seen"] == base["seen"] == 8
    assert np.array_equal(res["nt_per_class"], base["nt_per_class"])
    assert np.array_equal(res["nt_per_image"], base["nt_per_image"])
    p = FusedPredictor(m, conf=0.001, iou=0.7, multi_label=True, augment=True)
    st = DetectionStats(nc)
    for bt in batches:
        img = bt["img"].cuda()
        out, n = p.run_padded(img)
        st.update_batched(out, n, bt, imgsz=img.shape[2:], cm_conf=0.001, single_cls=False)
    hand = st.results()
    for k in RESULT_KEYS:
        assert res[k] == hand[k], k
    for k in ("p", "r", "ap", "ap_class_index"):
        assert np.array_equal(res[k], hand[k]), k
    assert np.array_equal(res["confusion_matrix"].matrix, hand["confusion_matrix"].matrix)
