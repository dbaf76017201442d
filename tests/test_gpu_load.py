"""DetectionModel.load on the GPU (yolo11n, bf16, 128 x 128, batch 2): a trainer built after the load trains on the
loaded weights, and a FusedPredictor built before it never predicts with the old packed / folded weights."""
import pytest
import torch

from conftest import ROOT
from gpu_util import load_recipe_into
from recipe import synthetic_images, synthetic_labels

pytestmark = pytest.mark.gpu
CFG = ROOT / "tests" / "configs" / "yolo11n.yaml"
IMG = 128


def _model():
    from adrefine.nn.tasks import DetectionModel
    m = DetectionModel(str(CFG), compute_dtype=torch.bfloat16)
    load_recipe_into(m)
    return m.cuda()


def _other_weights(seed):
    """The state of a model whose floating entries were scaled at random: another set of weights of the same keys."""
    m = _model()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for t in m.state_dict().values():
            if t.is_floating_point():
                t.mul_(1 + 0.3 * torch.rand(t.shape, generator=g).cuda())
    return m


def test_load_then_train_uses_the_loaded_weights(tmp_path):
    from adrefine.engine import checkpoint as C
    from adrefine.engine.trainer import FusedTrainer
    f = tmp_path / "pre.pt"
    C.save_checkpoint(FusedTrainer(_other_weights(5), nbs=2, batch_size=2), f, epoch=0)  # the EMA starts as the model
    ema = C.load_checkpoint(f)["ema"]
    batch = {"img": synthetic_images(2, IMG, seed=0).cuda(), **synthetic_labels(2, 20, seed=1)}

    def one_step(prepare):
        m = _model()
        prepare(m)
        items = FusedTrainer(m, nbs=2, batch_size=2).step(batch).clone()
        torch.cuda.synchronize()
        return items, m.state_dict()

    fresh, _ = one_step(lambda m: None)
    loaded, s1 = one_step(lambda m: m.load(f))
    direct, s2 = one_step(lambda m: m.load_state_dict({k: v.float() if v.is_floating_point() else v
                                                       for k, v in ema.items()}))
    assert bool(torch.isfinite(loaded).all()) and not torch.equal(loaded, fresh)
    assert torch.equal(loaded, direct) and all(torch.equal(s1[k], s2[k]) for k in s1)


def test_load_after_a_predictor_invalidates_it():
    """A FusedPredictor caches packed bf16 operands and folded eval BatchNorm coefficients, and its graph reads
    them: DetectionModel.load refreshes them in place, so the next predict equals a predictor built after the load."""
    from adrefine.engine.predictor import FusedPredictor
    img = (synthetic_images(2, IMG, seed=3) * 255).round().to(torch.uint8).cuda()
    sd = {k: v.clone() for k, v in _other_weights(9).state_dict().items()}
    m = _model().eval()
    pred = FusedPredictor(m, conf=0.001, max_det=50)
    old = [t.clone() for t in pred.run_padded(img)[:2]]
    pred.capture(img)
    assert pred.packs.specs and pred.packs.bn_coefs
    m.load(sd)
    new = [t.clone() for t in pred.run_padded(img)[:2]]  # the captured graph, on the refreshed buffers
    assert pred.graph is not None
    m2 = _model().eval()
    m2.load_state_dict(sd)
    want = [t.clone() for t in FusedPredictor(m2, conf=0.001, max_det=50).run_padded(img)[:2]]
    torch.cuda.synchronize()
    assert torch.equal(new[1], want[1]) and int(new[1].sum()) > 0
    rows = lambda out, n: [out[i, :int(k)] for i, k in enumerate(n.tolist())]  # noqa: E731 - the valid rows
    assert all(torch.equal(x, y) for x, y in zip(rows(*new), rows(*want)))
    assert not (torch.equal(new[1], old[1]) and all(torch.equal(x, y) for x, y in zip(rows(*new), rows(*old))))
