"""Transfer learning, host side: utils.torch_utils.intersect_dicts, DetectionModel.load from every accepted form
(the reference's nn/tasks.py:275-288 and utils/torch_utils.py:470-472) and cfg.pretrained in engine.fit
(models/yolo/detect/train.py:86-91). CPU only: models and trainers are built without running a step; the yardstick
is plain dict logic in torch."""
import copy
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

CFG = ROOT / "tests" / "configs" / "yolo11n.yaml"


def _model(nc, seed, cfg=CFG):
    from adrefine.nn.tasks import DetectionModel
    m = DetectionModel(str(cfg), nc=nc)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for t in m.state_dict().values():
            if t.is_floating_point():
                t.copy_(torch.randn(t.shape, generator=g) * 0.1 + 0.5)
    return m


@pytest.fixture(scope="module")
def src80():
    return _model(80, 1)


def _snapshot(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


# ---- intersect_dicts ---------------------------------------------------------------------------------------------

def test_intersect_dicts():
    from adrefine.utils.torch_utils import intersect_dicts
    da = {"a.w": torch.ones(2, 3), "b.w": torch.ones(4), "c.anchor": torch.ones(5), "d.w": torch.ones(1),
          "e.w": torch.ones(3, 2)}
    db = {"a.w": torch.zeros(2, 3), "b.w": torch.zeros(5), "c.anchor": torch.zeros(5), "e.w": torch.zeros(2, 3),
          "f.w": torch.zeros(1)}
    out = intersect_dicts(da, db)
    assert list(out) == ["a.w", "c.anchor"]  # b.w, e.w: shape differs (same numel is not enough); d.w: not in db
    assert all(out[k] is da[k] for k in out)  # values come from the first dict
    assert list(intersect_dicts(da, db, exclude=("anchor",))) == ["a.w"]
    assert list(intersect_dicts(da, db, exclude=("anchor", "a."))) == []
    assert intersect_dicts({}, db) == {} and intersect_dicts(da, {}) == {}


# ---- DetectionModel.load -----------------------------------------------------------------------------------------

def _expect(src_sd, own):
    """What load must transfer, by plain dict logic: same key, same shape."""
    return [k for k, v in src_sd.items() if k in own and tuple(v.shape) == tuple(own[k].shape)]


def _check_loaded(m, before, src_sd, counts):
    own = m.state_dict()
    moved = _expect(src_sd, before)
    assert counts == (len(moved), len(own))
    for k, v in own.items():
        if k in moved:
            want = src_sd[k].float() if src_sd[k].is_floating_point() else src_sd[k]
            assert v.dtype == before[k].dtype and torch.equal(v.float(), want.float()), k
        else:
            assert torch.equal(v, before[k]), k  # untouched, bitwise
    return moved


def test_load_state_dict_same_nc(src80):
    m = _model(80, 2)
    before = _snapshot(m)
    sd = src80.state_dict()
    moved = _check_loaded(m, before, sd, m.load(sd))
    assert len(moved) == len(sd)  # every entry, buffers included


def test_load_other_nc_keeps_class_tensors(src80):
    """An nc=80 checkpoint into an nc=3 model: everything but the tensors shaped by nc, which stay bitwise."""
    m = _model(3, 2)
    before = _snapshot(m)
    sd = src80.state_dict()
    moved = _check_loaded(m, before, sd, m.load(sd))
    kept = sorted(set(before) - set(moved))
    assert kept and all(".cv3." in k for k in kept), kept  # the class branch of the head
    # exactly the tensors whose shape follows nc (the class branch's width is max(ch[0], min(nc, 100)) too)
    assert all(tuple(sd[k].shape) != tuple(before[k].shape) for k in kept)
    assert any(tuple(before[k].shape)[0] == 3 and tuple(sd[k].shape)[0] == 80 for k in kept)
    assert len(moved) == len(sd) - len(kept)
    assert any(k.startswith(f"model.{len(m.model) - 1}.cv2.") for k in moved)  # the box branch does transfer


def test_load_checkpoint_dict_ema_then_model(src80):
    sd = {k: (v.half() if v.is_floating_point() else v.clone()) for k, v in src80.state_dict().items()}
    other = {k: torch.zeros_like(v) for k, v in sd.items()}
    m = _model(80, 3)
    before = _snapshot(m)
    _check_loaded(m, before, sd, m.load({"epoch": 3, "model": other, "ema": sd, "optimizer": None}))
    assert all(v.dtype == before[k].dtype for k, v in m.state_dict().items())  # fp16 in the file, fp32 in the model
    m = _model(80, 3)
    _check_loaded(m, _snapshot(m), sd, m.load({"epoch": 3, "model": sd, "ema": None}))  # 'ema' None: 'model'
    m = _model(80, 3)
    _check_loaded(m, _snapshot(m), src80.state_dict(), m.load({"ema": src80}))  # an entry that is a module


def test_load_module_leaves_the_source_alone(src80):
    half = copy.deepcopy(src80).half()
    m = _model(3, 4)
    before = _snapshot(m)
    want = {k: v.clone() for k, v in half.state_dict().items()}
    _check_loaded(m, before, want, m.load(half))
    assert all(v.dtype == want[k].dtype for k, v in half.state_dict().items())


def test_load_path_of_own_checkpoint(tmp_path):
    """A file written by checkpoint.save_checkpoint (fp16 EMA state_dict, weights_only) loads by its path."""
    from adrefine.engine import checkpoint as C
    from adrefine.engine.trainer import FusedTrainer
    src = _model(80, 5)
    tr = FusedTrainer(src, batch_size=16)
    f = tmp_path / "last.pt"
    C.save_checkpoint(tr, f, epoch=0)
    ema = torch.load(f, map_location="cpu", weights_only=True)["ema"]
    for as_path in (f, str(f)):
        m = _model(3, 6)
        _check_loaded(m, _snapshot(m), ema, m.load(as_path))


def test_load_rejects_what_it_cannot_read(tmp_path):
    m = _model(3, 7)
    for bad in (None, 3, [torch.zeros(1)], {}, {"epoch": 1}, {"ema": None, "model": None}, {"a": 1}):
        with pytest.raises(TypeError, match="state_dict"):
            m.load(bad)
    f = tmp_path / "pickled.pt"
    torch.save({"model": SimpleNamespace(x=1)}, f)  # a file that pickles a class, as the reference's .pt files do
    with pytest.raises(TypeError, match="state_dict"):
        m.load(f)


def test_load_under_a_live_trainer_raises(src80):
    from adrefine.engine.trainer import FusedTrainer
    m = _model(80, 8)
    before = _snapshot(m)
    tr = FusedTrainer(m, batch_size=16)
    with pytest.raises(RuntimeError, match="FusedTrainer"):
        m.load(src80.state_dict())
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())  # refused before anything moved
    assert tr is not None
    twin = copy.deepcopy(m)  # a copy (the validator's) is not the trainer's model
    assert twin.load(src80.state_dict())[0] == len(before)


# ---- fit ---------------------------------------------------------------------------------------------------------

class _Loader:
    def __len__(self):
        return 1

    def __iter__(self):
        return iter([{"k": 0}])

    def reset(self):
        pass


class _Set:
    def __len__(self):
        return 2


def test_fit_loads_pretrained_before_anything_copies_the_model(tmp_path, monkeypatch, src80):
    import adrefine.engine.trainer as T
    from adrefine.engine import fit
    seen = {}

    class StubTrainer:
        lr = [0.1, 0.2, 0.3]

        def __init__(self, model, **kw):
            seen["trainer_kw"] = kw
            seen["trainer_sees"] = _snapshot(model)

        def step(self, batch):
            return torch.ones(3)

    class StubValidator:
        def __init__(self, model):
            self.model = copy.deepcopy(model)  # as the default validator factory copies it

        def load_ema(self, trainer):
            pass

        def __call__(self, loader):
            from adrefine.engine.fit import METRIC_KEYS, VAL_KEYS
            return {**dict.fromkeys(METRIC_KEYS + VAL_KEYS, 0.5), "fitness": 0.5}

    monkeypatch.setattr(T, "FusedTrainer", StubTrainer)
    ckpt = SimpleNamespace(save_last_and_best=lambda *a, **k: seen.setdefault("train_args", k["train_args"]) and 0.5,
                           save_checkpoint=lambda *a, **k: None)
    sd = {k: v.clone() for k, v in src80.state_dict().items()}

    def run(model, **cfg):
        seen.clear()
        vals = []
        fit(model, SimpleNamespace(epochs=1, batch=2, close_mosaic=0, optimizer="SGD", **cfg), _Set(), _Set(),
            tmp_path, graphs=False, validator_factory=lambda mm, c: vals.append(StubValidator(mm)) or vals[-1],
            loader_factory=lambda *a: _Loader(), checkpoint=ckpt)
        return vals[0]

    m = _model(3, 13)
    before = _snapshot(m)
    val = run(m, pretrained=sd)
    moved = _expect(sd, before)
    assert 0 < len(moved) < len(sd)
    for k in before:  # the model, the trainer's view of it and the validator's copy all hold the loaded weights
        want = sd[k] if k in moved else before[k]
        for got in (m.state_dict()[k], seen["trainer_sees"][k], val.model.state_dict()[k]):
            assert torch.equal(got.float(), want.float()), k
    assert seen["train_args"]["pretrained"] is True  # the arguments, not a second copy of the weights
    # a path; and the values that load nothing
    from adrefine.engine import checkpoint as C
    f = tmp_path / "w.pt"
    torch.save({"ema": sd, "model": None}, f)
    m2 = _model(3, 13)
    run(m2, pretrained=str(f))
    assert seen["train_args"]["pretrained"] == str(f)
    assert all(torch.equal(m2.state_dict()[k], m.state_dict()[k]) for k in before)
    assert C.load_checkpoint(f)["model"] is None
    for nothing in (True, False, None):
        m3 = _model(3, 13)
        run(m3, pretrained=nothing)
        assert all(torch.equal(m3.state_dict()[k], before[k]) for k in before)
    m4 = _model(3, 13)
    run(m4)  # no such key in cfg: the default
    assert all(torch.equal(m4.state_dict()[k], before[k]) for k in before)
