"""Optimizer selection and the Adam / AdamW host side (engine/trainer.py resolve_optimizer, optimizer_iterations,
Schedule; engine/checkpoint.py) vs the reference's build_optimizer (engine/trainer.py:753-813), its iteration count
(:307), its warm-up loop (:369-381) and the state_dict torch.optim.Adam / AdamW saves. CPU only: the trainer's
host-side tables and buffers are built without running a step."""
import math

import pytest
import torch

from conftest import ROOT
from gpu_util import load_recipe_into

from adrefine.engine.trainer import Schedule, optimizer_iterations, resolve_optimizer

CFG = ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"


def test_resolve_auto():
    assert resolve_optimizer("auto", 0.01, 0.937, 0.1, 1, 10000) == ("AdamW", 0.002, 0.9, 0.0)
    assert resolve_optimizer("auto", 0.01, 0.937, 0.1, 80, 10000) == ("AdamW", 0.000119, 0.9, 0.0)
    assert resolve_optimizer("auto", 0.123, 0.5, 0.1, 80, 10001) == ("SGD", 0.01, 0.9, 0.0)
    assert resolve_optimizer("auto", 0.01, 0.937, 0.1, 1, 1)[0] == "AdamW"
    with pytest.raises(ValueError):
        resolve_optimizer("auto", 0.01, 0.937, 0.1, 1, None)


@pytest.mark.parametrize("name", ["SGD", "Adam", "AdamW"])
def test_resolve_explicit_passes_through(name):
    assert resolve_optimizer(name, 0.03, 0.8, 0.05, 7, None) == (name, 0.03, 0.8, 0.05)
    assert resolve_optimizer(name, 0.03, 0.8, 0.05, 7, 10 ** 6) == (name, 0.03, 0.8, 0.05)


@pytest.mark.parametrize("name", ["Adamax", "NAdam", "RAdam", "RMSProp"])
def test_resolve_unsupported_names_what_is_supported(name):
    with pytest.raises(NotImplementedError) as e:
        resolve_optimizer(name, 0.01, 0.9, 0.1, 1, 100)
    assert all(s in str(e.value) for s in ("SGD", "Adam", "AdamW", "auto"))


def test_resolve_nonsense_raises_reference_message():
    with pytest.raises(NotImplementedError, match="not found in list of available optimizers"):
        resolve_optimizer("Lion", 0.01, 0.9, 0.1, 1, 100)


@pytest.mark.parametrize("n,bs,nbs,epochs", [(1000, 16, 64, 100), (1000, 128, 64, 30), (1, 16, 64, 5),
                                             (640, 64, 64, 16), (641, 64, 64, 16)])
def test_optimizer_iterations(n, bs, nbs, epochs):
    assert optimizer_iterations(n, bs, nbs, epochs) == math.ceil(n / max(bs, nbs)) * epochs
    assert isinstance(optimizer_iterations(n, bs, nbs, epochs), int)


def test_optimizer_iterations_literals():
    assert optimizer_iterations(1000, 16, 64, 100) == 1600  # batch below nbs: nbs divides
    assert optimizer_iterations(1000, 128, 64, 30) == 240  # batch above nbs: the batch divides
    assert optimizer_iterations(640000, 64, 64, 1) == 10000 and optimizer_iterations(640001, 64, 64, 1) == 10001


_KW = dict(lr0=0.01, lrf=0.01, momentum=0.937, nbs=64, batch_size=64, epochs=100, nb=10, warmup_epochs=3.0,
           warmup_bias_lr=0.1, warmup_momentum=0.8)


def test_sgd_schedule_unchanged():
    """nb = 10: nw = max(round(3 * 10), 100) = 100; lf(e) = (1 - e / 100) * 0.99 + 0.01 (trainer.py:214);
    inside the warm-up every value is interpolated over [0, 100] (trainer.py:369-381)."""
    s = Schedule(**_KW)
    lrs, mom, acc = s.at(0)
    assert lrs == [0.0, 0.0, 0.1] and mom == 0.8 and acc == 1
    lrs, mom, acc = s.at(50)  # epoch 5: target 0.01 * 0.9505
    assert lrs == pytest.approx([0.0047525, 0.0047525, 0.0547525], rel=1e-12) and acc == 1
    assert mom == pytest.approx(0.8685, rel=1e-12)
    lrs, mom, acc = s.at(101)  # epoch 10, past the warm-up: 0.01 * 0.901
    assert lrs == pytest.approx([0.00901] * 3, rel=1e-12) and mom == 0.937 and acc == 1
    s4 = Schedule(**{**_KW, "batch_size": 16})
    assert s4.at(0)[2] == 1 and s4.at(50)[2] == 2 and s4.at(100)[2] == 4 and s4.at(500)[2] == 4


def test_adam_schedule_keeps_beta1():
    """Adam's param groups have no 'momentum' (trainer.py:379): beta1 is not warmed up; lrs as for SGD."""
    sgd = Schedule(**_KW)
    adam = Schedule(**_KW, warm_momentum=False)
    for ni in (0, 50, 101):
        lrs, beta1, acc = adam.at(ni)
        assert beta1 == 0.937
        assert lrs == sgd.at(ni)[0] and acc == sgd.at(ni)[2]
    assert Schedule(lr0=0.002, momentum=0.9, warm_momentum=False).at(7) == ([0.002] * 3, 0.9, 1)


# ---- checkpoint round trip -----------------------------------------------------------------------------------

def _trainer(seed, optimizer):
    from adrefine.engine.trainer import FusedTrainer
    from adrefine.nn.tasks import DetectionModel
    m = DetectionModel(str(CFG))
    load_recipe_into(m)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.01 * torch.randn(p.shape, generator=g))
    tr = FusedTrainer(m, lr0=0.002, momentum=0.9, batch_size=16, nb=100, epochs=10, optimizer=optimizer)
    for _, t, _, isp in tr.entries:
        if isp:
            t._adr_used = True
    return tr, g


@pytest.fixture(scope="module")
def sgd_ckpt(tmp_path_factory):
    from adrefine.engine import checkpoint as C
    tr, g = _trainer(3, "SGD")
    tr.mom.copy_(torch.randn(tr.mom.shape, generator=g))
    tr.updates = 5
    f = tmp_path_factory.mktemp("sgd") / "last.pt"
    C.save_checkpoint(tr, f, epoch=1)
    return tr, C.load_checkpoint(f)


@pytest.mark.parametrize("name", ["AdamW", "Adam"])
def test_adam_save_load_resume(tmp_path, name, sgd_ckpt):
    from adrefine.engine import checkpoint as C
    from adrefine.engine.trainer import param_groups
    tr, g = _trainer(1, name)
    assert tr.optimizer == name and tr.mom.shape == tr.sq.shape == (tr.nparam,)
    assert tr.mom.data_ptr() + 4 * tr.nparam == tr.sq.data_ptr()  # one allocation: sq at mom + nparam
    assert not tr.mom.any() and not tr.sq.any() and tr.opt_steps == 0
    tr.mom.copy_(0.1 * torch.randn(tr.mom.shape, generator=g))
    # second moments from 1e-12 (below fp16's 2^-24: flushed to zero in the file, as in the reference's) to 1
    tr.sq.copy_(10 ** (-12 * torch.rand(tr.sq.shape, generator=g)))
    tr.ema_flat.add_(0.05 * torch.randn(tr.ema_flat.shape, generator=g))
    tr.updates = 41
    tr.opt_steps = 37
    f = tmp_path / "last.pt"
    C.save_checkpoint(tr, f, epoch=4, best_fitness=0.3)
    ck = C.load_checkpoint(f)  # weights_only=True
    assert ck["updates"] == 41
    groups = param_groups(tr.model)
    params = dict(tr.model.named_parameters())
    cls = getattr(torch.optim, name)
    opt = cls([params[n] for n, _ in groups[2]], lr=0.002, betas=(0.9, 0.999), weight_decay=0.0)
    opt.add_param_group({"params": [params[n] for n, _ in groups[0]], "weight_decay": tr.wd})
    opt.add_param_group({"params": [params[n] for n, _ in groups[1]], "weight_decay": 0.0})
    own = opt.state_dict()["param_groups"]
    opt.load_state_dict(ck["optimizer"])
    pg = ck["optimizer"]["param_groups"]
    assert [set(a) - {"initial_lr"} for a in pg] == [set(b) for b in own]
    assert [a["betas"] for a in pg] == [(0.9, 0.999)] * 3
    assert [a["weight_decay"] for a in pg] == [0.0, tr.wd, 0.0] and tr.wd > 0
    assert [len(a["params"]) for a in pg] == [len(groups[2]), len(groups[0]), len(groups[1])]
    flushed = 0
    for ei, (pname, t, _, isp) in enumerate(tr.entries):
        if not isp:
            continue
        sl = slice(tr._goff[ei], tr._goff[ei] + t.numel())
        st = opt.state[params[pname]]
        assert torch.equal(st["exp_avg"].float(), tr.mom[sl].view(t.shape).half().float()), pname
        assert torch.equal(st["exp_avg_sq"].float(), tr.sq[sl].view(t.shape).half().float()), pname
        assert float(st["step"]) == 37.0 and st["step"].dtype == torch.float32 and st["step"].dim() == 0
        flushed += int(((st["exp_avg_sq"] == 0) & (tr.sq[sl].view(t.shape) > 0)).sum())
    assert flushed > 0
    raw = ck["optimizer"]["state"][0]
    assert list(raw) == ["step", "exp_avg", "exp_avg_sq"]
    assert raw["exp_avg"].dtype == raw["exp_avg_sq"].dtype == torch.float16 and raw["step"].dtype == torch.float32
    # resume into a trainer on a differently initialised model
    tr2, _ = _trainer(2, name)
    start, best = C.resume(tr2, ck)
    assert start == 5 and best == 0.3
    assert tr2.opt_steps == 37 and tr2.updates == 41 and tr2.ni == 500 and tr2.last_opt_step == -1
    assert torch.equal(tr2.mom, tr.mom.half().float()) and torch.equal(tr2.sq, tr.sq.half().float())
    # the other optimizer family's checkpoint is refused, both ways
    with pytest.raises(ValueError, match="SGD") as e:
        C.resume(tr2, sgd_ckpt[1])
    assert name in str(e.value)
    tr_sgd, _ = sgd_ckpt
    with pytest.raises(ValueError, match="Adam") as e:
        C.resume(tr_sgd, ck)
    assert "SGD" in str(e.value)


def test_sgd_trainer_default_unchanged(sgd_ckpt):
    """The default trainer is SGD with today's state: one momentum arena, and its checkpoints keep loading."""
    from adrefine.engine import checkpoint as C
    tr, ck = sgd_ckpt
    assert tr.optimizer == "SGD" and not tr.adam and tr.mom.shape == (tr.nparam,) and not hasattr(tr, "sq")
    assert set(ck["optimizer"]["state"][0]) == {"momentum_buffer"}
    tr2, _ = _trainer(4, "SGD")
    C.resume(tr2, ck)
    assert torch.equal(tr2.mom, tr.mom.half().float()) and tr2.updates == 5


def test_auto_needs_iterations_and_uses_head_nc():
    from adrefine.engine.trainer import FusedTrainer
    from adrefine.nn.tasks import DetectionModel
    m = DetectionModel(str(CFG))
    with pytest.raises(ValueError):
        FusedTrainer(m, optimizer="auto")
    nc = m.model[-1].nc
    tr = FusedTrainer(m, optimizer="auto", iterations=500, nb=10)
    assert (tr.optimizer, tr.sched.lr0, tr.momentum, tr.sched.warmup_bias_lr) == \
        resolve_optimizer("auto", 0.01, 0.937, 0.1, nc, 500) == ("AdamW", round(0.002 * 5 / (4 + nc), 6), 0.9, 0.0)
    assert tr.lr == [0.0, 0.0, 0.0]  # warm-up from 0 for every group, the bias group included
    tr = FusedTrainer(m, optimizer="auto", iterations=20000, nc=1)
    assert tr.optimizer == "SGD" and tr.sched.lr0 == 0.01 and tr.momentum == 0.9 and not tr.adam
