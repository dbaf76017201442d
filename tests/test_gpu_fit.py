"""GPU: engine.fit end to end on the tiny dataset (tests/dataset_util.py) — three epochs of yolo11n at 64 x 64 with
validation losses, results.csv, last.pt / best.pt, close_mosaic before the last epoch — and a resumed run that
continues with the bits of the uninterrupted one."""
import math
import warnings
from types import SimpleNamespace

import pytest
import torch

import dataset_util as D
from conftest import ROOT, golden
from gpu_util import load_recipe_into

pytestmark = pytest.mark.gpu

NC = 16  # the class count of tests/golden/val_loss.npz (adr_det_loss takes multiples of 8; the labels use 0..2)
EPOCHS = 3


def _cfg():
    # nbs = batch: one optimizer step per batch, so no gradient accumulation crosses an epoch boundary
    return SimpleNamespace(**vars(D.hyp()), imgsz=D.IMGSZ, rect=False, cache="gpu", single_cls=False, task="detect",
                           classes=None, fraction=1.0, epochs=EPOCHS, batch=2, nbs=2, close_mosaic=1, optimizer="auto",
                           patience=100, val=True, save=True)


def _setup(tree):
    from adrefine.data.build import build_yolo_dataset
    from adrefine.nn.tasks import DetectionModel
    cfg = _cfg()
    data = {"names": {i: str(i) for i in range(NC)}}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        train = build_yolo_dataset(cfg, tree, 2, data, mode="train")
        val = build_yolo_dataset(cfg, tree, 4, data, mode="val")
    m = DetectionModel(str(ROOT / "tests" / "configs" / "yolo11n.yaml"), nc=NC)
    load_recipe_into(m)
    return m.cuda(), cfg, train, val


def _seed(epoch):
    D.seed(100 + epoch)
    torch.manual_seed(100 + epoch)


def _has_mosaic(ds):
    from adrefine.data.augment import Mosaic

    def walk(t):  # close_mosaic keeps the Mosaic object in the rebuilt chain with p = 0, as the reference's does
        if isinstance(t, Mosaic):
            return t.p > 0
        return any(walk(c) for c in getattr(t, "transforms", []) or [])
    return walk(ds.transforms)


def _fit(tree, save_dir, stop_after=None, resume=None):
    """One fit() run; the augmentation RNGs are seeded per epoch (before the run for its first epoch, in on_epoch_end
    for the next), so an epoch's batches do not depend on where the run started. prefetch=0: the samples are built on
    the iterating thread, in step with the seeding."""
    from adrefine.engine import fit
    model, cfg, train, val = _setup(tree)
    rows, mosaic = [], []

    def hook(epoch, row):
        rows.append(row)
        mosaic.append(_has_mosaic(train))
        _seed(epoch + 1)
        return stop_after is not None and epoch + 1 >= stop_after

    start = 0 if resume is None else EPOCHS - 1
    _seed(start)
    out = fit(model, cfg, train, val, save_dir, resume=resume, graphs=False, prefetch=0, on_epoch_end=hook,
              exact_resume=True)
    return out, rows, mosaic


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return str(D.write_tree(tmp_path_factory.mktemp("fit") / "tiny", D.fixture_images(golden("dataset_tiny"))))


@pytest.fixture(scope="module")
def full_run(tree, tmp_path_factory):
    d = tmp_path_factory.mktemp("full")
    return d, _fit(tree, d)


def test_fit_end_to_end(full_run):
    from adrefine.engine.checkpoint import load_checkpoint
    from adrefine.engine.fit import CSV_KEYS
    d, ((results, last, best), rows, mosaic) = full_run
    lines = (d / "results.csv").read_text().splitlines()
    assert lines[0].split(",") == list(CSV_KEYS) and len(lines) == 1 + EPOCHS
    for k, line in enumerate(lines[1:]):
        vals = dict(zip(CSV_KEYS, (float(v) for v in line.split(","))))
        assert vals["epoch"] == k + 1
        for key in CSV_KEYS:
            if key.startswith(("train/", "val/")):
                assert math.isfinite(vals[key]) and vals[key] >= 0, (k, key, vals[key])
        assert vals["train/cls_loss"] > 0 and vals["val/cls_loss"] > 0
    assert mosaic == [True, True, False]  # closed before the last epoch (close_mosaic = 1)
    assert last is not None and best is not None
    for p in (last, best):
        ck = load_checkpoint(p)
        assert ck["ema"] and ck["epoch"] <= EPOCHS - 1
    assert load_checkpoint(last)["epoch"] == EPOCHS - 1
    assert results["fitness"] is not None and set(rows[-1]) == set(CSV_KEYS[2:])


def test_resumed_run_equals_uninterrupted(full_run, tree, tmp_path):
    from adrefine.engine.checkpoint import load_checkpoint
    _, ((res_full, last_full, _), rows_full, _) = full_run
    (_, last2, _), rows2, _ = _fit(tree, tmp_path, stop_after=EPOCHS - 1)
    assert len(rows2) == EPOCHS - 1 and load_checkpoint(last2)["epoch"] == EPOCHS - 2
    for a, b in zip(rows2, rows_full):  # the same run so far
        assert all(a[k] == b[k] for k in a if k.startswith("train/")), (a, b)
    (res3, last3, _), rows3, _ = _fit(tree, tmp_path, resume=last2)
    assert len(rows3) == 1
    lines = (tmp_path / "results.csv").read_text().splitlines()
    assert [l.split(",")[0] for l in lines[1:]] == ["1", "2", "3"]
    want, got = rows_full[-1], rows3[-1]
    print(f"[fit-resume] uninterrupted {[want[k] for k in want if k.startswith('train/')]} "
          f"resumed {[got[k] for k in got if k.startswith('train/')]}")
    # the unrounded fp32 running mean of the third epoch's loss items, and the fp32 EMA (and with it the model,
    # the optimizer moments and the counters) of FusedTrainer.state_dict() — not the rounded csv row or the fp16
    # checkpoint, which would hide a drift below their resolution
    tl_full, tl_res = res_full["tloss"], res3["tloss"]
    print(f"[fit-resume] unrounded tloss uninterrupted {tl_full.tolist()} resumed {tl_res.tolist()}")
    assert tl_full.dtype == torch.float32 and torch.equal(tl_res, tl_full)
    st_full = torch.load(last_full.with_name("last_state.pt"), weights_only=True)
    st_res = torch.load(last3.with_name("last_state.pt"), weights_only=True)
    assert st_full["epoch"] == st_res["epoch"] == EPOCHS - 1
    a, b = st_full["trainer"], st_res["trainer"]
    assert a["ema"].dtype == torch.float32 and torch.equal(a["ema"], b["ema"])
    assert torch.equal(a["moments"], b["moments"]) and torch.equal(a["grad"], b["grad"])
    assert all(torch.equal(a["model"][k], b["model"][k]) for k in a["model"])
    assert all(a[k] == b[k] for k in ("updates", "opt_steps", "ni", "last_opt_step"))
    ema_full, ema_res = load_checkpoint(last_full)["ema"], load_checkpoint(last3)["ema"]
    assert list(ema_full) == list(ema_res) and all(torch.equal(ema_full[k], ema_res[k]) for k in ema_full)
