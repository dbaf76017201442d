"""GPU: adr_augment_mix_u8 (csrc/adr_augment.hip) renders plans with a MixUp stage bit-exactly: against the reference's
own chain and dataset (tests/golden/aug_mixup_256.npz, dataset_mixup_tiny.npz; scripts/gen_mixup_golden.py) and, on a
hand-built batch, against the numpy executor of tests/mixup_util.py. A batch without a mixed plan still takes
adr_augment_u8."""
import copy
import ctypes
import warnings

import numpy as np
import pytest
import torch

import aug_util as A
import dataset_util as D
import mixup_util as X
from conftest import golden

pytestmark = pytest.mark.gpu


def _calls(monkeypatch):
    """Names of the status-returning library entries called from here on."""
    import adrefine.native as N
    names = []
    monkeypatch.setattr(N, "CALL_HOOK", lambda name, fn, a: (names.append(name), fn(*a))[1])
    return names


def test_chain_render_vs_reference(monkeypatch):
    from adrefine.data.augment import collate_fn
    g = golden(X.AUG["name"])
    names = _calls(monkeypatch)
    batch = collate_fn(X.run_chain(int(g["seed"])))
    torch.cuda.synchronize()
    assert [n for n in names if "augment" in n] == ["adr_augment_mix_u8"]
    img = batch["img"].cpu().numpy()
    assert img.dtype == np.uint8 and img.shape == g["img"].shape
    bad = np.argwhere(img != g["img"])
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    assert np.array_equal(batch["bboxes"].numpy(), g["bboxes"]) and np.array_equal(batch["cls"].numpy(), g["cls"])
    assert np.array_equal(batch["batch_idx"].numpy(), g["batch_idx"])


def _src(rs, h, w):
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)


def _mosaic(rs, W, H, xc, yc, M):
    """A 2W x 2H canvas with four tiles around (xc, yc) that leave border on every side, warped by M to W x H."""
    from adrefine.data.augment import ImagePlan
    p = ImagePlan(_src(rs, 8, 8))
    p.tiles = []
    for x1, y1, x2, y2 in ((xc - 13, yc - 9, xc, yc), (xc, yc - 11, xc + 15, yc), (xc - 10, yc, xc, yc + 12),
                           (xc, yc, xc + 14, yc + 10)):
        s = _src(rs, y2 - y1 + 3, x2 - x1 + 2)
        p.tiles.append((s, x1, y1, x2, y2, 2, 3))  # the tile starts inside its source
    p.canvas = (2 * W, 2 * H)
    p.M, p.size = np.asarray(M, dtype=np.float32), (W, H)
    return p


def _hand_built(r113, r114):
    from adrefine.data.augment import ImagePlan
    W, H = 32, 24
    rs = np.random.RandomState(7)
    # image 1: both layers warped mosaics; each canvas is mapped into a part of the output, so that the rest of it
    # shows the warp's border in both layers
    a = _mosaic(rs, W, H, 30, 22, [[0.62, 0.08, -6.3], [-0.07, 0.6, -3.1]])
    a.mixup(_mosaic(rs, W, H, 34, 26, [[0.55, -0.1, -2.2], [0.09, 0.58, -7.4]]), r113)
    a.rgb = True
    # image 2: the first layer un-warped with a single tile inside a border (a letterbox pad), the second warped;
    # HSV and both flips after the mix
    b = ImagePlan(_src(rs, 18, 25)).letterbox((25, 18), 3, 2, 4, 4)
    assert b.size == (W, H) and b.M is None and len(b.tiles) == 1
    b.mixup(_mosaic(rs, W, H, 31, 25, [[0.5, 0.0, 1.5], [0.0, 0.5, -2.0]]), r114)
    x = np.arange(256, dtype=np.float64)
    b.lut = np.stack([((x * 1.02) % 180).astype(np.uint8), np.clip(x * 0.7, 0, 255).astype(np.uint8),
                      np.clip(x * 1.2, 0, 255).astype(np.uint8)])
    b.flip_ud = b.flip_lr = b.rgb = True
    # image 3: not mixed (a warped mosaic with HSV, left-right flipped, BGR planes)
    c = _mosaic(rs, W, H, 33, 23, [[0.7, 0.12, -9.0], [-0.1, 0.66, -4.0]])
    c.lut, c.flip_lr = b.lut[::-1].copy() % 180, True
    return [a, b, c]


def test_hand_built_batch_vs_numpy_executor(monkeypatch):
    """32 x 24 outputs, three images (see _hand_built). With r113 the float64 blend of two 114 border pixels,
    114 * r + 114 * (1 - r), truncates to 113, with r114 it stays 114: wherever both layers show the border the
    output must read exactly that, and the whole batch equals the executor."""
    from adrefine.data.augment import render
    r113, r114 = X.border_ratio(113), X.border_ratio(114)
    plans = _hand_built(r113, r114)
    want = np.stack([X.execute_plan(p) for p in plans])
    both = [(X.execute_layer(p) == 114).all(-1) & (X.execute_layer(p.mix[0]) == 114).all(-1) for p in plans[:2]]
    assert both[0].sum() >= 8 and both[1].sum() >= 8 and not both[0].all() and not both[1].all()
    assert (want[0][:, both[0]] == 113).all()       # no HSV on image 1: the blended border itself
    assert len(np.unique(want[0])) > 100 and len(np.unique(want[1])) > 100
    names = _calls(monkeypatch)
    out = render(plans, "cuda")
    torch.cuda.synchronize()
    assert names == ["adr_augment_mix_u8"]
    got = out.cpu().numpy()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    assert (got[0][:, both[0]] == 113).all()
    # image 2 without its HSV and flips: the blended border stays 114 under r114, and would be 113 under r113
    for r, v in ((r114, 114), (r113, 113)):
        q = copy.copy(plans[1])
        q.lut, q.flip_ud, q.flip_lr, q.mix = None, False, False, (plans[1].mix[0], r, 1 - r)
        got = render([q], "cuda").cpu().numpy()[0]
        assert np.array_equal(got, X.execute_plan(q)) and (got[:, both[1]] == v).all(), v


def test_unmixed_batch_takes_the_unchanged_entry(monkeypatch):
    """aug_default_256 through render: the bytes it always gave, through adr_augment_u8 (not the mix entry)."""
    from adrefine.data.augment import render
    g = golden("aug_default_256")
    plans = [o["img"] for o in A.run_chain("aug_default_256")]
    names = _calls(monkeypatch)
    out = render(plans, "cuda")
    torch.cuda.synchronize()
    assert names == ["adr_augment_u8"]
    assert np.array_equal(out.cpu().numpy(), g["img"])


def _ds(tree, hyp, **kw):
    from adrefine.data.dataset import YOLODataset
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return YOLODataset(**dict(dict(img_path=tree, imgsz=D.IMGSZ, hyp=hyp, data={"names": D.NAMES}, augment=True,
                                       pad=0.0), **kw))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return str(D.write_tree(tmp_path_factory.mktemp("mix") / "tiny", D.fixture_images(golden("dataset_tiny"))))


@pytest.mark.parametrize("tag", list(X.DATASET))
def test_dataset_passes_equal_the_reference(tree, tag):
    """cache=None through build_dataloader (prefetch 1): both load_image calls of a sample go through the device
    pool, sized for two evictions per sample; buffer and batches are the reference's."""
    from adrefine.data.build import build_dataloader
    g, cfg = golden("dataset_mixup_tiny"), X.DATASET[tag]
    ds = _ds(tree, X.dataset_hyp(tag), cache=None, batch_size=cfg["collate"])
    assert ds.max_buffer_length == 8 and ds.pool_slots() == 8 + 2 * 2 * cfg["collate"]
    D.seed(cfg["seed"])
    batches = list(build_dataloader(ds, cfg["collate"], shuffle=False, prefetch=1, sampler=cfg["order"]))
    assert len(batches) == len(cfg["order"]) // cfg["collate"]
    for b, batch in enumerate(batches):
        img = batch["img"].cpu().numpy()
        bad = np.argwhere(img != g[f"{tag}_b{b}_img"])
        assert img.shape == g[f"{tag}_b{b}_img"].shape and len(bad) == 0, (tag, b, len(bad), bad[:5].tolist())
        for k in ("cls", "bboxes", "batch_idx"):
            assert np.array_equal(batch[k].numpy(), g[f"{tag}_b{b}_{k}"]), (tag, b, k)
    assert ds.buffer == [v for v in g[f"{tag}_buffers"][-1].tolist() if v >= 0]
    assert not ds._retired and len(ds.pool._size) == len(ds.buffer)  # every evicted image went back


def test_resident_and_host_sources_render_the_same(tree):
    """A mixed batch from a DevicePool (cache="gpu") equals the same plans rendered from host arrays, both layers;
    a second layer from the host under a resident first layer raises."""
    from adrefine.data.augment import collate_fn, render
    tiny = golden("dataset_tiny")
    ds = _ds(tree, X.dataset_hyp("half"), cache="gpu", batch_size=1)
    host = {id(ds.ims[i]): np.ascontiguousarray(tiny[f"load_img_{i}"]) for i in range(8)}
    D.seed(5)
    samples = [ds[i] for i in (3, 0, 6, 5)]
    plans = [s["img"] for s in samples]
    assert all(p.mix is not None for p in plans)
    assert len({q.canvas for p in plans for q in p.layers()}) == 2  # mosaic and letterboxed layers
    dev = collate_fn(samples)["img"]

    def on_host(p):
        q = copy.copy(p)
        q.tiles = [(host[id(t[0])],) + tuple(t[1:]) for t in p.tiles]
        return q

    hplans = []
    for p in plans:
        q = on_host(p)
        q.mix = (on_host(p.mix[0]),) + p.mix[1:]
        hplans.append(q)
    ref = render(hplans, "cuda")
    torch.cuda.synchronize()
    assert torch.equal(dev, ref)
    assert np.array_equal(ref.cpu().numpy(), np.stack([X.execute_plan(p) for p in hplans]))
    hplans[1].mix = plans[1].mix  # a resident second layer under host sources
    with pytest.raises(ValueError, match="mixes host and device"):
        render(hplans, "cuda")


def test_bad_mix_records_are_rejected_without_a_launch(monkeypatch):
    """`second` outside [B, ndesc) makes the entry return an error, and a record-size mismatch makes render raise,
    both before anything is launched: the output keeps its sentinel."""
    from adrefine.data import augment as G
    from adrefine.native import lib
    plans = _hand_built(0.5, 0.5)
    out = torch.full((3, 3, 24, 32), 0xA5, dtype=torch.uint8, device="cuda")
    seen = []

    def hook(name, fn, a):  # spoil the host records (what the entry validates) on their way in
        if name == "adr_augment_mix_u8":
            rec = ctypes.cast(a[4], ctypes.POINTER(G.AugMix))
            seen.append((a[2], [rec[i].second for i in range(a[5])]))
            rec[0].second = spoil(a[2], a[5])
        rc = fn(*a)
        if rc:
            raise RuntimeError(lib.lib.adr_last_error().decode())
        return rc

    import adrefine.native as N
    monkeypatch.setattr(N, "CALL_HOOK", hook)
    for spoil in (lambda ndesc, B: ndesc, lambda ndesc, B: B - 1, lambda ndesc, B: -2):
        with pytest.raises(RuntimeError, match="augment_mix: image 0 second="):
            G.render(plans, "cuda", out=out)
    assert seen == [(5, [3, 4, -1])] * 3
    monkeypatch.setattr(N, "CALL_HOOK", None)
    rc = lib.lib.adr_augment_mix_u8(None, None, 2, None, None, 3, None, None, None, 24, 32, None)
    assert rc != 0 and "ndesc=2 B=3" in lib.lib.adr_last_error().decode()

    class Other(ctypes.Structure):
        _fields_ = [("second", ctypes.c_int), ("r", ctypes.c_double), ("one_minus_r", ctypes.c_double),
                    ("more", ctypes.c_double)]

    assert lib.adr_augment_mix_desc_size() == ctypes.sizeof(G.AugMix) == 24 != ctypes.sizeof(Other)
    monkeypatch.setattr(G, "AugMix", Other)
    with pytest.raises(RuntimeError, match="layout mismatch"):
        G.render(plans, "cuda", out=out)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


MIXED_EPOCH_SEED = 0  # at mixup 0.15 this epoch's first batch has no mixed sample and its second has three


def test_mixup_dataset_to_trainer(tmp_path, monkeypatch):
    """cfg.mixup = 0.15: an 8-image directory at imgsz 320 -> build_yolo_dataset (cache=None: the pool sized for two
    evictions per sample) -> build_dataloader -> FusedTrainer steps with finite losses; the seeded epoch has mixed and
    unmixed samples, so both entries render."""
    from types import SimpleNamespace

    from adrefine.data.build import build_dataloader, build_yolo_dataset
    from adrefine.engine.trainer import FusedTrainer
    from adrefine.nn.tasks import DetectionModel
    from conftest import ROOT
    from gpu_util import load_recipe_into
    tiny = golden("dataset_tiny")
    imgs = {n: np.tile(tiny[f"native_{n}"], (4, 4, 1)) for n in list(D.SIZES)[:8]}
    tree = str(D.write_tree(tmp_path / "big", imgs))
    hyp = D.hyp()
    hyp.mixup = 0.15
    cfg = SimpleNamespace(**vars(hyp), imgsz=320, rect=False, cache=None, single_cls=False, task="detect",
                          classes=None, fraction=1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        train = build_yolo_dataset(cfg, tree, 4, {"names": {i: str(i) for i in range(80)}}, mode="train")
    assert train.pool_slots() == 8 + 2 * 2 * 4
    m = DetectionModel(str(ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"))
    load_recipe_into(m)
    tr = FusedTrainer(m.cuda(), lr0=0.01, momentum=0.937, weight_decay=5e-4, nbs=4, batch_size=4)
    names = _calls(monkeypatch)
    D.seed(MIXED_EPOCH_SEED)
    batches = list(build_dataloader(train, 4, shuffle=True, prefetch=1))
    renders = [n for n in names if n.startswith("adr_augment")]
    assert len(batches) == 2 and sorted(renders) == ["adr_augment_mix_u8", "adr_augment_u8"], renders
    monkeypatch.undo()
    for batch in batches:
        assert tuple(batch["img"].shape) == (4, 3, 320, 320)
        items = tr.step(batch)
        assert torch.isfinite(items).all(), items
