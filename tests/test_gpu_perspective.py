"""GPU: the warpPerspective branch of adr_augment_u8 / adr_augment_mix_u8 (csrc/adr_augment.hip, AugDesc.warp == 2)
renders plans with P bit-exactly: against the reference's own chain and dataset (tests/golden/aug_persp_256.npz,
dataset_persp_tiny.npz; scripts/gen_perspective_golden.py) and, on hand-built plans at the smallest shapes where the
kernel can go wrong, against the numpy restatement of tests/perspective_util.py. Exact equality throughout. Batches
without P give the bytes they always gave."""
import copy
import warnings

import numpy as np
import pytest
import torch

import aug_util as A
import dataset_util as D
import perspective_util as P
from conftest import golden

pytestmark = pytest.mark.gpu


def _calls(monkeypatch):
    """Names of the status-returning library entries called from here on."""
    import adrefine.native as N
    names = []
    monkeypatch.setattr(N, "CALL_HOOK", lambda name, fn, a: (names.append(name), fn(*a))[1])
    return names


def _render_equals(plans, want=None):
    from adrefine.data.augment import render
    want = np.stack([P.execute_plan(p) for p in plans]) if want is None else want
    out = render(plans, "cuda")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])],
                                                       want[tuple(bad[0])])
    return got


def test_chain_render_vs_reference(monkeypatch):
    from adrefine.data.augment import collate_fn
    g = golden(P.AUG["name"])
    names = _calls(monkeypatch)
    batch = collate_fn(P.run_chain(int(g["seed"])))
    torch.cuda.synchronize()
    assert [n for n in names if "augment" in n] == ["adr_augment_mix_u8"]
    img = batch["img"].cpu().numpy()
    assert img.dtype == np.uint8 and img.shape == g["img"].shape
    bad = np.argwhere(img != g["img"])
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    assert np.array_equal(batch["bboxes"].numpy(), g["bboxes"]) and np.array_equal(batch["cls"].numpy(), g["cls"])
    assert np.array_equal(batch["batch_idx"].numpy(), g["batch_idx"])


def _ds(tree, hyp, **kw):
    from adrefine.data.dataset import YOLODataset
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return YOLODataset(**dict(dict(img_path=tree, imgsz=D.IMGSZ, hyp=hyp, data={"names": D.NAMES}, augment=True,
                                       pad=0.0), **kw))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return str(D.write_tree(tmp_path_factory.mktemp("persp") / "tiny", D.fixture_images(golden("dataset_tiny"))))


@pytest.mark.parametrize("tag", list(P.DATASET))
def test_dataset_passes_equal_the_reference(tree, tag):
    """cache=None through build_dataloader: load_image's resize, the device pool and the render; "letterbox": the
    canvas under the warp is LetterBox's pad."""
    from adrefine.data.build import build_dataloader
    g, cfg = golden("dataset_persp_tiny"), P.DATASET[tag]
    ds = _ds(tree, P.dataset_hyp(tag), cache=None, batch_size=cfg["collate"])
    D.seed(cfg["seed"])
    batches = list(build_dataloader(ds, cfg["collate"], shuffle=False, prefetch=1, sampler=cfg["order"]))
    assert len(batches) == len(cfg["order"]) // cfg["collate"]
    for b, batch in enumerate(batches):
        img = batch["img"].cpu().numpy()
        bad = np.argwhere(img != g[f"{tag}_b{b}_img"])
        assert img.shape == g[f"{tag}_b{b}_img"].shape and len(bad) == 0, (tag, b, len(bad), bad[:5].tolist())
        for k in ("cls", "bboxes", "batch_idx"):
            assert np.array_equal(batch[k].numpy(), g[f"{tag}_b{b}_{k}"]), (tag, b, k)
    assert ds.buffer == g[f"{tag}_buffer"].tolist()


def _lut():
    x = np.arange(256, dtype=np.float64)
    return np.stack([((x * 1.02) % 180).astype(np.uint8), np.clip(x * 0.7, 0, 255).astype(np.uint8),
                     np.clip(x * 1.2, 0, 255).astype(np.uint8)])


# W x H: two blocks of 64 + 32; H < 16, so the block is 1024 / 8 = 128 wide (128 + 32); a single block
SHAPES = [(96, 40), (160, 8), (64, 16)]


@pytest.mark.parametrize("W,H", SHAPES)
def test_block_origin_and_flips(W, H, monkeypatch):
    """One source image warped to W x H: no flip, flip_lr, flip_lr + flip_ud (the block origin comes from the mirrored
    column), the last one with HSV and RGB planes. The executor's blocks are asserted to be what the case is for."""
    bw0 = min(1024 // min(16, H), W)
    assert (bw0, -(-W // bw0)) == {(96, 40): (64, 2), (160, 8): (128, 2), (64, 16): (64, 1)}[(W, H)]
    rs = np.random.RandomState(W + H)
    plans = []
    for k in range(3):
        p = P.single_plan(rs, W + 21, H + 13, W, H, P.gentle_matrix(rs, W + 21, H + 13, W, H, 0.002))
        p.flip_lr, p.flip_ud = k >= 1, k == 2
        plans.append(p)
    plans[2].lut, plans[2].rgb = _lut(), True
    names = _calls(monkeypatch)
    got = _render_equals(plans)
    assert names == ["adr_augment_u8"]
    assert all(len(np.unique(g)) > 100 for g in got)  # images, not borders


def test_mosaic_canvas_and_mixes(monkeypatch):
    """96 x 40: a four-tile mosaic canvas under P; a mix whose second layer alone has P (the first is affine), one
    whose layers both have P, and one whose first layer alone has it (the second un-warped, a letterbox pad)."""
    from adrefine.data.augment import ImagePlan
    W, H = 96, 40
    rs = np.random.RandomState(5)
    G = lambda persp: P.gentle_matrix(rs, 2 * W, 2 * H, W, H, persp)  # noqa: E731
    a = P.mosaic_plan(rs, W, H, G(0.002))
    assert len(a.tiles) == 4
    b = P.mosaic_plan(rs, W, H, G(0.0)[:2])
    b.mixup(P.mosaic_plan(rs, W, H, G(0.002)), 0.37)
    c = P.mosaic_plan(rs, W, H, G(0.002))
    c.mixup(P.mosaic_plan(rs, W, H, G(0.001)), 0.61)
    c.lut, c.flip_lr, c.rgb = _lut(), True, True
    d = P.mosaic_plan(rs, W, H, G(0.002))
    d.mixup(ImagePlan(P.src_image(rs, H - 6, W - 9)).letterbox((W - 9, H - 6), 4, 3, 5, 3), 0.5)
    assert b.M is not None and b.P is None and b.mix[0].P is not None and c.P is not None and c.mix[0].P is not None
    assert d.mix[0].P is None and d.mix[0].M is None and d.mix[0].size == (W, H)
    names = _calls(monkeypatch)
    _render_equals([a, b, c, d])
    assert names == ["adr_augment_mix_u8"]
    names.clear()
    _render_equals([a])
    assert names == ["adr_augment_u8"]


def test_strong_matrix_takes_the_clamp_paths():
    """A denominator that changes sign inside the image (P[2, 0] = 1/32 at 96 px): a pixel with W == 0 exactly, pixels
    whose quotient leaves the int range and pixels whose coordinate leaves the short range, asserted on the executor,
    then compared; with both flips as well."""
    W, H = 96, 40
    sx, sy, fx, fy, paths = P.perspective_coords(P.STRONG, (W, H))
    assert paths["w0"].sum() >= 1 and paths["int"].sum() >= 1 and paths["short"].sum() >= 1
    assert paths["w0"][0, 32] and (sx[1:, 32] == 32767).all() and (sy[1:, 32] == 32767).all()
    rs = np.random.RandomState(9)
    p = P.single_plan(rs, 96, 96, W, H, P.STRONG)
    q = copy.copy(p)
    q.flip_lr = q.flip_ud = True
    got = _render_equals([p, q])
    assert (got[0][:, paths["w0"]] == np.asarray(p.tiles[0][0])[0, 0][:, None]).all()  # W == 0 reads canvas (0, 0)
    assert len(np.unique(got[0])) > 100


def test_batch_of_affine_perspective_and_unwarped(monkeypatch):
    W, H = 96, 40
    rs = np.random.RandomState(11)
    a = P.single_plan(rs, W + 21, H + 13, W, H, P.gentle_matrix(rs, W + 21, H + 13, W, H, 0.0)[:2])
    b = P.single_plan(rs, W + 21, H + 13, W, H, P.gentle_matrix(rs, W + 21, H + 13, W, H, 0.002))
    c = P.single_plan(rs, W, H, W, H)
    d = P.mosaic_plan(rs, W, H, P.gentle_matrix(rs, 2 * W, 2 * H, W, H, 0.001))
    e = P.single_plan(rs, W + 5, H + 5, W, H, P.gentle_matrix(rs, W + 5, H + 5, W, H, 0.0)[:2])
    e.flip_lr, e.lut = True, _lut()
    # affine tables of W + W + H + H ints sit between the matrices: the second P needs the pad to an even offset or not
    plans = [a, b, c, d, e]
    names = _calls(monkeypatch)
    _render_equals(plans)
    _render_equals([b, a, d])
    _render_equals([c, b, a, e, d])
    assert names == ["adr_augment_u8"] * 3


def test_odd_table_offset_is_padded(monkeypatch):
    """The matrix must start at an even int offset of the tables. An affine image's tables are 2 W + 2 H ints, always
    even, so the pad never arises from today's tables: it is reached here by giving the affine tables one more int
    (which the kernel never reads). With the pad the images are still exact; W + H odd on top."""
    from adrefine.data import augment as G
    W, H = 33, 18
    rs = np.random.RandomState(13)
    a = P.single_plan(rs, W + 8, H + 8, W, H, P.gentle_matrix(rs, W + 8, H + 8, W, H, 0.0)[:2])
    b = P.single_plan(rs, W + 8, H + 8, W, H, P.gentle_matrix(rs, W + 8, H + 8, W, H, 0.003))
    _render_equals([a, b])
    real = G.warp_affine_tables
    monkeypatch.setattr(G, "warp_affine_tables", lambda M, dsize: real(M, dsize) + (np.zeros(1, np.int64),))
    _render_equals([a, b, a, b])


def test_batch_without_p_gives_the_bytes_it_always_gave(monkeypatch):
    """aug_rot_256 (warpAffine, HSV, both flips) through render: the fixture's bytes and the existing executor's,
    through adr_augment_u8."""
    from adrefine.data.augment import render
    g = golden("aug_rot_256")
    plans = [o["img"] for o in A.run_chain("aug_rot_256")]
    assert all(p.P is None and p.M is not None for p in plans)
    names = _calls(monkeypatch)
    out = render(plans, "cuda")
    torch.cuda.synchronize()
    assert names == ["adr_augment_u8"]
    got = out.cpu().numpy()
    assert np.array_equal(got, g["img"])
    assert np.array_equal(got, np.stack([A.execute_plan(p) for p in plans]))


def test_resident_and_host_sources_render_the_same(tree):
    """A batch with P from a DevicePool (cache="gpu") equals the same plans rendered from host arrays."""
    from adrefine.data.augment import collate_fn, render
    tiny = golden("dataset_tiny")
    ds = _ds(tree, P.dataset_hyp("mosaic"), cache="gpu", batch_size=1)
    host = {id(ds.ims[i]): np.ascontiguousarray(tiny[f"load_img_{i}"]) for i in range(8)}
    D.seed(5)
    samples = [ds[i] for i in (3, 0, 6, 5)]
    plans = [s["img"] for s in samples]
    assert all(p.P is not None and p.M is None for p in plans)
    dev = collate_fn(samples)["img"]
    hplans = []
    for p in plans:
        q = copy.copy(p)
        q.tiles = [(host[id(t[0])],) + tuple(t[1:]) for t in p.tiles]
        hplans.append(q)
    ref = render(hplans, "cuda")
    torch.cuda.synchronize()
    assert torch.equal(dev, ref)
    assert np.array_equal(ref.cpu().numpy(), np.stack([P.execute_plan(p) for p in hplans]))


def test_render_refuses_bad_matrices_without_a_launch(monkeypatch):
    from adrefine.data.augment import render
    rs = np.random.RandomState(17)
    bad = np.eye(3, dtype=np.float32)
    bad[2, 1] = np.inf
    p = P.single_plan(rs, 40, 30, 32, 24, bad)
    out = torch.full((1, 3, 24, 32), 0xA5, dtype=torch.uint8, device="cuda")
    names = _calls(monkeypatch)
    with pytest.raises(ValueError, match="not finite"):
        render([p], "cuda", out=out)
    p.P = np.eye(3, dtype=np.float32)
    p.M = np.eye(3, dtype=np.float32)[:2]
    with pytest.raises(ValueError, match="warpAffine and a warpPerspective"):
        render([p], "cuda", out=out)
    torch.cuda.synchronize()
    assert names == [] and bool((out == 0xA5).all())


def test_perspective_dataset_to_trainer(tmp_path):
    """cfg.perspective = 0.001: an 8-image directory at imgsz 320 -> build_yolo_dataset -> build_dataloader ->
    a FusedTrainer step with finite losses."""
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
    hyp.perspective = 0.001
    cfg = SimpleNamespace(**vars(hyp), imgsz=320, rect=False, cache=None, single_cls=False, task="detect",
                          classes=None, fraction=1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        train = build_yolo_dataset(cfg, tree, 4, {"names": {i: str(i) for i in range(80)}}, mode="train")
    m = DetectionModel(str(ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"))
    load_recipe_into(m)
    tr = FusedTrainer(m.cuda(), lr0=0.01, momentum=0.937, weight_decay=5e-4, nbs=4, batch_size=4)
    D.seed(0)
    batch = next(iter(build_dataloader(train, 4, shuffle=True, prefetch=0)))
    assert tuple(batch["img"].shape) == (4, 3, 320, 320)
    assert len(torch.unique(batch["img"])) > 100
    items = tr.step(batch)
    assert torch.isfinite(items).all(), items
