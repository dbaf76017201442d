"""GPU: adr_resize_u8 (csrc/adr_resize.hip), the DevicePool and YOLODataset / build_dataloader on the resident pool,
against tests/golden/dataset_tiny.npz (the reference's own YOLODataset on the same directory,
scripts/gen_dataset_golden.py; OpenCV's resize restated in tests/letterbox_util.py: PARITY UNPINNED)."""
import ctypes
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

import dataset_util as D
from conftest import ROOT, golden
from gpu_util import load_recipe_into

pytestmark = pytest.mark.gpu
CFG = ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def g():
    return golden("dataset_tiny")


@pytest.fixture(scope="module")
def tree(g, tmp_path_factory):
    return str(D.write_tree(tmp_path_factory.mktemp("ds") / "tiny", D.fixture_images(g)))


def _ds(tree, **kw):
    from adrefine.data.dataset import YOLODataset
    kw = dict(dict(img_path=tree, imgsz=D.IMGSZ, cache=None, hyp=D.hyp(), data={"names": D.NAMES}), **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return YOLODataset(**kw)


def _resize_launch(g, order, stage_off, pairs=None):
    """All eight images (or `pairs` of (source, expected)) in one adr_resize_u8 launch: sources packed from byte
    stage_off on, destinations 256-aligned in `order`, the pool filled with a sentinel. Returns (pool bytes,
    {image: (offset, shape)})."""
    from adrefine import kernels as K
    from adrefine.data.augment import resize_linear_tables
    from adrefine.data.pool import ResizeDesc, resize_mode, resize_prefix
    from adrefine.native import lib
    names = list(D.SIZES)[:8]
    srcs = [g[f"native_{n}"] for n in names] if pairs is None else [p[0] for p in pairs]
    dsts = [g[f"load_img_{i}"] for i in range(8)] if pairs is None else [p[1] for p in pairs]
    B = len(srcs)
    dst_off, top = {}, 0
    for i in order:
        dst_off[i] = top
        top += (dsts[i].size + 255) // 256 * 256 + 256  # a block of slack between the images
    stage = np.zeros(stage_off + sum(s.size for s in srcs), np.uint8)
    descs, tabs, ntab, off = (ResizeDesc * B)(), [], 0, stage_off
    for i, (s, t) in enumerate(zip(srcs, dsts)):
        stage[off:off + s.size] = s.reshape(-1)
        d = descs[i]
        d.src_off, d.dst_off, d.sw, d.sh, d.nw, d.nh = off, dst_off[i], s.shape[1], s.shape[0], t.shape[1], t.shape[0]
        d.mode = resize_mode(d.sw, d.sh, d.nw, d.nh)
        if d.mode == 1:
            tab = np.concatenate(resize_linear_tables(d.sw, d.nw) + resize_linear_tables(d.sh, d.nh))
            d.tab_off, ntab = ntab, ntab + tab.size
            tabs.append(tab)
        off += s.size
    assert {d.mode for d in descs} == {0, 1, 2}
    pre = resize_prefix([(d.nw, d.nh) for d in descs])
    assert len(set(pre.tolist())) == B  # more than one block, every image its own
    st = torch.from_numpy(stage).cuda()
    dd = torch.frombuffer(bytearray(descs), dtype=torch.uint8).cuda()
    pf, tb = torch.from_numpy(pre).cuda(), torch.from_numpy(np.concatenate(tabs)).cuda()
    pool = torch.full((top,), SENTINEL, dtype=torch.uint8, device="cuda")
    lib.adr_resize_u8(K.fptr(st), stage.size, K.fptr(dd), ctypes.cast(descs, ctypes.c_void_p), K.fptr(pf), B,
                      K.fptr(tb), ntab, K.fptr(pool), top, K.stream())
    torch.cuda.synchronize()
    return pool.cpu().numpy(), {i: (dst_off[i], dsts[i].shape) for i in range(B)}


@pytest.mark.parametrize("order,stage_off", [(list(range(8)), 0), ([5, 2, 7, 0, 3, 6, 1, 4], 13)])
def test_resize_kernel_bit_exact_and_writes_nothing_else(g, order, stage_off):
    """Upscale, exact 2x (area), general shrink, copy, tall, 10 x 10 and sizes whose byte count is no multiple of 4,
    in one launch; the second run permutes the destinations and packs the sources from an odd byte offset."""
    pool, where = _resize_launch(g, order, stage_off)
    untouched = np.ones(pool.size, bool)
    for i, (off, shape) in where.items():
        n = int(np.prod(shape))
        got = pool[off:off + n].reshape(shape)
        bad = np.argwhere(got != g[f"load_img_{i}"])
        assert len(bad) == 0, (i, shape, len(bad), bad[:5].tolist())
        untouched[off:off + n] = False
    assert (pool[untouched] == SENTINEL).all()


def test_resize_kernel_last_bytes_of_an_image(g):
    """load_image leaves one side at imgsz, so every fixture image is a whole number of dwords. Destinations of
    1173, 567, 90 and 75 bytes (remainders 1, 3, 2, 3; the last one smaller than a block's first wave) end in 1-3
    byte stores; expected: the cv2.resize restatement the fixture itself was made with (letterbox_util.resize),
    linear, area and copy."""
    import letterbox_util as U
    src = [g["native_im1"], g["native_im3"], g["native_im7"], g["native_im7"][:5, :5].copy(), g["native_im2"][:18, :14]]
    size = [(23, 17), (21, 9), (5, 6), (5, 5), (7, 9)]  # (nw, nh): copy, linear, linear, copy, area
    pairs = [(np.ascontiguousarray(s), s if (s.shape[1], s.shape[0]) == wh else U.resize(s, wh))
             for s, wh in zip(src, size)]
    assert sorted(p[1].size % 4 for p in pairs) == [1, 1, 2, 3, 3]
    pool, where = _resize_launch(g, [3, 0, 4, 2, 1], 7, pairs)
    untouched = np.ones(pool.size, bool)
    for i, (off, shape) in where.items():
        n = int(np.prod(shape))
        assert np.array_equal(pool[off:off + n].reshape(shape), pairs[i][1]), (i, shape)
        untouched[off:off + n] = False
    assert (pool[untouched] == SENTINEL).all()


def test_resize_good_descriptors_launch():
    """The valid launch whose one-rule violations tests/test_dataset.py::test_resize_entry_rejects rejects: it passes
    the entry's validation with the true buffer sizes and gives the restatement's pixels (copy, area, linear)."""
    import letterbox_util as U
    from adrefine import kernels as K
    from adrefine.data.augment import resize_linear_tables
    from adrefine.data.pool import ResizeDesc, resize_prefix
    from adrefine.native import lib
    rows = D.RESIZE_GOOD
    descs = (ResizeDesc * len(rows))()
    for i, r in enumerate(rows):
        (descs[i].src_off, descs[i].dst_off, descs[i].sw, descs[i].sh, descs[i].nw, descs[i].nh, descs[i].mode,
         descs[i].tab_off) = r
    stage = np.random.RandomState(4).randint(0, 256, D.RESIZE_SRC_BYTES).astype(np.uint8)
    tab = np.concatenate(resize_linear_tables(8, 5) + resize_linear_tables(8, 3))
    assert tab.size == D.RESIZE_NTAB
    st, tb = torch.from_numpy(stage).cuda(), torch.from_numpy(tab).cuda()
    dd = torch.frombuffer(bytearray(descs), dtype=torch.uint8).cuda()
    pf = torch.from_numpy(resize_prefix([(r[4], r[5]) for r in rows])).cuda()
    pool = torch.full((D.RESIZE_DST_BYTES,), SENTINEL, dtype=torch.uint8, device="cuda")
    lib.adr_resize_u8(K.fptr(st), D.RESIZE_SRC_BYTES, K.fptr(dd), ctypes.cast(descs, ctypes.c_void_p), K.fptr(pf),
                      len(rows), K.fptr(tb), D.RESIZE_NTAB, K.fptr(pool), D.RESIZE_DST_BYTES, K.stream())
    torch.cuda.synchronize()
    got, untouched = pool.cpu().numpy(), np.ones(D.RESIZE_DST_BYTES, bool)
    for s, d, sw, sh, nw, nh, mode, _ in rows:
        src = stage[s:s + sw * sh * 3].reshape(sh, sw, 3)
        want = src if mode == 0 else U.resize(src, (nw, nh))
        assert np.array_equal(got[d:d + nw * nh * 3].reshape(nh, nw, 3), want), mode
        untouched[d:d + nw * nh * 3] = False
    assert (got[untouched] == SENTINEL).all()


def test_pool_alloc_free_reuse_and_full():
    from adrefine.data.pool import DevicePool, PoolFull
    pool = DevicePool("cuda", 4 * 1024)
    a, b = pool.alloc(1000), pool.alloc(1024)
    assert (a, b) == (0, 1024) and pool.used_bytes == 2048
    pool.free(a)
    assert pool.alloc(700) == 2048          # another size class: not the freed block
    assert pool.alloc(1001) == a            # the same rounded size: reused
    with pytest.raises(MemoryError, match="no room"):
        pool.alloc(2000)
    assert isinstance(PoolFull("x"), MemoryError)
    with pytest.raises(KeyError):
        pool.free(12345)


def test_pool_flush_in_two_rounds_gives_the_same_bytes(g):
    from adrefine.data.pool import DevicePool
    names = list(D.SIZES)[:8]
    outs = []
    for staging in (256 << 20, 60000):  # the native images are 126 KB: 60000 bytes force several rounds
        pool = DevicePool("cuda", 1 << 20, staging_bytes=staging, workers=3)
        ims = []
        for i, n in enumerate(names):
            h, w = g[f"load_img_{i}"].shape[:2]
            im = pool.image(h, w)
            pool.queue(im, lambda n=n: g[f"native_{n}"], g[f"native_{n}"].shape[:2])
            ims.append(im)
        assert pool.flush() == 8 and pool.flush() == 0
        outs.append((pool.rounds, [im.numpy() for im in ims]))
        assert im.dtype == np.uint8 and im.ndim == 3 and im.shape == (h, w, 3) and im.size == h * w * 3
        pool.close()
    assert outs[0][0] == 1 and outs[1][0] >= 2
    for i in range(8):
        assert np.array_equal(outs[0][1][i], g[f"load_img_{i}"]) and np.array_equal(outs[1][1][i], g[f"load_img_{i}"])
    with pytest.raises(ValueError, match="expected"):
        pool = DevicePool("cuda", 1 << 16)
        pool.queue(pool.image(8, 8), lambda: np.zeros((9, 9, 3), np.uint8), (16, 16))
        pool.flush()


def _equal_batch(g, tag, batch):
    assert batch["img"].is_cuda and batch["img"].dtype == torch.uint8
    img = batch["img"].cpu().numpy()
    bad = np.argwhere(img != g[f"{tag}_img"])
    assert img.shape == g[f"{tag}_img"].shape and len(bad) == 0, (tag, len(bad), bad[:5].tolist())
    for k in ("cls", "bboxes", "batch_idx"):
        assert np.array_equal(batch[k].numpy(), g[f"{tag}_{k}"]), (tag, k)
    if f"{tag}_ratio_pad" in g.files:
        assert [Path(f).name for f in batch["im_file"]] == g[f"{tag}_im_file"].tolist()
        assert np.array_equal(np.array(batch["ori_shape"]), g[f"{tag}_ori_shape"])
        rp = np.array([[r[0][0], r[0][1], r[1][0], r[1][1]] for r in batch["ratio_pad"]], dtype=np.float64)
        assert np.array_equal(rp, g[f"{tag}_ratio_pad"])


@pytest.mark.parametrize("cache", ["gpu", None])
@pytest.mark.parametrize("prefetch", [0, 1])
def test_training_and_close_mosaic_passes_equal_the_reference(g, tree, cache, prefetch):
    from adrefine.data.build import build_dataloader
    hyp = D.hyp()
    ds = _ds(tree, cache=cache, augment=True, batch_size=D.TRAIN["batch_size"], pad=0.0, hyp=hyp)
    if cache == "gpu":  # everything resident in index order; the buffer rule left it as the reference's loop would
        assert ds.pool.capacity == ds._resident_bytes() and ds.pool.launches == 1
    ld = build_dataloader(ds, D.TRAIN["collate"], shuffle=False, prefetch=prefetch, sampler=D.TRAIN["order"])
    if cache is None:
        D.seed(D.TRAIN["seed"])
        batches = list(ld)
        assert len(batches) == 3
        for b, batch in enumerate(batches):
            _equal_batch(g, f"train_b{b}", batch)
        assert ds.buffer == [v for v in g["train_buffers"][-1].tolist() if v >= 0]
        # three images were evicted and their blocks went back; the reloads of images 0 and 1 took freed blocks or new
        # ones, and nothing but the buffer is live
        assert not ds._retired and len(ds.pool._size) == len(ds.buffer) == 7
        ds.close_mosaic(hyp)
        ld = build_dataloader(ds, 4, shuffle=False, prefetch=prefetch, sampler=D.CLOSE["order"])
        D.seed(D.CLOSE["seed"])
        (batch,) = list(ld)
        assert ds.buffer == g["close_buffer"].tolist()
        _equal_batch(g, "close_b0", batch)
    else:
        # resident: load_image never appends again, so the buffer stays what the index-order load left and Mosaic
        # draws from it, as the reference does with cache="ram" (the fixture's trainres pass)
        launches = ds.pool.launches
        assert ds.buffer == g["trainres_buffer"].tolist()
        D.seed(D.TRAIN["seed"])
        batches = list(ld)
        assert len(batches) == 3 and ds.pool.launches == launches and ds.buffer == g["trainres_buffer"].tolist()
        for b, batch in enumerate(batches[:D.RESIDENT_N // D.TRAIN["collate"]]):
            _equal_batch(g, f"trainres_b{b}", batch)
        ds.close_mosaic(hyp)
        D.seed(D.CLOSE["seed"])
        (batch,) = list(build_dataloader(ds, 4, shuffle=False, prefetch=prefetch, sampler=D.CLOSE["order"]))
        _equal_batch(g, "close_b0", batch)  # no mosaic: no buffer draw, the same batch as without the cache


@pytest.mark.parametrize("cache", ["gpu", None])
def test_validation_passes_equal_the_reference(g, tree, cache):
    from adrefine.data.build import build_dataloader
    for tag, kw in (("valrect", dict(rect=True, **D.RECT)), ("valsq", dict(rect=False, batch_size=4))):
        ds = _ds(tree, cache=cache, augment=False, **kw)
        # a rect dataset is never shuffled, whatever the argument says
        batches = list(build_dataloader(ds, kw["batch_size"], shuffle=tag == "valrect", prefetch=1))
        assert len(batches) == -(-8 // kw["batch_size"])
        for b, batch in enumerate(batches):
            _equal_batch(g, f"{tag}_b{b}", batch)
        if cache is None:  # every image but the last batch's went back to the pool, and blocks were reused
            assert len(ds.pool._size) == len(batches[-1]["im_file"])


def test_resident_and_host_sources_render_the_same(g, tree):
    """The same plans rendered from the resident pool and from host numpy sources (the fixture's resized arrays,
    uploaded with the batch: the path before the pool) are identical; a mixed batch raises."""
    from adrefine.data.augment import collate_fn, render
    hyp = D.hyp()
    ds = _ds(tree, cache="gpu", augment=True, batch_size=1, pad=0.0, hyp=hyp)
    host = {id(ds.ims[i]): np.ascontiguousarray(g[f"load_img_{i}"]) for i in range(8)}
    D.seed(21)
    samples = [ds[i] for i in (3, 0, 6, 5)]
    dev = collate_fn(samples)["img"]
    plans = [s["img"] for s in samples]
    assert any(len(p.tiles) > 1 for p in plans)
    import copy
    hplans = []
    for p in plans:
        q = copy.copy(p)
        q.tiles = [(host[id(t[0])],) + tuple(t[1:]) for t in p.tiles]
        hplans.append(q)
    ref = render(hplans, "cuda")
    torch.cuda.synchronize()
    assert torch.equal(dev, ref)
    hplans[1].tiles = list(plans[1].tiles)
    with pytest.raises(ValueError, match="mixes host and device"):
        render(hplans, "cuda")
    other = _ds(tree, cache="gpu", augment=False, batch_size=4)
    with pytest.raises(ValueError, match="two pools"):
        collate_fn([samples[0], dict(samples[1], img=other[0]["img"])])


def test_dataset_to_trainer_and_validator(g, tmp_path):
    """An 8-image directory at imgsz 320 (the fixture's images tiled up) -> build_yolo_dataset -> build_dataloader
    -> two FusedTrainer steps with finite losses; one val batch through DetectionValidator."""
    from types import SimpleNamespace

    from adrefine.data.build import build_dataloader, build_yolo_dataset
    from adrefine.engine.trainer import FusedTrainer
    from adrefine.engine.validator import DetectionValidator
    from adrefine.nn.tasks import DetectionModel
    imgs = {n: np.tile(g[f"native_{n}"], (4, 4, 1)) for n in list(D.SIZES)[:8]}
    tree = str(D.write_tree(tmp_path / "big", imgs))
    data = {"names": {i: str(i) for i in range(80)}}
    cfg = SimpleNamespace(**vars(D.hyp()), imgsz=320, rect=False, cache="gpu", single_cls=False, task="detect",
                          classes=None, fraction=1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        train = build_yolo_dataset(cfg, tree, 4, data, mode="train")
        val = build_yolo_dataset(cfg, tree, 4, data, mode="val")
    m = DetectionModel(str(CFG))
    load_recipe_into(m)
    tr = FusedTrainer(m.cuda(), lr0=0.01, momentum=0.937, weight_decay=5e-4, nbs=4, batch_size=4)
    D.seed(0)
    batches = list(build_dataloader(train, 4, shuffle=True, prefetch=1))
    assert len(batches) == 2 and tuple(batches[0]["img"].shape) == (4, 3, 320, 320)
    for batch in batches:
        items = tr.step(batch)
        assert torch.isfinite(items).all(), items
    vm = DetectionModel(str(CFG), compute_dtype=torch.float32)
    load_recipe_into(vm)
    v = DetectionValidator(vm.cuda().eval(), nc=80)
    res = v([next(iter(build_dataloader(val, 4, shuffle=False, prefetch=0)))])
    assert res["seen"] == 4 and np.isfinite(res["fitness"])
