"""CPU: YOLODataset / build_dataloader (adrefine/data/dataset.py, build.py) against tests/golden/dataset_tiny.npz, the
record of the reference's own YOLODataset on the same tiny directory (scripts/gen_dataset_golden.py), with a host
stand-in for the device pool (dataset_util.HostPool); and adr_resize_u8's entry validation (no launch)."""
import ctypes
import threading
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

import aug_util as A
import dataset_util as D
import letterbox_util as U
from conftest import golden


@pytest.fixture(scope="module")
def g():
    return golden("dataset_tiny")


@pytest.fixture()
def tree(g, tmp_path):
    return str(D.write_tree(tmp_path / "tiny", D.fixture_images(g)))


def _lookup(g):
    """HostPool.lookup: the fixture's reference-resized image of a decoded source."""
    by_src = {g[f"native_{n}"].tobytes(): g[f"load_img_{i}"] for i, n in enumerate(list(D.SIZES)[:8])}

    def lookup(src, hw):
        out = by_src[src.tobytes()]
        assert out.shape[:2] == tuple(hw)
        return out
    return lookup


def _ds(tree, pool=None, quiet=True, **kw):
    from adrefine.data.dataset import YOLODataset
    kw = dict(dict(img_path=tree, imgsz=D.IMGSZ, cache=None, hyp=D.hyp(), data={"names": D.NAMES},
                   pool=pool if pool is not None else D.HostPool()), **kw)
    with warnings.catch_warnings():
        if quiet:  # the duplicate row and the corrupt pair warn whenever the labels are verified anew
            warnings.simplefilter("ignore")
        return YOLODataset(**kw)


def _execute(p):
    return U.execute_chw(p) if p.resize is not None else A.execute_plan(p)


def _check_batch(g, tag, samples):
    img = np.stack([_execute(s["img"]) for s in samples])
    assert np.array_equal(img, g[f"{tag}_img"]), tag
    for k in ("cls", "bboxes"):
        assert np.array_equal(torch.cat([s[k] for s in samples], 0).numpy(), g[f"{tag}_{k}"]), (tag, k)
    bi = torch.cat([s["batch_idx"] + i for i, s in enumerate(samples)], 0).numpy()
    assert np.array_equal(bi, g[f"{tag}_batch_idx"]), tag
    if f"{tag}_ratio_pad" in g.files:
        assert [Path(s["im_file"]).name for s in samples] == g[f"{tag}_im_file"].tolist()
        assert np.array_equal(np.array([s["ori_shape"] for s in samples]), g[f"{tag}_ori_shape"])
        assert np.array_equal(np.array([tuple(int(v) for v in s["resized_shape"]) for s in samples]),
                              g[f"{tag}_resized_shape"])
        rp = np.array([[s["ratio_pad"][0][0], s["ratio_pad"][0][1], s["ratio_pad"][1][0], s["ratio_pad"][1][1]]
                       for s in samples], dtype=np.float64)
        assert np.array_equal(rp, g[f"{tag}_ratio_pad"])


def test_files_labels_and_shapes(g, tree):
    with pytest.warns(UserWarning, match="ignoring corrupt image/label"):
        ds = _ds(tree, quiet=False, augment=False, batch_size=4)
    assert [Path(f).name for f in ds.im_files] == g["im_files"].tolist()
    assert ds.ni == 8 and len(ds) == 8
    for i, lb in enumerate(ds.labels):
        assert lb["cls"].dtype == np.float32 and lb["cls"].shape[1:] == (1,) and lb["bboxes"].shape[1:] == (4,)
        assert np.array_equal(lb["cls"], g[f"labels_cls_{i}"]) and np.array_equal(lb["bboxes"], g[f"labels_bboxes_{i}"])
        assert tuple(lb["shape"]) == tuple(g[f"labels_shape_{i}"])
        assert lb["normalized"] is True and lb["bbox_format"] == "xywh" and lb["im_file"] == ds.im_files[i]
    assert len(ds.labels[1]["cls"]) == 3                                  # im2: the duplicated row is gone
    assert ds.labels[3]["bboxes"].shape == (0, 4) and ds.labels[4]["bboxes"].shape == (0, 4)  # empty, missing


def test_update_labels_classes_single_cls(g, tree):
    ds = _ds(tree, augment=False, batch_size=4, classes=D.CLASSES, single_cls=True)
    for i, lb in enumerate(ds.labels):
        assert np.array_equal(lb["cls"], g[f"labels_sel_cls_{i}"])
        assert np.array_equal(lb["bboxes"], g[f"labels_sel_bboxes_{i}"])
    assert sum(len(lb["cls"]) for lb in ds.labels) < sum(len(g[f"labels_cls_{i}"]) for i in range(8))


def test_set_rectangle(g, tree):
    ds = _ds(tree, augment=False, rect=True, **D.RECT)
    assert [Path(f).name for f in ds.im_files] == g["rect_im_files"].tolist()
    assert np.array_equal(ds.batch_shapes, g["rect_batch_shapes"]) and np.array_equal(ds.batch, g["rect_batch"])
    assert all("shape" not in lb for lb in ds.labels)


def test_load_image_shapes_and_pixels(g, tree):
    """(h0, w0), (h, w) of all eight images; through the stand-in pool's cv2.resize restatement the pixels too
    (image 8 from its .npy sibling: its PNG holds zeros)."""
    pool = D.HostPool()
    ds = _ds(tree, pool=pool, augment=False, batch_size=4)
    for i in range(8):
        im, hw0, hw = ds.load_image(i)
        assert tuple(hw0) == tuple(g[f"load_hw0_{i}"]) and tuple(hw) == tuple(g[f"load_hw_{i}"])
        assert im.shape == g[f"load_img_{i}"].shape and np.array_equal(im, g[f"load_img_{i}"]), i
    assert not ds.buffer and pool.allocs == 8


def test_seeded_training_and_close_mosaic_pass(g, tree):
    """The buffer after every sample, the evictions, and the collated batches (labels bit-exact; images through the
    CPU plan executor of aug_util) of the seeded training pass and of the close-mosaic pass that follows it."""
    pool = D.HostPool(_lookup(g))
    hyp = D.hyp()
    ds = _ds(tree, pool=pool, augment=True, batch_size=D.TRAIN["batch_size"], pad=0.0, hyp=hyp)
    assert ds.max_buffer_length == 8
    D.seed(D.TRAIN["seed"])
    samples = []
    for k, i in enumerate(D.TRAIN["order"]):
        ds.begin_batch(k // D.TRAIN["collate"])
        samples.append(ds[i])
        want = [v for v in g["train_buffers"][k].tolist() if v >= 0]
        assert ds.buffer == want, (k, ds.buffer, want)
        assert [j for j in range(8) if ds.ims[j] is not None] == sorted(set(want))  # evicted images are dropped
    nb = len(samples) // D.TRAIN["collate"]
    for b in range(nb):
        _check_batch(g, f"train_b{b}", samples[b * 4:b * 4 + 4])
    assert pool.frees == 0                       # nothing goes back before its batch has been rendered
    assert ds.end_batch(0) == 0 and ds.end_batch(1) == 1 and ds.end_batch(2) == 2 and pool.frees == 3
    assert len(pool.live) == len(ds.buffer) == 7
    ds.close_mosaic(hyp)
    D.seed(D.CLOSE["seed"])
    ds.begin_batch(nb)
    samples = [ds[i] for i in D.CLOSE["order"]]
    assert ds.buffer == g["close_buffer"].tolist()
    _check_batch(g, "close_b0", samples)


def test_validation_passes(g, tree):
    for tag, kw in (("valrect", dict(rect=True, **D.RECT)), ("valsq", dict(rect=False, batch_size=4))):
        pool = D.HostPool(_lookup(g))
        ds = _ds(tree, pool=pool, augment=False, **kw)
        bs = kw["batch_size"]
        for b, k in enumerate(range(0, ds.ni, bs)):
            ds.begin_batch(b)
            _check_batch(g, f"{tag}_b{b}", [ds[i] for i in range(k, min(k + bs, ds.ni))])
            ds.end_batch(b)
        # a validation image is freed once the batch after its own is done: the last batch's are still live
        assert pool.frees == ds.ni - len(range(k, ds.ni)) and len(pool.live) == ds.ni - pool.frees


def test_cache_modes(tree):
    for c in ("ram", "disk", True):
        with pytest.raises(NotImplementedError, match="gpu"):
            _ds(tree, cache=c)
    pool = D.HostPool()
    ds = _ds(tree, pool=pool, cache="gpu", augment=True, batch_size=1)
    assert all(im is not None for im in ds.ims) and pool.allocs == 8 and pool.flushes == 1
    before = list(ds.buffer)
    assert before == [1, 2, 3, 4, 5, 6, 7]       # index order; the reference's rule popped image 0
    D.seed(3)
    ds[0]
    assert ds.buffer == before and pool.allocs == 8 and not ds._retired  # resident: nothing loaded, nothing evicted


def test_npy_sibling_of_another_shape(g, tmp_path):
    """The reference takes (h0, w0) from whatever it loaded: a .npy sibling's shape wins over the image header's for
    load_image, while the label record keeps the header's."""
    root = tmp_path / "npy"
    D.write_tree(root, {"im1": g["native_im1"]})
    np.save(root / "images" / "im1.npy", g["native_im4"])  # 40 x 64 beside a 17 x 23 PNG
    ds = _ds(str(root / "images"), augment=False, batch_size=1)
    im, hw0, hw = ds.load_image(0)
    assert tuple(ds.labels[0]["shape"]) == (17, 23) and hw0 == (40, 64) and hw == (40, 64)
    assert np.array_equal(im, g["native_im4"])


def test_segment_rows_raise(g, tmp_path):
    root = tmp_path / "seg"
    D.write_tree(root, {"im1": g["native_im1"]})
    (root / "labels" / "im1.txt").write_text("0 0.1 0.1 0.5 0.1 0.5 0.5 0.1 0.5\n")
    with pytest.raises(NotImplementedError, match="segment"):
        _ds(str(root / "images"))


def test_label_cache_roundtrip_and_rebuild(g, tree):
    ds = _ds(tree, augment=False, batch_size=4)
    cache = Path(tree).parent / "labels.adrcache.npz"
    assert not ds.label_cache_hit and cache.exists() and not (Path(tree).parent / "labels.cache").exists()
    ds2 = _ds(tree, augment=False, batch_size=4)
    assert ds2.label_cache_hit and ds2.im_files == ds.im_files
    for a, b in zip(ds.labels, ds2.labels):
        assert np.array_equal(a["cls"], b["cls"]) and np.array_equal(a["bboxes"], b["bboxes"])
        assert tuple(a["shape"]) == tuple(b["shape"]) and a["cls"].dtype == b["cls"].dtype == np.float32
    lb = Path(tree).parent / "labels" / "im7.txt"
    lb.write_text(lb.read_text() + "0 0.25 0.25 0.125 0.125\n")  # another size: another hash
    ds3 = _ds(tree, augment=False, batch_size=4)
    assert not ds3.label_cache_hit and len(ds3.labels[6]["cls"]) == 2
    assert _ds(tree, augment=False, batch_size=4).label_cache_hit


class _Plain:
    """A dataset of indices for the loader's order tests."""
    rect = False

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i

    @staticmethod
    def collate_fn(batch):
        return list(batch)


class _Bad(_Plain):
    def __getitem__(self, i):
        return 1 // (3 - i)


def test_dataloader_order_and_split():
    from adrefine.data.build import SEED, build_dataloader
    assert SEED == 6148914691236517205
    ld = build_dataloader(_Plain(11), 4, shuffle=True, prefetch=0)
    gen = torch.Generator().manual_seed(SEED - 1)  # rank -1
    for _ in range(2):  # every epoch draws the generator's next permutation
        want = torch.randperm(11, generator=gen).tolist()
        got = list(ld)
        assert len(ld) == 3 and [len(b) for b in got] == [4, 4, 3] and sum(got, []) == want
    assert sum(list(build_dataloader(_Plain(11), 4, shuffle=False, prefetch=1)), []) == list(range(11))
    parts = []
    for rank in (0, 1):
        ld = build_dataloader(_Plain(11), 4, shuffle=True, rank=rank, world_size=2, prefetch=0)
        ld.set_epoch(3)
        ref = torch.utils.data.DistributedSampler(_Plain(11), num_replicas=2, rank=rank, shuffle=True)
        ref.set_epoch(3)
        got = sum(list(ld), [])
        assert got == list(ref) and len(got) == 6 and len(ld) == 2  # ceil(11 / 2): one padded index
        parts.append(got)
    assert set(parts[0]) | set(parts[1]) == set(range(11))
    rect = _Plain(5)
    rect.rect = True
    assert sum(list(build_dataloader(rect, 2, shuffle=True, prefetch=0)), []) == list(range(5))


def test_dataloader_prefetch_is_invisible(g, tree, monkeypatch):
    """prefetch 0 and 2 yield the same batches (compared at the plan level: collate_fn replaced by the CPU executor),
    and an error in the background thread reaches the caller."""
    from adrefine.data import build as Bd
    outs = []
    for prefetch in (0, 2):
        pool = D.HostPool(_lookup(g))
        ds = _ds(tree, pool=pool, augment=True, batch_size=2, pad=0.0, inflight=3)
        monkeypatch.setattr(ds, "collate_fn", lambda samples: [
            (_execute(s["img"]), s["cls"].numpy(), s["bboxes"].numpy()) for s in samples], raising=False)
        ld = Bd.build_dataloader(ds, 3, shuffle=True, prefetch=prefetch)
        D.seed(5)
        epoch = [b for _ in range(2) for b in ld]
        assert [len(b) for b in epoch] == [3, 3, 2, 3, 3, 2] and pool.flushes == 6
        assert len(pool.live) == len(ds.buffer) and not ds._retired  # every evicted image went back
        outs.append(epoch)
    for a, b in zip(*outs):
        for (ia, ca, ba), (ib, cb, bb) in zip(a, b):
            assert np.array_equal(ia, ib) and np.array_equal(ca, cb) and np.array_equal(ba, bb)
    with pytest.raises(ValueError, match="inflight"):
        Bd.build_dataloader(_ds(tree, augment=True, batch_size=2), 2, prefetch=2)
    with pytest.raises(ZeroDivisionError):
        list(Bd.build_dataloader(_Bad(4), 2, shuffle=False, prefetch=1))


class _BoundedPool(D.HostPool):
    """HostPool with the capacity a DevicePool made by the dataset would have (YOLODataset.pool_slots), and a flush
    that is as slow as a flush can be: it returns only when the background thread has gone as far ahead as the loader
    lets it (it has asked to begin the batch prefetch + 1 places on, or the epoch's last one). No clock is involved."""

    def __init__(self, lookup):
        super().__init__(lookup)
        self.slots, self.peak = None, 0
        self.cv = threading.Condition()
        self.asked, self.flushed, self.ahead, self.last = -1, 0, 0, 0

    def image(self, h, w):
        if len(self.live) >= self.slots:
            raise MemoryError(f"pool full: {len(self.live)} live of {self.slots}")
        a = super().image(h, w)
        self.peak = max(self.peak, len(self.live))
        return a

    def flush(self):
        with self.cv:
            want = min(self.flushed + self.ahead, self.last)
            assert self.cv.wait_for(lambda: self.asked >= want, timeout=60), "the background thread never got there"
            self.flushed += 1
        return super().flush()


@pytest.mark.parametrize("augment", [True, False])
def test_dataloader_never_outruns_the_pool(g, tmp_path, augment):
    """The iterating thread as the bottleneck, the pool exactly as large as the dataset sizes it (cache=None, the
    default inflight 2 with the default prefetch 1): however far the background thread runs ahead, at most
    prefetch + 1 batches are begun and not ended, and the pool never fills; training and validation."""
    from adrefine.data import build as Bd
    n, bs, prefetch = 40, 4, 1
    imgs = {f"im{k:02d}": g[f"native_im{1 + k % 8}"] for k in range(n)}
    saved = dict(D.LABEL_TEXTS)
    try:
        for k, name in enumerate(imgs):
            D.LABEL_TEXTS[name] = saved[f"im{1 + k % 8}"]
        tree = str(D.write_tree(tmp_path / "many", imgs))
    finally:
        D.LABEL_TEXTS.clear()
        D.LABEL_TEXTS.update(saved)
    pool = _BoundedPool(_lookup(g))
    ds = _ds(tree, pool=pool, augment=augment, batch_size=bs, pad=0.0)
    assert ds.inflight == prefetch + 1
    pool.slots = ds.pool_slots()
    assert pool.slots == (min(n, 8 * bs) + 2 * bs if augment else 3 * bs)
    ld = Bd.build_dataloader(ds, bs, shuffle=augment, prefetch=prefetch)
    begun, ended, worst = [0], [0], [0]
    admit, begin, end = ld._admit, ds.begin_batch, ds.end_batch

    def _admit(seq, permits, stop):
        with pool.cv:
            pool.asked = seq
            pool.cv.notify_all()
        return admit(seq, permits, stop)

    def _begin(k):
        begun[0] += 1
        worst[0] = max(worst[0], begun[0] - ended[0])
        return begin(k)

    def _end(k):
        out = end(k)
        ended[0] += 1
        return out

    ld._admit, ds.begin_batch, ds.end_batch = _admit, _begin, _end
    ds.collate_fn = lambda samples: len(samples)
    D.seed(9)
    for epoch in range(2):
        pool.ahead, pool.last = prefetch + 1, ds.batches_built + len(ld) - 1
        assert sum(ld) == n
    assert worst[0] == prefetch + 1 and begun[0] == ended[0] == 2 * len(ld)
    assert bs < pool.peak <= pool.slots


def test_build_yolo_dataset_argument_mapping(tree, monkeypatch):
    from types import SimpleNamespace

    from adrefine.data import build as Bd
    seen = {}
    monkeypatch.setattr(Bd, "YOLODataset", lambda **kw: seen.update(kw) or kw)
    cfg = SimpleNamespace(**vars(D.hyp()), imgsz=64, rect=False, cache=False, single_cls=False, task="detect",
                          classes=None, fraction=0.5)
    Bd.build_yolo_dataset(cfg, tree, 4, {"names": D.NAMES}, mode="train")
    assert (seen["augment"], seen["pad"], seen["fraction"], seen["rect"], seen["cache"]) == (True, 0.0, 0.5, False, None)
    Bd.build_yolo_dataset(cfg, tree, 4, {"names": D.NAMES}, mode="val", rect=True, stride=32.0)
    assert (seen["augment"], seen["pad"], seen["fraction"], seen["rect"], seen["stride"]) == (False, 0.5, 1.0, True, 32)


# ---- adr_resize_u8: the entry validates the host descriptors and launches nothing ----

def _entry():
    from adrefine.data.pool import ResizeDesc
    from adrefine.native import LIB_PATH
    lib = ctypes.CDLL(str(LIB_PATH))
    lib.adr_resize_u8.restype = ctypes.c_int
    lib.adr_resize_u8.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                  ctypes.c_void_p]
    lib.adr_last_error.restype = ctypes.c_char_p
    assert lib.adr_resize_desc_size() == ctypes.sizeof(ResizeDesc) == 40
    return lib, ResizeDesc


def _descs(R, rows):
    d = (R * len(rows))()
    for i, r in enumerate(rows):
        (d[i].src_off, d[i].dst_off, d[i].sw, d[i].sh, d[i].nw, d[i].nh, d[i].mode, d[i].tab_off) = r
    return d


GOOD, SRC_BYTES, DST_BYTES, NTAB = D.RESIZE_GOOD, D.RESIZE_SRC_BYTES, D.RESIZE_DST_BYTES, D.RESIZE_NTAB
# what: (changed sizes, descriptors, the message the entry must give)
BAD = {
    "source past src_bytes": (dict(src=SRC_BYTES - 1), GOOD, "image 2 source outside"),
    "destination past dst_bytes": (dict(dst=512 + 44), GOOD, "image 2 destination outside"),
    "overlapping destinations": ({}, [GOOD[0], (192, 128, 8, 8, 4, 4, 2, 0)], "overlap"),
    "mode 2 without an exact 2x": ({}, [(0, 0, 8, 8, 4, 3, 2, 0)], "image 0 area path"),
    "tables past ntab": (dict(ntab=NTAB - 1), GOOD, "image 2 tables"),
    "copy mode with a resize": ({}, [(0, 0, 8, 8, 4, 4, 0, 0)], "image 0 copy mode"),
    "empty image": ({}, [(0, 0, 8, 8, 0, 4, 1, 0)], "image 0 sizes"),
    "destination not dword aligned": ({}, [(0, 2, 8, 8, 8, 8, 0, 0)], "image 0 destination not 4-byte aligned"),
    "negative source offset": ({}, [(-1, 0, 8, 8, 8, 8, 0, 0)], "image 0 source outside"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_resize_entry_rejects(what):
    """Null stream, host-side fake device pointers that are never dereferenced: a rejected call launches nothing (a
    launch would need a device), and the message names the violated rule. The GOOD descriptors with the true sizes
    are launched in tests/test_gpu_dataset.py::test_resize_good_descriptors_launch."""
    lib, R = _entry()
    kw, rows, message = BAD[what]
    d = _descs(R, rows)
    buf = ctypes.create_string_buffer(1024)  # stands for every device pointer; 4-byte aligned
    p = ctypes.c_void_p(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16)
    rc = lib.adr_resize_u8(p, kw.get("src", SRC_BYTES), p, ctypes.cast(d, ctypes.c_void_p), p, len(rows), p,
                           kw.get("ntab", NTAB), p, kw.get("dst", DST_BYTES), None)
    assert rc != 0, what
    err = lib.adr_last_error().decode()
    assert err.startswith("resize:") and message in err, (what, err)


def test_resize_good_descriptors_are_consistent():
    """The rejected cases differ from a valid launch only in the one thing they name (sizes checked here on the host;
    the valid launch itself runs in the GPU suite)."""
    from adrefine.data.pool import resize_mode, resize_prefix
    for s, dst, sw, sh, nw, nh, mode, tab in GOOD:
        assert s + sw * sh * 3 <= SRC_BYTES and dst + nw * nh * 3 <= DST_BYTES and dst % 256 == 0
        assert resize_mode(sw, sh, nw, nh) == mode
    assert 3 * (5 + 3) == NTAB
    assert resize_prefix([(8, 8), (4, 4), (640, 640)]).tolist() == [0, 1, 2]
    assert resize_prefix([(640, 640), (10, 10)]).tolist() == [0, 1200]
