"""CPU: MixUp in the augmentation chain (adrefine/data/augment.py; reference data/augment.py:318-435, 866-949) against
fixtures made by running the reference's own chain and its own YOLODataset (scripts/gen_mixup_golden.py): the RNG
draws, the label concatenation and the two-layer plans. The plans are materialised by the numpy executor of
tests/mixup_util.py (the float64 blend as numpy evaluates the reference's expression); tests/test_gpu_mixup.py renders
the same plans with adr_augment_mix_u8."""
import warnings

import numpy as np
import pytest
import torch

import aug_util as A
import dataset_util as D
import mixup_util as X
from conftest import golden


def _labels_equal(out, g, tag=""):
    cls = torch.cat([o["cls"] for o in out]).numpy()
    bboxes = torch.cat([o["bboxes"] for o in out]).numpy()
    bidx = torch.cat([o["batch_idx"] + i for i, o in enumerate(out)]).numpy()
    assert np.array_equal(cls, g[f"{tag}cls"]) and np.array_equal(bidx, g[f"{tag}batch_idx"])
    assert bboxes.dtype == g[f"{tag}bboxes"].dtype and np.array_equal(bboxes, g[f"{tag}bboxes"])


def test_chain_labels_and_plans_vs_reference():
    g = golden(X.AUG["name"])
    assert g["order"].tolist() == X.AUG["order"] and int(g["imgsz"]) == X.AUG["imgsz"]
    out = X.run_chain(int(g["seed"]))
    mixed = [o["img"].mix is not None for o in out]
    assert mixed == g["mixed"].tolist() and sum(mixed) >= 2 and not all(mixed)
    for o, r in zip(out, g["ratio"].tolist()):
        if o["img"].mix is not None:
            q, r1, r2 = o["img"].mix
            assert r1 == r and r2 == 1 - r and q.size == o["img"].size == (256, 256)
            assert q.lut is None and not (q.flip_ud or q.flip_lr) and q.mix is None and q.M is not None
    _labels_equal(out, g)
    for i, o in enumerate(out):
        img = X.execute_plan(o["img"])
        diff = int(np.abs(img.astype(np.int32) - g["img"][i].astype(np.int32)).max())
        assert img.shape == g["img"][i].shape and diff == 0, (i, diff)


def test_truncation_not_rounding_is_pinned():
    """The fixture tells truncation from rounding, and an FMA-style blend (one product unrounded) from numpy's."""
    g = golden(X.AUG["name"])
    out = X.run_chain(int(g["seed"]))
    i = g["mixed"].tolist().index(True)
    p = out[i]["img"]
    q, r, omr = p.mix
    a, b = X.execute_layer(p).astype(np.float64), X.execute_layer(q).astype(np.float64)
    assert ((a * r + b * omr).astype(np.uint8) != np.rint(a * r + b * omr)).any()
    # where both layers show the border, a ratio exists for which the reference's blend gives 113: the kernel's case
    r113, r114 = X.border_ratio(113), X.border_ratio(114)
    assert int(114 * r113 + 114 * (1 - r113)) == 113 and int(114 * r114 + 114 * (1 - r114)) == 114


def _lookup(g):
    by_src = {g[f"native_{n}"].tobytes(): g[f"load_img_{i}"] for i, n in enumerate(list(D.SIZES)[:8])}
    return lambda src, hw: by_src[src.tobytes()]


def _ds(tree, hyp, pool, **kw):
    from adrefine.data.dataset import YOLODataset
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the duplicate row and the corrupt pair
        return YOLODataset(**dict(dict(img_path=tree, imgsz=D.IMGSZ, cache=None, hyp=hyp, data={"names": D.NAMES},
                                       pool=pool, augment=True, pad=0.0), **kw))


@pytest.mark.parametrize("tag", list(X.DATASET))
def test_dataset_pass_vs_reference(tag, tmp_path):
    """Our YOLODataset with mixup 1.0 against the reference's own on the same tree: the buffer after every sample
    (both load_image calls of a sample append and evict as the reference's do), the collated labels, and the images
    through the plan executor; "half": letterboxed layers meet mosaic layers."""
    tiny, g = golden("dataset_tiny"), golden("dataset_mixup_tiny")
    cfg = X.DATASET[tag]
    tree = str(D.write_tree(tmp_path / "tiny", D.fixture_images(tiny)))
    pool = D.HostPool(_lookup(tiny))
    ds = _ds(tree, X.dataset_hyp(tag), pool, batch_size=cfg["batch_size"])
    assert ds.max_buffer_length == 8 and int(g[f"{tag}_seed"]) == cfg["seed"]
    D.seed(cfg["seed"])
    samples = []
    for k, i in enumerate(cfg["order"]):
        ds.begin_batch(k // cfg["collate"])
        samples.append(ds[i])
        want = [v for v in g[f"{tag}_buffers"][k].tolist() if v >= 0]
        assert ds.buffer == want, (k, ds.buffer, want)
        p = samples[-1]["img"]
        assert p.mix is not None
        mosaics = sum(q.canvas == (2 * D.IMGSZ, 2 * D.IMGSZ) for q in p.layers())  # else letterboxed: 64 x 64
        assert mosaics == int(g[f"{tag}_mosaics"][k]), (k, mosaics)
    assert 1 in g[f"{tag}_mosaics"].tolist() or tag == "mix"
    assert pool.frees == 0  # nothing goes back before its batch has been rendered
    for b in range(len(samples) // cfg["collate"]):
        part = samples[b * cfg["collate"]:(b + 1) * cfg["collate"]]
        _labels_equal(part, g, f"{tag}_b{b}_")
        img = np.stack([X.execute_plan(s["img"]) for s in part])
        assert np.array_equal(img, g[f"{tag}_b{b}_img"]), (tag, b)
    freed = sum(ds.end_batch(b) for b in range(len(samples) // cfg["collate"]))
    assert freed == pool.frees and len(pool.live) == len(ds.buffer) and not ds._retired


def test_pool_slots_doubles_in_flight_term_with_mixup(tmp_path):
    tiny = golden("dataset_tiny")
    tree = str(D.write_tree(tmp_path / "tiny", D.fixture_images(tiny)))
    slots = {}
    for mixup in (0.0, 0.15):
        h = D.hyp()
        h.mixup = mixup
        ds = _ds(tree, h, D.HostPool(), batch_size=2, inflight=3)
        slots[mixup] = ds.pool_slots()
        assert ds.max_buffer_length == 8
    assert slots[0.0] == 8 + 3 * 2 and slots[0.15] == 8 + 2 * 3 * 2
    h = D.hyp()
    h.mixup = 0.15
    val = _ds(tree, h, D.HostPool(), batch_size=2, inflight=3, augment=False)
    assert val.pool_slots() == 4 * 2  # validation: no buffer, no MixUp


def _plans():
    rs = np.random.RandomState(0)
    from adrefine.data.augment import ImagePlan
    return [ImagePlan(rs.randint(0, 256, (24, 32, 3)).astype(np.uint8)) for _ in range(2)]


def test_mix_stage_order_is_enforced():
    from adrefine.data.augment import ImagePlan, LetterBox, RandomFlip, RandomHSV, _letterbox_geometry
    from adrefine.data.instance import Instances
    lut = np.zeros((3, 256), np.uint8)
    for spoil in ("lut", "flip_ud", "flip_lr", "resize", "mix"):
        for which in (0, 1):  # neither layer may carry a later stage
            a, b = _plans()
            bad = (a, b)[which]
            if spoil == "lut":
                bad.lut = lut
            elif spoil == "resize":
                bad = bad.letterbox((16, 12), 8, 6, 8, 6)
                assert bad.resize is not None
                a, b = (bad, b) if which == 0 else (a, bad)
            elif spoil == "mix":
                bad.mixup(ImagePlan(np.zeros((24, 32, 3), np.uint8)), 0.5)
            else:
                setattr(bad, spoil, True)
            with pytest.raises(NotImplementedError):
                a.mixup(b, 0.5)
    a, b = _plans()
    b.size = (16, 12)
    with pytest.raises(NotImplementedError, match="sizes"):
        a.mixup(b, 0.5)
    # after the mix: HSV and flips go on; a letterbox or a warp do not; render_letterbox does not take the plan
    a, b = _plans()
    a.mixup(b, 0.25)
    assert a.mix[1:] == (0.25, 0.75) and a.layers() == (a, b) and b.layers() == (b,)
    with pytest.raises(ValueError, match="mix"):
        _letterbox_geometry(a)
    with pytest.raises(NotImplementedError, match="letterbox"):
        LetterBox((64, 64))(image=a)
    with pytest.raises(NotImplementedError, match="warp"):
        a._stage(True, "warp")
    np.random.seed(0)
    ins = Instances(np.zeros((0, 4), np.float32), None, None, bbox_format="xywh", normalized=True)
    labels = RandomFlip(p=1.0, direction="horizontal")(RandomHSV()({"img": a, "instances": ins}))
    assert labels["img"] is a and a.lut is not None and a.flip_lr and a.mix[0] is b


def test_source_pool_sees_both_layers():
    from adrefine.data.augment import ImagePlan, _source_pool

    class Pool:
        pass

    class Dev:  # what data/pool.py's DeviceImage shows a plan
        def __init__(self, pool, off=0):
            self.pool, self.off = pool, off
            self.shape, self.dtype, self.ndim, self.size = (24, 32, 3), np.uint8, 3, 2304

    p1, p2 = Pool(), Pool()

    def mixed(s1, s2):
        a, b = ImagePlan(s1), ImagePlan(s2)
        a.mixup(b, 0.5)
        return [a]

    host = np.zeros((24, 32, 3), np.uint8)
    assert _source_pool(mixed(host, host), "t") is None
    assert _source_pool(mixed(Dev(p1), Dev(p1)), "t") is p1
    with pytest.raises(ValueError, match="host and device"):
        _source_pool(mixed(Dev(p1), host), "t")
    with pytest.raises(ValueError, match="two pools"):
        _source_pool(mixed(Dev(p1), Dev(p2)), "t")
    with pytest.raises(ValueError, match="released"):
        _source_pool(mixed(Dev(p1), Dev(p1, None)), "t")


def test_mixup_zero_leaves_the_chain_as_it_was():
    """mixup 0.0: the RNG stream (one uniform draw in BaseMixTransform.__call__) and the plans are what they were:
    aug_default_256 still comes out, and no plan has a mix stage."""
    g = golden("aug_default_256")
    out = A.run_chain("aug_default_256")
    assert all(o["img"].mix is None for o in out)
    _labels_equal(out, g)
    for i, o in enumerate(out):
        assert np.array_equal(X.execute_plan(o["img"]), g["img"][i]) and \
            np.array_equal(A.execute_plan(o["img"]), g["img"][i])
