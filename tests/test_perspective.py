"""CPU: RandomPerspective with perspective > 0 in the augmentation chain (adrefine/data/augment.py; reference
data/augment.py:1016-1077, 1079-1110) against fixtures made by running the reference's own chain and its own
YOLODataset (scripts/gen_perspective_golden.py): the RNG draws, the float32 3x3 product, the xy / w branch of
apply_bboxes and the plans with P. The plans are materialised by the numpy executor of tests/perspective_util.py (the
restatement of cv2.warpPerspective); tests/test_gpu_perspective.py renders the same plans with the kernel."""
import random
import warnings

import numpy as np
import pytest
import torch

import aug_util as A
import dataset_util as D
import perspective_util as P
from conftest import golden


def _labels_equal(out, g, tag=""):
    cls = torch.cat([o["cls"] for o in out]).numpy()
    bboxes = torch.cat([o["bboxes"] for o in out]).numpy()
    bidx = torch.cat([o["batch_idx"] + i for i, o in enumerate(out)]).numpy()
    assert np.array_equal(cls, g[f"{tag}cls"]) and np.array_equal(bidx, g[f"{tag}batch_idx"])
    assert bboxes.dtype == g[f"{tag}bboxes"].dtype and np.array_equal(bboxes, g[f"{tag}bboxes"])


@pytest.fixture(scope="module")
def chain():
    g = golden(P.AUG["name"])
    assert g["order"].tolist() == P.AUG["order"] and int(g["imgsz"]) == P.AUG["imgsz"]
    return g, P.run_chain(int(g["seed"]))


def test_chain_labels_and_plans_vs_reference(chain):
    g, out = chain
    mixed = [o["img"].mix is not None for o in out]
    assert mixed == g["mixed"].tolist() and any(mixed) and not all(mixed)
    for o in out:
        for q in o["img"].layers():  # every layer is a warped mosaic: the whole float32 3x3, not its first rows
            assert q.M is None and q.P.shape == (3, 3) and q.P.dtype == np.float32 and q.size == (256, 256)
            assert q.P[2, 0] != 0 and q.P[2, 1] != 0
    _labels_equal(out, g)


def test_chain_images_vs_reference(chain):
    g, out = chain
    for i, o in enumerate(out):
        img = P.execute_plan(o["img"])
        bad = np.argwhere(img != g["img"][i])
        assert img.shape == g["img"][i].shape and len(bad) == 0, (i, len(bad), bad[:5].tolist())


def test_fixture_tells_perspective_from_affine(chain):
    """With the third row dropped (what a plan holding M[:2] would render) the images are different ones."""
    g, out = chain
    p = out[g["mixed"].tolist().index(False)]["img"]
    affine = A.cv2_oracle.warpAffine(P.execute_layer(_without_warp(p)), p.P[:2], dsize=p.size,
                                     borderValue=(114, 114, 114))
    assert (affine != P.execute_layer(p)).any(-1).mean() > 0.1


def _without_warp(p):
    import copy
    q = copy.copy(p)
    q.P, q.size = None, p.canvas
    return q


def _lookup(g):
    by_src = {g[f"native_{n}"].tobytes(): g[f"load_img_{i}"] for i, n in enumerate(list(D.SIZES)[:8])}
    return lambda src, hw: by_src[src.tobytes()]


def _ds(tree, hyp, pool, **kw):
    from adrefine.data.dataset import YOLODataset
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the duplicate row and the corrupt pair
        return YOLODataset(**dict(dict(img_path=tree, imgsz=D.IMGSZ, cache=None, hyp=hyp, data={"names": D.NAMES},
                                       pool=pool, augment=True, pad=0.0), **kw))


@pytest.mark.parametrize("tag", list(P.DATASET))
def test_dataset_pass_vs_reference(tag, tmp_path):
    """Our YOLODataset with perspective 0.001 against the reference's own on the same tree: the buffer, the collated
    labels, and the images through the plan executor. "letterbox": mosaic 0.0, so LetterBox (pad only) is the
    canvas under the warp."""
    tiny, g = golden("dataset_tiny"), golden("dataset_persp_tiny")
    cfg = P.DATASET[tag]
    tree = str(D.write_tree(tmp_path / "tiny", D.fixture_images(tiny)))
    ds = _ds(tree, P.dataset_hyp(tag), D.HostPool(_lookup(tiny)), batch_size=cfg["batch_size"])
    assert int(g[f"{tag}_seed"]) == cfg["seed"]
    D.seed(cfg["seed"])
    samples = []
    for k, i in enumerate(cfg["order"]):
        ds.begin_batch(k // cfg["collate"])
        samples.append(ds[i])
    assert ds.buffer == g[f"{tag}_buffer"].tolist()
    canvas = (D.IMGSZ, D.IMGSZ) if tag == "letterbox" else (2 * D.IMGSZ, 2 * D.IMGSZ)
    for s in samples:
        p = s["img"]
        assert p.M is None and p.P is not None and p.mix is None and p.canvas == canvas and p.size == (64, 64)
    for b in range(len(samples) // cfg["collate"]):
        part = samples[b * cfg["collate"]:(b + 1) * cfg["collate"]]
        _labels_equal(part, g, f"{tag}_b{b}_")
        img = np.stack([P.execute_plan(s["img"]) for s in part])
        bad = np.argwhere(img != g[f"{tag}_b{b}_img"])
        assert len(bad) == 0, (tag, b, len(bad), bad[:5].tolist())


def test_inverse_agrees_with_warp_affine_on_an_affine_matrix():
    """warp_perspective_matrix of a 3x3 with last row (0, 0, 1) against the inverse warp_affine_tables uses
    (invertAffineTransform's form, restated here as augment.warp_affine_tables states it). The two are different
    expressions: cv::invert's closed form multiplies every cofactor by m22 = 1 and m12 * m21 = 0 terms (exact), so the
    2x2 part can agree to the last bit; the translation is -A11*b1 - A12*b2 of already rounded quotients in one and
    a cofactor difference times d in the other, which need not. What is found is recorded here:

      2x2 part (t0, t1, t3, t4): with m20 = m21 = 0, m22 = 1 the closed form's determinant and cofactors are the
                                 same operations on the same numbers (plus exact terms): equal to the last bit
                                 (asserted).
      translation (t2, t5):      with u = 2^-53, each form carries three roundings beyond the shared d, so the two
                                 differ by at most about 6u of |A11 b1| + |A12 b2| (asserted: <= 1e-15 of it).
                                 RECORDED on the six matrices below: 5 of the 12 entries are equal, 7 differ, by
                                 8.9e-16 to 3.6e-15 absolute (units in the last place of entries between 4 and
                                 64). They are not equal to the last bit.

    The third row comes out (0, 0, 1) exactly."""
    from adrefine.data.augment import warp_perspective_matrix
    rs = np.random.RandomState(0)
    worst = 0.0
    for k in range(6):
        M = P.gentle_matrix(rs, 128, 96, 64, 48, 0.0)
        assert M.dtype == np.float32 and M[2].tolist() == [0, 0, 1]
        t = warp_perspective_matrix(M)
        assert np.array_equal(t, P.invert3x3(M))  # the executor's own statement of the same closed form
        m = M[:2].astype(np.float64).reshape(6).copy()
        Dd = m[0] * m[4] - m[1] * m[3]
        Dd = 1.0 / Dd if Dd != 0 else 0.0
        A11, A22 = m[4] * Dd, m[0] * Dd
        m[0], m[4] = A11, A22
        m[1] *= -Dd
        m[3] *= -Dd
        b1 = -m[0] * m[2] - m[1] * m[5]
        b2 = -m[3] * m[2] - m[4] * m[5]
        print("affine inverse", k, "2x2 equal", [t[0] == m[0], t[1] == m[1], t[3] == m[3], t[4] == m[4]],
              "translation difference", t[2] - b1, t[5] - b2)
        assert t[6:].tolist() == [0, 0, 1]
        assert [t[0], t[1], t[3], t[4]] == [m[0], m[1], m[3], m[4]]
        for got, want, scale in ((t[2], b1, abs(m[0] * M[0, 2]) + abs(m[1] * M[1, 2])),
                                 (t[5], b2, abs(m[3] * M[0, 2]) + abs(m[4] * M[1, 2]))):
            worst = max(worst, abs(got - want) / scale)
    assert worst <= 1e-15, worst


def test_singular_matrix_gives_the_zero_matrix():
    """cv::invert's result for det == 0 is the zero matrix (every pixel then reads canvas (0, 0)); the exact matrix
    of the clamp cases inverts exactly. Finite float32 entries cannot overflow the double inverse (|det| >= 1e-135
    or 0), so a non-finite inverse needs a non-finite matrix: render refuses it (tests/test_gpu_perspective.py)."""
    from adrefine.data.augment import warp_perspective_matrix
    assert warp_perspective_matrix(np.ones((3, 3), np.float32)).tolist() == [0.0] * 9
    assert warp_perspective_matrix(P.STRONG).tolist() == [1, 0, 0, 0, 1, 0, -1 / 64, 2.0 ** -30, 0.5]
    bad = np.eye(3, dtype=np.float32)
    bad[2, 0] = np.nan
    assert not np.isfinite(warp_perspective_matrix(bad)).all()


def test_restatement_on_an_affine_matrix_is_close_to_warp_affine():
    """Not a parity statement (the two OpenCV functions round their coordinates differently): an anchor of the
    restatement outside itself. For a matrix with last row (0, 0, 1) both round the source coordinate to the nearest
    1/32 pixel (warpAffine from 1/1024 fixed point), so the coordinates differ by at most 1/32 + 2/1024 pixel; on a
    source that changes by at most 5 grey levels per pixel along x and not along y the bilinear values differ by less
    than 0.2, and the two roundings to uint8 add at most 1: the images differ by at most 1 grey level off the border
    taps (where one tap of 114 may enter: those pixels are left out)."""
    rs = np.random.RandomState(3)
    ramp = np.clip(np.rint(127.5 + 100 * np.sin(np.arange(128) * 0.05)), 0, 255)
    src = np.broadcast_to(ramp[None, :, None], (96, 128, 3)).astype(np.uint8)
    for _ in range(3):
        M = P.gentle_matrix(rs, 128, 96, 64, 48, 0.0)
        a = A.cv2_oracle.warpAffine(src, M[:2], dsize=(64, 48), borderValue=(114, 114, 114)).astype(np.int32)
        b = P.warpPerspective(src, M, dsize=(64, 48), borderValue=(114, 114, 114)).astype(np.int32)
        sx, sy, *_ = P.perspective_coords(M, (64, 48))
        inside = (sx >= 1) & (sx < 126) & (sy >= 1) & (sy < 94)
        assert inside.mean() > 0.5 and np.abs(a - b)[inside].max() <= 1


def test_strong_matrix_takes_every_clamp_path():
    *_, paths = P.perspective_coords(P.STRONG, (96, 40))
    assert paths["w0"].sum() >= 1 and paths["int"].sum() >= 1 and paths["short"].sum() >= 1
    assert paths["w0"][0, 32] and paths["int"][1:, 32].all()


def test_perspective_zero_leaves_the_chain_as_it_was():
    """perspective 0: the same draws (P[2, 0] / P[2, 1] are drawn either way), plans with M and without P, and the
    fixtures of the affine chain still come out."""
    for name in ("aug_default_256", "aug_rot_256"):
        g = golden(name)
        out = A.run_chain(name)
        assert all(q.P is None and q.M is not None for o in out for q in o["img"].layers())
        _labels_equal(out, g)
        for i, o in enumerate(out):
            assert np.array_equal(A.execute_plan(o["img"]), g["img"][i])
    out = P.run_chain(31, perspective=0.0)
    assert all(q.P is None and q.M is not None for o in out for q in o["img"].layers())


def _plans():
    from adrefine.data.augment import ImagePlan
    rs = np.random.RandomState(0)
    return [ImagePlan(rs.randint(0, 256, (24, 32, 3)).astype(np.uint8)) for _ in range(2)]


def test_stage_rules_treat_p_as_m():
    from adrefine.data.augment import LetterBox, Mosaic, RandomPerspective, _letterbox_geometry
    from adrefine.data.instance import Instances
    eye = np.eye(3, dtype=np.float32)
    a, b = _plans()
    a.P = b.P = eye
    a.mixup(b, 0.5)  # a MixUp layer may carry the warp, first or second
    assert a.layers() == (a, b) and a._layer_only() is False and b._layer_only()
    a, _ = _plans()
    a.P = eye
    with pytest.raises(NotImplementedError, match="letterbox"):  # a letterbox may not follow the warp
        LetterBox((64, 64))(image=a)
    with pytest.raises(ValueError, match="warp"):
        _letterbox_geometry(a)
    resized = _plans()[0].letterbox((16, 12), 8, 6, 8, 6)  # nor may a LetterBox resize precede it
    assert resized.resize is not None
    ins = Instances(np.zeros((0, 4), np.float32), None, None, bbox_format="xywh", normalized=True)
    random.seed(0)
    with pytest.raises(NotImplementedError, match="warp after a LetterBox that resizes"):
        RandomPerspective(perspective=0.001)({"img": resized, "instances": ins, "cls": np.zeros((0, 1), np.float32)})
    for first in ("P", "M"):  # no second warp on a warped plan
        a, _ = _plans()
        setattr(a, first, eye if first == "P" else eye[:2])
        ins = Instances(np.zeros((0, 4), np.float32), None, None, bbox_format="xywh", normalized=True)
        with pytest.raises(NotImplementedError, match="warp out of the supported chain order"):
            RandomPerspective(perspective=0.001)({"img": a, "instances": ins, "cls": np.zeros((0, 1), np.float32)})
    a, _ = _plans()
    a.P = eye

    class DS:
        buffer = [0]

        def get_image_and_label(self, i):
            return {"img": a, "resized_shape": (24, 32), "cls": np.zeros((0, 1), np.float32),
                    "instances": Instances(np.zeros((0, 4), np.float32), None, None, bbox_format="xywh",
                                           normalized=True)}

    with pytest.raises(NotImplementedError, match="untransformed"):  # a mosaic tile may not be warped
        Mosaic(DS(), imgsz=32, p=1.0)(DS().get_image_and_label(0))
