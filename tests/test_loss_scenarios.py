"""CPU side of the detection-loss edge-case suite (tests/loss_util.py): every scenario reaches the branch it is
there for (shown from the oracle alone), the oracle's discrete decisions are far enough from flipping that kernel
and oracle cannot disagree through a last-bit difference, and the host-side preprocess_targets equals the oracle's
bit for bit, non-square sizes included."""
import pytest
import torch

import adr_oracle as O
import loss_util as LU

MARGIN = 1e-3  # s^0.5 * u^6 in fp32 differs between implementations at the 1e-5 level: two orders of magnitude


@pytest.fixture(autouse=True)
def _threads(cpu_threads):
    yield


def test_shapes_meet_the_topk_contract():
    for name in LU.NAMES:
        feats, batch, nc, (H, W) = LU.scenario(name)
        B = feats[0].shape[0]
        A = sum(f.shape[2] * f.shape[3] for f in feats)
        assert A >= 640 and B in (2, 3), (name, A, B)
        assert [tuple(f.shape) for f in feats] == [(B, 64 + nc, H // s, W // s) for s in LU.STRIDES], name
        if (H, W) != (256, 256):  # A = 1344 = 32 * 42 at 256^2: no batch size avoids the multiple there
            assert (B * A) % 32 != 0, (name, B * A)
    assert {LU.scenario(n)[3] for n in LU.NAMES} == {(192, 192), (160, 256), (256, 256)}
    assert LU.trace("many_labels")["nmax"] > 64
    t = LU.trace("empty_image")
    assert t["B"] * t["nmax"] == 21 and not t["mask_gt"][1].any() and t["mask_gt"][0].all()
    assert LU.trace("no_labels")["nmax"] == 0 and LU.trace("no_labels")["n_fg"] == 0


def test_scenarios_are_deterministic():
    for name in ("trained_nonsquare", "many_labels", "exact_ties"):
        a = LU.scenario(name)
        LU.scenario.cache_clear()
        b = LU.scenario(name)
        assert all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
        assert all(torch.equal(a[1][k], b[1][k]) for k in a[1])


@pytest.mark.parametrize("name", [n for n in LU.NAMES if n != "no_labels"])
def test_has_positives(name):
    assert LU.trace(name)["n_fg"] > 0


@pytest.mark.parametrize("name", ["trained", "trained_nonsquare"])
def test_trained_regime(name):
    t = LU.trace(name)
    mu = t["mu"]
    assert float(t["ciou_fg"].mean()) >= 0.5, mu
    ts = t["t_scores"][t["t_scores"] > 0]
    n = (int((ts <= mu - 0.1).sum()), int(((ts > mu - 0.1) & (ts < mu)).sum()), int((ts >= mu).sum()))
    assert min(n) >= 10, (mu, n)


def test_many_labels_dfl_clamp():
    feats, batch, nc, (H, W) = LU.scenario("many_labels")
    t = LU.trace("many_labels")
    assert float((batch["bboxes"][:, 2] * W).max()) > 15 * 8
    frac = float((t["tltrb_fg"] > LU.RM - 1 - 0.01).float().mean())
    assert frac >= 0.05, frac
    assert sorted(torch.bincount(batch["batch_idx"].long(), minlength=3).tolist()) == [0, 2, 70]


def test_overlap_multi_claims():
    t = LU.trace("overlap")
    cl = LU.claimants("overlap")
    multi = cl.sum(1) > 1
    assert int(multi.sum()) >= 20, int(multi.sum())
    # the duplicate pair: image 1, labels 0 and 1 (same box, different classes)
    assert torch.equal(t["gt"][1, 0, 1:], t["gt"][1, 1, 1:]) and t["gt"][1, 0, 0] != t["gt"][1, 1, 0]
    both = multi[1] & cl[1, 0] & cl[1, 1] & t["fg"][1] & (t["tgi"][1] == 0)
    assert int(both.sum()) >= 1  # claimed by both duplicates, equal overlaps, resolved to the first


def test_degenerate_rows():
    feats, batch, nc, (H, W) = LU.scenario("degenerate")
    t = LU.trace("degenerate")
    gt = t["gt"]
    area = (gt[..., 3] - gt[..., 1]) * (gt[..., 4] - gt[..., 2])
    zero = (area == 0) & t["mask_gt"][..., 0]
    assert int(zero.sum()) == 2  # zero width, zero height
    tiny = (area > 0) & (area <= 4.0001)
    assert int(tiny.sum()) == 1
    for b, j in (zero | tiny).nonzero().tolist():
        assert t["mask_gt"][b, j, 0] and not t["in_gts"][b, j].any()
        assert not (t["fg"][b] & (t["tgi"][b] == j) & LU.claimants("degenerate")[b, j]).any()
    assert bool((gt[..., 3] > W).any() and (gt[..., 4] > H).any())  # past the right and bottom edge
    assert bool(((gt[..., 1] == 0) & (gt[..., 2] == 0) & (gt[..., 3] == W) & (gt[..., 4] == H)).any())


def test_exact_ties_reached():
    t = LU.trace("exact_ties")
    edge_ties = int((t["pbox_fg"] == t["tbox_fg"]).sum())
    assert edge_ties >= 50, edge_ties
    assert int(((t["pbox_fg"] == t["tbox_fg"]).sum(1) == 4).sum()) >= 1  # a positive whose box is its target exactly
    cut_ties = [a for a, b in LU.topk_rows("exact_ties") if a == b and a > 0]
    assert len(cut_ties) >= 1
    for dt in (torch.bfloat16,):  # every number is representable in bf16 as well
        assert all(torch.equal(f, g) for f, g in zip(LU.scenario("exact_ties")[0], LU.inputs("exact_ties", dt)[0]))


@pytest.mark.parametrize("dtype", [None, torch.bfloat16], ids=["fp32", "bf16in"])
@pytest.mark.parametrize("name", LU.NAMES)
def test_margins(name, dtype):
    """Also on the bf16-rounded inputs: the bf16 kernel assigns in fp32 from those, and is compared exactly too."""
    topk_gap, argmax_gap = LU.margins(name, dtype)
    assert topk_gap >= MARGIN and argmax_gap >= MARGIN, (topk_gap, argmax_gap)


@pytest.mark.parametrize("name", LU.NAMES)
def test_box_gradient_rows_are_the_positives(name):
    """What the GPU tests lean on to pin the assignment itself: in the oracle, the anchors with a non-zero box-channel
    gradient are exactly fg (no positive has weight 0 in any scenario), on fp32 and on bf16-rounded inputs."""
    for dt in (None, torch.bfloat16):
        o = LU.oracle(name, dt)
        assert torch.equal(LU.box_grad_rows(o["grads"], LU.scenario(name)[2]), o["fg"])
        assert int(o["fg"].sum()) == o["n_fg"]


@pytest.mark.parametrize("name", LU.NAMES)
def test_preprocess_targets_parity(name):
    from adrefine.utils.loss import preprocess_targets
    feats, batch, nc, (H, W) = LU.scenario(name)
    B = feats[0].shape[0]
    ref = O.preprocess_targets(batch["batch_idx"], batch["cls"], batch["bboxes"], B, torch.tensor([float(H), float(W)]))
    got = preprocess_targets(batch["batch_idx"], batch["cls"], batch["bboxes"], B, (float(H), float(W)))
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert torch.equal(got, ref)
