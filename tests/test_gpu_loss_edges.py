"""GPU parity: adr_det_loss (through v8DetectionLoss + backward) against oracle.detection_loss, elementwise, on the
edge-case scenarios of tests/loss_util.py: the trained regime (SlideLoss mu far above its 0.2 floor), non-square
levels, images and whole batches without labels, B * nmax no multiple of 4, nmax > 64, anchors claimed by several
labels (identical duplicates included), degenerate boxes, nc = 8 / 16 / 96, exact ties in min / max / clamp and in the
top-10 cut, and the bf16 gradient rows. tests/test_loss_scenarios.py shows on the CPU that each scenario reaches its
branch and that the oracle's discrete decisions have a margin >= 1e-3, so the assignment is compared exactly."""
import functools
from types import SimpleNamespace

import pytest
import torch

import loss_util as LU
from conftest import golden
from gpu_util import assert_close

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _model(nc):
    head = SimpleNamespace(stride=torch.tensor([8.0, 16.0, 32.0]), nc=nc, reg_max=LU.RM)
    return SimpleNamespace(model=[head], args=None)


def _run(name, dtype):
    from adrefine.utils.loss import v8DetectionLoss
    feats, batch, nc, _ = LU.scenario(name)
    fd = [f.to("cuda", dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True) for f in feats]
    crit = v8DetectionLoss(_model(nc))
    loss, items = crit(fd, batch)
    loss.backward()
    return dict(loss=loss.detach().float().cpu(), items=items.float().cpu(), n_fg=float(crit.n_fg),
                grads=[f.grad.float().cpu() for f in fd], raw=[f.grad.clone() for f in fd])


@functools.lru_cache(maxsize=None)
def _result(name, tag):
    return _run(name, DTYPES[tag])


def _ref(name, tag):
    return LU.oracle(name, None if tag == "fp32" else torch.bfloat16)


def _check_assignment(name, got, ref):
    nc = LU.scenario(name)[2]
    assert got["n_fg"] == ref["n_fg"], (got["n_fg"], ref["n_fg"])
    assert torch.equal(LU.box_grad_rows(got["grads"], nc), ref["fg"])


@pytest.mark.parametrize("name", LU.NAMES)
def test_fp32_matches_oracle(name):
    got, ref = _result(name, "fp32"), _ref(name, "fp32")
    dl = abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    dg = max(float((a - b).abs().max() / (b.abs().max() + 1e-30)) for a, b in zip(got["grads"], ref["grads"]))
    print(f"[loss-edges] fp32 {name}: loss rel {dl:.3e}, grad max|d|/max|ref| {dg:.3e}, n_fg {got['n_fg']:.0f}")
    _check_assignment(name, got, ref)
    assert_close(got["loss"], ref["loss"], rtol=1e-5, atol=1e-5, what="loss")
    assert_close(got["items"], ref["items"], rtol=1e-5, atol=1e-6, what="items")
    for i, (a, b) in enumerate(zip(got["grads"], ref["grads"])):
        assert_close(a, b, rtol=1e-4, atol=1e-7, what=f"gfeat{i}")
    if name in LU.GOLDEN:  # the reference's own numbers for the same inputs
        g = golden(f"loss_edge_{name}")
        assert got["n_fg"] == int(g["n_fg"])
        assert_close(got["loss"], g["loss"], rtol=1e-5, atol=1e-5, what="loss vs fixture")
        assert_close(got["items"], g["items"], rtol=1e-5, atol=1e-6, what="items vs fixture")
        for i, a in enumerate(got["grads"]):
            assert_close(a, g[f"gfeat{i}"], rtol=1e-4, atol=1e-7, what=f"gfeat{i} vs fixture")


@pytest.mark.parametrize("name", LU.NAMES)
def test_bf16_matches_oracle(name):
    """bf16 head outputs: the kernel computes in fp32 from the rounded inputs, so the assignment is compared exactly
    against the oracle on those inputs; every gradient element lies within one bf16 ulp of the oracle's fp32 value
    (half an ulp of output rounding, half for an fp32 difference that crosses a rounding boundary); the loss within
    loss_util.BF16_LOSS_RTOL = 1.956e-6, four times the largest deviation measured over these scenarios (4.890e-7)."""
    got, ref = _result(name, "bf16"), _ref(name, "bf16")
    dl = abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    di = float(((got["items"] - ref["items"]).abs() / ref["items"].abs().clamp_min(1e-30)).max())
    worst = max(float(((a - b).abs() / (2.0 ** -7 * b.abs() + 1e-7)).max()) for a, b in zip(got["grads"], ref["grads"]))
    print(f"[loss-edges] bf16 {name}: loss rel {dl:.3e}, items rel {di:.3e}, grad worst err/bound {worst:.3f}")
    assert all(g.dtype == torch.bfloat16 for g in got["raw"])
    _check_assignment(name, got, ref)
    for i, (a, b) in enumerate(zip(got["grads"], ref["grads"])):
        bad = (a - b).abs() > 2.0 ** -7 * b.abs() + 1e-7
        assert not bool(bad.any()), (i, int(bad.sum()), worst)
    assert dl <= LU.BF16_LOSS_RTOL, dl


def test_no_labels_exact_zeros():
    for tag in DTYPES:
        got = _result("no_labels", tag)
        assert float(got["items"][0]) == 0.0 and float(got["items"][2]) == 0.0 and got["n_fg"] == 0.0
        assert float(got["items"][1]) > 0.0
        for g in got["grads"]:
            assert not bool(g[:, :4 * LU.RM].any())
            assert bool(g[:, 4 * LU.RM:].all())


@pytest.mark.parametrize("name", ["exact_ties", "overlap"])
def test_ties_serial_topk_bitwise(name, monkeypatch):
    """The serial heap-select (ADR_TAL_TOPK_SERIAL=1) and the default top-10 give the same bits where the cut is an
    exact tie at T > 0 (exact_ties) and where labels compete for anchors (overlap)."""
    base = _result(name, "fp32")
    monkeypatch.setenv("ADR_TAL_TOPK_SERIAL", "1")
    ser = _run(name, torch.float32)
    assert torch.equal(ser["loss"], base["loss"]) and torch.equal(ser["items"], base["items"])
    assert ser["n_fg"] == base["n_fg"] > 0
    for a, b in zip(ser["raw"], base["raw"]):
        assert torch.equal(a, b)
