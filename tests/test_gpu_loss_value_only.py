"""GPU: adr_det_loss's value-only mode (null gradient pointers) — the five outputs carry the bits of the call with
gradients, no gradient is stored, a mix of null and non-null gradient pointers is refused before any launch, and
v8DetectionLoss takes the mode under torch.no_grad() without allocating gradient maps."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

import loss_util as LU
from conftest import golden
from gpu_util import assert_close

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
CASES = ("loss_320_bs4", "loss_edge_exact_ties", "loss_edge_trained_nonsquare")
CANARY = 0x5A


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """(feats fp32 CPU NCHW, label batch, nc, (H, W)) of a fixture case — the inputs the fixture's numbers belong to."""
    if case == "loss_320_bs4":
        g = golden(case)
        gen = torch.Generator().manual_seed(int(g["feat0_seed"][0]))
        feats = [torch.randn(4, 144, 320 // s, 320 // s, generator=gen) for s in (8, 16, 32)]
        for f in feats:
            f[:, :64] *= 2.0
        return feats, {k: torch.from_numpy(g[k]) for k in ("batch_idx", "cls", "bboxes")}, 80, (320, 320)
    feats, batch, nc, hw = LU.scenario(case[len("loss_edge_"):])
    return feats, batch, nc, hw


def _dev(feats, dtype):
    return [f.to("cuda", dtype).contiguous(memory_format=torch.channels_last) for f in feats]


def _gt(batch, B, hw):
    from adrefine.utils.loss import preprocess_targets
    return preprocess_targets(batch["batch_idx"], batch["cls"], batch["bboxes"], B, hw).cuda().float().contiguous()


def _call(fd, gt, nc, grads, out=None, raw=False):
    """adr_det_loss on channels-last device maps `fd`; grads: three tensors or None each. Returns out (5,)."""
    from adrefine import kernels as K
    from adrefine.native import lib
    B = fd[0].shape[0]
    A = sum(f.shape[2] * f.shape[3] for f in fd)
    vs = [K.nhwc(f) for f in fd]
    wsb = lib.adr_det_loss_workspace(B, gt.shape[1], A)
    ws = torch.empty(wsb // 4 + 16, dtype=torch.float32, device="cuda")
    out = torch.empty(5, dtype=torch.float32, device="cuda") if out is None else out
    fn = lib.lib.adr_det_loss if raw else lib.adr_det_loss
    rc = fn(K.dcode(fd[0].dtype), *[ctypes.c_void_p(v[1]) for v in vs], *[v[2] for v in vs],
            fd[0].shape[2], fd[0].shape[3], fd[1].shape[2], fd[1].shape[3], fd[2].shape[2], fd[2].shape[3],
            8.0, 16.0, 32.0, B, nc, K.fptr(gt), gt.shape[1],
            *[None if g is None else ctypes.c_void_p(g.data_ptr()) for g in grads], float(B), 7.5, 0.5, 1.5,
            K.fptr(out), K.fptr(ws), wsb, K.stream())
    torch.cuda.synchronize()
    return rc if raw else out


def _bytes(t):
    """The bytes of an NHWC activation (a permuted view) as a flat uint8 view."""
    return t.permute(0, 2, 3, 1).reshape(-1).view(torch.uint8)


def _grad_bufs(fd):
    from adrefine import kernels as K
    return [K.empty_act(f.shape[0], f.shape[1], f.shape[2], f.shape[3], f.dtype, f.device) for f in fd]


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("case", CASES)
def test_value_only_bits_equal_with_gradient(case, tag):
    feats, batch, nc, hw = _inputs(case)
    fd = _dev(feats, DTYPES[tag])
    gt = _gt(batch, fd[0].shape[0], hw)
    with_grad = _call(fd, gt, nc, _grad_bufs(fd))
    value = _call(fd, gt, nc, [None] * 3)
    assert float(with_grad[4]) > 0 and bool(torch.isfinite(value).all())
    assert torch.equal(value, with_grad), (value.tolist(), with_grad.tolist())


@pytest.mark.parametrize("case", CASES)
def test_value_only_matches_fixture(case):
    """The reference's numbers for the same inputs, at the tolerances tests/test_gpu_loss.py and
    tests/test_gpu_loss_edges.py apply to them (loss rtol 1e-5 atol 1e-5, items rtol 1e-5 atol 1e-6)."""
    from adrefine.utils.loss import v8DetectionLoss
    feats, batch, nc, _ = _inputs(case)
    g = golden(case)
    head = SimpleNamespace(stride=torch.tensor([8.0, 16.0, 32.0]), nc=nc, reg_max=LU.RM)
    crit = v8DetectionLoss(SimpleNamespace(model=[head], args=None))
    fd = [f.requires_grad_(True) for f in _dev(feats, torch.float32)]
    with torch.no_grad():
        loss, items = crit(fd, batch)
    assert not loss.requires_grad and loss.grad_fn is None
    assert_close(loss, g["loss"], rtol=1e-5, atol=1e-5, what="loss")
    assert_close(items, g["items"], rtol=1e-5, atol=1e-6, what="items")
    if "n_fg" in g.files:
        assert float(crit.n_fg) == int(g["n_fg"])


@pytest.mark.parametrize("tag", list(DTYPES))
def test_empty_targets(tag):
    """nmax = 0 (the memset branch) and an all-padding gt at B = 2, 64 x 96, nc = 8: value-only == with-gradient, box
    and dfl exactly zero, and the two spellings of 'no labels' agree."""
    nc = 8
    feats = LU._randn_feats(2, nc, 64, 96, seed=3)
    fd = _dev(feats, DTYPES[tag])
    outs = []
    for gt in (torch.zeros(2, 0, 5, device="cuda"), torch.zeros(2, 8, 5, device="cuda")):
        with_grad = _call(fd, gt, nc, _grad_bufs(fd))
        value = _call(fd, gt, nc, [None] * 3)
        assert torch.equal(value, with_grad)
        assert float(value[0]) == 0.0 and float(value[2]) == 0.0 and float(value[4]) == 0.0
        assert float(value[1]) > 0.0
        outs.append(value)
    assert torch.equal(outs[0], outs[1])


def test_no_grad_criterion_stores_no_gradient_and_allocates_no_map():
    """v8DetectionLoss under torch.no_grad(). The check that carries the weight is the memory bound: the call's peak
    growth stays below one (P3) gradient map, where the training call allocates three — so no map was allocated,
    and the library got null gradient pointers (a store through them would fault, not land somewhere). The canaries
    are buffers of the freed gradient maps' sizes, which the caching allocator usually (not always: the count is
    printed, not asserted) places on the very blocks the maps had; they must stay untouched."""
    from adrefine.utils.loss import v8DetectionLoss
    feats, batch, nc, _ = _inputs("loss_320_bs4")
    head = SimpleNamespace(stride=torch.tensor([8.0, 16.0, 32.0]), nc=nc, reg_max=LU.RM)
    crit = v8DetectionLoss(SimpleNamespace(model=[head], args=None))
    fd = [f.requires_grad_(True) for f in _dev(feats, torch.float32)]
    loss, items_grad = crit(fd, batch)  # the training call: its maps live in ctx until the graph is dropped
    maps = [(g.data_ptr(), g.numel() * g.element_size()) for g in loss.grad_fn.grads]
    nbytes = sum(n for _, n in maps)
    one_map = fd[0].numel() * fd[0].element_size()
    items_grad = items_grad.clone()
    del loss
    torch.cuda.synchronize()
    canaries = [torch.full((n,), CANARY, dtype=torch.uint8, device="cuda") for _, n in maps]  # same sizes: same blocks
    covered = sum(c.data_ptr() == p for c, (p, _) in zip(canaries, maps))
    print(f"[value-only] canaries lie on {covered} of the 3 former gradient maps")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        total, items = crit(fd, batch)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"[value-only] peak growth {peak} B, one gradient map {one_map} B, three maps {nbytes} B")
    assert peak < one_map, (peak, one_map)
    assert all(bool((c == CANARY).all()) for c in canaries)
    assert torch.equal(items, items_grad) and total.grad_fn is None
    assert all(f.grad is None for f in fd)


def test_mixed_null_gradient_pointers_are_refused():
    """One or two null gradient pointers: an error code, adr_last_error set, nothing launched (out and the gradient
    buffers that were passed keep their canary bytes)."""
    from adrefine.native import lib
    nc = 8
    fd = _dev(LU._randn_feats(2, nc, 64, 96, seed=3), torch.float32)
    gt = torch.zeros(2, 8, 5, device="cuda")
    for mask in ((1, 0, 0), (0, 1, 1), (1, 1, 0), (0, 0, 1)):
        bufs = _grad_bufs(fd)
        for b in bufs:
            _bytes(b).fill_(CANARY)
        out = torch.full((5,), 123.0, device="cuda")
        rc = _call(fd, gt, nc, [b if m else None for b, m in zip(bufs, mask)], out=out, raw=True)
        assert rc != 0
        assert b"gradient pointers" in lib.lib.adr_last_error()
        assert bool((out == 123.0).all())
        assert all(bool((_bytes(b) == CANARY).all()) for b in bufs)
