"""The float64 references of tests/pool_ref.py against something outside themselves (CPU): hand-written double
loops for the adaptive-pool windows and the bilinear taps, the max-pool tie rule on a plateau and a checkerboard, the
axis-mean layouts and the gate by index, MLCA's batch-axis pooling against an explicit mean over image rows. They
are what the HIP pooling kernels are held to, so they are themselves pinned to 1e-12 here. Plus the host-side size
guards, which need no device: every entry point refuses an empty map before it launches anything."""
import ctypes
import math

import pytest
import torch

import pool_ref as R

TOL = 1e-12


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def close(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


SIZES = [(7, 3), (3, 7), (5, 4), (1, 4)]


def window(o, n_in, n_out):
    return (o * n_in) // n_out, -((-(o + 1) * n_in) // n_out)


@pytest.mark.parametrize("hi,ho", SIZES)
@pytest.mark.parametrize("wi,wo", SIZES)
def test_adapool_windows(hi, ho, wi, wo):
    x = randn(2, 3, hi, wi, seed=1)
    want = torch.empty(2, 3, ho, wo, dtype=torch.float64)
    for i in range(ho):
        h0, h1 = window(i, hi, ho)
        for j in range(wo):
            w0, w1 = window(j, wi, wo)
            want[:, :, i, j] = x[:, :, h0:h1, w0:w1].sum((2, 3)) / ((h1 - h0) * (w1 - w0))
    close(R.ref_adapool(x, ho, wo), want)


def taps(o, n_in, n_out):
    src = max((o + 0.5) * n_in / n_out - 0.5, 0.0)
    i0 = min(int(math.floor(src)), n_in - 1)
    i1 = min(i0 + 1, n_in - 1)
    return i0, i1, src - i0


@pytest.mark.parametrize("hi,ho", SIZES)
@pytest.mark.parametrize("wi,wo", SIZES)
def test_bilinear_taps(hi, ho, wi, wo):
    x = randn(2, 3, hi, wi, seed=2)
    want = torch.empty(2, 3, ho, wo, dtype=torch.float64)
    for i in range(ho):
        h0, h1, lh = taps(i, hi, ho)
        for j in range(wo):
            w0, w1, lw = taps(j, wi, wo)
            want[:, :, i, j] = (1 - lh) * ((1 - lw) * x[:, :, h0, w0] + lw * x[:, :, h0, w1]) \
                + lh * ((1 - lw) * x[:, :, h1, w0] + lw * x[:, :, h1, w1])
    close(R.ref_bilinear(x, ho, wo), want)


def test_nearest_is_repeat():
    x = randn(2, 3, 3, 5, seed=3)
    for s in (1, 2, 3):
        close(R.ref_nearest(x, s), x.repeat_interleave(s, 2).repeat_interleave(s, 3))


def first_max_grad(x, k, up):
    """dx of the k x k stride-1 max pool by the rule itself: every window's gradient goes to its first maximum in
    row-major order over the in-range taps."""
    N, C, H, W = x.shape
    p = k // 2
    dx = torch.zeros_like(x)
    for n in range(N):
        for c in range(C):
            for h in range(H):
                for w in range(W):
                    best, at = None, None
                    for ih in range(max(0, h - p), min(H, h + p + 1)):
                        for iw in range(max(0, w - p), min(W, w + p + 1)):
                            v = float(x[n, c, ih, iw])
                            if best is None or v > best:
                                best, at = v, (ih, iw)
                    dx[n, c, at[0], at[1]] += up[n, c, h, w]
    return dx


@pytest.mark.parametrize("pattern", ["plateau", "checkerboard", "minus_inf"])
def test_maxpool_tie_rule(pattern):
    H, W, k = 5, 6, 3
    if pattern == "plateau":
        x = torch.full((1, 1, H, W), 2.0, dtype=torch.float64)
    elif pattern == "checkerboard":
        ij = torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)
        x = (ij % 2).double().view(1, 1, H, W) * 3 - 1
    else:  # nothing but -inf around one finite value: the first in-range tap takes an all -inf window's gradient
        x = torch.full((1, 1, H, W), -math.inf, dtype=torch.float64)
        x[0, 0, 2, 3] = 1.0
    up = randn(1, 1, H, W, seed=4)
    (out,), (dx,) = R.run(lambda t: R.ref_maxpool(t, k), [x], [up])
    close(dx, first_max_grad(x, k, up))
    if pattern == "plateau":  # window (h, w) starts at (max(0, h-1), max(0, w-1)): only rows / columns < H-1, W-1 get any
        assert float(dx[0, 0, H - 1].abs().max()) == 0 and float(dx[0, 0, :, W - 1].abs().max()) == 0
        assert torch.equal(out, x)


def test_axis_mean_layouts():
    N, C, H, W = 2, 3, 4, 4
    x = randn(N, C, H, W, seed=5)
    ela, (eh, ew), coord = R.ref_axis_mean(x, "ela"), R.ref_axis_mean(x, "ela2"), R.ref_axis_mean(x, "coord")
    assert ela.shape == (2 * N, C, H, 1) and eh.shape == (N, C, H, 1) and coord.shape == (N, C, H + W, 1)
    for n in range(N):
        for h in range(H):
            want = x[n, :, h, :].sum(1) / W
            for got in (ela[n, :, h, 0], eh[n, :, h, 0], coord[n, :, h, 0]):
                close(got, want)
        for w in range(W):
            want = x[n, :, :, w].sum(1) / H
            for got in (ela[N + n, :, w, 0], ew[n, :, w, 0], coord[n, :, H + w, 0]):
                close(got, want)
    y = randn(N, C, 3, 5, seed=6)
    rh, rw = R.ref_axis_mean(y, "ela2")
    assert rh.shape == (N, C, 3, 1) and rw.shape == (N, C, 5, 1)
    close(R.ref_axis_mean(y, "coord")[:, :, 3:, 0], y.sum(2) / 3)


@pytest.mark.parametrize("layout,H,W", [("ela", 4, 4), ("ela2", 3, 5), ("coord", 3, 5)])
@pytest.mark.parametrize("with_x", [True, False])
def test_gate_by_index(layout, H, W, with_x):
    N, C = 2, 3
    x = randn(N, C, H, W, seed=7) if with_x else None
    if layout == "ela":
        ah = aw = randn(2 * N, C, H, 1, seed=8)
    elif layout == "ela2":
        ah, aw = randn(N, C, H, 1, seed=8), randn(N, C, W, 1, seed=9)
    else:
        ah, aw = randn(N, C, H + W, 1, seed=8), randn(N, C, H + W, 1, seed=9)
    got = R.ref_gate(x, ah, aw, layout, N, H, W)
    for n in range(N):
        for h in range(H):
            for w in range(W):
                a = ah[n, :, h, 0]
                b = aw[N + n, :, w, 0] if layout == "ela" else aw[n, :, w if layout == "ela2" else H + w, 0]
                close(got[n, :, h, w], a * b * (x[n, :, h, w] if with_x else 1.0))
    if layout == "coord":  # the rows the gate does not read get a zero gradient
        up = randn(N, C, H, W, seed=10)
        _, (_, dah, daw) = R.run(lambda t, a, b: R.ref_gate(t, a, b, layout, N, H, W), [x, ah, aw], [up])
        assert float(dah[:, :, H:].abs().max()) == 0 and float(daw[:, :, :H].abs().max()) == 0
        assert float(dah[:, :, :H].abs().min()) > 0 and float(daw[:, :, H:].abs().min()) > 0


@pytest.mark.parametrize("B", [1, 2, 5, 7])
def test_mlca_batch_rows(B):
    """The global branch is pooled over the batch axis: bin row i of every image averages sigmoid(conv(g)) over the
    images rows(i) = [floor(i B / 5), ceil((i + 1) B / 5)). Rebuilt here from the reference's own pieces."""
    C, H, W, k, lw = 6, 7, 5, 3, 0.5
    y, wl, wg = randn(B, C, H, W, seed=11), randn(k, seed=12), randn(k, seed=13)
    local = R.ref_adapool(y, 5, 5)  # (B, C, 5, 5)
    seq = local.flatten(2).transpose(1, 2).reshape(B, 1, -1)  # (pos, chan) interleaved
    conv = lambda s, w_: torch.nn.functional.conv1d(s, w_.view(1, 1, k), padding=(k - 1) // 2)
    att_l = conv(seq, wl).reshape(B, 25, C).transpose(1, 2).reshape(B, C, 5, 5).sigmoid()
    sig_g = conv(local.mean((2, 3)).unsqueeze(1), wg).squeeze(1).sigmoid()  # (B, C)
    att = torch.empty(B, C, 5, 5, dtype=torch.float64)
    for i in range(5):
        r0, r1 = R.batch_rows(i, B)
        assert (r0, r1) == (math.floor(i * B / 5), math.ceil((i + 1) * B / 5)) and r1 > r0
        g = sig_g[r0:r1].mean(0)  # the same for every image of the batch
        att[:, :, i, :] = (1 - lw) * g.view(1, C, 1) + lw * att_l[:, :, i, :]
    want = y * R.ref_adapool(att, H, W)
    close(R.ref_mlca(y, None, wl, wg, lw), want)
    res = randn(B, C, H, W, seed=14)
    close(R.ref_mlca(y, res, wl, wg, lw), res + want)


def test_mlca_couples_the_batch():
    y, wl, wg = randn(2, 6, 7, 5, seed=15), randn(3, seed=16), randn(3, seed=17)
    y2 = y.clone()
    y2[1] += 1.0
    a, b = R.ref_mlca(y, None, wl, wg), R.ref_mlca(y2, None, wl, wg)
    assert float((a[0] - b[0]).abs().max()) > 1e-6


def test_bf16_restatements_round_only():
    """With bf16_round the identity the restatements are the references; with it they move by bf16 precision."""
    x, up = randn(2, 8, 7, 5, seed=20), randn(2, 8, 7, 5, seed=21)
    up3 = randn(2, 8, 3, 2, seed=22)
    wl, wg = randn(3, seed=23), randn(3, seed=24)
    cases = [
        (lambda: R.bf16_maxpool(x, 5, up), lambda t: R.ref_maxpool(t, 5), [x], [up]),
        (lambda: R.bf16_adapool(x, 3, 2, up3), lambda t: R.ref_adapool(t, 3, 2), [x], [up3]),
        (lambda: R.bf16_bilinear(up3, 7, 5, up), lambda t: R.ref_bilinear(t, 7, 5), [up3], [up]),
        (lambda: R.bf16_nearest(up3, 2, randn(2, 8, 6, 4, seed=25)), lambda t: R.ref_nearest(t, 2), [up3],
         [randn(2, 8, 6, 4, seed=25)]),
        (lambda: R.bf16_axis_mean(x, "coord", [randn(2, 8, 12, 1, seed=26)]), lambda t: R.ref_axis_mean(t, "coord"), [x],
         [randn(2, 8, 12, 1, seed=26)]),
        (lambda: R.bf16_gate(x, randn(2, 8, 7, 1, seed=27), randn(2, 8, 5, 1, seed=28), "ela2", 2, 7, 5, up),
         lambda t, a, b: R.ref_gate(t, a, b, "ela2", 2, 7, 5),
         [x, randn(2, 8, 7, 1, seed=27), randn(2, 8, 5, 1, seed=28)], [up]),
    ]
    for rest, fn, inputs, ups in cases:
        outs, grads = R.run(fn, inputs, ups)
        rounded = rest()
        saved, R.bf16_round = R.bf16_round, lambda t: t
        try:
            exact = rest()
        finally:
            R.bf16_round = saved
        for a, b in zip(exact[0] + exact[1], outs + grads):
            close(a, b)
        for a, b in zip(rounded[0] + rounded[1], outs + grads):
            assert float((a - b).abs().max()) <= 2.0 ** -8 * float(b.abs().max())
        assert any(float((a - b).abs().max()) > 0 for a, b in zip(rounded[0] + rounded[1], outs + grads))
    (o,), (dy, dres), (dwl, dwg) = R.bf16_mlca(x, up, wl, wg, 0.5, up)
    (ro,), (rdy, rdres, rdwl, rdwg) = R.run(lambda a, r, p, q: R.ref_mlca(a, r, p, q, 0.5), [x, up, wl, wg], [up])
    assert torch.equal(dres, rdres) and torch.equal(dres, up) and torch.equal(dwl, rdwl) and torch.equal(dwg, rdwg)
    assert 0 < float((o - ro).abs().max()) <= 2.0 ** -8 * float(ro.abs().max())
    assert 0 < float((dy - rdy).abs().max()) <= 2.0 ** -8 * float(rdy.abs().max())


def test_bf16_accumulated():
    a, b = randn(64, seed=30), randn(64, seed=31)
    got = R.bf16_accumulated([a, b])
    assert torch.equal(got, R.bf16_round(R.bf16_round(a) + b))
    assert torch.equal(got, R.bf16_round(got))
    assert float((got - (a + b)).abs().max()) <= 2 * 2.0 ** -8 * float((a + b).abs().max() + a.abs().max())
    assert torch.equal(R.bf16_accumulated([a]), R.bf16_round(a))


# ---- host-side guards (no device: each call returns before it would launch) -------------------------------------


def test_cross_scale_tssa_refuses_a_map_below_its_scale():
    """A 3x3 map (a 96x96 image at stride 32) with scale 4 asks for a 0x0 pool and a bilinear resize from it: the
    reference's F.interpolate raises there, and so must the module, before any kernel."""
    from adrefine.nn.modules.block import CrossScaleAttentionTSSA
    m = CrossScaleAttentionTSSA(16, num_heads=2)
    for H, W in ((3, 3), (8, 3), (1, 8)):
        with pytest.raises(RuntimeError, match=rf"{H}x{W} map is smaller than scale"):
            m(torch.zeros(1, 16, H, W))


def _dims(**kw):
    d = dict(N=2, H=3, W=4, C=8, OH=5, OW=6)
    d.update(kw)
    return d


@pytest.mark.parametrize("zero", ["N", "H", "W", "C", "OH", "OW"])
def test_entry_points_refuse_empty_maps(zero):
    """Null pointers throughout: a call that reached a launch would fault, a refused one only returns the error."""
    from adrefine import kernels as K
    from adrefine.native import lib
    d = _dims(**{zero: 0})
    N, H, W, C, OH, OW = (d[k] for k in ("N", "H", "W", "C", "OH", "OW"))
    nul, f32 = ctypes.c_void_p(None), K.F32
    resize = [
        lambda: lib.adr_adapool(f32, nul, C, N, H, W, C, nul, C, OH, OW, None),
        lambda: lib.adr_adapool_bwd(f32, nul, C, N, H, W, C, nul, C, OH, OW, 0, None),
        lambda: lib.adr_bilinear(f32, nul, C, N, H, W, C, nul, C, OH, OW, None),
        lambda: lib.adr_bilinear_bwd(f32, nul, C, N, H, W, C, nul, C, OH, OW, 0, None),
    ]
    maps = [
        lambda: lib.adr_axis_mean(f32, nul, C, N, H, W, C, nul, H * C, nul, W * C, None),
        lambda: lib.adr_axis_mean_bwd(f32, nul, H * C, nul, W * C, nul, C, N, H, W, C, 0, None),
        lambda: lib.adr_gate(f32, nul, C, nul, H * C, nul, W * C, nul, C, N, H, W, C, None),
        lambda: lib.adr_gate_bwd(f32, nul, C, nul, H * C, nul, W * C, nul, C, nul, C, nul, H * C, nul, W * C, N, H, W, C,
                                 0, 0, None),
        lambda: lib.adr_mlca_fwd(f32, nul, C, nul, C, nul, C, N, H, W, C, nul, nul, 3, 0.5, nul, nul, nul, nul, None),
        lambda: lib.adr_mlca_bwd(f32, nul, C, nul, C, nul, C, N, H, W, C, nul, nul, 3, 0.5, nul, nul, nul, nul, nul, nul,
                                 nul, 1 << 30, None),
    ]
    for call in resize + ([] if zero in ("OH", "OW") else maps):
        with pytest.raises(RuntimeError, match="empty map"):
            call()
