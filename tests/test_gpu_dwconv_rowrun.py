"""The row-run depthwise forward / data gradient (dw_run_kernel) and the one-launch backward (adr_dwconv_bwd_fused)
against the kernels they replace (ADR_DW_RUN=0, ADR_DW_FUSED=0): the output, dx, the weight gradient's partial rows
and the bias rows must be bitwise equal, on channel slices of wider tensors, with and without bias, writing and
accumulating dx. Each is also held to an fp64 torch restatement of the depthwise conv (nn.Conv2d(groups=C) in
ProgressiveFeatureFusion / EDFFN, block.py:2376-2710) at the tolerance of test_gpu_dwconv.py."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

N = 2
PADC = 16  # the tensors are [N][H][W][C + PADC]; the conv works on channels [8, 8 + C)
TOL = 1e-2  # bf16, as test_gpu_dwconv.py


def _wide(C, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(N, H, W, C + PADC, device="cuda", generator=g).to(torch.bfloat16)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() + 8 * t.element_size())


def _sl(t, C):
    return t[..., 8:8 + C]


def _switches(monkeypatch, on):
    monkeypatch.setenv("ADR_DW_RUN", "1" if on else "0")
    monkeypatch.setenv("ADR_DW_FUSED", "1" if on else "0")


def _forward(x, w, b, C, H, W, k):
    from adrefine import kernels as K
    from adrefine.native import lib
    y = _wide(C, H, W, 5)  # a fixed fill: the whole wide buffer is compared, the channels outside the slice too
    lib.adr_dwconv_fwd(K.BF16, _ptr(x), C + PADC, K.fptr(w), K.fptr(b), _ptr(y), C + PADC, N, H, W, C, k, K.stream())
    return y


def _backward(x, dy, w, C, H, W, k, bias, accumulate, reduce_dw=False):
    """dx (wide), the partial rows [N][k*k][C], the bias rows or None, dw or None — as DWConvFn.backward issues them:
    the one-launch entry where it is supported, else the data gradient and the weight gradient as two launches."""
    from adrefine import kernels as K
    from adrefine.native import lib
    cs = C + PADC
    dx = _wide(C, H, W, 6)
    wsb = lib.adr_dwconv_wgrad_workspace(N, H, W, C, k)
    ws = torch.zeros(wsb // 4, dtype=torch.float32, device="cuda")
    bpart = torch.zeros(N, 2, C, dtype=torch.float32, device="cuda") if bias else None
    dw = torch.zeros(C, k * k, dtype=torch.float32, device="cuda") if reduce_dw else None
    chunks = ctypes.c_int(0)
    fused = lib.adr_dwconv_bwd_fused_supported(K.BF16, H, W, C, k, cs, cs, cs)
    if fused:
        lib.adr_dwconv_bwd_fused(K.BF16, _ptr(x), cs, _ptr(dy), cs, K.fptr(w), _ptr(dx), cs, K.fptr(dw), N, H, W, C, k,
                                 accumulate, 0, K.fptr(ws), wsb, K.fptr(bpart), ctypes.byref(chunks), K.stream())
    else:
        lib.adr_dwconv_bwd(K.BF16, _ptr(x), cs, _ptr(dy), cs, K.fptr(w), _ptr(dx), cs, K.fptr(dw), N, H, W, C, k,
                           accumulate, 0, K.fptr(ws), wsb, K.stream())
        if bias:
            assert lib.adr_dwconv_wgrad_bias_fusable(K.BF16, H, W, C, k, cs, cs)
            lib.adr_dwconv_wgrad_partials_bias(K.BF16, _ptr(x), cs, _ptr(dy), cs, N, H, W, C, k, K.fptr(ws), wsb,
                                               K.fptr(bpart), ctypes.byref(chunks), K.stream())
        else:
            lib.adr_dwconv_wgrad_partials(K.BF16, _ptr(x), cs, _ptr(dy), cs, N, H, W, C, k, K.fptr(ws), wsb,
                                          ctypes.byref(chunks), K.stream())
    assert chunks.value == N
    return fused, dx, ws[:N * k * k * C].view(N, k * k, C), bpart, dw


def _reference(x, dy, w, b, C, k):
    """fp64 depthwise conv on the same bf16 operands: y without bias, dx, dw [C][k*k], db."""
    xr = _sl(x, C).permute(0, 3, 1, 2).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    br = b.double().requires_grad_(True)
    y = F.conv2d(xr, wr, br, 1, k // 2, groups=C)
    y.backward(_sl(dy, C).permute(0, 3, 1, 2).double())
    nhwc = lambda t: t.permute(0, 2, 3, 1)  # noqa: E731
    return nhwc(y.detach() - br.detach().view(1, C, 1, 1)), nhwc(xr.grad), wr.grad.view(C, k * k), br.grad


def _rel(a, r):
    return float((a.double() - r).norm() / r.norm())


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("H,W", [(20, 20), (13, 11), (8, 8), (40, 40)])
def test_rowrun_and_fused_bitwise_and_fp64(monkeypatch, H, W, k):
    """(40, 40) keeps dw_img_kernel and the two launches (its fp32 images do not fit the LDS plan) and must still
    match; the smaller maps must take the one-launch backward."""
    from adrefine import kernels as K
    from adrefine.native import lib
    for C in (8, 24, 40):
        torch.manual_seed(100 * k + C)
        x, dy = _wide(C, H, W, 1), _wide(C, H, W, 2)
        w = torch.randn(C, 1, k, k, device="cuda") * 0.2
        b = torch.randn(C, device="cuda") * 0.1
        y_ref, dx_ref, dw_ref, db_ref = _reference(x, dy, w, b, C, k)
        _switches(monkeypatch, True)
        assert lib.adr_dwconv_bwd_fused_supported(K.BF16, H, W, C, k, C + PADC, C + PADC, C + PADC) == (H < 40)
        for bias in (False, True):
            _switches(monkeypatch, False)
            y_old = _forward(x, w, b if bias else None, C, H, W, k)
            _switches(monkeypatch, True)
            y_new = _forward(x, w, b if bias else None, C, H, W, k)
            assert torch.equal(y_new, y_old), (C, bias)
            r = y_ref + b.double() if bias else y_ref
            assert _rel(_sl(y_new, C), r) < TOL, (C, bias, _rel(_sl(y_new, C), r))
            for accumulate in (0, 1):
                _switches(monkeypatch, False)
                f0, dx_old, rows_old, bp_old, _ = _backward(x, dy, w, C, H, W, k, bias, accumulate)
                assert not f0
                _switches(monkeypatch, True)
                f1, dx_new, rows_new, bp_new, _ = _backward(x, dy, w, C, H, W, k, bias, accumulate)
                assert bool(f1) == (H < 40)
                # the row-run data gradient on its own (the two-launch path with only ADR_DW_FUSED=0)
                monkeypatch.setenv("ADR_DW_FUSED", "0")
                f2, dx_run, rows_two, _, _ = _backward(x, dy, w, C, H, W, k, bias, accumulate)
                assert not f2
                tag = (C, bias, accumulate)
                assert torch.equal(dx_new, dx_old) and torch.equal(dx_run, dx_old), tag
                assert torch.equal(rows_new, rows_old) and torch.equal(rows_two, rows_old), tag
                if bias:
                    assert torch.equal(bp_new[:, 0], bp_old[:, 0]), tag
                    assert _rel(bp_new[:, 0].sum(0), db_ref) < TOL, tag
                r = dx_ref + _sl(_wide(C, H, W, 6), C).double() if accumulate else dx_ref
                assert _rel(_sl(dx_new, C), r) < TOL, (tag, _rel(_sl(dx_new, C), r))
                assert _rel(rows_new.sum(0).t(), dw_ref) < TOL, (tag, _rel(rows_new.sum(0).t(), dw_ref))


@pytest.mark.parametrize("H,W,C,k", [(20, 20, 24, 7), (13, 11, 40, 3)])
def test_fused_backward_reduces_dw(monkeypatch, H, W, C, k):
    """dw non-NULL: the one-launch entry reduces its partial rows as adr_dwconv_bwd does."""
    x, dy = _wide(C, H, W, 1), _wide(C, H, W, 2)
    w = torch.randn(C, 1, k, k, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 0.2
    _switches(monkeypatch, False)
    f0, dx_old, _, _, dw_old = _backward(x, dy, w, C, H, W, k, False, 0, reduce_dw=True)
    _switches(monkeypatch, True)
    f1, dx_new, _, _, dw_new = _backward(x, dy, w, C, H, W, k, False, 0, reduce_dw=True)
    assert f1 and not f0
    assert torch.equal(dx_new, dx_old) and torch.equal(dw_new, dw_old)
    assert float(dw_new.abs().max()) > 0


def test_dwconv_autograd_same_bits(monkeypatch):
    """DWConvFn through autograd (the immediate weight-gradient path): y, dx, dw, db with the new kernels are the bits
    of the old ones."""
    from adrefine import kernels as K
    out = []
    for on in (False, True):
        _switches(monkeypatch, on)
        torch.manual_seed(0)
        x = torch.randn(2, 24, 20, 20, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        w = (torch.randn(24, 1, 7, 7, device="cuda") * 0.2).requires_grad_(True)
        b = (torch.randn(24, device="cuda") * 0.1).requires_grad_(True)
        y = K.dwconv(x, w, b, 7)
        y.backward(torch.randn(y.shape, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last))
        out.append((y.detach(), x.grad, w.grad, b.grad))
    for a, r in zip(out[1], out[0]):
        assert torch.equal(a, r)
