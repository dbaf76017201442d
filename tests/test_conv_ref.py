"""Pins tests/conv_ref.py (the float64 reference of tests/test_gpu_conv_exact.py) against independent restatements
of the same gradients. CPU only."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("H,W", [(9, 7), (10, 8), (9, 8), (10, 7)])
@pytest.mark.parametrize("k,pad", [(3, 1), (1, 0), (5, 2)])
def test_dgrad_is_conv_transpose_with_output_padding(H, W, k, pad):
    """dx = conv_transpose2d(dy, w, stride 2, pad, output_padding), where output_padding restores the input rows /
    columns the strided forward never reached from its last window: (H + 2 pad - k) mod 2."""
    x, w = _rand((2, 3, H, W), 1), _rand((4, 3, k, k), 2)
    dy = _rand(tuple(R.forward(x, w, None, 2, pad).shape), 3)
    dx, _ = R.grads(x, w, dy, 2, pad)
    op = ((H + 2 * pad - k) % 2, (W + 2 * pad - k) % 2)
    want = F.conv_transpose2d(dy, w, None, 2, pad, output_padding=op)
    assert want.shape == dx.shape
    torch.testing.assert_close(dx, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", [(2, 3, 5, 6, 4, 3, 3, 1, (1, 1)), (2, 2, 7, 5, 3, 3, 1, 2, (1, 0))])
def test_wgrad_is_unfold_einsum(shape):
    """dw[k, c, r, s] = sum over (n, output pixel) of dy[n, k, p] * x[n, c, window p at (r, s)]."""
    N, C, H, W, K, Rr, S, st, pad = shape
    x, w = _rand((N, C, H, W), 4), _rand((K, C, Rr, S), 5)
    y = R.forward(x, w, None, st, pad)
    dy = _rand(tuple(y.shape), 6)
    _, dw = R.grads(x, w, dy, st, pad)
    cols = F.unfold(x, (Rr, S), padding=pad, stride=st)  # (N, C*R*S, P)
    want = torch.einsum("nkp,nqp->kq", dy.reshape(N, K, -1), cols).reshape(K, C, Rr, S)
    torch.testing.assert_close(dw, want, rtol=1e-12, atol=1e-12)
    # and the forward is the same unfold contracted with the weights
    yw = torch.einsum("kq,nqp->nkp", w.reshape(K, -1), cols).reshape(y.shape)
    torch.testing.assert_close(y, yw, rtol=1e-12, atol=1e-12)


def test_integer_inputs_give_integer_outputs():
    x = R.randint((2, 8, 9, 7), -3, 3, 10)
    w = R.randint((24, 8, 3, 3), -3, 3, 11)
    b = R.randint((24,), -3, 3, 12)
    y = R.forward(x, w, b, 2, 1)
    dy = R.randint(tuple(y.shape), -3, 3, 13)
    dx, dw = R.grads(x, w, dy, 2, 1)
    R.assert_integer(x, w, dy, y, dx, dw, R.bias_grad(dy), *R.channel_stats(y))
    sy, sdx, sdw = R.abs_maps(x, w, dy, 2, 1, b)
    R.assert_exact_ok(sy, sdx, sdw)
    assert bool((y.abs() <= sy).all() and (dx.abs() <= sdx).all() and (dw.abs() <= sdw).all())
    # position dependent, about a quarter zeros, the whole range used
    assert 0.15 < float((R.randint((4096,), -3, 3, 14) == 0).float().mean()) < 0.5
    assert set(R.randint((4096,), -3, 3, 15).tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    assert not torch.equal(R.randint((64,), -3, 3, 16), R.randint((64,), -3, 3, 17))


def test_precondition_rejects_sums_at_2_24():
    with pytest.raises(AssertionError):
        R.assert_exact_ok(torch.tensor([2.0 ** 24]))
    R.assert_exact_ok(torch.tensor([2.0 ** 24 - 1]))


def test_term_counts_and_accumulate():
    x, w = torch.zeros(1, 2, 4, 4), torch.zeros(3, 2, 3, 3)
    dy = torch.zeros(1, 3, 4, 4)
    ny, ndx, ndw = R.term_counts(x, w, dy, 1, 1)
    assert float(ny[0, 0, 1, 1]) == 18 and float(ny[0, 0, 0, 0]) == 8       # interior: 9 taps x 2 channels
    assert float(ndx[0, 0, 1, 1]) == 27 and float(ndw[0, 0, 1, 1]) == 16    # centre tap: every output pixel
    assert float(ndw[0, 0, 0, 0]) == 9
    y0 = torch.ones(1, 3, 4, 4)
    assert torch.equal(R.forward(x, w, None, 1, 1, y0), y0.double())
