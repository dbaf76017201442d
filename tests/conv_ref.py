"""Plain float64 definitions of the dense convolution and its gradients (CPU only), the integer input generators
and the exactness precondition of tests/test_gpu_conv_exact.py. Pinned by tests/test_conv_ref.py.

Everything here is logical NCHW / (K, C, R, S), as torch.nn.functional.conv2d takes it.

Exactness: with integer-valued inputs every product is an integer and every partial sum, in any order, is an integer
no larger in magnitude than S = sum |terms| of that output. Below 2^24 all of them are fp32 numbers, so an fp32
accumulation of any tiling, split count or order returns the float64 result bit for bit. S is the same convolution
of the absolute values (abs_maps)."""
import torch
import torch.nn.functional as F

LIMIT = float(2 ** 24)


def _pair(v):
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


def forward(x, w, b=None, stride=1, pad=0, y0=None):
    """y = conv2d(x, w) (+ b) (+ y0: the accumulate form), float64."""
    y = F.conv2d(x.double(), w.double(), None if b is None else b.double(), _pair(stride), _pair(pad))
    return y if y0 is None else y + y0.double()


def grads(x, w, dy, stride=1, pad=0):
    """(dx, dw) of sum(conv2d(x, w) * dy) by autograd of the float64 forward."""
    xd = x.double().detach().requires_grad_(True)
    wd = w.double().detach().requires_grad_(True)
    y = F.conv2d(xd, wd, None, _pair(stride), _pair(pad))
    dx, dw = torch.autograd.grad(y, (xd, wd), dy.double())
    return dx, dw


def bias_grad(dy):
    return dy.double().sum((0, 2, 3))


def channel_stats(y):
    """Per-channel (sum y, sum y^2) of a stored output."""
    yd = y.double()
    return yd.sum((0, 2, 3)), (yd * yd).sum((0, 2, 3))


def abs_maps(x, w, dy, stride=1, pad=0, b=None):
    """(Sy, Sdx, Sdw): sum |terms| of every element of y, dx and dw (the convolutions of the absolute values)."""
    xa, wa, da = x.double().abs(), w.double().abs(), dy.double().abs()
    sy = forward(xa, wa, None if b is None else b.abs(), stride, pad)
    sdx, sdw = grads(xa, wa, da, stride, pad)
    return sy, sdx, sdw


def term_counts(x, w, dy, stride=1, pad=0):
    """(ny, ndx, ndw): how many products each element of y, dx and dw sums (the convolutions of ones)."""
    return abs_maps(torch.ones_like(x), torch.ones_like(w), torch.ones_like(dy), stride, pad)


def randint(shape, lo, hi, seed, zero_frac=0.25):
    """Seeded integers in [lo, hi] as float32, position dependent, with about zero_frac of the entries set to zero."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi + 1, shape, generator=g).float()
    keep = torch.rand(shape, generator=g) >= zero_frac
    return v * keep


def assert_exact_ok(*smaps, limit=LIMIT):
    """The precondition of the exact tier, on the reference (before any device call): every sum of |terms| < 2^24."""
    for s in smaps:
        m = float(s.max()) if s.numel() else 0.0
        assert m < limit, f"sum |terms| = {m} reaches 2^24: the integer case is not exact by construction"


def assert_integer(*ts):
    for t in ts:
        assert bool((t == t.round()).all()), "reference is not integer valued"
