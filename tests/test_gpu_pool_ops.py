"""Op-level parity of the pooling, resampling, separable-gate (adr_pool.hip) and MLCA (adr_mlca.hip) kernels against
the float64 references of pool_ref.py, through the public wrappers of adrefine.kernels (and, for the scalar fallback
on misaligned views, the C entry points themselves), at the shapes where a path changes: channel counts that take
the 16-byte vector path or the scalar one, G = C / VW that does not divide 256 (idle lanes) or exceeds it (the cstep
channel loop, the second cb pass of the reductions), maps that are not square, not multiples of 5, smaller than the
pooling window or the 5x5 MLCA grid, non-uniform adaptive windows, non-integer bilinear ratios, a 1x1 bilinear source,
more pixels than the 65 536-block grid cap (the grid-stride step), accumulate=1 stores into a fan-out's shared
gradient, channel-sliced (strided) inputs and outputs.

Inputs are seeded CPU values rounded to the compute dtype; the same rounded values go to the reference (as doubles)
and to the device (as NHWC activations). Outputs, input gradients and parameter gradients are compared elementwise.

fp32 mode: the project's fp32 bar, max|a-b| <= 2e-4 + 2e-4 max|b| (gpu_util.TOL), and also max|a-b| <= 2e-4 max|b|.

bf16 mode: per tensor, the HIP error against the float64 reference may be at most twice the error of the ideal-bf16
restatement of the op (pool_ref.bf16_*: float64 maths, rounding only the stored output and activation gradients, an
accumulated gradient at the destination before the add and at the sum) plus one bf16 ulp (2^-8) of the tensor's max,
in max norm and in L2 norm. The bound comes from the restatement, never from the kernel. MLCA's weight gradients are
fp32: their restatement error is zero and only the ulp term is left.

Exact (torch.equal on the stored values): max-pool and nearest-upsample forward (copies of inputs); their backward
in fp32 with small-integer upstream gradients (sums of at most 64 integers); the gate on bf16-representable operands
(the fp32 products are exact) and its plane gradient along an axis of length 1; the axis-mean backward with one
upstream plane zero along an axis of length 1; the adaptive-pool backward over uniform windows of 4 or 16 pixels; the
rows zero_other clears in the 'coord' layout. For the last, a NaN-filled tensor of the same size is allocated and freed
just before the call so that the allocator is likely to hand the kernel memory that does not already hold zeros; that
is best effort, nothing guarantees the block is reused.

A fan-out's consumers run backward in reverse order of creation (autograd's rule), so the second consumer stores its
gradient plainly and the first accumulates; the restatement follows that order and the test asserts on the sink that
a plain claim and an accumulating one were handed out.

Measured on an MI355X, worst case over the shapes of each op (bf16: HIP error / restatement error, each relative
to max|ref|, for the worst tensor by ratio to its bound; fp32: worst max|a-b| / max|b|):
    op                   fp32      bf16 HIP   bf16 restatement   worst bf16 tensor
    maxpool (dx)         2.0e-7    2.56e-3    2.56e-3            dx, k=5, 5x7, C=2056
    adapool              1.8e-7    2.66e-3    2.66e-3            dx, 15x15->3x3, C=128
    bilinear             1.2e-6    2.07e-3    2.07e-3            y, 2x3->5x7, C=2056
    nearest (dx)         3.7e-7    3.55e-3    3.55e-3            dx, s=2, 5x7, C=2056
    axis_mean            2.3e-7    3.28e-3    3.28e-3            dx, coord, 5x7, C=2056
    gate                 6.0e-7    2.62e-3    2.62e-3            out, ela2, 21x13, C=128, x=None
    mlca                 9.3e-7    3.18e-3    3.18e-3            out, B=5, 21x13, C=128, k=7
    accumulate (6 ops)   4.0e-7    4.16e-3    4.16e-3            dx, adapool, C=128
    scalar C entry pts   3.8e-7    2.55e-3    2.55e-3            y, bilinear, store
No bf16 tensor uses more than 0.49 of its bound: the kernels' fp32 arithmetic rounds where the restatement does. Every
exact comparison (651 tensors) had no differing element.
"""
import ctypes

import pytest
import torch

import adrefine.kernels as K
import pool_ref as R
from adrefine.native import lib
from gpu_util import TOL

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
ULP = 2.0 ** -8
N2 = 2

NARROW = {F32: [(128, "vec_G32"), (24, "vec_G6_not_dividing_256"), (20, "vec_G5_not_dividing_256"), (13, "scalar")],
          BF16: [(128, "vec_G16"), (24, "vec_G3_not_dividing_256"), (20, "scalar"), (13, "scalar")]}
WIDE = {F32: [(257, "scalar_G257_gt_256_second_cb_pass"), (1028, "vec_G257_gt_256_second_cb_pass")],
        BF16: [(257, "scalar_G257_gt_256_second_cb_pass"), (2056, "vec_G257_gt_256_second_cb_pass")]}
ALIGNED = [pytest.param(dt, C, id=f"{'fp32' if dt == F32 else 'bf16'}-C{C}") for dt in (F32, BF16) for C in (128, 24)]


def chans(table):
    return [pytest.param(dt, C, id=f"{'fp32' if dt == F32 else 'bf16'}-C{C}-{path}")
            for dt in (F32, BF16) for C, path in table[dt]]


def tag(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def rnd(N, C, H, W, seed, dtype, ints=None):
    """Seeded CPU values rounded to dtype, logical (N, C, H, W); ints=(lo, hi): integers in [lo, hi]."""
    g = torch.Generator().manual_seed(seed)
    if ints is not None:
        t = torch.randint(ints[0], ints[1] + 1, (N, H, W, C), generator=g).float()
    else:
        t = torch.randn(N, H, W, C, generator=g)
    return t.to(dtype).permute(0, 3, 1, 2)


def dev(x, grad=True):
    """The NHWC activation on the device (a leaf)."""
    return x.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2).requires_grad_(grad)


def dev_slice(x, off=8):
    """The same activation as channels [off, off + C) of a wider NHWC leaf (the rest holds 3.0)."""
    N, C, H, W = x.shape
    wide = torch.full((N, H, W, off + C + 8), 3.0, dtype=x.dtype)
    wide[..., off:off + C] = x.permute(0, 2, 3, 1)
    leaf = wide.cuda().permute(0, 3, 1, 2).requires_grad_(True)
    return leaf, leaf[:, off:off + C]


def feed(x, sliced):
    """(leaf, activation): the activation is the leaf itself, or an aligned channel slice [8, 8 + C) of it."""
    if sliced:
        return dev_slice(x)
    d = dev(x)
    return d, d


def grad_of(leaf, x, sliced):
    if not sliced:
        return leaf.grad
    C = x.shape[1]
    g = leaf.grad
    assert float(g[:, :8].abs().max()) == 0 and float(g[:, 8 + C:].abs().max()) == 0
    return g[:, 8:8 + C]


def host(t):
    return t.detach().double().cpu()


def compare(dtype, what, got, ref, rest=None):
    """One tensor against the reference (see the module docstring); rest is the bf16 restatement of ref."""
    got = host(got).reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    if dtype == F32:
        print(f"POOLERR fp32 {what} err={err:.3e} scale={scale:.3e} rel={err / (scale + 1e-300):.3e}")
        t = TOL[F32]
        assert err <= t["atol"] + t["rtol"] * scale, f"{what}: max|d|={err:.3e} scale={scale:.3e}"
        assert err <= t["rtol"] * scale, f"{what}: max|d|={err:.3e} > 2e-4 * {scale:.3e}"
    else:
        rest = ref if rest is None else rest
        rerr, l2, rl2 = float((rest - ref).abs().max()), float((got - ref).norm()), float((rest - ref).norm())
        print(f"POOLERR bf16 {what} err={err:.3e} rest={rerr:.3e} l2={l2:.3e} restl2={rl2:.3e} scale={scale:.3e} "
              f"rel={err / (scale + 1e-300):.3e} restrel={rerr / (scale + 1e-300):.3e} "
              f"use={max(err / (2 * rerr + ULP * scale + 1e-300), l2 / (2 * rl2 + ULP * scale + 1e-300)):.3f}")
        assert err <= 2 * rerr + ULP * scale, f"{what}: max|d|={err:.3e} > 2 * {rerr:.3e} + ulp {ULP * scale:.3e}"
        assert l2 <= 2 * rl2 + ULP * scale, f"{what}: |d|_2={l2:.3e} > 2 * {rl2:.3e} + ulp {ULP * scale:.3e}"


def exact(what, got, ref):
    """The stored values themselves: the reference rounded to the storage dtype, no tolerance."""
    got = got.detach().cpu()
    want = ref.to(got.dtype).reshape(got.shape)
    print(f"POOLERR {tag(got.dtype)} {what} exact differing={int((got != want).sum())}")
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {got.numel()} stored values differ"


def rest_of(dtype, outs, grads):
    return R.bf16_stored(outs, grads) if dtype == BF16 else ([None] * len(outs), [None] * len(grads))


# ---- max pool -------------------------------------------------------------------------------------------------

MAXPOOL_MAPS = [(1, 1, 5), (2, 3, 5), (4, 4, 5), (5, 7, 5), (13, 13, 5), (20, 20, 5), (7, 5, 3), (7, 5, 13)]


def check_maxpool(dtype, C, H, W, k, sliced=False, N=N2, x=None, name=None):
    x = rnd(N, C, H, W, 100 + H * W + C, dtype) if x is None else x
    up = rnd(N, C, H, W, 150 + H * W + C, dtype)
    leaf, xd = feed(x, sliced)
    y = K.maxpool(xd, k)
    y.backward(dev(up, grad=False))
    (ro,), (rg,) = R.run(lambda t: R.ref_maxpool(t, k), [x], [up])
    (_,), (sg,) = rest_of(dtype, [ro], [rg])
    name = name or f"maxpool k={k} {H}x{W} C={C}{' sliced' if sliced else ''}"
    exact(f"{name} y", y, ro)
    compare(dtype, f"{name} dx", grad_of(leaf, x, sliced), rg, sg)


@pytest.mark.parametrize("dtype,C", chans(NARROW))
@pytest.mark.parametrize("H,W,k", MAXPOOL_MAPS, ids=[f"{h}x{w}-k{k}" for h, w, k in MAXPOOL_MAPS])
def test_maxpool(dtype, C, H, W, k):
    check_maxpool(dtype, C, H, W, k)


@pytest.mark.parametrize("dtype,C", chans(WIDE))
def test_maxpool_wide(dtype, C):
    check_maxpool(dtype, C, 5, 7, 5)


@pytest.mark.parametrize("C", [128, 24, 13, 257], ids=lambda c: f"fp32-C{c}")
@pytest.mark.parametrize("H,W", [(5, 7), (13, 13)])
def test_maxpool_ties_and_integer_gradients_exact(C, H, W):
    """A map of three distinct values (most windows tie) and integer upstream gradients: the first maximum in
    row-major window order takes the gradient, every sum is one of at most 25 small integers — exact in fp32."""
    x = rnd(N2, C, H, W, 200 + C, F32, ints=(0, 2))
    up = rnd(N2, C, H, W, 201 + C, F32, ints=(-3, 3))
    xd = dev(x)
    y = K.maxpool(xd, 5)
    y.backward(dev(up, grad=False))
    (ro,), (rg,) = R.run(lambda t: R.ref_maxpool(t, 5), [x], [up])
    exact(f"maxpool ties {H}x{W} C={C} y", y, ro)
    exact(f"maxpool ties {H}x{W} C={C} dx", xd.grad, rg)


@pytest.mark.parametrize("dtype,C", ALIGNED)
def test_maxpool_strided_in_and_out(dtype, C):
    """Input a channel slice of a wider leaf, output (out=) a channel slice of a wider buffer: no re-layout, and
    the rest of the buffer untouched."""
    H, W = 5, 7
    x = rnd(N2, C, H, W, 300 + C, dtype)
    n0 = K.relayout_count[0]
    check_maxpool(dtype, C, H, W, 5, sliced=True, x=x)
    buf = torch.full((N2, H, W, C + 16), 3.0, dtype=dtype, device="cuda").permute(0, 3, 1, 2)
    y = K.maxpool(dev_slice(x)[1].detach(), 5, out=buf[:, 8:8 + C])
    assert K.relayout_count[0] == n0
    exact(f"maxpool out= C={C} y", y, R.ref_maxpool(x.double(), 5))
    assert y.data_ptr() == buf[:, 8:8 + C].data_ptr()
    assert bool((buf[:, :8] == 3.0).all()) and bool((buf[:, 8 + C:] == 3.0).all())


@pytest.mark.parametrize("dtype,C", chans(NARROW))
def test_maxpool_nan_propagates(dtype, C):
    """One NaN per channel plane: every window that holds it outputs NaN and sends its gradient there."""
    H, W, k = 7, 9, 5
    x = rnd(N2, C, H, W, 400 + C, dtype).contiguous()
    x[:, :, 3, 4] = float("nan")
    up = rnd(N2, C, H, W, 401 + C, dtype)
    xd = dev(x)
    y = K.maxpool(xd, k)
    y.backward(dev(up, grad=False))
    (ro,), (rg,) = R.run(lambda t: R.ref_maxpool(t, k), [x], [up])
    yc, nan = y.detach().cpu(), torch.isnan(ro)
    assert int(nan.sum()) == N2 * C * 25 and torch.equal(torch.isnan(yc), nan)
    z = torch.zeros((), dtype=dtype)
    exact(f"maxpool nan C={C} y", torch.where(nan, z, yc), torch.where(nan, z.double(), ro))
    (_,), (sg,) = rest_of(dtype, [ro], [rg])
    compare(dtype, f"maxpool nan C={C} dx", xd.grad, rg, sg)
    assert float(rg[:, :, 3, 4].abs().min()) > 0


@pytest.mark.parametrize("dtype,C", chans(NARROW))
def test_maxpool_all_minus_inf_window(dtype, C):
    """-inf everywhere but one finite value: a window of nothing but -inf outputs -inf and routes its gradient to
    its first in-range tap, as ATen's kernel does (at a border that is not window position (0, 0))."""
    H, W, k = 7, 9, 5
    x = torch.full((N2, C, H, W), float("-inf"), dtype=dtype)
    x[:, :, 3, 4] = 1.5
    up = rnd(N2, C, H, W, 451 + C, dtype)
    xd = dev(x)
    y = K.maxpool(xd, k)
    y.backward(dev(up, grad=False))
    (ro,), (rg,) = R.run(lambda t: R.ref_maxpool(t, k), [x], [up])
    exact(f"maxpool -inf C={C} y", y, ro)
    assert float(rg[:, :, 0, 0].abs().min()) > 0  # the corner windows are all -inf: their gradient lands at (0, 0)
    (_,), (sg,) = rest_of(dtype, [ro], [rg])
    compare(dtype, f"maxpool -inf C={C} dx", xd.grad, rg, sg)


# ---- adaptive average pool, bilinear ----------------------------------------------------------------------------


def check_resize(op, dtype, C, H, W, OH, OW, sliced=False, N=N2):
    hip, ref = {"adapool": (K.adaptive_avg_pool, R.ref_adapool), "bilinear": (K.bilinear, R.ref_bilinear)}[op]
    x = rnd(N, C, H, W, 500 + 31 * H + W + C, dtype)
    up = rnd(N, C, OH, OW, 550 + 31 * OH + OW + C, dtype)
    leaf, xd = feed(x, sliced)
    y = hip(xd, OH, OW)
    y.backward(dev(up, grad=False))
    (ro,), (rg,) = R.run(lambda t: ref(t, OH, OW), [x], [up])
    (so,), (sg,) = rest_of(dtype, [ro], [rg])
    name = f"{op} {H}x{W}->{OH}x{OW} C={C}{' sliced' if sliced else ''}"
    compare(dtype, f"{name} y", y, ro, so)
    compare(dtype, f"{name} dx", grad_of(leaf, x, sliced), rg, sg)
    return x, up, xd, rg


PAIRS = [(20, 20, 2), (20, 20, 4), (21, 13, 2), (21, 13, 4), (15, 15, 2), (15, 15, 4), (7, 5, 2), (7, 5, 4)]
PAIR_IDS = ["20x20-s2-uniform", "20x20-s4-uniform", "21x13-s2-nonuniform_windows", "21x13-s4-noninteger_ratio",
            "15x15-s2-nonuniform_windows", "15x15-s4-noninteger_ratio", "7x5-s2", "7x5-s4-bilinear_from_1x1"]


@pytest.mark.parametrize("dtype,C", chans(NARROW))
@pytest.mark.parametrize("H,W,s", PAIRS, ids=PAIR_IDS)
def test_adapool_then_bilinear(dtype, C, H, W, s):
    """The pair CrossScaleAttentionTSSA makes, (H, W) -> (H // s, W // s) -> (H, W), each op on its own seeded
    input."""
    check_resize("adapool", dtype, C, H, W, H // s, W // s)
    check_resize("bilinear", dtype, C, H // s, W // s, H, W)


ALONE = [(7, 3), (3, 7), (5, 4), (1, 4), (13, 5)]


@pytest.mark.parametrize("dtype,C", chans(NARROW))
@pytest.mark.parametrize("a,b", ALONE, ids=[f"{a}to{b}" for a, b in ALONE])
@pytest.mark.parametrize("op", ["adapool", "bilinear"])
def test_resize_alone(op, dtype, C, a, b):
    check_resize(op, dtype, C, a, a, b, b)
    check_resize(op, dtype, C, a, b, b, a)  # the two axes in opposite directions


@pytest.mark.parametrize("dtype,C", chans(WIDE))
@pytest.mark.parametrize("op", ["adapool", "bilinear"])
def test_resize_wide(op, dtype, C):
    check_resize(op, dtype, C, 5, 7, 2, 3)
    check_resize(op, dtype, C, 2, 3, 5, 7)


@pytest.mark.parametrize("dtype,C", chans(NARROW))
@pytest.mark.parametrize("O", [10, 5])
def test_adapool_backward_uniform_windows_exact(dtype, C, O):
    """20x20 -> 10x10 / 5x5: every input pixel lies in one window of 4 / 16 pixels, so dx is one upstream value
    divided by a power of two."""
    x, up, xd, rg = check_resize("adapool", dtype, C, 20, 20, O, O)
    exact(f"adapool 20x20->{O}x{O} C={C} dx", xd.grad, rg)


@pytest.mark.parametrize("dtype,C", ALIGNED)
@pytest.mark.parametrize("op", ["adapool", "bilinear"])
def test_resize_strided(op, dtype, C):
    n0 = K.relayout_count[0]
    check_resize(op, dtype, C, 7, 5, 3, 4, sliced=True)
    assert K.relayout_count[0] == n0


# ---- axis means and the separable gate ----------------------------------------------------------------------------

LAYOUT_MAPS = [("ela", 20, 20), ("ela", 13, 13), ("ela2", 21, 13), ("ela2", 1, 9), ("ela2", 9, 1), ("coord", 16, 16),
               ("coord", 8, 4), ("coord", 5, 7)]
LAYOUT_IDS = [f"{lay}-{h}x{w}" for lay, h, w in LAYOUT_MAPS]


def plane_shapes(layout, N, C, H, W):
    return {"ela": [(2 * N, C, H, 1)], "ela2": [(N, C, H, 1), (N, C, W, 1)], "coord": [(N, C, H + W, 1)]}[layout]


def check_axis_mean(dtype, C, layout, H, W, sliced=False, N=N2):
    x = rnd(N, C, H, W, 600 + 31 * H + W + C, dtype)
    ups = [rnd(*s, 650 + i + C, dtype) for i, s in enumerate(plane_shapes(layout, N, C, H, W))]
    leaf, xd = feed(x, sliced)
    out = K.axis_mean(xd, layout)
    outs = list(out) if isinstance(out, tuple) else [out]
    torch.autograd.backward(outs, [dev(u, grad=False) for u in ups])
    ro, (rg,) = R.run(lambda t: R.ref_axis_mean(t, layout), [x], ups)
    so, (sg,) = rest_of(dtype, ro, [rg])
    name = f"axis_mean {layout} {H}x{W} C={C}{' sliced' if sliced else ''}"
    for i, (o, r, s) in enumerate(zip(outs, ro, so)):
        compare(dtype, f"{name} out{i}", o, r, s)
    compare(dtype, f"{name} dx", grad_of(leaf, x, sliced), rg, sg)


@pytest.mark.parametrize("dtype,C", chans(NARROW))
@pytest.mark.parametrize("layout,H,W", LAYOUT_MAPS, ids=LAYOUT_IDS)
def test_axis_mean(dtype, C, layout, H, W):
    check_axis_mean(dtype, C, layout, H, W)


@pytest.mark.parametrize("dtype,C", chans(WIDE))
@pytest.mark.parametrize("layout", ["ela2", "coord"])
def test_axis_mean_wide(dtype, C, layout):
    check_axis_mean(dtype, C, layout, 5, 7)


@pytest.mark.parametrize("dtype,C", chans(NARROW))
@pytest.mark.parametrize("H,W", [(9, 1), (1, 9)])
def test_axis_mean_backward_one_term_exact(dtype, C, H, W):
    """ela2 on a map one pixel wide (high), upstream only on the means along the long axis: dx = dh / 1 + 0 / 9 is
    that upstream value itself."""
    x = rnd(N2, C, H, W, 700 + C, dtype)
    uh, uw = rnd(N2, C, H, 1, 701 + C, dtype), rnd(N2, C, W, 1, 702 + C, dtype)
    if W == 1:
        uw = torch.zeros_like(uw)
    else:
        uh = torch.zeros_like(uh)
    xd = dev(x)
    oh, ow = K.axis_mean(xd, "ela2")
    torch.autograd.backward([oh, ow], [dev(uh, grad=False), dev(uw, grad=False)])
    _, (rg,) = R.run(lambda t: R.ref_axis_mean(t, "ela2"), [x], [uh, uw])
    exact(f"axis_mean ela2 {H}x{W} C={C} one-term dx", xd.grad, rg)
    exact(f"axis_mean ela2 {H}x{W} C={C} mean over one pixel", oh if W == 1 else ow, x.double().reshape(N2, C, -1, 1))


def gate_inputs(dtype, C, layout, H, W, N, with_x, seed):
    x = rnd(N, C, H, W, seed, dtype) if with_x else None
    shapes = plane_shapes(layout, N, C, H, W)
    if layout == "coord":
        shapes = shapes * 2
    planes = [rnd(*s, seed + 1 + i, dtype) for i, s in enumerate(shapes)]
    return x, planes, rnd(N, C, H, W, seed + 5, dtype)


def run_gate(x, planes, up, layout, sliced=False, poison=False):
    """-> out, [dx, dah, daw] on the device (daw None in the 'ela' layout, dx None without x)."""
    N, C, H, W = up.shape
    leaf, xd = feed(x, sliced) if x is not None else (None, None)
    pd = [dev(p) for p in planes]
    ah, aw = (pd[0], pd[0]) if layout == "ela" else pd
    out = K.gate(xd, ah, aw, layout, (N, C, H, W))
    upd = dev(up, grad=False)
    if poison:  # best effort: make the allocator's next blocks of this size hold NaN, not zeros
        junk = [torch.full_like(p, float("nan")) for p in pd]
        torch.cuda.synchronize()
        del junk
    out.backward(upd)
    return out, [None if x is None else grad_of(leaf, x, sliced), pd[0].grad, None if layout == "ela" else pd[1].grad]


def ref_gate_run(x, planes, up, layout):
    N, C, H, W = up.shape
    if layout == "ela":
        ro, (gx, ga) = R.run(lambda t, a: R.ref_gate(t, a, a, layout, N, H, W), [x, planes[0]], [up])
        return ro, [gx, ga, None]
    return R.run(lambda t, a, b: R.ref_gate(t, a, b, layout, N, H, W), [x] + planes, [up])


def check_gate(dtype, C, layout, H, W, with_x, sliced=False, N=N2):
    x, planes, up = gate_inputs(dtype, C, layout, H, W, N, with_x, 800 + 31 * H + W + C)
    out, grads = run_gate(x, planes, up, layout, sliced, poison=layout == "coord")
    ro, rg = ref_gate_run(x, planes, up, layout)
    so, sg = rest_of(dtype, ro, rg)
    name = f"gate {layout} {H}x{W} C={C}{'' if with_x else ' x=None'}{' sliced' if sliced else ''}"
    compare(dtype, f"{name} out", out, ro[0], so[0])
    for n, g, r, s in zip(("dx", "dah", "daw"), grads, rg, sg):
        if r is not None:
            compare(dtype, f"{name} {n}", g, r, s)
    if layout == "coord":  # the rows the gate never reads: zero_other clears them (see the module docstring)
        exact(f"{name} dah rows H..", grads[1][:, :, H:], rg[1][:, :, H:])
        exact(f"{name} daw rows ..H", grads[2][:, :, :H], rg[2][:, :, :H])
        assert float(rg[1][:, :, H:].abs().max()) == 0 and float(rg[2][:, :, :H].abs().max()) == 0


@pytest.mark.parametrize("dtype,C", chans(NARROW))
@pytest.mark.parametrize("with_x", [True, False], ids=["x", "x_None"])
@pytest.mark.parametrize("layout,H,W", LAYOUT_MAPS, ids=LAYOUT_IDS)
def test_gate(dtype, C, layout, H, W, with_x):
    check_gate(dtype, C, layout, H, W, with_x)


@pytest.mark.parametrize("dtype,C", chans(WIDE))
@pytest.mark.parametrize("layout", ["ela2", "coord"])
def test_gate_wide(dtype, C, layout):
    check_gate(dtype, C, layout, 5, 7, True)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [(300, 5), (5, 300)])
def test_long_reduce_axis(dtype, H, W):
    """L = 300 along the reduced axis at C = 24: each thread of the axis-mean and gate-gradient reductions walks its
    line more than once (256 / G line splits, G = 6 / 3)."""
    check_axis_mean(dtype, 24, "ela2", H, W)
    check_gate(dtype, 24, "ela2", H, W, True)


@pytest.mark.parametrize("dtype,C", chans(NARROW))
@pytest.mark.parametrize("layout,H,W", [("ela", 13, 13), ("ela2", 9, 1), ("ela2", 1, 9), ("coord", 5, 7)])
@pytest.mark.parametrize("with_x", [True, False], ids=["x", "x_None"])
def test_gate_exact_on_short_mantissas(dtype, C, layout, H, W, with_x):
    """Operands representable in bf16 (held in either dtype): a_h * a_w and its product with x or dout are exact in
    fp32, so out and dx have one term and one rounding, the store. Along an axis of length 1 so has the plane
    gradient."""
    x, planes, up = gate_inputs(BF16, C, layout, H, W, N2, with_x, 900 + C)
    x, planes, up = None if x is None else x.to(dtype), [p.to(dtype) for p in planes], up.to(dtype)
    out, grads = run_gate(x, planes, up, layout)
    ro, rg = ref_gate_run(x, planes, up, layout)
    name = f"gate exact {layout} {H}x{W} C={C}{'' if with_x else ' x=None'}"
    exact(f"{name} out", out, ro[0])
    if with_x:
        exact(f"{name} dx", grads[0], rg[0])
    if W == 1:
        exact(f"{name} dah", grads[1], rg[1])
    if H == 1:
        exact(f"{name} daw", grads[2], rg[2])


@pytest.mark.parametrize("dtype,C", ALIGNED)
@pytest.mark.parametrize("layout,H,W", [("ela", 13, 13), ("ela2", 21, 13), ("coord", 5, 7)])
def test_axis_mean_and_gate_strided(dtype, C, layout, H, W):
    n0 = K.relayout_count[0]
    check_axis_mean(dtype, C, layout, H, W, sliced=True)
    check_gate(dtype, C, layout, H, W, True, sliced=True)
    assert K.relayout_count[0] == n0


# ---- nearest upsample -----------------------------------------------------------------------------------------------

NEAREST = [(s, h, w) for s in (1, 2, 3, 8) for h, w in ((1, 1), (3, 5), (10, 10))]


def check_nearest(dtype, C, H, W, s, sliced=False, N=N2):
    x = rnd(N, C, H, W, 1000 + 31 * H + W + C, dtype)
    up = rnd(N, C, H * s, W * s, 1050 + s + C, dtype)
    leaf, xd = feed(x, sliced)
    y = K.upsample_nearest(xd, s)
    y.backward(dev(up, grad=False))
    (ro,), (rg,) = R.run(lambda t: R.ref_nearest(t, s), [x], [up])
    (_,), (sg,) = rest_of(dtype, [ro], [rg])
    name = f"nearest s={s} {H}x{W} C={C}{' sliced' if sliced else ''}"
    exact(f"{name} y", y, ro)
    compare(dtype, f"{name} dx", grad_of(leaf, x, sliced), rg, sg)


@pytest.mark.parametrize("dtype,C", chans(NARROW))
@pytest.mark.parametrize("s,H,W", NEAREST, ids=[f"s{s}-{h}x{w}" for s, h, w in NEAREST])
def test_upsample_nearest(dtype, C, s, H, W):
    check_nearest(dtype, C, H, W, s)


@pytest.mark.parametrize("dtype,C", chans(WIDE))
def test_upsample_nearest_wide(dtype, C):
    check_nearest(dtype, C, 5, 7, 2)


@pytest.mark.parametrize("C", [128, 24, 13, 257], ids=lambda c: f"fp32-C{c}")
@pytest.mark.parametrize("s", [1, 3, 8])
def test_upsample_nearest_integer_gradients_exact(C, s):
    """Integer upstream gradients in fp32: dx is a sum of s * s <= 64 small integers."""
    H, W = 3, 5
    x = rnd(N2, C, H, W, 1100 + C, F32)
    up = rnd(N2, C, H * s, W * s, 1101 + C, F32, ints=(-3, 3))
    xd = dev(x)
    K.upsample_nearest(xd, s).backward(dev(up, grad=False))
    _, (rg,) = R.run(lambda t: R.ref_nearest(t, s), [x], [up])
    exact(f"nearest ints s={s} C={C} dx", xd.grad, rg)


@pytest.mark.parametrize("dtype,C", ALIGNED)
def test_upsample_nearest_strided_in_and_out(dtype, C):
    H, W, s = 3, 5, 2
    n0 = K.relayout_count[0]
    check_nearest(dtype, C, H, W, s, sliced=True)
    x = rnd(N2, C, H, W, 1200 + C, dtype)
    buf = torch.full((N2, H * s, W * s, C + 16), 3.0, dtype=dtype, device="cuda").permute(0, 3, 1, 2)
    y = K.upsample_nearest(dev_slice(x)[1].detach(), s, out=buf[:, 8:8 + C])
    assert K.relayout_count[0] == n0
    exact(f"nearest out= C={C} y", y, R.ref_nearest(x.double(), s))
    assert y.data_ptr() == buf[:, 8:8 + C].data_ptr()
    assert bool((buf[:, :8] == 3.0).all()) and bool((buf[:, 8 + C:] == 3.0).all())


# ---- the grid-stride step ---------------------------------------------------------------------------------------------


def test_grid_stride_step_gate():
    """fp32, C = 129 (scalar, one pixel per block), 1 x 260 x 253 = 65 780 pixels: past the 65 536-block grid cap,
    so the blocks take a second pass of POOL_LOOP."""
    assert 260 * 253 > 65536
    check_gate(F32, 129, "ela2", 260, 253, True, N=1)


def test_grid_stride_step_upsample_nearest_backward():
    assert 260 * 253 > 65536
    check_nearest(F32, 129, 260, 253, 1, N=1)


# ---- accumulate=1 into a fan-out's shared gradient ----------------------------------------------------------------------


def _consumers(op, x, N, C, H, W, dtype, seed):
    """Two (hip, ref, upstream gradients) consumers of one activation for op."""
    def ups(j, *shapes):
        return [rnd(*s, seed + 100 * j + 7 * i, dtype) for i, s in enumerate(shapes)]
    full = (N, C, H, W)
    if op == "maxpool":
        return [(lambda t: K.maxpool(t, 5), lambda t: R.ref_maxpool(t, 5), ups(0, full)),
                (lambda t: K.maxpool(t, 3), lambda t: R.ref_maxpool(t, 3), ups(1, full))]
    if op == "adapool":
        return [(lambda t: K.adaptive_avg_pool(t, 3, 2), lambda t: R.ref_adapool(t, 3, 2), ups(0, (N, C, 3, 2))),
                (lambda t: K.adaptive_avg_pool(t, 4, 4), lambda t: R.ref_adapool(t, 4, 4), ups(1, (N, C, 4, 4)))]
    if op == "bilinear":
        return [(lambda t: K.bilinear(t, 11, 9), lambda t: R.ref_bilinear(t, 11, 9), ups(0, (N, C, 11, 9))),
                (lambda t: K.bilinear(t, 3, 3), lambda t: R.ref_bilinear(t, 3, 3), ups(1, (N, C, 3, 3)))]
    if op == "nearest":
        return [(lambda t: K.upsample_nearest(t, 2), lambda t: R.ref_nearest(t, 2), ups(0, (N, C, 2 * H, 2 * W))),
                (lambda t: K.upsample_nearest(t, 3), lambda t: R.ref_nearest(t, 3), ups(1, (N, C, 3 * H, 3 * W)))]
    if op == "axis_mean":
        return [(lambda t: K.axis_mean(t, "ela2"), lambda t: R.ref_axis_mean(t, "ela2"),
                 ups(0, (N, C, H, 1), (N, C, W, 1))),
                (lambda t: K.axis_mean(t, "coord"), lambda t: R.ref_axis_mean(t, "coord"), ups(1, (N, C, H + W, 1)))]
    assert op == "gate"
    out = []
    for j in range(2):
        ah, aw = rnd(N, C, H, 1, seed + 20 + j, dtype), rnd(N, C, W, 1, seed + 30 + j, dtype)
        out.append((lambda t, ah=ah, aw=aw: K.gate(t, dev(ah, False), dev(aw, False), "ela2", full),
                    lambda t, ah=ah, aw=aw: R.ref_gate(t, ah.double(), aw.double(), "ela2", N, H, W),
                    [rnd(*full, seed + 40 + j, dtype)]))
    return out


@pytest.mark.parametrize("dtype,C", ALIGNED)
@pytest.mark.parametrize("op", ["maxpool", "adapool", "bilinear", "nearest", "axis_mean", "gate"])
def test_accumulate_into_fanout_sink(monkeypatch, op, dtype, C):
    """Two consumers of K.fanout(x, 2): both write their dx into the fan-out's shared buffer, the one that runs
    second with accumulate=1 (vstore_acc); x's gradient is the sum of both references."""
    N, H, W = N2, 7, 5
    x = rnd(N, C, H, W, 1300 + C, dtype)
    cons = _consumers(op, x, N, C, H, W, dtype, 1310 + C)
    claims = []
    claim = K.GradSink.claim

    def recording(self, device, can_add=False):
        r = claim(self, device, can_add)
        claims.append(r[1])
        return r

    monkeypatch.setattr(K.GradSink, "claim", recording)
    xd = dev(x)
    outs, ups = [], []
    for view, (hip, _, u) in zip(K.fanout(xd, 2), cons):
        assert K._sink_of(view) is not None
        o = hip(view)
        outs += list(o) if isinstance(o, tuple) else [o]
        ups += [dev(t, grad=False) for t in u]
    torch.autograd.backward(outs, ups)
    assert claims == [0, 1], claims  # one plain store, one accumulating store: the sum was formed in the kernel
    gs = [R.run(ref, [x], u)[1][0] for _, ref, u in cons]
    want = gs[0] + gs[1]
    rest = R.bf16_accumulated([gs[1], gs[0]]) if dtype == BF16 else None  # the later consumer runs backward first
    compare(dtype, f"accumulate {op} C={C} dx", xd.grad, want, rest)
    assert float(gs[0].abs().max()) > 0 and float(gs[1].abs().max()) > 0


# ---- MLCA ---------------------------------------------------------------------------------------------------------------


def mlca_weights(k, seed):
    g = torch.Generator().manual_seed(seed)
    return [0.5 * torch.randn(1, 1, k, generator=g), 0.5 * torch.randn(1, 1, k, generator=g)]


def check_mlca(dtype, B, C, H, W, k=3, with_res=True, sliced=False, lw=0.5):
    y = rnd(B, C, H, W, 1400 + 31 * H + W + C + B, dtype)
    res = rnd(B, C, H, W, 1450 + 31 * H + W + C + B, dtype) if with_res else None
    up = rnd(B, C, H, W, 1480 + 31 * H + W + C + B, dtype)
    wl, wg = mlca_weights(k, 1490 + k)
    leaf, yd = feed(y, sliced)
    rd = dev(res) if with_res else None
    pl, pg = wl.cuda().requires_grad_(True), wg.cuda().requires_grad_(True)
    out = K.mlca(yd, rd, pl, pg, lw)
    out.backward(dev(up, grad=False))
    (ro,), (rdy, rdres, rdwl, rdwg) = R.run(lambda a, r, p, q: R.ref_mlca(a, r, p, q, lw), [y, res, wl, wg], [up])
    so, sdy = (R.bf16_round(ro), R.bf16_round(rdy)) if dtype == BF16 else (None, None)
    name = f"mlca B={B} {H}x{W} C={C} k={k}{'' if with_res else ' no-res'}{' sliced' if sliced else ''}"
    compare(dtype, f"{name} out", out, ro, so)
    compare(dtype, f"{name} dy", grad_of(leaf, y, sliced), rdy, sdy)
    if with_res:
        exact(f"{name} dres", rd.grad, up.double())  # handed on unchanged
        assert torch.equal(rdres, up.double())
    compare(dtype, f"{name} dwl", pl.grad, rdwl)
    compare(dtype, f"{name} dwg", pg.grad, rdwg)
    return y, res, wl, wg, out


MLCA_MAPS = [(20, 20, "multiple_of_5"), (13, 13, "not_divisible_by_5"), (21, 13, "not_divisible_by_5_rect"),
             (7, 5, "rect"), (5, 5, "the_grid"), (4, 4, "smaller_than_5_overlapping_windows"), (1, 1, "one_pixel")]


@pytest.mark.parametrize("dtype,C", chans(NARROW))
@pytest.mark.parametrize("H,W", [m[:2] for m in MLCA_MAPS], ids=[f"{h}x{w}-{t}" for h, w, t in MLCA_MAPS])
def test_mlca_maps(dtype, C, H, W):
    check_mlca(dtype, 2, C, H, W)


@pytest.mark.parametrize("dtype,C", chans(NARROW))
@pytest.mark.parametrize("B", [1, 5, 7], ids=lambda b: f"batch{b}")
@pytest.mark.parametrize("H,W", [(13, 13), (4, 4)])
def test_mlca_batches(dtype, C, B, H, W):
    """The global branch is averaged over images rows(i) = [floor(i B / 5), ceil((i + 1) B / 5)) per bin row."""
    check_mlca(dtype, B, C, H, W)


@pytest.mark.parametrize("dtype,C", chans(NARROW))
@pytest.mark.parametrize("with_res", [True, False], ids=["res", "no_res"])
def test_mlca_k7(dtype, C, with_res):
    check_mlca(dtype, 2, C, 7, 5, k=7, with_res=with_res)
    check_mlca(dtype, 5, C, 21, 13, k=7, with_res=with_res)


@pytest.mark.parametrize("dtype,C", chans(NARROW))
def test_mlca_no_res_k3(dtype, C):
    check_mlca(dtype, 2, C, 13, 13, with_res=False)


@pytest.mark.parametrize("dtype,C", ALIGNED)
def test_mlca_strided(dtype, C):
    n0 = K.relayout_count[0]
    check_mlca(dtype, 2, C, 7, 5, sliced=True)
    assert K.relayout_count[0] == n0


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_mlca_couples_the_images_of_a_batch(dtype):
    """Perturbing image 1 changes image 0's output (the reference pools the global attention over the batch axis),
    on the device as in the reference."""
    y, res, wl, wg, out = check_mlca(dtype, 2, 24, 7, 5)
    y2 = y.clone()
    y2[1] = (y2[1].float() + 1.0).to(dtype)
    with torch.no_grad():
        out2 = K.mlca(dev(y2, False), dev(res, False), wl.cuda(), wg.cuda(), 0.5)
    ro, ro2 = (R.ref_mlca(t.double(), res.double(), wl.double(), wg.double()) for t in (y, y2))
    moved = float((ro2[0] - ro[0]).abs().max())
    assert moved > 1e-2 * float(ro[0].abs().max())
    got = float((host(out2)[0] - host(out)[0]).abs().max())
    assert got > 0.5 * moved
    compare(dtype, "mlca coupled out", out2, ro2, R.bf16_round(ro2))


# ---- the scalar fallback on misaligned views (C entry points) -----------------------------------------------------------

# Channel stride 20 at C = 16, the base pointer 4 elements into the allocation: 8 bytes in bf16, so vec_ok is false
# and the launch is the scalar instantiation. In fp32 4 elements are 16 bytes and a stride of 20 is a multiple of 4,
# so that view still takes the vector path (kept: a strided vector case); 2 elements in reach the scalar one.
MIS_CS = 20
MIS = [pytest.param(F32, 4, id="fp32-off4-vector_strided"), pytest.param(F32, 2, id="fp32-off2-scalar_misaligned"),
       pytest.param(BF16, 4, id="bf16-off4-scalar_misaligned"), pytest.param(BF16, 2, id="bf16-off2-scalar_misaligned")]


def mis(x, off, fill=7.0):
    """x (N, C, H, W) placed in a buffer with channel stride 20, starting off elements in; -> (buffer, view)."""
    N, C, H, W = x.shape
    buf = torch.full((N * H * W * MIS_CS + 8,), fill, dtype=x.dtype)
    v = torch.as_strided(buf, (N, H, W, C), (H * W * MIS_CS, W * MIS_CS, MIS_CS, 1), off)
    v.copy_(x.permute(0, 2, 3, 1))
    buf = buf.cuda()
    view = torch.as_strided(buf, (N, C, H, W), (H * W * MIS_CS, 1, W * MIS_CS, MIS_CS), off)
    assert (view.data_ptr() % 16 != 0) == (off * x.element_size() % 16 != 0)
    return buf, view


def gaps_untouched(buf, shape, off, fill=7.0):
    N, C, H, W = shape
    m = torch.ones_like(buf, dtype=torch.bool)
    torch.as_strided(m, (N, H, W, C), (H * W * MIS_CS, W * MIS_CS, MIS_CS, 1), off).fill_(False)
    return bool((buf[m] == fill).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def acc_want(dtype, prior, g, acc):
    """(reference, restatement) of a gradient stored over prior with accumulate=acc."""
    if not acc:
        return g, (R.bf16_round(g) if dtype == BF16 else None)
    return prior.double() + g, (R.bf16_accumulated([prior.double(), g]) if dtype == BF16 else None)


@pytest.mark.parametrize("acc", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("dtype,off", MIS)
def test_scalar_fallback_gate(dtype, off, acc):
    N, C, H, W = N2, 16, 5, 7
    dt = K.dcode(dtype)
    x, (ah, aw), up = gate_inputs(dtype, C, "ela2", H, W, N, True, 1500)
    prior = rnd(N, C, H, W, 1510, dtype)
    (xb, xv), (ub, uv), (ob, ov), (db, dv) = (mis(t, off) for t in (x, up, torch.zeros_like(x), prior))
    ahd, awd = dev(ah, False), dev(aw, False)
    dah, daw = torch.empty_like(ahd), torch.empty_like(awd)
    lib.adr_gate(dt, _p(xv), MIS_CS, _p(ahd), H * C, _p(awd), W * C, _p(ov), MIS_CS, N, H, W, C, K.stream())
    lib.adr_gate_bwd(dt, _p(xv), MIS_CS, _p(ahd), H * C, _p(awd), W * C, _p(uv), MIS_CS, _p(dv), MIS_CS, _p(dah), H * C,
                     _p(daw), W * C, N, H, W, C, acc, 0, K.stream())
    ro, rg = ref_gate_run(x, [ah, aw], up, "ela2")
    name = f"scalar gate acc={acc}"
    compare(dtype, f"{name} out", ov, ro[0], R.bf16_round(ro[0]))
    compare(dtype, f"{name} dx", dv, *acc_want(dtype, prior, rg[0], acc))
    compare(dtype, f"{name} dah", dah, rg[1], R.bf16_round(rg[1]))
    compare(dtype, f"{name} daw", daw, rg[2], R.bf16_round(rg[2]))
    assert gaps_untouched(ob, x.shape, off) and gaps_untouched(db, x.shape, off)


@pytest.mark.parametrize("acc", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("dtype,off", MIS)
def test_scalar_fallback_maxpool(dtype, off, acc):
    N, C, H, W, k = N2, 16, 5, 7, 5
    dt = K.dcode(dtype)
    x, up, prior = (rnd(N, C, H, W, 1520 + i, dtype) for i in range(3))
    (xb, xv), (ub, uv), (ob, ov), (db, dv) = (mis(t, off) for t in (x, up, torch.zeros_like(x), prior))
    arg = torch.empty(N * H * W * C, dtype=torch.uint8, device="cuda")
    lib.adr_maxpool(dt, _p(xv), MIS_CS, _p(ov), MIS_CS, _p(arg), N, H, W, C, k, K.stream())
    lib.adr_maxpool_bwd(dt, _p(uv), MIS_CS, _p(arg), _p(dv), MIS_CS, N, H, W, C, k, acc, K.stream())
    (ro,), (rg,) = R.run(lambda t: R.ref_maxpool(t, k), [x], [up])
    exact(f"scalar maxpool acc={acc} y", ov, ro)
    compare(dtype, f"scalar maxpool acc={acc} dx", dv, *acc_want(dtype, prior, rg, acc))
    assert gaps_untouched(ob, x.shape, off) and gaps_untouched(db, x.shape, off)


@pytest.mark.parametrize("acc", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("dtype,off", MIS)
def test_scalar_fallback_bilinear(dtype, off, acc):
    N, C, H, W, OH, OW = N2, 16, 5, 7, 8, 9
    dt = K.dcode(dtype)
    x, prior, up = rnd(N, C, H, W, 1530, dtype), rnd(N, C, H, W, 1531, dtype), rnd(N, C, OH, OW, 1532, dtype)
    (xb, xv), (ub, uv), (ob, ov), (db, dv) = (mis(t, off) for t in (x, up, torch.zeros_like(up), prior))
    lib.adr_bilinear(dt, _p(xv), MIS_CS, N, H, W, C, _p(ov), MIS_CS, OH, OW, K.stream())
    lib.adr_bilinear_bwd(dt, _p(uv), MIS_CS, N, H, W, C, _p(dv), MIS_CS, OH, OW, acc, K.stream())
    (ro,), (rg,) = R.run(lambda t: R.ref_bilinear(t, OH, OW), [x], [up])
    compare(dtype, f"scalar bilinear acc={acc} y", ov, ro, R.bf16_round(ro))
    compare(dtype, f"scalar bilinear acc={acc} dx", dv, *acc_want(dtype, prior, rg, acc))
    assert gaps_untouched(ob, up.shape, off) and gaps_untouched(db, x.shape, off)
