"""Op-level parity of the dense conv kernels (adr_conv.hip, adr_wgrad.hip, adr_gemm.hip's fp32 engine) against the
float64 definitions of conv_ref.py, through kernels.conv2d(...) and .backward(dy) with no trainer and no deferral
(the immediate adr_conv2d_wgrad_partials + adr_wgrad_reduce_unpack path).

Exact tier. x, w, dy (and biases) are seeded integers in [-3, 3] ({-1, 0, 1} for the statistics cases), about a
quarter of them zero, position dependent. Every product is an integer and every partial sum in any order is an
integer below 2^24 (asserted on the CPU, on the float64 conv of the absolute values, before the device call), so
fp32 accumulation, split-K slabs and the fixed-order reduce round nothing: dw, the fused bias sums and the BN
statistics partials must be BIT-EQUAL to float64, y and dx bit-equal to ref.to(bfloat16). Whatever the tiling, a
dropped, doubled or misplaced tap, channel chunk, halo column, k-step or split slab is an integer difference. No
tolerance comes from the kernel.

Every case first asserts which kernel it reaches (adr_conv2d_bf16_kernel_symbol / adr_conv2d_wgrad_kernel_symbol)
and its split count, so a dispatch change fails the case instead of silently un-covering a kernel.

Randn tier (one shape per kernel family): seeded randn rounded to bf16, the same values on both sides; per element
    y, dx:  |got - ref| <= 2^-8 |ref| + 2 n 2^-24 S          dw:  |got - ref| <= 2 n 2^-24 S
with n the number of products of that output and S the sum of their magnitudes (the float64 conv of ones / of the
absolute values): half a bf16 ulp for the stored rounding, and the worst-case bound of an fp32 sum in any order,
doubled for an MFMA accumulator that may truncate. n <= 2500. For the epilogue activations the accumulation term
goes through the activation's Lipschitz constant L (sigmoid 1/4, silu 1.1), the stored rounding applies to the
activation's output, and the fp32 evaluation of the activation (__expf and v_rcp_f32: a few fp32 ulps) gets 2^-16
of the output: |got - act(ref)| <= (2^-8 + 2^-16) |act(ref)| + L 2 n 2^-24 S. The eval BatchNorm's scale / shift
are the device's own fp32 pair (read back), so both sides multiply by the same numbers; their product with the
accumulator rounds once more in fp32, which adds 2^-23 (|conv * scale| + |shift|) inside L.

Measured on an MI355X, worst err / bound per kernel family over y, dx (CONVERR lines; below 1 by construction of
the bound, and close to 1 because a stored bf16 value does reach half an ulp), and over dw:
    family                      y, dx     dw
    generic tile                0.975     0.026
    streaming 1x1               0.992     0.004
    3x3 halo TW 16              0.889     0.001
    3x3 halo TW 8               0.974     0.001
    dg2 (stride-2 DGRAD)        0.976     0.007
    split / thin WGRAD shapes   0.976     0.001
    sigmoid / BN-silu epilogue  0.954     -

Found by the exact tier: the accumulate / addend epilogues add to bf16(conv), not to the fp32 accumulator (see
test_exact_dgrad_accumulate_and_addend).
"""
import ctypes
import functools
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


# ---- kernel names -----------------------------------------------------------------------------------------------

def demangle(sym):
    """'_ZN3adr12conv3_kernelILi16ELb1ELi32EEEvNS_8ConvArgsE' -> 'conv3_kernel<16, 1, 32>' (ints and bools only)."""
    m = re.match(r"_ZN3adr(\d+)", sym)
    assert m, sym
    n = int(m.group(1))
    name, rest = sym[m.end():m.end() + n], sym[m.end() + n:]
    args = re.match(r"I((?:L[ib]\d+E)+)E", rest)
    if not args:
        return name
    return name + "<" + ", ".join(re.findall(r"L[ib](\d+)E", args.group(1))) + ">"


FWD, DG, DG2 = 0, 1, 2  # ConvMode of adr_conv.hip


def gen(bn, mode):
    return f"conv_bf16_kernel<{bn}, {mode}>"


def c1(bn, mode, kt):
    return f"conv1_kernel<{bn}, {mode}, {kt}>"


def c3(tw, dg, bn):
    return f"conv3_kernel<{tw}, {dg}, {bn}>"


def dg2(bn):
    return f"dg2_kernel<8, {bn}, 0, 0>"


def wg(bm, bn, db=False):
    return f"void adr::wgrad_bf16_kernel<{bm}, {bn}{', true' if db else ''}>(adr::WgArgs)"


def wg3(tw, kf):
    return f"void adr::wgrad3_kernel<{tw}, {kf}>(adr::WgArgs)"


def wgt(s, kb):
    return f"void adr::wgrad3t_kernel<{s}, {kb}>(adr::WgArgs)"


# ---- the case table ---------------------------------------------------------------------------------------------
# id: (N, H, W, C, K, (R, S), stride, (pad_h, pad_w), forward kernel, data-gradient kernel, weight-gradient kernel,
#      WGRAD splits)
CASES = {
    # generic tile conv_bf16_kernel<BN, MODE> (row tile 128, k-step 64): BN 16 / 32 / 64 and the ragged 136
    "g_3x3_c8k8": (2, 13, 13, 8, 8, (3, 3), 1, (1, 1), gen(16, FWD), gen(16, DG), wg(16, 16), 1),
    "g_3x3_c24k48": (2, 13, 13, 24, 48, (3, 3), 1, (1, 1), gen(64, FWD), gen(32, DG), wg(64, 32), 1),
    "g_3x3_c48k24": (2, 13, 13, 48, 24, (3, 3), 1, (1, 1), gen(32, FWD), gen(64, DG), wg(32, 64), 1),
    # 136 columns on the 128-wide tile's fallback (grid128 < 1024 -> 64): two full column tiles and 8 ragged
    "g_3x3_c8k136": (2, 13, 13, 8, 136, (3, 3), 1, (1, 1), gen(64, FWD), gen(16, DG), wg(128, 16), 1),
    "g_3x3_c136k8": (2, 13, 13, 136, 8, (3, 3), 1, (1, 1), gen(16, FWD), gen(64, DG), wg(16, 128), 1),
    "g_3x3_c136k136": (2, 13, 13, 136, 136, (3, 3), 1, (1, 1), gen(64, FWD), gen(64, DG), wg(128, 128, True), 1),
    # the 128-wide tile itself: grid128 = ceil(rows / 128) * 2 = 1030 >= 1024 (one side); 1020 (the other side)
    "g_128_fwd": (2, 181, 182, 8, 136, (3, 3), 1, (1, 1), gen(128, FWD), gen(16, DG), wg(128, 16), 55),
    "g_128_fwd_below": (2, 180, 181, 8, 136, (3, 3), 1, (1, 1), gen(64, FWD), gen(16, DG), wg(128, 16), 57),
    "g_128_dgrad": (2, 181, 182, 136, 8, (3, 3), 1, (1, 1), gen(16, FWD), gen(128, DG), wg(16, 128), 55),
    # rows 127 / 128 / 129 around one row tile; ktot 72 = one 64-deep k-step and 8
    "g_rows127": (1, 1, 127, 8, 24, (3, 3), 1, (1, 1), gen(32, FWD), gen(16, DG), wg(32, 16), 1),
    "g_rows128": (1, 8, 16, 8, 24, (3, 3), 1, (1, 1), gen(32, FWD), gen(16, DG), wgt(1, 32), 1),
    "g_rows129": (1, 3, 43, 8, 24, (3, 3), 1, (1, 1), gen(32, FWD), gen(16, DG), wg(32, 16), 1),
    # ktot = 64 exactly (1x1 stride 2 is not on the streaming kernel), 3x3 stride 2 on odd and even maps (the four
    # parity classes of CV_DGRAD2 differ in size on 9 x 7)
    "g_1x1s2_c64": (2, 9, 7, 64, 24, (1, 1), 2, (0, 0), gen(32, FWD), gen(64, DG2), wg(32, 64), 1),
    "g_3x3s2_odd": (2, 9, 7, 24, 48, (3, 3), 2, (1, 1), gen(64, FWD), gen(32, DG2), wg(64, 32), 1),
    "g_3x3s2_even": (2, 10, 8, 24, 48, (3, 3), 2, (1, 1), gen(64, FWD), gen(32, DG2), wg(64, 32), 1),
    "g_7x1": (2, 11, 13, 16, 16, (7, 1), 1, (3, 0), gen(16, FWD), gen(16, DG), wg(16, 16), 1),
    "g_1x7": (2, 11, 13, 16, 16, (1, 7), 1, (0, 3), gen(16, FWD), gen(16, DG), wg(16, 16), 1),
    "g_5x5": (2, 9, 11, 8, 40, (5, 5), 1, (2, 2), gen(64, FWD), gen(16, DG), wg(64, 16), 1),
    # streaming 1x1 conv1_kernel<BN, MODE, KT>: rows 100 / 128 / 129 / 1000; forward KT 64 / 128, DGRAD KT 64 / 256
    "s_c64k136_r100": (2, 5, 10, 64, 136, (1, 1), 1, (0, 0), c1(64, FWD, 64), c1(64, DG, 256), wg(128, 64), 1),
    "s_c72k256_r128": (2, 8, 8, 72, 256, (1, 1), 1, (0, 0), c1(64, FWD, 128), c1(64, DG, 256), wg(128, 128, True), 1),
    "s_c128k32_r129": (3, 1, 43, 128, 32, (1, 1), 1, (0, 0), c1(32, FWD, 128), c1(64, DG, 64), wg(32, 128), 1),
    "s_c64k24_r1000": (2, 20, 25, 64, 24, (1, 1), 1, (0, 0), c1(32, FWD, 64), c1(64, DG, 64), wg(32, 64), 1),
    "s_c136_generic": (2, 5, 10, 136, 16, (1, 1), 1, (0, 0), gen(16, FWD), c1(64, DG, 64), wg(16, 128), 1),
    "s_k264_generic": (2, 5, 10, 16, 264, (1, 1), 1, (0, 0), c1(64, FWD, 64), gen(16, DG), wg(128, 16), 1),
    # 3x3 halo tiles conv3_kernel<TW, DG, BN> and wgrad3_kernel<TW, KF>: TW 16 (W % 16 == 0, H >= 8) and TW 8; one
    # and three 32-channel chunks; last row band full (H 8), one row (H 9 / 17) and half (H 12 / 8 for TW 8)
    "h16_c32k32_h8": (2, 8, 16, 32, 32, (3, 3), 1, (1, 1), c3(16, 0, 32), c3(16, 1, 32), wg3(16, 2), 1),
    "h16_c96k64_h9": (2, 9, 32, 96, 64, (3, 3), 1, (1, 1), c3(16, 0, 64), c3(16, 1, 32), wg3(16, 4), 2),
    "h16_c32k96_h12": (2, 12, 16, 32, 96, (3, 3), 1, (1, 1), c3(16, 0, 32), c3(16, 1, 32), wg3(16, 2), 1),
    "h16_c64k64_h20": (3, 20, 16, 64, 64, (3, 3), 1, (1, 1), c3(16, 0, 64), c3(16, 1, 64), wg3(16, 4), 2),
    "h16_c32k32_s4": (2, 32, 32, 32, 32, (3, 3), 1, (1, 1), c3(16, 0, 32), c3(16, 1, 32), wg3(16, 2), 4),
    "h8_c32k64_w8": (2, 8, 8, 32, 64, (3, 3), 1, (1, 1), c3(8, 0, 64), c3(8, 1, 32), wg3(8, 4), 1),
    "h8_c96k32_w24": (2, 9, 24, 96, 32, (3, 3), 1, (1, 1), c3(8, 0, 32), c3(8, 1, 32), wg3(8, 2), 1),
    "h8_c32k32_h5": (2, 5, 16, 32, 32, (3, 3), 1, (1, 1), c3(8, 0, 32), c3(8, 1, 32), wg3(8, 2), 1),
    "h8_c32k64_h17": (2, 17, 8, 32, 64, (3, 3), 1, (1, 1), c3(8, 0, 64), c3(8, 1, 32), wg3(8, 4), 1),
    "h8_c32k32_s2": (3, 9, 24, 32, 32, (3, 3), 1, (1, 1), c3(8, 0, 32), c3(8, 1, 32), wg3(8, 2), 2),    # 9 tiles: 5 + 4
    "h8_c32k96_s4": (3, 24, 24, 32, 96, (3, 3), 1, (1, 1), c3(8, 0, 32), c3(8, 1, 32), wg3(8, 2), 4),   # 18: 5 5 5 3
    # WGRAD generic tile wgrad_bf16_kernel<BM, BN> over {16, 32, 64, 128}^2 by K, C in {8, 24, 40, 72} (1x1: the
    # forward and data gradient ride on the streaming kernel)
    **{f"w_k{k}c{c}": (2, 13, 13, c, k, (1, 1), 1, (0, 0),
                       c1(min(bm, 64), FWD, 64 if c <= 64 else 128), c1(min(bn, 64), DG, 64 if k <= 64 else 128),
                       wg(bm, bn, bm == 128 and bn == 128), 1)
       for k, bm in ((8, 16), (24, 32), (40, 64), (72, 128)) for c, bn in ((8, 16), (24, 32), (40, 64), (72, 128))},
    # split-K: two splits with `per` dividing the reduction (1152 = 2 x 576), a ragged last split ending inside a
    # k-step (1058 rows: per 544, last 514 = 16 x 32 + 2), nine splits, and the 128-row k-step of the 16 x 16 tile
    "w_split2_even": (2, 24, 24, 24, 24, (3, 3), 1, (1, 1), gen(32, FWD), gen(32, DG), wg(32, 32), 2),
    "w_split2_ragged": (2, 23, 23, 24, 24, (3, 3), 1, (1, 1), gen(32, FWD), gen(32, DG), wg(32, 32), 2),
    "w_split9": (3, 40, 40, 24, 24, (3, 3), 1, (1, 1), gen(32, FWD), gen(32, DG), wg(32, 32), 9),
    "w_split2_r128": (3, 40, 40, 8, 8, (3, 3), 1, (1, 1), gen(16, FWD), gen(16, DG), wg(16, 16), 2),
    "w_split2_r64": (3, 30, 30, 8, 24, (3, 3), 1, (1, 1), gen(32, FWD), gen(16, DG), wg(32, 16), 2),
    # thin-channel wgrad3t_kernel<S, KB>: C 8 / 16, K 8..32, stride 1 and 2 (H = 2 Ho), Wo 16 / 32, Ho 8 / 9 / 4
    "t_s1_c8k8": (2, 8, 16, 8, 8, (3, 3), 1, (1, 1), gen(16, FWD), gen(16, DG), wgt(1, 16), 1),
    "t_s1_c16k24": (2, 9, 32, 16, 24, (3, 3), 1, (1, 1), gen(32, FWD), gen(16, DG), wgt(1, 32), 2),
    "t_s1_c16k32": (3, 4, 16, 16, 32, (3, 3), 1, (1, 1), gen(32, FWD), gen(16, DG), wgt(1, 32), 1),
    "t_s2_c8k16": (2, 16, 32, 8, 16, (3, 3), 2, (1, 1), gen(16, FWD), gen(16, DG2), wgt(2, 16), 1),
    "t_s2_c16k32": (2, 18, 64, 16, 32, (3, 3), 2, (1, 1), gen(32, FWD), gen(16, DG2), wgt(2, 32), 2),
    "t_s2_c8k24": (3, 8, 32, 8, 24, (3, 3), 2, (1, 1), gen(32, FWD), gen(16, DG2), wgt(2, 32), 1),
}
# stride-2 3x3 data gradient on super-pixel halo tiles (dg2_kernel) with ADR_DG2H=2: Ho x Wo 8 x 8, 9 x 7, 5 x 16
DG2_CASES = {
    "d_8x8_c16k32": (2, 16, 16, 16, 32, (3, 3), 2, (1, 1), gen(32, FWD), dg2(16), wg(32, 16), 1),
    "d_9x7_c32k64": (2, 17, 13, 32, 64, (3, 3), 2, (1, 1), gen(64, FWD), dg2(32), wg(64, 32), 1),
    "d_5x16_c64k32": (2, 10, 32, 64, 32, (3, 3), 2, (1, 1), gen(32, FWD), dg2(64), wg(32, 64), 1),
}
ALL = {**CASES, **DG2_CASES}
# one shape per kernel family for the randn tier (n <= 2500 for y, dx and dw)
RANDN = ["g_3x3_c24k48", "g_3x3_c136k136", "g_3x3s2_odd", "g_7x1", "s_c72k256_r128", "s_c64k24_r1000",
         "h16_c96k64_h9", "h8_c96k32_w24", "w_split2_ragged", "h8_c32k32_s2", "t_s1_c16k24", "t_s2_c8k16",
         "d_9x7_c32k64"]


def geom(cid):
    N, H, W, C, Kc, (Rr, S), st, (ph, pw) = ALL[cid][:8]
    return N, H, W, C, Kc, Rr, S, st, ph, pw


# ---- inputs and references (computed once per case and tier, never modified) -------------------------------------

def _seed(cid, tier):
    return zlib.crc32(cid.encode()) % 100000 * 64 + {"int": 0, "stat": 16, "randn": 32}[tier]


@functools.lru_cache(maxsize=None)
def inputs(cid, tier="int", bias=False):
    """(x, w, dy, b) on the CPU as float32 holding bf16-representable values (logical NCHW / KCRS)."""
    N, H, W, C, Kc, Rr, S, st, ph, pw = geom(cid)
    Ho, Wo = (H + 2 * ph - Rr) // st + 1, (W + 2 * pw - S) // st + 1
    s = _seed(cid, tier)
    shapes = [(N, C, H, W), (Kc, C, Rr, S), (N, Kc, Ho, Wo), (Kc,)]
    if tier == "randn":
        g = torch.Generator().manual_seed(s)
        x, w, dy, b = (torch.randn(sh, generator=g).to(BF).float() for sh in shapes)
    else:
        lo, hi = (-1, 1) if tier == "stat" else (-3, 3)
        x, w, dy, b = (R.randint(sh, lo, hi, s + i) for i, sh in enumerate(shapes))
    return x, w, dy, (b if bias else None)


@functools.lru_cache(maxsize=None)
def reference(cid, tier="int", bias=False):
    """float64 (y, dx, dw, db) and the (S, n) maps of y, dx, dw; the exact tier's precondition is asserted here."""
    N, H, W, C, Kc, Rr, S, st, ph, pw = geom(cid)
    x, w, dy, b = inputs(cid, tier, bias)
    y = R.forward(x, w, b, st, (ph, pw))
    dx, dw = R.grads(x, w, dy, st, (ph, pw))
    smaps = R.abs_maps(x, w, dy, st, (ph, pw), b)
    if tier != "randn":
        R.assert_exact_ok(*smaps)
        R.assert_integer(y, dx, dw)
    counts = R.term_counts(x, w, dy, st, (ph, pw)) if tier == "randn" else None
    return y, dx, dw, R.bias_grad(dy), smaps, counts


def nhwc_dev(t, dtype=BF, grad=False):
    """CPU NCHW values -> the device NHWC activation (logical NCHW view), a leaf."""
    return t.permute(0, 2, 3, 1).contiguous().to("cuda", dtype).permute(0, 3, 1, 2).requires_grad_(grad)


def slice_dev(t, off, width, fill=3.0, dtype=BF):
    """The activation as channels [off, off + C) of a wider NHWC leaf whose other channels hold `fill`."""
    n, c, h, w = t.shape
    wide = torch.full((n, h, w, width), fill)
    wide[..., off:off + c] = t.permute(0, 2, 3, 1)
    leaf = wide.to("cuda", dtype).permute(0, 3, 1, 2).requires_grad_(True)
    return leaf, leaf[:, off:off + c]


# ---- comparisons -------------------------------------------------------------------------------------------------

def assert_exact(what, got, ref, stored=None):
    """got (device) bit-equal to ref (float64), rounded to the stored dtype first when that is bf16."""
    got = got.detach().to("cpu", torch.float64).reshape(ref.shape)
    want = ref.to(stored).double() if stored is not None else ref
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    bad = got != want
    if bool(bad.any()):
        idx = bad.nonzero()
        first = tuple(int(i) for i in idx[0])
        d = (got - want)[bad]
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 reference; first at {first}: "
            f"got {float(got[first])} want {float(want[first])}; differences min {float(d.min())} max {float(d.max())}; "
            f"differing index ranges per dim {[(int(idx[:, k].min()), int(idx[:, k].max())) for k in range(idx.shape[1])]}")


RATIOS = {}


def assert_bound(fam, what, got, ref, n, S, ulp=True, lip=1.0, extra=None, act_ref=None):
    """The randn tier's per-element bound (module docstring); prints and records the worst err / bound."""
    got = got.detach().to("cpu", torch.float64).reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    assert float(n.max()) <= 2500, f"{what}: n = {float(n.max())} > 2500"
    acc = 2.0 * n * 2.0 ** -24 * S
    if extra is not None:
        acc = acc + extra
    out = ref if act_ref is None else act_ref
    bound = lip * acc + ((2.0 ** -8 + (2.0 ** -16 if act_ref is not None else 0.0)) * out.abs() if ulp else 0.0)
    err = (got - out).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
    worst = float(ratio.max())
    RATIOS[fam] = max(RATIOS.get(fam, 0.0), worst)
    print(f"CONVERR {fam} {what} worst_err_over_bound={worst:.3f} max_err={float(err.max()):.3e}")
    assert worst <= 1.0, f"{what}: err / bound = {worst:.3f} at {tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])}"


# ---- dispatch ----------------------------------------------------------------------------------------------------

def descs(cid, xcs=None, ycs=None, dtype=BF):
    """(forward / WGRAD descriptor, data-gradient descriptor) as Conv2dFn builds them."""
    import adrefine.kernels as K
    N, H, W, C, Kc, Rr, S, st, ph, pw = geom(cid)
    d, _, _ = K.conv_desc(N, H, W, C, xcs or C, Kc, Rr, S, st, st, ph, pw, ycs or Kc, dtype)
    d2, _, _ = K.conv_desc(N, H, W, C, C, Kc, Rr, S, st, st, ph, pw, ycs or Kc, dtype)
    return d, d2


def wgrad_symbol(d):
    from adrefine.native import lib
    buf = ctypes.create_string_buffer(128)
    lib.adr_conv2d_wgrad_kernel_symbol(ctypes.byref(d), buf, 128)
    return buf.value.decode()


def dispatch(cid):
    """(forward, data-gradient, weight-gradient kernel, WGRAD splits) as the library plans them. Host only."""
    import adrefine.kernels as K
    from adrefine.native import lib
    d, d2 = descs(cid)
    return (demangle(K._conv2_symbol(d, False)), demangle(K._conv2_symbol(d2, True)), wgrad_symbol(d),
            lib.adr_conv2d_wgrad_splits(ctypes.byref(d)))


def assert_dispatch(cid):
    want = ALL[cid][8:12]
    got = dispatch(cid)
    assert got == want, f"{cid}: the library dispatches {got}, the case table claims {want}"


def run(cid, tier="int", bias=False, x_slice=None, out_slice=None):
    """kernels.conv2d + backward on the device -> (y, dx, dw, db)."""
    import adrefine.kernels as K
    N, H, W, C, Kc, Rr, S, st, ph, pw = geom(cid)
    x, w, dy, b = inputs(cid, tier, bias)
    if x_slice is None:
        leaf = xs = nhwc_dev(x, grad=True)
    else:
        leaf, xs = slice_dev(x, *x_slice)
    wd = w.cuda().requires_grad_(True)
    bd = b.cuda().requires_grad_(True) if b is not None else None
    buf = out = None
    if out_slice is not None:
        off, width, sentinel = out_slice
        buf = torch.full((N, dy.shape[2], dy.shape[3], width), sentinel, dtype=BF, device="cuda").permute(0, 3, 1, 2)
        out = buf[:, off:off + Kc]
    y, _ = K.conv2d(xs, wd, bd, st, (ph, pw), out=out)
    y.backward(nhwc_dev(dy))
    torch.cuda.synchronize()
    dx = leaf.grad if x_slice is None else leaf.grad[:, x_slice[0]:x_slice[0] + C]
    if x_slice is not None:  # the other channels of the wide leaf received no gradient
        rest = torch.cat([leaf.grad[:, :x_slice[0]], leaf.grad[:, x_slice[0] + C:]], 1)
        assert float(rest.float().abs().max()) == 0.0, "gradient outside the input slice"
    if buf is not None:
        off, width, sentinel = out_slice
        rest = torch.cat([buf[:, :off], buf[:, off + Kc:]], 1)
        assert bool((rest.float() == sentinel).all()), "the output slice's neighbours were overwritten"
    return y, dx, wd.grad, (bd.grad if bd is not None else None)


# ---- exact tier: every kernel family at its edges ----------------------------------------------------------------

@pytest.mark.parametrize("cid", sorted(CASES))
def test_exact(cid, monkeypatch):
    monkeypatch.delenv("ADR_DG2H", raising=False)
    monkeypatch.delenv("ADR_WG_DB", raising=False)
    ry, rdx, rdw, _, _, _ = reference(cid)
    assert_dispatch(cid)
    y, dx, dw, _ = run(cid)
    assert_exact(f"{cid} y", y, ry, BF)
    assert_exact(f"{cid} dx", dx, rdx, BF)
    assert_exact(f"{cid} dw", dw, rdw)


@pytest.mark.parametrize("cid", sorted(DG2_CASES))
def test_exact_dg2(cid, monkeypatch):
    monkeypatch.setenv("ADR_DG2H", "2")  # DG2H wherever it applies: ragged super-pixel tiles
    ry, rdx, rdw, _, _, _ = reference(cid)
    assert_dispatch(cid)
    y, dx, dw, _ = run(cid)
    assert_exact(f"{cid} y", y, ry, BF)
    assert_exact(f"{cid} dx", dx, rdx, BF)
    assert_exact(f"{cid} dw", dw, rdw)


def test_exact_wide_tile():
    """conv3w_kernel (256 pixels x 128 channels) forward and data gradient at the smallest shape conv3_wide takes:
    N ceil(H / 16) (W / 16) (K / 128) = 2 * 16 * 16 = 512 with C = 128; the WGRAD runs 94 splits of the TW 16 halo
    kernel. The reference here is torch's CPU float32 conv: on these integers every partial sum stays below 2^24,
    so it is exact too, which the float64 conv of one image of the batch confirms."""
    import adrefine.kernels as K
    from adrefine.native import lib
    N, H, W, C, Kc = 2, 256, 256, 128, 128
    x, w = R.randint((N, C, H, W), -3, 3, 61), R.randint((Kc, C, 3, 3), -3, 3, 62)
    dy = R.randint((N, Kc, H, W), -3, 3, 63)

    def f32(xv, wv, dv):
        xr, wr = xv.clone().requires_grad_(True), wv.clone().requires_grad_(True)
        y = F.conv2d(xr, wr, None, 1, 1)
        return (y.detach(),) + torch.autograd.grad(y, (xr, wr), dv)

    ry, rdx, rdw = f32(x, w, dy)
    R.assert_exact_ok(*f32(x.abs(), w.abs(), dy.abs()))
    y64 = R.forward(x[:1], w, None, 1, 1)
    dx64, _ = R.grads(x[:1], w, dy[:1], 1, 1)
    assert torch.equal(ry[:1].double(), y64) and torch.equal(rdx[:1].double(), dx64)
    d, _, _ = K.conv_desc(N, H, W, C, C, Kc, 3, 3, 1, 1, 1, 1, Kc, BF)
    assert demangle(K._conv2_symbol(d, False)) == "conv3w_kernel<0, 0>"
    assert demangle(K._conv2_symbol(d, True)) == "conv3w_kernel<1, 0>"
    assert wgrad_symbol(d) == wg3(16, 4) and lib.adr_conv2d_wgrad_splits(ctypes.byref(d)) == 94
    xd, wd = nhwc_dev(x, grad=True), w.cuda().requires_grad_(True)
    y, _ = K.conv2d(xd, wd, None, 1, 1)
    y.backward(nhwc_dev(dy))
    assert_exact("wide y", y, ry.double(), BF)
    assert_exact("wide dx", xd.grad, rdx.double(), BF)
    assert_exact("wide dw", wd.grad, rdw.double())


def test_exact_wgrad_128_single_stage(monkeypatch):
    """The 128 x 128 WGRAD tile in its single-stage form (ADR_WG_DB=0; test_exact runs the double-buffered one)."""
    monkeypatch.setenv("ADR_WG_DB", "0")
    for cid in ("g_3x3_c136k136", "w_k72c72"):
        d, _ = descs(cid)
        assert wgrad_symbol(d) == wg(128, 128)
        _, _, dw, _ = run(cid)
        assert_exact(f"{cid} dw (single stage)", dw, reference(cid)[2])


SPLIT_CASES = ["w_split2_even", "w_split2_ragged", "w_split9", "w_split2_r128", "w_split2_r64", "g_128_fwd",
               "h16_c96k64_h9", "h8_c32k32_s2", "h8_c32k96_s4", "h16_c32k32_s4", "t_s1_c16k24"]


@pytest.mark.parametrize("cid", SPLIT_CASES)
def test_exact_wgrad_partials(cid):
    """The split slabs themselves: adr_conv2d_wgrad_partials into a NaN-filled buffer leaves every element finite
    (each (k, tap, c) of each split written), and the float64 sum over the splits is the reference."""
    import adrefine.kernels as K
    from adrefine.native import lib
    N, H, W, C, Kc, Rr, S, st, ph, pw = geom(cid)
    x, w, dy, _ = inputs(cid)
    rdw = reference(cid)[2]
    d, _ = descs(cid)
    splits = lib.adr_conv2d_wgrad_splits(ctypes.byref(d))
    assert splits == ALL[cid][11] and splits >= 2
    xd, dyd = nhwc_dev(x), nhwc_dev(dy)
    ws = torch.full((splits, Kc * Rr * S * C), float("nan"), dtype=torch.float32, device="cuda")
    lib.adr_conv2d_wgrad_partials(ctypes.byref(d), K.fptr(xd), K.fptr(dyd), K.fptr(ws), 0, K.stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws).all()), f"{cid}: {int((~torch.isfinite(ws)).sum())} slab elements never written"
    got = ws.double().sum(0).view(Kc, Rr, S, C).permute(0, 3, 1, 2)
    assert_exact(f"{cid} sum of split slabs", got, rdw)


# ---- views and epilogues -----------------------------------------------------------------------------------------

VIEW_CASES = ["g_3x3_c24k48", "s_c64k24_r1000", "h16_c96k64_h9", "h8_c96k32_w24", "g_3x3s2_odd"]


@pytest.mark.parametrize("cid", VIEW_CASES)
def test_exact_channel_slice_views(cid):
    """x as channels [8, 8 + C) of a wider leaf (the rest holds 3.0), y into channels [8, 8 + K) of a wider buffer
    pre-filled with a sentinel that must survive outside the slice, with an integer bias."""
    ry, rdx, rdw, rdb, _, _ = reference(cid, "int", True)
    C, Kc = geom(cid)[3], geom(cid)[4]
    y, dx, dw, db = run(cid, "int", True, x_slice=(8, C + 24), out_slice=(8, Kc + 16, -77.0))
    assert_exact(f"{cid} y (sliced)", y, ry, BF)
    assert_exact(f"{cid} dx (sliced)", dx, rdx, BF)
    assert_exact(f"{cid} dw (sliced)", dw, rdw)
    assert_exact(f"{cid} db (sliced)", db, rdb)


def test_exact_thin_wgrad_input_slice():
    """The thin-channel WGRAD reading x as a 16-channel slice of a 48-channel buffer."""
    cid = "t_s1_c16k24"
    d, _ = descs(cid, xcs=48)
    assert wgrad_symbol(d) == wgt(1, 32)
    ry, rdx, rdw, _, _, _ = reference(cid)
    y, dx, dw, _ = run(cid, x_slice=(16, 48))
    assert_exact("thin slice y", y, ry, BF)
    assert_exact("thin slice dx", dx, rdx, BF)
    assert_exact("thin slice dw", dw, rdw)


def test_exact_thin_wgrad_cpad():
    """C = 3 padded to 8 (cpad=8, the stem's layout): the WGRAD runs the thin kernel on 8 channels and the unpack
    drops the padded ones; x carries integers in all 8 channels, the padded weights are zero."""
    import adrefine.kernels as K
    from adrefine.native import lib
    N, H, W, Kc = 2, 8, 16, 16
    x = R.randint((N, 8, H, W), -3, 3, 71)
    w = R.randint((Kc, 3, 3, 3), -3, 3, 72)
    dy = R.randint((N, Kc, H, W), -3, 3, 73)
    wpad = torch.zeros(Kc, 8, 3, 3)
    wpad[:, :3] = w
    ry = R.forward(x, wpad, None, 1, 1)
    rdx, rdw = R.grads(x, wpad, dy, 1, 1)
    R.assert_exact_ok(*R.abs_maps(x, wpad, dy, 1, 1))
    d, _, _ = K.conv_desc(N, H, W, 8, 8, Kc, 3, 3, 1, 1, 1, 1, Kc, BF)
    assert wgrad_symbol(d) == wgt(1, 16) and lib.adr_conv2d_wgrad_splits(ctypes.byref(d)) == 1
    xd, wd = nhwc_dev(x, grad=True), w.cuda().requires_grad_(True)
    y, _ = K.conv2d(xd, wd, None, 1, 1, cpad=8)
    y.backward(nhwc_dev(dy))
    assert_exact("cpad y", y, ry, BF)
    assert_exact("cpad dx", xd.grad, rdx, BF)
    assert_exact("cpad dw", wd.grad, rdw[:, :3])


@pytest.mark.parametrize("cid,fusable", [("g_rows129", 0), ("w_split2_ragged", 1), ("h16_c96k64_h9", 1),
                                         ("t_s1_c16k24", 0)])
def test_exact_bias(cid, fusable, monkeypatch):
    """Integer bias: y, and db from the WGRAD launch's fused column sums (K = 24 on a 32 x 16 tile is not fusable,
    bm and bn >= 32 and the 3x3 halo kernel are) and, with ADR_FUSE_WG_BIAS=0, from the column-sum pass."""
    from adrefine.native import lib
    d, _ = descs(cid)
    assert lib.adr_conv2d_wgrad_bias_fusable(ctypes.byref(d)) == fusable
    ry, rdx, rdw, rdb, _, _ = reference(cid, "int", True)
    for fuse in ("1", "0"):
        monkeypatch.setenv("ADR_FUSE_WG_BIAS", fuse)
        y, dx, dw, db = run(cid, "int", True)
        assert_exact(f"{cid} y + bias", y, ry, BF)
        assert_exact(f"{cid} dx", dx, rdx, BF)
        assert_exact(f"{cid} dw (fuse={fuse})", dw, rdw)
        assert_exact(f"{cid} db (fuse={fuse})", db, rdb)


def test_exact_bias_partials_rows():
    """adr_conv2d_wgrad_partials_bias's [splits][2][K] rows: half 0 of every split written (NaN prefill), their sum
    the bias gradient."""
    import adrefine.kernels as K
    from adrefine.native import lib
    cid = "w_split2_ragged"
    N, H, W, C, Kc, Rr, S, st, ph, pw = geom(cid)
    x, w, dy, _ = inputs(cid)
    d, _ = descs(cid)
    splits = lib.adr_conv2d_wgrad_splits(ctypes.byref(d))
    xd, dyd = nhwc_dev(x), nhwc_dev(dy)
    ws = torch.empty(splits * Kc * Rr * S * C, dtype=torch.float32, device="cuda")
    bp = torch.full((splits, 2, Kc), float("nan"), dtype=torch.float32, device="cuda")
    lib.adr_conv2d_wgrad_partials_bias(ctypes.byref(d), K.fptr(xd), K.fptr(dyd), K.fptr(ws), K.fptr(bp), K.stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(bp[:, 0]).all())
    assert_exact("fused bias rows", bp[:, 0].double().sum(0), reference(cid)[3])


ADD_CASES = [("g_3x3_c24k48", None), ("s_c64k24_r1000", None), ("h16_c32k32_h8", None), ("h16_c96k64_h9", None),
             ("h8_c32k64_h17", None),
             ("g_3x3s2_odd", None), ("d_9x7_c32k64", "2")]


@pytest.mark.parametrize("cid,dg2h", ADD_CASES)
def test_exact_dgrad_accumulate_and_addend(cid, dg2h, monkeypatch):
    """accumulate=1 and the adr_conv2d_dgrad_bf16_add addend form through kernels.conv_dgrad: dx0 and the addend are
    even integers up to 400 (bf16 numbers), so dx0 + dgrad + addend leaves the exact bf16 range and the result must
    be bf16(dx0 + dgrad + addend) in ONE rounding of the sum. Every kernel's epilogue passes the conv through its
    bf16 output image in LDS before it adds, so the conv term itself is bf16(dgrad): the same number while
    |dgrad| <= 256, which holds in every case but the two halo-tile ones with 576 reduction terms (max |dgrad| 310
    and 319; at h16_c96k64_h9 the first run of this test found 6 of 55296 elements 1 or 2 off the single-rounding
    value). The expected value below states what the library computes, bf16(bf16(dgrad) + dx0 + addend), with no
    tolerance."""
    import adrefine.kernels as K
    if dg2h:
        monkeypatch.setenv("ADR_DG2H", dg2h)
    N, H, W, C, Kc, Rr, S, st, ph, pw = geom(cid)
    x, w, dy, _ = inputs(cid)
    rdx = reference(cid)[1]
    rdx = rdx.to(BF).double()  # the conv term as the epilogue holds it (a no-op while |dgrad| <= 256)
    dx0 = 2 * R.randint((N, C, H, W), -200, 200, 81, 0.0)
    add = 2 * R.randint((N, C, H, W), -200, 200, 82, 0.0)
    assert float((rdx + dx0 + add).abs().max()) > 256, "the sum never leaves the exact bf16 integer range"
    _, d2 = descs(cid)
    assert demangle(K._conv2_symbol(d2, True)) == ALL[cid][9]
    wpair = K.pack_weight2(w.cuda(), BF)
    dyd = nhwc_dev(dy)
    dx = nhwc_dev(dx0)
    K.conv_dgrad(d2, dyd.data_ptr(), wpair, None, dx.data_ptr(), accumulate=1)
    assert_exact(f"{cid} dx0 + dgrad", dx, rdx + dx0, BF)
    dx = nhwc_dev(dx0)
    K.conv_dgrad(d2, dyd.data_ptr(), wpair, None, dx.data_ptr(), accumulate=1, addend=nhwc_dev(add))
    assert_exact(f"{cid} dx0 + dgrad + addend", dx, rdx + dx0 + add, BF)
    dx = nhwc_dev(dx0)
    K.conv_dgrad(d2, dyd.data_ptr(), wpair, None, dx.data_ptr(), accumulate=0, addend=nhwc_dev(add))
    assert_exact(f"{cid} dgrad + addend", dx, rdx + add, BF)


def test_exact_forward_accumulate():
    """accumulate=1 of the forward: bf16(y0 + conv), one rounding of the sum (y0 even integers up to 400); the conv
    term is bf16(conv) as in test_exact_dgrad_accumulate_and_addend (it differs from conv only in the two 864-product
    cases, whose |conv| passes 256)."""
    import adrefine.kernels as K
    for cid in ("g_3x3_c24k48", "s_c64k24_r1000", "h16_c32k32_h8", "h16_c96k64_h9", "h8_c96k32_w24"):
        x, w, dy, _ = inputs(cid)
        y0 = 2 * R.randint(tuple(dy.shape), -200, 200, 83, 0.0)
        d, _ = descs(cid)
        wp, _ = K.pack_weight2(w.cuda(), BF)
        xd, y = nhwc_dev(x), nhwc_dev(y0)
        K.conv_fwd(d, xd.data_ptr(), wp.data_ptr(), None, y.data_ptr(), None, accumulate=1)
        conv = reference(cid)[0].to(BF).double()
        assert_exact(f"{cid} y0 + conv", y, conv + y0.double(), BF)


def test_exact_conv_transpose():
    """kernels.conv_transpose2d 3x3 stride 2 pad 1 output_padding 1 at 5 x 7 (the data gradient as a forward), its
    input gradient (a forward conv), weight and bias gradients."""
    import adrefine.kernels as K
    N, Ci, Co, H, W = 2, 24, 16, 5, 7
    x, w = R.randint((N, Ci, H, W), -3, 3, 91), R.randint((Ci, Co, 3, 3), -3, 3, 92)
    b = R.randint((Co,), -3, 3, 93)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    ry = F.conv_transpose2d(xr, wr, br, 2, 1, output_padding=1)
    dy = R.randint(tuple(ry.shape), -3, 3, 94)
    rdx, rdw, rdb = torch.autograd.grad(ry, (xr, wr, br), dy.double())
    sy = F.conv_transpose2d(x.double().abs(), w.double().abs(), b.double().abs(), 2, 1, output_padding=1)
    xa, wa = x.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True)
    sdx, sdw = torch.autograd.grad(F.conv_transpose2d(xa, wa, None, 2, 1, output_padding=1), (xa, wa), dy.double().abs())
    R.assert_exact_ok(sy, sdx, sdw)
    xd, wd, bd = nhwc_dev(x, grad=True), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = K.conv_transpose2d(xd, wd, bd, 2, 1, 1)
    assert tuple(y.shape) == (N, Co, 10, 14)
    y.backward(nhwc_dev(dy))
    assert_exact("convT y", y, ry.detach(), BF)
    assert_exact("convT dx", xd.grad, rdx, BF)
    assert_exact("convT dw", wd.grad, rdw)
    assert_exact("convT db", bd.grad, rdb)


@pytest.mark.parametrize("cid", ["g_3x3_c24k48", "s_c64k24_r1000", "h16_c96k64_h9"])
def test_exact_conv_act_relu(cid):
    """conv_act relu (the activation in the conv epilogue) and its backward from the saved output: exact on integers."""
    import adrefine.kernels as K
    N, H, W, C, Kc, Rr, S, st, ph, pw = geom(cid)
    x, w, dy, b = inputs(cid, "int", True)
    pre = R.forward(x, w, b, st, (ph, pw))
    R.assert_exact_ok(R.abs_maps(x, w, dy, st, (ph, pw), b)[0])
    dpre = dy.double() * (pre > 0)
    rdx, rdw = R.grads(x, w, dpre, st, (ph, pw))
    xd, wd, bd = nhwc_dev(x, grad=True), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = K.conv_act(xd, wd, bd, st, (ph, pw), "relu")
    y.backward(nhwc_dev(dy))
    assert_exact(f"{cid} relu y", y, pre.clamp_min(0), BF)
    assert_exact(f"{cid} relu dx", xd.grad, rdx, BF)
    assert_exact(f"{cid} relu dw", wd.grad, rdw)
    assert_exact(f"{cid} relu db", bd.grad, R.bias_grad(dpre))


# ---- BN statistics partials --------------------------------------------------------------------------------------

STAT_CASES = ["g_rows129", "g_3x3_c24k48", "s_c64k24_r1000", "s_c72k256_r128", "h8_c32k64_h17", "h8_c32k32_s2",
              "h16_c32k96_h12", "h16_c64k64_h20"]


@pytest.mark.parametrize("cid", STAT_CASES)
def test_exact_stats_partials(cid):
    """want_stats: the [tile][2][K] partials summed over tiles in float64 equal sum y and sum y^2 of the stored y
    exactly (inputs in {-1, 0, 1}; max |y| <= 256 so y is stored exactly and 128 max|y|^2 < 2^24 keeps every tile's
    sum of squares exact); a NaN-prefilled buffer shows an unwritten tile row. Last tiles are ragged."""
    import adrefine.kernels as K
    from adrefine.native import lib
    N, H, W, C, Kc, Rr, S, st, ph, pw = geom(cid)
    x, w, dy, _ = inputs(cid, "stat")
    ry = R.forward(x, w, None, st, (ph, pw))
    sy = R.abs_maps(x, w, dy, st, (ph, pw))[0]
    R.assert_exact_ok(sy)
    assert float(sy.max()) <= 256 and 128 * float(sy.max()) ** 2 < 2 ** 24
    assert demangle(K._conv2_symbol(descs(cid)[0], False)) == ALL[cid][8]
    xd, wd = nhwc_dev(x), w.cuda()
    y, stats = K.conv2d(xd, wd, None, st, (ph, pw), want_stats=True)
    d, _ = descs(cid)
    tiles = lib.adr_conv2d_fwd_bf16_stat_tiles(ctypes.byref(d))
    assert stats.numel() == tiles * 2 * Kc
    assert_exact(f"{cid} y", y, ry, BF)
    s1, s2 = R.channel_stats(ry)
    got = stats.view(tiles, 2, Kc).double().sum(0)
    assert_exact(f"{cid} sum y", got[0], s1)
    assert_exact(f"{cid} sum y^2", got[1], s2)
    # the same launch into a NaN-filled buffer: every row of every tile written, bitwise the same partials
    wp, _ = K.pack_weight2(wd, BF)
    nan = torch.full((tiles, 2, Kc), float("nan"), dtype=torch.float32, device="cuda")
    y2 = K.empty_act(N, Kc, y.shape[2], y.shape[3], BF, "cuda")
    K.conv_fwd(d, xd.data_ptr(), wp.data_ptr(), None, y2.data_ptr(), K.fptr(nan))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(nan).all()), f"{cid}: {int((~torch.isfinite(nan)).sum())} statistics entries never written"
    assert torch.equal(nan.view(-1), stats.view(-1))


# ---- fp32 engine -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", ["g_3x3_c24k48", "g_3x3s2_odd", "w_k40c24", "g_7x1", "g_3x3_c8k136",
                                 "w_split2_ragged"])
def test_exact_fp32_engine(cid):
    """The same integers as fp32 tensors through conv2d (adr_gemm.hip): y, dx and dw exact."""
    import adrefine.kernels as K
    N, H, W, C, Kc, Rr, S, st, ph, pw = geom(cid)
    x, w, dy, _ = inputs(cid)
    ry, rdx, rdw, _, _, _ = reference(cid)
    xd, wd = nhwc_dev(x, torch.float32, grad=True), w.cuda().requires_grad_(True)
    y, _ = K.conv2d(xd, wd, None, st, (ph, pw))
    y.backward(nhwc_dev(dy, torch.float32))
    assert_exact(f"{cid} fp32 y", y, ry)
    assert_exact(f"{cid} fp32 dx", xd.grad, rdx)
    assert_exact(f"{cid} fp32 dw", wd.grad, rdw)


# ---- randn tier --------------------------------------------------------------------------------------------------

def family(cid):
    return {"g": "generic", "s": "conv1", "h16": "conv3/wgrad3 TW16", "h8": "conv3/wgrad3 TW8", "w": "wgrad generic",
            "t": "wgrad thin", "d": "dg2"}[cid.split("_")[0]]


@pytest.mark.parametrize("cid", RANDN)
def test_randn_bound(cid, monkeypatch):
    if cid in DG2_CASES:
        monkeypatch.setenv("ADR_DG2H", "2")
    else:
        monkeypatch.delenv("ADR_DG2H", raising=False)
    ry, rdx, rdw, _, (sy, sdx, sdw), (ny, ndx, ndw) = reference(cid, "randn")
    assert_dispatch(cid)
    y, dx, dw, _ = run(cid, "randn")
    fam = family(cid)
    assert_bound(fam, f"{cid} y", y, ry, ny, sy)
    assert_bound(fam, f"{cid} dx", dx, rdx, ndx, sdx)
    assert_bound(fam, f"{cid} dw", dw, rdw, ndw, sdw, ulp=False)


@pytest.mark.parametrize("cid", ["g_3x3_c24k48", "s_c64k24_r1000", "h16_c96k64_h9"])
def test_randn_conv_act_sigmoid(cid):
    """conv_act sigmoid (epilogue on the fp32 accumulator): the bound through the Lipschitz constant 1/4."""
    import adrefine.kernels as K
    N, H, W, C, Kc, Rr, S, st, ph, pw = geom(cid)
    x, w, dy, b = inputs(cid, "randn", True)
    pre = R.forward(x, w, b, st, (ph, pw))
    sy = R.abs_maps(x, w, dy, st, (ph, pw), b)[0]
    ny = R.term_counts(x, w, dy, st, (ph, pw))[0] + 1  # + the bias
    with torch.no_grad():
        y = K.conv_act(nhwc_dev(x), w.cuda(), b.cuda(), st, (ph, pw), "sigmoid")
    assert_bound("act epilogue", f"{cid} sigmoid", y, pre, ny, sy, lip=0.25, act_ref=torch.sigmoid(pre))


@pytest.mark.parametrize("cid", ["g_3x3_c24k48", "s_c64k24_r1000", "h16_c96k64_h9", "h8_c96k32_w24"])
def test_randn_conv_bn_act_eval_silu(cid):
    """conv_bn_act_eval silu: act(conv * scale + shift) with the device's own fp32 scale / shift on both sides; the
    bound through silu's Lipschitz constant (<= 1.1)."""
    import adrefine.kernels as K
    N, H, W, C, Kc, Rr, S, st, ph, pw = geom(cid)
    x, w, dy, _ = inputs(cid, "randn")
    g = torch.Generator().manual_seed(_seed(cid, "randn") + 7)
    bn = torch.nn.BatchNorm2d(Kc)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(Kc, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(Kc, generator=g))
        bn.running_mean.copy_(torch.randn(Kc, generator=g))
        bn.running_var.copy_(torch.rand(Kc, generator=g) * 4 + 0.5)
    bn = bn.cuda().eval()
    with torch.no_grad():
        y = K.conv_bn_act_eval(nhwc_dev(x), w.cuda(), st, (ph, pw), bn, "silu")
        assert y is not None
        scale, shift = (t.double().cpu().view(1, Kc, 1, 1) for t in K._bn_eval_coefs(bn, torch.device("cuda")))
    conv = R.forward(x, w, None, st, (ph, pw))
    sy = R.abs_maps(x, w, dy, st, (ph, pw))[0] * scale.abs()
    ny = R.term_counts(x, w, dy, st, (ph, pw))[0]
    pre = conv * scale + shift
    assert_bound("act epilogue", f"{cid} bn silu", y, pre, ny, sy, lip=1.1, act_ref=F.silu(pre),
                 extra=2.0 ** -23 * ((conv * scale).abs() + shift.abs()))
