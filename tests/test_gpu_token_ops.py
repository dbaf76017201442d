"""Op-level parity of the attention and token-mixer kernels against the float64 references of token_ref.py,
through the public wrappers of adrefine.kernels, at the sequence lengths / token counts where the tiling changes
path: exact multiples of the 64-row attention tile and one either side, fewer rows than one wave / one tile, a
single token, the TSSA token stride (128 fp32 / 256 bf16) and one either side, channel-sliced (strided) inputs,
near-one-hot softmax rows, q rows that are exactly zero.

Inputs are seeded CPU randn rounded to the compute dtype; the same rounded values go to the reference (as doubles)
and to the device (as NHWC activations). The output, every input gradient and every parameter gradient are compared
elementwise.

fp32 mode: the project's fp32 bar, max|a-b| <= 2e-4 + 2e-4 max|b| (gpu_util.TOL), and because most of these
tensors are far smaller than 1 (a TSSA output is O(1/N)), where the absolute term alone would pass anything, also
max|a-b| <= 2e-4 max|b|.

bf16 mode: per tensor, the HIP error against the float64 reference may be at most twice the error of the ideal-bf16
restatement of the op (token_ref.bf16_*: float64 maths, rounding only the stored output and activation gradients,
and for attention P before P.V, dS before dS.K / dS^T.Q and D = sum_d dO.O from the stored O) plus one bf16 ulp of
the tensor's max, in max norm and in L2 norm. The bound comes from the restatement, never from the kernel.
Parameter gradients are stored in fp32, so their restatement error is zero and only the ulp term is left.

Analytic zeros: d(tssa_stack)/dq is zero for every q (sum_d qn^2 is 1, or 0 at a zero row, whatever q is), and
without zero rows so is d/dtemp (the softmax gradient sums to zero over tokens when every token has the same
sum_d qn^2); attention's dq and dk are zero at L = 1 (a softmax over one key). The reference returns rounding
noise for them, so they are bounded absolutely: dq (dk) by 2e-4 max|dv| (the op's largest sibling gradient), dtemp
by 2e-4 times the sum of the magnitudes of its per-token summands (the quantity that cancels), which the reference
yields as the gradient of per-token temperatures.

tssa_stack runs two heads, one at temperature 1 and one at 30, so every N sees both in one launch.

Measured on an MI355X, worst case over the shapes of each op (bf16: HIP error / restatement error, each relative
to max|ref|, for the worst tensor by ratio to its bound; fp32: worst max|a-b| / max|b|):
    op                   fp32      bf16 HIP   bf16 restatement   worst bf16 tensor
    attention            9.4e-7    3.95e-3    3.26e-3            dk, L=17
    attention, +-60      3.7e-6    2.59e-3    2.59e-3            dv, L=128
    psa_attention        8.5e-7    3.95e-3    2.77e-3            dq, 4x4
    psa_attention, +-60  3.7e-6    3.57e-3    3.57e-3            dv, 16x8
    tssa_stack           7.2e-6    2.54e-3    2.54e-3            out, N=1600
    tssa1                2.7e-6    2.61e-3    2.61e-3            dw, N=400, 4 heads
    group_mean           7.5e-8    1.80e-3    1.80e-3            dx, S=3, N=65, C=128
    dyt                  4.0e-6    1.96e-3    1.96e-3            y, HW=400, C=256
    adyt                 9.9e-7    2.40e-3    2.40e-3            y, HW=400, C=256
    ln_mix               3.2e-7    3.06e-3    3.06e-3            dx, HW=400, C=256
No bf16 tensor uses more than 0.50 of its bound; the analytic zeros stay below 0.03 of theirs.
"""
import pytest
import torch

import adrefine.kernels as K
import token_ref as R
from gpu_util import TOL

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
B = 2
ULP = 2.0 ** -8


def randn(*shape, seed, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def act(x, H=None, W=1, grad=True):
    """(B, L, C) CPU tokens -> the (B, C, H, W) NHWC activation on the device (a leaf)."""
    b, L, C = x.shape
    H = L if H is None else H
    return x.cuda().reshape(b, H, W, C).permute(0, 3, 1, 2).requires_grad_(grad)


def act_slice(x, off, width, H=None, W=1):
    """The same activation as channels [off, off + C) of a wider NHWC leaf (the rest holds 3.0)."""
    b, L, C = x.shape
    H = L if H is None else H
    wide = torch.full((b, H, W, width), 3.0, dtype=x.dtype)
    wide[..., off:off + C] = x.reshape(b, H, W, C)
    leaf = wide.cuda().permute(0, 3, 1, 2).requires_grad_(True)
    return leaf, leaf[:, off:off + C]


def tok(t):
    b, C, H, W = t.shape
    return t.detach().permute(0, 2, 3, 1).reshape(b, H * W, C).double().cpu()


def param(t):
    return t.float().cuda().requires_grad_(True)


def ref_run(fn, acts, params, ups):
    """fn(*acts, *params) in float64 -> (outputs, activation gradients, parameter gradients) for the upstream
    gradients ups (None: that output is unused)."""
    a = [x.double().requires_grad_(True) for x in acts]
    p = [x.double().requires_grad_(True) for x in params]
    outs = fn(*a, *p)
    outs = outs if isinstance(outs, tuple) else (outs,)
    loss = sum((o * u.double()).sum() for o, u in zip(outs, ups) if u is not None)
    g = torch.autograd.grad(loss, a + p, allow_unused=True)
    g = [torch.zeros_like(t) if x is None else x for x, t in zip(g, a + p)]
    return [o.detach() for o in outs], g[:len(a)], g[len(a):]


def compare(dtype, what, got, ref, rest=None, zero_scale=None, strict=True):
    """One tensor against the reference (see the module docstring); rest is the bf16 restatement of ref."""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    tag = "bf16" if dtype == torch.bfloat16 else "fp32"
    if zero_scale is not None:
        print(f"TOKERR {tag} {what} zero err={err:.3e} bound={2e-4 * zero_scale:.3e}")
        assert err <= 2e-4 * zero_scale, f"{what}: |analytic zero| {err:.3e} > 2e-4 * {zero_scale:.3e}"
    elif dtype == torch.float32:
        print(f"TOKERR {tag} {what} err={err:.3e} scale={scale:.3e} rel={err / (scale + 1e-300):.3e}")
        t = TOL[torch.float32]
        assert err <= t["atol"] + t["rtol"] * scale, f"{what}: max|d|={err:.3e} scale={scale:.3e}"
        assert not strict or err <= t["rtol"] * scale, f"{what}: max|d|={err:.3e} > 2e-4 * {scale:.3e}"
    else:
        rest = ref if rest is None else rest
        rerr, l2, rl2 = float((rest - ref).abs().max()), float((got - ref).norm()), float((rest - ref).norm())
        print(f"TOKERR {tag} {what} err={err:.3e} rest={rerr:.3e} l2={l2:.3e} restl2={rl2:.3e} scale={scale:.3e} "
              f"rel={err / (scale + 1e-300):.3e} restrel={rerr / (scale + 1e-300):.3e} "
              f"use={max(err / (2 * rerr + ULP * scale + 1e-300), l2 / (2 * rl2 + ULP * scale + 1e-300)):.3f}")
        assert err <= 2 * rerr + ULP * scale, f"{what}: max|d|={err:.3e} > 2 * {rerr:.3e} + ulp {ULP * scale:.3e}"
        assert l2 <= 2 * rl2 + ULP * scale, f"{what}: |d|_2={l2:.3e} > 2 * {rl2:.3e} + ulp {ULP * scale:.3e}"


# ---- attention ------------------------------------------------------------------------------------------------


def sharpen(x, dtype, qcols, logits):
    """Scale the q channels so the scaled logits span about +-60 (softmax rows near one-hot)."""
    f = 60.0 / float(logits(x.double()).abs().max())
    x = x.clone()
    x[..., qcols] = (x[..., qcols].float() * f).to(dtype)
    return x


def mha_logits(heads):
    def f(qkv):
        E = qkv.shape[-1] // 3
        q, k = (R._heads(t, heads) for t in qkv.split(E, -1)[:2])
        return q @ k.transpose(-1, -2) * (E // heads) ** -0.5
    return f


def psa_logits(heads, kd, hd):
    def f(qkv):
        q, k, _ = R.psa_split(qkv, heads, kd, hd)
        return q @ k.transpose(-1, -2) * kd ** -0.5
    return f


def attention_case(dtype, L, heads, big=False):
    E = 64 * heads
    qkv = randn(B, L, 3 * E, seed=1000 + L, dtype=dtype)
    if big:
        qkv = sharpen(qkv, dtype, slice(0, E), mha_logits(heads))
    up = randn(B, L, E, seed=2000 + L, dtype=dtype)
    return qkv, up


def attention_hip(qkv, up, heads, sliced=False):
    leaf, x = act_slice(qkv, 16, qkv.shape[-1] + 40) if sliced else (None, act(qkv))
    o = K.attention(x, heads)
    o.backward(act(up, grad=False))
    g = leaf.grad if sliced else x.grad
    return o, g


def check_attention(dtype, L, heads, big=False, sliced=False):
    qkv, up = attention_case(dtype, L, heads, big)
    o, g = attention_hip(qkv, up, heads, sliced)
    (ro,), (rg,), _ = ref_run(lambda t: R.ref_mha(t, heads), [qkv], [], [up])
    so, sg = R.bf16_mha(qkv.double(), heads, up.double()) if dtype == torch.bfloat16 else (None, None)
    name = f"attention L={L} h={heads}{' big' if big else ''}{' sliced' if sliced else ''}"
    compare(dtype, f"{name} o", tok(o), ro, so)
    if sliced:
        wide = tok(g)
        C = qkv.shape[-1]
        assert float(wide[..., :16].abs().max()) == 0 and float(wide[..., 16 + C:].abs().max()) == 0
        g = g[:, 16:16 + C]
    E = 64 * heads
    # a softmax over one key is 1 whatever the logit: at L = 1 dq and dk are analytic zeros (bounded like TSSA's dq)
    zs = float(rg[..., 2 * E:].abs().max()) if L == 1 else None
    for i, n in enumerate(("dq", "dk", "dv")):
        compare(dtype, f"{name} {n}", tok(g)[..., i * E:(i + 1) * E], rg[..., i * E:(i + 1) * E],
                None if sg is None else sg[..., i * E:(i + 1) * E], zero_scale=zs if i < 2 else None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,heads", [(1, 2), (16, 2), (17, 2), (63, 2), (64, 2), (65, 2), (128, 2), (200, 2), (65, 4)])
def test_attention(dtype, L, heads):
    check_attention(dtype, L, heads)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [65, 128])
def test_attention_large_logits(dtype, L):
    check_attention(dtype, L, 2, big=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_strided(dtype):
    check_attention(dtype, 65, 2, sliced=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_deterministic(dtype):
    qkv, up = attention_case(dtype, 200, 2)
    (o1, g1), (o2, g2) = attention_hip(qkv, up, 2), attention_hip(qkv, up, 2)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)


# ---- C2PSA attention ------------------------------------------------------------------------------------------

KD, HD = 32, 64


def check_psa(dtype, H, W, heads, big=False, sliced=False, no_do=False):
    L, C, Ct = H * W, heads * HD, heads * (2 * KD + HD)
    qkv = randn(B, L, Ct, seed=3000 + L + heads, dtype=dtype)
    if big:
        qcols = torch.arange(Ct).view(heads, -1)[:, :KD].reshape(-1)
        qkv = sharpen(qkv, dtype, qcols, psa_logits(heads, KD, HD))
    do = torch.zeros(B, L, C, dtype=dtype) if no_do else randn(B, L, C, seed=3100 + L, dtype=dtype)
    dv = randn(B, L, C, seed=3200 + L, dtype=dtype)
    leaf, x = act_slice(qkv, 8, Ct + 24, H, W) if sliced else (None, act(qkv, H, W))
    o, v = K.psa_attention(x, heads, KD, HD)
    if no_do:  # only the pe branch carries gradient: backward sees do = None and zero-fills dq / dk
        v.backward(act(dv, H, W, grad=False))
    else:
        torch.autograd.backward([o, v], [act(do, H, W, grad=False), act(dv, H, W, grad=False)])
    g = leaf.grad[:, 8:8 + Ct] if sliced else x.grad
    (ro, rv), (rg,), _ = ref_run(lambda t: R.ref_psa(t, heads, KD, HD), [qkv], [], [do, dv])
    so, sv, sg = R.bf16_psa(qkv.double(), heads, KD, HD, do.double(), dv.double()) if dtype == torch.bfloat16 \
        else (None, None, None)
    name = f"psa {H}x{W} h={heads}{' big' if big else ''}{' sliced' if sliced else ''}{' no_do' if no_do else ''}"
    compare(dtype, f"{name} o", tok(o), ro, so)
    compare(dtype, f"{name} v", tok(v), rv, sv)
    per_head = lambda t: t.reshape(B, L, heads, 2 * KD + HD)
    zs = float(per_head(rg)[..., 2 * KD:].abs().max()) if L == 1 else None  # one key: dq, dk are analytic zeros
    for n, sl in (("dq", slice(0, KD)), ("dk", slice(KD, 2 * KD)), ("dv", slice(2 * KD, None))):
        compare(dtype, f"{name} {n}", per_head(tok(g))[..., sl], per_head(rg)[..., sl],
                None if sg is None else per_head(sg)[..., sl], zero_scale=None if n == "dv" else zs)
    if sliced:
        wide = tok(leaf.grad)
        assert float(wide[..., :8].abs().max()) == 0 and float(wide[..., 8 + Ct:].abs().max()) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W,heads", [(1, 1, 2), (4, 4, 2), (8, 8, 2), (5, 13, 2), (16, 8, 2), (10, 10, 2), (5, 13, 4)])
def test_psa_attention(dtype, H, W, heads):
    check_psa(dtype, H, W, heads)


@pytest.mark.parametrize("dtype", DTYPES)
def test_psa_attention_pe_only(dtype):
    check_psa(dtype, 5, 13, 2, no_do=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W", [(5, 13), (16, 8)])
def test_psa_attention_large_logits(dtype, H, W):
    check_psa(dtype, H, W, 2, big=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_psa_attention_strided(dtype):
    check_psa(dtype, 5, 13, 2, sliced=True)


# ---- TSSA (cross-scale stack) ---------------------------------------------------------------------------------

TEMPS = [[1.0, 30.0], [30.0, 1.0], [1.0, 30.0]]  # (scale, head): both temperatures at every N


def tssa_case(dtype, N, S, zero=False, tiny=False):
    C = 128
    qkvs = [randn(B, N, 3 * C, seed=4000 + 10 * N + s, dtype=dtype) for s in range(S)]
    for x in qkvs:
        if zero:  # a quarter of the tokens: head 0's q exactly zero (Pi no longer uniform, the 1e-12 clamp is taken)
            x[:, 1::4, 0:64] = 0
        if tiny:  # and another quarter far below 1 but above the clamp: still unit vectors after normalisation
            x[:, 3::4, 0:64] = (x[:, 3::4, 0:64].float() * 1e-9).to(dtype)
    temps = torch.tensor(TEMPS[:S]).view(S, 2, 1)
    up = randn(B, S * N, C, seed=4500 + N, dtype=dtype)
    return qkvs, temps, up


def tssa_hip(qkvs, temps, up, sliced=False):
    pairs = [act_slice(x, 8, x.shape[-1] + 16) if sliced else (None, act(x)) for x in qkvs]
    t = param(temps)
    out = K.tssa_stack(t, 2, [p[1] for p in pairs])
    out.backward(act(up, grad=False))
    w = qkvs[0].shape[-1]
    return out, [p[0].grad[:, 8:8 + w] if sliced else p[1].grad for p in pairs], t.grad


def check_tssa_stack(dtype, N, S, zero=False, sliced=False):
    C = 128
    qkvs, temps, up = tssa_case(dtype, N, S, zero)
    out, grads, dtemp = tssa_hip(qkvs, temps, up, sliced)
    # per-token temperatures: their gradients are the summands of dtemp
    tt = temps.expand(S, 2, N).contiguous()
    (ro,), rg, (rtt,) = ref_run(lambda *a: R.ref_tssa_stack(a[-1], 2, a[:-1]), qkvs, [tt], [up])
    so, sg = R.bf16_stored(ro, rg) if dtype == torch.bfloat16 else (None, [None] * S)
    name = f"tssa_stack N={N} S={S}{' zero-q' if zero else ''}{' sliced' if sliced else ''}"
    compare(dtype, f"{name} out", tok(out), ro, so)
    for s in range(S):
        g, r = tok(grads[s]), rg[s]
        sl = [slice(i * C, (i + 1) * C) for i in range(3)]
        compare(dtype, f"{name} dq{s}", g[..., sl[0]], r[..., sl[0]], zero_scale=float(r[..., sl[2]].abs().max()))
        for i, n in ((1, "dk"), (2, "dv")):
            compare(dtype, f"{name} {n}{s}", g[..., sl[i]], r[..., sl[i]], None if sg[s] is None else sg[s][..., sl[i]])
    if zero:
        compare(dtype, f"{name} dtemp", dtemp.view(S, 2), rtt.sum(-1))
    else:
        compare(dtype, f"{name} dtemp", dtemp.view(S, 2), rtt.sum(-1), zero_scale=float(rtt.abs().sum(-1).max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,S", [(n, 1) for n in (1, 7, 63, 64, 65, 127, 128, 129, 255, 256, 257, 400, 1600)]
                         + [(7, 3), (65, 3), (257, 3)])
def test_tssa_stack(dtype, N, S):
    check_tssa_stack(dtype, N, S)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [65, 257])
def test_tssa_stack_zero_q(dtype, N):
    check_tssa_stack(dtype, N, 1, zero=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [65, 257])
def test_tssa_stack_tiny_q_forward(dtype, N):
    """q rows of norm ~1e-9 sit above F.normalize's 1e-12 clamp: they normalise to unit vectors like any other row,
    next to rows that are exactly zero. Forward only: at such a row the analytically zero dq is the difference of
    two terms of size dss / |q|, which no fp32 implementation (torch's included) resolves."""
    qkvs, temps, up = tssa_case(dtype, N, 1, zero=True, tiny=True)
    with torch.no_grad():
        out = K.tssa_stack(temps.float().cuda(), 2, [act(x, grad=False) for x in qkvs])
    ro = R.ref_tssa_stack(temps.double(), 2, [x.double() for x in qkvs])
    compare(dtype, f"tssa_stack N={N} tiny-q out", tok(out), ro, R.bf16_round(ro))


@pytest.mark.parametrize("dtype", DTYPES)
def test_tssa_stack_strided(dtype):
    check_tssa_stack(dtype, 65, 1, sliced=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tssa_stack_deterministic(dtype):
    qkvs, temps, up = tssa_case(dtype, 257, 1)
    (o1, g1, t1), (o2, g2, t2) = tssa_hip(qkvs, temps, up), tssa_hip(qkvs, temps, up)
    assert torch.equal(o1, o2) and torch.equal(g1[0], g2[0]) and torch.equal(t1, t2)


# ---- AttentionTSSA core ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 7, 63, 64, 65, 127, 128, 129, 255, 256, 257, 400])
def test_tssa1(dtype, N):
    for heads in (1, 4):  # head dim 64 is the only one adr_tssa1_fwd admits
        C = 64 * heads
        w = randn(B, N, C, seed=5000 + 10 * N + heads, dtype=dtype)
        # close temperatures: at N = 1 the logits are 64 * temp, and the softmax over heads should stay mixed
        temp = torch.tensor([1.0, 0.97, 1.05, 1.02][:heads]).view(heads, 1)
        up = randn(B, N, C, seed=5500 + N, dtype=dtype)
        x, t = act(w), param(temp)
        out = K.tssa1(x, t, heads)
        out.backward(act(up, grad=False))
        (ro,), (rg,), (rt,) = ref_run(lambda a, p: R.ref_tssa1(a, p, heads), [w], [temp], [up])
        so, (sg,) = R.bf16_stored(ro, [rg]) if dtype == torch.bfloat16 else (None, [None])
        name = f"tssa1 N={N} h={heads}"
        compare(dtype, f"{name} out", tok(out), ro, so)
        # the part of dw that comes through the token-axis normalisation cancels (sum_n wn^2 is 1 per channel; at
        # N = 1 it cancels entirely, leaving fp32 noise of size ds / |w|); it rides on the direct -g pi attn term,
        # so dw is compared as a whole against its own max, in fp32 mode without the purely relative bound
        compare(dtype, f"{name} dw", tok(x.grad), rg, sg, strict=False)
        compare(dtype, f"{name} dtemp", t.grad, rt)


# ---- group mean, DynamicTanh, AdaptiveDynamicTanh, LayerNorm mix -------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_mean(dtype):
    for S in (1, 3):
        for N in (1, 65):
            for C in (8, 128):
                x = randn(B, S * N, C, seed=6000 + 100 * S + N + C, dtype=dtype)
                up = randn(B, N, C, seed=6500 + N + C, dtype=dtype)
                xd = act(x)
                y = K.group_mean(xd, S)
                y.backward(act(up, grad=False))
                (ro,), (rg,), _ = ref_run(lambda a: R.ref_group_mean(a, S), [x], [], [up])
                so, (sg,) = R.bf16_stored(ro, [rg]) if dtype == torch.bfloat16 else (None, [None])
                compare(dtype, f"group_mean S={S} N={N} C={C} y", tok(y), ro, so)
                compare(dtype, f"group_mean S={S} N={N} C={C} dx", tok(xd.grad), rg, sg)


HWS = [(2, 1, 15), (2, 17, 1), (2, 10, 10), (2, 1, 257), (2, 20, 20), (2, 1, 1), (1, 10, 10)]  # (images, H, W)


def pointwise_check(dtype, name, hip, ref, x, H, W, params, sliced=False):
    """y = op(x, *params): output, dx and every parameter gradient."""
    n, L, C = x.shape
    up = randn(n, L, C, seed=7900 + L + C, dtype=dtype)
    leaf, xd = act_slice(x, 8, C + 24, H, W) if sliced else (None, act(x, H, W))
    ps = [param(p) for p in params]
    y = hip(xd, *ps)
    y.backward(act(up, H, W, grad=False))
    (ro,), (rg,), rp = ref_run(ref, [x], params, [up])
    so, (sg,) = R.bf16_stored(ro, [rg]) if dtype == torch.bfloat16 else (None, [None])
    compare(dtype, f"{name} y", tok(y), ro, so)
    compare(dtype, f"{name} dx", tok(leaf.grad[:, 8:8 + C] if sliced else xd.grad), rg, sg)
    for i, (p, r) in enumerate(zip(ps, rp)):
        compare(dtype, f"{name} dparam{i}", p.grad, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,H,W", HWS)
def test_dyt(dtype, n, H, W):
    for C in (8, 64, 256):
        x = randn(n, H * W, C, seed=7000 + H * W + C, dtype=dtype)
        params = [torch.tensor([0.7]), 1 + 0.5 * randn(C, seed=7001), 0.5 * randn(C, seed=7002)]
        pointwise_check(dtype, f"dyt n={n} HW={H * W} C={C}", K.dyt, R.ref_dyt, x, H, W, params)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,H,W", HWS)
def test_adyt(dtype, n, H, W):
    for C in (8, 64, 256):
        x = randn(n, H * W, C, seed=7100 + H * W + C, dtype=dtype)
        params = [torch.linspace(0.3, 1.0, 3).view(1, 3, 1, 1), torch.softmax(randn(n, 3, seed=7101), 1),
                  1 + 0.5 * randn(C, seed=7102), 0.5 * randn(C, seed=7103)]
        pointwise_check(dtype, f"adyt n={n} HW={H * W} C={C}", K.adyt, R.ref_adyt, x, H, W, params)


def ln_params(C):
    return [1 + 0.5 * randn(C, seed=7201), 0.5 * randn(C, seed=7202), randn(C, 1, 1, seed=7203),
            1 + 0.5 * randn(C, 1, 1, seed=7204)]


def ln_hip(x, lw, lb, gm, gx):
    return K.ln_mix(x, lw, lb, gm, gx, 1e-5)


def ln_ref(x, lw, lb, gm, gx):
    return R.ref_ln_mix(x, lw, lb, gm, gx, 1e-5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,H,W", HWS)
def test_ln_mix(dtype, n, H, W):
    for C in (64, 256):  # C = 8 is refused, see test_ln_mix_refuses_8_channels
        x = randn(n, H * W, C, seed=7200 + H * W + C, dtype=dtype)
        pointwise_check(dtype, f"ln_mix n={n} HW={H * W} C={C}", ln_hip, ln_ref, x, H, W, ln_params(C))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_mix_strided(dtype):
    x = randn(B, 100, 64, seed=7300, dtype=dtype)
    pointwise_check(dtype, "ln_mix sliced HW=100 C=64", ln_hip, ln_ref, x, 10, 10, ln_params(64), sliced=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_mix_refuses_8_channels(dtype):
    """adr_ln_mix_fwd's ADR_REQUIRE (adr_mona.hip, 'ln_mix_fwd: C=%d unsupported') admits 8, 16, 32 or 64 lanes of
    one 16-byte vector per pixel: C = 8 is one lane (bf16) or two (fp32). It surfaces as the wrapper's error."""
    x = act(randn(B, 15, 8, seed=7400, dtype=dtype), grad=False)
    with pytest.raises(RuntimeError, match="adr_ln_mix_fwd: ln_mix_fwd: C=8 unsupported"):
        ln_hip(x, *[p.cuda() for p in ln_params(8)])
