"""Plain float64 references for the pooling, resampling, separable-gate and MLCA ops, on (N, C, H, W) tensors and
differentiated by torch autograd (tests/test_pool_ref.py holds them against hand-written loops and the oracle;
tests/test_gpu_pool_ops.py holds the HIP kernels against them).

The second half restates the ops for an ideal bf16 implementation: the same float64 maths with a bf16 round only
where the library stores bf16 — the output and each activation gradient, and for a gradient accumulated into a
shared destination (accumulate=1) the destination before the add and the sum after it. MLCA keeps local, att, sig_l
and sig_g in fp32 and both Conv1d weight gradients too, so none of those round. The restatement's own error against
the un-rounded reference is what the bf16 parity bound is built from."""
import torch
import torch.nn.functional as F

import adr_oracle

# ---- references ----------------------------------------------------------------------------------------------


def ref_maxpool(x, k):
    """k x k, stride 1, pad k // 2 (SPPF). Ties: the first maximum in row-major window order (ATen's CPU kernel)."""
    return F.max_pool2d(x, k, 1, k // 2)


def ref_adapool(x, oh, ow):
    return F.adaptive_avg_pool2d(x, (oh, ow))


def ref_bilinear(x, oh, ow):
    return F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False)


def ref_nearest(x, s):
    return F.interpolate(x, scale_factor=s, mode="nearest")


def ref_axis_mean(x, layout):
    """Row means over W and column means over H in the layouts AxisMeanFn documents:
    'ela' (2N, C, L, 1), H-means then W-means along the batch (H == W); 'ela2' the pair (N, C, H, 1), (N, C, W, 1);
    'coord' (N, C, H + W, 1), per image the H-means then the W-means."""
    mh, mw = x.mean(3), x.mean(2)
    if layout == "ela":
        assert x.shape[2] == x.shape[3]
        return torch.cat([mh, mw], 0).unsqueeze(-1)
    if layout == "ela2":
        return mh.unsqueeze(-1), mw.unsqueeze(-1)
    assert layout == "coord"
    return torch.cat([mh, mw], 2).unsqueeze(-1)


def gate_planes(ah, aw, layout, N, H, W):
    """(a_h (N, C, H), a_w (N, C, W)) out of the planes GateFn takes in each layout."""
    if layout == "ela":
        return ah[:N, :, :, 0], aw[N:, :, :, 0]
    if layout == "ela2":
        return ah[:, :, :, 0], aw[:, :, :, 0]
    assert layout == "coord"
    return ah[:, :, :H, 0], aw[:, :, H:, 0]


def ref_gate(x, ah, aw, layout, N, H, W):
    """(x or 1) * a_h[n, c, h] * a_w[n, c, w]."""
    a_h, a_w = gate_planes(ah, aw, layout, N, H, W)
    g = a_h[..., :, None] * a_w[..., None, :]
    return g if x is None else x * g


def ref_mlca(y, res, wl, wg, local_weight=0.5):
    """res + y * att, att as the oracle's MLCA forms it (the global branch pooled over the batch axis)."""
    P = {"m.conv_local.weight": wl.reshape(1, 1, -1), "m.conv.weight": wg.reshape(1, 1, -1)}
    out = adr_oracle.mlca_attn(P, "m", y, 5, local_weight)
    return out if res is None else res + out


def batch_rows(i, B, n=5):
    """The images MLCA's batch-axis pooling averages for bin row i of n: [floor(i B / n), ceil((i + 1) B / n))."""
    return (i * B) // n, -((-(i + 1) * B) // n)


def run(fn, inputs, ups):
    """fn(*inputs) in float64 -> (outputs, gradients of sum_i <out_i, up_i> to every input). inputs may hold None
    (passed through, gradient None); an input the outputs do not depend on gets a zero gradient."""
    a = [None if t is None else t.detach().double().requires_grad_(True) for t in inputs]
    outs = fn(*a)
    outs = outs if isinstance(outs, tuple) else (outs,)
    loss = sum((o * u.double()).sum() for o, u in zip(outs, ups) if u is not None)
    live = [t for t in a if t is not None]
    g = iter(torch.autograd.grad(loss, live, allow_unused=True))
    grads = []
    for t in a:
        gi = None if t is None else next(g)
        grads.append(None if t is None else (torch.zeros_like(t) if gi is None else gi))
    return [o.detach() for o in outs], grads


# ---- ideal-bf16 restatements ---------------------------------------------------------------------------------


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float64)


def bf16_stored(outs, act_grads):
    """Every op here keeps fp32 between loading its operands and storing its results: only the stored outputs and
    the stored activation gradients round."""
    return [bf16_round(o) for o in outs], [None if g is None else bf16_round(g) for g in act_grads]


def bf16_accumulated(grads):
    """A gradient destination shared by several consumers, in the order they store: the first stores its gradient,
    each later one (accumulate=1) reads the stored value back, adds its own in fp32 and stores the sum."""
    acc = bf16_round(grads[0])
    for g in grads[1:]:
        acc = bf16_round(bf16_round(acc) + g)
    return acc


def bf16_maxpool(x, k, up):
    out, (dx,) = run(lambda t: ref_maxpool(t, k), [x], [up])
    return bf16_stored(out, [dx])


def bf16_adapool(x, oh, ow, up):
    out, (dx,) = run(lambda t: ref_adapool(t, oh, ow), [x], [up])
    return bf16_stored(out, [dx])


def bf16_bilinear(x, oh, ow, up):
    out, (dx,) = run(lambda t: ref_bilinear(t, oh, ow), [x], [up])
    return bf16_stored(out, [dx])


def bf16_nearest(x, s, up):
    out, (dx,) = run(lambda t: ref_nearest(t, s), [x], [up])
    return bf16_stored(out, [dx])


def bf16_axis_mean(x, layout, ups):
    out, (dx,) = run(lambda t: ref_axis_mean(t, layout), [x], ups)
    return bf16_stored(out, [dx])


def bf16_gate(x, ah, aw, layout, N, H, W, up):
    """-> ([out], [dx, dah, daw]); in the 'ela' layout ah and aw are one tensor and daw is None."""
    if layout == "ela":
        out, (dx, da) = run(lambda t, a: ref_gate(t, a, a, layout, N, H, W), [x, ah], [up])
        return bf16_stored(out, [dx, da, None])
    out, g = run(lambda t, a, b: ref_gate(t, a, b, layout, N, H, W), [x, ah, aw], [up])
    return bf16_stored(out, g)


def bf16_mlca(y, res, wl, wg, local_weight, up):
    """-> ([out], [dy, dres], [dwl, dwg]): out and dy round, dres is the upstream gradient handed on unchanged, the
    fp32 weight gradients do not round."""
    out, (dy, dres, dwl, dwg) = run(lambda a, r, p, q: ref_mlca(a, r, p, q, local_weight), [y, res, wl, wg], [up])
    (o,), (sdy,) = bf16_stored(out, [dy])
    return [o], [sdy, dres], [dwl, dwg]
