"""Plain float64 references for the attention and token-mixer ops, written as the mathematical definition on
(B, L, C) token tensors and differentiated by torch autograd (tests/test_token_ref.py holds them against torch
and the oracle; tests/test_gpu_token_ops.py holds the HIP kernels against them).

The second half restates each op for an ideal bf16 implementation: the same float64 maths with a bf16 round at
the points where any bf16 implementation has to round — the stored output and the stored activation gradients,
and for attention also P before P·V and dS before dS·K / dSᵀ·Q (the matrix-core operands), with the softmax
gradient's row offset D = Σ_d dO·O taken from the output as stored: a flash-attention backward never holds a whole
row of P·dP, so D comes from O, and near one-hot rows dS is the small difference dP − D and inherits O's rounding
(without this point the restatement's dQ error at ±60 logits is 2.2-2.9x smaller in L2, and the kernel's dQ, which
reads D from O, sat at 2.2-2.5x of it). Parameter gradients are kept in fp32 by the library and are not rounded.
The restatement's own error against the un-rounded reference is what the bf16 parity bound is built from."""
import math

import torch
import torch.nn.functional as F


# ---- references ----------------------------------------------------------------------------------------------


def _heads(t, heads):
    B, L, E = t.shape
    return t.reshape(B, L, heads, E // heads).transpose(1, 2)  # (B, h, L, d)


def _unheads(t):
    B, h, L, d = t.shape
    return t.transpose(1, 2).reshape(B, L, h * d)


def ref_mha(qkv, heads):
    """qkv (B, L, 3E) planar [q|k|v] -> softmax(q k^T / sqrt(hd)) v, (B, L, E)."""
    E = qkv.shape[-1] // 3
    q, k, v = (_heads(t, heads) for t in qkv.split(E, -1))
    a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(E // heads), -1)
    return _unheads(a @ v)


def psa_split(qkv, heads, kd, hd):
    """(B, L, heads*(2kd+hd)) with per-head [q(kd) k(kd) v(hd)] -> q, k (B, h, L, kd) and v (B, h, L, hd)."""
    B, L, _ = qkv.shape
    t = qkv.reshape(B, L, heads, 2 * kd + hd).transpose(1, 2)
    return t[..., :kd], t[..., kd:2 * kd], t[..., 2 * kd:]


def ref_psa(qkv, heads, kd, hd):
    """C2PSA's Attention core: o = softmax(q k^T * kd^-0.5) v and the gathered v, both (B, L, heads*hd)."""
    q, k, v = psa_split(qkv, heads, kd, hd)
    a = torch.softmax(q @ k.transpose(-1, -2) * kd ** -0.5, -1)
    return _unheads(a @ v), _unheads(v)


def ref_tssa_stack(temps, heads, qkvs):
    """Per scale s: qn = normalize(q) over d, pi = softmax over tokens of temp * sum_d qn^2,
    attn = 1 / (1 + sum_n pi k^2), out = -v pi attn; the S outputs stacked along tokens, (B, S*N, C).
    temps holds S*heads values, or S*heads*N (one per token: the summands of the temperature gradient)."""
    S = len(qkvs)
    tp = temps.reshape(S, heads, -1)
    outs = []
    for s, qkv in enumerate(qkvs):
        C = qkv.shape[-1] // 3
        q, k, v = (_heads(t, heads) for t in qkv.split(C, -1))
        qn = F.normalize(q, dim=-1)
        pi = torch.softmax((qn ** 2).sum(-1) * tp[s], -1)  # (B, h, N)
        attn = 1.0 / (1.0 + (pi.unsqueeze(-1) * k ** 2).sum(-2, keepdim=True))  # (B, h, 1, d)
        outs.append(_unheads(-v * pi.unsqueeze(-1) * attn))
    return torch.cat(outs, 1)


def ref_tssa1(w, temp, heads):
    """AttentionTSSA core: wn = normalize(w) over TOKENS, pi = softmax over HEADS of temp * sum_d wn^2,
    attn = 1 / (1 + sum_n pi / (sum_n pi + 1e-8) w^2), out = -w pi attn; (B, N, C)."""
    x = _heads(w, heads)  # (B, h, N, d)
    wn = F.normalize(x, dim=-2)
    pi = torch.softmax((wn ** 2).sum(-1) * temp.reshape(heads, 1), 1)
    ph = pi / (pi.sum(-1, keepdim=True) + 1e-8)
    attn = 1.0 / (1.0 + (ph.unsqueeze(-1) * x ** 2).sum(-2, keepdim=True))
    return _unheads(-x * pi.unsqueeze(-1) * attn)


def ref_group_mean(x, S):
    """(B, S*N, C) -> mean over the S stacked groups, (B, N, C)."""
    B, SN, C = x.shape
    return x.reshape(B, S, SN // S, C).mean(1)


def ref_dyt(x, alpha, w, b):
    return torch.tanh(alpha.reshape(()) * x) * w + b


def ref_adyt(x, alphas, imp, w, b):
    """x (B, L, C), alphas 3 values, imp (B, 3): (sum_j tanh(alpha_j x) imp_j) * w + b."""
    a = alphas.reshape(-1)
    acc = sum(torch.tanh(a[j] * x) * imp[:, j, None, None] for j in range(a.numel()))
    return acc * w + b


def ref_ln_mix(x, lw, lb, gamma, gammax, eps):
    """LayerNorm over channels (biased variance) with weight / bias, times gamma, plus x times gammax."""
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    xn = (x - mu) / torch.sqrt(var + eps) * lw.reshape(-1) + lb.reshape(-1)
    return xn * gamma.reshape(-1) + x * gammax.reshape(-1)


# ---- ideal-bf16 restatements ---------------------------------------------------------------------------------


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float64)


def bf16_stored(out, act_grads):
    """The restatement of an op whose arithmetic stays in fp32 between loading its operands and storing its
    results (tssa_stack, tssa1, group_mean, dyt, adyt, ln_mix): only the stored output and the stored activation
    gradients round."""
    return bf16_round(out), [bf16_round(g) for g in act_grads]


def _attn_bf16(q, k, v, do, scale):
    """One attention core on (B, h, L, d) doubles with the bf16 rounding points; returns o, dq, dk, dv."""
    p = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
    pr = bf16_round(p)
    o = bf16_round(pr @ v)
    dv = bf16_round(pr.transpose(-1, -2) @ do)
    dp = do @ v.transpose(-1, -2)
    ds = bf16_round(p * (dp - (do * o).sum(-1, keepdim=True)))  # D from the stored (rounded) output
    dq = bf16_round(ds @ k * scale)
    dk = bf16_round(ds.transpose(-1, -2) @ q * scale)
    return o, dq, dk, dv


def bf16_mha(qkv, heads, do):
    """-> (o, dqkv) of ref_mha for the upstream gradient do, as an ideal bf16 implementation stores them."""
    E = qkv.shape[-1] // 3
    q, k, v = (_heads(t, heads) for t in qkv.split(E, -1))
    o, dq, dk, dv = _attn_bf16(q, k, v, _heads(do, heads), (E // heads) ** -0.5)
    return _unheads(o), torch.cat([_unheads(dq), _unheads(dk), _unheads(dv)], -1)


def bf16_psa(qkv, heads, kd, hd, do, dv_pe):
    """-> (o, v, dqkv) of ref_psa for the upstream gradients of o and of the gathered v."""
    q, k, v = psa_split(qkv, heads, kd, hd)
    o, dq, dk, dv = _attn_bf16(q, k, v, _heads(do, heads), kd ** -0.5)
    dv = bf16_round(dv + _heads(dv_pe, heads))  # the pe branch accumulates into the stored dv
    B, _, L, _ = q.shape
    g = torch.cat([dq, dk, dv], -1).transpose(1, 2).reshape(B, L, heads * (2 * kd + hd))
    return _unheads(o), _unheads(v), g
