"""The float64 references of tests/token_ref.py against torch and the oracle (CPU): they are what the HIP token
kernels are held to, so they are themselves pinned to 1e-12 here."""
import pytest
import torch
import torch.nn.functional as F

import adr_oracle
import token_ref as R

TOL = 1e-12


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def close(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


def to_map(t, H, W):
    """(B, L, C) tokens -> (B, C, H, W)."""
    B, L, C = t.shape
    return t.permute(0, 2, 1).reshape(B, C, H, W)


@pytest.mark.parametrize("L,heads", [(1, 2), (7, 2), (65, 4)])
def test_ref_mha_is_sdpa(L, heads):
    B, hd = 2, 64
    E = heads * hd
    qkv = randn(B, L, 3 * E, seed=1)
    q, k, v = (t.reshape(B, L, heads, hd).transpose(1, 2) for t in qkv.split(E, -1))
    want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, L, E)
    close(R.ref_mha(qkv, heads), want)


@pytest.mark.parametrize("H,W,heads", [(1, 1, 2), (5, 13, 2), (4, 4, 4)])
def test_ref_psa_is_oracle(monkeypatch, H, W, heads):
    B, kd, hd = 2, 32, 64
    qkv = randn(B, H * W, heads * (2 * kd + hd), seed=2)
    seen = {}

    def fake_conv(P, pre, x, *a, **kw):  # qkv conv -> the prepared qkv; pe -> 0 (and record its input); proj -> identity
        if pre.endswith(".qkv"):
            return to_map(qkv, H, W)
        if pre.endswith(".pe"):
            seen["v"] = x
            return torch.zeros_like(x)
        return x

    monkeypatch.setattr(adr_oracle, "conv_bn_act", fake_conv)
    want = adr_oracle.psa_attention({}, "a", torch.zeros(B, heads * hd, H, W, dtype=torch.float64), heads, True)
    o, v = R.ref_psa(qkv, heads, kd, hd)
    close(to_map(o, H, W), want)
    close(to_map(v, H, W), seen["v"])


@pytest.mark.parametrize("S", [1, 3])
def test_ref_tssa_stack_is_oracle(monkeypatch, S):
    B, C, H, W, heads = 2, 16, 3, 5, 2
    x = randn(B, C, H, W, seed=3)
    P = {f"a.qkv_projections.{i}.weight": randn(3 * C, C, seed=10 + i) for i in range(S)}
    P["a.temps"] = 1.0 + randn(S, heads, 1, seed=4).abs() * 5
    P["a.to_out.0.weight"], P["a.to_out.0.bias"] = torch.eye(C, dtype=torch.float64), None
    seen = {}

    def fake_mha(st, P, pre, heads):  # the stacked TSSA outputs are the attention's input
        seen["st"] = st
        return st

    monkeypatch.setattr(adr_oracle, "mha", fake_mha)
    adr_oracle.cross_scale_tssa(P, "a", x, heads, scales=(1,) * S)
    xt = x.flatten(2).permute(0, 2, 1)
    qkvs = [F.linear(xt, P[f"a.qkv_projections.{i}.weight"]) for i in range(S)]
    close(R.ref_tssa_stack(P["a.temps"], heads, qkvs), seen["st"])
    # per-token temperatures: the same output, and their gradients sum to the temperature's
    tok = P["a.temps"].expand(S, heads, H * W).clone().requires_grad_(True)
    t = P["a.temps"].clone().requires_grad_(True)
    g = randn(B, S * H * W, C, seed=5)
    close(R.ref_tssa_stack(tok, heads, qkvs).detach(), seen["st"])
    (R.ref_tssa_stack(tok, heads, qkvs) * g).sum().backward()
    (R.ref_tssa_stack(t, heads, qkvs) * g).sum().backward()
    assert float((tok.grad.sum(-1, keepdim=True) - t.grad).abs().max()) <= TOL * float(tok.grad.abs().sum(-1).max())


@pytest.mark.parametrize("heads", [1, 4])
def test_ref_tssa1_is_oracle(heads):
    B, N, C = 2, 11, 16
    w = randn(B, N, C, seed=6)
    eye = torch.eye(C, dtype=torch.float64)
    P = {"a.qkv.weight": eye, "a.temp": 1.0 + randn(heads, 1, seed=7).abs() * 5, "a.to_out.0.weight": eye,
         "a.to_out.0.bias": torch.zeros(C, dtype=torch.float64)}
    close(R.ref_tssa1(w, P["a.temp"], heads), adr_oracle.attention_tssa(P, "a", w, heads))


def test_ref_ln_mix_is_layer_norm():
    B, L, C, eps = 2, 9, 24, 1e-5
    x = randn(B, L, C, seed=8)
    lw, lb, gm, gx = (randn(C, seed=20 + i) for i in range(4))
    want = F.layer_norm(x, (C,), lw, lb, eps) * gm + x * gx
    close(R.ref_ln_mix(x, lw, lb, gm.view(C, 1, 1), gx.view(C, 1, 1), eps), want)


def test_ref_dyt_adyt_are_oracle():
    B, H, W, C = 2, 3, 4, 8
    x = randn(B, H * W, C, seed=9)
    xm = to_map(x, H, W)
    P = {"d.alpha": torch.tensor([0.7], dtype=torch.float64), "d.weight": randn(C, seed=30), "d.bias": randn(C, seed=31),
         "d.alphas": torch.linspace(0.3, 1.0, 3, dtype=torch.float64).view(1, 3, 1, 1),
         "d.importance_gate.1.weight": randn(4, C, 1, 1, seed=32), "d.importance_gate.1.bias": randn(4, seed=33),
         "d.importance_gate.3.weight": randn(3, 4, 1, 1, seed=34), "d.importance_gate.3.bias": randn(3, seed=35)}
    close(to_map(R.ref_dyt(x, P["d.alpha"], P["d.weight"], P["d.bias"]), H, W), adr_oracle.dyt(P, "d", xm))
    g = torch.relu(adr_oracle.conv2d_b(P, "d.importance_gate.1", xm.mean((2, 3), keepdim=True), 1))
    imp = torch.softmax(adr_oracle.conv2d_b(P, "d.importance_gate.3", g, 1), 1).view(B, 3)
    close(to_map(R.ref_adyt(x, P["d.alphas"], imp, P["d.weight"], P["d.bias"]), H, W), adr_oracle.adaptive_dyt(P, "d", xm))


def test_ref_group_mean():
    x = randn(2, 3 * 5, 8, seed=40)
    close(R.ref_group_mean(x, 3), torch.stack([x[:, 0:5], x[:, 5:10], x[:, 10:15]], 1).mean(1))
    close(R.ref_group_mean(x, 1), x)


def test_bf16_restatements_round_only():
    """Without rounding the restatements are the references: their float64 maths (the hand-written attention
    backward included) matches autograd to 1e-12 when bf16_round is the identity, and with it the outputs move by
    no more than bf16 precision."""
    B, L, heads, kd, hd = 2, 37, 2, 32, 64
    for name in ("mha", "psa"):
        C = 3 * heads * hd if name == "mha" else heads * (2 * kd + hd)
        qkv = randn(B, L, C, seed=50).requires_grad_(True)
        do, dv = randn(B, L, heads * hd, seed=51), randn(B, L, heads * hd, seed=52)
        if name == "mha":
            o = R.ref_mha(qkv, heads)
            (o * do).sum().backward()
            run = lambda: R.bf16_mha(qkv.detach(), heads, do)
        else:
            o, v = R.ref_psa(qkv, heads, kd, hd)
            ((o * do).sum() + (v * dv).sum()).backward()
            run = lambda: R.bf16_psa(qkv.detach(), heads, kd, hd, do, dv)
        rounded = run()
        saved, R.bf16_round = R.bf16_round, lambda t: t
        try:
            exact = run()
        finally:
            R.bf16_round = saved
        close(exact[0], o.detach())
        close(exact[-1], qkv.grad)
        for a, b in ((rounded[0], o.detach()), (rounded[-1], qkv.grad)):
            assert 0 < float((a - b).norm() / b.norm()) < 2 ** -7
