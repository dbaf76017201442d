"""BatchNorm finalize (adr_bn_finalize / adr_bn_bwd_finalize): the per-channel reduction of the [P][2][C] partial
rows every BN producer writes (reference nn/modules/conv.py:36-54 BatchNorm2d in train mode: batch mean and biased
variance, running stats with the unbiased variance; backward dgamma = sum g * xhat, dbeta = sum g and the
coefficients of dx = A g + B x + C). Long finalizes (P > 4096 rows, > 2048 at C >= 256) first pre-sum blocks of
rows over the whole chip (fin_presum_kernel) into scratch the caller sizes with adr_bn_finalize_scratch_floats and
owns; both forms must agree with an fp64 restatement of the same partials, and with each other to fp32 rounding,
across the P / C shapes of the n-scale step (P 64 - 25 600, C 8 - 256), both sides of the split threshold and ragged
row counts. The scratch is per call: every row the finalize reads was written by its own pre-sum, nothing is
written past the queried size, and finalizes on different streams do not meet."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(64, 256), (2048, 64), (3200, 128), (3200, 256), (4097, 32), (12800, 8), (25600, 16), (10240, 16),
          (7777, 48), (2049, 256), (4096, 32)]
LONG = {(2049, 256): True, (4096, 32): False, (4097, 32): True}  # the split threshold's edge: scratch query != 0
_QUERY = object()  # scratch argument: a fresh zeroed buffer of the queried size (None when the query says 0)


def _scratch(P, C, scratch, mode, dev):
    """The scratch tensor to pass: the caller's, or (by default) what adr_bn_finalize_scratch_floats asks for."""
    from adrefine.native import lib
    if scratch is not _QUERY:
        return scratch
    n = lib.adr_bn_finalize_scratch_floats(P, C)
    assert n in (0, 256 * 2 * C), n
    if mode == "0":
        assert n == 0, n
    return torch.zeros(n, device=dev) if n else None


def _fwd(part, P, C, count, monkeypatch, mode, scratch=_QUERY, sync=True):
    from adrefine import kernels as K
    from adrefine.native import lib
    monkeypatch.setenv("ADR_FIN_PRESUM", mode)
    dev = part.device
    scratch = _scratch(P, C, scratch, mode, dev)
    g = torch.linspace(0.5, 1.5, C, device=dev)
    b = torch.linspace(-0.2, 0.2, C, device=dev)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    sc, sh, mu, rs = (torch.full((C,), float("nan"), device=dev) for _ in range(4))
    fp = K.fptr
    lib.adr_bn_finalize(fp(part), P, C, count, fp(g), fp(b), fp(rm), fp(rv), 0.03, 1e-3, 1, fp(sc), fp(sh), fp(mu),
                        fp(rs), fp(scratch), K.stream())
    if sync:
        torch.cuda.synchronize()
    return dict(scale=sc, shift=sh, mean=mu, rstd=rs, rm=rm, rv=rv, g=g, b=b)


def _bwd(part, P, C, count, mean, rstd, monkeypatch, mode, scratch=_QUERY, sync=True):
    from adrefine import kernels as K
    from adrefine.native import lib
    monkeypatch.setenv("ADR_FIN_PRESUM", mode)
    dev = part.device
    scratch = _scratch(P, C, scratch, mode, dev)
    g = torch.linspace(0.5, 1.5, C, device=dev)
    dg, db, A, B, Cc = (torch.full((C,), float("nan"), device=dev) for _ in range(5))
    fp = K.fptr
    lib.adr_bn_bwd_finalize(fp(part), P, C, count, fp(mean), fp(rstd), fp(g), fp(dg), fp(db), fp(A), fp(B), fp(Cc), 1,
                            0, fp(scratch), K.stream())
    if sync:
        torch.cuda.synchronize()
    return dict(dgamma=dg, dbeta=db, A=A, B=B, C=Cc, g=g)


@pytest.mark.parametrize("P,C", SHAPES)
def test_bn_finalize_long_rows(monkeypatch, P, C):
    torch.manual_seed(P + C)
    rows = 128.0
    x1 = torch.randn(P, C, device="cuda") * 3 + 1.5               # per-row sums of 128 values
    x2 = x1 * x1 / rows + torch.rand(P, C, device="cuda") * rows  # sums of squares (>= sum^2 / n)
    part = torch.stack([x1, x2], 1).contiguous().view(-1)
    count = float(P * rows)
    if (P, C) in LONG:
        from adrefine.native import lib
        monkeypatch.setenv("ADR_FIN_PRESUM", "1")
        assert (lib.adr_bn_finalize_scratch_floats(P, C) != 0) == LONG[(P, C)]
    out = {m: _fwd(part, P, C, count, monkeypatch, m) for m in ("0", "1")}
    s1, s2 = x1.double().sum(0), x2.double().sum(0)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + 1e-3)
    for m, o in out.items():
        assert torch.isfinite(o["scale"]).all(), m
        torch.testing.assert_close(o["mean"].double(), mean, rtol=2e-6, atol=1e-7)
        torch.testing.assert_close(o["rstd"].double(), rstd, rtol=2e-6, atol=0)
        torch.testing.assert_close(o["scale"].double(), o["g"].double() * rstd, rtol=2e-6, atol=0)
        unb = var * count / (count - 1)
        torch.testing.assert_close(o["rv"].double(), 0.97 + 0.03 * unb, rtol=2e-6, atol=1e-7)
    for k in ("scale", "shift", "mean", "rstd"):
        torch.testing.assert_close(out["0"][k], out["1"][k], rtol=1e-6, atol=1e-7)

    # backward: partial rows (sum g, sum g * x) against the forward's mean / rstd
    gsum = torch.randn(P, C, device="cuda") * 2
    gx = torch.randn(P, C, device="cuda") * 5
    bpart = torch.stack([gsum, gx], 1).contiguous().view(-1)
    mu, rs = out["1"]["mean"], out["1"]["rstd"]
    bo = {m: _bwd(bpart, P, C, count, mu, rs, monkeypatch, m) for m in ("0", "1")}
    sg, sgxr = gsum.double().sum(0), gx.double().sum(0)
    sgx = (sgxr - mu.double() * sg) * rs.double()
    for m, o in bo.items():
        torch.testing.assert_close(o["dbeta"].double(), sg, rtol=1e-5, atol=1e-3)
        torch.testing.assert_close(o["dgamma"].double(), sgx, rtol=1e-5, atol=1e-3)
    # the sums are ~1e2 in magnitude from fp32 rows: the two orders differ by fp32 rounding of the pre-summed rows
    for k in ("dgamma", "dbeta"):
        torch.testing.assert_close(bo["0"][k], bo["1"][k], rtol=1e-5, atol=1e-4)
    for k in ("A", "B", "C"):
        torch.testing.assert_close(bo["0"][k], bo["1"][k], rtol=1e-5, atol=1e-9)


def test_bn_finalize_presum_deterministic(monkeypatch):
    """Two finalizes of the same long partials: bitwise equal (fixed split and order)."""
    torch.manual_seed(0)
    P, C = 12800, 32
    part = torch.randn(P * 2 * C, device="cuda").abs()
    a = _fwd(part, P, C, P * 128.0, monkeypatch, "1")
    b = _fwd(part, P, C, P * 128.0, monkeypatch, "1")
    for k in ("scale", "shift", "mean", "rstd"):
        assert torch.equal(a[k], b[k])


def _partials(P, C, seed):
    """Forward-like (sum, sum of squares) rows and backward-like (sum g, sum g * x) rows, as the test above."""
    torch.manual_seed(seed)
    x1 = torch.randn(P, C, device="cuda") * 3 + 1.5
    x2 = x1 * x1 / 128.0 + torch.rand(P, C, device="cuda") * 128.0
    gsum, gx = torch.randn(P, C, device="cuda") * 2, torch.randn(P, C, device="cuda") * 5
    return (torch.stack([x1, x2], 1).contiguous().view(-1), torch.stack([gsum, gx], 1).contiguous().view(-1))


_FWD_KEYS = ("scale", "shift", "mean", "rstd", "rm", "rv")
_BWD_KEYS = ("dgamma", "dbeta", "A", "B", "C")


@pytest.mark.parametrize("P,C", [(4097, 32), (2049, 256), (7777, 48)])
def test_bn_finalize_scratch_contract(monkeypatch, P, C):
    """A scratch of exactly the queried size, pre-filled with NaN and followed by 256 NaN guard floats: the results
    are bitwise those of a fresh zeroed scratch (every row the finalize reads was written by the pre-sum) and the
    guard stays NaN (nothing is written past the size contract)."""
    from adrefine.native import lib
    part, bpart = _partials(P, C, P + C)
    count = P * 128.0
    monkeypatch.setenv("ADR_FIN_PRESUM", "1")
    n = lib.adr_bn_finalize_scratch_floats(P, C)
    assert n == 256 * 2 * C
    ref = _fwd(part, P, C, count, monkeypatch, "1")
    bref = _bwd(bpart, P, C, count, ref["mean"], ref["rstd"], monkeypatch, "1")
    for fwd in (True, False):
        buf = torch.full((n + 256,), float("nan"), device="cuda")
        if fwd:
            got, want, keys = _fwd(part, P, C, count, monkeypatch, "1", scratch=buf[:n]), ref, _FWD_KEYS
        else:
            got = _bwd(bpart, P, C, count, ref["mean"], ref["rstd"], monkeypatch, "1", scratch=buf[:n])
            want, keys = bref, _BWD_KEYS
        for k in keys:
            assert torch.equal(got[k], want[k]), (fwd, k)
        assert torch.isnan(buf[n:]).all(), fwd


def test_bn_finalize_two_streams(monkeypatch):
    """Two long finalizes of different partials in flight on two streams, each with its own scratch: each is bitwise
    the same call made alone on the default stream."""
    (P1, C1), (P2, C2) = (12800, 32), (7777, 48)
    part1, _ = _partials(P1, C1, 1)
    part2, bpart2 = _partials(P2, C2, 2)
    f2 = _fwd(part2, P2, C2, P2 * 128.0, monkeypatch, "1")
    mu, rs = f2["mean"], f2["rstd"]
    alone = (_fwd(part1, P1, C1, P1 * 128.0, monkeypatch, "1"),
             _bwd(bpart2, P2, C2, P2 * 128.0, mu, rs, monkeypatch, "1"))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):  # inputs, outputs and scratch of each call are allocated on its own stream
        a = _fwd(part1, P1, C1, P1 * 128.0, monkeypatch, "1", sync=False)
    with torch.cuda.stream(s2):
        b = _bwd(bpart2, P2, C2, P2 * 128.0, mu, rs, monkeypatch, "1", sync=False)
    torch.cuda.synchronize()
    for k in _FWD_KEYS:
        assert torch.equal(a[k], alone[0][k]), k
    for k in _BWD_KEYS:
        assert torch.equal(b[k], alone[1][k]), k


def test_bn_finalize_no_scratch_is_single_launch(monkeypatch):
    """A long finalize handed no scratch is the single-launch finalize: bitwise ADR_FIN_PRESUM=0."""
    P, C = 12800, 32
    part, bpart = _partials(P, C, 3)
    count = P * 128.0
    f0 = _fwd(part, P, C, count, monkeypatch, "0")
    fn = _fwd(part, P, C, count, monkeypatch, "1", scratch=None)
    for k in _FWD_KEYS:
        assert torch.equal(fn[k], f0[k]), k
    b0 = _bwd(bpart, P, C, count, f0["mean"], f0["rstd"], monkeypatch, "0")
    bn = _bwd(bpart, P, C, count, f0["mean"], f0["rstd"], monkeypatch, "1", scratch=None)
    for k in _BWD_KEYS:
        assert torch.equal(bn[k], b0[k]), k
