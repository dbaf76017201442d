"""The batched entry points of the deferred parameter-gradient flush (one host scaffold, csrc/adr_common.h
launch_batches / batch_block), op by op: each is bitwise the immediate call include/adr.h documents it equal to, with
1 entry and with 100 (above every entry cap: several launches and a partial last one). The entries differ in size —
C over {8, 16, 24}, N over {1, 2}, HW over {5, 64, 130}, 1 or 3 chunks, 1 / 3 / 5 splits — the smallest shapes at which
a wrong start[] or block-local index reads another entry. Plus the three repeated-destination policies: GroupNorm
parameter gradients split the launch, partial sums and axpys reject."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

CS, NS, HWS = (8, 16, 24), (1, 2), (5, 64, 130)


def _shape(i):
    """(N, HW, C, rows_per_chunk, chunks) of entry i: every mix of the sizes, chunks 1 or 3."""
    C, N, HW = CS[i % 3], NS[i % 2], HWS[(i // 3) % 3]
    chunks = 1 if (i // 2) % 2 == 0 else 3
    rows = HW if chunks == 1 else -(-HW // 3)
    assert -(-HW // rows) == chunks
    return N, HW, C, rows, chunks


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _run(fn, T, entries, *extra):
    from adrefine import kernels as K
    fn((T * len(entries))(*entries), len(entries), *extra, K.stream())


def _f32(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.float32)


def _bf16(*shape):
    return torch.randn(*shape, device="cuda").to(torch.bfloat16)


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


@pytest.mark.parametrize("count", [1, 100])
def test_partial_sum_batched_bitwise(count):
    from adrefine import kernels as K
    lib = K.lib
    ents, got, ref, keep = [], [], [], []
    for i in range(count):
        P, C, which, acc = (1, 7, 300)[i % 3], CS[(i // 3) % 3], i % 2, (i // 2) % 2
        part, out = _f32(P, 2, C), _f32(C)
        want = out.clone()
        lib.adr_partial_sum(_p(part), P, C, which, _p(want), acc, K.stream())
        ents.append(K.PsumEntry(part.data_ptr(), out.data_ptr(), P, C, which, acc))
        got.append(out), ref.append(want), keep.append(part)
    _run(lib.adr_partial_sum_batched, K.PsumEntry, ents)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(g, r), i


@pytest.mark.parametrize("count", [1, 100])
def test_nc_reduce_batched_bitwise(count):
    from adrefine import kernels as K
    lib = K.lib
    ents, got, ref, keep = [], [], [], []
    for i in range(count):
        N, HW, C, rows, chunks = _shape(i)
        x = _bf16(N, HW, C)
        part, want = torch.full((N * chunks, 2, C), float("nan"), device="cuda"), torch.empty(N * chunks, 2, C, device="cuda")
        lib.adr_nc_reduce(K.BF16, 0, _p(x), C, 0, None, 0, 0, None, None, 0, 0, N, HW, C, rows, _p(want), K.stream())
        ents.append(K.ColsumEntry(x.data_ptr(), part.data_ptr(), C, N, HW, C, rows, chunks))
        got.append(part), ref.append(want), keep.append(x)
    _run(lib.adr_nc_reduce_batched, K.ColsumEntry, ents)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(g[:, 0], r[:, 0]), i  # the column sums (RED_STATS half 0; half 1: sums of squares)
        assert torch.equal(g[:, 1], r[:, 1]), i


def _gn_entry(K, i, dgamma=None, dbeta=None, acc=None):
    N, C = NS[i % 2], CS[(i // 2) % 3]
    G = C // 8
    part, mean, rstd = _f32(N, 2, C), _f32(N, G), _f32(N, G).abs() + 0.5
    dgamma = _f32(C) if dgamma is None else dgamma
    dbeta = _f32(C) if dbeta is None else dbeta
    acc = i % 2 if acc is None else acc
    e = K.GnParamEntry(part.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), N, 1, C,
                       G, acc, 0)
    return e, (part, mean, rstd), dgamma, dbeta


@pytest.mark.parametrize("count", [1, 100])
def test_gn_param_grad_batched_bitwise(count):
    from adrefine import kernels as K
    lib = K.lib
    ents, got, ref, keep = [], [], [], []
    for i in range(count):
        e, (part, mean, rstd), dg, db = _gn_entry(K, i)
        wg, wb = dg.clone(), db.clone()
        lib.adr_gn_param_grad(_p(part), e.N, e.C, e.G, _p(mean), _p(rstd), _p(wg), _p(wb), e.accumulate, K.stream())
        ents.append(e), got.append((dg, db)), ref.append((wg, wb)), keep.append((part, mean, rstd))
    _run(lib.adr_gn_param_grad_batched, K.GnParamEntry, ents)
    for i, ((dg, db), (wg, wb)) in enumerate(zip(got, ref)):
        assert torch.equal(dg, wg) and torch.equal(db, wb), i


def test_gn_param_grad_batched_splits_at_a_repeated_destination():
    """Entries 0 and 3 accumulate into the same dgamma / dbeta: the launch ends before entry 3, so the result is that
    of the entries issued one call at a time, in order."""
    from adrefine import kernels as K
    lib = K.lib
    C = CS[0]
    runs = []
    for batched in (True, False):
        torch.manual_seed(1)
        shared_g, shared_b = _f32(C), _f32(C)
        ents, outs, keep = [], [], []
        for i in range(5):
            rep = i in (0, 3)
            e, k, dg, db = _gn_entry(K, 0 if rep else i, shared_g if rep else None, shared_b if rep else None, acc=1)
            ents.append(e), outs.append((dg, db)), keep.append(k)
        if batched:
            _run(lib.adr_gn_param_grad_batched, K.GnParamEntry, ents)
        else:
            for e in ents:
                _run(lib.adr_gn_param_grad_batched, K.GnParamEntry, [e])
        torch.cuda.synchronize()
        runs.append(outs)
    for i, ((g0, b0), (g1, b1)) in enumerate(zip(*runs)):
        assert torch.equal(g0, g1) and torch.equal(b0, b1), i


@pytest.mark.parametrize("count", [1, 100])
def test_dotsum_batched_bitwise(count):
    from adrefine import kernels as K
    lib = K.lib
    ents, got, ref, keep = [], [], [], []
    for i in range(count):
        N, HW, C, rows, chunks = _shape(i)
        x, dz = _bf16(N, HW, C), _bf16(N, HW, C)
        part, wpart = torch.empty(N * chunks * 2 * C, device="cuda"), torch.empty(N * chunks * 2 * C, device="cuda")
        out, want = torch.full((1,), float("nan"), device="cuda"), torch.empty(1, device="cuda")
        lib.adr_dot_reduce(K.BF16, _p(x), C, _p(dz), C, N, HW, C, rows, _p(wpart), K.stream())
        lib.adr_nc_collapse(_p(wpart), N, chunks, C, 0, _p(want), 1, 1, 0, K.stream())
        ents.append(K.DotsumEntry(x.data_ptr(), dz.data_ptr(), part.data_ptr(), out.data_ptr(), C, C, N, HW, C, rows,
                                  chunks, 0))
        got.append(out), ref.append(want), keep.append((x, dz, part, wpart))
    _run(lib.adr_dotsum_batched, K.DotsumEntry, ents)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(g, r), i


@pytest.mark.parametrize("count", [1, 100])
def test_axpy_batched_bitwise(count):
    from adrefine import kernels as K
    lib = K.lib
    ents, got, ref, keep = [], [], [], []
    for i in range(count):
        n = (1, 1000, 1025, 5000)[i % 4]  # below, at and past one 1024-element block
        x, y = _f32(n), _f32(n)
        want = y.clone()
        lib.adr_axpy(n, 1.0, _p(x), _p(want), K.stream())
        ents.append(K.AxpyEntry(x.data_ptr(), y.data_ptr(), n))
        got.append(y), ref.append(want), keep.append(x)
    _run(lib.adr_axpy_batched, K.AxpyEntry, ents)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(g, r), i


@pytest.mark.parametrize("count", [1, 100])
def test_wgrad_reduce_batched_bitwise(count):
    from adrefine import kernels as K
    lib = K.lib
    ents, got, ref, keep = [], [], [], []
    for i in range(count):
        splits, Kc, (C, Cp), RS = (1, 3, 5)[i % 3], (3, 8)[i % 2], ((5, 8), (8, 8), (24, 24))[(i // 3) % 3], (1, 9)[(i // 2) % 2]
        tkc, acc = (i // 4) % 2, (i // 8) % 2
        n = Kc * RS * Cp
        part, dst = _f32(splits, n), _f32(Kc * C * RS)
        want = dst.clone()
        lib.adr_wgrad_reduce_unpack(_p(part), n, splits, _p(want), Kc, C, Cp, RS, tkc, acc, K.stream())
        ents.append(K.WgradEntry(part.data_ptr(), dst.data_ptr(), n, splits, Kc, C, Cp, RS, tkc, acc, 0))
        got.append(dst), ref.append(want), keep.append(part)
    _run(lib.adr_wgrad_reduce_batched, K.WgradEntry, ents)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(g, r), i


@pytest.mark.parametrize("pieces", [9, 20])
def test_copy_pieces_bitwise(pieces):
    from adrefine import kernels as K
    lib = K.lib
    npix = 2 * 65
    chans = [CS[i % 3] for i in range(pieces)]
    Ctot = sum(chans)
    out = torch.full((npix, Ctot), float("nan"), device="cuda", dtype=torch.bfloat16)
    ref = torch.empty_like(out)
    ents, keep, off = [], [], 0
    for i, c in enumerate(chans):
        scs = c + 8 * (i % 2)  # some sources are channel slices of a wider buffer
        src = _bf16(npix, scs)
        ref[:, off:off + c] = src[:, :c]
        ents.append(K.CopyPiece(src.data_ptr(), out.data_ptr() + 2 * off, scs, Ctot, c, 0))
        keep.append(src)
        off += c
    _run(lib.adr_copy_pieces, K.CopyPiece, ents, npix)
    assert torch.equal(out, ref)


def test_shared_destinations_are_rejected():
    """adr_partial_sum_batched and adr_axpy_batched refuse two entries of one launch with the same destination: an
    error return from the host-side check, before anything is launched."""
    from adrefine import kernels as K
    lib = K.lib
    part, out = _f32(4, 2, 8), _f32(8)
    before = out.clone()
    ents = [K.PsumEntry(part.data_ptr(), out.data_ptr(), 4, 8, w, 1) for w in (0, 1)]
    with pytest.raises(RuntimeError, match="share a destination"):
        _run(lib.adr_partial_sum_batched, K.PsumEntry, ents)
    x, y = _f32(100), _f32(100)
    ybefore = y.clone()
    with pytest.raises(RuntimeError, match="share a destination"):
        _run(lib.adr_axpy_batched, K.AxpyEntry, [K.AxpyEntry(x.data_ptr(), y.data_ptr(), 100)] * 2)
    assert torch.equal(out, before) and torch.equal(y, ybefore)
