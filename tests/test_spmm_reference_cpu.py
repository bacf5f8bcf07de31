"""CPU tier: tests/spmm_reference.py against a dense float64 product, scipy.sparse and torch's float64 autograd; the EXACT generator's
claim (the float64 result is an fp32 number, reached by fp32 arithmetic in any order); the row bound against an fp32 fmaf-chain
emulation in CSR order on RANDOM inputs (worst error / bound: 0.97 over the row lengths of the GPU module, printed with -s); and the
descriptor builders against the library's host planners on the same block-diagonal inputs."""
import ctypes
import zlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import spmm_reference as R


def _rng(*parts):
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


def _pattern(rng, n, n_cols, exact=False):
    lengths = rng.integers(0, 9, size=n)
    lengths[rng.random(n) < 0.2] = 0
    lengths[0] = 0
    lengths[-1] = min(40, n_cols)
    return R.make_csr(lengths, n_cols, rng, exact=exact)


@pytest.mark.parametrize("form", ["plain", "xrow", "xrow_zero", "compact"])
def test_spmm_against_dense_and_scipy(form):
    rng = _rng("dense", form)
    n, n_cols, H, n_tab = 60, 50, 7, 23
    rowptr, col, val = _pattern(rng, n, n_cols)
    assert all(np.all(np.diff(col[rowptr[r]:rowptr[r + 1]]) > 0) for r in range(n)), "columns ascend within a row"
    A = np.zeros((n, n_cols))
    A[np.repeat(np.arange(n), np.diff(rowptr)), col] = val.astype(np.float64)
    if form == "plain":
        X = rng.normal(size=(n_cols, H)).astype(np.float32)
        Xe, args = X.astype(np.float64), {}
    elif form == "compact":                                     # the column IS the operand row; rows >= 20 do not exist
        X = rng.normal(size=(20, H)).astype(np.float32)
        Xe = np.zeros((n_cols, H))
        Xe[:20] = X
        args = {"zero_from": 20}
    else:
        X = rng.normal(size=(n_tab, H)).astype(np.float32)
        xrow = rng.integers(0, n_tab, size=n_cols)
        zf = 15 if form == "xrow_zero" else -1
        Xe = X.astype(np.float64)[xrow]
        if zf >= 0:
            Xe[xrow >= zf] = 0.0
        args = {"xrow": xrow, "zero_from": zf}
    Y, S = R.spmm(rowptr, col, val, X, **args)
    assert np.allclose(Y, A @ Xe, rtol=1e-13, atol=1e-13) and np.allclose(S, np.abs(A) @ np.abs(Xe), rtol=1e-13, atol=1e-13)
    M = sp.csr_matrix((val.astype(np.float64), col, rowptr), shape=(n, n_cols))
    assert np.allclose(Y, M @ Xe, rtol=1e-13, atol=1e-13)
    assert np.all(Y[np.diff(rowptr) == 0] == 0), "an empty row is a row of zeros"


@pytest.mark.parametrize("epi", [0, R.sr.EPI_ELU, R.sr.EPI_DROPOUT, R.sr.EPI_ELU | R.sr.EPI_DROPOUT])
def test_epilogues_against_autograd(epi):
    rng = _rng("epi", epi)
    n, H = 40, 12
    z = rng.normal(size=(n, H))
    bias = rng.normal(size=H)
    keep = R.keep_by_hash(1234567, rng.permutation(100)[:n], H)
    assert 0.3 < keep.mean() < 0.7
    zt = torch.tensor(z, requires_grad=True)
    y = zt + torch.tensor(bias)
    if epi & R.sr.EPI_ELU:
        y = torch.nn.functional.elu(y)
    if epi & R.sr.EPI_DROPOUT:
        y = y * torch.tensor(keep) * 2.0
    out = R.forward(z, bias, epi | R.sr.EPI_BIAS, 0.5, keep)
    assert np.allclose(out, y.detach().numpy(), rtol=1e-14, atol=1e-15)
    g = rng.normal(size=(n, H))
    y.backward(torch.tensor(g))
    dZ, f = R.backward(g, out, epi, 0.5, keep)
    assert np.allclose(dZ, zt.grad.numpy(), rtol=1e-13, atol=1e-15) and np.array_equal(dZ, g * f)
    s, a = R.colsums(dZ, [[0, 10], [10, 10], [10, 40]])
    assert np.allclose(s.sum(0), dZ.sum(0)) and np.all(s[1] == 0) and np.allclose(a[2], np.abs(dZ[10:]).sum(0))


def _length_cases():
    return [("tile", R.cycle(R.TILE_LENGTHS, 48)), ("short", R.cycle([0, 1, 2, 4, 5, 9], 60)), ("hubs", np.array([3, 64, 65, 130, 200, 1, 0, 67]))]


@pytest.mark.parametrize("name,lengths", _length_cases(), ids=[c[0] for c in _length_cases()])
def test_exact_inputs_are_exact_in_any_order(name, lengths):
    rng = _rng("exact", name)
    n_cols, H = 320, 12
    rowptr, col, val = R.make_csr(lengths, n_cols, rng, exact=True)
    X = R.exact_signal(rng, (n_cols, H))
    Y, _ = R.spmm(rowptr, col, val, X)
    assert np.array_equal(Y, Y.astype(np.float32).astype(np.float64)), "the float64 result is not an fp32 number"
    for order in ("csr", "reverse", "first4"):
        assert np.array_equal(R.chain_f32(rowptr, col, val, X, order).astype(np.float64), Y), order
    # the epilogues on top: bias integers over 8, p = 0.5; ELU exact above zero; dZ and its certified column sums
    bias = (rng.integers(-8, 9, size=H) / 8.0).astype(np.float32)
    keep = rng.random(Y.shape) < 0.5
    out = R.forward(Y, bias, R.sr.EPI_BIAS | R.sr.EPI_DROPOUT, 0.5, keep)
    f32 = np.float32
    emu = np.where(keep, (Y.astype(f32) + bias[None, :]).astype(f32) * f32(2.0), f32(0.0))
    assert np.array_equal(out, emu.astype(np.float64))
    prev = R.exact_signal(rng, Y.shape)
    dZ, _ = R.backward(Y, prev, R.sr.EPI_ELU | R.sr.EPI_DROPOUT, 0.5, keep)
    e = (prev * f32(0.5)).astype(f32)
    d = (Y.astype(f32) * f32(2.0)).astype(f32)
    emu = np.where(keep, np.where(e > 0, d, (d * (e + f32(1.0)).astype(f32)).astype(f32)), f32(0.0))
    assert np.array_equal(dZ, emu.astype(np.float64))
    ranges = [[0, len(lengths)]]
    s, a = R.colsums(dZ, ranges)
    ok = R.colsum_is_exact(a, lengths.max())[0]
    assert ok.all(), "the EXACT column sums of these shapes are all certified"
    for perm in (np.arange(len(lengths)), np.arange(len(lengths))[::-1], rng.permutation(len(lengths))):
        acc = np.zeros(H, dtype=f32)
        for r in perm:
            acc = (acc + dZ[r].astype(f32)).astype(f32)
        assert np.array_equal(acc.astype(np.float64), s[0])


def test_fmaf_chain_stays_within_the_row_bound(capsys):
    worst = 0.0
    for name, lengths in _length_cases():
        rng = _rng("chain", name)
        n_cols, H = 320, 64
        rowptr, col, val = R.make_csr(lengths, n_cols, rng)
        assert np.all((np.abs(val) >= 0.05 - 1e-7) & (np.abs(val) <= 1.0))
        X = rng.normal(size=(n_cols, H)).astype(np.float32)
        Y, S = R.spmm(rowptr, col, val, X)
        bound = R.row_bound(rowptr, S)
        for order in ("csr", "first4"):
            err = np.abs(R.chain_f32(rowptr, col, val, X, order).astype(np.float64) - Y)
            assert np.all(err <= bound), (name, order)
            pos = bound > 0
            worst = max(worst, float((err[pos] / bound[pos]).max()))
        assert np.all(Y[lengths == 0] == 0) and np.all(bound[lengths == 0] == 0)
    with capsys.disabled():
        print(f"\n[ratio] fp32 fmaf chain in CSR order / row bound: {worst:.3g}")
    assert 0.05 < worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the builders against the host planners
# ---------------------------------------------------------------------------------------------------------------------------------
def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _block_diagonal(rng, sizes, hub_len=40):
    """A block-diagonal pattern: every row draws from its own block; the first row of a block of more than 20 rows is a hub."""
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(ptr[-1])
    lo = np.repeat(ptr[:-1], sizes)
    hi = np.repeat(ptr[1:], sizes)
    lengths = np.minimum(rng.integers(0, 6, size=n), hi - lo)
    for b, sz in enumerate(sizes):
        if sz > 20:
            lengths[ptr[b]] = min(hub_len, sz)
    return ptr, R.make_csr(lengths, n, rng, lo=lo, hi=hi)


SIZES = [3, 5, 16, 1, 40, 2, 2, 17, 100, 7, 9, 300, 4]


def test_pack_tiles_equals_make_tiles_host():
    from fitgnn_amd import _lib
    L = _lib.lib()
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    for max_rows in (1, 8, 16, 96):
        buf = np.zeros((len(SIZES) + int(ptr[-1]) // max_rows + 2, 4), dtype=np.int32)
        nt = ctypes.c_int64(0)
        assert L.fitgnn_make_tiles_host(_vp(ptr), len(SIZES), max_rows, _vp(buf), len(buf), ctypes.byref(nt)) == 0
        mine = R.pack_tiles(ptr, max_rows)
        assert [tuple(r) for r in buf[:nt.value].tolist()] == mine
        (rowptr, _, _) = _block_diagonal(_rng("pack"), SIZES)[1]
        recs = R.tile_records(rowptr, mine + [None])
        assert np.array_equal(recs[:-1, :4], buf[:nt.value]) and np.all(recs[-1] == 0)
        assert np.array_equal(recs[:-1, 4], rowptr[recs[:-1, 0]]) and np.array_equal(recs[:-1, 5], rowptr[recs[:-1, 1]])


def test_block_records_equal_split_blocks_host():
    from fitgnn_amd import _lib
    L = _lib.lib()
    ptr, (rowptr, col, val) = _block_diagonal(_rng("split"), SIZES)
    n = int(ptr[-1])
    for cap, limit, long_row in ((16, 128, 16), (16, 1000, 4), (4, 50, 2)):
        tiles4 = np.zeros((len(SIZES) + n // cap + 2, 4), dtype=np.int32)
        blocks = np.zeros((len(SIZES), 8), dtype=np.int32)
        longs = np.zeros(n, dtype=np.int32)
        nt, nl, nlong = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        assert L.fitgnn_split_blocks_host(_vp(ptr), len(SIZES), _vp(rowptr), cap, limit, long_row, _vp(tiles4), len(tiles4), ctypes.byref(nt),
                                          _vp(blocks), ctypes.byref(nl), _vp(longs), len(longs), ctypes.byref(nlong)) == 0
        t, b, lr = R.split_blocks(ptr, rowptr, cap, limit, long_row)
        assert [tuple(r) for r in tiles4[:nt.value].tolist()] == t
        assert np.array_equal(blocks[:nl.value], b) and np.array_equal(longs[:nlong.value], lr)
        assert nl.value > 0 and nlong.value > 0
    # by hand: listed long rows, an empty record
    b, lr = R.block_records(rowptr, [(0, 8), None, (8, 25)], long_rows={0: [5, 2], 2: [8]})
    assert b.tolist() == [[0, 8, 0, rowptr[8], 0, 2, 0, 0], [0] * 8, [8, 25, rowptr[8], rowptr[25], 2, 1, 0, 0]] and lr.tolist() == [2, 5, 8]


def test_planned_windows_resolve_to_the_entries_columns():
    from fitgnn_amd import _lib
    L = _lib.lib()
    ptr, (rowptr, col, val) = _block_diagonal(_rng("plan"), SIZES)
    n, nnz = int(ptr[-1]), int(rowptr[-1])
    # the host planner: contiguous windows for the packed small blocks, column-set windows for the large ones
    tiles = np.zeros((n, 8), dtype=np.int32)
    win, lcol = np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=np.int32)
    nt, nw = ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.fitgnn_plan_tiles_host(_vp(rowptr), _vp(col), n, n, _vp(ptr), len(SIZES), 16, 16, _vp(tiles), ctypes.byref(nt), _vp(win),
                                    ctypes.byref(nw), _vp(lcol)) == 0
    tiles = tiles[:nt.value]
    assert tiles[0, 0] == 0 and tiles[-1, 1] == n and np.array_equal(tiles[1:, 0], tiles[:-1, 1]) and tiles[:, 6].any() and not tiles[:, 6].all()
    assert np.array_equal(R.resolve_lcol(tiles, win, lcol, rowptr), col)
    # the builder on the planner's own tiling reproduces lcol wherever the planner staged the row (it may also leave a row unstaged)
    specs = [(int(t[0]), int(t[1]), [int(v) for v in win[t[2]:t[2] + t[3]]] if t[6] else (int(t[2]), int(t[3]))) for t in tiles]
    mt, mw, ml = R.plan_windows(rowptr, col, specs)
    assert np.array_equal(mt[:, [0, 1, 3, 4, 5, 6, 7]], tiles[:, [0, 1, 3, 4, 5, 6, 7]])
    assert np.array_equal(R.resolve_lcol(mt, mw, ml, rowptr), col)
    staged = lcol >= 0
    assert staged.any() and np.array_equal(ml[staged], lcol[staged])
    # a hand-made plan: a listed window that misses columns, a contiguous one, an empty record, rows left out
    mt, mw, ml = R.plan_windows(rowptr, col, [(0, 8, [0, 3, 4]), None, (8, 25, (10, 6))])
    res = R.resolve_lcol(mt, mw, ml, rowptr)
    e = int(rowptr[25])
    assert np.array_equal(res[:e], col[:e]) and np.all(res[e:] == -1) and (ml[:e] < 0).any() and (ml[:e] >= 0).any()


def test_segments():
    sp_, rs = R.segments([1, 5, 70, 2], [2, 0, 2])
    assert sp_.tolist() == [0, 1, 6, 76, 78] and rs.tolist() == [0, 2, 2, 4]
