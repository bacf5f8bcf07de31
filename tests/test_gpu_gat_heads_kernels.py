"""GPU tier: the multi-head attention kernels of csrc/gat_heads.hip through the C ABI against the float64 statements of
tests/gat_heads_reference.py, with the two regimes of tests/test_gpu_gat_kernels.py.

EXACT inputs (small integers, multiples of 1/4 or 1/64, slopes 0.25 / 0.5) keep every fp32 partial result exact, so a kernel must
return the float64 result bit for bit whatever its summation order: a dropped, doubled or misplaced entry of a 1 000-entry row, or a
head's sum that leaks into its neighbour's lanes, cannot hide under a tolerance.  RANDOM inputs are held per output to
k * 2^-24 * (sum of |terms| of that output), k the number of terms in the longest chain of roundings:
  scores, sddmm   C / 64 + 16   (a lane adds at most C / 64 + 4 products of a head in turn, then at most six butterfly steps; as
                                 test_gpu_gat_kernels.py derives it for one head)
  aggregate       len + 2       (one fused multiply-add per entry in CSR order, then the bias)
  softmax_bwd     len / 64 + 24 (the single-head test's bound, per head)
The edge softmax has no exact regime (__expf): per-entry relative error 1e-4 as for one head, and every (row, head) sums to 1 within
(len / 64 + 16) * 2^-24 (the sum z of a lane's len / 64 terms and six butterfly steps, its reciprocal, one product per entry).

Shapes: row lengths {0, 1, 2, 7, 8, 9, 63, 64, 65, 128, 129, 1000} in the mixes isolated, hub, several_per_wave and hub_in_leaves;
n in {1, 3, 4, 5, 255, 256, 257}; (heads, C) at every lane mapping listed beside HC below: heads sharing a 64-lane slot, a head
filling one slot, a head spanning two and four register slots, the width limit, scores beyond it, a head count that does not divide
the wave, the aggregate's float4 path with a non-power-of-two C / 4, one head, the scalar paths; a leading dimension above W and a
pointer one float past a 16-byte boundary."""
import numpy as np
import pytest
import torch

import gat_heads_reference as ghr
import gat_reference as gr
from test_gpu_gat_kernels import U, _check_softmax, _dev_csr, _exact_bwd_inputs, _f32, _seed, _strided

pytestmark = pytest.mark.gpu

# (heads, C), by lane mapping of the float4 kernels (L = C / 4 lanes per head):
#   (2, 4) (8, 8) (8, 64)      L = 1, 2, 16: several heads share a 64-lane slot
#   (4, 256) (16, 64)          L = 64: a head fills exactly one slot; W = 1024, the register-path width limit, MAXV = 4
#   (1, 512) (2, 512) (1, 1024)  L = 128, 128, 256: a head SPANS 2, 2, 4 register slots (slots added in the lane before the butterfly;
#                              MAXV = 2 with one head, MAXV = 4 with writer slots 0 and 2, MAXV = 4 with one writer slot)
#   (4, 512)                   W = 2048: scores still takes its float4 path (no width limit: slots 2k, 2k + 1 per head), aggregate and
#                              SDDMM their scalar kernels
#   (3, 32)                    a head count that does not divide the wave
#   (3, 12) (5, 20)            C % 4 == 0 with L = 3, 5 not a power of two: the aggregate's float4 path with heads that do not align to
#                              lane groups (hd = c / C per lane); scores and SDDMM take their scalar path
#   (1, 64)                    one head: the single-head kernels' bits
#   (2, 3) (5, 7) (3, 1)       C % 4 != 0: the scalar path everywhere
#   (2, 516)                   C % 4 == 0 past the register width (and L = 129): the scalar path
HC = [(2, 4), (8, 8), (8, 64), (4, 256), (16, 64), (1, 512), (2, 512), (1, 1024), (4, 512), (3, 32), (3, 12), (5, 20), (1, 64), (2, 3),
      (5, 7), (3, 1), (2, 516)]
HC_IDS = [f"{h}x{c}" for h, c in HC]
BRANCH_LENS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 128, 129, 1000]
ROW_CASES = ["isolated", "hub", "several_per_wave", "hub_in_leaves"]
N_CASES = [1, 3, 4, 5, 255, 256, 257]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from fitgnn_amd import _lib
    return _lib


def _run(L, fn, *args):
    L.check(getattr(L.lib(), fn)(*args, L.stream_ptr()), fn)
    torch.cuda.synchronize()


def _row_lengths(case, rng):
    if case == "isolated":            # n = 3: a row without entries, a self loop only, a pair
        return np.array([0, 1, 2])
    if case == "hub":                 # n = 1, one row of 1 000 entries
        return np.array([1000])
    if case == "several_per_wave":    # n = 257: every branch length once among short rows; waves with no, one and several long rows
        lens = rng.integers(0, 9, size=257)
        lens[np.linspace(66, 250, len(BRANCH_LENS)).astype(int)] = BRANCH_LENS
        lens[[3, 4, 6]] = [9, 129, 64]
        lens[256] = 65
        return lens
    if case == "hub_in_leaves":       # n = 255: a 1 000-entry row in a wave of leaves, two long neighbours
        lens = rng.integers(1, 5, size=255)
        lens[150], lens[151], lens[152] = 1000, 65, 129
        return lens
    raise ValueError(case)


def _lens_for_n(n, rng):
    """Rows of 0 to 9 entries, and from n = 3 on one row of 65 and one of 7 at the ends (the last wave's last lanes)."""
    lens = rng.integers(0, 10, size=n)
    if n >= 3:
        lens[n - 1], lens[0] = 65, 7
    return lens


def _n_cols(n):
    return max(n, 300)


def _csr(lens, n_cols, rng):
    rowptr = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    return rowptr, rng.integers(0, n_cols, size=int(rowptr[-1]))


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _np(t):
    return t.cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# launchers
# ---------------------------------------------------------------------------------------------------------------------------------
def _scores(L, hv, att_s, att_d, heads, C):
    n = hv.shape[0]
    a_s, a_d = _nan(n, heads), _nan(n, heads)
    _run(L, "fitgnn_gat_heads_scores_f32", L.dptr(hv), hv.stride(0), n, heads, C, L.dptr(att_s), L.dptr(att_d), L.dptr(a_s), L.dptr(a_d))
    return a_s, a_d


def _softmax(L, rowptr, col, a_s, a_d, slope):
    rp, cl = _dev_csr(rowptr, col)
    a_s, a_d = _f32(a_s), _f32(a_d)
    heads = a_s.shape[1]
    alpha = _nan(len(col), heads)
    _run(L, "fitgnn_gat_heads_edge_softmax_f32", L.dptr(rp), L.dptr(cl), L.dptr(a_s), L.dptr(a_d), float(slope), len(rowptr) - 1, len(col),
         heads, L.dptr(alpha))
    return alpha


def _aggregate(L, rowptr, col, alpha, Xv, heads, C, bias=None, ldy=None, y_offset=0):
    rp, cl = _dev_csr(rowptr, col)
    n = len(rowptr) - 1
    al = _f32(alpha)
    W = heads * C
    Y = _strided(np.full((n, W), np.nan, dtype=np.float32), ldy or W, offset=y_offset)
    b = None if bias is None else _f32(bias)
    _run(L, "fitgnn_gat_heads_aggregate_f32", L.dptr(rp), L.dptr(cl), L.dptr(al), L.dptr(Xv), Xv.stride(0), L.dptr(Y), Y.stride(0), n, len(col),
         heads, C, L.dptr(b))
    return Y


def _sddmm(L, rowptr, col, dv, hv, heads, C):
    rp, cl = _dev_csr(rowptr, col)
    dalpha = _nan(len(col), heads)
    _run(L, "fitgnn_gat_heads_sddmm_f32", L.dptr(rp), L.dptr(cl), L.dptr(dv), dv.stride(0), L.dptr(hv), hv.stride(0), len(rowptr) - 1, len(col),
         heads, C, L.dptr(dalpha))
    return dalpha


def _softmax_bwd(L, rowptr, col, a_s, a_d, alpha, dalpha, slope):
    rp, cl = _dev_csr(rowptr, col)
    n = len(rowptr) - 1
    ins = [_f32(a) for a in (a_s, a_d, alpha, dalpha)]
    heads = ins[0].shape[1]
    ds, da_dst = _nan(len(col), heads), _nan(n, heads)
    _run(L, "fitgnn_gat_heads_softmax_bwd_f32", L.dptr(rp), L.dptr(cl), *[L.dptr(t) for t in ins], float(slope), n, len(col), heads,
         L.dptr(ds), L.dptr(da_dst))
    return ds, da_dst


def _cases():
    """(id, lens maker) over the four row mixes and the seven row counts."""
    out = [(c, lambda rng, c=c: _row_lengths(c, rng)) for c in ROW_CASES]
    out += [(f"n{n}", lambda rng, n=n: _lens_for_n(n, rng)) for n in N_CASES]
    return out


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]
# every (heads, C) on the four row mixes; the row counts with a power-of-two mapping and the generic one
GRID = [(hc, case) for hc in HC for case in CASES[:4]] + [(hc, case) for hc in [(8, 8), (5, 7)] for case in CASES[4:]]
GRID_IDS = [f"{h}x{c}-{case[0]}" for (h, c), case in GRID]


# ---------------------------------------------------------------------------------------------------------------------------------
# scores
# ---------------------------------------------------------------------------------------------------------------------------------
def _score_inputs(n, W, rng, exact):
    if exact:
        return (rng.integers(-8, 9, size=(n, W)).astype(np.float32), rng.integers(-64, 65, size=W) / 64.0,
                rng.integers(-64, 65, size=W) / 64.0)
    return (rng.standard_normal((n, W)).astype(np.float32), rng.standard_normal(W).astype(np.float32),
            rng.standard_normal(W).astype(np.float32))


def _check_scores(L, h, att_s, att_d, heads, C, exact, what, ld=None, offset=0):
    hv = _strided(h, ld or h.shape[1], offset=offset)
    s, d = _f32(att_s), _f32(att_d)
    a_s, a_d = _scores(L, hv, s, d, heads, C)
    ref_s, ref_d, cs, cd = ghr.scores(h, att_s, att_d, heads)
    got_s, got_d = _np(a_s), _np(a_d)
    if exact:
        assert np.array_equal(got_s, ref_s) and np.array_equal(got_d, ref_d), what
    else:
        k = C / 64 + 16
        assert np.all(np.abs(got_s - ref_s) <= k * U * cs), (what, float(np.max(np.abs(got_s - ref_s) / np.maximum(cs, 1e-300))))
        assert np.all(np.abs(got_d - ref_d) <= k * U * cd), (what, float(np.max(np.abs(got_d - ref_d) / np.maximum(cd, 1e-300))))
    a2, d2 = _scores(L, hv, s, d, heads, C)
    assert torch.equal(a2, a_s) and torch.equal(d2, a_d), (what, "two launches gave different bits")
    return a_s, a_d


@pytest.mark.parametrize("heads,C", HC, ids=HC_IDS)
@pytest.mark.parametrize("n", N_CASES)
def test_scores(L, heads, C, n):
    rng = np.random.default_rng(_seed("scores", heads, C, n))
    for exact in (True, False):
        h, att_s, att_d = _score_inputs(n, heads * C, rng, exact)
        _check_scores(L, h, att_s, att_d, heads, C, exact, (heads, C, n, exact))


@pytest.mark.parametrize("ld_extra,offset", [(4, 0), (3, 0), (0, 1)], ids=["ld_W+4", "ld_W+3_scalar", "misaligned_scalar"])
def test_scores_strides_and_alignment(L, ld_extra, offset):
    """A leading dimension above W (NaN in the padding: a read past column W poisons the result) that is and is not a multiple of
    4, and h one float past a 16-byte boundary: the last two take the scalar path."""
    heads, C, n = 8, 8, 67
    rng = np.random.default_rng(_seed("scores-ld", ld_extra, offset))
    for exact in (True, False):
        h, att_s, att_d = _score_inputs(n, heads * C, rng, exact)
        _check_scores(L, h, att_s, att_d, heads, C, exact, (ld_extra, offset, exact), ld=heads * C + ld_extra, offset=offset)


def test_scores_one_head_has_the_single_head_kernels_bits(L):
    rng = np.random.default_rng(5)
    h, att_s, att_d = _score_inputs(67, 64, rng, True)
    hv, s, d = _strided(h, 64), _f32(att_s), _f32(att_d)
    a_s, a_d = _scores(L, hv, s, d, 1, 64)
    o_s, o_d = _nan(67), _nan(67)
    _run(L, "fitgnn_gat_scores_f32", L.dptr(hv), 64, 67, 64, L.dptr(s), L.dptr(d), L.dptr(o_s), L.dptr(o_d))
    assert torch.equal(a_s[:, 0], o_s) and torch.equal(a_d[:, 0], o_d)


# ---------------------------------------------------------------------------------------------------------------------------------
# edge softmax
# ---------------------------------------------------------------------------------------------------------------------------------
HEADS_ONLY = [1, 2, 3, 5, 8, 16]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("heads", HEADS_ONLY)
def test_edge_softmax(L, heads, case):
    """Per-entry relative error <= 1e-4 wherever alpha >= 1e-30, in a flat regime (every entry matters) and a wide one (a dominant
    entry, both LeakyReLU branches down to exp underflow); every (row, head) with entries sums to 1; rows without entries write
    nothing (the NaN sentinel of their neighbours' entries is never touched: there are none) and nothing divides by zero."""
    for regime, slope in (("flat", 0.2), ("wide", 0.2), ("flat", 0.0)):
        rng = np.random.default_rng(_seed("softmax", heads, case[0], regime, slope))
        lens = case[1](rng)
        n = len(lens)
        rowptr, col = _csr(lens, _n_cols(n), rng)
        if regime == "flat":
            a_s, a_d = rng.standard_normal((_n_cols(n), heads)), rng.standard_normal((n, heads))
        else:
            a_s, a_d = rng.uniform(-450.0, 20.0, size=(_n_cols(n), heads)), rng.uniform(-2.0, 2.0, size=(n, heads))
            for r in np.nonzero(lens > 8)[0]:   # the dominant score on entry 8, 9, 64 or the last, by head
                for hd in range(heads):
                    pos = [p for p in (8, 9, 64, lens[r] - 1) if p < lens[r]]
                    a_s[col[rowptr[r] + pos[hd % len(pos)]], hd] = 24.0
        a_s, a_d = a_s.astype(np.float32), a_d.astype(np.float32)
        alpha = _softmax(L, rowptr, col, a_s, a_d, slope)
        got = _np(alpha)
        assert not np.isnan(got).any(), "an entry was not written"
        ref = ghr.edge_softmax(rowptr, col, a_s, a_d, slope)
        _check_softmax(got.reshape(-1), ref.reshape(-1), (heads, case[0], regime, slope))
        rows = gr.entry_rows(rowptr)
        for hd in range(heads):
            tot = np.bincount(rows, weights=got[:, hd], minlength=n)
            k = lens / 64.0 + 16
            assert np.all(np.abs(tot[lens > 0] - 1.0) <= (k * U)[lens > 0]), (heads, case[0], regime, hd)
            assert np.all(tot[lens == 0] == 0.0)
        assert torch.equal(_softmax(L, rowptr, col, a_s, a_d, slope), alpha), "two launches gave different bits"


def test_edge_softmax_one_head_has_the_single_head_kernels_bits(L):
    rng = np.random.default_rng(6)
    lens = _row_lengths("several_per_wave", rng)
    n = len(lens)
    rowptr, col = _csr(lens, _n_cols(n), rng)
    a_s, a_d = rng.standard_normal((_n_cols(n), 1)).astype(np.float32), rng.standard_normal((n, 1)).astype(np.float32)
    alpha = _softmax(L, rowptr, col, a_s, a_d, 0.2)
    rp, cl = _dev_csr(rowptr, col)
    s1, d1 = _f32(a_s[:, 0]), _f32(a_d[:, 0])
    old = _nan(len(col))
    _run(L, "fitgnn_gat_edge_softmax_f32", L.dptr(rp), L.dptr(cl), L.dptr(s1), L.dptr(d1), 0.2, n, L.dptr(old))
    assert torch.equal(alpha[:, 0], old)


# ---------------------------------------------------------------------------------------------------------------------------------
# aggregate
# ---------------------------------------------------------------------------------------------------------------------------------
def _aggregate_inputs(nnz, n_cols, heads, C, rng, exact):
    W = heads * C
    if exact:   # alpha = k / 4, X and bias small integers: every partial sum of a 1 000-entry row is an exact multiple of 1/4
        return (rng.integers(0, 4, size=(nnz, heads)) / 4.0, rng.integers(-3, 4, size=(n_cols, W)).astype(np.float64),
                rng.integers(-5, 6, size=W).astype(np.float64))
    return (rng.uniform(0.0, 1.0, size=(nnz, heads)).astype(np.float32), rng.standard_normal((n_cols, W)).astype(np.float32),
            rng.standard_normal(W).astype(np.float32))


def _check_aggregate(L, lens, heads, C, rng, exact, what, with_bias=True, ld_extra=0, offset=0):
    n, W = len(lens), heads * C
    rowptr, col = _csr(lens, _n_cols(n), rng)
    alpha, X, bias = _aggregate_inputs(len(col), _n_cols(n), heads, C, rng, exact)
    if not with_bias:
        bias = None
    Xv = _strided(X, W + ld_extra, offset=offset)
    Y = _aggregate(L, rowptr, col, alpha, Xv, heads, C, bias=bias, ldy=W + ld_extra, y_offset=offset)
    ref, cond = ghr.aggregate(rowptr, col, alpha, X, bias)
    got = _np(Y)
    assert not np.isnan(got).any(), (what, "an output was not written")
    if exact:
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (what, "not bit-exact", bad[:6].tolist())
    else:
        k = (np.asarray(lens) + 2)[:, None]
        assert np.all(np.abs(got - ref) <= k * U * cond + 1e-38), (what, float(np.max(np.abs(got - ref) / (cond + 1e-38))))
    Y2 = _aggregate(L, rowptr, col, alpha, Xv, heads, C, bias=bias, ldy=W + ld_extra, y_offset=offset)
    assert torch.equal(Y2, Y), (what, "two launches gave different bits")


@pytest.mark.parametrize("hc,case", GRID, ids=GRID_IDS)
def test_aggregate(L, hc, case):
    heads, C = hc
    for exact in (True, False):
        rng = np.random.default_rng(_seed("aggregate", heads, C, case[0], exact))
        _check_aggregate(L, case[1](rng), heads, C, rng, exact, (heads, C, case[0], exact), with_bias=exact)


@pytest.mark.parametrize("ld_extra,offset", [(4, 0), (3, 0), (0, 1)], ids=["ld_W+4", "ld_W+3_scalar", "misaligned_scalar"])
def test_aggregate_strides_and_alignment(L, ld_extra, offset):
    for exact in (True, False):
        rng = np.random.default_rng(_seed("aggregate-ld", ld_extra, offset, exact))
        _check_aggregate(L, _row_lengths("hub_in_leaves", rng), 8, 8, rng, exact, (ld_extra, offset, exact), ld_extra=ld_extra, offset=offset)


@pytest.mark.parametrize("heads,C", [(8, 8), (4, 256), (5, 7), (2, 516)], ids=["8x8", "4x256", "5x7", "2x516"])
def test_aggregate_on_the_transposed_pattern_is_the_adjoint(L, heads, C):
    """<Y, A X> = <A^T Y, X> with A^T applied as the same entry point on the transposed pattern with alpha[perm_t]: within
    2 (longest row or column + 2) u sum |Y| alpha |X|."""
    rng = np.random.default_rng(_seed("adjoint", heads, C))
    lens = _row_lengths("hub_in_leaves", rng)
    n = len(lens)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    col = rng.integers(0, n, size=int(rowptr[-1]))          # square
    alpha = rng.uniform(0.0, 1.0, size=(len(col), heads)).astype(np.float32)
    X, Yv = rng.standard_normal((n, heads * C)).astype(np.float32), rng.standard_normal((n, heads * C)).astype(np.float32)
    rowptr_t, col_t, perm = gr.transpose(rowptr, col, n)
    AX = _np(_aggregate(L, rowptr, col, alpha, _strided(X, heads * C), heads, C))
    ATY = _np(_aggregate(L, rowptr_t, col_t, alpha[perm], _strided(Yv, heads * C), heads, C))
    lhs, rhs = float((Yv.astype(np.float64) * AX).sum()), float((ATY * X.astype(np.float64)).sum())
    _, cond = ghr.aggregate(rowptr, col, alpha, np.abs(X))
    bound = 2 * (max(lens.max(), np.diff(rowptr_t).max()) + 2) * U * float((np.abs(Yv) * cond).sum())
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# SDDMM
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_sddmm(L, lens, heads, C, rng, exact, what, ld_extra=0, offset=0):
    n, W = len(lens), heads * C
    rowptr, col = _csr(lens, _n_cols(n), rng)
    if exact:   # products are multiples of 1/4
        dout, h = rng.integers(-3, 4, size=(n, W)) / 4.0, rng.integers(-3, 4, size=(_n_cols(n), W)).astype(np.float64)
    else:
        dout, h = rng.standard_normal((n, W)), rng.standard_normal((_n_cols(n), W))
    dout, h = dout.astype(np.float32), h.astype(np.float32)
    dv, hv = _strided(dout, W + ld_extra, offset=offset), _strided(h, W + ld_extra, offset=offset)
    dalpha = _sddmm(L, rowptr, col, dv, hv, heads, C)
    ref, cond = ghr.sddmm(rowptr, col, dout, h, heads)
    got = _np(dalpha)
    assert not np.isnan(got).any(), (what, "an entry was not written")
    if exact:
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (what, "not bit-exact", bad[:6].tolist())
    else:
        k = C / 64 + 16
        assert np.all(np.abs(got - ref) <= k * U * cond + 1e-38), (what, float(np.max(np.abs(got - ref) / (cond + 1e-38))))
    assert torch.equal(_sddmm(L, rowptr, col, dv, hv, heads, C), dalpha), (what, "two launches gave different bits")
    return rowptr, col, dv, hv, dalpha


@pytest.mark.parametrize("hc,case", GRID, ids=GRID_IDS)
def test_sddmm(L, hc, case):
    heads, C = hc
    for exact in (True, False):
        rng = np.random.default_rng(_seed("sddmm", heads, C, case[0], exact))
        _check_sddmm(L, case[1](rng), heads, C, rng, exact, (heads, C, case[0], exact))


@pytest.mark.parametrize("ld_extra,offset", [(4, 0), (3, 0), (0, 1)], ids=["ld_W+4", "ld_W+3_scalar", "misaligned_scalar"])
def test_sddmm_strides_and_alignment(L, ld_extra, offset):
    for exact in (True, False):
        rng = np.random.default_rng(_seed("sddmm-ld", ld_extra, offset, exact))
        _check_sddmm(L, _row_lengths("hub_in_leaves", rng), 8, 8, rng, exact, (ld_extra, offset, exact), ld_extra=ld_extra, offset=offset)


def test_sddmm_one_head_has_the_single_head_kernels_bits(L):
    rng = np.random.default_rng(8)
    rowptr, col, dv, hv, dalpha = _check_sddmm(L, _row_lengths("several_per_wave", rng), 1, 64, rng, True, "1x64")
    rp, cl = _dev_csr(rowptr, col)
    old = _nan(len(col))
    _run(L, "fitgnn_sddmm_csr_f32", L.dptr(rp), L.dptr(cl), L.dptr(dv), 64, L.dptr(hv), 64, len(rowptr) - 1, 64, L.dptr(old))
    assert torch.equal(dalpha[:, 0], old)


# ---------------------------------------------------------------------------------------------------------------------------------
# softmax / LeakyReLU backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _exact_bwd_inputs_heads(rowptr, n, n_cols, heads, rng):
    per = [_exact_bwd_inputs(rowptr, n, n_cols, rng) for _ in range(heads)]
    return tuple(np.stack([p[i] for p in per], axis=1) for i in range(4))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("heads", HEADS_ONLY)
def test_softmax_backward_exact(L, heads, case):
    """Exact inputs per head (test_gpu_gat_kernels._exact_bwd_inputs): ds and da_dst equal the float64 result bit for bit at every
    row length, s == 0 taking the slope; a row without entries gets da_dst = 0; the same bits on a second launch."""
    for slope in (0.25, 0.5):
        rng = np.random.default_rng(_seed("bwd", heads, case[0], slope))
        lens = case[1](rng)
        n = len(lens)
        rowptr, col = _csr(lens, _n_cols(n), rng)
        a_s, a_d, alpha, dalpha = _exact_bwd_inputs_heads(rowptr, n, _n_cols(n), heads, rng)
        ds, da_dst = _softmax_bwd(L, rowptr, col, a_s, a_d, alpha, dalpha, slope)
        ref_ds, ref_dst = ghr.softmax_bwd(rowptr, col, a_s, a_d, alpha, dalpha, slope)
        got_ds, got_dst = _np(ds), _np(da_dst)
        bad = np.argwhere(got_ds != ref_ds)
        assert bad.size == 0, (heads, case[0], slope, bad[:6].tolist())
        bad = np.argwhere(got_dst != ref_dst)
        assert bad.size == 0, (heads, case[0], slope, bad[:6].tolist())
        assert np.all(got_dst[lens == 0] == 0.0)
        ds2, dst2 = _softmax_bwd(L, rowptr, col, a_s, a_d, alpha, dalpha, slope)
        assert torch.equal(ds2, ds) and torch.equal(dst2, da_dst)


@pytest.mark.parametrize("case", CASES[:4], ids=CASE_IDS[:4])
@pytest.mark.parametrize("heads", [1, 3, 8])
def test_softmax_backward_random(L, heads, case):
    """alpha from a real softmax, random dalpha: per entry |ds - ref| <= k u alpha |lrelu'| (|dalpha| + sum |alpha dalpha|), per
    (row, head) |da_dst - ref| <= 3 k u sum of those, k = len / 64 + 24."""
    for slope in (0.2, 0.0):
        rng = np.random.default_rng(_seed("bwd-r", heads, case[0], slope))
        lens = case[1](rng)
        n = len(lens)
        rowptr, col = _csr(lens, _n_cols(n), rng)
        a_s = rng.standard_normal((_n_cols(n), heads)).astype(np.float32)
        a_d = rng.standard_normal((n, heads)).astype(np.float32)
        alpha = ghr.edge_softmax(rowptr, col, a_s, a_d, slope).astype(np.float32)
        dalpha = rng.standard_normal((len(col), heads)).astype(np.float32)
        ds, da_dst = _softmax_bwd(L, rowptr, col, a_s, a_d, alpha, dalpha, slope)
        ref_ds, ref_dst = ghr.softmax_bwd(rowptr, col, a_s, a_d, alpha, dalpha, slope)
        rows = gr.entry_rows(rowptr)
        k = np.asarray(lens) / 64.0 + 24
        got_ds, got_dst = _np(ds), _np(da_dst)
        for hd in range(heads):
            al, da = alpha[:, hd].astype(np.float64), dalpha[:, hd].astype(np.float64)
            dot_abs = np.bincount(rows, weights=np.abs(al * da), minlength=n)
            lr = gr.leaky_relu_grad(gr.edge_scores(rowptr, col, a_s[:, hd], a_d[:, hd]), slope)
            cond = np.abs(al) * np.abs(lr) * (np.abs(da) + dot_abs[rows])
            assert np.all(np.abs(got_ds[:, hd] - ref_ds[:, hd]) <= k[rows] * U * cond + 1e-38), (heads, case[0], slope, hd)
            cond_dst = np.bincount(rows, weights=cond, minlength=n)
            assert np.all(np.abs(got_dst[:, hd] - ref_dst[:, hd]) <= 3 * k * U * cond_dst + 1e-38), (heads, case[0], slope, hd)


def test_softmax_backward_one_head_has_the_single_head_kernels_bits(L):
    rng = np.random.default_rng(9)
    lens = _row_lengths("several_per_wave", rng)
    n = len(lens)
    rowptr, col = _csr(lens, _n_cols(n), rng)
    a_s, a_d, alpha, dalpha = _exact_bwd_inputs_heads(rowptr, n, _n_cols(n), 1, rng)
    ds, da_dst = _softmax_bwd(L, rowptr, col, a_s, a_d, alpha, dalpha, 0.25)
    rp, cl = _dev_csr(rowptr, col)
    ins = [_f32(a[:, 0]) for a in (a_s, a_d, alpha, dalpha)]
    ods, odst = _nan(len(col)), _nan(n)
    _run(L, "fitgnn_gat_softmax_bwd_f32", L.dptr(rp), L.dptr(cl), *[L.dptr(t) for t in ins], 0.25, n, L.dptr(ods), L.dptr(odst))
    # (a row without entries: the single-head kernel writes 0 there as well)
    assert torch.equal(ds[:, 0], ods) and torch.equal(da_dst[:, 0], odst)
