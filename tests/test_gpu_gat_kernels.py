"""GPU tier: the GAT attention kernels of csrc/gat.hip through the C ABI against the float64 references of tests/gat_reference.py,
and the GAT layers on hub-heavy graphs and on the star-run layout against the float64 oracle.

Two kinds of input.  EXACT inputs (small integers, multiples of 1/4 or 1/64, slopes 0.25 / 0.5) keep every fp32 partial result
exact, so a kernel must return the float64 result bit for bit whatever its summation order: a dropped, doubled or misplaced entry
in a row of 20 000 entries cannot hide under a tolerance.  RANDOM inputs are held to a per-entry bound, k * 2^-24 * (sum of |terms|
of that entry), never to a fraction of the whole output's largest value.  Rows are shaped around the kernels' branches: at most
kShortRow = 8 entries on one thread, longer ones by the whole wave 64 entries per pass, several long rows of a wave in turn."""
import argparse
import zlib

import numpy as np
import pytest
import torch

import gat_reference as gr
from graph_fixtures import star_blocks

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # fp32 unit roundoff


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from fitgnn_amd import _lib
    return _lib


def _seed(*parts):
    """A seed fixed across processes (hash() of a str is not)."""
    return zlib.crc32(repr(parts).encode())


def _run(L, fn, *args):
    lib = L.lib()
    L.check(getattr(lib, fn)(*args, L.stream_ptr()), fn)
    torch.cuda.synchronize()


def _p(L, t):
    """Device pointer of t: the caller keeps t referenced until the launch has run (a temporary's memory goes back to the caching
    allocator as soon as its pointer is taken)."""
    return L.dptr(t)


# ---------------------------------------------------------------------------------------------------------------------------------
# row shapes
# ---------------------------------------------------------------------------------------------------------------------------------
BRANCH_LENS = [1, 2, 7, 8, 9, 63, 64, 65, 128, 129, 1000]


def _row_lengths(case, rng):
    """Row lengths of a case; n is never a multiple of 4 unless the case says so."""
    if case == "isolated":        # n = 1: a node with its self loop only
        return np.array([1])
    if case == "hub":             # n = 1, one row of more than 20 000 entries
        return np.array([20011])
    if case == "mixed":           # every branch length once, among short rows; n = 203
        lens = rng.integers(1, 9, size=203)
        lens[np.linspace(3, 199, len(BRANCH_LENS)).astype(int)] = BRANCH_LENS
        return lens
    if case == "several_per_wave":   # waves with none, one, and several long rows; n = 133
        lens = rng.integers(1, 9, size=133)
        lens[70] = 65
        lens[[128, 129, 131, 132]] = [9, 129, 64, 8]
        return lens
    if case == "whole_wave":      # all 64 rows of the second wave long, then two short rows; n = 130
        lens = rng.integers(1, 9, size=130)
        lens[64:128] = rng.integers(9, 300, size=64)
        lens[100] = 65
        return lens
    if case == "hub_in_leaves":   # one row of 20 000 entries in a wave of short rows, two long neighbours; n = 301
        lens = rng.integers(1, 5, size=301)
        lens[150], lens[151], lens[152] = 20000, 65, 129
        return lens
    raise ValueError(case)


ROW_CASES = ["isolated", "hub", "mixed", "several_per_wave", "whole_wave", "hub_in_leaves"]


def _n_cols(n):
    """Columns of a case's pattern: at least 257 distinct ones, so that the rows of a case with n = 1 see different operands."""
    return max(n, 257)


def _csr(lens, n_cols, rng):
    rowptr = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    col = rng.integers(0, n_cols, size=int(rowptr[-1]))
    return rowptr, col


def _dev_csr(rowptr, col):
    return (torch.from_numpy(rowptr.astype(np.int32)).cuda(), torch.from_numpy(col.astype(np.int32)).cuda())


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _strided(A, ld, offset=0):
    """A [n, C] (float32 values) as a device view with row stride ld, starting `offset` floats into its buffer; the padding
    columns hold NaN, so a kernel that reads past column C of a row poisons its result."""
    A = np.asarray(A, dtype=np.float32)
    n, C = A.shape
    buf = torch.full((offset + n * ld + 4,), float("nan"), dtype=torch.float32, device="cuda")
    v = buf[offset:offset + n * ld].view(n, ld)[:, :C]
    v.copy_(torch.from_numpy(A))
    return v


def _branch_positions(lens):
    """For every row longer than kShortRow: the entry that gets the row's dominant score -- entry 8, 9, 64, 65 or the last, in turn."""
    out = {}
    k = 0
    for r, n in enumerate(lens):
        if n > 8:
            cands = [p for p in (8, 9, 64, 65, n - 1) if p < n]
            out[r] = cands[k % len(cands)]
            k += 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# gat_scores
# ---------------------------------------------------------------------------------------------------------------------------------
WIDTHS = [1, 3, 4, 7, 64, 256, 260, 512, 516, 1000, 1024, 1028, 2048]


def _scores(L, hv, att_s, att_d):
    n, C = hv.shape
    a_s = torch.full((n,), float("nan"), device="cuda")
    a_d = torch.full((n,), float("nan"), device="cuda")
    _run(L, "fitgnn_gat_scores_f32", _p(L, hv), hv.stride(0), n, C, _p(L, att_s), _p(L, att_d), _p(L, a_s), _p(L, a_d))
    return a_s.cpu().numpy().astype(np.float64), a_d.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("C", WIDTHS)
def test_gat_scores(L, C):
    """Exact inputs bit for bit, random inputs per row within (C / 64 + 16) u sum |h att|; contiguous rows, strides > C that are
    and are not multiples of 4 (the float4 and the scalar path)."""
    rng = np.random.default_rng(C)
    n = 67
    lds = [C, C + 4, C + 3]
    for ld in lds:
        h = rng.integers(-8, 9, size=(n, C)).astype(np.float32)
        att_s, att_d = (rng.integers(-64, 65, size=C) / 64.0 for _ in range(2))
        got_s, got_d = _scores(L, _strided(h, ld), _f32(att_s), _f32(att_d))
        ref_s, ref_d, _, _ = gr.scores(h, att_s, att_d)
        assert np.array_equal(got_s, ref_s) and np.array_equal(got_d, ref_d), (C, ld)

        h = rng.standard_normal((n, C)).astype(np.float32)
        att_s, att_d = (rng.standard_normal(C).astype(np.float32) for _ in range(2))
        got_s, got_d = _scores(L, _strided(h, ld), _f32(att_s), _f32(att_d))
        ref_s, ref_d, cs, cd = gr.scores(h, att_s, att_d)
        k = C / 64 + 16
        assert np.all(np.abs(got_s - ref_s) <= k * U * cs), (C, ld, np.max(np.abs(got_s - ref_s) / cs))
        assert np.all(np.abs(got_d - ref_d) <= k * U * cd), (C, ld, np.max(np.abs(got_d - ref_d) / cd))


@pytest.mark.parametrize("C", [64, 1024])
def test_gat_scores_with_operands_that_are_not_16_byte_aligned(L, C):
    """h, att_src or att_dst one float past a 16-byte boundary (C and the stride multiples of 4): the float4 loads must not be used.
    Exact inputs: the same bits as the aligned call."""
    rng = np.random.default_rng(7)
    n = 33
    h = rng.integers(-8, 9, size=(n, C)).astype(np.float32)
    att_s, att_d = (rng.integers(-64, 65, size=C) / 64.0 for _ in range(2))
    ref_s, ref_d, _, _ = gr.scores(h, att_s, att_d)

    def shifted(a):
        buf = torch.zeros(a.size + 4, device="cuda")
        v = buf[1:1 + a.size]
        v.copy_(torch.from_numpy(np.asarray(a, dtype=np.float32)))
        assert v.data_ptr() % 16 == 4
        return v

    for hv, s, d in ((_strided(h, C, offset=1), _f32(att_s), _f32(att_d)),
                     (_strided(h, C + 4, offset=1), _f32(att_s), _f32(att_d)),
                     (_strided(h, C), shifted(att_s), _f32(att_d)),
                     (_strided(h, C), _f32(att_s), shifted(att_d))):
        got_s, got_d = _scores(L, hv, s, d)
        assert np.array_equal(got_s, ref_s) and np.array_equal(got_d, ref_d)


# ---------------------------------------------------------------------------------------------------------------------------------
# edge softmax
# ---------------------------------------------------------------------------------------------------------------------------------
def _softmax(L, rowptr, col, a_s, a_d, slope):
    rp, cl = _dev_csr(rowptr, col)
    a_s, a_d = _f32(a_s), _f32(a_d)
    alpha = torch.full((len(col),), float("nan"), device="cuda")
    _run(L, "fitgnn_gat_edge_softmax_f32", _p(L, rp), _p(L, cl), _p(L, a_s), _p(L, a_d), float(slope), len(rowptr) - 1, _p(L, alpha))
    return alpha


def _check_softmax(got, ref, what):
    big = ref >= 1e-30
    err = np.abs(got[big] - ref[big]) / ref[big]
    assert err.max(initial=0.0) <= 1e-4, (what, float(err.max()))
    assert np.all(np.abs(got[~big]) <= 1e-29), what   # underflowed entries stay (denormal or) zero


@pytest.mark.parametrize("case", ROW_CASES)
@pytest.mark.parametrize("slope", [0.2, 0.0])
@pytest.mark.parametrize("regime", ["flat", "wide"])
def test_edge_softmax(L, case, slope, regime):
    """Per-entry relative error <= 1e-4 wherever alpha >= 1e-30 (__expf: no exact regime).  flat: scores of one unit's spread, every
    entry of a row matters.  wide: each long row's dominant score sits on entry 8, 9, 64, 65 or its last entry (a kernel that skips
    that entry fails loudly); the rest spread over both LeakyReLU branches down to exp underflow."""
    rng = np.random.default_rng(_seed(case, slope, regime))
    lens = _row_lengths(case, rng)
    n = len(lens)
    hot = _n_cols(n)   # one extra column: the one of the dominant entries
    rowptr, col = _csr(lens, hot, rng)
    if regime == "flat":
        a_s, a_d = rng.standard_normal(hot + 1), rng.standard_normal(n)
    else:
        # positive scores up to 22, negative ones (x slope 0.2) down to -90: exp(e - max) from 1 to below fp32's range
        a_s, a_d = rng.uniform(-450.0, 20.0, size=hot + 1), rng.uniform(-2.0, 2.0, size=n)
        a_s[hot] = 24.0
        for r, pos in _branch_positions(lens).items():
            col[rowptr[r] + pos] = hot
    a_s, a_d = a_s.astype(np.float32), a_d.astype(np.float32)
    alpha = _softmax(L, rowptr, col, a_s, a_d, slope)
    ref = gr.edge_softmax(rowptr, col, a_s, a_d, slope)
    got = alpha.cpu().numpy().astype(np.float64)
    _check_softmax(got, ref, (case, slope, regime))
    if regime == "wide" and slope > 0 and len(col) > 100:
        assert ref.min() == 0.0 or ref.min() < 1e-30, "the scores do not reach exp underflow"
    assert torch.equal(_softmax(L, rowptr, col, a_s, a_d, slope), alpha), "two launches gave different bits"


# ---------------------------------------------------------------------------------------------------------------------------------
# SDDMM
# ---------------------------------------------------------------------------------------------------------------------------------
def _sddmm(L, rowptr, col, dv, hv, sel=None):
    rp, cl = _dev_csr(rowptr, col)
    C = hv.shape[1]
    dalpha = torch.full((len(col),), float("nan"), device="cuda")
    if sel is None:
        _run(L, "fitgnn_sddmm_csr_f32", _p(L, rp), _p(L, cl), _p(L, dv), dv.stride(0), _p(L, hv), hv.stride(0), len(rowptr) - 1, C,
             _p(L, dalpha))
    else:
        s = torch.from_numpy(np.asarray(sel, dtype=np.int64)).cuda()
        _run(L, "fitgnn_sddmm_csr_rows_f32", _p(L, rp), _p(L, cl), _p(L, dv), dv.stride(0), _p(L, hv), hv.stride(0), _p(L, s), len(sel), C,
             _p(L, dalpha))
    return dalpha


def _sddmm_case(L, lens, C, ld, rng, exact, sel=None):
    n = len(lens)
    rowptr, col = _csr(lens, _n_cols(n), rng)
    n_out = n if sel is None else len(sel)
    if exact:   # products are multiples of 1/4, every partial sum below 2^22 quarters
        dout, h = rng.integers(-3, 4, size=(n_out, C)) / 4.0, rng.integers(-3, 4, size=(_n_cols(n), C)).astype(np.float64)
    else:
        dout, h = rng.standard_normal((n_out, C)), rng.standard_normal((_n_cols(n), C))
    dout, h = dout.astype(np.float32), h.astype(np.float32)
    dalpha = _sddmm(L, rowptr, col, _strided(dout, ld), _strided(h, ld), sel)
    ref, cond = gr.sddmm(rowptr, col, dout, h, sel=sel)
    return dalpha, ref, cond, (rowptr, col, dout, h)


def _check_sddmm(got, ref, cond, C, exact, what):
    on = ~np.isnan(ref)
    assert np.array_equal(np.isnan(got), ~on), (what, "entries of unselected rows were written")
    if exact:
        bad = np.nonzero(got[on] != ref[on])[0]
        assert bad.size == 0, (what, "not bit-exact", bad[:8], got[on][bad[:8]], ref[on][bad[:8]])
    else:
        k = C / 64 + 16
        err = np.abs(got[on] - ref[on])
        assert np.all(err <= k * U * cond[on]), (what, float(np.max(err / cond[on])))


@pytest.mark.parametrize("C", WIDTHS)
def test_sddmm_widths_and_strides(L, C):
    """Every width branch (MAXV 1 / 2 / 4, the scalar kernel for C > 1024 or C % 4 != 0) with contiguous rows and strides > C that are
    and are not multiples of 4, on rows of every branch length (4-edge groups with n4 tails, 64-entry chunks)."""
    rng = np.random.default_rng(100 + C)
    lens = _row_lengths("mixed", rng)
    for ld in (C, C + 4, C + 3):
        for exact in (True, False):
            dalpha, ref, cond, _ = _sddmm_case(L, lens, C, ld, rng, exact)
            _check_sddmm(dalpha.cpu().numpy().astype(np.float64), ref, cond, C, exact, (C, ld, exact))


@pytest.mark.parametrize("case", ["hub", "hub_in_leaves", "whole_wave", "several_per_wave", "isolated"])
@pytest.mark.parametrize("C", [64, 516, 1028])
def test_sddmm_long_rows(L, case, C):
    """Rows of 65 to 20 011 entries through each kernel family, exact inputs bit for bit; the same bits on a second launch."""
    rng = np.random.default_rng(200 + C)
    lens = _row_lengths(case, rng)
    dalpha, ref, cond, (rowptr, col, dout, h) = _sddmm_case(L, lens, C, C, rng, True)
    _check_sddmm(dalpha.cpu().numpy().astype(np.float64), ref, cond, C, True, (case, C))
    assert torch.equal(_sddmm(L, rowptr, col, _strided(dout, C), _strided(h, C)), dalpha)


@pytest.mark.parametrize("C", [7, 256, 516, 2048])
def test_sddmm_on_selected_rows(L, C):
    """fitgnn_sddmm_csr_rows_f32: an unsorted selection that skips rows (the hub among them), compact dOut; entries of rows not
    selected keep the NaN sentinel, selected ones are exact."""
    rng = np.random.default_rng(300 + C)
    lens = _row_lengths("hub_in_leaves", rng)
    sel = np.array([152, 7, 150, 0, 300, 64, 63, 151, 200])
    dalpha, ref, cond, _ = _sddmm_case(L, lens, C, C, rng, True, sel=sel)
    _check_sddmm(dalpha.cpu().numpy().astype(np.float64), ref, cond, C, True, C)


# ---------------------------------------------------------------------------------------------------------------------------------
# softmax / LeakyReLU backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _softmax_bwd(L, rowptr, col, a_s, a_d, alpha, dalpha, slope, sel=None):
    rp, cl = _dev_csr(rowptr, col)
    n = len(rowptr) - 1
    ds = torch.full((len(col),), float("nan"), device="cuda")
    da_dst = torch.full((n,), float("nan"), device="cuda")
    ins = [_f32(a) for a in (a_s, a_d, alpha, dalpha)]
    args = [_p(L, rp), _p(L, cl)] + [_p(L, t) for t in ins] + [float(slope)]
    if sel is None:
        _run(L, "fitgnn_gat_softmax_bwd_f32", *args, n, _p(L, ds), _p(L, da_dst))
    else:
        s = torch.from_numpy(np.asarray(sel, dtype=np.int64)).cuda()
        _run(L, "fitgnn_gat_softmax_bwd_rows_f32", *args, _p(L, s), len(sel), _p(L, ds), _p(L, da_dst))
    return ds, da_dst


def _exact_bwd_inputs(rowptr, n, n_cols, rng):
    """alpha = k / 4, dalpha small integers, a_src / a_dst integers (s == 0 on many entries).  Within a row the products
    alpha dalpha cancel in pairs, and one entry with alpha > 0 gets dalpha + 1: sum_k alpha_k dalpha_k is a small nonzero multiple
    of 1/4, so every partial sum of the dot, of ds and of da_dst is an exact fp32 value even in a row of 20 000 entries."""
    nnz = int(rowptr[-1])
    alpha = np.empty(nnz)
    dalpha = np.empty(nnz)
    for r in range(n):
        e0, e1 = rowptr[r], rowptr[r + 1]
        m = e1 - e0
        half = m // 2
        a = rng.integers(0, 4, size=half) / 4.0
        d = rng.integers(-2, 3, size=half).astype(np.float64)
        aa = np.concatenate([a, a, rng.integers(1, 4, size=m - 2 * half) / 4.0])
        dd = np.concatenate([d, -d, np.zeros(m - 2 * half)])
        perm = rng.permutation(m)
        aa, dd = aa[perm], dd[perm]
        nz = np.nonzero(aa)[0]
        if nz.size:
            dd[nz[rng.integers(0, nz.size)]] += 1.0
        alpha[e0:e1], dalpha[e0:e1] = aa, dd
    a_s = rng.integers(-3, 4, size=n_cols).astype(np.float64)
    a_d = rng.integers(-2, 3, size=n).astype(np.float64)   # every row sees s < 0, s == 0 and s > 0
    return a_s, a_d, alpha, dalpha


@pytest.mark.parametrize("case", ROW_CASES)
@pytest.mark.parametrize("slope", [0.25, 0.5])
def test_softmax_backward_exact(L, case, slope):
    """Exact inputs: ds and da_dst equal the float64 result bit for bit at every row length, with s == 0 taking the slope
    (x > 0 ? 1 : slope, as F.leaky_relu's autograd); the same bits on a second launch."""
    rng = np.random.default_rng(_seed(case, slope))
    lens = _row_lengths(case, rng)
    n = len(lens)
    rowptr, col = _csr(lens, _n_cols(n), rng)
    a_s, a_d, alpha, dalpha = _exact_bwd_inputs(rowptr, n, _n_cols(n), rng)
    s = gr.edge_scores(rowptr, col, a_s, a_d)
    if len(col) > 16:
        assert (s == 0).any() and (s > 0).any() and (s < 0).any()
    ds, da_dst = _softmax_bwd(L, rowptr, col, a_s, a_d, alpha, dalpha, slope)
    ref_ds, ref_dst = gr.softmax_bwd(rowptr, col, a_s, a_d, alpha, dalpha, slope)
    got_ds, got_dst = ds.cpu().numpy().astype(np.float64), da_dst.cpu().numpy().astype(np.float64)
    bad = np.nonzero(got_ds != ref_ds)[0]
    assert bad.size == 0, (case, bad[:8], got_ds[bad[:8]], ref_ds[bad[:8]])
    bad = np.nonzero(got_dst != ref_dst)[0]
    assert bad.size == 0, (case, bad[:8], got_dst[bad[:8]], ref_dst[bad[:8]])
    ds2, dst2 = _softmax_bwd(L, rowptr, col, a_s, a_d, alpha, dalpha, slope)
    assert torch.equal(ds2, ds) and torch.equal(dst2, da_dst)


@pytest.mark.parametrize("case", ROW_CASES)
@pytest.mark.parametrize("slope", [0.2, 0.0])
def test_softmax_backward_random(L, case, slope):
    """alpha from a real softmax, random dalpha: per entry |ds - ref| <= k u alpha |lrelu'| (|dalpha| + sum |alpha dalpha|), per row
    |da_dst - ref| <= 3 k u sum of those, k = len / 64 + 24."""
    rng = np.random.default_rng(_seed(case, slope, "r"))
    lens = _row_lengths(case, rng)
    n = len(lens)
    rowptr, col = _csr(lens, _n_cols(n), rng)
    a_s, a_d = rng.standard_normal(_n_cols(n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    a_d[:3] = -a_s[:min(n, 3)]   # s == 0 exactly wherever a row of 0..2 meets its own column
    alpha = gr.edge_softmax(rowptr, col, a_s, a_d, slope).astype(np.float32)
    dalpha = rng.standard_normal(len(col)).astype(np.float32)
    ds, da_dst = _softmax_bwd(L, rowptr, col, a_s, a_d, alpha, dalpha, slope)
    ref_ds, ref_dst = gr.softmax_bwd(rowptr, col, a_s, a_d, alpha, dalpha, slope)
    rows = gr.entry_rows(rowptr)
    al, da = alpha.astype(np.float64), dalpha.astype(np.float64)
    dot_abs = np.bincount(rows, weights=np.abs(al * da), minlength=n)
    lr = gr.leaky_relu_grad(gr.edge_scores(rowptr, col, a_s, a_d), slope)
    cond = np.abs(al) * np.abs(lr) * (np.abs(da) + dot_abs[rows])
    k = np.asarray(lens) / 64.0 + 24
    got_ds, got_dst = ds.cpu().numpy().astype(np.float64), da_dst.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got_ds - ref_ds) <= k[rows] * U * cond + 1e-38), (case, float(np.max(np.abs(got_ds - ref_ds) / (cond + 1e-38))))
    cond_dst = np.bincount(rows, weights=cond, minlength=n)
    assert np.all(np.abs(got_dst - ref_dst) <= 3 * k * U * cond_dst + 1e-38), case


@pytest.mark.parametrize("slope", [0.25, 0.0])
def test_softmax_backward_on_selected_rows(L, slope):
    """fitgnn_gat_softmax_bwd_rows_f32 on an unsorted selection that skips rows: entries and da_dst of rows not selected keep the
    NaN sentinel, selected rows are exact."""
    rng = np.random.default_rng(11)
    lens = _row_lengths("hub_in_leaves", rng)
    n = len(lens)
    rowptr, col = _csr(lens, _n_cols(n), rng)
    a_s, a_d, alpha, dalpha = _exact_bwd_inputs(rowptr, n, _n_cols(n), rng)
    sel = np.array([152, 7, 150, 0, 300, 64, 63, 151, 200, 9])
    ds, da_dst = _softmax_bwd(L, rowptr, col, a_s, a_d, alpha, dalpha, slope, sel=sel)
    ref_ds, ref_dst = gr.softmax_bwd(rowptr, col, a_s, a_d, alpha, dalpha, slope)
    got_ds, got_dst = ds.cpu().numpy().astype(np.float64), da_dst.cpu().numpy().astype(np.float64)
    on_row = np.zeros(n, dtype=bool); on_row[sel] = True
    on = on_row[gr.entry_rows(rowptr)]
    assert np.isnan(got_ds[~on]).all() and np.isnan(got_dst[~on_row]).all(), "rows outside the selection were written"
    assert np.array_equal(got_ds[on], ref_ds[on]) and np.array_equal(got_dst[on_row], ref_dst[on_row])


# ---------------------------------------------------------------------------------------------------------------------------------
# row sum (da_src on the transposed order)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_csr_row_sum_exact(L):
    """Multiples of 1/8 on rows of 0 to 20 011 entries: the fixed-order sum equals the float64 one bit for bit."""
    rng = np.random.default_rng(5)
    lens = np.concatenate([[0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 63, 64, 65, 20011, 5000], rng.integers(0, 30, size=50)])
    rowptr = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    v = rng.integers(-40, 41, size=int(rowptr[-1])) / 8.0
    rp = torch.from_numpy(rowptr.astype(np.int32)).cuda()
    y = torch.full((len(lens),), float("nan"), device="cuda")
    vd = _f32(v)
    _run(L, "fitgnn_csr_row_sum_f32", _p(L, rp), _p(L, vd), len(lens), _p(L, y))
    ref, _ = gr.row_sum(rowptr, v)
    assert np.array_equal(y.cpu().numpy().astype(np.float64), ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# GAT layers on hub-heavy graphs against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def _undirected(a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    k = a != b
    ei = np.unique(np.concatenate([np.stack([a[k], b[k]]), np.stack([b[k], a[k]])], 1), axis=1)
    return torch.tensor(ei, dtype=torch.long)


def _hub_graph(kind):
    """(edge_index, n): star (20 000 leaves), ba (preferential attachment plus a hub of degree >= 1000), degrees (isolated nodes 0..9,
    nodes 10, 11, 12 of degree exactly 7, 8, 9: rows of 8, 9, 10 entries with the self loop)."""
    rng = np.random.default_rng(_seed(kind))
    if kind == "star":
        n = 20001
        return _undirected(np.zeros(n - 1), np.arange(1, n)), n
    if kind == "ba":
        n, m = 3000, 2
        # every new node links to m earlier ones drawn in proportion to their degree (the endpoint list), then node 0 becomes a hub
        ends = np.zeros(2 * m * n, dtype=np.int64)
        ends[:2] = [0, 1]
        cnt = 2
        a, b = [], []
        for v in range(2, n):
            for t in set(ends[rng.integers(0, cnt, size=m)].tolist()):
                a.append(v); b.append(t)
                ends[cnt:cnt + 2] = [v, t]
                cnt += 2
        hub = rng.choice(np.arange(1, n), size=1100, replace=False)
        a += [0] * len(hub); b += hub.tolist()
        ei = _undirected(a, b)
        assert np.bincount(ei[1].numpy(), minlength=n).max() >= 1000
        return ei, n
    if kind == "degrees":
        n = 401
        a, b = rng.integers(13, n, size=1200), rng.integers(13, n, size=1200)
        for node, deg in ((10, 7), (11, 8), (12, 9)):
            nb = rng.choice(np.arange(13, n), size=deg, replace=False)
            a = np.concatenate([a, np.full(deg, node)]); b = np.concatenate([b, nb])
        ei = _undirected(a, b)
        d = np.bincount(ei[1].numpy(), minlength=n)
        assert (d[:10] == 0).all() and d[10:13].tolist() == [7, 8, 9]
        return ei, n
    raise ValueError(kind)


def _hub_rows(ei, n, at_least=64):
    deg = np.bincount(ei[1].numpy(), minlength=n) + 1
    return torch.from_numpy(deg >= at_least)


def _rel_split(got, ref, hub, what, lim):
    """max |got - ref| / max |ref| separately over the hub rows and over the others."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    for name, m in (("hub", hub), ("rest", ~hub)):
        if bool(m.any()):
            r = float((got[m] - ref[m]).abs().max() / ref[m].abs().max().clamp(min=1e-30))
            assert r < lim, (what, name, r)


def _rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / ref.abs().max().clamp(min=1e-30))


@pytest.mark.parametrize("kind,C", [("star", 7), ("star", 64), ("star", 512), ("ba", 64), ("ba", 1000), ("degrees", 7),
                                    ("degrees", 512), ("degrees", 1000)])
def test_gatconv_on_hub_graphs_against_f64(kind, C):
    """fnn.GATConv forward and backward against gnn_oracle.gat_conv in float64: outputs 1e-4, gradients 1e-3, measured separately over
    the hub rows and the other rows."""
    from fitgnn_amd import nn as fnn
    from oracle import gnn_oracle as gorc

    ei, n = _hub_graph(kind)
    hub = _hub_rows(ei, n)
    torch.manual_seed(C)
    conv = fnn.GATConv(16, C).cuda()
    with torch.no_grad():
        conv.bias.normal_()
    x = torch.randn(n, 16)
    xg = x.cuda().requires_grad_(True)
    out = conv(xg, ei.cuda())
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.state_dict().items()}
    xc = x.double().requires_grad_(True)
    ref = gorc.gat_conv(xc, ei, P["lin.weight"], P["att_src"].view(-1), P["att_dst"].view(-1), P["bias"])
    _rel_split(out, ref, hub, "out", 1e-4)
    gout = torch.randn(n, C)
    out.backward(gout.cuda())
    ref.backward(gout.double())
    _rel_split(xg.grad, xc.grad, hub, "dx", 1e-3)
    for k, p in conv.named_parameters():
        assert _rel(p.grad.reshape(-1), P[k].grad.reshape(-1)) < 1e-3, k


def _classify_args(hidden, classes):
    return argparse.Namespace(num_layers1=2, layer_name="GATConv", num_features=16, hidden=hidden, num_classes=classes)


@pytest.mark.parametrize("kind", ["star", "ba", "degrees"])
def test_classify_node_gat_on_hub_graphs_against_f64(kind):
    """network.Classify_node with GATConv layers (eval) against classify_node_gat_fwd_bwd in float64: log-probabilities 1e-4 (hub
    rows and the rest separately), loss 1e-5, every parameter gradient 1e-3."""
    from fitgnn_amd import network
    from oracle import gnn_oracle as gorc

    ei, n = _hub_graph(kind)
    hub = _hub_rows(ei, n)
    torch.manual_seed(1)
    model = network.Classify_node(_classify_args(64, 7)).cuda().eval()
    x = torch.randn(n, 16)
    y = torch.randint(0, 7, (n,))
    out = model(x.cuda(), ei.cuda())
    loss = torch.nn.functional.nll_loss(out, y.cuda())
    loss.backward()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref_out, ref_loss, ref_g = gorc.classify_node_gat_fwd_bwd(sd, x, ei, y, dtype=torch.float64)
    _rel_split(out, ref_out, hub, "log_softmax", 1e-4)
    assert float(loss.detach()) == pytest.approx(float(ref_loss), rel=1e-5)
    for k, p in model.named_parameters():
        assert _rel(p.grad, ref_g[k]) < 1e-3, k


# ---------------------------------------------------------------------------------------------------------------------------------
# the star-run layout the bench uses
# ---------------------------------------------------------------------------------------------------------------------------------
STAR_SIZES = [100, 7, 17, 300, 3, 3, 64, 33, 2, 1000, 1, 3000, 9]


def _star_union():
    ei, n = star_blocks(STAR_SIZES, 2, seed=4)
    return ei, n, np.concatenate([[0], np.cumsum(STAR_SIZES)])


def _layouts(ei, n, ptr):
    """(name, device edge_index) whose registered 'gat' CSR is: default tiles; the whole-subgraph kernel and small tiles; a real
    SubgraphBatch's register_mode('gat')."""
    from fitgnn_amd import csr
    from fitgnn_amd import data as fdata

    e0 = ei.cuda().clone()
    csr.register(e0, csr.CSRGraph(e0, n, mode="gat"), "gat")
    e1 = ei.cuda().clone()
    g1 = csr.CSRGraph(e1, n, mode="gat", ptr=ptr, block_limit=4096)
    assert g1.f.blocks is not None and g1.t.blocks is not None, "the split did not happen"
    csr.register(e1, g1, "gat")
    sub = dict(ptr=ptr, node_id=np.arange(n), core=np.ones(n, dtype=bool), edge_index=ei.numpy())
    X0 = np.zeros((n, 4), dtype=np.float32)
    batch = fdata.SubgraphBatch(sub, X0, np.zeros(n, dtype=np.int64), np.ones(n, dtype=bool), device="cuda")
    g2 = batch.register_mode("gat")
    assert g2.n == n and np.array_equal(g2.ptr, ptr)
    return [("tiles", e0), ("whole_subgraph", e1), ("subgraph_batch", batch.edge_index)], batch


@pytest.mark.parametrize("stream_kernel", [False, True])
def test_gat_on_the_star_run_layout_against_f64(stream_kernel):
    """A star_blocks union (hub rows of up to 3 000 entries) with its GAT CSR built three ways: GATConv forward / backward, the
    de-duplicated first layer (RowIndex) and the loss-rows last layer (FusedGATLastLayerRows) against the float64 oracle."""
    from fitgnn_amd import network, ops
    from fitgnn_amd import nn as fnn
    from oracle import gnn_oracle as gorc

    ei, n, ptr = _star_union()
    hub = _hub_rows(ei, n)
    assert int(hub.sum()) >= 2
    layouts, _ = _layouts(ei, n, ptr)
    cfg = ops.OpConfig(stream_kernel=stream_kernel)
    torch.manual_seed(9)
    conv = fnn.GATConv(16, 64).cuda()
    conv.op_config = cfg
    with torch.no_grad():
        conv.bias.normal_()
    x = torch.randn(n, 16)
    gout = torch.randn(n, 64)
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.state_dict().items()}
    xc = x.double().requires_grad_(True)
    ref = gorc.gat_conv(xc, ei, P["lin.weight"], P["att_src"].view(-1), P["att_dst"].view(-1), P["bias"])
    ref.backward(gout.double())

    # the model: table of N0 rows, union row r = table row idx[r]; loss rows = a third of the rows, hubs among them
    N0 = n // 3
    idx = torch.randint(0, N0, (n,))
    idx[:N0] = torch.arange(N0)
    Xt = torch.randn(N0, 16)
    y = torch.randint(0, 5, (n,))
    mask = torch.rand(n) < 0.33
    mask[ptr[:-1][np.asarray(STAR_SIZES) > 1]] = True
    rows = torch.nonzero(mask).flatten()
    torch.manual_seed(10)
    model = network.Classify_node(_classify_args(64, 5)).cuda().eval().set_op_config(cfg)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref_out, ref_loss, ref_g = gorc.classify_node_gat_fwd_bwd(sd, Xt[idx], ei, y, dtype=torch.float64)
    ref_out_m, ref_loss_m, ref_g_m = gorc.classify_node_gat_fwd_bwd(sd, Xt[idx], ei, y, train_mask=mask, dtype=torch.float64)
    ridx = ops.RowIndex(idx.cuda(), N0)

    for name, e in layouts:
        conv.zero_grad()
        xg = x.cuda().requires_grad_(True)
        out = conv(xg, e)
        _rel_split(out, ref, hub, (name, "out"), 1e-4)
        out.backward(gout.cuda())
        _rel_split(xg.grad, xc.grad, hub, (name, "dx"), 1e-3)
        for k, p in conv.named_parameters():
            assert _rel(p.grad.reshape(-1), P[k].grad.reshape(-1)) < 1e-3, (name, k)

        model.zero_grad()   # de-duplicated first layer
        out = model(Xt.cuda(), e, x_index=ridx)
        loss = torch.nn.functional.nll_loss(out, y.cuda())
        loss.backward()
        _rel_split(out, ref_out, hub, (name, "dedup log_softmax"), 1e-4)
        assert float(loss.detach()) == pytest.approx(float(ref_loss), rel=1e-5), name
        for k, p in model.named_parameters():
            assert _rel(p.grad, ref_g[k]) < 1e-3, (name, "dedup", k)

        model.zero_grad()   # the last layer on the loss rows
        z = model.embed_and_head(Xt[idx].cuda(), e, loss_rows=rows.cuda())
        assert "FusedGATLastLayerRows" in type(z.grad_fn).__name__, type(z.grad_fn).__name__
        lp = torch.log_softmax(z.index_select(0, rows.cuda()), 1)
        loss = torch.nn.functional.nll_loss(lp, y[rows].cuda())
        loss.backward()
        _rel_split(lp, ref_out_m[rows], hub[rows], (name, "loss-rows log_softmax"), 1e-4)
        assert float(loss.detach()) == pytest.approx(float(ref_loss_m), rel=1e-5), name
        for k, p in model.named_parameters():
            assert _rel(p.grad, ref_g_m[k]) < 1e-3, (name, "loss rows", k)
