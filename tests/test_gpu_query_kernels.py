"""GPU tier: the two node-query kernels of csrc/query.hip through the C ABI against the float64 references of
tests/query_reference.py (the convention and helpers of tests/test_gpu_step_kernels.py).

EXACT inputs (tests/query_reference.py: integers over a power of two, power-of-two CSR values, every pre-activation >= 0 or <= -32
where fp32 ELU is exactly -1; proven exact on the CPU by tests/test_query_reference_cpu.py) must come back bit for bit.  RANDOM inputs
are held per entry to 2^-24 times the first-order bound the reference accumulates along the kernel's own operation order (docstrings
of query_reference.gather / tail / log_softmax_bound: one rounding per fmaf and per add, expm1f / expf / logf within 1 ulp as the HIP
math API states); nothing is added on top.

Launcher -> branch -> tests that reach it:

| launcher | branch (from the launch and kernel code) | tests |
|---|---|---|
| fitgnn_gcn_query_gather_f32 | column slabs: H = 4 (one live lane), 64, 256 (one full slab), 260 (second slab, one live lane), 512, 516 | test_gather_exact[*] |
| | query degree 0 (zeros over a NaN-filled G), 1, 2, 3, 4 (one entry per wave), 5, 9, 130 (uneven remainder: waves with none / one / many), 8, 17, 64, 65 | test_gather_exact[*] |
| | neighbour-row degree 0 (ELU(b0)), 1, 2, 63, 64, 65 (second 64-entry batch), 300 (five batches); groups of four with 1-3 missing | test_gather_exact[*] |
| | xrow NULL / given with repeated table rows and an entry at the last table row (NaN behind T); b0 NULL / given; ldt > H, ldg > H | test_gather_exact[*] |
| | Q = 1, 3, 64, 257; unsorted rows with duplicates; NaN guards behind and between the rows of G untouched | test_gather_rows |
| | RANDOM values of both signs (both ELU branches, expm1f); two launches give the same bits | test_gather_random, test_gather_rows |
| | T or G one float into its buffer -> FITGNN_E_ALIGN | test_gather_misaligned |
| fitgnn_gcn_query_tail_f32 | (H, H2) = (4, 16) one k-step, one column block; (64, 64) two k-stages; (68, 80) a 4-wide last stage, a fifth block on wave 1; (512, 512) two column passes of 256 | test_tail_exact[*] |
| | C = 1, 3, 7, 16, 47, 48 (head items 16 C > 256: second pass of the item loop); Q = 1, 15, 16, 17, 33 (partial last tile: nothing stored past row Q; guarded out, ldo > C, ldg > H) | test_tail_exact[*] |
| | b1 NULL / given, bl NULL / given; log-softmax off | test_tail_exact[*] |
| | RANDOM operands, log-softmax off and on, rows whose logits differ by 1e4; two launches give the same bits | test_tail_random |
| | G or out one float into its buffer -> FITGNN_E_ALIGN | test_tail_misaligned |

Worst observed error / bound per family on one MI355X run: gather random 0.34 (H = 260), gather rows 0.26; tail logits 0.020, tail
log-softmax 0.019 (both at (4, 16, 3, 1); 0.001 or less at H = H2 = 512, where the worst-case chain bound is loosest).
"""
import numpy as np
import pytest
import torch

import query_reference as qr
from test_gpu_step_kernels import E_ALIGN, L, U, _call, _dev, _np, _p, _rng, _run, _same, _strided, _within  # noqa: F401

pytestmark = pytest.mark.gpu


def _guarded(n, C, ld, tail_rows=2):
    """A NaN-filled [n + tail_rows, ld] device buffer and its [n, C] view: whatever is still NaN afterwards was not written."""
    buf = torch.full(((n + tail_rows) * ld,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[: n * ld].view(n, ld)[:, :C]


def _untouched(buf, n, C, ld, what):
    full = buf.view(-1, ld)
    assert torch.isnan(full[n:]).all(), f"{what}: rows past the last one were written"
    assert torch.isnan(full[:n, C:]).all(), f"{what}: columns past the last one were written"


def _gather(L, c, ldt_pad=4, ldg_pad=8, rows=None):
    H = c["T"].shape[1]
    rows = c["rows"] if rows is None else rows
    Td = _strided(c["T"], H + ldt_pad)
    buf, G = _guarded(len(rows), H, H + ldg_pad)
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["val"]),
            None if c["xrow"] is None else _dev(c["xrow"], torch.int32), None if c["b0"] is None else _dev(c["b0"]), _dev(rows, torch.int64)]
    rp, cl, vl, xr, b0, rw = keep
    args = (_p(L, rp), _p(L, cl), _p(L, vl), _p(L, Td), H + ldt_pad, _p(L, xr), _p(L, b0), _p(L, rw), len(rows), H, _p(L, G), H + ldg_pad)
    _run(L, "fitgnn_gcn_query_gather_f32", *args)
    first = G.clone()
    _untouched(buf, len(rows), H, H + ldg_pad, "gather")
    _run(L, "fitgnn_gcn_query_gather_f32", *args)
    assert torch.equal(first, G), "two launches differ"
    return _np(first)


@pytest.mark.parametrize("case", qr.EXACT_GATHER_CASES, ids=str)
def test_gather_exact(L, case):
    c = qr.exact_gather_case(*case)
    ref = qr.gather(c["rowptr"], c["col"], c["val"], c["T"], c["rows"], xrow=c["xrow"], b0=c["b0"], f32_elu=True)
    got = _gather(L, c)
    assert np.all(got[0] == 0), "a query row without entries must give zeros"
    _same(got, ref, f"gather {case}")


def _random_gather_case(tag, H, q_degs, n_degs, with_xrow, with_b0):
    rng = _rng("query-gather", tag, H)
    n_table = 41
    rowptr, col, val, xrow, n_rows = qr.query_csr(rng, q_degs, n_degs, n_table, with_xrow, pow2_val=False)
    T = rng.normal(0, 1, size=(n_table if with_xrow else n_rows, H)).astype(np.float32)
    b0 = rng.normal(0, 1, size=H).astype(np.float32) if with_b0 else None
    return dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=T, b0=b0, rows=np.arange(len(q_degs), dtype=np.int64), n_rows=n_rows)


def _ratio(got, ref, B, what):
    err = np.abs(got - ref)
    bound = U * B
    worst = float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))))
    print(f"{what}: worst error / bound = {worst:.3f}")
    _within(got, ref, bound, what)


@pytest.mark.parametrize("H,with_xrow,with_b0", [(64, True, True), (516, False, True), (260, True, False)], ids=str)
def test_gather_random(L, H, with_xrow, with_b0):
    c = _random_gather_case("random", H, qr.GATHER_QUERY_DEGS, qr.GATHER_NEIGHBOUR_DEGS, with_xrow, with_b0)
    ref, B = qr.gather(c["rowptr"], c["col"], c["val"], c["T"], c["rows"], xrow=c["xrow"], b0=c["b0"], sums=True)
    got = _gather(L, c)
    _ratio(got, ref, B, f"gather random H={H}")


@pytest.mark.parametrize("Q", [1, 3, 64, 257])
def test_gather_rows(L, Q):
    c = _random_gather_case("rows", 64, [3, 0, 7, 1, 12, 5, 2, 9, 4, 6], [2, 5, 1, 9, 0, 3], True, True)
    rng = _rng("query-rows", Q)
    rows = rng.integers(0, c["n_rows"], size=Q).astype(np.int64)   # unsorted, duplicates (Q > n_rows forces them), any row of the CSR
    if Q >= 3:
        rows[1] = rows[0]
    ref, B = qr.gather(c["rowptr"], c["col"], c["val"], c["T"], rows, xrow=c["xrow"], b0=c["b0"], sums=True)
    got = _gather(L, c, rows=rows)
    _ratio(got, ref, B, f"gather rows Q={Q}")


def test_gather_misaligned(L):
    c = _random_gather_case("align", 8, [2, 1], [1, 2], False, False)
    H = 8
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["val"]), _dev(c["rows"], torch.int64)]
    rp, cl, vl, rw = keep
    buf = torch.zeros(c["n_rows"] * H + 8, dtype=torch.float32, device="cuda")
    out = torch.zeros(2 * H + 8, dtype=torch.float32, device="cuda")
    good = (_p(L, rp), _p(L, cl), _p(L, vl), _p(L, buf), H, None, None, _p(L, rw), 2, H, _p(L, out), H)
    assert _call(L, "fitgnn_gcn_query_gather_f32", *good) == 0
    bad_T = good[:3] + (_p(L, buf[1:]),) + good[4:]
    assert _call(L, "fitgnn_gcn_query_gather_f32", *bad_T) == E_ALIGN
    bad_G = good[:10] + (_p(L, out[1:]), H)
    assert _call(L, "fitgnn_gcn_query_gather_f32", *bad_G) == E_ALIGN


# ---------------------------------------------------------------------------------------------------------------------------------
# tail
# ---------------------------------------------------------------------------------------------------------------------------------
def _tail(L, c, log_softmax, ldg_pad=4, ldo_pad=3):
    Q, H = c["G"].shape
    H2, C = c["W1"].shape[0], c["Wl"].shape[0]
    Gd = _strided(c["G"], H + ldg_pad)
    keep = [_dev(c["W1"]), None if c["b1"] is None else _dev(c["b1"]), _dev(c["Wl"]), None if c["bl"] is None else _dev(c["bl"])]
    W1, b1, Wl, bl = keep
    buf, out = _guarded(Q, C, C + ldo_pad, tail_rows=17)
    args = (_p(L, Gd), H + ldg_pad, Q, _p(L, W1), _p(L, b1), _p(L, Wl), _p(L, bl), H, H2, C, _p(L, out), C + ldo_pad, int(log_softmax))
    _run(L, "fitgnn_gcn_query_tail_f32", *args)
    first = out.clone()
    _untouched(buf, Q, C, C + ldo_pad, "tail")
    _run(L, "fitgnn_gcn_query_tail_f32", *args)
    assert torch.equal(first, out), "two launches differ"
    return _np(first)


@pytest.mark.parametrize("case", qr.EXACT_TAIL_CASES, ids=str)
def test_tail_exact(L, case):
    c = qr.exact_tail_case(*case)
    ref = qr.tail(c["G"], c["W1"], c["b1"], c["Wl"], c["bl"], f32_elu=True)
    _same(_tail(L, c, False), ref, f"tail {case}")


@pytest.mark.parametrize("H,H2,C,Q,extreme", [(4, 16, 3, 1, False), (64, 64, 7, 17, False), (68, 80, 47, 33, True), (512, 512, 48, 16, False),
                                              (512, 512, 7, 15, True)], ids=str)
def test_tail_random(L, H, H2, C, Q, extreme):
    rng = _rng("query-tail", H, H2, C, Q)
    c = dict(G=rng.normal(0, 1, size=(Q, H)).astype(np.float32), W1=(rng.normal(0, 1, size=(H2, H)) / np.sqrt(H)).astype(np.float32),
             b1=rng.normal(0, 1, size=H2).astype(np.float32), Wl=(rng.normal(0, 1, size=(C, H2)) / np.sqrt(H2)).astype(np.float32),
             bl=rng.normal(0, 1, size=C).astype(np.float32))
    if extreme:   # rows whose logits differ by 1e4: one class far above the others, on every other row through G's scale
        c["bl"][0] = 1e4
        c["G"][::2] *= 64.0
    logits, B = qr.tail(c["G"], c["W1"], c["b1"], c["Wl"], c["bl"], sums=True)
    _ratio(_tail(L, c, False), logits, B, f"tail logits {(H, H2, C, Q)}")
    ref = qr.tail(c["G"], c["W1"], c["b1"], c["Wl"], c["bl"], log_softmax=True)
    if extreme and C > 1:
        assert (logits.max(1) - logits.min(1)).max() >= 1e4
    _ratio(_tail(L, c, True), ref, qr.log_softmax_bound(logits, B), f"tail log-softmax {(H, H2, C, Q)}")


def test_tail_misaligned(L):
    rng = _rng("query-tail-align")
    Q, H, H2, C = 3, 8, 16, 4
    G = torch.zeros(Q * H + 8, dtype=torch.float32, device="cuda")
    W1, Wl = _dev(rng.normal(size=(H2, H))), _dev(rng.normal(size=(C, H2)))
    out = torch.zeros(Q * C + 8, dtype=torch.float32, device="cuda")
    good = (_p(L, G), H, Q, _p(L, W1), None, _p(L, Wl), None, H, H2, C, _p(L, out), C, 0)
    assert _call(L, "fitgnn_gcn_query_tail_f32", *good) == 0
    assert _call(L, "fitgnn_gcn_query_tail_f32", _p(L, G[1:]), *good[1:]) == E_ALIGN
    assert _call(L, "fitgnn_gcn_query_tail_f32", *good[:10], _p(L, out[1:]), C, 0) == E_ALIGN
