"""GPU tier: fitgnn_sage_query_gather_f32 (csrc/query.hip, sage_query_gather_kernel) through the C ABI against the float64 reference of
tests/sage_query_reference.py, and on through the unchanged fitgnn_gcn_query_tail_f32 with K = 2H (the convention and helpers of
tests/test_gpu_step_kernels.py / tests/test_gpu_query_kernels.py).

EXACT inputs (tests/sage_query_reference.py: both halves of T integers over 8, power-of-two CSR values, every pre-activation >= 0 or
<= -32 where fp32 ELU is exactly -1; proven exact on the CPU by tests/test_sage_query_reference_cpu.py) must come back bit for bit.
RANDOM inputs are held per entry to 2^-24 times the first-order bound the reference accumulates along the kernel's own operation
order (docstring of sage_query_reference.gather: one rounding per fmaf and per add, expm1f within 1 ulp as the HIP math API states);
nothing is added on top.

Launcher -> branch -> tests that reach it:

| launcher | branch (from the launch and kernel code) | tests |
|---|---|---|
| fitgnn_sage_query_gather_f32 | column slabs: H = 4 (one live lane), 64, 256 (one full slab), 260 (second slab, one live lane), 512, 516; the root float4 at + H in each | test_gather_exact[*] |
| | query degree 0 (g = 0 over a NaN-filled G, h_q still stored), 1, 2, 3 (the item after the last entry on a wave WITHOUT entries: waves 0-3), 4, 5, 8, 9, 17, 64, 65, 130 (on a wave behind its entries) | test_gather_exact[*] |
| | layer-0 row degree 0 (ELU(root + b0)), 1, 2, 63, 64, 65 (second 64-entry batch), 300 (five batches); groups of four with 1-3 missing | test_gather_exact[*] |
| | xrow NULL / given with repeated table rows and an entry at the last table row (NaN behind T); b0 NULL (no second add) / given; ldt > 2H, ldg > 2H; nothing written past column 2H or row Q | test_gather_exact[*] |
| | Q = 1, 3, 64, 257; unsorted rows with duplicates, any row of the CSR | test_gather_rows |
| | RANDOM values of both signs (both ELU branches, expm1f); two launches give the same bits | test_gather_random, test_gather_rows |
| | T or G one float into its buffer -> FITGNN_E_ALIGN; ldg = 2H - 4 -> FITGNN_E_BADARG | test_gather_errors |
| fitgnn_sage_query_gather_f32 -> fitgnn_gcn_query_tail_f32 | K = 2H with (H, H2, C) = (64, 64, 7) and (260, 80, 47): H != H2, a 8-wide last k-stage (520 = 16 x 32 + 8), 22 queries (a partial second tile) | test_gather_then_tail_exact[*] |

Worst observed error / bound per family on one MI355X run: gather random g 0.163 / 0.253 / 0.283 and h_q 0.429 / 0.499 / 0.377
(H = 64 / 516 / 260); gather rows 0.294, 0.458, 0.478, 0.478 (Q = 1, 3, 64, 257).
"""
import numpy as np
import pytest
import torch

import query_reference as qr
import sage_query_reference as sq
from test_gpu_query_kernels import _guarded, _ratio, _untouched
from test_gpu_step_kernels import E_ALIGN, E_BADARG, L, _call, _dev, _np, _p, _rng, _run, _same, _strided  # noqa: F401

pytestmark = pytest.mark.gpu
FN = "fitgnn_sage_query_gather_f32"


def _gather(L, c, ldt_pad=4, ldg_pad=8, rows=None, keep_device=False):
    H = c["T"].shape[1] // 2
    rows = c["rows"] if rows is None else rows
    Td = _strided(c["T"], 2 * H + ldt_pad)
    buf, G = _guarded(len(rows), 2 * H, 2 * H + ldg_pad)
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["val"]),
            None if c["xrow"] is None else _dev(c["xrow"], torch.int32), None if c["b0"] is None else _dev(c["b0"]), _dev(rows, torch.int64)]
    rp, cl, vl, xr, b0, rw = keep
    args = (_p(L, rp), _p(L, cl), _p(L, vl), _p(L, Td), 2 * H + ldt_pad, _p(L, xr), _p(L, b0), _p(L, rw), len(rows), H, _p(L, G),
            2 * H + ldg_pad)
    _run(L, FN, *args)
    first = G.clone()
    _untouched(buf, len(rows), 2 * H, 2 * H + ldg_pad, "sage gather")
    _run(L, FN, *args)
    assert torch.equal(first, G), "two launches differ"
    return (G, buf) if keep_device else _np(first)


@pytest.mark.parametrize("case", sq.EXACT_SAGE_CASES, ids=str)
def test_gather_exact(L, case):
    c = sq.exact_sage_case(*case)
    H = case[0]
    ref = sq.gather(c["rowptr"], c["col"], c["val"], c["T"], c["rows"], xrow=c["xrow"], b0=c["b0"], f32_elu=True)
    got = _gather(L, c)
    assert np.all(got[0, :H] == 0), "a query row without entries must give zeros in [0, H)"
    _same(got[0, H:], ref[0, H:], f"sage gather {case}: h_q of the query without entries")
    _same(got, ref, f"sage gather {case}")


def _random_case(tag, H, q_degs, n_degs, with_xrow, with_b0):
    rng = _rng("sage-query-gather", tag, H)
    n_table = 41
    rowptr, col, val, xrow, n_rows = qr.query_csr(rng, q_degs, n_degs, n_table, with_xrow, pow2_val=False)
    T = rng.normal(0, 1, size=(n_table if with_xrow else n_rows, 2 * H)).astype(np.float32)
    b0 = rng.normal(0, 1, size=H).astype(np.float32) if with_b0 else None
    return dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=T, b0=b0, rows=np.arange(len(q_degs), dtype=np.int64), n_rows=n_rows)


@pytest.mark.parametrize("H,with_xrow,with_b0", [(64, True, True), (516, False, True), (260, True, False)], ids=str)
def test_gather_random(L, H, with_xrow, with_b0):
    c = _random_case("random", H, sq.GATHER_QUERY_DEGS, sq.GATHER_NEIGHBOUR_DEGS, with_xrow, with_b0)
    ref, B = sq.gather(c["rowptr"], c["col"], c["val"], c["T"], c["rows"], xrow=c["xrow"], b0=c["b0"], sums=True)
    assert (ref < 0).any() and (ref > 0).any()    # both ELU branches
    got = _gather(L, c)
    _ratio(got[:, :H], ref[:, :H], B[:, :H], f"sage gather random H={H}: g")
    _ratio(got[:, H:], ref[:, H:], B[:, H:], f"sage gather random H={H}: h_q")


@pytest.mark.parametrize("Q", [1, 3, 64, 257])
def test_gather_rows(L, Q):
    c = _random_case("rows", 64, [3, 0, 7, 1, 12, 5, 2, 9, 4, 6], [2, 5, 1, 9, 0, 3], True, True)
    rng = _rng("sage-query-rows", Q)
    rows = rng.integers(0, c["n_rows"], size=Q).astype(np.int64)   # unsorted, duplicates (Q > n_rows forces them), any row of the CSR
    if Q >= 3:
        rows[1] = rows[0]
    ref, B = sq.gather(c["rowptr"], c["col"], c["val"], c["T"], rows, xrow=c["xrow"], b0=c["b0"], sums=True)
    got = _gather(L, c, rows=rows)
    _ratio(got, ref, B, f"sage gather rows Q={Q}")


@pytest.mark.parametrize("case", sq.CHAIN_CASES, ids=str)
def test_gather_then_tail_exact(L, case):
    H, H2, C = case
    c = sq.exact_chain_case(*case)
    Q = len(c["rows"])
    Gref = sq.gather(c["rowptr"], c["col"], c["val"], c["T"], c["rows"], xrow=c["xrow"], b0=c["b0"], f32_elu=True)
    ref = qr.tail(Gref, c["W1"], c["b1"], c["Wl"], c["bl"], f32_elu=True)
    G, gbuf = _gather(L, c, keep_device=True)
    _same(_np(G), Gref, f"sage chain {case}: G")
    keep = [_dev(c["W1"]), _dev(c["b1"]), _dev(c["Wl"]), _dev(c["bl"])]
    W1, b1, Wl, bl = keep
    buf, out = _guarded(Q, C, C + 3, tail_rows=17)
    _run(L, "fitgnn_gcn_query_tail_f32", _p(L, G), G.stride(0), Q, _p(L, W1), _p(L, b1), _p(L, Wl), _p(L, bl), 2 * H, H2, C, _p(L, out),
         C + 3, 0)
    _untouched(buf, Q, C, C + 3, "tail behind the sage gather")
    _same(_np(out), ref, f"sage chain {case}: logits")


def test_gather_errors(L):
    c = _random_case("align", 8, [2, 1], [1, 2], False, False)
    H = 8
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["val"]), _dev(c["rows"], torch.int64)]
    rp, cl, vl, rw = keep
    buf = torch.zeros(c["n_rows"] * 2 * H + 8, dtype=torch.float32, device="cuda")
    out = torch.zeros(2 * 2 * H + 8, dtype=torch.float32, device="cuda")
    good = (_p(L, rp), _p(L, cl), _p(L, vl), _p(L, buf), 2 * H, None, None, _p(L, rw), 2, H, _p(L, out), 2 * H)
    assert _call(L, FN, *good) == 0
    bad_T = good[:3] + (_p(L, buf[1:]),) + good[4:]
    assert _call(L, FN, *bad_T) == E_ALIGN
    bad_G = good[:10] + (_p(L, out[1:]), 2 * H)
    assert _call(L, FN, *bad_G) == E_ALIGN
    assert _call(L, FN, *good[:11], 2 * H - 4) == E_BADARG
    assert _call(L, FN, *good[:4], 2 * H - 4, *good[5:]) == E_BADARG
