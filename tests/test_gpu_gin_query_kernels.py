"""GPU tier: fitgnn_gin_query_hops_f32 and fitgnn_gin_query_tail_f32 (csrc/query.hip: gin_query_hops_kernel<NS, NP>,
gin_query_tail_kernel) through the C ABI against the float64 reference of tests/gin_query_reference.py (the convention and helpers of
tests/test_gpu_step_kernels.py / tests/test_gpu_query_kernels.py).

EXACT inputs (tests/gin_query_reference.py: T integers over 8, weights small integers over powers of two, eps in {0.5, -0.25},
power-of-two CSR values; proven exact on the CPU by tests/test_gin_query_reference_cpu.py, where a float32 replay of the stated order
gives the same bits) must come back bit for bit.  RANDOM inputs of both signs are held per entry to 2^-24 times the first-order bound
the reference accumulates along the kernels' own operation order (docstrings of gin_query_reference.hops / tail: one rounding per
fmaf and per add; no transcendental before the log-softmax, whose bound is query_reference.log_softmax_bound); nothing is added on top.

Launcher -> branch -> tests that reach it:

| launcher | branch (from the launch and kernel code) | tests |
|---|---|---|
| fitgnn_gin_query_hops_f32 | (Ha, Hb) = (4, 16): one k-step, one column block, one live lane; (40, 16): an 8-wide last k-stage; (64, 64); (256, 256): one full column pass; (260, 272): a second slot with one live lane, a second pass of one block <2, 2>; (512, 512); (272, 48) <2, 1>; (64, 272) <1, 2>: all four instantiations, unequal pairs | test_hops_exact[*] |
| | query degree 0 (only the self item: (1 + eps1) h_q over a NaN-filled G), 1, 3 (the self item formed by a wave without entries), 14, 15 (exactly one full tile), 16 (the self item alone in a second tile), 31, 32 (a third tile), 40; rows past the last item of a partial tile not folded (ReLU(b0b) != 0 with biases) | test_hops_exact[*] |
| | one-hop row degree 0 (ReLU((1 + eps0) root + b0a)), 1, 63, 64, 65 (a second 64-entry batch), 300 (five batches); groups of four with 1-3 missing | test_hops_exact[*] |
| | xrow NULL / given with repeated table rows and an entry at the last table row (NaN behind T); b0a, b0b NULL / given; eps0 != eps1 read from the device; ldt > Ha, ldg > Hb; nothing written past column Hb or row Q | test_hops_exact[*] |
| | Q = 1, 3, 64, 257; unsorted rows with duplicates, any row of the CSR | test_hops_rows |
| | RANDOM values of both signs (both ReLU branches in both stages); two launches give the same bits | test_hops_random, test_hops_rows |
| | T, W0b or G one float into its buffer -> FITGNN_E_ALIGN; ldt = Ha - 4, ldg = Hb - 4 -> FITGNN_E_BADARG | test_hops_errors |
| fitgnn_gin_query_tail_f32 | (K, H2a, H2b, C) = (64, 64, 64, 7) with 16 queries; (272, 80, 48, 47) with 22 (a partial second tile, a 16-wide last k-stage in both products); (16, 16, 272, 3) with 1 (a second pass in the SECOND product); biases NULL / given; ldg > K, ldo > C; nothing written past column C or row Q | test_tail_exact[*] |
| | RANDOM: logits and log-softmax (log_softmax 0 / 1), (512, 512, 512, 48) the default model's shape | test_tail_random[*] |
| | G or out one float into its buffer -> FITGNN_E_ALIGN; ldg = K - 4 -> FITGNN_E_BADARG; H2a = H2b = 1024 (LDS beyond 160 KiB) -> FITGNN_E_BADARG | test_tail_errors |
| fitgnn_gin_query_hops_f32 -> fitgnn_gin_query_tail_f32 | (Ha, Hb, H2a, H2b, C) = (64, 48, 64, 32, 7) and (260, 272, 80, 48, 47), 37 queries (a partial third tile), G handed on with its padded stride | test_hops_then_tail_exact[*] |

Worst observed error / bound per family on one MI355X run: hops random 0.027 / 0.005 / 0.006 ((Ha, Hb) = (64, 64) / (512, 512) /
(260, 272)); hops rows 0.010, 0.005, 0.024, 0.024 (Q = 1, 3, 64, 257); tail random logits and log-softmax below 0.0005 at all three
shapes (the bound charges each of a chain's K roundings with the whole sum of magnitudes, through three chained products; the EXACT
cases are the sharp check of the tail); the log-softmax of EXACT logits 0.245 / 0.338 / 0.167.
"""
import numpy as np
import pytest
import torch

import gin_query_reference as gq
import query_reference as qr
from test_gpu_query_kernels import _guarded, _ratio, _untouched
from test_gpu_step_kernels import E_ALIGN, E_BADARG, L, _call, _dev, _np, _p, _rng, _run, _same, _strided  # noqa: F401

pytestmark = pytest.mark.gpu
HOPS, TAIL = "fitgnn_gin_query_hops_f32", "fitgnn_gin_query_tail_f32"


def _opt(a, dtype=torch.float32):
    return None if a is None else _dev(a, dtype)


def _hops(L, c, ldt_pad=4, ldg_pad=8, rows=None, keep_device=False):
    Ha, Hb = c["T"].shape[1], c["W0b"].shape[0]
    rows = c["rows"] if rows is None else rows
    Td = _strided(c["T"], Ha + ldt_pad)
    buf, G = _guarded(len(rows), Hb, Hb + ldg_pad)
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["val"]), _opt(c["xrow"], torch.int32), _opt(c["b0a"]),
            _dev(np.array([c["eps0"]], dtype=np.float32)), _dev(c["W0b"]), _opt(c["b0b"]), _dev(np.array([c["eps1"]], dtype=np.float32)),
            _dev(rows, torch.int64)]
    rp, cl, vl, xr, b0a, e0, W, b0b, e1, rw = keep
    args = (_p(L, rp), _p(L, cl), _p(L, vl), _p(L, Td), Ha + ldt_pad, _p(L, xr), _p(L, b0a), _p(L, e0), _p(L, W), _p(L, b0b), _p(L, e1),
            _p(L, rw), len(rows), Ha, Hb, _p(L, G), Hb + ldg_pad)
    _run(L, HOPS, *args)
    first = G.clone()
    _untouched(buf, len(rows), Hb, Hb + ldg_pad, "gin hops")
    _run(L, HOPS, *args)
    assert torch.equal(first, G), "two launches differ"
    return (G, buf) if keep_device else _np(first)


def _ref_hops(c, rows=None, sums=False):
    return gq.hops(c["rowptr"], c["col"], c["val"], c["T"], c["eps0"], c["W0b"], c["b0b"], c["eps1"], c["rows"] if rows is None else rows,
                   xrow=c["xrow"], b0a=c["b0a"], sums=sums)


@pytest.mark.parametrize("case", gq.EXACT_HOPS_CASES, ids=str)
def test_hops_exact(L, case):
    c = gq.exact_hops_case(*case)
    ref = _ref_hops(c)
    got = _hops(L, c)
    _same(got[0], ref[0], f"gin hops {case}: the query without entries, (1 + eps1) h_q")
    _same(got, ref, f"gin hops {case}")


def _random_case(tag, Ha, Hb, q_degs, n_degs, with_xrow, with_bias):
    rng = _rng("gin-query-hops", tag, Ha, Hb)
    n_table = 41
    rowptr, col, val, xrow, n_rows = qr.query_csr(rng, q_degs, n_degs, n_table, with_xrow, pow2_val=False)
    T = rng.normal(0, 1, size=(n_table if with_xrow else n_rows, Ha)).astype(np.float32)
    W0b = (rng.normal(0, 1, size=(Hb, Ha)) / np.sqrt(Ha)).astype(np.float32)
    b0a = rng.normal(0, 1, size=Ha).astype(np.float32) if with_bias else None
    b0b = rng.normal(0, 1, size=Hb).astype(np.float32) if with_bias else None
    eps = rng.normal(0, 0.3, size=2).astype(np.float32)
    return dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=T, b0a=b0a, eps0=eps[0], W0b=W0b, b0b=b0b, eps1=eps[1],
                rows=np.arange(len(q_degs), dtype=np.int64), n_rows=n_rows)


@pytest.mark.parametrize("Ha,Hb,with_xrow,with_bias", [(64, 64, True, True), (512, 512, False, True), (260, 272, True, False)], ids=str)
def test_hops_random(L, Ha, Hb, with_xrow, with_bias):
    c = _random_case("random", Ha, Hb, gq.HOPS_QUERY_DEGS, gq.HOPS_ROW_DEGS, with_xrow, with_bias)
    ref, B = _ref_hops(c, sums=True)
    assert (ref == 0).any() and (ref > 0).any() and (c["T"] < 0).any()    # both ReLU branches reach the output
    _ratio(_hops(L, c), ref, B, f"gin hops random {(Ha, Hb)}")


@pytest.mark.parametrize("Q", [1, 3, 64, 257])
def test_hops_rows(L, Q):
    c = _random_case("rows", 64, 48, [3, 0, 7, 1, 12, 5, 2, 9, 4, 6, 18], [2, 5, 1, 9, 0, 3], True, True)
    rng = _rng("gin-query-rows", Q)
    rows = rng.integers(0, c["n_rows"], size=Q).astype(np.int64)   # unsorted, duplicates (Q > n_rows forces them), any row of the CSR
    if Q >= 3:
        rows[1] = rows[0]
    ref, B = _ref_hops(c, rows=rows, sums=True)
    _ratio(_hops(L, c, rows=rows), ref, B, f"gin hops rows Q={Q}")


def test_hops_errors(L):
    c = _random_case("align", 8, 16, [2, 1], [1, 2], False, False)
    Ha, Hb = 8, 16
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["val"]), _dev(c["rows"], torch.int64),
            _dev(np.array([c["eps0"], 0, 0, 0, c["eps1"]], dtype=np.float32))]
    rp, cl, vl, rw, eps = keep
    T = torch.zeros(c["n_rows"] * Ha + 8, dtype=torch.float32, device="cuda")
    W = torch.zeros(Hb * Ha + 8, dtype=torch.float32, device="cuda")
    out = torch.zeros(2 * Hb + 8, dtype=torch.float32, device="cuda")

    def call(T=T, ldt=Ha, W=W, out=out, ldg=Hb):   # eps needs no alignment: one float each, anywhere
        return _call(L, HOPS, _p(L, rp), _p(L, cl), _p(L, vl), _p(L, T), ldt, None, None, _p(L, eps[1:]), _p(L, W), None, _p(L, eps[4:]),
                     _p(L, rw), 2, Ha, Hb, _p(L, out), ldg)

    assert call() == 0
    assert call(T=T[1:]) == E_ALIGN and call(W=W[1:]) == E_ALIGN and call(out=out[1:]) == E_ALIGN
    assert call(ldt=Ha - 4) == E_BADARG and call(ldg=Hb - 4) == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# tail
# ---------------------------------------------------------------------------------------------------------------------------------
def _tail(L, c, log_softmax, G=None, ldg_pad=4, ldo_pad=3):
    Q, K = c["G"].shape if G is None else G.shape
    H2a, H2b, C = c["W1a"].shape[0], c["W1b"].shape[0], c["Wl"].shape[0]
    Gd = _strided(c["G"], K + ldg_pad) if G is None else G
    keep = [_dev(c["W1a"]), _opt(c["b1a"]), _dev(c["W1b"]), _opt(c["b1b"]), _dev(c["Wl"]), _opt(c["bl"])]
    W1a, b1a, W1b, b1b, Wl, bl = keep
    buf, out = _guarded(Q, C, C + ldo_pad, tail_rows=17)
    args = (_p(L, Gd), Gd.stride(0), Q, _p(L, W1a), _p(L, b1a), _p(L, W1b), _p(L, b1b), _p(L, Wl), _p(L, bl), K, H2a, H2b, C, _p(L, out),
            C + ldo_pad, int(log_softmax))
    _run(L, TAIL, *args)
    first = out.clone()
    _untouched(buf, Q, C, C + ldo_pad, "gin tail")
    _run(L, TAIL, *args)
    assert torch.equal(first, out), "two launches differ"
    return _np(first)


def _ref_tail(G, c, **kw):
    return gq.tail(G, c["W1a"], c["b1a"], c["W1b"], c["b1b"], c["Wl"], c["bl"], **kw)


@pytest.mark.parametrize("case", gq.EXACT_TAIL_CASES, ids=str)
def test_tail_exact(L, case):
    c = gq.exact_tail_case(*case)
    logits = _ref_tail(c["G"], c)
    _same(_tail(L, c, False), logits, f"gin tail {case}")
    # exact logits: only the log-softmax itself rounds
    _ratio(_tail(L, c, True), _ref_tail(c["G"], c, log_softmax=True), qr.log_softmax_bound(logits, np.zeros_like(logits)),
           f"gin tail log-softmax of exact logits {case}")


@pytest.mark.parametrize("K,H2a,H2b,C,Q", [(64, 64, 64, 7, 17), (272, 80, 48, 47, 22), (512, 512, 512, 48, 16)], ids=str)
def test_tail_random(L, K, H2a, H2b, C, Q):
    rng = _rng("gin-query-tail", K, H2a, H2b, C, Q)
    n = lambda *s: rng.normal(0, 1, size=s)   # noqa: E731
    c = dict(G=n(Q, K).astype(np.float32), W1a=(n(H2a, K) / np.sqrt(K)).astype(np.float32), b1a=n(H2a).astype(np.float32),
             W1b=(n(H2b, H2a) / np.sqrt(H2a)).astype(np.float32), b1b=n(H2b).astype(np.float32),
             Wl=(n(C, H2b) / np.sqrt(H2b)).astype(np.float32), bl=n(C).astype(np.float32))
    logits, B = _ref_tail(c["G"], c, sums=True)
    _ratio(_tail(L, c, False), logits, B, f"gin tail logits {(K, H2a, H2b, C, Q)}")
    _ratio(_tail(L, c, True), _ref_tail(c["G"], c, log_softmax=True), qr.log_softmax_bound(logits, B),
           f"gin tail log-softmax {(K, H2a, H2b, C, Q)}")


def test_tail_errors(L):
    rng = _rng("gin-query-tail-align")
    Q, K, H2a, H2b, C = 3, 8, 16, 32, 4
    G = torch.zeros(Q * K + 8, dtype=torch.float32, device="cuda")
    W1a, W1b, Wl = _dev(rng.normal(size=(H2a, K))), _dev(rng.normal(size=(H2b, H2a))), _dev(rng.normal(size=(C, H2b)))
    out = torch.zeros(Q * C + 8, dtype=torch.float32, device="cuda")

    def call(G=G, ldg=K, out=out, H2a=H2a, H2b=H2b):
        return _call(L, TAIL, _p(L, G), ldg, Q, _p(L, W1a), None, _p(L, W1b), None, _p(L, Wl), None, K, H2a, H2b, C, _p(L, out), C, 0)

    assert call() == 0
    assert call(G=G[1:]) == E_ALIGN and call(out=out[1:]) == E_ALIGN
    assert call(ldg=K - 4) == E_BADARG
    assert L.lib().fitgnn_gin_query_tail_lds_bytes(1024, 1024, C) > 160 * 1024
    assert call(H2a=1024, H2b=1024) == E_BADARG     # refused before any pointer is read


@pytest.mark.parametrize("case", gq.CHAIN_CASES, ids=str)
def test_hops_then_tail_exact(L, case):
    c = gq.exact_chain_case(*case)
    Gref = _ref_hops(c)
    ref = _ref_tail(Gref, c)
    G, gbuf = _hops(L, c, keep_device=True)
    _same(_np(G), Gref, f"gin chain {case}: G")
    _same(_tail(L, c, False, G=G), ref, f"gin chain {case}: logits")
