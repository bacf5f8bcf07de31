"""GPU tier: the two graph-query kernels of csrc/query.hip through the C ABI against the float64 references of
tests/graph_query_reference.py (the convention and helpers of tests/test_gpu_step_kernels.py and tests/test_gpu_query_kernels.py).

EXACT inputs (tests/graph_query_reference.py: integers over a power of two, power-of-two CSR values, every pre-activation >= 0 or
<= -32 where fp32 ELU is exactly -1, power-of-two segment lengths under the mean; proven exact on the CPU by
tests/test_graph_query_reference_cpu.py) must come back bit for bit.  RANDOM inputs are held per entry to 2^-24 times the first-order
bound the reference accumulates along the kernel's own operation order (docstrings of graph_query_reference.hops / pooled_tail /
softmax_bound: one rounding per fmaf, per add and for the division, expm1f / expf within 1 ulp as the HIP math API states); nothing
is added on top.  Every launch is made twice and must give the same bits; G and out are NaN-guarded behind and beside their rows.

Launcher -> branch -> tests that reach it:

| launcher | branch (from the launch and kernel code) | tests |
|---|---|---|
| fitgnn_gcn_graph_query_hops_f32 | column slabs: H = 4 (one live lane, a 16-byte window row), 64, 256 (one full slab), 260 (second slab, one live lane, window rows of 256), 512 | test_hops_exact[*], test_hops_random[*] |
| | graph row counts 1, 2, 3 (waves without a row), 4 (one each), 5 (wave 0 has two), 17; the same counts of pooled rows dealt to the waves | test_hops_exact[*] |
| | row degree 0 (phase 1: ELU(b0); phase 2: zeros over a NaN-filled G), 1, 63, 64, 65 (second 64-entry batch) in both phases; groups of four with 1-3 missing | test_hops_exact[*] |
| | pooled rows: all rows, the first half, a non-contiguous descending subset, none (pptr[i] == pptr[i + 1]: nothing written) | test_hops_exact[*] |
| | graphs unsorted with one repeated; Q = 1, 3, 257 | test_hops_exact[*], test_hops_graphs |
| | xrow NULL / given with repeated table rows and an entry at the last table row (NaN behind T); b0 NULL / given; ldt > H, ldg > H | test_hops_exact[*] |
| | the largest window fitgnn_gcn_graph_query_hops_lds_bytes allows at H (10 240 rows at H = 4, 640 at 64, 160 at 256 / 260 / 512: 160 KiB of dynamic LDS) exact; one more row -> FITGNN_E_BADARG, G untouched | test_hops_largest_window[*] |
| | a graph of more rows than max_rows: the workgroup returns, its rows of G are not written | test_hops_skips_a_graph_beyond_max_rows |
| | RANDOM values of both signs (both ELU branches, expm1f) | test_hops_random[*], test_hops_graphs |
| | T or G one float into its buffer -> FITGNN_E_ALIGN | test_hops_misaligned |
| fitgnn_gcn_graph_query_tail_f32 | (H, H2) = (4, 16) one k-step, one column block; (64, 64) two k-stages; (68, 80) a 4-wide last stage, a fifth block on wave 1; (512, 512) two column passes of 256, two pooled columns per thread | test_tail_exact[*] |
| | C = 1, 7, 47, 48; segment lengths 0 (p = 0: out = bl), 1, 15, 16 (a full tile), 17 (a second tile of one row), 33 (three tiles); under the mean 0, 1, 2, 4, 16, 32 exact and 0, 1, 15, 16, 17, 33 RANDOM | test_tail_exact[*], test_tail_random[*] |
| | pool max / mean; b1 NULL / given, bl NULL / given; ldg > H, ldo > C | test_tail_exact[*] |
| | dead tile rows (z = ELU(b1) = 32 against live z = -1) must not enter the pool | test_tail_dead_rows_stay_out[*] |
| | a following segment 1024 times larger must not enter the pool | test_tail_neighbour_rows_stay_out[*] |
| | softmax off / on, logits 1e4 apart (expf underflows to 0, the row still sums to 1); RANDOM operands | test_tail_random[*] |
| | Q = 1, 3, 257 | test_tail_graphs |
| | b1 and bl NULL (an empty segment then gives zeros) | test_tail_without_biases |
| | G or out one float into its buffer -> FITGNN_E_ALIGN | test_tail_misaligned |

Worst observed error / bound per family on one MI355X run: hops random 0.57 (H = 512), hops graphs 0.53 (Q = 257); tail logits 0.027
and tail softmax 0.006 (0.002 or less at H = H2 = 512, where the worst-case chain bound is loosest).
"""
import numpy as np
import pytest
import torch

import graph_query_reference as gq
from test_gpu_query_kernels import _guarded, _ratio, _untouched
from test_gpu_step_kernels import E_ALIGN, E_BADARG, L, _call, _dev, _np, _p, _rng, _run, _same, _strided  # noqa: F401

pytestmark = pytest.mark.gpu

HOPS, TAIL = "fitgnn_gcn_graph_query_hops_f32", "fitgnn_gcn_graph_query_tail_f32"


def _hops_args(L, c, ldt_pad=4, ldg_pad=8, max_rows=None):
    H, P = c["T"].shape[1], len(c["prow"])
    Td = _strided(c["T"], H + ldt_pad)
    buf, G = _guarded(P, H, H + ldg_pad)
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["val"]),
            None if c["xrow"] is None else _dev(c["xrow"], torch.int32), None if c["b0"] is None else _dev(c["b0"]),
            _dev(c["seg"], torch.int64), _dev(c["prow"], torch.int64), _dev(c["pptr"], torch.int64), Td]
    rp, cl, vl, xr, b0, sg, pr, pp, _ = keep
    args = (_p(L, rp), _p(L, cl), _p(L, vl), _p(L, Td), H + ldt_pad, _p(L, xr), _p(L, b0), _p(L, sg), _p(L, pr), _p(L, pp), len(c["seg"]), H,
            c["max_rows"] if max_rows is None else max_rows, _p(L, G), H + ldg_pad)
    return args, buf, G, keep


def _hops(L, c):
    args, buf, G, keep = _hops_args(L, c)
    H, P = c["T"].shape[1], len(c["prow"])
    _run(L, HOPS, *args)
    first = G.clone()
    _untouched(buf, P, H, G.stride(0), "hops")
    _run(L, HOPS, *args)
    assert torch.equal(first, G), "two launches differ"
    return _np(first)


def _hops_ref(c, **kw):
    return gq.hops(c["rowptr"], c["col"], c["val"], c["T"], c["seg"], c["prow"], c["pptr"], xrow=c["xrow"], b0=c["b0"], **kw)


@pytest.mark.parametrize("case", gq.EXACT_HOPS_CASES, ids=str)
def test_hops_exact(L, case):
    c = gq.hops_case(*case)
    got = _hops(L, c)
    deg = np.diff(c["rowptr"])[c["prow"]]
    assert (deg == 0).any() and np.all(got[deg == 0] == 0), "a pooled row without entries must give zeros"
    _same(got, _hops_ref(c, f32_elu=True), f"hops {case}")


@pytest.mark.parametrize("H,with_xrow,with_b0", [(4, False, True), (64, True, True), (256, False, False), (260, True, False),
                                                 (512, False, True)], ids=str)
def test_hops_random(L, H, with_xrow, with_b0):
    c = gq.hops_case(H, with_xrow, with_b0, exact=False)
    ref, B = _hops_ref(c, sums=True)
    _ratio(_hops(L, c), ref, B, f"hops random H={H}")


@pytest.mark.parametrize("Q", [1, 3, 257])
def test_hops_graphs(L, Q):
    c = gq.hops_case(64, True, True, exact=False, tag=Q)
    rng = _rng("graph-hops", Q)
    graphs = rng.integers(0, len(gq.HOPS_SIZES), size=Q)    # unsorted, repeats (Q > 6 forces them)
    if Q >= 3:
        graphs[1] = graphs[0]
    c["seg"], c["prow"], c["pptr"] = gq.pooled_rows(rng, c["gptr"], graphs.tolist(), ["all", "subset", "first", "all", "none"])
    c["max_rows"] = int((c["seg"][:, 1] - c["seg"][:, 0]).max())
    ref, B = _hops_ref(c, sums=True)
    _ratio(_hops(L, c), ref, B, f"hops graphs Q={Q}")


@pytest.mark.parametrize("H", [4, 64, 256, 260, 512])
def test_hops_largest_window(L, H):
    n = 160 * 1024 // int(L.lib().fitgnn_gcn_graph_query_hops_lds_bytes(1, H))
    assert L.lib().fitgnn_gcn_graph_query_hops_lds_bytes(n, H) == 160 * 1024
    c = gq.window_case(H, n)
    _same(_hops(L, c), _hops_ref(c, f32_elu=True), f"hops window H={H} rows={n}")
    args, buf, G, keep = _hops_args(L, gq.window_case(H, n + 1))   # a graph of one more row
    assert _call(L, HOPS, *args) == E_BADARG
    assert torch.isnan(buf).all(), "a refused launch wrote G"


def test_hops_skips_a_graph_beyond_max_rows(L):
    """max_rows = 5 sizes the window for the graphs of up to 5 rows: the graph of 17 rows is left out -- its rows of G stay NaN -- and
    every other graph is answered as before (GraphQueryEngine sends such a graph's rows through the per-row gather)."""
    c = gq.hops_case(64, True, True)
    args, buf, G, keep = _hops_args(L, c, max_rows=5)
    _run(L, HOPS, *args)
    got, ref = _np(G), _hops_ref(c, f32_elu=True)
    size = c["seg"][:, 1] - c["seg"][:, 0]
    skipped = np.repeat(size > 5, np.diff(c["pptr"]))
    assert skipped.any() and not skipped.all() and np.isnan(got[skipped]).all()
    _same(got[~skipped], ref[~skipped], "hops beside a skipped graph")


def test_hops_misaligned(L):
    c = gq.hops_case(8, False, False, exact=False)
    H, P, n = 8, len(c["prow"]), int(c["gptr"][-1])
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["val"]), _dev(c["seg"], torch.int64),
            _dev(c["prow"], torch.int64), _dev(c["pptr"], torch.int64)]
    rp, cl, vl, sg, pr, pp = keep
    T = torch.zeros(n * H + 8, dtype=torch.float32, device="cuda")
    out = torch.zeros(P * H + 8, dtype=torch.float32, device="cuda")
    good = (_p(L, rp), _p(L, cl), _p(L, vl), _p(L, T), H, None, None, _p(L, sg), _p(L, pr), _p(L, pp), len(c["seg"]), H, c["max_rows"],
            _p(L, out), H)
    assert _call(L, HOPS, *good) == 0
    assert _call(L, HOPS, *good[:3], _p(L, T[1:]), *good[4:]) == E_ALIGN
    assert _call(L, HOPS, *good[:13], _p(L, out[1:]), H) == E_ALIGN


# ---------------------------------------------------------------------------------------------------------------------------------
# tail
# ---------------------------------------------------------------------------------------------------------------------------------
def _tail(L, c, pool, softmax, ldg_pad=4, ldo_pad=3):
    P, H = c["G"].shape
    H2, C, Q = c["W1"].shape[0], c["Wl"].shape[0], len(c["pptr"]) - 1
    Gd = _strided(c["G"], H + ldg_pad)
    keep = [_dev(c["W1"]), None if c["b1"] is None else _dev(c["b1"]), _dev(c["Wl"]), None if c["bl"] is None else _dev(c["bl"]),
            _dev(c["pptr"], torch.int64)]
    W1, b1, Wl, bl, pp = keep
    buf, out = _guarded(Q, C, C + ldo_pad, tail_rows=3)
    args = (_p(L, Gd), H + ldg_pad, _p(L, pp), Q, _p(L, W1), _p(L, b1), _p(L, Wl), _p(L, bl), H, H2, C, {"max": 0, "mean": 1}[pool],
            int(softmax), _p(L, out), C + ldo_pad)
    _run(L, TAIL, *args)
    first = out.clone()
    _untouched(buf, Q, C, C + ldo_pad, "tail")
    _run(L, TAIL, *args)
    assert torch.equal(first, out), "two launches differ"
    return _np(first)


def _tail_ref(c, pool, **kw):
    return gq.pooled_tail(c["G"], c["pptr"], c["W1"], c["b1"], c["Wl"], c["bl"], pool=pool, **kw)


@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("case", gq.EXACT_TAIL_CASES, ids=str)
def test_tail_exact(L, case, pool):
    c = gq.exact_tail_case(*case, pool)
    _same(_tail(L, c, pool, False), _tail_ref(c, pool, f32_elu=True, f32_div=True), f"tail {case} {pool}")


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_tail_dead_rows_stay_out(L, pool):
    c = gq.dead_rows_case(pool)
    _same(_tail(L, c, pool, False), _tail_ref(c, pool, f32_elu=True, f32_div=True), f"tail dead rows {pool}")


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_tail_neighbour_rows_stay_out(L, pool):
    c = gq.neighbour_case(pool)
    _same(_tail(L, c, pool, False), _tail_ref(c, pool, f32_elu=True, f32_div=True), f"tail neighbour rows {pool}")


def _random_tail_case(tag, H, H2, C, lens, extreme=False):
    rng = _rng("graph-tail", tag, H, H2, C)
    pptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    P = int(pptr[-1])
    c = dict(G=rng.normal(0, 1, size=(P, H)).astype(np.float32), W1=(rng.normal(0, 1, size=(H2, H)) / np.sqrt(H)).astype(np.float32),
             b1=rng.normal(0, 1, size=H2).astype(np.float32), Wl=(rng.normal(0, 1, size=(C, H2)) / np.sqrt(H2)).astype(np.float32),
             bl=rng.normal(0, 1, size=C).astype(np.float32), pptr=pptr)
    if extreme:   # logits 1e4 apart: one class far above the others
        c["bl"][0] = 1e4
    return c


@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("H,H2,C,extreme", [(4, 16, 1, False), (64, 64, 7, False), (68, 80, 47, True), (512, 512, 48, False)], ids=str)
def test_tail_random(L, H, H2, C, extreme, pool):
    c = _random_tail_case("random", H, H2, C, gq.TAIL_SEGMENTS, extreme)
    logits, B = _tail_ref(c, pool, sums=True)
    _ratio(_tail(L, c, pool, False), logits, B, f"tail logits {(H, H2, C, pool)}")
    if extreme:
        assert (logits.max(1) - logits.min(1)).min() >= 1e4 - 100
    got = _tail(L, c, pool, True)
    _ratio(got, _tail_ref(c, pool, softmax=True), gq.softmax_bound(logits, B), f"tail softmax {(H, H2, C, pool)}")
    # s = sum_c e_c carries C - 1 roundings and every quotient one: the row sums to 1 within C units, first order (+ 2 for the rest)
    assert np.abs(got.sum(1) - 1).max() <= (C + 2) * 2.0 ** -24


@pytest.mark.parametrize("Q", [1, 3, 257])
def test_tail_graphs(L, Q):
    lens = _rng("graph-tail-lens", Q).integers(0, 20, size=Q).tolist()
    for pool, softmax in (("max", True), ("mean", False)):
        c = _random_tail_case(("graphs", Q), 64, 64, 7, lens)
        logits, B = _tail_ref(c, pool, sums=True)
        ref, bound = (_tail_ref(c, pool, softmax=True), gq.softmax_bound(logits, B)) if softmax else (logits, B)
        _ratio(_tail(L, c, pool, softmax), ref, bound, f"tail graphs Q={Q} {pool}")


def test_tail_without_biases(L):
    c = _random_tail_case("nobias", 68, 80, 7, [3, 17, 0, 1])
    c["b1"] = c["bl"] = None
    for pool in ("max", "mean"):
        logits, B = _tail_ref(c, pool, sums=True)
        got = _tail(L, c, pool, False)
        assert np.all(got[2] == 0), "an empty segment without bl gives zeros"
        _ratio(got, logits, B, f"tail no biases {pool}")


def test_tail_misaligned(L):
    rng = _rng("graph-tail-align")
    P, H, H2, C = 5, 8, 16, 4
    G = torch.zeros(P * H + 8, dtype=torch.float32, device="cuda")
    W1, Wl = _dev(rng.normal(size=(H2, H))), _dev(rng.normal(size=(C, H2)))
    pp = _dev(np.array([0, 2, 5]), torch.int64)
    out = torch.zeros(2 * C + 8, dtype=torch.float32, device="cuda")
    good = (_p(L, G), H, _p(L, pp), 2, _p(L, W1), None, _p(L, Wl), None, H, H2, C, 0, 1, _p(L, out), C)
    assert _call(L, TAIL, *good) == 0
    assert _call(L, TAIL, _p(L, G[1:]), *good[1:]) == E_ALIGN
    assert _call(L, TAIL, *good[:13], _p(L, out[1:]), C) == E_ALIGN
