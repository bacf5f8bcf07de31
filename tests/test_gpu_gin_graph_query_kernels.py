"""GPU tier: the two GIN graph-query kernels of csrc/query.hip through the C ABI against the float64 references of
tests/gin_graph_query_reference.py (the convention and helpers of tests/test_gpu_graph_query_kernels.py and
tests/test_gpu_gin_query_kernels.py).

EXACT inputs (integers over a power of two, power-of-two CSR values, 1 + eps = 1.5 or 0.75, power-of-two segment lengths under the
mean; proven exact on the CPU by tests/test_gin_graph_query_reference_cpu.py) must come back bit for bit -- and bit for bit equal to
fitgnn_gin_query_hops_f32 on the same pooled rows, whose fold differs only in its order.  RANDOM inputs are held per entry to 2^-24
times the first-order bound the reference accumulates along the kernel's own operation order (one rounding per fmaf, per add and for
the division; expf within 1 ulp under the softmax); nothing is added on top.  Every launch is made twice and must give the same bits;
G and out are NaN-guarded behind and beside their rows.

| launcher | branch | tests |
|---|---|---|
| fitgnn_gin_graph_query_hops_f32 | (Ha, Hb) = (4, 16) one k-step, one column block, a 20-float window row; (40, 16) an 8-wide last k-stage; (64, 64); (256, 256) one full slab; (260, 272) a second slab of one block, a second slot with one live lane; (512, 512) two slots, two slabs; (272, 48) two slots, one slab; (64, 272) one slot, two slabs | test_hops_exact[*], test_hops_random[*] |
| | graphs of 1, 2, 3 rows (waves without a row), 4, 5, 15 (one row short of a tile), 16 (one tile), 17 (one row into a second), 33 (three tiles); unsorted, one twice | test_hops_exact[*] |
| | row degrees 0 (a_r = ReLU(o0 root + b0a); a pooled row: fmaf(o1, h_r, 0)), 1, 2, 5, 63, 64, 65 (a second 64-entry batch) in both phases | test_hops_exact[*] |
| | pooled rows: all of a graph, the first half, a non-contiguous descending subset, one, none (nothing written) | test_hops_exact[*] |
| | xrow, b0a, b0b NULL / given; eps 0.5 and -0.25; ldt > Ha, ldg > Hb | test_hops_exact[*] |
| | a graph of exactly gin_graph_query_max_rows(Ha, Hb) rows at (64, 64) and (512, 512); one more row in max_rows -> FITGNN_E_BADARG, G untouched | test_hops_largest_window[*] |
| | a graph of more rows than max_rows: the workgroup returns, its rows of a pre-filled G stay, its neighbours are written | test_hops_largest_window[*], test_hops_skips_a_graph_beyond_max_rows |
| | T, W0b or G one float into its buffer -> FITGNN_E_ALIGN | test_hops_misaligned |
| fitgnn_gin_graph_query_tail_f32 | (K, H2a, H2b, C) = (16, 16, 16, 1), (64, 64, 64, 7), (272, 80, 48, 47), (512, 512, 512, 48); segments of 0 (p = 0: out = bl), 1, 15, 16, 17, 33 rows (mean, EXACT: 0, 1, 16, 2, 32, 4); max / mean; softmax off / on; biases NULL / given | test_tail_exact[*], test_tail_random[*] |
| | dead tile rows (z2 = 33 against live 17) must not enter the pool | test_tail_dead_rows_stay_out[*] |
| | a following segment 1024 times larger must not enter the pool | test_tail_neighbour_rows_stay_out[*] |
| | segments of one row each, softmax off: fitgnn_gin_query_tail_f32's bits | test_tail_of_single_rows_is_the_node_tail |
| | G or out one float into its buffer -> FITGNN_E_ALIGN | test_tail_misaligned |
| both | hops -> tail on EXACT inputs, max and mean | test_hops_then_tail_exact[*] |
"""
import numpy as np
import pytest
import torch

import gin_graph_query_reference as ggq
from test_gpu_query_kernels import _guarded, _ratio, _untouched
from test_gpu_step_kernels import E_ALIGN, E_BADARG, L, _call, _dev, _np, _p, _run, _same, _strided  # noqa: F401

pytestmark = pytest.mark.gpu

HOPS, TAIL = "fitgnn_gin_graph_query_hops_f32", "fitgnn_gin_graph_query_tail_f32"
NODE_HOPS, NODE_TAIL = "fitgnn_gin_query_hops_f32", "fitgnn_gin_query_tail_f32"


def _opt(a, dtype=torch.float32):
    return None if a is None else _dev(a, dtype)


def _hops_args(L, c, ldt_pad=4, ldg_pad=8, max_rows=None, fill=float("nan")):
    Ha, Hb, P = c["T"].shape[1], c["W0b"].shape[0], len(c["prow"])
    Td = _strided(c["T"], Ha + ldt_pad)
    buf, G = _guarded(P, Hb, Hb + ldg_pad)
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["val"]), _opt(c["xrow"], torch.int32), _opt(c["b0a"]),
            _dev(np.array([c["eps0"]], dtype=np.float32)), _dev(c["W0b"]), _opt(c["b0b"]), _dev(np.array([c["eps1"]], dtype=np.float32)),
            _dev(c["seg"], torch.int64), _dev(c["prow"], torch.int64), _dev(c["pptr"], torch.int64), Td]
    rp, cl, vl, xr, b0a, e0, W, b0b, e1, sg, pr, pp, _ = keep
    front = (_p(L, rp), _p(L, cl), _p(L, vl), _p(L, Td), Ha + ldt_pad, _p(L, xr), _p(L, b0a), _p(L, e0), _p(L, W), _p(L, b0b), _p(L, e1))
    args = front + (_p(L, sg), _p(L, pr), _p(L, pp), len(c["seg"]), Ha, Hb, c["max_rows"] if max_rows is None else max_rows, _p(L, G),
                    Hb + ldg_pad)
    node = front + (_p(L, pr), P, Ha, Hb)      # fitgnn_gin_query_hops_f32 on the same pooled rows: + (G, ldg)
    return args, node, buf, G, keep


def _hops(L, c, keep_device=False):
    args, node, buf, G, keep = _hops_args(L, c)
    Hb, P = c["W0b"].shape[0], len(c["prow"])
    _run(L, HOPS, *args)
    first = G.clone()
    _untouched(buf, P, Hb, G.stride(0), "gin graph hops")
    _run(L, HOPS, *args)
    assert torch.equal(first, G), "two launches differ"
    return (G, buf, node, keep) if keep_device else _np(first)


def _hops_ref(c, **kw):
    return ggq.hops(c["rowptr"], c["col"], c["val"], c["T"], c["eps0"], c["W0b"], c["b0b"], c["eps1"], c["seg"], c["prow"], c["pptr"],
                    xrow=c["xrow"], b0a=c["b0a"], **kw)


@pytest.mark.parametrize("case", ggq.EXACT_HOPS_CASES, ids=str)
def test_hops_exact(L, case):
    c = ggq.hops_case(*case)
    G, buf, node, keep = _hops(L, c, keep_device=True)
    got = _np(G)
    _same(got, _hops_ref(c), f"gin graph hops {case}")
    # the per-row kernel on the same pooled rows: exact inputs remove the fold-order difference
    P, Hb = got.shape
    nbuf, Gn = _guarded(P, Hb, Hb + 8)
    _run(L, NODE_HOPS, *node, _p(L, Gn), Hb + 8)
    assert torch.equal(Gn, G), f"gin graph hops {case}: differs from fitgnn_gin_query_hops_f32 on the same rows"


@pytest.mark.parametrize("case", ggq.EXACT_HOPS_CASES, ids=str)
def test_hops_random(L, case):
    c = ggq.hops_case(*case, exact=False)
    ref, B = _hops_ref(c, sums=True)
    assert (ref == 0).any() and (ref > 0).any() and (c["T"] < 0).any()    # both ReLU branches reach the output
    _ratio(_hops(L, c), ref, B, f"gin graph hops random {case[:2]}")


@pytest.mark.parametrize("Ha,Hb", [(64, 64), (512, 512)])
def test_hops_largest_window(L, Ha, Hb):
    """A graph of exactly gin_graph_query_max_rows rows fills the 160 KiB; with one row more it is skipped by the launch -- its rows of a
    pre-filled G stay as they were -- while both its neighbours are written; a window sized for it is refused."""
    from fitgnn_amd import ops
    n = ops.gin_graph_query_max_rows(Ha, Hb)
    lds = L.lib().fitgnn_gin_graph_query_hops_lds_bytes
    assert n == {(64, 64): 450, (512, 512): 90}[(Ha, Hb)] and lds(n, Ha, Hb) <= 160 * 1024 < lds(n + 1, Ha, Hb)
    c = ggq.window_case(Ha, Hb, n)
    _same(_hops(L, c), _hops_ref(c), f"gin graph hops window {(Ha, Hb)} rows={n}")
    c = ggq.window_case(Ha, Hb, n + 1)
    args, node, buf, G, keep = _hops_args(L, c, max_rows=n + 1)
    assert _call(L, HOPS, *args) == E_BADARG
    assert torch.isnan(buf).all(), "a refused launch wrote G"
    args, node, buf, G, keep = _hops_args(L, c, max_rows=n)
    G.fill_(-7.0)
    _run(L, HOPS, *args)
    got, ref = _np(G), _hops_ref(c)
    skipped = np.repeat(c["seg"][:, 1] - c["seg"][:, 0] > n, np.diff(c["pptr"]))
    assert skipped.sum() == n + 1 and (~skipped).sum() == 5 and not skipped[:3].any() and not skipped[-2:].any()
    assert (got[skipped] == -7.0).all(), "a graph beyond max_rows was written"
    _same(got[~skipped], ref[~skipped], "gin graph hops beside a skipped graph")


def test_hops_skips_a_graph_beyond_max_rows(L):
    """max_rows = 5 sizes the window for the graphs of up to 5 rows: the larger ones are left out -- their rows of G stay NaN -- and
    every other graph is answered as before (GraphQueryEngine sends such a graph's rows through fitgnn_gin_query_hops_f32)."""
    c = ggq.hops_case(64, 64, True, True, 0.5, 0.5)
    args, node, buf, G, keep = _hops_args(L, c, max_rows=5)
    _run(L, HOPS, *args)
    got, ref = _np(G), _hops_ref(c)
    skipped = np.repeat(c["seg"][:, 1] - c["seg"][:, 0] > 5, np.diff(c["pptr"]))
    assert skipped.any() and not skipped.all() and np.isnan(got[skipped]).all()
    _same(got[~skipped], ref[~skipped], "gin graph hops beside skipped graphs")


def test_hops_misaligned(L):
    c = ggq.hops_case(8, 16, False, False, 0.5, -0.25, exact=False)
    Ha, Hb, P, n = 8, 16, len(c["prow"]), int(c["gptr"][-1])
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["val"]), _dev(c["seg"], torch.int64),
            _dev(c["prow"], torch.int64), _dev(c["pptr"], torch.int64), _dev(np.array([0.5, 0, 0, 0, -0.25], dtype=np.float32))]
    rp, cl, vl, sg, pr, pp, eps = keep
    T = torch.zeros(n * Ha + 8, dtype=torch.float32, device="cuda")
    W = torch.zeros(Hb * Ha + 8, dtype=torch.float32, device="cuda")
    out = torch.zeros(P * Hb + 8, dtype=torch.float32, device="cuda")

    def call(T=T, ldt=Ha, W=W, out=out, ldg=Hb):   # eps needs no alignment: one float each, anywhere
        return _call(L, HOPS, _p(L, rp), _p(L, cl), _p(L, vl), _p(L, T), ldt, None, None, _p(L, eps[1:]), _p(L, W), None, _p(L, eps[4:]),
                     _p(L, sg), _p(L, pr), _p(L, pp), len(c["seg"]), Ha, Hb, c["max_rows"], _p(L, out), ldg)

    assert call() == 0
    assert call(T=T[1:]) == E_ALIGN and call(W=W[1:]) == E_ALIGN and call(out=out[1:]) == E_ALIGN
    assert call(ldt=Ha - 4) == E_BADARG and call(ldg=Hb - 4) == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# tail
# ---------------------------------------------------------------------------------------------------------------------------------
def _tail(L, c, pool, softmax, G=None, ldg_pad=4, ldo_pad=3):
    P, K = c["G"].shape if G is None else G.shape
    H2a, H2b, C, Q = c["W1a"].shape[0], c["W1b"].shape[0], c["Wl"].shape[0], len(c["pptr"]) - 1
    Gd = _strided(c["G"], K + ldg_pad) if G is None else G
    keep = [_dev(c["W1a"]), _opt(c["b1a"]), _dev(c["W1b"]), _opt(c["b1b"]), _dev(c["Wl"]), _opt(c["bl"]), _dev(c["pptr"], torch.int64)]
    W1a, b1a, W1b, b1b, Wl, bl, pp = keep
    buf, out = _guarded(Q, C, C + ldo_pad, tail_rows=3)
    args = (_p(L, Gd), Gd.stride(0), _p(L, pp), Q, _p(L, W1a), _p(L, b1a), _p(L, W1b), _p(L, b1b), _p(L, Wl), _p(L, bl), K, H2a, H2b, C,
            {"max": 0, "mean": 1}[pool], int(softmax), _p(L, out), C + ldo_pad)
    _run(L, TAIL, *args)
    first = out.clone()
    _untouched(buf, Q, C, C + ldo_pad, "gin graph tail")
    _run(L, TAIL, *args)
    assert torch.equal(first, out), "two launches differ"
    return _np(first)


def _tail_ref(G, c, pool, **kw):
    return ggq.pooled_tail(G, c["pptr"], c["W1a"], c["b1a"], c["W1b"], c["b1b"], c["Wl"], c["bl"], pool=pool, **kw)


@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("case", ggq.TAIL_CASES, ids=str)
def test_tail_exact(L, case, pool):
    c = ggq.tail_case(*case, pool)
    logits = _tail_ref(c["G"], c, pool, f32_div=True)
    _same(_tail(L, c, pool, False), logits, f"gin graph tail {case} {pool}")
    # exact logits: only the softmax itself rounds
    _ratio(_tail(L, c, pool, True), _tail_ref(c["G"], c, pool, softmax=True, f32_div=True), ggq.softmax_bound(logits, np.zeros_like(logits)),
           f"gin graph tail softmax of exact logits {case} {pool}")


@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("case", ggq.TAIL_CASES, ids=str)
def test_tail_random(L, case, pool):
    c = ggq.tail_case(*case, pool, exact=False)
    logits, B = _tail_ref(c["G"], c, pool, sums=True)
    _ratio(_tail(L, c, pool, False), logits, B, f"gin graph tail logits {case} {pool}")
    got = _tail(L, c, pool, True)
    _ratio(got, _tail_ref(c["G"], c, pool, softmax=True), ggq.softmax_bound(logits, B), f"gin graph tail softmax {case} {pool}")
    C = case[3]
    # s = sum_c e_c carries C - 1 roundings and every quotient one: the row sums to 1 within C units, first order (+ 2 for the rest)
    assert np.abs(got.sum(1) - 1).max() <= (C + 2) * 2.0 ** -24


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_tail_dead_rows_stay_out(L, pool):
    c = ggq.dead_rows_case(pool)
    _same(_tail(L, c, pool, False), _tail_ref(c["G"], c, pool, f32_div=True), f"gin graph tail dead rows {pool}")


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_tail_neighbour_rows_stay_out(L, pool):
    c = ggq.neighbour_case(pool)
    _same(_tail(L, c, pool, False), _tail_ref(c["G"], c, pool, f32_div=True), f"gin graph tail neighbour rows {pool}")


def test_tail_of_single_rows_is_the_node_tail(L):
    """Segments of one row each, no softmax: the pool is the identity (max: the first row; mean: s = 0 + z, s / 1), and the output is
    fitgnn_gin_query_tail_f32's without its log-softmax, bit for bit, on RANDOM operands."""
    c = ggq.tail_case(272, 80, 48, 47, True, "max", exact=False)
    P, K = c["G"].shape
    c["pptr"] = np.arange(P + 1, dtype=np.int64)
    Gd = _strided(c["G"], K + 4)
    keep = [_dev(c["W1a"]), _dev(c["b1a"]), _dev(c["W1b"]), _dev(c["b1b"]), _dev(c["Wl"]), _dev(c["bl"])]
    W1a, b1a, W1b, b1b, Wl, bl = keep
    buf, out = _guarded(P, 47, 50, tail_rows=17)
    _run(L, NODE_TAIL, _p(L, Gd), K + 4, P, _p(L, W1a), _p(L, b1a), _p(L, W1b), _p(L, b1b), _p(L, Wl), _p(L, bl), K, 80, 48, 47, _p(L, out),
         50, 0)
    node = _np(out)
    for pool in ("max", "mean"):
        assert np.array_equal(_tail(L, c, pool, False, G=Gd), node), pool


def test_tail_misaligned(L):
    P, K, H2a, H2b, C = 5, 8, 16, 32, 4
    rng = np.random.default_rng(67)
    G = torch.zeros(P * K + 8, dtype=torch.float32, device="cuda")
    W1a, W1b, Wl = _dev(rng.normal(size=(H2a, K))), _dev(rng.normal(size=(H2b, H2a))), _dev(rng.normal(size=(C, H2b)))
    pp = _dev(np.array([0, 2, 5]), torch.int64)
    out = torch.zeros(2 * C + 8, dtype=torch.float32, device="cuda")

    def call(G=G, ldg=K, out=out, H2a=H2a, H2b=H2b):
        return _call(L, TAIL, _p(L, G), ldg, _p(L, pp), 2, _p(L, W1a), None, _p(L, W1b), None, _p(L, Wl), None, K, H2a, H2b, C, 0, 1,
                     _p(L, out), C)

    assert call() == 0
    assert call(G=G[1:]) == E_ALIGN and call(out=out[1:]) == E_ALIGN
    assert call(ldg=K - 4) == E_BADARG
    assert call(H2a=1024, H2b=1024) == E_BADARG     # refused before any pointer is read


@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("case", ggq.CHAIN_CASES, ids=str)
def test_hops_then_tail_exact(L, case, pool):
    c = ggq.chain_case(*case, pool)
    Gref = _hops_ref(c)
    ref = _tail_ref(Gref, c, pool, f32_div=True)
    G, gbuf, node, keep = _hops(L, c, keep_device=True)
    _same(_np(G), Gref, f"gin graph chain {case} {pool}: G")
    _same(_tail(L, c, pool, False, G=G), ref, f"gin graph chain {case} {pool}: logits")
