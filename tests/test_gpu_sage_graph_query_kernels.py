"""GPU tier: the SAGE graph-query kernel of csrc/query.hip (fitgnn_sage_graph_query_hops_f32) through the C ABI against the float64
reference of tests/sage_graph_query_reference.py (the convention and helpers of tests/test_gpu_gat_graph_query_kernels.py).

EXACT inputs (sage_graph_query_reference.exact_case: every fp32 intermediate exact in any order; proven on the CPU by
tests/test_sage_graph_query_reference_cpu.py) must come back bit for bit -- and bit for bit equal to fitgnn_sage_query_gather_f32 on the
same pooled rows, whose four partials differ from the window's one chain only in their order.  RANDOM inputs (val = 1 / deg) are held
per entry, none left out, to 2^-24 times the first-order bound the reference accumulates along the kernel's own operation order (derived
in the reference's docstring); nothing is added on top.  On random inputs too G[:, H:2H] is bit-identical to the node kernel's: it is
the same sage_row.  Every launch is made twice and must give the same bits; G is NaN-guarded behind and beside its rows, with
ldt = 2H + 4 and ldg = 2H + 8.

| branch (from the launch and kernel code) | tests |
|---|---|
| column slabs: H = 4 (one live lane), 64, 256 (one full slab), 260 (second slab, one live lane), 512 (two full slabs) | test_exact[*], test_random[*] |
| graphs of 1 row, 2, 3 (waves without a row), 4, 5, 17 (more than one round of the waves); unsorted, one twice | test_exact[*], test_random[*] |
| rows with 0 (h = ELU(root + b0); a pooled row: g = 0 and still h_r), 1, 63, 64 (one full batch of entries) and 65 (a second batch) entries, as a layer-0 row and as a pooled row | test_exact[*], test_random[*] |
| pooled rows: all of a graph, the first half, a non-contiguous descending subset, none (nothing written) | test_exact[*], test_one_row_graph_and_a_graph_without_pooled_rows |
| xrow, b0 NULL / given (b0 NULL: no second add); ldt > 2H, ldg > 2H | test_exact[*], test_random[*] |
| the root half-row T[t(r)][H:2H]: read at + H, through xrow; the copy of h_r from the window to G[j][H:2H] | test_exact[*], test_random[*] (the h half equals the node kernel's bits) |
| 160 rows at H = 512 and 640 at H = 64: exactly the window; one more in max_rows -> FITGNN_E_BADARG, G untouched | test_largest_window[*] |
| a graph of more rows than max_rows: its rows of a sentinel-filled G stay, its neighbours in the launch are written | test_largest_window[*], test_skips_a_graph_beyond_max_rows |
| misaligned T, G; strides below 2H or not multiples of 4; H = 0, 14, 6; Q = -1; max_rows = -1; NULL pointers; Q = 0: the documented codes, nothing launched | test_refusals |
"""
import numpy as np
import pytest
import torch

import sage_graph_query_reference as sgq
from test_gpu_gat_graph_query_kernels import _opt
from test_gpu_query_kernels import _guarded, _ratio, _untouched
from test_gpu_step_kernels import E_ALIGN, E_BADARG, L, _call, _dev, _np, _p, _run, _same, _strided  # noqa: F401

pytestmark = pytest.mark.gpu

HOPS, NODE = "fitgnn_sage_graph_query_hops_f32", "fitgnn_sage_query_gather_f32"


def _hops_args(L, c, ldt_pad=4, ldg_pad=8, max_rows=None):
    H, P = c["T"].shape[1] // 2, len(c["prow"])
    Td = _strided(c["T"], 2 * H + ldt_pad)
    buf, G = _guarded(P, 2 * H, 2 * H + ldg_pad)
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["val"]), _opt(c["xrow"], torch.int32), _opt(c["b0"]),
            _dev(c["seg"], torch.int64), _dev(c["prow"], torch.int64), _dev(c["pptr"], torch.int64), Td]
    rp, cl, vl, xr, b0, sg, pr, pp, _ = keep
    front = (_p(L, rp), _p(L, cl), _p(L, vl), _p(L, Td), 2 * H + ldt_pad, _p(L, xr), _p(L, b0))
    args = front + (_p(L, sg), _p(L, pr), _p(L, pp), len(c["seg"]), H, c["max_rows"] if max_rows is None else max_rows, _p(L, G),
                    2 * H + ldg_pad)
    node = front + (_p(L, pr), P, H)      # fitgnn_sage_query_gather_f32 on the same pooled rows: + (G, ldg)
    return args, node, buf, G, keep


def _hops(L, c, keep_device=False):
    args, node, buf, G, keep = _hops_args(L, c)
    H, P = c["T"].shape[1] // 2, len(c["prow"])
    _run(L, HOPS, *args)
    first = G.clone()
    _untouched(buf, P, 2 * H, G.stride(0), "sage graph hops")
    _run(L, HOPS, *args)
    assert torch.equal(first, G), "two launches differ"
    return (G, node, keep) if keep_device else _np(first)


def _per_row_kernel(L, G, node):
    P, H2 = G.shape
    nbuf, Gn = _guarded(P, H2, H2 + 8)
    _run(L, NODE, *node, _p(L, Gn), H2 + 8)
    _untouched(nbuf, P, H2, H2 + 8, "sage per-row gather")
    return Gn


@pytest.mark.parametrize("case", sgq.EXACT_HOPS_CASES, ids=str)
def test_exact(L, case):
    H = case[0]
    c = sgq.exact_case(*case)       # ldt = 2H + 4, ldg = 2H + 8, NaN in the padding
    G, node, keep = _hops(L, c, keep_device=True)
    got = _np(G)
    ref = sgq.run(c, f32_elu=True)
    _same(got, ref, f"sage graph hops exact {case}")
    assert torch.equal(_per_row_kernel(L, G, node), G), f"sage graph hops exact {case}: differs from {NODE} on the same rows"
    deg = np.diff(c["rowptr"])[c["prow"]]
    lone = deg == 0
    assert lone.any() and np.all(got[lone, :H] == 0), "a pooled row without entries must give g = 0"
    assert np.array_equal(got[lone, H:], ref[lone, H:]) and np.any(got[lone, H:] != 0), "a pooled row without entries still has its h_r"


@pytest.mark.parametrize("H,with_xrow,with_b0", [(4, True, True), (64, True, True), (256, False, True), (260, False, False), (512, True, False)],
                         ids=str)
def test_random(L, H, with_xrow, with_b0):
    c = sgq.random_case(H, with_xrow, with_b0)
    deg = np.diff(c["rowptr"])
    assert {0, 1, 63, 64, 65} <= set(deg.tolist()) and {0, 1, 63, 64, 65} <= set(deg[c["prow"]].tolist())
    assert np.array_equal(c["val"], np.repeat((1.0 / np.maximum(deg, 1)).astype(np.float32), deg))
    ref, B = sgq.run(c, sums=True)
    G, node, keep = _hops(L, c, keep_device=True)
    got = _np(G)
    assert np.isfinite(got).all(), "NaN or Inf"
    _ratio(got, ref, B, f"sage graph hops random H={H}")     # every entry of every pooled row
    Gn = _per_row_kernel(L, G, node)
    assert torch.equal(Gn[:, H:], G[:, H:]), "the h half differs from the node kernel's: it is the same sage_row"


@pytest.mark.parametrize("H", [64, 512])
def test_largest_window(L, H):
    """A graph of exactly sage_graph_query_max_rows(H) rows fills the 160 KiB; a window sized for one row more is refused; with one row
    more the graph is skipped by the launch -- its rows of a sentinel-filled G stay as they were -- while both its neighbours are written."""
    from fitgnn_amd import ops
    n = ops.sage_graph_query_max_rows(H)
    lds = L.lib().fitgnn_sage_graph_query_hops_lds_bytes
    assert n == {64: 640, 512: 160}[H] and lds(n, H) <= 160 * 1024 < lds(n + 1, H)
    c = sgq.window_case(H, n)
    G, node, keep = _hops(L, c, keep_device=True)
    _same(_np(G), sgq.run(c, f32_elu=True), f"sage graph hops window H={H} rows={n}")
    assert torch.equal(_per_row_kernel(L, G, node), G), f"sage graph hops window H={H}: differs from {NODE}"
    r = sgq.window_case(H, n, exact=False)
    ref, B = sgq.run(r, sums=True)
    _ratio(_hops(L, r), ref, B, f"sage graph hops window random H={H}")
    c = sgq.window_case(H, n + 1)
    args, node, buf, G, keep = _hops_args(L, c, max_rows=n + 1)
    assert _call(L, HOPS, *args) == E_BADARG
    assert torch.isnan(buf).all(), "a refused launch wrote G"
    args, node, buf, G, keep = _hops_args(L, c, max_rows=n)
    G.fill_(-7.0)
    _run(L, HOPS, *args)
    got, ref = _np(G), sgq.run(c, f32_elu=True)
    skipped = np.repeat(c["seg"][:, 1] - c["seg"][:, 0] > n, np.diff(c["pptr"]))
    assert skipped.sum() == n + 1 and (~skipped).sum() == 5 and skipped[0] and not skipped[-5:].any()
    assert (got[skipped] == -7.0).all(), "a graph beyond max_rows was written"
    _same(got[~skipped], ref[~skipped], "sage graph hops beside a skipped graph")


def test_skips_a_graph_beyond_max_rows(L):
    """max_rows = 5 sizes the window for the graphs of up to 5 rows: the larger one, queried twice in the same launch, is left out -- its
    rows of G stay NaN -- and every other graph is answered as before (GraphQueryEngine sends such a graph's rows through
    fitgnn_sage_query_gather_f32)."""
    c = sgq.exact_case(64, True, True)
    args, node, buf, G, keep = _hops_args(L, c, max_rows=5)
    _run(L, HOPS, *args)
    got, ref = _np(G), sgq.run(c, f32_elu=True)
    skipped = np.repeat(c["seg"][:, 1] - c["seg"][:, 0] > 5, np.diff(c["pptr"]))
    assert skipped.any() and not skipped.all() and np.isnan(got[skipped]).all()
    _same(got[~skipped], ref[~skipped], "sage graph hops beside skipped graphs")


def test_one_row_graph_and_a_graph_without_pooled_rows(L):
    """A graph of one row whose only entry is itself (val = 1): g = h, both halves of its row of G hold the same bits.  A graph without
    pooled rows writes nothing; the launch of nothing but such graphs leaves G as it was."""
    H = 16
    c = sgq.random_case(H, False, True, sizes=[1, 3], degs=[[1], [2, 0, 1]], graphs=[0, 1, 0], kinds=["all", "none", "all"])
    assert np.diff(c["pptr"]).tolist() == [1, 0, 1] and c["col"][0] == 0 and c["val"][0] == 1.0
    ref, B = sgq.run(c, sums=True)
    got = _hops(L, c)
    _ratio(got, ref, B, "sage graph hops one-row graph")
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(got[0, :H], got[0, H:])             # fmaf(1, h, 0) = h
    none = dict(c)
    none["seg"], none["pptr"] = c["seg"][1:2], np.array([0, 0], dtype=np.int64)
    none["prow"] = np.array([1], dtype=np.int64)           # a buffer of one row that no graph claims
    args, node, buf, G, keep = _hops_args(L, none)
    _run(L, HOPS, *args)
    assert torch.isnan(buf).all(), "a graph without pooled rows wrote G"


def test_refusals(L):
    """Argument errors only: no launch here hands the kernel rows or columns outside their ranges."""
    c = sgq.random_case(16, False, False, sizes=[2, 3], degs=[1, 2], graphs=[0, 1], kinds=["all"])
    H, n = 16, int(c["gptr"][-1])
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["val"]), _dev(c["seg"], torch.int64), _dev(c["prow"], torch.int64),
            _dev(c["pptr"], torch.int64)]
    rp, cl, vl, sg, pr, pp = keep
    buf = torch.zeros(n * (2 * H + 4) + 8, dtype=torch.float32, device="cuda")
    out = torch.full((len(c["prow"]) * (2 * H + 4) + 8,), 3.0, dtype=torch.float32, device="cuda")
    d = dict(rp=rp, cl=cl, vl=vl, T=buf, ldt=2 * H, sg=sg, pr=pr, pp=pp, Q=2, H=H, mr=3, G=out, ldg=2 * H)

    def call(**kw):
        a = dict(d, **kw)
        return _call(L, HOPS, _p(L, a["rp"]), _p(L, a["cl"]), _p(L, a["vl"]), _p(L, a["T"]), a["ldt"], None, None, _p(L, a["sg"]), _p(L, a["pr"]),
                     _p(L, a["pp"]), a["Q"], a["H"], a["mr"], _p(L, a["G"]), a["ldg"])
    for k in ("T", "G"):
        assert call(**{k: d[k][1:]}) == E_ALIGN, k
    assert call(ldt=2 * H + 2) == E_ALIGN and call(ldg=2 * H + 6) == E_ALIGN
    assert call(ldt=2 * H - 4) == E_BADARG and call(ldg=2 * H - 4) == E_BADARG and call(ldt=H) == E_BADARG and call(ldg=H) == E_BADARG
    assert call(H=0) == E_BADARG and call(H=14) == E_BADARG and call(H=6) == E_BADARG
    assert call(Q=-1) == E_BADARG and call(mr=-1) == E_BADARG and call(mr=sgq.max_rows(H) + 1) == E_BADARG
    for k in ("rp", "cl", "vl", "T", "sg", "pr", "pp", "G"):
        assert call(**{k: None}) == E_BADARG, k
    assert (out == 3.0).all(), "a refused launch wrote G"
    assert call(Q=0) == 0 and call(Q=0, G=None) == 0 and (out == 3.0).all()
    assert call(ldt=2 * H + 4, ldg=2 * H + 4) == 0 and not (out == 3.0).all()
