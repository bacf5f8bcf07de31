"""GPU tier: the GAT graph-query kernel of csrc/query.hip (fitgnn_gat_graph_query_hops_f32) through the C ABI against the float64
reference of tests/gat_graph_query_reference.py (the convention and helpers of tests/test_gpu_graph_query_kernels.py and
tests/test_gpu_gat_query_kernels.py).

EXACT inputs (gat_graph_query_reference.exact_uniform_case / exact_selector_case: every fp32 intermediate exact, every softmax weight
exactly 0 or 1; proven on the CPU by tests/test_gat_graph_query_reference_cpu.py) must come back bit for bit -- and bit for bit equal to
fitgnn_gat_query_gather_f32 on the same pooled rows, whose four online-softmax partials differ from the window's one chain only in
their order.  RANDOM inputs are held per entry, none left out, to 2^-24 times the first-order bound the reference accumulates along the
kernel's own operation order (derived in the reference's docstring); nothing is added on top.  Every launch is made twice and must give
the same bits; G is NaN-guarded behind and beside its rows.

| branch (from the launch and kernel code) | tests |
|---|---|
| column slots: H = 16 (four live lanes), 64, 256 (one full slot, <1>), 260 (second slot, one live lane, <2>), 512 (both full) | test_exact[*], test_random[*] |
| graphs of 1 row, 2, 3 (waves without a row), 4, 5, 9, 18 (more than one round of the waves); unsorted, one twice | test_exact[*] |
| rows with 0 (h = ELU(b0); a pooled row: zeros), 1, 64, 65 (a second 64-entry batch) and 130 (a third) entries, as a layer-0 row and as a pooled row | test_exact[selector-*], test_random[*] |
| pooled rows: all of a graph, the first half, a non-contiguous descending subset, none (nothing written) | test_exact[*] |
| xrow, b0 NULL / given; ldt > H, ldg > H | test_exact[*], test_random[*] |
| a softmax whose losers underflow to 0 at both layers; ties; scores on both sides of both LeakyReLUs | test_exact[selector-*] |
| score spreads: ordinary, some tens, > 200 at both layers (weights that come back as 0; no NaN / Inf) | test_random[*] |
| 79 rows at H = 512 and 620 at H = 64: exactly the window; one more in max_rows -> FITGNN_E_BADARG, G untouched | test_largest_window[*] |
| a graph of more rows than max_rows: its rows of a sentinel-filled G stay, its neighbours in the launch are written | test_largest_window[*], test_skips_a_graph_beyond_max_rows |
| misaligned T, G, u_src, u_dst; strides too small or not multiples of 4; H = 516; NULL pointers; Q = 0: the documented codes, nothing launched | test_refusals |
"""
import numpy as np
import pytest
import torch

import gat_graph_query_reference as ggq
from test_gpu_query_kernels import _guarded, _ratio, _untouched
from test_gpu_step_kernels import E_ALIGN, E_BADARG, L, _call, _dev, _np, _p, _run, _same, _strided  # noqa: F401

pytestmark = pytest.mark.gpu

HOPS, NODE = "fitgnn_gat_graph_query_hops_f32", "fitgnn_gat_query_gather_f32"


def _opt(a, dtype=torch.float32):
    return None if a is None else _dev(a, dtype)


def _hops_args(L, c, ldt_pad=4, ldg_pad=8, max_rows=None):
    H, P = c["T"].shape[1], len(c["prow"])
    Td = _strided(c["T"], H + ldt_pad)
    buf, G = _guarded(P, H, H + ldg_pad)
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _opt(c["xrow"], torch.int32), _dev(c["a_src0"]), _dev(c["a_dst0"]),
            _opt(c["b0"]), _dev(c["u_src"]), _dev(c["u_dst"]), _dev(c["seg"], torch.int64), _dev(c["prow"], torch.int64),
            _dev(c["pptr"], torch.int64), Td]
    rp, cl, xr, a_s, a_d, b0, us, ud, sg, pr, pp, _ = keep
    front = (_p(L, rp), _p(L, cl), _p(L, Td), H + ldt_pad, _p(L, xr), _p(L, a_s), _p(L, a_d), _p(L, b0), float(c["slope0"]), _p(L, us),
             _p(L, ud), float(c["slope1"]))
    args = front + (_p(L, sg), _p(L, pr), _p(L, pp), len(c["seg"]), H, c["max_rows"] if max_rows is None else max_rows, _p(L, G), H + ldg_pad)
    node = front + (_p(L, pr), P, H)      # fitgnn_gat_query_gather_f32 on the same pooled rows: + (G, ldg)
    return args, node, buf, G, keep


def _hops(L, c, keep_device=False):
    args, node, buf, G, keep = _hops_args(L, c)
    H, P = c["T"].shape[1], len(c["prow"])
    _run(L, HOPS, *args)
    first = G.clone()
    _untouched(buf, P, H, G.stride(0), "gat graph hops")
    _run(L, HOPS, *args)
    assert torch.equal(first, G), "two launches differ"
    return (G, node, keep) if keep_device else _np(first)


def _equals_the_per_row_kernel(L, G, node, what):
    P, H = G.shape
    nbuf, Gn = _guarded(P, H, H + 8)
    _run(L, NODE, *node, _p(L, Gn), H + 8)
    assert torch.equal(Gn, G), f"{what}: differs from fitgnn_gat_query_gather_f32 on the same rows"


@pytest.mark.parametrize("case", ggq.EXACT_HOPS_CASES, ids=str)
@pytest.mark.parametrize("gen", sorted(ggq.EXACT_GENERATORS))
def test_exact(L, gen, case):
    c = ggq.EXACT_GENERATORS[gen](*case)       # ldt = H + 4, ldg = H + 8, NaN in the padding
    G, node, keep = _hops(L, c, keep_device=True)
    got = _np(G)
    deg = np.diff(c["rowptr"])[c["prow"]]
    assert (deg == 0).any() and np.all(got[deg == 0] == 0), "a pooled row without entries must give zeros"
    _same(got, ggq.run(c, f32_elu=True), f"gat graph hops {gen} {case}")
    _equals_the_per_row_kernel(L, G, node, f"gat graph hops {gen} {case}")


@pytest.mark.parametrize("H,with_xrow,with_b0,spread", [(64, True, True, "unit"), (260, False, True, "wide"), (512, True, False, "underflow"),
                                                        (16, False, False, "underflow"), (512, False, True, "unit"), (256, True, True, "wide")],
                         ids=str)
def test_random(L, H, with_xrow, with_b0, spread):
    c = ggq.random_case(H, with_xrow, with_b0, spread)
    ref, B = ggq.run(c, sums=True)
    s0, s1 = ggq.score_spreads(c)
    assert (s0 >= 200 and s1 >= 200) if spread == "underflow" else (s0 < 100 and s1 < 100), (s0, s1)
    deg = np.diff(c["rowptr"])
    assert {0, 1, 64, 65, 130} <= set(deg.tolist()) and {0, 1, 64, 65, 130} <= set(deg[c["prow"]].tolist())
    got = _hops(L, c)
    assert np.isfinite(got).all(), "NaN or Inf"
    _ratio(got, ref, B, f"gat graph hops random H={H} spread={spread}")     # every entry of every pooled row


@pytest.mark.parametrize("H", [64, 512])
def test_largest_window(L, H):
    """A graph of exactly gat_graph_query_max_rows(H) rows fills the 160 KiB; a window sized for one row more is refused; with one row
    more the graph is skipped by the launch -- its rows of a sentinel-filled G stay as they were -- while both its neighbours are written."""
    from fitgnn_amd import ops
    n = ops.gat_graph_query_max_rows(H)
    lds = L.lib().fitgnn_gat_graph_query_hops_lds_bytes
    assert n == {64: 620, 512: 79}[H] and lds(n, H) <= 160 * 1024 < lds(n + 1, H)
    c = ggq.window_case(H, n)
    G, node, keep = _hops(L, c, keep_device=True)
    _same(_np(G), ggq.run(c, f32_elu=True), f"gat graph hops window H={H} rows={n}")
    _equals_the_per_row_kernel(L, G, node, f"gat graph hops window H={H}")
    r = ggq.window_case(H, n, exact=False)
    ref, B = ggq.run(r, sums=True)
    _ratio(_hops(L, r), ref, B, f"gat graph hops window random H={H}")
    c = ggq.window_case(H, n + 1)
    args, node, buf, G, keep = _hops_args(L, c, max_rows=n + 1)
    assert _call(L, HOPS, *args) == E_BADARG
    assert torch.isnan(buf).all(), "a refused launch wrote G"
    args, node, buf, G, keep = _hops_args(L, c, max_rows=n)
    G.fill_(-7.0)
    _run(L, HOPS, *args)
    got, ref = _np(G), ggq.run(c, f32_elu=True)
    skipped = np.repeat(c["seg"][:, 1] - c["seg"][:, 0] > n, np.diff(c["pptr"]))
    assert skipped.sum() == n + 1 and (~skipped).sum() == 5 and skipped[0] and not skipped[-5:].any()
    assert (got[skipped] == -7.0).all(), "a graph beyond max_rows was written"
    _same(got[~skipped], ref[~skipped], "gat graph hops beside a skipped graph")


def test_skips_a_graph_beyond_max_rows(L):
    """max_rows = 5 sizes the window for the graphs of up to 5 rows: the larger one, queried twice in the same launch, is left out -- its
    rows of G stay NaN -- and every other graph is answered as before (GraphQueryEngine sends such a graph's rows through
    fitgnn_gat_query_gather_f32)."""
    c = ggq.exact_selector_case(64, True)
    args, node, buf, G, keep = _hops_args(L, c, max_rows=5)
    _run(L, HOPS, *args)
    got, ref = _np(G), ggq.run(c, f32_elu=True)
    skipped = np.repeat(c["seg"][:, 1] - c["seg"][:, 0] > 5, np.diff(c["pptr"]))
    assert skipped.any() and not skipped.all() and np.isnan(got[skipped]).all()
    _same(got[~skipped], ref[~skipped], "gat graph hops beside skipped graphs")


def test_one_row_graph_and_a_graph_without_pooled_rows(L):
    """A graph of one row whose only entry is itself: beta = 1, g = h.  A graph without pooled rows writes nothing; the launch of
    nothing but such graphs leaves G as it was."""
    H = 16
    c = ggq.random_case(H, False, True, "unit", sizes=[1, 3], degs=[[1], [2, 0, 1]], graphs=[0, 1, 0], kinds=["all", "none", "all"])
    assert np.diff(c["pptr"]).tolist() == [1, 0, 1] and c["col"][0] == 0
    ref, B = ggq.run(c, sums=True)
    got = _hops(L, c)
    _ratio(got, ref, B, "gat graph hops one-row graph")
    assert np.array_equal(got[0], got[1])
    h = ggq.layer0(c["rowptr"].astype(np.int64), c["col"].astype(np.int64), c["T"].astype(np.float64), c["a_src0"].astype(np.float64),
                   c["a_dst0"].astype(np.float64), [0], None, c["b0"], c["slope0"])[0][0]
    assert np.abs(got[0] - h).max() <= 2.0 ** -20 * np.abs(h).max()       # l = 1: g = h (1 / 1); h itself within a few roundings
    none = dict(c)
    none["seg"], none["pptr"] = c["seg"][1:2], np.array([0, 0], dtype=np.int64)
    none["prow"] = np.array([1], dtype=np.int64)           # a buffer of one row that no graph claims
    args, node, buf, G, keep = _hops_args(L, none)
    _run(L, HOPS, *args)
    assert torch.isnan(buf).all(), "a graph without pooled rows wrote G"


def test_refusals(L):
    c = ggq.random_case(16, False, False, "unit", sizes=[2, 3], degs=[1, 2], graphs=[0, 1], kinds=["all"])
    H, n = 16, int(c["gptr"][-1])
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["a_src0"]), _dev(c["a_dst0"]), _dev(c["seg"], torch.int64),
            _dev(c["prow"], torch.int64), _dev(c["pptr"], torch.int64)]
    rp, cl, a_s, a_d, sg, pr, pp = keep
    buf = torch.zeros(n * (H + 4) + 8, dtype=torch.float32, device="cuda")
    out = torch.full((len(c["prow"]) * (H + 4) + 8,), 3.0, dtype=torch.float32, device="cuda")
    u = torch.zeros(2 * H + 8, dtype=torch.float32, device="cuda")
    d = dict(rp=rp, cl=cl, T=buf, ldt=H, a_s=a_s, a_d=a_d, us=u, ud=u[H:], sg=sg, pr=pr, pp=pp, Q=2, H=H, mr=3, G=out, ldg=H)

    def call(**kw):
        a = dict(d, **kw)
        return _call(L, HOPS, _p(L, a["rp"]), _p(L, a["cl"]), _p(L, a["T"]), a["ldt"], None, _p(L, a["a_s"]), _p(L, a["a_d"]), None, 0.2,
                     _p(L, a["us"]), _p(L, a["ud"]), 0.2, _p(L, a["sg"]), _p(L, a["pr"]), _p(L, a["pp"]), a["Q"], a["H"], a["mr"], _p(L, a["G"]),
                     a["ldg"])
    for k in ("T", "G", "us", "ud"):
        assert call(**{k: d[k][1:]}) == E_ALIGN, k
    assert call(ldt=H + 2) == E_ALIGN and call(ldg=H + 6) == E_ALIGN
    assert call(ldt=H - 4) == E_BADARG and call(ldg=H - 4) == E_BADARG
    assert call(H=516, ldt=516, ldg=516) == E_BADARG and call(H=14) == E_BADARG and call(H=0) == E_BADARG
    assert call(Q=-1) == E_BADARG and call(mr=-1) == E_BADARG and call(mr=ggq.max_rows(H) + 1) == E_BADARG
    for k in ("rp", "cl", "T", "a_s", "a_d", "us", "ud", "sg", "pr", "pp", "G"):
        assert call(**{k: None}) == E_BADARG, k
    assert (out == 3.0).all(), "a refused launch wrote G"
    assert call(Q=0) == 0 and call(Q=0, G=None) == 0 and (out == 3.0).all()
    assert call(ldt=H + 4, ldg=H + 4) == 0 and not (out == 3.0).all()
