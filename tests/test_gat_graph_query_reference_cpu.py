"""CPU tier of the GAT graph-query path (fitgnn_amd/serve.py GraphQueryEngine gat_kernels, csrc/query.hip gat_graph_query_hops_kernel):
the float64 reference of tests/gat_graph_query_reference.py against a model forward composed from the oracle's GAT stack and against a
dense two-layer GAT per graph, the exactness of the EXACT inputs the GPU test sends through the kernel, the bound against float32
replays in three summation orders, the window arithmetic and the launcher's argument refusals -- all before any launch."""
import argparse

import numpy as np
import pytest
import torch

import gat_graph_query_reference as ggq
import gat_query_reference as gq
import graph_query_reference as gr
import query_reference as qr
from oracle import gnn_oracle as gorc
from test_gat_query_reference_cpu import _exactness_watch

f32, f64 = np.float32, np.float64
U = 2.0 ** -24


def _dense_gat(x, cnt, W, a_s, a_d, b, slope):
    """One GATConv layer on a graph given as a dense matrix of entry multiplicities cnt[target, source]."""
    z = x @ W.T
    e = (z @ a_s)[None, :] + (z @ a_d)[:, None]
    e = np.where(e > 0, e, slope * e)
    w = cnt * np.exp(e - np.where(cnt > 0, e, -np.inf).max(1, keepdims=True, initial=-1e300))
    den = w.sum(1, keepdims=True)
    return (w / np.where(den > 0, den, 1.0)) @ z + b


def _dense_graph_forward(X, rowptr, col, seg, prow, pptr, m, slopes, pool, softmax):
    out = []
    for i, (r0, r1) in enumerate(seg):
        n = r1 - r0
        cnt = np.zeros((n, n))
        for r in range(r0, r1):
            for e in range(rowptr[r], rowptr[r + 1]):
                cnt[r - r0, col[e] - r0] += 1
        x = X[r0:r1]
        for k in range(2):
            p = f"conv.{k}."
            x = qr.elu(_dense_gat(x, cnt, m[p + "lin.weight"], m[p + "att_src"].reshape(-1), m[p + "att_dst"].reshape(-1), m[p + "bias"],
                                  slopes[k]))
        rows = prow[pptr[i]:pptr[i + 1]] - r0
        pl = x[rows].max(0) if pool == "max" else x[rows].mean(0)
        y = pl @ m["lt1.weight"].T + m["lt1.bias"]
        if softmax:
            y = np.exp(y - y.max())
            y = y / y.sum()
        out.append(y)
    return np.stack(out)


@pytest.mark.parametrize("pool,softmax", [("max", True), ("mean", False)])
def test_reference_equals_the_oracle_forward_and_a_dense_gat_per_graph(pool, softmax):
    """hops + graph_query_reference.pooled_tail on small graphs == the whole-view float64 forward (ELU(gat_conv) twice), the per-graph
    pool, the head and the softmax, and == a dense GAT on each graph's own rows, to 1e-12: the identities att . (W1 h) = (W1^T att) . h
    and sum beta = 1, and that both layers read the one CSR row.  Distinct slopes; pooled rows: all of a graph, a subset, one."""
    rng = np.random.default_rng(79 + softmax)
    F, H, H2, C = 6, 16, 32, 5
    sizes = [1, 4, 7, 17, 2]
    gptr = np.concatenate([[0], np.cumsum(sizes)])
    n = int(gptr[-1])
    src, dst = [], []
    for g, k in enumerate(sizes):          # repeated edges and self loops inside each graph (replaced by exactly one per row)
        src += rng.integers(gptr[g], gptr[g + 1], size=3 * k).tolist()
        dst += rng.integers(gptr[g], gptr[g + 1], size=3 * k).tolist()
    ei = np.stack([src, dst]).astype(np.int64)
    g_ = lambda *s: rng.normal(0, 0.6, size=s)   # noqa: E731
    m = {"conv.0.lin.weight": g_(H, F), "conv.0.att_src": g_(1, 1, H), "conv.0.att_dst": g_(1, 1, H), "conv.0.bias": g_(H),
         "conv.1.lin.weight": g_(H2, H), "conv.1.att_src": g_(1, 1, H2), "conv.1.att_dst": g_(1, 1, H2), "conv.1.bias": g_(H2),
         "lt1.weight": g_(C, H2), "lt1.bias": g_(C)}
    X = rng.normal(size=(n, F))
    slopes = (0.2, 0.35)
    rowptr, col, _ = qr.gcn_csr(ei, n)
    seg, prow, pptr = gr.pooled_rows(rng, gptr, [3, 0, 2, 1, 3, 4], ["all", "all", "subset", "first", "subset", "first"])
    assert 1 in np.diff(pptr).tolist()
    T, W1 = X @ m["conv.0.lin.weight"].T, m["conv.1.lin.weight"]
    args = (rowptr, col, T, T @ m["conv.0.att_src"].reshape(-1), T @ m["conv.0.att_dst"].reshape(-1), W1.T @ m["conv.1.att_src"].reshape(-1),
            W1.T @ m["conv.1.att_dst"].reshape(-1))
    G = ggq.hops(*args, seg, prow, pptr, b0=m["conv.0.bias"], slope0=slopes[0], slope1=slopes[1])
    out = gr.pooled_tail(G, pptr, W1, m["conv.1.bias"], m["lt1.weight"], m["lt1.bias"], pool=pool, softmax=softmax)
    sd = {k: torch.from_numpy(v) for k, v in m.items()}
    ref = ggq.model_forward(gorc, sd, torch.from_numpy(X), torch.from_numpy(ei), seg, prow, pptr, pool, softmax, slopes)
    assert out.shape == ref.shape == (6, C) and np.abs(out - ref).max() <= 1e-12
    dense = _dense_graph_forward(X, rowptr, col, seg, prow, pptr, m, slopes, pool, softmax)
    assert np.abs(out - dense).max() <= 1e-12
    # the per-row reference forms the same g_r up to the order of its fold: the two agree to rounding
    Gn = gq.gather(*args, prow, b0=m["conv.0.bias"], slope0=slopes[0], slope1=slopes[1])
    assert np.abs(G - Gn).max() <= 1e-12 * np.abs(G).max()


def test_phase_1_is_the_per_row_references_row_routine():
    """layer0 is gat_query_reference.gather's row routine: the first "h" that gather shows for a query q is h_q, bit for bit, on
    random inputs with and without xrow and b0."""
    for with_xrow, with_b0 in ((True, True), (False, False)):
        c = ggq.random_case(16, with_xrow, with_b0, "unit")
        need = [r for r in range(len(c["rowptr"]) - 1) if c["rowptr"][r + 1] > c["rowptr"][r]]
        T, a_s, a_d = (np.asarray(c[k], dtype=f64) for k in ("T", "a_src0", "a_dst0"))
        mine = ggq.layer0(c["rowptr"].astype(np.int64), c["col"].astype(np.int64), T, a_s, a_d, need, c["xrow"], c["b0"], c["slope0"])
        for r in need[::3]:
            seen = []
            gq.gather(c["rowptr"], c["col"], c["T"], c["a_src0"], c["a_dst0"], c["u_src"], c["u_dst"], [r], xrow=c["xrow"], b0=c["b0"],
                      slope0=c["slope0"], slope1=c["slope1"], watch=lambda name, a: seen.append(np.array(a)) if name == "h" else None)
            assert np.array_equal(seen[0], mine[r][0])


def _graph_exactness_watch():
    inner, seen = _exactness_watch()

    def watch(name, a):
        if name in ("arg1",):
            a64 = np.asarray(a, dtype=f64)
            assert np.all((a64 == 0) | (a64 <= -104)), "a layer-1 exp argument inside (-104, 0): expf would round"
        inner(name, a)
    return watch, seen


@pytest.mark.parametrize("case", ggq.EXACT_HOPS_CASES, ids=str)
@pytest.mark.parametrize("gen", sorted(ggq.EXACT_GENERATORS))
def test_exact_inputs_are_exact(gen, case):
    """Rounding every watched intermediate to float32 changes nothing: what makes the bit-for-bit GPU tests meaningful.  Every weight is
    exactly 0 or 1, so the per-row kernel's order (four online-softmax partials) gives the same values as the window's one chain."""
    c = ggq.EXACT_GENERATORS[gen](*case)
    watch, seen = _graph_exactness_watch()
    G = ggq.run(c, watch=watch, f32_elu=True)
    assert seen["n"] > 1000 and np.isfinite(G).all() and G.shape == (len(c["prow"]), case[0])
    assert {"s", "e", "arg", "p", "l", "a", "inv", "pre", "h", "dot", "ds", "dd", "s1", "f", "arg1", "p1", "l1", "g", "inv1", "G"} <= seen["names"]
    assert np.abs(ggq.run(c) - G).max() <= 1e-12       # exp's underflow (< 1e-200) is all that float64 adds
    assert np.array_equal(ggq.run_rows(c, watch=watch, f32_elu=True), G)
    deg = np.diff(c["rowptr"])
    size = (c["seg"][:, 1] - c["seg"][:, 0]).tolist()
    assert len(size) > len(set(size)) and 1 in size and c["max_rows"] == 18
    want = set(ggq.UNIFORM_ROW_DEGS) if gen == "uniform" else {0, 1, 64, 65, 130}
    assert want <= set(deg.tolist()) and want <= set(deg[c["prow"]].tolist())     # as a layer-0 row and as a pooled row
    assert np.all(G[deg[c["prow"]] == 0] == 0)
    cnt = np.diff(c["pptr"])
    assert (cnt == 0).any() and (cnt == np.array(size)).any() and ((cnt > 0) & (cnt < np.array(size))).any()
    if c["xrow"] is not None:
        assert len(set(c["xrow"].tolist())) < len(c["xrow"])
    if c["b0"] is not None:
        assert (G < 0).any() and (G > 0).any()    # both ELU branches reach the output
    if gen == "selector":
        f, p = [], []
        ggq.run(c, watch=lambda name, a: (f if name == "f" else p).extend(np.ravel(a).tolist()) if name in ("f", "p", "p1") else None,
                f32_elu=True)
        assert min(f) < 0 and max(f) >= 0 and len(set(f)) > 8      # layer-1 scores on both sides of the LeakyReLU
        assert set(p) == {0.0, 1.0} and p.count(0.0) > 100         # losers at both layers, every weight exactly 0 or 1
        d = dict(c)                                                # a dropped, doubled or misplaced entry shows
        d["a_src0"] = c["a_src0"][::-1].copy()
        assert np.abs(ggq.run(d, f32_elu=True) - G).max() > 0


@pytest.mark.parametrize("H", [64, 512])
def test_exact_window_inputs_are_exact(H):
    from fitgnn_amd import ops
    n = ops.gat_graph_query_max_rows(H)
    assert n == ggq.max_rows(H) == {64: 620, 512: 79}[H]
    c = ggq.window_case(H, n + 1)
    assert (c["seg"][:, 1] - c["seg"][:, 0]).tolist() == [n + 1, 3, 2]
    c = ggq.window_case(H, n)
    watch, seen = _graph_exactness_watch()
    G = ggq.run(c, watch=watch, f32_elu=True)
    assert seen["n"] > 100 and np.isfinite(G).all() and np.array_equal(ggq.run_rows(c, f32_elu=True), G)


# ---- the stated order once more, in float32, and two other summation orders ----
def _fma(a, b, c):
    """fmaf: the product is exact in float64 (24 + 24 bits); the sum rounds to float64 and then to float32 (the double rounding moves a
    result by at most 2^-29 of a float32 rounding: far inside the bound's first-order slack)."""
    return (np.asarray(a, dtype=f64) * np.asarray(b, dtype=f64) + np.asarray(c, dtype=f64)).astype(f32)


def _exp32(x):
    with np.errstate(under="ignore"):
        return np.exp(np.asarray(x, dtype=f64)).astype(f32)    # correctly rounded: inside the 1 ulp the bound grants expf


def _elu32(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0).astype(f64)).astype(f32)).astype(f32)


def _lrelu32(s, slope):
    return np.where(s > 0, s, f32(slope) * s).astype(f32)


def _dot32(u, h):
    H = len(u)
    d = np.zeros(64, dtype=f32)
    for s in range(ggq.slots(H)):
        for i in range(4):
            c = s * 256 + 4 * np.arange(64) + i
            cc = np.minimum(c, H - 1)
            d = _fma(np.where(c < H, u[cc], f32(0)), h[cc], d)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        d = (d + d[idx ^ o]).astype(f32)
    return d[0]


def _softmax_sum32(p, rows, order):
    """(l, a) = (sum_k p_k, sum_k p_k rows_k) in float32: "csr" the kernel's chain, "reversed" the same chain from the last entry,
    "pairwise" NumPy's blocked pairwise sum of separately rounded products (one rounding for the product and at most D - 1 on a path)."""
    if order == "pairwise":
        return p.sum(dtype=f32), (p[:, None] * rows).astype(f32).sum(0, dtype=f32)
    l, a = f32(0), np.zeros(rows.shape[1], dtype=f32)
    for k in (range(len(p)) if order == "csr" else range(len(p) - 1, -1, -1)):
        l = f32(l + p[k])
        a = _fma(p[k], rows[k], a)
    return l, a


def _hops32(c, order):
    rowptr, col, xrow = c["rowptr"], c["col"], c["xrow"]
    T, a_s, a_d, u_s, u_d = (np.asarray(c[k], dtype=f32) for k in ("T", "a_src0", "a_dst0", "u_src", "u_dst"))
    H = T.shape[1]
    bias = np.zeros(H, dtype=f32) if c["b0"] is None else c["b0"].astype(f32)
    t = (lambda r: r) if xrow is None else (lambda r: xrow[r])
    G = np.zeros((len(c["prow"]), H), dtype=f32)
    for i, (r0, r1) in enumerate(c["seg"]):
        h = np.zeros((r1 - r0, H), dtype=f32)
        ds, dd = np.zeros(r1 - r0, dtype=f32), np.zeros(r1 - r0, dtype=f32)
        for r in range(r0, r1):
            nodes = [t(k) for k in col[rowptr[r]:rowptr[r + 1]]]
            a, inv = np.zeros(H, dtype=f32), f32(0)
            if nodes:
                e = _lrelu32((a_s[nodes] + a_d[t(r)]).astype(f32), c["slope0"])
                l, a = _softmax_sum32(_exp32((e - e.max()).astype(f32)), T[nodes], order)
                inv = f32(1) / l
            h[r - r0] = _elu32(_fma(a, inv, bias))
            ds[r - r0], dd[r - r0] = _dot32(u_s, h[r - r0]), _dot32(u_d, h[r - r0])
        for j in range(c["pptr"][i], c["pptr"][i + 1]):
            r = c["prow"][j]
            ents = col[rowptr[r]:rowptr[r + 1]] - r0
            if len(ents):
                f = _lrelu32((ds[ents] + dd[r - r0]).astype(f32), c["slope1"])
                l, g = _softmax_sum32(_exp32((f - f.max()).astype(f32)), h[ents], order)
                G[j] = (g * (f32(1) / l)).astype(f32)
    assert G.dtype == f32
    return G


@pytest.mark.parametrize("spread", ggq.SPREADS)
def test_the_bound_covers_float32_runs_in_three_summation_orders(spread):
    """sums=True: the reference's bound holds for the stated order carried out in float32, for the same chain run backwards and for a
    pairwise sum -- it counts roundings per path, which no order of D additions exceeds -- at every entry and at all three spreads."""
    c = ggq.random_case(16, True, True, spread, sizes=[1, 2, 5, 18], degs=[0, 1, 2, 7, 65, 30], graphs=[3, 0, 2, 1],
                        kinds=["all", "all", "subset", "first"])
    ref, B = ggq.run(c, sums=True)
    s0, s1 = ggq.score_spreads(c)
    assert (s0 >= 200 and s1 >= 200) if spread == "underflow" else (s0 < 100 and s1 < 100), (s0, s1)
    live = np.diff(c["rowptr"])[c["prow"]] > 0
    assert live.any() and (B[live] > 0).all() and (ref[~live] == 0).all()
    runs = []
    for order in ("csr", "reversed", "pairwise"):
        got = _hops32(c, order)
        err = np.abs(got.astype(f64) - ref)
        assert np.isfinite(got).all() and (err <= U * B).all() and err.max() > 0, (order, float((err / np.maximum(U * B, 1e-300)).max()))
        print(f"{spread} {order}: worst error / bound = {float((err[live] / (U * B[live])).max()):.3f}")
        runs.append(got)
    assert not any(np.array_equal(runs[a], runs[b]) for a, b in ((0, 1), (0, 2), (1, 2))), "the three orders gave the same bits"
    # the exact inputs come back bit for bit in every order
    e = ggq.exact_selector_case(16, True)
    for order in ("csr", "reversed", "pairwise"):
        assert np.array_equal(_hops32(e, order).astype(f64), ggq.run(e, f32_elu=True))


def test_window_arithmetic_and_launcher_refusals_without_touching_the_gpu():
    from fitgnn_amd import _lib, ops
    L = _lib.lib()
    lds = L.fitgnn_gat_graph_query_hops_lds_bytes
    assert lds(79, 512) == 79 * 514 * 4 <= 160 * 1024 < lds(80, 512) and lds(620, 64) == 620 * 66 * 4 <= 160 * 1024 < lds(621, 64)
    assert lds(7, 260) == 7 * 262 * 4 and lds(0, 64) == 0 and lds(-1, 64) == 0 and lds(4, 0) == 0
    assert ops.gat_graph_query_max_rows(512) == 79 and ops.gat_graph_query_max_rows(64) == 620 and ops.gat_graph_query_max_rows(0) == 0
    assert ops.gat_graph_query_max_rows(16) == ggq.max_rows(16) == 2275

    h = L.fitgnn_gat_graph_query_hops_f32
    N = None

    def hops(Q=4, H=512, max_rows=16, ldt=512, ldg=512):
        #        rowptr col T  ldt xrow a_s a_d b0 sl0  u_s u_d sl1  seg prow pptr Q  H  max_rows G  ldg stream
        return h(N, N, N, ldt, N, N, N, N, 0.2, N, N, 0.2, N, N, N, Q, H, max_rows, N, ldg, N)

    assert hops(Q=-1) == -1 and hops(max_rows=-1) == -1
    assert hops(H=0) == -1 and hops(H=510) == -1 and hops(H=516, ldt=516, ldg=516) == -1      # H < 4, H % 4, H > 512
    assert hops(ldt=508) == -1 and hops(ldg=508) == -1                                        # too small a stride
    assert hops(ldt=514) == -3 and hops(ldg=518) == -3                                        # strides not multiples of 4
    assert hops(Q=0) == 0                                                                     # nothing to do
    assert hops() == -1                                                                       # NULL pointers, refused not dereferenced
    assert hops(max_rows=80) == -1 and hops(Q=0, max_rows=80) == -1 and hops(H=64, ldt=64, ldg=64, max_rows=621) == -1   # beyond 160 KiB
    a = 64    # an aligned fake address: every call below is refused before a launch

    def at(T=a, G=a, us=a, ud=a):
        return h(a, a, T, 512, N, a, a, N, 0.2, us, ud, 0.2, a, a, a, 4, 512, 16, G, 512, N)
    assert at(T=a + 4) == -3 and at(G=a + 4) == -3 and at(us=a + 4) == -3 and at(ud=a + 4) == -3
    for miss in range(11):    # each required pointer in turn NULL
        ptrs = [a] * 11
        ptrs[miss] = N
        rp, cl, T, a_s, a_d, us, ud, sg, pr, pp, G = ptrs
        assert h(rp, cl, T, 512, N, a_s, a_d, N, 0.2, us, ud, 0.2, sg, pr, pp, 4, 512, 16, G, 512, N) == -1


def _model(layer="GATConv", layers=2, hidden=64, F=12):
    from fitgnn_amd import network
    args = argparse.Namespace(num_layers1=layers, layer_name=layer, num_features=F, hidden=hidden, num_classes=3)
    torch.manual_seed(0)
    return network.Classify_graph_gs(args).eval()


def test_gat_graph_query_supported_refuses_on_the_host():
    from fitgnn_amd import ops
    assert ops.gat_graph_query_supported(_model()) is False                       # two GATConv layers, but on the CPU
    assert ops.gat_graph_query_supported(_model(layer="GCNConv")) is False
    assert ops.gat_graph_query_supported(_model(layers=3)) is False
    assert ops.gat_graph_query_supported(_model(layers=1)) is False
    assert ops.gat_graph_query_supported(torch.nn.Linear(3, 3)) is False          # no conv stack at all
