"""CPU tier of the SAGE graph-query path (fitgnn_amd/serve.py GraphQueryEngine sage_kernels, csrc/query.hip
sage_graph_query_hops_kernel): the float64 reference of tests/sage_graph_query_reference.py against the per-row reference of
tests/sage_query_reference.py and against a dense float64 forward written out here, the exactness of the EXACT inputs the GPU test sends
through the kernel, a float32 NumPy replay of the stated operation order, the bound on such a replay, and the launcher's argument
refusals -- all before any launch."""
import numpy as np
import pytest
import torch

import graph_query_reference as gr
import sage_graph_query_reference as sgq
import sage_query_reference as sq
from oracle import gnn_oracle as gorc
from test_query_reference_cpu import _exactness_watch

f32 = np.float32


def _elu32(pre):
    return np.where(pre > 0, pre, np.expm1(np.minimum(pre, 0).astype(np.float64)).astype(f32)).astype(f32)


def _hops32(c):
    """The stated order once more, in float32 (exact inputs make every product exact: a separate product rounding cannot show)."""
    rowptr, col, val, T, xrow = c["rowptr"], c["col"], c["val"].astype(f32), c["T"].astype(f32), c["xrow"]
    H = T.shape[1] // 2
    t = (lambda r: r) if xrow is None else (lambda r: xrow[r])
    G = np.zeros((len(c["prow"]), 2 * H), dtype=f32)
    for i, (r0, r1) in enumerate(c["seg"]):
        hs = np.zeros((r1 - r0, H), dtype=f32)             # the window: every row of the graph, once
        for r in range(r0, r1):
            a = np.zeros(H, dtype=f32)
            for e in range(rowptr[r], rowptr[r + 1]):
                a = val[e] * T[t(col[e]), :H] + a
            pre = a + T[t(r), H:]
            if c["b0"] is not None:
                pre = pre + c["b0"]
            hs[r - r0] = _elu32(pre)
        for j in range(c["pptr"][i], c["pptr"][i + 1]):
            r = c["prow"][j]
            g = np.zeros(H, dtype=f32)
            for e in range(rowptr[r], rowptr[r + 1]):
                g = val[e] * hs[col[e] - r0] + g
            G[j, :H], G[j, H:] = g, hs[r - r0]
    assert G.dtype == f32
    return G


@pytest.mark.parametrize("case", sgq.EXACT_HOPS_CASES, ids=str)
def test_exact_inputs_are_exact(case):
    H = case[0]
    c = sgq.exact_case(*case)
    watch, seen = _exactness_watch()
    G = sgq.run(c, watch=watch, f32_elu=True)
    assert seen["n"] > 1000 and np.isfinite(G).all() and G.shape == (len(c["prow"]), 2 * H) and c["T"].shape[1] == 2 * H
    assert np.array_equal(c["T"] * 8, np.round(c["T"] * 8)) and set(np.unique(c["val"]).tolist()) <= {0.25, 0.5, 1.0}
    size = (c["seg"][:, 1] - c["seg"][:, 0]).tolist()
    assert sorted(set(size)) == sgq.HOPS_SIZES == [1, 2, 3, 4, 5, 17] and len(size) > len(set(size))   # every size, one graph twice
    assert size != sorted(size)                                                                        # queried unsorted
    deg = np.diff(c["rowptr"])
    assert set(deg.tolist()) == set(sgq.HOPS_ROW_DEGS) >= {0, 1, 63, 64, 65} and set(deg[c["prow"]].tolist()) == set(sgq.HOPS_ROW_DEGS)
    cnt = np.diff(c["pptr"])
    assert (cnt == 0).any() and (cnt == np.array(size)).any() and ((cnt > 1) & (cnt < np.array(size))).any()
    assert (np.diff(c["prow"]) < -1).any()                      # a non-contiguous descending subset
    lone = deg[c["prow"]] == 0
    assert lone.any() and np.all(G[lone, :H] == 0) and np.any(G[lone, H:] != 0)   # no entries: g = 0 and still h_r
    if c["xrow"] is not None:
        assert c["xrow"].max() == c["T"].shape[0] - 1 and len(set(c["xrow"].tolist())) < len(c["xrow"])
    if c["b0"] is not None:
        assert (G < 0).any() and (G > 0).any()                  # both ELU branches reach the output
    assert np.array_equal(_hops32(c).astype(np.float64), G), "the float32 replay of the stated order differs from the float64 reference"
    # exact inputs remove the fold-order difference: the per-row reference, four partials and all, gives the same values
    Gn = sgq.run_rows(c, watch=watch, f32_elu=True)
    assert np.array_equal(Gn, G)


@pytest.mark.parametrize("H", [64, 512])
def test_exact_window_inputs_are_exact(H):
    from fitgnn_amd import ops
    n = ops.sage_graph_query_max_rows(H)            # the GPU test's graph: exactly the largest window
    assert n == {64: 640, 512: 160}[H] == sgq.max_rows(H)
    c = sgq.window_case(H, n + 1)
    assert (c["seg"][:, 1] - c["seg"][:, 0]).tolist() == [n + 1, 3, 2] and np.diff(c["pptr"]).tolist() == [n + 1, 3, 2]
    c = sgq.window_case(H, n)
    assert c["max_rows"] == n
    watch, seen = _exactness_watch()
    G = sgq.run(c, watch=watch, f32_elu=True)
    assert seen["n"] > 100 and np.array_equal(_hops32(c).astype(np.float64), G)
    assert np.array_equal(sgq.run_rows(c, f32_elu=True), G)


@pytest.mark.parametrize("with_xrow,with_b0", [(False, True), (True, True), (True, False)], ids=str)
def test_hops_on_all_rows_agree_with_the_per_row_reference(with_xrow, with_b0):
    """Every row of a random view pooled: hops forms each layer-0 row once, sage_query_reference.gather forms it per entry and folds
    four partials -- the same values to 1e-12 relative; the h halves and their bounds are the same expression and agree exactly."""
    c = sgq.random_case(48, with_xrow, with_b0, graphs=[5, 0, 3, 1, 4, 2], kinds=["all"])
    assert len(c["prow"]) == int(c["gptr"][-1]) and np.allclose(c["val"][: 1], 1.0 / max(np.diff(c["rowptr"])[0], 1))
    G, B = sgq.run(c, sums=True)
    Gn, Bn = sgq.run_rows(c, sums=True)
    assert G.shape == Gn.shape == (len(c["prow"]), 96)
    assert np.abs(G - Gn).max() <= 1e-12 * np.abs(Gn).max() and np.abs(G).max() > 0.1
    assert np.array_equal(G[:, 48:], Gn[:, 48:]) and np.array_equal(B[:, 48:], Bn[:, 48:]) and (B[:, 48:] > 0).all()
    deg = np.diff(c["rowptr"])[c["prow"]]
    assert (B[deg == 0, :48] == 0).all() and (B[deg > 0, :48] > 0).all()


def _dense_forward(X, ei, gptr, m, seg, prow, pptr, pool, softmax):
    """Per queried graph, a plain dense float64 forward on the graph's own rows: A_mean (X W_l^T) + X W_r^T + b_l, ELU, twice, the pool
    over the pooled rows, the head, the softmax.  A_mean[i][j] = (number of edges j -> i) / max(in-degree(i), 1)."""
    elu = lambda a: np.where(a > 0, a, np.expm1(np.minimum(a, 0)))   # noqa: E731
    out = []
    for i, (r0, r1) in enumerate(seg):
        n = r1 - r0
        A = np.zeros((n, n))
        for s, d in ei.T:
            if r0 <= d < r1:
                assert r0 <= s < r1
                A[d - r0, s - r0] += 1.0
        A /= np.maximum(A.sum(1, keepdims=True), 1.0)
        h = X[r0:r1]
        for l in range(2):
            p = f"conv.{l}."
            h = elu(A @ (h @ m[p + "lin_l.weight"].T) + h @ m[p + "lin_r.weight"].T + m.get(p + "lin_l.bias", 0.0))
        rows = np.asarray(prow[pptr[i]:pptr[i + 1]], dtype=np.int64) - r0
        z = h[rows].max(0) if pool == "max" else h[rows].mean(0)
        y = z @ m["lt1.weight"].T + m["lt1.bias"]
        if softmax:
            y = np.exp(y - y.max())
            y = y / y.sum()
        out.append(y)
    return np.stack(out)


@pytest.mark.parametrize("pool,softmax,bias", [("max", True, True), ("mean", False, True), ("mean", True, False)])
def test_reference_equals_the_oracle_forward_and_a_dense_forward(pool, softmax, bias):
    """hops + graph_query_reference.pooled_tail (K = 2H, W1 = [W_l1 | W_r1], b1 = b_l1) == model_forward (gorc.sage_conv, twice, on the
    whole view) == the dense per-graph forward above, to 1e-12.  Pooled rows: all of a graph, a subset, one."""
    rng = np.random.default_rng(97 + softmax + 2 * bias)
    F, H, H2, C = 6, 16, 32, 5
    sizes = [1, 4, 7, 17, 2]
    gptr = np.concatenate([[0], np.cumsum(sizes)])
    n = int(gptr[-1])
    src, dst = [], []
    for g, k in enumerate(sizes):          # repeated edges and self loops inside each graph
        src += rng.integers(gptr[g], gptr[g + 1], size=3 * k).tolist()
        dst += rng.integers(gptr[g], gptr[g + 1], size=3 * k).tolist()
    ei = np.stack([src, dst]).astype(np.int64)
    ei = ei[:, (ei[1] != gptr[3] + 1) & (ei[1] != gptr[2])]      # two rows without entries (they still send edges): h = ELU(root + b0)
    g_ = lambda *s: rng.normal(0, 0.4, size=s)   # noqa: E731
    m = {"conv.0.lin_l.weight": g_(H, F), "conv.0.lin_r.weight": g_(H, F), "conv.1.lin_l.weight": g_(H2, H), "conv.1.lin_r.weight": g_(H2, H),
         "conv.1.lin_l.bias": g_(H2), "lt1.weight": g_(C, H2), "lt1.bias": g_(C)}
    if bias:
        m["conv.0.lin_l.bias"] = g_(H)
    X = rng.normal(size=(n, F))
    rowptr, col, val = sgq.mean_csr(ei, n)
    assert (np.diff(rowptr) == 0).sum() >= 2 and np.diff(rowptr).max() > 4
    seg, prow, pptr = gr.pooled_rows(rng, gptr, [3, 0, 2, 1, 3, 4], ["all", "all", "subset", "first", "subset", "first"])
    assert 1 in np.diff(pptr).tolist()
    T = X @ np.concatenate([m["conv.0.lin_l.weight"], m["conv.0.lin_r.weight"]], 0).T
    G = sgq.hops(rowptr, col, val, T, seg, prow, pptr, b0=m.get("conv.0.lin_l.bias"))
    assert G.shape == (len(prow), 2 * H)
    W1cat = np.concatenate([m["conv.1.lin_l.weight"], m["conv.1.lin_r.weight"]], 1)
    out = gr.pooled_tail(G, pptr, W1cat, m["conv.1.lin_l.bias"], m["lt1.weight"], m["lt1.bias"], pool=pool, softmax=softmax)
    sd = {k: torch.from_numpy(v) for k, v in m.items()}
    ref = sgq.model_forward(gorc, sd, torch.from_numpy(X), torch.from_numpy(ei), seg, prow, pptr, pool, softmax)
    dense = _dense_forward(X, ei, gptr, m, seg, prow, pptr, pool, softmax)
    assert out.shape == ref.shape == dense.shape == (6, C)
    assert np.abs(out - ref).max() <= 1e-12 and np.abs(ref - dense).max() <= 1e-12


def test_the_bound_covers_a_float32_run_of_the_same_order():
    """sums=True: the reference's bound holds for the same operation order carried out in float32.  NumPy's float32 arithmetic rounds
    every product on its own, which the bound's one-rounding-per-fmaf count does not cover: the CSR values are powers of two, so every
    product is exact and only the additions (and expm1) round."""
    rng = np.random.default_rng(101)
    rowptr, col, val, xrow, gptr = gr.graph_view(rng, [1, 2, 5, 17, 33], [0, 1, 2, 7, 30], 19, True, pow2_val=True)
    H = 8
    seg, prow, pptr = gr.pooled_rows(rng, gptr, [4, 0, 2, 3, 1], ["all", "all", "subset", "first", "all"])
    c = dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=rng.normal(0, 1, size=(19, 2 * H)).astype(f32),
             b0=rng.normal(0, 1, size=H).astype(f32), seg=seg, prow=prow, pptr=pptr)
    ref, B = sgq.run(c, sums=True)
    err = np.abs(_hops32(c).astype(np.float64) - ref)
    assert (err <= 2.0 ** -24 * B).all() and err.max() > 0 and (B[:, H:] > 0).all()
    deg = np.diff(rowptr)[prow]
    assert (B[deg == 0, :H] == 0).all() and (err[deg == 0, :H] == 0).all()


def test_launcher_refuses_bad_arguments_without_touching_the_gpu():
    from fitgnn_amd import _lib, ops
    L = _lib.lib()
    h = L.fitgnn_sage_graph_query_hops_f32
    N = None

    def hops(Q=4, H=512, max_rows=16, ldt=1024, ldg=1024):
        #        rowptr col val T  ldt xrow b0 seg prow pptr Q  H  max_rows G  ldg stream
        return h(N, N, N, N, ldt, N, N, N, N, N, Q, H, max_rows, N, ldg, N)

    assert hops(Q=-1) == -1 and hops(max_rows=-1) == -1
    assert hops(H=510) == -1 and hops(H=0) == -1 and hops(H=14) == -1 and hops(H=6) == -1     # H % 4, H < 4
    assert hops(ldt=1020) == -1 and hops(ldg=1020) == -1 and hops(ldt=512) == -1 and hops(ldg=512) == -1   # strides below 2H
    assert hops(ldt=1026) == -3 and hops(ldg=1030) == -3                                      # strides not multiples of 4
    assert hops(Q=0) == 0                                                                     # nothing to do
    assert hops() == -1                                                                       # NULL pointers, refused not dereferenced
    assert hops(Q=0, H=2048, ldt=4096, ldg=4096) == 0                                         # no H <= 512 limit
    a = 64    # an aligned fake address: every call below is refused before a launch
    assert h(a, a, a, a + 4, 1024, N, N, a, a, a, 4, 512, 16, a, 1024, N) == -3               # T misaligned, nothing launched
    assert h(a, a, a, a, 1024, N, N, a, a, a, 4, 512, 16, a + 4, 1024, N) == -3               # G
    for k in (0, 1, 2, 3, 7, 8, 9, 13):                                                       # every required pointer
        args = [a, a, a, a, 1024, N, N, a, a, a, 4, 512, 16, a, 1024, N]
        args[k] = N
        assert h(*args) == -1, k

    lds = L.fitgnn_sage_graph_query_hops_lds_bytes
    assert lds(160, 512) == 160 * 256 * 4 == 160 * 1024 < lds(161, 512) and lds(640, 64) == 640 * 64 * 4 == 160 * 1024 < lds(641, 64)
    assert lds(7, 260) == 7 * 256 * 4 and lds(7, 4) == 7 * 4 * 4 and lds(0, 64) == 0
    assert lds(-1, 64) == 0 and lds(4, 0) == 0 and lds(4, 3) == 0
    assert lds(9, 64) == L.fitgnn_gcn_graph_query_hops_lds_bytes(9, 64)
    assert ops.sage_graph_query_max_rows(512) == 160 and ops.sage_graph_query_max_rows(64) == 640 and ops.sage_graph_query_max_rows(0) == 0
    assert hops(max_rows=161) == -1 and hops(Q=0, max_rows=161) == -1 and hops(H=64, ldt=128, ldg=128, max_rows=641) == -1   # beyond 160 KiB
    assert hops(H=64, ldt=128, ldg=128, max_rows=640, Q=0) == 0
