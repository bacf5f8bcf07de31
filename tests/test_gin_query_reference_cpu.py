"""CPU tier of the GIN node-query path (fitgnn_amd/serve.py gin_kernels, csrc/query.hip gin_query_hops_kernel and
gin_query_tail_kernel): the float64 reference of tests/gin_query_reference.py against a two-layer GIN forward composed from the
oracle's gin_aggregate, the launchers' argument refusals, the exactness of the EXACT inputs the GPU test sends through the kernels,
and a float32 NumPy replay of the stated operation order that must give the float64 values bit for bit on those inputs."""
import numpy as np
import pytest
import torch

import gin_query_reference as gq
from oracle import gnn_oracle as gorc
from test_query_reference_cpu import _exactness_watch


def _graph(rng, n, n_edges):
    """A small directed graph with repeated edges, self loops, a node without incoming edges and one without any edge."""
    src, dst = rng.integers(0, n - 1, size=n_edges), rng.integers(1, n - 1, size=n_edges)   # row 0: no entry; node n - 1: isolated
    src[:3], dst[:3] = [2, 2, 5], [3, 3, 5]                                                     # a repeated edge, a self loop
    return np.stack([src, dst]).astype(np.int64)


@pytest.mark.parametrize("table", [False, True], ids=["rows", "table"])
def test_reference_equals_the_oracle_forward(table):
    """hops + tail on chosen rows == the whole-graph float64 forward (gin_aggregate, the MLP, ELU, twice, and the head), to 1e-12;
    with `table` the operand is a node table that several rows reference.  eps is non-zero in both layers."""
    rng = np.random.default_rng(31 + table)
    n, F, Ha, Hb, H2a, H2b, C = 40, 6, 16, 32, 48, 16, 5
    ei = _graph(rng, n, 150)
    g = lambda *s: rng.normal(0, 0.4, size=s)   # noqa: E731
    m = {"conv.0.nn.0.weight": g(Ha, F), "conv.0.nn.0.bias": g(Ha), "conv.0.nn.2.weight": g(Hb, Ha), "conv.0.nn.2.bias": g(Hb),
         "conv.1.nn.0.weight": g(H2a, Hb), "conv.1.nn.0.bias": g(H2a), "conv.1.nn.2.weight": g(H2b, H2a), "conv.1.nn.2.bias": g(H2b),
         "lt1.weight": g(C, H2b), "lt1.bias": g(C),
         "conv.0.eps": np.array([0.375], dtype=np.float32), "conv.1.eps": np.array([-0.625], dtype=np.float32)}   # 1 + eps exact in fp32
    n_nodes = 25 if table else n
    node_id = rng.integers(0, n_nodes, size=n) if table else np.arange(n)
    X = rng.normal(size=(n_nodes, F))
    x_union = X[node_id]
    rowptr, col, val = gq.sum_csr(ei, n)
    deg = np.diff(rowptr)
    assert deg[0] == 0 and deg[n - 1] == 0 and deg.max() > 4 and (val == 1).all()
    T = (X if table else x_union) @ m["conv.0.nn.0.weight"].T
    rows = np.concatenate([np.arange(n)[::-3], [0, n - 1, 0]])   # unsorted, with duplicates, a row without entries, the isolated node
    G = gq.hops(rowptr, col, val, T, m["conv.0.eps"][0], m["conv.0.nn.2.weight"], m["conv.0.nn.2.bias"], m["conv.1.eps"][0], rows,
                xrow=node_id if table else None, b0a=m["conv.0.nn.0.bias"])
    assert G.shape == (len(rows), Hb) and (G >= 0).all()
    sd = {k: torch.from_numpy(v) for k, v in m.items()}
    for lsm in (True, False):
        out = gq.tail(G, m["conv.1.nn.0.weight"], m["conv.1.nn.0.bias"], m["conv.1.nn.2.weight"], m["conv.1.nn.2.bias"], m["lt1.weight"],
                      m["lt1.bias"], log_softmax=lsm)
        ref = gq.oracle_forward(gorc, sd, torch.from_numpy(x_union), torch.from_numpy(ei), log_softmax=lsm).numpy()[rows]
        assert np.abs(out - ref).max() <= 1e-12


# ---- the stated order once more, in float32 ----
f32 = np.float32


def _chain32(A, W, b):
    acc = np.zeros((A.shape[0], W.shape[0]), dtype=f32)
    for k in range(A.shape[1]):
        acc = A[:, k:k + 1] * W[None, :, k] + acc
    return acc if b is None else acc + b[None, :]


def _hops32(c):
    rowptr, col, val, T, W, xrow = c["rowptr"], c["col"], c["val"].astype(f32), c["T"].astype(f32), c["W0b"].astype(f32), c["xrow"]
    t = (lambda r: r) if xrow is None else (lambda r: xrow[r])
    o0, o1 = f32(1.0) + f32(c["eps0"]), f32(1.0) + f32(c["eps1"])
    Hb = W.shape[0]

    def h(r):
        a = np.zeros(T.shape[1], dtype=f32)
        for e in range(rowptr[r], rowptr[r + 1]):
            a = val[e] * T[t(col[e])] + a
        a = o0 * T[t(r)] + a
        if c["b0a"] is not None:
            a = a + c["b0a"]
        return np.maximum(_chain32(np.maximum(a, f32(0))[None, :], W, c["b0b"])[0], f32(0))

    G = np.zeros((len(c["rows"]), Hb), dtype=f32)
    for i, q in enumerate(c["rows"]):
        P = np.zeros((4, Hb), dtype=f32)
        e0, e1 = rowptr[q], rowptr[q + 1]
        for k in range(e1 - e0 + 1):
            w, r = (val[e0 + k], col[e0 + k]) if k < e1 - e0 else (o1, q)
            P[(k % 16) // 4] = w * h(r) + P[(k % 16) // 4]
        G[i] = ((P[0] + P[1]) + P[2]) + P[3]
    assert G.dtype == f32
    return G


def _tail32(G, c):
    z1 = np.maximum(_chain32(G.astype(f32), c["W1a"], c["b1a"]), f32(0))
    z2 = np.maximum(_chain32(z1, c["W1b"], c["b1b"]), f32(0))
    out = _chain32(z2, c["Wl"], c["bl"])
    assert out.dtype == f32
    return out


def _hops64(c, watch=None, rows=None):
    return gq.hops(c["rowptr"], c["col"], c["val"], c["T"], c["eps0"], c["W0b"], c["b0b"], c["eps1"], c["rows"] if rows is None else rows,
                   xrow=c["xrow"], b0a=c["b0a"], watch=watch)


def _tail64(G, c, watch=None):
    return gq.tail(G, c["W1a"], c["b1a"], c["W1b"], c["b1b"], c["Wl"], c["bl"], watch=watch)


@pytest.mark.parametrize("case", gq.EXACT_HOPS_CASES, ids=str)
def test_exact_hops_inputs_are_exact(case):
    Ha, Hb, with_xrow, with_bias, eps0, eps1 = case
    c = gq.exact_hops_case(*case)
    watch, seen = _exactness_watch()
    G = _hops64(c, watch)
    assert seen["n"] > 1000 and np.isfinite(G).all() and G.shape == (len(c["rows"]), Hb) and c["W0b"].shape == (Hb, Ha)
    assert np.array_equal(c["T"] * 8, np.round(c["T"] * 8)) and (c["T"] < 0).any() and (c["T"] > 0).any()
    assert gq.one_plus(eps0) == 1.0 + eps0 and gq.one_plus(eps1) == 1.0 + eps1 and eps0 in (0.5, -0.25) and eps1 in (0.5, -0.25)
    deg = np.diff(c["rowptr"])
    assert deg[c["rows"]].tolist() == gq.HOPS_QUERY_DEGS
    assert set(gq.HOPS_ROW_DEGS) <= set(deg[c["col"][c["rowptr"][8]:c["rowptr"][9]]].tolist())   # the 40-entry query meets them all
    assert (G >= 0).all() and (G > 0).any() and (G[0] > 0).any()            # the query without entries still has (1 + eps1) h_q
    assert (G == 0).any() or Hb > 16                                        # ReLU's zero branch reaches the output somewhere
    if c["xrow"] is not None:
        assert c["xrow"][c["col"]].max() == c["T"].shape[0] - 1
        assert len(set(c["xrow"].tolist())) < len(c["xrow"])                # repeated table rows
    got = _hops32(c)
    assert np.array_equal(got.astype(np.float64), G), "the float32 replay of the stated order differs from the float64 reference"


@pytest.mark.parametrize("case", gq.EXACT_TAIL_CASES, ids=str)
def test_exact_tail_inputs_are_exact(case):
    K, H2a, H2b, C, Q, with_bias = case
    c = gq.exact_tail_case(*case)
    watch, seen = _exactness_watch()
    out = _tail64(c["G"], c, watch)
    assert seen["n"] >= K + H2a + H2b and np.isfinite(out).all() and out.shape == (Q, C)
    assert (out != 0).any() and len(np.unique(out)) > min(Q * C, 4) // 2
    assert np.array_equal(_tail32(c["G"], c).astype(np.float64), out)


@pytest.mark.parametrize("case", gq.CHAIN_CASES, ids=str)
def test_exact_chain_inputs_are_exact(case):
    Ha, Hb, H2a, H2b, C = case
    c = gq.exact_chain_case(*case)
    watch, seen = _exactness_watch()
    G = _hops64(c, watch)
    out = _tail64(G, c, watch)
    assert len(c["rows"]) > 32 and len(c["rows"]) % 16 != 0 and out.shape == (len(c["rows"]), C) and np.isfinite(out).all()
    assert set(np.unique(c["val"]).tolist()) <= {0.5, 1.0} and (G > 0).any() and len(np.unique(out)) > C
    G32 = _hops32(c)
    assert np.array_equal(G32.astype(np.float64), G) and np.array_equal(_tail32(G32, c).astype(np.float64), out)


def test_the_bound_covers_a_float32_run_of_the_same_order():
    """sums=True: the reference's bound holds for the same operation order carried out in float32.  NumPy's float32 arithmetic rounds
    every product on its own, which the bound's one-rounding-per-fmaf count does not cover: the CSR values and both 1 + eps are powers
    of two and W0b holds powers of two, so every product is exact and only the additions round."""
    rng = np.random.default_rng(3)
    rowptr, col, val, xrow, n_rows = gq.query_csr(rng, [0, 1, 2, 3, 4, 5, 9, 17, 33], [0, 1, 2, 7, 30], 19, True, pow2_val=True)
    Ha, Hb = 8, 16
    W0b = (rng.choice([-1.0, 1.0], size=(Hb, Ha)) * 2.0 ** rng.integers(-3, 1, size=(Hb, Ha))).astype(f32)
    c = dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=rng.normal(0, 1, size=(19, Ha)).astype(f32), b0a=rng.normal(0, 1, size=Ha).astype(f32),
             eps0=f32(1.0), W0b=W0b, b0b=rng.normal(0, 1, size=Hb).astype(f32), eps1=f32(-0.5), rows=np.arange(9, dtype=np.int64))
    ref, B = gq.hops(rowptr, col, val, c["T"], c["eps0"], W0b, c["b0b"], c["eps1"], c["rows"], xrow=xrow, b0a=c["b0a"], sums=True)
    err = np.abs(_hops32(c).astype(np.float64) - ref)
    assert (err <= 2.0 ** -24 * B).all() and err.max() > 0 and (B > 0).all()


def test_launchers_refuse_bad_arguments_without_touching_the_gpu():
    from fitgnn_amd import _lib
    L = _lib.lib()
    h = L.fitgnn_gin_query_hops_f32
    N = None

    def hops(Q=4, Ha=512, Hb=512, ldt=512, ldg=512):
        #        rowptr col val T  ldt xrow b0a eps0 W0b b0b eps1 rows Q  Ha  Hb  G  ldg stream
        return h(N, N, N, N, ldt, N, N, N, N, N, N, N, Q, Ha, Hb, N, ldg, N)

    assert hops(Q=-1) == -1
    assert hops(Ha=510) == -1 and hops(Ha=0) == -1 and hops(Ha=516, ldt=516) == -1           # Ha % 4, Ha < 4, Ha > 512
    assert hops(Hb=504) == -1 and hops(Hb=0) == -1 and hops(Hb=528, ldg=528) == -1           # Hb % 16, Hb < 16, Hb > 512
    assert hops(ldt=508) == -1 and hops(ldg=508) == -1                                      # too small a stride
    assert hops(ldt=514) == -3 and hops(ldg=518) == -3                                      # strides not multiples of 4
    assert hops(Q=0) == 0                                                                   # nothing to do
    assert hops() == -1                                                                     # NULL pointers, refused not dereferenced
    assert hops(Ha=4, Hb=16, ldt=4, ldg=16) == -1

    t = L.fitgnn_gin_query_tail_f32

    def tail(Q=4, K=512, H2a=512, H2b=512, C=7, ldg=512, ldo=7):
        #        G  ldg Q  W1a b1a W1b b1b Wl bl K  H2a  H2b  C  out ldo lsm stream
        return t(N, ldg, Q, N, N, N, N, N, N, K, H2a, H2b, C, N, ldo, 1, N)

    assert tail(Q=-1) == -1 and tail(K=510) == -1 and tail(K=0) == -1
    assert tail(H2a=520) == -1 and tail(H2a=0) == -1 and tail(H2b=520) == -1 and tail(H2b=0) == -1 and tail(C=0) == -1
    assert tail(ldg=508) == -1 and tail(ldo=6) == -1
    assert tail(ldg=514) == -3
    assert tail(Q=0) == 0 and tail() == -1
    lds = L.fitgnn_gin_query_tail_lds_bytes
    assert lds(512, 512, 48) == 4 * (16 * 516 * 2 + 256 * 36 + 16 * 36 + 16 * 48) <= 160 * 1024
    assert lds(0, 16, 1) == 0 and lds(16, 0, 1) == 0 and lds(16, 16, 0) == 0
    assert lds(1024, 1024, 7) > 160 * 1024 and tail(H2a=1024, H2b=1024) == -1 and tail(Q=0, H2a=1024, H2b=1024) == -1   # does not fit LDS
    assert lds(16, 16, 2400) > 160 * 1024 and tail(H2a=16, H2b=16, C=2400, ldo=2400) == -1
