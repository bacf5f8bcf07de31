"""CPU tier of the SAGE node-query path (fitgnn_amd/serve.py sage_kernels, csrc/query.hip sage_query_gather_kernel): the float64
reference of tests/sage_query_reference.py against a two-layer SAGE forward composed from the oracle's sage_conv, the launcher's
argument refusals, and the exactness of the EXACT inputs the GPU test sends through the kernel (and, for the chain cases, on through
the tail)."""
import numpy as np
import pytest
import torch

import query_reference as qr
import sage_query_reference as sq
from oracle import gnn_oracle as gorc
from test_query_reference_cpu import _exactness_watch


def _graph(rng, n, n_edges):
    """A small directed graph with repeated edges, self loops, a node without incoming edges and one without any edge."""
    src, dst = rng.integers(0, n - 1, size=n_edges), rng.integers(1, n - 1, size=n_edges)   # row 0: no entry; node n - 1: isolated
    src[:3], dst[:3] = [2, 2, 5], [3, 3, 5]                                                     # a repeated edge, a self loop
    return np.stack([src, dst]).astype(np.int64)


@pytest.mark.parametrize("table,bias", [(False, True), (True, True), (True, False)], ids=str)
def test_reference_equals_the_oracle_forward(table, bias):
    """gather + tail (K = 2H, W1 = [W_l1 | W_r1]) on chosen rows == ELU(sage_conv) twice and the head in float64 on the whole
    graph, to 1e-12; with `table` the operand is a node table that several rows reference."""
    rng = np.random.default_rng(11 + 2 * table + bias)
    n, F, H, H2, C = 40, 6, 16, 32, 5
    ei = _graph(rng, n, 150)
    g = lambda *s: rng.normal(0, 0.4, size=s)   # noqa: E731
    m = {"conv.0.lin_l.weight": g(H, F), "conv.0.lin_r.weight": g(H, F), "conv.1.lin_l.weight": g(H2, H), "conv.1.lin_r.weight": g(H2, H),
         "conv.1.lin_l.bias": g(H2), "lt1.weight": g(C, H2), "lt1.bias": g(C)}
    if bias:
        m["conv.0.lin_l.bias"] = g(H)
    n_nodes = 25 if table else n
    node_id = rng.integers(0, n_nodes, size=n) if table else np.arange(n)
    X = rng.normal(size=(n_nodes, F))
    x_union = X[node_id]
    rowptr, col, val = sq.mean_csr(ei, n)
    deg = np.diff(rowptr)
    assert deg[0] == 0 and deg[n - 1] == 0 and deg.max() > 4 and np.allclose(val[rowptr[3]:rowptr[4]], 1.0 / deg[3])
    T = (X if table else x_union) @ np.concatenate([m["conv.0.lin_l.weight"], m["conv.0.lin_r.weight"]], 0).T
    rows = np.concatenate([np.arange(n)[::-3], [0, n - 1, 0]])   # unsorted, with duplicates, a row without entries, the isolated node
    G = sq.gather(rowptr, col, val, T, rows, xrow=node_id if table else None, b0=m.get("conv.0.lin_l.bias"))
    assert G.shape == (len(rows), 2 * H) and np.all(G[-1, :H] == 0)
    W1cat = np.concatenate([m["conv.1.lin_l.weight"], m["conv.1.lin_r.weight"]], 1)
    sd = {k: torch.from_numpy(v) for k, v in m.items()}
    for lsm in (True, False):
        out = qr.tail(G, W1cat, m["conv.1.lin_l.bias"], m["lt1.weight"], m["lt1.bias"], log_softmax=lsm)
        ref = sq.oracle_forward(gorc, sd, torch.from_numpy(x_union), torch.from_numpy(ei), log_softmax=lsm).numpy()[rows]
        assert np.abs(out - ref).max() <= 1e-12


def test_the_bound_covers_a_float32_run_of_the_same_order():
    """sums=True: the reference's bound holds for the same operation order carried out in float32 (numpy float32 arithmetic rounds
    every product separately, which the bound's one-rounding-per-fmaf count does not cover: the products are made exact by
    power-of-two CSR values)."""
    rng = np.random.default_rng(3)
    rowptr, col, val, xrow, n_rows = qr.query_csr(rng, [0, 1, 2, 3, 4, 5, 9, 17], [0, 1, 2, 7, 30], 19, True, pow2_val=True)
    H = 8
    T = rng.normal(0, 1, size=(19, 2 * H)).astype(np.float32)
    b0 = rng.normal(0, 1, size=H).astype(np.float32)
    rows = np.arange(8)
    ref, B = sq.gather(rowptr, col, val, T, rows, xrow=xrow, b0=b0, sums=True)

    f = np.float32

    def row32(r):
        a = np.zeros(H, dtype=f)
        for e in range(rowptr[r], rowptr[r + 1]):
            a = f(val[e]) * T[xrow[col[e]], :H] + a
        pre = (a + T[xrow[r], H:]) + b0
        return np.where(pre > 0, pre, np.expm1(np.minimum(pre, 0).astype(np.float64)).astype(f)).astype(f)

    got = np.zeros((8, 2 * H), dtype=f)
    for i, q in enumerate(rows):
        part = np.zeros((4, H), dtype=f)
        for k, e in enumerate(range(rowptr[q], rowptr[q + 1])):
            part[k % 4] = f(val[e]) * row32(col[e]) + part[k % 4]
        got[i, :H] = ((part[0] + part[1]) + part[2]) + part[3]
        got[i, H:] = row32(q)
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= 2.0 ** -24 * B).all() and err.max() > 0 and (B[0, :H] == 0).all() and (B[:, H:] > 0).all()


def test_launcher_refuses_bad_arguments_without_touching_the_gpu():
    from fitgnn_amd import _lib
    g = _lib.lib().fitgnn_sage_query_gather_f32
    #        rowptr col  val   T    ldt   xrow  b0    rows  Q   H    G    ldg   stream
    assert g(None, None, None, None, 1024, None, None, None, -1, 512, None, 1024, None) == -1    # Q < 0
    assert g(None, None, None, None, 1024, None, None, None, 4, 510, None, 1024, None) == -1     # H % 4 != 0
    assert g(None, None, None, None, 1024, None, None, None, 4, 0, None, 1024, None) == -1       # H < 4
    assert g(None, None, None, None, 1020, None, None, None, 4, 512, None, 1024, None) == -1     # ldt < 2H
    assert g(None, None, None, None, 1024, None, None, None, 4, 512, None, 1020, None) == -1     # ldg < 2H
    assert g(None, None, None, None, 1026, None, None, None, 4, 512, None, 1024, None) == -3     # ldt % 4 != 0
    assert g(None, None, None, None, 1024, None, None, None, 4, 512, None, 1030, None) == -3     # ldg % 4 != 0
    assert g(None, None, None, None, 1024, None, None, None, 0, 512, None, 1024, None) == 0      # nothing to do
    assert g(None, None, None, None, 1024, None, None, None, 4, 512, None, 1024, None) == -1     # NULL pointers, refused not dereferenced
    assert g(None, None, None, None, 4096, None, None, None, 0, 2048, None, 4096, None) == 0     # no H <= 512 limit


@pytest.mark.parametrize("case", sq.EXACT_SAGE_CASES, ids=str)
def test_exact_gather_inputs_are_exact(case):
    c = sq.exact_sage_case(*case)
    H = case[0]
    watch, seen = _exactness_watch()
    G = sq.gather(c["rowptr"], c["col"], c["val"], c["T"], c["rows"], xrow=c["xrow"], b0=c["b0"], watch=watch, f32_elu=True)
    assert seen["n"] > 1000 and np.isfinite(G).all() and G.shape == (len(c["rows"]), 2 * H)
    assert c["T"].shape[1] == 2 * H and np.array_equal(c["T"] * 8, np.round(c["T"] * 8))
    deg = np.diff(c["rowptr"])
    assert deg[c["rows"]].tolist() == sq.GATHER_QUERY_DEGS
    assert sorted(set((deg[c["rows"]] % 4).tolist())) == [0, 1, 2, 3]          # the item after the last entry meets every wave
    assert set(sq.GATHER_NEIGHBOUR_DEGS) <= set(deg[c["col"][c["rowptr"][11]:c["rowptr"][12]]].tolist())   # the 130-entry query meets them all
    assert np.all(G[0, :H] == 0) and np.any(G[0, H:] != 0)                    # no entries: g = 0, h_q all the same
    if c["xrow"] is not None:
        assert c["xrow"][c["col"]].max() == c["T"].shape[0] - 1
        assert len(set(c["xrow"].tolist())) < len(c["xrow"])                   # repeated table rows
    if c["b0"] is not None:
        assert (G < 0).any() and (G > 0).any()    # both ELU branches reach the output


@pytest.mark.parametrize("case", sq.CHAIN_CASES, ids=str)
def test_exact_chain_inputs_are_exact(case):
    H, H2, C = case
    c = sq.exact_chain_case(*case)
    watch, seen = _exactness_watch()
    G = sq.gather(c["rowptr"], c["col"], c["val"], c["T"], c["rows"], xrow=c["xrow"], b0=c["b0"], watch=watch, f32_elu=True)
    assert c["W1"].shape == (H2, 2 * H) and len(c["rows"]) > 16
    out = qr.tail(G, c["W1"], c["b1"], c["Wl"], c["bl"], watch=watch, f32_elu=True)
    assert seen["n"] > 2 * H and np.isfinite(out).all() and out.shape == (len(c["rows"]), C)
    assert set(np.unique(c["val"]).tolist()) <= {0.5, 1.0}
