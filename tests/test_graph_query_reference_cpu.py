"""CPU tier of the graph-query path (fitgnn_amd/serve.py GraphQueryEngine, csrc/query.hip): the float64 references of
tests/graph_query_reference.py against a plain dense two-layer forward + pool + head, the exactness of the EXACT inputs the GPU test
sends through the kernels, the launchers' argument refusals and the LDS sizes they report."""
import numpy as np
import pytest

import graph_query_reference as gq
import query_reference as qr
from test_query_reference_cpu import _exactness_watch


@pytest.mark.parametrize("pool,softmax,with_xrow", [("max", True, False), ("mean", False, True), ("max", False, True)], ids=str)
def test_reference_equals_a_dense_forward_per_graph(pool, softmax, with_xrow):
    """hops + pooled_tail == per graph, A (X W0^T) ... on the graph's own rows, the pool over its pooled rows, the head: to 1e-12."""
    rng = np.random.default_rng(5)
    F, H, C, n_table = 6, 16, 5, 23
    rowptr, col, val, xrow, gptr = gq.graph_view(rng, [1, 4, 9, 17, 6], [0, 1, 2, 5, 3], n_table, with_xrow, pow2_val=False)
    n = int(gptr[-1])
    g = lambda *s: rng.normal(0, 0.4, size=s)   # noqa: E731
    W0, b0, W1, b1, Wl, bl = g(H, F), g(H), g(H, H), g(H), g(C, H), g(C)
    X = rng.normal(size=(n_table if with_xrow else n, F))
    seg, prow, pptr = gq.pooled_rows(rng, gptr, [3, 0, 4, 3, 1, 2], ["all", "all", "subset", "all", "first", "subset"])
    G = gq.hops(rowptr, col, val, X @ W0.T, seg, prow, pptr, xrow=xrow, b0=b0)
    out = gq.pooled_tail(G, pptr, W1, b1, Wl, bl, pool=pool, softmax=softmax)
    x_view = X[xrow] if with_xrow else X
    ref = gq.dense_graph_forward(x_view, rowptr, col, val, seg, prow, pptr, W0, b0, W1, b1, Wl, bl, pool, softmax)
    assert out.shape == (6, C) and np.abs(out - ref).max() <= 1e-12
    assert np.array_equal(out[0], out[3])        # the graph queried twice
    if softmax:
        assert np.abs(out.sum(1) - 1).max() <= 1e-12


def test_hops_equals_the_per_row_gather_apart_from_the_wave_partials():
    """The per-row gather forms the same h rows; its g differs only in how the row's entries are split over four partials."""
    c = gq.hops_case(64, True, True, exact=False)
    G = gq.hops(c["rowptr"], c["col"], c["val"], c["T"], c["seg"], c["prow"], c["pptr"], xrow=c["xrow"], b0=c["b0"])
    ref = qr.gather(c["rowptr"], c["col"], c["val"], c["T"], c["prow"], xrow=c["xrow"], b0=c["b0"])
    assert np.abs(G - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_an_empty_segment_pools_to_zeros_and_the_head_still_adds_its_bias():
    c = gq.exact_tail_case(4, 16, 1, True, True, "max")
    for pool in ("max", "mean"):
        out = gq.pooled_tail(c["G"], c["pptr"], c["W1"], c["b1"], c["Wl"], c["bl"], pool=pool)
        assert c["pptr"][1] == c["pptr"][0] and np.array_equal(out[0], c["bl"].astype(np.float64))


@pytest.mark.parametrize("case", gq.EXACT_HOPS_CASES, ids=str)
def test_exact_hops_inputs_are_exact(case):
    c = gq.hops_case(*case)
    watch, seen = _exactness_watch()
    G = gq.hops(c["rowptr"], c["col"], c["val"], c["T"], c["seg"], c["prow"], c["pptr"], xrow=c["xrow"], b0=c["b0"], watch=watch, f32_elu=True)
    assert seen["n"] > 1000 and np.isfinite(G).all()
    deg = np.diff(c["rowptr"])
    assert {0, 1, 63, 64, 65} <= set(deg.tolist()) and {0, 1, 63, 64, 65} <= set(deg[c["prow"]].tolist())
    assert sorted(set((c["seg"][:, 1] - c["seg"][:, 0]).tolist())) == [1, 2, 3, 4, 5, 17]
    assert (np.diff(c["pptr"]) == 0).any() and len(set(map(tuple, c["seg"].tolist()))) < len(c["seg"])   # a graph without pooled rows; a repeat
    if c["xrow"] is not None:
        assert c["xrow"][c["col"]].max() == c["T"].shape[0] - 1
    if c["b0"] is not None:
        assert (G < 0).any() and (G > 0).any()    # both ELU branches reach the output


@pytest.mark.parametrize("H", [4, 64, 256, 260, 512])
def test_exact_window_inputs_are_exact(H):
    from fitgnn_amd import _lib
    n = 160 * 1024 // int(_lib.lib().fitgnn_gcn_graph_query_hops_lds_bytes(1, H))
    assert n == 160 * 1024 // (4 * min(H, 256))
    c = gq.window_case(H, n)
    watch, seen = _exactness_watch()
    G = gq.hops(c["rowptr"], c["col"], c["val"], c["T"], c["seg"], c["prow"], c["pptr"], b0=c["b0"], watch=watch, f32_elu=True)
    assert G.shape == (n + 3, H) and seen["n"] > n


@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("case", gq.EXACT_TAIL_CASES, ids=str)
def test_exact_tail_inputs_are_exact(case, pool):
    c = gq.exact_tail_case(*case, pool)
    watch, seen = _exactness_watch()
    out = gq.pooled_tail(c["G"], c["pptr"], c["W1"], c["b1"], c["Wl"], c["bl"], pool=pool, watch=watch, f32_elu=True, f32_div=True)
    assert seen["n"] > case[0] and np.isfinite(out).all()
    lens = np.diff(c["pptr"]).tolist()
    assert lens == (gq.TAIL_SEGMENTS if pool == "max" else gq.TAIL_SEGMENTS_POW2)


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_the_trap_cases_are_exact_and_would_catch_their_bug(pool):
    c = gq.dead_rows_case(pool)
    watch, _ = _exactness_watch()
    out = gq.pooled_tail(c["G"], c["pptr"], c["W1"], c["b1"], c["Wl"], c["bl"], pool=pool, watch=watch, f32_elu=True, f32_div=True)
    # every pooled row is exactly -1: the logits are bl - sum_h Wl; a padded row (z = 32) in the pool would move them
    assert np.array_equal(out, np.tile(c["bl"] - c["Wl"].sum(1), (len(c["pptr"]) - 1, 1)).astype(np.float64))
    c = gq.neighbour_case(pool)
    watch, _ = _exactness_watch()
    out = gq.pooled_tail(c["G"], c["pptr"], c["W1"], c["b1"], c["Wl"], c["bl"], pool=pool, watch=watch, f32_elu=True, f32_div=True)
    z, _ = gq.layer1(c["G"], c["W1"], c["b1"])
    assert z[c["pptr"][1]:c["pptr"][2]].max() >= 256 * z[: c["pptr"][1]].max() > 0


def test_softmax_bound_covers_a_perturbed_softmax():
    """The bound with B = the perturbation (in units of 2^-24) covers the change of the float64 softmax, rows 1e4 apart included."""
    rng = np.random.default_rng(3)
    x = rng.normal(0, 3, size=(50, 7))
    x[::5, 0] += 1e4
    d = rng.uniform(-1, 1, size=x.shape) * 40 * 2.0 ** -24 * np.maximum(np.abs(x), 1)
    sm = lambda a: np.exp(a - a.max(1, keepdims=True)) / np.exp(a - a.max(1, keepdims=True)).sum(1, keepdims=True)   # noqa: E731
    bound = 2.0 ** -24 * gq.softmax_bound(x, np.abs(d) / 2.0 ** -24)
    assert np.all(np.abs(sm(x + d) - sm(x)) <= bound)


def test_launchers_refuse_bad_arguments_without_touching_the_gpu():
    from fitgnn_amd import _lib
    L = _lib.lib()
    h = L.fitgnn_gcn_graph_query_hops_f32
    #        rowptr col  val   T    ldt  xrow  b0    seg   prow  pptr  Q   H  max_rows G   ldg  stream
    assert h(None, None, None, None, 512, None, None, None, None, None, -1, 512, 8, None, 512, None) == -1     # Q < 0
    assert h(None, None, None, None, 512, None, None, None, None, None, 4, 510, 8, None, 512, None) == -1      # H % 4 != 0
    assert h(None, None, None, None, 508, None, None, None, None, None, 4, 512, 8, None, 512, None) == -1      # ldt < H
    assert h(None, None, None, None, 512, None, None, None, None, None, 4, 512, 8, None, 508, None) == -1      # ldg < H
    assert h(None, None, None, None, 512, None, None, None, None, None, 4, 512, -1, None, 512, None) == -1     # max_rows < 0
    assert h(None, None, None, None, 514, None, None, None, None, None, 4, 512, 8, None, 512, None) == -3      # ldt % 4 != 0
    assert h(None, None, None, None, 512, None, None, None, None, None, 4, 512, 161, None, 512, None) == -1    # the window beyond 160 KiB
    assert h(None, None, None, None, 512, None, None, None, None, None, 0, 512, 160, None, 512, None) == 0     # nothing to do
    assert h(None, None, None, None, 512, None, None, None, None, None, 4, 512, 160, None, 512, None) == -1    # NULL pointers, refused not dereferenced
    hl = L.fitgnn_gcn_graph_query_hops_lds_bytes
    assert hl(160, 512) == 160 * 1024 and hl(160, 256) == 160 * 1024 and hl(17, 260) == 17 * 1024 and hl(10240, 4) == 160 * 1024
    assert hl(3, 64) == 3 * 64 * 4 and hl(-1, 64) == 0 and hl(0, 64) == 0
    t = L.fitgnn_gcn_graph_query_tail_f32
    #        G    ldg  pptr  Q   W1    b1    Wl    bl    H    H2   C  pool sm out  ldo stream
    assert t(None, 512, None, -1, None, None, None, None, 512, 512, 7, 0, 0, None, 7, None) == -1       # Q < 0
    assert t(None, 512, None, 4, None, None, None, None, 510, 512, 7, 0, 0, None, 7, None) == -1        # H % 4 != 0
    assert t(None, 512, None, 4, None, None, None, None, 512, 520, 7, 0, 0, None, 7, None) == -1        # H2 % 16 != 0
    assert t(None, 508, None, 4, None, None, None, None, 512, 512, 7, 0, 0, None, 7, None) == -1        # ldg < H
    assert t(None, 512, None, 4, None, None, None, None, 512, 512, 7, 0, 0, None, 6, None) == -1        # ldo < C
    assert t(None, 512, None, 4, None, None, None, None, 512, 512, 7, 2, 0, None, 7, None) == -1        # pool outside {0, 1}
    assert t(None, 514, None, 4, None, None, None, None, 512, 512, 7, 0, 0, None, 7, None) == -3        # ldg % 4 != 0
    assert t(None, 512, None, 0, None, None, None, None, 512, 512, 7, 1, 1, None, 7, None) == 0         # nothing to do
    assert t(None, 512, None, 4, None, None, None, None, 512, 512, 7, 1, 1, None, 7, None) == -1        # NULL pointers
    assert t(None, 512, None, 4, None, None, None, None, 512, 4096, 7, 0, 0, None, 7, None) == -1       # z of the tile beyond 160 KiB of LDS
    tl = L.fitgnn_gcn_graph_query_tail_lds_bytes
    # z [16 x (H2 + 4)] + the W1 stage [256 x 36] + the G stage [16 x 36] + the pooled row [H2] + the logits [C]
    assert tl(512, 47) == (16 * 516 + 256 * 36 + 16 * 36 + 512 + 47) * 4
    assert tl(512, 48) <= 160 * 1024 and tl(0, 7) == 0 and tl(4096, 7) > 160 * 1024
