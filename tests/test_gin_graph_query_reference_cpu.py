"""CPU tier of the GIN graph-query path (fitgnn_amd/serve.py GraphQueryEngine gin_kernels, csrc/query.hip gin_graph_query_hops_kernel
and gin_graph_query_tail_kernel): the float64 reference of tests/gin_graph_query_reference.py against a model forward composed from
the oracle's GIN stack, the exactness of the EXACT inputs the GPU test sends through the kernels, a float32 NumPy replay of the stated
operation order, and the launchers' argument refusals -- all before any launch."""
import numpy as np
import pytest
import torch

import gin_graph_query_reference as ggq
import gin_query_reference as gq
import graph_query_reference as gr
from oracle import gnn_oracle as gorc
from test_query_reference_cpu import _exactness_watch

f32 = np.float32


def _hops64(c, **kw):
    return ggq.hops(c["rowptr"], c["col"], c["val"], c["T"], c["eps0"], c["W0b"], c["b0b"], c["eps1"], c["seg"], c["prow"], c["pptr"],
                    xrow=c["xrow"], b0a=c["b0a"], **kw)


def _tail64(G, c, pool, **kw):
    return ggq.pooled_tail(G, c["pptr"], c["W1a"], c["b1a"], c["W1b"], c["b1b"], c["Wl"], c["bl"], pool=pool, **kw)


@pytest.mark.parametrize("pool,softmax", [("max", True), ("mean", False)])
def test_reference_equals_the_oracle_forward(pool, softmax):
    """hops + pooled_tail on small graphs == the whole-view float64 forward (gin_aggregate, the MLP, ELU, twice), the per-graph pool,
    the head and the softmax, to 1e-12.  eps is non-zero in both layers; pooled rows: all of a graph, a subset, one."""
    rng = np.random.default_rng(59 + softmax)
    F, Ha, Hb, H2a, H2b, C = 6, 16, 32, 48, 16, 5
    sizes = [1, 4, 7, 17, 2]
    gptr = np.concatenate([[0], np.cumsum(sizes)])
    n = int(gptr[-1])
    src, dst = [], []
    for g, m in enumerate(sizes):          # repeated edges and self loops inside each graph; the graph of one row has a self loop or none
        k = 3 * m
        src += rng.integers(gptr[g], gptr[g + 1], size=k).tolist()
        dst += rng.integers(gptr[g], gptr[g + 1], size=k).tolist()
    ei = np.stack([src, dst]).astype(np.int64)
    g_ = lambda *s: rng.normal(0, 0.4, size=s)   # noqa: E731
    m = {"conv.0.nn.0.weight": g_(Ha, F), "conv.0.nn.0.bias": g_(Ha), "conv.0.nn.2.weight": g_(Hb, Ha), "conv.0.nn.2.bias": g_(Hb),
         "conv.1.nn.0.weight": g_(H2a, Hb), "conv.1.nn.0.bias": g_(H2a), "conv.1.nn.2.weight": g_(H2b, H2a), "conv.1.nn.2.bias": g_(H2b),
         "lt1.weight": g_(C, H2b), "lt1.bias": g_(C),
         "conv.0.eps": np.array([0.375], dtype=np.float32), "conv.1.eps": np.array([-0.625], dtype=np.float32)}   # 1 + eps exact in fp32
    X = rng.normal(size=(n, F))
    rowptr, col, val = gq.sum_csr(ei, n)
    seg, prow, pptr = gr.pooled_rows(rng, gptr, [3, 0, 2, 1, 3, 4], ["all", "all", "subset", "first", "subset", "first"])
    assert 1 in np.diff(pptr).tolist()
    T = X @ m["conv.0.nn.0.weight"].T
    G = ggq.hops(rowptr, col, val, T, m["conv.0.eps"][0], m["conv.0.nn.2.weight"], m["conv.0.nn.2.bias"], m["conv.1.eps"][0], seg, prow, pptr,
                 b0a=m["conv.0.nn.0.bias"])
    out = ggq.pooled_tail(G, pptr, m["conv.1.nn.0.weight"], m["conv.1.nn.0.bias"], m["conv.1.nn.2.weight"], m["conv.1.nn.2.bias"],
                          m["lt1.weight"], m["lt1.bias"], pool=pool, softmax=softmax)
    sd = {k: torch.from_numpy(v) for k, v in m.items()}
    ref = ggq.model_forward(gorc, sd, torch.from_numpy(X), torch.from_numpy(ei), seg, prow, pptr, pool, softmax)
    assert out.shape == ref.shape == (6, C) and np.abs(out - ref).max() <= 1e-12
    # the per-row reference forms the same s_r up to the order of its fold: the two hops agree to rounding
    Gn = gq.hops(rowptr, col, val, T, m["conv.0.eps"][0], m["conv.0.nn.2.weight"], m["conv.0.nn.2.bias"], m["conv.1.eps"][0], prow,
                 b0a=m["conv.0.nn.0.bias"])
    assert np.abs(G - Gn).max() <= 1e-12


# ---- the stated order once more, in float32 ----
def _chain32(A, W, b):
    acc = np.zeros((A.shape[0], W.shape[0]), dtype=f32)
    for k in range(A.shape[1]):
        acc = A[:, k:k + 1] * W[None, :, k] + acc
    return acc if b is None else acc + b[None, :]


def _hops32(c):
    rowptr, col, val, T, W, xrow = c["rowptr"], c["col"], c["val"].astype(f32), c["T"].astype(f32), c["W0b"].astype(f32), c["xrow"]
    t = (lambda r: r) if xrow is None else (lambda r: xrow[r])
    o0, o1 = f32(1.0) + f32(c["eps0"]), f32(1.0) + f32(c["eps1"])
    G = np.zeros((len(c["prow"]), W.shape[0]), dtype=f32)
    for i, (r0, r1) in enumerate(c["seg"]):
        A = np.zeros((r1 - r0, T.shape[1]), dtype=f32)
        for r in range(r0, r1):
            a = np.zeros(T.shape[1], dtype=f32)
            for e in range(rowptr[r], rowptr[r + 1]):
                a = val[e] * T[t(col[e])] + a
            a = o0 * T[t(r)] + a
            if c["b0a"] is not None:
                a = a + c["b0a"]
            A[r - r0] = np.maximum(a, f32(0))
        h = np.maximum(_chain32(A, W, c["b0b"]), f32(0))        # the window: every row of the graph, once
        for j in range(c["pptr"][i], c["pptr"][i + 1]):
            r = c["prow"][j]
            s = np.zeros(W.shape[0], dtype=f32)
            for e in range(rowptr[r], rowptr[r + 1]):
                s = val[e] * h[col[e] - r0] + s
            G[j] = o1 * h[r - r0] + s
    assert G.dtype == f32
    return G


def _tail32(G, c, pool):
    z1 = np.maximum(_chain32(G.astype(f32), c["W1a"], c["b1a"]), f32(0))
    z2 = np.maximum(_chain32(z1, c["W1b"], c["b1b"]), f32(0))
    Q, H2b = len(c["pptr"]) - 1, z2.shape[1]
    p = np.zeros((Q, H2b), dtype=f32)
    for i in range(Q):
        s0, s1 = c["pptr"][i], c["pptr"][i + 1]
        if s1 == s0:
            continue
        if pool == "max":
            m = z2[s0].copy()
            for r in range(s0 + 1, s1):
                m = np.maximum(m, z2[r])
            p[i] = m
        else:
            s = np.zeros(H2b, dtype=f32)
            for r in range(s0, s1):
                s = s + z2[r]
            p[i] = s / f32(s1 - s0)
    out = _chain32(p, c["Wl"], c["bl"])
    assert out.dtype == f32
    return out


@pytest.mark.parametrize("case", ggq.EXACT_HOPS_CASES, ids=str)
def test_exact_hops_inputs_are_exact(case):
    Ha, Hb, with_xrow, with_bias, eps0, eps1 = case
    c = ggq.hops_case(*case)
    watch, seen = _exactness_watch()
    G = _hops64(c, watch=watch)
    assert seen["n"] > 1000 and np.isfinite(G).all() and G.shape == (len(c["prow"]), Hb) and c["W0b"].shape == (Hb, Ha)
    assert gq.one_plus(eps0) == 1.0 + eps0 and gq.one_plus(eps1) == 1.0 + eps1 and eps0 in (0.5, -0.25) and eps1 in (0.5, -0.25)
    size = (c["seg"][:, 1] - c["seg"][:, 0]).tolist()
    assert sorted(set(size)) == ggq.HOPS_SIZES and len(size) > len(set(size))                 # every size, one graph twice
    deg = np.diff(c["rowptr"])
    assert set(deg.tolist()) == set(ggq.HOPS_ROW_DEGS) and set(deg[c["prow"]].tolist()) == set(ggq.HOPS_ROW_DEGS)
    cnt = np.diff(c["pptr"])
    assert (cnt == 0).any() and (cnt == 1).any() and (cnt == np.array(size)).any() and ((cnt > 1) & (cnt < np.array(size))).any()
    assert (G >= 0).all() and (G > 0).any()
    if c["xrow"] is not None:
        assert c["xrow"].max() == c["T"].shape[0] - 1 and len(set(c["xrow"].tolist())) < len(c["xrow"])
    assert np.array_equal(_hops32(c).astype(np.float64), G), "the float32 replay of the stated order differs from the float64 reference"
    # exact inputs remove the fold-order difference: the per-row reference gives the same values
    Gn = gq.hops(c["rowptr"], c["col"], c["val"], c["T"], c["eps0"], c["W0b"], c["b0b"], c["eps1"], c["prow"], xrow=c["xrow"], b0a=c["b0a"],
                 watch=watch)
    assert np.array_equal(Gn, G)


@pytest.mark.parametrize("Ha,Hb", [(64, 64), (512, 512)])
def test_exact_window_inputs_are_exact(Ha, Hb):
    from fitgnn_amd import ops
    n = ops.gin_graph_query_max_rows(Ha, Hb)        # the GPU test's graph: exactly the largest window
    assert n == {(64, 64): 450, (512, 512): 90}[(Ha, Hb)]
    c = ggq.window_case(Ha, Hb, n + 1)
    assert (c["seg"][:, 1] - c["seg"][:, 0]).tolist() == [3, n + 1, 2]
    c = ggq.window_case(Ha, Hb, n)
    watch, seen = _exactness_watch()
    G = _hops64(c, watch=watch)
    assert seen["n"] > 100 and np.array_equal(_hops32(c).astype(np.float64), G)


@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("case", ggq.TAIL_CASES, ids=str)
def test_exact_tail_inputs_are_exact(case, pool):
    K, H2a, H2b, C, with_bias = case
    c = ggq.tail_case(*case, pool)
    watch, seen = _exactness_watch()
    out = _tail64(c["G"], c, pool, watch=watch, f32_div=True)
    assert seen["n"] >= K + H2a + H2b and np.isfinite(out).all() and out.shape == (6, C)
    assert (out != 0).any()
    assert np.array_equal(out[0], np.zeros(C) if c["bl"] is None else c["bl"].astype(np.float64))   # an empty segment: p = 0
    assert np.array_equal(_tail32(c["G"], c, pool).astype(np.float64), out)


@pytest.mark.parametrize("pool", ["max", "mean"])
def test_dead_and_neighbour_cases_are_exact_and_tell(pool):
    c = ggq.dead_rows_case(pool)
    watch, _ = _exactness_watch()
    out = _tail64(c["G"], c, pool, watch=watch, f32_div=True)
    z2, _ = ggq.layer1(c["G"], c["W1a"], c["b1a"], c["W1b"], c["b1b"])
    dead, _ = ggq.layer1(np.zeros((1, 4)), c["W1a"], c["b1a"], c["W1b"], c["b1b"])
    assert (z2 == 17).all() and (dead == 33).all()          # a padded row's z2 is larger than every live row's
    assert np.array_equal(_tail32(c["G"], c, pool).astype(np.float64), out)
    c = ggq.neighbour_case(pool)
    out = _tail64(c["G"], c, pool, watch=watch, f32_div=True)
    z2, _ = ggq.layer1(c["G"], c["W1a"], c["b1a"], c["W1b"], c["b1b"])
    p = c["pptr"]
    assert z2[p[1]:p[2]].max() > 64 * z2[p[0]:p[1]].max() and z2[p[0]:p[1]].max() > 0
    assert np.array_equal(_tail32(c["G"], c, pool).astype(np.float64), out)


@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("case", ggq.CHAIN_CASES, ids=str)
def test_exact_chain_inputs_are_exact(case, pool):
    c = ggq.chain_case(*case, pool)
    watch, seen = _exactness_watch()
    G = _hops64(c, watch=watch)
    out = _tail64(G, c, pool, watch=watch, f32_div=True)
    assert out.shape == (len(c["seg"]), case[4]) and np.isfinite(out).all() and (G > 0).any() and len(np.unique(out)) > case[4]
    if pool == "mean":
        cnt = np.diff(c["pptr"])
        assert ((cnt & (cnt - 1)) == 0).all() and cnt.min() >= 1
    G32 = _hops32(c)
    assert np.array_equal(G32.astype(np.float64), G) and np.array_equal(_tail32(G32, c, pool).astype(np.float64), out)


def test_the_bound_covers_a_float32_run_of_the_same_order():
    """sums=True: the reference's bounds hold for the same operation order carried out in float32.  NumPy's float32 arithmetic rounds
    every product on its own, which the bounds' one-rounding-per-fmaf count does not cover: the CSR values and both 1 + eps are powers
    of two and the weights hold signed powers of two, so every product is exact and only the additions (and the mean's division) round."""
    rng = np.random.default_rng(61)
    pw = lambda *s: (rng.choice([-1.0, 1.0], size=s) * 2.0 ** rng.integers(-3, 1, size=s)).astype(f32)   # noqa: E731
    rowptr, col, val, xrow, gptr = gr.graph_view(rng, [1, 2, 5, 17, 33], [0, 1, 2, 7, 30], 19, True, pow2_val=True)
    Ha, Hb, H2a, H2b, C = 8, 16, 16, 32, 5
    seg, prow, pptr = gr.pooled_rows(rng, gptr, [4, 0, 2, 3, 1], ["all", "all", "subset", "first", "all"])
    c = dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=rng.normal(0, 1, size=(19, Ha)).astype(f32), b0a=rng.normal(0, 1, size=Ha).astype(f32),
             eps0=f32(1.0), W0b=pw(Hb, Ha), b0b=rng.normal(0, 1, size=Hb).astype(f32), eps1=f32(-0.5), seg=seg, prow=prow, pptr=pptr)
    ref, B = _hops64(c, sums=True)
    G32 = _hops32(c)
    err = np.abs(G32.astype(np.float64) - ref)
    assert (err <= 2.0 ** -24 * B).all() and err.max() > 0 and (B > 0).all()
    c.update(W1a=pw(H2a, Hb), b1a=rng.normal(0, 1, size=H2a).astype(f32), W1b=pw(H2b, H2a), b1b=rng.normal(0, 1, size=H2b).astype(f32),
             Wl=pw(C, H2b), bl=rng.normal(0, 1, size=C).astype(f32))
    for pool in ("max", "mean"):
        logits, Bt = _tail64(G32, c, pool, sums=True)          # the tail's bound takes G as its exact input
        err = np.abs(_tail32(G32, c, pool).astype(np.float64) - logits)
        assert (err <= 2.0 ** -24 * Bt).all() and err.max() > 0


def test_launchers_refuse_bad_arguments_without_touching_the_gpu():
    from fitgnn_amd import _lib, ops
    L = _lib.lib()
    h = L.fitgnn_gin_graph_query_hops_f32
    N = None

    def hops(Q=4, Ha=512, Hb=512, max_rows=16, ldt=512, ldg=512):
        #        rowptr col val T  ldt xrow b0a eps0 W0b b0b eps1 seg prow pptr Q  Ha  Hb  max_rows G  ldg stream
        return h(N, N, N, N, ldt, N, N, N, N, N, N, N, N, N, Q, Ha, Hb, max_rows, N, ldg, N)

    assert hops(Q=-1) == -1 and hops(max_rows=-1) == -1
    assert hops(Ha=510) == -1 and hops(Ha=0) == -1 and hops(Ha=516, ldt=516) == -1           # Ha % 4, Ha < 4, Ha > 512
    assert hops(Hb=504) == -1 and hops(Hb=0) == -1 and hops(Hb=528, ldg=528) == -1           # Hb % 16, Hb < 16, Hb > 512
    assert hops(ldt=508) == -1 and hops(ldg=508) == -1                                      # too small a stride
    assert hops(ldt=514) == -3 and hops(ldg=518) == -3                                      # strides not multiples of 4
    assert hops(Q=0) == 0                                                                   # nothing to do
    assert hops() == -1                                                                     # NULL pointers, refused not dereferenced
    assert hops(Ha=4, Hb=16, ldt=4, ldg=16) == -1
    a = 64    # an aligned fake address: every call below is refused before a launch
    assert h(a, a, a, a + 4, 512, N, N, a, a, N, a, a, a, a, 4, 512, 512, 16, a, 512, N) == -3       # T misaligned, nothing launched
    assert h(a, a, a, a, 512, N, N, a, a + 4, N, a, a, a, a, 4, 512, 512, 16, a, 512, N) == -3       # W0b
    assert h(a, a, a, a, 512, N, N, a, a, N, a, a, a, a, 4, 512, 512, 16, a + 4, 512, N) == -3       # G

    lds = L.fitgnn_gin_graph_query_hops_lds_bytes
    assert lds(0, 512, 512) == 4 * (16 * 516 + 256 * 36) and lds(90, 512, 512) == 4 * (16 * 516 + 256 * 36 + 90 * 260) <= 160 * 1024
    assert lds(91, 512, 512) > 160 * 1024 and lds(450, 64, 64) == 4 * (16 * 68 + 256 * 36 + 450 * 68) <= 160 * 1024 < lds(451, 64, 64)
    assert lds(7, 260, 272) == 4 * (16 * 264 + 256 * 36 + 7 * 260) and lds(7, 4, 16) == 4 * (16 * 8 + 256 * 36 + 7 * 20)
    assert lds(-1, 64, 64) == 0 and lds(4, 0, 64) == 0 and lds(4, 64, 0) == 0
    assert ops.gin_graph_query_max_rows(512, 512) == 90 and ops.gin_graph_query_max_rows(64, 64) == 450
    assert ops.gin_graph_query_max_rows(0, 64) == 0
    assert hops(max_rows=91) == -1 and hops(Q=0, max_rows=91) == -1 and hops(Ha=64, Hb=64, ldt=64, ldg=64, max_rows=451) == -1   # beyond 160 KiB

    t = L.fitgnn_gin_graph_query_tail_f32

    def tail(Q=4, K=512, H2a=512, H2b=512, C=7, ldg=512, ldo=7, pool=0):
        #        G  ldg pptr Q  W1a b1a W1b b1b Wl bl K  H2a  H2b  C  pool softmax out ldo stream
        return t(N, ldg, N, Q, N, N, N, N, N, N, K, H2a, H2b, C, pool, 1, N, ldo, N)

    assert tail(Q=-1) == -1 and tail(K=510) == -1 and tail(K=0) == -1
    assert tail(H2a=520) == -1 and tail(H2a=0) == -1 and tail(H2b=520) == -1 and tail(H2b=0) == -1 and tail(C=0) == -1
    assert tail(ldg=508) == -1 and tail(ldo=6) == -1 and tail(pool=2) == -1 and tail(pool=-1) == -1
    assert tail(ldg=514) == -3
    assert tail(Q=0) == 0 and tail() == -1
    assert t(a + 4, 512, a, 4, a, N, a, N, a, N, 512, 512, 512, 7, 0, 1, a, 7, N) == -3               # G misaligned
    assert t(a, 512, a, 4, a, N, a, N, a, N, 512, 512, 512, 7, 0, 1, a + 4, 7, N) == -3               # out
    tl = L.fitgnn_gin_graph_query_tail_lds_bytes
    assert tl(512, 512, 48) == L.fitgnn_gin_query_tail_lds_bytes(512, 512, 48) + 4 * (512 + 48) <= 160 * 1024
    assert tl(0, 16, 1) == 0 and tl(16, 0, 1) == 0 and tl(16, 16, 0) == 0
    assert tl(1024, 1024, 7) > 160 * 1024 and tail(H2a=1024, H2b=1024) == -1 and tail(Q=0, H2a=1024, H2b=1024) == -1   # does not fit LDS
    assert tl(16, 16, 2400) > 160 * 1024 and tail(H2a=16, H2b=16, C=2400, ldo=2400) == -1
