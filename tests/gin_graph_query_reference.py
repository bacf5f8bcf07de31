"""float64 references of the two GIN graph-query kernels (csrc/query.hip: gin_graph_query_hops_kernel, gin_graph_query_tail_kernel) in
the kernels' stated operation order, a float64 model forward composed from the oracle, and the input generators the CPU and GPU tests
share (test infrastructure only).  Built from tests/gin_query_reference.py (one_plus, the product chain, the oracle stack) and
tests/graph_query_reference.py (the pool, the head, the softmax, the hand-made views).

o0 = 1.0f + eps0, o1 = 1.0f + eps1: formed ONCE, in float32.
hops     phase 1, every row r of a queried graph's range [r0, r1): a = 0; a = val[e'] * T[t(col[e'])][c] + a over row r's entries in CSR
         order; a = o0 * T[t(r)][c] + a; a = a + b0a[c] (b0a None: this add is absent); a_r = max(a, 0);
         h_r[n] = max((sum over k ascending of a_r[k] * W0b[n][k], from 0) + b0b[n], 0) (b0b None: the add is of 0.0, no rounding):
         gin_query_reference.hops's "row r" and "product".
         phase 2, every pooled row: s = 0; s = val[e] * h_{col[e]}[c] + s over the row's entries in CSR order, ONE chain; then
         s = o1 * h_r[c] + s.
tail     z1[n] = max(sum_k ascending G[r][k] W1a[n][k] (+ b1a[n]), 0); z2[m] = max(sum_n ascending z1[n] W1b[m][n] (+ b1b[m]), 0) per row
         of a segment (gin_query_reference.tail's two stages); the pool, the head and the softmax of graph_query_reference.pooled_tail.

`watch` and f32_div as in those modules.
"""
import numpy as np

import gin_query_reference as gq
import graph_query_reference as gr
from query_reference import _see

_small = gq._small


def layer0(rowptr, col, val, T, eps0, W0b, b0b, rows, xrow=None, b0a=None, watch=None):
    """(h [len(rows), Hb], its bound in units of 2^-24) for the view rows `rows`, composed as gin_query_reference.hops composes them:
    E_a = (d + 1 + [b0a]) S_a with S_a = sum |val T| + |o0 root| + |b0a|; E_h = |W0b| E_a + (Ha + [b0b]) S_h with
    S_h = sum_k |a_r[k] W0b[n][k]| + |b0b[n]| (ReLU has slope <= 1)."""
    Ha = T.shape[1]
    o0 = gq.one_plus(eps0)
    tr = (lambda c: int(c)) if xrow is None else (lambda c: int(xrow[c]))
    A, EA = np.zeros((len(rows), Ha)), np.zeros((len(rows), Ha))
    for n, r in enumerate(rows):
        a, S = np.zeros(Ha), np.zeros(Ha)
        for e in range(rowptr[r], rowptr[r + 1]):
            term = val[e] * T[tr(col[e])]
            a = _see(watch, "a", term + a)
            S += np.abs(term)
        term = o0 * T[tr(r)]
        a = _see(watch, "a", term + a)
        S += np.abs(term)
        if b0a is not None:
            a = _see(watch, "a", a + b0a)
            S += np.abs(b0a)
        A[n] = np.maximum(a, 0)
        EA[n] = (rowptr[r + 1] - rowptr[r] + 1 + (b0a is not None)) * S
    acc, S = gq._chain(A, W0b, b0b, watch, "h")
    return np.maximum(acc, 0), EA @ np.abs(W0b).T + (Ha + (b0b is not None)) * S


def hops(rowptr, col, val, T, eps0, W0b, b0b, eps1, seg, prow, pptr, xrow=None, b0a=None, watch=None, sums=False):
    """G [P, Hb] float64.  sums=True: also B [P, Hb], the first-order error bound of every entry in units of 2^-24: a pooled row of
    degree d carries sum_e |val_e| E_h(col[e]) + |o1| E_h(r) + (d + 1) (sum_e |val_e h_{col[e]}| + |o1 h_r|), one chain of d + 1 fmaf."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    val, T, W = np.asarray(val, dtype=np.float64), np.asarray(T, dtype=np.float64), np.asarray(W0b, dtype=np.float64)
    seg, prow, pptr = (np.asarray(a, dtype=np.int64) for a in (seg, prow, pptr))
    assert W.shape[1] == T.shape[1]
    ba = None if b0a is None else np.asarray(b0a, dtype=np.float64)
    bb = None if b0b is None else np.asarray(b0b, dtype=np.float64)
    o1 = gq.one_plus(eps1)
    need = sorted({r for r0, r1 in seg for r in range(r0, r1)})
    Hm, EH = layer0(rowptr, col, val, T, eps0, W, bb, need, xrow, ba, watch)
    at = {r: n for n, r in enumerate(need)}
    Hb = W.shape[0]
    G, B = np.zeros((len(prow), Hb)), np.zeros((len(prow), Hb))
    for i, (r0, r1) in enumerate(seg):
        for j in range(pptr[i], pptr[i + 1]):
            r = int(prow[j])
            assert r0 <= r < r1, "a pooled row outside its graph's range"
            s, absum, inerr = np.zeros(Hb), np.zeros(Hb), np.zeros(Hb)
            for e in range(rowptr[r], rowptr[r + 1]):
                assert r0 <= col[e] < r1, "a column outside the graph's range: the view is not block-diagonal"
                n = at[int(col[e])]
                s = _see(watch, "s", val[e] * Hm[n] + s)
                absum += np.abs(val[e] * Hm[n])
                inerr += np.abs(val[e]) * EH[n]
            s = _see(watch, "s", o1 * Hm[at[r]] + s)
            absum += np.abs(o1 * Hm[at[r]])
            inerr += np.abs(o1) * EH[at[r]]
            G[j], B[j] = s, inerr + (rowptr[r + 1] - rowptr[r] + 1) * absum
    return (G, B) if sums else G


def layer1(G, W1a, b1a, W1b, b1b, watch=None):
    """(z2 [P, H2b], its bound in units of 2^-24): gin_query_reference.tail's two stages, E_1 = (K + [b1a]) S_1,
    E_2 = |W1b| E_1 + (H2a + [b1b]) S_2."""
    G, W1a, W1b = (np.asarray(a, dtype=np.float64) for a in (G, W1a, W1b))
    f = lambda b: None if b is None else np.asarray(b, dtype=np.float64)   # noqa: E731
    b1a, b1b = f(b1a), f(b1b)
    K, H2a = G.shape[1], W1a.shape[0]
    assert W1a.shape[1] == K and W1b.shape[1] == H2a
    acc, S1 = gq._chain(G, W1a, b1a, watch, "z1")
    z1 = np.maximum(acc, 0)
    acc, S2 = gq._chain(z1, W1b, b1b, watch, "z2")
    return np.maximum(acc, 0), ((K + (b1a is not None)) * S1) @ np.abs(W1b).T + (H2a + (b1b is not None)) * S2


def pooled_tail(G, pptr, W1a, b1a, W1b, b1b, Wl, bl, pool="max", softmax=False, watch=None, sums=False, f32_div=False):
    """out [Q, C] float64.  sums=True: also B [Q, C], the bound of the LOGITS in units of 2^-24.  The pool, the head, the softmax and
    their bounds are graph_query_reference.pooled_tail's own code, run with this module's two ReLU stages in the place of its one ELU
    layer (z2 and its bound go in where its layer1 is called; the substitution lasts for the call).  This is a workaround: it
    sets another test module's global for the duration of the call and relies on that pooled_tail calling layer1 once, by its global
    name, and reading W1 and b1 nowhere else.  An optional (z, zerr) argument there would be the clean way; that module is an existing
    test file which this change leaves as it is, and copying its pool and head here would let the two drift apart.  With softmax the
    result's bound is graph_query_reference.softmax_bound(logits, B)."""
    z = layer1(G, W1a, b1a, W1b, b1b, watch)
    saved = gr.layer1
    gr.layer1 = lambda *a, **k: z
    try:
        return gr.pooled_tail(G, pptr, None, None, Wl, bl, pool=pool, softmax=softmax, watch=watch, sums=sums, f32_div=f32_div)
    finally:
        gr.layer1 = saved


softmax_bound = gr.softmax_bound


def model_forward(gorc, sd, x, edge_index, seg, prow, pptr, pool, softmax):
    """The float64 model: gin_query_reference.oracle_forward's stack on the whole view (its node head switched off by an identity
    lt1), then per queried graph the pool over its pooled rows, the head and the softmax (network.py's Classify_graph_* / Regress_graph_*
    in eval mode).  sd: the model's state dict (torch tensors)."""
    import torch
    H2b = sd["lt1.weight"].shape[1]
    stack = dict(sd)
    stack["lt1.weight"], stack["lt1.bias"] = torch.eye(H2b, dtype=torch.float64), torch.zeros(H2b, dtype=torch.float64)
    z = gq.oracle_forward(gorc, stack, x, edge_index, log_softmax=False).numpy()
    Wl, bl = sd["lt1.weight"].double().numpy(), sd["lt1.bias"].double().numpy()
    out = []
    for i in range(len(seg)):
        rows = np.asarray(prow[pptr[i]:pptr[i + 1]], dtype=np.int64)
        p = z[rows].max(0) if pool == "max" else z[rows].mean(0)
        y = p @ Wl.T + bl
        if softmax:
            y = np.exp(y - y.max())
            y = y / y.sum()
        out.append(y)
    return np.stack(out)


# ---- inputs of the kernel tests ----
HOPS_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 33]     # waves without a row; one row short of a tile, exactly one, one row into a second; three tiles
HOPS_ROW_DEGS = [0, 1, 2, 5, 63, 64, 65]         # 65: a second 64-entry batch
HOPS_GRAPHS = [8, 0, 3, 1, 5, 8, 4, 2, 6, 7]     # unsorted, one graph twice
HOPS_KINDS = ["all", "all", "first", "subset", "all", "subset", "none", "all", "subset", "all"]
# (Ha, Hb, with_xrow, with_bias, eps0, eps1): gin_query_reference.EXACT_HOPS_CASES -- (4, 16) one k-step, one column block; (40, 16) an
# 8-wide last k-stage; (256, 256) one full slab; (260, 272) a second slab of one block and a second slot with one live lane;
# (512, 512) two slots, two slabs; (272, 48) / (64, 272) two slots with one slab / one slot with two slabs
EXACT_HOPS_CASES = gq.EXACT_HOPS_CASES


def hops_case(Ha, Hb, with_xrow, with_bias, eps0, eps1, exact=True):
    """The graphs of HOPS_SIZES, every row degree of HOPS_ROW_DEGS, queried unsorted with one graph twice, pooled rows of every kind.
    EXACT draws are gin_query_reference.exact_hops_case's: T in {-8..8}/8, CSR values in {1/4, 1/2, 1}, 1 + eps = 1.5 or 0.75, biases in
    {-8..8}/8, W0b in {-2..2}/4: a_r is a multiple of 1/32, h_r of 1/128, s_r of 1/512 (tests/test_gin_graph_query_reference_cpu.py
    proves every intermediate exact in fp32 for these draws)."""
    rng = np.random.default_rng([Ha, Hb, int(with_xrow), int(with_bias), int(exact), 37])
    n_table = 41
    rowptr, col, val, xrow, gptr = gr.graph_view(rng, HOPS_SIZES, HOPS_ROW_DEGS, n_table, with_xrow, pow2_val=exact)
    n_t = n_table if with_xrow else int(gptr[-1])
    if exact:
        T, W0b = _small(rng, (n_t, Ha), -8, 8, 8), _small(rng, (Hb, Ha), -2, 2, 4)
        b0a = _small(rng, Ha, -8, 8, 8) if with_bias else None
        b0b = _small(rng, Hb, -8, 8, 8) if with_bias else None
    else:
        T, W0b = rng.normal(0, 1, size=(n_t, Ha)).astype(np.float32), (rng.normal(0, 1, size=(Hb, Ha)) / np.sqrt(Ha)).astype(np.float32)
        b0a = rng.normal(0, 1, size=Ha).astype(np.float32) if with_bias else None
        b0b = rng.normal(0, 1, size=Hb).astype(np.float32) if with_bias else None
    seg, prow, pptr = gr.pooled_rows(rng, gptr, HOPS_GRAPHS, HOPS_KINDS)
    return dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=T, b0a=b0a, eps0=np.float32(eps0), W0b=W0b, b0b=b0b, eps1=np.float32(eps1),
                seg=seg, prow=prow, pptr=pptr, gptr=gptr, max_rows=int((seg[:, 1] - seg[:, 0]).max()))


def window_case(Ha, Hb, n_rows):
    """EXACT inputs: a graph of 3 rows, one of n_rows rows (small degrees: the reference walks every entry) and another of 2, every
    row pooled, queried large, small, small."""
    rng = np.random.default_rng([Ha, Hb, n_rows, 41])
    rowptr, col, val, xrow, gptr = gr.graph_view(rng, [3, n_rows, 2], [[1, 2], [0, 1, 2, 3, 5], [2, 1]], 1, False, pow2_val=True)
    n = int(gptr[-1])
    seg, prow, pptr = gr.pooled_rows(rng, gptr, [0, 1, 2], ["all"])
    return dict(rowptr=rowptr, col=col, val=val, xrow=None, T=_small(rng, (n, Ha), -8, 8, 8), b0a=_small(rng, Ha, -8, 8, 8),
                eps0=np.float32(0.5), W0b=_small(rng, (Hb, Ha), -2, 2, 4), b0b=_small(rng, Hb, -8, 8, 8), eps1=np.float32(-0.25), seg=seg,
                prow=prow, pptr=pptr, gptr=gptr, max_rows=n_rows)


TAIL_SEGMENTS = gr.TAIL_SEGMENTS                  # 0, 1, 15, 16, 17, 33
TAIL_SEGMENTS_POW2 = gr.TAIL_SEGMENTS_POW2        # the mean's division is exact: the head behind it stays exact too
# (K, H2a, H2b, C, with_bias)
TAIL_CASES = [(16, 16, 16, 1, True), (64, 64, 64, 7, False), (272, 80, 48, 47, True), (512, 512, 512, 48, True)]


def tail_case(K, H2a, H2b, C, with_bias, pool, exact=True):
    """EXACT: gin_query_reference.exact_tail_case's draws (G in {-4..4}/4, W1a and W1b in {-2..2}/2, Wl in {-1, 0, 1}, biases in
    {-8..8}/8: z1 a multiple of 1/8, z2 of 1/16) over the segments of TAIL_SEGMENTS (max) or TAIL_SEGMENTS_POW2 (mean)."""
    lens = TAIL_SEGMENTS if (pool == "max" or not exact) else TAIL_SEGMENTS_POW2
    rng = np.random.default_rng([K, H2a, H2b, C, int(with_bias), int(pool == "max"), int(exact), 43])
    pptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    P = int(pptr[-1])
    if exact:
        b = lambda n: _small(rng, n, -8, 8, 8) if with_bias else None   # noqa: E731
        return dict(G=_small(rng, (P, K), -4, 4, 4), W1a=_small(rng, (H2a, K), -2, 2, 2), b1a=b(H2a), W1b=_small(rng, (H2b, H2a), -2, 2, 2),
                    b1b=b(H2b), Wl=_small(rng, (C, H2b), -1, 1, 1), bl=b(C), pptr=pptr)
    g = lambda n, k: (rng.normal(0, 1, size=(n, k)) / np.sqrt(k)).astype(np.float32)   # noqa: E731
    b = lambda n: rng.normal(0, 1, size=n).astype(np.float32) if with_bias else None    # noqa: E731
    return dict(G=rng.normal(0, 1, size=(P, K)).astype(np.float32), W1a=g(H2a, K), b1a=b(H2a), W1b=g(H2b, H2a), b1b=b(H2b), Wl=g(C, H2b), bl=b(C),
                pptr=pptr)


def dead_rows_case(pool):
    """Every live row has z1 = ReLU(-4 + 8) = 4 and z2 = 16 * 4 / 4 + 1 = 17, while a padded tile row, whose G is zero, has
    z1 = ReLU(b1a) = 8 and z2 = 16 * 8 / 4 + 1 = 33 (positive biases): a pool that reads dead rows returns 33 (max) or a shifted mean.
    Segments of 1, 15, 17 and 2 rows (all but 16 leave dead rows in a tile); under the mean power-of-two counts keep the case exact."""
    K, H2a, H2b, C = 4, 16, 16, 3
    lens = [1, 15, 17, 2] if pool == "max" else [1, 2, 4, 1]
    pptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    G = np.ones((int(pptr[-1]), K), dtype=np.float32)
    W1a, b1a = np.full((H2a, K), -1.0, dtype=np.float32), np.full(H2a, 8.0, dtype=np.float32)      # live z1 = 4, dead z1 = 8
    W1b, b1b = np.full((H2b, H2a), 0.25, dtype=np.float32), np.full(H2b, 1.0, dtype=np.float32)    # live z2 = 17, dead z2 = 33
    Wl = (np.arange(C * H2b).reshape(C, H2b) % 5 - 2).astype(np.float32) / 2
    bl = np.array([0.5, -0.25, 1.0], dtype=np.float32)
    return dict(G=G, W1a=W1a, b1a=b1a, W1b=W1b, b1b=b1b, Wl=Wl, bl=bl, pptr=pptr)


def neighbour_case(pool):
    """Segments of 15 and 1 rows (2 and 1 under the mean) with entries in {0..4}/4 and non-negative weights, each followed by a
    segment whose rows are 1024 times larger: a tile that reads past its segment's end pools a neighbour's rows."""
    K, H2a, H2b, C = 8, 16, 16, 2
    lens = [15, 16, 1, 16] if pool == "max" else [2, 16, 1, 16]
    rng = np.random.default_rng([int(pool == "max"), 47])
    pptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    P = int(pptr[-1])
    G = _small(rng, (P, K), 0, 4, 4)
    for i in (1, 3):
        G[pptr[i]:pptr[i + 1]] *= 1024.0
    return dict(G=G, W1a=_small(rng, (H2a, K), 0, 2, 2), b1a=None, W1b=_small(rng, (H2b, H2a), 0, 2, 2), b1b=None,
                Wl=_small(rng, (C, H2b), -1, 1, 1), bl=_small(rng, C, -8, 8, 8), pptr=pptr)


# (Ha, Hb, H2a, H2b, C): hops -> tail
CHAIN_CASES = [(64, 48, 64, 32, 7), (260, 272, 80, 48, 47)]


def chain_case(Ha, Hb, H2a, H2b, C, pool):
    """Hops inputs whose s_r stays small enough for the tail's chains to be exact as well (gin_query_reference.exact_chain_case's
    draws): degrees up to 2, CSR values in {1/2, 1}, T in {-4..4}/8, the weights in {-1, 0, 1} with three entries in four zero, biases in
    {-8..8}/8.  Graphs of 1, 2, 4, 16, 17 and 33 rows; max: all six, unsorted, pooled rows of every kind; mean: the graphs of 1, 2, 4
    and 16 rows (one twice) with every row pooled, so that the division is by a power of two and stays exact."""
    rng = np.random.default_rng([Ha, Hb, H2a, H2b, C, int(pool == "max"), 53])
    sizes = [1, 2, 4, 16, 17, 33]
    rowptr, col, val, xrow, gptr = gr.graph_view(rng, sizes, [0, 1, 2], 23, True, pow2_val=True)
    val = np.maximum(val, np.float32(0.5))
    w = lambda *s: _small(rng, s, -1, 1, 1, p_zero=0.75)   # noqa: E731
    b = lambda n: _small(rng, n, -8, 8, 8)                  # noqa: E731
    graphs, kinds = ([5, 0, 3, 1, 4, 2], ["all", "all", "first", "all", "subset", "all"]) if pool == "max" else ([3, 0, 1, 2, 3], ["all"])
    seg, prow, pptr = gr.pooled_rows(rng, gptr, graphs, kinds)
    return dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=_small(rng, (23, Ha), -4, 4, 8), b0a=b(Ha), eps0=np.float32(0.5),
                W0b=w(Hb, Ha), b0b=b(Hb), eps1=np.float32(-0.25), seg=seg, prow=prow, pptr=pptr, gptr=gptr,
                max_rows=int((seg[:, 1] - seg[:, 0]).max()), W1a=w(H2a, Hb), b1a=b(H2a), W1b=w(H2b, H2a), b1b=b(H2b), Wl=w(C, H2b), bl=b(C))
