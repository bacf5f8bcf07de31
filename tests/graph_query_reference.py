"""float64 references of the two graph-query kernels (csrc/query.hip: graph_query_hops_kernel, graph_query_tail_kernel) in the kernels'
stated operation order, a dense float64 two-layer forward + pool + head, and the input generators the CPU and GPU tests share (test
infrastructure only; the conventions of tests/query_reference.py).

hops     phase 1, every row r of a queried graph's range [r0, r1): a = 0; a = val[e'] * T[t(col[e'])][c] + a over row r's entries in
         CSR order; h_r = ELU(a + b0[c]).  phase 2, every pooled row: g = 0; g = val[e] * h_{col[e]}[c] + g over the row's entries in
         CSR order, one chain.
tail     z_r[n] = ELU(sum_k ascending G[r][k] W1[n][k] (+ b1[n])) per row of a segment; the pool over the segment's rows ascending:
         max p = z_first, p = max(p, z_r); mean s = s + z_r from 0, p = s / cnt (one rounding); an empty segment: p = 0;
         logit[c] = sum_h ascending p[h] Wl[c][h] (+ bl[c]); softmax: m = max, e_c = exp(logit[c] - m), s = sum_c e_c ascending,
         out[c] = e_c / s.

`watch` and f32_elu as in query_reference.  f32_div rounds the mean's division to float32 (what the exact cases compare against:
the fp32 division of two exactly represented operands is the correctly rounded quotient, and float64 -> float32 rounding of a
quotient of two float32 numbers is innocuous).
"""
import numpy as np

import query_reference as qr
from query_reference import _see, elu

TINY = 2.0 ** -125   # 2^-149 (the spacing of fp32 below 2^-126) in units of 2^-24: what one rounding costs once a result underflows


def hops(rowptr, col, val, T, seg, prow, pptr, xrow=None, b0=None, watch=None, sums=False, f32_elu=False):
    """G [P, H] float64.  sums=True: also B [P, H], the first-order error bound of every entry in units of 2^-24: layer-0 row r of
    degree d_r with S_r = sum |val T| + |b0| carries E_r = (d_r + 1) S_r (the fmaf chain and the bias add) + 2 |h_r| where the
    pre-activation is <= 0 (expm1f within 1 ulp; ELU has slope <= 1); a pooled row of degree d: sum_e |val_e| E_{col[e]} +
    d sum_e |val_e h_{col[e]}| (one chain of d fmaf)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    val, T = np.asarray(val, dtype=np.float64), np.asarray(T, dtype=np.float64)
    seg, prow, pptr = (np.asarray(a, dtype=np.int64) for a in (seg, prow, pptr))
    H = T.shape[1]
    bias = np.zeros(H) if b0 is None else np.asarray(b0, dtype=np.float64)
    tr = (lambda c: c) if xrow is None else (lambda c: int(xrow[c]))
    G, B = np.zeros((len(prow), H)), np.zeros((len(prow), H))
    hcache, gcache = {}, {}
    for i, (r0, r1) in enumerate(seg):
        for r in range(r0, r1):
            if r in hcache:
                continue
            a, S = np.zeros(H), np.abs(bias).copy()
            for e in range(rowptr[r], rowptr[r + 1]):
                term = val[e] * T[tr(col[e])]
                a = _see(watch, "a", term + a)
                S += np.abs(term)
            pre = _see(watch, "pre", a + bias)
            h = _see(watch, "h", elu(pre, f32_elu))
            hcache[r] = (h, (rowptr[r + 1] - rowptr[r] + 1) * S + 2 * np.abs(h) * (pre <= 0))
        for j in range(pptr[i], pptr[i + 1]):
            r = int(prow[j])
            assert r0 <= r < r1, "a pooled row outside its graph's range"
            if r not in gcache:
                g, absum, inerr = np.zeros(H), np.zeros(H), np.zeros(H)
                for e in range(rowptr[r], rowptr[r + 1]):
                    assert r0 <= col[e] < r1, "a column outside the graph's range: the view is not block-diagonal"
                    h, herr = hcache[int(col[e])]
                    g = _see(watch, "g", val[e] * h + g)
                    absum += np.abs(val[e] * h)
                    inerr += np.abs(val[e]) * herr
                gcache[r] = (g, inerr + (rowptr[r + 1] - rowptr[r]) * absum)
            G[j], B[j] = gcache[r]
    return (G, B) if sums else G


def layer1(G, W1, b1, watch=None, f32_elu=False):
    """(z [P, H2], its bound in units of 2^-24): query_reference.tail's first half -- (H + 1) (sum_k |G W1| + |b1|) + 2 |z| where the
    pre-activation is <= 0."""
    G, W1 = np.asarray(G, dtype=np.float64), np.asarray(W1, dtype=np.float64)
    P, H = G.shape
    acc, S = np.zeros((P, W1.shape[0])), np.zeros((P, W1.shape[0]))
    for k in range(H):
        term = G[:, k:k + 1] * W1[None, :, k]
        acc = _see(watch, "acc", term + acc)
        S += np.abs(term)
    if b1 is not None:
        acc = _see(watch, "acc", acc + np.asarray(b1, dtype=np.float64)[None, :])
        S += np.abs(np.asarray(b1, dtype=np.float64))[None, :]
    _see(watch, "pre", acc)
    z = _see(watch, "z", elu(acc, f32_elu))
    return z, (H + 1) * S + 2 * np.abs(z) * (acc <= 0)


def pooled_tail(G, pptr, W1, b1, Wl, bl, pool="max", softmax=False, watch=None, sums=False, f32_elu=False, f32_div=False):
    """out [Q, C] float64.  sums=True: also B [Q, C], the first-order error bound of the LOGITS in units of 2^-24.  The pooled row:
    max -- the largest bound among the segment's rows (fmaxf is exact; the winner may be any row within its bound of the largest);
    mean -- (sum_r E_r + cnt sum_r |z_r|) / cnt for the cnt additions, + |p| for the division.  The head: sum_h |Wl[c][h]| E_p[h] +
    (H2 + 1) (sum_h |p Wl| + |bl|).  With softmax the result's bound is softmax_bound(logits, B)."""
    pptr = np.asarray(pptr, dtype=np.int64)
    Wl = np.asarray(Wl, dtype=np.float64)
    H2, C, Q = Wl.shape[1], Wl.shape[0], len(pptr) - 1
    z, zerr = layer1(G, W1, b1, watch, f32_elu)
    p, perr = np.zeros((Q, H2)), np.zeros((Q, H2))
    for i in range(Q):
        s0, s1 = pptr[i], pptr[i + 1]
        if s1 == s0:
            continue
        if pool == "max":
            m = z[s0].copy()
            for r in range(s0 + 1, s1):
                m = np.maximum(m, z[r])
            p[i], perr[i] = m, zerr[s0:s1].max(0)
        else:
            s = np.zeros(H2)
            for r in range(s0, s1):
                s = _see(watch, "s", s + z[r])
            cnt = float(s1 - s0)
            q = s / cnt
            p[i] = q.astype(np.float32).astype(np.float64) if f32_div else q
            perr[i] = (zerr[s0:s1].sum(0) + cnt * np.abs(z[s0:s1]).sum(0)) / cnt + np.abs(p[i])
        _see(watch, "p", p[i])
    lg, Lsum = np.zeros((Q, C)), np.zeros((Q, C))
    for h in range(H2):
        term = p[:, h:h + 1] * Wl[None, :, h]
        lg = _see(watch, "logit", term + lg)
        Lsum += np.abs(term)
    if bl is not None:
        lg = _see(watch, "logit", lg + np.asarray(bl, dtype=np.float64)[None, :])
        Lsum += np.abs(np.asarray(bl, dtype=np.float64))[None, :]
    B = perr @ np.abs(Wl).T + (H2 + 1) * Lsum
    out = lg
    if softmax:
        t = lg - lg.max(1, keepdims=True)
        s = np.zeros((Q, 1))
        for c in range(C):
            s = s + np.exp(t[:, c:c + 1])
        out = np.exp(t) / s
    return (out, B) if sums else out


def softmax_bound(logits, B):
    """First-order bound (in units of 2^-24) on the error of the kernel's softmax given per-logit bounds B.  d sm_c / d x_j =
    sm_c ([c == j] - sm_j), whose absolute values sum to 2 sm_c (1 - sm_c): the logits' errors reach out_c at most as 2 max B,
    relative.  t = x - m rounds once (|t_c|, relative in e_c) and expf is within 1 ulp (2); s carries the sm-weighted mean of the
    same two plus its C additions; the division rounds once.  All of that times sm_c.  A result below 2^-126 is a multiple of
    2^-149: TINY for expf's result and TINY for the quotient, absolute."""
    x = np.asarray(logits, dtype=np.float64)
    C = x.shape[1]
    t = x - x.max(1, keepdims=True)
    e = np.exp(t)
    sm = e / e.sum(1, keepdims=True)
    rel = 2 * B.max(1, keepdims=True) + (np.abs(t) + 2) + (sm * (np.abs(t) + 2)).sum(1, keepdims=True) + C + 1
    return sm * rel + 2 * TINY


def dense_graph_forward(x, rowptr, col, val, seg, prow, pptr, W0, b0, W1, b1, Wl, bl, pool, softmax):
    """Per queried graph, a plain dense float64 forward on the graph's own rows: A (X W0^T) + b0, ELU, A (h W1^T) + b1, ELU, the pool
    over the pooled rows, the head, the softmax (network.py:87-95, :158-166 in eval mode)."""
    out = []
    for i, (r0, r1) in enumerate(np.asarray(seg, dtype=np.int64)):
        n = r1 - r0
        A = np.zeros((n, n))
        for r in range(r0, r1):
            for e in range(rowptr[r], rowptr[r + 1]):
                A[r - r0, col[e] - r0] += val[e]
        h = elu(A @ (np.asarray(x[r0:r1], dtype=np.float64) @ W0.T) + b0)
        z = elu(A @ (h @ W1.T) + b1)
        rows = np.asarray(prow[pptr[i]:pptr[i + 1]], dtype=np.int64) - r0
        p = z[rows].max(0) if pool == "max" else z[rows].mean(0)
        y = p @ Wl.T + bl
        if softmax:
            y = np.exp(y - y.max())
            y = y / y.sum()
        out.append(y)
    return np.stack(out)


# ---- inputs of the kernel tests ----
HOPS_ROW_DEGS = [0, 1, 63, 64, 65, 2, 5]


def graph_view(rng, sizes, degs, n_table, with_xrow, pow2_val):
    """A hand-made block-diagonal view: graph g has sizes[g] rows; row k of the view has degs[g][k % len] entries (degs: one list for
    all graphs or one per graph) whose columns fall anywhere inside the row's own graph, repeats allowed.  With xrow: an indirection
    with repeated table rows, one row at the last table row.  pow2_val: values from {1/4, 1/2, 1}, else uniform.
    Returns rowptr, col, val, xrow, gptr (the graphs' row pointer)."""
    per_graph = isinstance(degs[0], (list, tuple))
    gptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rowptr, col = [0], []
    for g, n in enumerate(sizes):
        dg = degs[g] if per_graph else degs
        for k in range(n):
            d = dg[(k + g) % len(dg)]
            col += rng.integers(gptr[g], gptr[g + 1], size=d).tolist()
            rowptr.append(len(col))
    col = np.array(col, dtype=np.int32)
    val = (rng.choice([0.25, 0.5, 1.0], size=len(col)) if pow2_val else rng.uniform(0.05, 1.0, size=len(col))).astype(np.float32)
    n_rows = int(gptr[-1])
    xrow = None
    if with_xrow:
        xrow = rng.integers(0, n_table, size=n_rows).astype(np.int32)
        xrow[n_rows // 2:] = xrow[: n_rows - n_rows // 2]     # repeated table rows
        if len(col):
            xrow[col[0]] = n_table - 1                         # one entry at the last table row
    return np.array(rowptr, dtype=np.int32), col, val, xrow, gptr


def pooled_rows(rng, gptr, graphs, kinds):
    """seg [Q, 2], prow, pptr for the queried `graphs`; kinds[i % len]: "all", "first" (the first ceil(n / 2) rows), "subset" (every
    other row from the second, descending: non-contiguous and unsorted) or "none"."""
    seg, prow, pptr = [], [], [0]
    for i, g in enumerate(graphs):
        r0, r1 = int(gptr[g]), int(gptr[g + 1])
        kind = kinds[i % len(kinds)]
        rows = {"all": list(range(r0, r1)), "first": list(range(r0, r0 + (r1 - r0 + 1) // 2)),
                "subset": list(range(r0 + 1, r1, 2))[::-1], "none": []}[kind]
        seg.append((r0, r1))
        prow += rows
        pptr.append(len(prow))
    return np.array(seg, dtype=np.int64).reshape(-1, 2), np.array(prow, dtype=np.int64), np.array(pptr, dtype=np.int64)


HOPS_SIZES = [1, 2, 3, 4, 5, 17]                 # waves with none, one or two rows; more rows than one round of the waves
# (H, with_xrow, with_b0)
EXACT_HOPS_CASES = [(4, False, True), (64, True, False), (256, False, False), (260, True, True), (512, False, True)]


def hops_case(H, with_xrow, with_b0, exact=True, tag=7):
    """The graphs of HOPS_SIZES, each row degree of HOPS_ROW_DEGS, queried unsorted with one graph twice; pooled rows of every kind."""
    rng = np.random.default_rng([H, int(with_xrow), int(with_b0), int(exact), tag])
    n_table = 37
    rowptr, col, val, xrow, gptr = graph_view(rng, HOPS_SIZES, HOPS_ROW_DEGS, n_table, with_xrow, pow2_val=exact)
    n_t = n_table if with_xrow else int(gptr[-1])
    if exact:
        T, b0 = qr.exact_gather_inputs(rng, H, n_t, with_b0)
    else:
        T = rng.normal(0, 1, size=(n_t, H)).astype(np.float32)
        b0 = rng.normal(0, 1, size=H).astype(np.float32) if with_b0 else None
    graphs = [5, 0, 3, 1, 5, 4, 2]
    seg, prow, pptr = pooled_rows(rng, gptr, graphs, ["all", "all", "first", "subset", "subset", "none", "all"])
    return dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=T, b0=b0, seg=seg, prow=prow, pptr=pptr, gptr=gptr,
                max_rows=int((seg[:, 1] - seg[:, 0]).max()))


def window_case(H, n_rows, exact=True):
    """One graph of n_rows rows (small degrees: the reference walks every entry) beside a graph of 3, every row pooled: the largest
    window of the launch."""
    rng = np.random.default_rng([H, n_rows, int(exact), 13])
    rowptr, col, val, xrow, gptr = graph_view(rng, [3, n_rows], [[1, 2], [0, 1, 2, 3, 5]], 1, False, pow2_val=exact)
    if exact:
        T, b0 = qr.exact_gather_inputs(rng, H, int(gptr[-1]), True)
    else:
        T, b0 = rng.normal(0, 1, size=(int(gptr[-1]), H)).astype(np.float32), rng.normal(0, 1, size=H).astype(np.float32)
    seg, prow, pptr = pooled_rows(rng, gptr, [1, 0], ["all"])
    return dict(rowptr=rowptr, col=col, val=val, xrow=None, T=T, b0=b0, seg=seg, prow=prow, pptr=pptr, gptr=gptr, max_rows=n_rows)


TAIL_SEGMENTS = [0, 1, 15, 16, 17, 33]
TAIL_SEGMENTS_POW2 = [0, 1, 16, 2, 32, 4]        # the mean's division is exact: the head behind it stays exact too
# (H, H2, C, with_b1, with_bl)
EXACT_TAIL_CASES = [(4, 16, 1, True, True), (64, 64, 7, False, True), (68, 80, 47, True, False), (512, 512, 48, True, True)]


def exact_tail_case(H, H2, C, with_b1, with_bl, pool):
    """query_reference.exact_tail_inputs over the segments of TAIL_SEGMENTS (max) or TAIL_SEGMENTS_POW2 (mean)."""
    lens = TAIL_SEGMENTS if pool == "max" else TAIL_SEGMENTS_POW2
    rng = np.random.default_rng([H, H2, C, int(with_b1), int(with_bl), int(pool == "max"), 17])
    pptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    G, W1, b1, Wl, bl = qr.exact_tail_inputs(rng, int(pptr[-1]), H, H2, C, with_b1, with_bl)
    return dict(G=G, W1=W1, b1=b1, Wl=Wl, bl=bl, pptr=pptr)


def dead_rows_case(pool):
    """Every live z is exactly -1 (pre-activation -64 + 32) while a padded tile row, whose G is zero, has z = ELU(b1) = 32: a pool that
    reads dead rows returns 32 (max) or a shifted mean.  Segments of 1, 15, 17 and 2 rows (all but 16 leave dead rows in a tile)."""
    H, H2, C = 4, 16, 3
    lens = [1, 15, 17, 2] if pool == "max" else [1, 2, 4, 1]     # (mean: power-of-two counts keep the case exact; 1, 2 and 4 leave 15, 14, 12 dead rows)
    pptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    G = np.ones((int(pptr[-1]), H), dtype=np.float32)
    W1 = np.full((H2, H), -16.0, dtype=np.float32)
    b1 = np.full(H2, 32.0, dtype=np.float32)
    Wl = (np.arange(C * H2).reshape(C, H2) % 5 - 2).astype(np.float32) / 2
    bl = np.array([0.5, -0.25, 1.0], dtype=np.float32)
    return dict(G=G, W1=W1, b1=b1, Wl=Wl, bl=bl, pptr=pptr)


def neighbour_case(pool):
    """Segments of 15 and 1 rows with entries in {0..4}/4, each followed by a segment whose rows are 1024 times larger: a tile that
    reads past its segment's end pools a neighbour's rows."""
    H, H2, C = 8, 16, 2
    lens = [15, 16, 1, 16] if pool == "max" else [2, 16, 1, 16]
    rng = np.random.default_rng([int(pool == "max"), 19])
    pptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    G, W1, b1, Wl, bl = qr.exact_tail_inputs(rng, int(pptr[-1]), H, H2, C, False, True)
    for i in (1, 3):
        G[pptr[i]:pptr[i + 1]] *= 1024.0
    return dict(G=G, W1=W1, b1=b1, Wl=Wl, bl=bl, pptr=pptr)
