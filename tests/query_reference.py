"""float64 references of the two node-query kernels (csrc/query.hip) in the kernels' stated operation order, a dense float64
two-layer forward, and the input generators the CPU and GPU tests share (test infrastructure only).

gather   a = 0; a = val[e'] * T[.][c] + a over row j's entries in CSR order; h = ELU(a + b0[c]); entry i of row q (CSR order) belongs
         to wave i % 4, folded in ascending i: p_w = val[e] * h + p_w; g = ((p_0 + p_1) + p_2) + p_3.
tail     z[n] = ELU(sum_k ascending G[q][k] W1[n][k] (+ b1[n])); logit[c] = sum_h ascending z[h] Wl[c][h] (+ bl[c]);
         log-softmax: m = max, s = sum_c exp(logit[c] - m) ascending c, out[c] = (logit[c] - m) - log(s).

`watch` (optional callable) receives (name, array) for every intermediate: the EXACT-input test asserts each survives a round trip
through float32, i.e. that the fp32 kernel forms it without rounding, and that every pre-activation ("pre") is >= 0 or <= -32.
f32_elu rounds the ELU's result to float32 (what the exact cases compare against: float64 expm1(-32) is -1 + 1.3e-14, fp32's -1).
"""
import numpy as np

WAVES = 4


def elu(x, f32=False):
    """f32: the result rounded to float32, the value a correctly rounded fp32 ELU returns (x <= -32 gives exactly -1)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    return y.astype(np.float32).astype(np.float64) if f32 else y


def _see(watch, name, a):
    if watch is not None:
        watch(name, a)
    return a


def gather(rowptr, col, val, T, rows, xrow=None, b0=None, watch=None, sums=False, f32_elu=False):
    """G [Q, H] float64.  sums=True: also B [Q, H], the first-order error bound of every entry in units of 2^-24: per neighbour
    row j of degree d_j with S_j = sum |val T| + |b0|, (d_j + 1) S_j (the fmaf chain and the bias add) + 2 |h_j| where the
    pre-activation is <= 0 (expm1f within 1 ulp; ELU has slope <= 1, so the pre-activation's error passes at most unchanged), weighted
    by |val_e|; plus (ceil(deg / 4) + 3) sum |val_e h_j| for the longest wave chain and the three additions of the partials."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    val, T = np.asarray(val, dtype=np.float64), np.asarray(T, dtype=np.float64)
    H = T.shape[1]
    bias = np.zeros(H) if b0 is None else np.asarray(b0, dtype=np.float64)
    tr = (lambda c: c) if xrow is None else (lambda c: int(xrow[c]))
    G = np.zeros((len(rows), H))
    B = np.zeros((len(rows), H))
    hcache = {}
    for i, q in enumerate(np.asarray(rows, dtype=np.int64)):
        part = np.zeros((WAVES, H))
        absum = np.zeros(H)     # sum |val_e h_j|
        inerr = np.zeros(H)     # sum |val_e| ((d_j + 1) S_j + 2 |h_j| [pre <= 0])
        e0, e1 = rowptr[q], rowptr[q + 1]
        for k, e in enumerate(range(e0, e1)):
            j = col[e]
            if j not in hcache:
                a = np.zeros(H)
                S = np.abs(bias).copy()
                for e2 in range(rowptr[j], rowptr[j + 1]):
                    term = val[e2] * T[tr(col[e2])]
                    a = _see(watch, "a", term + a)
                    S += np.abs(term)
                pre = _see(watch, "pre", a + bias)
                h = _see(watch, "h", elu(pre, f32_elu))
                d = rowptr[j + 1] - rowptr[j]
                hcache[j] = (h, (d + 1) * S + 2 * np.abs(h) * (pre <= 0))
            h, herr = hcache[j]
            w = k % WAVES
            part[w] = _see(watch, "p", val[e] * h + part[w])
            absum += np.abs(val[e] * h)
            inerr += np.abs(val[e]) * herr
        g = part[0]
        for w in range(1, WAVES):
            g = _see(watch, "g", g + part[w])
        G[i] = g
        m = -(-(e1 - e0) // WAVES)   # longest wave chain
        B[i] = inerr + (m + WAVES - 1) * absum
    return (G, B) if sums else G


def tail(G, W1, b1, Wl, bl, log_softmax=False, watch=None, sums=False, f32_elu=False):
    """out [Q, C] float64.  sums=True: also B [Q, C], the first-order error bound of the LOGITS in units of 2^-24: z[n] carries
    (H + 1) (sum_k |G W1| + |b1|) + 2 |z| where its pre-activation is <= 0, weighted by |Wl[c][n]|; plus (H2 + 1) (sum_h |z Wl| + |bl|)
    for the head's chain and bias add.  With log_softmax the result's bound is log_softmax_bound(logits, B)."""
    G, W1, Wl = (np.asarray(a, dtype=np.float64) for a in (G, W1, Wl))
    Q, H = G.shape
    H2, C = W1.shape[0], Wl.shape[0]
    acc = np.zeros((Q, H2))
    S = np.zeros((Q, H2))
    for k in range(H):
        term = G[:, k:k + 1] * W1[None, :, k]
        acc = _see(watch, "acc", term + acc)
        S += np.abs(term)
    if b1 is not None:
        acc = _see(watch, "acc", acc + np.asarray(b1, dtype=np.float64)[None, :])
        S += np.abs(np.asarray(b1, dtype=np.float64))[None, :]
    _see(watch, "pre", acc)
    z = _see(watch, "z", elu(acc, f32_elu))
    zerr = (H + 1) * S + 2 * np.abs(z) * (acc <= 0)
    lg = np.zeros((Q, C))
    L = np.zeros((Q, C))
    for h in range(H2):
        term = z[:, h:h + 1] * Wl[None, :, h]
        lg = _see(watch, "logit", term + lg)
        L += np.abs(term)
    E = zerr @ np.abs(Wl).T
    if bl is not None:
        lg = _see(watch, "logit", lg + np.asarray(bl, dtype=np.float64)[None, :])
        L += np.abs(np.asarray(bl, dtype=np.float64))[None, :]
    B = E + (H2 + 1) * L
    out = lg
    if log_softmax:
        m = lg.max(1, keepdims=True)
        t = lg - m
        s = np.zeros((Q, 1))
        for c in range(C):
            s = s + np.exp(t[:, c:c + 1])
        out = t - np.log(s)
    return (out, B) if sums else out


def log_softmax_bound(logits, B):
    """First-order bound (in units of 2^-24) on the error of the kernel's log-softmax given per-logit bounds B: the logits' errors
    reach a row's result at most twice over (d out_c / d x is a difference of two probability vectors); t = x - m rounds once
    (|t|); expf is within 1 ulp (2 units) of exp of its rounded argument (sum_c sm_c |t_c|); the C additions of s; logf within
    1 ulp (2 |l|); the last subtraction (|out|)."""
    x = np.asarray(logits, dtype=np.float64)
    C = x.shape[1]
    m = x.max(1, keepdims=True)
    t = x - m
    s = np.exp(t).sum(1, keepdims=True)
    sm = np.exp(t) / s
    l = np.log(s)
    out = t - l
    return 2 * B.max(1, keepdims=True) + np.abs(t) + 2 + (sm * np.abs(t)).sum(1, keepdims=True) + C + 2 * np.abs(l) + np.abs(out)


# ---- graphs ----
def gcn_csr(edge_index, n):
    """float64 GCN-normalised CSR of a graph as csr.CSRGraph builds it: rows = targets, columns = sources ascending, existing self
    loops replaced by exactly one, val = d^-1/2[row] d^-1/2[col]."""
    src, dst = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    keep = src != dst
    loop = np.arange(n, dtype=np.int64)
    src, dst = np.concatenate([src[keep], loop]), np.concatenate([dst[keep], loop])
    order = np.lexsort((src, dst))
    src, dst = src[order], dst[order]
    deg = np.bincount(dst, minlength=n).astype(np.float64)
    dinv = np.where(deg > 0, deg ** -0.5, 0.0)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(dst, minlength=n))
    return rowptr, src, dinv[dst] * dinv[src]


def dense_forward(x, edge_index, W0, b0, W1, b1, Wl, bl, log_softmax=True):
    """The two-layer GCN forward on the whole graph with a dense float64 A_hat (network.py:29-35, eval mode)."""
    n = x.shape[0]
    rowptr, col, val = gcn_csr(edge_index, n)
    A = np.zeros((n, n))
    for r in range(n):
        A[r, col[rowptr[r]:rowptr[r + 1]]] = val[rowptr[r]:rowptr[r + 1]]
    h = elu(A @ (np.asarray(x, dtype=np.float64) @ W0.T) + b0)
    z = elu(A @ (h @ W1.T) + b1)
    y = z @ Wl.T + bl
    if log_softmax:
        y = y - y.max(1, keepdims=True)
        y = y - np.log(np.exp(y).sum(1, keepdims=True))
    return y


# ---- inputs of the kernel tests ----
def query_csr(rng, q_degs, n_degs, n_table, with_xrow, pow2_val):
    """A hand-made CSR for the gather: query row i has q_degs[i] entries pointing at neighbour rows whose own degrees cycle through
    n_degs; the neighbour rows' entries point anywhere (with xrow: through an indirection with repeated table rows, one entry at the
    last table row).  Rows: the queries first, then the neighbour rows.  pow2_val: values from {1/4, 1/2, 1}, else uniform."""
    nq = len(q_degs)
    n_nb = max(len(n_degs), max(q_degs) if q_degs else 1, 1)
    n_rows = nq + n_nb
    rowptr, col = [0], []
    for d in q_degs:
        start = int(rng.integers(0, n_nb))
        col += [nq + (start + k) % n_nb for k in range(d)]   # distinct while d <= n_nb
        rowptr.append(len(col))
    for k in range(n_nb):
        d = n_degs[k % len(n_degs)]
        col += rng.integers(0, n_rows, size=d).tolist()
        rowptr.append(len(col))
    col = np.array(col, dtype=np.int32)
    val = (rng.choice([0.25, 0.5, 1.0], size=len(col)) if pow2_val else rng.uniform(0.05, 1.0, size=len(col))).astype(np.float32)
    xrow = None
    if with_xrow:
        xrow = rng.integers(0, n_table, size=n_rows).astype(np.int32)
        xrow[n_rows // 2:] = xrow[: n_rows - n_rows // 2]     # repeated table rows
        if len(col):
            xrow[col[-1]] = n_table - 1                        # one entry at the last table row
    return np.array(rowptr, dtype=np.int32), col, val, xrow, n_rows


def exact_gather_inputs(rng, H, n_table, with_b0):
    """T and b0 for EXACT gather runs.  With b0: a column is either non-negative (T in {0..8}/8, b0 in {0..8}/8: every
    pre-activation >= 0, ELU the identity) or non-positive (T in {-8..0}/8, b0 = -32: every pre-activation <= -32, fp32 ELU exactly
    -1).  Without b0 every column is non-negative."""
    neg = (np.arange(H) % 2 == 1) if with_b0 else np.zeros(H, dtype=bool)   # every other column
    T = rng.integers(0, 9, size=(n_table, H)) / 8.0
    T[:, neg] *= -1.0
    b0 = None
    if with_b0:
        b0 = np.where(neg, -32.0, rng.integers(0, 9, size=H) / 8.0).astype(np.float32)
    return T.astype(np.float32), b0


def exact_tail_inputs(rng, Q, H, H2, C, with_b1, with_bl):
    """G in {0..4}/4; a row of W1 is non-negative ({0,1,2}/2, b1 in {0..8}/8) or, with b1, non-positive with b1 = -32 - so every
    pre-activation is >= 0 or <= -32; Wl in {-2..2}/2, bl in {-8..8}/8."""
    G = (rng.integers(0, 5, size=(Q, H)) / 4.0).astype(np.float32)
    neg = (np.arange(H2) % 2 == 1) if with_b1 else np.zeros(H2, dtype=bool)   # every other row of W1
    W1 = rng.integers(0, 3, size=(H2, H)) / 2.0
    W1[neg] *= -1.0
    b1 = np.where(neg, -32.0, rng.integers(0, 9, size=H2) / 8.0).astype(np.float32) if with_b1 else None
    Wl = (rng.integers(-2, 3, size=(C, H2)) / 2.0).astype(np.float32)
    bl = (rng.integers(-8, 9, size=C) / 8.0).astype(np.float32) if with_bl else None
    return G, W1.astype(np.float32), b1, Wl, bl


# the EXACT cases of tests/test_gpu_query_kernels.py (tests/test_query_reference_cpu.py proves each exact on the CPU)
GATHER_QUERY_DEGS = [0, 1, 2, 3, 4, 5, 8, 9, 17, 64, 65, 130]
GATHER_NEIGHBOUR_DEGS = [0, 1, 2, 63, 64, 65, 300]
# (H, with_xrow, with_b0)
EXACT_GATHER_CASES = [(4, False, True), (64, True, False), (256, False, False), (260, True, True), (512, False, True), (516, True, True)]
# (H, H2, C, Q, with_b1, with_bl)
EXACT_TAIL_CASES = [(4, 16, 1, 1, True, True), (64, 64, 3, 15, False, True), (68, 80, 7, 16, True, False), (512, 512, 47, 17, True, True),
                    (64, 64, 16, 33, True, True), (68, 80, 48, 17, False, False)]


def exact_gather_case(H, with_xrow, with_b0):
    rng = np.random.default_rng([H, int(with_xrow), int(with_b0), 7])
    n_table = 37
    rowptr, col, val, xrow, n_rows = query_csr(rng, GATHER_QUERY_DEGS, GATHER_NEIGHBOUR_DEGS, n_table, with_xrow, pow2_val=True)
    T, b0 = exact_gather_inputs(rng, H, n_table if with_xrow else n_rows, with_b0)
    rows = np.arange(len(GATHER_QUERY_DEGS), dtype=np.int64)
    return dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=T, b0=b0, rows=rows, n_rows=n_rows)


def exact_tail_case(H, H2, C, Q, with_b1, with_bl):
    rng = np.random.default_rng([H, H2, C, Q, int(with_b1), int(with_bl), 11])
    G, W1, b1, Wl, bl = exact_tail_inputs(rng, Q, H, H2, C, with_b1, with_bl)
    return dict(G=G, W1=W1, b1=b1, Wl=Wl, bl=bl)
