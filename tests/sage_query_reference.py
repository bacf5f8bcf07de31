"""float64 reference of the SAGE node-query gather (csrc/query.hip, sage_query_gather_kernel) in the kernel's stated operation
order, a float64 two-layer SAGE forward composed from the oracle, and the input generators the CPU and GPU tests share (test
infrastructure only).  The tail is tests/query_reference.tail, unchanged, on G = [g_q | h_q] with W1 = [W_l1 | W_r1].

row r    a = 0; a = val[e'] * T[t(col[e'])][c] + a over row r's entries in CSR order; h_r[c] = ELU((a + T[t(r)][H + c]) + b0[c])
         (b0 None: the second add is absent); t(r) = xrow[r] with an indirection, else r.
query q  the work items are q's entries in CSR order, then q itself; item i belongs to wave i % 4.  An entry item folds
         p_w = val[e] * h_{col[e]} + p_w; the last item is h_q, stored as G[i][H:2H].  G[i][0:H] = ((p_0 + p_1) + p_2) + p_3.

`watch`, `f32_elu` and `sums` as in tests/query_reference.py (whose elu, query_csr, tail, log_softmax_bound and degree lists are reused
by import).
"""
import numpy as np

from query_reference import (EXACT_GATHER_CASES, GATHER_NEIGHBOUR_DEGS, GATHER_QUERY_DEGS, WAVES, _see, elu, log_softmax_bound,  # noqa: F401
                             query_csr, tail)


def gather(rowptr, col, val, T, rows, xrow=None, b0=None, watch=None, sums=False, f32_elu=False):
    """G [Q, 2H] float64: G[i][0:H] = g_q, G[i][H:2H] = h_q for q = rows[i]; T is [n_table, 2H].  sums=True: also B [Q, 2H], the
    first-order error bound of every entry in units of 2^-24.  A layer-0 row r of degree d_r with S_r = sum |val T| + |root| + |b0|
    carries E_r = (d_r + 2) S_r (one rounding per fmaf of the chain, one for the root add, one for the bias add, each at most the
    sum of the magnitudes) + 2 |h_r| where the pre-activation is <= 0 (expm1f within 1 ulp; ELU has slope <= 1, so the
    pre-activation's error passes at most unchanged).  B[i][H:2H] = E_q.  B[i][0:H] = sum_e |val_e| E_{col[e]} + (ceil(deg / 4) + 3)
    sum_e |val_e h_{col[e]}| for the longest wave chain and the three additions of the partials."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    val, T = np.asarray(val, dtype=np.float64), np.asarray(T, dtype=np.float64)
    H = T.shape[1] // 2
    assert T.shape[1] == 2 * H
    bias = None if b0 is None else np.asarray(b0, dtype=np.float64)
    tr = (lambda c: int(c)) if xrow is None else (lambda c: int(xrow[c]))
    G = np.zeros((len(rows), 2 * H))
    B = np.zeros((len(rows), 2 * H))
    hcache = {}

    def row(r):
        if r not in hcache:
            a = np.zeros(H)
            S = np.zeros(H)
            for e2 in range(rowptr[r], rowptr[r + 1]):
                term = val[e2] * T[tr(col[e2]), :H]
                a = _see(watch, "a", term + a)
                S += np.abs(term)
            root = T[tr(r), H:]
            pre = _see(watch, "a", a + root)
            S += np.abs(root)
            if bias is not None:
                pre = pre + bias
                S += np.abs(bias)
            _see(watch, "pre", pre)
            h = _see(watch, "h", elu(pre, f32_elu))
            d = rowptr[r + 1] - rowptr[r]
            hcache[r] = (h, (d + 2) * S + 2 * np.abs(h) * (pre <= 0))
        return hcache[r]

    for i, q in enumerate(np.asarray(rows, dtype=np.int64)):
        q = int(q)
        part = np.zeros((WAVES, H))
        absum = np.zeros(H)     # sum |val_e h_j|
        inerr = np.zeros(H)     # sum |val_e| E_j
        e0, e1 = rowptr[q], rowptr[q + 1]
        for k, e in enumerate(range(e0, e1)):
            h, herr = row(int(col[e]))
            w = k % WAVES
            part[w] = _see(watch, "p", val[e] * h + part[w])
            absum += np.abs(val[e] * h)
            inerr += np.abs(val[e]) * herr
        g = part[0]
        for w in range(1, WAVES):
            g = _see(watch, "g", g + part[w])
        hq, hqerr = row(q)      # the item after the last entry, on wave deg % 4: the same bits on any wave
        G[i, :H], G[i, H:] = g, hq
        m = -(-(e1 - e0) // WAVES)   # longest wave chain
        B[i, :H], B[i, H:] = inerr + (m + WAVES - 1) * absum, hqerr
    return (G, B) if sums else G


# ---- graphs ----
def mean_csr(edge_index, n):
    """float64 mean CSR of a graph as csr.CSRGraph(mode="mean") builds it: rows = targets, columns = sources ascending, no self
    loops added or removed, val = 1 / max(in-degree(row), 1)."""
    src, dst = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    order = np.lexsort((src, dst))
    src, dst = src[order], dst[order]
    deg = np.bincount(dst, minlength=n)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    return rowptr, src, (1.0 / np.maximum(deg, 1))[dst]


def oracle_forward(gorc, sd, x, edge_index, log_softmax=True):
    """network.py:29-35 in eval mode with two SAGEConv layers, composed from oracle.gnn_oracle.sage_conv in float64 (torch tensors)."""
    import torch
    x = x.double()
    for i in range(2):
        p = f"conv.{i}."
        b = sd.get(p + "lin_l.bias")
        x = torch.nn.functional.elu(gorc.sage_conv(x, edge_index, sd[p + "lin_l.weight"].double(), None if b is None else b.double(),
                                                   sd[p + "lin_r.weight"].double()))
    y = x @ sd["lt1.weight"].double().t() + sd["lt1.bias"].double()
    return torch.log_softmax(y, dim=1) if log_softmax else y


# ---- inputs of the kernel tests ----
def exact_sage_inputs(rng, H, n_table, with_b0, negative=True, t_max=8, b_max=8):
    """T [n_table, 2H] and b0 for EXACT gather runs: both halves integers over 8.  With b0 and `negative`, every other column c (in both
    halves: c and H + c) is non-positive (T in {-t_max..0}/8, b0 = -32: every pre-activation <= -32, fp32 ELU exactly -1); the
    others are non-negative (T in {0..t_max}/8, b0 in {0..b_max}/8: ELU the identity).  Without b0 every column is non-negative."""
    neg = (np.arange(H) % 2 == 1) if (with_b0 and negative) else np.zeros(H, dtype=bool)
    T = rng.integers(0, t_max + 1, size=(n_table, 2 * H)) / 8.0
    T[:, np.concatenate([neg, neg])] *= -1.0
    b0 = None
    if with_b0:
        b0 = np.where(neg, -32.0, rng.integers(0, b_max + 1, size=H) / 8.0).astype(np.float32)
    return T.astype(np.float32), b0


# the EXACT cases of tests/test_gpu_sage_query_kernels.py (tests/test_sage_query_reference_cpu.py proves each exact on the CPU):
# (H, with_xrow, with_b0) as for the GCN gather -- H = 4 (one live lane), 64, 256 (one full slab), 260 (second slab, one live lane),
# 512, 516; the query degrees put the item after the last entry on every wave, on a wave without entries too (degrees 0, 1, 2, 3)
EXACT_SAGE_CASES = EXACT_GATHER_CASES
# (H, H2, C): gather -> tail with K = 2H
CHAIN_CASES = [(64, 64, 7), (260, 80, 47)]
CHAIN_QUERY_DEGS = [0, 1, 2, 3, 4, 5]
CHAIN_NEIGHBOUR_DEGS = [0, 1, 2]


def exact_sage_case(H, with_xrow, with_b0):
    rng = np.random.default_rng([H, int(with_xrow), int(with_b0), 13])
    n_table = 37
    rowptr, col, val, xrow, n_rows = query_csr(rng, GATHER_QUERY_DEGS, GATHER_NEIGHBOUR_DEGS, n_table, with_xrow, pow2_val=True)
    T, b0 = exact_sage_inputs(rng, H, n_table if with_xrow else n_rows, with_b0)
    rows = np.arange(len(GATHER_QUERY_DEGS), dtype=np.int64)
    return dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=T, b0=b0, rows=rows, n_rows=n_rows)


def exact_chain_case(H, H2, C):
    """Gather inputs whose G stays small enough for the tail's two chains to be exact as well, with the tail's operands: degrees up to
    5 and 2, CSR values in {1/2, 1}, T and b0 in {0..4}/8 (every column non-negative, so G >= 0, at most 10, a multiple of 1/32);
    W1cat [H2, 2H] in {0, 1}, every other row non-positive with b1 = -32 (else b1 in {0..8}/8); Wl in {-1, 0, 1}, bl in {-8..8}/8.
    z stays below 2^13 at a resolution of 1/32 and a logit below 2^19: 24 bits.  The queries are every row of the CSR, twice: 22 rows,
    two tiles of the tail."""
    rng = np.random.default_rng([H, H2, C, 17])
    rowptr, col, val, xrow, n_rows = query_csr(rng, CHAIN_QUERY_DEGS, CHAIN_NEIGHBOUR_DEGS, 23, True, pow2_val=True)
    val = np.maximum(val, np.float32(0.5))
    T, b0 = exact_sage_inputs(rng, H, 23, True, negative=False, t_max=4, b_max=4)
    neg = np.arange(H2) % 2 == 1
    W1 = rng.integers(0, 2, size=(H2, 2 * H)).astype(np.float64)
    W1[neg] *= -1.0
    b1 = np.where(neg, -32.0, rng.integers(0, 9, size=H2) / 8.0).astype(np.float32)
    Wl = rng.integers(-1, 2, size=(C, H2)).astype(np.float32)
    bl = (rng.integers(-8, 9, size=C) / 8.0).astype(np.float32)
    rows = np.concatenate([np.arange(n_rows), np.arange(n_rows)[::-1]]).astype(np.int64)
    return dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=T, b0=b0, rows=rows, n_rows=n_rows, W1=W1.astype(np.float32), b1=b1, Wl=Wl,
                bl=bl)
