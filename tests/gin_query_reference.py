"""float64 references of the two GIN node-query kernels (csrc/query.hip: gin_query_hops_kernel, gin_query_tail_kernel) in the kernels'
stated operation order, a float64 two-layer GIN forward composed from the oracle, and the input generators the CPU and GPU tests share
(test infrastructure only).

o0 = 1.0f + eps0, o1 = 1.0f + eps1: formed ONCE, in float32 (the kernel's own single operation, mirrored, not bounded).
row r    a = 0; a = val[e'] * T[t(col[e'])][c] + a over row r's entries in CSR order; a = o0 * T[t(r)][c] + a; a = a + b0a[c] (b0a None:
         this add is absent); a_r = max(a, 0); t(r) = xrow[r] with an indirection, else r.
product  h_r[n] = max((sum over k ascending of a_r[k] * W0b[n][k], from 0) + b0b[n], 0) (b0b None: the add is of 0.0, no rounding).
query q  the work items are q's entries in CSR order, then q itself, in tiles of 16; item i has weight val[e_i], the last one o1, and
         belongs to fold group (i % 16) // 4.  A group folds its items in ascending i across tiles: P_g = w_i * h_i + P_g from 0.
         s = ((P_0 + P_1) + P_2) + P_3.
tail     z1[n] = max(sum_k ascending G[q][k] W1a[n][k] (+ b1a[n]), 0); z2[m] = max(sum_n ascending z1[n] W1b[m][n] (+ b1b[m]), 0);
         logit[c] = sum_m ascending z2[m] Wl[c][m] (+ bl[c]); the log-softmax of tests/query_reference.tail.
There is no transcendental before the log-softmax: ReLU is exact.

`watch` (optional callable) receives (name, array) for every intermediate: the EXACT-input test asserts each survives a round trip
through float32, i.e. that the fp32 kernel forms it without rounding.
"""
import numpy as np

from query_reference import _see, log_softmax_bound, query_csr  # noqa: F401

GROUPS, TILE = 4, 16


def one_plus(eps):
    """1.0f + eps as the kernel forms it: one float32 addition."""
    return float(np.float32(1.0) + np.float32(eps))


def _chain(A, W, b, watch, name):
    """acc[r][n] = sum over k ascending of A[r][k] W[n][k], from 0, then + b; also S = sum |terms| + |b|."""
    acc = np.zeros((A.shape[0], W.shape[0]))
    S = np.zeros_like(acc)
    for k in range(A.shape[1]):
        term = A[:, k:k + 1] * W[None, :, k]
        acc = _see(watch, name, term + acc)
        S += np.abs(term)
    if b is not None:
        acc = _see(watch, name, acc + b[None, :])
        S += np.abs(b)[None, :]
    return acc, S


def hops(rowptr, col, val, T, eps0, W0b, b0b, eps1, rows, xrow=None, b0a=None, watch=None, sums=False):
    """G [Q, Hb] float64: G[i] = s_q for q = rows[i].  sums=True: also B [Q, Hb], the first-order error bound of every entry in
    units of 2^-24, one rounding per fmaf and per add, each at most the sum of the magnitudes it has seen:
      a_r   of degree d with S_a = sum |val T| + |o0 root| + |b0a|:  E_a = (d + 1 + [b0a]) S_a  (ReLU has slope <= 1: the error
            passes at most unchanged);
      h_r   with S_h = sum_k |a_r[k] W0b[n][k]| + |b0b[n]|:  E_h = |W0b| E_a + (Ha + [b0b]) S_h;
      s_q   sum_i |w_i| E_h(i) + (m + 3) sum_i |w_i h_i|, m = 4 (items // 16) + min(4, items % 16) the longest group chain, 3 for
            the additions of the four groups."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    val, T, W = np.asarray(val, dtype=np.float64), np.asarray(T, dtype=np.float64), np.asarray(W0b, dtype=np.float64)
    Ha, Hb = T.shape[1], W.shape[0]
    assert W.shape[1] == Ha
    ba = None if b0a is None else np.asarray(b0a, dtype=np.float64)
    bb = None if b0b is None else np.asarray(b0b, dtype=np.float64)
    o0, o1 = one_plus(eps0), one_plus(eps1)
    tr = (lambda c: int(c)) if xrow is None else (lambda c: int(xrow[c]))
    rows = np.asarray(rows, dtype=np.int64)

    need = sorted({int(q) for q in rows} | {int(c) for q in rows for c in col[rowptr[q]:rowptr[q + 1]]})
    A = np.zeros((len(need), Ha))
    EA = np.zeros((len(need), Ha))
    for n, r in enumerate(need):
        a = np.zeros(Ha)
        S = np.zeros(Ha)
        for e2 in range(rowptr[r], rowptr[r + 1]):
            term = val[e2] * T[tr(col[e2])]
            a = _see(watch, "a", term + a)
            S += np.abs(term)
        term = o0 * T[tr(r)]
        a = _see(watch, "a", term + a)
        S += np.abs(term)
        if ba is not None:
            a = _see(watch, "a", a + ba)
            S += np.abs(ba)
        A[n] = np.maximum(a, 0)
        EA[n] = (rowptr[r + 1] - rowptr[r] + 1 + (ba is not None)) * S
    acc, S = _chain(A, W, bb, watch, "h")
    Hm = np.maximum(acc, 0)
    EH = EA @ np.abs(W).T + (Ha + (bb is not None)) * S
    at = {r: n for n, r in enumerate(need)}

    G = np.zeros((len(rows), Hb))
    B = np.zeros((len(rows), Hb))
    for i, q in enumerate(rows):
        q = int(q)
        e0, e1 = rowptr[q], rowptr[q + 1]
        items = [(val[e], at[int(col[e])]) for e in range(e0, e1)] + [(o1, at[q])]
        P = np.zeros((GROUPS, Hb))
        absum = np.zeros(Hb)
        inerr = np.zeros(Hb)
        for k, (w, n) in enumerate(items):
            g = (k % TILE) // GROUPS
            P[g] = _see(watch, "p", w * Hm[n] + P[g])
            absum += np.abs(w * Hm[n])
            inerr += np.abs(w) * EH[n]
        s = P[0]
        for g in range(1, GROUPS):
            s = _see(watch, "s", s + P[g])
        G[i] = s
        m = 4 * (len(items) // TILE) + min(4, len(items) % TILE)
        B[i] = inerr + (m + GROUPS - 1) * absum
    return (G, B) if sums else G


def tail(G, W1a, b1a, W1b, b1b, Wl, bl, log_softmax=False, watch=None, sums=False):
    """out [Q, C] float64.  sums=True: also B [Q, C], the first-order error bound of the LOGITS in units of 2^-24 (G is the kernel's
    input: exact): E_1 = (K + [b1a]) S_1; E_2 = |W1b| E_1 + (H2a + [b1b]) S_2; B = |Wl| E_2 + (H2b + [bl]) S_l, with S the sums of
    the magnitudes of a chain's terms and its bias.  With log_softmax the result's bound is log_softmax_bound(logits, B)."""
    G, W1a, W1b, Wl = (np.asarray(a, dtype=np.float64) for a in (G, W1a, W1b, Wl))
    f = lambda b: None if b is None else np.asarray(b, dtype=np.float64)   # noqa: E731
    b1a, b1b, bl = f(b1a), f(b1b), f(bl)
    K, H2a, H2b = G.shape[1], W1a.shape[0], W1b.shape[0]
    assert W1a.shape[1] == K and W1b.shape[1] == H2a and Wl.shape[1] == H2b
    acc, S1 = _chain(G, W1a, b1a, watch, "z1")
    z1 = np.maximum(acc, 0)
    E1 = (K + (b1a is not None)) * S1
    acc, S2 = _chain(z1, W1b, b1b, watch, "z2")
    z2 = np.maximum(acc, 0)
    E2 = E1 @ np.abs(W1b).T + (H2a + (b1b is not None)) * S2
    lg, Sl = _chain(z2, Wl, bl, watch, "logit")
    B = E2 @ np.abs(Wl).T + (H2b + (bl is not None)) * Sl
    out = lg
    if log_softmax:
        m = lg.max(1, keepdims=True)
        t = lg - m
        s = np.zeros((lg.shape[0], 1))
        for c in range(lg.shape[1]):
            s = s + np.exp(t[:, c:c + 1])
        out = t - np.log(s)
    return (out, B) if sums else out


# ---- graphs ----
def sum_csr(edge_index, n):
    """float64 sum CSR of a graph as csr.CSRGraph(mode="sum") builds it: rows = targets, columns = sources ascending, no self loops
    added or removed, val = 1."""
    src, dst = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    order = np.lexsort((src, dst))
    src, dst = src[order], dst[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(dst, minlength=n))
    return rowptr, src, np.ones(len(src))


def oracle_forward(gorc, sd, x, edge_index, log_softmax=True):
    """network.py:29-35 in eval mode with two GINConv layers (nn = Linear, ReLU, Linear, ReLU), composed from
    oracle.gnn_oracle.gin_aggregate in float64 (torch tensors); the model's ELU after each conv is kept as it is."""
    import torch
    x = x.double()
    for i in range(2):
        p = f"conv.{i}."
        x = gorc.gin_aggregate(x, edge_index, sd[p + "eps"].double())
        for j in (0, 2):
            x = torch.relu(x @ sd[p + f"nn.{j}.weight"].double().t() + sd[p + f"nn.{j}.bias"].double())
        x = torch.nn.functional.elu(x)
    y = x @ sd["lt1.weight"].double().t() + sd["lt1.bias"].double()
    return torch.log_softmax(y, dim=1) if log_softmax else y


# ---- inputs of the kernel tests ----
# query degrees: 0 (only the self item), 1, 3 (the self item alone in fold group 0's last slot; a wave without entries forms it), 14,
# 15 (exactly one full tile), 16 (the self item alone in a second tile), 31, 32, 40; one-hop row degrees: 0, 1, 63, 64, 65 (a second
# 64-entry batch), 300 (five batches)
HOPS_QUERY_DEGS = [0, 1, 3, 14, 15, 16, 31, 32, 40]
HOPS_ROW_DEGS = [0, 1, 63, 64, 65, 300]
# (Ha, Hb, with_xrow, with_bias, eps0, eps1): (4, 16) one k-step, one column block; (40, 16) an 8-wide last k-stage; (256, 256) one
# full column pass; (260, 272) a second pass of one block and a second slot with one live lane; (272, 48) / (64, 272): two slots with
# one pass / one slot with two passes (the other two instantiations); unequal pairs show a swapped index
EXACT_HOPS_CASES = [(4, 16, False, True, 0.5, -0.25), (40, 16, True, False, -0.25, 0.5), (64, 64, True, True, 0.5, 0.5),
                    (256, 256, False, False, -0.25, -0.25), (260, 272, True, True, 0.5, -0.25), (512, 512, False, True, -0.25, 0.5),
                    (272, 48, True, False, 0.5, -0.25), (64, 272, False, True, -0.25, 0.5)]
# (K, H2a, H2b, C, Q, with_bias)
EXACT_TAIL_CASES = [(64, 64, 64, 7, 16, True), (272, 80, 48, 47, 22, True), (16, 16, 272, 3, 1, False)]
# (Ha, Hb, H2a, H2b, C): hops -> tail
CHAIN_CASES = [(64, 48, 64, 32, 7), (260, 272, 80, 48, 47)]
CHAIN_QUERY_DEGS = [0, 1, 2, 3, 5, 16, 17]
CHAIN_ROW_DEGS = [0, 1, 2]


def _small(rng, shape, lo, hi, den, p_zero=0.0):
    """Integers in [lo, hi] over den; p_zero: the share of entries set to 0 on top."""
    a = rng.integers(lo, hi + 1, size=shape) / float(den)
    if p_zero:
        a = a * (rng.random(size=shape) >= p_zero)
    return a.astype(np.float32)


def exact_hops_case(Ha, Hb, with_xrow, with_bias, eps0, eps1):
    """T in {-8..8}/8, CSR values in {1/4, 1/2, 1}, eps in {0.5, -0.25} (1 + eps = 1.5 or 0.75), b0a in {-8..8}/8: a_r is a multiple
    of 1/32.  W0b in {-2..2}/4 and b0b in {-8..8}/8: h_r is a multiple of 1/128, s_q of 1/512.  tests/test_gin_query_reference_cpu.py
    proves every intermediate exact in fp32 for these draws."""
    rng = np.random.default_rng([Ha, Hb, int(with_xrow), int(with_bias), 19])
    n_table = 37
    rowptr, col, val, xrow, n_rows = query_csr(rng, HOPS_QUERY_DEGS, HOPS_ROW_DEGS, n_table, with_xrow, pow2_val=True)
    T = _small(rng, (n_table if with_xrow else n_rows, Ha), -8, 8, 8)
    W0b = _small(rng, (Hb, Ha), -2, 2, 4)
    b0a = _small(rng, Ha, -8, 8, 8) if with_bias else None
    b0b = _small(rng, Hb, -8, 8, 8) if with_bias else None
    rows = np.arange(len(HOPS_QUERY_DEGS), dtype=np.int64)
    return dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=T, b0a=b0a, eps0=np.float32(eps0), W0b=W0b, b0b=b0b, eps1=np.float32(eps1),
                rows=rows, n_rows=n_rows)


def exact_tail_case(K, H2a, H2b, C, Q, with_bias):
    """G in {-4..4}/4 (both signs: a hops output is not, a tail input may be), W1a and W1b in {-2..2}/2, Wl in {-1, 0, 1}, biases in
    {-8..8}/8: z1 is a multiple of 1/8, z2 and the logits of 1/16."""
    rng = np.random.default_rng([K, H2a, H2b, C, Q, int(with_bias), 23])
    b = lambda n: _small(rng, n, -8, 8, 8) if with_bias else None   # noqa: E731
    return dict(G=_small(rng, (Q, K), -4, 4, 4), W1a=_small(rng, (H2a, K), -2, 2, 2), b1a=b(H2a), W1b=_small(rng, (H2b, H2a), -2, 2, 2),
                b1b=b(H2b), Wl=_small(rng, (C, H2b), -1, 1, 1), bl=b(C))


def exact_chain_case(Ha, Hb, H2a, H2b, C):
    """Hops inputs whose s_q stays small enough for the tail's three chains to be exact as well: degrees up to 17 and 2, CSR values in
    {1/2, 1}, T in {-4..4}/8, W0b, W1a, W1b and Wl in {-1, 0, 1} with three entries in four zero, biases in {-8..8}/8.  The queries are
    every row of the CSR, twice: more than 16 rows, a partial last tile of the tail."""
    rng = np.random.default_rng([Ha, Hb, H2a, H2b, C, 29])
    rowptr, col, val, xrow, n_rows = query_csr(rng, CHAIN_QUERY_DEGS, CHAIN_ROW_DEGS, 23, True, pow2_val=True)
    val = np.maximum(val, np.float32(0.5))
    w = lambda *s: _small(rng, s, -1, 1, 1, p_zero=0.75)   # noqa: E731
    b = lambda n: _small(rng, n, -8, 8, 8)                  # noqa: E731
    rows = np.concatenate([np.arange(n_rows), np.arange(n_rows)[::-1]])[:37].astype(np.int64)
    return dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=_small(rng, (23, Ha), -4, 4, 8), b0a=b(Ha), eps0=np.float32(0.5),
                W0b=w(Hb, Ha), b0b=b(Hb), eps1=np.float32(-0.25), rows=rows, n_rows=n_rows, W1a=w(H2a, Hb), b1a=b(H2a), W1b=w(H2b, H2a),
                b1b=b(H2b), Wl=w(C, H2b), bl=b(C))
