"""Plain float64 NumPy statements of the GAT attention kernels of csrc/gat.hip (test infrastructure only).

Every helper takes a CSR pattern (rowptr [n + 1], col [nnz]; row = target node, entries = its incoming edges) and returns the
float64 result of the kernel's operation, plus, where a tolerance needs it, the per-entry condition sum |terms|.  Composed into
a layer (gat_layer / gat_layer_backward) they must equal oracle.gnn_oracle.gat_conv and its autograd (tests/test_gat_reference_cpu.py).
"""
import numpy as np


def entry_rows(rowptr):
    """Row id of every CSR entry."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def leaky_relu(s, slope):
    return np.where(s > 0, s, slope * s)


def leaky_relu_grad(s, slope):
    """d leaky_relu / ds with the slope at s == 0 (F.leaky_relu's autograd)."""
    return np.where(s > 0, 1.0, slope)


def scores(h, att_src, att_dst):
    """a_src[i] = h_i . att_src, a_dst[i] = h_i . att_dst, and each one's condition sum_c |h_ic att_c|."""
    h = np.asarray(h, dtype=np.float64)
    s, d = np.asarray(att_src, dtype=np.float64), np.asarray(att_dst, dtype=np.float64)
    return h @ s, h @ d, np.abs(h) @ np.abs(s), np.abs(h) @ np.abs(d)


def edge_scores(rowptr, col, a_src, a_dst):
    """s_e = a_src[col[e]] + a_dst[row(e)] (before the LeakyReLU)."""
    return np.asarray(a_src, dtype=np.float64)[np.asarray(col, dtype=np.int64)] + np.asarray(a_dst, dtype=np.float64)[entry_rows(rowptr)]


def edge_softmax(rowptr, col, a_src, a_dst, slope):
    """alpha_e = softmax over the row of LeakyReLU(s_e)."""
    rows = entry_rows(rowptr)
    n = len(rowptr) - 1
    e = leaky_relu(edge_scores(rowptr, col, a_src, a_dst), slope)
    m = np.full(n, -np.inf)
    np.maximum.at(m, rows, e)
    p = np.exp(e - m[rows])
    z = np.bincount(rows, weights=p, minlength=n)
    return p / z[rows]


def _gathered_dots(rows, cols, A, B, chunk=1 << 14):
    """sum_c A[rows[e], c] B[cols[e], c] and sum_c |A B| per entry, in chunks of entries."""
    out, cond = np.empty(len(rows)), np.empty(len(rows))
    for k in range(0, len(rows), chunk):
        a, b = A[rows[k:k + chunk]], B[cols[k:k + chunk]]
        out[k:k + chunk] = np.einsum("ec,ec->e", a, b)
        cond[k:k + chunk] = np.einsum("ec,ec->e", np.abs(a), np.abs(b))
    return out, cond


def sddmm(rowptr, col, dout, h, sel=None):
    """dalpha_e = dOut[row(e)] . h[col[e]] and its condition sum_c |dOut h|.  sel: the rows covered (dOut is then compact:
    its row i belongs to row sel[i]); entries of other rows come back as NaN."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    dout, h = np.asarray(dout, dtype=np.float64), np.asarray(h, dtype=np.float64)
    rows = entry_rows(rowptr)
    if sel is None:
        return _gathered_dots(rows, col, dout, h)
    out, cond = np.full(len(col), np.nan), np.full(len(col), np.nan)
    for i, r in enumerate(np.asarray(sel, dtype=np.int64)):
        e0, e1 = rowptr[r], rowptr[r + 1]
        out[e0:e1] = h[col[e0:e1]] @ dout[i]
        cond[e0:e1] = np.abs(h[col[e0:e1]]) @ np.abs(dout[i])
    return out, cond


def softmax_bwd(rowptr, col, a_src, a_dst, alpha, dalpha, slope):
    """ds_e = alpha_e (dalpha_e - sum_k alpha_k dalpha_k) lrelu'(s_e) over the row, da_dst[row] = sum_e ds_e."""
    rows = entry_rows(rowptr)
    n = len(rowptr) - 1
    alpha, dalpha = np.asarray(alpha, dtype=np.float64), np.asarray(dalpha, dtype=np.float64)
    dot = np.bincount(rows, weights=alpha * dalpha, minlength=n)
    ds = alpha * (dalpha - dot[rows]) * leaky_relu_grad(edge_scores(rowptr, col, a_src, a_dst), slope)
    return ds, np.bincount(rows, weights=ds, minlength=n)


def row_sum(rowptr, v):
    """y[row] = sum of v over the row, and sum |v|."""
    rows = entry_rows(rowptr)
    n = len(rowptr) - 1
    v = np.asarray(v, dtype=np.float64)
    return np.bincount(rows, weights=v, minlength=n), np.bincount(rows, weights=np.abs(v), minlength=n)


def transpose(rowptr, col, n_cols):
    """The transposed pattern (rowptr_t, col_t) and perm with v_t = v[perm] (entries sorted by (col, row))."""
    rows = entry_rows(rowptr)
    perm = np.lexsort((rows, np.asarray(col, dtype=np.int64)))
    rowptr_t = np.zeros(n_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.asarray(col, dtype=np.int64), minlength=n_cols), out=rowptr_t[1:])
    return rowptr_t, rows[perm], perm


def gat_csr(edge_index, n):
    """GATConv's pattern: existing self loops dropped, one added per node, rows = targets, columns sorted within a row."""
    src, dst = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    keep = src != dst
    src = np.concatenate([src[keep], np.arange(n)])
    dst = np.concatenate([dst[keep], np.arange(n)])
    order = np.lexsort((src, dst))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=rowptr[1:])
    return rowptr, src[order]


def spmm(rowptr, col, val, X):
    """Y[row] = sum_e val_e X[col[e]]."""
    rows = entry_rows(rowptr)
    X = np.asarray(X, dtype=np.float64)
    Y = np.zeros((len(rowptr) - 1, X.shape[1]))
    np.add.at(Y, rows, np.asarray(val, dtype=np.float64)[:, None] * X[np.asarray(col, dtype=np.int64)])
    return Y


def gat_layer(x, W, att_src, att_dst, bias, rowptr, col, slope=0.2):
    """GATConv (heads 1) from the helpers above: h = x W^T, alpha by edge_softmax, out = A_alpha h + bias.
    Returns out and the intermediates the backward needs."""
    h = np.asarray(x, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T
    a_s, a_d, _, _ = scores(h, att_src, att_dst)
    alpha = edge_softmax(rowptr, col, a_s, a_d, slope)
    out = spmm(rowptr, col, alpha, h)
    if bias is not None:
        out = out + np.asarray(bias, dtype=np.float64)
    return out, dict(h=h, a_src=a_s, a_dst=a_d, alpha=alpha)


def gat_layer_backward(x, W, att_src, att_dst, rowptr, col, mid, dout, slope=0.2):
    """Gradients of gat_layer as GATAggregate.backward forms them: SDDMM, softmax backward, da_src as a row sum on the transposed
    order, dh = A_alpha^T dOut + da_src (x) att_src + da_dst (x) att_dst.  Returns dx, dW, datt_src, datt_dst, dbias."""
    x, W, dout = (np.asarray(a, dtype=np.float64) for a in (x, W, dout))
    h, alpha = mid["h"], mid["alpha"]
    n = len(rowptr) - 1
    dalpha, _ = sddmm(rowptr, col, dout, h)
    ds, da_dst = softmax_bwd(rowptr, col, mid["a_src"], mid["a_dst"], alpha, dalpha, slope)
    rowptr_t, col_t, perm = transpose(rowptr, col, n)
    da_src, _ = row_sum(rowptr_t, ds[perm])
    dh = spmm(rowptr_t, col_t, alpha[perm], dout)
    dh += np.outer(da_src, np.asarray(att_src, dtype=np.float64)) + np.outer(da_dst, np.asarray(att_dst, dtype=np.float64))
    return dh @ W, dh.T @ x, h.T @ da_src, h.T @ da_dst, dout.sum(0)
