"""Plain float64 NumPy statements of the multi-head attention kernels of csrc/gat_heads.hip (test infrastructure only), built on
tests/gat_reference.py's single-head helpers.

Layouts as the kernels': rows of h / X / dOut are W = heads * C wide with head hd owning columns hd*C .. (hd+1)*C; per-node scores
are [n, heads]; per-entry quantities (alpha, dalpha, ds) are [nnz, heads], entry-major.  Where a tolerance needs it a helper also
returns the condition sum of |terms| of every output.  Composed into a layer (gat_heads_layer / gat_heads_layer_backward) they must
equal, at heads = 1, gat_reference.gat_layer and its backward, and at any head count the column-wise concatenation of
oracle.gnn_oracle.gat_conv on each head's slice of the parameters (tests/test_gat_heads_reference_cpu.py)."""
import numpy as np

import gat_reference as gr


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _heads_view(a, heads):
    """[n, heads * C] -> [n, heads, C]."""
    a = _f64(a)
    assert a.shape[1] % heads == 0, (a.shape, heads)
    return a.reshape(a.shape[0], heads, a.shape[1] // heads)


def scores(h, att_src, att_dst, heads):
    """a_src[i, hd] = h_i[hd slice] . att_src[hd slice], a_dst likewise, and each one's condition sum_c |h att|  (all [n, heads])."""
    h3 = _heads_view(h, heads)
    s, d = _f64(att_src).reshape(heads, -1), _f64(att_dst).reshape(heads, -1)
    return (np.einsum("nhc,hc->nh", h3, s), np.einsum("nhc,hc->nh", h3, d),
            np.einsum("nhc,hc->nh", np.abs(h3), np.abs(s)), np.einsum("nhc,hc->nh", np.abs(h3), np.abs(d)))


def edge_softmax(rowptr, col, a_src, a_dst, slope):
    """alpha[e, hd] = softmax over the row of LeakyReLU(a_src[col[e], hd] + a_dst[row(e), hd])."""
    a_src, a_dst = _f64(a_src), _f64(a_dst)
    return np.stack([gr.edge_softmax(rowptr, col, a_src[:, k], a_dst[:, k], slope) for k in range(a_src.shape[1])], axis=1)


def aggregate(rowptr, col, alpha, X, bias=None):
    """Y[i, hd*C + c] = sum_e alpha[e, hd] X[col[e], hd*C + c] (+ bias) and the condition sum_e |alpha X| (+ |bias|)."""
    alpha = _f64(alpha)
    heads = alpha.shape[1]
    X3 = _heads_view(X, heads)
    n = len(rowptr) - 1
    rows = gr.entry_rows(rowptr)
    cols = np.asarray(col, dtype=np.int64)
    terms = alpha[:, :, None] * X3[cols]                       # [nnz, heads, C]
    Y, cond = np.zeros((n,) + X3.shape[1:]), np.zeros((n,) + X3.shape[1:])
    np.add.at(Y, rows, terms)
    np.add.at(cond, rows, np.abs(terms))
    Y, cond = Y.reshape(n, -1), cond.reshape(n, -1)
    if bias is not None:
        Y, cond = Y + _f64(bias), cond + np.abs(_f64(bias))
    return Y, cond


def sddmm(rowptr, col, dout, h, heads):
    """dalpha[e, hd] = dOut[row(e), hd slice] . h[col[e], hd slice] and its condition sum_c |dOut h|  ([nnz, heads])."""
    d3, h3 = _heads_view(dout, heads), _heads_view(h, heads)
    rows = gr.entry_rows(rowptr)
    cols = np.asarray(col, dtype=np.int64)
    out, cond = np.empty((len(cols), heads)), np.empty((len(cols), heads))
    for k in range(0, len(cols), 1 << 13):
        a, b = d3[rows[k:k + (1 << 13)]], h3[cols[k:k + (1 << 13)]]
        out[k:k + (1 << 13)] = np.einsum("ehc,ehc->eh", a, b)
        cond[k:k + (1 << 13)] = np.einsum("ehc,ehc->eh", np.abs(a), np.abs(b))
    return out, cond


def softmax_bwd(rowptr, col, a_src, a_dst, alpha, dalpha, slope):
    """ds[e, hd] = alpha (dalpha - sum_k alpha_k dalpha_k) lrelu'(s) per row and head; da_dst[row, hd] = sum_e ds[e, hd]."""
    a_src, a_dst, alpha, dalpha = _f64(a_src), _f64(a_dst), _f64(alpha), _f64(dalpha)
    pairs = [gr.softmax_bwd(rowptr, col, a_src[:, k], a_dst[:, k], alpha[:, k], dalpha[:, k], slope) for k in range(alpha.shape[1])]
    return np.stack([p[0] for p in pairs], axis=1), np.stack([p[1] for p in pairs], axis=1)


def column_sum(rowptr, col, ds):
    """da_src[j, hd] = the sum of ds[e, hd] over the entries of column j (the row sum on the transposed order)."""
    ds = _f64(ds)
    n = len(rowptr) - 1
    rowptr_t, _, perm = gr.transpose(rowptr, col, n)
    return np.stack([gr.row_sum(rowptr_t, ds[perm, k])[0] for k in range(ds.shape[1])], axis=1)


def gat_heads_layer(x, W, att_src, att_dst, bias, rowptr, col, heads, concat=True, slope=0.2):
    """GATConv(in, C, heads, concat): h = x W^T [n, heads * C], alpha per head, the concatenated aggregation; concat=False takes the
    mean over the heads.  bias [heads * C] with concat, else [C] (added after the mean).  Returns out and the intermediates."""
    h = _f64(x) @ _f64(W).T
    a_s, a_d, _, _ = scores(h, att_src, att_dst, heads)
    alpha = edge_softmax(rowptr, col, a_s, a_d, slope)
    out, _ = aggregate(rowptr, col, alpha, h)
    if not concat:
        out = _heads_view(out, heads).mean(axis=1)
    if bias is not None:
        out = out + _f64(bias)
    return out, dict(h=h, a_src=a_s, a_dst=a_d, alpha=alpha)


def gat_heads_layer_backward(x, W, att_src, att_dst, rowptr, col, mid, dout, heads, concat=True, slope=0.2):
    """Gradients of gat_heads_layer as ops.GATHeadsAggregate.backward forms them: SDDMM, softmax backward, da_src as a column sum,
    dh = A_alpha^T dOut + da_src (x) att_src + da_dst (x) att_dst per head.  Returns dx, dW, datt_src, datt_dst [heads * C], dbias."""
    x, W, dout = _f64(x), _f64(W), _f64(dout)
    h, alpha = mid["h"], mid["alpha"]
    n = len(rowptr) - 1
    dbias = dout.sum(0)
    if not concat:   # the mean's adjoint: every head gets dout / heads
        dout = np.repeat(dout[:, None, :] / heads, heads, axis=1).reshape(n, -1)
    dalpha, _ = sddmm(rowptr, col, dout, h, heads)
    ds, da_dst = softmax_bwd(rowptr, col, mid["a_src"], mid["a_dst"], alpha, dalpha, slope)
    da_src = column_sum(rowptr, col, ds)
    rowptr_t, col_t, perm = gr.transpose(rowptr, col, n)
    dh, _ = aggregate(rowptr_t, col_t, alpha[perm], dout)
    att_s, att_d = _f64(att_src).reshape(heads, -1), _f64(att_dst).reshape(heads, -1)
    dh = dh + (da_src[:, :, None] * att_s[None] + da_dst[:, :, None] * att_d[None]).reshape(n, -1)
    h3 = _heads_view(h, heads)
    datt_s = np.einsum("nh,nhc->hc", da_src, h3).reshape(-1)
    datt_d = np.einsum("nh,nhc->hc", da_dst, h3).reshape(-1)
    return dh @ W, dh.T @ x, datt_s, datt_d, dbias
