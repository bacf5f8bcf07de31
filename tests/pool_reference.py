"""Plain float64 NumPy statements of the graph-level pooling kernels of csrc/lift_pool.hip and of fitgnn_sum_leading_f32
(csrc/gcn_ops.hip) (test infrastructure only): segment sum / max and their backward forms, the mean pool fused with a narrow head,
and the sum over a leading axis.

A segment index is (off, members): segment s holds the rows members[off[s]:off[s + 1]] of X, in that order (members None: the rows
off[s] ... off[s + 1] - 1 themselves).  Rows may repeat and need not be sorted.  Each helper returns the float64 result of the
kernel's operation; every operation here is a sum of products, so the per-entry condition sum |terms| a tolerance needs is the
same helper on the absolute values of its inputs.
tests/test_pool_reference_cpu.py checks them against torch's own float64 operations and autograd.
"""
import numpy as np


def _rows(off, members, s):
    m0, m1 = int(off[s]), int(off[s + 1])
    return np.arange(m0, m1, dtype=np.int64) if members is None else np.asarray(members, dtype=np.int64)[m0:m1]


def segment_sum(off, members, X):
    """out[s] = sum of the segment's rows of X (an empty segment: zeros).  Its condition sum |terms| is segment_sum(off, members,
    |X|)."""
    X = np.asarray(X, dtype=np.float64)
    n_seg = len(off) - 1
    out = np.zeros((n_seg, X.shape[1]))
    for s in range(n_seg):
        out[s] = X[_rows(off, members, s)].sum(0)
    return out


def segment_max(off, members, X):
    """(out, arg): out[s][c] = max over the segment's rows of X[row][c], arg[s][c] = the first member, in segment order, that holds
    it.  An empty segment gives -inf and -1; a column in which every member is -inf gives -inf and the first member; a NaN anywhere
    in a segment's column gives NaN and the first NaN member (torch's amax propagates NaN from any position)."""
    X = np.asarray(X, dtype=np.float64)
    n_seg, F = len(off) - 1, X.shape[1]
    out = np.full((n_seg, F), -np.inf)
    arg = np.full((n_seg, F), -1, dtype=np.int64)
    cols = np.arange(F)
    for s in range(n_seg):
        r = _rows(off, members, s)
        if r.size == 0:
            continue
        v = X[r]                                   # [members x F]
        nan = np.isnan(v)
        has_nan = nan.any(0)
        best = np.where(nan, -np.inf, v).max(0)
        first_max = np.argmax(np.where(nan, -np.inf, v) == best[None, :], axis=0)   # argmax of a bool: its first True
        first_nan = np.argmax(nan, axis=0)
        pos = np.where(has_nan, first_nan, first_max)
        out[s] = np.where(has_nan, np.nan, best)
        arg[s] = r[pos]
        assert np.all(np.isnan(out[s]) | (v[pos, cols] == out[s]))
    return out, arg


def segment_max_bwd(g, arg, n_rows):
    """dst [n_rows x F], zero except dst[arg[s][c]][c] = g[s][c] where arg[s][c] >= 0.  The (row, column) pairs must be distinct
    (disjoint segments): the kernel stores, it does not add."""
    g, arg = np.asarray(g, dtype=np.float64), np.asarray(arg, dtype=np.int64)
    dst = np.zeros((n_rows, g.shape[1]))
    s, c = np.nonzero(arg >= 0)
    flat = arg[s, c] * g.shape[1] + c
    assert np.unique(flat).size == flat.size, "segment_max_bwd: an element is the maximum of two segments"
    dst[arg[s, c], c] = g[s, c]
    return dst


def segment_expand(src, seg_of_row, scale):
    """dst[r] = scale[seg] * src[seg] for seg = seg_of_row[r] >= 0 (scale None: 1), a row of zeros otherwise."""
    src, seg = np.asarray(src, dtype=np.float64), np.asarray(seg_of_row, dtype=np.int64)
    dst = np.zeros((seg.size, src.shape[1]))
    live = seg >= 0
    w = np.ones(src.shape[0]) if scale is None else np.asarray(scale, dtype=np.float64)
    dst[live] = src[seg[live]] * w[seg[live]][:, None]
    return dst


def pool_head(off, members, X, inv_cnt, W, b):
    """(pooled, y): pooled[s] = inv_cnt[s] * (sum of the segment's rows), y = pooled W^T + b (b None: 0).  With |X|, |inv_cnt|, |W|
    and |b| as arguments it returns the two conditions sum |terms|."""
    pooled = segment_sum(off, members, X) * np.asarray(inv_cnt, dtype=np.float64)[:, None]
    W = np.asarray(W, dtype=np.float64)
    bb = np.zeros(W.shape[0]) if b is None else np.asarray(b, dtype=np.float64)
    return pooled, pooled @ W.T + bb


def pool_head_bwd(dy, W, pooled, seg_of_row, inv_cnt):
    """The backward of pool_head for a loss with d loss / d y = dy: dx[r] = inv_cnt[s] * (dy[s] W) for a row of segment
    s = seg_of_row[r] >= 0, zeros otherwise (each row belongs to at most one segment, once); dW = dy^T pooled; db = column sums of
    dy.  Returns (dx, dW, db); with |dy|, |W|, |pooled| and |inv_cnt| as arguments, their conditions sum |terms|."""
    dy, W, pooled = (np.asarray(a, dtype=np.float64) for a in (dy, W, pooled))
    seg = np.asarray(seg_of_row, dtype=np.int64)
    per_seg = (dy @ W) * np.asarray(inv_cnt, dtype=np.float64)[:, None]
    dx = np.zeros((seg.size, W.shape[1]))
    live = seg >= 0
    dx[live] = per_seg[seg[live]]
    return dx, dy.T @ pooled, dy.sum(0)


def sum_leading(part):
    """out = part.sum(0) for part [B x W] (its condition: sum_leading(|part|))."""
    return np.asarray(part, dtype=np.float64).sum(0)
