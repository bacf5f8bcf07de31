"""Plain float64 NumPy statements of the APPNP propagation kernels of csrc/gat.hip (test infrastructure only): the narrow SpMM with
its teleport / accumulate epilogue, the K-step recurrence forward and backward, and the gather into the padded layout -- vectorised
(np.add.reduceat), so a 65 000-row case costs milliseconds.

A pattern is (rowptr, col, val): row r holds the entries rowptr[r] ... rowptr[r + 1] - 1; a row may be empty, columns may repeat.
val is what the kernel receives (float32), taken to float64 exactly.  alpha is the float32 the kernel receives; the kernels form
1.0f - alpha in fp32, so beta = float64(float32(1) - float32(alpha)) (`beta_of`).

The propagation helpers return (result, bound): bound is the per-entry error bound of a kernel that rounds row r's sum k_r[r] times
per step, carried through the steps (u = 2^-24):
  forward    b_0 = 0,   b_{k+1} = beta |A| b_k + k_r u (beta |A| |z_k| + alpha |z_0|)
             (k_r counts the fused adds of the row's sum on its longest path, the beta product and the teleport fma)
  backward   g: c_0 = 0, c_{k+1} = beta |A^T| c_k + (k_r - 1) u beta |A^T| |g_k|          (no teleport fma)
             S_k = alpha sum_{j<k} g_j, formed by one fma per step:  d_{k+1} = d_k + alpha c_k + u alpha sum_{j<=k} |g_j|
             result S_K + g_K (one more addition):  d_K + c_K + u (alpha sum_{j<K} |g_j| + |g_K|)
k_r = None gives a zero bound.

The EXACT generator (`make_csr(..., exact=True)`, `exact_signal`, alpha = 0.5): signal entries are integers in [-8, 8] over 8 (3
fraction bits), val[e] = +- 2^-ceil(log2(len(row))), so sum_e |val[e]| <= 1 in every row and with alpha = beta = 0.5 the signal's
magnitude never exceeds 1; a step adds at most ceil(log2 len) + 1 fraction bits.  Multiples of 2^-24 of magnitude <= 1 are fp32
numbers, so K steps over rows of at most len entries are exact in fp32 -- in ANY summation order -- while 3 + K (ceil(log2 len) + 1)
<= 24: K = 1 up to 2^20 entries, K = 2 up to 512, K = 3 up to 64 (`exact_cap`).  tests/test_appnp_reference_cpu.py evaluates every
(row lengths, K) the GPU tests use in fp32 in three orders and requires the float64 result bit for bit.
"""
import numpy as np

U = 2.0 ** -24


def alpha_of(alpha):
    return float(np.float32(alpha))


def beta_of(alpha):
    """1.0f - alpha as the kernels form it."""
    return float(np.float32(1.0) - np.float32(alpha))


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def spmv(rowptr, col, val, X):
    """A X in float64 (an empty row: zeros)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    X = _f64(X)
    n = len(rowptr) - 1
    out = np.zeros((n, X.shape[1]))
    if rowptr[-1] == 0:
        return out
    e0, e1 = rowptr[0], rowptr[-1]
    terms = _f64(val)[e0:e1, None] * X[np.asarray(col, dtype=np.int64)[e0:e1]]
    full = np.diff(rowptr) > 0
    out[full] = np.add.reduceat(terms, rowptr[:-1][full] - e0, axis=0)   # (the starts of the non-empty rows bound each other's segments)
    return out


def spmm_affine(rowptr, col, val, X, beta, Z0=None, gamma=0.0):
    """Y = beta (A X) + gamma Z0  (fitgnn_spmm_narrow_f32 / _padded_f32; Z0 None: no second term).  Its condition sum |terms| is
    the same helper on |val|, |X|, |Z0| with |beta|, |gamma|."""
    Y = beta * spmv(rowptr, col, val, X)
    return Y if Z0 is None else Y + gamma * _f64(Z0)


def accumulate(ACC, delta, X):
    """ACC + delta X: the accumulate form of the same launch (the backward's running alpha-sum)."""
    return _f64(ACC) + delta * _f64(X)


def _kvec(k_r, n, minus=0):
    if k_r is None:
        return np.zeros((n, 1))
    return np.maximum(_f64(k_r).reshape(n, 1) - minus, 0.0)


def appnp_forward(rowptr, col, val, X, K, alpha, k_r=None):
    """(z_K, bound) of z_{k+1} = beta A z_k + alpha z_0, z_0 = X."""
    a, b = alpha_of(alpha), beta_of(alpha)
    z0 = _f64(X)
    n = len(rowptr) - 1
    aval = np.abs(_f64(val))
    k = _kvec(k_r, n)
    z, bound = z0, np.zeros_like(z0)
    for _ in range(K):
        cond = b * spmv(rowptr, col, aval, np.abs(z)) + a * np.abs(z0)
        bound = b * spmv(rowptr, col, aval, bound) + k * U * cond
        z = b * spmv(rowptr, col, val, z) + a * z0
    return z, bound


def appnp_backward(rowptr_t, col_t, val_t, G, K, alpha, k_r=None):
    """(alpha sum_{k<K} g_k + g_K, bound) with g_0 = G, g_{k+1} = beta A^T g_k; the pattern handed in IS A^T."""
    a, b = alpha_of(alpha), beta_of(alpha)
    g = _f64(G)
    n = len(rowptr_t) - 1
    aval = np.abs(_f64(val_t))
    k = _kvec(k_r, n, minus=1)
    S, absS = np.zeros_like(g), np.zeros_like(g)
    c, d = np.zeros_like(g), np.zeros_like(g)
    for _ in range(K):
        absS = absS + a * np.abs(g)
        d = d + a * c + U * absS
        S = S + a * g
        c = b * spmv(rowptr_t, col_t, aval, c) + k * U * b * spmv(rowptr_t, col_t, aval, np.abs(g))
        g = b * spmv(rowptr_t, col_t, val_t, g)
    if K == 0:
        return g.copy(), np.zeros_like(g)
    return S + g, d + c + U * (absS + np.abs(g))


def gather_rows_padded(src, index, h4):
    """dst[r] = src[index[r]] (index None: src[r]) followed by zeros up to 4 h4 columns."""
    src = _f64(src)
    rows = src if index is None else src[np.asarray(index, dtype=np.int64)]
    out = np.zeros((rows.shape[0], 4 * h4))
    out[:, :src.shape[1]] = rows
    return out


def transpose(rowptr, col, val, n_cols=None):
    """The pattern of A^T (entries of a row in ascending source-row order)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    n_cols = n if n_cols is None else n_cols
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    col = np.asarray(col, dtype=np.int64)
    order = np.argsort(col, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_cols))])
    return rp.astype(np.int32), rows[order].astype(np.int32), np.asarray(val)[order]


# ---------------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------------
def exact_cap(K):
    """Longest row the EXACT generator may hold at K steps: 3 + K (ceil(log2 len) + 1) <= 24."""
    if K <= 1:
        return 1 << 20
    return 1 << ((24 - 3) // K - 1)


def cap_lengths(lengths, K):
    """The row lengths of an EXACT case at K steps: rows beyond exact_cap(K) are cut to it (300 -> 64 at K = 3)."""
    return np.minimum(np.asarray(lengths, dtype=np.int64), exact_cap(K))


def make_csr(rng, lengths, ranges=None, exact=False):
    """(rowptr int32, col int32, val float32) with the given row lengths.  ranges [m, 2]: every row inside a range [r0, r1) draws its
    columns from that range (a closed diagonal block), with repeats; rows outside every range, or ranges None: from [0, n).
    exact: val = +- 2^-ceil(log2 len); else normal / sqrt(len)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = len(lengths)
    lo, hi = np.zeros(n, dtype=np.int64), np.full(n, n, dtype=np.int64)
    if ranges is not None:
        for r0, r1 in np.asarray(ranges, dtype=np.int64).reshape(-1, 2):
            lo[r0:r1], hi[r0:r1] = r0, r1
    rowptr = np.concatenate([[0], np.cumsum(lengths)])
    rows = np.repeat(np.arange(n), lengths)
    col = lo[rows] + np.floor(rng.random(len(rows)) * (hi - lo)[rows]).astype(np.int64)
    ln = np.maximum(lengths[rows], 1)
    if exact:
        val = rng.choice([-1.0, 1.0], size=len(rows)) * 2.0 ** -np.ceil(np.log2(ln))
    else:
        val = rng.normal(size=len(rows)) / np.sqrt(ln)
    return rowptr.astype(np.int32), col.astype(np.int32), val.astype(np.float32)


def exact_signal(rng, shape):
    """Integers in [-8, 8] over 8."""
    return (rng.integers(-8, 9, size=shape) / 8.0).astype(np.float32)


EXACT_ALPHA = 0.5

# the row-length lists of the GPU module's EXACT cases (name -> lengths); G-dependent lists are made by per_step_lengths
SHORT_LDS = [0, 1, 2, 3, 4, 5, 6, 15, 16]
LONG_LDS = [17, 24, 32, 33, 40, 41, 300]
UNIT_LENGTHS = [0, 1, 3, 4, 5, 8, 9, 300]
NARROW_LENGTHS = [0, 1, 9, 300]


def per_step_lengths(G):
    """The row lengths of the per-step kernel's branches: the row's own lanes take the first 8 entries, the G slots the rest."""
    return [0, 1, 7, 8, 9, 8 + G - 1, 8 + G, 8 + G + 1, 8 + 2 * G + 1, 300]


def exact_cases():
    """(name, lengths, K) of every EXACT evaluation the GPU module makes: the CPU module proves each exact."""
    out = []
    for K in (1, 2, 3):
        for name, ln in (("lds", SHORT_LDS + LONG_LDS), ("units", UNIT_LENGTHS)):
            out.append((name, cap_lengths(ln, K), K))
        for G in (64, 21, 5, 4):
            out.append((f"step-G{G}", cap_lengths(per_step_lengths(G), K), K))
    out.append(("narrow", np.asarray(NARROW_LENGTHS), 1))
    out.append(("k1-1000", np.asarray([1000, 1, 0, 5]), 1))
    out.append(("k2-300", np.asarray([300, 1, 0, 5]), 2))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 evaluation in a chosen order (the CPU module's proof that the EXACT generator is exact)
# ---------------------------------------------------------------------------------------------------------------------------------
def _row_sums_f32(rowptr, col, val, Z, order):
    """sum_e val[e] Z[col[e]] per row, every product and addition rounded to fp32, entries taken in `order`: 'csr', 'reverse', or
    'slots' (eight running sums over every eighth entry, folded as a tree)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    lens = np.diff(rowptr)
    f = np.float32
    Z = Z.astype(f)
    val = np.asarray(val, dtype=f)
    col = np.asarray(col, dtype=np.int64)
    n_slots = 8 if order == "slots" else 1
    acc = np.zeros((n_slots, n, Z.shape[1]), dtype=f)
    for j in range(int(lens.max()) if n else 0):
        rows = np.nonzero(lens > j)[0]
        e = rowptr[rows] + (lens[rows] - 1 - j if order == "reverse" else j)
        term = (val[e][:, None] * Z[col[e]]).astype(f)
        s = j % n_slots
        acc[s, rows] = (acc[s, rows] + term).astype(f)
    while acc.shape[0] > 1:
        h = acc.shape[0] // 2
        acc = (acc[:h] + acc[h:]).astype(f)
    return acc[0]


def appnp_forward_f32(rowptr, col, val, X, K, alpha, order="csr"):
    f = np.float32
    a, b = f(alpha), f(1.0) - f(alpha)
    z0 = np.asarray(X, dtype=f)
    z = z0
    for _ in range(K):
        y = (b * _row_sums_f32(rowptr, col, val, z, order)).astype(f)
        z = ((a * z0).astype(f) + y).astype(f)
    return z


def appnp_backward_f32(rowptr_t, col_t, val_t, G, K, alpha, order="csr"):
    f = np.float32
    a, b = f(alpha), f(1.0) - f(alpha)
    g = np.asarray(G, dtype=f)
    S = np.zeros_like(g)
    for _ in range(K):
        S = (S + (a * g).astype(f)).astype(f)
        g = (b * _row_sums_f32(rowptr_t, col_t, val_t, g, order)).astype(f)
    return (S + g).astype(f)
