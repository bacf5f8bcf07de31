"""Plain NumPy statements of the Lanczos-step kernels of csrc/lanczos.hip (test infrastructure only), with every sum formed in
np.longdouble and the results returned as float64 (the nearest double of the extended sum).  The per-entry condition sum |terms| a
tolerance needs is the same helper on the absolute values of its inputs.

The basis is column-major as in the kernels: V [ncol x n], row c = basis vector c.
tests/test_lanczos_reference_cpu.py checks that steps composed of these helpers keep V^T V = I and V T V^T = H.
"""
import numpy as np

LD = np.longdouble


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _d(a):
    return np.asarray(a, dtype=np.float64)


def spmv(rowptr, col, val, x, alpha, beta):
    """y = alpha (A x) + beta x for a CSR matrix (columns in any order, repeats added).  Its condition sum |terms| is the same
    call on |val|, |x|, |alpha| and |beta|."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = rowptr.size - 1
    x, val = _ld(x), _ld(val)
    prod = val * x[col] if col.size else np.zeros(0, dtype=LD)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    ax = np.zeros(n, dtype=LD)
    np.add.at(ax, row, prod)
    return _d(LD(alpha) * ax + LD(beta) * x)


def dots(V, w):
    """(h, |w|^2, h_cond): h[c] = sum_i V[c][i] w[i], h_cond[c] = sum_i |V[c][i] w[i]|."""
    V, w = _ld(V), _ld(w)
    return _d(V @ w), float(w @ w), _d(np.abs(V) @ np.abs(w))


def project(V, w, h_in):
    """One projection pass: w_new = w - sum_c V[c] h_in[c] (h_in None: w_new = w), h = V w_new, |w_new|^2.  Returns
    (w_new, h, |w_new|^2); h and |w_new|^2 are those of the float64 w_new.  The condition of the subtraction,
    sum_c |V[c][i] h_in[c]|, is project_cond(V, h_in)."""
    w_new = _d(w) if h_in is None else _d(_ld(w) - _ld(h_in) @ _ld(V))
    h, nrm2, _ = dots(V, w_new)
    return w_new, h, nrm2


def project_cond(V, h_in):
    return np.zeros(np.asarray(V).shape[1]) if h_in is None else _d(np.abs(_ld(h_in)) @ np.abs(_ld(V)))


def reduce_parts(part):
    """Column sums of the partial rows part [n_part x ncol1] (no rows: zeros)."""
    return _d(_ld(part).sum(0))


def finish(w, ha, hb, nrm2, j):
    """(v_next, H column, beta): beta = sqrt(nrm2), v_next = w / max(beta, 1e-300), H column = [ha[c] + hb[c] for c <= j] followed
    by beta (j + 2 entries)."""
    beta = float(np.sqrt(LD(nrm2)))
    v = _d(_ld(w) / LD(max(beta, 1e-300)))
    col = np.concatenate([_d(ha)[:j + 1] + _d(hb)[:j + 1], [beta]])   # one IEEE double addition each: exactly the kernel's
    return v, col, beta


def rotate(V, S):
    """out[c] = sum_j S[j][c] V[j] (V [m x n], S [m x nk]); its condition is rotate(|V|, |S|)."""
    return _d(_ld(S).T @ _ld(V))


def lanczos_step(rowptr, col, val, V, j, alpha, beta):
    """One full step in the kernels' order: w = T V[j]; h = V w; w -= V^T h, h2 = V w; w -= V^T h2, |w|^2; finish.  V holds the
    vectors 0 ... j.  Returns (v_next, H column (j + 2 entries), w after both passes, (h, h2))."""
    Vj = _d(V)[:j + 1]
    w = spmv(rowptr, col, val, Vj[j], alpha, beta)
    _, h, _ = project(Vj, w, None)
    w, h2, _ = project(Vj, w, h)
    w, _, nrm2 = project(Vj, w, h2)
    v, colH, _ = finish(w, h, h2, nrm2, j)
    return v, colH, w, (h, h2)
