"""The extended-precision references of tests/lanczos_reference.py (CPU): each helper against a dense float64 statement of its
operation, and three composed steps on a 40-node path graph, which must keep the basis orthonormal and satisfy the Lanczos relation
V T V^T = H: the references the GPU kernel tests (tests/test_gpu_lanczos_kernels.py) trust are themselves checked here."""
import numpy as np

import lanczos_reference as lr


def _path_laplacian(n):
    """CSR Laplacian of the path graph on n nodes, each row's columns in descending (unsorted) order."""
    rowptr, col, val = [0], [], []
    for i in range(n):
        nb = [k for k in (i - 1, i + 1) if 0 <= k < n]
        ent = sorted([(i, float(len(nb)))] + [(k, -1.0) for k in nb], reverse=True)
        col += [c for c, _ in ent]
        val += [v for _, v in ent]
        rowptr.append(len(col))
    return np.array(rowptr), np.array(col), np.array(val)


def _dense(rowptr, col, val, n):
    A = np.zeros((n, n))
    for i in range(n):
        for e in range(rowptr[i], rowptr[i + 1]):
            A[i, col[e]] += val[e]
    return A


def test_spmv_against_the_dense_product():
    rng = np.random.default_rng(0)
    n = 23
    lens = rng.integers(0, 9, size=n)
    lens[4] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    col = rng.integers(0, n, size=rowptr[-1])      # unsorted, with repeats
    val = rng.normal(size=rowptr[-1])
    x = rng.normal(size=n)
    A = _dense(rowptr, col, val, n)
    np.testing.assert_allclose(lr.spmv(rowptr, col, val, x, -1.5, 0.75), -1.5 * (A @ x) + 0.75 * x, rtol=0, atol=1e-14)
    cond = lr.spmv(rowptr, col, np.abs(val), np.abs(x), 1.5, 0.75)
    assert np.all(cond >= np.abs(lr.spmv(rowptr, col, val, x, -1.5, 0.75)) - 1e-15) and cond[4] == 0.75 * abs(x[4])


def test_project_finish_rotate_against_dense_statements():
    rng = np.random.default_rng(1)
    V, w, h = rng.normal(size=(5, 30)), rng.normal(size=30), rng.normal(size=5)
    w0, h0, n0 = lr.project(V, w, None)
    assert np.array_equal(w0, w)
    np.testing.assert_allclose(h0, V @ w, rtol=0, atol=1e-13)
    np.testing.assert_allclose(n0, w @ w, rtol=1e-15)
    w1, h1, n1 = lr.project(V, w, h)
    np.testing.assert_allclose(w1, w - V.T @ h, rtol=0, atol=1e-13)
    np.testing.assert_allclose(h1, V @ w1, rtol=0, atol=1e-13)     # the dots are those of the UPDATED w
    np.testing.assert_allclose(n1, w1 @ w1, rtol=1e-15)
    np.testing.assert_allclose(lr.project_cond(V, h), np.abs(V).T @ np.abs(h), rtol=1e-15)
    v, colH, beta = lr.finish(w1, h0, h1, n1, 4)
    np.testing.assert_allclose(beta, np.sqrt(n1), rtol=1e-16)
    np.testing.assert_allclose(v, w1 / beta, rtol=1e-15)
    assert colH.shape == (6,) and np.array_equal(colH[:5], h0 + h1) and colH[5] == beta
    v, colH, beta = lr.finish(np.zeros(30), h0, h1, 0.0, 4)         # breakdown: a zero vector, not NaN
    assert beta == 0.0 and np.all(v == 0) and colH[5] == 0.0
    S = rng.normal(size=(5, 3))
    np.testing.assert_allclose(lr.rotate(V, S), S.T @ V, rtol=0, atol=1e-13)
    np.testing.assert_allclose(lr.reduce_parts(V), V.sum(0), rtol=0, atol=1e-14)
    assert np.array_equal(lr.reduce_parts(np.zeros((0, 4))), np.zeros(4))


def test_three_steps_on_a_path_graph_keep_the_lanczos_relation():
    n, steps = 40, 3
    rowptr, col, val = _path_laplacian(n)
    offset = 2.0 * 2.0                            # 2 max(dw): T = offset I - L
    T = offset * np.eye(n) - _dense(rowptr, col, val, n)
    rng = np.random.default_rng(2)
    V = np.zeros((steps + 1, n))
    v0 = rng.normal(size=n)
    V[0] = v0 / np.linalg.norm(v0)
    H = np.zeros((steps + 1, steps))
    for j in range(steps):
        V[j + 1], colH, w, (h, h2) = lr.lanczos_step(rowptr, col, val, V, j, -1.0, offset)
        H[:j + 2, j] = colH
        assert np.max(np.abs(h2)) < 1e-14 * offset, "the second pass of an orthonormal basis removes rounding only"
    assert np.max(np.abs(V @ V.T - np.eye(steps + 1))) <= 1e-13
    assert np.max(np.abs(V @ T @ V[:steps].T - H)) <= 1e-13
    assert np.max(np.abs(np.triu(H[:steps], 2))) <= 1e-13 and np.all(np.diag(H, -1) > 0)   # tridiagonal, positive sub-diagonal
