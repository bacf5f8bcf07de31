"""The float64 references of tests/appnp_reference.py against a dense torch float64 recurrence, autograd (the adjoint identity) and
oracle.gnn_oracle.appnp (CPU); the EXACT generator evaluated in fp32 in three summation orders at every (row lengths, K) the GPU
module (tests/test_gpu_appnp_kernels.py) uses it at; and hand-written tiny cases.  The references the GPU kernel tests trust are
themselves checked here."""
import numpy as np
import pytest
import torch

import appnp_reference as ar

D = torch.float64


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_allclose(a, b, rtol=tol, atol=tol)


def _dense(rowptr, col, val, n_cols=None):
    n = len(rowptr) - 1
    A = torch.zeros(n, n if n_cols is None else n_cols, dtype=D)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    A.index_put_((torch.from_numpy(rows), torch.from_numpy(col.astype(np.int64))), torch.from_numpy(val.astype(np.float64)), accumulate=True)
    return A


def _recurrence(A, z0, K, alpha):
    a, b = ar.alpha_of(alpha), ar.beta_of(alpha)
    z = z0
    for _ in range(K):
        z = b * (A @ z) + a * z0
    return z


LENGTHS = [0, 1, 3, 4, 5, 17, 0, 40, 9, 2]


@pytest.mark.parametrize("K", [0, 1, 2, 10])
@pytest.mark.parametrize("alpha", [0.1, 0.15, 0.5])
def test_forward_and_backward_against_the_dense_recurrence_and_autograd(K, alpha):
    rng = np.random.default_rng(K)
    rowptr, col, val = ar.make_csr(rng, LENGTHS * 3)
    n = len(rowptr) - 1
    A = _dense(rowptr, col, val)
    X = rng.normal(size=(n, 5))
    z0 = torch.from_numpy(X).requires_grad_(True)
    z = _recurrence(A, z0, K, alpha)
    got, bound = ar.appnp_forward(rowptr, col, val, X, K, alpha)
    _close(got, z.detach().numpy())
    assert np.all(bound == 0)
    # the adjoint: d <w, z_K> / d z_0 is the backward recurrence with A^T on w
    w = rng.normal(size=(n, 5))
    (z * torch.from_numpy(w)).sum().backward()
    rp_t, col_t, val_t = ar.transpose(rowptr, col, val)
    _close(_dense(rp_t, col_t, val_t).numpy(), A.t().numpy())
    back, _ = ar.appnp_backward(rp_t, col_t, val_t, w, K, alpha)
    _close(back, z0.grad.numpy())


def test_spmm_affine_accumulate_and_gather():
    rng = np.random.default_rng(7)
    rowptr, col, val = ar.make_csr(rng, LENGTHS)
    n = len(LENGTHS)
    A = _dense(rowptr, col, val).numpy()
    X, Z0, ACC = (rng.normal(size=(n, 6)) for _ in range(3))
    _close(ar.spmv(rowptr, col, val, X), A @ X)
    _close(ar.spmm_affine(rowptr, col, val, X, 0.9, Z0, 0.1), 0.9 * (A @ X) + 0.1 * Z0)
    _close(ar.spmm_affine(rowptr, col, val, X, 0.9), 0.9 * (A @ X))
    _close(ar.accumulate(ACC, 0.1, X), ACC + 0.1 * X)
    idx = np.array([3, 3, 0, 9, 1])
    out = ar.gather_rows_padded(X, idx, 2)
    assert out.shape == (5, 8) and np.array_equal(out[:, :6], X[idx]) and np.all(out[:, 6:] == 0)
    assert np.array_equal(ar.gather_rows_padded(X, None, 2)[:, :6], X)


def test_against_the_oracle_on_a_gcn_normalised_graph():
    from oracle import gnn_oracle as gorc

    rng = np.random.default_rng(3)
    n = 60
    i = np.arange(n)
    extra = rng.integers(0, n, size=(2, 40))
    extra = extra[:, extra[0] != extra[1]]
    src = np.concatenate([i, (i + 1) % n, extra[0], extra[1]])
    dst = np.concatenate([(i + 1) % n, i, extra[1], extra[0]])
    und = np.unique(np.stack([src, dst], 1), axis=0)
    ei = torch.from_numpy(und.T.copy())
    x = torch.from_numpy(rng.normal(size=(n, 7)))
    want = gorc.appnp(x, ei, 10, 0.1)                         # float64 throughout, alpha the Python double
    row, colt, w = gorc.gcn_norm(ei, n, D)                     # row = source, col = target
    order = np.argsort(colt.numpy(), kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(colt.numpy(), minlength=n))])
    got, _ = ar.appnp_forward(rowptr, row.numpy()[order], w.numpy()[order].astype(np.float32), x.numpy(), 10, 0.1)
    # fp32 weights and the fp32 alpha / beta against the oracle's doubles: 1e-7 relative per step
    np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=2e-6 * float(want.abs().max()))


@pytest.mark.parametrize("case", ar.exact_cases(), ids=lambda c: f"{c[0]}-K{c[2]}")
def test_the_exact_generator_is_exact_in_fp32_in_any_order(case):
    name, lengths, K = case
    rng = np.random.default_rng(len(name) + K)
    lengths = np.concatenate([lengths, lengths[::-1], rng.permutation(lengths)])
    n = len(lengths)
    ranges = np.array([[0, n // 2], [n // 2, n]])
    rowptr, col, val = ar.make_csr(rng, lengths, ranges, exact=True)
    assert lengths.max() <= ar.exact_cap(K)
    rows = np.repeat(np.arange(n), lengths)
    assert np.all(np.bincount(rows, weights=np.abs(val), minlength=n) <= 1.0)
    X = ar.exact_signal(rng, (n, 8))
    fwd, _ = ar.appnp_forward(rowptr, col, val, X, K, ar.EXACT_ALPHA)
    bwd, _ = ar.appnp_backward(rowptr, col, val, X, K, ar.EXACT_ALPHA)
    assert np.abs(fwd).max() <= 1.0 and np.abs(bwd).max() <= 1.0
    assert np.array_equal(fwd * 2.0 ** 24, np.round(fwd * 2.0 ** 24))   # multiples of 2^-24 of magnitude <= 1: fp32 numbers
    for order in ("csr", "reverse", "slots"):
        f32 = ar.appnp_forward_f32(rowptr, col, val, X, K, ar.EXACT_ALPHA, order)
        assert f32.dtype == np.float32 and np.array_equal(f32.astype(np.float64), fwd), (order, "forward")
        b32 = ar.appnp_backward_f32(rowptr, col, val, X, K, ar.EXACT_ALPHA, order)
        assert np.array_equal(b32.astype(np.float64), bwd), (order, "backward")


def test_fp32_orders_differ_on_random_input():
    """The three orders are different evaluations: on RANDOM values they do not agree bit for bit (so their agreement above means
    something), and each stays within the propagated bound."""
    rng = np.random.default_rng(11)
    lengths = np.array([40, 300, 17, 5] * 4)
    rowptr, col, val = ar.make_csr(rng, lengths)
    X = rng.normal(size=(len(lengths), 4)).astype(np.float32)
    k_r = lengths + 2 + 3
    ref, bound = ar.appnp_forward(rowptr, col, val, X, 3, 0.1, k_r)
    res = [ar.appnp_forward_f32(rowptr, col, val, X, 3, 0.1, o) for o in ("csr", "reverse", "slots")]
    assert not np.array_equal(res[0], res[1]) and not np.array_equal(res[0], res[2])
    for r in res:
        assert np.all(np.abs(r - ref) <= bound)


def test_tiny_cases_by_hand():
    # rows: 0 -> {1: 0.5, 2: -0.25}; 1 -> {} (empty); 2 -> {2: 1.0}
    rowptr, col, val = np.array([0, 2, 2, 3]), np.array([1, 2, 2]), np.array([0.5, -0.25, 1.0], dtype=np.float32)
    X = np.array([[1.0], [2.0], [4.0]])
    a, b = 0.5, 0.5
    z1 = np.array([[b * (0.5 * 2 - 0.25 * 4) + a * 1], [a * 2], [b * 4 + a * 4]])
    _close(ar.appnp_forward(rowptr, col, val, X, 1, 0.5)[0], z1)
    z2 = np.array([[b * (0.5 * z1[1, 0] - 0.25 * z1[2, 0]) + a * 1], [a * 2], [b * z1[2, 0] + a * 4]])
    _close(ar.appnp_forward(rowptr, col, val, X, 2, 0.5)[0], z2)
    # an empty row: alpha z_0 forward, alpha g_0 backward, for every K >= 1
    for K in (1, 2, 5):
        assert ar.appnp_forward(rowptr, col, val, X, K, 0.1)[0][1, 0] == ar.alpha_of(0.1) * 2.0
        assert ar.appnp_backward(rowptr, col, val, X, K, 0.1)[0][1, 0] == ar.alpha_of(0.1) * 2.0
    # K = 0: the input itself, both ways, with a zero bound
    for fn in (ar.appnp_forward, ar.appnp_backward):
        out, bound = fn(rowptr, col, val, X, 0, 0.1, np.array([4, 2, 3]))
        assert np.array_equal(out, X) and np.all(bound == 0)
    # backward by hand at K = 1: alpha g_0 + beta M g_0
    g1 = np.array([[b * (0.5 * 2 - 0.25 * 4)], [0.0], [b * 4]])
    _close(ar.appnp_backward(rowptr, col, val, X, 1, 0.5)[0], a * X + g1)
    # a one-row graph with a self entry: z_K = (beta v)^K x + alpha x sum_{j<K} (beta v)^j
    rp1, c1, v1 = np.array([0, 1]), np.array([0]), np.array([0.5], dtype=np.float32)
    q = ar.beta_of(0.25) * 0.5
    want = q ** 3 * 3.0 + 0.25 * 3.0 * (1 + q + q * q)
    _close(ar.appnp_forward(rp1, c1, v1, np.array([[3.0]]), 3, 0.25)[0], [[want]])
    _close(ar.appnp_backward(rp1, c1, v1, np.array([[3.0]]), 3, 0.25)[0], [[want]])   # (a 1 x 1 matrix is its own transpose)
    # beta is formed in fp32
    assert ar.beta_of(0.1) == float(np.float32(1.0) - np.float32(0.1)) and ar.beta_of(0.1) != 1.0 - 0.1


def test_the_bound_grows_with_the_roundings_and_the_steps():
    rng = np.random.default_rng(5)
    lengths = np.array(LENGTHS)
    rowptr, col, val = ar.make_csr(rng, lengths)
    X = rng.normal(size=(len(lengths), 3))
    _, b1 = ar.appnp_forward(rowptr, col, val, X, 1, 0.1, lengths + 2)
    _, b2 = ar.appnp_forward(rowptr, col, val, X, 2, 0.1, lengths + 2)
    cond = ar.spmm_affine(rowptr, col, np.abs(val), np.abs(X), ar.beta_of(0.1), np.abs(X), ar.alpha_of(0.1))
    _close(b1, (lengths + 2)[:, None] * ar.U * cond)
    assert np.all(b2 >= b1 * 0) and np.all(b2[lengths > 0] > 0)
    _, c1 = ar.appnp_backward(rowptr, col, val, X, 1, 0.1, lengths + 2)
    # one step back: (k - 1) roundings on beta M g_0, one on alpha g_0, one on the final addition
    g1c = ar.beta_of(0.1) * ar.spmv(rowptr, col, np.abs(val), np.abs(X))
    g1 = np.abs(ar.beta_of(0.1) * ar.spmv(rowptr, col, val, X))
    _close(c1, (lengths + 1)[:, None] * ar.U * g1c + ar.U * ar.alpha_of(0.1) * np.abs(X) + ar.U * (ar.alpha_of(0.1) * np.abs(X) + g1))
