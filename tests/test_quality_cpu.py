"""CPU tier for coarsening_quality: the quality entry points are exported, refuse bad arguments and undersized workspaces without
touching the GPU, and coarsening_quality raises its documented errors before any device work."""
import numpy as np
import pytest
import scipy.sparse as sp

from fitgnn_amd import _lib, coarsening

QUALITY = ("fitgnn_coarse_laplacian", "fitgnn_coarse_laplacian_workspace_bytes", "fitgnn_project_lift_f64",
           "fitgnn_project_lift_workspace_bytes", "fitgnn_laplacian_gram_f64", "fitgnn_laplacian_gram_workspace_bytes",
           "fitgnn_cross_atb_f64", "fitgnn_cross_atb_workspace_bytes")

FAKE = 0x1000  # never dereferenced: every call below is refused on its arguments first
BAD, WS = -1, -2


def test_quality_symbols_exported():
    L = _lib.lib()
    for name in QUALITY:
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
    assert hasattr(coarsening, "coarsening_quality")
    assert _lib.QUALITY_MAX_K == 64


def test_workspace_queries():
    L = _lib.lib()
    assert L.fitgnn_coarse_laplacian_workspace_bytes(100, 400, 50) > 100 * 8 + 400 * 8
    assert L.fitgnn_coarse_laplacian_workspace_bytes(-1, 400, 50) == 0
    assert L.fitgnn_project_lift_workspace_bytes(100, 50) >= 4 * 100 * 4
    # one k1 x k2 f64 partial per workgroup, at most 1024 workgroups
    assert L.fitgnn_laplacian_gram_workspace_bytes(10 ** 6, 30, 30) >= 1000 * 30 * 30 * 8
    assert L.fitgnn_laplacian_gram_workspace_bytes(10 ** 6, 64, 64) <= 1024 * 64 * 64 * 8 + 256
    assert L.fitgnn_laplacian_gram_workspace_bytes(100, 65, 1) == 0
    assert L.fitgnn_cross_atb_workspace_bytes(100, 7, 64) > 0
    assert L.fitgnn_cross_atb_workspace_bytes(100, 7, 65) == 0


def test_coarse_laplacian_rejects_bad_arguments():
    L = _lib.lib()
    f = L.fitgnn_coarse_laplacian
    ws = int(L.fitgnn_coarse_laplacian_workspace_bytes(10, 20, 5))
    ok = [10, FAKE, FAKE, FAKE, 20, FAKE, FAKE, FAKE, 5, FAKE, FAKE, FAKE, FAKE, FAKE, ws, None]
    for i, bad in ((0, -1), (4, -1), (8, -1), (1, None), (2, None), (5, None), (6, None), (7, None), (9, None), (10, None), (11, None),
                   (12, None)):
        a = list(ok)
        a[i] = bad
        assert f(*a) == BAD, (i, bad)
    a = list(ok)
    a[14] = ws - 1
    assert f(*a) == WS
    a = list(ok)
    a[13] = None
    assert f(*a) == WS


def test_project_lift_rejects_bad_arguments():
    L = _lib.lib()
    f = L.fitgnn_project_lift_f64
    ws = int(L.fitgnn_project_lift_workspace_bytes(10, 5))
    ok = [FAKE, FAKE, 10, 5, FAKE, 7, 7, FAKE, 7, FAKE, 7, FAKE, ws, None]
    for i, bad in ((2, -1), (3, -1), (6, -1), (6, 65), (0, None), (1, None), (4, None), (7, None), (5, 6), (8, 6), (10, 6)):
        a = list(ok)
        a[i] = bad
        if i == 6 and bad == 65:
            a[5] = a[8] = a[10] = 65
        assert f(*a) == BAD, (i, bad)
    a = list(ok)
    a[12] = ws - 1
    assert f(*a) == WS


def test_gram_and_cross_reject_bad_arguments():
    L = _lib.lib()
    g = L.fitgnn_laplacian_gram_f64
    ws = int(L.fitgnn_laplacian_gram_workspace_bytes(100, 30, 30))
    ok = [FAKE, FAKE, FAKE, FAKE, 100, FAKE, 30, 30, FAKE, 30, 30, FAKE, 30, FAKE, ws, None]
    for i, bad in ((4, -1), (7, -1), (10, -1), (7, 65), (10, 65), (0, None), (1, None), (3, None), (5, None), (8, None), (11, None),
                   (6, 29), (9, 29), (12, 29)):
        a = list(ok)
        a[i] = bad
        if bad == 65:
            a[i - 1] = 65
            a[12] = 65
        assert g(*a) == BAD, (i, bad)
    a = list(ok)
    a[14] = ws - 1
    assert g(*a) == WS
    x = L.fitgnn_cross_atb_f64
    ws = int(L.fitgnn_cross_atb_workspace_bytes(100, 7, 30))
    ok = [FAKE, 7, 7, FAKE, 30, 30, 100, FAKE, 30, FAKE, ws, None]
    for i, bad in ((2, -1), (5, -1), (6, -1), (2, 65), (5, 65), (0, None), (3, None), (7, None), (1, 6), (4, 29), (8, 29)):
        a = list(ok)
        a[i] = bad
        if bad == 65:
            a[i - 1] = 65
            a[8] = 65
        assert x(*a) == BAD, (i, bad)
    a = list(ok)
    a[10] = ws - 1
    assert x(*a) == WS


def _ring(n):
    i = np.arange(n)
    W = sp.csr_matrix((np.ones(2 * n), (np.concatenate([i, (i + 1) % n]), np.concatenate([(i + 1) % n, i]))), shape=(n, n))
    return coarsening.Graph(W)


def _pair_C(N):
    a = np.arange(N) // 2
    return sp.csc_matrix((np.full(N, 1 / np.sqrt(2)), (a, np.arange(N))), shape=(N // 2, N))


def test_coarsening_quality_refuses_self_loops():
    G = _ring(20)
    W = G.W.tolil()
    W[3, 3] = 1.0
    with pytest.raises(ValueError, match="self-loops"):
        coarsening.coarsening_quality(coarsening.Graph(W.tocsr()), _pair_C(20), kmax=4, device="cpu")


def test_coarsening_quality_refuses_two_nonzeros_in_a_column():
    C = _pair_C(20).tolil()
    C[1, 0] = 0.5
    with pytest.raises(NotImplementedError, match="one non-zero per column"):
        coarsening.coarsening_quality(_ring(20), C.tocsc(), kmax=4, device="cpu")


def test_coarsening_quality_refuses_mismatched_shapes():
    with pytest.raises(ValueError, match="columns"):
        coarsening.coarsening_quality(_ring(20), _pair_C(22), kmax=4, device="cpu")


def test_coarsening_quality_device_refuses_large_kmax():
    with pytest.raises(ValueError, match="kmax"):
        coarsening.coarsening_quality(_ring(200), _pair_C(200), kmax=100, spectral="device", device="cpu")


def test_coarsening_quality_has_no_cpu_path():
    with pytest.raises(_lib.FitgnnError):
        coarsening.coarsening_quality(_ring(20), _pair_C(20), kmax=4, device="cpu")
