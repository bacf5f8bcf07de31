"""GPU tier for coarsening_quality (coarsening_utils.py:257-351): the four quality kernels against float64 NumPy on random graphs
(bit-identical on a second launch), the end-to-end metrics against the unmodified reference (tests/golden/make_quality_golden.py)
with the spectral inputs injected, spectral='device' against a dense eigendecomposition, and one run at S-pubmed size."""
import json
import os
import time

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from fitgnn_amd import coarsening, data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def random_graph(N, avg_deg, seed):
    rng = np.random.default_rng(seed)
    E = max(1, N * avg_deg // 2)
    a, b = rng.integers(0, N, size=E), rng.integers(0, N, size=E)
    ok = a != b
    W = sp.coo_matrix((rng.uniform(0.5, 2.0, size=ok.sum()), (a[ok], b[ok])), shape=(N, N)).tocsr()
    W = W + W.T
    W.sort_indices()
    return W


def random_C(N, n, seed):
    rng = np.random.default_rng(seed)
    assign = np.concatenate([np.arange(n), rng.integers(0, n, size=N - n)])
    rng.shuffle(assign)
    cval = rng.uniform(0.2, 1.0, size=N)
    return assign.astype(np.int32), cval


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


GRAPHS = [(1, 7), (37, 7), (1000, 30), (5003, 64), (777, 1)]


@pytest.mark.parametrize("N,k", GRAPHS)
def test_kernels_against_numpy(N, k):
    W = random_graph(N, 6, seed=N)
    dw = np.ravel(W.sum(axis=0))
    n = max(1, N // 3)
    assign, cval = random_C(N, n, seed=N + 1)
    C = sp.csr_matrix((cval, (assign, np.arange(N))), shape=(n, N))
    L = sp.diags(dw) - W
    a_d, c_d = dev(assign, torch.int32), dev(cval)

    # Lc = C L C^T: structure (off-diagonal pattern of C W C^T plus the whole diagonal) and values
    Lc = coarsening.coarse_laplacian(W, dw, a_d, c_d, n)
    Lc_ref = (C @ L @ C.T).toarray()
    pat = ((C @ W @ C.T).toarray() != 0) | np.eye(n, dtype=bool)
    off = ~np.eye(n, dtype=bool)
    assert np.array_equal((Lc.toarray() != 0) & off, pat & off)
    Lc.sort_indices()
    assert np.array_equal(np.diff(Lc.indptr), pat.sum(1)), "every row holds its off-diagonal pattern and its diagonal"
    assert rel(Lc.toarray(), Lc_ref) < 1e-12
    Lc2 = coarsening.coarse_laplacian(W, dw, a_d, c_d, n)
    assert np.array_equal(Lc.data, Lc2.data) and np.array_equal(Lc.indices, Lc2.indices)

    rng = np.random.default_rng(k)
    U = rng.standard_normal((N, k))
    CU, Y = coarsening.project_lift(a_d, c_d, n, dev(U))
    CU_ref = C @ U
    assert rel(CU.cpu().numpy(), CU_ref) < 1e-12
    assert rel(Y.cpu().numpy(), C.T @ CU_ref) < 1e-12
    CU2, Y2 = coarsening.project_lift(a_d, c_d, n, dev(U))
    assert torch.equal(CU, CU2) and torch.equal(Y, Y2)

    Yh = Y.cpu().numpy()
    G = coarsening.laplacian_gram(W, dw, Y)
    G_ref = Yh.T @ (L @ Yh)
    assert rel(G.cpu().numpy(), G_ref) < 1e-12
    assert torch.equal(G, coarsening.laplacian_gram(W, dw, Y))

    B = rng.standard_normal((n, min(64, k + 3)))
    X = coarsening.cross_atb(CU, dev(B))
    assert rel(X.cpu().numpy(), CU_ref.T @ B) < 1e-12
    assert torch.equal(X, coarsening.cross_atb(CU, dev(B)))


def test_wide_operands_are_tiled():
    """k > 64 (an injected Uk wider than the kernels' 64 columns) runs as 64-column tiles."""
    N, n, k = 900, 300, 100
    W = random_graph(N, 6, seed=5)
    dw = np.ravel(W.sum(axis=0))
    assign, cval = random_C(N, n, seed=6)
    C = sp.csr_matrix((cval, (assign, np.arange(N))), shape=(n, N))
    U = np.random.default_rng(7).standard_normal((N, k))
    CU, Y = coarsening.project_lift(dev(assign, torch.int32), dev(cval), n, dev(U))
    Yh = C.T @ (C @ U)
    assert rel(Y.cpu().numpy(), Yh) < 1e-12
    assert rel(coarsening.laplacian_gram(W, dw, Y).cpu().numpy(), Yh.T @ ((sp.diags(dw) - W) @ Yh)) < 1e-12
    assert rel(coarsening.cross_atb(CU, CU).cpu().numpy(), (C @ U).T @ (C @ U)) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# end to end against the reference
# ---------------------------------------------------------------------------------------------------------------------
def quality_cases():
    with open(os.path.join(GOLDEN, "quality_manifest.json")) as f:
        return json.load(f)["cases"]


def case_id(c):
    return f"{c['name']}-r{int(round(c['r'] * 100))}-k{c['kmax']}"


def load_case(c):
    d = np.load(os.path.join(GOLDEN, f"coarsen_{c['name']}.npz"))
    q = np.load(os.path.join(GOLDEN, c["file"]))
    N = len(d["W_indptr"]) - 1
    W = sp.csr_matrix((d["W_data"], d["W_indices"], d["W_indptr"]), shape=(N, N))
    rp = f"r{int(round(c['r'] * 100)):02d}_"
    C = sp.csc_matrix((d[rp + "C_data"], d[rp + "C_indices"], d[rp + "C_indptr"]), shape=tuple(d[rp + "C_shape"]))
    p = f"{rp}k{c['kmax']}_"
    if c["inject"]:
        U, l = d["Uk"], d["lk"]
    else:
        U, l = q[p + "U"], q[p + "l"]
    return W, C, U, l, q, p


def close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    tol = np.maximum(1e-9 * np.abs(want), 1e-12)
    bad = np.abs(got - want) > tol
    assert not bad.any(), f"{what}: worst {np.abs(got - want).max():.3g} at {np.argwhere(bad)[:3].tolist()}"


@pytest.mark.parametrize("case", quality_cases(), ids=case_id)
def test_metrics_match_the_reference(case):
    W, C, U, l, q, p = load_case(case)
    l_in = l.copy()
    met = coarsening.coarsening_quality(coarsening.Graph(W), C, kmax=case["kmax"], Uk=U, lk=l_in, Uc=q[p + "Uc"], lc=q[p + "lc"])
    assert np.array_equal(l_in, l), "the caller's lk is not modified"
    assert met["r"] == float(q[p + "r"])
    assert met["m"] == int(q[p + "m"])
    for k in ("error_eigenvalue", "angle_matrix", "error_subspace", "error_sintheta"):
        close(met[k], q[p + k], k)


def test_coarsening_matrix_input_and_arpack_path():
    """A CoarseningMatrix from coarsen() is accepted, and the arpack path runs the reference's own eigsh calls."""
    W, C, U, l, q, p = load_case(next(c for c in quality_cases() if c["name"] == "ba600w"))
    Cm, _, _ = coarsening.coarsen(coarsening.Graph(W), K=10, r=0.5, Uk=U.copy(), lk=l.copy())
    met = coarsening.coarsening_quality(coarsening.Graph(W), Cm, kmax=10, Uk=U, lk=l.copy())
    assert met["angle_matrix"].shape == (10, 10) and met["error_eigenvalue"][0] == 0
    assert np.all(np.isfinite(met["error_subspace"])) and np.all(np.isfinite(met["error_sintheta"]))


# ---------------------------------------------------------------------------------------------------------------------
# spectral='device' against a dense eigendecomposition (Cora's giant component, kmax = 30)
# ---------------------------------------------------------------------------------------------------------------------
def test_device_spectral_against_dense_eigh():
    d = np.load(os.path.join(GOLDEN, "coarsen_cora_giant.npz"))
    N = len(d["W_indptr"]) - 1
    W = sp.csr_matrix((d["W_data"], d["W_indices"], d["W_indptr"]), shape=(N, N))
    C = sp.csc_matrix((d["r50_C_data"], d["r50_C_indices"], d["r50_C_indptr"]), shape=tuple(d["r50_C_shape"]))
    kmax = 30
    G = coarsening.Graph(W)
    l, U = np.linalg.eigh(G.L.toarray())
    Lc = (C @ G.L @ C.T).toarray()
    lc, Uc = np.linalg.eigh(Lc)
    exact = coarsening.coarsening_quality(G, C, kmax=kmax, Uk=U[:, :kmax], lk=l[:kmax].copy(), Uc=Uc[:, :kmax], lc=lc[:kmax])
    met = coarsening.coarsening_quality(G, C, kmax=kmax, spectral="device")
    # coarsening_quality asks lanczos_smallest for kmax + 5 pairs: its stopping rule bounds the residuals by tol times the
    # largest shifted eigenvalue, which left the last wanted Ritz values of a kmax-pair run at up to 7e-4 relative error here
    ee = np.abs(met["error_eigenvalue"] - exact["error_eigenvalue"])
    assert ee.max() < 1e-6, ee.max()
    # eigenvector metrics are defined by subspaces: compared where the spectra have a gap at k (Lanczos at tol 1e-5: the
    # error of a subspace scales as tol / gap); the angle matrix's last columns also need the gap of Lc at kmax
    def gap(v, k):
        return abs(v[k + 1] - v[k]) > 1e-3 * max(abs(v[k + 1]), 1e-12)
    ks = [k for k in range(1, kmax - 1) if gap(l, k) and gap(lc, k)]
    assert len(ks) >= 10
    es = np.abs(met["error_subspace"] - exact["error_subspace"])[ks]
    assert es.max() < 1e-4, es.max()
    if gap(lc, kmax - 1):
        st = np.abs(met["error_sintheta"] - exact["error_sintheta"])[ks]
        assert st.max() < 1e-4, st.max()


# ---------------------------------------------------------------------------------------------------------------------
# at scale: S-pubmed size, no dense N x N object
# ---------------------------------------------------------------------------------------------------------------------
TIME_LIMIT_S = 120.0  # the whole test: coarsen(), two Lanczos solves, the quality kernels and the torch check


def test_spubmed_size_device_run():
    t0 = time.time()
    N, E = 19717, 44324
    ei = data.synthetic_graph(N, E, seed=0)
    W = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(N, N))
    G = coarsening.Graph(W)
    C, _, _ = coarsening.coarsen(G, K=10, r=0.5, spectral="device")
    met = coarsening.coarsening_quality(G, C, kmax=30, spectral="device")
    for k in ("error_eigenvalue", "angle_matrix", "error_subspace", "error_sintheta"):
        assert np.all(np.isfinite(met[k])), k
    assert met["error_eigenvalue"][0] == 0
    assert np.abs(met["angle_matrix"]).max() <= 1 + 1e-12
    assert met["angle_matrix"].shape == (30, 30) and met["error_subspace"].shape == (30,)
    # G = Y^T L Y against torch f64 on the same U (sparse L, no dense N x N)
    U = np.random.default_rng(0).standard_normal((N, 30))
    Cc = sp.csc_matrix(C)
    a_d, c_d = dev(Cc.indices, torch.int32), dev(Cc.data)
    _, Y = coarsening.project_lift(a_d, c_d, C.shape[0], dev(U))
    Gd = coarsening.laplacian_gram(G.W, G.dw, Y)
    Lco = G.L.tocoo()
    Lt = torch.sparse_coo_tensor(np.vstack([Lco.row, Lco.col]), Lco.data, (N, N), dtype=torch.float64, device=DEV)
    Gt = Y.T @ torch.sparse.mm(Lt, Y)
    assert rel(Gd.cpu().numpy(), Gt.cpu().numpy()) < 1e-10
    assert time.time() - t0 < TIME_LIMIT_S
