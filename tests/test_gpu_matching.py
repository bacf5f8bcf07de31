"""GPU tier of the matching-based coarsening methods: every device stage fed with the reference's own inputs
(tests/golden/make_matching_golden.py), end-to-end coarsen() against the reference's stable-tie run, the batched path against
per-component coarsen(), the node-level pipeline on Cora, and the matching rounds on a graph with > 1e5 edges."""
import json
import os
import time

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import matching_reference as mr
from fitgnn_amd import coarsening

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
K = 10

with open(os.path.join(GOLDEN, "matching_manifest.json")) as _f:
    MAN = json.load(_f)
CASES = MAN["cases"]
NAMES = sorted({c["name"] for c in CASES})
_Z = {}


def fixture(name):
    if name not in _Z:
        _Z[name] = dict(np.load(os.path.join(GOLDEN, f"matching_{name}.npz")))
    return _Z[name]


def graph(z):
    N = len(z["W_indptr"]) - 1
    return coarsening.Graph(sp.csr_matrix((z["W_data"], z["W_indices"], z["W_indptr"]), shape=(N, N)))


def x0(z):
    """The level-1 draw of the random methods: np.random.seed(seed); randn(N, K) / sqrt(N) (checked by the generator)."""
    N = len(z["W_indptr"]) - 1
    return np.random.RandomState(MAN["seed"]).randn(N, K) / np.sqrt(N)


def prefix(case):
    return f"{case['method']}_r{int(round(case['r'] * 100)):02d}_"


def ulp_diff(a, b):
    a = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


@pytest.mark.parametrize("name", NAMES)
def test_edge_list_and_proximities_from_reference_inputs(name):
    z = fixture(name)
    G = graph(z)
    el = coarsening.EdgeList(G)
    t = sp.tril(G.W, -1).tocoo()                     # get_edge_list(): tril(W) in row-major order
    assert el.M == t.nnz
    assert np.array_equal(el.src.cpu().numpy(), t.row) and np.array_equal(el.dst.cpu().numpy(), t.col)
    prox = coarsening.proximity(el, "heavy_edge").cpu().numpy()
    assert np.array_equal(prox, z["heavy_edge_w1"])
    if "algebraic_JC_X" in z:                        # the reference's test vectors are stored for the smaller graphs
        XJ = torch.from_numpy(z["algebraic_JC_X"]).cuda()
        assert np.array_equal(coarsening.proximity(el, "algebraic_JC", XJ).cpu().numpy(), z["algebraic_JC_w1"])
        XG = torch.from_numpy(z["affinity_GS_X"]).cuda()
        pg = coarsening.proximity(el, "affinity_GS", XG).cpu().numpy()
        assert ulp_diff(pg, z["affinity_GS_w1"]).max() <= 2
        # what the kernel's operation count allows (matching_reference.affinity_interval): between the float32 roundings of the two
        # ends of the float64 interval, which lie at most one float32 apart -- and the long-double value rounds to the recorded one
        p, c, cmax, cond = mr.affinity(t.row, t.col, z["affinity_GS_X"], G.N)
        lo, hi = (v.astype(np.float32) for v in mr.affinity_interval(t.row, t.col, G.N, p, c, cmax, cond))
        assert ulp_diff(lo, hi).max() <= 1 and ulp_diff(p.astype(np.float32), z["affinity_GS_w1"]).max() == 0
        assert np.all((lo <= pg) & (pg <= hi)), f"{int((~((lo <= pg) & (pg <= hi))).sum())} proximities outside the rounded interval"
    A = coarsening._spectral_level1(G, K, z["Uk"].copy(), z["lk"].copy())
    cost = coarsening.edge_costs(el, A).cpu().numpy()
    # the closed form and the reference's 2 x K matrix products round differently only where a_i - a_j cancels (twin nodes,
    # costs ~1e-28 next to ~1): relative 1e-12 of the largest cost
    ref = -z["variation_edges_w1"]
    np.testing.assert_allclose(cost, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["method"] == "algebraic_JC" and c["r"] == 0.5 and c["N"] <= MAN["X_max_N"]])
def test_test_vectors_from_the_reference_draw(name):
    z = fixture(name)
    el = coarsening.EdgeList(graph(z))
    G = graph(z)
    rowptr, col, w, dw = G.W.indptr, G.W.indices, G.W.data, np.asarray(el.dw.cpu().numpy())
    for m in coarsening.RANDOM_METHODS:
        X = coarsening.test_vectors(el, m, x0(z)).cpu().numpy()
        np.testing.assert_allclose(X, z[f"{m}_X"], rtol=1e-10, atol=1e-14 * np.abs(z[f"{m}_X"]).max())
        # every operation of both kernels and its order is fixed: the float64 reference bit for bit, which itself meets the recorded
        # vectors to 1e-13 of the largest entry (tests/test_matching_reference_cpu.py)
        ref = (mr.jacobi(rowptr, col, w, dw, x0(z), 20) if m == "algebraic_JC"
               else mr.gauss_seidel_ordered(rowptr, col, w, dw, [0, G.N], x0(z)))
        assert np.array_equal(X.view(np.int64), ref.view(np.int64)), f"{m}: {int((X != ref).sum())} entries differ from the float64 reference"
        assert np.abs(X - z[f"{m}_X"]).max() <= 1e-13 * np.abs(z[f"{m}_X"]).max()


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['name']}-{c['method']}-{c['r']}")
def test_matching_on_reference_weights_is_the_stable_greedy(case):
    z = fixture(case["name"])
    p = prefix(case)
    el = coarsening.EdgeList(graph(z))
    w = torch.from_numpy(np.asarray(z[f"{case['method']}_w1"], dtype=np.float64)).cuda()
    res = coarsening.greedy_matching(el, w, coarsening.match_keep(case["N"], float(z[p + "r_cur1"])))
    pairs = res.sel_mem.reshape(-1, 2)
    assert np.array_equal(res.sel_off, 2 * np.arange(len(pairs) + 1))
    assert np.array_equal(pairs, z[p + "match_stable"])   # = the unpatched reference too where the manifest says they agree
    assert 1 <= res.rounds <= case["N"] // 2 + 1


def exact_expected(case):
    """Where coarsen() must reproduce the reference's stable run bit for bit: heavy_edge everywhere (its weights are exact);
    the others where no two distinct weights of any level are closer than the device's rounding can move them."""
    m = case["method"]
    if m == "heavy_edge":
        return True
    if m == "variation_edges":
        # tiny costs are |a_i - a_j|^2 of near-twin rows: cancellation leaves rounding noise that orders them
        return case["min_rel_gap"] >= 1e-12 and case["tiny_weights"] == 0
    return case["min_rel_gap"] >= 1e-6


def check_structure(C, N, n_expected_max):
    C = sp.csc_matrix(C)
    assert np.all(np.diff(C.indptr) == 1)
    sizes = np.bincount(C.indices, minlength=C.shape[0])
    assert sizes.min() >= 1
    assert C.shape[0] <= N and C.shape[0] >= n_expected_max


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['name']}-{c['method']}-{c['r']}")
def test_coarsen_end_to_end(case):
    z = fixture(case["name"])
    p = prefix(case)
    G = graph(z)
    N = G.N
    kw = dict(K=K, r=case["r"], method=case["method"])
    if case["method"] == "variation_edges":
        kw.update(Uk=z["Uk"].copy(), lk=z["lk"].copy())
    np.random.seed(MAN["seed"])
    C, Gc, maps = coarsening.coarsen(G, **kw)
    C = sp.csc_matrix(C)
    assert all(all(k == v for k, v in d.items()) for d in maps) and len(maps[0]) == N
    if exact_expected(case):
        assert [len(d) for d in maps] == z[p + "maps_len"].tolist()
        Cr = sp.csc_matrix((z[p + "C_data"], z[p + "C_indices"], np.arange(N + 1)), shape=tuple(z[p + "C_shape"]))
        assert C.shape == Cr.shape
        assert np.array_equal(C.indices, Cr.indices) and np.array_equal(C.indptr, Cr.indptr)
        np.testing.assert_allclose(C.data, Cr.data, rtol=1e-12, atol=0)
        GW = sp.csr_matrix(Gc.W)
        assert (GW != GW.T).nnz == 0 and not GW.diagonal().any()
        GW = sp.tril(GW, -1).tocsr()                         # stored: the strict lower triangle of the symmetric Gc.W
        GW.sort_indices()
        assert np.array_equal(GW.indptr, z[p + "GcWl_indptr"]) and np.array_equal(GW.indices, z[p + "GcWl_indices"])
        np.testing.assert_allclose(GW.data, z[p + "GcWl_data"], rtol=1e-12, atol=0)
    else:
        # a valid contraction of pairs per level, reaching the reference's size to within what near-ties can change
        check_structure(C, N, 1)
        assert abs(C.shape[0] - case["n"]) <= max(2, case["n"] // 50)


def test_level_matching_is_maximal_and_truncated_by_the_stopping_rule():
    z = fixture("cora_giant")
    G = graph(z)
    el = coarsening.EdgeList(G)
    np.random.seed(1)
    X = coarsening.test_vectors(el, "algebraic_JC", np.random.randn(G.N, K) / np.sqrt(G.N))
    w = coarsening.proximity(el, "algebraic_JC", X)
    full = coarsening.greedy_matching(el, w, G.N)            # untruncated: a maximal matching
    pairs = full.sel_mem.reshape(-1, 2)
    used = np.zeros(G.N, dtype=bool)
    assert not np.any(np.bincount(pairs.ravel(), minlength=G.N) > 1)
    used[pairs.ravel()] = True
    coo = sp.tril(G.W, -1).tocoo()
    assert not np.any(~used[coo.row] & ~used[coo.col]), "an edge with two free ends remains"
    for r in (0.1, 0.3):
        k = coarsening.match_keep(G.N, r)
        part = coarsening.greedy_matching(el, w, k).sel_mem.reshape(-1, 2)
        assert np.array_equal(part, pairs[:k])               # the truncated scan = the first k by rank


def cora_components():
    from fitgnn_amd import pipeline

    data, _ = pipeline.load_planetoid(os.path.join(GOLDEN, "cora_raw"), "cora")
    ei = np.asarray(data.edge_index)
    N = data.num_nodes
    W = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(N, N))
    W.data[:] = 1.0
    comps = [H for H in coarsening.Graph(W).extract_components() if H.N > 1]
    return data, comps


@pytest.mark.parametrize("method", ["heavy_edge", "variation_edges"])
def test_coarsen_batch_equals_per_component_coarsen(method):
    _, comps = cora_components()
    comps = [H for H in comps if H.N <= 200]               # the small components (the giant one runs alone either way)
    A0, blocks = [], []
    for H in comps:
        if method == "variation_edges":
            lk, U = np.linalg.eigh(H.L.toarray())
            k = min(K, H.N)
            A0.append((lk[:k].copy(), U[:, :k].copy()))
        blocks.append(H.W)
    W = sp.block_diag(blocks).tocsr()
    off = np.concatenate([[0], np.cumsum([H.N for H in comps])])
    A_in = None
    if method == "variation_edges":
        A_in = [coarsening._spectral_level1(H, min(K, H.N), U.copy(), lk.copy()) for H, (lk, U) in zip(comps, A0)]
    bc = coarsening.coarsen_batch(W, off, r=0.5, method=method, A0=A_in)
    for c, H in enumerate(comps):
        kw = {}
        if method == "variation_edges":
            lk, U = A0[c]
            kw = dict(K=min(K, H.N), Uk=U.copy(), lk=lk.copy())
        C, Gc, _ = coarsening.coarsen(H, r=0.5, method=method, **kw)
        C = sp.csc_matrix(C)
        b, e, cb, ce = off[c], off[c + 1], bc.cluster_off[c], bc.cluster_off[c + 1]
        assert ce - cb == C.shape[0], (c, H.N)
        assert np.array_equal(bc.assign[b:e] - cb, C.indices)
        np.testing.assert_allclose(bc.cval[b:e], C.data, rtol=1e-12, atol=0)
        assert (bc.Wc[cb:ce, cb:ce] != sp.csr_matrix(Gc.W)).nnz == 0


def utils_167_map(C):
    """utils.py:167-180 restated: column j -> row of its non-zero; nodes without one -> the row with the largest sum."""
    C = sp.csc_matrix(C)
    rows, cols = C.nonzero()
    md = {int(j): int(i) for i, j in zip(rows, cols)}
    col_sum = np.asarray(C.sum(axis=1))
    top = int(np.argwhere(col_sum == col_sum.max())[0][0])
    for node in set(range(C.shape[1])) - set(md):
        md[node] = top
    return np.array([md[j] for j in range(C.shape[1])])


def test_pipeline_runs_heavy_edge_on_cora():
    from fitgnn_amd import pipeline

    data, _ = cora_components()
    co_v = pipeline.coarsening_classification(None, data, 0.5, "variation_neighborhoods")
    co_h = pipeline.coarsening_classification(None, data, 0.5, "heavy_edge")
    assert not np.array_equal(co_v.assign, co_h.assign), "heavy_edge ran the variation method"
    for H, C, off in zip(co_h.components, co_h.all_C, co_h.comp_cluster_off):
        idx = np.asarray(H.info["orig_idx"])
        if C is None:
            continue
        Cr, _, _ = coarsening.coarsen(H, r=0.5, method="heavy_edge")   # deterministic: the same C again
        assert np.array_equal(co_h.assign[idx] - off, utils_167_map(Cr))
    with pytest.raises(NotImplementedError, match="affinity_GS"):
        pipeline.coarsening_classification(None, data, 0.5, "affinity_GS")


def test_rounds_terminate_on_a_large_graph():
    from fitgnn_amd import data as fdata

    N, E = 40000, 120000
    ei = fdata.synthetic_graph(N, E, seed=3)
    W = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(N, N))
    G = coarsening.Graph(W)
    assert sp.tril(G.W, -1).nnz >= 100000
    t0 = time.time()
    C, Gc, maps = coarsening.coarsen(G, r=0.6, method="heavy_edge")
    torch.cuda.synchronize()
    assert time.time() - t0 < 120
    assert len(maps) >= 2                                        # two levels at least: r = 0.6 needs more than one matching
    check_structure(C, N, 1)
    el = coarsening.EdgeList(G)
    res = coarsening.greedy_matching(el, coarsening.proximity(el, "heavy_edge"), coarsening.match_keep(N, 0.6))
    assert 1 <= res.rounds <= N // 2 + 1
    print("rounds", res.rounds)
