"""CPU tier of the matching-based coarsening methods (heavy_edge, algebraic_JC, affinity_GS, variation_edges): the new ABI
symbols and their host-side size queries, the method validation of coarsen() / coarsen_batch() / the CLIs, and the reference
fixtures (tests/golden/make_matching_golden.py) against a restatement of the stable tie rule."""
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from fitgnn_amd import _lib, coarsening

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "fit-gnn_amd"))

NEW_SYMBOLS = ("fitgnn_edge_list", "fitgnn_heavy_edge_proximity_workspace_bytes", "fitgnn_heavy_edge_proximity", "fitgnn_jc_proximity",
               "fitgnn_affinity_proximity_workspace_bytes", "fitgnn_affinity_proximity", "fitgnn_edge_variation_costs_f64",
               "fitgnn_jacobi_vectors_workspace_bytes", "fitgnn_jacobi_vectors_f64", "fitgnn_gauss_seidel_vectors_f64",
               "fitgnn_greedy_matching_workspace_bytes", "fitgnn_greedy_matching")


def manifest():
    with open(os.path.join(GOLDEN, "matching_manifest.json")) as f:
        return json.load(f)


def test_matching_symbols_exported_and_sized_without_a_gpu():
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n) and n in _lib.SIGNATURES, n
    assert L.fitgnn_heavy_edge_proximity_workspace_bytes(1000) >= 1000 * 8
    assert L.fitgnn_affinity_proximity_workspace_bytes(1000, 5000) >= 1000 * 8 + 5000 * 8
    assert L.fitgnn_jacobi_vectors_workspace_bytes(1000, 10) >= 1000 * 10 * 8
    assert L.fitgnn_jacobi_vectors_workspace_bytes(1000, 17) == 0          # K > FITGNN_MAX_K: unsupported
    ws = L.fitgnn_greedy_matching_workspace_bytes(1000, 5000, 3)
    assert ws >= 5000 * (8 + 8 + 4 * 6) and ws > L.fitgnn_greedy_matching_workspace_bytes(1000, 100, 3)
    assert L.fitgnn_greedy_matching_workspace_bytes(-1, 5, 1) == 0
    # argument errors are reported before any device work
    assert L.fitgnn_jc_proximity(None, None, 10, None, 0, 0, None, None) == -1
    assert L.fitgnn_edge_variation_costs_f64(None, None, 10, None, None, 10, 5, None, None) == -1
    assert L.fitgnn_greedy_matching(None, None, None, -1, None, None, None, 0, None, 1, None, None, 0, None, None, None, None, None, None,
                                    0, None) == -1


def _ring(n):
    i = np.arange(n)
    return coarsening.Graph(sp.csr_matrix((np.ones(2 * n), (np.r_[i, (i + 1) % n], np.r_[(i + 1) % n, i])), shape=(n, n)))


@pytest.mark.parametrize("method", ["kron", "variation_cliques", "heavy_edges", "bogus"])
def test_coarsen_refuses_unsupported_methods(method):
    with pytest.raises(NotImplementedError, match="supported: variation_neighborhoods, heavy_edge, algebraic_JC, affinity_GS"):
        coarsening.coarsen(_ring(10), method=method)


def test_coarsen_refuses_optimal_matching_and_batched_random_methods():
    with pytest.raises(NotImplementedError, match="greedy"):
        coarsening.coarsen(_ring(10), method="heavy_edge", algorithm="optimal")
    W = sp.block_diag([_ring(6).W, _ring(5).W]).tocsr()
    for m in coarsening.RANDOM_METHODS:
        with pytest.raises(NotImplementedError, match="per component"):
            coarsening.coarsen_batch(W, [0, 6, 11], method=m)
    with pytest.raises(NotImplementedError):
        coarsening.coarsen_batch(W, [0, 6, 11], method="kron")


def test_cli_refuses_methods_outside_the_supported_set():
    import inference
    import main

    for build, base in ((main.build_parser, ["--output_dir", "x"]), (inference.build_parser, [])):
        p = build()
        for m in ("heavy_edge", "algebraic_JC", "variation_edges", "variation_neighborhoods"):
            assert p.parse_args(base + ["--coarsening_method", m]).coarsening_method == m
        for m in ("kron", "variation_cliques", "affinity_GS", "heavy"):
            with pytest.raises(SystemExit):
                p.parse_args(base + ["--coarsening_method", m])
    assert set(main.COARSENING_METHODS) == set(coarsening.SUPPORTED_METHODS) - {"affinity_GS"}


def stable_greedy(src, dst, weights, N, r):
    """matching_greedy (coarsening_utils.py:931-993) under the project's tie rule, restated: visit edges by (-weight, edge
    index), take an edge whose ends are both unmarked, stop once N - taken <= (1 - r) N."""
    order = np.lexsort((np.arange(len(weights)), -np.asarray(weights, dtype=np.float64)))
    marked = np.zeros(N, dtype=bool)
    out, n, n_target = [], N, (1 - r) * N
    for e in order:
        i, j = int(src[e]), int(dst[e])
        if marked[i] or marked[j]:
            continue
        marked[i] = marked[j] = True
        out.append((i, j))
        n -= 1
        if n <= n_target:
            break
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def test_fixtures_load_and_follow_the_stable_tie_rule():
    man = manifest()
    assert set(man["methods"]) == set(coarsening.MATCHING_METHODS)
    assert len(man["cases"]) == 4 * len(man["methods"]) * len(man["ratios"])
    cache = {}
    for case in man["cases"]:
        z = cache.setdefault(case["file"], np.load(os.path.join(GOLDEN, case["file"])))
        m, p = case["method"], f"{case['method']}_r{int(round(case['r'] * 100)):02d}_"
        N = case["N"]
        W = sp.csr_matrix((z["W_data"], z["W_indices"], z["W_indptr"]), shape=(N, N))
        t = sp.tril(W, -1).tocoo()                                               # the edge numbering: tril(W), row-major
        src, dst = t.row, t.col
        assert len(src) == case["M"] and np.all(src > dst)
        w1 = z[f"{m}_w1"]
        assert w1.dtype == (np.float64 if m == "variation_edges" else np.float32)
        r_cur = float(z[p + "r_cur1"])
        stable = z[p + "match_stable"]
        assert np.array_equal(stable_greedy(src, dst, w1, N, r_cur), stable), (case["name"], m, case["r"])
        assert len(stable) == min(coarsening.match_keep(N, r_cur), len(stable_greedy(src, dst, w1, N, 0.999)))
        # the stable run's C: one non-zero per column (stored without its indptr), identity level dicts
        assert len(z[p + "C_indices"]) == len(z[p + "C_data"]) == N
        C = sp.csc_matrix((z[p + "C_data"], z[p + "C_indices"], np.arange(N + 1)), shape=tuple(z[p + "C_shape"]))
        assert C.shape == (case["n"], N) and np.all(np.bincount(C.indices, minlength=C.shape[0]) >= 1)
        assert np.all(z[p + "maps_identity"])
        assert z[p + "maps_len"][0] == N


def test_match_keep_restates_the_float64_stopping_rule():
    for N in (2, 3, 10, 26, 100, 2485):
        for r in (0.0, 0.3, 0.5, 1 - 70 / 100, 0.7, 0.99):
            n, n_target, k = N, (1 - r) * N, 0
            while True:
                k += 1
                n -= 1
                if n <= n_target:
                    break
            assert coarsening.match_keep(N, r) == k, (N, r)
