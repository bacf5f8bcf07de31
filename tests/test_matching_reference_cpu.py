"""The references of tests/matching_reference.py against what the unmodified reference recorded (tests/golden/matching_*.npz from
make_matching_golden.py, graph_matching.npz from make_graph_matching_golden.py) and on the reference's own edge cases (CPU): the
references the GPU kernel tests (tests/test_gpu_matching_kernels.py) trust are themselves checked here."""
import json
import os

import numpy as np
import pytest

import matching_reference as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "matching_manifest.json")) as _f:
    MAN = json.load(_f)
CASES = MAN["cases"]
NAMES = sorted({c["name"] for c in CASES})
WITH_X = [n for n in NAMES if n != "cora_giant"]          # the reference's test vectors are stored up to X_max_N nodes
K = MAN["K"]
_Z, _E = {}, {}


def fixture(name):
    if name not in _Z:
        _Z[name] = dict(np.load(os.path.join(GOLDEN, f"matching_{name}.npz")))
    return _Z[name]


def edges(name):
    """(rowptr, col, w, dw, edge list) of a fixture graph, made once."""
    if name not in _E:
        z = fixture(name)
        rowptr, col, w = z["W_indptr"].astype(np.int64), z["W_indices"].astype(np.int64), z["W_data"]
        dw = np.add.reduceat(w, rowptr[:-1])             # every fixture row has entries
        _E[name] = (rowptr, col, w, dw, mr.edge_list(rowptr, col, w))
    return _E[name]


def x0(name):
    N = len(fixture(name)["W_indptr"]) - 1
    return np.random.RandomState(MAN["seed"]).randn(N, K) / np.sqrt(N)


def ulp_diff(a, b):
    a = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.mark.parametrize("name", NAMES)
def test_edge_list_is_tril_in_row_major_order(name):
    rowptr, col, w, _, (edge_off, src, dst, ew, csr_eid) = edges(name)
    N = len(rowptr) - 1
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    low = col < rows
    assert np.array_equal(src, rows[low]) and np.array_equal(dst, col[low]) and np.array_equal(ew, w[low])
    assert np.array_equal(edge_off, np.r_[0, np.cumsum(np.bincount(rows[low], minlength=N))])
    hi, lo = np.maximum(rows, col), np.minimum(rows, col)
    assert np.array_equal(src[csr_eid], hi) and np.array_equal(dst[csr_eid], lo)


@pytest.mark.parametrize("name", NAMES)
def test_heavy_edge_is_the_recorded_proximity_bit_for_bit(name):
    rowptr, col, w, _, (_, src, dst, ew, _) = edges(name)
    assert np.array_equal(_bits(mr.heavy_edge(rowptr, col, w, src, dst, ew)), _bits(fixture(name)["heavy_edge_w1"]))


@pytest.mark.parametrize("name", WITH_X)
def test_jc_from_the_recorded_vectors_is_the_recorded_proximity_bit_for_bit(name):
    _, _, _, _, (_, src, dst, _, _) = edges(name)
    z = fixture(name)
    assert np.array_equal(_bits(mr.jc(src, dst, z["algebraic_JC_X"])), _bits(z["algebraic_JC_w1"]))


@pytest.mark.parametrize("name", WITH_X)
def test_affinity_from_the_recorded_vectors_rounds_to_the_recorded_proximity(name):
    rowptr, _, _, _, (_, src, dst, _, _) = edges(name)
    z = fixture(name)
    p, _, _, _ = mr.affinity(src, dst, z["affinity_GS_X"], len(rowptr) - 1)
    assert ulp_diff(p.astype(np.float32), z["affinity_GS_w1"]).max() == 0


def test_affinity_on_cora_giant_from_the_reference_draw():
    """cora_giant's test vectors are not recorded: they are remade here from the manifest's draw by gauss_seidel, so the recorded
    proximities (SciPy's triangular solve, BLAS dot products, float64) are met to 1 float32 ulp, not 0."""
    rowptr, col, w, dw, (_, src, dst, _, _) = edges("cora_giant")
    N = len(rowptr) - 1
    X, _ = mr.gauss_seidel(rowptr, col, w, dw, [0, N], x0("cora_giant"))
    p, _, _, _ = mr.affinity(src, dst, X, N)
    d = ulp_diff(p.astype(np.float32), fixture("cora_giant")["affinity_GS_w1"])
    print(f"[cora_giant] affinity_GS proximities that differ from the recorded ones: {int((d > 0).sum())} of {len(d)}, worst {int(d.max())} ulp")
    assert d.max() <= 1


@pytest.mark.parametrize("name", WITH_X)
def test_test_vectors_from_the_reference_draw(name):
    """Measured max |X - recorded| / max |recorded| on an x86-64 CPU: Jacobi 1.0e-15 (ba600w; ring100 2.2e-16, cora26 4.0e-16),
    Gauss-Seidel 3.4e-16 (ba600w; ring100 2.1e-16, cora26 8.8e-17), the same for both summation orders.  The bound 1e-13 leaves about two orders for SciPy's summation order (Dinv (D - L) is formed
    as one matrix there, the triangular solve sums in its own order)."""
    rowptr, col, w, dw, _ = edges(name)
    z = fixture(name)
    N = len(rowptr) - 1
    for got, ref in ((mr.jacobi(rowptr, col, w, dw, x0(name), 20), z["algebraic_JC_X"]),
                     (mr.gauss_seidel(rowptr, col, w, dw, [0, N], x0(name))[0], z["affinity_GS_X"]),
                     (mr.gauss_seidel_ordered(rowptr, col, w, dw, [0, N], x0(name)), z["affinity_GS_X"])):
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"[{name}] test vectors: {err:.3g} of max|X|")
        assert err <= 1e-13


@pytest.mark.parametrize("name", WITH_X)
def test_ordered_gauss_seidel_is_within_the_derived_bound_of_the_mathematical_one(name):
    rowptr, col, w, dw, _ = edges(name)
    N = len(rowptr) - 1
    a, bound = mr.gauss_seidel(rowptr, col, w, dw, [0, N], x0(name))
    b = mr.gauss_seidel_ordered(rowptr, col, w, dw, [0, N], x0(name))
    assert np.all(np.abs(a - b) <= bound)
    assert bound.max() <= 1e-12 * np.abs(a).max()       # the bound itself stays a rounding-sized quantity


@pytest.mark.parametrize("name", NAMES)
def test_edge_cost_is_the_recorded_variation_edges_weight(name):
    """The closed form against the reference's 2 x K matrix products: they round differently only where a_i - a_j cancels (twin
    nodes), relative 1e-12 of the largest cost (the bound tests/test_gpu_matching.py holds the kernel to)."""
    _, _, _, dw, (_, src, dst, _, _) = edges(name)
    z = fixture(name)
    lk = z["lk"].copy()
    mask = lk < 1e-10
    lk[mask] = 1
    lsinv = lk ** (-0.5)
    lsinv[mask] = 0
    cost, cond = mr.edge_cost(src, dst, dw, z["Uk"][:, :K] * lsinv[:K])
    ref = -z["variation_edges_w1"]
    assert np.array_equal(cost, cond)                    # non-negative degrees: the expression is its own condition
    np.testing.assert_allclose(cost.astype(np.float64), ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['name']}-{c['method']}-{c['r']}")
def test_stable_greedy_on_the_recorded_weights_is_the_recorded_matching(case):
    z = fixture(case["name"])
    _, _, _, _, (_, src, dst, _, _) = edges(case["name"])
    p = f"{case['method']}_r{int(round(case['r'] * 100)):02d}_"
    weight = np.asarray(z[f"{case['method']}_w1"], dtype=np.float64)
    keep = mr.match_keep(case["N"], float(z[p + "r_cur1"]))
    pairs, taken, sel_off, sel_count = mr.stable_greedy(src, dst, weight, case["N"], None, keep, 0)
    assert np.array_equal(pairs, z[p + "match_stable"])
    assert taken.tolist() == [len(pairs)] and sel_count.tolist() == [len(pairs), 2 * len(pairs)]
    assert np.array_equal(sel_off, 2 * np.arange(len(pairs) + 1))


def test_match_keep_is_the_stopping_rule_of_the_sequential_scan():
    for N in (2, 3, 7, 10, 100, 2485):
        for r in (0.0, 0.01, 0.3, 0.5, 1 - 0.7, 0.7, 0.99, 0.999):
            n, taken, n_target = N, 0, (1 - r) * N
            while True:                                  # matching_greedy :969-987 with an endless supply of free edges
                n -= 1
                taken += 1
                if n <= n_target:
                    break
            assert mr.match_keep(N, r) == taken, (N, r)


def test_sort_key_order_on_ties_zeros_infinities_denormals_and_nans():
    nan, inf, tiny = float("nan"), float("inf"), 5e-324
    w = np.array([1.0, nan, -0.0, inf, 0.0, -1.0, tiny, 1.0, -inf, nan, -tiny, 0.0, inf])
    # -weight ascending = weight descending: +inf (3, 12), 1.0 (0, 7), +denormal (6), the zeros of either sign by id (2, 4, 11),
    # -denormal (10), -1.0 (5), -inf (8), then the NaNs by id (1, 9)
    assert mr.sort_key_order(w).tolist() == [3, 12, 0, 7, 6, 2, 4, 11, 10, 5, 8, 1, 9]


def _path(n, w=None):
    rowptr, col = [0], []
    for i in range(n):
        col += [j for j in (i - 1, i + 1) if 0 <= j < n]
        rowptr.append(len(col))
    return np.array(rowptr), np.array(col, dtype=np.int64), (None if w is None else np.asarray(w, dtype=np.float64))


def test_dominant_rounds_of_the_unit_path_and_of_a_star():
    rowptr, col, _ = _path(300)
    _, src, dst, ew, csr_eid = mr.edge_list(rowptr, col)
    rounds, taken = mr.dominant_rounds(rowptr, col, csr_eid, src, dst, ew, 300)
    pairs, _, _, _ = mr.stable_greedy(src, dst, ew, 300)
    assert rounds == 150                                 # all ties: edge (i + 1, i) has rank i, one match per round
    assert np.array_equal(np.c_[src[taken], dst[taken]], pairs)
    n = 40                                               # a star: the hub's best edge in round 1, nothing left for round 2
    rowptr = np.r_[0, n - 1, n - 1 + np.arange(1, n)]
    col = np.r_[np.arange(1, n), np.zeros(n - 1, dtype=np.int64)]
    _, src, dst, ew, csr_eid = mr.edge_list(rowptr, col)
    rounds, taken = mr.dominant_rounds(rowptr, col, csr_eid, src, dst, ew, n)
    assert rounds == 1 and taken.tolist() == [0]


def test_dominant_rounds_give_the_sequential_matching_on_recorded_weights():
    rowptr, col, _, _, (_, src, dst, _, csr_eid) = edges("ba600w")
    for m in MAN["methods"]:
        weight = np.asarray(fixture("ba600w")[f"{m}_w1"], dtype=np.float64)
        rounds, taken = mr.dominant_rounds(rowptr, col, csr_eid, src, dst, weight, 600)
        pairs, _, _, _ = mr.stable_greedy(src, dst, weight, 600)
        assert 1 <= rounds <= 301
        assert sorted(map(tuple, np.c_[src[taken], dst[taken]].tolist())) == sorted(map(tuple, pairs.tolist()))


# ---------------------------------------------------------------------------------------------------------------------------------
# the level loop against the graph-level fixture
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["heavy_edge", "algebraic_JC"])
@pytest.mark.parametrize("r", [0.3, 0.5, 0.7])
def test_coarsen_levels_reproduces_the_graph_level_fixture(method, r):
    """What test_in_order_kernel_against_the_reference_fixture demands of the kernel: C, Gc.W and the applied levels exact on every
    graph before the first near-tie of algebraic_JC (the fixture has none), and the np.random stream after the loop."""
    z = np.load(os.path.join(GOLDEN, "graph_matching.npz"))
    off = z["comp_off"]
    rowptr, col, w = z["W_indptr"].astype(np.int64), z["W_indices"].astype(np.int64), z["W_data"]
    p = f"{method}_r{int(round(r * 100)):02d}_"
    n, lv, gap = z[p + "n"], z[p + "levels"], z[p + "min_rel_gap"]
    assert method == "heavy_edge" or not (gap < 1e-6).any()
    pool = np.random.RandomState(0).randn(2 * K * 10 * int(off[-1]))      # randn(a); randn(b) == randn(a + b) for even a
    used = row_o = ent_o = 0
    for g in range(len(n)):
        b, e = int(off[g]), int(off[g + 1])
        rp = z[p + "gcw_indptr"][row_o: row_o + int(n[g]) + 1]
        nz = int(rp[-1])
        ci, cd = z[p + "gcw_indices"][ent_o: ent_o + nz], z[p + "gcw_data"][ent_o: ent_o + nz]
        row_o += int(n[g]) + 1
        ent_o += nz
        if e - b <= 1:
            continue
        p0, p1 = rowptr[b], rowptr[e]
        assign, cval, (wr, wc, ww), levels, du = mr.coarsen_levels(rowptr[b: e + 1] - p0, col[p0:p1] - b, w[p0:p1], r, method, K,
                                                                  pool[used:], 10, 0.99)
        used += du
        assert levels == int(lv[g]) and len(wr) - 1 == int(n[g]), g
        assert np.array_equal(assign, z[p + "assign"][b:e]) and np.array_equal(cval, z[p + "cval"][b:e]), g
        assert np.array_equal(wr, rp) and np.array_equal(wc, ci) and np.array_equal(ww, cd), g
    assert (used > 0) == (method == "algebraic_JC")
    assert np.array_equal(pool[used: used + 8], z[p + "next_randn"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's own edge cases
# ---------------------------------------------------------------------------------------------------------------------------------
def test_empty_graph():
    rowptr, col = np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    edge_off, src, dst, ew, csr_eid = mr.edge_list(rowptr, col)
    assert edge_off.tolist() == [0] and len(src) == len(dst) == len(ew) == len(csr_eid) == 0
    assert len(mr.heavy_edge(rowptr, col, None, src, dst, ew)) == 0 and len(mr.jc(src, dst, np.zeros((0, 3)))) == 0
    assert mr.jacobi(rowptr, col, None, np.zeros(0), np.zeros((0, 3)), 20).shape == (0, 3)
    pairs, taken, sel_off, sel_count = mr.stable_greedy(src, dst, ew, 0)
    assert pairs.shape == (0, 2) and taken.tolist() == [0] and sel_off.tolist() == [0] and sel_count.tolist() == [0, 0]
    assert mr.dominant_rounds(rowptr, col, csr_eid, src, dst, ew, 0)[0] == 0


def test_single_edge():
    rowptr, col, w = np.array([0, 1, 2]), np.array([1, 0]), np.array([0.5, 0.5])
    edge_off, src, dst, ew, csr_eid = mr.edge_list(rowptr, col, w)
    assert edge_off.tolist() == [0, 0, 1] and (src.tolist(), dst.tolist(), ew.tolist(), csr_eid.tolist()) == ([1], [0], [0.5], [0, 0])
    assert mr.heavy_edge(rowptr, col, w, src, dst, ew)[0] == np.float32(0.5 / (0.5 + 1e-5))
    X = np.array([[1.0, 2.0], [1.0, 5.0]])
    assert mr.jc(src, dst, X)[0] == np.float32(1.0 / 9.0)                 # min(1 / 1e-6, 1 / 9)
    p, c, cmax, cond = mr.affinity(src, dst, np.array([[1.0, 0.0], [2.0, 0.0]]), 2)  # c = 2^2 / (1^2 4^2); its own maximum twice
    assert (p.tolist(), c.tolist(), cmax.tolist(), cond.tolist()) == ([4.0], [0.25], [0.25, 0.25], [1.0])
    cost, _ = mr.edge_cost(src, dst, np.array([0.5, 0.5]), X)
    assert cost[0] == 9.0 * 0.25 * 2.0
    pairs, taken, _, _ = mr.stable_greedy(src, dst, ew, 2)
    assert pairs.tolist() == [[1, 0]] and taken.tolist() == [1]
    assert mr.stable_greedy(src, dst, ew, 2, None, 5, 2)[0].shape == (0, 2)          # one pair <= min_gain: kept none
    # a 2-node component: its one pair is <= 2 pairs, the level is not applied
    assign, cval, (wr, wc, ww), levels, used = mr.coarsen_levels(rowptr, col, w, 0.5, "heavy_edge")
    assert (assign.tolist(), cval.tolist(), levels, used) == ([0, 1], [1.0, 1.0], 0, 0)
    assert (wr.tolist(), wc.tolist(), ww.tolist()) == ([0, 1, 2], [1, 0], [0.5, 0.5])


def test_isolated_node_and_zero_iterations():
    rowptr, col, w = np.array([0, 1, 2, 2]), np.array([1, 0]), np.array([0.1, 0.1])       # node 2 has no edge
    dw = np.array([0.1, 0.1, 0.0])
    X0 = np.array([[1.0, -3.0], [0.25, 7.0], [6.0, -2.0]])
    assert np.array_equal(mr.jacobi(rowptr, col, w, dw, X0, 0), X0)
    X1 = mr.jacobi(rowptr, col, w, dw, X0, 1)
    assert np.array_equal(X1[2], 0.5 * X0[2])                             # deg = 0: deg^-1 = inf is set to 0 (:839)
    # f32(0.1) != 0.1: the diagonal of D - L is f32(dw) - dw, not 0, and Dinv is the float32 reciprocal
    degf = np.float32(0.1)
    dinv = float(np.float32(1.0) / degf)
    assert np.array_equal(X1[0], 0.5 * X0[0] + 0.5 * (dinv * (0.1 * X0[1] + (float(degf) - 0.1) * X0[0])))
    _, src, dst, ew, _ = mr.edge_list(rowptr, col, w)
    assert mr.heavy_edge(rowptr, col, w, src, dst, ew).tolist() == [float(np.float32(0.1 / (0.1 + 1e-5)))]
    # a stored entry that is not positive never enters the column maximum
    wn = np.array([-2.0, -2.0])
    assert mr.heavy_edge(rowptr, col, wn, src, dst, wn[:1]).tolist() == [float(np.float32(-2.0 / 1e-5))]
