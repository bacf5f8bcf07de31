"""GPU tier: every launcher of csrc/matching.hip and fitgnn_match_small (csrc/match_small.hip) through the C ABI against the
references of tests/matching_reference.py, with the helpers of tests/test_gpu_step_kernels.py.  Each stage gets its inputs from the
host reference (the edge list of one test is not made by the kernel of another).  Every buffer carries NaN / -1 guard elements
behind it, padding columns (ldx > K) hold NaN, every output starts as NaN / -1: a lane that should not write, or a stale read, shows.

Launcher -> branch -> tests that reach it:

| launcher | branch (from the launch code and the kernel) | tests |
|---|---|---|
| fitgnn_edge_list (tril_count, scan.h in place, tril_fill) | paths with a chord hub of degree >= 65 at N = 1, 2 (no hub), 1023 (scan: one partial pass), 1024 (exactly one pass), 1025 (a second pass with one live element), 2049 (a third pass); rows with no lower entry (row 0) and with only lower entries (row N - 1); the binary search of tril_fill in a 65+ entry row; all integer outputs exact; N = 1 has no stored entry: its empty col array is still a non-NULL pointer (the launcher refuses NULL: it cannot see nnz) | test_edge_list |
| | N = 0: edge_off[0] = 0, nothing else touched | test_edge_list_empty |
| | w NULL (e_w all 1.0); e_w NULL and csr_eid NULL; m_cap < M (ids >= m_cap not written, guards intact, csr_eid complete); m_cap = 0 with NULL edge arrays | test_edge_list_optional_outputs |
| | N < 0, m_cap < 0, edge_off NULL, e_src NULL with m_cap > 0 refused | test_edge_list_refusals |
| fitgnn_heavy_edge_proximity (col_max, heavy_edge) | M = 255, 256, 257 (one workgroup partial / full, a second with one live thread); w given (random: both outcomes of wj > wi) / NULL (unit: equality); stored 0.0, -0.0 and negative entries never enter the maximum (a node with only such entries has wmax = 0); bits | test_heavy_edge |
| | M = 0 returns 0, prox untouched; workspace one byte short -> FITGNN_E_WORKSPACE; NULLs refused | test_heavy_edge_refusals |
| fitgnn_jc_proximity | K = 1, 10, 16 x ldx = K, K + 3 x M = 15, 16, 17 (sixteen 16-lane groups per workgroup: one partial, full, a second workgroup with one live group); twin rows (1e6), one column just above the clamp (d^2 = 4e-6); bits | test_jc |
| fitgnn_affinity_proximity (affinity_c, affinity_prox) | the same K / ldx / M; EXACT inputs bit for bit; RANDOM inputs inside the rounded interval; an edge whose end has its maximum on another edge; two launches, same bits (the maxima come from atomics) | test_affinity_exact, test_affinity_random |
| fitgnn_edge_variation_costs_f64 | the same K / lda / M; EXACT bit for bit; RANDOM within the bound; twin rows cost exactly 0.0 | test_edge_cost_exact, test_edge_cost_random |
| the three above | M = 0 returns 0; K = 0, K = 17, ldx < K, M < 0, NULLs refused; affinity workspace one byte short | test_proximity_refusals |
| fitgnn_jacobi_vectors_f64 | iterations = 0 (copy), 1 with work NULL, 2, 3, 20 (the ping-pong's parity lands the last step in X) x (N, K) = (15, 1), (16, 10), (17, 16); an isolated node (dw = 0 -> 0.5 x); weights in tenths (f32(dw) != dw: the correction term is live); bits | test_jacobi |
| | w NULL (unit weights: the correction vanishes) | test_jacobi_unit_weights |
| | X0 == X, iterations < 0, K = 17 refused; workspace one byte short at iterations = 2; N = 0 returns 0 | test_jacobi_refusals |
| fitgnn_gauss_seidel_vectors_f64 | n_comp = 3 (components of 2, 40, 200 nodes in one launch) and n_comp = 1 (the 40-node component; the 200-node path: every row reads the row written just before it); rows of degree 1, 3, 4, 5, 9 (one to four live lane groups, a second and a third trip); K = 1, 10, 16; w NULL / given; ordered reference as bits, mathematical reference within its bound | test_gauss_seidel |
| | X0 == X, K = 0 refused; n_comp = 0 returns 0 | test_gauss_seidel_refusals |
| fitgnn_greedy_matching | n_comp = 1 (no second sort), 2 (one key bit), 3 (two); weights all equal (tie -> edge id), +-0 mixed, NaN (last), +-inf, negatives, denormals; k_keep < 0, 0, 1, more than the matching holds, per component; min_gain = 0, 2 (a component taking <= 2 keeps none, comp_taken still reports the count); sel_off, sel_mem (pair order), sel_count | test_greedy_matching |
| | a star: one live round | test_greedy_matching_star |
| | the unit-weight 300-node path: 150 live rounds (chunks 1, 2 ... 64, then a second chunk of 64) | test_greedy_matching_150_rounds |
| | a path with M > 1024 (the two scans take a second pass), random weights | test_greedy_matching_long_path |
| | N = 0, M = 0: sel_count zeros; comp_taken NULL and rounds NULL; workspace short -> FITGNN_E_WORKSPACE; sel_off NULL refused | test_greedy_matching_empty_and_refusals |
| fitgnn_match_small | both methods x r = 0, 0.5, 0.7 on: 2 nodes, a 3-path (level not applied, levels == 0), a star, K5, weighted rings with chords, the 128-node / 1024-entry limit; assign, cval, Wc, levels as bits | test_match_small |
| | w NULL | test_match_small_unit_weights |
| | K = 1 and 12 (algebraic_JC) | test_match_small_K |
| | max_levels = 0 and 1 | test_match_small_max_levels |
| | over-size component -> FITGNN_MATCH_TOO_BIG (the chain stops there, heavy_edge's other workgroups finish) | test_match_small_too_big |
| | unsorted columns, a diagonal entry, an asymmetric pattern -> FITGNN_MATCH_BAD_INPUT; the chain's progress = {component, draws used} | test_match_small_bad_input |
| | too few draws stops the chain before that component; c_begin == c_end writes {c_begin, 0} | test_match_small_draws_and_empty_range |
| | r outside [0, 1], K = 13, caps over the budget, max_levels < 0, unknown method refused | test_match_small_refusals |

Inputs left out because the reference's own definition is ambiguous there, not the kernel's: NaN proximities out of the weight kernels
(a zero test-vector row divides 0 by 0 in affinity_GS in the reference too) and single-node Gauss-Seidel components (dw = 0).

Bounds that are not bit-exact (u = 2^-53), with the worst observed figure of one MI355X run in brackets:
* affinity_GS: a dot product over the 16-lane xor tree rounds each product once and each of the 4 tree levels once (lanes k >= K add
  exact zeros): x_i.x_j is within gamma_5 cond of its value, cond = sum |x_ik x_jk| / |x_i.x_j|; x_i.x_i and x_j.x_j (sums of squares)
  within gamma_5.  c_e = (ij * ij) / ((ii * ii) * (jj * jj)) squares each (twice the error, one rounding), multiplies and divides:
  relative error a_e = gamma(10 cond + 25), plus 1 for the second-order terms (cond < 1e6 is asserted).  A node's maximum is the
  maximum of the computed c: off by at most the largest a_e c_e of its edges, relative rm_i.  p = c / (mi * mj) rounds twice more:
      p (1 - a)(1 - u)^2 / ((1 + rm_i)(1 + rm_j))  <=  computed float64 p  <=  p (1 + a)(1 + u)^2 / ((1 - rm_i)(1 - rm_j)).
  The float32 proximity must lie between the float32 roundings of the two ends (rounding is monotone: no ulp allowance).
  [on the 288 edges of test_affinity_random the two ends round to the same float32 on every one, so the check was a bit check
  there; worst distance from the rounded reference: 0 ulp]
* variation_edges: d = a_i - a_j rounds once, d * d once more (three factors on d^2), the tree 4 times, * 0.25 and 2 * dw are exact, the
  sum of the degrees and the final product round once each: |cost - ref| <= gamma_9 cond, cond the expression on |terms|.
  [worst error / bound: 0.32]
* Gauss-Seidel against the mathematical order: matching_reference.gauss_seidel's bound (each side within gamma(deg + 1) sum |w v| / dw
  of the exact row given its own earlier rows, plus what those rows pass on).  [worst error / bound: 0.20]
"""
import ctypes

import numpy as np
import pytest
import torch

import matching_reference as mr
from test_gpu_step_kernels import E_BADARG, E_WORKSPACE, L, _call, _dev, _exact, _np, _rng, _run, _same, _strided, _within  # noqa: F401

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
LD = np.longdouble
U64 = 2.0 ** -53
HE, JC = 0, 1                                   # FITGNN_MATCH_HEAVY_EDGE, FITGNN_MATCH_ALGEBRAIC_JC
DONE, TOO_BIG, BAD_INPUT = 1, 2, 3
MAX_NODES, MAX_NNZ = 128, 1024
GUARD = 4
WORST = {}
_DTYPES = {torch.int32: -1, torch.int64: -1, torch.float32: NAN, torch.float64: NAN}      # what a guard / a fresh output holds


def _p(L, t):
    """test_gpu_step_kernels._p; an empty view still gives the address of its (guarded) buffer, where torch's data_ptr() gives NULL:
    a graph without stored entries has an empty col array, not a missing one."""
    if t is None or t.numel():
        return L.dptr(t)
    return ctypes.c_void_p(t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size())


def _in(a, dtype):
    """A host array as a device tensor followed by GUARD guard elements (-1 / NaN)."""
    a = np.array(a)
    buf = torch.full((a.size + GUARD,), _DTYPES[dtype], dtype=dtype, device="cuda")
    if a.size:
        buf[:a.size] = torch.from_numpy(a.ravel()).to(dtype).cuda()
    return buf[:a.size].view(a.shape)


def _out(shape, dtype):
    """(buffer, view): an output of `shape` holding -1 / NaN, followed by GUARD guard elements."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), _DTYPES[dtype], dtype=dtype, device="cuda")
    return buf, buf[:n].view(*(int(v) for v in np.atleast_1d(shape)))


def _untouched(buf, n, what):
    """The elements of buf from n on still hold their -1 / NaN."""
    tail = buf[n:].cpu().numpy()
    ok = np.isnan(tail) if tail.dtype.kind == "f" else tail == _DTYPES[buf.dtype]
    assert ok.all(), f"{what}: wrote past element {n} (at {n + int(np.argmin(ok))})"


def _strided64(A, ld):
    """A [n, K] float64 as a device view with row stride ld; padding columns and the guard behind hold NaN."""
    A = np.asarray(A, dtype=np.float64)
    n, K = A.shape
    buf = torch.full((max(n, 1) * ld + GUARD,), NAN, dtype=torch.float64, device="cuda")
    v = buf[:n * ld].view(n, ld)[:, :K]
    v.copy_(torch.from_numpy(A))
    return v


def _bits_equal(got, ref, what):
    """Bit-for-bit equality of two float arrays of the same type (+0 and -0 differ, NaNs compare by payload)."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    it = np.int32 if got.dtype == np.float32 else np.int64
    bad = got.view(it) != ref.view(it)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:3]} vs {ref[bad][:3]}"


def _ratio(family, err, bound, what):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    pos = bound > 0
    r = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), r)
    print(f"[ratio] {family}: {what}: {r:.3g} (family worst {WORST[family]:.3g})")


def _csr(n, edges, w=None):
    """The symmetric CSR triple (ascending columns) of undirected edges; explicit zeros stay stored."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    wv = np.ones(len(e)) if w is None else np.asarray(w, dtype=np.float64)
    r, c, v = np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]], np.r_[wv, wv]
    o = np.lexsort((c, r))
    return np.r_[0, np.cumsum(np.bincount(r, minlength=n))].astype(np.int64), c[o], v[o]


class Graph:
    """A host graph with its reference edge list; dev() uploads it once.  unit: w is passed as NULL."""

    def __init__(self, n, edges, w=None, unit=False):
        self.N = n
        self.rowptr, self.col, self.w = _csr(n, edges, w)
        self.unit = unit
        assert not unit or w is None
        self.dw = np.zeros(n)
        for i in range(n):
            for p in range(self.rowptr[i], self.rowptr[i + 1]):
                self.dw[i] = self.dw[i] + self.w[p]
        self.edge_off, self.src, self.dst, self.ew, self.csr_eid = mr.edge_list(self.rowptr, self.col, self.w)
        self.M = len(self.src)
        self._d = None

    @property
    def wref(self):
        return None if self.unit else self.w

    def dev(self):
        if self._d is None:
            i32, f64 = torch.int32, torch.float64
            self._d = dict(rowptr=_in(self.rowptr, i32), col=_in(self.col, i32), w=None if self.unit else _in(self.w, f64),
                           dw=_in(self.dw, f64), edge_off=_in(self.edge_off, i32), src=_in(self.src, i32), dst=_in(self.dst, i32),
                           ew=_in(self.ew, f64), csr_eid=_in(self.csr_eid, i32))
        return self._d


def _path_edges(n):
    return [(i + 1, i) for i in range(n - 1)]


def _hub_path(n):
    """A path on n nodes; from 200 nodes on, node n // 2 is a hub with chords to every third node below 210 (degree >= 65)."""
    e = set(_path_edges(n))
    if n >= 200:
        h = n // 2
        e |= {(max(h, t), min(h, t)) for t in range(0, 210, 3) if abs(t - h) > 1}
    return sorted(e)


def _random_edges(rng, n, m):
    """m distinct pairs (i > j) on n nodes in row-major order; every node below min(n, m + 1) has an edge."""
    allp = [(i, j) for i in range(n) for j in range(i)]
    base = [(i, int(rng.integers(0, i))) for i in range(1, min(n, m + 1))]
    rest = [p for p in allp if p not in set(base)]
    pick = rng.permutation(len(rest))[: m - len(base)]
    return sorted(base + [rest[t] for t in pick])


# ---------------------------------------------------------------------------------------------------------------------------------
# fitgnn_edge_list (and scan.h)
# ---------------------------------------------------------------------------------------------------------------------------------
def _edge_list(L, g, m_cap=None, want_ew=True, want_eid=True, null_edges=False):
    d = g.dev()
    m_cap = g.M if m_cap is None else m_cap
    bo, off = _out(g.N + 1, torch.int32)
    bs, src = _out(m_cap, torch.int32)
    bd, dst = _out(m_cap, torch.int32)
    bw, ew = _out(m_cap, torch.float64)
    bi, eid = _out(len(g.col), torch.int32)
    rc = _call(L, "fitgnn_edge_list", _p(L, d["rowptr"]), _p(L, d["col"]), _p(L, d["w"]), g.N, _p(L, off),
               None if null_edges else _p(L, src), None if null_edges else _p(L, dst), _p(L, ew) if want_ew and not null_edges else None,
               m_cap, _p(L, eid) if want_eid else None)
    for b, n, what in ((bo, g.N + 1, "edge_off"), (bs, m_cap, "e_src"), (bd, m_cap, "e_dst"), (bw, m_cap, "e_w"), (bi, len(g.col), "csr_eid")):
        _untouched(b, n, what)
    return rc, off.cpu().numpy(), src.cpu().numpy(), dst.cpu().numpy(), ew.cpu().numpy(), eid.cpu().numpy()


@pytest.mark.parametrize("N", [1, 2, 1023, 1024, 1025, 2049], ids=lambda n: f"N{n}")
def test_edge_list(L, N):
    rng = _rng("edge_list", N)
    e = _hub_path(N)
    g = Graph(N, e, w=rng.integers(1, 64, size=len(e)) / 8.0)
    assert N < 200 or (np.diff(g.rowptr).max() >= 65 and g.edge_off[-1] == g.M > N)
    rc, off, src, dst, ew, eid = _edge_list(L, g)
    L.check(rc, "fitgnn_edge_list")
    assert np.array_equal(off, g.edge_off), f"edge_off differs first at {np.argmax(off != g.edge_off)}"
    assert np.array_equal(src, g.src) and np.array_equal(dst, g.dst) and np.array_equal(eid, g.csr_eid)
    _bits_equal(ew, g.ew, "e_w")


def test_edge_list_empty(L):
    bo, off = _out(1, torch.int32)
    L.check(_call(L, "fitgnn_edge_list", None, None, None, 0, _p(L, off), None, None, None, 0, None), "fitgnn_edge_list")
    assert off.item() == 0
    _untouched(bo, 1, "edge_off")


def test_edge_list_optional_outputs(L):
    e = _hub_path(1025)
    g = Graph(1025, e, unit=True)
    rc, off, src, dst, ew, eid = _edge_list(L, g)                                  # w NULL: unit edge weights
    L.check(rc, "fitgnn_edge_list")
    assert np.array_equal(off, g.edge_off) and np.array_equal(src, g.src) and np.array_equal(dst, g.dst) and np.array_equal(eid, g.csr_eid)
    _bits_equal(ew, np.ones(g.M), "e_w")
    rc, off, src, dst, ew, eid = _edge_list(L, g, want_ew=False, want_eid=False)
    L.check(rc, "fitgnn_edge_list")
    assert np.array_equal(off, g.edge_off) and np.array_equal(src, g.src) and np.array_equal(dst, g.dst)
    assert np.isnan(ew).all() and (eid == -1).all()
    cap = g.M - 37                                                                 # ids >= m_cap are not written (the guards are checked)
    rc, off, src, dst, ew, eid = _edge_list(L, g, m_cap=cap)
    L.check(rc, "fitgnn_edge_list")
    assert np.array_equal(off, g.edge_off) and np.array_equal(src, g.src[:cap]) and np.array_equal(dst, g.dst[:cap])
    _bits_equal(ew, np.ones(cap), "e_w")
    assert np.array_equal(eid, g.csr_eid)                                          # still complete
    rc, off, src, dst, ew, eid = _edge_list(L, g, m_cap=0, null_edges=True)
    L.check(rc, "fitgnn_edge_list")
    assert np.array_equal(off, g.edge_off) and np.array_equal(eid, g.csr_eid)


def test_edge_list_refusals(L):
    g = Graph(5, _path_edges(5))
    d = g.dev()
    _, off = _out(6, torch.int32)
    _, s = _out(4, torch.int32)
    args = lambda N, o, src, cap: (_p(L, d["rowptr"]), _p(L, d["col"]), None, N, o, src, _p(L, s), None, cap, None)  # noqa: E731
    assert _call(L, "fitgnn_edge_list", *args(-1, _p(L, off), _p(L, s), 4)) == E_BADARG
    assert _call(L, "fitgnn_edge_list", *args(5, None, _p(L, s), 4)) == E_BADARG
    assert _call(L, "fitgnn_edge_list", *args(5, _p(L, off), _p(L, s), -1)) == E_BADARG
    assert _call(L, "fitgnn_edge_list", *args(5, _p(L, off), None, 4)) == E_BADARG
    assert (off == -1).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# fitgnn_heavy_edge_proximity
# ---------------------------------------------------------------------------------------------------------------------------------
def _heavy_edge(L, g, short=0):
    d = g.dev()
    wb = int(L.lib().fitgnn_heavy_edge_proximity_workspace_bytes(g.N))
    work = torch.empty(wb + 8, dtype=torch.uint8, device="cuda")
    bp, prox = _out(g.M, torch.float32)
    rc = _call(L, "fitgnn_heavy_edge_proximity", _p(L, d["rowptr"]), _p(L, d["col"]), _p(L, d["w"]), g.N, _p(L, d["src"]), _p(L, d["dst"]),
               _p(L, d["ew"]), g.M, _p(L, prox), _p(L, work), wb - short)
    _untouched(bp, g.M, "prox")
    return rc, prox.cpu().numpy()


@pytest.mark.parametrize("unit", [False, True], ids=["w", "unit"])
@pytest.mark.parametrize("M", [255, 256, 257], ids=lambda m: f"M{m}")
def test_heavy_edge(L, M, unit):
    rng = _rng("heavy_edge", M)
    e = _path_edges(M - 3) + [(M - 4, 0), (M - 5, 1), (M - 6, 2), (M - 7, 3)]      # M edges on M - 3 nodes
    if unit:
        g = Graph(M - 3, e, unit=True)
    else:
        w = rng.integers(1, 9, size=M) / 8.0                                       # ties and both orders of (wmax_src, wmax_dst)
        w[[5, 6]] = [0.0, -0.0]                                                    # stored zeros of both signs and a negative entry:
        w[20] = -0.75                                                              # none of them enters a column maximum
        w[[40, 41]] = [-0.0, -1.5]                                                 # node 41: only such entries, wmax = 0
        g = Graph(M - 3, e, w=w)
        wmax = np.zeros(g.N)
        np.maximum.at(wmax, g.col, np.maximum(g.w, 0.0))
        assert wmax[41] == 0 and (wmax[g.src] > wmax[g.dst]).any() and (wmax[g.src] < wmax[g.dst]).any() and (wmax[g.src] == wmax[g.dst]).any()
    assert g.M == M
    rc, prox = _heavy_edge(L, g)
    L.check(rc, "fitgnn_heavy_edge_proximity")
    _bits_equal(prox, mr.heavy_edge(g.rowptr, g.col, g.wref, g.src, g.dst, g.ew), "prox")


def test_heavy_edge_refusals(L):
    g = Graph(6, _path_edges(6))
    d = g.dev()
    assert _heavy_edge(L, g, short=1)[0] == E_WORKSPACE
    bp, prox = _out(4, torch.float32)
    assert _call(L, "fitgnn_heavy_edge_proximity", None, None, None, 6, None, None, None, 0, _p(L, prox), None, 0) == 0      # M = 0
    assert _call(L, "fitgnn_heavy_edge_proximity", _p(L, d["rowptr"]), _p(L, d["col"]), None, 6, _p(L, d["src"]), _p(L, d["dst"]),
                 None, g.M, _p(L, prox), None, 0) == E_BADARG
    assert _call(L, "fitgnn_heavy_edge_proximity", _p(L, d["rowptr"]), _p(L, d["col"]), None, -1, _p(L, d["src"]), _p(L, d["dst"]),
                 _p(L, d["ew"]), g.M, _p(L, prox), None, 0) == E_BADARG
    assert torch.isnan(bp).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# fitgnn_jc_proximity, fitgnn_affinity_proximity, fitgnn_edge_variation_costs_f64
# ---------------------------------------------------------------------------------------------------------------------------------
PROX_SHAPES = [(K, K + pad, M) for K in (1, 10, 16) for pad in (0, 3) for M in (15, 16, 17)]
PROX_IDS = [f"K{K}-ld{ld}-M{M}" for K, ld, M in PROX_SHAPES]
PN = 12                                         # nodes of the proximity graphs


def _prox_edges(tag, M):
    rng = _rng(tag, M)
    e = np.array(_random_edges(rng, PN, M), dtype=np.int64)
    return rng, e[:, 0].copy(), e[:, 1].copy()


def _edge_kernel(L, fn, src, dst, X, ld, N=None, dw=None, short=0, out_dtype=torch.float32):
    """One of the three K-vector edge kernels on the edge list (src, dst) and the [n, K] matrix X with row stride ld."""
    M, K = len(src), X.shape[1]
    sd, dd, Xd = _in(src, torch.int32), _in(dst, torch.int32), _strided64(X, ld)
    bo, out = _out(M, out_dtype)
    if fn == "fitgnn_jc_proximity":
        rc = _call(L, fn, _p(L, sd), _p(L, dd), M, _p(L, Xd), K, ld, _p(L, out))
    elif fn == "fitgnn_affinity_proximity":
        wb = int(L.lib().fitgnn_affinity_proximity_workspace_bytes(N, M))
        work = torch.empty(wb + 8, dtype=torch.uint8, device="cuda")
        rc = _call(L, fn, N, _p(L, sd), _p(L, dd), M, _p(L, Xd), K, ld, _p(L, out), _p(L, work), wb - short)
    else:
        dwd = _in(dw, torch.float64)
        rc = _call(L, fn, _p(L, sd), _p(L, dd), M, _p(L, dwd), _p(L, Xd), K, ld, _p(L, out))
    _untouched(bo, M, "out")
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("K,ld,M", PROX_SHAPES, ids=PROX_IDS)
def test_jc(L, K, ld, M):
    rng, src, dst = _prox_edges("jc", M)
    X = rng.normal(size=(PN, K)) / np.sqrt(PN)
    t = int(np.nonzero((dst >= 2) & (src != dst[0]) & (src != src[0]))[0][-1])          # an edge away from edge 0's two nodes
    X[dst[t]] = X[src[t]]
    X[dst[t], K - 1] += 2e-3                                 # one column just above the clamp: 1 / 4e-6, not 1e6
    X[dst[0]] = X[src[0]]                                    # twin rows: every difference under the clamp -> 1e6
    ref = mr.jc(src, dst, X)
    assert ref[0] == np.float32(1e6) and 2e5 < ref[t] < 3e5 and len(np.unique(ref)) > M // 2
    rc, prox = _edge_kernel(L, "fitgnn_jc_proximity", src, dst, X, ld)
    L.check(rc, "fitgnn_jc_proximity")
    _bits_equal(prox, ref, "prox")


def _affinity_exact_X(rng, K):
    """Rows of one or two equal powers of two (column 0, and column 1 or 2 where K allows): every dot product, square, product and
    quotient of the expression is a power of two, so the float32 proximity is exact whatever the order."""
    X = np.zeros((PN, K))
    mag = 2.0 ** rng.integers(-2, 3, size=PN)
    X[:, 0] = mag * rng.choice([-1.0, 1.0], size=PN)
    if K >= 3:
        X[np.arange(PN), 1 + np.arange(PN) % 2] = X[:, 0]
    return X


@pytest.mark.parametrize("K,ld,M", PROX_SHAPES, ids=PROX_IDS)
def test_affinity_exact(L, K, ld, M):
    rng, src, dst = _prox_edges("affinity_exact", M)
    X = _affinity_exact_X(rng, K)
    p, c, cmax, _ = mr.affinity(src, dst, X, PN)
    ref = p.astype(np.float32)
    assert np.array_equal(ref.astype(LD), p) and len(np.unique(ref)) >= 3          # representable, and not all the same
    rc, prox = _edge_kernel(L, "fitgnn_affinity_proximity", src, dst, X, ld, N=PN)
    L.check(rc, "fitgnn_affinity_proximity")
    _bits_equal(prox, ref, "prox")


@pytest.mark.parametrize("K,ld,M", PROX_SHAPES, ids=PROX_IDS)
def test_affinity_random(L, K, ld, M):
    rng, src, dst = _prox_edges("affinity_random", M)
    X = rng.normal(size=(PN, K)) / np.sqrt(PN)
    p, c, cmax, cond = mr.affinity(src, dst, X, PN)
    assert ((c < cmax[src]) & (c < cmax[dst])).any()         # an edge both of whose ends have their maximum on another edge
    lo, hi = mr.affinity_interval(src, dst, PN, p, c, cmax, cond)
    rc, prox = _edge_kernel(L, "fitgnn_affinity_proximity", src, dst, X, ld, N=PN)
    L.check(rc, "fitgnn_affinity_proximity")
    lo32, hi32, ref = lo.astype(np.float32), hi.astype(np.float32), p.astype(np.float32)
    d = np.abs(prox.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    WORST["affinity_open"] = WORST.get("affinity_open", 0) + int((lo32 != hi32).sum())
    WORST["affinity_ulp"] = max(WORST.get("affinity_ulp", 0), int(d.max()))
    print(f"[ratio] affinity: K {K} M {M}: interval ends round apart on {int((lo32 != hi32).sum())} edges (total {WORST['affinity_open']}), "
          f"worst distance from the rounded reference {int(d.max())} ulp (family worst {WORST['affinity_ulp']})")
    bad = ~((lo32 <= prox) & (prox <= hi32))
    assert not bad.any(), f"prox outside the rounded interval at {np.argwhere(bad)[:3].tolist()}: {prox[bad][:3]} vs [{lo32[bad][:3]}, {hi32[bad][:3]}]"
    rc, again = _edge_kernel(L, "fitgnn_affinity_proximity", src, dst, X, ld, N=PN)
    _bits_equal(again, prox, "second launch")


@pytest.mark.parametrize("K,ld,M", PROX_SHAPES, ids=PROX_IDS)
def test_edge_cost_exact(L, K, ld, M):
    rng, src, dst = _prox_edges("cost_exact", M)
    A = rng.integers(-8, 9, size=(PN, K)) / 64.0
    dw = rng.integers(0, 21, size=PN) / 4.0
    A[dst[0]] = A[src[0]]                                    # twin rows cost exactly 0.0
    cost, _ = mr.edge_cost(src, dst, dw, A)
    ref = cost.astype(np.float64)
    assert np.array_equal(ref.astype(LD), cost) and ref[0] == 0.0
    rc, got = _edge_kernel(L, "fitgnn_edge_variation_costs_f64", src, dst, A, ld, dw=dw, out_dtype=torch.float64)
    L.check(rc, "fitgnn_edge_variation_costs_f64")
    _bits_equal(got, ref, "cost")


@pytest.mark.parametrize("K,ld,M", PROX_SHAPES, ids=PROX_IDS)
def test_edge_cost_random(L, K, ld, M):
    rng, src, dst = _prox_edges("cost_random", M)
    A = rng.normal(size=(PN, K))
    dw = rng.uniform(0.5, 9.0, size=PN)
    A[dst[0]] = A[src[0]]
    cost, cond = mr.edge_cost(src, dst, dw, A)
    rc, got = _edge_kernel(L, "fitgnn_edge_variation_costs_f64", src, dst, A, ld, dw=dw, out_dtype=torch.float64)
    L.check(rc, "fitgnn_edge_variation_costs_f64")
    assert got[0] == 0.0
    err = np.abs(got.astype(LD) - cost).astype(np.float64)
    bound = (9 * U64 / (1 - 9 * U64) * cond).astype(np.float64)
    _ratio("edge_cost", err, bound, f"K {K} M {M}")
    assert (err <= bound).all(), f"cost: worst error / bound {(err / np.maximum(bound, 1e-300)).max()}"
    rc, again = _edge_kernel(L, "fitgnn_edge_variation_costs_f64", src, dst, A, ld, dw=dw, out_dtype=torch.float64)
    _bits_equal(again, got, "second launch")


def test_proximity_refusals(L):
    _, src, dst = _prox_edges("refusals", 15)
    X = np.ones((PN, 16))
    dw = np.ones(PN)
    sd, dd, Xd, dwd = _in(src, torch.int32), _in(dst, torch.int32), _strided64(X, 16), _in(dw, torch.float64)
    bo, o32 = _out(15, torch.float32)
    b6, o64 = _out(15, torch.float64)
    wb = int(L.lib().fitgnn_affinity_proximity_workspace_bytes(PN, 15))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    s, d, x, o, o6, dwp, wk = _p(L, sd), _p(L, dd), _p(L, Xd), _p(L, o32), _p(L, o64), _p(L, dwd), _p(L, work)
    jc = lambda *a: _call(L, "fitgnn_jc_proximity", *a)                             # noqa: E731
    af = lambda *a: _call(L, "fitgnn_affinity_proximity", PN, *a)                   # noqa: E731
    ec = lambda *a: _call(L, "fitgnn_edge_variation_costs_f64", *a)                 # noqa: E731
    for K, ld, M in ((0, 16, 15), (17, 17, 15), (10, 9, 15), (10, 16, -1)):
        assert jc(s, d, M, x, K, ld, o) == E_BADARG, (K, ld, M)
        assert af(s, d, M, x, K, ld, o, wk, wb) == E_BADARG, (K, ld, M)
        assert ec(s, d, M, dwp, x, K, ld, o6) == E_BADARG, (K, ld, M)
    assert jc(None, d, 15, x, 10, 16, o) == E_BADARG and jc(s, d, 15, None, 10, 16, o) == E_BADARG and jc(s, d, 15, x, 10, 16, None) == E_BADARG
    assert af(s, None, 15, x, 10, 16, o, wk, wb) == E_BADARG and af(s, d, 15, x, 10, 16, o, None, wb) == E_BADARG
    assert ec(s, d, 15, None, x, 10, 16, o6) == E_BADARG and ec(s, d, 15, dwp, x, 10, 16, None) == E_BADARG
    assert af(s, d, 15, x, 10, 16, o, wk, wb - 1) == E_WORKSPACE
    assert jc(None, None, 0, None, 10, 16, None) == 0 and af(None, None, 0, None, 10, 16, None, None, 0) == 0     # M = 0
    assert ec(None, None, 0, None, None, 10, 16, None) == 0
    assert torch.isnan(bo).all() and torch.isnan(b6).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# fitgnn_jacobi_vectors_f64
# ---------------------------------------------------------------------------------------------------------------------------------
def _jacobi_graph(N, unit=False):
    """A ring with chords on nodes 0 .. N - 2 and the isolated node N - 1; weights in tenths (f32(dw) != dw) unless unit."""
    rng = _rng("jacobi_graph", N)
    n = N - 1
    e = sorted({(max(i, (i + 1) % n), min(i, (i + 1) % n)) for i in range(n)} | {(n // 2, 0), (n - 2, 3), (9, 2)})
    return Graph(N, e, unit=True) if unit else Graph(N, e, w=rng.integers(1, 30, size=len(e)) / 10.0)


def _jacobi(L, g, X0, iterations, null_work=False, short=0, alias=False):
    d = g.dev()
    N, K = X0.shape
    X0d = _in(X0, torch.float64)
    bx, X = _out((N, K), torch.float64)
    wb = int(L.lib().fitgnn_jacobi_vectors_workspace_bytes(N, K))
    bw, work = _out(wb // 8, torch.float64)
    rc = _call(L, "fitgnn_jacobi_vectors_f64", _p(L, d["rowptr"]), _p(L, d["col"]), _p(L, d["w"]), _p(L, d["dw"]), N, _p(L, X0d), K, iterations,
               _p(L, X0d) if alias else _p(L, X), None if null_work else _p(L, work), 0 if null_work else wb - short)
    _untouched(bx, N * K, "X")
    _untouched(bw, wb // 8, "work")
    return rc, X.cpu().numpy()


@pytest.mark.parametrize("N,K", [(15, 1), (16, 10), (17, 16)], ids=lambda v: str(v))
@pytest.mark.parametrize("iterations", [0, 1, 2, 3, 20], ids=lambda v: f"it{v}")
def test_jacobi(L, iterations, N, K):
    g = _jacobi_graph(N)
    assert g.dw[N - 1] == 0 and (g.dw.astype(np.float32).astype(np.float64) != g.dw).any()
    X0 = _rng("jacobi", N, K).normal(size=(N, K)) / np.sqrt(N)
    rc, X = _jacobi(L, g, X0, iterations, null_work=iterations <= 1)
    L.check(rc, "fitgnn_jacobi_vectors_f64")
    ref = mr.jacobi(g.rowptr, g.col, g.w, g.dw, X0, iterations)
    assert iterations == 0 or np.array_equal(ref[N - 1], 0.5 ** iterations * X0[N - 1])      # the isolated node
    _bits_equal(X, ref, "X")


def test_jacobi_unit_weights(L):
    g = _jacobi_graph(16, unit=True)
    X0 = _rng("jacobi_unit").normal(size=(16, 10))
    rc, X = _jacobi(L, g, X0, 20)
    L.check(rc, "fitgnn_jacobi_vectors_f64")
    _bits_equal(X, mr.jacobi(g.rowptr, g.col, None, g.dw, X0, 20), "X")


def test_jacobi_refusals(L):
    g = _jacobi_graph(16)
    X0 = np.ones((16, 10))
    assert _jacobi(L, g, X0, 2, alias=True)[0] == E_BADARG
    assert _jacobi(L, g, X0, 2, short=1)[0] == E_WORKSPACE
    assert _jacobi(L, g, X0, 2, null_work=True)[0] == E_BADARG
    assert _jacobi(L, g, X0, -1)[0] == E_BADARG
    assert _jacobi(L, g, np.ones((16, 17)), 1)[0] == E_BADARG
    rc, X = _jacobi(L, g, X0, 1, short=1)                    # one step needs no workspace
    assert rc == 0 and not np.isnan(X).any()
    assert _call(L, "fitgnn_jacobi_vectors_f64", None, None, None, None, 0, None, 10, 20, None, None, 0) == 0      # N = 0


# ---------------------------------------------------------------------------------------------------------------------------------
# fitgnn_gauss_seidel_vectors_f64
# ---------------------------------------------------------------------------------------------------------------------------------
def _gs_components():
    """(edges, size) of a 2-node component, a 40-node component with rows of degree 1, 3, 4, 5 and 9, and a 200-node path."""
    c40 = set(_path_edges(40)) | {(t, 10) for t in range(20, 27)} | {(33, 30), (35, 30)} | {(15, 2), (15, 5), (37, 15)}
    return [([(1, 0)], 2), (sorted(c40), 40), (_path_edges(200), 200)]


def _gs_graph(which, unit):
    comps = _gs_components()
    rng = _rng("gs_graph", which)
    edges, off = [], [0]
    for c in which:
        e, n = comps[c]
        edges += [(i + off[-1], j + off[-1]) for i, j in e]
        off.append(off[-1] + n)
    g = Graph(off[-1], edges, unit=True) if unit else Graph(off[-1], edges, w=rng.integers(1, 40, size=len(edges)) / 10.0)
    return g, np.array(off, dtype=np.int64)


def _gauss_seidel(L, g, comp_off, X0, alias=False):
    d = g.dev()
    N, K = X0.shape
    X0d, cod = _in(X0, torch.float64), _in(comp_off, torch.int32)
    bx, X = _out((N, K), torch.float64)
    rc = _call(L, "fitgnn_gauss_seidel_vectors_f64", _p(L, d["rowptr"]), _p(L, d["col"]), _p(L, d["w"]), _p(L, d["dw"]), N, len(comp_off) - 1,
               _p(L, cod), _p(L, X0d), K, _p(L, X0d) if alias else _p(L, X))
    _untouched(bx, N * K, "X")
    return rc, X.cpu().numpy()


@pytest.mark.parametrize("unit", [False, True], ids=["w", "unit"])
@pytest.mark.parametrize("K", [1, 10, 16], ids=lambda k: f"K{k}")
@pytest.mark.parametrize("which", [(0, 1, 2), (1,), (2,)], ids=["three", "c40", "path200"])
def test_gauss_seidel(L, which, K, unit):
    g, off = _gs_graph(which, unit)
    if 1 in which:
        assert {1, 3, 4, 5, 9} <= set(np.diff(g.rowptr).tolist())
    X0 = _rng("gs", which, K).normal(size=(g.N, K)) / np.sqrt(g.N)
    rc, X = _gauss_seidel(L, g, off, X0)
    L.check(rc, "fitgnn_gauss_seidel_vectors_f64")
    _bits_equal(X, mr.gauss_seidel_ordered(g.rowptr, g.col, g.wref, g.dw, off, X0), "X against the ordered reference")
    ref, bound = mr.gauss_seidel(g.rowptr, g.col, g.wref, g.dw, off, X0)
    _ratio("gauss_seidel", np.abs(X - ref), bound, f"{which} K {K}")
    _within(X, ref, bound, "X against the mathematical reference")


def test_gauss_seidel_refusals(L):
    g, off = _gs_graph((1,), False)
    X0 = np.ones((40, 10))
    assert _gauss_seidel(L, g, off, X0, alias=True)[0] == E_BADARG
    assert _gauss_seidel(L, g, off, np.ones((40, 17)))[0] == E_BADARG
    d = g.dev()
    bx, X = _out((40, 10), torch.float64)
    X0d = _in(X0, torch.float64)
    for K, n_comp in ((0, 1), (10, -1)):
        assert _call(L, "fitgnn_gauss_seidel_vectors_f64", _p(L, d["rowptr"]), _p(L, d["col"]), None, _p(L, d["dw"]), 40, n_comp, None, _p(L, X0d), K,
                     _p(L, X)) == E_BADARG
    assert _call(L, "fitgnn_gauss_seidel_vectors_f64", None, None, None, None, 40, 0, None, None, 10, None) == 0        # n_comp = 0
    assert torch.isnan(bx).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# fitgnn_greedy_matching
# ---------------------------------------------------------------------------------------------------------------------------------
def _greedy(L, g, weight, comp_off=None, k_keep=None, min_gain=0, want_taken=True, want_rounds=True, short=0):
    d = g.dev()
    comp_off = np.array([0, g.N]) if comp_off is None else np.asarray(comp_off)
    n_comp = len(comp_off) - 1
    k_keep = np.broadcast_to(np.asarray(g.N if k_keep is None else k_keep, dtype=np.int64), (n_comp,))
    wd, cod, kd = _in(weight, torch.float64), _in(comp_off, torch.int32), _in(k_keep, torch.int64)
    wb = int(L.lib().fitgnn_greedy_matching_workspace_bytes(g.N, g.M, n_comp))
    work = torch.empty(wb + 8, dtype=torch.uint8, device="cuda")
    bo, sel_off = _out(g.N + 1, torch.int32)
    bm, sel_mem = _out(g.N, torch.int32)
    bc, sel_count = _out(2, torch.int32)
    bt, taken = _out(n_comp, torch.int32)
    rounds = ctypes.c_int32(-7)
    rc = _call(L, "fitgnn_greedy_matching", _p(L, d["rowptr"]), _p(L, d["col"]), _p(L, d["csr_eid"]), g.N, _p(L, d["edge_off"]), _p(L, d["src"]),
               _p(L, d["dst"]), g.M, _p(L, wd), n_comp, _p(L, cod), _p(L, kd), min_gain, _p(L, sel_off), _p(L, sel_mem), _p(L, sel_count),
               _p(L, taken) if want_taken else None, ctypes.byref(rounds) if want_rounds else None, _p(L, work), wb - short)
    for b, n, what in ((bo, g.N + 1, "sel_off"), (bm, g.N, "sel_mem"), (bc, 2, "sel_count"), (bt, n_comp, "comp_taken")):
        _untouched(b, n, what)
    return rc, sel_off.cpu().numpy(), sel_mem.cpu().numpy(), sel_count.cpu().numpy(), taken.cpu().numpy(), rounds.value


def _check_greedy(g, weight, comp_off, k_keep, min_gain, res):
    rc, sel_off, sel_mem, sel_count, taken, rounds = res
    assert rc == 0, rc
    pairs, ref_taken, ref_off, ref_count = mr.stable_greedy(g.src, g.dst, weight, g.N, comp_off, k_keep, min_gain)
    S = len(pairs)
    assert sel_count.tolist() == ref_count.tolist(), (sel_count, ref_count)
    assert np.array_equal(sel_off[:S + 1], ref_off) and (sel_off[S + 1:] == -1).all()
    assert np.array_equal(sel_mem[:2 * S].reshape(-1, 2), pairs), "pairs differ (members, their order, or the pair order)"
    assert (sel_mem[2 * S:] == -1).all()
    assert np.array_equal(taken, ref_taken), (taken, ref_taken)
    return pairs, rounds


def _three_components():
    """Random connected components of 7, 20 and 33 nodes in one block graph; comp_off for 1, 2 and 3 components."""
    rng = _rng("greedy_components")
    edges, base = [], 0
    for n, m in ((7, 12), (20, 45), (33, 80)):
        edges += [(i + base, j + base) for i, j in _random_edges(rng, n, m)]
        base += n
    return Graph(60, edges), {1: [0, 60], 2: [0, 27, 60], 3: [0, 7, 27, 60]}


def _weights(kind, M):
    rng = _rng("greedy_weights", kind)
    tiny = 5e-324
    if kind == "equal":
        return np.full(M, 0.5)
    if kind == "zeros":
        return rng.choice([0.0, -0.0, 1.0], size=M)
    if kind == "negative":                                   # variation_edges passes -cost
        return -rng.uniform(0.0, 3.0, size=M)
    assert kind == "special"
    return rng.choice([NAN, INF, -INF, 0.0, -0.0, tiny, -tiny, 3 * tiny, 1.0, -1.0, 2.5, 1e300, -1e300], size=M)


@pytest.mark.parametrize("min_gain", [0, 2], ids=lambda v: f"gain{v}")
@pytest.mark.parametrize("kind", ["equal", "zeros", "special", "negative"])
@pytest.mark.parametrize("n_comp", [1, 2, 3], ids=lambda v: f"comp{v}")
def test_greedy_matching(L, n_comp, kind, min_gain):
    g, offs = _three_components()
    off = offs[n_comp]
    weight = _weights(kind, g.M)
    if kind == "special":
        assert np.isnan(weight).sum() >= 2 and (weight == 0).sum() >= 2 and np.signbit(weight[weight == 0]).any()
    ref_rounds = mr.dominant_rounds(g.rowptr, g.col, g.csr_eid, g.src, g.dst, weight, g.N, off)[0]
    for k_keep in ([1000, 1000, 1000][:n_comp], [1, 0, -5][:n_comp], [-1, 1000, 1][-n_comp:], [3, 2, 4][:n_comp]):
        _, rounds = _check_greedy(g, weight, off, k_keep, min_gain, _greedy(L, g, weight, off, k_keep, min_gain))
        assert rounds == ref_rounds                          # the rounds make the whole matching, whatever is kept of it


def test_greedy_matching_star(L):
    n = 70
    g = Graph(n, [(i, 0) for i in range(1, n)])
    weight = _rng("star").uniform(size=g.M)
    pairs, rounds = _check_greedy(g, weight, None, None, 0, _greedy(L, g, weight))
    assert rounds == 1 and pairs.tolist() == [[int(np.argmax(weight)) + 1, 0]]


def test_greedy_matching_150_rounds(L):
    g = Graph(300, _path_edges(300))
    weight = np.ones(g.M)
    ref_rounds, _ = mr.dominant_rounds(g.rowptr, g.col, g.csr_eid, g.src, g.dst, weight, g.N)
    assert ref_rounds == 150                                 # chunks of 1, 2 ... 64 rounds reach 127; the second chunk of 64 ends it
    pairs, rounds = _check_greedy(g, weight, None, None, 0, _greedy(L, g, weight))
    assert rounds == ref_rounds and len(pairs) == 150


def test_greedy_matching_long_path(L):
    g = Graph(1500, _path_edges(1500))
    assert g.M > 1024
    weight = _rng("long_path").integers(0, 50, size=g.M).astype(np.float64)          # ties among 1499 edges
    for k_keep, min_gain in ((None, 0), (400, 0), (2, 2)):
        _, rounds = _check_greedy(g, weight, None, k_keep, min_gain, _greedy(L, g, weight, None, k_keep, min_gain))
    assert rounds == mr.dominant_rounds(g.rowptr, g.col, g.csr_eid, g.src, g.dst, weight, g.N)[0]


def test_greedy_matching_empty_and_refusals(L):
    g, offs = _three_components()
    weight = _weights("negative", g.M)
    res = _greedy(L, g, weight, offs[3], None, 0, want_taken=False, want_rounds=False)
    assert (res[4] == -1).all() and res[5] == -7                                     # neither was written
    ref = mr.stable_greedy(g.src, g.dst, weight, g.N, offs[3])
    assert res[0] == 0 and res[3].tolist() == ref[3].tolist() and np.array_equal(res[2][:2 * len(ref[0])].reshape(-1, 2), ref[0])
    assert _greedy(L, g, weight, offs[3], short=1)[0] == E_WORKSPACE
    iso = Graph(5, [])                                                               # M = 0
    rc, sel_off, sel_mem, sel_count, taken, rounds = _greedy(L, iso, np.zeros(0))
    assert rc == 0 and sel_count.tolist() == [0, 0] and sel_off[0] == 0 and (sel_mem == -1).all() and taken.tolist() == [0] and rounds == 0
    empty = Graph(0, [])                                                             # N = 0
    rc, sel_off, sel_mem, sel_count, taken, rounds = _greedy(L, empty, np.zeros(0), comp_off=[0, 0])
    assert rc == 0 and sel_count.tolist() == [0, 0] and sel_off[0] == 0 and rounds == 0
    d = g.dev()
    _, cnt = _out(2, torch.int32)
    assert _call(L, "fitgnn_greedy_matching", _p(L, d["rowptr"]), _p(L, d["col"]), _p(L, d["csr_eid"]), g.N, _p(L, d["edge_off"]), _p(L, d["src"]),
                 _p(L, d["dst"]), g.M, None, 1, None, None, 0, None, None, _p(L, cnt), None, None, None, 0) == E_BADARG
    assert (cnt == -1).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# fitgnn_match_small
# ---------------------------------------------------------------------------------------------------------------------------------
def _ring_chords(n, seed, weighted=True, extra=2):
    rng = _rng("ring", n, seed)
    e = {(max(i, (i + 1) % n), min(i, (i + 1) % n)) for i in range(n)}
    while len(e) < n + extra:
        a, b = sorted(int(v) for v in rng.integers(0, n, size=2))
        if a != b:
            e.add((b, a))
    e = sorted(e)
    return _csr(n, e, rng.integers(4, 17, size=len(e)) / 8.0 if weighted else None)


def _small_components(weighted=True):
    """2 nodes, a 3-path, a star, K5, rings with chords (6, 14, 23 nodes), and the 128-node / 1024-entry limit."""
    comps = [_csr(2, [(1, 0)]), _csr(3, [(1, 0), (2, 1)]), _csr(9, [(i, 0) for i in range(1, 9)]),
             _csr(5, [(i, j) for i in range(5) for j in range(i)])]
    comps += [_ring_chords(n, 1, weighted) for n in (6, 14, 23)]
    comps.append(_ring_chords(128, 2, weighted, extra=512 - 128))
    assert len(comps[-1][1]) == MAX_NNZ
    return comps


def _match_small(L, method, comps, r, K=10, max_levels=10, max_level_r=0.99, draws=None, n_draws=None, c_begin=0, c_end=None,
                 max_nodes=None, max_nnz=None, unit=False, null_progress=False):
    """fitgnn_match_small on the block-diagonal graph of the CSR triples `comps`; every output as a host array."""
    sizes = [len(c[0]) - 1 for c in comps]
    off = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    poff = np.r_[0, np.cumsum([len(c[1]) for c in comps])].astype(np.int64)
    rowptr = np.concatenate([[0]] + [np.asarray(c[0][1:]) + poff[i] for i, c in enumerate(comps)])
    col = np.concatenate([np.asarray(c[1]) + off[i] for i, c in enumerate(comps)])
    w = np.concatenate([np.asarray(c[2], dtype=np.float64) for c in comps])
    n_comp, N0, nnz = len(comps), int(off[-1]), int(poff[-1])
    c_end = n_comp if c_end is None else c_end
    i32, f64 = torch.int32, torch.float64
    bufs = {}
    out = {}
    for name, n, dt in (("assign", N0, i32), ("cval", N0, f64), ("n_out", n_comp, i32), ("levels", n_comp, i32), ("status", n_comp, i32),
                        ("wc_rowptr", N0 + n_comp + 1, i32), ("wc_col", nnz, i32), ("wc_w", nnz, f64), ("progress", 2, torch.int64)):
        bufs[name], out[name] = _out(n, dt)
    dr = None if draws is None else _in(draws, f64)
    sq = _in(np.sqrt(np.arange(MAX_NODES + 1)), f64)
    rd, cd, wd, od = _in(rowptr, i32), _in(col, i32), _in(w, f64), _in(off, i32)     # named: they must outlive the call
    rc = _call(L, "fitgnn_match_small", method, _p(L, rd), _p(L, cd), None if unit else _p(L, wd),
               _p(L, od), c_begin, c_end, r, K, max_levels, max_level_r, _p(L, dr),
               (0 if draws is None else len(draws)) if n_draws is None else n_draws, _p(L, sq) if method == JC else None,
               max(sizes) if max_nodes is None else max_nodes, max(len(c[1]) for c in comps) if max_nnz is None else max_nnz,
               _p(L, out["assign"]), _p(L, out["cval"]), _p(L, out["n_out"]), _p(L, out["levels"]), _p(L, out["status"]), _p(L, out["wc_rowptr"]),
               _p(L, out["wc_col"]), _p(L, out["wc_w"]), None if null_progress or method != JC else _p(L, out["progress"]))
    for name, b in bufs.items():
        _untouched(b, out[name].numel(), name)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(rc=rc, off=off, poff=poff)
    return res


_REFS = {}


def _small_refs(tag, comps, method, r, K, max_levels, draws, unit=False):
    """coarsen_levels of every component, the draws running on from one component to the next; made once per case."""
    key = (tag, method, r, K, max_levels, unit)
    if key not in _REFS:
        used, refs = 0, []
        for rp, col, w in comps:
            ref = mr.coarsen_levels(rp, col, None if unit else w, r, "algebraic_JC" if method == JC else "heavy_edge", K,
                                    None if draws is None else draws[used:], max_levels, 0.99)
            used += ref[4]
            refs.append(ref)
        _REFS[key] = (refs, used)
    return _REFS[key]


def _check_small(res, comps, refs, which=None):
    """Component c of the launch against its reference: assign, cval, Wc, levels bit for bit, the rest of its slots untouched."""
    off, poff = res["off"], res["poff"]
    for c in (range(len(comps)) if which is None else which):
        assign, cval, (wr, wc, ww), levels, _ = refs[c]
        b, e, p0, p1 = int(off[c]), int(off[c + 1]), int(poff[c]), int(poff[c + 1])
        n, nz = len(wr) - 1, len(wc)
        assert res["status"][c] == DONE and res["n_out"][c] == n and res["levels"][c] == levels, (c, res["status"][c], res["n_out"][c], res["levels"][c], n, levels)
        assert np.array_equal(res["assign"][b:e], assign), c
        _bits_equal(res["cval"][b:e], cval, f"cval of component {c}")
        assert np.array_equal(res["wc_rowptr"][b + c: b + c + n + 1], wr), c
        assert (res["wc_rowptr"][b + c + n + 1: e + c + 1] == -1).all(), c
        assert np.array_equal(res["wc_col"][p0: p0 + nz], wc), c
        _bits_equal(res["wc_w"][p0: p0 + nz], ww, f"Wc of component {c}")
        assert (res["wc_col"][p0 + nz: p1] == -1).all() and np.isnan(res["wc_w"][p0 + nz: p1]).all(), c


def _draw_pool(comps, K, max_levels, tag):
    return _rng("draws", tag).normal(size=int(sum(K * (len(c[0]) - 1) * max_levels for c in comps)))


@pytest.mark.parametrize("r", [0.0, 0.5, 0.7], ids=lambda v: f"r{v}")
@pytest.mark.parametrize("method", [HE, JC], ids=["heavy_edge", "algebraic_JC"])
def test_match_small(L, method, r):
    comps = _small_components()
    draws = _draw_pool(comps, 10, 10, "main") if method == JC else None
    refs, used = _small_refs("main", comps, method, r, 10, 10, draws)
    lv = [ref[3] for ref in refs]
    assert lv[0] == lv[1] == lv[3] == 0 and max(lv) == (0 if r == 0.0 else 1 if (method, r) == (JC, 0.5) else 2)
    res = _match_small(L, method, comps, r, draws=draws)
    assert res["rc"] == 0
    _check_small(res, comps, refs)
    if method == JC:
        assert res["progress"].tolist() == [len(comps), used]


@pytest.mark.parametrize("method", [HE, JC], ids=["heavy_edge", "algebraic_JC"])
def test_match_small_unit_weights(L, method):
    comps = _small_components(weighted=False)[:7]
    draws = _draw_pool(comps, 10, 10, "unit") if method == JC else None
    refs, used = _small_refs("unit", comps, method, 0.5, 10, 10, draws, unit=True)
    res = _match_small(L, method, comps, 0.5, draws=draws, unit=True)
    assert res["rc"] == 0
    _check_small(res, comps, refs)


@pytest.mark.parametrize("K", [1, 12], ids=lambda v: f"K{v}")
def test_match_small_K(L, K):
    comps = _small_components()[2:7]
    draws = _draw_pool(comps, K, 10, K)
    refs, used = _small_refs("K", comps, JC, 0.6, K, 10, draws)
    res = _match_small(L, JC, comps, 0.6, K=K, draws=draws)
    assert res["rc"] == 0 and res["progress"].tolist() == [len(comps), used]
    _check_small(res, comps, refs)


@pytest.mark.parametrize("max_levels", [0, 1])
@pytest.mark.parametrize("method", [HE, JC], ids=["heavy_edge", "algebraic_JC"])
def test_match_small_max_levels(L, method, max_levels):
    comps = _small_components()[2:7]
    draws = _draw_pool(comps, 10, max_levels, "levels") if method == JC and max_levels else None
    refs, used = _small_refs("levels", comps, method, 0.7, 10, max_levels, draws)
    assert max(ref[3] for ref in refs) == max_levels
    res = _match_small(L, method, comps, 0.7, max_levels=max_levels, draws=draws)
    assert res["rc"] == 0
    _check_small(res, comps, refs)


@pytest.mark.parametrize("method", [HE, JC], ids=["heavy_edge", "algebraic_JC"])
def test_match_small_too_big(L, method):
    comps = _small_components()[2:7]                         # star 9, K5, rings of 6, 14, 23 nodes
    draws = _draw_pool(comps, 10, 10, "too_big") if method == JC else None
    refs, used = _small_refs("too_big", comps[:3], method, 0.5, 10, 10, draws)
    res = _match_small(L, method, comps, 0.5, draws=draws, max_nodes=22)           # the 23-node ring is over the cap
    assert res["rc"] == 0 and res["status"][4] == TOO_BIG
    _check_small(res, comps, refs, which=(0, 1, 2))
    b = int(res["off"][4])
    assert (res["assign"][b:] == -1).all() and np.isnan(res["cval"][b:]).all()     # nothing of it was written
    if method == JC:                                                               # the chain stops there
        assert res["progress"].tolist()[0] == 4 and res["status"][3] == DONE
    res = _match_small(L, method, comps, 0.5, draws=draws, max_nnz=len(comps[4][1]) - 1)
    assert res["rc"] == 0 and res["status"][4] == TOO_BIG and (res["status"][:3] == DONE).all()


def _bad_components():
    lower = ([0, 0, 1, 3, 6], [0, 0, 1, 0, 1, 2], np.ones(6))                       # only the lower triangle of K4 is stored
    unsorted = ([0, 2, 3, 4], [2, 1, 0, 0], np.ones(4))                             # row 0 holds columns 2, 1
    diagonal = ([0, 2, 3, 4], [0, 1, 0, 2], np.ones(4))                             # (0, 0) and (2, 2) are stored
    return {"asymmetric": lower, "unsorted": unsorted, "diagonal": diagonal}


@pytest.mark.parametrize("kind", ["asymmetric", "unsorted", "diagonal"])
@pytest.mark.parametrize("method", [HE, JC], ids=["heavy_edge", "algebraic_JC"])
def test_match_small_bad_input(L, method, kind):
    small = _csr(4, [(1, 0), (2, 1), (3, 2), (3, 0)])
    comps = [small, _bad_components()[kind], small]
    comps = [(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(c, dtype=np.float64)) for a, b, c in comps]
    draws = _draw_pool([small] * 3, 10, 10, "bad") if method == JC else None   # the worst case of three 4-node components
    refs, used = _small_refs("bad", [small], method, 0.5, 10, 10, draws)
    # max_nnz = 8 entries (the 4-ring's), so the edge arrays hold 4 edges: the lower-only K4 has 6
    res = _match_small(L, method, comps, 0.5, draws=draws, max_nodes=4, max_nnz=8)
    assert res["rc"] == 0 and res["status"][1] == BAD_INPUT
    _check_small(res, comps, [refs[0]], which=(0,))
    if method == JC:                                                               # the chain stops: component 2 is not run
        assert res["progress"].tolist() == [1, used] and res["status"][2] == -1
    else:
        assert res["status"][2] == DONE


def test_match_small_draws_and_empty_range(L):
    sc = _small_components()
    comps = [sc[3], sc[4], sc[2], sc[5]]                     # 5, 6, 9, 14 nodes: the worst-case need K * N * max_levels grows
    K, ml = 10, 10
    draws = _draw_pool(comps, K, ml, "few")
    refs, _ = _small_refs("few", comps, JC, 0.5, K, ml, draws)
    need = [K * (len(c[0]) - 1) * ml for c in comps]
    used3 = refs[0][4] + refs[1][4] + refs[2][4]
    # the pool covers components 0, 1 and 2 and the worst case of component 3 less one draw
    res = _match_small(L, JC, comps, 0.5, draws=draws, n_draws=used3 + need[3] - 1)
    assert res["rc"] == 0 and res["progress"].tolist() == [3, used3] and res["status"].tolist() == [DONE, DONE, DONE, -1]
    _check_small(res, comps, refs, which=(0, 1, 2))
    res = _match_small(L, JC, comps, 0.5, draws=draws, c_begin=2, c_end=2)          # an empty range
    assert res["rc"] == 0 and res["progress"].tolist() == [2, 0] and (res["status"] == -1).all() and (res["assign"] == -1).all()
    res = _match_small(L, HE, comps, 0.5, c_begin=1, c_end=1)
    assert res["rc"] == 0 and (res["status"] == -1).all()
    # a range inside the sequence: components 1 and 2 only, the draws from the start of the pool
    refs12, used12 = _small_refs("few12", comps[1:3], JC, 0.5, K, ml, draws)
    res = _match_small(L, JC, comps, 0.5, draws=draws, c_begin=1, c_end=3)
    assert res["progress"].tolist() == [3, used12] and res["status"].tolist() == [-1, DONE, DONE, -1]
    _check_small(res, comps, [None] + refs12, which=(1, 2))


def test_match_small_refusals(L):
    comps = _small_components()[2:4]
    draws = _draw_pool(comps, 10, 10, "refusals")
    for kw in (dict(r=-0.1), dict(r=1.1), dict(r=NAN), dict(r=0.5, K=13), dict(r=0.5, K=0), dict(r=0.5, max_nodes=MAX_NODES + 1),
               dict(r=0.5, max_nnz=MAX_NNZ + 1), dict(r=0.5, max_levels=-1), dict(r=0.5, max_level_r=1.5), dict(r=0.5, c_begin=2, c_end=1),
               dict(r=0.5, null_progress=True), dict(r=0.5, n_draws=-1)):
        res = _match_small(L, JC, comps, draws=draws, **kw)
        assert res["rc"] == E_BADARG, kw
        assert (res["status"] == -1).all() and (res["assign"] == -1).all() and (res["progress"] == -1).all(), kw
    assert _match_small(L, 2, comps, 0.5)["rc"] == E_BADARG                          # unknown method
    assert _match_small(L, HE, comps, 0.5, max_nodes=MAX_NODES + 1)["rc"] == E_BADARG
    assert _match_small(L, HE, comps, 0.5, K=13)["rc"] == 0                          # heavy_edge has no test vectors: K is not read
