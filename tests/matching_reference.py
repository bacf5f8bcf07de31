"""Plain NumPy statements of the matching-based coarsening stages of csrc/matching.hip and csrc/match_small.hip (test infrastructure
only): the edge list, the four edge weights (heavy_edge, algebraic_JC, affinity_GS, variation_edges), the Jacobi and Gauss-Seidel
test vectors, the matching's sort order, the sequential greedy matching, the count of locally-dominant rounds, and the whole
multilevel loop of a small component.  Written from the reference's definition (graph_coarsening/coarsening_utils.py: proximities
:658-730, test vectors :813-848, matching_greedy :931-993, coarsen :60-182) and the order DESIGN.md "Matching methods" fixes.

A graph is its CSR triple (rowptr, col, w): symmetric, columns ascending in every row, no diagonal; w None means unit weights.  An
edge list is tril(W) in row-major order: edge e = (src[e], dst[e]) with src > dst.

Two kinds of function.  Where every operation and its order is fixed by the definition (heavy_edge, jc, jacobi, gauss_seidel_ordered,
the level loop) the function evaluates one IEEE float64 operation at a time in that order and the tests hold the kernels to its bits.
Where the order is the kernel's own choice (affinity, edge_cost, gauss_seidel) the function returns the value in higher precision
(np.longdouble) or in the mathematical order, together with the condition the tests' bounds need.
tests/test_matching_reference_cpu.py checks all of them against what the unmodified reference recorded.
"""
import numpy as np

LD = np.longdouble
JACOBI_STEPS = 20


def _w(rowptr, w):
    return np.ones(int(rowptr[-1])) if w is None else np.asarray(w, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# edge list
# ---------------------------------------------------------------------------------------------------------------------------------
def edge_list(rowptr, col, w=None):
    """tril(W) in row-major order (get_edge_list()): (edge_off [N + 1], src, dst, ew, csr_eid); edge_off[i] = edges of the rows
    before i, csr_eid[p] = the id of the undirected edge that holds the stored entry p (-1 for a diagonal entry)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    N = len(rowptr) - 1
    wv = _w(rowptr, w)
    edge_off = np.zeros(N + 1, dtype=np.int64)
    src, dst, ew, ids = [], [], [], {}
    csr_eid = np.full(int(rowptr[-1]), -1, dtype=np.int64)
    for i in range(N):
        for p in range(rowptr[i], rowptr[i + 1]):
            j = int(col[p])
            if j < i:
                ids[(i, j)] = csr_eid[p] = len(src)
                src.append(i), dst.append(j), ew.append(wv[p])
        edge_off[i + 1] = len(src)
    for i in range(N):
        for p in range(rowptr[i], rowptr[i + 1]):
            if col[p] > i:
                csr_eid[p] = ids[(int(col[p]), i)]
    return edge_off, np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64), np.array(ew, dtype=np.float64), csr_eid


# ---------------------------------------------------------------------------------------------------------------------------------
# edge weights
# ---------------------------------------------------------------------------------------------------------------------------------
def heavy_edge(rowptr, col, w, src, dst, ew):
    """float32(ew / max(wmax_src + 1e-5, wmax_dst + 1e-5)) (:691-697), wmax = np.max(W, 0): the column maximum with the implicit
    zeros taking part, so a stored entry <= 0 never enters it and wmax >= 0."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    wv = _w(rowptr, w)
    wmax = np.zeros(len(rowptr) - 1)
    for p in range(len(col)):
        if wv[p] > 0.0 and wv[p] > wmax[col[p]]:
            wmax[col[p]] = wv[p]
    wi, wj = wmax[src] + 1e-5, wmax[dst] + 1e-5
    m = np.where(wj > wi, wj, wi)                       # Python's max([wi, wj])
    return (np.asarray(ew, dtype=np.float64) / m).astype(np.float32)


def jc(src, dst, X):
    """float32(min_k 1 / max((x_ik - x_jk)^2, 1e-6)) (:700-710): the reference's running float32 minimum is the float32 rounding of
    the float64 minimum, rounding being monotone."""
    X = np.asarray(X, dtype=np.float64)
    d = X[src] - X[dst]
    d2 = d * d
    t = 1.0 / np.where(d2 > 1e-6, d2, 1e-6)
    return t.min(axis=1).astype(np.float32) if len(src) else np.zeros(0, dtype=np.float32)


def affinity(src, dst, X, N):
    """affinity_GS (:713-727) in np.longdouble, BEFORE the float32 rounding: c_e = (x_i.x_j)^2 / ((x_i.x_i)^2 (x_j.x_j)^2), the
    per-node maximum cmax of c over the incident edges (the row maxima of the reference's dense symmetric c, 0 without an edge),
    p_e = c_e / (cmax_i cmax_j).  Returns (p, c, cmax, cond): cond_e = sum_k |x_ik x_jk| / |x_i.x_j|, the condition of the one sum of
    the expression that can cancel (x_i.x_i and x_j.x_j are sums of squares: condition 1)."""
    X = np.asarray(X, dtype=LD)
    xi, xj = X[src], X[dst]
    ij, ii, jj = (xi * xj).sum(1), (xi * xi).sum(1), (xj * xj).sum(1)
    c = (ij * ij) / ((ii * ii) * (jj * jj))
    cmax = np.zeros(N, dtype=LD)
    np.maximum.at(cmax, src, c)
    np.maximum.at(cmax, dst, c)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.abs(xi * xj).sum(1) / np.abs(ij)
    return c / (cmax[src] * cmax[dst]), c, cmax, cond


def affinity_interval(src, dst, N, p, c, cmax, cond):
    """(lo, hi) around affinity()'s p for a float64 evaluation that forms each dot product in a 16-leaf tree: a product rounds once
    and each of the 4 tree levels once, so x_i.x_j is within gamma_5 cond of its value and the two sums of squares within gamma_5;
    c_e squares each (twice the error and one rounding), multiplies and divides: relative error a_e = gamma(10 cond + 25), one more
    for the second-order terms (cond < 1e6).  A node's maximum is the maximum of the computed c: off by at most the largest a_e c_e of
    its edges, relative rm_i.  p = c / (mi * mj) rounds twice more:
        p (1 - a)(1 - u)^2 / ((1 + rm_i)(1 + rm_j))  <=  computed p  <=  p (1 + a)(1 + u)^2 / ((1 - rm_i)(1 - rm_j)).
    Rounding to float32 is monotone: the float32 proximity lies between the float32 roundings of the two ends."""
    assert np.isfinite(cond.astype(np.float64)).all() and cond.max() < 1e6
    u = LD(2) ** -53
    k = 10 * cond + 26
    a = k * u / (1 - k * u)
    dm = np.zeros(N, dtype=LD)
    np.maximum.at(dm, src, a * c)
    np.maximum.at(dm, dst, a * c)
    rm = dm / np.where(cmax > 0, cmax, 1)
    hi = p * (1 + a) * (1 + u) ** 2 / ((1 - rm[src]) * (1 - rm[dst]))
    lo = p * (1 - a) * (1 - u) ** 2 / ((1 + rm[src]) * (1 + rm[dst]))
    return lo, hi


def edge_cost(src, dst, dw, A):
    """variation_edges' cost (:495-514) |a_i - a_j|^2 / 4 * (2 dw_i + 2 dw_j) in np.longdouble.  Returns (cost, cond): cond is the
    same expression on |terms| (the squares are non-negative already; dw enters as |dw|)."""
    A, dw = np.asarray(A, dtype=LD), np.asarray(dw, dtype=LD)
    d = A[src] - A[dst]
    s = (d * d).sum(1) * LD(0.25)
    return s * (2 * dw[src] + 2 * dw[dst]), s * (2 * np.abs(dw[src]) + 2 * np.abs(dw[dst]))


# ---------------------------------------------------------------------------------------------------------------------------------
# test vectors
# ---------------------------------------------------------------------------------------------------------------------------------
def jacobi(rowptr, col, w, dw, X0, iterations=JACOBI_STEPS):
    """`iterations` steps x <- 0.5 x + 0.5 Dinv (D - L) x (:834-848) with the reference's float32 deg and float32 1 / deg (0 where
    deg == 0): (D - L) = W + diag(f32(dw) - dw).  One IEEE operation at a time, as csrc/match_arith.h states the step:
        acc = 0; for every stored entry of the row in CSR order: acc = acc + w * x_j
        x_i <- 0.5 * x_i + 0.5 * (dinv * (acc + (f64(f32(dw)) - dw) * x_i))."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    wv, dw = _w(rowptr, w), np.asarray(dw, dtype=np.float64)
    X = np.array(X0, dtype=np.float64, copy=True)
    N = len(rowptr) - 1
    if N == 0:
        return X
    deg = np.diff(rowptr)
    degf = dw.astype(np.float32)
    with np.errstate(divide="ignore"):
        dinv = np.where(degf == 0, 0.0, (1.0 / degf.astype(np.float64)).astype(np.float32).astype(np.float64))
    corr = degf.astype(np.float64) - dw
    for _ in range(iterations):
        acc = np.zeros_like(X)
        for t in range(int(deg.max(initial=0))):        # the t-th entry of every row that has one: CSR order within each row
            rows = np.nonzero(deg > t)[0]
            p = rowptr[rows] + t
            acc[rows] = acc[rows] + wv[p][:, None] * X[col[p]]
        mx = dinv[:, None] * (acc + corr[:, None] * X)
        X = 0.5 * X + 0.5 * mx
    return X


def gauss_seidel(rowptr, col, w, dw, comp_off, X0):
    """One Gauss-Seidel sweep x <- -(D + L_lower)^-1 L_upper x (:822-832) on L = diag(dw) - W, per component of node range
    comp_off[c]:comp_off[c + 1], row by row: out_i = (sum_j w_ij v_j) / dw_i with v_j = x_j for j > i and out_j for j < i, summed in
    CSR order.  Returns (out, bound): bound_i limits the distance of ANY evaluation of the same recurrence that rounds each product
    once and adds the row's terms in some order: each side is within gamma(deg_i + 1) sum |w_ij v_j| / dw_i of the exact row given its
    own earlier rows, and inherits sum_{j<i} |w_ij| bound_j / dw_i from them."""
    return _gauss_seidel(rowptr, col, w, dw, comp_off, X0, ordered=False)


def gauss_seidel_ordered(rowptr, col, w, dw, comp_off, X0):
    """The same sweep in the kernel's documented summation: the row's stored entries p = rowptr[i] + g (mod 4) go to partial sum
    g (each from 0.0, in ascending p), the row is (s0 + s1) + (s2 + s3), then one division by dw_i.  Held to bits."""
    return _gauss_seidel(rowptr, col, w, dw, comp_off, X0, ordered=True)[0]


def _gauss_seidel(rowptr, col, w, dw, comp_off, X0, ordered):
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    wv, dw = _w(rowptr, w), np.asarray(dw, dtype=np.float64)
    X0 = np.asarray(X0, dtype=np.float64)
    out, bound = np.full_like(X0, np.nan), np.zeros_like(X0)
    u = 2.0 ** -53
    for c in range(len(comp_off) - 1):
        for i in range(int(comp_off[c]), int(comp_off[c + 1])):
            s = [np.zeros(X0.shape[1]) for _ in range(4)]
            mag, inherit = np.zeros(X0.shape[1]), np.zeros(X0.shape[1])
            b, e = int(rowptr[i]), int(rowptr[i + 1])
            for p in range(b, e):
                j = int(col[p])
                if j == i:
                    continue
                v = X0[j] if j > i else out[j]
                g = (p - b) % 4 if ordered else 0
                s[g] = s[g] + wv[p] * v
                mag += np.abs(wv[p] * v)
                if j < i:
                    inherit += np.abs(wv[p]) * bound[j]
            out[i] = ((s[0] + s[1]) + (s[2] + s[3])) / dw[i]
            k = (e - b + 1) * u
            bound[i] = (2 * k / (1 - k) * mag + inherit) / abs(dw[i]) * (1 + 4 * u)
    return out, bound


# ---------------------------------------------------------------------------------------------------------------------------------
# matching
# ---------------------------------------------------------------------------------------------------------------------------------
def sort_key_order(weight):
    """The matching's rank: -weight ascending, then edge id ascending; -0 == +0, NaN last (numpy's sort order)."""
    weight = np.asarray(weight, dtype=np.float64)
    return np.lexsort((np.arange(len(weight)), -weight))


def match_keep(N, r):
    """Pairs matching_greedy (:969-987) takes before it stops: it starts at n = N, takes a pair, n -= 1, and stops once
    n <= (1 - r) * N in float64; at least one pair is taken before the test."""
    n_target = (1 - r) * N
    k = 1
    while N - k > n_target:
        k += 1
    return k


def stable_greedy(src, dst, weight, N, comp_off=None, k_keep=None, min_gain=0):
    """matching_greedy under the stable order, per component (node ranges comp_off; default one): a sequential scan of the
    component's edges in sort_key_order that takes an edge when both ends are free and stops after max(k_keep[c], 0) pairs.
    A component that took <= min_gain pairs keeps none (:131-135).  Returns (pairs [S, 2] with the larger id first, components in
    order and rank order within, comp_taken before the min_gain filter, sel_off = 2 * arange(S + 1), sel_count = [S, 2 S])."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    comp_off = np.array([0, N]) if comp_off is None else np.asarray(comp_off, dtype=np.int64)
    n_comp = len(comp_off) - 1
    k_keep = np.broadcast_to(np.asarray(N if k_keep is None else k_keep, dtype=np.int64), (n_comp,))
    order = sort_key_order(weight)
    comp_of_edge = np.searchsorted(comp_off, src[order], side="right") - 1
    marked = np.zeros(N, dtype=bool)
    pairs, comp_taken = [], np.zeros(n_comp, dtype=np.int64)
    for c in range(n_comp):
        mine = []
        for e in order[comp_of_edge == c]:
            if len(mine) >= max(int(k_keep[c]), 0):
                break
            i, j = int(src[e]), int(dst[e])
            if marked[i] or marked[j]:
                continue
            marked[i] = marked[j] = True
            mine.append((i, j))
        comp_taken[c] = len(mine)
        if len(mine) > min_gain:
            pairs += mine
    pairs = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    S = len(pairs)
    return pairs, comp_taken, 2 * np.arange(S + 1), np.array([S, 2 * S])


def dominant_rounds(rowptr, col, csr_eid, src, dst, weight, N, comp_off=None):
    """Live rounds of the locally-dominant matching (DESIGN.md "Matching methods"): in a round every unmatched node points at its
    best-ranked edge to an unmatched neighbour, and an edge both of whose ends point at it is matched.  A round is live when some
    node still points; the count is that of the live rounds (each matches at least one edge).  Returns (rounds, matched edge ids)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    comp_off = np.array([0, N]) if comp_off is None else np.asarray(comp_off, dtype=np.int64)
    order = sort_key_order(weight)
    comp = np.searchsorted(comp_off, np.asarray(src)[order], side="right") - 1
    order = order[np.argsort(comp, kind="stable")]
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    matched = np.zeros(N, dtype=bool)
    in_match, rounds = [], 0
    while True:
        ptr = np.full(N, -1, dtype=np.int64)
        for v in range(N):
            if matched[v]:
                continue
            cand = [rank[csr_eid[p]] for p in range(rowptr[v], rowptr[v + 1]) if col[p] != v and not matched[col[p]]]
            if cand:
                ptr[v] = min(cand)
        if not (ptr >= 0).any():
            return rounds, np.array(sorted(in_match), dtype=np.int64)
        rounds += 1
        for v in range(N):
            if ptr[v] >= 0:
                e = order[ptr[v]]
                if src[e] == v and ptr[dst[e]] == ptr[v]:
                    matched[v] = matched[dst[e]] = True
                    in_match.append(int(e))


# ---------------------------------------------------------------------------------------------------------------------------------
# the level loop of one small component (csrc/match_small.hip's header comment)
# ---------------------------------------------------------------------------------------------------------------------------------
def lift(rowptr, col, w, nid, cv, nc):
    """The lift Wc = sym(zero-diagonal(P^T W P)), P's column weights p_v = c_v * (1 / c_v), in fitgnn_lift_adjacency's order:
    y[u][b] = sum_v w_uv p_v over the entries of row u whose column lies in cluster b (ascending v), s[a][b] = sum_u y[u][b] p_u over
    the members u of cluster a (ascending u), Wc[a][b] = (s_ab + s_ba) / 2, exact zeros dropped.  Returns the CSR triple of Wc."""
    N = len(rowptr) - 1
    p = cv * (1.0 / cv)
    s = {}
    for u in range(N):                                   # ascending u within (a, b)
        a, y = int(nid[u]), {}
        for q in range(rowptr[u], rowptr[u + 1]):        # ascending v within (u, b)
            v, b = int(col[q]), int(nid[col[q]])
            if b == a:
                continue
            t = w[q] * p[v]
            y[b] = y[b] + t if b in y else t
        for b, yb in y.items():
            t = yb * p[u]
            s[(a, b)] = s[(a, b)] + t if (a, b) in s else t
    rp, cc, ww = [0], [], []
    for a in range(nc):
        for b in sorted(bb for (aa, bb) in s if aa == a):
            v = (s[(a, b)] + s.get((b, a), 0.0)) / 2.0
            if v != 0.0:
                cc.append(b), ww.append(v)
        rp.append(len(cc))
    return np.array(rp, dtype=np.int64), np.array(cc, dtype=np.int64), np.array(ww, dtype=np.float64)


def coarsen_levels(rowptr, col, w, r, method, K=10, draws=None, max_levels=10, max_level_r=0.99):
    """coarsen() (:60-182) of one connected component with method heavy_edge or algebraic_JC, level by level:
        r_cur = clip(1 - n_target / n, 0, max_level_r), n_target = ceil((1 - r) N)                                      (:65)
        weights: heavy_edge, or algebraic_JC from X0 = the next n * K draws (row-major) / sqrt(n) and 20 Jacobi steps, dw the row sum
        of W in column order; stable greedy matching stopped after match_keep(n, r_cur) pairs;
        a level of <= 2 pairs is not applied and ends the loop                                                     (:131-135)
        the pair (i, j), i > j, keeps row i; survivors are numbered in node order; C's value is 1 / sqrt(2) on a pair, 1 elsewhere,
        multiplied into the running value; then lift()
        stop once n <= n_target or after max_levels levels                                                              (:180)
    Returns (assign [N], cval [N], (rowptr, col, w) of Wc, applied levels, draws used)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    w = _w(rowptr, w)
    N = len(rowptr) - 1
    assign, cval = np.arange(N, dtype=np.int64), np.ones(N)
    n, levels, used = N, 0, 0
    n_target = np.ceil((1.0 - r) * N)
    for _ in range(max_levels if N > 1 else 0):
        r_cur = min(max(1.0 - n_target / n, 0.0), max_level_r)
        _, src, dst, ew, _ = edge_list(rowptr, col, w)
        if method == "heavy_edge":
            weight = heavy_edge(rowptr, col, w, src, dst, ew)
        elif method == "algebraic_JC":
            X0 = np.asarray(draws[used: used + n * K], dtype=np.float64).reshape(n, K) / np.sqrt(float(n))
            used += n * K
            dw = np.zeros(n)
            for i in range(n):
                for q in range(rowptr[i], rowptr[i + 1]):
                    dw[i] = dw[i] + w[q]
            weight = jc(src, dst, jacobi(rowptr, col, w, dw, X0, JACOBI_STEPS))
        else:
            raise ValueError(method)
        pairs, _, _, _ = stable_greedy(src, dst, weight.astype(np.float64), n, None, match_keep(n, r_cur), 0)
        if len(pairs) <= 2:
            break
        root, cv = np.arange(n), np.ones(n)
        root[pairs[:, 1]] = pairs[:, 0]
        cv[pairs.ravel()] = 1.0 / np.sqrt(2.0)
        survivor = root == np.arange(n)
        nid = (np.cumsum(survivor) - 1)[root]
        nc = n - len(pairs)
        cval = cv[assign] * cval
        assign = nid[assign]
        rowptr, col, w = lift(rowptr, col, w, nid, cv, nc)
        n = nc
        levels += 1
        if n <= n_target:
            break
    return assign, cval, (rowptr, col, w), levels, used
