"""`coarsen()` with the reference's signature and return values, contraction step on the MI355X.

Mirror of graph_coarsening/coarsening_utils.py:18-182 (`coarsen`).  variation_neighborhoods (the method
BASELINE.json's north_star names), per level:

    host   spectral prelude  A = Uk diag(lk^-1/2)            (:75-96;  ARPACK / LAPACK)
           or               A = B diag(d^-1/2) V             (:99-105)
    device candidate family + local-variation costs          (:571-578, :555-561)   fitgnn_variation_costs_f64
    device greedy disjoint selection with re-costing         (:604-650)             fitgnn_greedy_select
    device assignment vector / C values                      (:212-254, :168-179)   fitgnn_build_assignment
    device adjacency lift Wc = zero_diag(P^T W P) symmetrised (:138-139, :201-205)   fitgnn_lift_adjacency

The matching-based methods heavy_edge, algebraic_JC, affinity_GS and variation_edges (:115-127, :483-527,
:658-848, :931-993) run per level:

    host   test vectors X0 = randn(N, K)/sqrt(N) (JC, GS: the reference's draw, same place and order)
           or spectral prelude as above (variation_edges)
    device edge list tril(W) in row-major order                                           fitgnn_edge_list
    device test-vector smoothing (20 Jacobi steps / one Gauss-Seidel sweep)    fitgnn_jacobi_vectors_f64 / _gauss_seidel_
    device per-edge proximity (f32) or variation cost (f64)                           fitgnn_*_proximity / _edge_variation_
    device greedy matching, stable rank (-weight, edge id), truncated as :983-985     fitgnn_greedy_matching
    device assignment / lift as above

Returned objects expose what FIT-GNN's callers touch (utils.py:159-184, :723-752, main.py:144-151):
`C` is a scipy csc matrix (subclass whose `.dot(dense)` runs the pooling kernel), `Gc` a light graph with
`.N .W .A .dw .L`, `mapping_dict_list` the per-level dicts.  There is no CPU path for the contraction step.
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib


# ---------------------------------------------------------------------------------------------
# light graph object (what the variation path reads from pygsp.graphs.Graph)
# ---------------------------------------------------------------------------------------------
class Graph:
    def __init__(self, W, coords=None):
        W = sp.csr_matrix(W, dtype=np.float64)
        W.eliminate_zeros()
        W.sort_indices()
        self.W = W
        self.N = W.shape[0]
        self._A = self._dw = self._L = None
        if coords is not None:
            self.coords = coords
        self.info = {}

    @property
    def A(self):
        if self._A is None:
            self._A = (self.W > 0).tocsr()
        return self._A

    @property
    def dw(self):
        if self._dw is None:
            self._dw = np.ravel(self.W.sum(axis=0))
        return self._dw

    @property
    def L(self):
        if self._L is None:
            self._L = (sp.diags(self.dw, 0) - self.W).tocsc()
        return self._L

    @property
    def Ne(self):
        return sp.tril(self.W).nnz

    def is_directed(self):
        return (abs(self.W - self.W.T) > 1e-12).nnz > 0

    def subgraph(self, ind):
        return Graph(self.W[ind, :][:, ind])

    def extract_components(self):
        ncomp, lab = sp.csgraph.connected_components(self.W, directed=False)
        order = np.argsort(lab, kind="stable")
        bounds = np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=ncomp))])
        firsts = [order[bounds[k]] for k in range(ncomp)]
        out = []
        for k in np.argsort(firsts, kind="stable"):  # pygsp discovers components by lowest unvisited node
            idx = np.sort(order[bounds[k]:bounds[k + 1]])
            g = self.subgraph(idx)
            g.info = {"orig_idx": idx.tolist()}
            out.append(g)
        return out


# ---------------------------------------------------------------------------------------------
# host prelude (not part of the accelerated step; same NumPy/SciPy calls as the reference)
# ---------------------------------------------------------------------------------------------
def _spectral_level1(G, K, Uk, lk):
    import scipy.sparse.linalg as spla

    if (Uk is not None) and (lk is not None) and (len(lk) >= K):
        mask = lk < 1e-10
        lk[mask] = 1
        lsinv = lk ** (-0.5)
        lsinv[mask] = 0
        return Uk[:, :K] @ np.diag(lsinv[:K])
    offset = 2 * max(G.dw)
    T = offset * sp.eye(G.N, format="csc") - G.L
    if K >= G.N:
        lk, Uk = spla.eigsh(T.toarray(), k=K, which="LM", tol=1e-5)
    else:
        lk, Uk = spla.eigsh(T, k=K, which="LM", tol=1e-5)
    lk = (offset - lk)[::-1]
    Uk = Uk[:, ::-1]
    mask = lk < 1e-10
    lk[mask] = 1
    lsinv = lk ** (-0.5)
    lsinv[mask] = 0
    return Uk @ np.diag(lsinv)


def lanczos_smallest(L, K, device="cuda", tol=1e-5, m=None, max_restarts=300, seed=0):
    """The K smallest eigenpairs of the graph Laplacian L on the device: thick-restart Lanczos with full (two-pass)
    reorthogonalisation in float64 on T = 2 max(diag L) I - L, the shifted operator the reference hands to ARPACK
    (coarsening_utils.py:83-90), same relative tolerance.  SURVEY §8 f4: 42 % of the reference's coarsening time is this
    solve.  One Lanczos step = five launches of csrc/lanczos.hip over a column-major basis (the CSR product, three projection
    passes, the normalisation; fixed-order sums: reproducible); the projected m x m eigenproblem and the basis rotation of a
    restart are small dense library calls.  Returns (lk ascending, Uk) as NumPy arrays, the (lk, Uk) coarsen() accepts."""
    Lh = _lib.lib()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.FitgnnError("lanczos_smallest runs on the MI355X (spectral='host' is the reference's ARPACK call)")
    # L is symmetric: a CSC matrix's arrays ARE the CSR arrays of the same matrix (Graph.L is CSC) -- no conversion, no T on the host:
    # the device product computes y = offset x - L x
    Lc = L if sp.isspmatrix_csc(L) or sp.isspmatrix_csr(L) else sp.csr_matrix(L)
    N = Lc.shape[0]
    offset = 2.0 * float(Lc.diagonal().max())
    rowptr = torch.from_numpy(np.ascontiguousarray(Lc.indptr, dtype=np.int32)).to(dev)
    col = torch.from_numpy(np.ascontiguousarray(Lc.indices, dtype=np.int32)).to(dev)
    val = torch.from_numpy(np.ascontiguousarray(Lc.data, dtype=np.float64)).to(dev)
    m = int(m or min(N - 1, max(4 * K + 20, 60)))
    if m + 1 > 128:
        raise ValueError("lanczos_smallest: at most 127 basis vectors (fitgnn_lanczos_project_f64)")
    K = min(K, m - 1)
    st = _lib.stream_ptr(dev)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    V = torch.zeros(m + 1, N, dtype=torch.float64, device=dev)        # basis vector c = V[c] (contiguous)
    V2 = torch.zeros_like(V)                                           # the rotated basis of a restart
    v = torch.randn(N, generator=gen, dtype=torch.float64).to(dev)
    V[0] = v / v.norm()
    H = torch.zeros(m + 1, m, dtype=torch.float64, device=dev)
    w = torch.empty(N, dtype=torch.float64, device=dev)
    parts = int(Lh.fitgnn_lanczos_parts(N))
    part = torch.empty(parts * (m + 2), dtype=torch.float64, device=dev)
    ha, hb, hc = (torch.empty(m + 2, dtype=torch.float64, device=dev) for _ in range(3))

    def project(ncol, h_in, h_out):
        _lib.call("fitgnn_lanczos_project_f64", V, N, ncol, w, N, h_in, part, st)
        _lib.call("fitgnn_lanczos_reduce_f64", part, parts, ncol + 1, h_out, st)

    def rotate(src, Smat, dst):
        """dst[c] = sum_j Smat[j, c] src[j] (Smat: host array [m, nk]); the kernel rotates at most 16 columns per launch: groups."""
        for c0 in range(0, int(Smat.shape[1]), 16):
            blk = Smat[:, c0:c0 + 16]
            Sd = torch.from_numpy(np.ascontiguousarray(blk, dtype=np.float64)).to(dev)
            _lib.call("fitgnn_lanczos_rotate_f64", src, N, int(blk.shape[0]), Sd, int(blk.shape[1]), dst[c0:], N, N, st)

    j0 = 0
    for _ in range(max_restarts):
        for j in range(j0, m):
            _lib.call("fitgnn_lanczos_spmv_f64", rowptr, col, val, V[j], w, N, -1.0, offset, st)
            # h = V^T w;  w -= V h, h2 = V^T w;  w -= V h2, |w|^2;  v_{j+1} = w / |w|, H[:, j] = h + h2
            project(j + 1, None, ha)
            project(j + 1, ha, hb)
            project(j + 1, hb, hc)
            _lib.call("fitgnn_lanczos_finish_f64", V, N, j, w, N, ha, hb, hc, H, m, st)
        # the projected m x m eigenproblem on the host (60 x 60: LAPACK takes less than the launch of a device solver)
        Hh = H.cpu().numpy()
        Hm = (Hh[:m, :m] + Hh[:m, :m].T) / 2
        theta, S = np.linalg.eigh(Hm)
        order = np.argsort(-theta, kind="stable")
        idx = order[:K]
        resid = np.abs(Hh[m, m - 1] * S[m - 1, idx])
        if float(resid.max()) <= tol * float(np.abs(theta).max()):
            break
        keep = order[:min(K + 5, m - 2)]
        nk = int(keep.size)
        rotate(V, S[:, keep], V2)                 # V2[:nk] = the kept Ritz vectors
        V2[nk].copy_(V[m])
        Hn = np.zeros_like(Hh)
        Hn[:nk, :nk] = np.diag(theta[keep])
        Hn[nk, :nk] = Hh[m, m - 1] * S[m - 1, keep]
        V, V2 = V2, V
        H.copy_(torch.from_numpy(Hn))
        j0 = nk
    lk = offset - theta[idx]
    rotate(V, S[:, idx], V2)
    Uk = V2[:K].T.contiguous().cpu().numpy()
    o = np.argsort(lk)
    return lk[o], np.ascontiguousarray(Uk[:, o])


def _spectral_next(G, iC, B):
    B = iC.dot(B)
    d, V = np.linalg.eig(B.T @ (G.L).dot(B))
    mask = d == 0
    d[mask] = 1
    dinvsqrt = d ** (-1 / 2)
    dinvsqrt[mask] = 0
    return B, B @ np.diag(dinvsqrt) @ V


# ---------------------------------------------------------------------------------------------
# device pipeline for one level
# ---------------------------------------------------------------------------------------------
def _dev(a, dtype, device):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(device)


class LevelResult:
    __slots__ = ("N", "n", "assign", "cval", "cost0", "sel_off", "sel_mem", "rowptr", "col", "w", "device")


def contract_level(G, A, r_cur, device="cuda", keep_debug=False):
    """One contraction level on the GPU.  Returns LevelResult with device tensors assign (int32[N]),
    cval (float64[N]) and n (int)."""
    L = _lib.lib()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.FitgnnError("contract_level needs the MI355X (no CPU fallback)")
    st = _lib.stream_ptr(dev)
    N = G.N
    W = G.W
    A = np.ascontiguousarray(np.real(A), dtype=np.float64)
    K = A.shape[1]
    if not (1 <= K <= _lib.MAX_K):
        raise _lib.FitgnnError(f"K={K} outside [1,{_lib.MAX_K}]")
    rowptr = _dev(W.indptr, torch.int32, dev)
    col = _dev(W.indices, torch.int32, dev)
    w = _dev(W.data, torch.float64, dev)
    dw = _dev(G.dw, torch.float64, dev)
    Ad = _dev(A, torch.float64, dev)
    nnz = int(W.nnz)
    set_off = torch.empty(N + 1, dtype=torch.int32, device=dev)
    set_mem = torch.empty(nnz + N, dtype=torch.int32, device=dev)
    _lib.call("fitgnn_closed_neighbourhoods", rowptr, col, N, set_off, set_mem, st)
    set_len = (set_off[1:] - set_off[:-1]).contiguous()
    cost0 = torch.empty(N, dtype=torch.float64, device=dev)
    _lib.call("fitgnn_variation_costs_f64", rowptr, col, w, dw, Ad, K, K, set_off, set_len, set_mem, N, cost0, st)
    n_reduce = int(np.floor(r_cur * N))  # coarsening_utils.py:612
    total = nnz + N
    wb = int(L.fitgnn_greedy_select_workspace_bytes(N, total))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    sel_off = torch.empty(N + 1, dtype=torch.int32, device=dev)
    sel_mem = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    sel_count = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.call("fitgnn_greedy_select", rowptr, col, w, dw, Ad, K, K, N, set_off, set_mem, cost0, n_reduce, sel_off, sel_mem, sel_count, work, wb, st)
    assign = torch.empty(N, dtype=torch.int32, device=dev)
    cval = torch.empty(N, dtype=torch.float64, device=dev)
    n_out = torch.zeros(1, dtype=torch.int32, device=dev)
    wb2 = int(L.fitgnn_build_assignment_workspace_bytes(N))
    work2 = torch.empty(wb2, dtype=torch.uint8, device=dev)
    _lib.call("fitgnn_build_assignment", N, sel_off, sel_mem, sel_count, assign, cval, n_out, work2, wb2, st)
    res = LevelResult()
    res.N, res.n, res.assign, res.cval, res.device = N, int(n_out.item()), assign, cval, dev
    res.rowptr, res.col, res.w = rowptr, col, w
    res.cost0 = cost0 if keep_debug else None
    if keep_debug:
        cnt = sel_count.cpu().numpy()
        res.sel_off = sel_off[: cnt[0] + 1].cpu().numpy()
        res.sel_mem = sel_mem[: cnt[1]].cpu().numpy()
    else:
        res.sel_off = res.sel_mem = None
    return res


def lift_adjacency(res):
    """Wc (scipy csr f64) = symmetrised zero-diagonal P^T W P of a LevelResult."""
    L = _lib.lib()
    dev = res.device
    st = _lib.stream_ptr(dev)
    nnz = int(res.col.numel())
    wb = int(L.fitgnn_lift_adjacency_workspace_bytes(res.N, nnz, res.n))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    rp = torch.empty(res.n + 1, dtype=torch.int32, device=dev)
    cc = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    wc = torch.empty(max(nnz, 1), dtype=torch.float64, device=dev)
    nz = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("fitgnn_lift_adjacency", res.N, res.rowptr, res.col, res.w, res.assign, res.cval, res.n, rp, cc, wc, nz, work, wb, st)
    m = int(nz.item())
    return sp.csr_matrix((wc[:m].cpu().numpy(), cc[:m].cpu().numpy(), rp.cpu().numpy()), shape=(res.n, res.n))


# ---------------------------------------------------------------------------------------------
# matching-based methods (coarsening_utils.py:115-127, :483-527, :658-848, :931-993)
# ---------------------------------------------------------------------------------------------
MATCHING_METHODS = ("heavy_edge", "algebraic_JC", "affinity_GS", "variation_edges")
RANDOM_METHODS = ("algebraic_JC", "affinity_GS")          # draw np.random.randn test vectors at every level
SUPPORTED_METHODS = ("variation_neighborhoods",) + MATCHING_METHODS


def check_method(method, algorithm="greedy"):
    """Refuse what coarsen() does not implement (no silent fall-back to another method)."""
    if "variation_neighborhood" in method:
        return
    if method not in MATCHING_METHODS:
        raise NotImplementedError(f"coarsening method '{method}' is not supported; supported: {', '.join(SUPPORTED_METHODS)}")
    if algorithm != "greedy":
        raise NotImplementedError(f"algorithm '{algorithm}' is not supported for '{method}' (greedy matching only)")


def match_keep(N, r):
    """Matches matching_greedy (:983-985) takes before it stops: n = N - k <= (1 - r) N in float64, at least one."""
    n_target = (1 - r) * N
    k = max(1, int(np.ceil(N - n_target)))
    while k > 1 and N - (k - 1) <= n_target:
        k -= 1
    while N - k > n_target:
        k += 1
    return k


class EdgeList:
    """tril(W) in row-major order on the device (the reference's get_edge_list() numbering): src > dst per edge."""
    __slots__ = ("N", "M", "rowptr", "col", "w", "dw", "edge_off", "src", "dst", "ew", "csr_eid", "device")

    def __init__(self, G, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.FitgnnError("the matching methods run on the MI355X (no CPU fallback)")
        W = G.W
        if W.diagonal().any():
            raise ValueError("the matching methods need a graph without self-loops (the reference would match (i, i))")
        self.N, self.M, self.device = G.N, int(sp.tril(W, -1).nnz), dev
        self.rowptr, self.col = _dev(W.indptr, torch.int32, dev), _dev(W.indices, torch.int32, dev)
        self.w, self.dw = _dev(W.data, torch.float64, dev), _dev(G.dw, torch.float64, dev)
        m = max(self.M, 1)
        self.edge_off = torch.empty(self.N + 1, dtype=torch.int32, device=dev)
        self.src, self.dst = (torch.empty(m, dtype=torch.int32, device=dev) for _ in range(2))
        self.ew = torch.empty(m, dtype=torch.float64, device=dev)
        self.csr_eid = torch.empty(max(int(W.nnz), 1), dtype=torch.int32, device=dev)
        _lib.call("fitgnn_edge_list", self.rowptr, self.col, self.w, self.N, self.edge_off, self.src, self.dst, self.ew, self.M, self.csr_eid,
                  _lib.stream_ptr(dev))


def test_vectors(el, method, X0):
    """generate_test_vectors (:813-848) from the host draw X0 [N x K]: 20 Jacobi steps (algebraic_JC) or one Gauss-Seidel
    sweep (affinity_GS).  Returns a device f64 [N x K] tensor."""
    L = _lib.lib()
    dev, N = el.device, el.N
    X0 = np.ascontiguousarray(X0, dtype=np.float64)
    K = int(X0.shape[1])
    if not (1 <= K <= _lib.MAX_K):
        raise _lib.FitgnnError(f"K={K} outside [1,{_lib.MAX_K}]")
    X0d = _dev(X0, torch.float64, dev)
    X = torch.empty_like(X0d)
    st = _lib.stream_ptr(dev)
    if method == "algebraic_JC":
        wb = int(L.fitgnn_jacobi_vectors_workspace_bytes(N, K))
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        _lib.call("fitgnn_jacobi_vectors_f64", el.rowptr, el.col, el.w, el.dw, N, X0d, K, 20, X, work, wb, st)
    elif method == "affinity_GS":
        comp_off = torch.tensor([0, N], dtype=torch.int32, device=dev)
        _lib.call("fitgnn_gauss_seidel_vectors_f64", el.rowptr, el.col, el.w, el.dw, N, 1, comp_off, X0d, K, X, st)
    else:
        raise ValueError(method)
    return X


def proximity(el, method, X=None):
    """get_proximity_measure (:658-730) for heavy_edge / algebraic_JC / affinity_GS: device float32 [M].  X: the device test
    vectors of test_vectors() (JC, GS)."""
    L = _lib.lib()
    dev, st = el.device, _lib.stream_ptr(el.device)
    prox = torch.empty(max(el.M, 1), dtype=torch.float32, device=dev)
    if method == "heavy_edge":
        wb = int(L.fitgnn_heavy_edge_proximity_workspace_bytes(el.N))
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        _lib.call("fitgnn_heavy_edge_proximity", el.rowptr, el.col, el.w, el.N, el.src, el.dst, el.ew, el.M, prox, work, wb, st)
    elif method == "algebraic_JC":
        K = int(X.shape[1])
        _lib.call("fitgnn_jc_proximity", el.src, el.dst, el.M, X, K, K, prox, st)
    elif method == "affinity_GS":
        K = int(X.shape[1])
        wb = int(L.fitgnn_affinity_proximity_workspace_bytes(el.N, el.M))
        work = torch.empty(wb, dtype=torch.uint8, device=dev)
        _lib.call("fitgnn_affinity_proximity", el.N, el.src, el.dst, el.M, X, K, K, prox, work, wb, st)
    else:
        raise ValueError(method)
    return prox[: el.M]


def edge_costs(el, A):
    """variation_edges' per-edge cost (:495-514) from the level's spectral matrix A (host [N x K], or a device f64 tensor)."""
    if not torch.is_tensor(A) and np.iscomplexobj(A):
        # np.linalg.eig at later levels can return a complex basis (:98-104); the reference's Frobenius norm then sums squared
        # moduli: the cost of the real part plus the cost of the imaginary part
        return edge_costs(el, np.ascontiguousarray(A.real)) + edge_costs(el, np.ascontiguousarray(A.imag))
    Ad = A if torch.is_tensor(A) else _dev(A, torch.float64, el.device)
    K = int(Ad.shape[1])
    if not (1 <= K <= _lib.MAX_K):
        raise _lib.FitgnnError(f"K={K} outside [1,{_lib.MAX_K}]")
    cost = torch.empty(max(el.M, 1), dtype=torch.float64, device=el.device)
    _lib.call("fitgnn_edge_variation_costs_f64", el.src, el.dst, el.M, el.dw, Ad, K, K, cost, _lib.stream_ptr(el.device))
    return cost[: el.M]


class MatchLevelResult(LevelResult):
    __slots__ = ("rounds", "weight", "comp_taken")


def greedy_matching(el, weight, k_keep, comp_off=None, min_gain=0):
    """matching_greedy (:931-993) on the device under the stable order (-weight, edge id): the first k_keep[c] edges of the
    full greedy matching of every component c (node ranges comp_off, default: one component), contracted by
    fitgnn_build_assignment; components that would keep <= min_gain pairs keep none (comp_taken counts before that filter).
    weight: device tensor [M] (f32 proximities or f64).  Returns MatchLevelResult."""
    L = _lib.lib()
    dev, N, st = el.device, el.N, _lib.stream_ptr(el.device)
    comp_off = np.array([0, N]) if comp_off is None else np.asarray(comp_off)
    n_comp = len(comp_off) - 1
    k_keep = np.broadcast_to(np.asarray(k_keep, dtype=np.int64), (n_comp,))
    wd = weight.to(torch.float64).contiguous()
    co_d, k_d = _dev(comp_off, torch.int32, dev), _dev(k_keep, torch.int64, dev)   # named: they must outlive the call
    wb = int(L.fitgnn_greedy_matching_workspace_bytes(N, el.M, n_comp))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    sel_off = torch.empty(N + 1, dtype=torch.int32, device=dev)
    sel_mem = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    sel_count = torch.zeros(2, dtype=torch.int32, device=dev)
    taken = torch.zeros(max(n_comp, 1), dtype=torch.int32, device=dev)
    rounds = _lib.c_i32(0)
    _lib.call("fitgnn_greedy_matching", el.rowptr, el.col, el.csr_eid, N, el.edge_off, el.src, el.dst, el.M, wd, n_comp, co_d, k_d, int(min_gain),
              sel_off, sel_mem, sel_count, taken, _lib.ctypes.byref(rounds), work, wb, st)
    assign = torch.empty(N, dtype=torch.int32, device=dev)
    cval = torch.empty(N, dtype=torch.float64, device=dev)
    n_out = torch.zeros(1, dtype=torch.int32, device=dev)
    wb2 = int(L.fitgnn_build_assignment_workspace_bytes(N))
    work2 = torch.empty(wb2, dtype=torch.uint8, device=dev)
    _lib.call("fitgnn_build_assignment", N, sel_off, sel_mem, sel_count, assign, cval, n_out, work2, wb2, st)
    res = MatchLevelResult()
    res.N, res.n, res.assign, res.cval, res.device = N, int(n_out.item()), assign, cval, dev
    res.rowptr, res.col, res.w = el.rowptr, el.col, el.w
    res.cost0, res.rounds, res.weight = None, int(rounds.value), weight
    cnt = sel_count.cpu().numpy()
    res.sel_off = sel_off[: cnt[0] + 1].cpu().numpy()
    res.sel_mem = sel_mem[: cnt[1]].cpu().numpy()
    res.comp_taken = taken[:n_comp].cpu().numpy()
    return res


def contract_matching(G, method, r_cur, K=10, A=None, device="cuda"):
    """One level of a matching method (:106-127): weights, greedy matching truncated at r_cur, assignment.  JC / GS draw
    their test vectors from np.random here, as get_proximity_measure does.  A: the level's spectral matrix (variation_edges)."""
    el = EdgeList(G, device=device)
    if method == "variation_edges":
        weight = -edge_costs(el, A)                       # matching_greedy(G, weights=-weights) (:522-524)
    else:
        X = None
        if method in RANDOM_METHODS:
            X = test_vectors(el, method, np.random.randn(G.N, K) / np.sqrt(G.N))   # generate_test_vectors (:816)
        weight = proximity(el, method, X)
    return greedy_matching(el, weight, match_keep(G.N, r_cur))


def pool_rows(assign, cval, n, X, want_f64=False):
    """Xc = C . X on the device.  assign int32[N], cval float64[N] device tensors; X float32 [N,F] device."""
    L = _lib.lib()
    _lib.require_cuda(assign, cval, X)
    dev = X.device
    X = X.float().contiguous()
    N, F = X.shape
    Xc = torch.empty((n, F), dtype=torch.float32, device=dev)
    Xc64 = torch.empty((n, F), dtype=torch.float64, device=dev) if want_f64 else None
    wb = int(L.fitgnn_pool_rows_workspace_bytes(N, n))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    _lib.call("fitgnn_pool_rows_f32", assign, cval, N, n, X, F, F, Xc, F, Xc64, work, wb, _lib.stream_ptr(dev))
    return (Xc, Xc64) if want_f64 else Xc


class CoarseningMatrix(sp.csc_matrix):
    """scipy csc matrix C [n x N] whose product with a dense [N x F] operand runs on the MI355X.

    FIT-GNN pools features and labels with `C.dot(X)` (utils.py:161,393,738,827); this subclass keeps that
    spelling working: `.dot(ndarray | torch.Tensor)` returns the float64 ndarray scipy would return, computed
    by fitgnn_pool_rows_f32 (f64 accumulation in ascending member order: bit-identical).  `.pool(X)` is the
    device-to-device form (float32 tensor in, float32 tensor out) the build's own pipeline uses.
    """

    def _vectors(self, device):
        key = str(device)
        cache = self.__dict__.setdefault("_fitgnn_dev", {})
        if key not in cache:
            csc = sp.csc_matrix(self)
            assert np.all(np.diff(csc.indptr) == 1), "C must have exactly one non-zero per column"
            cache[key] = (torch.as_tensor(csc.indices.astype(np.int32)).to(device),
                          torch.as_tensor(csc.data.astype(np.float64)).to(device))
        return cache[key]

    def pool(self, X):
        assign, cval = self._vectors(X.device)
        return pool_rows(assign, cval, self.shape[0], X)

    def dot(self, other):
        dense = torch.is_tensor(other) or (isinstance(other, np.ndarray) and other.ndim == 2)
        if not dense or not torch.cuda.is_available():
            if not dense:
                return sp.csc_matrix.dot(self, other)
            raise _lib.FitgnnError("C.dot(dense) runs on the MI355X only (no CPU fallback)")
        Xt = other if torch.is_tensor(other) else torch.from_numpy(np.ascontiguousarray(other))
        if Xt.dtype == torch.float64 and not torch.is_tensor(other):
            # label/mask pooling passes small f64 one-hot matrices (utils.py:726-742): values are exactly
            # representable in f32, so the f32 kernel input loses nothing
            pass
        dev = torch.device("cuda")
        assign, cval = self._vectors(dev)
        _, x64 = pool_rows(assign, cval, self.shape[0], Xt.to(dev).float(), want_f64=True)
        return x64.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# the drop-in driver
# ---------------------------------------------------------------------------------------------
def coarsen(G, K=10, r=0.5, max_levels=10, method="variation_neighborhood", algorithm="greedy", Uk=None, lk=None,
            max_level_r=0.99, device="cuda", spectral="arpack"):
    """Same contract as graph_coarsening.coarsening_utils.coarsen (coarsening_utils.py:18-182) for
    method in {'variation_neighborhood', 'variation_neighborhoods', 'heavy_edge', 'algebraic_JC', 'affinity_GS',
    'variation_edges'} (the matching methods with algorithm='greedy'): returns (C, Gc, mapping_dict_list).
    The matching methods break ties by edge index; algebraic_JC / affinity_GS draw from np.random exactly
    where the reference does, so a caller who seeds numpy gets the reference's test vectors."""
    return _coarsen(G, K, r, max_levels, method, algorithm, Uk, lk, max_level_r, device, spectral)[:3]


def _coarsen(G, K, r, max_levels, method, algorithm, Uk, lk, max_level_r, device, spectral):
    """coarsen()'s body: (C, Gc, mapping_dict_list, applied levels)."""
    check_method(method, algorithm)
    matching = method in MATCHING_METHODS
    if not hasattr(G, "W"):
        raise TypeError("G must expose .W (scipy sparse adjacency) and .N")
    if not isinstance(G, Graph):
        G = Graph(G.W, coords=getattr(G, "coords", None))
    r = np.clip(r, 0, 0.999)
    N = G.N
    n, n_target = N, np.ceil((1 - r) * N)
    dev = torch.device(device)
    assign_tot = torch.arange(N, dtype=torch.int32, device=dev)
    cval_tot = torch.ones(N, dtype=torch.float64, device=dev)
    Gc = G
    mapping_dict_list = []
    B = iC = None
    applied = 0
    for level in range(1, max_levels + 1):
        G = Gc
        r_cur = np.clip(1 - n_target / n, 0.0, max_level_r)
        A = None
        if "variation" in method:
            if level == 1:
                if spectral == "device" and Uk is None and G.N > 4 * K:  # extension: the eigensolve on the MI355X
                    lk, Uk = lanczos_smallest(G.L, K, device=dev)
                B = _spectral_level1(G, K, Uk, lk)
                A = B
            else:
                B, A = _spectral_next(G, iC, B)
        if matching:
            res = contract_matching(G, method, r_cur, K=K, A=A, device=dev)
        else:
            res = contract_level(G, A, r_cur, device=dev)
        assign_h = res.assign.cpu().numpy()
        iC = sp.csc_matrix((res.cval.cpu().numpy(), (assign_h, np.arange(G.N))), shape=(res.n, G.N))
        if iC.shape[1] - iC.shape[0] <= 2:  # :131-135 avoid too many levels for so few nodes
            mapping_dict_list.append({i: i for i in range(G.N)})
            break
        _lib.call("fitgnn_compose_levels", N, res.assign, res.cval, assign_tot, cval_tot, _lib.stream_ptr(dev))
        Wc = lift_adjacency(res)
        coords = None
        if hasattr(G, "coords"):
            coords = (iC.power(2)).dot(G.coords)  # coarsen_vector :190-191 (plot coordinates only)
        Gc = Graph(Wc, coords=coords)
        n = Gc.N
        applied += 1
        if matching:
            md = {i: i for i in range(N)}  # :168: the matching methods keep the identity dict at every level
        else:
            # level mapping :168-179: keys 0..N-1 of the ORIGINAL graph, identity-padded past the level's size
            md = {i: int(assign_h[i]) for i in range(G.N)}
            for i in range(G.N, N):
                md[i] = res.n + (i - G.N)
        mapping_dict_list.append(md)
        if n <= n_target:
            break
    a = assign_tot.cpu().numpy()
    C = CoarseningMatrix(sp.csc_matrix((cval_tot.cpu().numpy(), (a, np.arange(N))), shape=(int(a.max()) + 1 if N else 0, N)))
    return C, Gc, mapping_dict_list, applied


# ---------------------------------------------------------------------------------------------
# many graphs at once: the reference's per-component / per-dataset-graph Python loop as one batch
# ---------------------------------------------------------------------------------------------
class BatchCoarsening:
    """Result of coarsen_batch: `assign` int64[N] (global cluster id of every node; a component's clusters are a
    contiguous id range in ascending order of their minimum member, i.e. per-component id = assign - cluster_off[c]),
    `cval` float64[N] (the non-zero of C in that node's column), `comp_off` / `cluster_off` int64[n_comp+1],
    `Wc` scipy csr (block-diagonal coarse adjacency, global cluster ids), `levels` per-component level count, `fallback`
    int64 ids of the components coarsen_in_order handed to coarsen() (over the whole-component kernel's LDS budget; empty
    for coarsen_batch)."""
    __slots__ = ("assign", "cval", "comp_off", "cluster_off", "Wc", "levels", "n_clusters", "fallback", "_dev")

    def C(self):
        N = len(self.assign)
        return CoarseningMatrix(sp.csc_matrix((self.cval, (self.assign, np.arange(N))), shape=(self.n_clusters, N)))

    def pool(self, X):
        """C . X for every component at once (device tensor in / out)."""
        a, c = self._dev
        return pool_rows(a.to(X.device), c.to(X.device), self.n_clusters, X)


def _dense_prelude(W, b, e, K):
    """Level-1 spectral input of one small component from a dense symmetric eigendecomposition (all eigenpairs,
    smallest K kept) -- same formula as coarsening_utils.py:89-96, exact eigenvectors instead of ARPACK's tol=1e-5."""
    Wd = W[b:e, b:e].toarray()
    Ld = np.diag(Wd.sum(0)) - Wd
    lk, Uk = np.linalg.eigh(Ld)
    k = min(K, e - b)
    lk, Uk = lk[:k].copy(), Uk[:, :k]
    mask = lk < 1e-10
    lk[mask] = 1
    lsinv = lk ** (-0.5)
    lsinv[mask] = 0
    return Uk @ np.diag(lsinv)


def _dense_prelude_batch(W, off, comps, K, A, Kc):
    """_dense_prelude for many components at once: components of equal size are stacked into one [G, n, n] array and
    handed to a single batched np.linalg.eigh (the same LAPACK routine per matrix as the one-at-a-time form).  Fills
    A[rows of c, :k] and Kc[c] in place."""
    coo = W.tocoo()
    comp_of = np.searchsorted(off, coo.row, side="right") - 1
    size = np.diff(off)
    todo = np.zeros(len(size), dtype=bool)
    todo[comps] = True
    for n in np.unique(size[comps]):
        ids = np.nonzero(todo & (size == n))[0]
        slot = np.full(len(size), -1, dtype=np.int64)
        slot[ids] = np.arange(len(ids))
        sel = slot[comp_of] >= 0
        g, r, c = slot[comp_of[sel]], coo.row[sel] - off[comp_of[sel]], coo.col[sel] - off[comp_of[sel]]
        Wd = np.zeros((len(ids), n, n))
        np.add.at(Wd, (g, r, c), coo.data[sel])
        Ld = -Wd
        Ld[:, np.arange(n), np.arange(n)] += Wd.sum(1)
        lk, Uk = np.linalg.eigh(Ld)
        k = int(min(K, n))
        lk, Uk = lk[:, :k].copy(), Uk[:, :, :k]
        mask = lk < 1e-10
        lk[mask] = 1
        lsinv = lk ** (-0.5)
        lsinv[mask] = 0
        Ag = Uk * lsinv[:, None, :]
        rows = (off[ids][:, None] + np.arange(n)[None, :]).ravel()
        A[rows, :k] = Ag.reshape(-1, k)
        Kc[ids] = k


def coarsen_batch(W, comp_off, r=0.5, K=10, max_levels=10, A0=None, max_level_r=0.99, device="cuda", spectral="arpack",
                  method="variation_neighborhoods"):
    """coarsen() (coarsening_utils.py:18-182, method variation_neighborhoods) applied independently to every connected
    component of the block-diagonal adjacency W (scipy sparse [N x N]); component c = node range
    comp_off[c]:comp_off[c+1] and must be connected.  Per level ONE launch each of the family, cost, selection (one
    wavefront per component), assignment and lift kernels covers all components; a component leaves the loop exactly
    when the reference's driver would (target reached :180, or a level that removes <= 2 nodes :131-135, which is not
    applied).  The spectral prelude stays on the host per component (level 1: ARPACK as the reference, or
    spectral='dense'; later levels: the K x K eigenproblem of :98-104).  A0: optional list of per-component level-1
    matrices A (n_c x K_c), e.g. from injected (Uk, lk).  method: also the deterministic matching methods heavy_edge and
    variation_edges (one edge list, one proximity / cost launch and one matching over all components per level; the
    matching is component-agnostic and truncated per component).  Returns BatchCoarsening."""
    check_method(method)
    if method in RANDOM_METHODS:
        raise NotImplementedError(f"coarsen_batch: '{method}' draws random test vectors per component and level; use coarsen() "
                                  "per component (the reference's draw order)")
    matching = method in MATCHING_METHODS
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.FitgnnError("coarsen_batch needs the MI355X (no CPU fallback)")
    st = _lib.stream_ptr(dev)
    W = sp.csr_matrix(W).astype(np.float64)
    W.sort_indices()
    comp_off = np.asarray(comp_off, dtype=np.int64)
    n_comp, N0 = len(comp_off) - 1, int(comp_off[-1])
    assert W.shape == (N0, N0)
    r = float(np.clip(r, 0, 0.999))
    size0 = np.diff(comp_off)
    n_cur = size0.copy()
    n_target = np.ceil((1 - r) * size0)
    active = size0 > 1
    levels = np.zeros(n_comp, dtype=np.int64)
    assign_tot = torch.arange(N0, dtype=torch.int32, device=dev)
    cval_tot = torch.ones(N0, dtype=torch.float64, device=dev)
    B = None            # pooled spectral basis [N_level x Kmax], rows of inactive components are not used
    node_K = None
    iC = None
    off = comp_off.copy()
    G = Graph(W)
    for level in range(1, max_levels + 1):
        if not active.any():
            break
        N = G.N
        r_cur = np.clip(1 - n_target / np.maximum(n_cur, 1), 0.0, max_level_r)
        n_reduce = np.where(active, np.floor(r_cur * n_cur), 0).astype(np.int64)  # :612 per component
        if method == "heavy_edge":
            pass                               # no spectral prelude
        elif level == 1:
            Kc = np.where(size0 <= K, size0, K).astype(np.int32)  # eigsh(dense, k=K >= N) returns N pairs (:85-86)
            Kmax = int(max(K, Kc.max()))
            A = np.zeros((N, Kmax))
            todo = [c for c in np.nonzero(active)[0] if A0 is None or A0[c] is None]
            if spectral == "dense" and todo:
                _dense_prelude_batch(W, off, np.asarray(todo), K, A, Kc)
                todo = []
            for c in np.nonzero(active)[0]:
                b, e = int(off[c]), int(off[c + 1])
                if A0 is not None and A0[c] is not None:
                    Ac = np.asarray(A0[c], dtype=np.float64)
                elif c in todo:
                    Ac = _spectral_level1(Graph(W[b:e, b:e]), K, None, None)
                else:
                    continue
                Kc[c] = Ac.shape[1]
                A[b:e, :Ac.shape[1]] = np.real(Ac)
            node_K_comp = Kc
            B = A
        else:
            B = iC.dot(B)                      # :97, all components at once (rows are independent)
            LB = G.L.dot(B)
            A = np.zeros(B.shape, dtype=complex if method == "variation_edges" else B.dtype)  # edge costs take |.|^2 of a complex A
            for c in np.nonzero(active)[0]:    # :98-104, K x K per component
                b, e, k = int(off[c]), int(off[c + 1]), int(node_K_comp[c])
                Bc = B[b:e, :k]
                d, V = np.linalg.eig(Bc.T @ LB[b:e, :k])
                mask = d == 0
                d[mask] = 1
                dinvsqrt = d ** (-1 / 2)
                dinvsqrt[mask] = 0
                Ac = Bc @ np.diag(dinvsqrt) @ V
                A[b:e, :k] = Ac if np.iscomplexobj(A) else np.real(Ac)
        if matching:
            # ---- device: edge list, proximity / cost, one matching over all components, assignment ----
            el = EdgeList(G, device=dev)
            weight = -edge_costs(el, A) if method == "variation_edges" else proximity(el, method)
            k_keep = [match_keep(int(n_cur[c]), r_cur[c]) if active[c] else 0 for c in range(n_comp)]
            mres = greedy_matching(el, weight, k_keep, comp_off=off, min_gain=2)
            assign, cval, n_out_h = mres.assign, mres.cval, mres.n
            gain = mres.comp_taken.astype(np.int64)
            rowptr, col, w = el.rowptr, el.col, el.w
        else:
            assign, cval, gain, n_out_h, rowptr, col, w = _select_level_batch(G, A, node_K_comp, off, n_comp, n_reduce, dev, st)
        applied = active & (gain > 2)          # :131-135: a level removing <= 2 nodes is not applied and ends the loop
        levels[applied] += 1
        active = applied.copy()
        if not applied.any():
            break
        _lib.call("fitgnn_compose_levels", N0, assign, cval, assign_tot, cval_tot, st)
        res = LevelResult()
        res.N, res.n, res.assign, res.cval, res.device = N, n_out_h, assign, cval, dev
        res.rowptr, res.col, res.w = rowptr, col, w
        Wc = lift_adjacency(res)
        assign_h = assign.cpu().numpy()
        iC = sp.csc_matrix((cval.cpu().numpy(), (assign_h, np.arange(N))), shape=(res.n, N))
        n_cur = np.where(applied, n_cur - gain, n_cur)
        new_off = np.zeros(n_comp + 1, dtype=np.int64)
        np.cumsum(n_cur, out=new_off[1:])
        assert int(new_off[-1]) == res.n, (level, int(new_off[-1]), res.n, gain.tolist(), n_reduce.tolist())
        off = new_off
        G = Graph(Wc)
        active &= n_cur > n_target             # :180
    out = BatchCoarsening()
    out.assign = assign_tot.cpu().numpy().astype(np.int64)
    out.cval = cval_tot.cpu().numpy()
    out.comp_off, out.cluster_off, out.Wc, out.levels = comp_off, off, G.W, levels
    out.n_clusters = int(off[-1])
    out.fallback = np.zeros(0, dtype=np.int64)
    out._dev = (assign_tot, cval_tot)
    return out


class DrawPool:
    """Gaussians of the global np.random stream drawn ahead in chunks, handed out in order, and given back: sync() leaves the
    global state exactly where it would be had only the consumed draws been taken.  Exact because the legacy RandomState
    keeps its cached second Gaussian across calls: randn(a) followed by randn(b) draws what randn(a + b) draws and ends in
    the same state."""

    ADVANCE = 1 << 20   # draws per randn call while advancing the state (bounds the host memory of a long chain)

    def __init__(self, chunk=1 << 22):
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        self.chunk = int(chunk)
        self.rebase()

    def rebase(self):
        """Start from the current global state (nothing drawn ahead, nothing consumed)."""
        self._base = np.random.get_state()
        self._buf = np.empty(0)
        self._used = 0
        self.consumed = 0

    def ensure(self, need):
        """The unconsumed draws, at least `need` of them (drawing chunks ahead as needed)."""
        rest = self._buf[self._used:]
        if rest.size < need:
            rest = np.concatenate([rest, np.random.randn(max(self.chunk, int(need) - rest.size))])
            self._buf, self._used = rest, 0
        return rest

    def consume(self, k):
        k = int(k)
        if k < 0 or self._used + k > self._buf.size:
            raise ValueError(f"consume({k}): only {self._buf.size - self._used} draws are available")
        self._used += k
        self.consumed += k

    def sync(self):
        """Put the global state at base + consumed and rebase there."""
        np.random.set_state(self._base)
        left = self.consumed
        while left > 0:
            step = min(left, self.ADVANCE)
            np.random.randn(step)
            left -= step
        self.rebase()


IN_ORDER_METHODS = ("heavy_edge", "algebraic_JC")


def _small_fits(n, nnz, method, K):
    """Components the whole-component kernel takes (fitgnn_match_small's LDS budget)."""
    ok = (n <= _lib.MATCH_SMALL_MAX_NODES) & (nnz <= _lib.MATCH_SMALL_MAX_NNZ)
    if method == "algebraic_JC" and not (1 <= K <= _lib.MATCH_SMALL_MAX_K):
        ok[:] = False
    return ok


def coarsen_in_order(W, comp_off, r=0.5, K=10, max_levels=10, method="algebraic_JC", max_level_r=0.99, device="cuda",
                     chunk=1 << 22):
    """coarsen() (method heavy_edge or algebraic_JC) on every component comp_off[c]:comp_off[c+1] of the block-diagonal
    symmetric adjacency W, one after another in component order -- the reference's per-component loop (utils.py:163-182,
    :398-411), including its np.random draw order: per component, assign / cval / Wc / levels and the global np.random state
    afterwards are bit-identical to calling coarsen() on each component of more than one node in turn.

    Components within the LDS budget (FITGNN_MATCH_SMALL_MAX_NODES nodes, _MAX_NNZ stored entries) are coarsened whole on
    the device by fitgnn_match_small: algebraic_JC as one chain that reads the draws from a host pool of `chunk` Gaussians
    (DrawPool), heavy_edge as one workgroup per component.  A component over the budget runs coarsen() at its place in the
    order, with the global state at exactly that position.  Returns a BatchCoarsening (levels: applied levels)."""
    if method not in IN_ORDER_METHODS:
        raise NotImplementedError(f"coarsen_in_order: method '{method}' is not supported; supported: {', '.join(IN_ORDER_METHODS)}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.FitgnnError("coarsen_in_order needs the MI355X (no CPU fallback)")
    st = _lib.stream_ptr(dev)
    W = sp.csr_matrix(W).astype(np.float64)
    W.sum_duplicates()
    W.eliminate_zeros()
    W.sort_indices()
    comp_off = np.asarray(comp_off, dtype=np.int64)
    n_comp, N0 = len(comp_off) - 1, int(comp_off[-1])
    if W.shape != (N0, N0):
        raise ValueError(f"W is {W.shape}, comp_off spans {N0} nodes")
    if W.diagonal().any():
        raise ValueError("the matching methods need a graph without self-loops (the reference would match (i, i))")
    if (W != W.T).nnz:
        raise ValueError("coarsen_in_order needs an exactly symmetric W")
    coo = W.tocoo()
    comp_of = np.repeat(np.arange(n_comp), np.diff(comp_off))
    if N0 and (comp_of[coo.row] != comp_of[coo.col]).any():
        raise ValueError("W couples two components: it must be block-diagonal over comp_off")
    r = float(np.clip(r, 0, 0.999))
    size = np.diff(comp_off)
    nnz = W.indptr[comp_off[1:]] - W.indptr[comp_off[:-1]]
    mcode = _lib.MATCH_ALGEBRAIC_JC if method == "algebraic_JC" else _lib.MATCH_HEAVY_EDGE
    fits = _small_fits(size, nnz, method, K)
    # device outputs at the input's node / entry slots (fitgnn_match_small's layout)
    rowptr, col, w = _dev(W.indptr, torch.int32, dev), _dev(W.indices, torch.int32, dev), _dev(W.data, torch.float64, dev)
    co_d = _dev(comp_off, torch.int32, dev)
    assign = torch.empty(max(N0, 1), dtype=torch.int32, device=dev)
    cval = torch.empty(max(N0, 1), dtype=torch.float64, device=dev)
    n_out = torch.zeros(max(n_comp, 1), dtype=torch.int32, device=dev)
    levels = torch.zeros(max(n_comp, 1), dtype=torch.int32, device=dev)
    status = torch.zeros(max(n_comp, 1), dtype=torch.int32, device=dev)
    wc_rowptr = torch.zeros(N0 + n_comp + 1, dtype=torch.int32, device=dev)
    wc_col = torch.empty(max(int(W.nnz), 1), dtype=torch.int32, device=dev)
    wc_w = torch.empty(max(int(W.nnz), 1), dtype=torch.float64, device=dev)
    cap_n = int(max(size[fits].max(initial=1), 1))
    cap_z = int(nnz[fits].max(initial=0))
    fallback = {}                                           # component -> (C, Gc, applied levels) from coarsen()

    def run_coarsen(c):
        b, e = int(comp_off[c]), int(comp_off[c + 1])
        C, Gc, _, lv = _coarsen(Graph(W[b:e, b:e]), K, r, max_levels, method, "greedy", None, None, max_level_r, dev, "arpack")
        fallback[c] = (sp.csc_matrix(C), Gc.W, lv)

    def launch(c0, c1, draws=None, sqrt_n=None, progress=None):
        nd = 0 if draws is None else int(draws.numel())
        _lib.call("fitgnn_match_small", mcode, rowptr, col, w, co_d, int(c0), int(c1), r, int(K), int(max_levels), float(max_level_r), draws, nd,
                  sqrt_n, cap_n, cap_z, assign, cval, n_out, levels, status, wc_rowptr, wc_col, wc_w, progress, st)

    if method == "heavy_edge":
        if fits.any():
            launch(0, n_comp)
        for c in np.nonzero(~fits & (size > 1))[0]:
            run_coarsen(int(c))
    else:
        pool = DrawPool(chunk)
        sqrt_n = _dev(np.sqrt(np.arange(_lib.MATCH_SMALL_MAX_NODES + 1)), torch.float64, dev)
        progress = torch.zeros(2, dtype=torch.int64, device=dev)
        c = 0
        while c < n_comp:
            if size[c] <= 1:                                # the reference coarsens components of more than one node
                c += 1
                continue
            if not fits[c]:                                 # coarsen() at its place in the draw order
                pool.sync()
                run_coarsen(c)
                pool.rebase()
                c += 1
                continue
            c1 = c
            while c1 < n_comp and fits[c1]:
                c1 += 1
            draws = _dev(pool.ensure(K * int(size[c]) * max_levels), torch.float64, dev)
            launch(c, c1, draws, sqrt_n, progress)
            done, used = (int(v) for v in progress.cpu().numpy())
            if done <= c and used == 0:
                raise _lib.FitgnnError(f"match_small made no progress at component {c} (status {int(status[c].item())})")
            pool.consume(used)
            c = done
        pool.sync()
    st_h = status[:n_comp].cpu().numpy()
    bad = np.nonzero(st_h == _lib.MATCH_BAD_INPUT)[0]
    if bad.size:
        raise ValueError(f"coarsen_in_order: component {int(bad[0])} is malformed (unsorted, out-of-component or diagonal entries)")
    todo = fits & (size > 1) & (st_h != _lib.MATCH_DONE)
    if todo.any():
        raise _lib.FitgnnError(f"match_small left {int(todo.sum())} components undone (first: {int(np.nonzero(todo)[0][0])})")

    # ---- assemble the block-diagonal result: device components from their slots, coarsen() ones from C / Gc ----
    n_c = np.where(size > 1, n_out[:n_comp].cpu().numpy(), size).astype(np.int64)
    lv = np.where(size > 1, levels[:n_comp].cpu().numpy(), 0).astype(np.int64)
    a_loc = assign[:N0].cpu().numpy().astype(np.int64)
    cv = cval[:N0].cpu().numpy()
    rp_h, col_h, w_h = wc_rowptr.cpu().numpy().astype(np.int64), wc_col.cpu().numpy(), wc_w.cpu().numpy()
    p_in = W.indptr[comp_off[:-1]].astype(np.int64)
    single = size <= 1                                      # one node, no level: identity, no entries
    a_loc[np.repeat(single, size)] = 0
    cv[np.repeat(single, size)] = 1.0
    rp_h[(comp_off[:-1] + np.arange(n_comp))[single]] = 0
    rp_h[(comp_off[:-1] + np.arange(n_comp) + size)[single]] = 0
    for c, (C, Wc, lvc) in fallback.items():
        b, e = int(comp_off[c]), int(comp_off[c + 1])
        a_loc[b:e], cv[b:e] = C.indices, C.data
        n_c[c], lv[c] = C.shape[0], lvc
        Wc = sp.csr_matrix(Wc)
        rp_h[b + c: b + c + Wc.shape[0] + 1] = Wc.indptr
        col_h[p_in[c]: p_in[c] + Wc.nnz], w_h[p_in[c]: p_in[c] + Wc.nnz] = Wc.indices, Wc.data
    cluster_off = np.zeros(n_comp + 1, dtype=np.int64)
    np.cumsum(n_c, out=cluster_off[1:])
    rows_base = comp_off[:-1] + np.arange(n_comp)          # component c's local rowptr starts here
    row_comp = np.repeat(np.arange(n_comp), n_c)
    row_local = np.arange(int(cluster_off[-1])) - cluster_off[row_comp]
    r0 = rp_h[rows_base[row_comp] + row_local]
    r1 = rp_h[rows_base[row_comp] + row_local + 1]
    lens = r1 - r0
    indptr = np.zeros(int(cluster_off[-1]) + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    ent_row = np.repeat(np.arange(int(cluster_off[-1])), lens)
    src = p_in[row_comp[ent_row]] + r0[ent_row] + (np.arange(int(indptr[-1])) - indptr[ent_row])
    n_cl = int(cluster_off[-1])
    Wc_all = sp.csr_matrix((w_h[src], col_h[src].astype(np.int64) + cluster_off[row_comp[ent_row]], indptr), shape=(n_cl, n_cl))
    out = BatchCoarsening()
    out.assign = a_loc + np.repeat(cluster_off[:-1], size)
    out.cval = cv
    out.comp_off, out.cluster_off, out.Wc, out.levels = comp_off, cluster_off, Wc_all, lv
    out.n_clusters = n_cl
    out.fallback = np.array(sorted(fallback), dtype=np.int64)
    out._dev = (torch.as_tensor(out.assign.astype(np.int32)).to(dev), torch.as_tensor(out.cval).to(dev))
    return out


def _select_level_batch(G, A, node_K_comp, off, n_comp, n_reduce, dev, st):
    """coarsen_batch's variation_neighborhoods level on the device: family, costs, per-component selection, assignment.
    Returns (assign, cval, gain, n_out, rowptr, col, w)."""
    L = _lib.lib()
    N = G.N
    node_K = np.repeat(node_K_comp, np.diff(off)).astype(np.int32)
    # ---- device: family, costs, per-component selection, assignment ----
    Wl = G.W
    rowptr, col = _dev(Wl.indptr, torch.int32, dev), _dev(Wl.indices, torch.int32, dev)
    w, dw = _dev(Wl.data, torch.float64, dev), _dev(G.dw, torch.float64, dev)
    Ad, nK = _dev(A, torch.float64, dev), _dev(node_K, torch.int32, dev)
    lda = int(A.shape[1])
    nnz = int(Wl.nnz)
    set_off = torch.empty(N + 1, dtype=torch.int32, device=dev)
    set_mem = torch.empty(nnz + N, dtype=torch.int32, device=dev)
    _lib.call("fitgnn_closed_neighbourhoods", rowptr, col, N, set_off, set_mem, st)
    set_len = (set_off[1:] - set_off[:-1]).contiguous()
    cost0 = torch.empty(N, dtype=torch.float64, device=dev)
    _lib.call("fitgnn_variation_costs_batch_f64", rowptr, col, w, dw, Ad, lda, lda, nK, set_off, set_len, set_mem, N, cost0, st)
    wb = int(L.fitgnn_greedy_select_batch_workspace_bytes(N, nnz + N, n_comp))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    sel_off = torch.empty(N + 1, dtype=torch.int32, device=dev)
    sel_mem = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    sel_count = torch.zeros(2, dtype=torch.int32, device=dev)
    gain_d = torch.zeros(n_comp, dtype=torch.int64, device=dev)
    off_d, n_reduce_d = _dev(off, torch.int32, dev), _dev(n_reduce, torch.int64, dev)  # named: they must outlive the call
    _lib.call("fitgnn_greedy_select_batch", rowptr, col, w, dw, Ad, lda, lda, N, set_off, set_mem, cost0, n_comp, off_d, n_reduce_d, 2, nK, sel_off,
              sel_mem, sel_count, gain_d, work, wb, st)
    assign = torch.empty(N, dtype=torch.int32, device=dev)
    cval = torch.empty(N, dtype=torch.float64, device=dev)
    n_out = torch.zeros(1, dtype=torch.int32, device=dev)
    wb2 = int(L.fitgnn_build_assignment_workspace_bytes(N))
    work2 = torch.empty(wb2, dtype=torch.uint8, device=dev)
    _lib.call("fitgnn_build_assignment", N, sel_off, sel_mem, sel_count, assign, cval, n_out, work2, wb2, st)
    return assign, cval, gain_d.cpu().numpy(), int(n_out.item()), rowptr, col, w


# ---------------------------------------------------------------------------------------------
# coarsening quality (coarsening_utils.py:257-351): k x k results only, no dense N x N or |E| x N object
# ---------------------------------------------------------------------------------------------
QUALITY_DEVICE_MAX_KMAX = 55          # spectral='device': kmax + 5 pairs, 2 (kmax + 5) + 7 <= 127 Lanczos basis vectors


def _col_tiles(k):
    w = _lib.QUALITY_MAX_K
    return [(c, min(k, c + w)) for c in range(0, k, w)]


def _off(t, row0, col0):
    """Device pointer of t[row0, col0] (a contiguous 2-D f64 tensor)."""
    return _lib.ctypes.c_void_p(t.data_ptr() + (row0 * t.shape[1] + col0) * t.element_size())


def coarse_laplacian(W, dw, assign, cval, n):
    """Lc = C L C^T (scipy csr, diagonal stored) on the device.  W: scipy csr (no self-loops); assign / cval: device tensors."""
    L = _lib.lib()
    dev = assign.device
    N, nnz = int(W.shape[0]), int(W.nnz)
    rowptr, col = _dev(W.indptr, torch.int32, dev), _dev(W.indices, torch.int32, dev)
    w, dwd = _dev(W.data, torch.float64, dev), _dev(dw, torch.float64, dev)
    wb = int(L.fitgnn_coarse_laplacian_workspace_bytes(N, nnz, n))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    rp = torch.empty(n + 1, dtype=torch.int32, device=dev)
    cc = torch.empty(max(nnz + n, 1), dtype=torch.int32, device=dev)
    vv = torch.empty(max(nnz + n, 1), dtype=torch.float64, device=dev)
    nz = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("fitgnn_coarse_laplacian", N, rowptr, col, w, nnz, dwd, assign, cval, n, rp, cc, vv, nz, work, wb, _lib.stream_ptr(dev))
    m = int(nz.item())
    return sp.csr_matrix((vv[:m].cpu().numpy(), cc[:m].cpu().numpy(), rp.cpu().numpy()), shape=(n, n))


def project_lift(assign, cval, n, U, want_Y=True):
    """(C U [n x k], Y = C^T C U [N x k]) on the device; U: device f64 [N x k].  Columns in tiles of QUALITY_MAX_K."""
    L = _lib.lib()
    dev = U.device
    U = U.contiguous()
    N, k = int(U.shape[0]), int(U.shape[1])
    CU = torch.empty((n, k), dtype=torch.float64, device=dev)
    Y = torch.empty((N, k), dtype=torch.float64, device=dev) if want_Y else None
    wb = int(L.fitgnn_project_lift_workspace_bytes(N, n))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    for c0, c1 in _col_tiles(k):
        _lib.call("fitgnn_project_lift_f64", assign, cval, N, n, _off(U, 0, c0), k, c1 - c0, _off(CU, 0, c0), k, _off(Y, 0, c0) if want_Y else None,
                  k, work, wb, _lib.stream_ptr(dev))
    return CU, Y


def laplacian_gram(W, dw, Y):
    """G = Y^T L Y (device f64 [k x k]) with L = diag(dw) - W; one CSR pass per (column tile, column tile) pair."""
    L = _lib.lib()
    dev = Y.device
    Y = Y.contiguous()
    N, k = int(Y.shape[0]), int(Y.shape[1])
    rowptr = _dev(W.indptr, torch.int32, dev)
    # an edgeless graph still hands the kernel non-NULL entry arrays (never read)
    col = _dev(W.indices if W.nnz else np.zeros(1), torch.int32, dev)
    w, dwd = _dev(W.data if W.nnz else np.zeros(1), torch.float64, dev), _dev(dw, torch.float64, dev)
    G = torch.empty((k, k), dtype=torch.float64, device=dev)
    for p0, p1 in _col_tiles(k):
        for q0, q1 in _col_tiles(k):
            wb = int(L.fitgnn_laplacian_gram_workspace_bytes(N, p1 - p0, q1 - q0))
            work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
            _lib.call("fitgnn_laplacian_gram_f64", rowptr, col, w, dwd, N, _off(Y, 0, p0), k, p1 - p0, _off(Y, 0, q0), k, q1 - q0, _off(G, p0, q0), k,
                      work, wb, _lib.stream_ptr(dev))
    return G


def cross_atb(A, B):
    """A^T B (device f64 [k1 x k2]) for device f64 A [n x k1], B [n x k2]."""
    L = _lib.lib()
    dev = A.device
    A, B = A.contiguous(), B.contiguous()
    n, k1, k2 = int(A.shape[0]), int(A.shape[1]), int(B.shape[1])
    assert int(B.shape[0]) == n
    out = torch.empty((k1, k2), dtype=torch.float64, device=dev)
    for p0, p1 in _col_tiles(k1):
        for q0, q1 in _col_tiles(k2):
            wb = int(L.fitgnn_cross_atb_workspace_bytes(n, p1 - p0, q1 - q0))
            work = torch.empty(max(wb, 1), dtype=torch.uint8, device=dev)
            _lib.call("fitgnn_cross_atb_f64", _off(A, 0, p0), k1, p1 - p0, _off(B, 0, q0), k2, q1 - q0, n, _off(out, p0, q0), k2, work, wb,
                      _lib.stream_ptr(dev))
    return out


def _quality_inputs(G, C):
    """Host checks of coarsening_quality's inputs (before any device work).  Returns (W csr, dw, assign, cval, n)."""
    if not hasattr(G, "W"):
        raise TypeError("G must expose .W (scipy sparse adjacency) and .N")
    W = sp.csr_matrix(G.W, dtype=np.float64)
    W.eliminate_zeros()
    W.sort_indices()
    N = W.shape[0]
    if W.shape != (N, N):
        raise ValueError(f"W must be square, got {W.shape}")
    if W.diagonal().any():
        raise ValueError("coarsening_quality needs a graph without self-loops (S^T S = L, which the metrics rest on, fails there)")
    Cc = sp.csc_matrix(C)
    if Cc.shape[1] != N:
        raise ValueError(f"C has {Cc.shape[1]} columns, the graph has {N} nodes")
    Cc.sort_indices()
    if not np.all(np.diff(Cc.indptr) == 1):
        raise NotImplementedError("coarsening_quality needs a C with exactly one non-zero per column (what coarsen() produces)")
    dw = np.ravel(W.sum(axis=0))
    return W, dw, Cc.indices.astype(np.int32), Cc.data.astype(np.float64), int(Cc.shape[0])


def _lanczos_pairs(Lmat, k):
    """The k smallest eigenpairs by lanczos_smallest, run for k + 5 pairs: its stopping rule bounds every wanted residual by
    tol times the largest shifted eigenvalue, so the last wanted pairs are the loosest; the 5 extra ones absorb that."""
    N = Lmat.shape[0]
    K = k + 5
    m = min(127, N - 1, 4 * K + 20)
    if 2 * K + 7 > m:
        raise ValueError(f"spectral='device' cannot serve kmax={k} on a graph of {N} nodes (lanczos_smallest keeps at most "
                         f"min(127, N - 1) basis vectors and needs 2 (kmax + 5) + 7 of them); use spectral='arpack'")
    l, U = lanczos_smallest(Lmat, K, m=m)
    return l[:k], np.ascontiguousarray(U[:, :k])


def coarsening_quality(G, C, kmax=30, Uk=None, lk=None, device="cuda", spectral="arpack", Uc=None, lc=None, timings=None):
    """coarsening_quality (coarsening_utils.py:257-351) with the reference's arguments and returned dict: r, m, error_eigenvalue,
    angle_matrix, error_subspace, error_sintheta, with the reference's shapes in every branch (U = Uk whole when
    len(lk) >= kmax; the dense eig(Lc) branch when kmax > n / 2; kmax clipped to [1, n] and [2, n]).

    The reference's dense S (|E| x N) and M = S Pi U diag(l^-1/2) are never formed: ||M[:, :k+1]||_2 is the square root of the
    largest eigenvalue of the leading block of D U^T Pi L Pi U D (S^T S = L without self-loops).  On the device: Lc = C L C^T,
    C U and Y = C^T C U, G = Y^T L Y (one CSR pass per 64-column tile pair), the angle matrix (C U)^T Uc.  On the host: the
    eigenvalues of the leading blocks of D G D, the Frobenius norms, the coarse eigenproblem of the dense branch.

    spectral='arpack': the reference's eigsh(..., which='SM', tol=1e-3) calls and np.linalg.eigh for the dense branch;
    spectral='device': lanczos_smallest (tol 1e-5, kmax + 5 pairs) for L and Lc (kmax <= QUALITY_DEVICE_MAX_KMAX; the dense
    branch stays the n x n eigh, n < 2 kmax).  Uc, lc (extension): injected coarse eigenpairs, used instead of any coarse eigensolve.
    timings (extension): a dict that receives the seconds of each stage (the stream is synchronised between stages).
    Unlike the reference, the caller's lk is not modified (the reference sets lk[0] = 1 in place).
    C: a CoarseningMatrix or any scipy n x N matrix with exactly one non-zero per column (else NotImplementedError).
    Raises ValueError for a graph with self-loops or a C whose width is not G.N; there is no CPU fallback."""
    import time

    import scipy.sparse.linalg as spla

    W, dw, assign_h, cval_h, n = _quality_inputs(G, C)
    if spectral not in ("arpack", "device"):
        raise ValueError(f"spectral must be 'arpack' or 'device', got {spectral!r}")
    if spectral == "device" and kmax > QUALITY_DEVICE_MAX_KMAX:
        raise ValueError(f"spectral='device' serves kmax <= {QUALITY_DEVICE_MAX_KMAX} (lanczos_smallest: at most 127 basis vectors)")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.FitgnnError("coarsening_quality runs on the MI355X (no CPU fallback)")
    N = W.shape[0]
    tm = timings if timings is not None else {}

    def stage(name, t0):
        if timings is not None:
            torch.cuda.synchronize(dev)
        tm[name] = tm.get(name, 0.0) + time.perf_counter() - t0

    Lfull = (sp.diags(dw, 0) - W).tocsc()
    t0 = time.perf_counter()
    if (Uk is not None) and (lk is not None) and (len(lk) >= kmax):
        U, l = np.asarray(Uk), np.array(lk, dtype=np.float64)
    elif hasattr(G, "U") and hasattr(G, "e"):
        U, l = np.asarray(G.U), np.array(G.e, dtype=np.float64)
    elif spectral == "device":
        l, U = _lanczos_pairs(Lfull, kmax)
    else:
        l, U = spla.eigsh(Lfull, k=kmax, which="SM", tol=1e-3)
    stage("eig_L", t0)
    l = np.array(l, dtype=np.float64)
    l[0] = 1
    linv = l ** (-0.5)
    linv[0] = 0

    t0 = time.perf_counter()
    assign, cval = _dev(assign_h, torch.int32, dev), _dev(cval_h, torch.float64, dev)
    Lc = coarse_laplacian(W, dw, assign, cval, n)
    stage("Lc", t0)

    t0 = time.perf_counter()
    if Uc is not None and lc is not None:
        Uc, lc = np.asarray(Uc), np.asarray(lc)
    elif kmax > n / 2:
        lc, Uc = np.linalg.eigh(Lc.toarray())      # graph_utils.eig: ascending
        o = lc.argsort()
        lc, Uc = np.real(lc[o]), Uc[:, o]
    elif spectral == "device":
        lc, Uc = _lanczos_pairs(Lc, kmax)
    else:
        lc, Uc = spla.eigsh(Lc, k=kmax, which="SM", tol=1e-3)
    stage("eig_Lc", t0)

    metrics = {"r": 1 - n / N, "m": int((np.count_nonzero(Lc.data) - n) / 2)}
    ke = int(np.clip(kmax, 1, n))
    err = np.abs(l[:ke] - lc[:ke]) / l[:ke]
    err[0] = 0
    metrics["error_eigenvalue"] = err

    kl = int(np.clip(ke, 2, n))
    kU = U.shape[1]
    kg = min(kl, kU)                       # M's columns the loop reads
    t0 = time.perf_counter()
    Ud = _dev(np.real(U), torch.float64, dev)
    CU, Y = project_lift(assign, cval, n, Ud)
    stage("project", t0)
    t0 = time.perf_counter()
    Gd = laplacian_gram(W, dw, Y[:, :kg]).cpu().numpy()
    stage("gram", t0)
    t0 = time.perf_counter()
    Ucd = _dev(np.real(Uc), torch.float64, dev)
    ang = cross_atb(CU, Ucd).cpu().numpy()
    if np.iscomplexobj(Uc):
        ang = ang + 1j * cross_atb(CU, _dev(np.imag(Uc), torch.float64, dev)).cpu().numpy()
    stage("cross", t0)
    metrics["angle_matrix"] = ang

    MtM = linv[:kg, None] * Gd * linv[None, :kg]
    MtM = (MtM + MtM.T) / 2
    error_subspace = np.zeros(kl)
    error_sintheta = np.zeros(kl)
    for kIdx in range(1, kl):
        b = min(kIdx + 1, kg)
        lam = float(np.linalg.eigvalsh(MtM[:b, :b])[-1])
        error_subspace[kIdx] = np.abs(np.sqrt(max(lam, 0.0)) - 1)
        error_sintheta[kIdx] = np.linalg.norm(ang[0:kIdx + 1, kIdx + 1:], ord="fro") ** 2
    metrics["error_subspace"] = error_subspace
    metrics["error_sintheta"] = error_sintheta
    return metrics
