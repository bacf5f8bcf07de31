// matching.hip -- the matching-based coarsening methods of FIT-GNN's coarsen() (graph_coarsening/coarsening_utils.py):
// heavy_edge, algebraic_JC, affinity_GS (:658-811, test vectors :813-848) and variation_edges (:483-527), all of which
// contract a greedy matching (matching_greedy, :931-993).  The contraction's back half (fitgnn_build_assignment and after)
// is shared with variation_neighborhoods.
//
//   edge list        tril(W) in row-major order: the reference's get_edge_list() numbering, the matching's tie-break
//   proximity        one 16-lane group per edge, the edge's two K-vectors on its lanes (K <= FITGNN_MAX_K)
//   test vectors     Jacobi: row-parallel, one launch per iteration, ping-pong buffers;
//                    Gauss-Seidel: a forward substitution, one wavefront per component walking its rows in order
//   matching         stable rank (-weight, edge id) by radix sort, then locally-dominant rounds driven from the host
//
// This translation unit is compiled with -ffp-contract=off: the proximities are float32 roundings of float64 expressions
// the reference evaluates one operation at a time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "fitgnn_hip.h"
#include "match_arith.h"
#include "scan.h"

namespace {

constexpr size_t kAlign = 256;
inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }
inline dim3 blocks_for(int64_t threads, int block = 256) { return dim3((unsigned)((threads + block - 1) / block)); }

constexpr int kGroup = 16;     // lanes per edge / per row in the K-vector kernels (FITGNN_MAX_K == 16)
constexpr int kMaxChunk = 64;  // matching rounds launched between two reads of the round flags

// ------------------------------------------------------------------------------------------------
// edge list
// ------------------------------------------------------------------------------------------------
__global__ void tril_count_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int32_t N,
                                  int32_t *__restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int c = 0;
    for (int p = rowptr[i]; p < rowptr[i + 1] && col[p] < i; ++p) ++c;  // ascending columns: the lower part leads
    cnt[i] = c;
}

__global__ void tril_fill_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ w,
                                 int32_t N, const int32_t *__restrict__ edge_off, int64_t m_cap, int32_t *__restrict__ e_src,
                                 int32_t *__restrict__ e_dst, double *__restrict__ e_w, int32_t *__restrict__ csr_eid) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int b = rowptr[i], e = rowptr[i + 1];
    for (int p = b; p < e; ++p) {
        const int j = col[p];
        int32_t id = -1;
        if (j < i) {
            id = edge_off[i] + (p - b);
            if (id < m_cap) {
                e_src[id] = i;
                e_dst[id] = j;
                if (e_w) e_w[id] = w ? w[p] : 1.0;
            }
        } else if (j > i) {  // edge (j, i): position of i in row j
            int lo = rowptr[j], hi = rowptr[j + 1];
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (col[mid] < i) lo = mid + 1; else hi = mid;
            }
            id = edge_off[j] + (lo - rowptr[j]);
        }
        if (csr_eid) csr_eid[p] = id;
    }
}

// ------------------------------------------------------------------------------------------------
// proximity measures (get_proximity_measure, :658-730) and the variation_edges cost (:495-514)
// ------------------------------------------------------------------------------------------------
// column maxima of W (np.max(G.W, 0): implicit zeros take part, so the maximum is >= 0).  Non-negative doubles order like
// their bit patterns: an integer atomic max is exact and order-free.
__global__ void col_max_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ w,
                               int32_t N, unsigned long long *__restrict__ wmax_bits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    for (int p = rowptr[i]; p < rowptr[i + 1]; ++p) {
        const double v = w ? w[p] : 1.0;
        if (v > 0.0) atomicMax(&wmax_bits[col[p]], (unsigned long long)__double_as_longlong(v));
    }
}

__global__ void heavy_edge_kernel(const int32_t *__restrict__ e_src, const int32_t *__restrict__ e_dst, const double *__restrict__ e_w,
                                  int64_t M, const unsigned long long *__restrict__ wmax_bits, float *__restrict__ prox) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= M) return;
    prox[e] = fitgnn_match::heavy_edge_prox(e_w[e], __longlong_as_double((long long)wmax_bits[e_src[e]]),
                                            __longlong_as_double((long long)wmax_bits[e_dst[e]]));
}

__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = kGroup / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kGroup);
    return v;
}
__device__ __forceinline__ double group_min(double v) {
#pragma unroll
    for (int o = kGroup / 2; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, kGroup));
    return v;
}

// algebraic_JC: min_k 1 / max((X[i,k] - X[j,k])^2, 1e-6), rounded once to float32 (rounding is monotone: the
// reference's running float32 minimum is the rounded float64 minimum)
__global__ void jc_proximity_kernel(const int32_t *__restrict__ e_src, const int32_t *__restrict__ e_dst, int64_t M,
                                    const double *__restrict__ X, int32_t K, int64_t ldx, float *__restrict__ prox) {
    const int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    const int k = threadIdx.x % kGroup;
    if (e >= M) return;  // whole groups leave together (256 / kGroup groups per block)
    double v = __builtin_inf();
    if (k < K) v = fitgnn_match::jc_term(X[(int64_t)e_src[e] * ldx + k], X[(int64_t)e_dst[e] * ldx + k]);
    v = group_min(v);
    if (k == 0) prox[e] = (float)v;
}

// affinity_GS, first half: c_e = (x_i.x_j)^2 / ((x_i.x_i)^2 (x_j.x_j)^2) and the per-node maxima of c over incident edges
// (= the row maxima of the reference's dense symmetric c, whose other entries are 0)
__global__ void affinity_c_kernel(const int32_t *__restrict__ e_src, const int32_t *__restrict__ e_dst, int64_t M,
                                  const double *__restrict__ X, int32_t K, int64_t ldx, double *__restrict__ c,
                                  unsigned long long *__restrict__ cmax_bits) {
    const int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    const int k = threadIdx.x % kGroup;
    if (e >= M) return;
    const int i = e_src[e], j = e_dst[e];
    double xi = 0.0, xj = 0.0;
    if (k < K) {
        xi = X[(int64_t)i * ldx + k];
        xj = X[(int64_t)j * ldx + k];
    }
    const double ij = group_sum(xi * xj), ii = group_sum(xi * xi), jj = group_sum(xj * xj);
    if (k != 0) return;
    const double v = (ij * ij) / ((ii * ii) * (jj * jj));
    c[e] = v;
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);  // v >= 0
    atomicMax(&cmax_bits[i], b);
    atomicMax(&cmax_bits[j], b);
}
__global__ void affinity_prox_kernel(const int32_t *__restrict__ e_src, const int32_t *__restrict__ e_dst, int64_t M,
                                     const double *__restrict__ c, const unsigned long long *__restrict__ cmax_bits,
                                     float *__restrict__ prox) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= M) return;
    const double mi = __longlong_as_double((long long)cmax_bits[e_src[e]]);
    const double mj = __longlong_as_double((long long)cmax_bits[e_dst[e]]);
    prox[e] = (float)(c[e] / (mi * mj));
}

// variation_edges: ||B^T L2 B||_F with B = (I - 11^T/2) A[[i,j],:] is |a_i - a_j|^2 / 4 * (2 d_i + 2 d_j)
__global__ void edge_cost_kernel(const int32_t *__restrict__ e_src, const int32_t *__restrict__ e_dst, int64_t M,
                                 const double *__restrict__ dw, const double *__restrict__ A, int32_t K, int64_t lda,
                                 double *__restrict__ cost) {
    const int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    const int k = threadIdx.x % kGroup;
    if (e >= M) return;
    const int i = e_src[e], j = e_dst[e];
    double d = 0.0;
    if (k < K) d = A[(int64_t)i * lda + k] - A[(int64_t)j * lda + k];
    const double s = group_sum(d * d);
    if (k == 0) cost[e] = (s * 0.25) * (2.0 * dw[i] + 2.0 * dw[j]);
}

// ------------------------------------------------------------------------------------------------
// test vectors (generate_test_vectors, :813-848)
// ------------------------------------------------------------------------------------------------
// One Jacobi step x <- 0.5 x + 0.5 Dinv (D - L) x with the reference's float32 deg and deg^-1 (:836-840):
// (D - L) = W + diag(f32(dw) - dw), Dinv = f32(1 / f32(dw)) (0 where dw == 0).  One 16-lane group per row.
__global__ void jacobi_step_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ w,
                                   const double *__restrict__ dw, int32_t N, int32_t K, const double *__restrict__ x,
                                   double *__restrict__ y) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    const int k = threadIdx.x % kGroup;
    if (i >= N || k >= K) return;
    double acc = 0.0;
    for (int p = rowptr[i]; p < rowptr[i + 1]; ++p) acc = fitgnn_match::jacobi_acc(acc, w ? w[p] : 1.0, x[(int64_t)col[p] * K + k]);
    y[i * K + k] = fitgnn_match::jacobi_update(acc, x[i * K + k], dw[i]);
}

// One Gauss-Seidel sweep x <- -(D + L_lower)^-1 L_upper x (:822-832) on L = diag(dw) - W (zero diagonal of W):
//   out_i = (sum_{j>i} w_ij x_j + sum_{j<i} w_ij out_j) / dw_i
// One wavefront per component walks the component's rows in order; lanes split the row's entries (4 groups) x K (16 lanes).
// Rows written earlier are read back from L2 (agent-scope loads after the writer's fence): no other wavefront touches the
// component and nothing waits on another workgroup.
__global__ __launch_bounds__(64) void gauss_seidel_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                          const double *__restrict__ w, const double *__restrict__ dw, int32_t n_comp,
                                                          const int32_t *__restrict__ comp_off, int32_t K, const double *__restrict__ x,
                                                          double *out) {
    const int c = blockIdx.x;
    if (c >= n_comp) return;
    const int lane = threadIdx.x, k = lane % kGroup, g = lane / kGroup;
    for (int i = comp_off[c]; i < comp_off[c + 1]; ++i) {
        double acc = 0.0;
        if (k < K) {
            for (int p = rowptr[i] + g; p < rowptr[i + 1]; p += 64 / kGroup) {
                const int j = col[p];
                const double wij = w ? w[p] : 1.0;
                if (j > i) acc += wij * x[(int64_t)j * K + k];
                else if (j < i) acc += wij * __hip_atomic_load(&out[(int64_t)j * K + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        acc += __shfl_xor(acc, 16);
        acc += __shfl_xor(acc, 32);
        if (g == 0 && k < K) __hip_atomic_store(&out[(int64_t)i * K + k], acc / dw[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");  // row i is in L2 before any lane reads it for a later row
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------------
// greedy matching (matching_greedy, :931-993)
// ------------------------------------------------------------------------------------------------
// sort key of -weight: IEEE order as unsigned integers, -0 == +0, NaN last (numpy's argsort order)
__global__ void match_keys_kernel(const double *__restrict__ weight, int64_t M, uint64_t *__restrict__ keys, int32_t *__restrict__ ids) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= M) return;
    keys[e] = fitgnn_match::match_sort_key(weight[e]);
    ids[e] = (int32_t)e;
}
__global__ void node_comp_kernel(int32_t n_comp, const int32_t *__restrict__ comp_off, int32_t *__restrict__ comp_of) {
    const int c = blockIdx.x;
    if (c >= n_comp) return;
    for (int i = comp_off[c] + threadIdx.x; i < comp_off[c + 1]; i += blockDim.x) comp_of[i] = c;
}
__global__ void edge_comp_key_kernel(const int32_t *__restrict__ order1, const int32_t *__restrict__ e_src,
                                     const int32_t *__restrict__ comp_of, int64_t M, uint32_t *__restrict__ ckey) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < M) ckey[p] = (uint32_t)comp_of[e_src[order1[p]]];
}
__global__ void rank_kernel(const int32_t *__restrict__ order, int64_t M, int32_t *__restrict__ rank) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < M) rank[order[p]] = (int32_t)p;
}

// round, first half: every unmatched vertex points at the best-ranked incident edge whose other end is unmatched
__global__ void match_point_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                   const int32_t *__restrict__ csr_eid, int32_t N, const int32_t *__restrict__ rank,
                                   const uint8_t *__restrict__ matched, int32_t *__restrict__ ptr, int32_t *__restrict__ live) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    int32_t best = INT32_MAX;
    if (!matched[v]) {
        for (int p = rowptr[v]; p < rowptr[v + 1]; ++p) {
            const int u = col[p];
            if (u == v || matched[u]) continue;
            const int32_t r = rank[csr_eid[p]];
            best = r < best ? r : best;
        }
    }
    ptr[v] = best == INT32_MAX ? -1 : best;
    if (best != INT32_MAX) *live = 1;
}
// round, second half: an edge both of whose ends point at it joins the matching (its larger end writes)
__global__ void match_take_kernel(int32_t N, const int32_t *__restrict__ ptr, const int32_t *__restrict__ order,
                                  const int32_t *__restrict__ e_src, const int32_t *__restrict__ e_dst, uint8_t *__restrict__ matched,
                                  uint8_t *__restrict__ in_match) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    const int32_t r = ptr[v];
    if (r < 0) return;
    const int32_t e = order[r];
    if (e_src[e] != v) return;
    const int u = e_dst[e];
    if (ptr[u] != r) return;
    matched[v] = 1;
    matched[u] = 1;
    in_match[e] = 1;
}

__global__ void sorted_flag_kernel(const int32_t *__restrict__ order, int64_t M, const uint8_t *__restrict__ in_match,
                                   int32_t *__restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < M) flag[p] = in_match[order[p]];
}
// per component: matched edges kept = min(k_keep, matched); the component's edges occupy the sorted positions
// [edge_off[comp_off[c]], edge_off[comp_off[c+1]])
// (components that would keep <= min_gain pairs keep none: coarsening_utils.py:131-135 does not apply such a level)
__global__ void comp_take_kernel(int32_t n_comp, const int32_t *__restrict__ comp_off, const int32_t *__restrict__ edge_off,
                                 const int32_t *__restrict__ pos, const int64_t *__restrict__ k_keep, int64_t min_gain,
                                 int32_t *__restrict__ taken, int32_t *__restrict__ comp_taken) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_comp) return;
    const int64_t m = pos[edge_off[comp_off[c + 1]]] - pos[edge_off[comp_off[c]]];
    const int64_t k = k_keep[c] < 0 ? 0 : k_keep[c];
    const int32_t t = (int32_t)(m < k ? m : k);
    if (comp_taken) comp_taken[c] = t;
    taken[c] = t > min_gain ? t : 0;
}
__global__ void sel_write_kernel(const int32_t *__restrict__ order, int64_t M, const int32_t *__restrict__ flag,
                                 const int32_t *__restrict__ pos, const int32_t *__restrict__ e_src, const int32_t *__restrict__ e_dst,
                                 const int32_t *__restrict__ comp_of, const int32_t *__restrict__ comp_off,
                                 const int32_t *__restrict__ edge_off, const int32_t *__restrict__ taken,
                                 const int32_t *__restrict__ cbase, int32_t n_comp, int32_t *__restrict__ sel_off,
                                 int32_t *__restrict__ sel_mem, int32_t *__restrict__ sel_count) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) {
        const int32_t S = cbase[n_comp];
        sel_off[S] = 2 * S;
        sel_count[0] = S;
        sel_count[1] = 2 * S;
    }
    if (p >= M || !flag[p]) return;
    const int32_t e = order[p], i = e_src[e], c = comp_of[i];
    const int32_t q = pos[p] - pos[edge_off[comp_off[c]]];
    if (q < 0 || q >= taken[c]) return;
    const int32_t s = cbase[c] + q;
    sel_off[s] = 2 * s;
    sel_mem[2 * s] = i;  // the larger id keeps its row (get_coarsening_matrix :239, subgraph[0])
    sel_mem[2 * s + 1] = e_dst[e];
}

struct MatchLayout {
    size_t keys_in, keys_out, ids, order1, order, rank, ckey_in, ckey_out, comp_of, matched, ptr, in_match, flag, pos, taken, cbase,
        live, sort_tmp, sort_tmp_bytes, total;
};
MatchLayout match_layout(int32_t N, int64_t M, int32_t n_comp) {
    MatchLayout L{};
    size_t o = 0;
    const size_t n = (size_t)(N > 0 ? N : 1), m = (size_t)(M > 0 ? M : 1), c = (size_t)(n_comp > 0 ? n_comp : 1);
    L.keys_in = o; o += align_up(m * 8);
    L.keys_out = o; o += align_up(m * 8);
    L.ids = o; o += align_up(m * 4);
    L.order1 = o; o += align_up(m * 4);
    L.order = o; o += align_up(m * 4);
    L.rank = o; o += align_up(m * 4);
    L.ckey_in = o; o += align_up(m * 4);
    L.ckey_out = o; o += align_up(m * 4);
    L.comp_of = o; o += align_up(n * 4);
    L.matched = o; o += align_up(n);
    L.ptr = o; o += align_up(n * 4);
    L.in_match = o; o += align_up(m);
    L.flag = o; o += align_up((m + 1) * 4);
    L.pos = o; o += align_up((m + 1) * 4);
    L.taken = o; o += align_up((c + 1) * 4);
    L.cbase = o; o += align_up((c + 1) * 4);
    L.live = o; o += align_up(kMaxChunk * 4);
    size_t t64 = 0, t32 = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t64, (uint64_t *)nullptr, (uint64_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, m, 0,
                                    64, (hipStream_t)0);
    (void)rocprim::radix_sort_pairs(nullptr, t32, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, m, 0,
                                    32, (hipStream_t)0);
    L.sort_tmp_bytes = std::max(t64, t32);
    L.sort_tmp = o; o += align_up(L.sort_tmp_bytes);
    L.total = o;
    return L;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int fitgnn_edge_list(const int32_t *rowptr, const int32_t *col, const double *w, int32_t N, int32_t *edge_off,
                                int32_t *e_src, int32_t *e_dst, double *e_w, int64_t m_cap, int32_t *csr_eid, void *stream) {
    if (N < 0 || m_cap < 0 || !edge_off) return FITGNN_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) return (int)hipMemsetAsync(edge_off, 0, sizeof(int32_t), s);
    if (!rowptr || !col || (m_cap > 0 && (!e_src || !e_dst))) return FITGNN_E_BADARG;
    hipLaunchKernelGGL(tril_count_kernel, blocks_for(N), dim3(256), 0, s, rowptr, col, N, edge_off);
    fitgnn::exclusive_scan_i32(edge_off, edge_off, N, s);
    hipLaunchKernelGGL(tril_fill_kernel, blocks_for(N), dim3(256), 0, s, rowptr, col, w, N, edge_off, m_cap, e_src, e_dst, e_w, csr_eid);
    return (int)hipGetLastError();
}

extern "C" size_t fitgnn_heavy_edge_proximity_workspace_bytes(int32_t N) {
    if (N < 0) return 0;
    return align_up((size_t)(N > 0 ? N : 1) * 8);
}

extern "C" int fitgnn_heavy_edge_proximity(const int32_t *rowptr, const int32_t *col, const double *w, int32_t N, const int32_t *e_src,
                                           const int32_t *e_dst, const double *e_w, int64_t M, float *prox, void *work,
                                           size_t work_bytes, void *stream) {
    if (N < 0 || M < 0) return FITGNN_E_BADARG;
    if (M == 0) return 0;
    if (!rowptr || !col || !e_src || !e_dst || !e_w || !prox || !work) return FITGNN_E_BADARG;
    if (work_bytes < fitgnn_heavy_edge_proximity_workspace_bytes(N)) return FITGNN_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *wmax = (unsigned long long *)work;
    FITGNN_RETURN_IF_HIP(hipMemsetAsync(wmax, 0, (size_t)N * 8, s));
    hipLaunchKernelGGL(col_max_kernel, blocks_for(N), dim3(256), 0, s, rowptr, col, w, N, wmax);
    hipLaunchKernelGGL(heavy_edge_kernel, blocks_for(M), dim3(256), 0, s, e_src, e_dst, e_w, M, wmax, prox);
    return (int)hipGetLastError();
}

extern "C" int fitgnn_jc_proximity(const int32_t *e_src, const int32_t *e_dst, int64_t M, const double *X, int32_t K, int64_t ldx,
                                   float *prox, void *stream) {
    if (M < 0 || K < 1 || K > FITGNN_MAX_K || ldx < K) return FITGNN_E_BADARG;
    if (M == 0) return 0;
    if (!e_src || !e_dst || !X || !prox) return FITGNN_E_BADARG;
    hipLaunchKernelGGL(jc_proximity_kernel, blocks_for(M * kGroup), dim3(256), 0, (hipStream_t)stream, e_src, e_dst, M, X, K, ldx, prox);
    return (int)hipGetLastError();
}

extern "C" size_t fitgnn_affinity_proximity_workspace_bytes(int32_t N, int64_t M) {
    if (N < 0 || M < 0) return 0;
    return align_up((size_t)(N > 0 ? N : 1) * 8) + align_up((size_t)(M > 0 ? M : 1) * 8);
}

extern "C" int fitgnn_affinity_proximity(int32_t N, const int32_t *e_src, const int32_t *e_dst, int64_t M, const double *X, int32_t K,
                                         int64_t ldx, float *prox, void *work, size_t work_bytes, void *stream) {
    if (N < 0 || M < 0 || K < 1 || K > FITGNN_MAX_K || ldx < K) return FITGNN_E_BADARG;
    if (M == 0) return 0;
    if (!e_src || !e_dst || !X || !prox || !work) return FITGNN_E_BADARG;
    if (work_bytes < fitgnn_affinity_proximity_workspace_bytes(N, M)) return FITGNN_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *cmax = (unsigned long long *)work;
    double *c = (double *)((char *)work + align_up((size_t)(N > 0 ? N : 1) * 8));
    FITGNN_RETURN_IF_HIP(hipMemsetAsync(cmax, 0, (size_t)N * 8, s));
    hipLaunchKernelGGL(affinity_c_kernel, blocks_for(M * kGroup), dim3(256), 0, s, e_src, e_dst, M, X, K, ldx, c, cmax);
    hipLaunchKernelGGL(affinity_prox_kernel, blocks_for(M), dim3(256), 0, s, e_src, e_dst, M, c, cmax, prox);
    return (int)hipGetLastError();
}

extern "C" int fitgnn_edge_variation_costs_f64(const int32_t *e_src, const int32_t *e_dst, int64_t M, const double *dw, const double *A,
                                               int32_t K, int64_t lda, double *cost, void *stream) {
    if (M < 0 || K < 1 || K > FITGNN_MAX_K || lda < K) return FITGNN_E_BADARG;
    if (M == 0) return 0;
    if (!e_src || !e_dst || !dw || !A || !cost) return FITGNN_E_BADARG;
    hipLaunchKernelGGL(edge_cost_kernel, blocks_for(M * kGroup), dim3(256), 0, (hipStream_t)stream, e_src, e_dst, M, dw, A, K, lda, cost);
    return (int)hipGetLastError();
}

extern "C" size_t fitgnn_jacobi_vectors_workspace_bytes(int32_t N, int32_t K) {
    if (N < 0 || K < 1 || K > FITGNN_MAX_K) return 0;
    return align_up((size_t)(N > 0 ? N : 1) * K * 8);
}

extern "C" int fitgnn_jacobi_vectors_f64(const int32_t *rowptr, const int32_t *col, const double *w, const double *dw, int32_t N,
                                         const double *X0, int32_t K, int32_t iterations, double *X, void *work, size_t work_bytes,
                                         void *stream) {
    if (N < 0 || K < 1 || K > FITGNN_MAX_K || iterations < 0) return FITGNN_E_BADARG;
    if (N == 0) return 0;
    if (!rowptr || !col || !dw || !X0 || !X || X0 == X || (iterations > 1 && !work)) return FITGNN_E_BADARG;
    if (iterations > 1 && work_bytes < fitgnn_jacobi_vectors_workspace_bytes(N, K)) return FITGNN_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (iterations == 0) return (int)hipMemcpyAsync(X, X0, (size_t)N * K * 8, hipMemcpyDeviceToDevice, s);
    double *tmp = (double *)work;
    const double *src = X0;
    for (int t = 0; t < iterations; ++t) {
        double *dst = ((iterations - 1 - t) % 2 == 0) ? X : tmp;  // the last step lands in X
        hipLaunchKernelGGL(jacobi_step_kernel, blocks_for((int64_t)N * kGroup), dim3(256), 0, s, rowptr, col, w, dw, N, K, src, dst);
        src = dst;
    }
    return (int)hipGetLastError();
}

extern "C" int fitgnn_gauss_seidel_vectors_f64(const int32_t *rowptr, const int32_t *col, const double *w, const double *dw, int32_t N,
                                               int32_t n_comp, const int32_t *comp_off, const double *X0, int32_t K, double *X,
                                               void *stream) {
    if (N < 0 || n_comp < 0 || K < 1 || K > FITGNN_MAX_K) return FITGNN_E_BADARG;
    if (N == 0 || n_comp == 0) return 0;
    if (!rowptr || !col || !dw || !comp_off || !X0 || !X || X0 == X) return FITGNN_E_BADARG;
    hipLaunchKernelGGL(gauss_seidel_kernel, dim3(n_comp), dim3(64), 0, (hipStream_t)stream, rowptr, col, w, dw, n_comp, comp_off, K, X0, X);
    return (int)hipGetLastError();
}

extern "C" size_t fitgnn_greedy_matching_workspace_bytes(int32_t N, int64_t M, int32_t n_comp) {
    if (N < 0 || M < 0 || M > INT32_MAX || n_comp < 0) return 0;
    return match_layout(N, M, n_comp).total;
}

extern "C" int fitgnn_greedy_matching(const int32_t *rowptr, const int32_t *col, const int32_t *csr_eid, int32_t N,
                                      const int32_t *edge_off, const int32_t *e_src, const int32_t *e_dst, int64_t M, const double *weight,
                                      int32_t n_comp, const int32_t *comp_off, const int64_t *k_keep, int64_t min_gain, int32_t *sel_off,
                                      int32_t *sel_mem, int32_t *sel_count, int32_t *comp_taken, int32_t *rounds, void *work,
                                      size_t work_bytes, void *stream) {
    if (N < 0 || M < 0 || M > INT32_MAX || n_comp < 0 || min_gain < 0 || !sel_off || !sel_count) return FITGNN_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (rounds) *rounds = 0;
    if (comp_taken && n_comp > 0) FITGNN_RETURN_IF_HIP(hipMemsetAsync(comp_taken, 0, (size_t)n_comp * 4, s));
    if (N == 0 || M == 0 || n_comp == 0) {
        FITGNN_RETURN_IF_HIP(hipMemsetAsync(sel_off, 0, sizeof(int32_t), s));
        return (int)hipMemsetAsync(sel_count, 0, 2 * sizeof(int32_t), s);
    }
    if (!rowptr || !col || !csr_eid || !edge_off || !e_src || !e_dst || !weight || !comp_off || !k_keep || !sel_mem || !work)
        return FITGNN_E_BADARG;
    const MatchLayout L = match_layout(N, M, n_comp);
    if (work_bytes < L.total) return FITGNN_E_WORKSPACE;
    char *base = (char *)work;
    uint64_t *keys_in = (uint64_t *)(base + L.keys_in), *keys_out = (uint64_t *)(base + L.keys_out);
    int32_t *ids = (int32_t *)(base + L.ids), *order1 = (int32_t *)(base + L.order1), *order = (int32_t *)(base + L.order);
    int32_t *rank = (int32_t *)(base + L.rank), *comp_of = (int32_t *)(base + L.comp_of), *ptr = (int32_t *)(base + L.ptr);
    uint32_t *ckey_in = (uint32_t *)(base + L.ckey_in), *ckey_out = (uint32_t *)(base + L.ckey_out);
    uint8_t *matched = (uint8_t *)(base + L.matched), *in_match = (uint8_t *)(base + L.in_match);
    int32_t *flag = (int32_t *)(base + L.flag), *pos = (int32_t *)(base + L.pos), *taken = (int32_t *)(base + L.taken),
            *cbase = (int32_t *)(base + L.cbase), *live = (int32_t *)(base + L.live);

    // rank = position in (component, -weight, edge id) order: stable 64-bit sort on -weight, then a stable sort on the component
    hipLaunchKernelGGL(match_keys_kernel, blocks_for(M), dim3(256), 0, s, weight, M, keys_in, ids);
    size_t tmp = L.sort_tmp_bytes;
    FITGNN_RETURN_IF_HIP(rocprim::radix_sort_pairs((void *)(base + L.sort_tmp), tmp, keys_in, keys_out, ids, n_comp > 1 ? order1 : order,
                                                   (size_t)M, 0, 64, s));
    hipLaunchKernelGGL(node_comp_kernel, dim3(n_comp), dim3(64), 0, s, n_comp, comp_off, comp_of);
    if (n_comp > 1) {
        int bits = 1;
        while ((1ll << bits) < (long long)n_comp) ++bits;
        hipLaunchKernelGGL(edge_comp_key_kernel, blocks_for(M), dim3(256), 0, s, order1, e_src, comp_of, M, ckey_in);
        tmp = L.sort_tmp_bytes;
        FITGNN_RETURN_IF_HIP(
            rocprim::radix_sort_pairs((void *)(base + L.sort_tmp), tmp, ckey_in, ckey_out, order1, order, (size_t)M, 0, bits, s));
    }
    hipLaunchKernelGGL(rank_kernel, blocks_for(M), dim3(256), 0, s, order, M, rank);

    // locally-dominant rounds: under a strict total order the mutual best edges of the unmatched vertices are edges the
    // sequential greedy scan takes, and the best remaining edge is always one of them (>= 1 match per live round).  The host
    // reads the rounds' "some vertex still points" flags after chunks of 1, 2, 4 .. 64 rounds; rounds past the last live one
    // find nothing to do.
    FITGNN_RETURN_IF_HIP(hipMemsetAsync(matched, 0, (size_t)N, s));
    FITGNN_RETURN_IF_HIP(hipMemsetAsync(in_match, 0, (size_t)M, s));
    int32_t live_h[kMaxChunk];
    int64_t n_rounds = 0;
    const int64_t max_rounds = (int64_t)N / 2 + 2;
    for (int chunk = 1;; chunk = std::min(2 * chunk, kMaxChunk)) {
        FITGNN_RETURN_IF_HIP(hipMemsetAsync(live, 0, (size_t)chunk * 4, s));
        for (int t = 0; t < chunk; ++t) {
            hipLaunchKernelGGL(match_point_kernel, blocks_for(N), dim3(256), 0, s, rowptr, col, csr_eid, N, rank, matched, ptr, live + t);
            hipLaunchKernelGGL(match_take_kernel, blocks_for(N), dim3(256), 0, s, N, ptr, order, e_src, e_dst, matched, in_match);
        }
        FITGNN_RETURN_IF_HIP(hipGetLastError());
        FITGNN_RETURN_IF_HIP(hipMemcpyAsync(live_h, live, (size_t)chunk * 4, hipMemcpyDeviceToHost, s));
        FITGNN_RETURN_IF_HIP(hipStreamSynchronize(s));
        int nl = 0;
        while (nl < chunk && live_h[nl]) ++nl;
        n_rounds += nl;
        if (nl < chunk) break;
        if (n_rounds > max_rounds) return FITGNN_E_BADARG;  // impossible under a total order; never spin
    }
    if (rounds) *rounds = (int32_t)n_rounds;

    // keep the first k_keep[c] matched edges of every component in rank order (matching_greedy's stopping rule, :983-985)
    hipLaunchKernelGGL(sorted_flag_kernel, blocks_for(M), dim3(256), 0, s, order, M, in_match, flag);
    fitgnn::exclusive_scan_i32(flag, pos, (int32_t)M, s);
    hipLaunchKernelGGL(comp_take_kernel, blocks_for(n_comp), dim3(256), 0, s, n_comp, comp_off, edge_off, pos, k_keep, min_gain, taken, comp_taken);
    fitgnn::exclusive_scan_i32(taken, cbase, n_comp, s);
    hipLaunchKernelGGL(sel_write_kernel, blocks_for(M), dim3(256), 0, s, order, M, flag, pos, e_src, e_dst, comp_of, comp_off, edge_off,
                       taken, cbase, n_comp, sel_off, sel_mem, sel_count);
    return (int)hipGetLastError();
}
