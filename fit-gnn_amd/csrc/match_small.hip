// match_small.hip -- the whole multilevel matching coarsening of small connected components in one wavefront each, state
// in LDS: coarsen() (coarsening_utils.py:60-182) with method heavy_edge or algebraic_JC, level by level, as the multi-launch
// path of matching.hip / coarsen.hip / lift_pool.hip computes it (same per-element arithmetic: match_arith.h).
//
// Per level, on the component's current graph (CSR with ascending columns, symmetric, no diagonal):
//   r_cur = clip(1 - n_target / n, 0, max_level_r)                                             (:65)
//   edge list tril(W) in row-major order (get_edge_list() numbering)
//   weights: heavy_edge proximity, or algebraic_JC: X0 = next n*K draws / sqrt(n), 20 Jacobi steps, proximity
//   rank (-weight, edge id), NaN last; sequential greedy scan stopped after match_keep(n, r_cur) pairs
//   a level of <= 2 pairs is not applied and ends the loop                                    (:131-135)
//   assignment as fitgnn_build_assignment (the larger end keeps its row), composed into the running C
//   lift: y[u][b] = sum_v w_uv p_v (ascending v), s[a][b] = sum_u y[u][b] p_u (ascending u), (s_ab + s_ba) / 2,
//         zeros dropped -- fitgnn_lift_adjacency's summation order
//   stop once n <= n_target or after max_levels levels                                         (:180)
//
// algebraic_JC runs as ONE chain (one workgroup walks the components in order: the draws of component c start where
// component c-1's ended); heavy_edge draws nothing, so every component is a workgroup of its own.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "common.h"
#include "fitgnn_hip.h"
#include "match_arith.h"

namespace {

constexpr int kThreads = 64;  // one wavefront per component
constexpr int kJacobiSteps = 20;
// algebraic_JC's single chain uses the full-budget layout, fixed at compile time: its LDS offsets are instruction immediates
// (a layout computed at run time costs the chain ~20 scalar registers, and the kernel spilled them)

// LDS carve-up for components of at most cn nodes and cz stored entries (X only for algebraic_JC: kx columns, two buffers)
struct SmallLayout {
    uint32_t flags, rowA, colA, wA, rowB, colB, wB, dw, x0, x1, cval, root, newid, partner, cnt, eoff, esrc, key, order, total;
};
__host__ __device__ constexpr uint32_t al16(uint32_t x) { return (x + 15u) & ~15u; }
__host__ __device__ constexpr SmallLayout small_layout(int cn, int cz, int kx) {
    SmallLayout L{};
    uint32_t o = 0;
    const uint32_t n = (uint32_t)cn, z = (uint32_t)cz, m = (uint32_t)(cz / 2 > 0 ? cz / 2 : 1), k = (uint32_t)kx;
    L.flags = o; o += 16;
    L.rowA = o; o += al16((n + 1) * 4);
    L.colA = o; o += al16(z * 4);
    L.wA = o; o += al16(z * 8);
    L.rowB = o; o += al16((n + 1) * 4);
    L.colB = o; o += al16(z * 4);
    L.wB = o; o += al16(z * 8);
    L.dw = o; o += al16(n * 8);
    L.x0 = o; o += al16(n * k * 8);
    L.x1 = o; o += al16(n * k * 8);
    L.cval = o; o += al16(n * 8);
    L.root = o; o += al16(n * 4);
    L.newid = o; o += al16(n * 4);
    L.partner = o; o += al16(n * 4);
    L.cnt = o; o += al16((n + 1) * 4);
    L.eoff = o; o += al16((n + 1) * 4);
    L.esrc = o; o += al16(m * 4);
    L.key = o; o += al16(m * 8);
    L.order = o; o += al16(m * 4);
    L.total = o;
    return L;
}

// a uniform pointer held in vector registers: the chain's input, output and draw pointers are offset by a lane index or
// used by one lane; in scalar registers they pushed the chain past the scalar register file (it spilled)
template <class T>
__device__ __forceinline__ T *in_vgpr(T *p) {
    uint64_t v = (uint64_t)p;
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    asm volatile("" : "+v"(lo));
    asm volatile("" : "+v"(hi));
    return (T *)(((uint64_t)hi << 32) | lo);
}

// matching_greedy's stopping rule (:983-985), as coarsening.match_keep computes it in float64
__device__ int64_t match_keep_dev(int64_t N, double r) {
#pragma clang fp contract(off)
    const double n_target = (1.0 - r) * (double)N;
    int64_t k = (int64_t)ceil((double)N - n_target);
    if (k < 1) k = 1;
    while (k > 1 && (double)(N - (k - 1)) <= n_target) --k;
    while ((double)(N - k) > n_target) ++k;
    return k;
}

// exclusive scan of a[0..n) in place by lane 0 (n <= FITGNN_MATCH_SMALL_MAX_NODES); a[n] = total
__device__ __forceinline__ void scan_lane0(int32_t *a, int n) {
    if (threadIdx.x == 0) {
        int32_t s = 0;
        for (int i = 0; i < n; ++i) { const int32_t v = a[i]; a[i] = s; s += v; }
        a[n] = s;
    }
    __syncthreads();
}

// entries of the current graph's row u whose column lies in cluster b (cluster of v = nid[v]), folded in ascending v:
// y = sum w_uv p_v; returns false when there are none
__device__ __forceinline__ bool lift_row_sum(const int32_t *row, const int32_t *col, const double *w, const int32_t *nid,
                                             const double *cv, int u, int b, double &y) {
    bool any = false;
    for (int p = row[u]; p < row[u + 1]; ++p) {
        const int v = col[p];
        if (nid[v] != b) continue;
        const double t = fitgnn_match::lift_mul(w[p], fitgnn_match::lift_p(cv[v]));
        y = any ? fitgnn_match::lift_add(y, t) : t;
        any = true;
    }
    return any;
}

// smallest cluster id > last among the neighbours of u (cluster a excluded), or INT32_MAX
__device__ __forceinline__ int next_cluster(const int32_t *row, const int32_t *col, const int32_t *nid, int u, int a, int last) {
    int best = INT32_MAX;
    for (int p = row[u]; p < row[u + 1]; ++p) {
        const int b = nid[col[p]];
        if (b != a && b > last && b < best) best = b;
    }
    return best;
}

template <bool JC>
__global__ __launch_bounds__(kThreads) void match_small_kernel(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ w,
    const int32_t *__restrict__ comp_off, int32_t c_begin, int32_t c_end, double r, int32_t K, int32_t max_levels,
    double max_level_r, const double *__restrict__ draws, int64_t n_draws, const double *__restrict__ sqrt_n, int32_t cn,
    int32_t cz, int32_t *__restrict__ assign, double *__restrict__ cval_out, int32_t *__restrict__ n_out,
    int32_t *__restrict__ levels_out, int32_t *__restrict__ status, int32_t *__restrict__ wc_rowptr, int32_t *__restrict__ wc_col,
    double *__restrict__ wc_w, int64_t *__restrict__ progress) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char lds[];
    constexpr SmallLayout kJcLayout = small_layout(FITGNN_MATCH_SMALL_MAX_NODES, FITGNN_MATCH_SMALL_MAX_NNZ, FITGNN_MATCH_SMALL_MAX_K);
    const SmallLayout Ly = JC ? kJcLayout : small_layout(cn, cz, 0);
    int32_t *rowA = (int32_t *)(lds + Ly.rowA), *colA = (int32_t *)(lds + Ly.colA);
    int32_t *rowB = (int32_t *)(lds + Ly.rowB), *colB = (int32_t *)(lds + Ly.colB);
    double *wA = (double *)(lds + Ly.wA), *wB = (double *)(lds + Ly.wB), *dw = (double *)(lds + Ly.dw);
    double *xa = (double *)(lds + Ly.x0), *xb = (double *)(lds + Ly.x1), *cv = (double *)(lds + Ly.cval);
    int32_t *root = (int32_t *)(lds + Ly.root), *nid = (int32_t *)(lds + Ly.newid), *partner = (int32_t *)(lds + Ly.partner);
    int32_t *cnt = (int32_t *)(lds + Ly.cnt), *eoff = (int32_t *)(lds + Ly.eoff), *esrc = (int32_t *)(lds + Ly.esrc);
    int32_t *order = (int32_t *)(lds + Ly.order);
    uint64_t *key = (uint64_t *)(lds + Ly.key);
    int32_t &s_flag = ((int32_t *)(lds + Ly.flags))[0], &s_taken = ((int32_t *)(lds + Ly.flags))[1];
    if (JC) {
        assign = in_vgpr(assign), cval_out = in_vgpr(cval_out), wc_rowptr = in_vgpr(wc_rowptr), wc_col = in_vgpr(wc_col);
        wc_w = in_vgpr(wc_w), draws = in_vgpr(draws), sqrt_n = in_vgpr(sqrt_n), col = in_vgpr(col), w = in_vgpr(w);
        status = in_vgpr(status), n_out = in_vgpr(n_out), levels_out = in_vgpr(levels_out), progress = in_vgpr(progress);
    }
    const int tid = threadIdx.x;
    const int m_cap = cz / 2 > 0 ? cz / 2 : 1;

    int64_t used = 0;  // draws consumed by the chain so far
    int c = JC ? c_begin : c_begin + (int)blockIdx.x;
    for (; c < c_end; ++c) {
        const int b0 = comp_off[c], N = comp_off[c + 1] - b0;
        const int p0 = rowptr[b0], nnz = rowptr[b0 + N] - p0;
        if (N < 0 || nnz < 0 || N > cn || nnz > cz) {  // reported back, never skipped silently
            if (tid == 0) status[c] = FITGNN_MATCH_TOO_BIG;
            break;
        }
        if (JC && used + (int64_t)K * N * max_levels > n_draws) break;  // worst-case need: N*K draws per level

        // ---- load and check the component ----
        if (tid == 0) s_flag = 0;
        for (int i = tid; i <= N; i += kThreads) rowA[i] = rowptr[b0 + i] - p0;
        for (int p = tid; p < nnz; p += kThreads) {
            colA[p] = col[p0 + p] - b0;
            wA[p] = w ? w[p0 + p] : 1.0;
        }
        __syncthreads();
        for (int i = tid; i < N; i += kThreads) {
            bool bad = rowA[i] > rowA[i + 1];
            for (int p = rowA[i]; p < rowA[i + 1] && !bad; ++p)
                bad = colA[p] < 0 || colA[p] >= N || colA[p] == i || (p > rowA[i] && colA[p] <= colA[p - 1]);
            if (bad) s_flag = 1;
        }
        for (int j = b0 + tid; j < b0 + N; j += kThreads) {
            assign[j] = j - b0;
            cval_out[j] = 1.0;
        }
        __syncthreads();
        if (s_flag) {
            if (tid == 0) status[c] = FITGNN_MATCH_BAD_INPUT;
            break;
        }

        // ---- the levels (:60-182) ----
        const double n_target = ceil((1.0 - r) * (double)N);
        int n = N, levels = 0;
        #pragma unroll 1
        for (int level = 1; level <= max_levels && N > 1; ++level) {
            const double rr = 1.0 - n_target / (double)n;
            const double r_cur = rr < 0.0 ? 0.0 : (rr > max_level_r ? max_level_r : rr);
            // edge list tril(W): edges of row i are its entries with a column < i (ascending columns: the leading ones)
            for (int i = tid; i < n; i += kThreads) {
                int k = 0;
                for (int p = rowA[i]; p < rowA[i + 1] && colA[p] < i; ++p) ++k;
                eoff[i] = k;
                double s = 0.0, mx = 0.0;  // degree (scipy's column sum: the row in column order) / column maximum
                for (int p = rowA[i]; p < rowA[i + 1]; ++p) {
                    s = s + wA[p];
                    if (wA[p] > mx) mx = wA[p];
                }
                dw[i] = JC ? s : mx;
            }
            __syncthreads();
            scan_lane0(eoff, n);
            const int M = eoff[n];
            if (M > m_cap) {  // an asymmetric pattern; never write past the edge arrays
                if (tid == 0) s_flag = 1;
                break;
            }
            for (int i = tid; i < n; i += kThreads)
                for (int q = 0; q < eoff[i + 1] - eoff[i]; ++q) esrc[eoff[i] + q] = i;
            if (JC) {
                // generate_test_vectors (:816): X0 = randn(n, K) / sqrt(n), row-major, then 20 Jacobi steps (:836-846)
                const double sq = sqrt_n[n];
                for (int t = tid; t < n * K; t += kThreads) xa[t] = draws[used + t] / sq;
                used += (int64_t)n * K;
                __syncthreads();
                #pragma unroll 1
                for (int it = 0; it < kJacobiSteps; ++it) {  // even steps xa -> xb, odd steps xb -> xa
                    const double *src = (it & 1) ? xb : xa;
                    double *dst = (it & 1) ? xa : xb;
                    for (int t = tid; t < n * K; t += kThreads) {
                        const int i = t / K, k = t - i * K;
                        double acc = 0.0;
                        for (int p = rowA[i]; p < rowA[i + 1]; ++p) acc = fitgnn_match::jacobi_acc(acc, wA[p], src[colA[p] * K + k]);
                        dst[t] = fitgnn_match::jacobi_update(acc, src[t], dw[i]);
                    }
                    __syncthreads();
                }
                const double *src = (kJacobiSteps & 1) ? xb : xa;
                for (int e = tid; e < M; e += kThreads) {
                    const int i = esrc[e], p = rowA[i] + (e - eoff[i]), j = colA[p];
                    double v = __builtin_inf();
                    for (int k = 0; k < K; ++k) v = fmin(v, fitgnn_match::jc_term(src[i * K + k], src[j * K + k]));
                    key[e] = fitgnn_match::match_sort_key((double)(float)v);
                }
            } else {
                __syncthreads();
                for (int e = tid; e < M; e += kThreads) {
                    const int i = esrc[e], p = rowA[i] + (e - eoff[i]), j = colA[p];
                    key[e] = fitgnn_match::match_sort_key((double)fitgnn_match::heavy_edge_prox(wA[p], dw[i], dw[j]));
                }
            }
            __syncthreads();
            // stable rank (key, edge id): position = number of edges before it
            for (int e = tid; e < M; e += kThreads) {
                const uint64_t ke = key[e];
                int pos = 0;
                #pragma unroll 1
                for (int f = 0; f < M; ++f) pos += (key[f] < ke || (key[f] == ke && f < e)) ? 1 : 0;
                order[pos] = e;
            }
            for (int i = tid; i < n; i += kThreads) { partner[i] = -1; root[i] = i; }
            __syncthreads();
            // greedy scan in rank order, truncated at match_keep (matching_greedy :931-993)
            if (tid == 0) {
                const int64_t keep = match_keep_dev(n, r_cur);
                int taken = 0;
                #pragma unroll 1
                for (int t = 0; t < M && taken < keep; ++t) {
                    const int e = order[t], i = esrc[e], j = colA[rowA[i] + (e - eoff[i])];
                    if (partner[i] >= 0 || partner[j] >= 0) continue;
                    partner[i] = j;
                    partner[j] = i;
                    root[j] = i;  // the larger id keeps its row (get_coarsening_matrix :239)
                    ++taken;
                }
                s_taken = taken;
            }
            __syncthreads();
            const int taken = s_taken;
            if (taken <= 2) break;  // :131-135: not applied, and the loop ends
            // assignment (fitgnn_build_assignment): survivors numbered in node order
            const double cpair = fitgnn_match::set_cval(2);
            for (int i = tid; i < n; i += kThreads) {
                cnt[i] = root[i] == i ? 1 : 0;
                cv[i] = partner[i] >= 0 ? cpair : 1.0;
            }
            __syncthreads();
            scan_lane0(cnt, n);
            for (int i = tid; i < n; i += kThreads) nid[i] = cnt[root[i]];
            const int nc = n - taken;
            __syncthreads();
            for (int j = b0 + tid; j < b0 + N; j += kThreads) {  // fitgnn_compose_levels
                const int prev = assign[j];
                cval_out[j] = fitgnn_match::lift_mul(cv[prev], cval_out[j]);
                assign[j] = nid[prev];
            }
            // lift, unsymmetrised, into B: coarse row a = cluster of survivor s, members (partner(s) < s, s)
            for (int s = tid; s < n; s += kThreads) {
                if (root[s] != s) continue;
                const int a = nid[s], u0 = partner[s] >= 0 ? partner[s] : s, u1 = partner[s] >= 0 ? s : -1;
                int k = 0;
                for (int last = -1;;) {
                    int bb = next_cluster(rowA, colA, nid, u0, a, last);
                    if (u1 >= 0) { const int b1 = next_cluster(rowA, colA, nid, u1, a, last); bb = b1 < bb ? b1 : bb; }
                    if (bb == INT32_MAX) break;
                    ++k;
                    last = bb;
                }
                cnt[a] = k;
            }
            __syncthreads();
            scan_lane0(cnt, nc);
            for (int s = tid; s < n; s += kThreads) {
                if (root[s] != s) continue;
                const int a = nid[s], u0 = partner[s] >= 0 ? partner[s] : s, u1 = partner[s] >= 0 ? s : -1;
                int q = cnt[a];
                rowB[a] = q;
                for (int last = -1;;) {
                    int bb = next_cluster(rowA, colA, nid, u0, a, last);
                    if (u1 >= 0) { const int b1 = next_cluster(rowA, colA, nid, u1, a, last); bb = b1 < bb ? b1 : bb; }
                    if (bb == INT32_MAX) break;
                    double y0 = 0.0, y1 = 0.0, sab = 0.0;
                    bool any = false;
                    if (lift_row_sum(rowA, colA, wA, nid, cv, u0, bb, y0)) {
                        sab = fitgnn_match::lift_mul(y0, fitgnn_match::lift_p(cv[u0]));
                        any = true;
                    }
                    if (u1 >= 0 && lift_row_sum(rowA, colA, wA, nid, cv, u1, bb, y1)) {
                        const double t = fitgnn_match::lift_mul(y1, fitgnn_match::lift_p(cv[u1]));
                        sab = any ? fitgnn_match::lift_add(sab, t) : t;
                    }
                    colB[q] = bb;
                    wB[q] = sab;
                    ++q;
                    last = bb;
                }
            }
            if (tid == 0) rowB[nc] = cnt[nc];
            __syncthreads();
            // symmetrise (s_ab + s_ba) / 2, drop zeros, back into A
            for (int a = tid; a < nc; a += kThreads) {
                int k = 0;
                for (int q = rowB[a]; q < rowB[a + 1]; ++q) {
                    const int bb = colB[q];
                    double t = 0.0;
                    for (int p = rowB[bb]; p < rowB[bb + 1]; ++p)
                        if (colB[p] == a) { t = wB[p]; break; }
                    k += fitgnn_match::lift_sym(wB[q], t) != 0.0 ? 1 : 0;
                }
                cnt[a] = k;
            }
            __syncthreads();
            scan_lane0(cnt, nc);
            for (int a = tid; a < nc; a += kThreads) {
                int o = cnt[a];
                rowA[a] = o;
                for (int q = rowB[a]; q < rowB[a + 1]; ++q) {
                    const int bb = colB[q];
                    double t = 0.0;
                    for (int p = rowB[bb]; p < rowB[bb + 1]; ++p)
                        if (colB[p] == a) { t = wB[p]; break; }
                    const double v = fitgnn_match::lift_sym(wB[q], t);
                    if (v != 0.0) { colA[o] = bb; wA[o] = v; ++o; }
                }
            }
            if (tid == 0) rowA[nc] = cnt[nc];
            __syncthreads();
            n = nc;
            ++levels;
            if ((double)n <= n_target) break;  // :180
        }
        __syncthreads();
        if (s_flag) {
            if (tid == 0) status[c] = FITGNN_MATCH_BAD_INPUT;
            break;
        }
        // ---- results: final Wc at the component's input slots ----
        const int nz = rowA[n];
        for (int i = tid; i <= n; i += kThreads) wc_rowptr[b0 + c + i] = rowA[i];
        for (int q = tid; q < nz; q += kThreads) {
            wc_col[p0 + q] = colA[q];
            wc_w[p0 + q] = wA[q];
        }
        if (tid == 0) {
            n_out[c] = n;
            levels_out[c] = levels;
            status[c] = FITGNN_MATCH_DONE;
        }
        __syncthreads();
        if (!JC) break;
    }
    if (JC && tid == 0 && progress) {
        progress[0] = c;
        progress[1] = used;
    }
}

// an empty chain's progress words: {c_begin, 0 draws}
__global__ void progress_kernel(int64_t *progress, int64_t c_begin) {
    progress[0] = c_begin;
    progress[1] = 0;
}

}  // namespace

extern "C" size_t fitgnn_match_small_lds_bytes(int32_t method, int32_t max_nodes, int32_t max_nnz, int32_t K) {
    if (method != FITGNN_MATCH_HEAVY_EDGE && method != FITGNN_MATCH_ALGEBRAIC_JC) return 0;
    if (max_nodes < 1 || max_nodes > FITGNN_MATCH_SMALL_MAX_NODES || max_nnz < 0 || max_nnz > FITGNN_MATCH_SMALL_MAX_NNZ) return 0;
    if (method == FITGNN_MATCH_ALGEBRAIC_JC && (K < 1 || K > FITGNN_MATCH_SMALL_MAX_K)) return 0;
    const size_t b = method == FITGNN_MATCH_ALGEBRAIC_JC
                         ? small_layout(FITGNN_MATCH_SMALL_MAX_NODES, FITGNN_MATCH_SMALL_MAX_NNZ, FITGNN_MATCH_SMALL_MAX_K).total
                         : small_layout(max_nodes, max_nnz, 0).total;
    return b <= FITGNN_MATCH_SMALL_LDS_BUDGET ? b : 0;
}

extern "C" int fitgnn_match_small(int32_t method, const int32_t *rowptr, const int32_t *col, const double *w, const int32_t *comp_off,
                                  int32_t c_begin, int32_t c_end, double r, int32_t K, int32_t max_levels, double max_level_r,
                                  const double *draws, int64_t n_draws, const double *sqrt_n, int32_t max_nodes, int32_t max_nnz,
                                  int32_t *assign, double *cval, int32_t *n_out, int32_t *levels, int32_t *status, int32_t *wc_rowptr,
                                  int32_t *wc_col, double *wc_w, int64_t *progress, void *stream) {
    const bool jc = method == FITGNN_MATCH_ALGEBRAIC_JC;
    if (method != FITGNN_MATCH_HEAVY_EDGE && !jc) return FITGNN_E_BADARG;
    if (c_begin < 0 || c_end < c_begin || max_levels < 0 || !(r >= 0.0 && r <= 1.0) || !(max_level_r >= 0.0 && max_level_r <= 1.0))
        return FITGNN_E_BADARG;
    const size_t lds = fitgnn_match_small_lds_bytes(method, max_nodes, max_nnz, K);
    if (lds == 0) return FITGNN_E_BADARG;  // over the LDS budget, or K / the caps out of range
    if (jc && (n_draws < 0 || (n_draws > 0 && !draws) || !sqrt_n || !progress)) return FITGNN_E_BADARG;
    if (c_end == c_begin) {
        if (jc) {
            hipLaunchKernelGGL(progress_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, progress, (int64_t)c_begin);
            return (int)hipGetLastError();
        }
        return 0;
    }
    if (!rowptr || !col || !comp_off || !assign || !cval || !n_out || !levels || !status || !wc_rowptr || !wc_col || !wc_w)
        return FITGNN_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (jc)
        hipLaunchKernelGGL(match_small_kernel<true>, dim3(1), dim3(kThreads), lds, s, rowptr, col, w, comp_off, c_begin, c_end, r, K,
                           max_levels, max_level_r, draws, n_draws, sqrt_n, max_nodes, max_nnz, assign, cval, n_out, levels, status,
                           wc_rowptr, wc_col, wc_w, progress);
    else
        hipLaunchKernelGGL(match_small_kernel<false>, dim3((unsigned)(c_end - c_begin)), dim3(kThreads), lds, s, rowptr, col, w, comp_off,
                           c_begin, c_end, r, K, max_levels, max_level_r, nullptr, (int64_t)0, nullptr, max_nodes, max_nnz, assign, cval,
                           n_out, levels, status, wc_rowptr, wc_col, wc_w, nullptr);
    return (int)hipGetLastError();
}
