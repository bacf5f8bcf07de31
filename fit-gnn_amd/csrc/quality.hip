// quality.hip -- the device half of coarsening_quality (graph_coarsening/coarsening_utils.py:257-351) on gfx950.
//
// The reference forms the dense incidence matrix S (E x N, graph_utils.py:45-61) and M = S Pi U diag(l^-1/2); only k x k
// results are needed: M^T M = D U^T Pi L Pi U D (S^T S = L without self-loops), so the device computes
//   Lc = C L C^T                         fitgnn_coarse_laplacian
//   CU = C U,  Y = C^T (C U) = Pi U      fitgnn_project_lift_f64
//   G  = Y1^T L Y2                       fitgnn_laplacian_gram_f64   (one pass over W's CSR per column tile)
//   A^T B (tall-skinny, n rows)          fitgnn_cross_atb_f64        ((C U)^T Uc: the angle matrix)
// All arithmetic is f64; every sum runs in a fixed order (per-workgroup partials over a row split that depends only on the
// sizes, then a fixed-order reduction): two launches give identical bits.  No floating-point atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "fitgnn_hip.h"

namespace {

constexpr size_t kAlign = 256;
inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }
inline dim3 blocks_for(int64_t threads, int block = 256) { return dim3((unsigned)((threads + block - 1) / block)); }
constexpr int kMaxCols = 64;        // FITGNN_QUALITY_MAX_K
constexpr int kMaxParts = 1024;     // workgroups of a Gram / cross-product pass (partials in the workspace)

// ---------------------------------------------------------------------------------------------------------------------
// cluster membership: members[off[a] .. off[a+1]) = the nodes of cluster a in ascending order (stable radix sort)
// ---------------------------------------------------------------------------------------------------------------------
struct MemberLayout {
    size_t key_in, key_out, id_in, members, off, sort_tmp, sort_tmp_bytes, total;
};
MemberLayout member_layout(int32_t N, int32_t n, size_t base) {
    MemberLayout L{};
    const size_t m = (size_t)(N > 0 ? N : 1);
    size_t o = base;
    L.key_in = o; o += align_up(m * 4);
    L.key_out = o; o += align_up(m * 4);
    L.id_in = o; o += align_up(m * 4);
    L.members = o; o += align_up(m * 4);
    L.off = o; o += align_up(((size_t)n + 1) * 4);
    size_t t = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
                                    m, 0, 32, (hipStream_t)0);
    L.sort_tmp_bytes = t;
    L.sort_tmp = o; o += align_up(t);
    L.total = o;
    return L;
}

__global__ void member_keys_kernel(int32_t N, const int32_t *__restrict__ assign, uint32_t *__restrict__ key, int32_t *__restrict__ id) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) { key[i] = (uint32_t)assign[i]; id[i] = i; }
}

__global__ void member_offsets_kernel(const uint32_t *__restrict__ skey, int32_t N, int32_t n, int32_t *__restrict__ off) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n) return;
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (skey[mid] < (uint32_t)c) lo = mid + 1; else hi = mid;
    }
    off[c] = lo;
}

int build_members(const MemberLayout &L, char *base, int32_t N, int32_t n, const int32_t *assign, hipStream_t s) {
    uint32_t *key_in = (uint32_t *)(base + L.key_in), *key_out = (uint32_t *)(base + L.key_out);
    int32_t *id_in = (int32_t *)(base + L.id_in), *members = (int32_t *)(base + L.members);
    if (N > 0) {
        hipLaunchKernelGGL(member_keys_kernel, blocks_for(N), dim3(256), 0, s, N, assign, key_in, id_in);
        size_t st = L.sort_tmp_bytes;
        FITGNN_RETURN_IF_HIP(rocprim::radix_sort_pairs((void *)(base + L.sort_tmp), st, key_in, key_out, id_in, members, (size_t)N, 0,
                                                       32, s));
    }
    hipLaunchKernelGGL(member_offsets_kernel, blocks_for((int64_t)n + 1), dim3(256), 0, s, key_out, N, n, (int32_t *)(base + L.off));
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// coarse Laplacian
// ---------------------------------------------------------------------------------------------------------------------
// ws[e] = c_u w_ue c_v for every CSR entry (u, v); ones[i] = 1 (the lift then sums c-scaled weights: C W C^T)
__global__ void scale_weights_kernel(int32_t N, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                     const double *__restrict__ w, const double *__restrict__ cval, double *__restrict__ ws,
                                     double *__restrict__ ones) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= N) return;
    ones[u] = 1.0;
    const double cu = cval[u];
    for (int e = rowptr[u]; e < rowptr[u + 1]; ++e) ws[e] = (cu * (w ? w[e] : 1.0)) * cval[col[e]];
}

// t_i = c_i^2 d_i - c_i sum_{j in N(i), assign j = assign i} w_ij c_j   (node i's share of its cluster's diagonal)
__global__ void diag_share_kernel(int32_t N, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                  const double *__restrict__ w, const double *__restrict__ dw, const int32_t *__restrict__ assign,
                                  const double *__restrict__ cval, double *__restrict__ t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int a = assign[i];
    double in = 0.0;
    for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) {
        const int j = col[e];
        if (assign[j] == a) in += (w ? w[e] : 1.0) * cval[j];
    }
    const double ci = cval[i];
    t[i] = ci * ci * dw[i] - ci * in;
}

// one thread per cluster: diagonal = sum of its members' shares in ascending node order, then its CSR row: -(off-diagonal
// lift entries) with the diagonal inserted at its sorted position
__global__ void coarse_rows_kernel(int32_t n, const int32_t *__restrict__ off, const int32_t *__restrict__ members,
                                   const double *__restrict__ t, const int32_t *__restrict__ rp_o, const int32_t *__restrict__ col_o,
                                   const double *__restrict__ val_o, int32_t *__restrict__ rowptr_c, int32_t *__restrict__ col_c,
                                   double *__restrict__ val_c, int32_t *__restrict__ nnz_c) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a > n) return;
    if (a == n) {
        rowptr_c[n] = rp_o[n] + n;
        nnz_c[0] = rp_o[n] + n;
        return;
    }
    double d = 0.0;
    for (int p = off[a]; p < off[a + 1]; ++p) d += t[members[p]];
    int o = rp_o[a] + a;
    rowptr_c[a] = o;
    bool placed = false;
    for (int e = rp_o[a]; e < rp_o[a + 1]; ++e) {
        const int b = col_o[e];
        if (!placed && b > a) { col_c[o] = a; val_c[o] = d; ++o; placed = true; }
        col_c[o] = b;
        val_c[o] = -val_o[e];
        ++o;
    }
    if (!placed) { col_c[o] = a; val_c[o] = d; }
}

struct CoarseLayout {
    size_t ones, ws, rp_o, col_o, val_o, nnz_o, t, lift, lift_bytes, total;
    MemberLayout mem;
};
CoarseLayout coarse_layout(int32_t N, int64_t nnz, int32_t n) {
    CoarseLayout L{};
    const size_t m = (size_t)(nnz > 0 ? nnz : 1), NN = (size_t)(N > 0 ? N : 1);
    size_t o = 0;
    L.ones = o; o += align_up(NN * 8);
    L.ws = o; o += align_up(m * 8);
    L.rp_o = o; o += align_up(((size_t)n + 1) * 4);
    L.col_o = o; o += align_up(m * 4);
    L.val_o = o; o += align_up(m * 8);
    L.nnz_o = o; o += align_up(4);
    L.t = o; o += align_up(NN * 8);
    L.mem = member_layout(N, n, o);
    o = L.mem.total;
    L.lift_bytes = fitgnn_lift_adjacency_workspace_bytes(N, nnz, n);
    L.lift = o; o += align_up(L.lift_bytes);
    L.total = o;
    return L;
}

// ---------------------------------------------------------------------------------------------------------------------
// project and lift
// ---------------------------------------------------------------------------------------------------------------------
// one wave per cluster, lane = column: CU[a][c] = sum over members (ascending) of cval[i] U[i][c]
__global__ __launch_bounds__(256) void project_kernel(const int32_t *__restrict__ off, const int32_t *__restrict__ members,
                                                      const double *__restrict__ cval, int32_t n, const double *__restrict__ U,
                                                      int64_t ldu, int32_t k, double *__restrict__ CU, int64_t ldcu) {
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int c = threadIdx.x & 63;
    if (a >= n || c >= k) return;
    double s = 0.0;
    for (int p = off[a]; p < off[a + 1]; ++p) {
        const int i = members[p];
        s += cval[i] * U[(int64_t)i * ldu + c];
    }
    CU[(int64_t)a * ldcu + c] = s;
}

__global__ void lift_rows_kernel(const int32_t *__restrict__ assign, const double *__restrict__ cval, int32_t N, const double *__restrict__ CU,
                                 int64_t ldcu, int32_t k, double *__restrict__ Y, int64_t ldy) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)N * k) return;
    const int i = (int)(t / k), c = (int)(t % k);
    Y[(int64_t)i * ldy + c] = cval[i] * CU[(int64_t)assign[i] * ldcu + c];
}

// ---------------------------------------------------------------------------------------------------------------------
// Gram / cross product: per-workgroup partials of sum_i y_i z_i^T over a contiguous row range, then a fixed-order reduction.
//   LAP:  y_i = Y1[i, :k1], z_i = dw_i Y2[i, :k2] - sum_j w_ij Y2[j, :k2]  (z = (L Y2)_i, formed in registers, staged in LDS)
//   else: y_i = A[i, :k1],  z_i = B[i, :k2]
// KP = padded column count (8, 16, 32, 64).  Phase A: lane c of a KP-lane group forms column c of one row; a tile holds TR rows.
// Phase B: each thread owns a BP x BP block of the KP x KP partial (S row subsets when KP^2 < 256), accumulated over the tile.
// ---------------------------------------------------------------------------------------------------------------------
template <int KP>
struct GramShape {
    static constexpr int ROWS_PER_PASS = 256 / KP;
    static constexpr int TR = ROWS_PER_PASS > 16 ? ROWS_PER_PASS : 16;
    static constexpr int PASSES = TR / ROWS_PER_PASS;
    static constexpr int ENT = KP * KP;
    static constexpr int BP = ENT >= 4096 ? 4 : (ENT >= 1024 ? 2 : 1);
    static constexpr int NB = KP / BP;
    static constexpr int S = 256 / (NB * NB);  // row subsets (1 unless KP = 8)
};

template <int KP, bool LAP>
__global__ __launch_bounds__(256) void gram_partial_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                           const double *__restrict__ w, const double *__restrict__ dw, int32_t N,
                                                           int32_t chunk, const double *__restrict__ Y1, int64_t ld1, int32_t k1,
                                                           const double *__restrict__ Y2, int64_t ld2, int32_t k2,
                                                           double *__restrict__ part) {
    using Sh = GramShape<KP>;
    __shared__ double sY[Sh::TR][KP];
    __shared__ double sZ[Sh::TR][KP + 1];
    __shared__ double sC[Sh::S > 1 ? Sh::S * KP * KP : 1];
    const int tid = threadIdx.x;
    const int r0 = tid / KP, c = tid % KP;
    const int sub = tid / (Sh::NB * Sh::NB), blk = tid % (Sh::NB * Sh::NB);
    const int bp = blk / Sh::NB, bq = blk % Sh::NB;
    double acc[Sh::BP][Sh::BP];
#pragma unroll
    for (int p = 0; p < Sh::BP; ++p)
#pragma unroll
        for (int q = 0; q < Sh::BP; ++q) acc[p][q] = 0.0;
    const int rbeg = blockIdx.x * chunk;
    const int rend = min(N, rbeg + chunk);
    for (int t0 = rbeg; t0 < rend; t0 += Sh::TR) {
        // ---- phase A: the tile's rows of y and z ----
#pragma unroll
        for (int ps = 0; ps < Sh::PASSES; ++ps) {
            const int r = ps * Sh::ROWS_PER_PASS + r0;
            const int i = t0 + r;
            double y = 0.0, z = 0.0;
            if (i < rend) {
                if (c < k1) y = Y1[(int64_t)i * ld1 + c];
                if (c < k2) {
                    if (LAP) {
                        double s = 0.0;
                        const int e1 = rowptr[i + 1];
                        for (int e = rowptr[i]; e < e1; ++e) s += (w ? w[e] : 1.0) * Y2[(int64_t)col[e] * ld2 + c];
                        z = dw[i] * Y2[(int64_t)i * ld2 + c] - s;
                    } else {
                        z = Y2[(int64_t)i * ld2 + c];
                    }
                }
            }
            sY[r][c] = y;
            sZ[r][c] = z;
        }
        __syncthreads();
        // ---- phase B: acc += y_r z_r^T over the tile's rows of this thread's subset ----
        for (int r = sub; r < Sh::TR; r += Sh::S) {
            double yv[Sh::BP], zv[Sh::BP];
#pragma unroll
            for (int p = 0; p < Sh::BP; ++p) yv[p] = sY[r][bp * Sh::BP + p];
#pragma unroll
            for (int q = 0; q < Sh::BP; ++q) zv[q] = sZ[r][bq * Sh::BP + q];
#pragma unroll
            for (int p = 0; p < Sh::BP; ++p)
#pragma unroll
                for (int q = 0; q < Sh::BP; ++q) acc[p][q] += yv[p] * zv[q];
        }
        __syncthreads();
    }
    double *out = part + (int64_t)blockIdx.x * k1 * k2;
    if (Sh::S > 1) {  // BP = 1: combine the row subsets in order
        sC[sub * KP * KP + blk] = acc[0][0];
        __syncthreads();
        if (sub == 0 && bp < k1 && bq < k2) {
            double s = sC[blk];
            for (int u = 1; u < Sh::S; ++u) s += sC[u * KP * KP + blk];
            out[bp * k2 + bq] = s;
        }
        return;
    }
#pragma unroll
    for (int p = 0; p < Sh::BP; ++p)
#pragma unroll
        for (int q = 0; q < Sh::BP; ++q) {
            const int gp = bp * Sh::BP + p, gq = bq * Sh::BP + q;
            if (gp < k1 && gq < k2) out[gp * k2 + gq] = acc[p][q];
        }
}

// out[p][q] = sum over the n_part partials in order: 64 entries per block, the four waves sum consecutive quarters, combined in order
__global__ __launch_bounds__(256) void partial_reduce_kernel(const double *__restrict__ part, int32_t n_part, int32_t k1, int32_t k2,
                                                             double *__restrict__ out, int64_t ldo) {
    __shared__ double sQ[4][64];
    const int ent = k1 * k2;
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    const int wv = threadIdx.x >> 6;
    const int q0 = (int)((int64_t)n_part * wv / 4), q1 = (int)((int64_t)n_part * (wv + 1) / 4);
    double s = 0.0;
    if (e < ent)
        for (int b = q0; b < q1; ++b) s += part[(int64_t)b * ent + e];
    sQ[wv][threadIdx.x & 63] = s;
    __syncthreads();
    if (wv == 0 && e < ent) {
        const int l = threadIdx.x;
        out[(int64_t)(e / k2) * ldo + (e % k2)] = ((sQ[0][l] + sQ[1][l]) + sQ[2][l]) + sQ[3][l];
    }
}

inline int pad_cols(int k) { return k <= 8 ? 8 : (k <= 16 ? 16 : (k <= 32 ? 32 : 64)); }
inline int tile_rows(int kp) { return kp == 8 ? 32 : 16; }

// the row split: depends on the sizes only (never on the device), so the sums are reproducible across devices
inline void row_split(int32_t N, int kp, int32_t &chunk, int32_t &parts) {
    const int tr = tile_rows(kp);
    const int64_t per = ((int64_t)N + kMaxParts - 1) / kMaxParts;
    chunk = (int32_t)((per + tr - 1) / tr * tr);
    if (chunk < tr) chunk = tr;
    parts = N > 0 ? (int32_t)(((int64_t)N + chunk - 1) / chunk) : 0;
}

size_t gram_workspace(int32_t N, int32_t k1, int32_t k2) {
    int32_t chunk = 0, parts = 0;
    row_split(N, pad_cols(k1 > k2 ? k1 : k2), chunk, parts);
    return align_up((size_t)(parts > 0 ? parts : 1) * (size_t)k1 * (size_t)k2 * 8);
}

template <bool LAP>
int launch_gram(int kp, const int32_t *rowptr, const int32_t *col, const double *w, const double *dw, int32_t N, const double *Y1,
                int64_t ld1, int32_t k1, const double *Y2, int64_t ld2, int32_t k2, double *G, int64_t ldg, double *part, hipStream_t s) {
    int32_t chunk = 0, parts = 0;
    row_split(N, kp, chunk, parts);
    const dim3 g(parts), b(256);
    switch (kp) {
        case 8: hipLaunchKernelGGL((gram_partial_kernel<8, LAP>), g, b, 0, s, rowptr, col, w, dw, N, chunk, Y1, ld1, k1, Y2, ld2, k2, part); break;
        case 16: hipLaunchKernelGGL((gram_partial_kernel<16, LAP>), g, b, 0, s, rowptr, col, w, dw, N, chunk, Y1, ld1, k1, Y2, ld2, k2, part); break;
        case 32: hipLaunchKernelGGL((gram_partial_kernel<32, LAP>), g, b, 0, s, rowptr, col, w, dw, N, chunk, Y1, ld1, k1, Y2, ld2, k2, part); break;
        default: hipLaunchKernelGGL((gram_partial_kernel<64, LAP>), g, b, 0, s, rowptr, col, w, dw, N, chunk, Y1, ld1, k1, Y2, ld2, k2, part); break;
    }
    hipLaunchKernelGGL(partial_reduce_kernel, blocks_for((int64_t)k1 * k2, 64), b, 0, s, part, parts, k1, k2, G, ldg);
    return (int)hipGetLastError();
}

int zero_block(double *G, int64_t ldg, int32_t k1, int32_t k2, hipStream_t s) {
    if (k1 == 0 || k2 == 0) return 0;
    return (int)hipMemset2DAsync(G, (size_t)ldg * 8, 0, (size_t)k2 * 8, (size_t)k1, s);
}

}  // namespace

extern "C" size_t fitgnn_coarse_laplacian_workspace_bytes(int32_t N, int64_t nnz, int32_t n) {
    if (N < 0 || nnz < 0 || n < 0) return 0;
    return coarse_layout(N, nnz, n).total;
}

extern "C" int fitgnn_coarse_laplacian(int32_t N, const int32_t *rowptr, const int32_t *col, const double *w, int64_t nnz,
                                       const double *dw, const int32_t *assign, const double *cval, int32_t n, int32_t *rowptr_c,
                                       int32_t *col_c, double *val_c, int32_t *nnz_c, void *work, size_t work_bytes, void *stream) {
    if (N < 0 || nnz < 0 || n < 0 || nnz > INT32_MAX - (int64_t)n || !rowptr_c || !nnz_c) return FITGNN_E_BADARG;
    if (n > 0 && (!col_c || !val_c)) return FITGNN_E_BADARG;
    if (N > 0 && (!rowptr || !dw || !assign || !cval || (nnz > 0 && !col))) return FITGNN_E_BADARG;
    if (n == 0 && N > 0) return FITGNN_E_BADARG;
    const CoarseLayout L = coarse_layout(N, nnz, n);
    if (!work || work_bytes < L.total) return FITGNN_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *base = (char *)work;
    double *ones = (double *)(base + L.ones), *ws = (double *)(base + L.ws), *t = (double *)(base + L.t);
    int32_t *rp_o = (int32_t *)(base + L.rp_o), *col_o = (int32_t *)(base + L.col_o), *nnz_o = (int32_t *)(base + L.nnz_o);
    double *val_o = (double *)(base + L.val_o);
    if (N > 0) hipLaunchKernelGGL(scale_weights_kernel, blocks_for(N), dim3(256), 0, s, N, rowptr, col, w, cval, ws, ones);
    FITGNN_RETURN_IF_HIP(hipGetLastError());
    // off-diagonal part: the lift of the c-scaled weights with unit C values = zero_diag(C W C^T), symmetrised, zeros dropped
    int rc = 0;
    if (nnz > 0) {
        rc = fitgnn_lift_adjacency(N, rowptr, col, ws, assign, ones, n, rp_o, col_o, val_o, nnz_o, base + L.lift, L.lift_bytes, stream);
        if (rc != 0) return rc;
    } else {  // no edges: no off-diagonal entries
        FITGNN_RETURN_IF_HIP(hipMemsetAsync(rp_o, 0, ((size_t)n + 1) * sizeof(int32_t), s));
    }
    rc = build_members(L.mem, base, N, n, assign, s);
    if (rc != 0) return rc;
    if (N > 0) hipLaunchKernelGGL(diag_share_kernel, blocks_for(N), dim3(256), 0, s, N, rowptr, col, w, dw, assign, cval, t);
    hipLaunchKernelGGL(coarse_rows_kernel, blocks_for((int64_t)n + 1), dim3(256), 0, s, n, (const int32_t *)(base + L.mem.off),
                       (const int32_t *)(base + L.mem.members), t, rp_o, col_o, val_o, rowptr_c, col_c, val_c, nnz_c);
    return (int)hipGetLastError();
}

extern "C" size_t fitgnn_project_lift_workspace_bytes(int32_t N, int32_t n) {
    if (N < 0 || n < 0) return 0;
    return member_layout(N, n, 0).total;
}

extern "C" int fitgnn_project_lift_f64(const int32_t *assign, const double *cval, int32_t N, int32_t n, const double *U, int64_t ldu,
                                       int32_t k, double *CU, int64_t ldcu, double *Y, int64_t ldy, void *work, size_t work_bytes,
                                       void *stream) {
    if (N < 0 || n < 0 || k < 0 || k > kMaxCols) return FITGNN_E_BADARG;
    if (k == 0 || (N == 0 && n == 0)) return 0;
    if (!assign || !cval || !U || !CU || ldu < k || ldcu < k || (Y && ldy < k)) return FITGNN_E_BADARG;
    if (n == 0 && N > 0) return FITGNN_E_BADARG;
    const MemberLayout L = member_layout(N, n, 0);
    if (!work || work_bytes < L.total) return FITGNN_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *base = (char *)work;
    int rc = build_members(L, base, N, n, assign, s);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, (const int32_t *)(base + L.off),
                       (const int32_t *)(base + L.members), cval, n, U, ldu, k, CU, ldcu);
    if (Y && N > 0) hipLaunchKernelGGL(lift_rows_kernel, blocks_for((int64_t)N * k), dim3(256), 0, s, assign, cval, N, CU, ldcu, k, Y, ldy);
    return (int)hipGetLastError();
}

extern "C" size_t fitgnn_laplacian_gram_workspace_bytes(int32_t N, int32_t k1, int32_t k2) {
    if (N < 0 || k1 < 0 || k2 < 0 || k1 > kMaxCols || k2 > kMaxCols) return 0;
    return gram_workspace(N, k1, k2);
}

extern "C" int fitgnn_laplacian_gram_f64(const int32_t *rowptr, const int32_t *col, const double *w, const double *dw, int32_t N,
                                         const double *Y1, int64_t ld1, int32_t k1, const double *Y2, int64_t ld2, int32_t k2, double *G,
                                         int64_t ldg, void *work, size_t work_bytes, void *stream) {
    if (N < 0 || k1 < 0 || k2 < 0 || k1 > kMaxCols || k2 > kMaxCols) return FITGNN_E_BADARG;
    if (k1 == 0 || k2 == 0) return 0;
    if (!G || ldg < k2) return FITGNN_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) return zero_block(G, ldg, k1, k2, s);
    if (!rowptr || !col || !dw || !Y1 || !Y2 || ld1 < k1 || ld2 < k2) return FITGNN_E_BADARG;
    if (!work || work_bytes < gram_workspace(N, k1, k2)) return FITGNN_E_WORKSPACE;
    return launch_gram<true>(pad_cols(k1 > k2 ? k1 : k2), rowptr, col, w, dw, N, Y1, ld1, k1, Y2, ld2, k2, G, ldg, (double *)work, s);
}

extern "C" size_t fitgnn_cross_atb_workspace_bytes(int32_t n, int32_t k1, int32_t k2) {
    if (n < 0 || k1 < 0 || k2 < 0 || k1 > kMaxCols || k2 > kMaxCols) return 0;
    return gram_workspace(n, k1, k2);
}

extern "C" int fitgnn_cross_atb_f64(const double *A, int64_t lda, int32_t k1, const double *B, int64_t ldb, int32_t k2, int32_t n,
                                    double *out, int64_t ldo, void *work, size_t work_bytes, void *stream) {
    if (n < 0 || k1 < 0 || k2 < 0 || k1 > kMaxCols || k2 > kMaxCols) return FITGNN_E_BADARG;
    if (k1 == 0 || k2 == 0) return 0;
    if (!out || ldo < k2) return FITGNN_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return zero_block(out, ldo, k1, k2, s);
    if (!A || !B || lda < k1 || ldb < k2) return FITGNN_E_BADARG;
    if (!work || work_bytes < gram_workspace(n, k1, k2)) return FITGNN_E_WORKSPACE;
    return launch_gram<false>(pad_cols(k1 > k2 ? k1 : k2), nullptr, nullptr, nullptr, nullptr, n, A, lda, k1, B, ldb, k2, out, ldo,
                              (double *)work, s);
}
