// query.hip -- node queries on the two-hop receptive field (inference.py:668-688 of the reference: the model on the ONE subgraph
// that holds the queried node, of whose output one row is kept).
//
// For the reference's default model (two GCNConv layers, ELU, lt1, eval mode) row q of the block-diagonal union needs only
//     T     = X W0^T                                                       (once per model: fitgnn_gemm_exact_f32)
//     h_j   = ELU(sum_{e' in row j} val[e'] T[xrow[col[e']]] + b0)          for j in row q's columns
//     g_q   = sum_{e in row q} val[e] h_{col[e]}                            fitgnn_gcn_query_gather_f32
//     z_q   = ELU(W1 g_q + b1);  out_q = Wl z_q + bl  (log_softmax)         fitgnn_gcn_query_tail_f32
// The union is block-diagonal, so both hops stay inside the query's subgraph: the values are the per-subgraph forward's.
// Two GATConv layers take the same tail behind fitgnn_gat_query_gather_f32 (attention over both hops: see gat_query_hops_kernel).
// Two GATConv layers of 2..8 heads have fitgnn_mhgat_query_gather_f32 (every head's attention over both hops: see mhgat_hops_kernel)
// and fitgnn_mhgat_query_tail_f32 (the tail with a grouped first product: see mhgat_tail_kernel).
// Two SAGEConv layers take it behind fitgnn_sage_query_gather_f32 (a gather plus a root term: see sage_query_gather_kernel).
// Two GINConv layers have launches of their own, fitgnn_gin_query_hops_f32 and fitgnn_gin_query_tail_f32 (a dense product behind a
// ReLU per one-hop row: see gin_query_hops_kernel).
// Graph-level models (a pool over a graph's rows in front of the head) have fitgnn_gcn_graph_query_hops_f32 and
// fitgnn_gcn_graph_query_tail_f32: a graph's layer-0 rows are formed once, in LDS (see graph_query_hops_kernel).  Two GINConv layers
// have fitgnn_gin_graph_query_hops_f32 and fitgnn_gin_graph_query_tail_f32: the dense product behind layer 0's ReLU runs once per
// row of the graph (see gin_graph_query_hops_kernel).  Two GATConv layers have fitgnn_gat_graph_query_hops_f32 in front of the GCN graph
// tail: a graph's attention rows and their two score dots are formed once, in LDS (see gat_graph_query_hops_kernel).  Two SAGEConv
// layers have fitgnn_sage_graph_query_hops_f32 in front of the same tail: a graph's mean-plus-root rows are formed once, in LDS, and
// a pooled row's own h is copied from there (see sage_graph_query_hops_kernel).
//
// Operation order (tests/query_reference.py mirrors it):
//   gather  a = 0; a = fmaf(val[e'], T[.][c], a) over row j's entries in CSR order; h = ELU(a + b0[c]), ELU(x) = x > 0 ? x : expm1f(x);
//           entry i of row q (CSR order) belongs to wave i % 4, which folds its entries in ascending i: p_w = fmaf(val[e], h, p_w);
//           g = ((p_0 + p_1) + p_2) + p_3 (a wave without entries holds 0).
//   tail    z[n] = ELU(fmaf chain over k ascending of G[q][k] W1[n][k], from 0, + b1[n])   (v_mfma_f32_16x16x4_f32: exact fp32,
//           bit-equal to that chain); logit[c] = (fmaf chain over h ascending of z[h] Wl[c][h], from 0) + bl[c];
//           log-softmax: m = max_c logit, s = sum_c expf(logit[c] - m) ascending c, out[c] = (logit[c] - m) - logf(s).
#include <algorithm>

#include "common.h"
#include "fitgnn_hip.h"

namespace {

constexpr int kGatherWaves = 4;

__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : expm1f(x); }

// One wave: columns c .. c + 3 of the sum of layer-0 row j before its bias, a = fmaf(val[e'], T[t(col[e'])][c], a) from 0 in CSR
// order.  Tc: the lane's column in T.  The row's entries are fetched 64 at a time and broadcast by v_readlane, four table rows in flight.
__device__ __forceinline__ float4 gcn_row(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
                                          const float *__restrict__ Tc, int64_t ldt, const int32_t *__restrict__ xrow, int j, int lane) {
    const int n0 = __builtin_amdgcn_readfirstlane(rowptr[j]), n1 = __builtin_amdgcn_readfirstlane(rowptr[j + 1]);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = n0; base < n1; base += 64) {
        const int cnt = min(64, n1 - base);
        int my = 0, mv = 0;
        if (lane < cnt) {
            const int cc = col[base + lane];
            my = xrow ? xrow[cc] : cc;
            mv = __float_as_int(val[base + lane]);
        }
        for (int k = 0; k < cnt; k += 4) {
            float4 t[4];
            float wv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // always four loads: a missing one re-reads entry k and is not folded
                const int idx = k + u < cnt ? k + u : k;
                const int node = __builtin_amdgcn_readlane(my, idx);
                wv[u] = __int_as_float(__builtin_amdgcn_readlane(mv, idx));
                t[u] = *reinterpret_cast<const float4 *>(Tc + (int64_t)node * ldt);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (k + u < cnt) {
                    a.x = fmaf(wv[u], t[u].x, a.x);
                    a.y = fmaf(wv[u], t[u].y, a.y);
                    a.z = fmaf(wv[u], t[u].z, a.z);
                    a.w = fmaf(wv[u], t[u].w, a.w);
                }
            }
        }
    }
    return a;
}

// One workgroup per (query, 256-column slab), the slab fastest so that all of a table row's slabs are in flight together; 64 lanes x
// float4 per slab (the columns are independent: the bits do not depend on the split).  The query's entries are dealt round-robin to
// the four waves; a wave forms its neighbour's layer-0 row from the table (gcn_row), applies + b0 and ELU and folds the row into its
// partial.  Any degree is served by the loops; the partials meet in LDS in wave order.
__global__ __launch_bounds__(256) void query_gather_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                           const float *__restrict__ val, const float *__restrict__ T, int64_t ldt,
                                                           const int32_t *__restrict__ xrow, const float *__restrict__ b0,
                                                           const int64_t *__restrict__ rows, int32_t H, float *__restrict__ G,
                                                           int64_t ldg, int32_t n_slabs) {
    __shared__ float4 part[kGatherWaves][64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = blockIdx.x / n_slabs, c0 = (blockIdx.x % n_slabs) * 256;
    const int64_t q = rows[qi];
    const int e0 = __builtin_amdgcn_readfirstlane(rowptr[q]), e1 = __builtin_amdgcn_readfirstlane(rowptr[q + 1]);
    const int deg = e1 - e0;
    const int c = c0 + lane * 4;
    const bool live = c < H;  // H % 4 == 0: a live lane owns four whole columns
    const float *Tc = T + (live ? c : 0);
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b0 && live) bias = make_float4(b0[c], b0[c + 1], b0[c + 2], b0[c + 3]);
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = w; i < deg; i += kGatherWaves) {
        const int j = __builtin_amdgcn_readfirstlane(col[e0 + i]);
        const float vq = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(val[e0 + i])));
        const float4 a = gcn_row(rowptr, col, val, Tc, ldt, xrow, j, lane);
        p.x = fmaf(vq, elu1(a.x + bias.x), p.x);
        p.y = fmaf(vq, elu1(a.y + bias.y), p.y);
        p.z = fmaf(vq, elu1(a.z + bias.z), p.z);
        p.w = fmaf(vq, elu1(a.w + bias.w), p.w);
    }
    part[w][lane] = p;
    __syncthreads();
    if (w == 0 && live) {
        float4 g = part[0][lane];
#pragma unroll
        for (int o = 1; o < kGatherWaves; ++o) {
            const float4 r = part[o][lane];
            g.x += r.x; g.y += r.y; g.z += r.z; g.w += r.w;
        }
        *reinterpret_cast<float4 *>(G + (int64_t)qi * ldg + c) = g;
    }
}

// ---- attention over both hops (two GATConv layers, heads = 1) ----
//   h_r = ELU(sum_k alpha_rk T[t(k)] + b0),  alpha_r. = softmax_k lrelu(a0s[t(k)] + a0d[t(r)], slope0)     k in CSR row r
//   g_q = sum_j beta_j h_j,                  beta     = softmax_j lrelu(u_s . h_j + u_d . h_q, slope1)      j in CSR row q
// Operation order (tests/gat_query_reference.py mirrors it).  A wave holds a whole row: lane l owns columns 4 l .. 4 l + 3 and, for
// H > 256, 256 + 4 l .. 256 + 4 l + 3.
//   row r    s = a0s[t(k)] + a0d[t(r)]; e = s > 0 ? s : slope0 * s; m = max_k e; p_k = expf(e_k - m); over the entries in CSR order
//            l = l + p_k, a = fmaf(p_k, T[t(k)][c], a) (both from 0); h = ELU(fmaf(a, 1 / l, b0[c])); a row without entries: ELU(b0).
//   dot      u . h: per lane d = fmaf(u[c], h[c], d) from 0 over its columns ascending, then d += d of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.
//   query q  every wave that has entries forms h_q itself (the same bits in each) and c_q = u_d . h_q.  Entry i of row q (CSR order)
//            belongs to wave i % 4, which folds its entries in ascending i into (M, L, P) = (-inf, 0, 0):
//            f = lrelu((u_s . h_j) + c_q, slope1);  f > M: x = expf(M - f), L = fmaf(L, x, 1), P = fmaf(P, x, h_j), M = f;
//            otherwise x = expf(f - M), L = L + x, P = fmaf(x, h_j, P).
//   merge    M = max_w M_w; x_w = expf(M_w - M); over w ascending L = fmaf(x_w, L_w, L), P = fmaf(x_w, P_w, P) (from 0);
//            g = P * (1 / L).  A wave without entries holds (-inf, 0, 0): x_w = 0.  A query without entries gives zeros.
constexpr int kHopsWaves = 4;

__device__ __forceinline__ float lrelu1(float x, float slope) {
#pragma clang fp contract(off)  // the product is rounded on its own: the row's maximum minus itself is exactly 0
    return x > 0.f ? x : slope * x;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

template <int NS>
__device__ __forceinline__ float row_dot(const float4 (&u)[NS], const float4 (&h)[NS]) {
    float d = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        d = fmaf(u[s].x, h[s].x, d);
        d = fmaf(u[s].y, h[s].y, d);
        d = fmaf(u[s].z, h[s].z, d);
        d = fmaf(u[s].w, h[s].w, d);
    }
    return wave_sum(d);
}

// One wave: layer-0 row r of the union into h.  Tc[s]: the lane's column of slot s in T (a lane past H reads column 0 and is never
// stored or counted: its u is 0).  The row's entries are fetched 64 at a time -- the table row and the weight ride on the lanes -- and
// broadcast by v_readlane, four table rows in flight.
template <int NS>
__device__ __forceinline__ void gat_row(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *const (&Tc)[NS],
                                        int64_t ldt, const int32_t *__restrict__ xrow, const float *__restrict__ a_src0,
                                        const float *__restrict__ a_dst0, float slope0, const float4 (&bias)[NS], int r, int lane,
                                        float4 (&h)[NS]) {
    const int n0 = __builtin_amdgcn_readfirstlane(rowptr[r]), n1 = __builtin_amdgcn_readfirstlane(rowptr[r + 1]);
    const int tr = __builtin_amdgcn_readfirstlane(xrow ? xrow[r] : r);
    const float ad = a_dst0[tr];
    float mx = -INFINITY;
    for (int base = n0 + lane; base < n1; base += 64) {
        const int cc = col[base];
        mx = fmaxf(mx, lrelu1(a_src0[xrow ? xrow[cc] : cc] + ad, slope0));
    }
    mx = wave_max(mx);
    float l = 0.f;
    float4 a[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) a[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = n0; base < n1; base += 64) {
        const int cnt = min(64, n1 - base);
        int my = 0, mv = 0;
        if (lane < cnt) {
            const int cc = col[base + lane];
            my = xrow ? xrow[cc] : cc;
            mv = __float_as_int(expf(lrelu1(a_src0[my] + ad, slope0) - mx));
        }
        for (int k = 0; k < cnt; k += 4) {
            float4 t[4][NS];
            float wv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // always four loads: a missing one re-reads entry k and is not folded
                const int idx = k + u < cnt ? k + u : k;
                const int node = __builtin_amdgcn_readlane(my, idx);
                wv[u] = __int_as_float(__builtin_amdgcn_readlane(mv, idx));
#pragma unroll
                for (int s = 0; s < NS; ++s) t[u][s] = *reinterpret_cast<const float4 *>(Tc[s] + (int64_t)node * ldt);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (k + u < cnt) {
                    l += wv[u];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        a[s].x = fmaf(wv[u], t[u][s].x, a[s].x);
                        a[s].y = fmaf(wv[u], t[u][s].y, a[s].y);
                        a[s].z = fmaf(wv[u], t[u][s].z, a[s].z);
                        a[s].w = fmaf(wv[u], t[u][s].w, a[s].w);
                    }
                }
            }
        }
    }
    const float inv = n1 > n0 ? 1.f / l : 0.f;  // l >= 1: the row's largest score gives expf(0)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        h[s].x = elu1(fmaf(a[s].x, inv, bias[s].x));
        h[s].y = elu1(fmaf(a[s].y, inv, bias[s].y));
        h[s].z = elu1(fmaf(a[s].z, inv, bias[s].z));
        h[s].w = elu1(fmaf(a[s].w, inv, bias[s].w));
    }
}

// One workgroup of four waves per query, every wave on whole rows of H <= 256 NS columns (the layer-1 score is a dot over the whole
// row of h_j).  The four online-softmax states meet in LDS in wave order.
template <int NS>
__global__ __launch_bounds__(256) void gat_query_hops_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                             const float *__restrict__ T, int64_t ldt, const int32_t *__restrict__ xrow,
                                                             const float *__restrict__ a_src0, const float *__restrict__ a_dst0,
                                                             const float *__restrict__ b0, float slope0, const float *__restrict__ u_src,
                                                             const float *__restrict__ u_dst, float slope1,
                                                             const int64_t *__restrict__ rows, int32_t H, float *__restrict__ G, int64_t ldg) {
    __shared__ float4 part[kHopsWaves][NS][64];
    __shared__ float ml[kHopsWaves][2];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = blockIdx.x;
    const int q = (int)rows[qi];
    const int e0 = __builtin_amdgcn_readfirstlane(rowptr[q]), e1 = __builtin_amdgcn_readfirstlane(rowptr[q + 1]);
    const int deg = e1 - e0;
    const float *Tc[NS];
    float4 bias[NS], us[NS], P[NS];
    bool live[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = s * 256 + lane * 4;
        live[s] = c < H;  // H % 4 == 0: a live lane owns four whole columns
        Tc[s] = T + (live[s] ? c : 0);
        bias[s] = us[s] = P[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live[s]) {
            if (b0) bias[s] = make_float4(b0[c], b0[c + 1], b0[c + 2], b0[c + 3]);
            us[s] = *reinterpret_cast<const float4 *>(u_src + c);
        }
    }
    float M = -INFINITY, Lw = 0.f;
    if (w < deg) {
        float4 h[NS];
        float cq;
        {
            float4 ud[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s)
                ud[s] = live[s] ? *reinterpret_cast<const float4 *>(u_dst + s * 256 + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            gat_row<NS>(rowptr, col, Tc, ldt, xrow, a_src0, a_dst0, slope0, bias, q, lane, h);
            cq = row_dot<NS>(ud, h);
        }
        for (int i = w; i < deg; i += kHopsWaves) {
            const int j = __builtin_amdgcn_readfirstlane(col[e0 + i]);
            gat_row<NS>(rowptr, col, Tc, ldt, xrow, a_src0, a_dst0, slope0, bias, j, lane, h);
            const float f = lrelu1(row_dot<NS>(us, h) + cq, slope1);
            if (f > M) {  // wave-uniform: every lane holds the butterfly's bits
                const float x = expf(M - f);
                Lw = fmaf(Lw, x, 1.f);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    P[s].x = fmaf(P[s].x, x, h[s].x);
                    P[s].y = fmaf(P[s].y, x, h[s].y);
                    P[s].z = fmaf(P[s].z, x, h[s].z);
                    P[s].w = fmaf(P[s].w, x, h[s].w);
                }
                M = f;
            } else {
                const float x = expf(f - M);
                Lw += x;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    P[s].x = fmaf(x, h[s].x, P[s].x);
                    P[s].y = fmaf(x, h[s].y, P[s].y);
                    P[s].z = fmaf(x, h[s].z, P[s].z);
                    P[s].w = fmaf(x, h[s].w, P[s].w);
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) part[w][s][lane] = P[s];
    if (lane == 0) {
        ml[w][0] = M;
        ml[w][1] = Lw;
    }
    __syncthreads();
    if (w != 0) return;
    float4 g[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) g[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (deg > 0) {
        float Mx = ml[0][0];
#pragma unroll
        for (int o = 1; o < kHopsWaves; ++o) Mx = fmaxf(Mx, ml[o][0]);
        float Ls = 0.f;
#pragma unroll
        for (int o = 0; o < kHopsWaves; ++o) {
            const float x = expf(ml[o][0] - Mx);  // a wave without entries: expf(-inf) = 0
            Ls = fmaf(x, ml[o][1], Ls);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float4 r = part[o][s][lane];
                g[s].x = fmaf(x, r.x, g[s].x);
                g[s].y = fmaf(x, r.y, g[s].y);
                g[s].z = fmaf(x, r.z, g[s].z);
                g[s].w = fmaf(x, r.w, g[s].w);
            }
        }
        const float inv = 1.f / Ls;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            g[s].x *= inv; g[s].y *= inv; g[s].z *= inv; g[s].w *= inv;
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s)
        if (live[s]) *reinterpret_cast<float4 *>(G + (int64_t)qi * ldg + s * 256 + lane * 4) = g[s];
}

// ---- attention over both hops, several heads (two GATConv layers with the same heads in 2..8, concat) ----
//   h_r[c]      = ELU(sum_k alpha^{hd(c)}_rk T[t(k)][c] + b0[c]),  alpha^{hd}_r. = softmax_k lrelu(a0s[t(k)][hd] + a0d[t(r)][hd], slope0)
//   G_q[hd H + c] = sum_j beta^{hd}_j h_j[c],                      beta^{hd} = softmax_j lrelu(U_s[hd] . h_j + U_d[hd] . h_q, slope1)
// hd(c) = c / C0, C0 = H / heads, C0 % 4 == 0: a lane's float4 lies in one head.  Every head weighs the SAME rows h_j, by a dot over
// all of H, so G is heads times as wide as h.  The operation order is gat_query_hops_kernel's, head by head (tests/
// mhgat_query_reference.py mirrors it): "row r" with the maximum, the weights and l of the column's own head; "dot", "query q" and
// "merge" once per head with (U_s[hd], U_d[hd]) and a state (M, L, P) of its own.  With equal layer-0 scores in every head, block hd
// of G holds the bits of gat_query_hops_kernel on (a0s[:, 0], a0d[:, 0], U_s[hd], U_d[hd]).
//
// How the weights reach the lanes: entries ride on the lanes, as in gat_row; lane k forms expf(e_k^{hd} - m^{hd}) for every head and
// writes it to a per-wave LDS tile wt[hd][64]; at entry k a lane reads wt[hd(its slot)][k], one broadcast per head group, and sums
// l of its slot's head from those values in CSR order: the very floats gat_row's v_readlane hands out, so l and everything after it
// have the single-head bits.
// Registers and LDS: a lane keeps a, h and four table rows in flight (as gat_row); the per-head scalars (a0d, m, c_q, M, L) ride on
// lane hd of one register each and are read by v_readlane; U_s[hd] and U_d[hd] are read from global memory per row (16 KiB: L1);
// the heads accumulators P^{hd} live in a per-wave LDS slab [heads][NS][64] float4, each lane reading and writing its own entries.
// LDS per workgroup: 4 heads NS KiB (P) + 8 KiB (wt) + 256 B (M, L): 72.25 KiB at heads = 8, H > 256 -- two workgroups per CU.
constexpr int kMhMaxHeads = 8;

__host__ __device__ constexpr size_t mhgat_hops_lds_bytes(int heads, int ns) {
    return ((size_t)kHopsWaves * heads * ns * 64 * 4 + (size_t)kHopsWaves * kMhMaxHeads * 64 + (size_t)kHopsWaves * kMhMaxHeads * 2) * sizeof(float);
}
static_assert(2 * mhgat_hops_lds_bytes(kMhMaxHeads, 2) <= 160 * 1024, "two workgroups per CU at heads = 8, H = 512");

__device__ __forceinline__ float lane_get(float v, int g) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), g)); }

// the lanes of ONE wave exchange values through LDS: the wave's LDS operations run in order, the compiler keeps them so
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// gat_row with a softmax per head: hd[s] is the head of the lane's columns in slot s, wt the wave's weight tile [kMhMaxHeads][64].
template <int NS>
__device__ __forceinline__ void mhgat_row(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *const (&Tc)[NS],
                                          int64_t ldt, const int32_t *__restrict__ xrow, const float *__restrict__ a_src0,
                                          const float *__restrict__ a_dst0, int heads, float slope0, const float4 (&bias)[NS],
                                          const int (&hd)[NS], float *wt, int r, int lane, float4 (&h)[NS]) {
    const int n0 = __builtin_amdgcn_readfirstlane(rowptr[r]), n1 = __builtin_amdgcn_readfirstlane(rowptr[r + 1]);
    const int tr = __builtin_amdgcn_readfirstlane(xrow ? xrow[r] : r);
    const float adv = lane < heads ? a_dst0[(int64_t)tr * heads + lane] : 0.f;  // lane g: a0d[t(r)][g]
    float mxv = -INFINITY;                                                     // lane g: the maximum of head g
    for (int base = n0; base < n1; base += 64) {
        const float *as = nullptr;
        if (base + lane < n1) {
            const int cc = col[base + lane];
            as = a_src0 + (int64_t)(xrow ? xrow[cc] : cc) * heads;
        }
        for (int g = 0; g < heads; ++g) {
            const float ad = lane_get(adv, g);
            float e = -INFINITY;
            if (as) e = lrelu1(as[g] + ad, slope0);
            e = wave_max(e);
            if (lane == g) mxv = fmaxf(mxv, e);
        }
    }
    float l[NS];
    float4 a[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        l[s] = 0.f;
        a[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int base = n0; base < n1; base += 64) {
        const int cnt = min(64, n1 - base);
        int my = 0;
        wave_lds_order();  // the previous tile has been read
        if (lane < cnt) {
            const int cc = col[base + lane];
            my = xrow ? xrow[cc] : cc;
        }
        for (int g = 0; g < heads; ++g) {
            const float ad = lane_get(adv, g), mx = lane_get(mxv, g);
            if (lane < cnt) wt[g * 64 + lane] = expf(lrelu1(a_src0[(int64_t)my * heads + g] + ad, slope0) - mx);
        }
        wave_lds_order();
        for (int k = 0; k < cnt; k += 4) {
            float4 t[4][NS];
            float wv[4][NS];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // always four loads: a missing one re-reads entry k and is not folded
                const int idx = k + u < cnt ? k + u : k;
                const int node = __builtin_amdgcn_readlane(my, idx);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    wv[u][s] = wt[hd[s] * 64 + idx];
                    t[u][s] = *reinterpret_cast<const float4 *>(Tc[s] + (int64_t)node * ldt);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (k + u < cnt) {
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        l[s] += wv[u][s];
                        a[s].x = fmaf(wv[u][s], t[u][s].x, a[s].x);
                        a[s].y = fmaf(wv[u][s], t[u][s].y, a[s].y);
                        a[s].z = fmaf(wv[u][s], t[u][s].z, a[s].z);
                        a[s].w = fmaf(wv[u][s], t[u][s].w, a[s].w);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const float inv = n1 > n0 ? 1.f / l[s] : 0.f;  // l >= 1: the head's largest score gives expf(0)
        h[s].x = elu1(fmaf(a[s].x, inv, bias[s].x));
        h[s].y = elu1(fmaf(a[s].y, inv, bias[s].y));
        h[s].z = elu1(fmaf(a[s].z, inv, bias[s].z));
        h[s].w = elu1(fmaf(a[s].w, inv, bias[s].w));
    }
}

// One workgroup of four waves per query, every wave on whole rows of H <= 256 NS columns; per head the four online-softmax states
// meet in LDS in wave order (wave w merges heads w, w + 4).  Dynamic LDS: mhgat_hops_lds_bytes(heads, NS).
template <int NS>
__global__ __launch_bounds__(256) void mhgat_hops_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                               const float *__restrict__ T, int64_t ldt, const int32_t *__restrict__ xrow,
                                                               const float *__restrict__ a_src0, const float *__restrict__ a_dst0,
                                                               int32_t heads, const float *__restrict__ b0, float slope0,
                                                               const float *__restrict__ U_src, const float *__restrict__ U_dst,
                                                               float slope1, const int64_t *__restrict__ rows, int32_t H,
                                                               float *__restrict__ G, int64_t ldg) {
    extern __shared__ float4 mh_smem[];
    float4 *part = mh_smem;                                                              // [waves][heads][NS][64]
    float *wt_all = reinterpret_cast<float *>(part + (size_t)kHopsWaves * heads * NS * 64);  // [waves][kMhMaxHeads][64]
    float *ml = wt_all + kHopsWaves * kMhMaxHeads * 64;                                  // [waves][kMhMaxHeads][2]
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = blockIdx.x;
    const int q = (int)rows[qi];
    const int e0 = __builtin_amdgcn_readfirstlane(rowptr[q]), e1 = __builtin_amdgcn_readfirstlane(rowptr[q + 1]);
    const int deg = e1 - e0;
    const int C0 = H / heads;
    float4 *Pw = part + (size_t)w * heads * NS * 64 + lane;  // head g, slot s: Pw[(g * NS + s) * 64]
    float *wt = wt_all + w * kMhMaxHeads * 64;
    const float *Tc[NS];
    float4 bias[NS];
    bool live[NS];
    int hd[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = s * 256 + lane * 4;
        live[s] = c < H;  // H % 4 == 0: a live lane owns four whole columns
        Tc[s] = T + (live[s] ? c : 0);
        hd[s] = live[s] ? c / C0 : 0;
        bias[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live[s] && b0) bias[s] = make_float4(b0[c], b0[c + 1], b0[c + 2], b0[c + 3]);
    }
    for (int g = 0; g < heads * NS; ++g) Pw[g * 64] = make_float4(0.f, 0.f, 0.f, 0.f);
    float Mv = -INFINITY, Lv = 0.f;  // lane g: the state of head g
    if (w < deg) {
        float4 h[NS], u[NS];
        float cqv = 0.f;  // lane g: U_d[g] . h_q
        mhgat_row<NS>(rowptr, col, Tc, ldt, xrow, a_src0, a_dst0, heads, slope0, bias, hd, wt, q, lane, h);
        for (int g = 0; g < heads; ++g) {
#pragma unroll
            for (int s = 0; s < NS; ++s)
                u[s] = live[s] ? *reinterpret_cast<const float4 *>(U_dst + (int64_t)g * H + s * 256 + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float c = row_dot<NS>(u, h);
            if (lane == g) cqv = c;
        }
        for (int i = w; i < deg; i += kHopsWaves) {
            const int j = __builtin_amdgcn_readfirstlane(col[e0 + i]);
            mhgat_row<NS>(rowptr, col, Tc, ldt, xrow, a_src0, a_dst0, heads, slope0, bias, hd, wt, j, lane, h);
            for (int g = 0; g < heads; ++g) {
#pragma unroll
                for (int s = 0; s < NS; ++s)
                    u[s] = live[s] ? *reinterpret_cast<const float4 *>(U_src + (int64_t)g * H + s * 256 + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float f = lrelu1(row_dot<NS>(u, h) + lane_get(cqv, g), slope1);
                const float M = lane_get(Mv, g);
                float4 *Pg = Pw + g * NS * 64;
                if (f > M) {  // wave-uniform: every lane holds the butterfly's bits
                    const float x = expf(M - f);
                    if (lane == g) {
                        Lv = fmaf(Lv, x, 1.f);
                        Mv = f;
                    }
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        float4 p = Pg[s * 64];
                        p.x = fmaf(p.x, x, h[s].x);
                        p.y = fmaf(p.y, x, h[s].y);
                        p.z = fmaf(p.z, x, h[s].z);
                        p.w = fmaf(p.w, x, h[s].w);
                        Pg[s * 64] = p;
                    }
                } else {
                    const float x = expf(f - M);
                    if (lane == g) Lv += x;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        float4 p = Pg[s * 64];
                        p.x = fmaf(x, h[s].x, p.x);
                        p.y = fmaf(x, h[s].y, p.y);
                        p.z = fmaf(x, h[s].z, p.z);
                        p.w = fmaf(x, h[s].w, p.w);
                        Pg[s * 64] = p;
                    }
                }
            }
        }
    }
    if (lane < heads) {
        ml[(w * kMhMaxHeads + lane) * 2] = Mv;
        ml[(w * kMhMaxHeads + lane) * 2 + 1] = Lv;
    }
    __syncthreads();
    for (int g = w; g < heads; g += kHopsWaves) {
        float4 o4[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) o4[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (deg > 0) {
            float Mx = ml[g * 2];
#pragma unroll
            for (int o = 1; o < kHopsWaves; ++o) Mx = fmaxf(Mx, ml[(o * kMhMaxHeads + g) * 2]);
            float Ls = 0.f;
#pragma unroll
            for (int o = 0; o < kHopsWaves; ++o) {
                const float x = expf(ml[(o * kMhMaxHeads + g) * 2] - Mx);  // a wave without entries: expf(-inf) = 0
                Ls = fmaf(x, ml[(o * kMhMaxHeads + g) * 2 + 1], Ls);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const float4 r = part[((size_t)(o * heads + g) * NS + s) * 64 + lane];
                    o4[s].x = fmaf(x, r.x, o4[s].x);
                    o4[s].y = fmaf(x, r.y, o4[s].y);
                    o4[s].z = fmaf(x, r.z, o4[s].z);
                    o4[s].w = fmaf(x, r.w, o4[s].w);
                }
            }
            const float inv = 1.f / Ls;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                o4[s].x *= inv; o4[s].y *= inv; o4[s].z *= inv; o4[s].w *= inv;
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (live[s]) *reinterpret_cast<float4 *>(G + (int64_t)qi * ldg + (int64_t)g * H + s * 256 + lane * 4) = o4[s];
    }
}

// ---- mean aggregation plus a root term (two SAGEConv layers) ----
//   T     = X [W_l0 ; W_r0]^T                                   [n_table x 2H]: columns [0, H) = X W_l0^T, [H, 2H) = X W_r0^T
//   h_r   = ELU(sum_{k in row r} val[k] T[t(col[k])][0:H] + T[t(r)][H:2H] + b_l0)           t(r) = xrow ? xrow[r] : r
//   g_q   = sum_{j in row q} val[j] h_{col[j]};   G[i] = [g_q | h_q]: the tail with K = 2H, W1 = [W_l1 | W_r1], b1 = b_l1 finishes.
// Operation order (tests/sage_query_reference.py mirrors it):
//   row r    a = 0; a = fmaf(val[e'], T[t(col[e'])][c], a) over row r's entries in CSR order; h_r[c] = ELU((a + T[t(r)][H + c]) + b0[c])
//            (b0 == NULL: the second add is absent), ELU(x) = x > 0 ? x : expm1f(x); a row without entries: ELU(T[t(r)][H + c] + b0[c]).
//   query q  the work items are q's deg(q) entries in CSR order followed by one more, q itself; item i belongs to wave i % 4, which
//            takes its items in ascending i.  An entry item folds p_w = fmaf(val[e], h_{col[e]}, p_w); the last item stores h_q straight
//            to G[i][H + c] and touches no partial.  g = ((p_0 + p_1) + p_2) + p_3 (a wave without entries holds 0).  A query without
//            entries gives g = 0 and still h_q.
// Every h is formed by the same code on a whole wave, whichever wave: the bits depend neither on the slab split nor on the wave.

// One wave: columns c .. c + 3 of layer-0 row r.  Tc: the lane's column in T's aggregate half; the root float4 at + H is requested
// before the entry loads, so that it is in flight with them.  The entries are fetched 64 at a time and broadcast by v_readlane,
// four table rows in flight (query_gather_kernel's scheme).
__device__ __forceinline__ float4 sage_row(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                           const float *__restrict__ val, const float *__restrict__ Tc, int64_t ldt, int32_t H,
                                           const int32_t *__restrict__ xrow, bool has_bias, const float4 &bias, int r, int lane) {
    const int n0 = __builtin_amdgcn_readfirstlane(rowptr[r]), n1 = __builtin_amdgcn_readfirstlane(rowptr[r + 1]);
    const int tr = __builtin_amdgcn_readfirstlane(xrow ? xrow[r] : r);
    const float4 root = *reinterpret_cast<const float4 *>(Tc + (int64_t)tr * ldt + H);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = n0; base < n1; base += 64) {
        const int cnt = min(64, n1 - base);
        int my = 0, mv = 0;
        if (lane < cnt) {
            const int cc = col[base + lane];
            my = xrow ? xrow[cc] : cc;
            mv = __float_as_int(val[base + lane]);
        }
        for (int k = 0; k < cnt; k += 4) {
            float4 t[4];
            float wv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // always four loads: a missing one re-reads entry k and is not folded
                const int idx = k + u < cnt ? k + u : k;
                const int node = __builtin_amdgcn_readlane(my, idx);
                wv[u] = __int_as_float(__builtin_amdgcn_readlane(mv, idx));
                t[u] = *reinterpret_cast<const float4 *>(Tc + (int64_t)node * ldt);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (k + u < cnt) {
                    a.x = fmaf(wv[u], t[u].x, a.x);
                    a.y = fmaf(wv[u], t[u].y, a.y);
                    a.z = fmaf(wv[u], t[u].z, a.z);
                    a.w = fmaf(wv[u], t[u].w, a.w);
                }
            }
        }
    }
    a.x += root.x; a.y += root.y; a.z += root.z; a.w += root.w;
    if (has_bias) {  // wave-uniform
        a.x += bias.x; a.y += bias.y; a.z += bias.z; a.w += bias.w;
    }
    return make_float4(elu1(a.x), elu1(a.y), elu1(a.z), elu1(a.w));
}

// One workgroup per (query, 256-column slab), the slab fastest; 64 lanes x float4 per slab.  The query's entries and, after them,
// the query itself are dealt round-robin to the four waves; the partials meet in LDS in wave order.
__global__ __launch_bounds__(256) void sage_query_gather_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                const float *__restrict__ val, const float *__restrict__ T, int64_t ldt,
                                                                const int32_t *__restrict__ xrow, const float *__restrict__ b0,
                                                                const int64_t *__restrict__ rows, int32_t H, float *__restrict__ G,
                                                                int64_t ldg, int32_t n_slabs) {
    __shared__ float4 part[kGatherWaves][64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int qi = blockIdx.x / n_slabs, c0 = (blockIdx.x % n_slabs) * 256;
    const int q = __builtin_amdgcn_readfirstlane((int)rows[qi]);
    const int e0 = __builtin_amdgcn_readfirstlane(rowptr[q]), e1 = __builtin_amdgcn_readfirstlane(rowptr[q + 1]);
    const int deg = e1 - e0;
    const int c = c0 + lane * 4;
    const bool live = c < H;  // H % 4 == 0: a live lane owns four whole columns
    const float *Tc = T + (live ? c : 0);
    const bool has_bias = b0 != nullptr;
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_bias && live) bias = make_float4(b0[c], b0[c + 1], b0[c + 2], b0[c + 3]);
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = w; i <= deg; i += kGatherWaves) {
        const bool self = i == deg;  // wave-uniform: the item after the last entry is q itself
        int j = q;
        float vq = 0.f;
        if (!self) {
            j = __builtin_amdgcn_readfirstlane(col[e0 + i]);
            vq = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(val[e0 + i])));
        }
        const float4 h = sage_row(rowptr, col, val, Tc, ldt, H, xrow, has_bias, bias, j, lane);
        if (self) {
            if (live) *reinterpret_cast<float4 *>(G + (int64_t)qi * ldg + H + c) = h;
        } else {
            p.x = fmaf(vq, h.x, p.x);
            p.y = fmaf(vq, h.y, p.y);
            p.z = fmaf(vq, h.z, p.z);
            p.w = fmaf(vq, h.w, p.w);
        }
    }
    part[w][lane] = p;
    __syncthreads();
    if (w == 0 && live) {
        float4 g = part[0][lane];
#pragma unroll
        for (int o = 1; o < kGatherWaves; ++o) {
            const float4 r = part[o][lane];
            g.x += r.x; g.y += r.y; g.z += r.z; g.w += r.w;
        }
        *reinterpret_cast<float4 *>(G + (int64_t)qi * ldg + c) = g;
    }
}

// ---- tail ----
constexpr int kTailQ = 16;      // queries per workgroup: one MFMA tile of rows
constexpr int kTailKS = 32;      // k-stage
constexpr int kTailLd = kTailKS + 4;  // stage row stride: 16 rows x 36 floats + the four k of a step fall on 64 distinct banks
constexpr int kTailCols = 256;   // columns of z per pass: 4 waves x 4 accumulators x 16
constexpr size_t kTailLdsMax = 160 * 1024;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr size_t tail_lds_floats(int H2, int C) {
    return (size_t)kTailQ * (H2 + 4) + (size_t)kTailCols * kTailLd + (size_t)kTailQ * kTailLd + (size_t)kTailQ * C;
}
static_assert(tail_lds_floats(512, 48) * sizeof(float) <= kTailLdsMax, "the default model's tail must fit LDS");

// The head and the log-softmax of a tile whose z [16][zld] is in LDS (written before a barrier): logits into lg [16][C], then out.
__device__ __forceinline__ void tail_head(const float *zs, int zld, int32_t H2, const float *__restrict__ Wl, const float *__restrict__ bl,
                                          int32_t C, float *lg, float *__restrict__ out, int64_t ldo, int q0, int nq, int32_t log_softmax) {
    const int tid = threadIdx.x;
    // the head: 16 consecutive lanes share a class (one broadcast read of Wl) and read 16 rows of z, 4 banks apart
    for (int o = tid; o < kTailQ * C; o += 256) {
        const int qi = o & (kTailQ - 1), c = o >> 4;
        const float *wl = Wl + (int64_t)c * H2;
        const float *z = zs + qi * zld;
        float s = 0.f;
        for (int h = 0; h < H2; h += 4) {
            const float4 wv = *reinterpret_cast<const float4 *>(wl + h);
            const float4 zv = *reinterpret_cast<const float4 *>(z + h);
            s = fmaf(zv.x, wv.x, s);
            s = fmaf(zv.y, wv.y, s);
            s = fmaf(zv.z, wv.z, s);
            s = fmaf(zv.w, wv.w, s);
        }
        lg[qi * C + c] = bl ? s + bl[c] : s;
    }
    __syncthreads();
    if (log_softmax) {
        if (tid < nq) {
            float *row = lg + tid * C;
            float m = row[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, row[c]);
            float s = 0.f;
            for (int c = 0; c < C; ++c) s += expf(row[c] - m);
            const float l = logf(s);
            for (int c = 0; c < C; ++c) row[c] = (row[c] - m) - l;
        }
        __syncthreads();
    }
    for (int o = tid; o < nq * C; o += 256) {  // rows of a partial last tile are not stored
        const int qi = o / C, c = o - qi * C;
        out[(int64_t)(q0 + qi) * ldo + c] = lg[o];
    }
}

// zs[r][n] = act(G[q0 + r] W1^T + b1), act = ELU or (kRelu) ReLU, for the 16 rows of a tile (rows r >= nq are computed as zeros and
// never read by the callers) and every column n < H2, on v_mfma_f32_16x16x4_f32 (A: lane l holds G[l & 15][k = l >> 4], B: W1[n = l & 15][k = l >> 4], C/D:
// column l & 15, rows 4 (l >> 4) + r), W1 and the tile's rows of G staged through LDS in k-stages of 32.  The first barrier of the
// first stage orders the readers of a previous tile's zs; the caller puts a barrier in front of its own reads.
template <bool kRelu>
__device__ __forceinline__ void tail_tile_z(const float *__restrict__ G, int64_t ldg, int64_t q0, int nq, const float *__restrict__ W1,
                                            const float *__restrict__ b1, int32_t H, int32_t H2, float *zs, int zld, float *Ws, float *Gs) {
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
    for (int n0 = 0; n0 < H2; n0 += kTailCols) {
        const int ncols = min(kTailCols, H2 - n0);  // a multiple of 16
        f32x4 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < H; k0 += kTailKS) {
            const int k4 = min(kTailKS, H - k0) >> 2;  // float4 per staged row (H % 4 == 0)
            __syncthreads();                           // the previous stage has been consumed
            for (int idx = tid; idx < ncols * k4; idx += 256) {
                const int n = idx / k4, kk = idx - n * k4;
                *reinterpret_cast<float4 *>(Ws + n * kTailLd + kk * 4) =
                    *reinterpret_cast<const float4 *>(W1 + (int64_t)(n0 + n) * H + k0 + kk * 4);
            }
            for (int idx = tid; idx < kTailQ * k4; idx += 256) {
                const int r = idx / k4, kk = idx - r * k4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);  // rows past Q: computed as zeros, never stored
                if (r < nq) v = *reinterpret_cast<const float4 *>(G + (int64_t)(q0 + r) * ldg + k0 + kk * 4);
                *reinterpret_cast<float4 *>(Gs + r * kTailLd + kk * 4) = v;
            }
            __syncthreads();
            for (int kk = 0; kk < k4; ++kk) {
                const float a = Gs[r16 * kTailLd + kk * 4 + kq];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int nb = (w * 4 + u) * 16;
                    if (nb < ncols) {  // wave-uniform
                        const float b = Ws[(nb + r16) * kTailLd + kk * 4 + kq];
                        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[u], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int nb = (w * 4 + u) * 16;
            if (nb < ncols) {
                const int n = n0 + nb + r16;
                const float bias = b1 ? b1[n] : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) zs[(kq * 4 + r) * zld + n] = kRelu ? fmaxf(acc[u][r] + bias, 0.f) : elu1(acc[u][r] + bias);
            }
        }
    }
}

// One workgroup per tile of up to 16 queries.  z = ELU(G W1^T + b1) by tail_tile_z; the tile's z stays in LDS, the head reads it
// from there.
__global__ __launch_bounds__(256) void query_tail_kernel(const float *__restrict__ G, int64_t ldg, int32_t Q, const float *__restrict__ W1,
                                                         const float *__restrict__ b1, const float *__restrict__ Wl,
                                                         const float *__restrict__ bl, int32_t H, int32_t H2, int32_t C,
                                                         float *__restrict__ out, int64_t ldo, int32_t log_softmax) {
    extern __shared__ float smem[];
    const int zld = H2 + 4;
    float *zs = smem;
    float *Ws = zs + (size_t)kTailQ * zld;
    float *Gs = Ws + kTailCols * kTailLd;
    float *lg = Gs + kTailQ * kTailLd;
    const int q0 = blockIdx.x * kTailQ;
    const int nq = min(kTailQ, Q - q0);

    tail_tile_z<false>(G, ldg, q0, nq, W1, b1, H, H2, zs, zld, Ws, Gs);
    __syncthreads();

    tail_head(zs, zld, H2, Wl, bl, C, lg, out, ldo, q0, nq, log_softmax);
}

// query_tail_kernel behind mhgat_hops_kernel: G is [Q][heads H] and z's block hd takes block hd of G only,
//     z[n] = ELU(W1[n, :] . G[q][hd1(n) H : (hd1(n) + 1) H] + b1[n]),   hd1(n) = n / C1, C1 = H2 / heads, C1 % 16 == 0.
// tail_tile_z's sweep with the A operand chosen per 16-column block: a pass of 256 columns of z walks k ONCE for all the heads it
// touches -- a k-stage holds W1[n][k0 .. k0 + 32) of the pass's columns and G[.][hd H + k0 .. + 32) of each of its heads, and the
// block of columns nb reads the rows of its own head -- so a tile costs the (H2 / 256) (H / 32) stages of the single-head tail, not
// heads times as many.  Every z[n] is still ONE fmaf chain over its block's k ascending on v_mfma_f32_16x16x4_f32: the chain of
// query_tail_kernel on the block-expanded W1 [H2][heads H] (zeros elsewhere: a product with 0 changes no finite partial sum).
__host__ __device__ constexpr size_t mhgat_tail_lds_floats(int H2, int C, int heads) {
    return (size_t)kTailQ * (H2 + 4) + (size_t)kTailCols * kTailLd + (size_t)heads * kTailQ * kTailLd + (size_t)kTailQ * C;
}
static_assert(mhgat_tail_lds_floats(512, 48, 8) * sizeof(float) <= kTailLdsMax, "the widest model's tail must fit LDS");

__global__ __launch_bounds__(256) void mhgat_tail_kernel(const float *__restrict__ G, int64_t ldg, int32_t Q, const float *__restrict__ W1,
                                                         const float *__restrict__ b1, const float *__restrict__ Wl,
                                                         const float *__restrict__ bl, int32_t H, int32_t H2, int32_t heads, int32_t C,
                                                         float *__restrict__ out, int64_t ldo, int32_t log_softmax) {
    extern __shared__ float smem[];
    const int zld = H2 + 4;
    float *zs = smem;
    float *Ws = zs + (size_t)kTailQ * zld;
    float *Gs = Ws + kTailCols * kTailLd;                // [heads of the pass][16][kTailLd]
    float *lg = Gs + (size_t)heads * kTailQ * kTailLd;
    const int q0 = blockIdx.x * kTailQ;
    const int nq = min(kTailQ, Q - q0);
    const int C1 = H2 / heads;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;

    for (int n0 = 0; n0 < H2; n0 += kTailCols) {
        const int ncols = min(kTailCols, H2 - n0);  // a multiple of 16
        const int g0 = n0 / C1, ng = (n0 + ncols - 1) / C1 - g0 + 1;  // the heads of this pass
        f32x4 acc[4];
        int arow[4];  // the staged row of G that block u's lanes read: its head's slab, row r16
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int nb = (w * 4 + u) * 16;
            arow[u] = (((nb < ncols ? (n0 + nb) / C1 : g0) - g0) * kTailQ + r16) * kTailLd;
        }
        for (int k0 = 0; k0 < H; k0 += kTailKS) {
            const int k4 = min(kTailKS, H - k0) >> 2;  // float4 per staged row (H % 4 == 0)
            __syncthreads();                           // the previous stage (and a previous tile's zs) has been consumed
            for (int idx = tid; idx < ncols * k4; idx += 256) {
                const int n = idx / k4, kk = idx - n * k4;
                *reinterpret_cast<float4 *>(Ws + n * kTailLd + kk * 4) =
                    *reinterpret_cast<const float4 *>(W1 + (int64_t)(n0 + n) * H + k0 + kk * 4);
            }
            for (int idx = tid; idx < ng * kTailQ * k4; idx += 256) {
                const int gr = idx / k4, kk = idx - gr * k4, g = gr / kTailQ, r = gr - g * kTailQ;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);  // rows past Q: computed as zeros, never stored
                if (r < nq) v = *reinterpret_cast<const float4 *>(G + (int64_t)(q0 + r) * ldg + (int64_t)(g0 + g) * H + k0 + kk * 4);
                *reinterpret_cast<float4 *>(Gs + gr * kTailLd + kk * 4) = v;
            }
            __syncthreads();
            for (int kk = 0; kk < k4; ++kk) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int nb = (w * 4 + u) * 16;
                    if (nb < ncols) {  // wave-uniform
                        const float a = Gs[arow[u] + kk * 4 + kq];
                        const float b = Ws[(nb + r16) * kTailLd + kk * 4 + kq];
                        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[u], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int nb = (w * 4 + u) * 16;
            if (nb < ncols) {
                const int n = n0 + nb + r16;
                const float bias = b1 ? b1[n] : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) zs[(kq * 4 + r) * zld + n] = elu1(acc[u][r] + bias);
            }
        }
    }
    __syncthreads();

    tail_head(zs, zld, H2, Wl, bl, C, lg, out, ldo, q0, nq, log_softmax);
}

// ---- an MLP over both hops (two GINConv layers, nn = Linear, ReLU, Linear, ReLU) ----
//   T     = X W0a^T                                                                  [n_table x Ha]   t(r) = xrow ? xrow[r] : r
//   a_r   = ReLU(sum_{k in row r} val[k] T[t(col[k])] + (1 + eps0) T[t(r)] + b0a)    [Ha]
//   h_r   = ReLU(W0b a_r + b0b)                                                      [Hb]: a dense product per one-hop row
//   s_q   = sum_{j in row q} val[j] h_{col[j]} + (1 + eps1) h_q                      [Hb] -> G[i];  gin_query_tail_kernel finishes.
// Only W0a commutes with the aggregation; W0b sits behind a ReLU, so every one-hop row of the query takes the product itself.
// Operation order (tests/gin_query_reference.py mirrors it), with o0 = 1.0f + eps0[0] and o1 = 1.0f + eps1[0] formed once in fp32:
//   row r    a = 0; a = fmaf(val[e'], T[t(col[e'])][c], a) over row r's entries in CSR order; a = fmaf(o0, T[t(r)][c], a);
//            a = a + b0a[c] (b0a == NULL: this add is absent); a_r[c] = max(a, 0).
//   product  h_r[n] = max((fmaf chain over k ascending of a_r[k] W0b[n][k], from 0) + b0b[n], 0)   (v_mfma_f32_16x16x4_f32: exact fp32,
//            bit-equal to that chain; b0b == NULL adds 0.0f).
//   query q  the work items are q's deg(q) entries in CSR order followed by q itself, taken in tiles of 16; item i has weight
//            w_i = val[e_i], the query's own item o1.  Item i belongs to fold group (i % 16) / 4.  A group folds its items in ascending i,
//            across tiles: P_g = fmaf(w_i, h_i, P_g) from 0; the rows past the last item of a partial tile are not folded.
//            s = ((P_0 + P_1) + P_2) + P_3 (a group without items holds 0).  A query without entries gives fmaf(o1, h_q, 0).
// The bits depend on no split: a row of a_r is formed by one wave, whichever; a column of h and its fold live in one lane per group.
constexpr int kGinRows = 16;  // items per tile: one MFMA tile of rows

__host__ __device__ constexpr size_t gin_hops_lds_floats(int Ha) { return (size_t)kGinRows * (Ha + 4) + (size_t)kTailCols * kTailLd; }
static_assert(2 * gin_hops_lds_floats(512) * sizeof(float) <= kTailLdsMax, "two workgroups per CU at Ha = 512");

// One wave: row r of a (before the dense product) into a[].  Tc[s]: the lane's column of slot s in T (a lane past Ha reads column 0
// and is never stored).  sage_row's scheme: the root float4 is requested first, the entries are fetched 64 at a time and broadcast
// by v_readlane, four table rows in flight.
template <int NS>
__device__ __forceinline__ void gin_row(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
                                        const float *const (&Tc)[NS], int64_t ldt, const int32_t *__restrict__ xrow, float o0, bool has_bias,
                                        const float4 (&bias)[NS], int r, int lane, float4 (&a)[NS]) {
    const int n0 = __builtin_amdgcn_readfirstlane(rowptr[r]), n1 = __builtin_amdgcn_readfirstlane(rowptr[r + 1]);
    const int tr = __builtin_amdgcn_readfirstlane(xrow ? xrow[r] : r);
    float4 root[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        root[s] = *reinterpret_cast<const float4 *>(Tc[s] + (int64_t)tr * ldt);
        a[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int base = n0; base < n1; base += 64) {
        const int cnt = min(64, n1 - base);
        int my = 0, mv = 0;
        if (lane < cnt) {
            const int cc = col[base + lane];
            my = xrow ? xrow[cc] : cc;
            mv = __float_as_int(val[base + lane]);
        }
        for (int k = 0; k < cnt; k += 4) {
            float4 t[4][NS];
            float wv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // always four loads: a missing one re-reads entry k and is not folded
                const int idx = k + u < cnt ? k + u : k;
                const int node = __builtin_amdgcn_readlane(my, idx);
                wv[u] = __int_as_float(__builtin_amdgcn_readlane(mv, idx));
#pragma unroll
                for (int s = 0; s < NS; ++s) t[u][s] = *reinterpret_cast<const float4 *>(Tc[s] + (int64_t)node * ldt);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (k + u < cnt) {
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        a[s].x = fmaf(wv[u], t[u][s].x, a[s].x);
                        a[s].y = fmaf(wv[u], t[u][s].y, a[s].y);
                        a[s].z = fmaf(wv[u], t[u][s].z, a[s].z);
                        a[s].w = fmaf(wv[u], t[u][s].w, a[s].w);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        a[s].x = fmaf(o0, root[s].x, a[s].x);
        a[s].y = fmaf(o0, root[s].y, a[s].y);
        a[s].z = fmaf(o0, root[s].z, a[s].z);
        a[s].w = fmaf(o0, root[s].w, a[s].w);
        if (has_bias) {  // wave-uniform
            a[s].x += bias[s].x; a[s].y += bias[s].y; a[s].z += bias[s].z; a[s].w += bias[s].w;
        }
        a[s] = make_float4(fmaxf(a[s].x, 0.f), fmaxf(a[s].y, 0.f), fmaxf(a[s].z, 0.f), fmaxf(a[s].w, 0.f));
    }
}

// acc += A W^T for one pass of up to 256 columns n0 .. n0 + ncols of W [N x K] (row-major, contiguous), the tile's 16 rows of A in
// LDS (row stride lda): W staged through LDS in k-stages of 32 with query_tail_kernel's lane layout (A: lane l holds A[l & 15][k = l >> 4],
// B: W[n = l & 15][k = l >> 4], C/D: column l & 15, rows 4 (l >> 4) + r).  The barrier in front of every stage also orders A's writers.
__device__ __forceinline__ void lds_tile_product(const float *As, int lda, const float *__restrict__ W, int K, int n0, int ncols, float *Ws,
                                                 f32x4 (&acc)[4]) {
    const int tid = threadIdx.x, w = tid >> 6, r16 = tid & 15, kq = (tid & 63) >> 4;
    for (int k0 = 0; k0 < K; k0 += kTailKS) {
        const int k4 = min(kTailKS, K - k0) >> 2;  // float4 per staged row (K % 4 == 0)
        __syncthreads();                           // the previous stage has been consumed; A is complete
        for (int idx = tid; idx < ncols * k4; idx += 256) {
            const int n = idx / k4, kk = idx - n * k4;
            *reinterpret_cast<float4 *>(Ws + n * kTailLd + kk * 4) = *reinterpret_cast<const float4 *>(W + (int64_t)(n0 + n) * K + k0 + kk * 4);
        }
        __syncthreads();
        for (int kk = 0; kk < k4; ++kk) {
            const float a = As[r16 * lda + k0 + kk * 4 + kq];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int nb = (w * 4 + u) * 16;
                if (nb < ncols) {  // wave-uniform
                    const float b = Ws[(nb + r16) * kTailLd + kk * 4 + kq];
                    acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[u], 0, 0, 0);
                }
            }
        }
    }
}

// One workgroup of four waves per query.  Per tile of 16 items the waves form the rows a_r into LDS (item i by wave i % 4, whole rows
// of Ha <= 256 NS columns), then all four multiply the tile by W0b^T (NP passes of 256 columns of Hb) and fold the rows of h into the
// running sums: a lane keeps one column of each of its accumulators for its fold group l >> 4.  The groups meet by v shuffles at the end.
template <int NS, int NP>
__global__ __launch_bounds__(256) void gin_query_hops_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                             const float *__restrict__ val, const float *__restrict__ T, int64_t ldt,
                                                             const int32_t *__restrict__ xrow, const float *__restrict__ b0a,
                                                             const float *__restrict__ eps0, const float *__restrict__ W0b,
                                                             const float *__restrict__ b0b, const float *__restrict__ eps1,
                                                             const int64_t *__restrict__ rows, int32_t Ha, int32_t Hb, float *__restrict__ G,
                                                             int64_t ldg) {
    extern __shared__ float smem[];
    const int ald = Ha + 4;
    float *As = smem;
    float *Ws = As + (size_t)kGinRows * ald;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, kq = lane >> 4;
    const int qi = blockIdx.x;
    const int q = __builtin_amdgcn_readfirstlane((int)rows[qi]);
    const int e0 = __builtin_amdgcn_readfirstlane(rowptr[q]), e1 = __builtin_amdgcn_readfirstlane(rowptr[q + 1]);
    const int deg = e1 - e0, items = deg + 1;
    const float o0 = 1.0f + eps0[0], o1 = 1.0f + eps1[0];
    const bool has_bias = b0a != nullptr;
    const float *Tc[NS];
    float4 bias[NS];
    bool live[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = s * 256 + lane * 4;
        live[s] = c < Ha;  // Ha % 4 == 0: a live lane owns four whole columns
        Tc[s] = T + (live[s] ? c : 0);
        bias[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (has_bias && live[s]) bias[s] = make_float4(b0a[c], b0a[c + 1], b0a[c + 2], b0a[c + 3]);
    }
    float P[NP][4];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int u = 0; u < 4; ++u) P[p][u] = 0.f;

    for (int t0 = 0; t0 < items; t0 += kGinRows) {
        __syncthreads();  // the previous tile's product has read As
        for (int i = w; i < kGinRows; i += 4) {
            const int item = t0 + i;
            float4 a[NS];
            if (item < items) {  // wave-uniform
                const int r = item < deg ? __builtin_amdgcn_readfirstlane(col[e0 + item]) : q;
                gin_row<NS>(rowptr, col, val, Tc, ldt, xrow, o0, has_bias, bias, r, lane, a);
            } else {  // a defined row for the MFMA; its h is never folded
#pragma unroll
                for (int s = 0; s < NS; ++s) a[s] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (live[s]) *reinterpret_cast<float4 *>(As + i * ald + s * 256 + lane * 4) = a[s];
        }
        float wt[4];
        bool on[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // the lane's four rows of the tile
            const int item = t0 + kq * 4 + r;
            on[r] = item < items;
            wt[r] = item < deg ? val[e0 + item] : o1;
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int n0 = p * kTailCols;
            const int ncols = min(kTailCols, Hb - n0);  // a multiple of 16; NP > 1 only when Hb > 256
            f32x4 acc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            lds_tile_product(As, ald, W0b, Ha, n0, ncols, Ws, acc);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int nb = (w * 4 + u) * 16;
                if (nb < ncols) {
                    const float b = b0b ? b0b[n0 + nb + r16] : 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (on[r]) P[p][u] = fmaf(wt[r], fmaxf(acc[u][r] + b, 0.f), P[p][u]);
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int n0 = p * kTailCols;
        const int ncols = min(kTailCols, Hb - n0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int nb = (w * 4 + u) * 16;
            if (nb < ncols) {  // wave-uniform: all 64 lanes take part in the shuffles
                const float v = P[p][u];
                const float v1 = __shfl(v, r16 + 16, 64), v2 = __shfl(v, r16 + 32, 64), v3 = __shfl(v, r16 + 48, 64);
                if (kq == 0) G[(int64_t)qi * ldg + n0 + nb + r16] = ((v + v1) + v2) + v3;
            }
        }
    }
}

// ---- the GIN tail: two dense stages, then the head ----
__host__ __device__ constexpr size_t gin_tail_lds_floats(int H2a, int H2b, int C) {
    return (size_t)kTailQ * (H2a + 4) + (size_t)kTailQ * (H2b + 4) + (size_t)kTailCols * kTailLd + (size_t)kTailQ * kTailLd + (size_t)kTailQ * C;
}
static_assert(gin_tail_lds_floats(512, 512, 48) * sizeof(float) <= kTailLdsMax, "the default model's tail must fit LDS");

// zs[r][n] = max(A W^T + b, 0) for the tile's 16 rows of A in LDS and every column n < N, in passes of 256 columns.
__device__ __forceinline__ void relu_stage(const float *As, int lda, const float *__restrict__ W, const float *__restrict__ b, int K, int N,
                                           float *Ws, float *zs, int zld) {
    const int w = threadIdx.x >> 6, r16 = threadIdx.x & 15, kq = (threadIdx.x & 63) >> 4;
    for (int n0 = 0; n0 < N; n0 += kTailCols) {
        const int ncols = min(kTailCols, N - n0);  // a multiple of 16
        f32x4 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        lds_tile_product(As, lda, W, K, n0, ncols, Ws, acc);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int nb = (w * 4 + u) * 16;
            if (nb < ncols) {
                const int n = n0 + nb + r16;
                const float bias = b ? b[n] : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) zs[(kq * 4 + r) * zld + n] = fmaxf(acc[u][r] + bias, 0.f);
            }
        }
    }
}

// One workgroup per tile of up to 16 queries: z1 = ReLU(S W1a^T + b1a) with the tile's rows of S = G staged through LDS beside W1a
// (tail_tile_z<true>: query_tail_kernel's first product behind a ReLU), z2 = ReLU(z1 W1b^T + b1b) from z1 in LDS, both on
// v_mfma_f32_16x16x4_f32, then tail_head on z2.
__global__ __launch_bounds__(256) void gin_query_tail_kernel(const float *__restrict__ G, int64_t ldg, int32_t Q, const float *__restrict__ W1a,
                                                             const float *__restrict__ b1a, const float *__restrict__ W1b,
                                                             const float *__restrict__ b1b, const float *__restrict__ Wl,
                                                             const float *__restrict__ bl, int32_t K, int32_t H2a, int32_t H2b, int32_t C,
                                                             float *__restrict__ out, int64_t ldo, int32_t log_softmax) {
    extern __shared__ float smem[];
    const int z1ld = H2a + 4, z2ld = H2b + 4;
    float *z1 = smem;
    float *z2 = z1 + (size_t)kTailQ * z1ld;
    float *Ws = z2 + (size_t)kTailQ * z2ld;
    float *Gs = Ws + kTailCols * kTailLd;
    float *lg = Gs + kTailQ * kTailLd;
    const int q0 = blockIdx.x * kTailQ;
    const int nq = min(kTailQ, Q - q0);

    tail_tile_z<true>(G, ldg, q0, nq, W1a, b1a, K, H2a, z1, z1ld, Ws, Gs);
    relu_stage(z1, z1ld, W1b, b1b, H2a, H2b, Ws, z2, z2ld);  // its first barrier orders z1's writers
    __syncthreads();
    tail_head(z2, z2ld, H2b, Wl, bl, C, lg, out, ldo, q0, nq, log_softmax);
}

// ---- graph queries (two GCNConv layers, a pool over a graph's rows, the head) ----
// A graph is a contiguous row range [r0, r1) of a block-diagonal view, so its layer-0 rows fit in LDS: each is formed ONCE per
// (graph, slab) -- the per-row gather above forms row j once per entry that reaches it -- and layer 1 reads them from there.
//   h_r   = ELU(sum_{e' in row r} val[e'] T[t(col[e'])] + b0)          r in [r0, r1)                     graph_query_hops_kernel
//   g_r   = sum_{e in row r} val[e] h_{col[e]}                          r among the graph's pooled rows
//   z_r   = ELU(W1 g_r + b1);  p = max_r z_r | mean_r z_r;  out = Wl p + bl  (softmax)                   graph_query_tail_kernel
// Operation order (tests/graph_query_reference.py mirrors it):
//   hops  phase 1: a = 0; a = fmaf(val[e'], T[t(col[e'])][c], a) over row r's entries in CSR order (gcn_row); h_r[c] = ELU(a + b0[c]);
//         a row without entries: ELU(b0).  phase 2: g = 0; g = fmaf(val[e], h_{col[e]}[c], g) over the pooled row's entries in CSR
//         order, ONE chain (no wave partials); a pooled row without entries gives zeros.
//   tail  z_r[n] as query_tail_kernel's (tail_tile_z, tiles of 16 rows of the segment); the pool folds the segment's rows ascending,
//         live rows only: max p[n] = z_first[n], then p[n] = fmaxf(p[n], z_r[n]); mean s[n] = s[n] + z_r[n] from 0, p[n] = s[n] / (float)cnt;
//         an empty segment: p = 0.  logit[c] = (fmaf chain over h ascending of p[h] Wl[c][h], from 0) + bl[c]; softmax: m = max_c logit,
//         e_c = expf(logit[c] - m), s = sum_c e_c ascending c from 0, out[c] = e_c / s.

// One workgroup of four waves per (graph, 256-column slab), the slab fastest.  The graph's rows are dealt round-robin to the waves,
// which form them (gcn_row, + b0, ELU) into the LDS window hs [r1 - r0][min(H, 256)]: a wave writes and later reads 64 consecutive
// float4, every bank once.  After the barrier the graph's pooled rows are dealt round-robin to the waves; a wave fetches the row's
// entries 64 at a time and broadcasts (window row, value) by v_readlane.
__global__ __launch_bounds__(256) void graph_query_hops_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                               const float *__restrict__ val, const float *__restrict__ T, int64_t ldt,
                                                               const int32_t *__restrict__ xrow, const float *__restrict__ b0,
                                                               const int64_t *__restrict__ seg, const int64_t *__restrict__ prow,
                                                               const int64_t *__restrict__ pptr, int32_t H, int32_t max_rows,
                                                               float *__restrict__ G, int64_t ldg, int32_t n_slabs) {
    extern __shared__ float4 hs[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gi = blockIdx.x / n_slabs, c0 = (blockIdx.x % n_slabs) * 256;
    const int r0 = __builtin_amdgcn_readfirstlane((int)seg[2 * (int64_t)gi]), r1 = __builtin_amdgcn_readfirstlane((int)seg[2 * (int64_t)gi + 1]);
    if (r1 - r0 > max_rows) return;  // workgroup-uniform: the window was sized for max_rows
    const int w4 = min(H, 256) >> 2;  // float4 per window row
    const int c = c0 + lane * 4;
    const bool live = c < H;  // H % 4 == 0: a live lane owns four whole columns
    const float *Tc = T + (live ? c : 0);
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b0 && live) bias = make_float4(b0[c], b0[c + 1], b0[c + 2], b0[c + 3]);
    for (int r = r0 + w; r < r1; r += kGatherWaves) {
        const float4 a = gcn_row(rowptr, col, val, Tc, ldt, xrow, r, lane);
        if (live) hs[(r - r0) * w4 + lane] = make_float4(elu1(a.x + bias.x), elu1(a.y + bias.y), elu1(a.z + bias.z), elu1(a.w + bias.w));
    }
    __syncthreads();
    const int64_t p1 = pptr[gi + 1];
    for (int64_t j = pptr[gi] + w; j < p1; j += kGatherWaves) {
        const int r = __builtin_amdgcn_readfirstlane((int)prow[j]);
        const int n0 = __builtin_amdgcn_readfirstlane(rowptr[r]), n1 = __builtin_amdgcn_readfirstlane(rowptr[r + 1]);
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int base = n0; base < n1; base += 64) {
            const int cnt = min(64, n1 - base);
            int my = 0, mv = 0;
            if (lane < cnt) {
                my = col[base + lane] - r0;
                mv = __float_as_int(val[base + lane]);
            }
            for (int k = 0; k < cnt; ++k) {
                const int node = __builtin_amdgcn_readlane(my, k);
                const float wv = __int_as_float(__builtin_amdgcn_readlane(mv, k));
                if (live) {
                    const float4 h = hs[node * w4 + lane];
                    g.x = fmaf(wv, h.x, g.x);
                    g.y = fmaf(wv, h.y, g.y);
                    g.z = fmaf(wv, h.z, g.z);
                    g.w = fmaf(wv, h.w, g.w);
                }
            }
        }
        if (live) *reinterpret_cast<float4 *>(G + j * ldg + c) = g;
    }
}

__host__ __device__ constexpr size_t graph_tail_lds_floats(int H2, int C) {
    return (size_t)kTailQ * (H2 + 4) + (size_t)kTailCols * kTailLd + (size_t)kTailQ * kTailLd + (size_t)H2 + (size_t)C;
}
static_assert(graph_tail_lds_floats(512, 48) * sizeof(float) <= kTailLdsMax, "the default model's graph tail must fit LDS");

// The pool over a tile's z [16][zld] in LDS (written before a barrier): thread t folds the tile's live rows, ascending, into ps[n] for
// its columns n = t, t + 256, ...  first: the segment's first tile (the maximum starts from its first row).
__device__ __forceinline__ void graph_pool_fold(const float *zs, int zld, int32_t H2, int nq, bool first, int32_t pool, float *ps) {
    for (int n = threadIdx.x; n < H2; n += 256) {
        float p = ps[n];
        int r = 0;
        if (pool == 0 && first) {  // the maximum starts from the segment's first row
            p = zs[n];
            r = 1;
        }
        for (; r < nq; ++r) {  // live rows only: a padded row holds act(b1)
            const float z = zs[r * zld + n];
            p = pool == 0 ? fmaxf(p, z) : p + z;
        }
        ps[n] = p;
    }
}

// The mean's division, the head's chain over ps (one thread per class) and the softmax of one graph; lg [C] in LDS, out: the graph's row.
__device__ __forceinline__ void graph_pool_head(float *ps, int32_t H2, int64_t cnt_rows, int32_t pool, const float *__restrict__ Wl,
                                                const float *__restrict__ bl, int32_t C, int32_t softmax, float *lg, float *__restrict__ out) {
    const int tid = threadIdx.x;
    if (pool != 0 && cnt_rows > 0) {
        const float cnt = (float)cnt_rows;
        for (int n = tid; n < H2; n += 256) ps[n] = ps[n] / cnt;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const float *wl = Wl + (int64_t)c * H2;
        float s = 0.f;
        for (int h = 0; h < H2; h += 4) {
            const float4 wv = *reinterpret_cast<const float4 *>(wl + h);
            const float4 pv = *reinterpret_cast<const float4 *>(ps + h);
            s = fmaf(pv.x, wv.x, s);
            s = fmaf(pv.y, wv.y, s);
            s = fmaf(pv.z, wv.z, s);
            s = fmaf(pv.w, wv.w, s);
        }
        lg[c] = bl ? s + bl[c] : s;
    }
    __syncthreads();
    if (softmax) {
        if (tid == 0) {
            float m = lg[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, lg[c]);
            float s = 0.f;
            for (int c = 0; c < C; ++c) {
                const float e = expf(lg[c] - m);
                lg[c] = e;
                s += e;
            }
            for (int c = 0; c < C; ++c) lg[c] = lg[c] / s;
        }
        __syncthreads();
    }
    for (int c = tid; c < C; c += 256) out[c] = lg[c];
}

// One workgroup per graph: its segment of G in tiles of 16 rows through tail_tile_z; after each tile thread t folds the tile's live
// rows into ps[n] for its columns n = t, t + 256, ... (the same thread owns a column from the first tile to the division, so ps
// needs no barrier of its own before the head).  One thread per class then runs the head's chain over ps.
__global__ __launch_bounds__(256) void graph_query_tail_kernel(const float *__restrict__ G, int64_t ldg, const int64_t *__restrict__ pptr,
                                                               const float *__restrict__ W1, const float *__restrict__ b1,
                                                               const float *__restrict__ Wl, const float *__restrict__ bl, int32_t H,
                                                               int32_t H2, int32_t C, int32_t pool, int32_t softmax,
                                                               float *__restrict__ out, int64_t ldo) {
    extern __shared__ float smem[];
    const int zld = H2 + 4;
    float *zs = smem;
    float *Ws = zs + (size_t)kTailQ * zld;
    float *Gs = Ws + kTailCols * kTailLd;
    float *ps = Gs + kTailQ * kTailLd;  // 16-byte aligned: every part in front of it is a multiple of four floats
    float *lg = ps + H2;
    const int tid = threadIdx.x;
    const int64_t s0 = pptr[blockIdx.x], s1 = pptr[blockIdx.x + 1];
    for (int n = tid; n < H2; n += 256) ps[n] = 0.f;
    for (int64_t t0 = s0; t0 < s1; t0 += kTailQ) {
        const int nq = (int)min((int64_t)kTailQ, s1 - t0);
        tail_tile_z<false>(G, ldg, t0, nq, W1, b1, H, H2, zs, zld, Ws, Gs);
        __syncthreads();
        graph_pool_fold(zs, zld, H2, nq, t0 == s0, pool, ps);
    }
    graph_pool_head(ps, H2, s1 - s0, pool, Wl, bl, C, softmax, lg, out + (int64_t)blockIdx.x * ldo);
}

// ---- graph queries for two GINConv layers (nn = Linear, ReLU, Linear, ReLU) ----
// gin_query_hops_kernel on every pooled row of a graph forms h_c once per entry that reaches row c plus once for c itself: sum_r (deg(r) + 1)
// dense row-products of Hb x Ha.  Here every row of the graph takes the product ONCE per (graph, slab) and stays in LDS:
//   a_r   = ReLU(sum_{k in row r} val[k] T[t(col[k])] + (1 + eps0) T[t(r)] + b0a)      EVERY r in [r0, r1)      gin_graph_query_hops_kernel
//   h_r   = ReLU(W0b a_r + b0b)                                                        EVERY r in [r0, r1), in the LDS window
//   s_r   = sum_{e in row r} val[e] h_{col[e]} + (1 + eps1) h_r                        r among the graph's pooled rows -> G
//   z_r   = ReLU(W1b ReLU(W1a s_r + b1a) + b1b);  p = max_r z_r | mean_r z_r;  out = Wl p + bl  (softmax)      gin_graph_query_tail_kernel
// Operation order (tests/gin_graph_query_reference.py mirrors it), with o0 = 1.0f + eps0[0] and o1 = 1.0f + eps1[0] formed once in fp32:
//   hops  phase 1: a_r and h_r exactly as gin_query_hops_kernel's "row r" and "product" (gin_row, lds_tile_product: the same bits; a slab
//         takes its own 256 columns of W0b, every slab forms the same a_r).  phase 2: s = 0; s = fmaf(val[e], h_{col[e]}[c], s) over the
//         pooled row's entries in CSR order, ONE chain (no fold groups: the sum differs from gin_query_hops_kernel's s_q only by that
//         order); then s = fmaf(o1, h_r[c], s).  A pooled row without entries gives fmaf(o1, h_r, 0).
//   tail  z1 = ReLU(fmaf chain over k ascending of G[r][k] W1a[n][k], from 0, + b1a[n]), z2 = ReLU(the same chain of z1 and W1b + b1b[n])
//         as gin_query_tail_kernel's, in tiles of 16 rows of the segment; the pool, the head and the softmax as graph_query_tail_kernel's
//         (graph_pool_fold, graph_pool_head: live rows only, ascending; an empty segment: p = 0).
constexpr int kGinWinPad = 4;  // the window's row stride is min(Hb, 256) + 4 floats: see gin_graph_query_hops_kernel

__host__ __device__ constexpr size_t gin_graph_hops_lds_floats(int max_rows, int Ha, int Hb) {
    return gin_hops_lds_floats(Ha) + (size_t)max_rows * ((Hb < kTailCols ? Hb : kTailCols) + kGinWinPad);
}

// One workgroup of four waves per (graph, 256-column slab of Hb), the slab fastest.  Phase 1, per tile of 16 rows of the graph: the
// waves form a_r into the A stage (row i of the tile by wave i % 4, all Ha columns in NS slots; rows past r1 are zeros), all four
// multiply the tile by the slab's rows of W0b (lds_tile_product) and store ReLU(. + b0b) for the tile's live rows into the window
// hs [r1 - r0][wld].  wld = min(Hb, 256) + 4: the MFMA result gives lane l rows 4 (l >> 4) + r of column l & 15, so one store
// instruction writes 16 consecutive columns of four rows that lie 4 wld floats apart; ds_write_b32 banks are (address / 4) % 32
// within a half wave (rows 4 kq + r for kq = 0, 1 or 2, 3), and 4 wld = 16 (mod 32) puts the half's two rows on disjoint halves of
// the banks (a stride of min(Hb, 256) itself would put both on the same 16: 2-way).  wld stays a multiple of 4, so phase 2's rows
// are 16-byte aligned and a wave reads 64 consecutive float4 of one row, as graph_query_hops_kernel does.  One barrier, then phase 2:
// the graph's pooled rows dealt round-robin to the waves, entries fetched 64 at a time, (window row, value) broadcast by v_readlane.
template <int NS>
__global__ __launch_bounds__(256) void gin_graph_query_hops_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                   const float *__restrict__ val, const float *__restrict__ T, int64_t ldt,
                                                                   const int32_t *__restrict__ xrow, const float *__restrict__ b0a,
                                                                   const float *__restrict__ eps0, const float *__restrict__ W0b,
                                                                   const float *__restrict__ b0b, const float *__restrict__ eps1,
                                                                   const int64_t *__restrict__ seg, const int64_t *__restrict__ prow,
                                                                   const int64_t *__restrict__ pptr, int32_t Ha, int32_t Hb, int32_t max_rows,
                                                                   float *__restrict__ G, int64_t ldg, int32_t n_slabs) {
    extern __shared__ float smem[];
    const int ald = Ha + 4, wld = min(Hb, kTailCols) + kGinWinPad;
    float *As = smem;
    float *Ws = As + (size_t)kGinRows * ald;
    float *hs = Ws + kTailCols * kTailLd;  // 16-byte aligned: both parts in front of it are multiples of four floats
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, kq = lane >> 4;
    const int gi = blockIdx.x / n_slabs, c0 = (blockIdx.x % n_slabs) * kTailCols;
    const int r0 = __builtin_amdgcn_readfirstlane((int)seg[2 * (int64_t)gi]), r1 = __builtin_amdgcn_readfirstlane((int)seg[2 * (int64_t)gi + 1]);
    if (r1 - r0 > max_rows) return;  // workgroup-uniform: the window was sized for max_rows
    const int ncols = min(kTailCols, Hb - c0);  // the slab's columns: a multiple of 16
    const float o0 = 1.0f + eps0[0], o1 = 1.0f + eps1[0];
    const bool has_bias = b0a != nullptr;
    const float *Tc[NS];
    float4 bias[NS];
    bool live[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = s * 256 + lane * 4;
        live[s] = c < Ha;  // Ha % 4 == 0: a live lane owns four whole columns
        Tc[s] = T + (live[s] ? c : 0);
        bias[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (has_bias && live[s]) bias[s] = make_float4(b0a[c], b0a[c + 1], b0a[c + 2], b0a[c + 3]);
    }
    for (int t0 = r0; t0 < r1; t0 += kGinRows) {
        __syncthreads();  // the previous tile's product has read As
        for (int i = w; i < kGinRows; i += 4) {
            float4 a[NS];
            if (t0 + i < r1) {  // wave-uniform
                gin_row<NS>(rowptr, col, val, Tc, ldt, xrow, o0, has_bias, bias, t0 + i, lane, a);
            } else {  // a defined row for the MFMA; its h is never stored
#pragma unroll
                for (int s = 0; s < NS; ++s) a[s] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (live[s]) *reinterpret_cast<float4 *>(As + i * ald + s * 256 + lane * 4) = a[s];
        }
        f32x4 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        lds_tile_product(As, ald, W0b, Ha, c0, ncols, Ws, acc);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int nb = (w * 4 + u) * 16;
            if (nb < ncols) {
                const float b = b0b ? b0b[c0 + nb + r16] : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = t0 + kq * 4 + r;
                    if (row < r1) hs[(row - r0) * wld + nb + r16] = fmaxf(acc[u][r] + b, 0.f);
                }
            }
        }
    }
    __syncthreads();
    const bool on = lane * 4 < ncols;  // ncols % 4 == 0: a live lane owns four whole columns of the slab
    const float *hc = hs + (on ? lane * 4 : 0);
    const int64_t p1 = pptr[gi + 1];
    for (int64_t j = pptr[gi] + w; j < p1; j += kGatherWaves) {
        const int r = __builtin_amdgcn_readfirstlane((int)prow[j]);
        const int n0 = __builtin_amdgcn_readfirstlane(rowptr[r]), n1 = __builtin_amdgcn_readfirstlane(rowptr[r + 1]);
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int base = n0; base < n1; base += 64) {
            const int cnt = min(64, n1 - base);
            int my = 0, mv = 0;
            if (lane < cnt) {
                my = col[base + lane] - r0;
                mv = __float_as_int(val[base + lane]);
            }
            for (int k = 0; k < cnt; ++k) {
                const int node = __builtin_amdgcn_readlane(my, k);
                const float wv = __int_as_float(__builtin_amdgcn_readlane(mv, k));
                if (on) {
                    const float4 h = *reinterpret_cast<const float4 *>(hc + node * wld);
                    g.x = fmaf(wv, h.x, g.x);
                    g.y = fmaf(wv, h.y, g.y);
                    g.z = fmaf(wv, h.z, g.z);
                    g.w = fmaf(wv, h.w, g.w);
                }
            }
        }
        if (on) {
            const float4 h = *reinterpret_cast<const float4 *>(hc + (r - r0) * wld);
            g.x = fmaf(o1, h.x, g.x);
            g.y = fmaf(o1, h.y, g.y);
            g.z = fmaf(o1, h.z, g.z);
            g.w = fmaf(o1, h.w, g.w);
            *reinterpret_cast<float4 *>(G + j * ldg + c0 + lane * 4) = g;
        }
    }
}

__host__ __device__ constexpr size_t gin_graph_tail_lds_floats(int H2a, int H2b, int C) {
    return gin_tail_lds_floats(H2a, H2b, C) + (size_t)H2b + (size_t)C;
}
static_assert(gin_graph_tail_lds_floats(512, 512, 48) * sizeof(float) <= kTailLdsMax, "the default model's graph tail must fit LDS");

// One workgroup per graph: its segment of G in tiles of 16 rows through gin_query_tail_kernel's two stages (tail_tile_z<true>, then
// relu_stage from z1 in LDS), the tile's live rows of z2 folded into ps as graph_query_tail_kernel does, then its head.  The LDS is
// gin_query_tail_kernel's (whose 16 C floats of logits are not used here) with ps [H2b] and lg [C] behind it.
__global__ __launch_bounds__(256) void gin_graph_query_tail_kernel(const float *__restrict__ G, int64_t ldg, const int64_t *__restrict__ pptr,
                                                                   const float *__restrict__ W1a, const float *__restrict__ b1a,
                                                                   const float *__restrict__ W1b, const float *__restrict__ b1b,
                                                                   const float *__restrict__ Wl, const float *__restrict__ bl, int32_t K,
                                                                   int32_t H2a, int32_t H2b, int32_t C, int32_t pool, int32_t softmax,
                                                                   float *__restrict__ out, int64_t ldo) {
    extern __shared__ float smem[];
    const int z1ld = H2a + 4, z2ld = H2b + 4;
    float *z1 = smem;
    float *z2 = z1 + (size_t)kTailQ * z1ld;
    float *Ws = z2 + (size_t)kTailQ * z2ld;
    float *Gs = Ws + kTailCols * kTailLd;
    float *ps = Gs + kTailQ * kTailLd;  // 16-byte aligned: every part in front of it is a multiple of four floats
    float *lg = ps + H2b;
    const int tid = threadIdx.x;
    const int64_t s0 = pptr[blockIdx.x], s1 = pptr[blockIdx.x + 1];
    for (int n = tid; n < H2b; n += 256) ps[n] = 0.f;
    for (int64_t t0 = s0; t0 < s1; t0 += kTailQ) {
        const int nq = (int)min((int64_t)kTailQ, s1 - t0);
        tail_tile_z<true>(G, ldg, t0, nq, W1a, b1a, K, H2a, z1, z1ld, Ws, Gs);  // its first barrier orders the previous tile's readers
        relu_stage(z1, z1ld, W1b, b1b, H2a, H2b, Ws, z2, z2ld);                 // its first barrier orders z1's writers
        __syncthreads();
        graph_pool_fold(z2, z2ld, H2b, nq, t0 == s0, pool, ps);
    }
    graph_pool_head(ps, H2b, s1 - s0, pool, Wl, bl, C, softmax, lg, out + (int64_t)blockIdx.x * ldo);
}

// ---- graph queries for two GATConv layers (heads = 1) ----
// gat_query_hops_kernel on every pooled row q of a graph re-forms the layer-0 row h_j of every neighbour j (a softmax over row j, a
// gather of deg(j) table rows) and its score dot u_s . h_j once per entry that reaches j, and h_q once per wave: sum_r (deg(r) + 1)
// layer-0 rows for a graph whose rows are all pooled.  Here every row of the graph is formed ONCE and stays in LDS with its two dots:
//   h_r   = ELU(sum_k alpha_rk T[t(k)] + b0),  alpha_r. = softmax_k lrelu(a0s[t(k)] + a0d[t(r)], slope0)   EVERY r in [r0, r1)
//   ds_r  = u_s . h_r,  dd_r = u_d . h_r                                                                    EVERY r in [r0, r1)
//   g_r   = sum_j beta_j h_j,  beta = softmax_j lrelu(ds_j + dd_r, slope1)      j in CSR row r, r among the graph's pooled rows -> G
// and graph_query_tail_kernel finishes (sum beta = 1, so W1 g_r + b1 is conv1's output: the node path's argument).
// Operation order (tests/gat_graph_query_reference.py mirrors it):
//   hops  phase 1: h_r exactly as gat_query_hops_kernel's "row r" (gat_row: the same bits); ds_r and dd_r as its "dot" (row_dot: per
//         lane d = fmaf(u[c], h[c], d) from 0 over its columns ascending, then the butterfly ^ 32 .. ^ 1).
//         phase 2, pooled row r with entries e in CSR order: f_e = lrelu(ds[col[e] - r0] + dd[r - r0], slope1), lrelu(s) = s > 0 ? s :
//         slope1 * s; m = max_e f_e; p_e = expf(f_e - m); from 0, over the entries in CSR order, ONE chain (no wave partials, no online
//         rescaling): l = l + p_e, g[c] = fmaf(p_e, h_{col[e]}[c], g[c]); G[j][c] = g[c] * (1 / l).  A pooled row without entries gives
//         zeros.  The sum differs from gat_query_hops_kernel's g_q only by that order (and by the one maximum in place of four running ones).
//   tail  graph_query_tail_kernel's, unchanged.

// One workgroup of four waves per graph, every wave on whole rows of H <= 256 NS columns (a score is a dot over all of H: no column
// slabs).  Phase 1: the graph's rows dealt round-robin to the waves, each h_r into the window hs [r1 - r0][H] (a wave writes and later
// reads 64 consecutive float4 per slot, every bank once), lane 0 stores the row's two dots into ds / dd [max_rows] behind the window.
// One barrier, then phase 2: the graph's pooled rows dealt round-robin to the waves; a wave fetches the row's entries 64 at a time --
// a lane reads ds of its entry (one scalar LDS read per lane) -- and broadcasts (window row, weight) by v_readlane.
template <int NS>
__global__ __launch_bounds__(256) void gat_graph_query_hops_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                   const float *__restrict__ T, int64_t ldt, const int32_t *__restrict__ xrow,
                                                                   const float *__restrict__ a_src0, const float *__restrict__ a_dst0,
                                                                   const float *__restrict__ b0, float slope0, const float *__restrict__ u_src,
                                                                   const float *__restrict__ u_dst, float slope1,
                                                                   const int64_t *__restrict__ seg, const int64_t *__restrict__ prow,
                                                                   const int64_t *__restrict__ pptr, int32_t H, int32_t max_rows,
                                                                   float *__restrict__ G, int64_t ldg) {
    extern __shared__ float4 hs4[];
    float *hs = reinterpret_cast<float *>(hs4);
    float *ds = hs + (size_t)max_rows * H;  // the window was sized for max_rows
    float *dd = ds + max_rows;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gi = blockIdx.x;
    const int r0 = __builtin_amdgcn_readfirstlane((int)seg[2 * (int64_t)gi]), r1 = __builtin_amdgcn_readfirstlane((int)seg[2 * (int64_t)gi + 1]);
    if (r1 - r0 > max_rows) return;  // workgroup-uniform
    bool live[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) live[s] = s * 256 + lane * 4 < H;  // H % 4 == 0: a live lane owns four whole columns
    {
        const float *Tc[NS];
        float4 bias[NS], us[NS], ud[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int c = s * 256 + lane * 4;
            Tc[s] = T + (live[s] ? c : 0);
            bias[s] = us[s] = ud[s] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live[s]) {
                if (b0) bias[s] = make_float4(b0[c], b0[c + 1], b0[c + 2], b0[c + 3]);
                us[s] = *reinterpret_cast<const float4 *>(u_src + c);
                ud[s] = *reinterpret_cast<const float4 *>(u_dst + c);
            }
        }
        for (int r = r0 + w; r < r1; r += kHopsWaves) {
            float4 h[NS];
            gat_row<NS>(rowptr, col, Tc, ldt, xrow, a_src0, a_dst0, slope0, bias, r, lane, h);
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (live[s]) *reinterpret_cast<float4 *>(hs + (size_t)(r - r0) * H + s * 256 + lane * 4) = h[s];
            const float s_r = row_dot<NS>(us, h), d_r = row_dot<NS>(ud, h);
            if (lane == 0) {
                ds[r - r0] = s_r;
                dd[r - r0] = d_r;
            }
        }
    }
    __syncthreads();
    const int64_t p1 = pptr[gi + 1];
    for (int64_t j = pptr[gi] + w; j < p1; j += kHopsWaves) {
        const int r = __builtin_amdgcn_readfirstlane((int)prow[j]);
        const int n0 = __builtin_amdgcn_readfirstlane(rowptr[r]), n1 = __builtin_amdgcn_readfirstlane(rowptr[r + 1]);
        const float dr = dd[r - r0];
        float mx = -INFINITY;
        for (int base = n0 + lane; base < n1; base += 64) mx = fmaxf(mx, lrelu1(ds[col[base] - r0] + dr, slope1));
        mx = wave_max(mx);
        float l = 0.f;
        float4 g[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) g[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int base = n0; base < n1; base += 64) {
            const int cnt = min(64, n1 - base);
            int my = 0, mv = 0;
            if (lane < cnt) {
                my = col[base + lane] - r0;
                mv = __float_as_int(expf(lrelu1(ds[my] + dr, slope1) - mx));
            }
            for (int k = 0; k < cnt; ++k) {
                const int node = __builtin_amdgcn_readlane(my, k);
                const float wv = __int_as_float(__builtin_amdgcn_readlane(mv, k));
                l += wv;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (live[s]) {
                        const float4 h = *reinterpret_cast<const float4 *>(hs + (size_t)node * H + s * 256 + lane * 4);
                        g[s].x = fmaf(wv, h.x, g[s].x);
                        g[s].y = fmaf(wv, h.y, g[s].y);
                        g[s].z = fmaf(wv, h.z, g[s].z);
                        g[s].w = fmaf(wv, h.w, g[s].w);
                    }
                }
            }
        }
        const float inv = n1 > n0 ? 1.f / l : 0.f;  // l >= 1: the row's largest score gives expf(0)
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (live[s])
                *reinterpret_cast<float4 *>(G + j * ldg + s * 256 + lane * 4) = make_float4(g[s].x * inv, g[s].y * inv, g[s].z * inv, g[s].w * inv);
    }
}

// ---- graph queries for two SAGEConv layers ----
// The view's MEAN CSR (no self loops, val = 1 / max(deg, 1)) and the table T = X [W_l0 ; W_r0]^T of sage_query_gather_kernel.  The
// per-row gather forms a layer-0 row once per entry that reaches it and once more for the row itself; here each is formed ONCE
// per (graph, slab), in the LDS window, and a pooled row's own h is a copy from there.
//   h_r  = ELU(sum_{k in row r} val[k] T[t(col[k])][0:H] + T[t(r)][H:2H] + b_l0)       r in [r0, r1)
//   g_r  = sum_{e in row r} val[e] h_{col[e]}                                           r among the graph's pooled rows
//   G[j] = [g_r | h_r]: graph_query_tail_kernel with K = 2H, W1 = [W_l1 | W_r1], b1 = b_l1 finishes (pool, head, softmax).
// Operation order (tests/sage_graph_query_reference.py mirrors it):
//   phase 1  row r by sage_row, unchanged: a = 0; a = fmaf(val[e'], T[t(col[e'])][c], a) over row r's entries in CSR order;
//            h_r[c] = ELU((a + T[t(r)][H + c]) + b0[c]) (b0 == NULL: the second add is absent); a row without entries:
//            ELU(T[t(r)][H + c] + b0[c]).  The same bits as the node kernel's h, on any wave and any slab.
//   phase 2  g = 0; g = fmaf(val[e], h_{col[e]}[c], g) over the pooled row's entries in CSR order, ONE chain (no wave partials);
//            G[j][c] = g, G[j][H + c] = h_r[c] from the window.  A pooled row without entries gives g = 0 and still its h_r.

// One workgroup of four waves per (graph, 256-column slab), the slab fastest.  The graph's rows are dealt round-robin to the waves,
// which form them (sage_row) into the LDS window hs [r1 - r0][min(H, 256)]: a wave writes and later reads 64 consecutive float4,
// every bank once, so the window needs no padding.  After the one barrier the graph's pooled rows are dealt round-robin to the waves;
// a wave fetches the row's entries 64 at a time and broadcasts (window row, value) by v_readlane.  A graph beyond max_rows returns
// before it touches anything; a graph without pooled rows writes nothing.
__global__ __launch_bounds__(256) void sage_graph_query_hops_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                    const float *__restrict__ val, const float *__restrict__ T,
                                                                    int64_t ldt, const int32_t *__restrict__ xrow,
                                                                    const float *__restrict__ b0, const int64_t *__restrict__ seg,
                                                                    const int64_t *__restrict__ prow, const int64_t *__restrict__ pptr,
                                                                    int32_t H, int32_t max_rows, float *__restrict__ G, int64_t ldg,
                                                                    int32_t n_slabs) {
    extern __shared__ float4 hs[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int gi = blockIdx.x / n_slabs, c0 = (blockIdx.x % n_slabs) * 256;
    const int r0 = __builtin_amdgcn_readfirstlane((int)seg[2 * (int64_t)gi]), r1 = __builtin_amdgcn_readfirstlane((int)seg[2 * (int64_t)gi + 1]);
    if (r1 - r0 > max_rows) return;  // workgroup-uniform: the window was sized for max_rows
    const int w4 = min(H, 256) >> 2;  // float4 per window row
    const int c = c0 + lane * 4;
    const bool live = c < H;  // H % 4 == 0: a live lane owns four whole columns
    const float *Tc = T + (live ? c : 0);
    const bool has_bias = b0 != nullptr;
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_bias && live) bias = make_float4(b0[c], b0[c + 1], b0[c + 2], b0[c + 3]);
    for (int r = r0 + w; r < r1; r += kGatherWaves) {
        const float4 h = sage_row(rowptr, col, val, Tc, ldt, H, xrow, has_bias, bias, r, lane);
        if (live) hs[(r - r0) * w4 + lane] = h;
    }
    __syncthreads();
    const int64_t p1 = pptr[gi + 1];
    for (int64_t j = pptr[gi] + w; j < p1; j += kGatherWaves) {
        const int r = __builtin_amdgcn_readfirstlane((int)prow[j]);
        const int n0 = __builtin_amdgcn_readfirstlane(rowptr[r]), n1 = __builtin_amdgcn_readfirstlane(rowptr[r + 1]);
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int base = n0; base < n1; base += 64) {
            const int cnt = min(64, n1 - base);
            int my = 0, mv = 0;
            if (lane < cnt) {
                my = col[base + lane] - r0;
                mv = __float_as_int(val[base + lane]);
            }
            for (int k = 0; k < cnt; ++k) {
                const int node = __builtin_amdgcn_readlane(my, k);
                const float wv = __int_as_float(__builtin_amdgcn_readlane(mv, k));
                if (live) {
                    const float4 h = hs[node * w4 + lane];
                    g.x = fmaf(wv, h.x, g.x);
                    g.y = fmaf(wv, h.y, g.y);
                    g.z = fmaf(wv, h.z, g.z);
                    g.w = fmaf(wv, h.w, g.w);
                }
            }
        }
        if (live) {
            *reinterpret_cast<float4 *>(G + j * ldg + c) = g;
            *reinterpret_cast<float4 *>(G + j * ldg + H + c) = hs[(r - r0) * w4 + lane];
        }
    }
}

}  // namespace

extern "C" int fitgnn_gcn_query_gather_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *T, int64_t ldt,
                                           const int32_t *xrow, const float *b0, const int64_t *rows, int32_t Q, int32_t H, float *G,
                                           int64_t ldg, void *stream) {
    if (Q < 0 || H < 4 || (H % 4) != 0 || ldt < H || ldg < H) return FITGNN_E_BADARG;
    if ((ldt % 4) != 0 || (ldg % 4) != 0) return FITGNN_E_ALIGN;
    if (Q == 0) return 0;
    if (!rowptr || !col || !val || !T || !rows || !G) return FITGNN_E_BADARG;
    if ((((uintptr_t)T | (uintptr_t)G) % 16) != 0) return FITGNN_E_ALIGN;
    const int n_slabs = (H + 255) / 256;
    if ((int64_t)Q * n_slabs > 0x7fffffffLL) return FITGNN_E_BADARG;
    hipLaunchKernelGGL(query_gather_kernel, dim3((unsigned)(Q * n_slabs)), dim3(256), 0, (hipStream_t)stream, rowptr, col, val, T, ldt, xrow,
                       b0, rows, H, G, ldg, n_slabs);
    return (int)hipGetLastError();
}

extern "C" int fitgnn_gat_query_gather_f32(const int32_t *rowptr, const int32_t *col, const float *T, int64_t ldt, const int32_t *xrow,
                                           const float *a_src0, const float *a_dst0, const float *b0, float slope0, const float *u_src,
                                           const float *u_dst, float slope1, const int64_t *rows, int32_t Q, int32_t H, float *G,
                                           int64_t ldg, void *stream) {
    if (Q < 0 || H < 4 || (H % 4) != 0 || H > 512 || ldt < H || ldg < H) return FITGNN_E_BADARG;
    if ((ldt % 4) != 0 || (ldg % 4) != 0) return FITGNN_E_ALIGN;
    if (Q == 0) return 0;
    if (!rowptr || !col || !T || !a_src0 || !a_dst0 || !u_src || !u_dst || !rows || !G) return FITGNN_E_BADARG;
    if ((((uintptr_t)T | (uintptr_t)G | (uintptr_t)u_src | (uintptr_t)u_dst) % 16) != 0) return FITGNN_E_ALIGN;
    if (H <= 256)
        hipLaunchKernelGGL(gat_query_hops_kernel<1>, dim3((unsigned)Q), dim3(256), 0, (hipStream_t)stream, rowptr, col, T, ldt, xrow, a_src0,
                           a_dst0, b0, slope0, u_src, u_dst, slope1, rows, H, G, ldg);
    else
        hipLaunchKernelGGL(gat_query_hops_kernel<2>, dim3((unsigned)Q), dim3(256), 0, (hipStream_t)stream, rowptr, col, T, ldt, xrow, a_src0,
                           a_dst0, b0, slope0, u_src, u_dst, slope1, rows, H, G, ldg);
    return (int)hipGetLastError();
}

extern "C" int fitgnn_sage_query_gather_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *T, int64_t ldt,
                                            const int32_t *xrow, const float *b0, const int64_t *rows, int32_t Q, int32_t H, float *G,
                                            int64_t ldg, void *stream) {
    if (Q < 0 || H < 4 || (H % 4) != 0 || ldt < 2 * (int64_t)H || ldg < 2 * (int64_t)H) return FITGNN_E_BADARG;
    if ((ldt % 4) != 0 || (ldg % 4) != 0) return FITGNN_E_ALIGN;
    if (Q == 0) return 0;
    if (!rowptr || !col || !val || !T || !rows || !G) return FITGNN_E_BADARG;
    if ((((uintptr_t)T | (uintptr_t)G) % 16) != 0) return FITGNN_E_ALIGN;
    const int n_slabs = (H + 255) / 256;
    if ((int64_t)Q * n_slabs > 0x7fffffffLL) return FITGNN_E_BADARG;
    hipLaunchKernelGGL(sage_query_gather_kernel, dim3((unsigned)(Q * n_slabs)), dim3(256), 0, (hipStream_t)stream, rowptr, col, val, T, ldt,
                       xrow, b0, rows, H, G, ldg, n_slabs);
    return (int)hipGetLastError();
}

extern "C" size_t fitgnn_gcn_query_tail_lds_bytes(int32_t H2, int32_t C) {
    if (H2 <= 0 || C <= 0) return 0;
    return tail_lds_floats(H2, C) * sizeof(float);
}

extern "C" int fitgnn_gcn_query_tail_f32(const float *G, int64_t ldg, int32_t Q, const float *W1, const float *b1, const float *Wl,
                                         const float *bl, int32_t H, int32_t H2, int32_t C, float *out, int64_t ldo, int32_t log_softmax,
                                         void *stream) {
    if (Q < 0 || H < 4 || (H % 4) != 0 || H2 < 16 || (H2 % 16) != 0 || C < 1 || ldg < H || ldo < C) return FITGNN_E_BADARG;
    if ((ldg % 4) != 0) return FITGNN_E_ALIGN;
    const size_t lds = fitgnn_gcn_query_tail_lds_bytes(H2, C);
    if (lds > kTailLdsMax) return FITGNN_E_BADARG;  // z of the tile does not fit LDS
    if (Q == 0) return 0;
    if (!G || !W1 || !Wl || !out) return FITGNN_E_BADARG;
    if ((((uintptr_t)G | (uintptr_t)W1 | (uintptr_t)Wl | (uintptr_t)out) % 16) != 0) return FITGNN_E_ALIGN;
    static std::atomic<uint64_t> lds_done{0};
    if (const int rc = fitgnn_lds_limit_once((const void *)query_tail_kernel, (int)kTailLdsMax, lds_done)) return rc;
    hipLaunchKernelGGL(query_tail_kernel, dim3((unsigned)((Q + kTailQ - 1) / kTailQ)), dim3(256), lds, (hipStream_t)stream, G, ldg, Q, W1, b1,
                       Wl, bl, H, H2, C, out, ldo, log_softmax);
    return (int)hipGetLastError();
}

template <int NS>
static int launch_mhgat_hops(const int32_t *rowptr, const int32_t *col, const float *T, int64_t ldt, const int32_t *xrow, const float *a_src0,
                             const float *a_dst0, int32_t heads, const float *b0, float slope0, const float *U_src, const float *U_dst,
                             float slope1, const int64_t *rows, int32_t Q, int32_t H, float *G, int64_t ldg, hipStream_t stream) {
    static std::atomic<uint64_t> lds_done{0};
    if (const int rc = fitgnn_lds_limit_once((const void *)mhgat_hops_kernel<NS>, (int)mhgat_hops_lds_bytes(kMhMaxHeads, NS), lds_done))
        return rc;
    hipLaunchKernelGGL((mhgat_hops_kernel<NS>), dim3((unsigned)Q), dim3(256), mhgat_hops_lds_bytes(heads, NS), stream, rowptr, col, T, ldt,
                       xrow, a_src0, a_dst0, heads, b0, slope0, U_src, U_dst, slope1, rows, H, G, ldg);
    return (int)hipGetLastError();
}

extern "C" int fitgnn_mhgat_query_gather_f32(const int32_t *rowptr, const int32_t *col, const float *T, int64_t ldt, const int32_t *xrow,
                                             const float *a_src0, const float *a_dst0, int32_t heads, const float *b0, float slope0,
                                             const float *U_src, const float *U_dst, float slope1, const int64_t *rows, int32_t Q, int32_t H,
                                             float *G, int64_t ldg, void *stream) {
    if (Q < 0 || heads < 2 || heads > kMhMaxHeads || H < 8 || H > 512 || (H % heads) != 0 || ((H / heads) % 4) != 0 || ldt < H ||
        ldg < (int64_t)heads * H)
        return FITGNN_E_BADARG;
    if ((ldt % 4) != 0 || (ldg % 4) != 0) return FITGNN_E_ALIGN;
    if (Q == 0) return 0;
    if (!rowptr || !col || !T || !a_src0 || !a_dst0 || !U_src || !U_dst || !rows || !G) return FITGNN_E_BADARG;
    if ((((uintptr_t)T | (uintptr_t)G | (uintptr_t)U_src | (uintptr_t)U_dst) % 16) != 0) return FITGNN_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    return H <= 256 ? launch_mhgat_hops<1>(rowptr, col, T, ldt, xrow, a_src0, a_dst0, heads, b0, slope0, U_src, U_dst, slope1, rows, Q, H, G, ldg, st)
                    : launch_mhgat_hops<2>(rowptr, col, T, ldt, xrow, a_src0, a_dst0, heads, b0, slope0, U_src, U_dst, slope1, rows, Q, H, G, ldg, st);
}

extern "C" size_t fitgnn_mhgat_query_tail_lds_bytes(int32_t H2, int32_t C, int32_t heads) {
    if (H2 <= 0 || C <= 0 || heads < 2 || heads > kMhMaxHeads) return 0;
    return mhgat_tail_lds_floats(H2, C, heads) * sizeof(float);
}

extern "C" int fitgnn_mhgat_query_tail_f32(const float *G, int64_t ldg, int32_t Q, const float *W1, const float *b1, const float *Wl,
                                           const float *bl, int32_t H, int32_t H2, int32_t heads, int32_t C, float *out, int64_t ldo,
                                           int32_t log_softmax, void *stream) {
    if (Q < 0 || heads < 2 || heads > kMhMaxHeads || H < 4 || (H % 4) != 0 || H2 < 16 || (H2 % heads) != 0 || ((H2 / heads) % 16) != 0 || C < 1 ||
        ldg < (int64_t)heads * H || ldo < C)
        return FITGNN_E_BADARG;
    if ((ldg % 4) != 0) return FITGNN_E_ALIGN;
    const size_t lds = fitgnn_mhgat_query_tail_lds_bytes(H2, C, heads);
    if (lds > kTailLdsMax) return FITGNN_E_BADARG;  // z of the tile does not fit LDS
    if (Q == 0) return 0;
    if (!G || !W1 || !Wl || !out) return FITGNN_E_BADARG;
    if ((((uintptr_t)G | (uintptr_t)W1 | (uintptr_t)Wl | (uintptr_t)out) % 16) != 0) return FITGNN_E_ALIGN;
    static std::atomic<uint64_t> lds_done{0};
    if (const int rc = fitgnn_lds_limit_once((const void *)mhgat_tail_kernel, (int)kTailLdsMax, lds_done)) return rc;
    hipLaunchKernelGGL(mhgat_tail_kernel, dim3((unsigned)((Q + kTailQ - 1) / kTailQ)), dim3(256), lds, (hipStream_t)stream, G, ldg, Q, W1,
                       b1, Wl, bl, H, H2, heads, C, out, ldo, log_softmax);
    return (int)hipGetLastError();
}

template <int NS, int NP>
static int launch_gin_hops(const int32_t *rowptr, const int32_t *col, const float *val, const float *T, int64_t ldt, const int32_t *xrow,
                           const float *b0a, const float *eps0, const float *W0b, const float *b0b, const float *eps1, const int64_t *rows,
                           int32_t Q, int32_t Ha, int32_t Hb, float *G, int64_t ldg, hipStream_t stream) {
    static std::atomic<uint64_t> lds_done{0};
    const size_t lds = gin_hops_lds_floats(Ha) * sizeof(float);
    if (const int rc = fitgnn_lds_limit_once((const void *)gin_query_hops_kernel<NS, NP>, (int)(gin_hops_lds_floats(512) * sizeof(float)), lds_done))
        return rc;
    hipLaunchKernelGGL((gin_query_hops_kernel<NS, NP>), dim3((unsigned)Q), dim3(256), lds, stream, rowptr, col, val, T, ldt, xrow, b0a, eps0, W0b,
                       b0b, eps1, rows, Ha, Hb, G, ldg);
    return (int)hipGetLastError();
}

extern "C" int fitgnn_gin_query_hops_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *T, int64_t ldt,
                                         const int32_t *xrow, const float *b0a, const float *eps0, const float *W0b, const float *b0b,
                                         const float *eps1, const int64_t *rows, int32_t Q, int32_t Ha, int32_t Hb, float *G, int64_t ldg,
                                         void *stream) {
    if (Q < 0 || Ha < 4 || (Ha % 4) != 0 || Ha > 512 || Hb < 16 || (Hb % 16) != 0 || Hb > 512 || ldt < Ha || ldg < Hb) return FITGNN_E_BADARG;
    if ((ldt % 4) != 0 || (ldg % 4) != 0) return FITGNN_E_ALIGN;
    if (Q == 0) return 0;
    if (!rowptr || !col || !val || !T || !eps0 || !W0b || !eps1 || !rows || !G) return FITGNN_E_BADARG;
    if ((((uintptr_t)T | (uintptr_t)G | (uintptr_t)W0b) % 16) != 0) return FITGNN_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    if (Ha <= 256)
        return Hb <= 256 ? launch_gin_hops<1, 1>(rowptr, col, val, T, ldt, xrow, b0a, eps0, W0b, b0b, eps1, rows, Q, Ha, Hb, G, ldg, st)
                         : launch_gin_hops<1, 2>(rowptr, col, val, T, ldt, xrow, b0a, eps0, W0b, b0b, eps1, rows, Q, Ha, Hb, G, ldg, st);
    return Hb <= 256 ? launch_gin_hops<2, 1>(rowptr, col, val, T, ldt, xrow, b0a, eps0, W0b, b0b, eps1, rows, Q, Ha, Hb, G, ldg, st)
                     : launch_gin_hops<2, 2>(rowptr, col, val, T, ldt, xrow, b0a, eps0, W0b, b0b, eps1, rows, Q, Ha, Hb, G, ldg, st);
}

extern "C" size_t fitgnn_gin_query_tail_lds_bytes(int32_t H2a, int32_t H2b, int32_t C) {
    if (H2a <= 0 || H2b <= 0 || C <= 0) return 0;
    return gin_tail_lds_floats(H2a, H2b, C) * sizeof(float);
}

extern "C" int fitgnn_gin_query_tail_f32(const float *G, int64_t ldg, int32_t Q, const float *W1a, const float *b1a, const float *W1b,
                                         const float *b1b, const float *Wl, const float *bl, int32_t K, int32_t H2a, int32_t H2b, int32_t C,
                                         float *out, int64_t ldo, int32_t log_softmax, void *stream) {
    if (Q < 0 || K < 4 || (K % 4) != 0 || H2a < 16 || (H2a % 16) != 0 || H2b < 16 || (H2b % 16) != 0 || C < 1 || ldg < K || ldo < C)
        return FITGNN_E_BADARG;
    if ((ldg % 4) != 0) return FITGNN_E_ALIGN;
    const size_t lds = fitgnn_gin_query_tail_lds_bytes(H2a, H2b, C);
    if (lds > kTailLdsMax) return FITGNN_E_BADARG;  // z1 and z2 of the tile do not fit LDS
    if (Q == 0) return 0;
    if (!G || !W1a || !W1b || !Wl || !out) return FITGNN_E_BADARG;
    if ((((uintptr_t)G | (uintptr_t)W1a | (uintptr_t)W1b | (uintptr_t)Wl | (uintptr_t)out) % 16) != 0) return FITGNN_E_ALIGN;
    static std::atomic<uint64_t> lds_done{0};
    if (const int rc = fitgnn_lds_limit_once((const void *)gin_query_tail_kernel, (int)kTailLdsMax, lds_done)) return rc;
    hipLaunchKernelGGL(gin_query_tail_kernel, dim3((unsigned)((Q + kTailQ - 1) / kTailQ)), dim3(256), lds, (hipStream_t)stream, G, ldg, Q, W1a,
                       b1a, W1b, b1b, Wl, bl, K, H2a, H2b, C, out, ldo, log_softmax);
    return (int)hipGetLastError();
}

extern "C" size_t fitgnn_gcn_graph_query_hops_lds_bytes(int32_t max_rows, int32_t H) {
    if (max_rows < 0 || H < 4) return 0;
    return (size_t)max_rows * (size_t)std::min(H, 256) * sizeof(float);
}

extern "C" int fitgnn_gcn_graph_query_hops_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *T, int64_t ldt,
                                               const int32_t *xrow, const float *b0, const int64_t *seg, const int64_t *prow,
                                               const int64_t *pptr, int32_t Q, int32_t H, int32_t max_rows, float *G, int64_t ldg,
                                               void *stream) {
    if (Q < 0 || H < 4 || (H % 4) != 0 || max_rows < 0 || ldt < H || ldg < H) return FITGNN_E_BADARG;
    if ((ldt % 4) != 0 || (ldg % 4) != 0) return FITGNN_E_ALIGN;
    const size_t lds = fitgnn_gcn_graph_query_hops_lds_bytes(max_rows, H);
    if (lds > kTailLdsMax) return FITGNN_E_BADARG;  // the largest graph's layer-0 rows do not fit LDS
    if (Q == 0) return 0;
    if (!rowptr || !col || !val || !T || !seg || !prow || !pptr || !G) return FITGNN_E_BADARG;
    if ((((uintptr_t)T | (uintptr_t)G) % 16) != 0) return FITGNN_E_ALIGN;
    const int n_slabs = (H + 255) / 256;
    if ((int64_t)Q * n_slabs > 0x7fffffffLL) return FITGNN_E_BADARG;
    static std::atomic<uint64_t> lds_done{0};
    if (const int rc = fitgnn_lds_limit_once((const void *)graph_query_hops_kernel, (int)kTailLdsMax, lds_done)) return rc;
    hipLaunchKernelGGL(graph_query_hops_kernel, dim3((unsigned)(Q * n_slabs)), dim3(256), lds, (hipStream_t)stream, rowptr, col, val, T, ldt,
                       xrow, b0, seg, prow, pptr, H, max_rows, G, ldg, n_slabs);
    return (int)hipGetLastError();
}

extern "C" size_t fitgnn_gcn_graph_query_tail_lds_bytes(int32_t H2, int32_t C) {
    if (H2 <= 0 || C <= 0) return 0;
    return graph_tail_lds_floats(H2, C) * sizeof(float);
}

extern "C" int fitgnn_gcn_graph_query_tail_f32(const float *G, int64_t ldg, const int64_t *pptr, int32_t Q, const float *W1, const float *b1,
                                               const float *Wl, const float *bl, int32_t H, int32_t H2, int32_t C, int32_t pool,
                                               int32_t softmax, float *out, int64_t ldo, void *stream) {
    if (Q < 0 || H < 4 || (H % 4) != 0 || H2 < 16 || (H2 % 16) != 0 || C < 1 || ldg < H || ldo < C || pool < 0 || pool > 1)
        return FITGNN_E_BADARG;
    if ((ldg % 4) != 0) return FITGNN_E_ALIGN;
    const size_t lds = fitgnn_gcn_graph_query_tail_lds_bytes(H2, C);
    if (lds > kTailLdsMax) return FITGNN_E_BADARG;  // z of the tile and the pooled row do not fit LDS
    if (Q == 0) return 0;
    if (!G || !pptr || !W1 || !Wl || !out) return FITGNN_E_BADARG;
    if ((((uintptr_t)G | (uintptr_t)W1 | (uintptr_t)Wl | (uintptr_t)out) % 16) != 0) return FITGNN_E_ALIGN;
    static std::atomic<uint64_t> lds_done{0};
    if (const int rc = fitgnn_lds_limit_once((const void *)graph_query_tail_kernel, (int)kTailLdsMax, lds_done)) return rc;
    hipLaunchKernelGGL(graph_query_tail_kernel, dim3((unsigned)Q), dim3(256), lds, (hipStream_t)stream, G, ldg, pptr, W1, b1, Wl, bl, H, H2, C,
                       pool, softmax, out, ldo);
    return (int)hipGetLastError();
}

extern "C" size_t fitgnn_gin_graph_query_hops_lds_bytes(int32_t max_rows, int32_t Ha, int32_t Hb) {
    if (max_rows < 0 || Ha < 4 || Hb < 16) return 0;
    return gin_graph_hops_lds_floats(max_rows, Ha, Hb) * sizeof(float);
}

template <int NS>
static int launch_gin_graph_hops(const int32_t *rowptr, const int32_t *col, const float *val, const float *T, int64_t ldt, const int32_t *xrow,
                                 const float *b0a, const float *eps0, const float *W0b, const float *b0b, const float *eps1,
                                 const int64_t *seg, const int64_t *prow, const int64_t *pptr, int32_t Q, int32_t Ha, int32_t Hb,
                                 int32_t max_rows, float *G, int64_t ldg, size_t lds, int n_slabs, hipStream_t stream) {
    static std::atomic<uint64_t> lds_done{0};
    if (const int rc = fitgnn_lds_limit_once((const void *)gin_graph_query_hops_kernel<NS>, (int)kTailLdsMax, lds_done)) return rc;
    hipLaunchKernelGGL((gin_graph_query_hops_kernel<NS>), dim3((unsigned)(Q * n_slabs)), dim3(256), lds, stream, rowptr, col, val, T, ldt, xrow,
                       b0a, eps0, W0b, b0b, eps1, seg, prow, pptr, Ha, Hb, max_rows, G, ldg, n_slabs);
    return (int)hipGetLastError();
}

extern "C" int fitgnn_gin_graph_query_hops_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *T, int64_t ldt,
                                               const int32_t *xrow, const float *b0a, const float *eps0, const float *W0b, const float *b0b,
                                               const float *eps1, const int64_t *seg, const int64_t *prow, const int64_t *pptr, int32_t Q,
                                               int32_t Ha, int32_t Hb, int32_t max_rows, float *G, int64_t ldg, void *stream) {
    if (Q < 0 || Ha < 4 || (Ha % 4) != 0 || Ha > 512 || Hb < 16 || (Hb % 16) != 0 || Hb > 512 || max_rows < 0 || ldt < Ha || ldg < Hb)
        return FITGNN_E_BADARG;
    if ((ldt % 4) != 0 || (ldg % 4) != 0) return FITGNN_E_ALIGN;
    const size_t lds = fitgnn_gin_graph_query_hops_lds_bytes(max_rows, Ha, Hb);
    if (lds > kTailLdsMax) return FITGNN_E_BADARG;  // the largest graph's layer-0 rows do not fit LDS beside the two stages
    if (Q == 0) return 0;
    if (!rowptr || !col || !val || !T || !eps0 || !W0b || !eps1 || !seg || !prow || !pptr || !G) return FITGNN_E_BADARG;
    if ((((uintptr_t)T | (uintptr_t)G | (uintptr_t)W0b) % 16) != 0) return FITGNN_E_ALIGN;
    const int n_slabs = (Hb + kTailCols - 1) / kTailCols;
    if ((int64_t)Q * n_slabs > 0x7fffffffLL) return FITGNN_E_BADARG;
    const hipStream_t st = (hipStream_t)stream;
    return Ha <= 256 ? launch_gin_graph_hops<1>(rowptr, col, val, T, ldt, xrow, b0a, eps0, W0b, b0b, eps1, seg, prow, pptr, Q, Ha, Hb, max_rows,
                                                G, ldg, lds, n_slabs, st)
                     : launch_gin_graph_hops<2>(rowptr, col, val, T, ldt, xrow, b0a, eps0, W0b, b0b, eps1, seg, prow, pptr, Q, Ha, Hb, max_rows,
                                                G, ldg, lds, n_slabs, st);
}

extern "C" size_t fitgnn_gin_graph_query_tail_lds_bytes(int32_t H2a, int32_t H2b, int32_t C) {
    if (H2a <= 0 || H2b <= 0 || C <= 0) return 0;
    return gin_graph_tail_lds_floats(H2a, H2b, C) * sizeof(float);
}

extern "C" int fitgnn_gin_graph_query_tail_f32(const float *G, int64_t ldg, const int64_t *pptr, int32_t Q, const float *W1a, const float *b1a,
                                               const float *W1b, const float *b1b, const float *Wl, const float *bl, int32_t K, int32_t H2a,
                                               int32_t H2b, int32_t C, int32_t pool, int32_t softmax, float *out, int64_t ldo, void *stream) {
    if (Q < 0 || K < 4 || (K % 4) != 0 || H2a < 16 || (H2a % 16) != 0 || H2b < 16 || (H2b % 16) != 0 || C < 1 || ldg < K || ldo < C ||
        pool < 0 || pool > 1)
        return FITGNN_E_BADARG;
    if ((ldg % 4) != 0) return FITGNN_E_ALIGN;
    const size_t lds = fitgnn_gin_graph_query_tail_lds_bytes(H2a, H2b, C);
    if (lds > kTailLdsMax) return FITGNN_E_BADARG;  // z1, z2 of the tile and the pooled row do not fit LDS
    if (Q == 0) return 0;
    if (!G || !pptr || !W1a || !W1b || !Wl || !out) return FITGNN_E_BADARG;
    if ((((uintptr_t)G | (uintptr_t)W1a | (uintptr_t)W1b | (uintptr_t)Wl | (uintptr_t)out) % 16) != 0) return FITGNN_E_ALIGN;
    static std::atomic<uint64_t> lds_done{0};
    if (const int rc = fitgnn_lds_limit_once((const void *)gin_graph_query_tail_kernel, (int)kTailLdsMax, lds_done)) return rc;
    hipLaunchKernelGGL(gin_graph_query_tail_kernel, dim3((unsigned)Q), dim3(256), lds, (hipStream_t)stream, G, ldg, pptr, W1a, b1a, W1b, b1b, Wl,
                       bl, K, H2a, H2b, C, pool, softmax, out, ldo);
    return (int)hipGetLastError();
}

extern "C" size_t fitgnn_gat_graph_query_hops_lds_bytes(int32_t max_rows, int32_t H) {
    if (max_rows < 0 || H < 4) return 0;
    return (size_t)max_rows * ((size_t)H + 2) * sizeof(float);
}

template <int NS>
static int launch_gat_graph_hops(const int32_t *rowptr, const int32_t *col, const float *T, int64_t ldt, const int32_t *xrow,
                                 const float *a_src0, const float *a_dst0, const float *b0, float slope0, const float *u_src,
                                 const float *u_dst, float slope1, const int64_t *seg, const int64_t *prow, const int64_t *pptr, int32_t Q,
                                 int32_t H, int32_t max_rows, float *G, int64_t ldg, size_t lds, hipStream_t stream) {
    static std::atomic<uint64_t> lds_done{0};
    if (const int rc = fitgnn_lds_limit_once((const void *)gat_graph_query_hops_kernel<NS>, (int)kTailLdsMax, lds_done)) return rc;
    hipLaunchKernelGGL((gat_graph_query_hops_kernel<NS>), dim3((unsigned)Q), dim3(256), lds, stream, rowptr, col, T, ldt, xrow, a_src0, a_dst0,
                       b0, slope0, u_src, u_dst, slope1, seg, prow, pptr, H, max_rows, G, ldg);
    return (int)hipGetLastError();
}

extern "C" int fitgnn_gat_graph_query_hops_f32(const int32_t *rowptr, const int32_t *col, const float *T, int64_t ldt, const int32_t *xrow,
                                               const float *a_src0, const float *a_dst0, const float *b0, float slope0, const float *u_src,
                                               const float *u_dst, float slope1, const int64_t *seg, const int64_t *prow,
                                               const int64_t *pptr, int32_t Q, int32_t H, int32_t max_rows, float *G, int64_t ldg,
                                               void *stream) {
    if (Q < 0 || H < 4 || (H % 4) != 0 || H > 512 || max_rows < 0 || ldt < H || ldg < H) return FITGNN_E_BADARG;
    if ((ldt % 4) != 0 || (ldg % 4) != 0) return FITGNN_E_ALIGN;
    const size_t lds = fitgnn_gat_graph_query_hops_lds_bytes(max_rows, H);
    if (lds > kTailLdsMax) return FITGNN_E_BADARG;  // the largest graph's layer-0 rows and their dots do not fit LDS
    if (Q == 0) return 0;
    if (!rowptr || !col || !T || !a_src0 || !a_dst0 || !u_src || !u_dst || !seg || !prow || !pptr || !G) return FITGNN_E_BADARG;
    if ((((uintptr_t)T | (uintptr_t)G | (uintptr_t)u_src | (uintptr_t)u_dst) % 16) != 0) return FITGNN_E_ALIGN;
    const hipStream_t st = (hipStream_t)stream;
    return H <= 256 ? launch_gat_graph_hops<1>(rowptr, col, T, ldt, xrow, a_src0, a_dst0, b0, slope0, u_src, u_dst, slope1, seg, prow, pptr, Q, H,
                                               max_rows, G, ldg, lds, st)
                    : launch_gat_graph_hops<2>(rowptr, col, T, ldt, xrow, a_src0, a_dst0, b0, slope0, u_src, u_dst, slope1, seg, prow, pptr, Q, H,
                                               max_rows, G, ldg, lds, st);
}

extern "C" size_t fitgnn_sage_graph_query_hops_lds_bytes(int32_t max_rows, int32_t H) {
    if (max_rows < 0 || H < 4) return 0;
    return (size_t)max_rows * (size_t)std::min(H, 256) * sizeof(float);
}

extern "C" int fitgnn_sage_graph_query_hops_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *T, int64_t ldt,
                                                const int32_t *xrow, const float *b0, const int64_t *seg, const int64_t *prow,
                                                const int64_t *pptr, int32_t Q, int32_t H, int32_t max_rows, float *G, int64_t ldg,
                                                void *stream) {
    if (Q < 0 || H < 4 || (H % 4) != 0 || max_rows < 0 || ldt < 2 * (int64_t)H || ldg < 2 * (int64_t)H) return FITGNN_E_BADARG;
    if ((ldt % 4) != 0 || (ldg % 4) != 0) return FITGNN_E_ALIGN;
    const size_t lds = fitgnn_sage_graph_query_hops_lds_bytes(max_rows, H);
    if (lds > kTailLdsMax) return FITGNN_E_BADARG;  // the largest graph's layer-0 rows do not fit LDS
    if (Q == 0) return 0;
    if (!rowptr || !col || !val || !T || !seg || !prow || !pptr || !G) return FITGNN_E_BADARG;
    if ((((uintptr_t)T | (uintptr_t)G) % 16) != 0) return FITGNN_E_ALIGN;
    const int n_slabs = (H + 255) / 256;
    if ((int64_t)Q * n_slabs > 0x7fffffffLL) return FITGNN_E_BADARG;
    static std::atomic<uint64_t> lds_done{0};
    if (const int rc = fitgnn_lds_limit_once((const void *)sage_graph_query_hops_kernel, (int)kTailLdsMax, lds_done)) return rc;
    hipLaunchKernelGGL(sage_graph_query_hops_kernel, dim3((unsigned)(Q * n_slabs)), dim3(256), lds, (hipStream_t)stream, rowptr, col, val, T,
                       ldt, xrow, b0, seg, prow, pptr, H, max_rows, G, ldg, n_slabs);
    return (int)hipGetLastError();
}
