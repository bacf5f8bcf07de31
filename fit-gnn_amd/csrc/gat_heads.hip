// gat_heads.hip -- multi-head graph attention on the CSR batch (PyG GATConv(in, out, heads = Hd), concat layout).
//
//   h = x W^T is [n, W], W = Hd * C, head hd owning columns hd*C .. (hd+1)*C;  per head:
//   s_ij = a_src[j, hd] + a_dst[i, hd];  alpha_ij = softmax_j LeakyReLU(s_ij) over CSR row i;  out_i[hd slice] = sum_j alpha_ij h_j[hd slice].
// Per-node scores are [n, Hd] row-major; per-entry quantities (alpha, dalpha, ds) are [nnz, Hd] ENTRY-major: a row's entries and an
// entry's heads are contiguous.  The kernels of gat.hip put a wavefront on a row and its lanes on the row's columns; called once per
// head on a C-column slice they would keep C / 4 of 64 lanes busy and read the column indices Hd times.  Here a wavefront reads each
// operand row ONCE at full width (16-byte lane loads, the row of dOut / the accumulator in registers up to W = 1024), each column
// index once for all heads, and the per-head sums of the score dots and of the SDDMM are butterflies over the C / 4 lanes of a head.
// No atomics, no LDS: every sum has a fixed order, two launches give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "fitgnn_hip.h"

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
// the sum over the aligned group of w lanes the lane sits in (w a power of two <= 64, wave-uniform); every lane of the group gets it
__device__ __forceinline__ float group_sum(float v, int w) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        if (off < w) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// a_src[i, hd] = h_i[hd slice] . att_src[hd slice],  a_dst likewise          (one wave per row, one pass over the row)
// vec (decided by the host): C / 4 = L is a power of two, so the float4s of a head sit on L consecutive lanes (L <= 64: 64 / L heads
// per 256-column slot, one L-lane butterfly each) or fill L / 64 whole slots (their partial sums add up in the lane, then one 64-lane
// butterfly); ldh a multiple of 4 and h, att_src, att_dst 16-byte aligned.  Otherwise: the heads in turn, scalar loads, 64-lane sums.
__global__ __launch_bounds__(256) void gat_heads_scores_kernel(const float *__restrict__ h, int64_t ldh, int32_t n, int32_t Hd, int32_t C,
                                                               const float *__restrict__ att_src, const float *__restrict__ att_dst,
                                                               float *__restrict__ a_src, float *__restrict__ a_dst, bool vec) {
    const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const float *hr = h + (int64_t)row * ldh;
    const int W = Hd * C;
    if (vec) {
        const int L = C >> 2;
        const int lw = L < 64 ? L : 64;
        float s = 0.f, d = 0.f;
        for (int base = 0; base < W; base += 256) {   // wave-uniform
            const int c = base + lane * 4;
            if (c < W) {
                const float4 v = *reinterpret_cast<const float4 *>(hr + c);
                s += dot4(v, *reinterpret_cast<const float4 *>(att_src + c));
                d += dot4(v, *reinterpret_cast<const float4 *>(att_dst + c));
            }
            if (L <= 64 || (base + 256) % C == 0) {   // the slot ends its heads
                s = group_sum(s, lw);
                d = group_sum(d, lw);
                if (c < W && (lane & (lw - 1)) == 0) {
                    a_src[row * Hd + c / C] = s;
                    a_dst[row * Hd + c / C] = d;
                }
                s = d = 0.f;
            }
        }
    } else {
        for (int hd = 0; hd < Hd; ++hd) {
            const int o = hd * C;
            float s = 0.f, d = 0.f;
            for (int c = lane; c < C; c += 64) { s += hr[o + c] * att_src[o + c]; d += hr[o + c] * att_dst[o + c]; }
            s = wave_sum(s);
            d = wave_sum(d);
            if (lane == 0) { a_src[row * Hd + hd] = s; a_dst[row * Hd + hd] = d; }
        }
    }
}

// alpha[e, hd] over each CSR row and head: softmax_j LeakyReLU(a_src[col[e], hd] + a_dst[row, hd]).  gat_edge_softmax_kernel's split
// with one item per (row, head), the heads of a row on neighbouring threads (their reads of a_src[col] and writes of alpha are
// contiguous): an item of at most kShortRow entries on its thread, scores in registers between the three passes; the long items of
// a wave one after the other by the whole wave (entries on lanes).  An item without entries writes nothing (z is never divided by).
constexpr int kShortRow = 8;

__global__ __launch_bounds__(256) void gat_heads_edge_softmax_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                     const float *__restrict__ a_src, const float *__restrict__ a_dst,
                                                                     float slope, int32_t n, int32_t Hd, float *__restrict__ alpha) {
    const int64_t tl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // item (row, head); n * Hd < 2^31 (the host refuses more)
    const int lane = threadIdx.x & 63;
    const bool on = tl < (int64_t)n * Hd;
    const int t = on ? (int)tl : 0;
    int e0 = 0, len = 0, hd = 0;
    float ad = 0.f;
    if (on) {
        const int row = t / Hd;
        hd = t - row * Hd;
        e0 = rowptr[row];
        len = rowptr[row + 1] - e0;
        ad = a_dst[t];
    }
    if (on && len <= kShortRow) {
        float sc[kShortRow];
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < kShortRow; ++k) {
            float v = -INFINITY;
            if (k < len) {
                v = a_src[col[e0 + k] * Hd + hd] + ad;
                v = v > 0.f ? v : slope * v;
            }
            sc[k] = v;
            m = fmaxf(m, v);
        }
        float z = 0.f;
#pragma unroll
        for (int k = 0; k < kShortRow; ++k) {
            const float p = k < len ? __expf(sc[k] - m) : 0.f;
            sc[k] = p;
            z += p;
        }
        const float inv = z > 0.f ? 1.0f / z : 0.f;
#pragma unroll
        for (int k = 0; k < kShortRow; ++k)
            if (k < len) alpha[(e0 + k) * Hd + hd] = sc[k] * inv;
    }
    unsigned long long longs = __ballot(on && len > kShortRow);
    while (longs) {   // wave-uniform
        const int src = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const int b0 = __shfl(e0, src, 64), b1 = b0 + __shfl(len, src, 64);
        const int hl = __shfl(hd, src, 64);
        const float adr = __shfl(ad, src, 64);
        float m = -INFINITY;
        for (int e = b0 + lane; e < b1; e += 64) {
            float v = a_src[col[e] * Hd + hl] + adr;
            v = v > 0.f ? v : slope * v;
            m = fmaxf(m, v);
        }
        m = wave_max(m);
        float z = 0.f;
        for (int e = b0 + lane; e < b1; e += 64) {
            float v = a_src[col[e] * Hd + hl] + adr;
            v = v > 0.f ? v : slope * v;
            const float p = __expf(v - m);
            alpha[e * Hd + hl] = p;
            z += p;
        }
        z = wave_sum(z);
        const float inv = z > 0.f ? 1.0f / z : 0.f;
        for (int e = b0 + lane; e < b1; e += 64) alpha[e * Hd + hl] *= inv;
    }
}

// Y[i, hd*C + c] = sum_e alpha[e, hd] X[col[e], hd*C + c] (+ bias)          (one wave per row, the accumulator in registers)
// C % 4 == 0: no float4 straddles two heads, a lane's float4 of slot v belongs to head hd[v].  The row's column ids sit on the lanes,
// four entries per step with their operand rows all in flight before the first multiply-add (as gat_sddmm_kernel); the additions
// stay in CSR order.  A step's last group is padded with its last entry at weight 0.
template <int MAXV>  // MAXV float4 per lane: W <= 256 * MAXV
__global__ __launch_bounds__(256) void gat_heads_aggregate_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                  const float *__restrict__ alpha, const float *__restrict__ X, int64_t ldx,
                                                                  float *__restrict__ Y, int64_t ldy, int32_t n, int32_t Hd, int32_t C,
                                                                  const float *__restrict__ bias) {
    const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const int W = Hd * C;
    int hd[MAXV];
    float4 acc[MAXV];
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
        const int c = (v * 64 + lane) * 4;
        hd[v] = c < W ? c / C : 0;
        acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int base = e0; base < e1; base += 64) {
        const int cnt = min(64, e1 - base);
        const int my_c = lane < cnt ? col[base + lane] : 0;
        for (int k = 0; k < cnt; k += 4) {
            const int n4 = min(4, cnt - k);  // wave-uniform
            float4 x[4][MAXV];
            float a[4][MAXV];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int jj = min(j, n4 - 1);
                const int cj = __builtin_amdgcn_readlane(my_c, k + jj);
                const float *xr = X + (int64_t)cj * ldx;
                const float *ar = alpha + (base + k + jj) * Hd;
#pragma unroll
                for (int v = 0; v < MAXV; ++v) {
                    const int c = (v * 64 + lane) * 4;
                    x[j][v] = c < W ? *reinterpret_cast<const float4 *>(xr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
                    a[j][v] = (c < W && j < n4) ? ar[hd[v]] : 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int v = 0; v < MAXV; ++v) {
                    acc[v].x = fmaf(a[j][v], x[j][v].x, acc[v].x); acc[v].y = fmaf(a[j][v], x[j][v].y, acc[v].y);
                    acc[v].z = fmaf(a[j][v], x[j][v].z, acc[v].z); acc[v].w = fmaf(a[j][v], x[j][v].w, acc[v].w);
                }
        }
    }
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
        const int c = (v * 64 + lane) * 4;
        if (c < W) {
            float4 y = acc[v];
            if (bias) { y.x += bias[c]; y.y += bias[c + 1]; y.z += bias[c + 2]; y.w += bias[c + 3]; }
            *reinterpret_cast<float4 *>(Y + (int64_t)row * ldy + c) = y;
        }
    }
}
// any heads, C, strides and alignment: a lane on columns lane, lane + 64, ... of the row, the entries in CSR order per column
__global__ __launch_bounds__(256) void gat_heads_aggregate_scalar_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                         const float *__restrict__ alpha, const float *__restrict__ X,
                                                                         int64_t ldx, float *__restrict__ Y, int64_t ldy, int32_t n, int32_t Hd,
                                                                         int32_t C, const float *__restrict__ bias) {
    const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const int W = Hd * C;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int c = lane; c < W; c += 64) {
        const int hd = c / C;
        float acc = 0.f;
        for (int e = e0; e < e1; ++e) acc = fmaf(alpha[e * Hd + hd], X[(int64_t)col[e] * ldx + c], acc);
        Y[(int64_t)row * ldy + c] = bias ? acc + bias[c] : acc;
    }
}

// dalpha[e, hd] = dOut[row, hd slice] . h[col[e], hd slice]          (SDDMM; one wave per row keeps dOut[row] in registers)
// C / 4 = L a power of two (the host decides): the per-lane products of slot v belong to head hd[v], and a head's sum is
//   L <= 64: an L-lane butterfly inside the slot (64 / L heads per slot);
//   L  > 64: the head fills sph = L / 64 whole slots: their products add up in the lane first, then one 64-lane butterfly.
// The first lane of each head's group writes the head's value of the step's four entries.
template <int MAXV>  // MAXV float4 per lane: W <= 256 * MAXV
__global__ __launch_bounds__(256) void gat_heads_sddmm_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                              const float *__restrict__ dOut, int64_t ldo, const float *__restrict__ h,
                                                              int64_t ldh, int32_t n, int32_t Hd, int32_t C, float *__restrict__ dalpha) {
    const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const int W = Hd * C;
    const int L = C >> 2;
    const int lw = L < 64 ? L : 64;
    const int sph = L > 64 ? L >> 6 : 1;   // slots per head
    float4 g[MAXV];
    int hd[MAXV];
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
        const int c = (v * 64 + lane) * 4;
        g[v] = c < W ? *reinterpret_cast<const float4 *>(dOut + (int64_t)row * ldo + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        hd[v] = c < W ? c / C : 0;
    }
    const bool writer = (lane & (lw - 1)) == 0;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int base = e0; base < e1; base += 64) {
        const int cnt = min(64, e1 - base);
        const int my_c = lane < cnt ? col[base + lane] : 0;
        for (int k = 0; k < cnt; k += 4) {
            const int n4 = min(4, cnt - k);  // wave-uniform
            float4 x[4][MAXV];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cj = __builtin_amdgcn_readlane(my_c, k + min(j, n4 - 1));
                const float *hr = h + (int64_t)cj * ldh;
#pragma unroll
                for (int v = 0; v < MAXV; ++v) {
                    const int c = (v * 64 + lane) * 4;
                    x[j][v] = c < W ? *reinterpret_cast<const float4 *>(hr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            float s[4][MAXV];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int v = 0; v < MAXV; ++v) s[j][v] = dot4(g[v], x[j][v]);
            if constexpr (MAXV >= 2) {
                if (sph >= 2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int v = 0; v + 1 < MAXV; v += 2) s[j][v] += s[j][v + 1];
                }
            }
            if constexpr (MAXV >= 4) {
                if (sph >= 4) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) s[j][0] += s[j][2];
                }
            }
#pragma unroll
            for (int v = 0; v < MAXV; ++v) {
                if ((v & (sph - 1)) != 0) continue;   // (wave-uniform) not the first slot of its head
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j][v] = group_sum(s[j][v], lw);
                if (writer && (v * 64 + lane) * 4 < W) {
                    float *o = dalpha + (base + k) * Hd + hd[v];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < n4) o[j * Hd] = s[j][v];
                }
            }
        }
    }
}
// any heads, C, strides and alignment: the heads in turn with a 64-lane sum each, as gat_sddmm_scalar_kernel does for one head
__global__ __launch_bounds__(256) void gat_heads_sddmm_scalar_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                     const float *__restrict__ dOut, int64_t ldo,
                                                                     const float *__restrict__ h, int64_t ldh, int32_t n, int32_t Hd,
                                                                     int32_t C, float *__restrict__ dalpha) {
    const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const float *gr = dOut + (int64_t)row * ldo;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int e = e0; e < e1; ++e) {
        const float *hr = h + (int64_t)col[e] * ldh;
        for (int hd = 0; hd < Hd; ++hd) {
            const int o = hd * C;
            float s = 0.f;
            for (int c = lane; c < C; c += 64) s += gr[o + c] * hr[o + c];
            s = wave_sum(s);
            if (lane == 0) dalpha[e * Hd + hd] = s;
        }
    }
}

// softmax + LeakyReLU backward per row and head:  ds[e, hd] = alpha (dalpha - sum_k alpha_k dalpha_k) * lrelu'(s);
// da_dst[row, hd] = sum_e ds[e, hd].  ds stays per entry for the column-side sum (on the transposed order).  Items, threads and
// waves as in the forward kernel; an item without entries writes da_dst = 0.
__global__ __launch_bounds__(256) void gat_heads_softmax_bwd_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                    const float *__restrict__ a_src, const float *__restrict__ a_dst,
                                                                    const float *__restrict__ alpha, const float *__restrict__ dalpha,
                                                                    float slope, int32_t n, int32_t Hd, float *__restrict__ ds,
                                                                    float *__restrict__ da_dst) {
    const int64_t tl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool on = tl < (int64_t)n * Hd;
    const int t = on ? (int)tl : 0;
    int e0 = 0, len = 0, hd = 0;
    float ad = 0.f;
    if (on) {
        const int row = t / Hd;
        hd = t - row * Hd;
        e0 = rowptr[row];
        len = rowptr[row + 1] - e0;
        ad = a_dst[t];
    }
    if (on && len <= kShortRow) {
        float al[kShortRow], da[kShortRow];
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < kShortRow; ++k) {
            al[k] = k < len ? alpha[(e0 + k) * Hd + hd] : 0.f;
            da[k] = k < len ? dalpha[(e0 + k) * Hd + hd] : 0.f;
            dot += al[k] * da[k];
        }
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < kShortRow; ++k)
            if (k < len) {
                const float sv = a_src[col[e0 + k] * Hd + hd] + ad;
                const float d = al[k] * (da[k] - dot) * (sv > 0.f ? 1.0f : slope);
                ds[(e0 + k) * Hd + hd] = d;
                acc += d;
            }
        da_dst[t] = acc;
    }
    unsigned long long longs = __ballot(on && len > kShortRow);
    while (longs) {   // wave-uniform
        const int src = __ffsll((long long)longs) - 1;
        longs &= longs - 1;
        const int b0 = __shfl(e0, src, 64), b1 = b0 + __shfl(len, src, 64);
        const int hl = __shfl(hd, src, 64);
        const float adr = __shfl(ad, src, 64);
        const int t_l = __shfl(t, src, 64);
        float dot = 0.f;
        for (int e = b0 + lane; e < b1; e += 64) dot += alpha[e * Hd + hl] * dalpha[e * Hd + hl];
        dot = wave_sum(dot);
        float acc = 0.f;
        for (int e = b0 + lane; e < b1; e += 64) {
            const float sv = a_src[col[e] * Hd + hl] + adr;
            const float d = alpha[e * Hd + hl] * (dalpha[e * Hd + hl] - dot) * (sv > 0.f ? 1.0f : slope);
            ds[e * Hd + hl] = d;
            acc += d;
        }
        acc = wave_sum(acc);
        if (lane == 0) da_dst[t_l] = acc;
    }
}

inline dim3 wave_grid(int32_t n) { return dim3((unsigned)(((int64_t)n * 64 + 255) / 256)); }
inline dim3 thread_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

constexpr int64_t kIndexLimit = (int64_t)1 << 31;
constexpr int kRegisterWidth = 1024;   // W a wave holds in registers (MAXV = 4, as gat_sddmm_kernel)

// sizes every entry point refuses: 32-bit indices n * heads + hd, e * heads + hd and heads * C + c must exist
inline bool bad_sizes(int32_t n, int64_t nnz, int32_t heads, int32_t C) {
    return n < 0 || nnz < 0 || heads < 1 || C < 1 || (int64_t)heads * C >= kIndexLimit || (int64_t)n * heads >= kIndexLimit ||
           nnz >= kIndexLimit || nnz * heads >= kIndexLimit;
}
inline bool pow2(int32_t v) { return v > 0 && (v & (v - 1)) == 0; }
inline bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16) == 0;
}

}  // namespace

extern "C" int fitgnn_gat_heads_scores_f32(const float *h, int64_t ldh, int32_t n, int32_t heads, int32_t C, const float *att_src,
                                           const float *att_dst, float *a_src, float *a_dst, void *stream) {
    if (bad_sizes(n, 0, heads, C) || ldh < (int64_t)heads * C) return FITGNN_E_BADARG;
    if (n == 0) return 0;
    if (!h || !att_src || !att_dst || !a_src || !a_dst) return FITGNN_E_BADARG;
    const bool vec = (C % 4 == 0) && pow2(C / 4) && (ldh % 4 == 0) && aligned16(h, att_src, att_dst);
    hipLaunchKernelGGL(gat_heads_scores_kernel, wave_grid(n), dim3(256), 0, (hipStream_t)stream, h, ldh, n, heads, C, att_src, att_dst,
                       a_src, a_dst, vec);
    return (int)hipGetLastError();
}

extern "C" int fitgnn_gat_heads_edge_softmax_f32(const int32_t *rowptr, const int32_t *col, const float *a_src, const float *a_dst,
                                                 float negative_slope, int32_t n, int64_t nnz, int32_t heads, float *alpha, void *stream) {
    if (bad_sizes(n, nnz, heads, 1)) return FITGNN_E_BADARG;
    if (n == 0) return 0;
    if (!rowptr || !a_src || !a_dst || (nnz > 0 && (!col || !alpha))) return FITGNN_E_BADARG;
    hipLaunchKernelGGL(gat_heads_edge_softmax_kernel, thread_grid((int64_t)n * heads), dim3(256), 0, (hipStream_t)stream, rowptr, col, a_src,
                       a_dst, negative_slope, n, heads, alpha);
    return (int)hipGetLastError();
}

extern "C" int fitgnn_gat_heads_aggregate_f32(const int32_t *rowptr, const int32_t *col, const float *alpha, const float *X, int64_t ldx,
                                              float *Y, int64_t ldy, int32_t n, int64_t nnz, int32_t heads, int32_t C, const float *bias,
                                              void *stream) {
    if (bad_sizes(n, nnz, heads, C) || ldx < (int64_t)heads * C || ldy < (int64_t)heads * C) return FITGNN_E_BADARG;
    if (n == 0) return 0;
    if (!rowptr || !X || !Y || (nnz > 0 && (!col || !alpha))) return FITGNN_E_BADARG;
    const int W = heads * C;
    const bool vec = (C % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && aligned16(X, Y) && W <= kRegisterWidth;
    hipStream_t s = (hipStream_t)stream;
    if (vec && W <= 256)
        hipLaunchKernelGGL(gat_heads_aggregate_kernel<1>, wave_grid(n), dim3(256), 0, s, rowptr, col, alpha, X, ldx, Y, ldy, n, heads, C, bias);
    else if (vec && W <= 512)
        hipLaunchKernelGGL(gat_heads_aggregate_kernel<2>, wave_grid(n), dim3(256), 0, s, rowptr, col, alpha, X, ldx, Y, ldy, n, heads, C, bias);
    else if (vec)
        hipLaunchKernelGGL(gat_heads_aggregate_kernel<4>, wave_grid(n), dim3(256), 0, s, rowptr, col, alpha, X, ldx, Y, ldy, n, heads, C, bias);
    else
        hipLaunchKernelGGL(gat_heads_aggregate_scalar_kernel, wave_grid(n), dim3(256), 0, s, rowptr, col, alpha, X, ldx, Y, ldy, n, heads, C,
                           bias);
    return (int)hipGetLastError();
}

extern "C" int fitgnn_gat_heads_sddmm_f32(const int32_t *rowptr, const int32_t *col, const float *dOut, int64_t ldo, const float *h,
                                          int64_t ldh, int32_t n, int64_t nnz, int32_t heads, int32_t C, float *dalpha, void *stream) {
    if (bad_sizes(n, nnz, heads, C) || ldo < (int64_t)heads * C || ldh < (int64_t)heads * C) return FITGNN_E_BADARG;
    if (n == 0) return 0;
    if (!rowptr || !dOut || !h || (nnz > 0 && (!col || !dalpha))) return FITGNN_E_BADARG;
    const int W = heads * C;
    const bool vec = (C % 4 == 0) && pow2(C / 4) && (ldo % 4 == 0) && (ldh % 4 == 0) && aligned16(dOut, h) && W <= kRegisterWidth;
    hipStream_t s = (hipStream_t)stream;
    if (vec && W <= 256)
        hipLaunchKernelGGL(gat_heads_sddmm_kernel<1>, wave_grid(n), dim3(256), 0, s, rowptr, col, dOut, ldo, h, ldh, n, heads, C, dalpha);
    else if (vec && W <= 512)
        hipLaunchKernelGGL(gat_heads_sddmm_kernel<2>, wave_grid(n), dim3(256), 0, s, rowptr, col, dOut, ldo, h, ldh, n, heads, C, dalpha);
    else if (vec)
        hipLaunchKernelGGL(gat_heads_sddmm_kernel<4>, wave_grid(n), dim3(256), 0, s, rowptr, col, dOut, ldo, h, ldh, n, heads, C, dalpha);
    else
        hipLaunchKernelGGL(gat_heads_sddmm_scalar_kernel, wave_grid(n), dim3(256), 0, s, rowptr, col, dOut, ldo, h, ldh, n, heads, C, dalpha);
    return (int)hipGetLastError();
}

extern "C" int fitgnn_gat_heads_softmax_bwd_f32(const int32_t *rowptr, const int32_t *col, const float *a_src, const float *a_dst,
                                                const float *alpha, const float *dalpha, float negative_slope, int32_t n, int64_t nnz,
                                                int32_t heads, float *ds, float *da_dst, void *stream) {
    if (bad_sizes(n, nnz, heads, 1)) return FITGNN_E_BADARG;
    if (n == 0) return 0;
    if (!rowptr || !a_src || !a_dst || !da_dst || (nnz > 0 && (!col || !alpha || !dalpha || !ds))) return FITGNN_E_BADARG;
    hipLaunchKernelGGL(gat_heads_softmax_bwd_kernel, thread_grid((int64_t)n * heads), dim3(256), 0, (hipStream_t)stream, rowptr, col, a_src,
                       a_dst, alpha, dalpha, negative_slope, n, heads, ds, da_dst);
    return (int)hipGetLastError();
}
