// common.h -- small device helpers shared by the fitgnn HIP kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fitgnn {

// Counter-based dropout: one 64-bit hash per group of 4 consecutive elements (group g = (row*H + col) >> 2)
// yields 4 x 16 uniform bits; element (g, sub) is kept iff its 16 bits >= floor(p * 65536).
// Forward (spmm.hip) and backward (gcn_ops.hip) regenerate the same decisions; no mask is stored.
// FITGNN_EPI_SEED_DEVICE (= 8): `seed` carries a device pointer to the seed
__device__ __forceinline__ uint64_t resolve_seed(uint64_t seed, uint32_t epi) {
    return ((epi & 8u) && (epi & 4u)) ? *reinterpret_cast<const uint64_t *>(seed) : seed;
}

// Two 32-bit murmur3 finalisers over (group, seed) instead of one splitmix64: 64-bit multiplies cost the vector ALU four
// 32-bit ones each, and the hash sits in the epilogue of HBM-bound kernels (the forward SpMM, the epilogue-backward kernels, the
// dH @ W GEMM) where it was most of a row's arithmetic.
__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu;
    h ^= h >> 13; h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}
__host__ __device__ __forceinline__ uint64_t dropout_bits(uint64_t seed, uint64_t group) {
    const uint32_t g = (uint32_t)group * 0x9E3779B1u + (uint32_t)(group >> 32) * 0x85EBCA77u;
    const uint32_t lo = fmix32(g ^ (uint32_t)seed);
    const uint32_t hi = fmix32((g + 0x7F4A7C15u) ^ (uint32_t)(seed >> 32) ^ 0x68E31DA4u);
    return ((uint64_t)hi << 32) | lo;
}
__host__ __device__ __forceinline__ uint32_t dropout_threshold(float p) { return (uint32_t)(p * 65536.0f); }
__host__ __device__ __forceinline__ bool dropout_keep(uint64_t bits, int sub, uint32_t thresh) {
    return (uint32_t)((bits >> (16 * sub)) & 0xFFFFull) >= thresh;
}

// The keep decision of ONE element idx = row*H + col, for a thread that owns a single element of the group of four: only the 32-bit
// half of dropout_bits(seed, idx >> 2) that holds the element's 16 bits is hashed.  Same decision as dropout_keep on the whole hash.
__host__ __device__ __forceinline__ bool dropout_keep_elem(uint64_t seed, uint64_t idx, uint32_t thresh) {
    const uint64_t group = idx >> 2;
    const int sub = (int)(idx & 3);
    const uint32_t g = (uint32_t)group * 0x9E3779B1u + (uint32_t)(group >> 32) * 0x85EBCA77u;
    const uint32_t half = (sub & 2) ? fmix32((g + 0x7F4A7C15u) ^ (uint32_t)(seed >> 32) ^ 0x68E31DA4u) : fmix32(g ^ (uint32_t)seed);
    return ((half >> (16 * (sub & 1))) & 0xFFFFu) >= thresh;
}

// The forward store epilogue of one element (spmm.hip finish_row, gcn_ops.hip epilogue_fwd_rows_kernel: same flags, same arithmetic):
// dropout(ELU(x + bias)); idx = row*H + col of the element whose dropout hash / mask entry it takes.  epi bits: 1 bias, 2 ELU, 4 dropout.
__device__ __forceinline__ float finish_elem(float x, float bias, uint32_t epi, float keep_scale, uint32_t thresh, uint64_t seed,
                                             const uint8_t *__restrict__ mask, uint64_t idx) {
    float y = x + ((epi & 1u) ? bias : 0.f);
    if (epi & 2u) y = y > 0.f ? y : __expf(y) - 1.0f;
    if (epi & 4u) {
        const bool keep = mask ? (mask[idx] != 0) : dropout_keep_elem(seed, idx, thresh);
        y = keep ? y * keep_scale : 0.f;
    }
    return y;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// Cache policy of the GCN step's once-touched HBM streams: a stream whose bit is set in FITGNN_NT_STREAMS is loaded / stored with the
// non-temporal hint (global_load / global_store ... nt), the others with the default policy.  Everything re-read from L2 or the
// Infinity Cache (CSR, tile and block tables, compact operands, column-sum partials, gathered operand rows) keeps the default.
// The default mask holds the streams tools/nt_probe.py measured faster with nt (profiles/r05_nt_probe_S-products.log);
// `make EXTRA=-DFITGNN_NT_STREAMS=<mask>` builds another mix for the probe.
enum NtStream : uint32_t {
    kNtOutTable = 1u << 0,   // whole-subgraph SpMM over a row-indirected table (layer 0 forward): output row stores
    kNtOutPlain = 1u << 1,   // whole-subgraph SpMM, plain operand (layer 1 forward): output row stores
    kNtOutTwoHop = 1u << 2,  // two-hop backward: stores of G
    kNtWinPlain = 1u << 3,   // plain whole-subgraph launch: window staging loads of the dense operand
    kNtWinTwoHop = 1u << 4,  // two-hop launch: window staging loads (side-table rows and `prev` slices of simple rows)
    kNtPrev = 1u << 5,       // side-table kernel: its rows' `prev` slices, read once
    kNtWinTable = 1u << 6,   // layer-0 launch: window staging loads from the de-duplicated table (rows re-read ~50x)
    kNtSideStore = 1u << 7,  // side-table kernel: stores of ZT
    kNtSegLoad = 1u << 8,    // segment sum: member row loads
    kNtSegStore = 1u << 9,   // segment sum: output row stores
};
#ifndef FITGNN_NT_STREAMS
#define FITGNN_NT_STREAMS (fitgnn::kNtOutPlain | fitgnn::kNtOutTwoHop | fitgnn::kNtPrev | fitgnn::kNtSideStore | fitgnn::kNtSegLoad)
#endif
typedef float nt_f4 __attribute__((ext_vector_type(4)));
template <uint32_t S>
__device__ __forceinline__ float4 load4(const float *p) {
    if constexpr ((FITGNN_NT_STREAMS & S) != 0u) {
        const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4 *>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    } else {
        return *reinterpret_cast<const float4 *>(p);
    }
}
template <uint32_t S>
__device__ __forceinline__ void store4(float *p, const float4 &v) {
    if constexpr ((FITGNN_NT_STREAMS & S) != 0u) {
        __builtin_nontemporal_store(nt_f4{v.x, v.y, v.z, v.w}, reinterpret_cast<nt_f4 *>(p));
    } else {
        *reinterpret_cast<float4 *>(p) = v;
    }
}

}  // namespace fitgnn

// Raise a kernel's dynamic-LDS limit ONCE per process and device (done: one bit per device ordinal).  hipFuncSetAttribute is a
// host call into the runtime; issued before every launch it is a per-launch cost and a point where launches on different
// streams meet.
#include <atomic>
inline int fitgnn_lds_limit_once(const void *kernel, int bytes, std::atomic<uint64_t> &done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return 0;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    done.fetch_or(bit, std::memory_order_release);
    return 0;
}

#define FITGNN_RETURN_IF_HIP(expr)            \
    do {                                      \
        hipError_t _e = (expr);               \
        if (_e != hipSuccess) return (int)_e; \
    } while (0)
