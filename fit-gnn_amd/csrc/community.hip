// community.hip -- modularity community detection for --use_community_detection (the reference's main.py:257-258 runs
// leidenalg.find_partition(..., ModularityVertexPartition); DESIGN §4 "Community detection" states the rule built here): the
// local-move sweep of a multilevel Louvain scheme, the statistics its acceptance test reads, and the connectivity finish.
//
//   sweep        per active node a hash table keyed by neighbour community (int32 sums, integer atomics), every slot scored in
//                int64, reduced in the order (score descending, community id ascending).  Three launch branches by row length.
//   stats        tot[], size[], moved, sum of in[c], sum of tot[c]^2 of a labelling: what the host needs to accept a sweep
//   components   label[i] = min over same-community neighbours, then pointer jumping, until a pass changes nothing
//
// All arithmetic is integer and every atomic is an integer add, min, max or compare-and-swap whose outcome does not depend on
// the order of arrival: two runs give identical bytes.  With M2 < 2^31 each product of a score is below 2^62.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "common.h"
#include "fitgnn_hip.h"

namespace {

// The launch branches of the sweep, by row length d.  Both cut-offs are unmeasured guesses.
constexpr int kWaveMaxRow = 128;            // d <= : one wavefront per node, table in LDS per wave
constexpr int kBlockMaxRow = 4096;          // d <= : one workgroup per node, table in LDS (64 KiB); longer: table in the workspace
constexpr int kWaveSlots = 2 * kWaveMaxRow;    // a table has 2 * pow2ceil(d) >= 2 d slots: probing ends at an empty slot
constexpr int kBlockSlots = 2 * kBlockMaxRow;
constexpr int kGlobalTables = 16;           // workgroups of the long-row branch in flight, one workspace table each
constexpr int kMaxRowLimit = 1 << 30;       // 2 * pow2ceil(d) must fit 32 bits
constexpr int kStatsBlocks = 4096;
constexpr int kMaxChunk = 64;               // component passes launched between two reads of their flags

constexpr size_t kAlign = 256;
inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }
inline int64_t pow2ceil_host(int64_t d) {
    int64_t p = 1;
    while (p < d) p <<= 1;
    return p;
}

constexpr int32_t kEmpty = -1;
constexpr int32_t kNoComm = INT32_MAX;
constexpr int64_t kNoScore = INT64_MIN;

__device__ __forceinline__ uint32_t pow2ceil(uint32_t d) { return d <= 1 ? 1u : 1u << (32 - __clz(d - 1)); }
__device__ __forceinline__ uint32_t slot_of(int32_t c, int bits) { return ((uint32_t)c * 2654435761u) >> (32 - bits); }
__device__ __forceinline__ bool is_active(int32_t i, int32_t t) { return (((uint32_t)i + (uint32_t)t) & 1u) == 0; }  // (i + t) even
__device__ __forceinline__ bool better(int64_t s1, int32_t c1, int64_t s2, int32_t c2) { return s1 > s2 || (s1 == s2 && c1 < c2); }
__device__ __forceinline__ int32_t load_agent(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ------------------------------------------------------------------------------------------------
// sweep
// ------------------------------------------------------------------------------------------------
struct SweepArgs {
    const int32_t *rowptr, *col, *w, *k, *comm, *tot, *size;
    int64_t M2;
    int32_t t;
    const int32_t *list;
    int32_t n_list;
    int32_t *comm_out;
};

// what a node brings to its scores
struct Node {
    int32_t i, a, k_i, tot_a, size_a, begin, end, bits;
    uint32_t slots;
};
__device__ __forceinline__ Node load_node(const SweepArgs &A, int32_t i) {
    Node n;
    n.i = i;
    n.a = A.comm[i];
    n.k_i = A.k[i];
    n.tot_a = A.tot[n.a];
    n.size_a = A.size[n.a];
    n.begin = A.rowptr[i];
    n.end = A.rowptr[i + 1];
    n.slots = 2 * pow2ceil((uint32_t)(n.end - n.begin));
    n.bits = 31 - __clz(n.slots);
    return n;
}

template <bool GLOBAL>
__device__ __forceinline__ void table_clear(int32_t *keys, int32_t *sums, uint32_t slots, int tid, int threads) {
    for (uint32_t s = tid; s < slots; s += threads) {
        keys[s] = kEmpty;
        sums[s] = 0;
    }
    if (GLOBAL) __threadfence();  // the stores are in L2 before another thread's atomic meets them
}

// acc[comm[j]] += w_ij over the row's off-diagonal entries
template <bool GLOBAL>
__device__ __forceinline__ void table_fill(const SweepArgs &A, const Node &n, int32_t *keys, int32_t *sums, int tid, int threads) {
    const uint32_t mask = n.slots - 1;
    for (int p = n.begin + tid; p < n.end; p += threads) {
        const int32_t j = A.col[p];
        if (j == n.i) continue;
        const int32_t c = A.comm[j], wij = A.w ? A.w[p] : 1;
        for (uint32_t h = slot_of(c, n.bits);; h = (h + 1) & mask) {
            const int32_t prev = atomicCAS(&keys[h], kEmpty, c);
            if (prev == kEmpty || prev == c) {
                atomicAdd(&sums[h], wij);
                break;
            }
        }
    }
    if (GLOBAL) __threadfence();
}

// this thread's best candidate among its slots, and acc[a] if one of them holds the node's own community
template <bool GLOBAL>
__device__ __forceinline__ void table_score(const SweepArgs &A, const Node &n, const int32_t *keys, const int32_t *sums, int tid, int threads,
                                            int64_t &best_s, int32_t &best_c, int32_t &acc_a) {
    best_s = kNoScore;
    best_c = kNoComm;
    acc_a = 0;
    for (uint32_t s = tid; s < n.slots; s += threads) {
        const int32_t c = GLOBAL ? load_agent(&keys[s]) : keys[s];
        if (c == kEmpty) continue;
        const int32_t acc = GLOBAL ? load_agent(&sums[s]) : sums[s];
        if (c == n.a) {
            acc_a = acc;
            continue;
        }
        if (n.size_a == 1 && c > n.a && A.size[c] == 1) continue;  // two singletons do not swap
        const int64_t sc = A.M2 * (int64_t)acc - (int64_t)n.k_i * (int64_t)A.tot[c];
        if (better(sc, c, best_s, best_c)) {
            best_s = sc;
            best_c = c;
        }
    }
}

__device__ __forceinline__ void wave_best(int64_t &s, int32_t &c, int32_t &acc_a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t s2 = __shfl_xor(s, off, 64);
        const int32_t c2 = __shfl_xor(c, off, 64);
        if (better(s2, c2, s, c)) {
            s = s2;
            c = c2;
        }
        acc_a += __shfl_xor(acc_a, off, 64);
    }
}

__device__ __forceinline__ void decide(const SweepArgs &A, const Node &n, int64_t best_s, int32_t best_c, int32_t acc_a) {
    const int64_t s_a = A.M2 * (int64_t)acc_a - (int64_t)n.k_i * ((int64_t)n.tot_a - (int64_t)n.k_i);
    if (best_c != kNoComm && best_s > s_a) A.comm_out[n.i] = best_c;
}

// d <= kWaveMaxRow: four nodes per workgroup, one wavefront and one table each.  The barriers are the workgroup's: every wave
// runs the same three phases whether or not its node is active.
__global__ __launch_bounds__(256) void louvain_sweep_wave_kernel(SweepArgs A) {
    __shared__ int32_t keys_s[4][kWaveSlots];
    __shared__ int32_t sums_s[4][kWaveSlots];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + wave;
    const int32_t i = idx < A.n_list ? A.list[idx] : -1;
    bool active = i >= 0 && is_active(i, A.t);
    Node n{};
    if (active) {
        n = load_node(A, i);
        active = n.slots <= (uint32_t)kWaveSlots;
    }
    int32_t *keys = keys_s[wave], *sums = sums_s[wave];
    if (active) table_clear<false>(keys, sums, n.slots, lane, 64);
    __syncthreads();
    if (active) table_fill<false>(A, n, keys, sums, lane, 64);
    __syncthreads();
    if (!active) return;
    int64_t best_s;
    int32_t best_c, acc_a;
    table_score<false>(A, n, keys, sums, lane, 64, best_s, best_c, acc_a);
    wave_best(best_s, best_c, acc_a);
    if (lane == 0) decide(A, n, best_s, best_c, acc_a);
}

// the four waves' results meet in LDS; thread 0 decides
__device__ __forceinline__ void block_decide(const SweepArgs &A, const Node &n, int64_t best_s, int32_t best_c, int32_t acc_a, int64_t *red_s,
                                             int32_t *red_c, int32_t *red_a) {
    wave_best(best_s, best_c, acc_a);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        red_s[wave] = best_s;
        red_c[wave] = best_c;
        red_a[wave] = acc_a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < 4; ++v) {
            if (better(red_s[v], red_c[v], best_s, best_c)) {
                best_s = red_s[v];
                best_c = red_c[v];
            }
            acc_a += red_a[v];
        }
        decide(A, n, best_s, best_c, acc_a);
    }
}

// kWaveMaxRow < d <= kBlockMaxRow: one workgroup per node, the table in LDS (64 KiB: two workgroups per CU)
__global__ __launch_bounds__(256) void louvain_sweep_block_kernel(SweepArgs A) {
    __shared__ int32_t keys[kBlockSlots];
    __shared__ int32_t sums[kBlockSlots];
    __shared__ int64_t red_s[4];
    __shared__ int32_t red_c[4], red_a[4];
    const int32_t i = A.list[blockIdx.x];
    if (!is_active(i, A.t)) return;  // the whole workgroup
    const Node n = load_node(A, i);
    if (n.slots > (uint32_t)kBlockSlots) return;
    table_clear<false>(keys, sums, n.slots, threadIdx.x, 256);
    __syncthreads();
    table_fill<false>(A, n, keys, sums, threadIdx.x, 256);
    __syncthreads();
    int64_t best_s;
    int32_t best_c, acc_a;
    table_score<false>(A, n, keys, sums, threadIdx.x, 256, best_s, best_c, acc_a);
    block_decide(A, n, best_s, best_c, acc_a, red_s, red_c, red_a);
}

// d > kBlockMaxRow: a workgroup walks its share of the long rows with one table of table_slots slots in the workspace (global
// atomics; read back at agent scope, past this CU's vector cache)
__global__ __launch_bounds__(256) void louvain_sweep_global_kernel(SweepArgs A, int32_t *tables, uint32_t table_slots) {
    __shared__ int64_t red_s[4];
    __shared__ int32_t red_c[4], red_a[4];
    int32_t *keys = tables + (size_t)blockIdx.x * 2 * table_slots, *sums = keys + table_slots;
    for (int32_t idx = blockIdx.x; idx < A.n_list; idx += gridDim.x) {
        const int32_t i = A.list[idx];
        if (!is_active(i, A.t)) continue;
        const Node n = load_node(A, i);
        if (n.slots > table_slots) continue;
        table_clear<true>(keys, sums, n.slots, threadIdx.x, 256);
        __syncthreads();
        table_fill<true>(A, n, keys, sums, threadIdx.x, 256);
        __syncthreads();
        int64_t best_s;
        int32_t best_c, acc_a;
        table_score<true>(A, n, keys, sums, threadIdx.x, 256, best_s, best_c, acc_a);
        block_decide(A, n, best_s, best_c, acc_a, red_s, red_c, red_a);
        __syncthreads();  // the table and red_* are free again
    }
}

// rows by branch, once per level: lists[b * N ..] = the rows of branch b in any order (a node's result does not depend on its
// place in a list), counts[0..2] their numbers, counts[3] the longest row.  Rows without entries are in no list.
__global__ __launch_bounds__(256) void louvain_bucket_kernel(const int32_t *__restrict__ rowptr, int64_t N, int32_t *__restrict__ lists,
                                                             int32_t *__restrict__ counts) {
    __shared__ int32_t cnt[3], base[3], longest;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t d = i < N ? rowptr[i + 1] - rowptr[i] : 0;
    const int b = d <= 0 ? -1 : d <= kWaveMaxRow ? 0 : d <= kBlockMaxRow ? 1 : 2;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    if (threadIdx.x == 3) longest = 0;
    __syncthreads();
    const int32_t r = b >= 0 ? atomicAdd(&cnt[b], 1) : 0;
    if (d > 0) atomicMax(&longest, d);
    __syncthreads();
    if (threadIdx.x < 3) base[threadIdx.x] = cnt[threadIdx.x] ? atomicAdd(&counts[threadIdx.x], cnt[threadIdx.x]) : 0;
    if (threadIdx.x == 3 && longest) atomicMax(&counts[3], longest);
    __syncthreads();
    if (b >= 0) lists[(int64_t)b * N + base[b] + r] = (int32_t)i;
}

struct SweepLayout {
    size_t counts, lists, tables, total;
    uint32_t table_slots;
};
SweepLayout sweep_layout(int64_t N, int32_t max_row) {
    SweepLayout L{};
    size_t o = 0;
    const size_t n = (size_t)(N > 0 ? N : 1);
    L.counts = o; o += align_up(4 * sizeof(int32_t));
    L.lists = o; o += align_up(3 * n * sizeof(int32_t));
    L.tables = o;
    if (max_row > kBlockMaxRow) {
        L.table_slots = (uint32_t)(2 * pow2ceil_host(max_row));
        o += align_up((size_t)std::min<int64_t>(kGlobalTables, N) * 2 * L.table_slots * sizeof(int32_t));
    }
    L.total = o;
    return L;
}
inline bool sizes_ok(int64_t N, int64_t max_row) { return N >= 0 && N <= INT32_MAX && max_row >= 0 && max_row <= kMaxRowLimit && max_row <= N; }

// ------------------------------------------------------------------------------------------------
// stats
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// the workgroup's sum, added to *dst by one atomic
__device__ __forceinline__ void block_add(int64_t v, int64_t *red, int64_t *dst) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t s = red[0] + red[1] + red[2] + red[3];
        if (s) atomicAdd((unsigned long long *)dst, (unsigned long long)s);
    }
    __syncthreads();
}

// one wavefront per row, rows dealt round-robin over a fixed grid: tot / size by 32-bit atomics (tot <= M2 < 2^31), moved and
// sum of in[c] gathered per workgroup.  out = {moved, sum in, sum tot^2}
__global__ __launch_bounds__(256) void louvain_stats_rows_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                 const int32_t *__restrict__ w, const int32_t *__restrict__ k, int64_t N,
                                                                 const int32_t *__restrict__ comm, const int32_t *__restrict__ snapshot,
                                                                 int32_t *__restrict__ tot, int32_t *__restrict__ size, int64_t *__restrict__ out) {
    __shared__ int64_t red[4];
    const int lane = threadIdx.x & 63;
    int64_t moved = 0, in = 0;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < N; i += (int64_t)gridDim.x * 4) {
        const int32_t c = comm[i];
        if (lane == 0) {
            atomicAdd(&tot[c], k[i]);
            atomicAdd(&size[c], 1);
            moved += c != snapshot[i];
        }
        for (int p = rowptr[i] + lane; p < rowptr[i + 1]; p += 64)
            if (comm[col[p]] == c) in += w ? w[p] : 1;
    }
    block_add(moved, red, out);
    block_add(in, red, out + 1);
}
__global__ __launch_bounds__(256) void louvain_stats_tot2_kernel(const int32_t *__restrict__ tot, int64_t N, int64_t *__restrict__ out) {
    __shared__ int64_t red[4];
    int64_t s = 0;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < N; c += (int64_t)gridDim.x * 256) s += (int64_t)tot[c] * tot[c];
    block_add(s, red, out + 2);
}

// ------------------------------------------------------------------------------------------------
// components
// ------------------------------------------------------------------------------------------------
__global__ void label_init_kernel(int64_t N, int32_t *__restrict__ label) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) label[i] = (int32_t)i;
}
// label[i] = min(label[i], label[j]) over the neighbours j in i's community; the node's current representative takes the same
// minimum (a member of the same piece).  One wavefront per row.  Labels only fall and stay member ids of the node's piece.
__global__ __launch_bounds__(256) void components_hook_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t N,
                                                              const int32_t *__restrict__ comm, int32_t *label, int32_t *__restrict__ flag) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < N; i += (int64_t)gridDim.x * 4) {
        const int32_t c = comm[i], li = load_agent(&label[i]);
        int32_t m = li;
        for (int p = rowptr[i] + lane; p < rowptr[i + 1]; p += 64) {
            const int32_t j = col[p];
            if (j != i && comm[j] == c) m = min(m, load_agent(&label[j]));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off, 64));
        if (lane == 0 && m < li) {
            atomicMin(&label[i], m);
            atomicMin(&label[li], m);
            *flag = 1;
        }
    }
}
// pointer jumping: label[i] = the end of its chain (label[r] == r).  A chain strictly falls, so the walk ends.
__global__ void components_jump_kernel(int64_t N, int32_t *label) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int32_t l = load_agent(&label[i]);
    for (int32_t nx = load_agent(&label[l]); nx < l; nx = load_agent(&label[l])) l = nx;
    __hip_atomic_store(&label[i], l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

inline dim3 blocks_for(int64_t threads, int block = 256) { return dim3((unsigned)((threads + block - 1) / block)); }
inline dim3 row_grid(int64_t N) { return dim3((unsigned)std::min<int64_t>((N + 3) / 4, kStatsBlocks)); }

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" size_t fitgnn_louvain_sweep_workspace_bytes(int64_t N, int32_t max_row) {
    if (!sizes_ok(N, max_row)) return 0;
    return sweep_layout(N, max_row).total;
}

extern "C" int fitgnn_louvain_bucket_rows(const int32_t *rowptr, int64_t N, int32_t max_row, int32_t *counts, void *work, size_t work_bytes,
                                          void *stream) {
    if (!sizes_ok(N, max_row) || !counts) return FITGNN_E_BADARG;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (N == 0) return 0;
    if (!rowptr || !work) return FITGNN_E_BADARG;
    const SweepLayout L = sweep_layout(N, max_row);
    if (work_bytes < L.total) return FITGNN_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *base = (char *)work;
    int32_t *d_counts = (int32_t *)(base + L.counts);
    FITGNN_RETURN_IF_HIP(hipMemsetAsync(d_counts, 0, 4 * sizeof(int32_t), s));
    hipLaunchKernelGGL(louvain_bucket_kernel, blocks_for(N), dim3(256), 0, s, rowptr, N, (int32_t *)(base + L.lists), d_counts);
    FITGNN_RETURN_IF_HIP(hipGetLastError());
    FITGNN_RETURN_IF_HIP(hipMemcpyAsync(counts, d_counts, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    FITGNN_RETURN_IF_HIP(hipStreamSynchronize(s));
    return counts[3] > max_row ? FITGNN_E_BADARG : 0;  // the workspace was sized for shorter rows
}

extern "C" int fitgnn_louvain_sweep(const int32_t *rowptr, const int32_t *col, const int32_t *w, const int32_t *k, int64_t N, int64_t M2,
                                    const int32_t *comm, const int32_t *tot, const int32_t *size, int32_t t, const int32_t *counts,
                                    int32_t max_row, int32_t *comm_out, void *work, size_t work_bytes, void *stream) {
    if (!sizes_ok(N, max_row) || M2 < 0 || M2 > INT32_MAX || t < 0 || !counts) return FITGNN_E_BADARG;
    if (N == 0) return 0;
    if (!rowptr || !col || !k || !comm || !tot || !size || !comm_out || comm == comm_out || !work) return FITGNN_E_BADARG;
    const int64_t n_wave = counts[0], n_block = counts[1], n_global = counts[2];
    if (n_wave < 0 || n_block < 0 || n_global < 0 || n_wave + n_block + n_global > N || counts[3] > max_row) return FITGNN_E_BADARG;
    const SweepLayout L = sweep_layout(N, max_row);
    if (work_bytes < L.total) return FITGNN_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char *base = (char *)work;
    const int32_t *lists = (const int32_t *)(base + L.lists);
    FITGNN_RETURN_IF_HIP(hipMemcpyAsync(comm_out, comm, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, s));  // who does not move
    SweepArgs A{rowptr, col, w, k, comm, tot, size, M2, t, lists, (int32_t)n_wave, comm_out};
    if (n_wave) hipLaunchKernelGGL(louvain_sweep_wave_kernel, blocks_for(n_wave, 4), dim3(256), 0, s, A);
    if (n_block) {
        A.list = lists + N;
        A.n_list = (int32_t)n_block;
        hipLaunchKernelGGL(louvain_sweep_block_kernel, dim3((unsigned)n_block), dim3(256), 0, s, A);
    }
    if (n_global) {
        if (!L.table_slots) return FITGNN_E_BADARG;
        A.list = lists + 2 * N;
        A.n_list = (int32_t)n_global;
        hipLaunchKernelGGL(louvain_sweep_global_kernel, dim3((unsigned)std::min<int64_t>(n_global, std::min<int64_t>(kGlobalTables, N))), dim3(256),
                           0, s, A, (int32_t *)(base + L.tables), L.table_slots);
    }
    return (int)hipGetLastError();
}

extern "C" int fitgnn_louvain_stats(const int32_t *rowptr, const int32_t *col, const int32_t *w, const int32_t *k, int64_t N, int64_t M2,
                                    const int32_t *comm, const int32_t *snapshot, int32_t *tot, int32_t *size, int64_t *out, void *stream) {
    if (N < 0 || N > INT32_MAX || M2 < 0 || M2 > INT32_MAX || !out) return FITGNN_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (N > 0 && (!rowptr || !col || !k || !comm || !snapshot || !tot || !size)) return FITGNN_E_BADARG;
    FITGNN_RETURN_IF_HIP(hipMemsetAsync(out, 0, 3 * sizeof(int64_t), s));
    if (N == 0) return 0;
    FITGNN_RETURN_IF_HIP(hipMemsetAsync(tot, 0, (size_t)N * sizeof(int32_t), s));
    FITGNN_RETURN_IF_HIP(hipMemsetAsync(size, 0, (size_t)N * sizeof(int32_t), s));
    hipLaunchKernelGGL(louvain_stats_rows_kernel, row_grid(N), dim3(256), 0, s, rowptr, col, w, k, N, comm, snapshot, tot, size, out);
    hipLaunchKernelGGL(louvain_stats_tot2_kernel, dim3((unsigned)std::min<int64_t>((N + 255) / 256, kStatsBlocks)), dim3(256), 0, s, tot, N, out);
    return (int)hipGetLastError();
}

extern "C" size_t fitgnn_louvain_components_workspace_bytes(int64_t N) {
    if (N < 0 || N > INT32_MAX) return 0;
    return align_up(kMaxChunk * sizeof(int32_t));
}

extern "C" int fitgnn_louvain_components(const int32_t *rowptr, const int32_t *col, int64_t N, const int32_t *comm, int32_t *label,
                                         int32_t *passes, void *work, size_t work_bytes, void *stream) {
    if (N < 0 || N > INT32_MAX) return FITGNN_E_BADARG;
    if (passes) *passes = 0;
    if (N == 0) return 0;
    if (!rowptr || !col || !comm || !label || !work) return FITGNN_E_BADARG;
    if (work_bytes < fitgnn_louvain_components_workspace_bytes(N)) return FITGNN_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int32_t *flags = (int32_t *)work;
    hipLaunchKernelGGL(label_init_kernel, blocks_for(N), dim3(256), 0, s, N, label);
    // The host reads the passes' "something fell" flags after chunks of 1, 2, 4 .. 64 passes; a pass past the fixed point changes
    // nothing.  Every live pass lowers a label, and labels are bounded below: at most N passes in all.
    int32_t flags_h[kMaxChunk];
    int64_t n_passes = 0;
    for (int chunk = 1;; chunk = std::min(2 * chunk, kMaxChunk)) {
        FITGNN_RETURN_IF_HIP(hipMemsetAsync(flags, 0, (size_t)chunk * sizeof(int32_t), s));
        for (int p = 0; p < chunk; ++p) {
            hipLaunchKernelGGL(components_hook_kernel, row_grid(N), dim3(256), 0, s, rowptr, col, N, comm, label, flags + p);
            hipLaunchKernelGGL(components_jump_kernel, blocks_for(N), dim3(256), 0, s, N, label);
        }
        FITGNN_RETURN_IF_HIP(hipGetLastError());
        FITGNN_RETURN_IF_HIP(hipMemcpyAsync(flags_h, flags, (size_t)chunk * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        FITGNN_RETURN_IF_HIP(hipStreamSynchronize(s));
        int live = 0;
        while (live < chunk && flags_h[live]) ++live;
        n_passes += live;
        if (live < chunk) break;
        if (n_passes > N + 2) return FITGNN_E_BADARG;  // impossible: labels only fall; never spin
    }
    if (passes) *passes = (int32_t)std::min<int64_t>(n_passes, INT32_MAX);
    return 0;
}
