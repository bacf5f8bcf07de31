// match_arith.h -- per-element arithmetic of the matching methods and of the adjacency lift, shared by the multi-launch
// kernels (matching.hip, lift_pool.hip, coarsen.hip) and the whole-component kernel (match_small.hip).  One definition of
// every rounding step: the two paths are bit-identical because they run these functions, not restatements of them.
// Every function is evaluated without contraction (the reference evaluates one float64 operation at a time).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fitgnn_match {

// heavy_edge (:680-686): e_w / max(wmax_src, wmax_dst) with wmax = column maximum + 1e-5, rounded once to float32
__device__ __forceinline__ float heavy_edge_prox(double e_w, double wmax_src, double wmax_dst) {
#pragma clang fp contract(off)
    const double wi = wmax_src + 1e-5;
    const double wj = wmax_dst + 1e-5;
    const double m = wj > wi ? wj : wi;  // Python's max([wi, wj]): the first unless the second is larger
    return (float)(e_w / m);
}

// algebraic_JC (:689-698), one test vector: 1 / max((x_src - x_dst)^2, 1e-6); the proximity is the minimum over k, rounded
// once to float32 (min is exact and order-free)
__device__ __forceinline__ double jc_term(double x_src, double x_dst) {
#pragma clang fp contract(off)
    const double d = x_src - x_dst;
    const double d2 = d * d;
    return 1.0 / (d2 > 1e-6 ? d2 : 1e-6);
}

// Jacobi step (:836-846) of row i, one column: acc = sum_j w_ij x_j in CSR order (accumulated by the caller from 0.0);
// x <- 0.5 x + 0.5 Dinv (acc + (f32(dw) - dw) x) with the reference's float32 deg and deg^-1
__device__ __forceinline__ double jacobi_update(double acc, double xi, double dw) {
#pragma clang fp contract(off)
    const float degf = (float)dw;
    // f32 reciprocal computed in f64 and rounded once: the correctly rounded float32 1/deg
    const double dinv = degf == 0.0f ? 0.0 : (double)(float)(1.0 / (double)degf);
    const double mx = dinv * (acc + ((double)degf - dw) * xi);
    return 0.5 * xi + 0.5 * mx;
}
__device__ __forceinline__ double jacobi_acc(double acc, double w, double xj) {
#pragma clang fp contract(off)
    return acc + w * xj;
}

// sort key of an edge weight for the matching's rank (-weight ascending, then edge id): IEEE order of -weight as unsigned
// integers, -0 == +0, NaN last (numpy's argsort order)
__device__ __forceinline__ uint64_t match_sort_key(double weight) {
    const double v = -weight;
    if (v != v) return ~0ull;
    uint64_t b = (uint64_t)__double_as_longlong(v == 0.0 ? 0.0 : v);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

// value of C in the column of every member of a contracted set of nc nodes (coarsening_utils.py:168-179)
__device__ __forceinline__ double set_cval(int nc) {
#pragma clang fp contract(off)
    return 1.0 / sqrt((double)nc);
}

// the lift's Pinv weight of a node: p = c * (1 / c)
__device__ __forceinline__ double lift_p(double c) {
#pragma clang fp contract(off)
    return c * (1.0 / c);
}
__device__ __forceinline__ double lift_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double lift_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
// symmetrisation (Wc + Wc^T) / 2 of one entry (:139)
__device__ __forceinline__ double lift_sym(double ab, double ba) {
#pragma clang fp contract(off)
    return (ab + ba) / 2.0;
}

}  // namespace fitgnn_match
