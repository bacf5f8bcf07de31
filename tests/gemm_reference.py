"""Float64 references, derived error bounds, fp32 emulations and plan models of the dense GEMM kernels (test infrastructure only):
csrc/gemm_f32.hip (the `exact` product on v_mfma_f32_32x32x2_f32), csrc/gemm_nt.hip and csrc/gemm_atb.hip (three bf16 products of a
two-term split).  tests/test_gemm_reference_cpu.py checks the emulations against the bounds and the case list of
tests/test_gpu_gemm_kernels.py against the plan model.

Operand forms of the `exact` product c[I x J] (the kernel's "k-minor" = k contiguous, "k-major" = k is the row index):
    nt   a [I x K], b [J x K]     c = a b^T       (forward of a Linear)
    nn   a [I x K], b [K x J]     c = a b         (input gradient)
    tn   a [K x I], b [K x J]     c = a^T b       (weight gradient, split over k)

Bounds, u = 2^-24, first order, S[i][j] = sum_k |a_ik| |b_kj| (per entry, never the output's largest value), no allowance on top.

* `exact`, one launch.  v_mfma_f32_32x32x2_f32 multiplies fp32 operands exactly and adds each product to the fp32 accumulator with
  one rounding: an fmaf chain of K links (within an octet of k the kernel's order is 0, 4, 1, 5, 2, 6, 3, 7: a lane half holds four
  consecutive k; the bound does not depend on the order).  Link t rounds the partial sum s_t, |s_t| <= sum_{k <= t} |a_k b_k| <= S,
  so |c - c64| <= K u S.
* `exact`, split over k (nchunks > 1, or the tail launch's rows with 8 chunks).  Chunk c is a chain of at most chunk_k links over
  its own terms, S_c: sum_c chunk_k u S_c = chunk_k u S.  sum_chunks_kernel adds the partials into eight running sums (partial 8 q +
  r into sum r; the first addition is to zero and exact: ceil(nchunks / 8) - 1 roundings), then adds the eight sums in order (seven
  roundings); every intermediate is at most S in magnitude.  |c - c64| <= (chunk_k + ceil(nchunks / 8) + 6) u S.
* bf16 three-product split.  The kernels split x into hi = bf16_rne(x) (csrc/gemm_nt.hip and csrc/gemm_atb.hip both convert with
  __builtin_convertvector, round to nearest even; the header comment of gemm_atb.hip said truncation until it was corrected with
  these tests) and lo = bf16_rne(x - hi); x - hi is exact in fp32 either way.  With |x - hi| <= d |x| (d = 2^-8 for rounding, 2^-7
  for truncation) and lo rounded to 8 significant bits, x = hi + lo + e with |e| <= 2^-9 d |x| and |lo| <= (1 + 2^-9) d |x|.
  a b - (ha hb + ha lb + la hb) = la lb + ea b + eb a - ea eb, so per product
      |dropped| <= (d^2 (1 + 2^-9)^2 + 2^-8 d + 2^-18 d^2) |a| |b| =: c_split(d) |a| |b|          (d = 2^-8: 3.06e-5)
  Products of two bf16 are exact in fp32.  The 3 K terms of an entry are accumulated in fp32 in the MFMA's own order; any order of
  n - 1 fp32 additions errs by at most (n - 1) u (sum of |terms|), and sum of |terms| <= T(d) S with
  T(d) = (1 + d)^2 + 2 (1 + d)(1 + 2^-9) d.   gemm_nt:  |c - c64| <= (c_split + 3 K u T) S.
  gemm_atb (rows split into nchunks chunks of chunk_rows, then atb_reduce_kernel: eight running sums, seven additions, and the last
  R % 32 rows as acc += a * b in fp32, two roundings per row):
      |c - c64| <= (c_split + (3 chunk_rows + nchunks / 8 + 6) u T + 2 (R % 32) u) S.

EXACT inputs (test_gpu_step_kernels._exact: integers in [-8, 8] over 64) have four significant bits, so hi = x, lo = 0, every product
is a multiple of 2^-12 and every partial sum, in any order, is a multiple of 2^-12 of magnitude at most S: exact in fp32 while
S 2^12 < 2^24 (product_is_exact).  |a| |b| <= 2^-6 per term, so this holds for K < 2^18.
"""
import math

import numpy as np

U = 2.0 ** -24
KBK = 32   # k per stage of gemm_f32.hip; rows per stage of gemm_atb.hip and gemm_nt.hip

# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------------------
FORMS = ("nt", "nn", "tn")
KMAJOR = {"nt": (0, 0), "nn": (0, 1), "tn": (1, 1)}   # (a_kmajor, b_kmajor)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def as_ik_kj(a, b, form):
    """(a as [I x K], b as [K x J]) views of the operands of a form."""
    a, b = np.asarray(a), np.asarray(b)
    return (a.T if form == "tn" else a), (b.T if form == "nt" else b)


def operand_shapes(form, I, J, K):
    """Shapes in memory of (a, b)."""
    return ((K, I) if form == "tn" else (I, K)), ((J, K) if form == "nt" else (K, J))


def product(a, b, form):
    """(c, S): the float64 product and the per-entry condition sum |a| |b|."""
    A, B = as_ik_kj(a, b, form)
    A, B = _f64(A), _f64(B)
    return A @ B, np.abs(A) @ np.abs(B)


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds (module docstring)
# ---------------------------------------------------------------------------------------------------------------------------------
def exact_links(K, nchunks=1, chunk_k=None):
    """Roundings on the longest path of an entry of the `exact` product."""
    if nchunks <= 1:
        return int(K)
    return int(chunk_k) + -(-int(nchunks) // 8) + 6


def exact_bound(S, K, nchunks=1, chunk_k=None):
    return exact_links(K, nchunks, chunk_k) * U * _f64(S)


def exact_bound_plan(S, K, plan):
    """Per entry, for a plan of plan_exact: the rows of a tail launch are split eight ways."""
    S = _f64(S)
    bound = exact_bound(S, K, plan.nchunks, plan.chunk_k)
    if plan.main_rows > 0:
        bound = bound.copy()
        bound[plan.main_rows:] = exact_bound(S[plan.main_rows:], K, plan.rem_chunks, plan.rem_chunk_k)
    return bound


D_RNE, D_TRUNC = 2.0 ** -8, 2.0 ** -7


def split_dropped(d=D_RNE):
    return d * d * (1 + 2.0 ** -9) ** 2 + 2.0 ** -8 * d + 2.0 ** -18 * d * d


def split_terms(d=D_RNE):
    return (1 + d) ** 2 + 2 * (1 + d) * (1 + 2.0 ** -9) * d


def nt_bound(S, K, d=D_RNE):
    return (split_dropped(d) + 3 * int(K) * U * split_terms(d)) * _f64(S)


def atb_bound(S, R, plan, d=D_RNE):
    adds = 3 * plan.chunk_rows + plan.nchunks // 8 + 6
    return (split_dropped(d) + adds * U * split_terms(d) + 2 * (int(R) % KBK) * U) * _f64(S)


def product_is_exact(S):
    """Per entry, from the float64 condition sum of EXACT operands: no partial sum of the entry's products, in any order, can have
    rounded in fp32 (multiples of 2^-12 below 2^12).  Every EXACT case must satisfy it; it is never a reason to skip one."""
    return _f64(S) * 2.0 ** 12 < 2.0 ** 24


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 emulations
# ---------------------------------------------------------------------------------------------------------------------------------
def _f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bf16_trunc(x):
    """The upper 16 bits of fp32 x, as fp32."""
    return (_f32_bits(x) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_rne(x):
    """fp32 x rounded to the nearest bf16 (ties to even), as fp32 (finite x)."""
    bits = _f32_bits(x).astype(np.uint64)
    bits = bits + np.uint64(0x7FFF) + ((bits >> np.uint64(16)) & np.uint64(1))
    return (bits & np.uint64(0xFFFF0000)).astype(np.uint32).view(np.float32)


def split_bf16(x, hi="rne"):
    """(hi, lo) of the kernels' two-term split: hi = bf16_rne(x) as the kernels convert it (hi='trunc': the upper 16 bits, the form
    the bound's d = 2^-7 covers), lo = bf16_rne(x - hi) with x - hi exact in fp32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = bf16_rne(x) if hi == "rne" else bf16_trunc(x)
    r = x - h
    assert np.array_equal(_f64(x) - _f64(h), _f64(r)), "x - hi is exact in fp32"
    return h, bf16_rne(r)


def _fma32(acc, x, y):
    """fl32(acc + x * y) per entry: the product of two fp32 is exact in float64, the sum is rounded to float64 and then to fp32 (a
    double rounding that can differ from fmaf's single one by the last bit in rare ties: inside the bound's u per link to 2^-29)."""
    return (acc.astype(np.float64) + x.astype(np.float64) * y.astype(np.float64)).astype(np.float32)


def mfma_f32_k_order(k_begin, k_end):
    """The order in which gemm_f32_kernel accumulates k in [k_begin, k_end): stages of 32 from k_begin, octets in order, within an
    octet 0, 4, 1, 5, 2, 6, 3, 7 (k past k_end contributes an exact zero)."""
    order = []
    for k0 in range(k_begin, k_end, 8):
        order += [k for k in (k0 + s + 4 * h for s in range(4) for h in range(2)) if k < k_end]
    return order


def chain_f32(a, b, form, k_order=None):
    """The product as one fp32 fmaf chain per entry over `k_order` (default: the kernel's order over all of K)."""
    A, B = as_ik_kj(a, b, form)
    A, B = np.asarray(A, dtype=np.float32), np.asarray(B, dtype=np.float32)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    for k in (mfma_f32_k_order(0, A.shape[1]) if k_order is None else k_order):
        acc = _fma32(acc, A[:, k:k + 1], B[k:k + 1, :])
    return acc


def sum_chunks_f32(partials):
    """sum_chunks_kernel / atb_reduce_kernel: partial 8 q + r into running sum r, then the eight sums added in order, in fp32."""
    part = [np.zeros_like(partials[0], dtype=np.float32) for _ in range(8)]
    for c, p in enumerate(partials):
        part[c % 8] = (part[c % 8] + np.asarray(p, dtype=np.float32)).astype(np.float32)
    acc = part[0]
    for u in range(1, 8):
        acc = (acc + part[u]).astype(np.float32)
    return acc


def exact_emulated(a, b, form, nchunks=1, chunk_k=None):
    """fitgnn_gemm_exact_f32's arithmetic in NumPy fp32 for a plan (nchunks, chunk_k)."""
    K = as_ik_kj(a, b, form)[0].shape[1]
    if nchunks <= 1:
        return chain_f32(a, b, form)
    parts = [chain_f32(a, b, form, mfma_f32_k_order(min(c * chunk_k, K), min((c + 1) * chunk_k, K))) for c in range(nchunks)]
    return sum_chunks_f32(parts)


def split_emulated(a, b, form="nt", hi="rne"):
    """The three-product bf16 split with fp32 accumulation: per 16 k, the kernels' operand order (lo_a hi_b, hi_a hi_b, hi_a lo_b), each
    product exact and added to the fp32 accumulator with one rounding (the MFMA's internal order is not modelled: one of the orders the
    bound covers)."""
    A, B = as_ik_kj(a, b, form)
    (ha, la), (hb, lb) = split_bf16(A, hi), split_bf16(B, hi)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    K = A.shape[1]
    for k0 in range(0, K, 16):
        for x, y in ((la, hb), (ha, hb), (ha, lb)):
            for k in range(k0, min(k0 + 16, K)):
                acc = _fma32(acc, x[:, k:k + 1], y[k:k + 1, :])
    return acc


def atb_emulated(a, b, plan, hi="rne"):
    """fitgnn_gemm_atb_f32's arithmetic for a [R x M], b [R x N] under an AtbPlan: the split product of every chunk's rows, the chunks
    added as atb_reduce_kernel adds them, then the last R % 32 rows as fl(acc + fl(a b))."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    parts = []
    for c, stages in enumerate(plan.chunk_stages()):
        r0 = c * plan.chunk_rows
        rows = slice(r0, r0 + stages * KBK)
        parts.append(split_emulated(a[rows], b[rows], "tn", hi) if stages else np.zeros((plan.M, plan.N), dtype=np.float32))
    acc = sum_chunks_f32(parts)
    for r in range(plan.r_main, plan.R):
        acc = (acc + a[r][:, None] * b[r][None, :]).astype(np.float32)   # fp32 product, then fp32 sum
    return acc


# ---------------------------------------------------------------------------------------------------------------------------------
# plan models: which branch a case is expected to reach (the GPU tests check plan_exact against fitgnn_gemm_exact_plan)
# ---------------------------------------------------------------------------------------------------------------------------------
S256, S256x128, S64x512, S128, S64x128, S128x64, S64x64 = range(7)
SHAPE_NAMES = ("S256", "S256x128", "S64x512", "S128", "S64x128", "S128x64", "S64x64")
SHAPE_DIM = ((256, 256, 1), (256, 128, 1), (64, 512, 1), (128, 128, 2), (64, 128, 2), (128, 64, 2), (64, 64, 4))   # ti, tj, per_cu


class ExactPlan:
    """make_plan of csrc/gemm_f32.hip."""

    def __init__(self, I, J, K, akm, bkm):
        I, J, K, akm, bkm = int(I), int(J), int(K), bool(akm), bool(bkm)

        def tiles_of(sh):
            return -(-I // SHAPE_DIM[sh][0]) * -(-J // SHAPE_DIM[sh][1])

        if akm and bkm:
            shape = S64x512 if I <= 64 else S128 if (J <= 128 or K < 65536) else S256
        elif J <= 64:
            shape = S128x64
        else:
            cand = (S256x128 if J <= 128 else S256, S128, S64x128, S64x64)
            eff = (1.0, 1.0 if K <= 256 else 0.85, 0.94, 0.85)
            best_cost = 0.0
            for q in range(4):
                sh = cand[q]
                t = tiles_of(sh)
                rounds = float((t + 255) // 256)
                if q == 0 and not akm and t // 256 >= 1 and 0 < t % 256 <= 96 and K >= 8 * 2 * KBK:
                    rounds = float(t // 256) + 0.15
                cost = rounds * SHAPE_DIM[sh][0] * SHAPE_DIM[sh][1] / eff[q]
                if q == 0 or cost < best_cost:
                    best_cost, shape = cost, sh
            if K >= 4096 and tiles_of(S256) <= 512 and J > 128:
                shape = S128
        TI, TJ, per_cu = SHAPE_DIM[shape]
        slots = 256.0 * per_cu
        self.shape = shape
        self.tiles_i, self.tiles_j = -(-I // TI), -(-J // TJ)
        self.nchunks, self.chunk_k = 1, K
        ntile = float(self.tiles_i * self.tiles_j)
        t_tile = 2.0 * TI * TJ * float(K) / (0.45e12 / per_cu)
        most = K // (4 * KBK)
        best = math.ceil(ntile / slots) * t_tile
        c = 8
        while c <= most and c <= 256:
            t = math.ceil(ntile * float(c) / slots) * t_tile / float(c) + float(c + 1) * float(I) * float(J) * 4.0 / 3.0e12 + 4e-6
            if t < 0.92 * best:
                best, self.nchunks = t, c
            c += 8
        if self.nchunks > 1:
            per = -(-K // self.nchunks)
            self.chunk_k = -(-per // KBK) * KBK
        self.main_rows, self.rem_tiles_i, self.rem_chunks, self.rem_chunk_k = 0, 0, 1, K
        T = self.tiles_i * self.tiles_j
        full, rem = T // 256, T % 256
        if not akm and per_cu == 1 and self.nchunks == 1 and full >= 1 and 0 < rem <= 96 and K >= 8 * 2 * KBK:
            main_tiles_i = full * 256 // self.tiles_j
            if 1 <= main_tiles_i < self.tiles_i:
                self.main_rows = main_tiles_i * TI
                self.rem_tiles_i = self.tiles_i - main_tiles_i
                self.rem_chunks = 8
                eighth = -(-K // 8)
                self.rem_chunk_k = -(-eighth // KBK) * KBK
        self.I, self.J, self.K = I, J, K

    def answer(self):
        """What fitgnn_gemm_exact_plan reports."""
        return self.shape, self.nchunks, self.main_rows

    def workspace_bytes(self):
        if self.main_rows > 0:
            return self.rem_chunks * (self.I - self.main_rows) * self.J * 4
        return self.nchunks * self.I * self.J * 4 if self.nchunks > 1 else 0

    def branch(self, form):
        """(form, tile shape, split over k, tail launch)."""
        return form, SHAPE_NAMES[self.shape], self.nchunks > 1, self.main_rows > 0


def plan_exact(form, I, J, K):
    akm, bkm = KMAJOR[form]
    return ExactPlan(I, J, K, akm, bkm)


def exact_admissible(form, I, J, K):
    """The arguments fitgnn_gemm_exact_f32 accepts (leading dimensions and alignment aside)."""
    a_inner, b_inner = (I if form == "tn" else K), (K if form == "nt" else J)
    return I > 0 and J > 0 and K > 0 and a_inner >= 4 and b_inner >= 4 and a_inner % 4 == 0 and b_inner % 4 == 0


class AtbPlan:
    """make_plan of csrc/gemm_atb.hip."""

    def __init__(self, R, M, N):
        R, M, N = int(R), int(M), int(N)
        self.tiles_m, self.tiles_n = -(-M // 256), -(-N // 256)
        self.ntile = self.tiles_m * self.tiles_n
        want = (256 + self.ntile - 1) // self.ntile
        self.r_main = R - R % KBK
        most = max(self.r_main // KBK, 1)
        want = min(want, most)
        self.nchunks = -(-want // 8) * 8
        rows = -(-self.r_main // self.nchunks)
        self.chunk_rows = -(-rows // KBK) * KBK
        self.R, self.M, self.N = R, M, N

    def workspace_bytes(self):
        return self.nchunks * self.M * self.N * 4

    def chunk_stages(self):
        """Stages of every chunk; a chunk that begins at or beyond r_main has none and stores zeros."""
        out = []
        for c in range(self.nchunks):
            k_begin = c * self.chunk_rows
            k_end = min(k_begin + self.chunk_rows, self.r_main)
            out.append(max(k_end - k_begin, 0) // KBK)
        return out

    def trailing_chunks_beyond(self):
        """Chunks whose first row lies strictly beyond r_main (k_begin > R_main)."""
        return sum(1 for c in range(self.nchunks) if c * self.chunk_rows > self.r_main)


def nt_variant(R, N):
    """launch_nt's tile choice for a plain b: 2 -> 128 x 128 tiles, 4 -> 256 x 256."""
    return 2 if -(-int(R) // 256) * -(-int(N) // 256) < 128 else 4


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_gemm_kernels.py: (form, I, J, K, tile shape, nchunks, main_rows) -- the last three are what
# fitgnn_gemm_exact_plan must answer, written out (the smallest shapes found for each branch by a search over the plan model)
# ---------------------------------------------------------------------------------------------------------------------------------
def _both(I, J, K, *answer):
    return [("nt", I, J, K) + answer, ("nn", I, J, K) + answer]


EXACT_CASES = (
    # 128 x 64 tiles (J <= 64): one tile with one live row and one live column group, K of one partial stage; a second stage of one
    # group; J % 4 != 0 (nt); a full tile; a second row tile of one row; 8 and 9 row tiles
    _both(1, 4, 4, "S128x64", 1, 0) + _both(5, 4, 36, "S128x64", 1, 0) + [("nt", 5, 47, 100, "S128x64", 1, 0)]
    + _both(128, 64, 32, "S128x64", 1, 0) + _both(129, 64, 64, "S128x64", 1, 0) + _both(897, 8, 36, "S128x64", 1, 0)
    + _both(1025, 64, 100, "S128x64", 1, 0)
    # ... split over k: 8 chunks of 128; chunk_k 160 (chunk 6 holds 68 k: a third stage of one group, chunk 7 is empty); 16 chunks
    + _both(5, 4, 1024, "S128x64", 8, 0) + _both(5, 4, 1028, "S128x64", 8, 0) + _both(129, 4, 2048, "S128x64", 16, 0)
    + [("nt", 1025, 4, 1024, "S128x64", 8, 0)]
    # 64 x 64 tiles: a second column tile of one group; 2 x 2 tiles with one live row and group (and J = 69); full tiles; 8, 9 row tiles
    + _both(1, 68, 4, "S64x64", 1, 0) + _both(65, 68, 36, "S64x64", 1, 0) + [("nt", 65, 69, 36, "S64x64", 1, 0)]
    + _both(64, 128, 32, "S64x64", 1, 0) + _both(449, 68, 64, "S64x64", 1, 0) + _both(513, 68, 100, "S64x64", 1, 0)
    + _both(65, 68, 1024, "S64x64", 8, 0) + _both(200, 68, 2048, "S64x64", 16, 0) + [("nt", 1, 68, 1028, "S64x64", 8, 0)]
    # 64 x 128 tiles: from 257 tiles of 64 x 64 on
    + _both(5441, 132, 36, "S64x128", 1, 0) + [("nt", 8256, 128, 4, "S64x128", 1, 0)] + _both(449, 2052, 32, "S64x128", 1, 0)
    + _both(513, 2048, 64, "S64x128", 1, 0)
    + _both(8193, 68, 100, "S64x128", 1, 0) + _both(1217, 772, 1024, "S64x128", 8, 0)
    # 128 x 128 tiles: one round of them against two of 64 x 128; split: the K >= 4096 && J > 128 override (24 chunks of 192: two empty)
    + _both(7169, 388, 36, "S128", 1, 0) + _both(897, 4096, 32, "S128", 1, 0)
    + [("nt", 8320, 384, 4, "S128", 1, 0), ("nn", 9984, 260, 64, "S128", 1, 0), ("nt", 32513, 68, 100, "S128", 1, 0)]
    + _both(1, 132, 4096, "S128", 32, 0) + _both(129, 132, 4096, "S128", 32, 0)
    + [("nt", 897, 132, 4096, "S128", 32, 0), ("nn", 1025, 132, 4096, "S128", 24, 0)]
    # 256 x 256 tiles: one full round (128 x 2, 28 x 9 tiles); a tail launch of one row (K = 516: rem_chunk_k 96, the tail's chunks 6
    # and 7 empty, chunk 5 of 36 k) and of three row tiles; split over k
    + [("nt", 32513, 388, 4, "S256", 1, 0), ("nn", 32513, 388, 32, "S256", 1, 0), ("nn", 32513, 388, 100, "S256", 1, 0)]
    + _both(6913, 2052, 36, "S256", 1, 0)
    + [("nt", 6912, 2052, 64, "S256", 1, 0)] + _both(4097, 4096, 516, "S256", 1, 4096) + [("nt", 7681, 2052, 512, "S256", 1, 7168)]
    + _both(7681, 2052, 1024, "S256", 8, 0)
    # 256 x 128 tiles (J <= 128, 256 tiles or more): tails of 1 and of 96 tiles; 97 tiles: no tail launch (the plan then prefers 64 x 128)
    + _both(65281, 68, 4, "S256x128", 1, 0) + [("nt", 65536, 128, 32, "S256x128", 1, 0), ("nn", 65281, 68, 100, "S256x128", 1, 0),
                                                ("nt", 65281, 68, 36, "S256x128", 1, 0), ("nn", 65281, 128, 64, "S256x128", 1, 0)]
    + _both(65537, 68, 516, "S256x128", 1, 65536) + _both(89857, 68, 512, "S256x128", 1, 65536) + _both(90113, 68, 512, "S64x128", 1, 0)
    + _both(65537, 68, 1024, "S256x128", 8, 0)
    # tn, 64 x 512 tiles (I <= 64): K = 1, 31, 33 rows; a second column tile of one group
    + [("tn", 4, 4, 1, "S64x512", 1, 0), ("tn", 4, 4, 4, "S64x512", 1, 0), ("tn", 64, 512, 32, "S64x512", 1, 0),
       ("tn", 4, 516, 31, "S64x512", 1, 0), ("tn", 8, 4, 33, "S64x512", 1, 0), ("tn", 64, 516, 36, "S64x512", 1, 0),
       ("tn", 60, 8, 100, "S64x512", 1, 0), ("tn", 4, 4, 64, "S64x512", 1, 0), ("tn", 4, 4, 1024, "S64x512", 8, 0),
       ("tn", 64, 516, 1028, "S64x512", 8, 0), ("tn", 4, 4, 2048, "S64x512", 16, 0)]
    # tn, 128 x 128 tiles
    + [("tn", 68, 4, 1, "S128", 1, 0), ("tn", 132, 132, 31, "S128", 1, 0), ("tn", 128, 128, 32, "S128", 1, 0),
       ("tn", 900, 4, 33, "S128", 1, 0), ("tn", 1028, 4, 36, "S128", 1, 0), ("tn", 68, 132, 64, "S128", 1, 0),
       ("tn", 132, 4, 100, "S128", 1, 0), ("tn", 68, 4, 1024, "S128", 8, 0), ("tn", 132, 132, 1028, "S128", 8, 0),
       ("tn", 900, 4, 1024, "S128", 8, 0), ("tn", 1028, 4, 2048, "S128", 16, 0)]
    # tn, 256 x 256 tiles (K >= 65536): 248 chunks of 288 (chunk 227 holds 160 k, 20 chunks are empty), 64 chunks on 2 x 2 tiles, 8 and 9
    # row tiles; WITHOUT a split only where the tiles fill the 256 slots so evenly that no chunk count pays: 15 x 16 tiles at the least
    + [("tn", 68, 132, 65536, "S256", 248, 0), ("tn", 260, 260, 65536, "S256", 64, 0), ("tn", 1796, 132, 65536, "S256", 32, 0),
       ("tn", 2052, 132, 65536, "S256", 56, 0), ("tn", 3588, 4096, 65536, "S256", 1, 0)]
)

# fitgnn_gemm_exact_epi_f32: one case per tile shape reachable with nt, and tail launches (J % 4 == 0 for ELU / dropout); K = 516 leaves
# the tail's chunks 6 and 7 empty, K = 512 fills all eight (a chunk sum that dropped its last running sum would pass the former)
EPI_CASES = [("nt", 129, 64, 36, "S128x64", 1, 0), ("nt", 65, 68, 36, "S64x64", 1, 0), ("nt", 5441, 132, 36, "S64x128", 1, 0),
             ("nt", 7169, 388, 36, "S128", 1, 0), ("nt", 32513, 388, 36, "S256", 1, 0), ("nt", 65281, 68, 36, "S256x128", 1, 0),
             ("nt", 65537, 68, 516, "S256x128", 1, 65536), ("nt", 65537, 68, 512, "S256x128", 1, 65536),
             ("nt", 4097, 4096, 516, "S256", 1, 4096)]

# fitgnn_gemm_nt_f32 (R, N, K): the 128-tile variant (tiles of 256 x 256 < 128) with 1, 2 and 9 row tiles, N % 4 != 0, a second
# column tile of one column group; the 256-tile variant from 128 tiles of 256 rows on
NT_CASES = [(R, N, K) for R in (1, 5, 128, 129, 1025) for (N, K) in ((4, 32), (47, 64), (128, 96), (132, 32))] + \
           [(32513, 4, 32), (32513, 4, 96), (32769, 8, 64)]
# fitgnn_gemm_nt_pre_f32 (always 256 x 256 tiles)
NT_PRE_CASES = [(R, N, K) for R in (1, 255, 256, 257, 2049) for N in (4, 128, 260) for K in (32, 64, 96)]

# fitgnn_gemm_atb_f32 (R, M, N)
ATB_CASES = [(R, M, N) for R in (1, 31, 32, 33, 63, 64, 293) for (M, N) in ((4, 4), (36, 260), (256, 36), (260, 256), (4, 260))] + \
            [(8192 + 5, 4, 4), (2048 + 5, 260, 260), (4096, 256, 256)]


def case_id(c):
    return "-".join(str(x) for x in c)
