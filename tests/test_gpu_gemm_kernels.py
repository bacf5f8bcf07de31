"""GPU tier: the dense GEMM kernels -- csrc/gemm_f32.hip (fitgnn_gemm_exact_f32, fitgnn_gemm_exact_epi_f32), csrc/gemm_nt.hip
(fitgnn_gemm_nt_f32, fitgnn_gemm_nt_presplit_f32 + fitgnn_gemm_nt_pre_f32) and csrc/gemm_atb.hip (fitgnn_gemm_atb_f32) -- through the
C ABI against float64 products, at every branch of their launch code.  References, bounds, emulations, plan models and the case
lists are in tests/gemm_reference.py (read its docstring for the derivations); tests/test_gemm_reference_cpu.py checks them.

Every product launch: the operands are strided views (leading dimension = extent + 4) in NaN-filled buffers, two rows of NaN behind
the last valid row (for k-major operands that is behind row K - 1); the output [I x ldc], ldc > J, is NaN before the launch and
followed by guard elements, and the columns J ... ldc and the guards must still be NaN afterwards; a workspace has exactly the
bytes the library asks for, followed by a NaN guard.  EXACT operands (integers in [-8, 8] over 64) must give the float64 product
bit for bit (gemm_reference.product_is_exact holds for every case: asserted, never a reason to skip); RANDOM (normal) operands are
held per entry to the derived bound; a second launch must give the same bits.  Operands above 2^22 elements are drawn on the
device (same value sets), their float64 products are torch float64 products on the device.

Bounds (u = 2^-24, S = |a| |b| per entry, first order, no allowance):
* exact product: K u S; split over k or tail rows: (chunk_k + ceil(nchunks / 8) + 6) u S
* gemm_nt: (3.06e-5 + 3 K u T) S; gemm_atb: (3.06e-5 + (3 chunk_rows + nchunks / 8 + 6) u T + 2 (R % 32) u) S, T = 1.0118
* fused forward epilogue: test_gpu_step_kernels._check_fwd with the product's bound as the error of z

Launcher -> branch (from the launch code and the kernel) -> tests (case ids are form-I-J-K-shape-nchunks-main_rows):

| launcher | branch | tests |
|---|---|---|
| fitgnn_gemm_exact_f32 | operand forms nt (<false, false>), nn (<false, true>: b k-major), tn (<true, true>); (k-major a, k-minor b) refused | test_gemm_exact[nt-* / nn-* / tn-*], test_gemm_exact_refusals |
| | S128x64 <4,1,1,2> (J <= 64; nt, nn): one tile with one live row and one live group of 4 columns, K = 4 (one partial stage) [1-4-4]; K = 36 (second stage of one 4-group) [5-4-36]; J = 47 (nt: columns not a multiple of 4) [5-47-100]; full tile [128-64-32]; second row tile of one row [129-64-64]; 8 row tiles [897-8-36]; 9 (ti = 8 on XCD slot 0 of the second group of eight, the slots of ti = 9 ... 15 return) [1025-64-100] | test_gemm_exact[*-S128x64-1-0] |
| | ... split over k: 8 chunks [5-4-1024]; chunk_k 160: chunk 6 of 68 k (a third stage of one group), chunk 7 empty (stores zeros) [5-4-1028]; 16 chunks (second XCD group) on two row tiles [129-4-2048]; 9 row tiles [1025-4-1024] | test_gemm_exact[*-S128x64-8-0 / -16-0] |
| | S64x64 <2,2,1,1>: [1-68-4] (second column tile of one group), [65-68-36] (2 x 2 tiles, one live row and group), [65-69-36] (nt, J odd), [64-128-32] full, [449-68-64] 8 row tiles, [513-68-100] 9; split [65-68-1024], [200-68-2048] (16 chunks), [1-68-1028] (empty and partial chunk) | test_gemm_exact[*-S64x64-*] |
| | S64x128 <2,2,1,2> (from 257 tiles of 64 x 64 on): [5441-132-36] (86 x 2 tiles, partial in i and j), [8256-128-4] full, [449-2052-32] 8 row tiles x 17, [513-2048-64] 9 x 16, [8193-68-100] 129 x 1; split [1217-772-1024] | test_gemm_exact[*-S64x128-*] |
| | S128 <2,2,2,2>: [7169-388-36] (57 x 4, partial in i and j), [897-4096-32] 8 row tiles, [8320-384-4] full, [9984-260-64], [32513-68-100] (255 x 1); no plan without a split has 9 row tiles | test_gemm_exact[*-S128-1-0] |
| | ... the K >= 4096 && J > 128 override to S128 with a split: 32 chunks [1-132-4096], [129-132-4096], [897-132-4096]; 24 chunks of 192, two of them empty [1025-132-4096] | test_gemm_exact[*-S128-32-0 / -24-0] |
| | S256 <4,2,2,4> (nt, nn): one full round, 128 x 2 tiles [32513-388-4 / -32 / -100], 28 x 9 [6913-2052-36] (one live row, one live group), [6912-2052-64]; split [7681-2052-1024]; no plan reaches it with fewer than 128 tiles | test_gemm_exact[*-S256-1-0 / -8-0] |
| | ... tail launch (main_rows > 0: pm over the full rounds, pr = the last round's rows split 8 ways into the workspace, sum_chunks_kernel): one row in the tail, K = 516 so that rem_chunk_k = 96 rounds UP (chunk 5 of 36 k, chunks 6 and 7 empty) [4097-4096-516]; three row tiles [7681-2052-512] | test_gemm_exact[*-S256-1-4096 / -7168] |
| | S256x128 <4,1,2,4> (J <= 128, >= 256 tiles): [65281-68-4 / -36 / -100], [65536-128-32] full, [65281-128-64]; split [65537-68-1024]; tail of 1 tile [65537-68-516], of 96 [89857-68-512]; 97 tiles: no tail launch, the plan takes S64x128 [90113-68-512] | test_gemm_exact[*-S256x128-*], test_gemm_exact[*-90113-68-512-S64x128-1-0] |
| | tn S64x512 <1,4,2,4> (I <= 64): K = 1, 4, 31, 32, 33, 36, 64, 100 rows; second column tile of one group [4-516-31], [64-516-36]; split 8 [4-4-1024], 16 [4-4-2048], empty + partial chunk [64-516-1028] | test_gemm_exact[tn-*-S64x512-*] |
| | tn S128: K = 1 [68-4-1], 31 [132-132-31] (2 x 2, partial), 32, 33 with 8 row tiles [900-4-33], 36 with 9 [1028-4-36], 64, 100; split [68-4-1024], [132-132-1028] (empty + partial), [900-4-1024], [1028-4-2048] (16) | test_gemm_exact[tn-*-S128-*] |
| | tn S256 (I > 64, J > 128, K >= 65536): 248 chunks of 288, chunk 227 of 160 k, 20 empty (chunk >= nchunks returns: 248 is 31 XCD groups) [68-132-65536]; 2 x 2 tiles [260-260-65536]; 8 and 9 row tiles [1796- / 2052-132-65536]; without a split (15 x 16 tiles: the smallest grid on which no chunk count pays) [3588-4096-65536] | test_gemm_exact[tn-*-S256-*] |
| | refusals, each with its code and the output untouched: ldc < J; inner extent % 4 != 0 or < 4 (K for nt, J for nn, I for tn); lda, ldb % 4 != 0 or below the extent; a / b one float into its buffer (FITGNN_E_ALIGN); NULL or 8-byte-aligned workspace where the plan splits or has a tail; (k-major, k-minor); NULL operands | test_gemm_exact_refusals |
| fitgnn_gemm_exact_plan / _workspace_bytes | answers (shape, nchunks, main_rows) and bytes of every case against the case list and the Python model | every test_gemm_exact / test_gemm_exact_epi case |
| fitgnn_gemm_exact_epi_f32 | gemm_f32_kernel<..., EPI = true> per tile shape reachable with nt: S128x64, S64x64, S64x128, S128, S256, S256x128; rows given / NULL (row0 + i); BIAS + DROPOUT by mask on EXACT operands bit for bit over the whole output, BIAS + ELU + DROPOUT by hash on RANDOM operands against step_reference.epilogue_fwd | test_gemm_exact_epi |
| | tail launch: pm with the epilogue in the store, the tail's chunks through sum_chunks_kernel<true> with se.rows / se.row0 moved to main_rows [65537-68-516, 4097-4096-516; 65537-68-512: all eight chunks of the tail hold k] | test_gemm_exact_epi[*-65536-* / *-4096-*] |
| | refusals: a plan split over k, J % 4 != 0 with ELU, BIAS without bias, p = 1, unknown flag, NULL workspace for a tail plan | test_gemm_exact_epi_refusals |
| fitgnn_gemm_nt_f32 | gemm_nt_kernel<2, false, false> (big_grid < 128): R = 1, 5 (rows clamped), 128, 129 (second row tile of one row), 1025 (9 row tiles); N = 4, 47 (not a multiple of 4), 128, 132 (second column tile); K = 32 (every prefetch re-reads the one stage), 64, 96 | test_gemm_nt[R-N-K] |
| | gemm_nt_kernel<4, false, false> (big_grid >= 128): R = 32513 (128 row tiles, one column group wide), 32769 (129) | test_gemm_nt[32513-* / 32769-*] |
| | R = 0 returns 0 and touches nothing; refusals of launch_nt (K < 32, K % 32, lda < K, lda % 4, ldb < K, ldb % 4, ldc < N, N = 0, R < 0, NULL, FITGNN_E_ALIGN) | test_gemm_nt_empty_and_refusals |
| fitgnn_gemm_nt_presplit_f32 + fitgnn_gemm_nt_pre_f32 | gemm_nt_kernel<4, false, true> (LDS-DMA of the b image): R = 1, 255, 256, 257, 2049 x N = 4, 128, 260 x K = 32, 64, 96; b read through plain and through transposed strides; image of exactly fitgnn_gemm_nt_presplit_bytes + NaN guard | test_gemm_nt_pre |
| | K_valid < K: b holds K_valid columns, NaN beyond them in memory, the image's k >= K_valid are zero | test_gemm_nt_pre_k_valid |
| | refusals of fitgnn_gemm_nt_presplit_f32 (N = 0, K < 32, K % 32, K_valid = 0, K_valid > K, NULL, image misaligned: FITGNN_E_ALIGN) | test_gemm_nt_empty_and_refusals |
| fitgnn_gemm_atb_f32 | R = 1, 31: r_main = 0, chunk_rows = 0, every output from atb_reduce_kernel's scalar loop over zeroed partials; R = 32, 64 (no remainder), 33, 63 (remainder of 1, 31 rows) | test_gemm_atb[1-* ... 64-*] |
| | R = 293: 9 stages over 16 chunks of 32 rows, chunks 10 ... 15 begin beyond r_main (no stage, zeros); R = 8197, M = N = 4: 256 chunks of one stage; R = 2053 on 2 x 2 tiles: nchunks = 64; R = 4096, 256 x 256: 128 chunks, one full tile | test_gemm_atb[293-*, 8197-4-4, 2053-260-260, 4096-256-256] |
| | M, N in {4, 36, 256, 260}: the column clamp (col + 4 <= ncols ? col : ncols - 4), a second tile of one column group | test_gemm_atb[*-M-N] |
| | refusals: R = 0, M / N < 4 or % 4, lda < M, lda / ldb % 4, NULL, a / b / out / workspace misaligned (FITGNN_E_ALIGN) | test_gemm_atb_refusals |

Worst observed error / bound over all entries of one MI355X run (printed with -s; every family stayed inside its bound, no EXACT
case differed in a bit):
* exact product, one launch: nt 0.79, nn 0.81 (K = 4), tn 0.93 (K = 1: a single rounding reaches u on its own); 0.19 at K = 32, 0.07 at K = 100,
  0.012 at K = 512: the bound grows with K, the error of normal operands with sqrt K.  Split over k: nt 0.010, nn 0.010, tn 0.006;
  tail rows: 0.018.  The fp32 fmaf-chain emulation of tests/test_gemm_reference_cpu.py: 0.61 (K = 4), 0.09 with chunks
* gemm_nt <2> 0.19, <4> 0.19, image path 0.21 at K_valid >= 20 and 0.77 at K_valid = 1 (one product: the dropped lo.lo term and the
  rounding of lo are all there is); the emulation: 0.42
* gemm_atb 0.17 (R = 32: one stage), 0.007 where every row goes through the scalar loop (R < 32); the emulation: 0.11

Arithmetic-only changes to a scratch copy of gemm_f32.hip / gemm_nt.hip / gemm_atb.hip (none moves a store, a loop bound of a
kernel or a launch dimension), this module and the GEMM tests of tests/test_gpu_spmm.py (-k "gemm or presplit": 63) run once per
change on one MI355X -- failed tests of the 496 here / of the 63 there:
* (a) sum_chunks_kernel adds seven of its eight running sums:                                            70 / 14  (a first run
  failed nothing in test_gemm_exact_epi: its tail cases had K = 516, which leaves the tail's chunk 7 empty; the K = 512 tail
  case was added for this and fails its 4)
* (b) load_slab returns the clamped last valid k instead of zero for k >= klim (both operand forms):     138 / 16
* (c) atb_reduce_kernel's loop over the last R % 32 rows starts at r_begin + 1:                          54 / 8
* (d) gemm_nt_kernel stores no lo part for the a side (the lo.hi product dropped):                       78 / 10  (every RANDOM case)
* (e) make_plan rounds the tail launch's rem_chunk_k down instead of up:                                 16 / 0   (the K = 516 tails;
  every K the other module uses is a multiple of 256)
* (f) atb_reduce_kernel adds seven of its eight running sums:                                            16 / 7   (R >= 293: chunk 7
  holds rows only from 8 stages on)
* (g) nt_presplit_kernel stores no lo part (hi.lo dropped on the image path):                            55 / 5
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import gemm_reference as G
import step_reference as sr
from test_gpu_step_kernels import (E_ALIGN, E_BADARG, L, U, _call, _check_fwd, _dev, _exact, _np, _p, _rng, _run, _same,  # noqa: F401
                                   _strided, _within)

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 8
WORST = {}
BIG = 1 << 22        # operands and outputs above this many elements stay on the device
SEED = 0x1234_5678_9ABC_DEF1 & 0x7FFF_FFFF_FFFF_FFFF


# ---------------------------------------------------------------------------------------------------------------------------------
# operands, outputs, comparisons
# ---------------------------------------------------------------------------------------------------------------------------------
def _values(kind, shape, *parts):
    """[n x C] EXACT (integers in [-8, 8] over 64) or RANDOM (normal) values on the device."""
    if shape[0] * shape[1] <= BIG:
        rng = _rng(kind, shape, *parts)
        return _dev(_exact(rng, shape) if kind == "exact" else rng.normal(size=shape).astype(np.float32))
    g = torch.Generator(device="cuda")
    g.manual_seed(zlib.crc32(repr((kind, shape) + parts).encode()))
    if kind == "exact":
        return torch.randint(-8, 9, shape, generator=g, device="cuda", dtype=torch.int32).to(torch.float32) / 64.0
    return torch.randn(shape, generator=g, device="cuda", dtype=torch.float32)


def _padded(vals, ld=None, behind=2):
    """vals [n x C] as a view with row stride ld (default: C rounded up to 4, plus 4) in a NaN buffer: NaN in the padding columns and
    `behind` rows of NaN after the last row -- a kernel that loads there poisons a live output."""
    n, C = vals.shape
    ld = (C + 3) // 4 * 4 + 4 if ld is None else ld
    if n * C <= BIG:
        v = _strided(np.vstack([vals.cpu().numpy(), np.full((behind, C), NAN, dtype=np.float32)]), ld)[:n]
    else:
        buf = torch.full(((n + behind) * ld + 4,), NAN, dtype=torch.float32, device="cuda")
        v = buf[:n * ld].view(n, ld)[:, :C]
        v.copy_(vals)
    assert v.stride() == (ld, 1) and v.data_ptr() % 16 == 0
    return v


def _output(I, J, ldc):
    """(buffer, [I x J] view): NaN everywhere, GUARD elements behind row I - 1."""
    buf = torch.full((I * ldc + GUARD,), NAN, dtype=torch.float32, device="cuda")
    return buf, buf[:I * ldc].view(I, ldc)[:, :J]


def _untouched(buf, I, J, ldc, what):
    full = buf[:I * ldc].view(I, ldc)
    assert torch.isnan(full[:, J:]).all().item(), f"{what}: wrote into the columns J ... ldc"
    assert torch.isnan(buf[I * ldc:]).all().item(), f"{what}: wrote past the last row"


def _workspace(nbytes):
    """(tensor or None, pointer): exactly nbytes, followed by a NaN guard."""
    assert nbytes % 4 == 0
    if nbytes == 0:
        return None, None
    ws = torch.full((nbytes // 4 + GUARD,), NAN, dtype=torch.float32, device="cuda")
    return ws, ctypes.c_void_p(ws.data_ptr())


def _ws_guard(ws, nbytes, what):
    if ws is not None:
        assert torch.isnan(ws[nbytes // 4:]).all().item(), f"{what}: wrote past the workspace"


def _product64(a, b, form):
    """(float64 product, S = |a| |b|) on the device."""
    A = (a.t() if form == "tn" else a).to(torch.float64)
    B = (b.t() if form == "nt" else b).to(torch.float64)
    ref = A @ B
    return ref, A.abs_() @ B.abs_()


def _bit_equal(got, ref, S, what):
    """EXACT operands: the predicate holds and the output is the float64 product bit for bit."""
    premise = G.product_is_exact(S.cpu().numpy()).all() if S.numel() <= BIG else bool((S * 2.0 ** 12 < 2.0 ** 24).all().item())
    assert premise, f"{what}: a partial sum of the EXACT operands can round"
    if got.numel() <= BIG or bool((got.to(torch.float64) != ref).any().item()):
        _same(_np(got), ref.cpu().numpy(), what)


def _bounded(family, got, ref, bound, what):
    """Per entry |got - ref| <= bound, and the worst error / bound ratio of the family printed (run with -s) for the module
    docstring.  Device tensors; the small ones go through _within as they are, the large ones when they fail."""
    err = (got.to(torch.float64) - ref).abs()
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max().item()) if bool(pos.any().item()) else 0.0
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"[ratio] {family}: {what}: {ratio:.3g} (family worst {WORST[family]:.3g})")
    if got.numel() <= BIG or not bool((err <= bound).all().item()):
        _within(_np(got), ref.cpu().numpy(), bound.cpu().numpy(), what)


def _eq(x, y):
    return torch.equal(torch.nan_to_num(x, nan=12345.0), torch.nan_to_num(y, nan=12345.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# fitgnn_gemm_exact_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def _lib_plan(L, form, I, J, K):
    akm, bkm = G.KMAJOR[form]
    shape, nchunks, main_rows = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
    assert L.lib().fitgnn_gemm_exact_plan(I, J, K, akm, bkm, ctypes.byref(shape), ctypes.byref(nchunks), ctypes.byref(main_rows)) == 0
    return (shape.value, nchunks.value, main_rows.value), int(L.lib().fitgnn_gemm_exact_workspace_bytes(I, J, K, akm, bkm))


def _assert_plan(L, case):
    """The library's plan is the one the case was chosen for, and the Python model's."""
    form, I, J, K, shape, nchunks, main_rows = case
    plan = G.plan_exact(form, I, J, K)
    answer, nbytes = _lib_plan(L, form, I, J, K)
    assert (G.SHAPE_NAMES[answer[0]], answer[1], answer[2]) == (shape, nchunks, main_rows), f"{case}: the library plans {answer}"
    assert answer == plan.answer() and nbytes == plan.workspace_bytes(), f"{case}: plan model {plan.answer()}, {plan.workspace_bytes()} bytes"
    return plan, nbytes


def _operands(kind, form, I, J, K):
    sa, sb = G.operand_shapes(form, I, J, K)
    return _padded(_values(kind, sa, "a", form)), _padded(_values(kind, sb, "b", form))


def _gemm_exact(L, form, a, b, I, J, K, nbytes, ldc=None):
    akm, bkm = G.KMAJOR[form]
    ldc = J + 4 + (I & 1) if ldc is None else ldc
    cbuf, c = _output(I, J, ldc)
    ws, wp = _workspace(nbytes)
    rc = _call(L, "fitgnn_gemm_exact_f32", _p(L, a), a.stride(0), akm, _p(L, b), b.stride(0), bkm, I, J, K, _p(L, c), ldc, wp)
    _untouched(cbuf, I, J, ldc, "c")
    _ws_guard(ws, nbytes, "exact")
    return rc, c


def _exact_bound_dev(S, K, plan):
    bound = G.exact_links(K, plan.nchunks, plan.chunk_k) * U * S
    if plan.main_rows > 0:
        bound[plan.main_rows:] = G.exact_links(K, plan.rem_chunks, plan.rem_chunk_k) * U * S[plan.main_rows:]
    return bound


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", G.EXACT_CASES, ids=G.case_id)
def test_gemm_exact(L, case, kind):
    form, I, J, K = case[:4]
    plan, nbytes = _assert_plan(L, case)
    a, b = _operands(kind, form, I, J, K)
    rc, c = _gemm_exact(L, form, a, b, I, J, K, nbytes)
    L.check(rc, "fitgnn_gemm_exact_f32")
    ref, S = _product64(a, b, form)
    if kind == "exact":
        _bit_equal(c, ref, S, f"c {case}")
    else:
        family = f"exact {form}" + (", split" if plan.nchunks > 1 else ", tail" if plan.main_rows else "")
        _bounded(family, c, ref, _exact_bound_dev(S, K, plan), f"c {case}")
    rc, c2 = _gemm_exact(L, form, a, b, I, J, K, nbytes)
    assert rc == 0 and _eq(c, c2), "two launches on the same input differ"


def test_gemm_exact_refusals(L):
    def launch(form="nt", I=8, J=8, K=8, lda=None, ldb=None, ldc=None, a_off=0, b_off=0, ws="plan", forms=None):
        sa, sb = G.operand_shapes(form, I, J, K)
        a = _padded(_values("exact", sa, "ra"), lda if lda is not None and lda >= sa[1] else None)
        b = _padded(_values("exact", sb, "rb"), ldb if ldb is not None and ldb >= sb[1] else None)
        lda = a.stride(0) if lda is None else lda
        ldb = b.stride(0) if ldb is None else ldb
        ldc_buf = max(J + 4, ldc or 0)
        cbuf, c = _output(I, J, ldc_buf)
        akm, bkm = G.KMAJOR[form] if forms is None else forms
        nbytes = int(L.lib().fitgnn_gemm_exact_workspace_bytes(I, J, K, akm, bkm))
        wbuf = torch.full((nbytes // 4 + GUARD,), NAN, dtype=torch.float32, device="cuda")
        wp = {"plan": ctypes.c_void_p(wbuf.data_ptr()), "null": None, "8": ctypes.c_void_p(wbuf.data_ptr() + 8)}[ws]
        pa, pb = ctypes.c_void_p(a.data_ptr() + 4 * a_off), ctypes.c_void_p(b.data_ptr() + 4 * b_off)
        rc = _call(L, "fitgnn_gemm_exact_f32", pa, lda, akm, pb, ldb, bkm, I, J, K, _p(L, c), ldc_buf if ldc is None else ldc, wp)
        if rc != 0:
            assert torch.isnan(cbuf).all().item() and torch.isnan(wbuf).all().item(), "a refused call wrote"
        return rc

    assert launch() == 0 and launch("nn") == 0 and launch("tn") == 0
    assert launch(ldc=7) == E_BADARG                                                       # ldc < J
    assert launch(K=6) == E_BADARG and launch(K=2) == E_BADARG                             # nt: the inner extent of both is K
    assert launch("nn", J=6) == E_BADARG and launch("nn", J=2) == E_BADARG                 # nn: b's is J
    assert launch("tn", I=6) == E_BADARG and launch("tn", I=2, J=8) == E_BADARG            # tn: a's is I
    assert launch("nt", J=6) == 0 and launch("nn", I=6) == 0 and launch("tn", K=6) == 0    # (the outer extents are free)
    assert launch(lda=9) == E_BADARG and launch(ldb=10) == E_BADARG and launch(lda=4) == E_BADARG and launch(ldb=4) == E_BADARG
    assert launch(a_off=1) == E_ALIGN and launch(b_off=1) == E_ALIGN and launch("tn", a_off=2) == E_ALIGN
    assert launch(a_off=4) == 0
    assert launch(forms=(1, 0)) == E_BADARG                                                # (k-major a, k-minor b)
    for form, I, J, K in (("nt", 5, 4, 1024), ("tn", 4, 4, 1024), ("nn", 65537, 68, 516)):  # plans with a split / a tail launch
        p = G.plan_exact(form, I, J, K)
        assert p.nchunks > 1 or p.main_rows > 0
        assert launch(form, I, J, K, ws="null") == E_BADARG and launch(form, I, J, K, ws="8") == E_BADARG
    assert L.lib().fitgnn_gemm_exact_f32(None, 8, 0, None, 8, 0, 8, 8, 8, None, 8, None, None) == E_BADARG
    bad = ctypes.c_int32()
    assert L.lib().fitgnn_gemm_exact_plan(0, 8, 8, 0, 0, ctypes.byref(bad), ctypes.byref(bad), None) == E_BADARG
    assert L.lib().fitgnn_gemm_exact_workspace_bytes(0, 8, 8, 0, 0) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# fitgnn_gemm_exact_epi_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def _gemm_epi(L, a, b, I, J, K, rows, bias, epi, p, seed, mask, nbytes, ldc=None, ws="plan"):
    ldc = J + 4 if ldc is None else ldc
    cbuf, c = _output(I, J, max(ldc, J + 4))
    wbuf, wp = _workspace(nbytes)
    if ws == "null":
        wp = None
    rc = _call(L, "fitgnn_gemm_exact_epi_f32", _p(L, a), a.stride(0), _p(L, b), b.stride(0), I, J, K, _p(L, c), ldc, _p(L, rows), _p(L, bias),
               epi, p, seed, _p(L, mask), wp)
    if rc == 0:
        _untouched(cbuf, I, J, ldc, "c")
    else:
        assert torch.isnan(cbuf).all().item(), "a refused call wrote"
    _ws_guard(wbuf, nbytes, "epi")
    return rc, c


def _sample_rows(I, main_rows, rng):
    """All rows of a small output; of a large one the first and last 200, the 200 on either side of main_rows, 600 others."""
    edges = [np.arange(200), np.arange(I - 200, I), rng.integers(0, I, size=600)]
    if main_rows:
        edges.append(np.arange(main_rows - 200, min(main_rows + 200, I)))
    return np.unique(np.concatenate(edges))


@pytest.mark.parametrize("with_rows", [False, True], ids=["row0", "rows"])
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", G.EPI_CASES, ids=G.case_id)
def test_gemm_exact_epi(L, case, kind, with_rows):
    """EXACT: bias + dropout by mask at p = 0.5 (z + bias and the scale 2 are exact) over the whole output, bit for bit.  RANDOM:
    bias + ELU + dropout by hash of the ORIGINAL row against step_reference.epilogue_fwd of the float64 product, per entry."""
    form, I, J, K = case[:4]
    plan, nbytes = _assert_plan(L, case)
    rng = _rng("epi", case, kind, with_rows)
    a, b = _operands(kind, form, I, J, K)
    total = I + 37
    rows = torch.randperm(total, device="cuda")[:I].contiguous() if with_rows else None
    orig = rows if with_rows else torch.arange(I, device="cuda")
    ref, S = _product64(a, b, form)
    if kind == "exact":
        bias = _dev(_exact(rng, (J,)))
        mask = (torch.rand((total, J), device="cuda") < 0.5).to(torch.uint8)
        epi = sr.EPI_BIAS | sr.EPI_DROPOUT
        rc, c = _gemm_epi(L, a, b, I, J, K, rows, bias, epi, 0.5, 0, mask, nbytes)
        L.check(rc, "fitgnn_gemm_exact_epi_f32")
        want = torch.where(mask[orig] != 0, (ref + bias.to(torch.float64)[None, :]) * 2.0, torch.zeros((), dtype=torch.float64, device="cuda"))
        _bit_equal(c, want, S + 0.125, f"epi {case}")
        sub = np.arange(min(I, 300))           # ... and step_reference's statement of the same epilogue on the first rows
        _same(_np(c[:len(sub)]), sr.epilogue_fwd(ref[:len(sub)].cpu().numpy(), _np(bias), epi, 0.5, mask[orig[:len(sub)]].cpu().numpy() != 0), "epi")
    else:
        bias = _dev(rng.normal(size=J).astype(np.float32))
        epi = sr.EPI_BIAS | sr.EPI_ELU | sr.EPI_DROPOUT
        word = torch.tensor([SEED], dtype=torch.int64, device="cuda") if with_rows else None     # seed by pointer / by value
        rc, c = _gemm_epi(L, a, b, I, J, K, rows, bias, epi | (sr.EPI_SEED_DEVICE if with_rows else 0), 0.5,
                          word.data_ptr() if with_rows else SEED, None, nbytes)
        L.check(rc, "fitgnn_gemm_exact_epi_f32")
        sel = np.arange(I) if I * J <= BIG else _sample_rows(I, plan.main_rows, rng)
        st = torch.from_numpy(sel).cuda()
        keep = sr.keep_matrix(SEED, orig[st].cpu().numpy(), J, 0.5)
        ez = _exact_bound_dev(S, K, plan)[st].cpu().numpy()
        _check_fwd(_np(c[st]), ref[st].cpu().numpy(), ez, _np(bias), epi, 0.5, keep, f"epi {case}")
        rc, c2 = _gemm_epi(L, a, b, I, J, K, rows, bias, epi | (sr.EPI_SEED_DEVICE if with_rows else 0), 0.5,
                           word.data_ptr() if with_rows else SEED, None, nbytes)
        assert rc == 0 and _eq(c, c2), "two launches on the same input differ"
        del word


def test_gemm_exact_epi_refusals(L):
    def launch(I=8, J=8, K=8, epi=sr.EPI_BIAS, p=0.0, bias=True, **kw):
        a, b = _operands("exact", "nt", I, J, K)
        bd = _dev(np.zeros(J, dtype=np.float32)) if bias else None
        nbytes = int(L.lib().fitgnn_gemm_exact_workspace_bytes(I, J, K, 0, 0))
        return _gemm_epi(L, a, b, I, J, K, None, bd, epi, p, 0, None, nbytes, **kw)[0]

    assert launch() == 0 and launch(J=6) == 0                                   # bias alone: any J
    assert launch(J=6, epi=sr.EPI_ELU) == E_BADARG and launch(J=6, epi=sr.EPI_DROPOUT, p=0.5) == E_BADARG
    assert launch(bias=False) == E_BADARG and launch(epi=sr.EPI_ELU, bias=False) == 0
    assert launch(epi=sr.EPI_DROPOUT, p=1.0) == E_BADARG and launch(epi=sr.EPI_DROPOUT, p=0.5) == 0
    assert launch(epi=16) == E_BADARG
    assert launch(K=6) == E_BADARG and launch(ldc=7) == E_BADARG
    assert G.plan_exact("nt", 5, 4, 1024).nchunks > 1 and launch(I=5, J=4, K=1024) == E_BADARG   # a plan split over k
    assert G.plan_exact("nt", 65537, 68, 516).main_rows > 0 and launch(I=65537, J=68, K=516, ws="null") == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# fitgnn_gemm_nt_f32, fitgnn_gemm_nt_presplit_f32 + fitgnn_gemm_nt_pre_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def _nt_bound_dev(S, K):
    return (G.split_dropped() + 3 * K * U * G.split_terms()) * S


def _check_product(family, kind, c, a, b, form, bound_of, what):
    ref, S = _product64(a, b, form)
    if kind == "exact":
        _bit_equal(c, ref, S, what)
    else:
        _bounded(family, c, ref, bound_of(S), what)


def _gemm_nt(L, a, b, R, N, K, ldc=None):
    ldc = N + 4 + (R & 1) if ldc is None else ldc
    cbuf, c = _output(R, N, ldc)
    rc = _call(L, "fitgnn_gemm_nt_f32", _p(L, a), a.stride(0), _p(L, b), b.stride(0), R, N, K, _p(L, c), ldc)
    _untouched(cbuf, R, N, ldc, "c")
    return rc, c


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("R,N,K", G.NT_CASES, ids=lambda v: str(v))
def test_gemm_nt(L, R, N, K, kind):
    variant = G.nt_variant(R, N)
    assert variant == (4 if R >= 32513 else 2), "the case reaches the tile variant it was chosen for"
    a, b = _padded(_values(kind, (R, K), "nt a")), _padded(_values(kind, (N, K), "nt b"))
    rc, c = _gemm_nt(L, a, b, R, N, K)
    L.check(rc, "fitgnn_gemm_nt_f32")
    _check_product(f"gemm_nt <{variant}>", kind, c, a, b, "nt", lambda S: _nt_bound_dev(S, K), f"c {(R, N, K)}")
    rc, c2 = _gemm_nt(L, a, b, R, N, K)
    assert rc == 0 and _eq(c, c2), "two launches on the same input differ"


def _image(L, b, K, K_valid, transposed):
    """The pre-split image of b [N x K_valid] for a stage width K, read through plain strides (ldb, 1) or through those of a transposed
    copy (1, ldb); exactly fitgnn_gemm_nt_presplit_bytes, NaN before the launch, followed by a guard."""
    N = b.shape[0]
    nbytes = int(L.lib().fitgnn_gemm_nt_presplit_bytes(N, K))
    assert nbytes == -(-N // 256) * (K // 32) * 32768
    img = torch.full((nbytes // 4 + GUARD,), NAN, dtype=torch.float32, device="cuda")
    if transposed:
        bt = _padded(b.t().contiguous())                     # element (n, k) at bt[k * ld + n]
        sn, sk, src = 1, bt.stride(0), bt
    else:
        src = _padded(b)                                      # NaN from column K_valid on
        sn, sk = src.stride(0), 1
    _run(L, "fitgnn_gemm_nt_presplit_f32", _p(L, src), sn, sk, N, K, K_valid, _p(L, img))
    assert torch.isnan(img[nbytes // 4:]).all().item(), "wrote past the image"
    return img


def _gemm_nt_pre(L, a, img, R, N, K):
    ldc = N + 4 + (R & 1)
    cbuf, c = _output(R, N, ldc)
    rc = _call(L, "fitgnn_gemm_nt_pre_f32", _p(L, a), a.stride(0), _p(L, img), R, N, K, _p(L, c), ldc)
    _untouched(cbuf, R, N, ldc, "c")
    return rc, c


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("R,N,K", G.NT_PRE_CASES, ids=lambda v: str(v))
def test_gemm_nt_pre(L, R, N, K, kind):
    a, b = _padded(_values(kind, (R, K), "pre a")), _values(kind, (N, K), "pre b")
    img = _image(L, b, K, K, transposed=(R + N // 4 + K // 32) % 2 == 0)
    rc, c = _gemm_nt_pre(L, a, img, R, N, K)
    L.check(rc, "fitgnn_gemm_nt_pre_f32")
    _check_product("gemm_nt_pre", kind, c, a, b, "nt", lambda S: _nt_bound_dev(S, K), f"c {(R, N, K)}")
    rc, c2 = _gemm_nt_pre(L, a, img, R, N, K)
    assert rc == 0 and _eq(c, c2), "two launches on the same input differ"


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("K,K_valid", [(32, 1), (32, 20), (32, 31), (64, 33), (96, 64)])
@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
def test_gemm_nt_pre_k_valid(L, transposed, K, K_valid, kind):
    """b has K_valid columns (the image's k >= K_valid are zero whatever lies behind them in memory: NaN here); a has all K, finite."""
    R, N = 257, 132
    a, b = _padded(_values(kind, (R, K), "kv a")), _values(kind, (N, K_valid), "kv b")
    img = _image(L, b, K, K_valid, transposed)
    rc, c = _gemm_nt_pre(L, a, img, R, N, K)
    L.check(rc, "fitgnn_gemm_nt_pre_f32")
    _check_product("gemm_nt_pre", kind, c, a[:, :K_valid], b, "nt", lambda S: _nt_bound_dev(S, K), f"c K_valid {K_valid} of {K}")


def test_gemm_nt_empty_and_refusals(L):
    R, N, K = 8, 8, 32
    a, b = _padded(_values("exact", (R, K), "ra")), _padded(_values("exact", (N, K), "rb"))
    lda = ldb = a.stride(0)
    img = _image(L, b, K, K, False)

    def nt(R=R, N=N, K=K, lda=lda, ldb=ldb, ldc=N + 4, pa=_p(L, a), pb=_p(L, b), null_c=False):
        cbuf, c = _output(max(R, 1), 8, 12)
        rc = _call(L, "fitgnn_gemm_nt_f32", pa, lda, pb, ldb, R, N, K, None if null_c else _p(L, c), ldc)
        if rc != 0 or R == 0:
            assert torch.isnan(cbuf).all().item(), "a refused or empty call wrote"
        return rc

    def pre(R=R, N=N, K=K, lda=lda, ldc=N + 4, pa=_p(L, a), pimg=_p(L, img)):
        cbuf, c = _output(max(R, 1), 8, 12)
        rc = _call(L, "fitgnn_gemm_nt_pre_f32", pa, lda, pimg, R, N, K, _p(L, c), ldc)
        if rc != 0 or R == 0:
            assert torch.isnan(cbuf).all().item(), "a refused or empty call wrote"
        return rc

    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + 4 * n)   # noqa: E731
    assert nt() == 0 and pre() == 0
    assert nt(R=0) == 0 and nt(R=0, pa=None, pb=None, null_c=True) == 0 and pre(R=0) == 0 and pre(R=0, pa=None, pimg=None) == 0
    assert nt(R=-1) == E_BADARG and nt(N=0) == E_BADARG and nt(K=16) == E_BADARG and nt(K=0) == E_BADARG
    assert nt(K=48, lda=52, ldb=52) == E_BADARG                                  # K % 32 != 0
    assert nt(lda=K - 4) == E_BADARG and nt(lda=K + 1) == E_BADARG and nt(ldb=K - 4) == E_BADARG and nt(ldb=K + 2) == E_BADARG
    assert nt(ldc=N - 1) == E_BADARG
    assert nt(pa=None) == E_BADARG and nt(pb=None) == E_BADARG and nt(null_c=True) == E_BADARG
    assert nt(pa=off(a, 1)) == E_ALIGN and nt(pb=off(b, 2)) == E_ALIGN and nt(pa=off(a, 4)) == 0
    assert pre(K=16) == E_BADARG and pre(lda=K + 1) == E_BADARG and pre(ldc=N - 1) == E_BADARG and pre(pimg=None) == E_BADARG
    assert pre(pa=off(a, 1)) == E_ALIGN and pre(pimg=ctypes.c_void_p(img.data_ptr() + 8)) == E_ALIGN

    def presplit(N=N, K=K, K_valid=K, pb=_p(L, b), shift=0):
        out = torch.full((32768 // 4 + GUARD,), NAN, dtype=torch.float32, device="cuda")
        rc = _call(L, "fitgnn_gemm_nt_presplit_f32", pb, ldb, 1, N, K, K_valid, ctypes.c_void_p(out.data_ptr() + shift))
        if rc != 0:
            assert torch.isnan(out).all().item(), "a refused call wrote"
        return rc

    assert presplit() == 0 and presplit(K_valid=1) == 0
    assert presplit(N=0) == E_BADARG and presplit(K=16) == E_BADARG and presplit(K=48) == E_BADARG
    assert presplit(K_valid=0) == E_BADARG and presplit(K_valid=K + 1) == E_BADARG and presplit(pb=None) == E_BADARG
    assert _call(L, "fitgnn_gemm_nt_presplit_f32", _p(L, b), ldb, 1, N, K, K, None) == E_BADARG
    assert presplit(shift=8) == E_ALIGN
    assert L.lib().fitgnn_gemm_nt_presplit_bytes(0, 32) == 0 and L.lib().fitgnn_gemm_nt_presplit_bytes(8, 48) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# fitgnn_gemm_atb_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def _gemm_atb(L, a, b, R, M, N):
    plan = G.AtbPlan(R, M, N)
    nbytes = int(L.lib().fitgnn_gemm_atb_workspace_bytes(R, M, N))
    assert nbytes == plan.workspace_bytes()
    obuf, out = _output(M, N, N)
    ws, wp = _workspace(nbytes)
    rc = _call(L, "fitgnn_gemm_atb_f32", _p(L, a), a.stride(0), _p(L, b), b.stride(0), R, M, N, _p(L, out), wp)
    _untouched(obuf, M, N, N, "out")
    _ws_guard(ws, nbytes, "atb")
    return rc, out, plan


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("R,M,N", G.ATB_CASES, ids=lambda v: str(v))
def test_gemm_atb(L, R, M, N, kind):
    a, b = _padded(_values(kind, (R, M), "atb a")), _padded(_values(kind, (R, N), "atb b"))
    rc, out, plan = _gemm_atb(L, a, b, R, M, N)
    L.check(rc, "fitgnn_gemm_atb_f32")
    coef = G.atb_bound(np.ones(()), R, plan)
    family = "gemm_atb" + (", scalar rows only" if plan.r_main == 0 else "")
    _check_product(family, kind, out, a, b, "tn", lambda S: float(coef) * S, f"out {(R, M, N)}")
    rc, out2, _ = _gemm_atb(L, a, b, R, M, N)
    assert rc == 0 and _eq(out, out2), "two launches on the same input differ"


def test_gemm_atb_refusals(L):
    R = 40
    a, b = _padded(_values("exact", (R, 8), "ra")), _padded(_values("exact", (R, 8), "rb"))
    ld = a.stride(0)
    out = torch.full((64 + GUARD,), NAN, dtype=torch.float32, device="cuda")
    ws = torch.full((int(L.lib().fitgnn_gemm_atb_workspace_bytes(R, 8, 8)) // 4 + GUARD,), NAN, dtype=torch.float32, device="cuda")
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)   # noqa: E731

    def atb(R=R, M=8, N=8, lda=ld, ldb=ld, pa=_p(L, a), pb=_p(L, b), po=_p(L, out), pw=_p(L, ws)):
        rc = _call(L, "fitgnn_gemm_atb_f32", pa, lda, pb, ldb, R, M, N, po, pw)
        if rc != 0:
            assert torch.isnan(out).all().item() and torch.isnan(ws).all().item(), "a refused call wrote"
        return rc

    assert atb(R=0) == E_BADARG and atb(R=-1) == E_BADARG
    assert atb(M=0) == E_BADARG and atb(M=2) == E_BADARG and atb(M=6) == E_BADARG and atb(N=2) == E_BADARG and atb(N=7) == E_BADARG
    assert atb(lda=4) == E_BADARG and atb(ldb=4) == E_BADARG and atb(lda=9) == E_BADARG and atb(ldb=10) == E_BADARG
    assert atb(pa=None) == E_BADARG and atb(pb=None) == E_BADARG and atb(po=None) == E_BADARG and atb(pw=None) == E_BADARG
    assert atb(pa=off(a, 4)) == E_ALIGN and atb(pb=off(b, 8)) == E_ALIGN and atb(po=off(out, 4)) == E_ALIGN and atb(pw=off(ws, 8)) == E_ALIGN
    assert L.lib().fitgnn_gemm_atb_workspace_bytes(0, 8, 8) == 0
    assert atb() == 0
