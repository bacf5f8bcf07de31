"""GPU tier: the exact product with operand rows read through a list (csrc/gemm_f32.hip: fitgnn_gemm_exact_rows_f32,
fitgnn_gemm_exact_epi_rows_f32) -- a_rows for a k-minor a (nt, nn), b_rows for a k-major b (tn, nn) -- through the C ABI.

Conventions of tests/test_gpu_gemm_kernels.py (its helpers, value sets and bounds are imported, not copied).  On top of them: the
source matrix is about three times as tall as the list is long and every row the list does not name is NaN; the list is unsorted,
repeats an entry and names the first and the last source row; it is followed by guard entries that hold the index of a NaN row (a
valid address), so a kernel that reads past the list poisons an output and cannot fault.  Every case is compared three ways:
torch.equal with the existing entry point on the gathered operand, EXACT values bit for bit with the float64 product, RANDOM values
inside the bound of gemm_reference; a second launch gives the same bits.

| branch | cases (form-I-J-K-shape-nchunks-main_rows) |
|---|---|
| a_rows, nt | S128x64 one tile [5-47-100], 9 row tiles [1025-64-100]; S256 with a tail launch whose list is moved by main_rows = 4096 and holds only the last entry [4097-4096-516] |
| a_rows, nn | S64x64 [65-68-36] (also with b_rows at once); S256 with a tail of three row tiles [7681-2052-512] |
| b_rows, tn | K not a multiple of 32, the list ends inside a stage: [132-132-31], [900-4-33]; S64x512 [64-516-36]; split over k, 20 empty chunks that must read no index [68-132-65536] |
| fused store | tails [65537-68-516], [65537-68-512]; S128 [7169-388-36]; BIAS + DROPOUT by mask bit for bit, BIAS + ELU + DROPOUT by hash through _check_fwd; a_rows and the dropout pattern's rows are the same array, as in the step |
| refusals | a_rows with a k-major a, b_rows with a k-minor b (FITGNN_E_BADARG), a list 4 bytes off (FITGNN_E_ALIGN): the output untouched |
"""
import ctypes

import numpy as np
import pytest
import torch

import gemm_reference as G
import step_reference as sr
from test_gpu_gemm_kernels import (GUARD, NAN, SEED, _assert_plan, _bit_equal, _bounded, _exact_bound_dev, _gemm_epi, _gemm_exact, _output,
                                   _padded, _product64, _untouched, _values, _workspace, _ws_guard)
from test_gpu_step_kernels import E_ALIGN, E_BADARG, L, _call, _check_fwd, _dev, _exact, _np, _p, _rng  # noqa: F401

pytestmark = pytest.mark.gpu

A_CASES = [("nt", 5, 47, 100, "S128x64", 1, 0), ("nt", 1025, 64, 100, "S128x64", 1, 0), ("nt", 4097, 4096, 516, "S256", 1, 4096),
           ("nn", 65, 68, 36, "S64x64", 1, 0), ("nn", 7681, 2052, 512, "S256", 1, 7168)]
B_CASES = [("tn", 132, 132, 31, "S128", 1, 0), ("tn", 900, 4, 33, "S128", 1, 0), ("tn", 64, 516, 36, "S64x512", 1, 0),
           ("tn", 68, 132, 65536, "S256", 248, 0), ("nn", 65, 68, 36, "S64x64", 1, 0)]
EPI_CASES = [("nt", 65537, 68, 516, "S256x128", 1, 65536), ("nt", 65537, 68, 512, "S256x128", 1, 65536), ("nt", 7169, 388, 36, "S128", 1, 0)]


def _row_list(n, rng):
    """(list with guards [n + GUARD] on the device, R): n entries of [0, R), R = 3 n + 2, unsorted, its last entry a repeat, rows 0 and
    R - 1 named; the guards hold a row the list does not name."""
    R = 3 * n + 2
    idx = rng.integers(0, R, size=n)
    if n >= 4:
        idx[n - 1] = idx[n - 2]
    idx[n // 2], idx[0] = 0, R - 1          # the first source row in the middle of the list, the last one at its head
    free = np.setdiff1d(np.arange(R), idx)
    guard = int(free[len(free) // 2])
    return _dev(np.concatenate([idx, np.full(GUARD, guard)]), torch.int64), R


def _source(kind, R, C, lst, n, *parts):
    """A [R x C] strided source whose rows outside lst[:n] are NaN, and the gathered operand as a strided matrix of its own."""
    vals = _values(kind, (R, C), *parts)
    named = torch.zeros(R, dtype=torch.bool, device="cuda")
    named[lst[:n]] = True
    vals[~named] = NAN
    src = _padded(vals)
    return src, _padded(src.index_select(0, lst[:n]))


def _lp(L, t):
    """Pointer of a list: a tensor, None, or a raw pointer (a misaligned one)."""
    return t if isinstance(t, ctypes.c_void_p) else _p(L, t)


def _gemm_rows(L, form, a, a_rows, b, b_rows, I, J, K, nbytes, ldc=None):
    akm, bkm = G.KMAJOR[form]
    ldc = J + 4 + (I & 1) if ldc is None else ldc
    cbuf, c = _output(I, J, ldc)
    ws, wp = _workspace(nbytes)
    rc = _call(L, "fitgnn_gemm_exact_rows_f32", _p(L, a), a.stride(0), akm, _lp(L, a_rows), _p(L, b), b.stride(0), bkm, _lp(L, b_rows), I, J, K,
               _p(L, c), ldc, wp)
    if rc == 0:
        _untouched(cbuf, I, J, ldc, "c")
    else:
        assert torch.isnan(cbuf).all().item(), "a refused call wrote"
    _ws_guard(ws, nbytes, "rows")
    return rc, c


def _check_case(L, case, kind, use_a, use_b):
    form, I, J, K = case[:4]
    plan, nbytes = _assert_plan(L, case)
    rng = _rng("rows", case, kind, use_a, use_b)
    sa, sb = G.operand_shapes(form, I, J, K)
    if use_a:
        la, Ra = _row_list(I, rng)
        a, ag = _source(kind, Ra, sa[1], la, I, "a", case)
    else:
        la, a = None, _padded(_values(kind, sa, "a", case))
        ag = a
    if use_b:
        lb, Rb = _row_list(K, rng)
        b, bg = _source(kind, Rb, sb[1], lb, K, "b", case)
    else:
        lb, b = None, _padded(_values(kind, sb, "b", case))
        bg = b
    rc, c = _gemm_rows(L, form, a, la, b, lb, I, J, K, nbytes)
    L.check(rc, "fitgnn_gemm_exact_rows_f32")
    rc, cg = _gemm_exact(L, form, ag, bg, I, J, K, nbytes)
    assert rc == 0 and torch.equal(c, cg), f"{case}: differs from the product of the gathered operand"
    ref, S = _product64(ag, bg, form)
    if kind == "exact":
        _bit_equal(c, ref, S, f"c {case}")
    else:
        _bounded(f"rows {form}", c, ref, _exact_bound_dev(S, K, plan), f"c {case}")
    rc, c2 = _gemm_rows(L, form, a, la, b, lb, I, J, K, nbytes)
    assert rc == 0 and torch.equal(c, c2), "two launches on the same input differ"


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", A_CASES, ids=G.case_id)
def test_gemm_a_rows(L, case, kind):
    _check_case(L, case, kind, True, False)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", B_CASES, ids=G.case_id)
def test_gemm_b_rows(L, case, kind):
    _check_case(L, case, kind, case[0] == "nn", True)   # (nn: both lists at once)


def _gemm_epi_rows(L, a, a_rows, b, I, J, K, rows, bias, epi, p, seed, mask, nbytes):
    ldc = J + 4
    cbuf, c = _output(I, J, ldc)
    wbuf, wp = _workspace(nbytes)
    rc = _call(L, "fitgnn_gemm_exact_epi_rows_f32", _p(L, a), a.stride(0), _lp(L, a_rows), _p(L, b), b.stride(0), I, J, K, _p(L, c), ldc,
               _p(L, rows), _p(L, bias), epi, p, seed, _p(L, mask), wp)
    if rc == 0:
        _untouched(cbuf, I, J, ldc, "c")
    else:
        assert torch.isnan(cbuf).all().item(), "a refused call wrote"
    _ws_guard(wbuf, nbytes, "epi rows")
    return rc, c


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", EPI_CASES, ids=G.case_id)
def test_gemm_epi_a_rows(L, case, kind):
    """The list is both a_rows and the dropout pattern's original rows.  EXACT: bias + dropout by mask at p = 0.5, bit for bit over
    the whole output.  RANDOM: bias + ELU + dropout by hash against step_reference.epilogue_fwd of the float64 product."""
    form, I, J, K = case[:4]
    plan, nbytes = _assert_plan(L, case)
    rng = _rng("epi rows", case, kind)
    lst, R = _row_list(I, rng)
    a, ag = _source(kind, R, K, lst, I, "a", case)
    b = _padded(_values(kind, (J, K), "b", case))
    orig = lst[:I]
    ref, S = _product64(ag, b, form)
    if kind == "exact":
        bias = _dev(_exact(rng, (J,)))
        mask = (torch.rand((R, J), device="cuda") < 0.5).to(torch.uint8)
        args = (bias, sr.EPI_BIAS | sr.EPI_DROPOUT, 0.5, 0, mask, nbytes)
    else:
        bias = _dev(rng.normal(size=J).astype(np.float32))
        args = (bias, sr.EPI_BIAS | sr.EPI_ELU | sr.EPI_DROPOUT, 0.5, SEED, None, nbytes)
    rc, c = _gemm_epi_rows(L, a, lst, b, I, J, K, lst, *args)
    L.check(rc, "fitgnn_gemm_exact_epi_rows_f32")
    rc, cg = _gemm_epi(L, ag, b, I, J, K, orig.contiguous(), *args)
    assert rc == 0 and torch.equal(c, cg), f"{case}: differs from the fused product of the gathered operand"
    if kind == "exact":
        want = torch.where(mask[orig] != 0, (ref + bias.to(torch.float64)[None, :]) * 2.0, torch.zeros((), dtype=torch.float64, device="cuda"))
        _bit_equal(c, want, S + 0.125, f"epi {case}")
    else:
        sel = np.unique(np.concatenate([np.arange(200), np.arange(I - 200, I), rng.integers(0, I, size=600),
                                        np.arange(max(plan.main_rows - 200, 0), min(plan.main_rows + 200, I))]))
        st = torch.from_numpy(sel).cuda()
        keep = sr.keep_matrix(SEED, orig[st].cpu().numpy(), J, 0.5)
        ez = _exact_bound_dev(S, K, plan)[st].cpu().numpy()
        _check_fwd(_np(c[st]), ref[st].cpu().numpy(), ez, _np(bias), args[1], 0.5, keep, f"epi {case}")
    rc, c2 = _gemm_epi_rows(L, a, lst, b, I, J, K, lst, *args)
    assert rc == 0 and torch.equal(c, c2), "two launches on the same input differ"


def test_gemm_rows_refusals(L):
    rng = _rng("rows refusals")
    I = J = K = 8
    lst, R = _row_list(8, rng)
    off = ctypes.c_void_p(lst.data_ptr() + 4)
    bias = _dev(np.zeros(J, dtype=np.float32))

    def launch(form, a_rows=None, b_rows=None):
        sa, sb = G.operand_shapes(form, I, J, K)
        a = _padded(_values("exact", (R if a_rows is not None and form != "tn" else sa[0], sa[1]), "ra"))
        b = _padded(_values("exact", (R if b_rows is not None and form != "nt" else sb[0], sb[1]), "rb"))
        return _gemm_rows(L, form, a, a_rows, b, b_rows, I, J, K, 0)[0]

    def epi(a_rows):
        a, b = _padded(_values("exact", (R, K), "ra")), _padded(_values("exact", (J, K), "rb"))
        return _gemm_epi_rows(L, a, a_rows, b, I, J, K, None, bias, sr.EPI_BIAS, 0.0, 0, None, 0)[0]

    assert launch("nt", a_rows=lst) == 0 and launch("nn", a_rows=lst, b_rows=lst) == 0 and launch("tn", b_rows=lst) == 0 and epi(lst) == 0
    assert launch("tn", a_rows=lst) == E_BADARG                       # a list for a k-major a
    assert launch("nt", b_rows=lst) == E_BADARG                       # a list for a k-minor b
    assert launch("nt", a_rows=off) == E_ALIGN and launch("tn", b_rows=off) == E_ALIGN and launch("nn", b_rows=off) == E_ALIGN
    assert epi(off) == E_ALIGN
