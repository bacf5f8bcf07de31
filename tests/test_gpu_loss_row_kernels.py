"""GPU tier: the loss-row kernels of the GCN step after their memory-access rewrite -- the head backward with one LDS read of the
head's weight per class and U rows (epilogue_bwd_kernel, HEAD path), the loss and the narrow column sum through an LDS row tile
(softmax_nll_kernel, narrow_colsum_kernel) and the forward epilogue in the exact GEMM's store (fitgnn_gemm_exact_epi_f32) -- through
the C ABI against the float64 references of tests/step_reference.py, in the style of tests/test_gpu_step_kernels.py: EXACT inputs bit
for bit, RANDOM inputs within the reference's derived bound (that module's docstring derives the softmax bound used here).

Head backward.  A workgroup takes a chunk of chunk_rows_for(n) rows (4 up to n = 4 096, 8 at 4 097, 20 at 20 011), wave w of it the
rows w, w + 4, ... in groups of U = 4: n in {1, 15, 16, 17, 31, 33, 4097} put the last chunk's end at every position of a group of
one or two rows; n = 20 011 (added here) has chunks of 20 rows = a full group of four rows per wave and a group of one.  Rows of
zeros in dy sit first (row 0), last (row 13) and alone (row 6) inside such a group, and fill one whole group (rows 3, 7, 11, 15: no
product is formed).  Class c's dy value is fetched by lane c, so a head needs C <= (columns of the last 256-column slab) / 4 lanes
whenever H % 4 == 0 (and C <= columns of the last 64-column slab in the one-column form, which operands one float off 16-byte
alignment take): of C in {17, 47, 48} x H in {36, 260, 512} the launcher takes H = 512 (both forms) and refuses the others, which
test_head_backward_refusals holds it to; C = 9 at H = 36 (both forms) and C = 1 at H = 260 (the ragged last slab) are added so
that those widths are computed as well.

Fused GEMM store.  The two-launch result (fitgnn_gemm_exact_f32, then fitgnn_epilogue_fwd_rows_f32 or torch's broadcast add) is
the reference, compared with torch.equal.  test_fused_gemm_cases_cover_the_plans holds the case list to at least two tile shapes
and one plan with the tail sub-launch (33 000 x 512 x 512: 129 x 2 tiles of 256 x 256 = one round and two tiles).
"""
import ctypes

import numpy as np
import pytest
import torch

import step_reference as sr
from graph_fixtures import star_blocks
from test_gpu_step_kernels import (E_BADARG, L, _check_softmax, _colsum, _dev, _dropout, _exact, _np, _offset_copy,  # noqa: F401
                                   _out_exact, _p, _rng, _run, _call, _same, _softmax_nll)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------------
# head backward on selected rows
# ---------------------------------------------------------------------------------------------------------------------------------
HEAD_N = [1, 15, 16, 17, 31, 33, 4097]
# (C, H, offset in floats of out / dZ): offset 1 takes the one-column form
HEAD_TAKEN = [(9, 36, 0), (9, 36, 1), (17, 512, 0), (47, 512, 0), (48, 512, 0), (17, 512, 1), (47, 512, 1), (48, 512, 1), (1, 260, 0)]
HEAD_REFUSED = [(17, 36, 0), (17, 36, 1), (47, 36, 0), (48, 36, 0), (47, 36, 1), (48, 36, 1), (17, 260, 0), (47, 260, 0), (48, 260, 0), (17, 260, 1)]


def _zero_rows(n):
    z = [r for r in (0, 13, 6, 3, 7, 11, 15) if r < n]
    return np.array(z + ([n - 1] if n > 40 else []), dtype=np.int64)


def _head_rows_case(L, n, C, H, offset, compact_in, drop, R_extra=29):
    rng = _rng("loss_rows_head", n, C, H, offset, compact_in, drop)
    R = n + R_extra
    sel = rng.permutation(R)[:n]
    dy = _exact(rng, (R, C), lo=-4, hi=4)
    dy[sel[rng.random(n) < 0.15]] = 0.0
    dy[sel[_zero_rows(n)]] = 0.0
    Wl = _exact(rng, (C, H), lo=-4, hi=4)
    out = _out_exact(rng, (R, H), den=8)
    epi, seed, mask, word, keep = _dropout(drop, R, H, rng)
    epi |= sr.EPI_ELU
    take = (lambda a: a[sel]) if compact_in else (lambda a: a)
    dyd, Wd, st = _dev(take(dy)), _dev(Wl), _dev(sel, torch.int64)
    od = _offset_copy(take(out), offset)
    wb = int(L.lib().fitgnn_epilogue_bwd_head_workspace_bytes(n, H, C))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    rdZ, rdb, _, _, _ = sr.epilogue_bwd_head(dy[sel], Wl, out[sel], epi, 0.5, keep(sel))
    for with_db in (True, False):
        dZ = _offset_copy(np.full((n, H), np.nan, np.float32), offset)
        db = torch.full((H,), float("nan"), device="cuda") if with_db else None
        _run(L, "fitgnn_epilogue_bwd_head_rows_f32", _p(L, dyd), _p(L, Wd), C, _p(L, od), _p(L, st), n, compact_in, _p(L, dZ), H, epi, 0.5,
             seed, _p(L, mask), _p(L, db), None, _p(L, work), wb)
        got = _np(dZ)
        _same(got, rdZ, "dZ")
        zero = np.all(dy[sel] == 0, axis=1)
        assert not np.signbit(got[zero]).any(), "a row outside the loss must be +0"
        if with_db:
            _same(_np(db), rdb, "db")
    del word


@pytest.mark.parametrize("drop", ["hash", "hash_ptr", "mask"])
@pytest.mark.parametrize("compact_in", [0, 1])
@pytest.mark.parametrize("C,H,offset", HEAD_TAKEN, ids=lambda v: str(v))
@pytest.mark.parametrize("n", HEAD_N)
def test_head_backward_rows(L, n, C, H, offset, compact_in, drop):
    _head_rows_case(L, n, C, H, offset, compact_in, drop)


@pytest.mark.parametrize("compact_in", [0, 1])
@pytest.mark.parametrize("C,offset", [(47, 0), (17, 1)])
def test_head_backward_full_groups(L, C, offset, compact_in):
    """chunks of 20 rows: every wave has a full group of U rows in flight, then a group of one"""
    _head_rows_case(L, 20011, C, 512, offset, compact_in, "hash")


@pytest.mark.parametrize("C,H,offset", HEAD_REFUSED, ids=lambda v: str(v))
def test_head_backward_refusals(L, C, H, offset):
    n = 8
    dy, Wl = torch.zeros(n, C, device="cuda"), torch.zeros(C, H, device="cuda")
    out = _offset_copy(np.zeros((n, H), np.float32), offset)
    dZ = _offset_copy(np.zeros((n, H), np.float32), offset)
    st = torch.arange(n, device="cuda")
    wb = int(L.lib().fitgnn_epilogue_bwd_head_workspace_bytes(n, H, C))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    rc = _call(L, "fitgnn_epilogue_bwd_head_rows_f32", _p(L, dy), _p(L, Wl), C, _p(L, out), _p(L, st), n, 1, _p(L, dZ), H, 0, 0.0, 0, None,
               None, None, _p(L, work), wb)
    assert rc in (-1, -3), rc   # FITGNN_E_BADARG, or FITGNN_E_ALIGN where only the alignment rules the float4 form out


# ---------------------------------------------------------------------------------------------------------------------------------
# softmax + NLL through the LDS row tile
# ---------------------------------------------------------------------------------------------------------------------------------
# (n, C, ldz); C = 130 is beyond the 128-column tile: the row-walking form
@pytest.mark.parametrize("consecutive", [False, True])
@pytest.mark.parametrize("n,C,ldz", [(1, 1, 1), (255, 2, 2), (256, 47, 47), (257, 47, 50), (513, 64, 67), (300, 128, 128), (300, 130, 131)],
                         ids=lambda v: str(v))
def test_softmax_nll_tile(L, n, C, ldz, consecutive):
    rng = _rng("loss_rows_softmax", n, C, consecutive)
    n_rows = n + 37
    z = rng.normal(0, 3, size=(n_rows, C)).astype(np.float32)
    idx = (5 + np.arange(n)) if consecutive else rng.permutation(n_rows)[:n]   # consecutive + ldz == C: one contiguous span
    labels = rng.integers(0, C, size=n)
    loss, dz = _softmax_nll(L, z, ldz, idx, labels, 0.125)
    _check_softmax(z, idx, labels, 0.125, loss, dz, ldz)


def test_softmax_nll_tile_extreme_rows(L):
    rng = _rng("loss_rows_softmax_extreme")
    C, n_rows = 47, 600
    z = rng.normal(0, 3, size=(n_rows, C)).astype(np.float32)
    z[3] = np.where(np.arange(C) % 2 == 0, 80.0, -80.0)
    z[4] = -80.0
    z[5] = 0.0; z[5, 7] = 120.0                    # dominant: every other exp(z - lse) is below fp32's range
    idx = np.concatenate([[3, 4, 5], 6 + rng.permutation(n_rows - 6)[:297]])   # 300 rows: the tile of 256 and a ragged one
    labels = rng.integers(0, C, size=300); labels[2] = 7
    loss, dz = _softmax_nll(L, z, C, idx, labels, 0.25)
    _check_softmax(z, idx, labels, 0.25, loss, dz, C)
    assert torch.all(dz[5] == 0).item(), "the dominant row's gradient must underflow to exactly zero (its label is the dominant class)"


# ---------------------------------------------------------------------------------------------------------------------------------
# narrow column sum through the LDS row tile
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C", [(1, 5), (255, 47), (257, 47), (65537, 64)])
def test_colsum_narrow_tile(L, n, C):
    x = _exact(_rng("loss_rows_colsum", n, C), (n, C))
    rc, out = _colsum(L, x, C + 3)
    L.check(rc, "colsum")
    _same(_np(out[:C]), sr.colsum(x)[0], f"n={n}")
    assert np.isnan(out[C].item()), "wrote past column C"


# ---------------------------------------------------------------------------------------------------------------------------------
# the forward epilogue in the exact GEMM's store
# ---------------------------------------------------------------------------------------------------------------------------------
GEMM_CASES = [(I, J, K) for I in (1, 33, 257, 1300) for J in (64, 260, 512) for K in (32, 100, 512)] + [(33000, 512, 512)]
EPI_KINDS = [("bias", False, "none"), ("bias+elu", True, "none"), ("bias+elu+hash", True, "hash"), ("elu+mask", True, "mask"),
             ("hash_ptr", False, "hash_ptr")]


def _plan(L, I, J, K):
    shape, nchunks, main_rows = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    assert L.lib().fitgnn_gemm_exact_plan(I, J, K, 0, 0, ctypes.byref(shape), ctypes.byref(nchunks), ctypes.byref(main_rows)) == 0
    return shape.value, nchunks.value, main_rows.value


def _ws(L, I, J, K):
    wb = int(L.lib().fitgnn_gemm_exact_workspace_bytes(I, J, K, 0, 0))
    return torch.empty(max(wb // 4, 4), dtype=torch.float32, device="cuda")


def _gemm_two_launches(L, a, b, I, J, K, ldc, rows, bias, epi, p, seed, mask):
    c = torch.full((I, ldc), float("nan"), device="cuda")
    ws = _ws(L, I, J, K)
    _run(L, "fitgnn_gemm_exact_f32", _p(L, a), a.stride(0), 0, _p(L, b), b.stride(0), 0, I, J, K, _p(L, c), ldc, _p(L, ws))
    if J % 4 == 0:
        _run(L, "fitgnn_epilogue_fwd_rows_f32", _p(L, c), ldc, _p(L, rows), I, J, _p(L, bias), epi, p, seed, _p(L, mask))
    else:   # the head: y + bl
        assert epi == sr.EPI_BIAS
        c[:, :J] = c[:, :J] + bias
    return c


def _gemm_fused(L, a, b, I, J, K, ldc, rows, bias, epi, p, seed, mask):
    c = torch.full((I, ldc), float("nan"), device="cuda")
    ws = _ws(L, I, J, K)
    rc = _call(L, "fitgnn_gemm_exact_epi_f32", _p(L, a), a.stride(0), _p(L, b), b.stride(0), I, J, K, _p(L, c), ldc, _p(L, rows), _p(L, bias),
               epi, p, seed, _p(L, mask), _p(L, ws))
    return rc, c


def test_fused_gemm_cases_cover_the_plans(L):
    plans = [_plan(L, *case) for case in GEMM_CASES]
    assert all(nc == 1 for _, nc, _ in plans), "a case splits k: the fused entry refuses it"
    assert len({sh for sh, _, _ in plans}) >= 2, plans
    assert any(mr > 0 for _, _, mr in plans), "no case has the tail sub-launch"


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("I,J,K", GEMM_CASES, ids=lambda v: str(v))
def test_fused_gemm_store_equals_two_launches(L, I, J, K, with_rows):
    rng = _rng("loss_rows_gemm", I, J, K, with_rows)
    R = I + 50
    a = _dev(rng.normal(0, 1, size=(I, K)).astype(np.float32))
    b = _dev(rng.normal(0, 1, size=(J, K)).astype(np.float32) / np.float32(np.sqrt(K)))
    bias = _dev(rng.normal(0, 1, size=J).astype(np.float32))
    rows = _dev(rng.permutation(R)[:I], torch.int64) if with_rows else None
    ldc = J + 4
    for name, elu, drop in EPI_KINDS:
        epi, seed, mask, word, _ = _dropout(drop, R, J, rng)
        epi |= (sr.EPI_BIAS if "bias" in name else 0) | (sr.EPI_ELU if elu else 0)
        ref = _gemm_two_launches(L, a, b, I, J, K, ldc, rows, bias, epi, 0.5, seed, mask)
        rc, got = _gemm_fused(L, a, b, I, J, K, ldc, rows, bias, epi, 0.5, seed, mask)
        assert rc == 0, (name, rc)
        assert torch.equal(got[:, :J], ref[:, :J]), f"{name}: {(got[:, :J] != ref[:, :J]).sum().item()} entries differ"
        assert torch.isnan(got[:, J:]).all().item(), f"{name}: wrote into the row padding"
        if drop != "none":
            assert (got[:, :J] == 0).float().mean().item() > 0.3, f"{name}: dropout dropped too little to have been applied"
        del word


@pytest.mark.parametrize("K", [32, 512])
@pytest.mark.parametrize("I", [1, 33, 257, 1300])
def test_fused_gemm_bias_only_head(L, I, K):
    J = 47
    rng = _rng("loss_rows_gemm_head", I, K)
    a = _dev(rng.normal(0, 1, size=(I, K)).astype(np.float32))
    b = _dev(rng.normal(0, 1, size=(J, K)).astype(np.float32))
    bias = _dev(rng.normal(0, 1, size=J).astype(np.float32))
    ref = _gemm_two_launches(L, a, b, I, J, K, J, None, bias, sr.EPI_BIAS, 0.0, 0, None)
    rc, got = _gemm_fused(L, a, b, I, J, K, J, None, bias, sr.EPI_BIAS, 0.0, 0, None)
    assert rc == 0
    assert torch.equal(got, ref)


def test_fused_gemm_refusals(L):
    a, b47, bias = torch.zeros(64, 32, device="cuda"), torch.zeros(47, 32, device="cuda"), torch.zeros(512, device="cuda")
    # ELU / dropout index groups of four columns of a row: J % 4 != 0 is refused (the bias alone is not)
    for epi in (sr.EPI_ELU, sr.EPI_DROPOUT, sr.EPI_BIAS | sr.EPI_ELU):
        rc, _ = _gemm_fused(L, a, b47, 64, 47, 32, 47, None, bias, epi, 0.5, 1, None)
        assert rc == E_BADARG, epi
    rc, _ = _gemm_fused(L, a, b47, 64, 47, 32, 47, None, bias, sr.EPI_BIAS, 0.0, 0, None)
    assert rc == 0
    rc, _ = _gemm_fused(L, a, b47, 64, 47, 32, 47, None, None, sr.EPI_BIAS, 0.0, 0, None)
    assert rc == E_BADARG, "bias flag without a bias"
    # a plan that splits k has no single store for the epilogue
    I, J, K = 256, 512, 8192
    assert _plan(L, I, J, K)[1] > 1
    ak, bk = torch.zeros(I, K, device="cuda"), torch.zeros(J, K, device="cuda")
    rc, _ = _gemm_fused(L, ak, bk, I, J, K, J, None, bias, sr.EPI_BIAS, 0.0, 0, None)
    assert rc == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the route: FusedGCNLastLayerRows with the epilogue in the GEMM's store and as launches of its own
# ---------------------------------------------------------------------------------------------------------------------------------
def test_last_layer_rows_fused_store_gives_the_same_bits(L):
    from fitgnn_amd import csr, ops
    sizes = [40, 7, 130, 64, 300, 19, 90]
    ei, n = star_blocks(sizes, 2, seed=11)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    g = csr.CSRGraph(ei.cuda(), n, mode="gcn", ptr=ptr)
    K, H, C = 64, 256, 47   # (the head backward takes C <= H / 4 classes)
    torch.manual_seed(5)
    rows = torch.randperm(n).cuda()[: n // 3].sort().values
    labels = torch.randint(0, C, (rows.numel(),)).cuda()
    base = [torch.randn(n, K).cuda(), torch.randn(H, K).cuda() / 8, torch.randn(H).cuda(), torch.randn(C, H).cuda() / 8, torch.randn(C).cuda()]
    results = []
    for fused in (True, False):
        cfg = ops.OpConfig(fused_gemm_epilogue=fused)
        X, W, b, Wl, bl = (t.clone().requires_grad_(True) for t in base)
        y = ops.FusedGCNLastLayerRows.apply(X, W, b, Wl, bl, g, 0.5, True, 1234, None, rows, cfg, None, True)
        loss = torch.nn.functional.cross_entropy(y, labels)
        loss.backward()
        results.append([y.detach(), loss.detach()] + [t.grad for t in (X, W, b, Wl, bl)])
    for name, u, v in zip(("logits", "loss", "dX", "dW", "db", "dWl", "dbl"), *results):
        assert torch.equal(u, v), name
    assert (results[0][0] != 0).any().item()
