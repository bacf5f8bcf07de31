"""GPU tier: the small per-step kernels of csrc/gcn_ops.hip (the losses, Adam, the head on the loss rows, the narrow column sum, the
epilogue backward / forward on rows, the narrow-K layer and its backward) through the C ABI against the float64 references of
tests/step_reference.py.

Two kinds of input.  EXACT inputs (small integers times 1/64 or 1/32, dropout p = 0.5, power-of-two scales) keep every fp32
partial result exact, so a kernel must return the float64 result bit for bit whatever its summation order.  RANDOM inputs are held
to a per-entry bound, k * 2^-24 * (sum of |terms| of that entry), never to a fraction of the whole output's largest value.

Launcher -> branch -> tests that reach it:

| launcher | branch (from the launch code) | tests |
|---|---|---|
| fitgnn_softmax_nll_f32 | n = 0: dz cleared, loss 0 | test_softmax_nll_empty |
| | one block (n <= 256) / several; sum_partials_kernel with blocks > 256 (n = 70 001: 274 partials, two per thread) | test_softmax_nll[n1-*, n255-*, n256-*, n257-*, n70001-*] |
| | C = 1, 2, 47, 64, 65, 1000; ldz > C (ldz % 4 != 0); unsorted idx, unselected rows exactly 0 | test_softmax_nll[*] |
| | logits +-80, one dominant logit (the others' dz underflow to 0) | test_softmax_nll_extreme_rows |
| fitgnn_l1_loss_f32 | n = 0, 1, 255, 256, 257, 100 000 (one workgroup, grid-stride), ties | test_l1_loss |
| fitgnn_adam_step_f32 | n = 4, n / 4 = 1 300 (not a multiple of 256), 4 000 000; wd 0 / > 0; state at t = 0, 1 000, 10 000 | test_adam_one_step[plain-*] |
| fitgnn_adam_step_acc_f32 | the same shapes (1 300 float4: two workgroups, the second partial; 10^6: 977 workgroups of tickets); g_new NULL / given; seeds advanced once, ticket back to 0, step count + 1, g_new cleared | test_adam_one_step[acc-*] |
| | bias corrections formed in double (first 30 steps against the f64 formula with the fp32 betas) | test_adam_first_steps |
| | captured graph replayed 50 times == 50 eager steps | test_adam_graph_replay_equals_eager |
| | 1 000 steps against torch.optim.Adam | test_adam_against_torch_optim_adam |
| fitgnn_head_rows_f32 | P = 64 / pow2(C) lanes per class capped by H / 4: C in {1, 3, 16, 17, 47, 64} x H in {4, 12, 36, 512, 1024} where the LDS fits (P = 1 ... 64) | test_head_rows_grid |
| | second class pass: C = 65, 130 at H = 36, 128 | test_head_rows_second_class_pass |
| | n_rows = 1, 5 (ragged group), 4 097, 20 000 (grid-stride: blocks capped at 256); ldo > H; out_compact 0 / 1; bl NULL | test_head_rows_rows |
| | LDS refusal (H = 512, C = 65: 166 928 bytes) | test_head_rows_lds_refusal |
| fitgnn_colsum_narrow_f32 (+ colsum_partials_kernel) | C = 1 ... 64, ldx > C; C = 65 refused; n = 1, 70 000 (rows_per_block = 274 > 256) | test_colsum_narrow_every_width, test_colsum_narrow_rows |
| fitgnn_epilogue_bwd_f32 | <4, false, 0> (H % 4 == 0), <1, false, 0> (H = 37; H = 64 with out offset by one float); n across chunk_rows_for's switch (4 096 / 4 097); mask, hash by value, hash by pointer | test_epilogue_bwd_plain |
| fitgnn_epilogue_bwd_head_f32 | <4, true, 0>, <1, true, 0> (no dWl, C up to 48); <4 / 1, true, 4> (dWl, C = 1, 4); <4 / 1, true, 16> (dWl, C = 5, 16) | test_epilogue_bwd_head |
| | refusals: C = 17 with dWl, C = 49 without; head_supported at H = 260; unaligned H = 68 -> FITGNN_E_ALIGN | test_epilogue_bwd_head_refusals |
| fitgnn_epilogue_bwd_head_rows_f32 / _rows_f32 | sel with compact_in 0 / 1, hash of the ORIGINAL row | test_epilogue_bwd_selected_rows |
| fitgnn_epilogue_fwd_rows_f32 | rows NULL / given, ldz > H, mask / hash, ELU with __expf | test_epilogue_fwd_rows |
| fitgnn_dense_narrow_k_f32 | K = 1, 8, 11, 31, 32; H = 4, 16, 36 (item loop: H / 4 does not divide 256), 512; K = 32 at H = 512 refused; n = 1, 7, 4 096, 4 097, 60 000 (rows_per_block 8 / 9 / 118); lda, ldw > K, ldo > H; every flag combination | test_dense_narrow_k_shapes, test_dense_narrow_k_epilogues, test_dense_narrow_k_lds_refusal |
| fitgnn_narrow_atb_f32 | KT = 8 (K = 1, 8), 16 (K = 9, 16), 32 (K = 17, 32); H = 16, 64, 512, 1 024; H = 96 refused; n = 1, 15, 16, 17, 50 000; prev NULL / given with ELU, dropout (mask / hash) | test_narrow_atb_shapes, test_narrow_atb_epilogues, test_narrow_atb_refusal |
| fitgnn_gemm_nt_epilogue_bwd_f32 (csrc/gemm_nt.hip, <4, true, PRE>) | operand forms: plain b with ldb > K (PRE = false: waves 0-3 stage a, 4-7 stage b) and the pre-split image made by fitgnn_gemm_nt_presplit_f32 from a transposed view (ldb == 0, PRE = true: LDS-DMA); K = 32 (one stage: every prefetch re-reads it), 96 (three) | test_gemm_nt_epilogue_bwd_exact[plain-* / image-*] |
| | row tiles: R = 1, 5 (rows clamped to R - 1, one live row group), 255, 256, 257 (a second tile of one row), 2049 (9 tiles: the second group of eight, tm = 8 on XCD slot 0, the slots of tm = 9 ... 15 return); bias-gradient partials of a partial tile | test_gemm_nt_epilogue_bwd_exact[*-R*] |
| | column tiles: N = 4 (one live lane per half wave, nc clamped to N - 4 = 0), 128 (wn = 1 dead), 260 (second column tile with one live lane: its dropout group and its `out` reads at nc = N - 4) | test_gemm_nt_epilogue_bwd_exact[*-N*] |
| | epilogue: flags 0, ELU, DROPOUT, both; mask, hash seed by value, by pointer; db given / NULL (no fitgnn_colsum_partials_f32 launch) | test_gemm_nt_epilogue_bwd_exact, test_gemm_nt_epilogue_bwd_without_db |
| | RANDOM operands against float64; two launches give the same bits | test_gemm_nt_epilogue_bwd_random |
| | N = 6, p = 1, `out` one float into its buffer (FITGNN_E_ALIGN), workspace one byte short (FITGNN_E_WORKSPACE), K = 48, lda % 4 != 0 | test_gemm_nt_epilogue_bwd_refusals |
| all fixed-order sums | two launches on RANDOM inputs give the same bits | test_repeat_launches_give_the_same_bits |

Bounds that are not bit-exact:
* softmax: dz[c] of a selected row within scale * (sm_c * 4u (|z_c| + 2|lse| + |m| + C + 8) + 2u |sm_c - onehot|), sm the float64
  softmax, lse / m the float64 logsumexp / max of the row (expf's and logf's few-ulp errors, the argument z - lse rounded).
* Adam, one step against the float64 formula with the fp32 betas the kernel receives: |p - p64| <= u |p64| + 12u |update| +
  (lr / bc1) / denom * 4u (b1 |m_old| + (1 - b1)(|g| + wd |p|)); m and v likewise.
* Adam against torch.optim.Adam (fp32 on the GPU, Python-double betas) over T = 1 000 steps, same gradients:
  |p - p_torch| <= T lr (3.2 * 1e-5 + 6 * 32 u) + 2u sum_t max|p_t|.  The per-update relative gap is at most 6.5e-6 from the
  betas alone (torch weights exp_avg_sq with fp32(1 - 0.999) and bias-corrects with 1 - 0.999^t, the kernel uses fp32(0.999)
  for both), under 1e-5 with both sides' rounding; an Adam update is at most lr (1 - b1) / sqrt(1 - b2) < 3.2 lr; the moment
  rounding can reach 3u |g|max / rms(g) <= 3u * 32 of an update per side.
* ELU through __expf (forward epilogue, dense_narrow_k): for y = z + b <= 0, |elu - expm1(y)| <= u (exp(y)(4 + 2|y| + e_y / u) +
  |expm1(y)|) with e_y the bound on y itself (the exp2 argument y log2(e) rounds twice, v_exp_f32 is within 1 ulp, the
  subtraction of 1 rounds once); times 2 as margin, and the dropout scale.
* gemm_nt_epilogue_bwd on RANDOM operands: |dZ - ref| <= 2e-5 max|a b^T| |factor| + 2u |ref| per entry: 2e-5 of the largest product
  entry is what test_linear_gemm_matches_f64 holds the three-product bf16 split to (the dropped lo.lo terms are 2^-16 relative per
  product, fp32 accumulation over K adds K u); at p = 0.5 the scale 2 and o = out / 2 are exact, so the epilogue rounds twice
  (o + 1, then the product).  db: the sum of its column's dZ bounds plus (R + 8) u sum |dZ| for the additions (256 rows per tile in
  8 fixed levels, then the tiles).  Worst observed error / bound on one MI355X run: dZ 0.33, db 0.12.
"""
import zlib

import numpy as np
import pytest
import torch

import step_reference as sr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # fp32 unit roundoff
E_BADARG, E_WORKSPACE, E_ALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from fitgnn_amd import _lib
    return _lib


def _rng(*parts):
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


def _call(L, fn, *args):
    rc = getattr(L.lib(), fn)(*args, L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _run(L, fn, *args):
    L.check(_call(L, fn, *args), fn)


def _p(L, t):
    return L.dptr(t)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _exact(rng, shape, lo=-8, hi=8, den=64.0):
    """Small integers times 1/den: every product and sum the tests form stays exact in fp32."""
    return (rng.integers(lo, hi + 1, size=shape) / den).astype(np.float32)


def _strided(A, ld, offset=0, fill=float("nan")):
    """A [n, C] as a device view with row stride ld, `offset` floats into a buffer whose padding holds `fill` (NaN: a kernel that
    reads past column C poisons its result)."""
    A = np.asarray(A, dtype=np.float32)
    n, C = A.shape
    buf = torch.full((offset + max(n, 1) * ld + 4,), fill, dtype=torch.float32, device="cuda")
    v = buf[offset:offset + n * ld].view(n, ld)[:, :C]
    v.copy_(torch.from_numpy(A))
    return v


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _within(got, ref, bound, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {bad.sum()} entries out of bound, worst {err[bad].max()} at {np.argwhere(bad)[:3].tolist()}"


def _same(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bad = got != ref
    assert not bad.any(), f"{what}: {bad.sum()} entries differ, first at {np.argwhere(bad)[:3].tolist()}: {got[bad][:3]} vs {ref[bad][:3]}"


def _dropout(epi_kind, rows_total, H, rng, seed=0x1234_5678_9ABC_DEF1 & 0x7FFF_FFFF_FFFF_FFFF):
    """(flags, seed argument, mask tensor or None, seed word kept alive, keep(original rows) function) of a dropout form:
    'none', 'mask', 'hash' (seed by value) or 'hash_ptr' (seed read from a device word)."""
    if epi_kind == "none":
        return 0, 0, None, None, lambda rows: None
    if epi_kind == "mask":
        m = rng.integers(0, 2, size=(rows_total, H), dtype=np.uint8).astype(bool)
        mt = _dev(m.astype(np.uint8), torch.uint8)
        return sr.EPI_DROPOUT, 0, mt, None, lambda rows: m[np.asarray(rows, dtype=np.int64)]
    if epi_kind == "hash":
        return sr.EPI_DROPOUT, seed, None, None, lambda rows: sr.keep_matrix(seed, rows, H, 0.5)
    word = torch.tensor([seed], dtype=torch.int64, device="cuda")
    return (sr.EPI_DROPOUT | sr.EPI_SEED_DEVICE, word.data_ptr(), None, word,
            lambda rows: sr.keep_matrix(seed, rows, H, 0.5))


# ---------------------------------------------------------------------------------------------------------------------------------
# softmax + NLL
# ---------------------------------------------------------------------------------------------------------------------------------
def _softmax_nll(L, z, ldz, idx, labels, scale, n_rows=None):
    n_rows = z.shape[0] if n_rows is None else n_rows
    C = z.shape[1]
    zd = _strided(z, ldz)
    dz = torch.full((n_rows * ldz + 4,), float("nan"), device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    it, lt = _dev(idx, torch.int64), _dev(labels, torch.int64)
    wb = int(L.lib().fitgnn_softmax_nll_workspace_bytes(len(idx)))
    work = torch.empty(max(wb, 4), dtype=torch.uint8, device="cuda")
    _run(L, "fitgnn_softmax_nll_f32", _p(L, zd), ldz, n_rows, C, _p(L, it), _p(L, lt), len(idx), scale, _p(L, loss), _p(L, dz),
         _p(L, work), wb)
    return float(loss.item()), dz[:n_rows * ldz].view(n_rows, ldz)


def _check_softmax(z, idx, labels, scale, loss, dzfull, ldz):
    C = z.shape[1]
    z64 = z.astype(np.float64)
    ref_loss, ref_dz, lse = sr.softmax_nll(z64, idx, labels, scale)
    got = _np(dzfull)
    assert np.all(got[:, C:] == 0), "padding columns of dz are not zero"
    got = got[:, :C]
    sel = np.zeros(z.shape[0], dtype=bool); sel[idx] = True
    assert np.all(got[~sel] == 0), "an unselected row of dz is not exactly zero"
    zs = z64[idx]
    m = zs.max(1)
    sm = np.exp(zs - lse[:, None])
    oh = np.zeros_like(sm); oh[np.arange(len(idx)), labels] = 1.0
    bound = scale * (sm * 4 * U * (np.abs(zs) + 2 * np.abs(lse)[:, None] + np.abs(m)[:, None] + C + 8) + 2 * U * np.abs(sm - oh))
    bound = bound + scale * np.where(sm < 2.0 ** -125, sm, 0.0)   # fp32 underflow of exp(z - lse)
    _within(got[idx], ref_dz[idx], bound, "dz")
    terms = (lse - zs[np.arange(len(idx)), labels]) * scale
    lb = (4 * U * scale * (np.abs(lse) + np.abs(m) + np.abs(zs[np.arange(len(idx)), labels]) + C + 8).sum()
          + (np.ceil(np.log2(len(idx) + 1)) + len(idx) / 256 + 9) * U * np.abs(terms).sum())
    assert abs(loss - ref_loss) <= lb, (loss, ref_loss, lb)


@pytest.mark.parametrize("n,C,ldz", [(1, 1, 1), (1, 5, 7), (255, 2, 2), (256, 47, 47), (257, 64, 67), (300, 65, 65),
                                     (100, 1000, 1003), (70001, 3, 5)],
                         ids=lambda v: str(v))
def test_softmax_nll(L, n, C, ldz):
    rng = _rng("softmax", n, C)
    n_rows = n + 37
    z = rng.normal(0, 3, size=(n_rows, C)).astype(np.float32)
    idx = rng.permutation(n_rows)[:n]             # unsorted, distinct; 37 rows stay unselected
    labels = rng.integers(0, C, size=n)
    loss, dz = _softmax_nll(L, z, ldz, idx, labels, 0.125)
    _check_softmax(z, idx, labels, 0.125, loss, dz, ldz)


def test_softmax_nll_empty(L):
    z = np.ones((10, 5), dtype=np.float32)
    loss, dz = _softmax_nll(L, z, 6, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 1.0)
    assert loss == 0.0
    assert torch.all(dz == 0).item()


def test_softmax_nll_extreme_rows(L):
    rng = _rng("softmax_extreme")
    C, n_rows = 47, 300
    z = rng.normal(0, 3, size=(n_rows, C)).astype(np.float32)
    z[3] = np.where(np.arange(C) % 2 == 0, 80.0, -80.0)
    z[4] = -80.0
    z[5] = 0.0; z[5, 7] = 120.0                    # dominant: every other exp(z - lse) is below fp32's range
    idx = np.concatenate([[3, 4, 5], 6 + rng.permutation(n_rows - 6)[:197]])
    labels = rng.integers(0, C, size=200); labels[2] = 7
    loss, dz = _softmax_nll(L, z, C, idx, labels, 0.25)
    _check_softmax(z, idx, labels, 0.25, loss, dz, C)
    assert torch.all(dz[5] == 0).item(), "the dominant row's gradient must underflow to exactly zero (its label is the dominant class)"


# ---------------------------------------------------------------------------------------------------------------------------------
# L1 loss
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100000])
def test_l1_loss(L, n):
    rng = _rng("l1", n)
    out = _exact(rng, n); tgt = _exact(rng, n)
    tgt[::7] = out[::7]                            # ties: gradient exactly 0
    ot, tt = _dev(out), _dev(tgt)
    grad = torch.full((max(n, 1),), float("nan"), device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    _run(L, "fitgnn_l1_loss_f32", _p(L, ot) if n else None, _p(L, tt) if n else None, n, 0.25, _p(L, loss), _p(L, grad) if n else None)
    ref_loss, ref_grad = sr.l1_loss(out, tgt, 0.25)
    assert float(loss.item()) == ref_loss
    if n:
        _same(_np(grad[:n]), ref_grad, "grad")


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------------
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 0.01
B1F, B2F, LRF = float(np.float32(B1)), float(np.float32(B2)), float(np.float32(LR))


class _Adam:
    """One flat parameter buffer with its state; `step()` launches the kernel under test."""

    def __init__(self, L, n, kind, wd, t0, seed, with_new=True, n_seeds=3):
        self.L, self.n, self.kind, self.wd = L, n, kind, wd
        g = torch.Generator(device="cuda"); g.manual_seed(seed)
        self.p = torch.randn(n, device="cuda", generator=g)
        self.g = torch.randn(n, device="cuda", generator=g) * 0.1
        self.gn = torch.randn(n, device="cuda", generator=g) * 0.1 if (with_new and kind == "acc") else None
        if t0 == 0:
            self.m, self.v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        else:   # a state loaded from a checkpoint at step t0
            self.m = torch.randn(n, device="cuda", generator=g) * 0.05
            self.v = torch.rand(n, device="cuda", generator=g) * 0.01
        self.state = torch.tensor([float(t0), 0.0], device="cuda")
        self.seeds = torch.tensor([1, 2 ** 62 + 5, -3], dtype=torch.int64, device="cuda")[:n_seeds]
        self.stride = 0x9E3779B97F4A7C15

    def launch(self):
        L = self.L
        if self.kind == "plain":
            return L.lib().fitgnn_adam_step_f32(_p(L, self.p), _p(L, self.g), _p(L, self.m), _p(L, self.v), self.n, LR, B1, B2, EPS,
                                                self.wd, _p(L, self.state), L.stream_ptr())
        return L.lib().fitgnn_adam_step_acc_f32(_p(L, self.p), _p(L, self.g), _p(L, self.gn), _p(L, self.m), _p(L, self.v), self.n, LR,
                                                B1, B2, EPS, self.wd, _p(L, self.state), _p(L, self.seeds), self.seeds.numel(),
                                                self.stride, L.stream_ptr())

    def step(self):
        rc = self.launch()
        torch.cuda.synchronize()
        self.L.check(rc, "adam")

    def snapshot(self):
        return {k: (None if getattr(self, k) is None else getattr(self, k).clone()) for k in ("p", "g", "gn", "m", "v", "state", "seeds")}


def _adam_ref_and_bounds(before, t, wd):
    f = lambda k: None if before[k] is None else _np(before[k])   # noqa: E731
    p, g, gn, m, v = f("p"), f("g"), f("gn"), f("m"), f("v")
    if gn is not None:   # the kernel adds the two gradients in fp32 (and stores that sum): the update starts from it
        g, gn = (before["g"].cpu().numpy() + before["gn"].cpu().numpy()).astype(np.float64), None
    p1, g1, m1, v1 = sr.adam(p, g, gn, m, v, t, LRF, B1F, B2F, float(np.float32(EPS)), float(np.float32(wd)))
    gk = np.abs(g1) + wd * np.abs(p)
    step = t + 1.0
    step_size = LRF / (1 - B1F ** step)
    denom = np.sqrt(v1) / np.sqrt(1 - B2F ** step) + EPS
    em = 4 * U * (B1F * np.abs(m) + (1 - B1F) * gk)
    bp = U * np.abs(p1) + 12 * U * np.abs(p1 - p) + step_size / denom * em + 2 ** -149
    bm = em + 2 ** -149
    bv = 5 * U * np.abs(v1) + 2 ** -149
    return (p1, g1, m1, v1), (bp, bm, bv)


def _check_adam_step(a, before, t):
    (p1, g1, m1, v1), (bp, bm, bv) = _adam_ref_and_bounds(before, t, a.wd)
    _within(_np(a.p), p1, bp, "param")
    _within(_np(a.m), m1, bm, "exp_avg")
    _within(_np(a.v), v1, bv, "exp_avg_sq")
    if a.gn is not None:
        _same(_np(a.g), (before["g"].cpu().numpy() + before["gn"].cpu().numpy()).astype(np.float32), "grad_acc + grad_new")
        assert torch.all(a.gn == 0).item(), "grad_new not cleared"
    else:
        assert torch.equal(a.g, before["g"]), "the gradient buffer changed"
    assert float(a.state[0]) == t + 1.0, "step count not advanced exactly once"
    assert int(a.state.view(torch.int32)[1]) == 0, "ticket word not left at zero"
    if a.kind == "acc":
        want = [(int(s) + a.stride) & 0xFFFFFFFFFFFFFFFF for s in before["seeds"].cpu().numpy().view(np.uint64)]
        assert a.seeds.cpu().numpy().view(np.uint64).tolist() == want, "seeds not advanced exactly once by seed_stride"


ADAM_CASES = [(n, t0, wd, new) for n in (4, 5200) for (t0, wd, new) in ((0, 0.0, True), (1000, 5e-4, True), (10000, 5e-4, False))]
ADAM_CASES += [(4_000_000, 0, 5e-4, True), (4_000_000, 10000, 0.0, False)]


@pytest.mark.parametrize("kind", ["plain", "acc"])
@pytest.mark.parametrize("n,t0,wd,with_new", ADAM_CASES, ids=lambda v: str(v))
def test_adam_one_step(L, kind, n, t0, wd, with_new):
    a = _Adam(L, n, kind, wd, t0, seed=n + t0, with_new=with_new)
    for k in range(2):   # twice: the ticket word must be back at zero for the second launch to advance the count
        before = a.snapshot()
        a.step()
        _check_adam_step(a, before, t0 + k)


@pytest.mark.parametrize("kind", ["plain", "acc"])
def test_adam_first_steps(L, kind):
    """The first 30 steps, each against the f64 formula with the fp32 betas from the kernel's own previous state: 1 - b2^t is where
    an fp32 evaluation cancels (3e-6 relative at t = 2)."""
    a = _Adam(L, 5200, kind, 5e-4, 0, seed=7)
    for t in range(30):
        before = a.snapshot()
        a.step()
        _check_adam_step(a, before, t)
        if a.gn is not None:
            a.gn.copy_(before["gn"])


def test_adam_graph_replay_equals_eager(L):
    eager = _Adam(L, 5200, "acc", 5e-4, 0, seed=11)
    src = eager.gn.clone()
    cap = _Adam(L, 5200, "acc", 5e-4, 0, seed=11)
    for a in (eager, cap):
        a.gn.copy_(src)
    for _ in range(50):
        eager.gn.copy_(src)
        eager.step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        cap.gn.copy_(src)
        rc = cap.launch()
    L.check(rc, "capture")
    for _ in range(50):
        graph.replay()
    torch.cuda.synchronize()
    for k in ("p", "g", "m", "v", "state", "seeds", "gn"):
        assert torch.equal(getattr(eager, k), getattr(cap, k)), f"{k}: graph replay differs from eager steps"
    assert float(cap.state[0]) == 50.0


def test_adam_against_torch_optim_adam(L):
    n, T, wd = 4096, 1000, 5e-4
    a = _Adam(L, n, "acc", wd, 0, seed=13, with_new=False)
    a.g.zero_()
    pt = a.p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    pmax = 0.0
    for t in range(T):
        g = torch.randn(n, device="cuda", generator=gen) * torch.linspace(1e-3, 1.0, n, device="cuda")
        a.g.copy_(g)
        pt.grad = g.clone()
        opt.step()
        rc = a.launch()
        L.check(rc, "adam")
        if t % 100 == 0:
            pmax = max(pmax, float(a.p.abs().max()))
    torch.cuda.synchronize()
    pmax = max(pmax, float(a.p.abs().max())) + 100 * 3.2 * LR   # max |p_t| between two samples
    bound = T * LR * (3.2 * 1e-5 + 6 * 32 * U) + 2 * U * T * pmax
    diff = float((a.p - pt.detach()).abs().max())
    assert diff <= bound, (diff, bound)
    assert float(a.state[0]) == T


# ---------------------------------------------------------------------------------------------------------------------------------
# head on the loss rows
# ---------------------------------------------------------------------------------------------------------------------------------
def _head_rows(L, out_np, ldo, rows, Wl, bl, R, compact):
    H = out_np.shape[1]
    C = Wl.shape[0]
    od = _strided(out_np, ldo)
    Wd = _dev(Wl); bd = None if bl is None else _dev(bl)
    y = torch.full((R, C + 3), float("nan"), device="cuda")   # ldy > C
    rt = _dev(rows, torch.int64)
    rc = _call(L, "fitgnn_head_rows_f32", _p(L, od), ldo, _p(L, rt), len(rows), _p(L, Wd), _p(L, bd), C, H, _p(L, y), C + 3,
               1 if compact else 0)
    return rc, y


def _check_head(L, H, C, n, ldo, compact, with_bias, rng):
    R = 2 * n + 3
    rows = rng.permutation(R)[:n]
    out_full = _exact(rng, (R, H))
    Wl = _exact(rng, (C, H)); bl = _exact(rng, C) if with_bias else None
    src = out_full[rows] if compact else out_full
    rc, y = _head_rows(L, src, ldo, rows, Wl, bl, R, compact)
    L.check(rc, "fitgnn_head_rows_f32")
    ref, _ = sr.head_rows(out_full[rows], Wl, bl)
    got = _np(y)
    _same(got[rows, :C], ref, f"y (H={H}, C={C}, n={n})")
    other = np.setdiff1d(np.arange(R), rows)
    assert np.all(np.isnan(got[other])) and np.all(np.isnan(got[:, C:])), "a row or column outside the selection was written"


def _head_fits(L, H, C):
    return int(L.lib().fitgnn_head_rows_lds_bytes(H, C)) <= 160 * 1024


HEAD_GRID = [(C, H) for C in (1, 3, 16, 17, 47, 64) for H in (4, 12, 36, 512, 1024)]


@pytest.mark.parametrize("C,H", HEAD_GRID, ids=lambda v: str(v))
def test_head_rows_grid(L, C, H):
    if not _head_fits(L, H, C):
        rc, _ = _head_rows(L, np.zeros((5, H), np.float32), H, np.arange(5), np.zeros((C, H), np.float32), None, 5, False)
        assert rc == E_BADARG
        return
    _check_head(L, H, C, 5, H, False, True, _rng("head", C, H))


@pytest.mark.parametrize("C,H", [(65, 36), (130, 36), (65, 128), (130, 128)])
def test_head_rows_second_class_pass(L, C, H):
    assert _head_fits(L, H, C)
    _check_head(L, H, C, 37, H + 8, False, True, _rng("head2", C, H))


@pytest.mark.parametrize("n,C,H,compact,bias", [(1, 3, 36, False, True), (5, 47, 512, True, False), (4097, 3, 36, True, True),
                                                 (20000, 47, 128, False, True), (20000, 1, 256, True, False)],
                         ids=lambda v: str(v))
def test_head_rows_rows(L, n, C, H, compact, bias):
    _check_head(L, H, C, n, H + 4, compact, bias, _rng("head_rows", n, C, H))


def test_head_rows_lds_refusal(L):
    from fitgnn_amd import ops
    assert int(L.lib().fitgnn_head_rows_lds_bytes(512, 65)) == 166928
    rc, _ = _head_rows(L, np.zeros((5, 512), np.float32), 512, np.arange(5), np.zeros((65, 512), np.float32), None, 5, False)
    assert rc == E_BADARG
    assert not ops.head_rows_supported(torch.zeros(4, 512, device="cuda"), torch.zeros(65, 512, device="cuda"))
    assert ops.head_rows_supported(torch.zeros(4, 512, device="cuda"), torch.zeros(47, 512, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------------------
# narrow column sum
# ---------------------------------------------------------------------------------------------------------------------------------
def _colsum(L, x, ldx):
    n, C = x.shape
    xd = _strided(x, ldx)
    out = torch.full((C + 1,), float("nan"), device="cuda")
    wb = int(L.lib().fitgnn_colsum_narrow_workspace_bytes(n, C))
    work = torch.empty(max(wb, 4), dtype=torch.uint8, device="cuda")
    rc = _call(L, "fitgnn_colsum_narrow_f32", _p(L, xd), ldx, n, C, _p(L, out), _p(L, work), wb)
    return rc, out


def test_colsum_narrow_every_width(L):
    rng = _rng("colsum")
    for C in range(1, 65):
        x = _exact(rng, (300, C))
        rc, out = _colsum(L, x, C + 3)
        L.check(rc, "colsum")
        _same(_np(out[:C]), sr.colsum(x)[0], f"C={C}")
        assert np.isnan(out[C].item()), "wrote past column C"
    rc, _ = _colsum(L, _exact(rng, (300, 65)), 65)
    assert rc == E_BADARG


@pytest.mark.parametrize("n,C", [(1, 5), (70000, 47), (65537, 64)])
def test_colsum_narrow_rows(L, n, C):
    x = _exact(_rng("colsum_rows", n, C), (n, C))
    rc, out = _colsum(L, x, C + 3)
    L.check(rc, "colsum")
    _same(_np(out[:C]), sr.colsum(x)[0], f"n={n}")


# ---------------------------------------------------------------------------------------------------------------------------------
# epilogue backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _out_exact(rng, shape, den=32):
    """A forward output whose ELU factor (out * 0.5 + 1 below zero) stays a multiple of 1 / (2 den) above zero."""
    return _exact(rng, shape, lo=-(den - 2), hi=den - 2, den=float(den))


def _epi_case(rng, n_total, H, elu, drop_kind):
    epi, seed, mask, word, keep = _dropout(drop_kind, n_total, H, rng)
    epi |= sr.EPI_ELU if elu else 0
    return epi, seed, mask, word, keep


def _offset_copy(a_np, offset):
    """A device copy of a [n, H] array `offset` floats into its buffer (offset 1: not 16-byte aligned)."""
    a_np = np.ascontiguousarray(a_np, dtype=np.float32)
    buf = torch.empty(a_np.size + 4, device="cuda")
    v = buf[offset:offset + a_np.size].view(a_np.shape)
    v.copy_(torch.from_numpy(a_np))
    return v


@pytest.mark.parametrize("H,offset", [(64, 0), (37, 0), (64, 1), (260, 0)])
@pytest.mark.parametrize("n", [4096, 4097])
@pytest.mark.parametrize("elu,drop", [(False, "none"), (True, "mask"), (True, "hash"), (False, "hash_ptr")])
def test_epilogue_bwd_plain(L, H, offset, n, elu, drop):
    rng = _rng("ebwd", H, offset, n, elu, drop)
    dOut = _exact(rng, (n, H), lo=1, hi=8)          # no zero: dZ is zero exactly where the element was dropped
    dOut *= np.where(rng.random((n, H)) < 0.5, -1, 1).astype(np.float32)
    out = _out_exact(rng, (n, H))
    epi, seed, mask, word, keep = _epi_case(rng, n, H, elu, drop)
    dOd, od = _offset_copy(dOut, offset), _offset_copy(out, offset)
    dZ = _offset_copy(np.full((n, H), np.nan, np.float32), offset)
    db = torch.full((H,), float("nan"), device="cuda")
    wb = int(L.lib().fitgnn_epilogue_bwd_workspace_bytes(n, H))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    _run(L, "fitgnn_epilogue_bwd_f32", _p(L, dOd), _p(L, od), _p(L, dZ), n, H, epi, 0.5, seed, _p(L, mask), _p(L, db), _p(L, work), wb)
    rdZ, rdb, _ = sr.epilogue_bwd(dOut, out, epi, 0.5, keep(np.arange(n)))
    _same(_np(dZ), rdZ, "dZ")
    _same(_np(db), rdb, "db")
    del word


def _head_launchable(C, H, offset):
    vec = H % 4 == 0 and offset == 0
    return C <= ((H - 1) % (256 if vec else 64) + 1) // (4 if vec else 1)


# (C, with dWl) x (H, offset of `out` / dZ in floats): <4 | 1, true, 0 | 4 | 16>; refusals are test_epilogue_bwd_head_refusals
HEAD_CASES = [(C, w, H, o) for (C, w) in ((1, True), (4, True), (5, True), (16, True), (1, False), (17, False), (48, False))
              for (H, o) in ((256, 0), (261, 0), (192, 1)) if _head_launchable(C, H, o)]


@pytest.mark.parametrize("C,with_dWl,H,offset", HEAD_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("drop", ["hash", "mask"])
def test_epilogue_bwd_head(L, C, with_dWl, H, offset, drop):
    rng = _rng("ebwd_head", C, with_dWl, H, offset, drop)
    n = 600
    dy = _exact(rng, (n, C), lo=-4, hi=4)
    dy[rng.random(n) < 0.2] = 0.0                  # rows outside the loss: dZ must be +0 there
    Wl = _exact(rng, (C, H), lo=-4, hi=4)
    out = _out_exact(rng, (n, H), den=8)
    epi, seed, mask, word, keep = _epi_case(rng, n, H, True, drop)
    dyd, Wd = _dev(dy), _dev(Wl)
    od = _offset_copy(out, offset)
    dZ = _offset_copy(np.full((n, H), np.nan, np.float32), offset)
    db = torch.full((H,), float("nan"), device="cuda")
    dWl = torch.full((C, H), float("nan"), device="cuda") if with_dWl else None
    wb = int(L.lib().fitgnn_epilogue_bwd_head_workspace_bytes(n, H, C))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    _run(L, "fitgnn_epilogue_bwd_head_f32", _p(L, dyd), _p(L, Wd), C, _p(L, od), _p(L, dZ), n, H, epi, 0.5, seed, _p(L, mask), _p(L, db),
         _p(L, dWl), _p(L, work), wb)
    rdZ, rdb, rdWl, _, _ = sr.epilogue_bwd_head(dy, Wl, out, epi, 0.5, keep(np.arange(n)))
    _same(_np(dZ), rdZ, "dZ")
    _same(_np(db), rdb, "db")
    if with_dWl:
        _same(_np(dWl), rdWl, "dWl")
    del word


def test_epilogue_bwd_head_refusals(L):
    lib = L.lib()
    assert lib.fitgnn_epilogue_bwd_head_supported(256, 16, 1) == 1 and lib.fitgnn_epilogue_bwd_head_supported(256, 17, 1) == 0
    assert lib.fitgnn_epilogue_bwd_head_supported(256, 48, 0) == 1 and lib.fitgnn_epilogue_bwd_head_supported(256, 49, 0) == 0
    assert lib.fitgnn_epilogue_bwd_head_supported(260, 1, 0) == 1 and lib.fitgnn_epilogue_bwd_head_supported(260, 2, 0) == 0
    assert lib.fitgnn_epilogue_bwd_head_supported(68, 17, 0) == 1

    def launch(H, C, with_dWl, offset=0):
        n = 8
        dy, Wl = torch.zeros(n, C, device="cuda"), torch.zeros(C, H, device="cuda")
        out = _offset_copy(np.zeros((n, H), np.float32), offset)
        dZ = _offset_copy(np.zeros((n, H), np.float32), offset)
        dWl = torch.zeros(C, H, device="cuda") if with_dWl else None
        db = torch.zeros(H, device="cuda")
        wb = int(lib.fitgnn_epilogue_bwd_head_workspace_bytes(n, H, C))
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        return _call(L, "fitgnn_epilogue_bwd_head_f32", _p(L, dy), _p(L, Wl), C, _p(L, out), _p(L, dZ), n, H, 0, 0.0, 0, None, _p(L, db),
                     _p(L, dWl), _p(L, work), wb)

    assert launch(256, 17, True) == E_BADARG
    assert launch(256, 49, False) == E_BADARG
    assert launch(260, 2, False) == E_BADARG
    assert launch(260, 1, False) == 0
    # H % 4 == 0 but `out` not 16-byte aligned: the one-column form's last slab of H = 68 has 4 columns, so 17 classes are refused
    assert launch(68, 17, False, offset=1) == E_ALIGN
    assert launch(68, 4, True, offset=1) == 0


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("compact_in", [0, 1])
@pytest.mark.parametrize("drop", ["hash", "hash_ptr", "mask"])
def test_epilogue_bwd_selected_rows(L, head, compact_in, drop):
    rng = _rng("ebwd_sel", head, compact_in, drop)
    R, H, C, n_sel = 3000, 128, 5, 911
    sel = rng.permutation(R)[:n_sel]
    out = _out_exact(rng, (R, H), den=8 if head else 32)
    dy = _exact(rng, (R, C)); Wl = _exact(rng, (C, H))
    dOut = _exact(rng, (R, H), lo=1, hi=8)
    epi, seed, mask, word, keep = _epi_case(rng, R, H, True, drop)
    take = (lambda a: a[sel]) if compact_in else (lambda a: a)
    od = _dev(take(out))
    dZ = torch.full((n_sel, H), float("nan"), device="cuda")
    db = torch.full((H,), float("nan"), device="cuda")
    st = _dev(sel, torch.int64)
    wb = int(L.lib().fitgnn_epilogue_bwd_head_workspace_bytes(n_sel, H, C))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    if head:
        dWl = torch.full((C, H), float("nan"), device="cuda")
        dyd, Wd = _dev(take(dy)), _dev(Wl)
        _run(L, "fitgnn_epilogue_bwd_head_rows_f32", _p(L, dyd), _p(L, Wd), C, _p(L, od), _p(L, st), n_sel, compact_in, _p(L, dZ), H, epi,
             0.5, seed, _p(L, mask), _p(L, db), _p(L, dWl), _p(L, work), wb)
        rdZ, rdb, rdWl, _, _ = sr.epilogue_bwd_head(dy[sel], Wl, out[sel], epi, 0.5, keep(sel))
        _same(_np(dWl), rdWl, "dWl")
    else:
        dOd = _dev(take(dOut))
        _run(L, "fitgnn_epilogue_bwd_rows_f32", _p(L, dOd), _p(L, od), _p(L, st), n_sel, compact_in, _p(L, dZ), H, epi, 0.5, seed,
             _p(L, mask), _p(L, db), _p(L, work), wb)
        rdZ, rdb, _ = sr.epilogue_bwd(dOut[sel], out[sel], epi, 0.5, keep(sel))
    _same(_np(dZ), rdZ, "dZ")
    _same(_np(db), rdb, "db")
    del word


# ---------------------------------------------------------------------------------------------------------------------------------
# forward epilogue on rows, dense_narrow_k
# ---------------------------------------------------------------------------------------------------------------------------------
def _elu_bound(y, ey, scale):
    """The __expf bound of the module docstring for y <= 0, with ey the bound on y itself; 0 above zero (handled by the caller)."""
    y = np.minimum(y, 0.0)
    return 2 * scale * (U * (np.exp(y) * (4 + 2 * np.abs(y)) + np.abs(np.expm1(y))) + np.exp(y) * ey)


def _check_fwd(got, z_ref, ez, bias, epi, p, keep, what):
    """got = dropout(ELU(z + bias)) where the float64 z_ref is known to within ez (per entry)."""
    b = np.zeros(z_ref.shape[1]) if not (epi & sr.EPI_BIAS) else np.asarray(bias, dtype=np.float64)
    y = z_ref + b[None, :]
    ey = ez + U * (np.abs(z_ref) + np.abs(b)[None, :])
    ref = sr.epilogue_fwd(z_ref, bias, epi, p, keep)
    scale = 1.0 / (1.0 - float(np.float32(p))) if epi & sr.EPI_DROPOUT else 1.0
    lin = scale * (ey + U * np.abs(y)) * (1 + 2 * U)
    bound = np.where(y <= 0, _elu_bound(y, ey, scale), lin) if epi & sr.EPI_ELU else lin
    bound = bound + 4 * U * np.abs(ref)
    if epi & sr.EPI_DROPOUT:
        assert np.all(got[~keep] == 0), f"{what}: a dropped element is not zero"
    _within(got, ref, bound, what)


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("drop", ["none", "mask", "hash", "hash_ptr"])
def test_epilogue_fwd_rows(L, with_rows, drop):
    rng = _rng("efwd", with_rows, drop)
    n, H, R, ldz = 700, 36, 2000, 44
    rows = rng.permutation(R)[:n] if with_rows else np.arange(n)
    z = rng.normal(0, 2, size=(n, H)).astype(np.float32)
    bias = rng.normal(0, 1, size=H).astype(np.float32)
    epi, seed, mask, word, keep = _dropout(drop, R, H, rng)
    epi |= sr.EPI_BIAS | sr.EPI_ELU
    zd = _strided(z, ldz)
    bd = _dev(bias)
    rt = _dev(rows, torch.int64) if with_rows else None
    _run(L, "fitgnn_epilogue_fwd_rows_f32", _p(L, zd), ldz, _p(L, rt), n, H, _p(L, bd), epi, 0.5, seed, _p(L, mask))
    k = keep(rows)
    _check_fwd(_np(zd), z.astype(np.float64), 0.0, bias, epi, 0.5, k if k is not None else np.ones((n, H), bool), "z")
    assert torch.isnan(zd.as_strided((n, ldz), (ldz, 1))[:, H:]).all().item(), "wrote into the row padding"
    del word


def _dense_narrow_k(L, a, lda, W, ldw, bias, epi, p, seed, mask, H, ldo):
    n, K = a.shape
    ad, Wd = _strided(a, lda), _strided(W, ldw)
    bd = None if bias is None else _dev(bias)
    out = torch.full((max(n, 1), ldo), float("nan"), device="cuda")
    rc = _call(L, "fitgnn_dense_narrow_k_f32", _p(L, ad), lda, _p(L, Wd), ldw, n, K, H, _p(L, bd), epi, p, seed, _p(L, mask), _p(L, out), ldo)
    return rc, out


NK_SHAPES = [(1, 4, 1), (8, 16, 7), (11, 36, 4097), (31, 512, 4096), (32, 16, 60000), (32, 36, 7), (8, 4, 4097), (11, 128, 60000),
             (1, 512, 7)]


@pytest.mark.parametrize("K,H,n", NK_SHAPES, ids=lambda v: str(v))
def test_dense_narrow_k_shapes(L, K, H, n):
    rng = _rng("nk", K, H, n)
    a = _exact(rng, (n, K)); W = _exact(rng, (H, K)); b = _exact(rng, H)
    epi, seed, mask, word, keep = _dropout("hash", n, H, rng)
    epi |= sr.EPI_BIAS
    rc, out = _dense_narrow_k(L, a, K + 3, W, K + 1, b, epi, 0.5, seed, mask, H, H + 4)
    L.check(rc, "fitgnn_dense_narrow_k_f32")
    ref, _, _ = sr.dense_narrow_k(a, W, b, epi, 0.5, keep(np.arange(n)))
    got = _np(out)
    _same(got[:, :H], ref, "out")
    assert np.all(np.isnan(got[:, H:])), "wrote past column H"


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("elu", [False, True])
@pytest.mark.parametrize("drop", ["none", "mask", "hash", "hash_ptr"])
@pytest.mark.parametrize("H", [36, 512])
def test_dense_narrow_k_epilogues(L, bias, elu, drop, H):
    rng = _rng("nk_epi", bias, elu, drop, H)
    n, K = 1001, 11
    a = rng.normal(size=(n, K)).astype(np.float32); W = rng.normal(size=(H, K)).astype(np.float32)
    b = rng.normal(size=H).astype(np.float32)
    epi, seed, mask, word, keep = _dropout(drop, n, H, rng)
    epi |= (sr.EPI_BIAS if bias else 0) | (sr.EPI_ELU if elu else 0)
    rc, out = _dense_narrow_k(L, a, K, W, K, b if bias else None, epi, 0.5, seed, mask, H, H)
    L.check(rc, "fitgnn_dense_narrow_k_f32")
    _, z, cond = sr.dense_narrow_k(a, W, None, 0)
    k = keep(np.arange(n))
    _check_fwd(_np(out), z, (K + 2) * U * cond, b, epi, 0.5, k if k is not None else np.ones((n, H), bool), "out")
    del word


def test_dense_narrow_k_lds_refusal(L):
    lib = L.lib()
    assert int(lib.fitgnn_dense_narrow_k_lds_bytes(31, 512)) == (31 * 512 + 16 * 31) * 4
    assert int(lib.fitgnn_dense_narrow_k_lds_bytes(32, 512)) == 0
    rc, _ = _dense_narrow_k(L, np.zeros((4, 32), np.float32), 32, np.zeros((512, 32), np.float32), 32, None, 0, 0.0, 0, None, 512, 512)
    assert rc == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# narrow_atb
# ---------------------------------------------------------------------------------------------------------------------------------
def _narrow_atb(L, d, ldd, prev, epi, p, seed, mask, a, lda):
    n, H = d.shape
    K = a.shape[1]
    dd, ad = _strided(d, ldd), _strided(a, lda)
    pd = None if prev is None else _dev(prev)
    dW = torch.full((H, K), float("nan"), device="cuda")
    db = torch.full((H,), float("nan"), device="cuda")
    wb = int(L.lib().fitgnn_narrow_atb_workspace_bytes(n, K, H))
    work = torch.empty(max(wb, 4), dtype=torch.uint8, device="cuda")
    rc = _call(L, "fitgnn_narrow_atb_f32", _p(L, dd), ldd, _p(L, pd), epi, p, seed, _p(L, mask), _p(L, ad), lda, n, K, H, _p(L, dW),
               _p(L, db), _p(L, work), wb)
    return rc, dW, db


ATB_SHAPES = [(1, 16, 1), (8, 64, 15), (9, 512, 16), (16, 1024, 17), (17, 16, 50000), (32, 64, 50000), (32, 1024, 15), (11, 512, 4097)]


@pytest.mark.parametrize("K,H,n", ATB_SHAPES, ids=lambda v: str(v))
def test_narrow_atb_shapes(L, K, H, n):
    rng = _rng("atb", K, H, n)
    d = _exact(rng, (n, H), lo=-4, hi=4); a = _exact(rng, (n, K), lo=-4, hi=4)
    rc, dW, db = _narrow_atb(L, d, H + 4, None, 0, 0.0, 0, None, a, K + 2)
    L.check(rc, "fitgnn_narrow_atb_f32")
    rdW, rdb, _, _ = sr.narrow_atb(d, a)
    _same(_np(dW), rdW, "dW")
    _same(_np(db), rdb, "db")


ATB_EPI = [(elu, drop, n, K, H) for (elu, drop, n) in ((True, "none", 4097), (True, "hash", 17), (True, "mask", 4097), (True, "hash_ptr", 1000))
           for (K, H) in ((11, 512), (17, 64), (8, 1024))]
ATB_EPI += [(False, "hash", 50000, 17, 64), (False, "mask", 50000, 8, 16), (False, "hash_ptr", 16, 32, 1024)]


@pytest.mark.parametrize("elu,drop,n,K,H", ATB_EPI, ids=lambda v: str(v))
def test_narrow_atb_epilogues(L, elu, drop, n, K, H):
    rng = _rng("atb_epi", elu, drop, n, K, H)
    d = _exact(rng, (n, H), lo=-4, hi=4); a = _exact(rng, (n, K), lo=-4, hi=4)
    prev = _exact(rng, (n, H), lo=-30, hi=30, den=32.0) if elu else _exact(rng, (n, H))
    epi, seed, mask, word, keep = _dropout(drop, n, H, rng)
    epi |= sr.EPI_ELU if elu else 0
    rc, dW, db = _narrow_atb(L, d, H, prev, epi, 0.5, seed, mask, a, K)
    L.check(rc, "fitgnn_narrow_atb_f32")
    rdW, rdb, _, _ = sr.narrow_atb(d, a, prev=prev, epi=epi, p=0.5, keep=keep(np.arange(n)))
    _same(_np(dW), rdW, "dW")
    _same(_np(db), rdb, "db")
    del word


def test_narrow_atb_refusal(L):
    lib = L.lib()
    assert int(lib.fitgnn_narrow_atb_workspace_bytes(10, 8, 96)) == 0
    assert int(lib.fitgnn_narrow_atb_workspace_bytes(10, 33, 64)) == 0
    rc, _, _ = _narrow_atb(L, np.zeros((10, 96), np.float32), 96, None, 0, 0.0, 0, None, np.zeros((10, 8), np.float32), 8)
    assert rc == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# fixed-order sums: the same bits on every launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["softmax_nll", "l1_loss", "colsum", "epilogue_bwd_head", "narrow_atb", "head_rows"])
def test_repeat_launches_give_the_same_bits(L, kernel):
    rng = _rng("repeat", kernel)

    def once():
        r = np.random.default_rng(3)
        if kernel == "softmax_nll":
            z = r.normal(size=(70001, 47)).astype(np.float32)
            loss, dz = _softmax_nll(L, z, 47, r.permutation(70001), r.integers(0, 47, 70001), 1.0 / 70001)
            return [np.array([loss]), _np(dz)]
        if kernel == "l1_loss":
            o = _dev(r.normal(size=100000)); t = _dev(r.normal(size=100000))
            from fitgnn_amd import ops
            loss, g = ops.l1_loss_raw(o, t, 1e-5)
            return [_np(loss), _np(g)]
        if kernel == "colsum":
            return [_np(_colsum(L, r.normal(size=(70000, 47)).astype(np.float32), 47)[1][:47])]
        if kernel == "narrow_atb":
            rc, dW, db = _narrow_atb(L, r.normal(size=(50000, 512)).astype(np.float32), 512, None, 0, 0.0, 0, None,
                                     r.normal(size=(50000, 11)).astype(np.float32), 11)
            L.check(rc, "atb")
            return [_np(dW), _np(db)]
        if kernel == "head_rows":
            rc, y = _head_rows(L, r.normal(size=(20000, 512)).astype(np.float32), 512, r.permutation(20000), r.normal(size=(47, 512)).astype(np.float32),
                               r.normal(size=47).astype(np.float32), 20000, False)
            L.check(rc, "head")
            return [_np(y)]
        n, H, C = 9000, 512, 16
        dy, Wl, out = (torch.from_numpy(r.normal(size=s).astype(np.float32)).cuda() for s in ((n, C), (C, H), (n, H)))
        dZ = torch.empty(n, H, device="cuda"); db = torch.empty(H, device="cuda"); dWl = torch.empty(C, H, device="cuda")
        wb = int(L.lib().fitgnn_epilogue_bwd_head_workspace_bytes(n, H, C))
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        _run(L, "fitgnn_epilogue_bwd_head_f32", _p(L, dy), _p(L, Wl), C, _p(L, out), _p(L, dZ), n, H, sr.EPI_ELU, 0.0, 0, None, _p(L, db),
             _p(L, dWl), _p(L, work), wb)
        return [_np(dZ), _np(db), _np(dWl)]

    first, second = once(), once()
    for x, y in zip(first, second):
        assert np.array_equal(x, y, equal_nan=True), f"{kernel}: two launches on the same input differ"
    del rng


# ---------------------------------------------------------------------------------------------------------------------------------
# the dX GEMM with the previous layer's epilogue backward (csrc/gemm_nt.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def _presplit(L, b):
    """The pre-split image of b [N x K], read through the strides of a transposed view (b^T [K x N + 4] is what is in memory)."""
    N, K = b.shape
    bT = _strided(np.ascontiguousarray(b.T), N + 4)            # element (n, k) at bT[k * (N + 4) + n]
    nbytes = int(L.lib().fitgnn_gemm_nt_presplit_bytes(N, K))
    assert nbytes == -(-N // 256) * (K // 32) * 32768
    img = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _run(L, "fitgnn_gemm_nt_presplit_f32", _p(L, bT), 1, N + 4, N, K, K, _p(L, img))
    return img


def _gemm_epi_bwd(L, a, b, out, form, epi, p, seed, mask, with_db=True, out_offset=0, short=0, lda=None):
    R, K = a.shape
    N = b.shape[0]
    lda = K + 4 if lda is None else lda
    ad = _strided(a, lda)
    if form == "image":
        bd, ldb = _presplit(L, b), 0
    else:
        bd, ldb = _strided(b, K + 4), K + 4
    od = _offset_copy(out, out_offset)
    dbuf = torch.full((R * N + 4,), float("nan"), device="cuda")
    dZ = dbuf[:R * N].view(R, N)
    db = torch.full((N + 1,), float("nan"), device="cuda") if with_db else None
    wb = int(L.lib().fitgnn_gemm_nt_epilogue_bwd_workspace_bytes(R, N))
    assert wb == -(-R // 256) * N * 4
    work = torch.empty(max(wb, 4), dtype=torch.uint8, device="cuda")
    rc = _call(L, "fitgnn_gemm_nt_epilogue_bwd_f32", _p(L, ad), lda, _p(L, bd), ldb, R, N, K, _p(L, od), _p(L, dZ), epi, p, seed, _p(L, mask),
               _p(L, db), _p(L, work), wb - short)
    assert torch.isnan(dbuf[-4:]).all().item(), "wrote past the end of dZ"
    return rc, dZ, db


GEMM_SHAPES = [(R, N, K) for R in (1, 5, 255, 256, 257, 2049) for N in (4, 128, 260) for K in (32, 96)]
GEMM_EPI = [(False, "none"), (True, "none"), (False, "mask"), (False, "hash"), (True, "hash_ptr"), (True, "mask"), (True, "hash")]


@pytest.mark.parametrize("elu,drop", GEMM_EPI, ids=lambda v: str(v))
@pytest.mark.parametrize("R,N,K", GEMM_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("form", ["plain", "image"])
def test_gemm_nt_epilogue_bwd_exact(L, form, R, N, K, elu, drop):
    """a, b = integers in [-8, 8] over 64 (four significant bits: the bf16 high part is the value, the low part zero), `out` integers
    over 8, p = 0.5: every product, every fp32 partial sum and the epilogue's factor are exact, so dZ and db must equal the float64
    result bit for bit at every row and column -- tile edges, the clamped rows and the ragged column tile's dropout group included."""
    rng = _rng("gemm_epi", R, N, K, elu, drop)
    a, b = _exact(rng, (R, K)), _exact(rng, (N, K))
    out = _out_exact(rng, (R, N), den=8)
    epi, seed, mask, word, keep = _epi_case(rng, R, N, elu, drop)
    ref = (a.astype(np.float64) @ b.astype(np.float64).T) * sr.epilogue_bwd_factor(out, epi, 0.5, keep(np.arange(R)))
    # the premise of exactness: every dZ is a multiple of 2^-15 (2^-12 products, the scale 2, o + 1 a multiple of 2^-4) and a column's
    # absolute sum stays below 2^24 of them
    assert np.all(ref * 2.0 ** 15 == np.round(ref * 2.0 ** 15)) and np.abs(ref).sum(0).max() < 2.0 ** 9
    rc, dZ, db = _gemm_epi_bwd(L, a, b, out, form, epi, 0.5, seed, mask)
    L.check(rc, "fitgnn_gemm_nt_epilogue_bwd_f32")
    _same(_np(dZ), ref, "dZ")
    _same(_np(db[:N]), sr.colsum(ref)[0], "db")
    assert np.isnan(db[N].item()), "wrote past column N of db"
    del word


@pytest.mark.parametrize("form", ["plain", "image"])
def test_gemm_nt_epilogue_bwd_without_db(L, form):
    rng = _rng("gemm_epi_nodb", form)
    R, N, K = 257, 260, 32
    a, b, out = _exact(rng, (R, K)), _exact(rng, (N, K)), _out_exact(rng, (R, N), den=8)
    epi, seed, mask, word, keep = _epi_case(rng, R, N, True, "hash")
    rc, dZ, db = _gemm_epi_bwd(L, a, b, out, form, epi, 0.5, seed, mask, with_db=False)
    L.check(rc, "fitgnn_gemm_nt_epilogue_bwd_f32")
    _same(_np(dZ), (a.astype(np.float64) @ b.astype(np.float64).T) * sr.epilogue_bwd_factor(out, epi, 0.5, keep(np.arange(R))), "dZ")


@pytest.mark.parametrize("elu,drop", [(True, "hash"), (True, "none"), (False, "mask")], ids=lambda v: str(v))
@pytest.mark.parametrize("R,N,K", [(5, 4, 32), (257, 260, 96), (2049, 128, 32)], ids=lambda v: str(v))
@pytest.mark.parametrize("form", ["plain", "image"])
def test_gemm_nt_epilogue_bwd_random(L, form, R, N, K, elu, drop):
    rng = _rng("gemm_epi_random", R, N, K, elu, drop)
    a, b = rng.normal(size=(R, K)).astype(np.float32), rng.normal(size=(N, K)).astype(np.float32)
    out = rng.normal(size=(R, N)).astype(np.float32)
    epi, seed, mask, word, keep = _epi_case(rng, R, N, elu, drop)
    rc, dZ, db = _gemm_epi_bwd(L, a, b, out, form, epi, 0.5, seed, mask)
    L.check(rc, "fitgnn_gemm_nt_epilogue_bwd_f32")
    prod = a.astype(np.float64) @ b.astype(np.float64).T
    factor = sr.epilogue_bwd_factor(out, epi, 0.5, keep(np.arange(R)))
    ref = prod * factor
    bound = 2e-5 * np.abs(prod).max() * np.abs(factor) + 2 * U * np.abs(ref)
    got, gdb = _np(dZ), _np(db[:N])
    bdb = bound.sum(0) + (R + 8) * U * np.abs(ref).sum(0)
    live = bound > 0
    print(f"[ratio] gemm_nt_epilogue_bwd dZ: {(np.abs(got - ref)[live] / bound[live]).max():.3g}, db: {(np.abs(gdb - ref.sum(0)) / bdb).max():.3g}")
    _within(got, ref, bound, "dZ")
    _within(gdb, ref.sum(0), bdb, "db")
    rc, dZ2, db2 = _gemm_epi_bwd(L, a, b, out, form, epi, 0.5, seed, mask)
    assert torch.equal(dZ, dZ2) and torch.equal(db[:N], db2[:N]), "two launches on the same input differ"
    del word


def test_gemm_nt_epilogue_bwd_refusals(L):
    rng = _rng("gemm_epi_refusals")
    R, K = 8, 32

    def launch(N=8, K=K, epi=0, p=0.0, **kw):
        return _gemm_epi_bwd(L, _exact(rng, (R, K)), _exact(rng, (N, K)), _out_exact(rng, (R, N), den=8), "plain", epi, p, 0, None, **kw)[0]

    assert launch() == 0
    assert launch(N=6) == E_BADARG                  # a dropout group of four columns would straddle two rows
    assert launch(epi=sr.EPI_DROPOUT, p=1.0) == E_BADARG
    assert launch(epi=sr.EPI_DROPOUT, p=0.5) == 0
    assert launch(out_offset=1) == E_ALIGN
    assert launch(short=1) == E_WORKSPACE
    assert launch(K=48) == E_BADARG                 # K % 32 != 0
    assert launch(lda=K + 1) == E_BADARG            # rows of a not 16-byte aligned
