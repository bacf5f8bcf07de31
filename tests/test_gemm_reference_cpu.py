"""CPU tier: tests/gemm_reference.py.  The fp32 emulations of the dense GEMM kernels (an fmaf chain in the MFMA's order with the
fixed-order chunk sum; the three-product bf16 split) stay inside the derived per-entry bounds on RANDOM operands; the EXACT operands
are exact (the emulations return the float64 product bit for bit at every K, chunking and form the GPU module uses); the bf16
rounding equals torch's; the Python plan models are self-consistent and the GPU module's case list reaches every (form, tile shape,
split, tail) combination the plan model produces over a sweep of admissible arguments.

Worst error / bound of the emulations on normal operands (printed with -s):
* fmaf chain, one launch, K = 4 ... 512:                 0.61  (K = 4; 0.11 at K = 32, 0.006 at K = 512: the bound grows with K, the
                                                               error of normal operands with sqrt K)
* fmaf chain with 8, 16, 24 chunks:                      0.09
* three-product split, hi rounded (d = 2^-8), gemm_nt:   0.42  (K = 4; 0.15 at K = 32, 0.009 at K = 512)
* three-product split, hi truncated, under d = 2^-7:     0.43
* gemm_atb's chunks, reduce and remainder rows:          0.11  (R = 33; 0.03 at R = 293)
"""
import itertools

import numpy as np
import pytest
import torch

import gemm_reference as G
from test_gpu_step_kernels import _exact, _rng

WORST = {}


def _ratio(family, got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(bound > 0)
    r = float((err / bound).max())
    WORST[family] = max(WORST.get(family, 0.0), r)
    print(f"[ratio] {family}: {r:.3g} (family worst {WORST[family]:.3g})")
    assert np.all(err <= bound), f"{family}: the emulation leaves the derived bound (worst ratio {r})"


def _normal(rng, form, I, J, K):
    sa, sb = G.operand_shapes(form, I, J, K)
    return rng.normal(size=sa).astype(np.float32), rng.normal(size=sb).astype(np.float32)


def _chunk_k(K, nchunks):
    return -(-(-(-K // nchunks)) // G.KBK) * G.KBK if nchunks > 1 else K


@pytest.mark.parametrize("nchunks", [1, 8, 16, 24])
@pytest.mark.parametrize("K", [4, 32, 36, 100, 512])
@pytest.mark.parametrize("form", G.FORMS)
def test_fmaf_chain_stays_inside_the_exact_bound(form, K, nchunks):
    rng = _rng("chain", form, K, nchunks)
    a, b = _normal(rng, form, 44, 40, K)
    ref, S = G.product(a, b, form)
    ck = _chunk_k(K, nchunks)
    got = G.exact_emulated(a, b, form, nchunks, ck)
    _ratio("chain" if nchunks == 1 else "chain, chunks", got, ref, G.exact_bound(S, K, nchunks, ck))
    if nchunks == 1:   # another order of the same chain: the bound does not depend on it
        _ratio("chain", G.chain_f32(a, b, form, list(range(K))[::-1]), ref, G.exact_bound(S, K))


@pytest.mark.parametrize("hi", ["rne", "trunc"])
@pytest.mark.parametrize("K", [4, 32, 36, 100, 512])
def test_bf16_split_stays_inside_the_nt_bound(K, hi):
    rng = _rng("split", K, hi)
    a, b = _normal(rng, "nt", 44, 40, K)
    ref, S = G.product(a, b, "nt")
    got = G.split_emulated(a, b, "nt", hi)
    _ratio(f"split {hi}", got, ref, G.nt_bound(S, K, G.D_RNE if hi == "rne" else G.D_TRUNC))
    # the bound sees the split: hi.hi alone (d |x| per operand) leaves it
    ha, hb = G.split_bf16(a, hi)[0], G.split_bf16(b, hi)[0]
    assert np.any(np.abs(G.product(ha, hb, "nt")[0] - ref) > 2 * G.nt_bound(S, K))


@pytest.mark.parametrize("R,M,N", [(1, 4, 8), (31, 8, 4), (32, 4, 4), (33, 8, 8), (64, 4, 4), (293, 8, 12), (8197, 4, 4), (2053, 260, 260)])
def test_atb_emulation_stays_inside_the_atb_bound(R, M, N):
    rng = _rng("atb", R, M, N)
    plan = G.AtbPlan(R, M, N)
    a, b = rng.normal(size=(R, M)).astype(np.float32), rng.normal(size=(R, N)).astype(np.float32)
    sub = (slice(None), slice(0, 8))            # the plan of the full shape, the arithmetic of a few columns
    plan.M, plan.N = a[sub].shape[1], b[sub].shape[1]
    ref, S = G.product(a[sub], b[sub], "tn")
    _ratio("atb", G.atb_emulated(a[sub], b[sub], plan), ref, G.atb_bound(S, R, plan))


def test_bf16_rounding_is_torchs():
    rng = _rng("bf16")
    x = np.concatenate([rng.normal(size=4000), rng.normal(size=4000) * 1e-20, rng.normal(size=4000) * 1e20,
                        [0.0, -0.0, 1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 2.0 ** -130]]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(G.bf16_rne(x).view(np.uint32), want.view(np.uint32))
    t = G.bf16_trunc(x)
    assert np.all(t.view(np.uint32) & 0xFFFF == 0) and np.all(np.abs(t) <= np.abs(x)) and np.all(np.abs(x - t) <= G.D_TRUNC * np.abs(x))
    hi, lo = G.split_bf16(x)
    n = np.abs(x) > 1e-30                        # (normal numbers: the relative statements of the derivation)
    assert np.all(np.abs(x - hi)[n] <= G.D_RNE * np.abs(x)[n]) and np.all(np.abs(lo)[n] <= (1 + 2.0 ** -9) * G.D_RNE * np.abs(x)[n])
    assert np.all(np.abs(x.astype(np.float64) - hi - lo)[n] <= 2.0 ** -9 * G.D_RNE * np.abs(x)[n])


# ---------------------------------------------------------------------------------------------------------------------------------
# EXACT operands
# ---------------------------------------------------------------------------------------------------------------------------------
def _exact_ops(rng, form, I, J, K):
    sa, sb = G.operand_shapes(form, I, J, K)
    return _exact(rng, sa), _exact(rng, sb)


EXACT_ARITH = sorted({(c[0], c[3], p.nchunks, p.chunk_k) for c in G.EXACT_CASES for p in [G.plan_exact(*c[:4])]}
                     | {(c[0], c[3], 8, p.rem_chunk_k) for c in G.EXACT_CASES for p in [G.plan_exact(*c[:4])] if p.main_rows})


@pytest.mark.parametrize("form,K,nchunks,chunk_k", EXACT_ARITH, ids=lambda v: str(v))
def test_exact_operands_are_exact_in_the_exact_product(form, K, nchunks, chunk_k):
    """Every (form, K, chunking) of the GPU module's cases, on a block of the output small enough to emulate: the fp32 chain with
    its chunk sum returns the float64 product bit for bit, and the predicate certifies it."""
    rng = _rng("exact", form, K, nchunks)
    a, b = _exact_ops(rng, form, 12, 8, K)
    ref, S = G.product(a, b, form)
    assert G.product_is_exact(S).all() and np.all(S <= K * 2.0 ** -6)
    assert np.array_equal(G.exact_emulated(a, b, form, nchunks, chunk_k).astype(np.float64), ref)


def test_exact_predicate_holds_for_every_case_size():
    """|a| |b| <= 2^-6 per term: S <= K 2^-6 < 2^12 for every K of every family's cases, so the predicate holds for any EXACT draw."""
    ks = [c[3] for c in G.EXACT_CASES + G.EPI_CASES] + [c[2] for c in G.NT_CASES + G.NT_PRE_CASES] + [c[0] for c in G.ATB_CASES]
    worst = np.full((1, 1), max(ks) * 2.0 ** -6)
    assert G.product_is_exact(worst).all() and not G.product_is_exact(np.full((1, 1), 2.0 ** 18 * 2.0 ** -6)).any()


@pytest.mark.parametrize("K", sorted({c[2] for c in G.NT_CASES + G.NT_PRE_CASES}))
def test_exact_operands_are_exact_in_the_split(K):
    rng = _rng("exact split", K)
    a, b = _exact(rng, (12, K)), _exact(rng, (8, K))
    for x in (a, b):
        hi, lo = G.split_bf16(x)
        assert np.array_equal(hi, x) and not lo.any() and np.array_equal(G.bf16_trunc(x), x)
    ref, S = G.product(a, b, "nt")
    assert G.product_is_exact(S).all()
    assert np.array_equal(G.split_emulated(a, b, "nt").astype(np.float64), ref)


@pytest.mark.parametrize("R,M,N", G.ATB_CASES, ids=lambda v: str(v))
def test_exact_operands_are_exact_in_atb(R, M, N):
    rng = _rng("exact atb", R, M, N)
    plan = G.AtbPlan(R, M, N)
    a, b = _exact(rng, (R, 4)), _exact(rng, (R, 4))
    plan.M = plan.N = 4
    ref, S = G.product(a, b, "tn")
    assert G.product_is_exact(S).all()
    assert np.array_equal(G.atb_emulated(a, b, plan).astype(np.float64), ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# plan models and the coverage of the case lists
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_case_is_admissible_and_names_its_plan():
    for c in G.EXACT_CASES + G.EPI_CASES:
        form, I, J, K, shape, nchunks, main_rows = c
        assert G.exact_admissible(form, I, J, K), c
        p = G.plan_exact(form, I, J, K)
        assert (G.SHAPE_NAMES[p.shape], p.nchunks, p.main_rows) == (shape, nchunks, main_rows), (c, p.answer())
    assert len(set(G.EXACT_CASES)) == len(G.EXACT_CASES)
    assert all(c[0] == "nt" and c[5] == 1 for c in G.EPI_CASES), "the fused epilogue refuses a plan split over k"


SWEEP_I = sorted({x for m in (64, 128, 256) for k in (1, 2, 3, 8, 9, 16, 17, 28, 31, 57, 65, 86, 128, 129, 256, 257, 352, 353, 513)
                  for x in (m * k, m * (k - 1) + 1, m * (k - 1) + 4)} | {5, 8, 200})
SWEEP_J = (4, 8, 47, 64, 68, 100, 128, 132, 256, 260, 384, 388, 512, 516, 772, 1024, 2052, 4096)
SWEEP_K = (1, 4, 31, 32, 33, 36, 64, 100, 256, 260, 508, 512, 516, 1024, 1028, 2048, 4092, 4096, 8448, 65536, 165000)


def test_cases_reach_every_branch_the_plan_model_produces():
    """(form, tile shape, split, tail) over a sweep of admissible arguments -- tile multiples and their neighbours in I, the J and K at
    which make_plan decides -- against the branches of the GPU module's cases."""
    produced, tiles_seen = {}, set()
    for form, I, J, K in itertools.product(G.FORMS, SWEEP_I, SWEEP_J, SWEEP_K):
        if G.exact_admissible(form, I, J, K):
            p = G.plan_exact(form, I, J, K)
            produced.setdefault(p.branch(form), (I, J, K))
            if p.nchunks == 1:
                tiles_seen.add((form, G.SHAPE_NAMES[p.shape], p.tiles_i))
    reached = {G.plan_exact(*c[:4]).branch(c[0]) for c in G.EXACT_CASES}
    assert len(produced) == 34
    missing = set(produced) - reached
    assert not missing, {b: produced[b] for b in missing}
    assert not reached - set(produced), "a case reaches a branch the sweep does not produce: widen the sweep"
    # no (k-major a) plan has a tail launch, no tn plan another shape than these three
    assert not any(b[0] == "tn" and (b[3] or b[1] not in ("S64x512", "S128", "S256")) for b in produced)
    # tile counts per shape the cases reach: 8 and 9 row tiles (the slot mapping of a launch without a split: ti = xcd + 8 (slot /
    # tiles_j), the slots past tiles_i return) wherever a plan with them exists
    have = {(c[0], c[4], G.plan_exact(*c[:4]).tiles_i) for c in G.EXACT_CASES if c[5] == 1}
    lacking = {k for k in tiles_seen if k[2] in (8, 9) and k not in have}
    assert not lacking, lacking


def test_split_cases_cover_empty_partial_and_second_xcd_group():
    plans = [(c, G.plan_exact(*c[:4])) for c in G.EXACT_CASES if c[5] > 1]
    for form in G.FORMS:
        mine = [p for c, p in plans if c[0] == form]
        lens = [[max(min((q + 1) * p.chunk_k, p.K) - min(q * p.chunk_k, p.K), 0) for q in range(p.nchunks)] for p in mine]
        assert any(l[-1] == 0 for l in lens), f"{form}: no case with an empty last chunk"
        assert any(0 < x < p.chunk_k for p, l in zip(mine, lens) for x in l), f"{form}: no case with a partial chunk"
        assert any(p.nchunks == 8 for p in mine) and any(p.nchunks > 8 for p in mine)
    assert any(p.nchunks % 8 == 0 and p.nchunks > 8 and p.shape == G.S128 and p.K >= 4096 and p.J > 128 for _, p in plans), "the K >= 4096 override"
    tails = [G.plan_exact(*c[:4]) for c in G.EXACT_CASES if c[6] > 0]
    assert {(p.rem_tiles_i * p.tiles_j) for p in tails} >= {1, 96} and any(p.rem_chunk_k * 8 > p.K + G.KBK for p in tails)
    assert {c[0] for c in G.EXACT_CASES if c[6] > 0} == {"nt", "nn"}


def test_atb_plan_edges():
    P = G.AtbPlan
    assert (P(1, 4, 4).r_main, P(31, 4, 4).chunk_rows, P(31, 4, 4).nchunks) == (0, 0, 8)           # all from the scalar loop
    assert sum(P(32, 4, 4).chunk_stages()) == 1 and P(33, 4, 4).r_main == 32 and sum(P(64, 4, 4).chunk_stages()) == 2
    p = P(293, 36, 260)                                                                              # 9 stages over 16 chunks of 32 rows
    assert (p.nchunks, p.chunk_rows, sum(p.chunk_stages()), p.trailing_chunks_beyond()) == (16, 32, 9, 6)
    p = P(8197, 4, 4)
    assert (p.nchunks, p.chunk_rows, p.chunk_stages()) == (256, 32, [1] * 256)
    p = P(2053, 260, 260)
    assert (p.ntile, p.nchunks, p.chunk_rows, p.r_main) == (4, 64, 32, 2048)
    for R, M, N in G.ATB_CASES:
        p = P(R, M, N)
        assert sum(p.chunk_stages()) * G.KBK == p.r_main, "every row of r_main belongs to exactly one chunk"
    assert {G.nt_variant(R, N) for R, N, _ in G.NT_CASES} == {2, 4}
    assert G.nt_variant(32512, 4) == 2 and G.nt_variant(32513, 4) == 4
