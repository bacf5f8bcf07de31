"""GPU tier: the graph-level pooling kernels of csrc/lift_pool.hip and fitgnn_sum_leading_f32 (csrc/gcn_ops.hip) through the C ABI
against the float64 references of tests/pool_reference.py, with the helpers and the two kinds of input of
tests/test_gpu_step_kernels.py: EXACT inputs (small integers over 64, power-of-two scales) must come back bit for bit; RANDOM inputs
are held to k * 2^-24 * (sum of |terms| of that entry), k the number of roundings on that entry's path.

Launcher -> branch -> tests that reach it:

| launcher | branch (from the launch code and the kernel) | tests |
|---|---|---|
| fitgnn_segment_sum_f32 | <4> (F % 4 == 0, ldx % 4 == 0, ldo % 4 == 0, aligned): F = 4, 256 (one slab), 260 (second slab: one live lane, the others re-read columns F - 4 ...), 516 (third slab); ldx > F, ldo > F | test_segment_sum[vec-*] |
| | <1>: F = 1, 37, 65 (second 64-column slab: one live lane); F = 64 with X one float into its buffer; ldx = 4 ceil(F / 4) with ldo = F (the de-duplicated layer-0 adjoint's call); F = 64 with ldo % 4 != 0 | test_segment_sum[one-*] |
| | member loop: 0 members (zeros), cnt % 4 = 1, 2, 3, 0 (lengths 1, 5 / 3, 63 / 4, 64, 68), a second and a fifth 64-member chunk (65, 68, 129, 300) with its tail; unsorted members with repeats; members at the last row of X (NaN behind it) | every test_segment_sum case: one index holds all lengths |
| | n_seg = 1, 5 (last workgroup: one live wave), 8, 11 (three live waves) | test_segment_sum[*-nseg*] |
| | fixed order: two launches, same bits; RANDOM values | test_segment_sum_random |
| | n_seg = 0 returns 0; members NULL, ldx < F, ldo < F refused | test_segment_refusals |
| fitgnn_segment_max_f32 | float4 loads (f0 + 4 <= F) and the scalar column tail (F = 3, ldx = 4: tail only; F = 37, ldx = 40: nine groups + a tail of one); one slab (F <= 256) and a second slab with one live lane (F = 260); members given / NULL; the same lengths, 0 members -> -inf / -1; n_seg = 5, 11 | test_segment_max |
| | update rule: two- and three-way ties (first in MEMBER order, which is not the smallest row id), a column of -inf (first member) | test_segment_max_ties_and_inf |
| | NaN as first, middle, last member (and two NaNs: the first one is arg) | test_segment_max_nan_position |
| | F = 0 returns 0; X one float into its buffer, ldx % 4 != 0 -> FITGNN_E_ALIGN; ldx < F refused | test_segment_refusals |
| fitgnn_segment_max_bwd_f32 | n = n_seg F on both sides of a multiple of 256; arg = -1 writes nothing; ldd > F; everything but the arg elements untouched | test_segment_max_bwd |
| | n_seg = 0 returns 0; ldd < F refused | test_segment_refusals |
| fitgnn_segment_expand_f32 | n_rows F / 4 = 255, 256, 257 (F = 4) and 9 x 250 (F = 36); seg_of_row = -1 -> zeros over NaN; scale NULL / given | test_segment_expand |
| | n_rows = 0 returns 0; F % 4 != 0 refused; src one float into its buffer -> FITGNN_E_ALIGN | test_segment_refusals |
| fitgnn_pool_head_f32 | F = 4 ... 1024 (PH = 256 / (F / 4) = 256, 64, 16, 4, 2, 1 row phases; tree depth log2(F / 4) = 0 ... 8) x C = 1, 3, 8; member loop: 0, 1, PH, PH + 1, 4 PH - 1, 4 PH, 4 PH + 1, 9 PH + 2 members (no trip; one trip with 3, 2, 0 clamped loads; two and three trips); ldx > F; b NULL / given | test_pool_head_exact |
| | RANDOM values; fixed order: two launches, same bits | test_pool_head_random |
| | C = 9, F = 12, F = 2048, ldx % 4 != 0, ldx < F refused; pooled one float into its buffer -> FITGNN_E_ALIGN | test_pool_head_refusals |
| fitgnn_pool_head_bwd_f32 | dx blocks: n_rows F / 4 = 255, 256, 257 (F = 4), 240, 256, 272 (F = 64), one and three float4 rows of F = 1024; rows of no segment -> zeros; weight blocks: none launched (dW = db = NULL), launched with one of them NULL, both given; (C F + C) on both sides of a multiple of 256; n_seg = 1, 37 (the 8-unrolled loop: 0 and 4 full rounds + 1 and 5 left over) | test_pool_head_bwd_exact |
| | RANDOM values; fixed order | test_pool_head_bwd_random |
| | C = 9, F = 12 refused; dx NULL with rows refused | test_pool_head_refusals |
| fitgnn_sum_leading_f32 | B = 1, 3 (tail loop only), 4, 5, 91 (22 rounds of four + 3); W / 4 = 1, 255, 256, 257 (one workgroup partial / full, a second with one live thread) | test_sum_leading_exact |
| | the two-stage use of ops.mm_at_b: [B / G, G W] then G + B % G rows | test_sum_leading_two_stage |
| | RANDOM values; fixed order; W = 0 returns 0; B = 0, W % 4 != 0 refused, `part` one float in -> FITGNN_E_ALIGN | test_sum_leading_random, test_segment_refusals |

Bounds that are not bit-exact (u = 2^-24, cond = the same operation on |inputs|: the sum of |terms| of that entry), with the worst
observed error / bound over all entries of one MI355X run in brackets.  k is the derived count with no allowance on top, so an
entry whose path has one to three roundings can come close to its bound (a single rounding reaches u on its own): the second figure
is the worst over the entries with k >= 8.
* segment_sum: a segment's n member values enter one running fp32 sum in member order (the padding loads add exact zeros): n - 1
  roundings, |err| <= (n - 1) u cond.  [0.61 at segments of 3 to 5 members; 0.042 for k >= 8]
* segment_expand with a general scale: one product, u |ref|.  [0.80]
* pool_head, pooled: phase q sums members q, q + PH, ... (ceil(n / PH) values: one rounding less), phase 0's lanes add the min(n, PH)
  non-empty phase totals in ascending order (min(n, PH) - 1 roundings that are not + 0), the scale rounds once:
  k_p = ceil(n / PH) + min(n, PH) - 1, |err| <= k_p u cond_p.  [0.60; 0.26 for k >= 8]
  y: each lane's four-term fma chain rounds 4 times, the LDS tree log2(F / 4) times, the bias once, on top of the pooled row's own
  error carried through |W|: |err| <= (bound_p |W|^T) + (5 + log2(F / 4)) u cond_y.  [0.094]
* pool_head_bwd: dx = C fused multiply-adds (C roundings) and the scale: (C + 1) u cond; dW = n_seg fused multiply-adds: n_seg u cond;
  db = n_seg - 1 additions: (n_seg - 1) u cond.  [dx 0.87 at C = 1 (two roundings), 0.35 at C = 8; dW 0.29; db 0.027]
* sum_leading: row b goes to running sum b % 4 (B // 4 values each: one rounding less), the B % 4 left-over rows to sum 0, then two
  levels combine the four: k = B // 4 + B % 4 + 1 roundings, |err| <= k u cond.  [0.51 at B = 5 (three roundings); 0.035 at B = 91]
"""
import numpy as np
import pytest
import torch

import pool_reference as pr
from test_gpu_step_kernels import (E_ALIGN, E_BADARG, L, U, _call, _dev, _exact, _np, _offset_copy, _p, _rng, _run,  # noqa: F401
                                   _same, _strided, _within)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 68, 129, 300]
WORST = {}


def _bounded(family, got, ref, bound, what, k=None):
    """_within, and the worst error / bound ratio of the family printed (run with -s) for the module docstring; with the roundings
    count k of every entry, also the worst ratio over the entries whose path has at least 8 roundings."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"[ratio] {family}: {what}: {ratio:.3g} (family worst {WORST[family]:.3g})")
    if k is not None:
        long = pos & (np.broadcast_to(np.asarray(k), err.shape) >= 8)
        if long.any():
            print(f"[ratio] {family}, k >= 8: {what}: {float((err[long] / bound[long]).max()):.3g} (family worst as printed)")
    _within(got, ref, bound, what)


def _same_nan(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern differs at {np.argwhere(np.isnan(got) != np.isnan(ref))[:3].tolist()}"
    _same(np.nan_to_num(got, nan=0.0), np.nan_to_num(ref, nan=0.0), what)


def _index(rng, lengths, n_rows, distinct=False):
    """(off, members) of segments with the given lengths: unsorted rows with repeats (or distinct ones); wherever a segment has
    members, one of them is the last row of X."""
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    if distinct:
        members = rng.permutation(n_rows)[:off[-1]]
    else:
        members = rng.integers(0, n_rows, size=off[-1])
        for s in range(len(lengths)):
            if lengths[s]:
                members[rng.integers(off[s], off[s + 1])] = n_rows - 1
    return off, members.astype(np.int64)


def _i32(a):
    return _dev(np.asarray(a), torch.int32)


def _guarded(shape, fill=NAN, dtype=torch.float32):
    """A contiguous device array followed by 4 guard elements holding `fill`."""
    n = int(np.prod(shape))
    buf = torch.full((n + 4,), fill, dtype=dtype, device="cuda")
    return buf, buf[:n].view(*shape)


def _lengths_for(n_seg):
    return LENGTHS[-n_seg:]


# ---------------------------------------------------------------------------------------------------------------------------------
# segment sum
# ---------------------------------------------------------------------------------------------------------------------------------
# (id, F, ldx, ldo, offset of X in floats)
SUM_FORMS = [("vec-F4", 4, 8, 12, 0), ("vec-F256", 256, 260, 264, 0), ("vec-F260", 260, 264, 268, 0), ("vec-F516", 516, 520, 520, 0),
             ("one-F1", 1, 4, 2, 0), ("one-F37", 37, 40, 38, 0), ("one-F65", 65, 68, 66, 0), ("one-F64-offset", 64, 68, 64, 1),
             ("one-F37-dedup", 37, 40, 37, 0), ("one-F64-ldo", 64, 64, 65, 0)]


def _segment_sum(L, off, members, X, ldx, ldo, offset):
    n_seg, F = len(off) - 1, X.shape[1]
    Xd = _strided(X, ldx, offset)
    out = torch.full((n_seg, ldo), NAN, device="cuda")
    ot, mt = _i32(off), _i32(members)
    rc = _call(L, "fitgnn_segment_sum_f32", _p(L, ot), _p(L, mt), n_seg, _p(L, Xd), ldx, F, _p(L, out), ldo)
    return rc, out


@pytest.mark.parametrize("n_seg", [1, 5, 8, 11], ids=lambda v: f"nseg{v}")
@pytest.mark.parametrize("form", SUM_FORMS, ids=lambda f: f[0])
def test_segment_sum(L, form, n_seg):
    _, F, ldx, ldo, offset = form
    rng = _rng("segsum", form, n_seg)
    n_rows = 211
    off, members = _index(rng, _lengths_for(n_seg), n_rows)
    X = _exact(rng, (n_rows, F))
    rc, out = _segment_sum(L, off, members, X, ldx, ldo, offset)
    L.check(rc, "fitgnn_segment_sum_f32")
    got = _np(out)
    _same(got[:, :F], pr.segment_sum(off, members, X), "out")      # a read past a row's F columns would be NaN here
    assert np.all(np.isnan(got[:, F:])), "wrote past column F of out"


@pytest.mark.parametrize("form", [SUM_FORMS[2], SUM_FORMS[5]], ids=lambda f: f[0])
def test_segment_sum_random(L, form):
    _, F, ldx, ldo, offset = form
    rng = _rng("segsum_random", form)
    off, members = _index(rng, LENGTHS, 211)
    X = rng.normal(size=(211, F)).astype(np.float32)
    rc, out = _segment_sum(L, off, members, X, ldx, ldo, offset)
    L.check(rc, "fitgnn_segment_sum_f32")
    k = np.maximum(np.diff(off) - 1, 0)[:, None]
    _bounded("segment_sum", _np(out)[:, :F], pr.segment_sum(off, members, X), k * U * pr.segment_sum(off, members, np.abs(X)), "out", k)
    rc, again = _segment_sum(L, off, members, X, ldx, ldo, offset)
    assert torch.equal(out[:, :F], again[:, :F]), "two launches on the same input differ"


# ---------------------------------------------------------------------------------------------------------------------------------
# segment max
# ---------------------------------------------------------------------------------------------------------------------------------
def _segment_max(L, off, members, X, ldx, offset=0):
    n_seg, F = len(off) - 1, X.shape[1]
    Xd = _strided(X, ldx, offset)
    obuf, out = _guarded((n_seg, F))
    abuf, arg = _guarded((n_seg, F), fill=-7, dtype=torch.int32)
    ot = _i32(off)
    mt = None if members is None else _i32(members)
    rc = _call(L, "fitgnn_segment_max_f32", _p(L, ot), _p(L, mt), n_seg, _p(L, Xd), ldx, F, _p(L, out), _p(L, arg))
    assert torch.isnan(obuf[-4:]).all().item() and torch.all(abuf[-4:] == -7).item(), "wrote past the end of out / arg"
    return rc, out, arg


def _check_max(L, off, members, X, ldx, what):
    rc, out, arg = _segment_max(L, off, members, X, ldx)
    L.check(rc, "fitgnn_segment_max_f32")
    rout, rarg = pr.segment_max(off, members, X)
    _same_nan(_np(out), rout, f"{what}: out")
    _same(arg.cpu().numpy(), rarg, f"{what}: arg")
    return rarg


MAX_FORMS = [(3, 4), (37, 40), (256, 260), (260, 264)]


@pytest.mark.parametrize("n_seg", [5, 11], ids=lambda v: f"nseg{v}")
@pytest.mark.parametrize("with_members", [True, False], ids=["members", "identity"])
@pytest.mark.parametrize("F,ldx", MAX_FORMS, ids=lambda v: str(v))
def test_segment_max(L, F, ldx, with_members, n_seg):
    rng = _rng("segmax", F, with_members, n_seg)
    lengths = _lengths_for(n_seg)
    n_rows = 750 if with_members else int(np.sum(lengths))
    off, members = _index(rng, lengths, n_rows)
    X = _exact(rng, (n_rows, F))                  # 17 distinct values over up to 300 members: ties in every long segment
    _check_max(L, off, members if with_members else None, X, ldx, f"F={F}")


@pytest.mark.parametrize("F,ldx", [(3, 4), (37, 40), (260, 264)], ids=lambda v: str(v))
def test_segment_max_ties_and_inf(L, F, ldx):
    """Column c takes pattern c % 3 of: a two-way tie, a three-way tie, all -inf.  Segment 0 lists rows 6, 2, 4, 1, 5: the first
    maximum in member order is row 6 (two-way: rows 6 and 1; three-way: rows 6, 4, 1), the smallest row id holding it is row 1."""
    X = np.zeros((8, F), dtype=np.float32)
    pat = np.arange(F) % 3
    for row, (two, three) in {6: (2.0, 5.0), 2: (1.0, -1.0), 4: (-3.0, 5.0), 1: (2.0, 5.0), 5: (0.5, 4.0)}.items():
        X[row] = np.where(pat == 0, two, np.where(pat == 1, three, -INF))
    X[[0, 3, 7]] = 9.0                              # rows of no segment
    off, members = np.array([0, 5, 5, 7]), np.array([6, 2, 4, 1, 5, 5, 2])
    rarg = _check_max(L, off, members, X, ldx, "ties")
    assert np.all(rarg[0] == 6) and np.all(rarg[1] == -1)
    assert np.all(rarg[2][pat != 2] == np.where(pat == 0, 2, 5)[pat != 2]) and np.all(rarg[2][pat == 2] == 5)


@pytest.mark.parametrize("F,ldx", [(3, 4), (37, 40), (260, 264)], ids=lambda v: str(v))
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_segment_max_nan_position(L, where, F, ldx):
    """One NaN per segment and column group, at the given position of the member list, makes that output NaN with arg = its row, as
    torch's amax does from any position; odd columns get a second, later NaN, which must not replace the first as arg."""
    rng = _rng("segmax_nan", where, F)
    off, members = _index(rng, LENGTHS, 750, distinct=True)
    X = _exact(rng, (750, F))
    want = np.full((len(LENGTHS), F), -1)
    for s in range(len(LENGTHS)):
        n = int(off[s + 1] - off[s])
        if n == 0:
            continue
        pos = {"first": 0, "middle": n // 2, "last": n - 1}[where]
        X[members[off[s] + pos], ::2] = NAN
        want[s, ::2] = members[off[s] + pos]
        if n >= 3:                                 # two NaNs in the odd columns: the earlier one is arg
            X[members[off[s] + n // 3], 1::2] = NAN
            X[members[off[s] + n - 1], 1::2] = NAN
            want[s, 1::2] = members[off[s] + n // 3]
    rc, out, arg = _segment_max(L, off, members, X, ldx)
    L.check(rc, "fitgnn_segment_max_f32")
    rout, rarg = pr.segment_max(off, members, X)
    nonempty = np.diff(off) > 0
    assert np.all(np.isnan(rout[nonempty][:, ::2])) and np.all(rarg[:, ::2] == want[:, ::2])
    assert np.all(rarg[:, 1::2][np.diff(off) >= 3] == want[:, 1::2][np.diff(off) >= 3])
    _same_nan(_np(out), rout, "out")
    _same(arg.cpu().numpy(), rarg, "arg")


@pytest.mark.parametrize("F,ldd", [(3, 5), (37, 40), (256, 260)], ids=lambda v: str(v))
def test_segment_max_bwd(L, F, ldd):
    rng = _rng("segmax_bwd", F)
    off, members = _index(rng, LENGTHS, 750, distinct=True)     # disjoint segments; lengths[0] = 0: a segment whose arg is -1
    X = _exact(rng, (750, F))
    _, arg = pr.segment_max(off, members, X)
    g = _exact(rng, arg.shape, lo=1, hi=8)          # no zero: a missing store shows
    dst = torch.full((750, ldd), NAN, device="cuda")
    dst[:, :F] = 0.0
    gd, ad = _dev(g), _i32(arg)
    _run(L, "fitgnn_segment_max_bwd_f32", _p(L, gd), _p(L, ad), len(LENGTHS), F, _p(L, dst), ldd)
    got = _np(dst)
    ref = pr.segment_max_bwd(g, arg, 750)
    _same(got[:, :F], ref, "dst")
    assert np.count_nonzero(ref) == (len(LENGTHS) - 1) * F and np.all(np.isnan(got[:, F:])), "wrote outside the arg elements"


# ---------------------------------------------------------------------------------------------------------------------------------
# segment expand
# ---------------------------------------------------------------------------------------------------------------------------------
def _segment_expand(L, src, seg_of_row, scale, F):
    n_rows = len(seg_of_row)
    sd, st = _dev(src), _i32(seg_of_row)
    wd = None if scale is None else _dev(scale)
    buf, dst = _guarded((n_rows, F))
    rc = _call(L, "fitgnn_segment_expand_f32", _p(L, sd), _p(L, st), _p(L, wd), n_rows, F, _p(L, dst))
    assert torch.isnan(buf[-4:]).all().item(), "wrote past the end of dst"
    return rc, dst


@pytest.mark.parametrize("scale_kind", ["none", "pow2", "random"])
@pytest.mark.parametrize("n_rows,F", [(255, 4), (256, 4), (257, 4), (250, 36)], ids=lambda v: str(v))
def test_segment_expand(L, n_rows, F, scale_kind):
    rng = _rng("expand", n_rows, F, scale_kind)
    n_seg = 9
    seg_of_row = rng.integers(-1, n_seg, size=n_rows)
    seg_of_row[[0, n_rows - 1]] = [-1, n_seg - 1]
    src = _exact(rng, (n_seg, F), lo=1, hi=8)
    scale = {"none": None, "pow2": (2.0 ** rng.integers(-5, 3, size=n_seg)).astype(np.float32),
             "random": rng.uniform(0.01, 1.0, size=n_seg).astype(np.float32)}[scale_kind]
    rc, dst = _segment_expand(L, src, seg_of_row, scale, F)
    L.check(rc, "fitgnn_segment_expand_f32")
    ref = pr.segment_expand(src, seg_of_row, scale)
    got = _np(dst)
    assert np.all(got[seg_of_row < 0] == 0) and not np.isnan(got).any(), "a row of no segment is not zero / a row was not written"
    if scale_kind == "random":
        _bounded("segment_expand", got, ref, U * np.abs(ref), "dst")
    else:
        _same(got, ref, "dst")


def test_segment_refusals(L):
    z = lambda *s: torch.zeros(*s, device="cuda")   # noqa: E731
    off, mem = _i32([0, 2, 4]), _i32([0, 1, 2, 3])
    X8, out, arg = z(4, 8), z(2, 8), torch.zeros(2, 8, dtype=torch.int32, device="cuda")
    S = lambda *a: _call(L, "fitgnn_segment_sum_f32", *a)   # noqa: E731
    assert S(_p(L, off), _p(L, mem), 2, _p(L, X8), 8, 8, _p(L, out), 8) == 0
    assert S(_p(L, off), None, 2, _p(L, X8), 8, 8, _p(L, out), 8) == E_BADARG
    assert S(_p(L, off), _p(L, mem), 2, _p(L, X8), 7, 8, _p(L, out), 8) == E_BADARG
    assert S(_p(L, off), _p(L, mem), 2, _p(L, X8), 8, 8, _p(L, out), 7) == E_BADARG
    M = lambda *a: _call(L, "fitgnn_segment_max_f32", *a)   # noqa: E731
    Xo = _offset_copy(np.zeros((4, 8), np.float32), 1)
    assert M(_p(L, off), _p(L, mem), 2, _p(L, X8), 8, 8, _p(L, out), _p(L, arg)) == 0
    assert M(_p(L, off), _p(L, mem), 2, _p(L, Xo), 8, 8, _p(L, out), _p(L, arg)) == E_ALIGN
    assert M(_p(L, off), _p(L, mem), 2, _p(L, X8), 7, 6, _p(L, out), _p(L, arg)) == E_ALIGN     # ldx % 4 != 0
    assert M(_p(L, off), _p(L, mem), 2, _p(L, X8), 4, 8, _p(L, out), _p(L, arg)) == E_BADARG    # ldx < F
    seg = _i32([0, 1, -1, 0])
    E = lambda *a: _call(L, "fitgnn_segment_expand_f32", *a)   # noqa: E731
    assert E(_p(L, out), _p(L, seg), None, 4, 8, _p(L, X8)) == 0
    assert E(_p(L, out), _p(L, seg), None, 4, 6, _p(L, X8)) == E_BADARG                         # F % 4 != 0
    src_off = _offset_copy(np.zeros((2, 8), np.float32), 1)
    assert E(_p(L, src_off), _p(L, seg), None, 4, 8, _p(L, X8)) == E_ALIGN
    G = lambda *a: _call(L, "fitgnn_segment_max_bwd_f32", *a)   # noqa: E731
    assert G(_p(L, out), _p(L, arg), 2, 8, _p(L, X8), 7) == E_BADARG                            # ldd < F
    # nothing to do: 0 before any pointer is looked at
    assert S(None, None, 0, None, 8, 8, None, 8) == 0 and M(None, None, 2, None, 0, 0, None, None) == 0
    assert G(None, None, 0, 8, None, 8) == 0 and E(None, None, None, 0, 8, None) == 0
    B = lambda *a: _call(L, "fitgnn_sum_leading_f32", *a)   # noqa: E731
    assert B(None, 4, 0, None) == 0
    assert B(_p(L, X8), 4, 8, _p(L, out)) == 0
    assert B(_p(L, X8), 0, 8, _p(L, out)) == E_BADARG
    assert B(_p(L, X8), 4, 6, _p(L, out)) == E_BADARG
    assert B(_p(L, Xo), 4, 8, _p(L, out)) == E_ALIGN


# ---------------------------------------------------------------------------------------------------------------------------------
# mean pool + head
# ---------------------------------------------------------------------------------------------------------------------------------
def _ph_lengths(F):
    PH = 256 // (F // 4)
    return PH, [0, 1, PH, PH + 1, 4 * PH - 1, 4 * PH, 4 * PH + 1, 9 * PH + 2]


def _pool_head(L, off, members, X, ldx, inv_cnt, W, b):
    n_seg, F, C = len(off) - 1, X.shape[1], W.shape[0]
    Xd = _strided(X, ldx)
    ot, mt, it, Wd = _i32(off), _i32(members), _dev(inv_cnt), _dev(W)
    bd = None if b is None else _dev(b)
    pbuf, pooled = _guarded((n_seg, F))
    ybuf, y = _guarded((n_seg, C))
    rc = _call(L, "fitgnn_pool_head_f32", _p(L, ot), _p(L, mt), n_seg, _p(L, Xd), ldx, F, _p(L, it), _p(L, Wd), _p(L, bd), C, _p(L, pooled),
               _p(L, y))
    assert torch.isnan(pbuf[-4:]).all().item() and torch.isnan(ybuf[-4:]).all().item(), "wrote past the end of pooled / y"
    return rc, pooled, y


@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("F", [4, 16, 64, 256, 512, 1024])
def test_pool_head_exact(L, F, C):
    rng = _rng("pool_head", F, C)
    PH, lengths = _ph_lengths(F)
    n_rows = int(np.sum(lengths)) // 2 + 3          # fewer rows than members: repeats
    off, members = _index(rng, lengths, n_rows)
    X = _exact(rng, (n_rows, F))
    inv = (2.0 ** -(np.arange(len(lengths)) % 3)).astype(np.float32)
    W = _exact(rng, (C, F), lo=-4, hi=4)
    b = None if C == 3 else _exact(rng, C)
    # the premise of exactness: every term of y is a multiple of 2^-14 and their absolute sum stays below 2^24 of them
    _, ycond = pr.pool_head(off, members, np.abs(X), inv, np.abs(W), None if b is None else np.abs(b))
    assert ycond.max() < 2.0 ** 10
    rc, pooled, y = _pool_head(L, off, members, X, F + 4, inv, W, b)
    L.check(rc, "fitgnn_pool_head_f32")
    rp, ry = pr.pool_head(off, members, X, inv, W, b)
    _same(_np(pooled), rp, f"pooled (PH={PH})")
    _same(_np(y), ry, "y")


@pytest.mark.parametrize("F,C", [(4, 3), (64, 8), (512, 1), (1024, 3)], ids=lambda v: str(v))
def test_pool_head_random(L, F, C):
    rng = _rng("pool_head_random", F, C)
    PH, lengths = _ph_lengths(F)
    n_rows = int(np.sum(lengths)) + 5
    off, members = _index(rng, lengths, n_rows)
    X = rng.normal(size=(n_rows, F)).astype(np.float32)
    n = np.diff(off)
    inv = (1.0 / np.maximum(n, 1)).astype(np.float32)
    W = rng.normal(size=(C, F)).astype(np.float32)
    b = rng.normal(size=C).astype(np.float32)
    rc, pooled, y = _pool_head(L, off, members, X, F + 8, inv, W, b)
    L.check(rc, "fitgnn_pool_head_f32")
    rp, ry = pr.pool_head(off, members, X, inv, W, b)
    pc, _ = pr.pool_head(off, members, np.abs(X), inv, np.abs(W), np.abs(b))
    k_p = np.maximum(-(-n // PH) + np.minimum(n, PH) - 1, 0)[:, None]
    bp = k_p * U * pc
    _bounded("pool_head pooled", _np(pooled), rp, bp, "pooled", k_p)
    ycond = np.abs(rp) @ np.abs(W.astype(np.float64)).T + np.abs(b.astype(np.float64))
    _bounded("pool_head y", _np(y), ry, bp @ np.abs(W.astype(np.float64)).T + (5 + np.log2(F // 4)) * U * ycond, "y")
    rc, pooled2, y2 = _pool_head(L, off, members, X, F + 8, inv, W, b)
    assert torch.equal(pooled, pooled2) and torch.equal(y, y2), "two launches on the same input differ"


def _pool_head_bwd(L, dy, W, pooled, seg_of_row, inv, with_dW, with_db):
    n_seg, C, F, n_rows = dy.shape[0], W.shape[0], W.shape[1], len(seg_of_row)
    dyd, Wd, pd, st, it = _dev(dy), _dev(W), _dev(pooled), _i32(seg_of_row), _dev(inv)
    xbuf, dx = _guarded((n_rows, F))
    wbuf, dW = _guarded((C, F))
    bbuf, db = _guarded((C,))
    rc = _call(L, "fitgnn_pool_head_bwd_f32", _p(L, dyd), _p(L, Wd), C, _p(L, pd), _p(L, st), _p(L, it), n_rows, n_seg, F, _p(L, dx),
               _p(L, dW) if with_dW else None, _p(L, db) if with_db else None)
    assert torch.isnan(xbuf[-4:]).all().item() and torch.isnan(wbuf[-4:]).all().item() and torch.isnan(bbuf[-4:]).all().item()
    if not with_dW:
        assert torch.isnan(dW).all().item(), "dW written although NULL was passed"
    if not with_db:
        assert torch.isnan(db).all().item(), "db written although NULL was passed"
    return rc, dx, dW, db


# (F, n_rows, C, n_seg): n_rows F / 4 and C F + C on both sides of a multiple of 256
PHB_SHAPES = [(4, 255, 1, 37), (4, 256, 3, 1), (4, 257, 8, 37), (64, 15, 3, 37), (64, 16, 8, 1), (64, 17, 1, 37), (1024, 1, 8, 1),
              (1024, 3, 1, 37), (16, 200, 3, 37), (256, 9, 1, 37), (512, 5, 8, 37), (256, 300, 3, 5)]


def _phb_inputs(rng, F, n_rows, C, n_seg, exact):
    seg_of_row = rng.integers(-1, n_seg, size=n_rows)
    seg_of_row[0] = -1 if n_rows > 1 else 0
    seg_of_row[-1] = n_seg - 1
    if exact:
        dy, W, pooled = _exact(rng, (n_seg, C), lo=-4, hi=4), _exact(rng, (C, F), lo=-4, hi=4), _exact(rng, (n_seg, F))
        inv = (2.0 ** -(np.arange(n_seg) % 4)).astype(np.float32)
    else:
        dy, W, pooled = (rng.normal(size=s).astype(np.float32) for s in ((n_seg, C), (C, F), (n_seg, F)))
        inv = rng.uniform(0.01, 1.0, size=n_seg).astype(np.float32)
    return dy, W, pooled, seg_of_row, inv


@pytest.mark.parametrize("with_dW,with_db", [(False, False), (True, False), (False, True), (True, True)], ids=["none", "dW", "db", "both"])
@pytest.mark.parametrize("F,n_rows,C,n_seg", PHB_SHAPES, ids=lambda v: str(v))
def test_pool_head_bwd_exact(L, F, n_rows, C, n_seg, with_dW, with_db):
    rng = _rng("pool_head_bwd", F, n_rows, C, n_seg)
    dy, W, pooled, seg_of_row, inv = _phb_inputs(rng, F, n_rows, C, n_seg, True)
    rc, dx, dW, db = _pool_head_bwd(L, dy, W, pooled, seg_of_row, inv, with_dW, with_db)
    L.check(rc, "fitgnn_pool_head_bwd_f32")
    rdx, rdW, rdb = pr.pool_head_bwd(dy, W, pooled, seg_of_row, inv)
    got = _np(dx)
    assert np.all(got[seg_of_row < 0] == 0), "a row of no segment is not zero"
    _same(got, rdx, "dx")
    if with_dW:
        _same(_np(dW), rdW, "dW")
    if with_db:
        _same(_np(db), rdb, "db")


@pytest.mark.parametrize("F,n_rows,C,n_seg", [(4, 257, 8, 37), (64, 17, 3, 37), (1024, 3, 8, 37), (256, 300, 1, 5)], ids=lambda v: str(v))
def test_pool_head_bwd_random(L, F, n_rows, C, n_seg):
    rng = _rng("pool_head_bwd_random", F, n_rows, C, n_seg)
    dy, W, pooled, seg_of_row, inv = _phb_inputs(rng, F, n_rows, C, n_seg, False)
    rc, dx, dW, db = _pool_head_bwd(L, dy, W, pooled, seg_of_row, inv, True, True)
    L.check(rc, "fitgnn_pool_head_bwd_f32")
    rdx, rdW, rdb = pr.pool_head_bwd(dy, W, pooled, seg_of_row, inv)
    cdx, cdW, cdb = pr.pool_head_bwd(np.abs(dy), np.abs(W), np.abs(pooled), seg_of_row, inv)
    _bounded("pool_head_bwd dx", _np(dx), rdx, (C + 1) * U * cdx, "dx", C + 1)
    _bounded("pool_head_bwd dW", _np(dW), rdW, n_seg * U * cdW, "dW")
    _bounded("pool_head_bwd db", _np(db), rdb, (n_seg - 1) * U * cdb, "db")
    rc, dx2, dW2, db2 = _pool_head_bwd(L, dy, W, pooled, seg_of_row, inv, True, True)
    assert torch.equal(dx, dx2) and torch.equal(dW, dW2) and torch.equal(db, db2), "two launches on the same input differ"


def test_pool_head_refusals(L):
    lib = L.lib()
    assert [lib.fitgnn_pool_head_supported(F, C) for F, C in ((1024, 8), (4, 1), (1024, 9), (12, 1), (2048, 1), (6, 1))] == [1, 1, 0, 0, 0, 0]
    rng = _rng("pool_head_refusals")

    def fwd(F, C, ldx, pooled_offset=0):
        off, members = np.array([0, 2, 3]), np.array([0, 1, 2])
        Xd = _strided(np.zeros((3, F), np.float32), max(ldx, F))
        pooled = _offset_copy(np.zeros((2, F), np.float32), pooled_offset)
        y = torch.zeros(2, C, device="cuda")
        ot, mt, it, Wd = _i32(off), _i32(members), _dev(np.ones(2, np.float32)), _dev(np.zeros((C, F), np.float32))
        return _call(L, "fitgnn_pool_head_f32", _p(L, ot), _p(L, mt), 2, _p(L, Xd), ldx, F, _p(L, it), _p(L, Wd), None, C, _p(L, pooled), _p(L, y))

    assert fwd(16, 8, 20) == 0
    assert fwd(16, 9, 20) == E_BADARG
    assert fwd(12, 1, 12) == E_BADARG               # 256 % (12 / 4) != 0
    assert fwd(2048, 1, 2048) == E_BADARG
    assert fwd(16, 1, 18) == E_BADARG               # ldx % 4 != 0
    assert fwd(16, 1, 12) == E_BADARG               # ldx < F
    assert fwd(16, 1, 16, pooled_offset=1) == E_ALIGN

    def bwd(F, C, with_dx=True):
        dy, W, pooled, seg_of_row, inv = _phb_inputs(rng, F, 5, C, 2, True)
        t = [_dev(dy), _dev(W), _dev(pooled), _i32(seg_of_row), _dev(inv), torch.zeros(5, F, device="cuda")]
        return _call(L, "fitgnn_pool_head_bwd_f32", _p(L, t[0]), _p(L, t[1]), C, _p(L, t[2]), _p(L, t[3]), _p(L, t[4]), 5, 2, F,
                     _p(L, t[5]) if with_dx else None, None, None)

    assert bwd(16, 8) == 0
    assert bwd(16, 9) == E_BADARG and bwd(12, 1) == E_BADARG and bwd(16, 1, with_dx=False) == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# sum over the leading axis
# ---------------------------------------------------------------------------------------------------------------------------------
def _sum_leading(L, part_t, B, W):
    buf, out = _guarded((W,))
    rc = _call(L, "fitgnn_sum_leading_f32", _p(L, part_t), B, W, _p(L, out))
    assert torch.isnan(buf[-4:]).all().item(), "wrote past the end of out"
    return rc, out


@pytest.mark.parametrize("W", [4, 1020, 1024, 1028])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 91])
def test_sum_leading_exact(L, B, W):
    part = _exact(_rng("sum_leading", B, W), (B, W))
    rc, out = _sum_leading(L, _dev(part), B, W)
    L.check(rc, "fitgnn_sum_leading_f32")
    _same(_np(out), pr.sum_leading(part), "out")


def test_sum_leading_two_stage(L):
    """ops.mm_at_b's fold of many partials: viewed as [B // G, G W] the kernel sums every G-th partial, then the G sums and the B % G
    left-over partials."""
    B, G, W = 91, 4, 1028
    part = _exact(_rng("sum_leading_two_stage"), (B, W))
    flat = _dev(part)
    Bg = B // G
    stage = torch.full((G + B - Bg * G, W), NAN, device="cuda")
    _run(L, "fitgnn_sum_leading_f32", _p(L, flat), Bg, G * W, _p(L, stage))
    assert torch.isnan(stage[G:]).all().item(), "the first stage wrote past its G rows"
    _same(_np(stage[:G]), part[:Bg * G].reshape(Bg, G, W).astype(np.float64).sum(0), "stage")
    stage[G:].copy_(flat[Bg * G:])
    rc, out = _sum_leading(L, stage, int(stage.shape[0]), W)
    L.check(rc, "fitgnn_sum_leading_f32")
    _same(_np(out), pr.sum_leading(part), "out")


@pytest.mark.parametrize("B,W", [(5, 1028), (91, 1020)])
def test_sum_leading_random(L, B, W):
    part = _rng("sum_leading_random", B, W).normal(size=(B, W)).astype(np.float32)
    pt = _dev(part)
    rc, out = _sum_leading(L, pt, B, W)
    L.check(rc, "fitgnn_sum_leading_f32")
    _bounded("sum_leading", _np(out), pr.sum_leading(part), (B // 4 + B % 4 + 1) * U * pr.sum_leading(np.abs(part)), "out",
             B // 4 + B % 4 + 1)
    rc, again = _sum_leading(L, pt, B, W)
    assert torch.equal(out, again), "two launches on the same input differ"
