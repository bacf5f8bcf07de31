"""GPU tier: the APPNP propagation kernels of csrc/gat.hip through the C ABI against the float64 references of
tests/appnp_reference.py, with the helpers of tests/test_gpu_step_kernels.py.  The CSR is built in NumPy (appnp_reference.make_csr):
row lengths, values and empty rows are the test's choice.  Two kinds of input:
EXACT (signal = integers in [-8, 8] over 8, alpha = 0.5, val = +- 2^-ceil(log2 len): every fp32 partial result is exact up to K = 3
steps over rows of <= 64 entries, K = 2 over <= 512, K = 1 over any -- tests/test_appnp_reference_cpu.py) must come back bit for
bit; RANDOM (normal signal and values, alpha 0.1 / 0.15) is held per entry to the reference's propagated bound.  Every output buffer
is NaN before the launch and followed by guard elements; rows a launch must not touch must still be NaN; the last column of every
signal is a zero pad column and must come back exactly 0.  G = 64 / h4 throughout.

Launcher -> branch -> tests that reach it:

| launcher | branch (from the launch code and the kernel) | tests |
|---|---|---|
| fitgnn_gather_rows_padded_f32 | H = 1, 3, 4, 47, 48, 64 at h4 = ceil(H / 4) (the four `c + i < H` column guards) and H = 3 at h4 = 2 (a float4 of pad only); lds = H + 3 with NaN behind each row; index NULL / with repeats, out of order; n h4 on both sides of 256 | test_gather_rows_padded |
| | 4 h4 < H, lds < H refused; dst one float into its buffer -> FITGNN_E_ALIGN | test_gather_refusals |
| fitgnn_spmm_narrow_f32 | H = 1, 3, 47, 64, 65; n H on both sides of a multiple of 256; rows of 0, 1, 9, 300 entries; Z0 / ACC given or NULL, ACC pre-loaded | test_spmm_narrow_exact, test_spmm_narrow_random |
| fitgnn_spmm_narrow_padded_f32 | h4 = 1, 3, 12, 16 (G = 64, 21, 5, 4; at h4 = 3, 12 lanes of no slot); row lengths 0, 1, 7, 8 (own lanes only), 9, 8 + G - 1, 8 + G, 8 + G + 1, 8 + 2 G + 1, 300 (one slot, all but one, all, a second round for slot 0, three rounds, many); groups with no / one / several / G long rows; n % G != 0; columns anywhere; Z0 / ACC forms | test_step_exact, test_step_random |
| | n = 1 (rows of 0, 5, 300 entries) | test_step_one_row |
| | more than 16 384 groups (h4 = 16, n = 65 537): two groups per wave, the last wave one | test_step_many_groups |
| | h4 = 0, 17 refused; an unaligned pointer -> FITGNN_E_ALIGN | test_step_refusals |
| fitgnn_appnp_units_f32 | h4 = 1, 3, 12, 16 (capacity from fitgnn_appnp_unit_rows); units of 1, 2, cap - 1, cap rows; one unit of exactly fitgnn_appnp_unit_entries() entries; rows of 0, 1, 3, 4, 5, 8, 9 entries and a 300-entry centre (groups of four with 0 ... 3 padded); units out of order, rows of no unit stay NaN; K = 0 ... 3; forward / backward | test_units_exact |
| | max_rows = 7 (not a multiple of 4, far below the capacity) | test_units_small_launch |
| | K = 10 RANDOM; two launches, same bits | test_units_random |
| | max_rows above the capacity, max_entries 0 and 2 049 refused; unaligned -> FITGNN_E_ALIGN | test_units_refusals |
| fitgnn_appnp_blocks_f32 | ranges of 1, G - 1, G, G + 1, 16 G (one group per wave), 16 G + 1 (a second round for wave 0), 1 000 rows; the per-step row lengths; K = 1, 2, 3 (which scratch signal is read last; the backward's k == 0 and last branches together at K = 1); forward / backward; rows outside the blocks stay NaN in Y, T1, T2 | test_blocks_exact |
| | one block of 4 096 rows and exactly 16 384 entries: more than 64 KiB of LDS (hipFuncSetAttribute) | test_blocks_at_capacity |
| | K = 10 RANDOM == K launches of the per-step kernel bit for bit; two launches, same bits | test_blocks_random_equals_steps |
| | aliased X / Y / T1 / T2, K = 0, capacities exceeded refused | test_blocks_refusals |
| fitgnn_appnp_lds_f32 | (threads, slice) = (64, 1), (64, 4), (128, 2), (256, 4), (1024, 1), (1024, 4) x h4 = 1, 3, 7, 13, 16 (slice passes 1; 2 + 1; 4 + 2 + 1; 4 + 4 + 4 + 1; 4 x 4); short rows of 0 ... 6, 15, 16 entries (the hoisted four, the pair loop with odd and even tails); long rows of 17, 24, 32, 33, 40, 41, 300 (partial slots, one and two rounds of 32, many); n_long = 0, 1, W (8 / w), W (8 / w) + 1 (a second round over the long-row list); ranges of 1 row, of 4 threads / slice rows (four items per thread) and one row fewer; a range of empty rows; K = 0 ... 3; forward / backward; at 1 024 threads more than 64 KiB of LDS | test_lds_exact |
| | a range of empty rows only, max_entries = 0: alpha z_0 / alpha g_0 | test_lds_empty_rows |
| | a range beyond max_rows, one beyond max_entries: skipped (NaN kept), the others right | test_lds_skips_what_it_was_not_sized_for |
| | K = 7, 10 RANDOM; the same bits under every (threads, slice); two launches, same bits | test_lds_random_same_bits_for_every_launch |
| | ranges of short rows: the same bits as fitgnn_appnp_units_f32 | test_lds_equals_units_on_short_rows |
| ops.APPNPPropagate | C = 3, 47, K = 10, alpha = 0.1 on a GCN-normalised block-diagonal graph, forward and d / d z0, per route: default plan (units on the sliced kernel + lds_launches), appnp_sliced=False (whole-signal units + open rows), MIN_BLOCKS = 1 (blocks kernel), a 4 097-row block (open rows beside the LDS routes), appnp_in_lds=False, a RowIndex; each route asserted from the plan and cfg.profile | test_dispatcher_routes |

Bounds (u = 2^-24).  A kernel that rounds row r's sum k_r times per step is held to appnp_reference's propagated bound
b_{k+1} = beta |A| b_k + k_r u (beta |A| |z_k| + alpha |z_0|) (backward: k_r - 1 on g, one rounding per alpha-sum fma, one for the
final addition), first order in u (the second-order terms are below 300 u = 2e-5 of the bound).  k_r from each kernel's code, no
allowance on top:
* per-step and blocks kernels: a row of len <= 8 entries: len fused adds, the beta product, the teleport fma: len + 2.  A longer row:
  8 fused adds by its own lanes, ceil((len - 8) / G) per slot, G fold additions, one to join the two, then the same two:
  8 + ceil((len - 8) / G) + G + 3.
* units kernel: len fused adds in CSR order (the padded entries add exact zeros) + 2.
* lds kernel: a short row (<= 16 entries) len + 2; a long row ceil(len / 8) fused adds per slot, 3 tree levels, + 2.
* spmm_narrow_f32: len fused adds, the beta product, the Z0 fma when given; ACC: one fma, u (|ACC| + |delta X|).
* the dispatcher's gradient under a RowIndex: the segment sum of m rows adds (m - 1) u sum |terms| to the sum of their bounds.
Worst observed error / bound over all entries of one MI355X run (second figure: over the entries with k_r >= 8):
* spmm_narrow_f32: Y 0.81 (0.20); ACC 0.96 (a single rounding reaches u on its own).
* per-step kernel (one launch): Y 0.83 (0.48); ACC 1.00 (0.996: one rounding).
* units kernel, K = 10: forward 0.47 (0.11), backward 0.36 (0.17).
* blocks kernel, K = 10: forward 0.52 (0.15), backward 0.34 (0.087).
* lds kernel, K = 7 and 10: forward 0.47 (0.025), backward 0.26 (0.035).
* dispatcher, K = 10, worst over the six routes: forward 0.37 (0.070), gradient 0.25.
With the empty-row handling of appnp_lds_kernel as it was before this module (count 0 = "not this thread's item") 90 of the 277 tests
fail: all 30 test_lds_empty_rows cases, all 30 of test_lds_exact, and the tests whose ranges hold an empty row.
"""
import numpy as np
import pytest
import torch

import appnp_reference as ar
from test_gpu_step_kernels import (E_ALIGN, E_BADARG, L, U, _call, _dev, _exact, _np, _offset_copy, _p, _rng, _run,  # noqa: F401
                                   _same, _strided, _within)

pytestmark = pytest.mark.gpu

NAN = float("nan")
WORST = {}
H4S = [1, 3, 12, 16]


def _bounded(family, got, ref, bound, what, k=None):
    """_within, and the worst error / bound ratio of the family printed (run with -s) for the module docstring; with the roundings
    count k of every row, also the worst ratio over the entries whose path has at least 8 roundings."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"[ratio] {family}: {what}: {ratio:.3g} (family worst {WORST[family]:.3g})")
    if k is not None:
        long = pos & (np.broadcast_to(np.asarray(k).reshape(-1, 1), err.shape) >= 8)
        if long.any():
            r8 = float((err[long] / bound[long]).max())
            WORST[family + ", k >= 8"] = max(WORST.get(family + ", k >= 8", 0.0), r8)
            print(f"[ratio] {family}, k >= 8: {what}: {r8:.3g} (family worst {WORST[family + ', k >= 8']:.3g})")
    _within(got, ref, bound, what)


def _i32(a):
    return _dev(np.asarray(a), torch.int32)


def _guarded(shape, fill=NAN):
    """A contiguous device array followed by 4 guard elements, all holding `fill`."""
    n = int(np.prod(shape))
    buf = torch.full((n + 4,), fill, dtype=torch.float32, device="cuda")
    return buf, buf[:n].view(*shape)


def _guard_ok(*bufs):
    for b in bufs:
        assert torch.isnan(b[-4:]).all().item(), "wrote past the end of an output"


def _cycle(values, n, start=0):
    return np.array([values[(start + i) % len(values)] for i in range(n)], dtype=np.int64)


def _ranges(sizes):
    b = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.stack([b[:-1], b[1:]], 1)


class Pattern:
    """A CSR made by appnp_reference.make_csr, on the host and on the device (never an empty device array: a NULL col is refused)."""

    def __init__(self, rng, lengths, ranges=None, exact=False):
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.n = len(self.lengths)
        self.rowptr, self.col, self.val = ar.make_csr(rng, self.lengths, ranges, exact)
        pad = len(self.col) == 0
        self.dev = (_i32(self.rowptr), _i32([0] if pad else self.col), _dev(np.zeros(1, np.float32) if pad else self.val))

    def ptrs(self, L):
        return [_p(L, t) for t in self.dev]

    def entries(self, ranges):
        r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
        return self.rowptr[r[:, 1]].astype(np.int64) - self.rowptr[r[:, 0]]

    @property
    def csr(self):
        return self.rowptr, self.col, self.val


def _signal(rng, n, h4, exact):
    """[n, 4 h4] with a zero last column (a pad column)."""
    X = ar.exact_signal(rng, (n, 4 * h4)) if exact else rng.normal(size=(n, 4 * h4)).astype(np.float32)
    X[:, -1] = 0.0
    return X


def _mask(n, ranges):
    m = np.zeros(n, dtype=bool)
    for a, b in np.asarray(ranges).reshape(-1, 2):
        m[a:b] = True
    return m


def _check(got_t, ref, touched, what, bound=None, family=None, k=None):
    """Rows outside `touched` still NaN, rows inside: bit for bit (bound None) or within the bound; the pad column exactly 0."""
    got = _np(got_t)
    assert np.all(np.isnan(got[~touched])), f"{what}: a row outside the launch's ranges was written"
    assert not np.isnan(got[touched]).any(), f"{what}: a row of the launch's ranges was not written"
    assert np.all(got[touched][:, -1] == 0), f"{what}: the pad column is not exactly 0"
    if bound is None:
        _same(got[touched], ref[touched], what)
    else:
        _bounded(family, got[touched], ref[touched], bound[touched], what, None if k is None else k[touched])


# roundings of a row's path per step, from the kernels' code (see the module docstring)
def k_step(lens, G):
    lens = np.asarray(lens, dtype=np.int64)
    return np.where(lens <= 8, lens + 2, 8 + -(-(lens - 8) // G) + G + 3)


def k_units(lens):
    return np.asarray(lens, dtype=np.int64) + 2


def k_lds(lens):
    lens = np.asarray(lens, dtype=np.int64)
    return np.where(lens <= 16, lens + 2, -(-lens // 8) + 3 + 2)


def _reference(P, X, K, alpha, backward, k_r=None):
    return (ar.appnp_backward if backward else ar.appnp_forward)(*P.csr, X, K, alpha, k_r)


# ---------------------------------------------------------------------------------------------------------------------------------
# gather into the padded layout
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_index", [False, True], ids=["identity", "index"])
@pytest.mark.parametrize("H,h4", [(1, 1), (3, 1), (4, 1), (47, 12), (48, 12), (64, 16), (3, 2)], ids=lambda v: str(v))
def test_gather_rows_padded(L, H, h4, with_index):
    rng = _rng("gather", H, h4, with_index)
    for n in sorted({255 // h4, -(-256 // h4), 256 // h4 + 1}):
        n_src = n + 3 if with_index else n
        src = rng.normal(size=(n_src, H)).astype(np.float32)
        idx = None
        if with_index:
            idx = rng.integers(0, n_src, size=n)
            idx[:3] = [n_src - 1, 0, 0]                       # the last source row first, a repeat
        sd = _strided(src, H + 3)                             # NaN behind every row
        it = None if idx is None else _i32(idx)
        buf, dst = _guarded((n, 4 * h4))
        _run(L, "fitgnn_gather_rows_padded_f32", _p(L, sd), H + 3, H, _p(L, it), n, _p(L, dst), h4)
        _guard_ok(buf)
        _same(_np(dst), ar.gather_rows_padded(src, idx, h4), f"dst (n={n})")   # the pad columns: exactly 0, never NaN


def test_gather_refusals(L):
    src, dst = torch.zeros(8, 8, device="cuda"), torch.zeros(8, 8, device="cuda")
    Gt = lambda *a: _call(L, "fitgnn_gather_rows_padded_f32", *a)   # noqa: E731
    assert Gt(_p(L, src), 8, 5, None, 8, _p(L, dst), 2) == 0
    assert Gt(_p(L, src), 8, 5, None, 8, _p(L, dst), 1) == E_BADARG      # 4 h4 < H
    assert Gt(_p(L, src), 4, 5, None, 8, _p(L, dst), 2) == E_BADARG      # lds < H
    assert Gt(_p(L, src), 8, 5, None, 8, _p(L, _offset_copy(np.zeros((8, 8), np.float32), 1)), 2) == E_ALIGN
    assert Gt(None, 8, 5, None, 0, None, 2) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the unpadded narrow SpMM
# ---------------------------------------------------------------------------------------------------------------------------------
FORMS = {"neither": (False, False), "z0": (True, False), "acc": (False, True), "both": (True, True)}


def _narrow(L, fn, P, X, width_arg, beta, Z0, gamma, ACC, delta):
    """One launch of fitgnn_spmm_narrow_f32 (width_arg = H) or fitgnn_spmm_narrow_padded_f32 (h4): (rc, Y, ACC after)."""
    Xd = _dev(X)
    zd = None if Z0 is None else _dev(Z0)
    ybuf, Y = _guarded(X.shape)
    abuf = acc = None
    if ACC is not None:
        abuf, acc = _guarded(X.shape)
        acc.copy_(torch.from_numpy(ACC))
    rc = _call(L, fn, *P.ptrs(L), _p(L, Xd), _p(L, Y), P.n, width_arg, beta, _p(L, zd), gamma, _p(L, acc), delta)
    _guard_ok(ybuf, *([] if abuf is None else [abuf]))
    return rc, Y, acc


def _narrow_case(L, fn, P, width_arg, n_cols, form, exact, rng, family=None, k_sum=None):
    with_z0, with_acc = FORMS[form]
    mk = (lambda: ar.exact_signal(rng, (P.n, n_cols))) if exact else (lambda: rng.normal(size=(P.n, n_cols)).astype(np.float32))
    X, Z0, ACC = mk(), (mk() if with_z0 else None), (mk() if with_acc else None)
    beta, gamma, delta = (0.5, 0.5, 0.5) if exact else (ar.beta_of(0.1), ar.alpha_of(0.1), ar.alpha_of(0.15))
    rc, Y, acc = _narrow(L, fn, P, X, width_arg, beta, Z0, gamma, ACC, delta)
    L.check(rc, fn)
    ref = ar.spmm_affine(*P.csr, X, beta, Z0, gamma)
    got = _np(Y)
    assert not np.isnan(got).any(), "a row was not written"
    if exact:
        _same(got, ref, "Y")
        if with_acc:
            _same(_np(acc), ar.accumulate(ACC, delta, X), "ACC")
    else:
        k = k_sum + 1 + (1 if with_z0 else 0)
        cond = ar.spmm_affine(P.rowptr, P.col, np.abs(P.val), np.abs(X), beta, None if Z0 is None else np.abs(Z0), gamma)
        _bounded(family, got, ref, k[:, None] * U * cond, f"Y ({form})", k)
        if with_acc:
            _bounded(family + " ACC", _np(acc), ar.accumulate(ACC, delta, X), U * ar.accumulate(np.abs(ACC), delta, np.abs(X)), "ACC")
        rc, Y2, acc2 = _narrow(L, fn, P, X, width_arg, beta, Z0, gamma, ACC, delta)
        assert torch.equal(Y, Y2) and (acc is None or torch.equal(acc, acc2)), "two launches on the same input differ"


def _narrow_ns(H):
    m = 256
    while m // H < 4:
        m += 256
    return sorted({(m - 1) // H, -(-m // H), m // H + 1})


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("H", [1, 3, 47, 64, 65])
def test_spmm_narrow_exact(L, H, form):
    rng = _rng("narrow", H, form)
    for n in _narrow_ns(H):
        P = Pattern(rng, _cycle([300, 9, 1, 0], n), exact=True)
        _narrow_case(L, "fitgnn_spmm_narrow_f32", P, H, H, form, True, rng)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("H", [3, 65])
def test_spmm_narrow_random(L, H, form):
    rng = _rng("narrow_random", H, form)
    P = Pattern(rng, _cycle([300, 9, 1, 0], _narrow_ns(H)[-1]))
    _narrow_case(L, "fitgnn_spmm_narrow_f32", P, H, H, form, False, rng, "spmm_narrow", P.lengths)


# ---------------------------------------------------------------------------------------------------------------------------------
# the per-step kernel on the padded layout
# ---------------------------------------------------------------------------------------------------------------------------------
def _step_lengths(G, cap=None):
    """Groups of G rows with no long row, one, several, all G long, and a last partial group."""
    ln = ar.per_step_lengths(G)
    short, long = [v for v in ln if v <= 8], [v for v in ln if v > 8]
    none = _cycle(short, G)
    one = _cycle(short, G, 1)
    one[G // 2] = 300
    several = _cycle(short, G, 2)
    at = np.arange(0, G, max(G // len(long), 2))[:len(long)]
    several[at] = long[:len(at)]
    every = _cycle(long, G)
    tail = np.array([9, 0, 1][:min(3, G - 1)], dtype=np.int64)
    out = np.concatenate([none, one, several, every, tail])
    return out if cap is None else np.minimum(out, cap)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("h4", H4S)
def test_step_exact(L, h4, form):
    rng = _rng("step", h4, form)
    P = Pattern(rng, _step_lengths(64 // h4), exact=True)
    assert P.n % (64 // h4) != 0
    _narrow_case(L, "fitgnn_spmm_narrow_padded_f32", P, h4, 4 * h4, form, True, rng)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("h4", H4S)
def test_step_random(L, h4, form):
    rng = _rng("step_random", h4, form)
    G = 64 // h4
    P = Pattern(rng, _step_lengths(G))
    _narrow_case(L, "fitgnn_spmm_narrow_padded_f32", P, h4, 4 * h4, form, False, rng, "per-step", k_step(P.lengths, G) - 2)


@pytest.mark.parametrize("length", [0, 5, 300])
@pytest.mark.parametrize("h4", H4S)
def test_step_one_row(L, h4, length):
    rng = _rng("step_one", h4, length)
    _narrow_case(L, "fitgnn_spmm_narrow_padded_f32", Pattern(rng, [length], exact=True), h4, 4 * h4, "both", True, rng)


def test_step_many_groups(L):
    """h4 = 16: G = 4 rows per group; 65 537 rows = 16 385 groups, above the 16 384 waves of a launch: two groups per wave, 8 193 waves,
    the last one with a single group."""
    rng = _rng("step_many")
    n = 4 * 16384 + 1
    P = Pattern(rng, rng.integers(1, 4, size=n), exact=True)
    _narrow_case(L, "fitgnn_spmm_narrow_padded_f32", P, 16, 64, "z0", True, rng)


def test_step_refusals(L):
    rng = _rng("step_refusals")
    P = Pattern(rng, [1, 2, 3, 0], exact=True)
    X = _dev(np.zeros((4, 64), np.float32))
    Y = torch.zeros(4, 64, device="cuda")
    S = lambda x, y, h4: _call(L, "fitgnn_spmm_narrow_padded_f32", *P.ptrs(L), _p(L, x), _p(L, y), 4, h4, 0.5, None, 0.0, None, 0.0)   # noqa: E731
    assert S(X, Y, 16) == 0 and S(X, Y, 1) == 0
    assert S(X, Y, 0) == E_BADARG and S(X, Y, 17) == E_BADARG
    off = _offset_copy(np.zeros((4, 64), np.float32), 1)
    assert S(off, Y, 16) == E_ALIGN and S(X, off, 16) == E_ALIGN


# ---------------------------------------------------------------------------------------------------------------------------------
# the units kernel
# ---------------------------------------------------------------------------------------------------------------------------------
LIGHT = [0, 1, 3, 1, 0, 4, 1, 5, 0, 1, 8, 1, 0, 9, 1, 1]      # 35 entries per 16 rows: a unit of 768 rows stays below 2 048


def _fill_to(total, rows, first):
    """`rows` lengths that sum to `total`: `first`, then the rest spread evenly."""
    rest = total - first
    per, extra = divmod(rest, rows - 1)
    out = np.full(rows, per, dtype=np.int64)
    out[0] = first
    out[1:1 + extra] += 1
    assert out.sum() == total
    return out


def _run_ranged(L, fn, P, ranges, X, h4, K, alpha, backward, tail=(), max_rows=None, max_entries=None):
    """fitgnn_appnp_units_f32 (tail ()) or fitgnn_appnp_lds_f32 (tail (threads, slice)) on the listed ranges: (rc, Y)."""
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    rt = _i32(r.reshape(-1))
    mr = int((r[:, 1] - r[:, 0]).max()) if max_rows is None else max_rows
    me = int(P.entries(r).max()) if max_entries is None else max_entries
    Xd = _dev(X)
    buf, Y = _guarded(X.shape)
    rc = _call(L, fn, *P.ptrs(L), _p(L, rt), len(r), mr, me, _p(L, Xd), _p(L, Y), h4, K, alpha, backward, *tail)
    _guard_ok(buf)
    return rc, Y


def _unit_layout(L, h4, K):
    """(lengths, all ranges, the listed units out of order, the small units): gaps of rows that belong to no unit between them."""
    cap, cap_e = int(L.lib().fitgnn_appnp_unit_rows(h4)), int(L.lib().fitgnn_appnp_unit_entries())
    centre = int(ar.cap_lengths([300], K)[0])
    parts = [("gap", _cycle([2, 0, 7], 3)), ("one", np.array([3])), ("two", np.array([centre, 5])), ("cap-1", _cycle(LIGHT, cap - 1, 3)),
             ("gap", _cycle([1, 9, 0, 4, 2], 5)), ("cap", _cycle(LIGHT, cap)), ("entries", _fill_to(cap_e, min(cap, 40), centre)),
             ("seven", np.array([centre, 0, 1, 3, 4, 5, 9]))]
    rng_all = _ranges([len(p[1]) for p in parts])
    pick = lambda names: np.array([rng_all[i] for i, p in enumerate(parts) if p[0] in names])   # noqa: E731
    listed = pick(("one", "two", "cap-1", "cap", "entries", "seven"))[[3, 0, 5, 2, 1, 4]]
    return np.concatenate([p[1] for p in parts]), rng_all, listed, pick(("seven", "one", "two")), cap, cap_e


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("K", [0, 1, 2, 3], ids=lambda v: f"K{v}")
@pytest.mark.parametrize("h4", H4S)
def test_units_exact(L, h4, K, backward):
    rng = _rng("units", h4, K, backward)
    lengths, all_r, listed, _, cap, cap_e = _unit_layout(L, h4, K)
    P = Pattern(rng, lengths, all_r, exact=True)
    assert int((listed[:, 1] - listed[:, 0]).max()) == cap and int(P.entries(listed).max()) == cap_e
    X = _signal(rng, P.n, h4, True)
    rc, Y = _run_ranged(L, "fitgnn_appnp_units_f32", P, listed, X, h4, K, ar.EXACT_ALPHA, backward)
    L.check(rc, "fitgnn_appnp_units_f32")
    _check(Y, _reference(P, X, K, ar.EXACT_ALPHA, backward)[0], _mask(P.n, listed), "Y")


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("h4", H4S)
def test_units_small_launch(L, h4, backward):
    """max_rows = 7: the launch's LDS is sized for 8 rows, far below the capacity."""
    rng = _rng("units_small", h4, backward)
    lengths, all_r, _, small, _, _ = _unit_layout(L, h4, 2)
    P = Pattern(rng, lengths, all_r, exact=True)
    X = _signal(rng, P.n, h4, True)
    rc, Y = _run_ranged(L, "fitgnn_appnp_units_f32", P, small, X, h4, 2, ar.EXACT_ALPHA, backward)
    L.check(rc, "fitgnn_appnp_units_f32")
    assert int((small[:, 1] - small[:, 0]).max()) == 7
    _check(Y, _reference(P, X, 2, ar.EXACT_ALPHA, backward)[0], _mask(P.n, small), "Y")


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("h4,alpha", [(1, 0.1), (3, 0.15), (12, 0.1), (16, 0.15)], ids=lambda v: str(v))
def test_units_random(L, h4, alpha, backward):
    rng = _rng("units_random", h4, backward)
    lengths, all_r, listed, _, _, _ = _unit_layout(L, h4, 1)
    P = Pattern(rng, lengths, all_r)
    X = _signal(rng, P.n, h4, False)
    rc, Y = _run_ranged(L, "fitgnn_appnp_units_f32", P, listed, X, h4, 10, alpha, backward)
    L.check(rc, "fitgnn_appnp_units_f32")
    k = k_units(P.lengths)
    ref, bound = _reference(P, X, 10, alpha, backward, k)
    _check(Y, ref, _mask(P.n, listed), "Y", bound, "units " + ("backward" if backward else "forward"), k)
    rc, Y2 = _run_ranged(L, "fitgnn_appnp_units_f32", P, listed, X, h4, 10, alpha, backward)
    assert torch.equal(torch.nan_to_num(Y), torch.nan_to_num(Y2)), "two launches on the same input differ"


def test_units_refusals(L):
    rng = _rng("units_refusals")
    P = Pattern(rng, [1, 2, 3, 0], [[0, 4]], exact=True)
    X = _signal(rng, 4, 3, True)
    cap, cap_e = int(L.lib().fitgnn_appnp_unit_rows(3)), int(L.lib().fitgnn_appnp_unit_entries())
    assert (cap, cap_e) == (256, 2048) and [int(L.lib().fitgnn_appnp_unit_rows(h)) for h in (1, 12, 16, 17)] == [768, 64, 48, 0]
    run = lambda **kw: _run_ranged(L, "fitgnn_appnp_units_f32", P, [[0, 4]], X, 3, 2, 0.5, 0, **kw)[0]   # noqa: E731
    assert run() == 0 and run(max_rows=cap, max_entries=cap_e) == 0
    assert run(max_rows=cap + 1) == E_BADARG and run(max_entries=0) == E_BADARG and run(max_entries=cap_e + 1) == E_BADARG
    rt, Xo, Y = _i32([0, 4]), _offset_copy(X, 1), torch.zeros(4, 12, device="cuda")
    assert _call(L, "fitgnn_appnp_units_f32", *P.ptrs(L), _p(L, rt), 1, 4, 6, _p(L, Xo), _p(L, Y), 3, 2, 0.5, 0) == E_ALIGN


# ---------------------------------------------------------------------------------------------------------------------------------
# the blocks kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def _block_layout(h4, K):
    """Closed ranges of 1, G - 1, G, G + 1, 16 G, 16 G + 1 and 1 000 rows with gaps between them; the small ones cycle through the
    per-step row lengths, the large ones carry a long row every 16th row (a block holds at most 16 384 entries)."""
    G = 64 // h4
    ln = [int(v) for v in ar.cap_lengths(ar.per_step_lengths(G), K)]
    short, long = [v for v in ln if v <= 8], [v for v in ln if v > 8]
    parts, listed = [], []
    for i, size in enumerate([1, G - 1, G, G + 1, 16 * G, 16 * G + 1, 1000]):
        if size > 2 * G:
            rows = _cycle(short, size, i)
            at = np.arange(i % 16, size, 16)
            rows[at] = _cycle(long, len(at), i)
        else:
            rows = _cycle(ln[::-1], size, i)
        parts += [rows, _cycle([2, 0, 9], 1 + i % 3)]          # the block, then rows of no block
        listed.append(len(parts) - 2)
    all_r = _ranges([len(p) for p in parts])
    order = [4, 0, 6, 2, 1, 5, 3]
    return np.concatenate(parts), all_r, all_r[listed][order]


def _run_blocks(L, P, blocks, X, h4, K, alpha, backward, max_rows=None, max_entries=None):
    r = np.asarray(blocks, dtype=np.int64).reshape(-1, 2)
    rt = _i32(r.reshape(-1))
    mr = int((r[:, 1] - r[:, 0]).max()) if max_rows is None else max_rows
    me = int(P.entries(r).max()) if max_entries is None else max_entries
    Xd = _dev(X)
    bufs = [_guarded(X.shape) for _ in range(3)]
    (_, Y), (_, T1), (_, T2) = bufs
    rc = _call(L, "fitgnn_appnp_blocks_f32", *P.ptrs(L), _p(L, rt), len(r), mr, me, _p(L, Xd), _p(L, Y), _p(L, T1), _p(L, T2), h4, K, alpha,
               backward)
    _guard_ok(*[b[0] for b in bufs])
    return rc, Y, T1, T2


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("K", [1, 2, 3], ids=lambda v: f"K{v}")
@pytest.mark.parametrize("h4", H4S)
def test_blocks_exact(L, h4, K, backward):
    rng = _rng("blocks", h4, K, backward)
    lengths, all_r, listed = _block_layout(h4, K)
    P = Pattern(rng, lengths, all_r, exact=True)
    assert int(P.entries(listed).max()) <= int(L.lib().fitgnn_appnp_block_entries())
    X = _signal(rng, P.n, h4, True)
    rc, Y, T1, T2 = _run_blocks(L, P, listed, X, h4, K, ar.EXACT_ALPHA, backward)
    L.check(rc, "fitgnn_appnp_blocks_f32")
    inside = _mask(P.n, listed)
    _check(Y, _reference(P, X, K, ar.EXACT_ALPHA, backward)[0], inside, "Y")
    for T in (T1, T2):
        assert torch.isnan(T[torch.from_numpy(~inside).cuda()]).all().item(), "a scratch row outside the blocks was written"


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("h4", [3, 16])
def test_blocks_at_capacity(L, h4, backward):
    """One block of 4 096 rows and exactly 16 384 entries (its LDS need, (rows + 4) 4 + (entries + 4) 8 bytes, is above 64 KiB: the
    launcher raises the kernel's dynamic LDS limit first), a small one beside it."""
    rows, ents = int(L.lib().fitgnn_appnp_block_rows()), int(L.lib().fitgnn_appnp_block_entries())
    assert (rows, ents) == (4096, 16384) and (rows + 4) * 4 + (ents + 4) * 8 > 64 * 1024
    rng = _rng("blocks_cap", h4, backward)
    big = _cycle([1, 7, 3, 5, 0, 8, 4, 4], rows)
    big[:8] = [9, 23, 0, 0, 0, 0, 0, 0]                         # two rows beyond the own-lane entries, the same 32 entries per 8 rows
    lengths = np.concatenate([[3, 0], big, [2], [5, 1, 9]])
    all_r = _ranges([2, rows, 1, 3])
    listed = all_r[[3, 1]]
    P = Pattern(rng, lengths, all_r, exact=True)
    assert P.entries(listed).tolist() == [15, ents]
    X = _signal(rng, P.n, h4, True)
    rc, Y, _, _ = _run_blocks(L, P, listed, X, h4, 2, ar.EXACT_ALPHA, backward)
    L.check(rc, "fitgnn_appnp_blocks_f32")
    _check(Y, _reference(P, X, 2, ar.EXACT_ALPHA, backward)[0], _mask(P.n, listed), "Y")


def _steps(L, P, X, h4, K, alpha, backward):
    """K launches of the per-step kernel over every row, as ops.APPNPPropagate drives it."""
    a, b = ar.alpha_of(alpha), ar.beta_of(alpha)
    x0 = _dev(X)
    z = x0
    acc = torch.zeros_like(x0) if backward else None
    for _ in range(K):
        nxt = torch.empty_like(x0)
        if backward:
            _run(L, "fitgnn_spmm_narrow_padded_f32", *P.ptrs(L), _p(L, z), _p(L, nxt), P.n, h4, b, None, 0.0, _p(L, acc), a)
        else:
            _run(L, "fitgnn_spmm_narrow_padded_f32", *P.ptrs(L), _p(L, z), _p(L, nxt), P.n, h4, b, _p(L, x0), a, None, 0.0)
        z = nxt
    return acc + z if backward else z


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("h4,alpha", [(1, 0.1), (3, 0.15), (12, 0.1), (16, 0.15)], ids=lambda v: str(v))
def test_blocks_random_equals_steps(L, h4, alpha, backward):
    rng = _rng("blocks_random", h4, backward)
    lengths, all_r, listed = _block_layout(h4, 1)
    P = Pattern(rng, lengths, all_r)
    X = _signal(rng, P.n, h4, False)
    rc, Y, _, _ = _run_blocks(L, P, listed, X, h4, 10, alpha, backward)
    L.check(rc, "fitgnn_appnp_blocks_f32")
    k = k_step(P.lengths, 64 // h4)
    ref, bound = _reference(P, X, 10, alpha, backward, k)
    inside = _mask(P.n, listed)
    _check(Y, ref, inside, "Y", bound, "blocks " + ("backward" if backward else "forward"), k)
    rows = torch.from_numpy(inside).cuda()
    assert torch.equal(Y[rows], _steps(L, P, X, h4, 10, alpha, backward)[rows]), "the blocks kernel and K per-step launches differ in bits"
    rc, Y2, _, _ = _run_blocks(L, P, listed, X, h4, 10, alpha, backward)
    assert torch.equal(Y[rows], Y2[rows]), "two launches on the same input differ"


def test_blocks_refusals(L):
    rng = _rng("blocks_refusals")
    P = Pattern(rng, [1, 2, 3, 0], [[0, 4]], exact=True)
    rt = _i32([0, 4])
    X, Y, T1, T2 = (torch.zeros(4, 12, device="cuda") for _ in range(4))
    B = lambda x, y, t1, t2, K=2, mr=4, me=6: _call(L, "fitgnn_appnp_blocks_f32", *P.ptrs(L), _p(L, rt), 1, mr, me, _p(L, x), _p(L, y),   # noqa: E731
                                                    _p(L, t1), _p(L, t2), 3, K, 0.5, 0)
    assert B(X, Y, T1, T2) == 0
    for args in ((X, X, T1, T2), (X, Y, T1, T1), (X, Y, X, T2), (X, Y, T1, X), (X, Y, Y, T2), (X, Y, T1, Y)):
        assert B(*args) == E_BADARG, "aliased signals accepted"
    assert B(X, Y, T1, T2, K=0) == E_BADARG
    assert B(X, Y, T1, T2, mr=4097) == E_BADARG and B(X, Y, T1, T2, me=16385) == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the column-sliced LDS kernel
# ---------------------------------------------------------------------------------------------------------------------------------
LAUNCHES = [(64, 1), (64, 4), (128, 2), (256, 4), (1024, 1), (1024, 4)]
LDS_H4S = [1, 3, 7, 13, 16]
LONG_FEW = [17, 24, 32, 33, 40, 41]


def _pow2(v):
    return 1 << (int(v).bit_length() - 1)


def _lds_layout(threads, slice_, h4, K):
    """(lengths, ranges): one row; short rows only (n_long = 0); one long row; W (8 / w) long rows; one more (a second round over the
    long-row list); 4 threads / slice rows (four items per thread where w = slice) and one row fewer; empty rows only."""
    W, w0 = threads // 64, min(slice_, _pow2(h4))
    per_round = W * (8 // w0)
    n_max = 4 * threads // slice_
    centre = int(ar.cap_lengths([300], K)[0])
    short = ar.SHORT_LDS

    def with_long(n_long):
        rows = np.concatenate([_cycle(LONG_FEW, n_long), short])
        rows[0] = centre
        return np.roll(rows, 3)

    def full(n):
        rows = _cycle([0, 1, 2, 1], n)
        m = min(n, 2 * len(short))
        rows[:m] = _cycle(short, m)
        return rows

    parts = [np.array([5]), _cycle(short, 2 * len(short)), with_long(1), with_long(per_round), with_long(per_round + 1), full(n_max),
             full(n_max - 1), np.zeros(6, dtype=np.int64)]
    assert all(len(p) <= n_max for p in parts)
    return np.concatenate(parts), _ranges([len(p) for p in parts])


def _lds_fits(L, P, ranges, slice_):
    r = np.asarray(ranges).reshape(-1, 2)
    need = int(L.lib().fitgnn_appnp_lds_bytes(int((r[:, 1] - r[:, 0]).max()), int(P.entries(r).max()), slice_))
    assert 0 < need <= int(L.lib().fitgnn_appnp_lds_max_bytes()), need
    return need


@pytest.mark.parametrize("h4", LDS_H4S)
@pytest.mark.parametrize("threads,slice_", LAUNCHES, ids=lambda v: str(v))
def test_lds_exact(L, threads, slice_, h4):
    for K in (0, 1, 2, 3):
        rng = _rng("lds", threads, slice_, h4, K)
        lengths, ranges = _lds_layout(threads, slice_, h4, K)
        P = Pattern(rng, lengths, ranges, exact=True)
        need = _lds_fits(L, P, ranges, slice_)
        assert threads < 1024 or need > 64 * 1024              # the launcher raises the kernel's dynamic LDS limit
        X = _signal(rng, P.n, h4, True)
        for backward in (0, 1):
            rc, Y = _run_ranged(L, "fitgnn_appnp_lds_f32", P, ranges, X, h4, K, ar.EXACT_ALPHA, backward, (threads, slice_))
            L.check(rc, "fitgnn_appnp_lds_f32")
            _check(Y, _reference(P, X, K, ar.EXACT_ALPHA, backward)[0], np.ones(P.n, dtype=bool), f"Y (K={K}, backward={backward})")


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("K", [1, 2, 3], ids=lambda v: f"K{v}")
@pytest.mark.parametrize("threads,slice_,h4", [(64, 1, 1), (64, 4, 3), (128, 2, 7), (256, 4, 13), (1024, 4, 16)], ids=lambda v: str(v))
def test_lds_empty_rows(L, threads, slice_, h4, K, backward):
    """Ranges whose rows have no entries, in a launch sized with max_entries = 0: alpha z_0 forward, alpha g_0 backward -- the units,
    blocks and per-step kernels' result for such rows."""
    rng = _rng("lds_empty", threads, slice_, h4, K, backward)
    lengths = np.array([0, 0, 0, 0, 0, 4, 2, 0, 0, 0], dtype=np.int64)
    ranges = np.array([[0, 5], [7, 10]])
    P = Pattern(rng, lengths, [[0, 5], [5, 7], [7, 10]], exact=True)
    X = _signal(rng, P.n, h4, True)
    X[X == 0] = 0.5
    X[:, -1] = 0.0
    rc, Y = _run_ranged(L, "fitgnn_appnp_lds_f32", P, ranges, X, h4, K, ar.EXACT_ALPHA, backward, (threads, slice_), max_entries=0)
    L.check(rc, "fitgnn_appnp_lds_f32")
    ref = _reference(P, X, K, ar.EXACT_ALPHA, backward)[0]
    touched = _mask(P.n, ranges)
    assert np.array_equal(ref[touched], 0.5 * X[touched].astype(np.float64))
    _check(Y, ref, touched, "Y")
    ref_u = _run_ranged(L, "fitgnn_appnp_units_f32", P, [[0, 5], [7, 10]], X, h4, K, ar.EXACT_ALPHA, backward, max_entries=1)[1]
    assert torch.equal(torch.nan_to_num(Y), torch.nan_to_num(ref_u)), "the units kernel gives another result for rows without entries"


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
def test_lds_skips_what_it_was_not_sized_for(L, backward):
    rng = _rng("lds_skip", backward)
    parts = [_cycle(ar.SHORT_LDS, 5), _cycle(ar.SHORT_LDS, 20, 2), np.array([300, 1, 2, 0, 3, 1]), _cycle(ar.SHORT_LDS, 7, 4)]
    ranges = _ranges([len(p) for p in parts])
    P = Pattern(rng, np.concatenate(parts), ranges, exact=True)
    X = _signal(rng, P.n, 3, True)
    me = int(P.entries(ranges[[0, 3]]).max())
    assert me < P.entries(ranges)[2]                              # range 1 has too many rows, range 2 (6 rows) too many entries
    rc, Y = _run_ranged(L, "fitgnn_appnp_lds_f32", P, ranges, X, 3, 2, ar.EXACT_ALPHA, backward, (64, 4), max_rows=7, max_entries=me)
    L.check(rc, "fitgnn_appnp_lds_f32")
    _check(Y, _reference(P, X, 2, ar.EXACT_ALPHA, backward)[0], _mask(P.n, ranges[[0, 3]]), "Y")


def _lds_random_layout():
    """Ranges that fit every launch of LAUNCHES (<= 64 rows): twelve long rows among short ones (a second round over the long-row
    list at 64 threads for every slice width), one row, short rows only, empty rows only."""
    mixed = np.concatenate([_cycle(ar.LONG_LDS, 12), _cycle(ar.SHORT_LDS, 52)])
    parts = [np.roll(mixed, 5), np.array([3]), _cycle(ar.SHORT_LDS, 30, 1), np.zeros(4, dtype=np.int64)]
    return np.concatenate(parts), _ranges([len(p) for p in parts])


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("K,alpha", [(7, 0.15), (10, 0.1)], ids=lambda v: str(v))
@pytest.mark.parametrize("h4", LDS_H4S)
def test_lds_random_same_bits_for_every_launch(L, h4, K, alpha, backward):
    rng = _rng("lds_random", h4, K, backward)
    lengths, ranges = _lds_random_layout()
    P = Pattern(rng, lengths, ranges)
    X = _signal(rng, P.n, h4, False)
    k = k_lds(P.lengths)
    ref, bound = _reference(P, X, K, alpha, backward, k)
    first = None
    for threads, slice_ in LAUNCHES:
        _lds_fits(L, P, ranges, slice_)
        rc, Y = _run_ranged(L, "fitgnn_appnp_lds_f32", P, ranges, X, h4, K, alpha, backward, (threads, slice_))
        L.check(rc, "fitgnn_appnp_lds_f32")
        if first is None:
            first = Y
            _check(Y, ref, np.ones(P.n, dtype=bool), "Y", bound, "lds " + ("backward" if backward else "forward"), k)
            rc, Y2 = _run_ranged(L, "fitgnn_appnp_lds_f32", P, ranges, X, h4, K, alpha, backward, (threads, slice_))
            assert torch.equal(Y, Y2), "two launches on the same input differ"
        else:
            assert torch.equal(first, Y), f"the result depends on the launch: {LAUNCHES[0]} vs {(threads, slice_)}"


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("h4", [1, 3, 7, 16])
def test_lds_equals_units_on_short_rows(L, h4, backward):
    """Rows of at most 16 entries: both kernels sum in CSR order from zero and apply the same beta product and teleport fma."""
    rng = _rng("lds_units", h4, backward)
    cap = min(int(L.lib().fitgnn_appnp_unit_rows(h4)), 100)
    parts = [_cycle(ar.SHORT_LDS, cap), np.array([16]), _cycle(ar.SHORT_LDS, 37, 5), np.zeros(3, dtype=np.int64)]
    ranges = _ranges([len(p) for p in parts])
    P = Pattern(rng, np.concatenate(parts), ranges)
    X = _signal(rng, P.n, h4, False)
    rc, Yu = _run_ranged(L, "fitgnn_appnp_units_f32", P, ranges, X, h4, 10, 0.1, backward)
    L.check(rc, "fitgnn_appnp_units_f32")
    rc, Yl = _run_ranged(L, "fitgnn_appnp_lds_f32", P, ranges, X, h4, 10, 0.1, backward, (256, 4))
    L.check(rc, "fitgnn_appnp_lds_f32")
    assert not torch.isnan(Yu).any().item() and torch.equal(Yu, Yl), "the sliced kernel and the units kernel differ in bits"


# ---------------------------------------------------------------------------------------------------------------------------------
# the dispatcher
# ---------------------------------------------------------------------------------------------------------------------------------
def _gcn_blocks(sizes, rng, hub_every=3):
    """Block-diagonal symmetric pattern: every block a ring plus chords, every hub_every-th node also tied to the block's first."""
    src, dst, off = [], [], 0
    for sz in sizes:
        sz = int(sz)
        ring = np.arange(sz)
        und = {(min(a, b), max(a, b)) for a, b in zip(ring, np.roll(ring, -1)) if a != b}
        for _ in range(sz // 2):
            a, b = rng.integers(0, sz, size=2)
            if a != b:
                und.add((int(min(a, b)), int(max(a, b))))
        und |= {(0, int(j)) for j in range(hub_every, sz, hub_every)}
        if und:
            u = np.array(sorted(und), dtype=np.int64) + off
            src += [u[:, 0], u[:, 1]]
            dst += [u[:, 1], u[:, 0]]
        off += sz
    return torch.from_numpy(np.stack([np.concatenate(src), np.concatenate(dst)])).cuda(), off


def _route_k(plan, lens, h4):
    """The roundings count of every row under the plan's routing."""
    k = k_step(lens, 64 // h4)                                  # open rows, the blocks kernel, no plan at all
    if plan is None:
        return k
    listed = [(plan.units.cpu().numpy(), k_lds if plan.sliced else k_units)] if plan.n_units else []
    listed += [(la[1].cpu().numpy(), k_lds) for la in plan.lds_launches]
    for ranges, fn in listed:
        for a, b in ranges:
            k[a:b] = fn(lens[a:b])
    return k


ROUTES = ["default", "whole", "blocks", "open4097", "steps", "row_index"]


@pytest.mark.parametrize("C", [3, 47])
@pytest.mark.parametrize("route", ROUTES)
def test_dispatcher_routes(L, monkeypatch, route, C):
    from fitgnn_amd import csr, ops

    K, alpha = 10, 0.1
    h4 = (C + 3) // 4
    cap = int(L.lib().fitgnn_appnp_unit_rows(h4))
    rng = _rng("dispatcher", route, C)
    sizes = [5] * 6 + [3, 40, 1, 2, cap + 6, cap + 40] + ([4097] if route == "open4097" else [])
    if route == "blocks":
        monkeypatch.setattr(ops.AppnpPlan, "MIN_BLOCKS", 1)
    ei, n = _gcn_blocks(sizes, rng)
    g = csr.CSRGraph(ei, n, mode="gcn")
    cfg = {"whole": ops.DEFAULT.replace(appnp_sliced=False), "blocks": ops.DEFAULT.replace(appnp_sliced=False),
           "steps": ops.DEFAULT.replace(appnp_in_lds=False)}.get(route, ops.DEFAULT).replace(profile=[])
    ri = idx = None
    n_in = n
    if route == "row_index":
        n_in = n // 2
        idx = rng.integers(0, n_in, size=n)
        ri = ops.RowIndex(torch.from_numpy(idx).cuda(), n_in)
    z_in = rng.normal(size=(n_in, C)).astype(np.float32)
    w = rng.normal(size=(n, C)).astype(np.float32)
    zz = _dev(z_in).requires_grad_(True)
    out = ops.APPNPPropagate.apply(zz, g, K, alpha, cfg, ri)
    (out * _dev(w)).sum().backward()
    torch.cuda.synchronize()
    kinds = [e[2] for e in cfg.profile]
    plan = ops.appnp_plan(g, h4, cfg.appnp_blocks, cfg.appnp_sliced) if cfg.appnp_in_lds else None
    # the route ran
    if route in ("default", "row_index"):
        assert plan.sliced and plan.n_units > 0 and len(plan.lds_launches) > 0 and plan.n_open == 0 and plan.n_blocks == 0
        assert set(kinds) == {"appnp_units", "appnp_lds_blocks", "appnp_units_t", "appnp_lds_blocks_t"}
    elif route == "whole":
        assert not plan.sliced and plan.n_units > 0 and plan.n_open == 2 * cap + 46 and plan.n_blocks == 0 and not plan.lds_launches
        assert set(kinds) == {"appnp_units", "appnp_step", "appnp_units_t", "appnp_step_t"} and kinds.count("appnp_step") == K
    elif route == "blocks":
        assert not plan.sliced and plan.n_units > 0 and plan.n_blocks == 2 and plan.n_open == 0
        assert set(kinds) == {"appnp_units", "appnp_blocks", "appnp_units_t", "appnp_blocks_t"}
    elif route == "open4097":
        assert plan.n_open == 4097 and plan.n_units > 0 and len(plan.lds_launches) > 0
        assert set(kinds) == {"appnp_units", "appnp_lds_blocks", "appnp_step", "appnp_units_t", "appnp_lds_blocks_t", "appnp_step_t"}
    else:
        assert plan is None and kinds.count("appnp_step") == K and kinds.count("appnp_step_t") == K and len(kinds) == 2 * K
    # the values
    f = tuple(t.cpu().numpy() for t in (g.f.rowptr, g.f.col, g.f.val))
    t = tuple(t.cpu().numpy() for t in (g.t.rowptr, g.t.col, g.t.val))
    kf, kt = _route_k(plan, np.diff(f[0]), h4), _route_k(plan, np.diff(t[0]), h4)
    z0 = z_in if idx is None else z_in[idx]
    ref, bound = ar.appnp_forward(*f, z0, K, alpha, kf)
    assert out.shape == (n, C)
    _bounded(f"dispatcher forward ({route})", _np(out), ref, bound, "z_K", kf)
    back, bbound = ar.appnp_backward(*t, w, K, alpha, kt)
    if idx is not None:                                         # the adjoint of the gather: a segment sum of m rows, m - 1 roundings
        m = np.bincount(idx, minlength=n_in)[:, None]
        seg = lambda a: np.stack([np.bincount(idx, weights=a[:, c], minlength=n_in) for c in range(C)], 1)   # noqa: E731
        back, bbound = seg(back), seg(bbound) + np.maximum(m - 1, 0) * U * seg(np.abs(back))
    assert zz.grad.shape == (n_in, C)
    _bounded(f"dispatcher gradient ({route})", _np(zz.grad), back, bbound, "d z0")
