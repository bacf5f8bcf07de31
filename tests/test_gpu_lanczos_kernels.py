"""GPU tier: the Lanczos-step kernels of csrc/lanczos.hip through the C ABI against the np.longdouble references of
tests/lanczos_reference.py.  All operands are float64.  EXACT inputs (integers over 8: every product and sum is exact in double) must
come back bit for bit whatever the summation order; RANDOM inputs are held to k * 2^-53 * (sum of |terms| of that entry), k the number
of roundings on that entry's path, counted without relying on the compiler fusing a multiply with its add.

Launcher -> branch -> tests that reach it:

| launcher | branch (from the launch code and the kernel) | tests |
|---|---|---|
| fitgnn_lanczos_spmv_f64 | 8 lanes per row, 32 rows per workgroup: n = 1, 31, 32, 33 (a second workgroup with one live row), 1000; row lengths 0 (no trip), 1, 7 (one lane idle), 8, 9 (a second trip on lane 0), 51, 600 in one matrix; unsorted columns with repeats; alpha, beta general and the solver's (-1, 2 max dw) | test_spmv_exact, test_spmv_random |
| | n = 0 returns 0, n < 0 / NULL refused | test_refusals |
| fitgnn_lanczos_project_f64 | 512 rows per workgroup, two per thread: n = 1, 256 (first row of every thread only), 257, 511, 512 (one full workgroup), 513 (a second one with one row), 1025 (three); ncol = 1, 2, 60, 128; ldv > n over NaN; h_in NULL (w untouched, bit for bit) / given (w updated in place, the dots are the updated w's, the last column |w|^2); partial layout [fitgnn_lanczos_parts(n)][ncol + 1] | test_project_exact, test_project_random |
| | ncol = 0, 129, ldv < n refused | test_refusals |
| fitgnn_lanczos_reduce_f64 | four interleaved sums: n_part = 0 (zeros), 1, 3 (some sums empty), 4, 5, 323; 64 columns per round: ncol1 = 1, 64, 65 (a second round with one live column), 129 (a third) | test_reduce_exact, test_reduce_random |
| | ncol1 = 0, 130 refused | test_refusals |
| fitgnn_lanczos_finish_f64 | j = 0, 1, 127 (the H column written by workgroup 0's first j + 1 threads); n = 1, 255, 257 (one workgroup partial, a second with one row) and n = 262 444 > 1024 x 256: the grid is capped at 1024 workgroups and the first 300 threads make a second trip; ldh > j + 1, ldv > n; only column j of H and vector j + 1 of V are written | test_finish_exact, test_finish_random |
| | breakdown (w = 0, |w|^2 = 0): a zero vector and beta = 0, not NaN | test_finish_breakdown |
| | j = 128, ldh < j + 1, ldv < n refused | test_refusals |
| fitgnn_lanczos_rotate_f64 | m = 1, 60, 128 (S staged through LDS: m nk up to 2048 in 256-thread strides); nk = 1, 10, 16; n = 1, 255, 256, 257; ldv > n, ldo > n; out two whole columns into its buffer (the solver's second group of sixteen) | test_rotate_exact, test_rotate_random |
| | nk = 17, m = 129, ldo < n refused | test_refusals |
| one whole step | spmv, three project + reduce passes, finish for j = 0 ... 5 on a 700-node Laplacian, each step against the reference run on the same basis | test_composed_steps |
| all fixed-order sums | two launches on RANDOM inputs give the same bits | the *_random tests |

Bounds that are not bit-exact (u = 2^-53, cond = the same operation on |inputs|), with the worst observed error / bound over all
entries of one MI355X run in brackets:
* spmv: a row of len entries gives each of 8 lanes ceil(len / 8) products and as many additions less one, three shuffle additions
  follow, then alpha s, beta x and their sum: k = 2 ceil(len / 8) + 5, |err| <= k u (|alpha| sum |val x| + |beta x|).  [0.28]
* project, w: sum_c V[c][i] h[c] is ncol products and ncol - 1 additions in one running sum, then one subtraction:
  |err| <= 2 ncol u (|w| + sum_c |V h|).  [0.40]
  Partial dots (of the w the kernel itself stored): two products and one addition per thread, six butterfly levels, three additions
  over the four waves: k = 12.  [0.16]
* reduce: each of the four running sums takes ceil(n_part / 4) rows (one rounding less), three additions combine them:
  k = ceil(n_part / 4) + 2.  [0.36]
* finish: beta = sqrt, correctly rounded by the device library: u |beta| (the reference rounds the same real number, so the
  observed error is 0; an answer one ulp off would miss this bound).  v = w * (1 / beta): beta's u, the reciprocal's u, the
  product's u: 3u |v|.  [beta 0, v 0.67]
* rotate: m products and m - 1 additions in one running sum: (2m - 1) u cond.  [0.021: the compiler fuses each product with its
  addition, which halves the roundings]
* composed step, H[c][j] = ha[c] + hb[c] against the reference step on the same basis: the spmv's and the first pass's elementwise
  errors of w carried through |V[c]|, 15 u (cond of the first dot + cond of the second) for the two dots (12 in the partial, at most 3
  in the two-row reduce), u |H| for the sum; the (V V^T - I) ha term is common to both sides.  H[j + 1][j] = beta: the 2-norm of all
  three passes' elementwise errors of w and of the second dots' errors, plus (15 / 2 + 2) u beta.  [H 0.027, beta 0.011; these
  bounds add worst cases over 700 rows, the errors themselves add like a random walk.  max |V V^T - I| = 2.5 u of the 64 u allowed]
"""
import numpy as np
import pytest
import torch

import lanczos_reference as lr
from test_gpu_step_kernels import E_BADARG, L, _call, _p, _rng, _run, _same, _within  # noqa: F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NAN = float("nan")
WORST = {}
LD = np.longdouble


def _bounded(family, got, ref, bound, what):
    """_within, and the worst error / bound ratio of the family printed (run with -s) for the module docstring."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"[ratio] {family}: {what}: {ratio:.3g} (family worst {WORST[family]:.3g})")
    _within(got, ref, bound, what)


def _d64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _ints(rng, shape, lo=-8, hi=8, den=8.0):
    return rng.integers(lo, hi + 1, size=shape) / den


def _cols(A, ld, lead=0, fill=NAN):
    """A [ncol x n] as a device view with column stride ld, `lead` whole columns into a buffer whose every other element holds
    `fill`.  Returns (buffer viewed as [lead + ncol, ld], the view)."""
    A = np.asarray(A, dtype=np.float64)
    ncol, n = A.shape
    buf = torch.full(((lead + ncol) * ld + 4,), fill, dtype=torch.float64, device="cuda")
    full = buf[:(lead + ncol) * ld].view(lead + ncol, ld)
    v = full[lead:, :n]
    v.copy_(torch.from_numpy(A))
    return full, v


def _guarded(shape, fill=NAN):
    n = int(np.prod(shape))
    buf = torch.full((n + 4,), fill, dtype=torch.float64, device="cuda")
    return buf, buf[:n].view(*shape)


def _np(t):
    return t.detach().cpu().numpy()


def _bits_equal(a, b, what):
    assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), f"{what}: differs"


# ---------------------------------------------------------------------------------------------------------------------------------
# the sparse product
# ---------------------------------------------------------------------------------------------------------------------------------
ROW_LENGTHS = [600, 51, 9, 8, 7, 1, 0]


def _csr(rng, n, exact):
    lens = np.array([ROW_LENGTHS[i % len(ROW_LENGTHS)] for i in range(n)])
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    col = rng.integers(0, n, size=rowptr[-1])      # unsorted, with repeats
    val = _ints(rng, rowptr[-1]) if exact else rng.normal(size=rowptr[-1])
    x = _ints(rng, n) if exact else rng.normal(size=n)
    return lens, rowptr, col, val, x


def _spmv(L, rowptr, col, val, x, alpha, beta):
    n = len(x)
    rp, ci, vd, xd = _i32(rowptr), _i32(col), _d64(val), _d64(x)
    buf, y = _guarded((n,))
    _run(L, "fitgnn_lanczos_spmv_f64", _p(L, rp), _p(L, ci), _p(L, vd), _p(L, xd), _p(L, y), n, alpha, beta)
    assert torch.isnan(buf[-4:]).all().item(), "wrote past the end of y"
    return y


@pytest.mark.parametrize("alpha,beta", [(-1.5, 0.75), (-1.0, 2.0 * 8.0)], ids=["general", "solver"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_spmv_exact(L, n, alpha, beta):
    lens, rowptr, col, val, x = _csr(_rng("spmv", n), n, True)
    y = _spmv(L, rowptr, col, val, x, alpha, beta)
    _same(_np(y), lr.spmv(rowptr, col, val, x, alpha, beta), "y")


@pytest.mark.parametrize("n", [33, 1000])
def test_spmv_random(L, n):
    lens, rowptr, col, val, x = _csr(_rng("spmv_random", n), n, False)
    alpha, beta = -1.0, 2.0 * 7.3
    y = _spmv(L, rowptr, col, val, x, alpha, beta)
    k = 2 * -(-lens // 8) + 5
    cond = lr.spmv(rowptr, col, np.abs(val), np.abs(x), abs(alpha), abs(beta))
    _bounded("spmv", _np(y), lr.spmv(rowptr, col, val, x, alpha, beta), k * U * cond, "y")
    _bits_equal(_np(_spmv(L, rowptr, col, val, x, alpha, beta)), _np(y), "two launches")


# ---------------------------------------------------------------------------------------------------------------------------------
# projection pass
# ---------------------------------------------------------------------------------------------------------------------------------
def _project(L, V, ldv, w, h_in):
    """Launch one pass; returns (w after the pass, partial rows [parts x (ncol + 1)], the V view for the padding check)."""
    ncol, n = V.shape
    Vfull, Vd = _cols(V, ldv)
    wbuf, wd = _guarded((n,))
    wd.copy_(torch.from_numpy(np.asarray(w, dtype=np.float64)))
    hd = None if h_in is None else _d64(h_in)
    parts = int(L.lib().fitgnn_lanczos_parts(n))
    assert parts == -(-n // 512)
    pbuf, part = _guarded((parts, ncol + 1))
    _run(L, "fitgnn_lanczos_project_f64", _p(L, Vfull), ldv, ncol, _p(L, wd), n, _p(L, hd), _p(L, part))
    assert torch.isnan(wbuf[-4:]).all().item() and torch.isnan(pbuf[-4:]).all().item(), "wrote past the end of w / the partial rows"
    assert torch.isnan(Vfull[:, n:]).all().item() and torch.equal(Vd.cpu(), torch.from_numpy(np.asarray(V, dtype=np.float64))), "V changed"
    return _np(wd), _np(part)


def _partial_refs(V, w):
    """The reference partial rows of the w the kernel left: workgroup b's dots over rows [512 b, 512 (b + 1)), and their conditions."""
    n = len(w)
    rows, conds = [], []
    for r0 in range(0, n, 512):
        h, nrm2, cond = lr.dots(V[:, r0:r0 + 512], w[r0:r0 + 512])
        rows.append(np.concatenate([h, [nrm2]]))
        conds.append(np.concatenate([cond, [nrm2]]))
    return np.array(rows), np.array(conds)


@pytest.mark.parametrize("ncol", [1, 2, 60, 128])
@pytest.mark.parametrize("n", [1, 256, 257, 511, 512, 513, 1025])
def test_project_exact(L, n, ncol):
    rng = _rng("project", n, ncol)
    V, w, h = _ints(rng, (ncol, n)), _ints(rng, n), _ints(rng, ncol)
    w0, part0 = _project(L, V, n + 3, w, None)
    _bits_equal(w0, w, "h_in NULL: w")
    _same(part0, _partial_refs(V, w)[0], "h_in NULL: partial rows")
    w1, part1 = _project(L, V, n + 3, w, h)
    rw, rh, rn = lr.project(V, w, h)
    _same(w1, rw, "w")
    _same(part1, _partial_refs(V, rw)[0], "partial rows of the updated w")
    _same(part1.sum(0), np.concatenate([rh, [rn]]), "the partial rows add up to the dots of the updated w")


@pytest.mark.parametrize("n,ncol", [(513, 60), (1025, 128), (257, 2)])
def test_project_random(L, n, ncol):
    rng = _rng("project_random", n, ncol)
    V, w, h = rng.normal(size=(ncol, n)) / np.sqrt(n), rng.normal(size=n), rng.normal(size=ncol)
    w1, part1 = _project(L, V, n + 5, w, h)
    rw, _, _ = lr.project(V, w, h)
    _bounded("project w", w1, rw, 2 * ncol * U * (np.abs(w) + lr.project_cond(V, h)), "w")
    ref, cond = _partial_refs(V, w1)               # the dots are those of the w the kernel stored
    _bounded("project dots", part1, ref, 12 * U * cond, "partial rows")
    w2, part2 = _project(L, V, n + 5, w, h)
    _bits_equal(w2, w1, "two launches: w")
    _bits_equal(part2, part1, "two launches: partial rows")


# ---------------------------------------------------------------------------------------------------------------------------------
# reduce
# ---------------------------------------------------------------------------------------------------------------------------------
def _reduce(L, part):
    n_part, ncol1 = part.shape
    pd = _d64(part if n_part else np.zeros((1, ncol1)))
    buf, out = _guarded((ncol1,))
    _run(L, "fitgnn_lanczos_reduce_f64", _p(L, pd), n_part, ncol1, _p(L, out))
    assert torch.isnan(buf[-4:]).all().item(), "wrote past the end of out"
    return _np(out)


@pytest.mark.parametrize("ncol1", [1, 64, 65, 129])
@pytest.mark.parametrize("n_part", [0, 1, 3, 4, 5, 323])
def test_reduce_exact(L, n_part, ncol1):
    part = _ints(_rng("reduce", n_part, ncol1), (n_part, ncol1))
    _same(_reduce(L, part), lr.reduce_parts(part), "out")


@pytest.mark.parametrize("n_part,ncol1", [(5, 65), (323, 129)])
def test_reduce_random(L, n_part, ncol1):
    part = _rng("reduce_random", n_part, ncol1).normal(size=(n_part, ncol1))
    out = _reduce(L, part)
    _bounded("reduce", out, lr.reduce_parts(part), (-(-n_part // 4) + 2) * U * lr.reduce_parts(np.abs(part)), "out")
    _bits_equal(_reduce(L, part), out, "two launches")


# ---------------------------------------------------------------------------------------------------------------------------------
# finish
# ---------------------------------------------------------------------------------------------------------------------------------
def _finish(L, Vprev, j, w, ha, hb, nrm2):
    """Launch on a basis holding the vectors 0 ... j (Vprev) with NaN in place of vector j + 1.  Returns (v_next, H as [j + 2, ldh])
    after checking that nothing but vector j + 1 and column j of H was written."""
    n = len(w)
    ldv, ldh = n + 3, j + 4
    Vin = np.concatenate([Vprev, np.full((1, n), NAN)])
    Vfull, Vd = _cols(Vin, ldv)
    hc = np.full(j + 2, NAN); hc[j + 1] = nrm2
    wd, had, hbd, hcd = _d64(w), _d64(ha), _d64(hb), _d64(hc)
    hbuf, H = _guarded((j + 2, ldh))
    _run(L, "fitgnn_lanczos_finish_f64", _p(L, Vfull), ldv, j, _p(L, wd), n, _p(L, had), _p(L, hbd), _p(L, hcd), _p(L, H), ldh)
    assert torch.isnan(hbuf[-4:]).all().item() and torch.isnan(Vfull[:, n:]).all().item(), "wrote into the padding of H / V"
    assert torch.equal(Vd[:j + 1].cpu(), torch.from_numpy(Vprev)), "an earlier basis vector changed"
    Hn = _np(H)
    other = np.ones(Hn.shape, dtype=bool); other[:, j] = False
    assert np.all(np.isnan(Hn[other])), "wrote outside column j of H"
    return _np(Vd[j + 1]), Hn[:, j]


FINISH_SHAPES = [(j, n) for j in (0, 1, 127) for n in (1, 255, 257)] + [(1, 1024 * 256 + 300)]


@pytest.mark.parametrize("j,n", FINISH_SHAPES, ids=lambda v: str(v))
def test_finish_exact(L, j, n):
    rng = _rng("finish", j, n)
    Vprev, w = _ints(rng, (j + 1, n)), _ints(rng, n)
    ha, hb = rng.normal(size=j + 2), rng.normal(size=j + 2) * 1e-9
    v, colH = _finish(L, Vprev, j, w, ha, hb, 4.0)       # beta = 2, 1 / beta = 0.5: v = w / 2 exactly
    rv, rcol, beta = lr.finish(w, ha, hb, 4.0, j)
    assert beta == 2.0
    _same(v, rv, "v_next")
    _same(colH, rcol, "H[:, j]")
    _same(colH[:j + 1], ha[:j + 1] + hb[:j + 1], "H[c][j] = ha[c] + hb[c]")


@pytest.mark.parametrize("j,n", [(0, 257), (127, 255), (1, 1024 * 256 + 300)], ids=lambda v: str(v))
def test_finish_random(L, j, n):
    rng = _rng("finish_random", j, n)
    Vprev, w = rng.normal(size=(j + 1, n)), rng.normal(size=n)
    ha, hb = rng.normal(size=j + 2), rng.normal(size=j + 2)
    nrm2 = float(w @ w)
    v, colH = _finish(L, Vprev, j, w, ha, hb, nrm2)
    rv, rcol, beta = lr.finish(w, ha, hb, nrm2, j)
    _bounded("finish v", v, rv, 3 * U * np.abs(rv), "v_next")
    _same(colH[:j + 1], rcol[:j + 1], "H[c][j] = ha[c] + hb[c]")
    _bounded("finish beta", colH[j + 1:], rcol[j + 1:], U * beta, "beta")
    v2, colH2 = _finish(L, Vprev, j, w, ha, hb, nrm2)
    _bits_equal(v2, v, "two launches: v_next")
    _bits_equal(colH2, colH, "two launches: H column")


def test_finish_breakdown(L):
    j, n = 2, 300
    Vprev = _ints(_rng("finish_breakdown"), (j + 1, n))
    ha, hb = np.arange(1.0, j + 3), np.ones(j + 2)
    v, colH = _finish(L, Vprev, j, np.zeros(n), ha, hb, 0.0)
    assert np.all(v == 0.0), "breakdown: v_next is not a zero vector"
    assert colH[j + 1] == 0.0 and np.array_equal(colH[:j + 1], ha[:j + 1] + hb[:j + 1])


# ---------------------------------------------------------------------------------------------------------------------------------
# rotate
# ---------------------------------------------------------------------------------------------------------------------------------
def _rotate(L, V, S, lead=2):
    m, n = V.shape
    nk = S.shape[1]
    ldv, ldo = n + 1, n + 2
    Vfull, _ = _cols(V, ldv)
    Sd = _d64(S)
    Ofull, Od = _cols(np.full((nk, n), NAN), ldo, lead=lead)
    _run(L, "fitgnn_lanczos_rotate_f64", _p(L, Vfull), ldv, m, _p(L, Sd), nk, _p(L, Ofull[lead:]), ldo, n)
    assert torch.isnan(Ofull[:lead]).all().item() and torch.isnan(Ofull[:, n:]).all().item(), "wrote outside the nk columns of out"
    return _np(Od)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("nk", [1, 10, 16])
@pytest.mark.parametrize("m", [1, 60, 128])
def test_rotate_exact(L, m, nk, n):
    rng = _rng("rotate", m, nk, n)
    V, S = _ints(rng, (m, n)), _ints(rng, (m, nk))
    _same(_rotate(L, V, S), lr.rotate(V, S), "out")


@pytest.mark.parametrize("m,nk,n", [(60, 10, 257), (128, 16, 255)])
def test_rotate_random(L, m, nk, n):
    rng = _rng("rotate_random", m, nk, n)
    V, S = rng.normal(size=(m, n)), rng.normal(size=(m, nk))
    out = _rotate(L, V, S)
    _bounded("rotate", out, lr.rotate(V, S), (2 * m - 1) * U * lr.rotate(np.abs(V), np.abs(S)), "out")
    _bits_equal(_rotate(L, V, S), out, "two launches")


def test_refusals(L):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")   # noqa: E731
    zi = torch.zeros(16, dtype=torch.int32, device="cuda")
    a, b, c, big = z(16), z(16), z(16), z(130 * 16)
    lib = L.lib()
    assert lib.fitgnn_lanczos_parts(0) == 0 and lib.fitgnn_lanczos_parts(512) == 1 and lib.fitgnn_lanczos_parts(513) == 2
    C = lambda fn, *args: _call(L, fn, *args)   # noqa: E731
    assert C("fitgnn_lanczos_spmv_f64", None, None, None, None, None, 0, -1.0, 2.0) == 0
    assert C("fitgnn_lanczos_spmv_f64", _p(L, zi), _p(L, zi), _p(L, a), _p(L, b), _p(L, c), -1, -1.0, 2.0) == E_BADARG
    assert C("fitgnn_lanczos_spmv_f64", _p(L, zi), _p(L, zi), _p(L, a), None, _p(L, c), 4, -1.0, 2.0) == E_BADARG
    part, out, Hm, rot = z(130), z(130), z(130 * 130), z(17 * 16)
    P = lambda ldv, ncol, n: C("fitgnn_lanczos_project_f64", _p(L, big), ldv, ncol, _p(L, a), n, None, _p(L, part))   # noqa: E731
    assert P(16, 128, 16) == 0
    assert P(16, 129, 16) == E_BADARG and P(16, 0, 16) == E_BADARG and P(15, 4, 16) == E_BADARG
    R = lambda n_part, ncol1: C("fitgnn_lanczos_reduce_f64", _p(L, big), n_part, ncol1, _p(L, out))   # noqa: E731
    assert R(2, 129) == 0
    assert R(2, 130) == E_BADARG and R(2, 0) == E_BADARG and R(-1, 4) == E_BADARG
    F = lambda ldv, j, n, ldh: C("fitgnn_lanczos_finish_f64", _p(L, big), ldv, j, _p(L, a), n, _p(L, part), _p(L, part), _p(L, part),   # noqa: E731
                                 _p(L, Hm), ldh)
    assert F(16, 127, 16, 128) == 0
    assert F(16, 128, 16, 130) == E_BADARG and F(16, 3, 16, 3) == E_BADARG and F(15, 3, 16, 8) == E_BADARG
    T = lambda m, nk, ldo: C("fitgnn_lanczos_rotate_f64", _p(L, big), 16, m, _p(L, big), nk, _p(L, rot), ldo, 16)   # noqa: E731
    assert T(128, 16, 16) == 0
    assert T(128, 17, 16) == E_BADARG and T(129, 16, 16) == E_BADARG and T(4, 4, 15) == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# one whole step, six times
# ---------------------------------------------------------------------------------------------------------------------------------
def _random_laplacian(rng, n, deg):
    """CSR Laplacian L = D - W of a random weighted graph (each row's columns in random order); returns (rowptr, col, val, max dw)."""
    i = np.repeat(np.arange(n), deg)
    k = rng.integers(0, n, size=i.size)
    keep = i != k
    i, k = i[keep], k[keep]
    wt = rng.uniform(0.5, 1.5, size=i.size)
    W = np.zeros((n, n))
    np.add.at(W, (i, k), wt)
    W = W + W.T
    Lm = np.diag(W.sum(1)) - W
    rowptr, col, val = [0], [], []
    for r in range(n):
        nz = np.nonzero(Lm[r])[0]
        nz = nz[rng.permutation(nz.size)]
        col += nz.tolist(); val += Lm[r, nz].tolist()
        rowptr.append(len(col))
    return np.array(rowptr), np.array(col), np.array(val), float(np.diag(Lm).max())


def test_composed_steps(L):
    rng = _rng("composed")
    n, steps, m = 700, 6, 8
    rowptr, col, val, dmax = _random_laplacian(rng, n, 4)
    offset = 2.0 * dmax
    lens = np.diff(rowptr)
    lib = L.lib()
    rp, ci, vd = _i32(rowptr), _i32(col), _d64(val)
    v0 = rng.normal(size=n)
    V = torch.zeros(m + 1, n, dtype=torch.float64, device="cuda")
    V[0] = _d64(v0 / np.linalg.norm(v0))
    H = torch.zeros(m + 1, m, dtype=torch.float64, device="cuda")
    w = torch.empty(n, dtype=torch.float64, device="cuda")
    parts = int(lib.fitgnn_lanczos_parts(n))
    part = torch.empty(parts * (m + 2), dtype=torch.float64, device="cuda")
    ha, hb, hc = (torch.empty(m + 2, dtype=torch.float64, device="cuda") for _ in range(3))

    def project(ncol, h_in, h_out):
        _run(L, "fitgnn_lanczos_project_f64", _p(L, V), n, ncol, _p(L, w), n, _p(L, h_in), _p(L, part))
        _run(L, "fitgnn_lanczos_reduce_f64", _p(L, part), parts, ncol + 1, _p(L, h_out))

    for j in range(steps):
        Vj = _np(V[:j + 1]).copy()
        _run(L, "fitgnn_lanczos_spmv_f64", _p(L, rp), _p(L, ci), _p(L, vd), _p(L, V[j]), _p(L, w), n, -1.0, offset)
        project(j + 1, None, ha)
        project(j + 1, ha, hb)
        project(j + 1, hb, hc)
        _run(L, "fitgnn_lanczos_finish_f64", _p(L, V), n, j, _p(L, w), n, _p(L, ha), _p(L, hb), _p(L, hc), _p(L, H), m)
        # the reference step on the same basis, and the elementwise error bounds of w after the product and after each pass
        ncol = j + 1
        w_s = lr.spmv(rowptr, col, val, Vj[j], -1.0, offset)
        e_s = (2 * -(-lens // 8) + 5) * U * lr.spmv(rowptr, col, np.abs(val), np.abs(Vj[j]), 1.0, offset)
        _, h1, _ = lr.project(Vj, w_s, None)
        w1, h2, _ = lr.project(Vj, w_s, h1)
        e_1 = 2 * ncol * U * (np.abs(w_s) + lr.project_cond(Vj, h1))
        w2, _, nrm2 = lr.project(Vj, w1, h2)
        e_2 = 2 * ncol * U * (np.abs(w1) + lr.project_cond(Vj, h2))
        _, rcol, beta = lr.finish(w2, h1, h2, nrm2, j)
        _, _, c1 = lr.dots(Vj, w_s)
        _, _, c2 = lr.dots(Vj, w1)
        d2 = 15 * U * c2
        bound_h = np.abs(Vj) @ (e_s + e_1) + 15 * U * c1 + d2 + U * np.abs(rcol[:ncol])
        bound_beta = np.linalg.norm(e_s + e_1 + e_2) + np.linalg.norm(d2) + (15 / 2 + 2) * U * beta
        Hcol = _np(H[:, j])
        _bounded("composed H", Hcol[:ncol], rcol[:ncol], bound_h, f"step {j}: H[:{ncol}, {j}]")
        _bounded("composed beta", Hcol[ncol:ncol + 1], rcol[ncol:], bound_beta, f"step {j}: beta")
        assert np.all(Hcol[ncol + 1:] == 0), "wrote below the sub-diagonal of H"
        Vl = _np(V[:j + 2]).astype(LD)
        ortho = float(np.max(np.abs(Vl @ Vl.T - np.eye(j + 2, dtype=LD))))
        print(f"[ratio] composed orthogonality: step {j}: {ortho / (64 * U):.3g} of 64 u")
        assert ortho <= 64 * U, f"step {j}: max |V V^T - I| = {ortho} > 64 * 2^-53"
        # both passes really subtract: the coefficients of the second pass are at rounding level, those of the first are not
        assert np.max(np.abs(_np(hb[:ncol]))) <= 1e-10 * offset and np.max(np.abs(_np(ha[:ncol]))) > 1e-3 * offset
