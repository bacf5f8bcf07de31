"""GPU tier: the attention query kernel of csrc/query.hip (fitgnn_gat_query_gather_f32) through the C ABI against the float64
reference of tests/gat_query_reference.py (the convention and helpers of tests/test_gpu_query_kernels.py).

EXACT inputs (gat_query_reference.exact_uniform_case / exact_selector_case: every fp32 intermediate exact in any summation order,
proven on the CPU by tests/test_gat_query_reference_cpu.py) must come back bit for bit.  RANDOM inputs are held per entry to 2^-24
times the first-order bound the reference accumulates along the kernel's own operation order (derived in the reference's docstring:
one rounding per fmaf, add and product, expf / expm1f / the division within 1 ulp); nothing is added on top.

Launcher -> branch -> tests that reach it:

| branch (from the launch and kernel code) | tests |
|---|---|
| column slots: H = 4 (one live lane), 64, 256 (one full slot, <1>), 260 (second slot, one live lane, <2>), 512 | test_exact[*] |
| query degree 0 (zeros over a NaN-filled G), 1, 2, 3 (waves without entries), 4, 5, 8, 9, 17, 64, 65, 130; 16, 128 | test_exact[selector-*], [uniform-*] |
| neighbour degree 0 (ELU(b0)), 1, 2, 63, 64, 65 (second 64-entry fetch), 300; 4, 128, 256; groups of four with 1-3 missing | test_exact[*] |
| xrow NULL / given (repeated table rows, an entry at the last table row, NaN behind T); b0 NULL / given; ldt > H, ldg > H | test_exact[*] |
| rows repeated and permuted; NaN guards behind and between the rows of G untouched | test_exact[*] (second launch), test_rows |
| online softmax: a new maximum (rescale), an entry below it, ties; the merge of waves with and without entries | test_exact[selector-*], test_random |
| scores of ordinary size on both sides of both LeakyReLUs; a spread >= 200 in a row (underflowing weights, no NaN / Inf) | test_random[*] |
| two launches give the same bits | every test (_gather) |
| a query without entries -> zeros; a neighbour without entries -> ELU(b0) | test_edge_rows |
| T, G, u_src or u_dst one float into its buffer -> FITGNN_E_ALIGN | test_misaligned |
"""
import numpy as np
import pytest
import torch

import gat_query_reference as gq
import query_reference as qr
from test_gpu_query_kernels import _guarded, _ratio, _untouched
from test_gpu_step_kernels import E_ALIGN, L, U, _call, _dev, _np, _p, _rng, _run, _same, _strided  # noqa: F401

pytestmark = pytest.mark.gpu
FN = "fitgnn_gat_query_gather_f32"


def _gather(L, c, ldt_pad=4, ldg_pad=8, rows=None):
    H = c["T"].shape[1]
    rows = c["rows"] if rows is None else rows
    Td = _strided(c["T"], H + ldt_pad)
    buf, G = _guarded(len(rows), H, H + ldg_pad)
    opt = lambda a, dt=torch.float32: None if a is None else _dev(a, dt)   # noqa: E731
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), opt(c["xrow"], torch.int32), _dev(c["a_src0"]), _dev(c["a_dst0"]),
            opt(c["b0"]), _dev(c["u_src"]), _dev(c["u_dst"]), _dev(rows, torch.int64)]
    rp, cl, xr, a_s, a_d, b0, us, ud, rw = keep
    args = (_p(L, rp), _p(L, cl), _p(L, Td), H + ldt_pad, _p(L, xr), _p(L, a_s), _p(L, a_d), _p(L, b0), float(c["slope0"]), _p(L, us), _p(L, ud),
            float(c["slope1"]), _p(L, rw), len(rows), H, _p(L, G), H + ldg_pad)
    _run(L, FN, *args)
    first = G.clone()
    _untouched(buf, len(rows), H, H + ldg_pad, "gat gather")
    _run(L, FN, *args)
    assert torch.equal(first, G), "two launches differ"
    return _np(first)


@pytest.mark.parametrize("case", gq.EXACT_GATHER_CASES, ids=str)
@pytest.mark.parametrize("gen", sorted(gq.EXACT_GENERATORS))
def test_exact(L, gen, case):
    c = gq.EXACT_GENERATORS[gen](*case)
    ref = gq.run(c, f32_elu=True)
    got = _gather(L, c)           # ldt = H + 4, ldg = H + 8, NaN in the padding
    assert np.all(got[0] == 0), "a query row without entries must give zeros"
    _same(got, ref, f"gat gather {gen} {case}")
    rng = _rng("gat-query-exact-rows", gen, case)
    rows = np.concatenate([rng.permutation(c["rows"]), c["rows"][::-1], c["rows"][:3]]).astype(np.int64)   # permuted, every row repeated
    _same(_gather(L, c, rows=rows), gq.run(c, rows=rows, f32_elu=True), f"gat gather {gen} {case} rows")


def _random_case(tag, H, q_degs, n_degs, with_xrow, with_b0, spread):
    """Scores of ordinary size: a0s, a0d ~ N(0, 1), u ~ N(0, 1) / sqrt(H) on h of size 1.  spread: some table rows get a0s lowered
    by 1200 (240 after the LeakyReLU) and one column of T is scaled so that the layer-1 scores of a row differ by more than 200 as
    well."""
    rng = _rng("gat-query-gather", tag, H, spread)
    n_table = 41
    rowptr, col, _, xrow, n_rows = qr.query_csr(rng, q_degs, n_degs, n_table, with_xrow, pow2_val=False)
    nt = n_table if with_xrow else n_rows
    T = rng.normal(0, 1, size=(nt, H)).astype(np.float32)
    a_src0, a_dst0 = rng.normal(0, 1, size=nt).astype(np.float32), rng.normal(0, 1, size=nt).astype(np.float32)
    u_src, u_dst = (rng.normal(0, 1, size=H) / np.sqrt(H)).astype(np.float32), (rng.normal(0, 1, size=H) / np.sqrt(H)).astype(np.float32)
    if spread:
        a_src0[::3] -= 1200.0
        T[::2, 1] *= 1000.0
        u_src[1] = 1.0
    b0 = rng.normal(0, 1, size=H).astype(np.float32) if with_b0 else None
    return dict(rowptr=rowptr, col=col, xrow=xrow, T=T, b0=b0, a_src0=a_src0, a_dst0=a_dst0, u_src=u_src, u_dst=u_dst, slope0=0.2, slope1=0.3,
                rows=np.arange(len(q_degs), dtype=np.int64), n_rows=n_rows)


def _score_spreads(c):
    """(largest spread of the layer-0 scores within a row, of the layer-1 scores within a query) from the reference's intermediates."""
    spread = {"e": 0.0}
    per_q = []

    def watch(name, a):
        if name == "e":
            spread["e"] = max(spread["e"], float(np.max(a) - np.min(a)))
        elif name == "cq":
            per_q.append([])
        elif name == "f":
            per_q[-1].append(float(a))
    gq.run(c, watch=watch)
    return spread["e"], max(max(f) - min(f) for f in per_q if f)


@pytest.mark.parametrize("H,with_xrow,with_b0,spread", [(64, True, True, False), (260, False, True, False), (512, True, False, False),
                                                        (64, False, True, True), (512, True, True, True)], ids=str)
def test_random(L, H, with_xrow, with_b0, spread):
    c = _random_case("random", H, qr.GATHER_QUERY_DEGS, qr.GATHER_NEIGHBOUR_DEGS, with_xrow, with_b0, spread)
    ref, B = gq.run(c, sums=True)
    if spread:
        s0, s1 = _score_spreads(c)
        assert s0 >= 200 and s1 >= 200, (s0, s1)
    got = _gather(L, c)
    assert np.isfinite(got).all(), "NaN or Inf"
    _ratio(got, ref, B, f"gat gather random H={H} spread={spread}")


@pytest.mark.parametrize("Q", [1, 3, 64, 257])
def test_rows(L, Q):
    c = _random_case("rows", 64, [3, 0, 7, 1, 12, 5, 2, 9, 4, 6], [2, 5, 1, 9, 0, 3], True, True, False)
    rng = _rng("gat-query-rows", Q)
    rows = rng.integers(0, c["n_rows"], size=Q).astype(np.int64)   # unsorted, duplicates, any row of the CSR (h_q from the row itself)
    if Q >= 3:
        rows[1] = rows[0]
    ref, B = gq.run(c, rows=rows, sums=True)
    _ratio(_gather(L, c, rows=rows), ref, B, f"gat gather rows Q={Q}")


def test_edge_rows(L):
    """A query without entries gives zeros, not NaN; a query whose only neighbour has no entries gives ELU(b0) (beta = 1)."""
    H = 8
    rng = _rng("gat-query-edge")
    #        row 0: no entries; row 1: -> row 2; row 2: no entries; row 3: -> rows 2, 2
    c = dict(rowptr=np.array([0, 0, 1, 1, 3], dtype=np.int32), col=np.array([2, 2, 2], dtype=np.int32), xrow=None,
             T=rng.normal(size=(4, H)).astype(np.float32), b0=np.array([-3, -1, -0.5, 0, 0.25, 1, 2, -40], dtype=np.float32),
             a_src0=rng.normal(size=4).astype(np.float32), a_dst0=rng.normal(size=4).astype(np.float32),
             u_src=rng.normal(size=H).astype(np.float32), u_dst=rng.normal(size=H).astype(np.float32), slope0=0.2, slope1=0.2,
             rows=np.array([0, 1, 3, 2], dtype=np.int64), n_rows=4)
    got = _gather(L, c)
    ref, B = gq.run(c, sums=True)
    assert np.all(got[0] == 0) and np.all(got[3] == 0)
    elu_b0 = qr.elu(c["b0"])
    assert np.all(np.abs(got[1] - elu_b0) <= 2 * U * np.abs(elu_b0))    # one entry: L = 1, g = h (1 / 1); expm1f within 1 ulp
    assert np.all(got[1][c["b0"] > 0] == c["b0"][c["b0"] > 0])
    _ratio(got, ref, B, "gat gather edge rows")


def test_misaligned(L):
    c = _random_case("align", 8, [2, 1], [1, 2], False, False, False)
    H = 8
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["a_src0"]), _dev(c["a_dst0"]), _dev(c["rows"], torch.int64)]
    rp, cl, a_s, a_d, rw = keep
    buf = torch.zeros(c["n_rows"] * H + 8, dtype=torch.float32, device="cuda")
    out = torch.zeros(2 * H + 8, dtype=torch.float32, device="cuda")
    u = torch.zeros(2 * H + 8, dtype=torch.float32, device="cuda")

    def args(T=buf, G=out, us=u, ud=u[H:]):
        return (_p(L, rp), _p(L, cl), _p(L, T), H, None, _p(L, a_s), _p(L, a_d), None, 0.2, _p(L, us), _p(L, ud), 0.2, _p(L, rw), 2, H, _p(L, G), H)
    assert _call(L, FN, *args()) == 0
    assert _call(L, FN, *args(T=buf[1:])) == E_ALIGN
    assert _call(L, FN, *args(G=out[1:])) == E_ALIGN
    assert _call(L, FN, *args(us=u[1:])) == E_ALIGN
    assert _call(L, FN, *args(ud=u[H + 1:])) == E_ALIGN
