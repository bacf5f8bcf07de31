"""GPU tier: the multi-head attention query kernels of csrc/query.hip (fitgnn_mhgat_query_gather_f32, fitgnn_mhgat_query_tail_f32)
through the C ABI against the float64 reference of tests/mhgat_query_reference.py (the convention and helpers of
tests/test_gpu_gat_query_kernels.py).

EXACT inputs (mhgat_query_reference.exact_uniform_case / exact_selector_case: every fp32 intermediate exact in any summation order,
the even and the odd heads selecting different entries at both layers, proven on the CPU by tests/test_mhgat_query_reference_cpu.py)
must come back bit for bit.  With equal layer-0 scores in every head, block hd of G must hold the bits of the single-head kernel on
(U_src[hd], U_dst[hd]).  RANDOM inputs are held per entry to 2^-24 times the first-order bound the reference accumulates along the
kernel's own operation order (derived in the reference's docstring); nothing is added on top.  The tail must hold the bits of
fitgnn_gcn_query_tail_f32 on the block-expanded W1.

Launcher -> branch -> tests that reach it:

| branch (from the launch and kernel code) | tests |
|---|---|
| (heads, H) = (2, 8) one live float4 per head; (4, 64); (8, 256) a full slot, <1>; (5, 260) an odd head count, second slot with one live lane, <2>; (2, 512) a head is a whole slot; (8, 512) both slots full | test_exact[*] |
| query degree 0 (zeros over a NaN-filled G), 1, 2, 3 (waves without entries), 4, 5, 8, 9, 17, 64, 65, 130; 16, 128 | test_exact[selector-*], [uniform-*] |
| neighbour degree 0 (ELU(b0)), 1, 2, 63, 64, 65 (second 64-entry weight tile), 300; 4, 128, 256; groups of four with 1-3 missing | test_exact[*] |
| xrow NULL / given (repeated table rows, an entry at the last table row, NaN behind T); b0 NULL / given; ldt > H, ldg > heads H | test_exact[*] |
| rows repeated and permuted; NaN guards behind and between the rows of G untouched | test_exact[*] (second launch), test_rows |
| a lane's two slots in two heads; heads that merge on waves 0..3 and a second head per wave (heads > 4) | test_exact[(8, 512)], [(5, 260)], test_random |
| per-head online softmax: a new maximum (rescale), an entry below it, ties; the merge of waves with and without entries | test_exact[selector-*], test_random |
| the single-head kernel's bits per block when the heads share their layer-0 scores | test_shared_scores_equal_the_single_head_kernel |
| scores of ordinary size on both sides of both LeakyReLUs; a spread >= 200 in a row in some heads only | test_random[*] |
| two launches give the same bits | every test (_gather) |
| a query without entries -> zeros; a neighbour without entries -> ELU(b0) in every block | test_edge_rows |
| T, G, U_src or U_dst one float into its buffer -> FITGNN_E_ALIGN | test_misaligned |
| tail: C1 = 16 (one column block per head; H = 8 one k-stage, 64 two, 260 a 4-wide last stage), C1 = 64 at H = 512; Q = 1, 16, 17, 33 (full and partial tiles); b1, bl, log_softmax on and off | test_tail_equals_the_expanded_product[*] |
"""
import numpy as np
import pytest
import torch

import gat_query_reference as gq
import mhgat_query_reference as mq
import query_reference as qr
from test_gpu_query_kernels import _guarded, _ratio, _untouched
from test_gpu_step_kernels import E_ALIGN, L, U, _call, _dev, _np, _p, _rng, _run, _same, _strided  # noqa: F401

pytestmark = pytest.mark.gpu
FN, ONE, TAIL, GCN_TAIL = "fitgnn_mhgat_query_gather_f32", "fitgnn_gat_query_gather_f32", "fitgnn_mhgat_query_tail_f32", "fitgnn_gcn_query_tail_f32"


def _gather(L, c, ldt_pad=4, ldg_pad=8, rows=None):
    H, heads = c["T"].shape[1], c["heads"]
    W = heads * H
    rows = c["rows"] if rows is None else rows
    Td = _strided(c["T"], H + ldt_pad)
    buf, G = _guarded(len(rows), W, W + ldg_pad)
    opt = lambda a, dt=torch.float32: None if a is None else _dev(a, dt)   # noqa: E731
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), opt(c["xrow"], torch.int32), _dev(c["a_src0"]), _dev(c["a_dst0"]),
            opt(c["b0"]), _dev(c["U_src"]), _dev(c["U_dst"]), _dev(rows, torch.int64)]
    rp, cl, xr, a_s, a_d, b0, us, ud, rw = keep
    args = (_p(L, rp), _p(L, cl), _p(L, Td), H + ldt_pad, _p(L, xr), _p(L, a_s), _p(L, a_d), heads, _p(L, b0), float(c["slope0"]), _p(L, us),
            _p(L, ud), float(c["slope1"]), _p(L, rw), len(rows), H, _p(L, G), W + ldg_pad)
    _run(L, FN, *args)
    first = G.clone()
    _untouched(buf, len(rows), W, W + ldg_pad, "mhgat gather")
    _run(L, FN, *args)
    assert torch.equal(first, G), "two launches differ"
    return _np(first)


@pytest.mark.parametrize("case", mq.EXACT_GATHER_CASES, ids=str)
@pytest.mark.parametrize("gen", sorted(mq.EXACT_GENERATORS))
def test_exact(L, gen, case):
    c = mq.EXACT_GENERATORS[gen](*case)
    ref = mq.run(c, f32_elu=True)
    got = _gather(L, c)           # ldt = H + 4, ldg = heads H + 8, NaN in the padding
    assert np.all(got[0] == 0), "a query row without entries must give zeros"
    _same(got, ref, f"mhgat gather {gen} {case}")
    rng = _rng("mhgat-query-exact-rows", gen, case)
    rows = np.concatenate([rng.permutation(c["rows"]), c["rows"][::-1], c["rows"][:3]]).astype(np.int64)   # permuted, every row repeated
    _same(_gather(L, c, rows=rows), ref[rows], f"mhgat gather {gen} {case} rows")   # (rows = arange: the reference's row q is ref[q])


def _random_case(tag, heads, H, q_degs, n_degs, with_xrow, with_b0, spread):
    """Scores of ordinary size: a0s, a0d ~ N(0, 1) per head, U ~ N(0, 1) / sqrt(H) on h of size 1.  spread: in the EVEN heads some table
    rows get a0s lowered by 1200 (240 after the LeakyReLU) and one column of the head's block of T is scaled, with U_src[hd] = 1
    there, so that the layer-1 scores of a row differ by more than 200 as well; the odd heads keep ordinary scores."""
    rng = _rng("mhgat-query-gather", tag, heads, H, spread)
    n_table = 41
    C0 = H // heads
    rowptr, col, _, xrow, n_rows = qr.query_csr(rng, q_degs, n_degs, n_table, with_xrow, pow2_val=False)
    nt = n_table if with_xrow else n_rows
    T = rng.normal(0, 1, size=(nt, H)).astype(np.float32)
    a_src0, a_dst0 = rng.normal(0, 1, size=(nt, heads)).astype(np.float32), rng.normal(0, 1, size=(nt, heads)).astype(np.float32)
    U_src = (rng.normal(0, 1, size=(heads, H)) / np.sqrt(H)).astype(np.float32)
    U_dst = (rng.normal(0, 1, size=(heads, H)) / np.sqrt(H)).astype(np.float32)
    if spread:
        for g in range(0, heads, 2):
            a_src0[::3, g] -= 1200.0
            T[::2, g * C0 + 1] *= 1000.0
            U_src[g, g * C0 + 1] = 1.0
    b0 = rng.normal(0, 1, size=H).astype(np.float32) if with_b0 else None
    return dict(rowptr=rowptr, col=col, xrow=xrow, T=T, b0=b0, a_src0=a_src0, a_dst0=a_dst0, U_src=U_src, U_dst=U_dst, slope0=0.2, slope1=0.3,
                rows=np.arange(len(q_degs), dtype=np.int64), n_rows=n_rows, heads=heads)


def _score_spreads(c):
    """Per head (largest spread of the layer-0 scores within a row, of the layer-1 scores within a query), from the reference's
    intermediates."""
    heads = c["heads"]
    s0 = np.zeros(heads)
    s1 = np.zeros(heads)
    st = {"g": 0, "f": []}

    def flush():
        if st["f"]:
            s1[st["g"]] = max(s1[st["g"]], max(st["f"]) - min(st["f"]))

    def watch(name, a):
        if name == "e":
            np.maximum(s0, np.max(a, 0) - np.min(a, 0), out=s0)
        elif name == "head":
            flush()
            st["g"], st["f"] = int(a), []
        elif name == "f":
            st["f"].append(float(a))
    ref, B = mq.run(c, watch=watch, sums=True)
    flush()
    return ref, B, s0, s1


@pytest.mark.parametrize("heads,H,with_xrow,with_b0,spread", [(4, 64, True, True, False), (5, 260, False, True, False),
                                                              (8, 512, True, False, False), (2, 64, False, True, True),
                                                              (8, 512, True, True, True)], ids=str)
def test_random(L, heads, H, with_xrow, with_b0, spread):
    c = _random_case("random", heads, H, qr.GATHER_QUERY_DEGS, qr.GATHER_NEIGHBOUR_DEGS, with_xrow, with_b0, spread)
    ref, B, s0, s1 = _score_spreads(c)
    if spread:
        assert np.any((s0 >= 200) & (s1 >= 200)), (s0, s1)       # in at least one head, at both layers
        assert np.any(s0 < 50), s0                               # and not in every head
    got = _gather(L, c)
    assert np.isfinite(got).all(), "NaN or Inf"
    _ratio(got, ref, B, f"mhgat gather random heads={heads} H={H} spread={spread}")


@pytest.mark.parametrize("heads,H", [(4, 64), (2, 512)], ids=str)
def test_shared_scores_equal_the_single_head_kernel(L, heads, H):
    """a0s and a0d with `heads` equal columns: block hd of G is, bit for bit, fitgnn_gat_query_gather_f32 called with one column of the
    scores and (U_src[hd], U_dst[hd])."""
    c = _random_case("shared", heads, H, qr.GATHER_QUERY_DEGS, qr.GATHER_NEIGHBOUR_DEGS, True, True, False)
    c["a_src0"] = np.repeat(c["a_src0"][:, :1], heads, axis=1)
    c["a_dst0"] = np.repeat(c["a_dst0"][:, :1], heads, axis=1)
    got = _gather(L, c)
    Q = len(c["rows"])
    Td = _strided(c["T"], H + 4)
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["xrow"], torch.int32), _dev(c["a_src0"][:, 0]),
            _dev(c["a_dst0"][:, 0]), _dev(c["b0"]), _dev(c["U_src"]), _dev(c["U_dst"]), _dev(c["rows"], torch.int64)]
    rp, cl, xr, a_s, a_d, b0, us, ud, rw = keep
    for g in range(heads):
        buf, G1 = _guarded(Q, H, H + 8)
        _run(L, ONE, _p(L, rp), _p(L, cl), _p(L, Td), H + 4, _p(L, xr), _p(L, a_s), _p(L, a_d), _p(L, b0), 0.2, _p(L, us[g]), _p(L, ud[g]), 0.3,
             _p(L, rw), Q, H, _p(L, G1), H + 8)
        _same(got[:, g * H:(g + 1) * H], _np(G1), f"mhgat gather shared scores heads={heads} H={H} block {g}")
    assert not np.array_equal(got[:, :H], got[:, H:2 * H])     # the blocks themselves differ: U does


@pytest.mark.parametrize("Q", [1, 3, 64, 257])
def test_rows(L, Q):
    c = _random_case("rows", 4, 64, [3, 0, 7, 1, 12, 5, 2, 9, 4, 6], [2, 5, 1, 9, 0, 3], True, True, False)
    rng = _rng("mhgat-query-rows", Q)
    rows = rng.integers(0, c["n_rows"], size=Q).astype(np.int64)   # unsorted, duplicates, any row of the CSR (h_q from the row itself)
    if Q >= 3:
        rows[1] = rows[0]
    uniq, inv = np.unique(rows, return_inverse=True)
    ref, B = mq.run(c, rows=uniq, sums=True)
    _ratio(_gather(L, c, rows=rows), ref[inv], B[inv], f"mhgat gather rows Q={Q}")


def test_edge_rows(L):
    """A query without entries gives zeros, not NaN; a query whose only neighbour has no entries gives ELU(b0) in every block
    (beta = 1 in every head)."""
    H, heads = 8, 2
    rng = _rng("mhgat-query-edge")
    #        row 0: no entries; row 1: -> row 2; row 2: no entries; row 3: -> rows 2, 2
    c = dict(rowptr=np.array([0, 0, 1, 1, 3], dtype=np.int32), col=np.array([2, 2, 2], dtype=np.int32), xrow=None,
             T=rng.normal(size=(4, H)).astype(np.float32), b0=np.array([-3, -1, -0.5, 0, 0.25, 1, 2, -40], dtype=np.float32),
             a_src0=rng.normal(size=(4, heads)).astype(np.float32), a_dst0=rng.normal(size=(4, heads)).astype(np.float32),
             U_src=rng.normal(size=(heads, H)).astype(np.float32), U_dst=rng.normal(size=(heads, H)).astype(np.float32), slope0=0.2,
             slope1=0.2, rows=np.array([0, 1, 3, 2], dtype=np.int64), n_rows=4, heads=heads)
    got = _gather(L, c)
    ref, B = mq.run(c, sums=True)
    assert np.all(got[0] == 0) and np.all(got[3] == 0)
    elu_b0 = qr.elu(c["b0"])
    for g in range(heads):
        blk = got[1, g * H:(g + 1) * H]
        assert np.all(np.abs(blk - elu_b0) <= 2 * U * np.abs(elu_b0))    # one entry: L = 1, g = h (1 / 1); expm1f within 1 ulp
        assert np.all(blk[c["b0"] > 0] == c["b0"][c["b0"] > 0])
    _ratio(got, ref, B, "mhgat gather edge rows")


def test_misaligned(L):
    heads, H = 2, 8
    c = _random_case("align", heads, H, [2, 1], [1, 2], False, False, False)
    keep = [_dev(c["rowptr"], torch.int32), _dev(c["col"], torch.int32), _dev(c["a_src0"]), _dev(c["a_dst0"]), _dev(c["rows"], torch.int64)]
    rp, cl, a_s, a_d, rw = keep
    buf = torch.zeros(c["n_rows"] * H + 8, dtype=torch.float32, device="cuda")
    out = torch.zeros(2 * heads * H + 8, dtype=torch.float32, device="cuda")
    u = torch.zeros(2 * heads * H + 8, dtype=torch.float32, device="cuda")

    def args(T=buf, G=out, us=u, ud=u[heads * H:]):
        return (_p(L, rp), _p(L, cl), _p(L, T), H, None, _p(L, a_s), _p(L, a_d), heads, None, 0.2, _p(L, us), _p(L, ud), 0.2, _p(L, rw), 2, H,
                _p(L, G), heads * H)
    assert _call(L, FN, *args()) == 0
    assert _call(L, FN, *args(T=buf[1:])) == E_ALIGN
    assert _call(L, FN, *args(G=out[1:])) == E_ALIGN
    assert _call(L, FN, *args(us=u[1:])) == E_ALIGN
    assert _call(L, FN, *args(ud=u[heads * H + 1:])) == E_ALIGN


@pytest.mark.parametrize("log_softmax", [False, True], ids=["raw", "log_softmax"])
@pytest.mark.parametrize("biases", [False, True], ids=["no_bias", "bias"])
@pytest.mark.parametrize("heads,H,H2,C,Q", [(2, 8, 32, 3, 1), (4, 64, 64, 7, 17), (5, 260, 80, 5, 16), (8, 512, 512, 47, 33)], ids=str)
def test_tail_equals_the_expanded_product(L, heads, H, H2, C, Q, biases, log_softmax):
    """out is, bit for bit, fitgnn_gcn_query_tail_f32 on the same G with K = heads H and the block-expanded W1: every z[n] is one fmaf
    chain over its block's k ascending, and a product with the expansion's zeros changes no partial sum.  Guard rows past Q and the
    padding of out stay NaN."""
    rng = _rng("mhgat-query-tail", heads, H, H2, C, Q, biases)
    K = heads * H
    Gh = rng.normal(0, 1, size=(Q, K)).astype(np.float32)
    W1 = (rng.normal(0, 1, size=(H2, H)) / np.sqrt(H)).astype(np.float32)
    Wl = (rng.normal(0, 1, size=(C, H2)) / np.sqrt(H2)).astype(np.float32)
    b1 = _dev(rng.normal(0, 1, size=H2).astype(np.float32)) if biases else None
    bl = _dev(rng.normal(0, 1, size=C).astype(np.float32)) if biases else None
    Gd = _strided(Gh, K + 8)
    W1d, W1big, Wld = _dev(W1), _dev(mq.tail_expanded(W1, heads)), _dev(Wl)
    ldo = C + 5
    assert 0 < L.lib().fitgnn_gcn_query_tail_lds_bytes(H2, C) <= 160 * 1024
    buf, out = _guarded(Q, C, ldo)
    args = (_p(L, Gd), K + 8, Q, _p(L, W1d), _p(L, b1), _p(L, Wld), _p(L, bl), H, H2, heads, C, _p(L, out), ldo, int(log_softmax))
    _run(L, TAIL, *args)
    first = out.clone()
    _untouched(buf, Q, C, ldo, "mhgat tail")
    _run(L, TAIL, *args)
    assert torch.equal(first, out), "two launches differ"
    buf2, want = _guarded(Q, C, ldo)
    _run(L, GCN_TAIL, _p(L, Gd), K + 8, Q, _p(L, W1big), _p(L, b1), _p(L, Wld), _p(L, bl), K, H2, C, _p(L, want), ldo, int(log_softmax))
    assert torch.isfinite(first).all()
    assert torch.equal(first, want), f"mhgat tail {(heads, H, H2, C, Q)}: differs from the GCN tail on the expanded W1"
    # and it is the product the formula states: query_reference.tail's own bound on the expanded product, nothing added
    big, hb1, hbl = mq.tail_expanded(W1, heads), None if b1 is None else _np(b1), None if bl is None else _np(bl)
    logits, B = qr.tail(Gh, big, hb1, Wl, hbl, sums=True)
    if log_softmax:
        _ratio(_np(first), qr.tail(Gh, big, hb1, Wl, hbl, log_softmax=True), qr.log_softmax_bound(logits, B), f"mhgat tail log-softmax {(heads, H, H2, C, Q)}")
    else:
        _ratio(_np(first), logits, B, f"mhgat tail logits {(heads, H, H2, C, Q)}")
