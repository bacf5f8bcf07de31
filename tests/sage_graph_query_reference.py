"""float64 reference of the SAGE graph-query launch (csrc/query.hip, fitgnn_sage_graph_query_hops_f32) in the kernel's stated operation
order, a float64 model forward composed from the oracle's sage_conv plus the pool, the head and the softmax, and the input generators
the CPU and GPU tests share (test infrastructure only; the conventions of tests/sage_query_reference.py and
tests/graph_query_reference.py, whose graph_view, pooled_rows, HOPS_SIZES, HOPS_ROW_DEGS, exact_sage_inputs, mean_csr and elu are reused
by import).  The tail is fitgnn_gcn_graph_query_tail_f32, unchanged, on G = [g_r | h_r] with W1 = [W_l1 | W_r1] and b1 = b_l1:
graph_query_reference.pooled_tail is its reference.

phase 1  EVERY row r of a queried graph's range [r0, r1), once: a = 0; a = val[e'] * T[t(col[e'])][c] + a over row r's entries in CSR
         order; h_r[c] = ELU((a + T[t(r)][H + c]) + b0[c]) (b0 None: the second add is absent); t(r) = xrow[r] with an indirection, else
         r.  sage_query_reference.gather's "row r": tests/test_sage_graph_query_reference_cpu.py holds the two together.
phase 2  pooled row r = prow[j]: g = 0; g = val[e] * h_{col[e]}[c] + g over the row's entries in CSR order, ONE chain (no wave
         partials); G[j][0:H] = g, G[j][H:2H] = h_r.  A pooled row without entries gives g = 0 and still its h_r.

`watch` receives (name, array) for every intermediate; f32_elu rounds the result of ELU to float32 (query_reference.elu).

The error bound of hops(sums=True), in units of u = 2^-24, first order in u:

  layer 0, row r of degree d_r with S_r = sum_e' |val T| + |root| + |b0|: one rounding per fmaf of the chain, one for the root add and
  one for the bias add, each at most the sum of the magnitudes; expm1f is within 1 ulp, and ELU has slope <= 1, so the
  pre-activation's error passes at most unchanged:
      E_r = (d_r + 2) S_r + 2 |h_r| [pre <= 0]                        (sage_query_reference.gather's E_r, the same expression)
  B[j][H:2H] = E_r: the window's copy adds nothing.

  layer 1, pooled row r of degree d = deg(r): the inputs' errors weighted by |val_e|, and ONE chain of d fmaf, each rounding at most
  the sum of the magnitudes:
      B[j][0:H] = sum_e |val_e| E_{col[e]} + d sum_e |val_e h_{col[e]}|
  (the node kernel's four partials have ceil(d / 4) + 3 in the place of d: its g may differ from this one in the last bits).
"""
import numpy as np

import graph_query_reference as gr
import sage_query_reference as sq
from graph_query_reference import HOPS_ROW_DEGS, HOPS_SIZES, graph_view, pooled_rows  # noqa: F401
from query_reference import _see, elu
from sage_query_reference import exact_sage_inputs, mean_csr  # noqa: F401


def hops(rowptr, col, val, T, seg, prow, pptr, xrow=None, b0=None, watch=None, sums=False, f32_elu=False):
    """G [P, 2H] float64: G[j][0:H] = g_r, G[j][H:2H] = h_r for r = prow[j]; T is [n_table, 2H].  sums=True: also B [P, 2H], the
    first-order error bound of every entry in units of 2^-24 (module docstring)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    val, T = np.asarray(val, dtype=np.float64), np.asarray(T, dtype=np.float64)
    seg = np.asarray(seg, dtype=np.int64).reshape(-1, 2)
    prow, pptr = np.asarray(prow, dtype=np.int64), np.asarray(pptr, dtype=np.int64)
    H = T.shape[1] // 2
    assert T.shape[1] == 2 * H
    bias = None if b0 is None else np.asarray(b0, dtype=np.float64)
    tr = (lambda c: int(c)) if xrow is None else (lambda c: int(xrow[c]))
    G, B = np.zeros((len(prow), 2 * H)), np.zeros((len(prow), 2 * H))
    window = {}
    for i, (r0, r1) in enumerate(seg):
        for r in range(r0, r1):     # phase 1: every row of the graph, once
            if r in window:
                continue
            a, S = np.zeros(H), np.zeros(H)
            for e in range(rowptr[r], rowptr[r + 1]):
                term = val[e] * T[tr(col[e]), :H]
                a = _see(watch, "a", term + a)
                S += np.abs(term)
            root = T[tr(r), H:]
            pre = _see(watch, "a", a + root)
            S += np.abs(root)
            if bias is not None:
                pre = pre + bias
                S += np.abs(bias)
            _see(watch, "pre", pre)
            h = _see(watch, "h", elu(pre, f32_elu))
            window[r] = (h, (rowptr[r + 1] - rowptr[r] + 2) * S + 2 * np.abs(h) * (pre <= 0))
        for j in range(pptr[i], pptr[i + 1]):   # phase 2
            r = int(prow[j])
            assert r0 <= r < r1, "a pooled row outside its graph's range"
            g, absum, inerr = np.zeros(H), np.zeros(H), np.zeros(H)
            for e in range(rowptr[r], rowptr[r + 1]):
                assert r0 <= col[e] < r1, "a column outside the graph's range: the view is not block-diagonal"
                h, herr = window[int(col[e])]
                g = _see(watch, "g", val[e] * h + g)
                absum += np.abs(val[e] * h)
                inerr += np.abs(val[e]) * herr
            G[j, :H], G[j, H:] = g, window[r][0]
            B[j, :H], B[j, H:] = inerr + (rowptr[r + 1] - rowptr[r]) * absum, window[r][1]
    return (G, B) if sums else G


def run(c, **kw):
    """hops() on a case dict."""
    return hops(c["rowptr"], c["col"], c["val"], c["T"], c["seg"], c["prow"], c["pptr"], xrow=c["xrow"], b0=c["b0"], **kw)


def run_rows(c, **kw):
    """sage_query_reference.gather (the per-row kernel's order) on the case's pooled rows."""
    return sq.gather(c["rowptr"], c["col"], c["val"], c["T"], c["prow"], xrow=c["xrow"], b0=c["b0"], **kw)


def max_rows(H):
    """The window arithmetic: max_rows * min(H, 256) floats within 160 KiB."""
    return (160 * 1024) // (4 * min(H, 256))


# ---- the float64 forward the reference is proven against ----
def model_forward(gorc, sd, x, edge_index, seg, prow, pptr, pool, softmax):
    """The float64 model: sage_query_reference.oracle_forward's stack (gorc.sage_conv and ELU, twice) on the whole view, its node head
    switched off by an identity lt1, then per queried graph the pool over its pooled rows, the head and the softmax (network.py's
    Classify_graph_* / Regress_graph_* in eval mode).  sd: the model's state dict (torch tensors)."""
    import torch
    H2 = sd["lt1.weight"].shape[1]
    stack = dict(sd)
    stack["lt1.weight"], stack["lt1.bias"] = torch.eye(H2, dtype=torch.float64), torch.zeros(H2, dtype=torch.float64)
    z = sq.oracle_forward(gorc, stack, x, edge_index, log_softmax=False).numpy()
    Wl, bl = sd["lt1.weight"].double().numpy(), sd["lt1.bias"].double().numpy()
    out = []
    for i in range(len(seg)):
        rows = np.asarray(prow[pptr[i]:pptr[i + 1]], dtype=np.int64)
        p = z[rows].max(0) if pool == "max" else z[rows].mean(0)
        y = p @ Wl.T + bl
        if softmax:
            y = np.exp(y - y.max())
            y = y / y.sum()
        out.append(y)
    return np.stack(out)


# ---- inputs of the kernel tests ----
# (H, with_xrow, with_b0): 4 (one live lane), 64, 256 (one full slab), 260 (second slab, one live lane), 512
EXACT_HOPS_CASES = gr.EXACT_HOPS_CASES
HOPS_GRAPHS = [5, 0, 3, 1, 5, 4, 2]               # unsorted, one graph twice
HOPS_KINDS = ["all", "all", "first", "subset", "subset", "none", "all"]


def _finish(rng, d, gptr, graphs=HOPS_GRAPHS, kinds=HOPS_KINDS):
    seg, prow, pptr = pooled_rows(rng, gptr, graphs, kinds)
    d.update(seg=seg, prow=prow, pptr=pptr, gptr=gptr, max_rows=int((seg[:, 1] - seg[:, 0]).max()))
    return d


def _mean_val(rowptr):
    """val = 1 / max(deg, 1) per entry, in float32: what csr.CSRGraph(mode="mean") holds."""
    deg = np.diff(np.asarray(rowptr, dtype=np.int64))
    return np.repeat((np.float32(1.0) / np.maximum(deg, 1).astype(np.float32)).astype(np.float32), deg)


def exact_case(H, with_xrow, with_b0):
    """The graphs of HOPS_SIZES (1, 2, 3, 4, 5 and 17 rows) with every degree of HOPS_ROW_DEGS (0, 1, 63, 64, 65, 2, 5), queried unsorted
    with one graph twice, pooled rows of every kind.  CSR values in {1/4, 1/2, 1} and sage_query_reference.exact_sage_inputs' table:
    both halves of T in {0..8}/8 (with b0 every other column non-positive, b0 = -32 there: the fp32 ELU is exactly -1; elsewhere the
    identity).  A pre-activation is a multiple of 1/32 of size at most 67, or at most -32; h_r a multiple of 1/32 in [0, 67] or -1; a sum
    of up to 65 products val h a multiple of 1/128 below 2^13: 20 bits, so every intermediate is exact in fp32 in ANY order and the
    node kernel's four partials give the same bits as the window's one chain."""
    rng = np.random.default_rng([H, int(with_xrow), int(with_b0), 79])
    n_table = 37
    rowptr, col, val, xrow, gptr = graph_view(rng, HOPS_SIZES, HOPS_ROW_DEGS, n_table, with_xrow, pow2_val=True)
    T, b0 = exact_sage_inputs(rng, H, n_table if with_xrow else int(gptr[-1]), with_b0)
    return _finish(rng, dict(rowptr=rowptr, col=col, val=val, xrow=xrow, T=T, b0=b0), gptr)


def random_case(H, with_xrow, with_b0, sizes=HOPS_SIZES, degs=HOPS_ROW_DEGS, graphs=HOPS_GRAPHS, kinds=HOPS_KINDS):
    """Ordinary floats: T, b0 ~ N(0, 1), val = 1 / deg as the mean CSR holds it, the same graphs, degrees and pooled rows."""
    rng = np.random.default_rng([H, int(with_xrow), int(with_b0), 83])
    n_table = 41
    rowptr, col, _, xrow, gptr = graph_view(rng, sizes, degs, n_table, with_xrow, pow2_val=False)
    nt = n_table if with_xrow else int(gptr[-1])
    T = rng.normal(0, 1, size=(nt, 2 * H)).astype(np.float32)
    b0 = rng.normal(0, 1, size=H).astype(np.float32) if with_b0 else None
    return _finish(rng, dict(rowptr=rowptr, col=col, val=_mean_val(rowptr), xrow=xrow, T=T, b0=b0), gptr, graphs, kinds)


def window_case(H, n_rows, exact=True):
    """A graph of 3 rows, one of n_rows rows (small degrees: the reference walks every entry) and another of 2, every row pooled,
    queried large, small, small.  EXACT: exact_case's draws with degrees 0, 1, 2, 3, 5."""
    rng = np.random.default_rng([H, n_rows, int(exact), 89])
    rowptr, col, val, _, gptr = graph_view(rng, [3, n_rows, 2], [[1, 2], [0, 1, 2, 3, 5], [2, 1]], 1, False, pow2_val=True)
    n = int(gptr[-1])
    if exact:
        T, b0 = exact_sage_inputs(rng, H, n, True)
    else:
        T, b0 = rng.normal(0, 1, size=(n, 2 * H)).astype(np.float32), rng.normal(0, 1, size=H).astype(np.float32)
        val = _mean_val(rowptr)
    d = _finish(rng, dict(rowptr=rowptr, col=col, val=val, xrow=None, T=T, b0=b0), gptr, [1, 0, 2], ["all"])
    d["max_rows"] = n_rows
    return d
