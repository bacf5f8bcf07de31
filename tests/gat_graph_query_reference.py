"""float64 reference of the GAT graph-query launch (csrc/query.hip, fitgnn_gat_graph_query_hops_f32) in the kernel's stated operation
order, a float64 model forward composed from the oracle's GAT stack plus the pool, the head and the softmax, and the input generators the
CPU and GPU tests share (test infrastructure only; the conventions of tests/gat_query_reference.py and tests/graph_query_reference.py).
The tail is fitgnn_gcn_graph_query_tail_f32, unchanged: graph_query_reference.pooled_tail is its reference.

A wave holds a whole row: lane l owns columns 4 l .. 4 l + 3 and, for H > 256, 256 + 4 l .. 256 + 4 l + 3.

phase 1  EVERY row r of a queried graph's range [r0, r1), once: h_r as gat_query_reference's "row r" (layer0 below is that routine, kept
         per row; tests/test_gat_graph_query_reference_cpu.py holds the two together bit for bit); ds_r = u_s . h_r and dd_r = u_d . h_r
         in gat_query_reference.lane_dot's order.
phase 2  pooled row r with entries e in CSR order: s_e = ds[col[e]] + dd[r]; f_e = s_e > 0 ? s_e : slope1 s_e; m = max_e f_e;
         p_e = exp(f_e - m); from 0 in CSR order, ONE chain: l = l + p_e, g = p_e h_{col[e]} + g; G = g (1 / l).  A pooled row without
         entries gives zeros.

`watch` receives (name, array) for every intermediate; f32_elu rounds the results of ELU AND of exp to float32 (gat_query_reference).

The error bound of hops(sums=True), in units of u = 2^-24, first order in u, in gat_query_reference's terms:

  layer 0 and the dots carry over unchanged: herr_c(r) for every row of the graph, and for a dot
      dc(u, r) = (4 NS + 6) sum_c |u_c h_rc| + sum_c |u_c| herr_c(r)          (ds_j: u = u_s, row j; dd_r: u = u_d, row r).

  layer 1, pooled row r of degree D: the two-pass softmax's bound, as at layer 0.  s_e rounds once (|s_e|) and carries both dots'
  errors; the LeakyReLU has Lipschitz constant max(1, |slope1|) and one more rounded product where s_e <= 0 (|f_e|).  A softmax does
  not see a common shift of its scores, so the value of m matters only through the rounding of f_e - m (|f_e - m|); expf adds 2:
      Phi_e = max(1, |slope1|) (dc(u_s, col[e]) + dc(u_d, r) + |s_e|) + [s_e <= 0] |f_e| + |f_e - m| + 2
  and with beta_e the true softmax weight the sum g_c = sum_e beta_e h_{col[e]c} moves by at most
      B_c(r) = sum_e beta_e Phi_e |h_ec| + |g_c| sum_e beta_e Phi_e + sum_e beta_e herr_c(col[e])
               + D sum_e beta_e |h_ec|          the D fmafs of the one chain
               + (D + 3) |g_c|                  the D additions of l, the division (2) and the final product
               + tiny sum_e |h_ec|              (a weight below the smallest normal number may come back as 0).
"""
import numpy as np

import gat_query_reference as gq
import graph_query_reference as gr
import query_reference as qr
from gat_query_reference import TINY, _exp, lane_dot, lrelu, slots
from query_reference import _see, elu


def layer0(rowptr, col, T, a_src0, a_dst0, need, xrow=None, b0=None, slope0=0.2, watch=None, f32_elu=False):
    """{r: (h_r, herr_r)} for the rows in `need`: gat_query_reference.gather's row routine (the same statements in the same order)."""
    H = T.shape[1]
    bias = np.zeros(H) if b0 is None else np.asarray(b0, dtype=np.float64)
    tr = (lambda c: int(c)) if xrow is None else (lambda c: int(xrow[c]))
    out = {}
    for r in need:
        n0, n1 = rowptr[r], rowptr[r + 1]
        d = int(n1 - n0)
        nodes = [tr(col[e]) for e in range(n0, n1)]
        l, a = 0.0, np.zeros(H)
        herr = np.zeros(H)
        if d:
            s = _see(watch, "s", a_src0[nodes] + a_dst0[tr(r)])
            e = _see(watch, "e", lrelu(s, slope0))
            m = e.max()
            arg = _see(watch, "arg", e - m)
            p = _see(watch, "p", _exp(arg, f32_elu))
            for k in range(d):
                l = _see(watch, "l", l + p[k])
                a = _see(watch, "a", p[k] * T[nodes[k]] + a)
            inv = _see(watch, "inv", 1.0 / l)
            alpha = p / l
            theta = (1 + (s <= 0)) * np.abs(e) + np.abs(arg) + 2
            absT = np.abs(T[nodes])
            A = a * inv
            herr = ((alpha * theta) @ absT + np.abs(A) * float(alpha @ theta) + d * (alpha @ absT) + (d + 2) * np.abs(A)
                    + TINY * absT.sum(0))
        else:
            inv = 0.0
        pre = _see(watch, "pre", a * inv + bias)
        h = _see(watch, "h", elu(pre, f32_elu))
        if d:
            herr = herr + np.abs(pre)
        herr = herr + 2 * np.abs(h) * (pre <= 0)
        out[int(r)] = (h, herr)
    return out


def hops(rowptr, col, T, a_src0, a_dst0, u_src, u_dst, seg, prow, pptr, xrow=None, b0=None, slope0=0.2, slope1=0.2, watch=None, sums=False,
         f32_elu=False):
    """G [P, H] float64.  sums=True: also B [P, H], the first-order error bound of every entry in units of 2^-24 (module docstring)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    T, a_src0, a_dst0, u_src, u_dst = (np.asarray(a, dtype=np.float64) for a in (T, a_src0, a_dst0, u_src, u_dst))
    seg = np.asarray(seg, dtype=np.int64).reshape(-1, 2)
    H = T.shape[1]
    ns = slots(H)
    lip = max(1.0, abs(slope1))
    need = sorted({r for r0, r1 in seg for r in range(r0, r1)})
    rows = layer0(rowptr, col, T, a_src0, a_dst0, need, xrow, b0, slope0, watch, f32_elu)
    ds, dd, dcs, dcd = {}, {}, {}, {}
    for r in need:   # the window's two float arrays: both dots of every row, once
        h, herr = rows[r]
        ds[r] = _see(watch, "ds", lane_dot(u_src, h, watch))
        dd[r] = _see(watch, "dd", lane_dot(u_dst, h, watch))
        dcs[r] = (4 * ns + 6) * np.abs(u_src * h).sum() + np.abs(u_src) @ herr
        dcd[r] = (4 * ns + 6) * np.abs(u_dst * h).sum() + np.abs(u_dst) @ herr
    G, B = np.zeros((len(prow), H)), np.zeros((len(prow), H))
    for i, (r0, r1) in enumerate(seg):
        for j in range(pptr[i], pptr[i + 1]):
            r = int(prow[j])
            assert r0 <= r < r1, "a pooled row outside its graph's range"
            ents = [int(c) for c in col[rowptr[r]:rowptr[r + 1]]]
            assert all(r0 <= c < r1 for c in ents), "a column outside the graph's range: the view is not block-diagonal"
            D = len(ents)
            if D == 0:
                continue
            s = _see(watch, "s1", np.array([ds[c] for c in ents]) + dd[r])
            f = _see(watch, "f", lrelu(s, slope1))
            m = f.max()
            arg = _see(watch, "arg1", f - m)
            p = _see(watch, "p1", _exp(arg, f32_elu))
            l, g = 0.0, np.zeros(H)
            for k, c in enumerate(ents):
                l = _see(watch, "l1", l + p[k])
                g = _see(watch, "g", p[k] * rows[c][0] + g)
            inv = _see(watch, "inv1", 1.0 / l)
            G[j] = _see(watch, "G", g * inv)
            if sums:
                beta = p / l
                absH = np.abs(np.stack([rows[c][0] for c in ents]))
                herrs = np.stack([rows[c][1] for c in ents])
                phi = lip * (np.array([dcs[c] for c in ents]) + dcd[r] + np.abs(s)) + (s <= 0) * np.abs(f) + np.abs(arg) + 2
                B[j] = ((beta * phi) @ absH + np.abs(G[j]) * float(beta @ phi) + beta @ herrs + D * (beta @ absH) + (D + 3) * np.abs(G[j])
                        + TINY * absH.sum(0))
    return (G, B) if sums else G


def run(c, **kw):
    """hops() on a case dict."""
    return hops(c["rowptr"], c["col"], c["T"], c["a_src0"], c["a_dst0"], c["u_src"], c["u_dst"], c["seg"], c["prow"], c["pptr"], xrow=c["xrow"],
                b0=c["b0"], slope0=c["slope0"], slope1=c["slope1"], **kw)


def run_rows(c, **kw):
    """gat_query_reference.gather (the per-row kernel's order) on the case's pooled rows."""
    return gq.gather(c["rowptr"], c["col"], c["T"], c["a_src0"], c["a_dst0"], c["u_src"], c["u_dst"], c["prow"], xrow=c["xrow"], b0=c["b0"],
                     slope0=c["slope0"], slope1=c["slope1"], **kw)


def max_rows(H):
    """The window arithmetic: max_rows (H + 2) floats within 160 KiB."""
    return (160 * 1024) // (4 * (H + 2))


# ---- the float64 forward the reference is proven against ----
def model_forward(gorc, sd, x, edge_index, seg, prow, pptr, pool, softmax, slopes=(0.2, 0.2)):
    """The float64 model: gat_query_reference.oracle_forward's stack on the whole view (its node head switched off by an identity lt1),
    then per queried graph the pool over its pooled rows, the head and the softmax (network.py's Classify_graph_* / Regress_graph_* in
    eval mode).  sd: the model's state dict (torch tensors)."""
    import torch
    H2 = sd["lt1.weight"].shape[1]
    stack = dict(sd)
    stack["lt1.weight"], stack["lt1.bias"] = torch.eye(H2, dtype=torch.float64), torch.zeros(H2, dtype=torch.float64)
    z = gq.oracle_forward(gorc, stack, x, edge_index, slopes, log_softmax=False).numpy()
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
# (H, with_xrow, with_b0): 16 (four live lanes), 64, 256 (one full slot, <1>), 260 (second slot, one live lane, <2>), 512 (both full)
EXACT_HOPS_CASES = [(16, False, True), (64, True, False), (256, False, False), (260, True, True), (512, False, True)]
HOPS_SIZES = [1, 2, 3, 4, 5, 18]                  # waves with none, one or two rows; more rows than one round of the waves
HOPS_GRAPHS = [5, 0, 3, 1, 5, 4, 2]               # unsorted, one graph twice
HOPS_KINDS = ["all", "all", "first", "subset", "subset", "none", "all"]
UNIFORM_ROW_DEGS = [0, 1, 64, 2, 128, 4]          # powers of two: l = the degree and 1 / l are exact
ROW_DEGS = [0, 1, 64, 65, 130, 2, 5]              # a second and a third 64-entry batch


def _finish(rng, d, gptr, graphs=HOPS_GRAPHS, kinds=HOPS_KINDS):
    seg, prow, pptr = gr.pooled_rows(rng, gptr, graphs, kinds)
    d.update(seg=seg, prow=prow, pptr=pptr, gptr=gptr, max_rows=int((seg[:, 1] - seg[:, 0]).max()))
    return d


def exact_uniform_case(H, with_xrow, with_b0):
    """All four attention vectors zero: every score is 0, every weight exp(0) = 1 and l the degree -- a power of two, so 1 / l is exact;
    T in {0..8}/8 with the column trick of query_reference.exact_gather_inputs.  h_r is a multiple of 1/1024 in [0, 2] or exactly -1 and
    a sum of up to 128 of them takes 18 bits: every intermediate is exact in any order.  The graphs of HOPS_SIZES with every degree of
    UNIFORM_ROW_DEGS, queried unsorted with one graph twice, pooled rows of every kind."""
    rng = np.random.default_rng([H, int(with_xrow), int(with_b0), 61])
    n_table = 37
    rowptr, col, _, xrow, gptr = gr.graph_view(rng, HOPS_SIZES, UNIFORM_ROW_DEGS, n_table, with_xrow, pow2_val=True)
    nt = n_table if with_xrow else int(gptr[-1])
    T, b0 = qr.exact_gather_inputs(rng, H, nt, with_b0)
    z, zH = np.zeros(nt, dtype=np.float32), np.zeros(H, dtype=np.float32)
    return _finish(rng, dict(rowptr=rowptr, col=col, xrow=xrow, T=T, b0=b0, a_src0=z, a_dst0=z.copy(), u_src=zH, u_dst=zH.copy(), slope0=0.2,
                             slope1=0.2), gptr)


LO, BIG, CSTAR, CQ = gq.LO, gq.BIG, gq.CSTAR, gq.CQ
SELECTOR_SLOPES = gq.SELECTOR_SLOPES
SELECTOR_SIZES = [1, 2, 3, 4, 9, 18]
SELECTOR_HI_DEGS = [1, 64, 65, 130, 2, 5]         # rows of a large graph whose entries are looked at: never without entries
SELECTOR_LO_DEGS = [0, 1, 65, 3, 130, 64]
SELECTOR_SMALL_DEGS = [0, 1, 2, 64, 4]            # a graph too small for three kinds of row: every entry of a row is the same column


def exact_selector_case(H, with_xrow, with_b0=True):
    """Scores that select, at both layers, through the ONE CSR row both layers of a graph read.  A TABLE row has a class: A and B win
    at layer 0 (a0s = 0), Z loses (a0s = -LO: >= 448 below after the LeakyReLU); T[., CSTAR] is BIG for A and 0 for B.  u_src = e_CSTAR, so
    ds_r = h_r[CSTAR] is BIG for a row whose layer-0 winners are all of class A (kind "hi") and 0 for a row whose winners are all of class
    B or that has no entries (kind "lo"): a hi column lies BIG above a lo column at layer 1, >= 1024 after the LeakyReLU.  In a graph
    of >= 9 rows row k is (A, hi), (B, hi) or (Z, lo) by k % 3.  A row with d entries takes a power-of-two count c <= d of winners --
    (A, hi) rows for a hi row, (B, hi) rows for a lo row -- and d - c (Z, lo) rows: the same c entries win at BOTH layers, tie at
    exp(0) = 1, every other weight underflows to exactly 0, l = c and 1 / l are exact, and h and g are power-of-two means.
    u_dst = -2 e_CQ with T[., CQ] a positive multiple of 2048 puts dd_r in [-16384, -4096] and f on both sides of 0.  a0d takes a
    distinct multiple of 1/2 in [-64, 64] per table row.  In a graph of fewer rows all entries of a row name one column and tie
    (degrees are powers of two).  Without xrow the table row is the view row; with it, xrow picks a table row of the wanted class."""
    rng = np.random.default_rng([H, int(with_xrow), int(with_b0), 67])
    gptr = np.concatenate([[0], np.cumsum(SELECTOR_SIZES)]).astype(np.int64)
    n_rows = int(gptr[-1])
    nt = 37 if with_xrow else n_rows
    want = np.zeros(n_rows, dtype=np.int64)                   # the class of the row's table row: 0 = A, 1 = B, 2 = Z
    rowptr, col = [0], []
    for g, n in enumerate(SELECTOR_SIZES):
        r0 = int(gptr[g])
        role = np.arange(n) % 3
        want[r0:r0 + n] = role if n >= 9 else rng.integers(0, 3, size=n)
        for k in range(n):
            if n < 9:
                d = SELECTOR_SMALL_DEGS[(k + g) % len(SELECTOR_SMALL_DEGS)]
                col += [int(rng.integers(r0, r0 + n))] * d
            else:
                degs = SELECTOR_LO_DEGS if role[k] == 2 else SELECTOR_HI_DEGS
                d = degs[(k // 3) % len(degs)]
                if d:
                    c = 1 << int(rng.integers(0, d.bit_length()))        # a power of two <= d
                    win = r0 + np.nonzero(role == (1 if role[k] == 2 else 0))[0]
                    lose = r0 + np.nonzero(role == 2)[0]
                    col += rng.permutation(np.concatenate([rng.choice(win, size=c), rng.choice(lose, size=d - c)])).tolist()
            rowptr.append(len(col))
    rowptr, col = np.array(rowptr, dtype=np.int32), np.array(col, dtype=np.int32)
    if with_xrow:
        cls_t = np.arange(nt) % 3
        xrow = np.array([rng.choice(np.nonzero(cls_t == w)[0]) for w in want], dtype=np.int32)
        xrow[col[-1]] = nt - 1 - (nt - 1 - want[col[-1]]) % 3          # one entry at (one of) the last table rows of its class
    else:
        cls_t, xrow = want, None
    T, b0 = qr.exact_gather_inputs(rng, H, nt, with_b0)
    T[:, CSTAR] = np.where(cls_t == 0, BIG, np.where(cls_t == 1, 0.0, rng.choice([0.0, BIG], size=nt)))
    T[:, CQ] = 2048.0 * rng.integers(1, 5, size=nt)
    a_src0 = np.where(cls_t == 2, -LO, 0.0).astype(np.float32)
    a_dst0 = (rng.permutation(257)[:nt] - 128).astype(np.float32) / 2.0
    u_src, u_dst = np.zeros(H, dtype=np.float32), np.zeros(H, dtype=np.float32)
    u_src[CSTAR], u_dst[CQ] = 1.0, -2.0
    if b0 is not None:
        b0[CSTAR] = b0[CQ] = 0.0
    return _finish(rng, dict(rowptr=rowptr, col=col, xrow=xrow, T=T.astype(np.float32), b0=b0, a_src0=a_src0, a_dst0=a_dst0, u_src=u_src,
                             u_dst=u_dst, slope0=SELECTOR_SLOPES[0], slope1=SELECTOR_SLOPES[1]), gptr)


EXACT_GENERATORS = {"uniform": exact_uniform_case, "selector": exact_selector_case}
SPREADS = ["unit", "wide", "underflow"]


def random_case(H, with_xrow, with_b0, spread, sizes=HOPS_SIZES, degs=ROW_DEGS, graphs=HOPS_GRAPHS, kinds=HOPS_KINDS):
    """Scores of ordinary size ("unit": a0s, a0d ~ N(0, 1), u ~ N(0, 1) / sqrt(H) on h of size 1), ten times wider ("wide": spreads of
    some tens within a row, most weights small but alive) or, as tests/test_gpu_gat_query_kernels.py draws them, with some table rows'
    a0s lowered by 1200 and one column of T scaled so that the scores of a row differ by more than 200 at both layers ("underflow")."""
    rng = np.random.default_rng([H, int(with_xrow), int(with_b0), SPREADS.index(spread), 71])
    n_table = 41
    rowptr, col, _, xrow, gptr = gr.graph_view(rng, sizes, degs, n_table, with_xrow, pow2_val=False)
    nt = n_table if with_xrow else int(gptr[-1])
    f = lambda *s: rng.normal(0, 1, size=s).astype(np.float32)   # noqa: E731
    T, a_src0, a_dst0 = f(nt, H), f(nt), f(nt)
    u_src, u_dst = (f(H) / np.sqrt(H)).astype(np.float32), (f(H) / np.sqrt(H)).astype(np.float32)
    if spread == "wide":
        a_src0, u_src = a_src0 * np.float32(10), u_src * np.float32(10)
    elif spread == "underflow":
        a_src0[::3] -= 1200.0
        T[::2, 1] *= 1000.0
        u_src[1] = 8.0
    b0 = f(H) if with_b0 else None
    return _finish(rng, dict(rowptr=rowptr, col=col, xrow=xrow, T=T, b0=b0, a_src0=a_src0, a_dst0=a_dst0, u_src=u_src, u_dst=u_dst, slope0=0.2,
                             slope1=0.3), gptr, graphs, kinds)


def score_spreads(c):
    """(largest spread of the layer-0 scores within a row, of the layer-1 scores within a pooled row) from the reference's intermediates."""
    spread = {"e": 0.0, "f": 0.0}

    def watch(name, a):
        if name in spread and np.size(a):
            spread[name] = max(spread[name], float(np.max(a) - np.min(a)))
    run(c, watch=watch)
    return spread["e"], spread["f"]


def window_case(H, n_rows, exact=True):
    """A graph of 3 rows, one of n_rows rows (small degrees: the reference walks every entry) and another of 2, every row pooled,
    queried large, small, small.  EXACT: the uniform case's draws with degrees 0, 1, 2, 4."""
    rng = np.random.default_rng([H, n_rows, int(exact), 73])
    rowptr, col, _, _, gptr = gr.graph_view(rng, [3, n_rows, 2], [[1, 2], [0, 1, 2, 4, 1], [2, 1]], 1, False, pow2_val=True)
    n = int(gptr[-1])
    if exact:
        T, b0 = qr.exact_gather_inputs(rng, H, n, True)
        z, zH = np.zeros(n, dtype=np.float32), np.zeros(H, dtype=np.float32)
        d = dict(T=T, b0=b0, a_src0=z, a_dst0=z.copy(), u_src=zH, u_dst=zH.copy(), slope0=0.2, slope1=0.2)
    else:
        f = lambda *s: rng.normal(0, 1, size=s).astype(np.float32)   # noqa: E731
        d = dict(T=f(n, H), b0=f(H), a_src0=f(n), a_dst0=f(n), u_src=(f(H) / np.sqrt(H)).astype(np.float32),
                 u_dst=(f(H) / np.sqrt(H)).astype(np.float32), slope0=0.2, slope1=0.3)
    d.update(rowptr=rowptr, col=col, xrow=None)
    d = _finish(rng, d, gptr, [1, 0, 2], ["all"])
    d["max_rows"] = n_rows
    return d
