"""float64 reference of the multi-head attention query kernel (csrc/query.hip, fitgnn_mhgat_query_gather_f32) in the kernel's stated
operation order, the block-expanded W1 of its tail's test, a float64 two-layer multi-head GAT forward composed from the oracle, and
the input generators the CPU and GPU tests share (test infrastructure only; the conventions of tests/gat_query_reference.py).

H = heads C0 columns; hd(c) = c // C0 is the head of column c.  The order is gat_query_reference's, head by head:

row r    per head hd: s = a0s[t(k)][hd] + a0d[t(r)][hd]; e = s > 0 ? s : slope0 s; m = max_k e; p_k = exp(e_k - m).  Over the entries in
         CSR order, column c with ITS head's weights: l = l + p_k, a = p_k T[t(k)][c] + a; h = ELU(a (1 / l) + b0[c]); a row without
         entries: ELU(b0).  (The kernel hands a lane its head's p_k through an LDS tile: the float the single-head kernel broadcasts by
         v_readlane, no rounding more or less.)
dot      gat_query_reference.lane_dot over ALL H columns, once per head with U[hd].
query q  h_q from row q itself, c_q[hd] = U_d[hd] . h_q.  Entry i of row q (CSR order) belongs to wave i % 4, folded in ascending i
         into one state (M, L, P) per head, P [H] wide: f = lrelu((U_s[hd] . h_j) + c_q[hd], slope1) and the two branches of
         gat_query_reference.
merge    per head, over the waves ascending; G[q][hd H + c] = P[c] (1 / L).  A query without entries gives zeros over heads H.

`watch`, f32_elu and sums are gat_query_reference.gather's; before each head's fold at layer 1 watch also receives ("head", hd).

The error bound of gather(sums=True) is gat_query_reference's derivation, restated head by head (u = 2^-24; one rounding of a result
x costs at most u |x|; expf, expm1f and the division within 1 ulp = 2 u |x|; first order in u):

  layer 0, row r of degree d, column c of head g = hd(c).  In head g: s rounds once and passes LeakyReLU with slope 1 (s > 0) or
  through one more rounded product (s <= 0); the value of m matters only through the rounding of e_k - m; expf adds 2:
      Theta_k = (1 + [s_k <= 0]) |e_k| + |e_k - m| + 2            (all of head g)
  and the computed weight is p_k (1 + theta_k), |theta_k| <= Theta_k u; alpha_k = p_k / l (head g) moves by at most the weight times
  the error on either side, so A_c = sum_k alpha_k T_kc moves by sum_k alpha_k Theta_k |T_kc| + |A_c| sum_k alpha_k Theta_k.  The d
  fmafs of a add d sum_k alpha_k |T_kc|; the d additions of l, the division and the final fmaf (d + 2) |A_c| + |pre_c|; ELU has slope
  <= 1 and expm1f adds 2 |h_c| where pre_c <= 0:
      herr_c(r) = sum_k alpha_k Theta_k |T_kc| + |A_c| sum_k alpha_k Theta_k + d sum_k alpha_k |T_kc| + (d + 2) |A_c| + |pre_c|
                  + 2 |h_c| [pre_c <= 0] + tiny sum_k |T_kc|          (alpha, Theta: those of column c's own head)

  score dots, per head g with u = U[g]: dc_j = (4 NS + 6) sum_c |u_c h_jc| + sum_c |u_c| herr_c(j) over ALL columns c (each with its
  own head's herr); likewise dc_q with U_d[g] and h_q.

  layer 1, query q of degree D, n = ceil(D / 4), per head g: f_j = lrelu(c_j + c_q), werr_j as in gat_query_reference (its own
  |f_j - M| + 2, every later rescaling of its wave, |M_w - M| + 2 at the merge), all of head g's state:
      Phi_j = max(1, |slope1|) (dc_j + dc_q + |s_j|) + [s_j <= 0] |f_j| + werr_j
      B[g H + c](q) = sum_j beta_j Phi_j |h_jc| + |G_c| sum_j beta_j Phi_j + sum_j beta_j herr_c(j)
                      + (n + 4) sum_j beta_j |h_jc| + (n + 7) |G_c| + tiny sum_j |h_jc|          (beta, Phi: head g's; G_c = G[g H + c])
"""
import numpy as np

import gat_query_reference as gq
import query_reference as qr
from gat_query_reference import LANES, TINY, WAVES, _exp, lane_dot, lrelu, slots  # noqa: F401
from query_reference import _see, elu


def gather(rowptr, col, T, a_src0, a_dst0, U_src, U_dst, rows, xrow=None, b0=None, slope0=0.2, slope1=0.2, watch=None, sums=False,
           f32_elu=False):
    """G [Q, heads H] float64.  sums=True: also B of that shape, the first-order error bound of every entry in units of 2^-24."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    T, a_src0, a_dst0, U_src, U_dst = (np.asarray(a, dtype=np.float64) for a in (T, a_src0, a_dst0, U_src, U_dst))
    H = T.shape[1]
    heads = U_src.shape[0]
    assert a_src0.shape[1] == heads and a_dst0.shape[1] == heads and U_src.shape == (heads, H) == U_dst.shape and H % heads == 0
    hdc = np.arange(H) // (H // heads)
    ns = slots(H)
    bias = np.zeros(H) if b0 is None else np.asarray(b0, dtype=np.float64)
    tr = (lambda c: int(c)) if xrow is None else (lambda c: int(xrow[c]))
    lip = max(1.0, abs(slope1))
    cache = {}

    def row(r):
        if r in cache:
            return cache[r]
        n0, n1 = rowptr[r], rowptr[r + 1]
        d = int(n1 - n0)
        nodes = [tr(col[e]) for e in range(n0, n1)]
        l, a = np.zeros(heads), np.zeros(H)
        herr = np.zeros(H)
        if d:
            s = _see(watch, "s", a_src0[nodes] + a_dst0[tr(r)][None, :])       # [d, heads]
            e = _see(watch, "e", lrelu(s, slope0))
            m = e.max(0)
            arg = _see(watch, "arg", e - m[None, :])
            p = _see(watch, "p", _exp(arg, f32_elu))
            for k in range(d):
                l = _see(watch, "l", l + p[k])
                a = _see(watch, "a", p[k][hdc] * T[nodes[k]] + a)
            inv = _see(watch, "inv", 1.0 / l)[hdc]
            alpha = (p / l[None, :])[:, hdc]                                    # [d, H]: each column with its head's weights
            theta = ((1 + (s <= 0)) * np.abs(e) + np.abs(arg) + 2)[:, hdc]
            absT = np.abs(T[nodes])
            A = a * inv
            at = (alpha * theta).sum(0)
            herr = ((alpha * theta * absT).sum(0) + np.abs(A) * at + d * (alpha * absT).sum(0) + (d + 2) * np.abs(A) + TINY * absT.sum(0))
        else:
            inv = np.zeros(H)
        pre = _see(watch, "pre", a * inv + bias)
        h = _see(watch, "h", elu(pre, f32_elu))
        if d:
            herr = herr + np.abs(pre)
        herr = herr + 2 * np.abs(h) * (pre <= 0)
        cache[r] = (h, herr)
        return cache[r]

    G = np.zeros((len(rows), heads * H))
    B = np.zeros((len(rows), heads * H))
    for i, q in enumerate(np.asarray(rows, dtype=np.int64)):
        e0, e1 = rowptr[q], rowptr[q + 1]
        D = int(e1 - e0)
        if D == 0:
            continue
        hq, hqerr = row(int(q))
        nbrs = [row(int(col[e])) for e in range(e0, e1)]
        for g in range(heads):
            _see(watch, "head", np.float64(g))
            u_src, u_dst = U_src[g], U_dst[g]
            cq = _see(watch, "cq", lane_dot(u_dst, hq, watch))
            dcq = (4 * ns + 6) * np.abs(u_dst * hq).sum() + np.abs(u_dst) @ hqerr
            M = [-np.inf] * WAVES
            Lw = [0.0] * WAVES
            P = [np.zeros(H) for _ in range(WAVES)]
            ents = [[] for _ in range(WAVES)]     # per wave: [entry index k, accumulated log-weight error]
            info = []                             # per entry: (f, s, dc)
            for k, (h, herr) in enumerate(nbrs):
                w = k % WAVES
                cj = _see(watch, "cj", lane_dot(u_src, h, watch))
                dcj = (4 * ns + 6) * np.abs(u_src * h).sum() + np.abs(u_src) @ herr
                sj = _see(watch, "s1", cj + cq)
                f = float(_see(watch, "f", lrelu(sj, slope1)))
                info.append((f, sj, dcj))
                if f > M[w]:
                    first = not np.isfinite(M[w])
                    x = float(_see(watch, "x", _exp(_see(watch, "x_arg", M[w] - f), f32_elu)))
                    step = 0.0 if first else abs(M[w] - f) + 2
                    Lw[w] = _see(watch, "L", Lw[w] * x + 1.0)
                    P[w] = _see(watch, "P", P[w] * x + h)
                    for ent in ents[w]:
                        ent[1] += step
                    ents[w].append([k, 0.0])
                    M[w] = f
                else:
                    x = float(_see(watch, "x", _exp(_see(watch, "x_arg", f - M[w]), f32_elu)))
                    Lw[w] = _see(watch, "L", Lw[w] + x)
                    P[w] = _see(watch, "P", x * h + P[w])
                    ents[w].append([k, abs(f - M[w]) + 2])
            Mx = max(M)
            Ls, acc = 0.0, np.zeros(H)
            werr = np.zeros(D)
            for w in range(WAVES):
                x = float(_see(watch, "x", _exp(_see(watch, "x_arg", M[w] - Mx), f32_elu)))
                Ls = _see(watch, "L", x * Lw[w] + Ls)
                acc = _see(watch, "P", x * P[w] + acc)
                for k, err in ents[w]:
                    werr[k] = err + abs(M[w] - Mx) + 2
            inv = _see(watch, "inv", 1.0 / Ls)
            Gg = _see(watch, "g", acc * inv)
            G[i, g * H:(g + 1) * H] = Gg
            if sums:
                f = np.array([t[0] for t in info])
                beta = _exp(f - f.max(), False)
                beta = beta / beta.sum()
                absH = np.abs(np.stack([t[0] for t in nbrs]))
                herrs = np.stack([t[1] for t in nbrs])
                s1 = np.array([t[1] for t in info])
                dc = np.array([t[2] for t in info])
                phi = lip * (dc + dcq + np.abs(s1)) + (s1 <= 0) * np.abs(f) + werr
                n = -(-D // WAVES)
                B[i, g * H:(g + 1) * H] = ((beta * phi) @ absH + np.abs(Gg) * float(beta @ phi) + beta @ herrs + (n + 4) * (beta @ absH)
                                           + (n + 7) * np.abs(Gg) + TINY * absH.sum(0))
    return (G, B) if sums else G


def tail_expanded(W1, heads):
    """W1big [H2, heads H]: row n holds W1[n, :] at columns hd1(n) H .., hd1(n) = n // (H2 // heads), zeros elsewhere."""
    W1 = np.asarray(W1)
    H2, H = W1.shape
    C1 = H2 // heads
    big = np.zeros((H2, heads * H), dtype=W1.dtype)
    for g in range(heads):
        big[g * C1:(g + 1) * C1, g * H:(g + 1) * H] = W1[g * C1:(g + 1) * C1]
    return big


def u_vectors(W1, att, heads):
    """U [heads, H] float64: U[hd] = W1[hd C1 : (hd + 1) C1, :]^T att[hd]."""
    W1 = np.asarray(W1, dtype=np.float64)
    C1 = W1.shape[0] // heads
    att = np.asarray(att, dtype=np.float64).reshape(heads, C1)
    return np.stack([att[g] @ W1[g * C1:(g + 1) * C1] for g in range(heads)])


# ---- the float64 forward the reference is proven against ----
def oracle_forward(gorc, sd, x, edge_index, heads, slopes=(0.2, 0.2), log_softmax=True):
    """network.py:29-35 in eval mode with two GATConv(heads, concat=True) layers: each layer is the concatenation over the heads of
    oracle.gnn_oracle.gat_conv on that head's block of W, att and bias, in float64 (torch tensors)."""
    import torch
    x = x.double()
    for i in range(2):
        p = f"conv.{i}."
        W, bias = sd[p + "lin.weight"].double(), sd[p + "bias"].double()
        C = W.shape[0] // heads
        a_s, a_d = sd[p + "att_src"].double().reshape(heads, C), sd[p + "att_dst"].double().reshape(heads, C)
        x = torch.nn.functional.elu(torch.cat([gorc.gat_conv(x, edge_index, W[g * C:(g + 1) * C], a_s[g], a_d[g], bias[g * C:(g + 1) * C],
                                                             slopes[i]) for g in range(heads)], dim=1))
    y = x @ sd["lt1.weight"].double().t() + sd["lt1.bias"].double()
    return torch.log_softmax(y, dim=1) if log_softmax else y


# ---- inputs of the kernel tests ----
UNIFORM_QUERY_DEGS, UNIFORM_NEIGHBOUR_DEGS = gq.UNIFORM_QUERY_DEGS, gq.UNIFORM_NEIGHBOUR_DEGS
# (heads, H, with_xrow, with_b0): one live float4 per head; one slot, part full; a full slot; an odd head count with one live lane in the
# second slot; a head is a whole slot; both slots full -- xrow and b0 mixed as gat_query_reference.EXACT_GATHER_CASES mixes them
EXACT_GATHER_CASES = [(2, 8, False, True), (4, 64, True, False), (8, 256, False, False), (5, 260, True, True), (2, 512, False, True),
                      (8, 512, True, True)]
SELECTOR_SLOPES = gq.SELECTOR_SLOPES
LO, BIG = gq.LO, gq.BIG
CSTAR, CQ = 0, 2   # within every head's block of columns: the columns U_src[hd] and U_dst[hd] select


def exact_uniform_case(heads, H, with_xrow, with_b0):
    """gat_query_reference.exact_uniform_case with all four attention arrays zero in every head: every weight is exp(0) = 1, l the
    degree (a power of two) in every head, and every block of G is the same exact mean."""
    rng = np.random.default_rng([heads, H, int(with_xrow), int(with_b0), 23])
    n_table = 37
    rowptr, col, _, xrow, n_rows = qr.query_csr(rng, UNIFORM_QUERY_DEGS, UNIFORM_NEIGHBOUR_DEGS, n_table, with_xrow, pow2_val=True)
    nt = n_table if with_xrow else n_rows
    T, b0 = qr.exact_gather_inputs(rng, H, nt, with_b0)
    z = np.zeros((nt, heads), dtype=np.float32)
    zH = np.zeros((heads, H), dtype=np.float32)
    return dict(rowptr=rowptr, col=col, xrow=xrow, T=T, b0=b0, a_src0=z, a_dst0=z.copy(), U_src=zH, U_dst=zH.copy(), slope0=0.2, slope1=0.2,
                rows=np.arange(len(UNIFORM_QUERY_DEGS), dtype=np.int64), n_rows=n_rows, heads=heads)


def exact_selector_case(heads, H, with_xrow, with_b0=True):
    """Scores that select, differently per head.  The rows and degrees are query_reference.query_csr's; the columns are re-pointed.

    The heads fall into two groups, i = hd % 2.  A TABLE row t has a type t % 3: type i wins at layer 0 in the heads of group i
    (a0s[t][hd] = 0) and loses in the other group's (a0s = -LO); type 2 loses in every head.  It also carries a flag A / B per group,
    F[t][i]: T[t][hd C0 + CSTAR] is BIG where F[t][hd % 2] = A and 0 otherwise.  A row with d >= 2 entries gets a power-of-two count
    of type-0 entries and a power-of-two count of type-1 entries (both >= 1) and type-2 entries otherwise; within a row the type-i
    entries all carry the same flag F[.][i].  In a head of group i the type-i entries tie at exp(0) = 1 and every other weight
    underflows to exactly 0: h_r[hd C0 + CSTAR] is BIG or 0, the flag of the row's type-i entries, and all of the head's block is a
    power-of-two mean of table rows -- another set of table rows in the other group's heads.  A neighbour row of type i with entries
    takes flag A for its type-i entries and B for the others (type 2: B for both; a row with ONE entry points at a table row with
    those two flags; a row without entries has h = ELU(b0) = 0 there: B for both).  A query with D >= 2 entries takes a power-of-two
    count of type-0 neighbour rows with entries, a power-of-two count of type-1 ones and type-2 rows otherwise, so in a head of
    group i the type-i entries win at BOTH layers: U_src[hd] = e_{hd C0 + CSTAR} puts them BIG above the others before the LeakyReLU,
    and U_dst[hd] = -2 e_{hd C0 + CQ} with T[., hd C0 + CQ] a positive multiple of 2048 puts c_q in [-16384, -4096], f on both sides
    of 0.  The even and the odd heads of a query therefore select different entries, at both layers.  a0s is read through xrow; a0d
    takes a multiple of 1/2 in [-64, 64] per table row AND head, on both sides of 0."""
    rng = np.random.default_rng([heads, H, int(with_xrow), int(with_b0), 29])
    n_table = 37
    C0 = H // heads
    q_degs, n_degs = qr.GATHER_QUERY_DEGS, qr.GATHER_NEIGHBOUR_DEGS
    rowptr, col, _, xrow, n_rows = qr.query_csr(rng, q_degs, n_degs, n_table, with_xrow, pow2_val=True)
    nq = len(q_degs)
    nt = n_table if with_xrow else n_rows
    last = int(col[-1])                                       # (with xrow: the union row that sits at the last table row)
    ty_t = np.arange(nt) % 3
    F_t = rng.integers(0, 2, size=(nt, 2))                    # 1 = A, 0 = B
    for i in range(2):                                        # a type's own flag alternates: both pools are there
        own = np.nonzero(ty_t == i)[0]
        F_t[own, i] = np.arange(len(own)) % 2
    tab = xrow if with_xrow else np.arange(n_rows)            # union row -> table row
    ty, F = ty_t[tab], F_t[tab]
    deg = np.diff(rowptr)
    rows_all = np.arange(n_rows)
    nb = np.arange(nq, n_rows)
    pool = {(i, a): rows_all[(ty == i) & (F[:, i] == a)] for i in range(2) for a in range(2)}
    pool_z = rows_all[ty == 2]
    want = {0: (1, 0), 1: (0, 1), 2: (0, 0)}                  # a neighbour row's flags by its own type
    cat = {i: nb[(ty[nb] == i) & (deg[nb] > 0)] for i in range(2)}
    cat_z = nb[ty[nb] == 2]
    assert all(len(p) for p in pool.values()) and len(pool_z) and all(len(c) for c in cat.values()) and len(cat_z)

    def pow2_pair(d):
        c = [1, 1]
        while True:
            i = int(rng.integers(0, 2))
            if c[0] + c[1] + c[i] > d or rng.integers(0, 4) == 0:
                return c
            c[i] *= 2

    col = col.copy()
    for r in range(n_rows):
        d = int(deg[r])
        if d == 0:
            continue
        if r < nq:
            src = (cat[0], cat[1], cat_z)
            one = np.concatenate(src)
        else:
            w = want[int(ty[r])]
            src = (pool[(0, w[0])], pool[(1, w[1])], pool_z)
            one = rows_all[(F[:, 0] == w[0]) & (F[:, 1] == w[1])]
            assert len(one)
        if d == 1:
            ent = rng.choice(one, size=1)
        else:
            c = pow2_pair(d)
            ent = np.concatenate([rng.choice(src[0], size=c[0]), rng.choice(src[1], size=c[1]), rng.choice(src[2], size=d - c[0] - c[1])])
        col[rowptr[r]:rowptr[r + 1]] = rng.permutation(ent)
    if with_xrow:   # keep one entry at the last table row: an entry of the same type and flags moves there
        same = np.nonzero((ty[col] == ty[last]) & (F[col] == F[last]).all(1) & (np.arange(len(col)) >= rowptr[nq]))[0]
        col[same[-1]] = last
    T, b0 = qr.exact_gather_inputs(rng, H, nt, with_b0)
    a_src0 = np.zeros((nt, heads), dtype=np.float32)
    U_src, U_dst = np.zeros((heads, H), dtype=np.float32), np.zeros((heads, H), dtype=np.float32)
    for g in range(heads):
        a_src0[:, g] = np.where(ty_t == g % 2, 0.0, -LO)
        T[:, g * C0 + CSTAR] = np.where(F_t[:, g % 2] == 1, BIG, 0.0)
        T[:, g * C0 + CQ] = 2048.0 * rng.integers(1, 5, size=nt)
        U_src[g, g * C0 + CSTAR] = 1.0
        U_dst[g, g * C0 + CQ] = -2.0
        if b0 is not None:
            b0[g * C0 + CSTAR] = b0[g * C0 + CQ] = 0.0
    a_dst0 = (rng.integers(-128, 129, size=(nt, heads)) / 2.0).astype(np.float32)
    return dict(rowptr=rowptr, col=col, xrow=xrow, T=T.astype(np.float32), b0=b0, a_src0=a_src0, a_dst0=a_dst0, U_src=U_src, U_dst=U_dst,
                slope0=SELECTOR_SLOPES[0], slope1=SELECTOR_SLOPES[1], rows=np.arange(nq, dtype=np.int64), n_rows=n_rows, heads=heads)


EXACT_GENERATORS = {"uniform": exact_uniform_case, "selector": exact_selector_case}


def run(c, rows=None, **kw):
    """gather() on a case dict."""
    return gather(c["rowptr"], c["col"], c["T"], c["a_src0"], c["a_dst0"], c["U_src"], c["U_dst"], c["rows"] if rows is None else rows,
                  xrow=c["xrow"], b0=c["b0"], slope0=c["slope0"], slope1=c["slope1"], **kw)


def single_head_case(c, g, scores_of=0):
    """The gat_query_reference case dict of head g's layer 1 on head `scores_of`'s layer-0 scores."""
    d = dict(c)
    d.update(a_src0=np.ascontiguousarray(c["a_src0"][:, scores_of]), a_dst0=np.ascontiguousarray(c["a_dst0"][:, scores_of]),
             u_src=np.ascontiguousarray(c["U_src"][g]), u_dst=np.ascontiguousarray(c["U_dst"][g]))
    return d


def selected_entries(c, **kw):
    """{(query, head): frozenset of the entry positions whose layer-1 score is the head's largest in the query} from the reference's
    intermediates: in the selector case the entries that carry all of the head's weight."""
    out, st = {}, {"q": -1, "g": None, "f": None}

    def flush():
        if st["f"]:
            f = np.array(st["f"])
            out[(st["q"], st["g"])] = frozenset(np.nonzero(f == f.max())[0].tolist())

    def watch(name, a):
        if name == "head":
            flush()
            if int(a) == 0:
                st["q"] += 1
            st["g"], st["f"] = int(a), []
        elif name == "f":
            st["f"].append(float(a))
    run(c, watch=watch, **kw)
    flush()
    return out
