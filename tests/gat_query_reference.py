"""float64 reference of the attention query kernel (csrc/query.hip, fitgnn_gat_query_gather_f32) in the kernel's stated operation
order, a float64 two-layer GAT forward composed from the oracle, and the input generators the CPU and GPU tests share (test
infrastructure only; the conventions of tests/query_reference.py).

A wave holds a whole row: lane l owns columns 4 l .. 4 l + 3 and, for H > 256, 256 + 4 l .. 256 + 4 l + 3.

row r    s = a0s[t(k)] + a0d[t(r)]; e = s > 0 ? s : slope0 s; m = max_k e; p_k = exp(e_k - m); over the entries in CSR order
         l = l + p_k, a = p_k T[t(k)][c] + a; h = ELU(a (1 / l) + b0[c]); a row without entries: ELU(b0).
dot      u . h: per lane d = u[c] h[c] + d over its columns ascending, then d += d of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.
query q  h_q from row q itself, c_q = u_d . h_q.  Entry i of row q (CSR order) belongs to wave i % 4, folded in ascending i into
         (M, L, P) = (-inf, 0, 0): f = lrelu((u_s . h_j) + c_q, slope1); f > M: x = exp(M - f), L = L x + 1, P = P x + h_j, M = f;
         otherwise x = exp(f - M), L = L + x, P = x h_j + P.
merge    M = max_w M_w; x_w = exp(M_w - M); over w ascending L = x_w L_w + L, P = x_w P_w + P; g = P (1 / L).  A wave without
         entries holds (-inf, 0, 0); a query without entries gives zeros.

`watch` receives (name, array) for every intermediate, as in query_reference.  f32_elu rounds the results of ELU AND of exp to
float32: what a correctly rounded fp32 expm1f / expf returns where the EXACT inputs send them (ELU(x <= -32) = -1, exp(0) = 1,
exp(x <= -104) = 0: e^-104 = 6.8e-46 lies below half the smallest denormal, 7.0e-46).

The error bound of gather(sums=True), in units of u = 2^-24 (one rounding of a result x costs at most u |x|; expf, expm1f and the
division are taken within 1 ulp = 2 u |x|, as the HIP math API states), first order in u:

  layer 0, row r of degree d, column c.  s rounds once and passes LeakyReLU with slope 1 (s > 0) or through one more rounded
  product (s <= 0): |de_k| <= (1 + [s_k <= 0]) |e_k|.  A softmax does not see a common shift of its scores, so the value of m
  matters only through the rounding of e_k - m: |e_k - m|.  expf adds 2 to the weight's relative error.  With
      Theta_k = (1 + [s_k <= 0]) |e_k| + |e_k - m| + 2
  the computed weight is p_k (1 + theta_k), |theta_k| <= Theta_k u, and the normalised weight alpha_k = p_k / l moves by
  alpha_k (theta_k - sum_k' alpha_k' theta_k'): at most the weight itself times the error, on either side.  The sum
  A_c = sum_k alpha_k T_kc therefore moves by at most  sum_k alpha_k Theta_k |T_kc| + |A_c| sum_k alpha_k Theta_k.  The d fmafs of
  a add d sum_k alpha_k |T_kc|; the d additions of l, the division and the final fmaf's rounding (d + 2) |A_c| + |pre_c|.  ELU has
  slope <= 1 and expm1f adds 2 |h_c| where pre_c <= 0:
      herr_c(r) = sum_k alpha_k Theta_k |T_kc| + |A_c| sum_k alpha_k Theta_k + d sum_k alpha_k |T_kc| + (d + 2) |A_c| + |pre_c|
                  + 2 |h_c| [pre_c <= 0] + tiny sum_k |T_kc|
  (tiny = 2^-102 units = 2^-126 absolute: a weight below the smallest normal number may come back as 0.)

  score dots.  A lane's chain of 4 NS fmafs (NS = 1 for H <= 256, else 2) and the 6 butterfly additions round 4 NS + 6 times
  at most on any path: dc_j = (4 NS + 6) sum_c |u_c h_jc| + sum_c |u_c| herr_c(j); likewise dc_q with u_d and h_q.

  layer 1, query q of degree D, longest wave chain n = ceil(D / 4).  f_j = lrelu(c_j + c_q): one rounding of the sum (|s_j|), a
  Lipschitz constant max(1, |slope1|), one rounded product where s_j <= 0.  Every rescaling factor and every entry's own
  exp(f - M) multiplies L and P alike, so each enters an entry's weight once, with |argument| + 2 (the rounded difference and
  expf): werr_j = its own |f_j - M| + 2 (0 when it became the maximum: the weight is exactly 1) + the same for every later
  rescaling of its wave (none for the first, from -inf: exactly 0) + |M_w - M| + 2 at the merge.
      Phi_j = max(1, |slope1|) (dc_j + dc_q + |s_j|) + [s_j <= 0] |f_j| + werr_j
  and with beta_j = the true softmax weight, as at layer 0,
      B_c(q) = sum_j beta_j Phi_j |h_jc| + |g_c| sum_j beta_j Phi_j + sum_j beta_j herr_c(j)
               + (n + 4) sum_j beta_j |h_jc|         the wave's fmafs of P and the merge's four
               + (n + 7) |g_c|                       the same roundings of L, the division (2) and the final product
               + tiny sum_j |h_jc|.
"""
import numpy as np

import query_reference as qr
from query_reference import _see, elu

WAVES, LANES = 4, 64
TINY = 2.0 ** -102


def lrelu(x, slope):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x > 0, x, slope * x)


def _exp(x, f32):
    with np.errstate(under="ignore"):
        y = np.exp(np.asarray(x, dtype=np.float64))
        return y.astype(np.float32).astype(np.float64) if f32 else y


def slots(H):
    return 1 if H <= 256 else 2


def lane_dot(u, h, watch=None):
    """u . h in the kernel's order: per-lane chains over the lane's columns, then the xor butterfly 32, 16, 8, 4, 2, 1."""
    H = len(u)
    d = np.zeros(LANES)
    for s in range(slots(H)):
        for i in range(4):
            c = s * 256 + 4 * np.arange(LANES) + i
            cc = np.minimum(c, H - 1)
            d = _see(watch, "dot", np.where(c < H, u[cc] * h[cc], 0.0) + d)
    idx = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        d = _see(watch, "dot", d + d[idx ^ o])
    return float(d[0])


def gather(rowptr, col, T, a_src0, a_dst0, u_src, u_dst, rows, xrow=None, b0=None, slope0=0.2, slope1=0.2, watch=None, sums=False,
           f32_elu=False):
    """G [Q, H] float64.  sums=True: also B [Q, H], the first-order error bound of every entry in units of 2^-24 (module docstring)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    T, a_src0, a_dst0, u_src, u_dst = (np.asarray(a, dtype=np.float64) for a in (T, a_src0, a_dst0, u_src, u_dst))
    H = T.shape[1]
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
        cache[r] = (h, herr)
        return cache[r]

    G = np.zeros((len(rows), H))
    B = np.zeros((len(rows), H))
    for i, q in enumerate(np.asarray(rows, dtype=np.int64)):
        e0, e1 = rowptr[q], rowptr[q + 1]
        D = int(e1 - e0)
        if D == 0:
            continue
        hq, hqerr = row(int(q))
        cq = _see(watch, "cq", lane_dot(u_dst, hq, watch))
        dcq = (4 * ns + 6) * np.abs(u_dst * hq).sum() + np.abs(u_dst) @ hqerr
        M = [-np.inf] * WAVES
        Lw = [0.0] * WAVES
        P = [np.zeros(H) for _ in range(WAVES)]
        ents = [[] for _ in range(WAVES)]     # per wave: [entry index k, accumulated log-weight error]
        info = []                             # per entry: (h, herr, f, s, dc)
        for k, e in enumerate(range(e0, e1)):
            w = k % WAVES
            h, herr = row(int(col[e]))
            cj = _see(watch, "cj", lane_dot(u_src, h, watch))
            dcj = (4 * ns + 6) * np.abs(u_src * h).sum() + np.abs(u_src) @ herr
            sj = _see(watch, "s1", cj + cq)
            f = float(_see(watch, "f", lrelu(sj, slope1)))
            info.append((h, herr, f, sj, dcj))
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
        Ls, g = 0.0, np.zeros(H)
        werr = np.zeros(D)
        for w in range(WAVES):
            x = float(_see(watch, "x", _exp(_see(watch, "x_arg", M[w] - Mx), f32_elu)))
            Ls = _see(watch, "L", x * Lw[w] + Ls)
            g = _see(watch, "P", x * P[w] + g)
            for k, err in ents[w]:
                werr[k] = err + abs(M[w] - Mx) + 2
        inv = _see(watch, "inv", 1.0 / Ls)
        G[i] = _see(watch, "g", g * inv)
        if sums:
            f = np.array([t[2] for t in info])
            beta = _exp(f - f.max(), False)
            beta = beta / beta.sum()
            absH = np.abs(np.stack([t[0] for t in info]))
            herrs = np.stack([t[1] for t in info])
            s1 = np.array([t[3] for t in info])
            dc = np.array([t[4] for t in info])
            phi = lip * (dc + dcq + np.abs(s1)) + (s1 <= 0) * np.abs(f) + werr
            n = -(-D // WAVES)
            B[i] = ((beta * phi) @ absH + np.abs(G[i]) * float(beta @ phi) + beta @ herrs + (n + 4) * (beta @ absH) + (n + 7) * np.abs(G[i])
                    + TINY * absH.sum(0))
    return (G, B) if sums else G


# ---- the float64 forward the reference is proven against ----
def oracle_forward(gorc, sd, x, edge_index, slopes=(0.2, 0.2), log_softmax=True):
    """network.py:29-35 in eval mode with two GATConv layers, composed from oracle.gnn_oracle.gat_conv in float64 (torch tensors)."""
    import torch
    x = x.double()
    for i in range(2):
        p = f"conv.{i}."
        x = torch.nn.functional.elu(gorc.gat_conv(x, edge_index, sd[p + "lin.weight"].double(), sd[p + "att_src"].double().reshape(-1),
                                                  sd[p + "att_dst"].double().reshape(-1), sd[p + "bias"].double(), slopes[i]))
    y = x @ sd["lt1.weight"].double().t() + sd["lt1.bias"].double()
    return torch.log_softmax(y, dim=1) if log_softmax else y


# ---- inputs of the kernel tests ----
UNIFORM_QUERY_DEGS = [0, 1, 2, 4, 8, 16, 64, 128]
UNIFORM_NEIGHBOUR_DEGS = [0, 1, 2, 4, 64, 128, 256]
# (H, with_xrow, with_b0): the column slots of the kernel -- one live lane, one full slot, the second slot with one live lane, both full
EXACT_GATHER_CASES = [(4, False, True), (64, True, False), (256, False, False), (260, True, True), (512, False, True)]
SELECTOR_SLOPES = (0.5, 0.25)


def exact_uniform_case(H, with_xrow, with_b0):
    """All four attention vectors zero: every score is 0, every weight exp(0) = 1 and l the degree -- a power of two, so 1 / l is
    exact; T in {0..8}/8 with the column trick of query_reference.exact_gather_inputs.  Every intermediate is exact in any order."""
    rng = np.random.default_rng([H, int(with_xrow), int(with_b0), 23])
    n_table = 37
    rowptr, col, _, xrow, n_rows = qr.query_csr(rng, UNIFORM_QUERY_DEGS, UNIFORM_NEIGHBOUR_DEGS, n_table, with_xrow, pow2_val=True)
    nt = n_table if with_xrow else n_rows
    T, b0 = qr.exact_gather_inputs(rng, H, nt, with_b0)
    z = np.zeros(nt, dtype=np.float32)
    zH = np.zeros(H, dtype=np.float32)
    return dict(rowptr=rowptr, col=col, xrow=xrow, T=T, b0=b0, a_src0=z, a_dst0=z.copy(), u_src=zH, u_dst=zH.copy(), slope0=0.2, slope1=0.2,
                rows=np.arange(len(UNIFORM_QUERY_DEGS), dtype=np.int64), n_rows=n_rows)


LO = 1024.0      # a losing layer-0 score lies this far below a winner before the LeakyReLU: >= 480 below after it (slope 0.5, |a0d| <= 64)
BIG = 4096.0     # T in the selecting column: a layer-1 score of a type-A neighbour lies 4096 above the others, >= 1024 after slope 0.25
CSTAR, CQ = 0, 2   # the columns u_src and u_dst select


def exact_selector_case(H, with_xrow, with_b0=True):
    """Scores that select.  The rows and degrees are query_reference.query_csr's; the columns are re-pointed by class.  Every TABLE
    row has a class: A and B win at layer 0 (a0s = 0), Z loses (a0s = -LO); T[., CSTAR] is BIG for A, 0 for B.  A row with entries
    gets a power-of-two count of winners -- rows of class A all of class A, the others all of class B -- and class-Z rows otherwise:
    the winners tie at exp(0) = 1, a loser's exp underflows to exactly 0, so h_r[CSTAR] is BIG for a class-A row and 0 for every
    other, and all of h_r is a power-of-two mean of table rows.  A query's entries are a power-of-two count of class-A neighbour
    rows with entries and class-Z neighbour rows otherwise, so the same entries win at both layers: u_src = e_CSTAR, and
    u_dst = -2 e_CQ with T[., CQ] a positive multiple of 2048 puts c_q in [-16384, -4096], f on both sides of 0 and a type-A entry
    BIG above the others before the LeakyReLU.  a0s is read through xrow; a0d takes a distinct multiple of 1/2 in [-64, 64] per table
    row, on both sides of 0."""
    rng = np.random.default_rng([H, int(with_xrow), int(with_b0), 29])
    n_table = 37
    q_degs, n_degs = qr.GATHER_QUERY_DEGS, qr.GATHER_NEIGHBOUR_DEGS
    rowptr, col, _, xrow, n_rows = qr.query_csr(rng, q_degs, n_degs, n_table, with_xrow, pow2_val=True)
    nq = len(q_degs)
    nt = n_table if with_xrow else n_rows
    last = int(col[-1])                                       # (with xrow: the union row that sits at the last table row)
    cls_t = np.arange(nt) % 3                                 # 0 = A, 1 = B, 2 = Z
    cls = cls_t[xrow] if with_xrow else cls_t                 # per union row
    deg = np.diff(rowptr)
    nb = np.arange(nq, n_rows)
    pool = {k: np.nonzero(cls == k)[0] for k in range(3)}
    nb_A = nb[(cls[nb] == 0) & (deg[nb] > 0)]
    nb_Z = nb[cls[nb] == 2]
    assert all(len(p) for p in pool.values()) and len(nb_A) and len(nb_Z)
    col = col.copy()
    for r in range(n_rows):
        d = int(deg[r])
        if d == 0:
            continue
        c = 1 << int(rng.integers(0, d.bit_length()))        # a power of two <= d
        if r < nq:
            win, lose = nb_A, nb_Z
        else:
            win, lose = pool[0 if cls[r] == 0 else 1], pool[2]
        ent = np.concatenate([rng.choice(win, size=c), rng.choice(lose, size=d - c)])
        col[rowptr[r]:rowptr[r + 1]] = rng.permutation(ent)
    if with_xrow:   # keep one entry at the last table row: an entry of the same class moves there
        same = np.nonzero((cls[col] == cls[last]) & (np.arange(len(col)) >= rowptr[nq]))[0]
        col[same[-1]] = last
    T, b0 = qr.exact_gather_inputs(rng, H, nt, with_b0)
    T[:, CSTAR] = np.where(cls_t == 0, BIG, np.where(cls_t == 1, 0.0, rng.choice([0.0, BIG], size=nt)))
    a_src0 = np.where(cls_t == 2, -LO, 0.0).astype(np.float32)
    a_dst0 = (rng.permutation(257)[:nt] - 128).astype(np.float32) / 2.0
    u_src, u_dst = np.zeros(H, dtype=np.float32), np.zeros(H, dtype=np.float32)
    u_src[CSTAR] = 1.0
    if b0 is not None:
        b0[CSTAR] = 0.0
    if H > CQ:
        T[:, CQ] = 2048.0 * rng.integers(1, 5, size=nt)
        u_dst[CQ] = -2.0
        if b0 is not None:
            b0[CQ] = 0.0
    return dict(rowptr=rowptr, col=col, xrow=xrow, T=T.astype(np.float32), b0=b0, a_src0=a_src0, a_dst0=a_dst0, u_src=u_src, u_dst=u_dst,
                slope0=SELECTOR_SLOPES[0], slope1=SELECTOR_SLOPES[1], rows=np.arange(nq, dtype=np.int64), n_rows=n_rows)


EXACT_GENERATORS = {"uniform": exact_uniform_case, "selector": exact_selector_case}


def run(c, rows=None, **kw):
    """gather() on a case dict."""
    return gather(c["rowptr"], c["col"], c["T"], c["a_src0"], c["a_dst0"], c["u_src"], c["u_dst"], c["rows"] if rows is None else rows,
                  xrow=c["xrow"], b0=c["b0"], slope0=c["slope0"], slope1=c["slope1"], **kw)
