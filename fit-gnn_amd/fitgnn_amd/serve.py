"""QueryEngine: predictions for node ids, computed on each node's two-hop receptive field inside its own subgraph.

FIT-GNN answers a node query by running the model on the ONE subgraph that holds the node (inference.py:668-688 of the reference)
and keeping one row.  For a model of two layers of one of the kinds in PATHS -- GCNConv always; GATConv, SAGEConv, GINConv behind their
switches -- any number of queries take two launches: the kind's per-row gather over both hops (rows_hops), from a table T made once per
set of weights (prepare), then its tail (node_tail).  The union is block-diagonal, so both hops stay inside the query's subgraph and the
values are the per-subgraph forward's.  Each kind's mathematics is its object's docstring.

Any other model (a GAT, SAGE or GIN model without its flag, a GIN model with another MLP, one or three layers, hidden sizes the
kernels do not take) is answered by that per-subgraph forward itself, each subgraph cut out of the union once and kept.

GraphQueryEngine: predictions for GRAPH ids of a graph_data.GraphSet (the reference's graph_cls / graph_reg tasks, inference.py:288-538:
the model on ONE graph's subgraph set, coarse graph or -- the baseline -- uncoarsened graph).  Every graph of a predict() call shares
two launches: the kind's window launch (window_hops), which forms EVERY layer-0 row of a graph once, in LDS, and aggregates them for
the graph's pooled rows, then its pooling tail (graph_tail).

A graph is a contiguous, block-diagonal row range of its view, so the layer-0 rows of a graph of up to 160 rows at hidden 512 fit the
LDS window of one workgroup; calling the per-row gather on every pooled row would form each h_r once per entry that reaches it.  A
larger graph's pooled rows take that per-row gather all the same (correct for any size), into the same G in front of the one tail.
Without its flag, and for any model the kernels do not take, the model's own forward answers.
"""
import numpy as np
import torch

from . import ops
from .csr import csr_for


def core_row_table(node_id, core, n_nodes=None):
    """Host function.  int64 [n_nodes]: the union row at which original node v is a core (own-cluster) row, -1 where the batch holds
    no such row (a shard holds only some clusters).  node_id / core: per union row, the original node and whether the row is its
    cluster's own copy (every node is core in exactly one subgraph of the full union)."""
    node_id = np.asarray(node_id, dtype=np.int64)
    core = np.asarray(core, dtype=bool)
    rows = np.nonzero(core)[0]
    ids = node_id[rows]
    n = int(n_nodes) if n_nodes is not None else (int(node_id.max()) + 1 if node_id.size else 0)
    table = np.full(n, -1, dtype=np.int64)
    table[ids[::-1]] = rows[::-1]   # a node listed twice keeps its first core row
    return table


def first_missing(table, node_ids):
    """Host function.  The first of node_ids that has no core row in `table` (outside it, or -1 there); None when all have one."""
    ids = np.asarray(node_ids, dtype=np.int64).reshape(-1)
    inside = (ids >= 0) & (ids < len(table))
    ok = inside.copy()
    ok[inside] = table[ids[inside]] >= 0
    bad = np.nonzero(~ok)[0]
    return None if bad.size == 0 else int(ids[bad[0]])


def _product(X, W, model):
    """X W^T as the layers' own Linear makes it, contiguous."""
    return ops.Linear.apply(X.float(), W, model.op_config).contiguous()


class GCNPath:
    """Two GCNConv layers, ELU, lt1, eval mode (the reference's default model), over the GCN-normalised CSR.  Row q of the union needs only

        T     = X W0^T                                                     once per model, every table row (ops.Linear)
        h_j   = ELU(sum_{e' in row j} val[e'] T[xrow[col[e']]] + b0)        j in row q's columns
        g_q   = sum_{e in row q} val[e] h_{col[e]}                          ops.gcn_query_gather: one launch for any number of queries
        out_q = Wl ELU(W1 g_q + b1) + bl   (+ log_softmax)                  ops.gcn_query_tail:   one launch

    and the graphs of one GraphQueryEngine.predict() call

        T     = X W0^T                                                     once per set of weights, every row of the view
        h_r   = ELU(sum_{e' in row r} val[e'] T[col[e']] + b0)              EVERY row r of the graph, formed once, in LDS
        g_r   = sum_{e in row r} val[e] h_{col[e]}                          r among the graph's pooled rows     ops.gcn_graph_query_hops
        out   = Wl pool_r ELU(W1 g_r + b1) + bl   (softmax)                 max | mean over the pooled rows      ops.gcn_graph_query_tail

    The members below are what an engine asks of a kind: name / flag (the engine's switch, None: always on), csr_mode (the csr_for
    mode of its pattern), key_params (what decides whether the kernels take the model), supported, weights (the tensors whose storage
    or version invalidates the prepared state), prepare (the state tuple, T first), table_bytes, rows_hops (the per-row launch),
    window_hops / window_limit / g_width (the window launch, the rows it holds, the width of G) and the two tails."""
    name, flag, csr_mode = "gcn", None, "gcn"

    def key_params(self, m):
        return [p for c in m.conv for p in (getattr(getattr(c, "lin", None), "weight", None), getattr(c, "bias", None))] + [m.lt1.weight, m.lt1.bias]

    def supported(self, m, graph):
        return ops.graph_query_supported(m) if graph else ops.query_supported(m)

    def weights(self, m):
        return [m.conv[0].lin.weight]

    def prepare(self, X, m):
        return (_product(X, m.conv[0].lin.weight, m),)

    def table_bytes(self, state):
        return int(state[0].numel()) * state[0].element_size()

    def rows_hops(self, f, state, m, rows, xrow=None, out=None):
        return ops.gcn_query_gather(f.rowptr, f.col, f.val, state[0], rows, xrow=xrow, b0=m.conv[0].bias, out=out)

    def window_hops(self, f, state, m, seg, prow, pptr, window, out):
        return ops.gcn_graph_query_hops(f.rowptr, f.col, f.val, state[0], seg, prow, pptr, window, b0=m.conv[0].bias, out=out)

    def window_limit(self, state, m):
        return ops.graph_query_max_rows(self.g_width(state, m))

    def g_width(self, state, m):
        return int(state[0].shape[1])

    def _layer1(self, state, m):
        """(W1, b1) of the tails."""
        return m.conv[1].lin.weight, m.conv[1].bias

    def node_tail(self, G, state, m, log_softmax):
        return ops.gcn_query_tail(G, *self._layer1(state, m), m.lt1.weight, m.lt1.bias, log_softmax=log_softmax)

    def graph_tail(self, G, pptr, state, m, pool, softmax):
        return ops.gcn_graph_query_tail(G, pptr, *self._layer1(state, m), m.lt1.weight, m.lt1.bias, pool=pool, softmax=softmax)


class GATPath(GCNPath):
    """With gat_kernels=True a model of two GATConv layers (heads = 1) takes the same two launches, attention over both hops
    (ops.gat_query_gather, then the same tail: sum beta = 1, so W1 (sum_j beta_j h_j) + b1 is conv1's output):

        T, a0s = T att_src0, a0d = T att_dst0                               once per set of weights, per table row
        u_s = W1^T att_src1, u_d = W1^T att_dst1                            (att . (W1 h) = (W1^T att) . h)
        h_r   = ELU(sum_k alpha_rk T[t(k)] + b0)                            alpha_r. = softmax_k lrelu(a0s[t(k)] + a0d[t(r)], slope0)
        g_q   = sum_j beta_j h_j                                            beta = softmax_j lrelu(u_s . h_j + u_d . h_q, slope1)

    The kernel ignores val, and the "gcn" and "gat" CSR modes have the same pattern (existing self loops removed, one added per node),
    so the node engine hands it the CSR its batch already holds.

    On the graph engine it takes one launch of its own over the view's "gat" CSR (existing self loops removed, one added per row) in
    front of the GCN graph tail, unchanged (sum beta = 1, as on the node engine).  The per-row kernel (ops.gat_query_gather) re-forms
    h_j -- a softmax over row j and a gather of deg(j) table rows -- and its H-long score dot once per entry that reaches j,
    sum_r (deg(r) + 1) layer-0 rows per graph; the window forms each ONCE and keeps its two dots beside it, so a layer-1 score is two
    LDS scalar reads and an add:

        T, a0s, a0d, u_s, u_d                                               as on the node engine, once per set of the six weights
        h_r   = ELU(sum_k alpha_rk T[k] + b0)                               EVERY row r of the graph, formed once, in LDS
        ds_r  = u_s . h_r,  dd_r = u_d . h_r                                EVERY row r of the graph, behind the window
        g_r   = sum_j beta_j h_j,  beta = softmax_j lrelu(ds_j + dd_r, slope1)   r among the graph's pooled rows   ops.gat_graph_query_hops
        out   = Wl pool_r ELU(W1 g_r + b1) + bl   (softmax)                                                       ops.gcn_graph_query_tail

    A wave holds a whole row (a score is a dot over all of H), so the window's row is H floats: ops.gat_graph_query_max_rows(H) rows,
    79 at hidden 512 and 620 at 64.  A larger graph's pooled rows take ops.gat_query_gather (the same g_r up to the summation order),
    into the same G in front of the one tail.  Opt-in: its speed against the forward is not measured yet."""
    name, flag, csr_mode = "gat", "gat_kernels", "gat"

    def key_params(self, m):
        return [getattr(c, a, None) for c in m.conv for a in ("att_src", "att_dst")]

    def supported(self, m, graph):
        return ops.gat_graph_query_supported(m) if graph else ops.gat_query_supported(m)

    def weights(self, m):
        c0, c1 = m.conv
        return [c0.lin.weight, c0.att_src, c0.att_dst, c1.lin.weight, c1.att_src, c1.att_dst]

    def prepare(self, X, m):
        """(T, a0s, a0d, u_s, u_d): a0s / a0d = T att0 per table row (fitgnn_gat_scores_f32) and u = W1^T att1, formed in float64 and
        rounded once."""
        from . import _lib
        W0, as0, ad0, W1, as1, ad1 = self.weights(m)
        T = _product(X, W0, m)
        n, H = T.shape
        a0s = torch.empty(n, dtype=torch.float32, device=T.device)
        a0d = torch.empty(n, dtype=torch.float32, device=T.device)
        as0, ad0 = as0.detach().reshape(-1).contiguous(), ad0.detach().reshape(-1).contiguous()
        _lib.call("fitgnn_gat_scores_f32", T, T.stride(0), n, H, as0, ad0, a0s, a0d, _lib.stream_ptr(T.device))
        W1d = W1.detach().double()
        u_s = (as1.detach().reshape(1, -1).double() @ W1d).reshape(-1).float().contiguous()
        u_d = (ad1.detach().reshape(1, -1).double() @ W1d).reshape(-1).float().contiguous()
        return (T, a0s, a0d, u_s, u_d)

    def table_bytes(self, state):
        T, a0s, a0d = state[:3]
        return int(T.numel()) * T.element_size() + int(a0s.numel() + a0d.numel()) * a0s.element_size()

    def rows_hops(self, f, state, m, rows, xrow=None, out=None):
        return ops.gat_query_gather(f.rowptr, f.col, *state, rows, xrow=xrow, b0=m.conv[0].bias, slope0=m.conv[0].negative_slope,
                                    slope1=m.conv[1].negative_slope, out=out)

    def window_hops(self, f, state, m, seg, prow, pptr, window, out):
        return ops.gat_graph_query_hops(f.rowptr, f.col, *state, seg, prow, pptr, window, b0=m.conv[0].bias,
                                        slope0=m.conv[0].negative_slope, slope1=m.conv[1].negative_slope, out=out)

    def window_limit(self, state, m):
        return ops.gat_graph_query_max_rows(self.g_width(state, m))


class GATHeadsPath(GATPath):
    """With gat_heads_kernels=True a model of two GATConv(heads, concat) layers with the same heads in 2..8 takes two launches of its
    own on the node engine (ops.mhgat_query_gather, ops.mhgat_query_tail).  With H = heads C0 and H2 = heads C1 the layers' widths:

        T, a0s, a0d [n_table, heads]                                        the per-head score dots of T, once per set of weights
        U_s[hd] = W1[block hd]^T att_src1[hd], U_d[hd] likewise [heads, H]   (att . (W1 h)[block hd] = (W1[block hd]^T att) . h)
        h_r[c]  = ELU(sum_k alpha^{hd(c)}_rk T[t(k)][c] + b0[c])            alpha^{hd}_r. = softmax_k lrelu(a0s[t(k), hd] + a0d[t(r), hd])
        G_q[hd H + c] = sum_j beta^{hd}_j h_j[c]                            beta^{hd} = softmax_j lrelu(U_s[hd] . h_j + U_d[hd] . h_q)
        out_q   = Wl ELU(z_q) + bl,  z_q[block hd] = W1[block hd] G_q[block hd] + b1[block hd]      (sum_j beta^{hd}_j = 1)

    Every head weighs the same rows h_j, so G is heads times as wide as h and the tail's first product is grouped.  The graph engine
    has no multi-head path (supported(m, graph=True) is False: it answers such a model with its forward).  Opt-in, as the other
    kinds: tools/query_latency.py --layer GATConv --heads measures it against the per-subgraph forward."""
    name, flag, csr_mode = "gat_heads", "gat_heads_kernels", "gat"

    def key_params(self, m):
        return GATPath.key_params(self, m) + [x for c in m.conv for x in (getattr(c, "heads", None), getattr(c, "concat", None))]

    def supported(self, m, graph):
        return False if graph else ops.mhgat_query_supported(m)

    def prepare(self, X, m):
        """(T, a0s, a0d, U_s, U_d): a0s / a0d [n_table, heads] = the per-head dots of T with att0 (fitgnn_gat_heads_scores_f32) and
        U[hd] = W1[block hd]^T att1[hd] [heads, H], formed in float64 and rounded once."""
        from . import _lib
        W0, as0, ad0, W1, as1, ad1 = self.weights(m)
        heads = m.conv[0].heads
        T = _product(X, W0, m)
        n, H = T.shape
        a0s = torch.empty((n, heads), dtype=torch.float32, device=T.device)
        a0d = torch.empty((n, heads), dtype=torch.float32, device=T.device)
        as0, ad0 = as0.detach().reshape(-1).contiguous(), ad0.detach().reshape(-1).contiguous()
        _lib.call("fitgnn_gat_heads_scores_f32", T, T.stride(0), n, heads, H // heads, as0, ad0, a0s, a0d, _lib.stream_ptr(T.device))
        W1b = W1.detach().double().view(heads, -1, H)                        # [heads, C1, H]
        U_s = torch.einsum("gc,gch->gh", as1.detach().double().view(heads, -1), W1b).float().contiguous()
        U_d = torch.einsum("gc,gch->gh", ad1.detach().double().view(heads, -1), W1b).float().contiguous()
        return (T, a0s, a0d, U_s, U_d)

    def rows_hops(self, f, state, m, rows, xrow=None, out=None):
        return ops.mhgat_query_gather(f.rowptr, f.col, *state, rows, xrow=xrow, b0=m.conv[0].bias, slope0=m.conv[0].negative_slope,
                                      slope1=m.conv[1].negative_slope, out=out)

    def g_width(self, state, m):
        return int(state[0].shape[1]) * int(state[3].shape[0])

    def node_tail(self, G, state, m, log_softmax):
        return ops.mhgat_query_tail(G, *self._layer1(state, m), m.lt1.weight, m.lt1.bias, int(state[3].shape[0]), log_softmax=log_softmax)


class SAGEPath(GCNPath):
    """With sage_kernels=True a model of two SAGEConv layers takes two launches as well: its layer is a gather plus a root term, over
    the union's mean CSR (no self loops added, val = 1 / max(deg, 1): what nn.SAGEConv.forward looks up), with t(r) the table row of
    union row r:

        T     = X [W_l0 ; W_r0]^T    [n_table, 2H]                          once per set of weights (one ops.Linear)
        h_r   = ELU(sum_{k in row r} val[k] T[t(col[k])][0:H] + T[t(r)][H:2H] + b_l0)
        G_q   = [sum_{j in row q} val[j] h_{col[j]} | h_q]                   ops.sage_query_gather
        out_q = Wl ELU([W_l1 | W_r1] G_q + b_l1) + bl   (+ log_softmax)      ops.gcn_query_tail, unchanged, with K = 2H

    On the graph engine it takes one launch of its own over the view's mean CSR in front of the GCN graph tail, unchanged, called with
    K = 2H.  The per-row kernel (ops.sage_query_gather) re-forms h_c -- a gather of deg(c) + 1 table half-rows -- once per entry that
    reaches c and once more for c itself, sum_r (deg(r) + 1) layer-0 rows per graph; the window forms each ONCE, and a pooled row's own
    h is a copy from it:

        T     = X [W_l0 ; W_r0]^T    [n_rows, 2H]                           once per set of the four weights (one ops.Linear)
        h_r   = ELU(sum_{k in row r} val[k] T[col[k]][0:H] + T[r][H:2H] + b_l0)     EVERY row r of the graph, formed once, in LDS
        G_r   = [sum_{e in row r} val[e] h_{col[e]} | h_r]                  r among the graph's pooled rows     ops.sage_graph_query_hops
        out   = Wl pool_r ELU([W_l1 | W_r1] G_r + b_l1) + bl   (softmax)                                        ops.gcn_graph_query_tail

    The columns of h are independent, so the window's row is one 256-column slab: ops.sage_graph_query_max_rows(H) rows, 160 at hidden
    512 and 640 at 64, as on the GCN path.  A larger graph's pooled rows take ops.sage_query_gather (the same [g | h] layout; g up to
    the summation order), into the same G in front of the one tail.  Opt-in, for the same reason as the GAT kind."""
    name, flag, csr_mode = "sage", "sage_kernels", "mean"

    def key_params(self, m):
        return [getattr(getattr(c, l, None), a, None) for c in m.conv for l in ("lin_l", "lin_r") for a in ("weight", "bias")]

    def supported(self, m, graph):
        return ops.sage_graph_query_supported(m) if graph else ops.sage_query_supported(m)

    def weights(self, m):
        c0, c1 = m.conv
        return [c0.lin_l.weight, c0.lin_r.weight, c1.lin_l.weight, c1.lin_r.weight]

    def prepare(self, X, m):
        """(T = X [W_l0 ; W_r0]^T [n_table, 2H] (one product), W1cat = [W_l1 | W_r1] [H2, 2H])."""
        Wl0, Wr0, Wl1, Wr1 = (w.detach() for w in self.weights(m))
        return (_product(X, torch.cat([Wl0, Wr0], 0).contiguous(), m), torch.cat([Wl1, Wr1], 1).contiguous())

    def rows_hops(self, f, state, m, rows, xrow=None, out=None):
        return ops.sage_query_gather(f.rowptr, f.col, f.val, state[0], rows, xrow=xrow, b0=m.conv[0].lin_l.bias, out=out)

    def window_hops(self, f, state, m, seg, prow, pptr, window, out):
        return ops.sage_graph_query_hops(f.rowptr, f.col, f.val, state[0], seg, prow, pptr, window, b0=m.conv[0].lin_l.bias, out=out)

    def window_limit(self, state, m):   # G = [g_r | h_r]: its width, and the tail's K, is 2H
        return ops.sage_graph_query_max_rows(self.g_width(state, m) // 2)

    def _layer1(self, state, m):
        return state[1], m.conv[1].lin_l.bias


class GINPath(GCNPath):
    """With gin_kernels=True a model of two GINConv layers whose nn is Linear, ReLU, Linear, ReLU (network._make_convs) takes two
    launches of its own, over the union's sum CSR (no self loops added, val = 1: what nn.GINConv.forward looks up).  Only the first
    Linear of a layer commutes with the aggregation; the second sits behind a ReLU and runs once per one-hop row of the query, inside
    the first launch:

        T     = X W0a^T    [n_table, Ha]                                    once per set of weights (one ops.Linear, no bias)
        a_r   = ReLU(sum_{k in row r} val[k] T[t(col[k])] + (1 + eps0) T[t(r)] + b0a)
        h_r   = ReLU(W0b a_r + b0b)                                         the dense product, per one-hop row
        s_q   = sum_{j in row q} val[j] h_{col[j]} + (1 + eps1) h_q         ops.gin_query_hops (eps read on the device)
        out_q = Wl ReLU(W1b ReLU(W1a s_q + b1a) + b1b) + bl  (+ log_softmax) ops.gin_query_tail

    (the model's ELU after each conv is the identity on a ReLU output: the path holds only for an MLP that ends in ReLU).  Its latency
    against the per-subgraph forward is not measured, so it is opt-in as the other two are.

    On the graph engine it takes two launches of its own over the view's sum CSR.  A GIN layer-0 row carries a dense Hb x Ha product
    behind a ReLU; the per-row kernel (ops.gin_query_hops) forms it once per entry that reaches the row and once for the row itself,
    sum_r (deg(r) + 1) products for a graph whose rows are all pooled, where the window forms each ONCE:

        T     = X W0a^T    [n_rows, Ha]                                     once per set of weights (one ops.Linear, no bias)
        a_r   = ReLU(sum_{k in row r} val[k] T[col[k]] + (1 + eps0) T[r] + b0a)     EVERY row r of the graph
        h_r   = ReLU(W0b a_r + b0b)                                         EVERY row r of the graph, formed once, in LDS
        s_r   = sum_{e in row r} val[e] h_{col[e]} + (1 + eps1) h_r         r among the graph's pooled rows     ops.gin_graph_query_hops
        out   = Wl pool_r ReLU(W1b ReLU(W1a s_r + b1a) + b1b) + bl  (softmax)                                   ops.gin_graph_query_tail

    The window shares LDS with the product's two stages: ops.gin_graph_query_max_rows(Ha, Hb) rows, about 90 at 512 / 512 and about
    450 at 64 / 64.  A larger graph's pooled rows take ops.gin_query_hops (the same s_r), into the same G in front of the one tail."""
    name, flag, csr_mode = "gin", "gin_kernels", "sum"

    def key_params(self, m):
        mlps = [getattr(c, "nn", None) for c in m.conv]
        subs = [list(n) if isinstance(n, torch.nn.Sequential) else [] for n in mlps]
        params = [getattr(l, a, None) for n in subs for l in n for a in ("weight", "bias")] + [getattr(c, "eps", None) for c in m.conv]
        return params + [type(l) for n in subs for l in n]     # an activation swapped in place changes no parameter

    def supported(self, m, graph):
        return ops.gin_graph_query_supported(m) if graph else ops.gin_query_supported(m)

    def weights(self, m):
        return [m.conv[0].nn[0].weight]

    def prepare(self, X, m):
        """(T = X W0a^T [n_table, Ha],): the first Linear of conv0's MLP, without its bias (the kernel adds it behind the aggregation);
        every other weight and both eps are read at every call."""
        return (_product(X, m.conv[0].nn[0].weight, m),)

    def _hops(self, state, m):
        """T, eps0, W0b, b0b, eps1: eps0 / eps1 stay on the device, the kernels read them."""
        c0, c1 = m.conv
        return state[0], c0.eps.detach(), c0.nn[2].weight, c0.nn[2].bias, c1.eps.detach()

    def rows_hops(self, f, state, m, rows, xrow=None, out=None):
        return ops.gin_query_hops(f.rowptr, f.col, f.val, *self._hops(state, m), rows, xrow=xrow, b0a=m.conv[0].nn[0].bias, out=out)

    def window_hops(self, f, state, m, seg, prow, pptr, window, out):
        return ops.gin_graph_query_hops(f.rowptr, f.col, f.val, *self._hops(state, m), seg, prow, pptr, window, b0a=m.conv[0].nn[0].bias,
                                        out=out)

    def window_limit(self, state, m):
        return ops.gin_graph_query_max_rows(int(state[0].shape[1]), self.g_width(state, m))

    def g_width(self, state, m):
        return int(m.conv[0].nn[2].weight.shape[0])

    def _layer1(self, state, m):
        """(W1a, b1a, W1b, b1b) of the tails."""
        l1a, _, l1b, _ = m.conv[1].nn
        return l1a.weight, l1a.bias, l1b.weight, l1b.bias

    def node_tail(self, G, state, m, log_softmax):
        return ops.gin_query_tail(G, *self._layer1(state, m), m.lt1.weight, m.lt1.bias, log_softmax=log_softmax)

    def graph_tail(self, G, pptr, state, m, pool, softmax):
        return ops.gin_graph_query_tail(G, pptr, *self._layer1(state, m), m.lt1.weight, m.lt1.bias, pool=pool, softmax=softmax)


PATHS = (GCNPath(), GATPath(), GATHeadsPath(), SAGEPath(), GINPath())   # in precedence order


class _Engine:
    """What both engines share: which kind of PATHS answers, its CSR and its prepared state.  An engine sets graph_level (which of a
    kind's two `supported` it asks), calls _setup and defines _operand() -> (X, xrow)."""

    def _setup(self, model, flags, edge_index, csrs):
        """flags: (gat_kernels, sage_kernels, gin_kernels, gat_heads_kernels); edge_index: what csr_for is keyed on; csrs: mode -> the
        CSRs at hand."""
        self.model = model
        self.gat_kernels, self.sage_kernels, self.gin_kernels, self.gat_heads_kernels = (bool(f) for f in flags)
        self._edge_index, self._csrs = edge_index, dict(csrs)
        self._fused = None      # (key of the model's layers and parameters, the kind of PATHS that answers or None)
        self._state = None      # ([(tensor, version)] of the kind's weights(model), its prepared state: T first)

    def path(self):
        """The first kind of PATHS whose flag is None or set and whose kernels take the model (None: no kernels answer), re-evaluated
        only when a layer or a parameter's storage, type or shape has changed."""
        m = self.model
        on = [p for p in PATHS if p.flag is None or getattr(self, p.flag)]
        params = [x for p in on for x in p.key_params(m)]
        key = tuple(type(c) for c in m.conv) + tuple((p.data_ptr(), p.dtype, p.shape) if torch.is_tensor(p) else p for p in params)
        if self._fused is None or self._fused[0] != key:
            self._fused = (key, next((p for p in on if p.supported(m, graph=self.graph_level)), None))
            self._state = None
        return self._fused[1]

    def _kind(self):
        """The name of path(): "gcn", "gat", "gat_heads", "sage", "gin" or None."""
        return getattr(self.path(), "name", None)

    @property
    def fused(self):
        """The query kernels answer for the model (otherwise its own forward does)."""
        return self.path() is not None

    def refresh(self):
        """Remake the prepared state -- T and whatever else the kind's prepare makes -- from the model's current weights (done
        automatically when the storage or version of one of the kind's weights(model) changes).  Nothing to do when no kernels answer."""
        path = self.path()
        if path is not None:
            ws = path.weights(self.model)
            with torch.no_grad():
                self._state = ([(w, w._version) for w in ws], path.prepare(self._operand()[0], self.model))
        return self

    def state(self, path=None):
        """The kind's prepared state (T first), remade when the storage or version of any of its weights(model) has changed."""
        path = path if path is not None else self.path()
        ws = path.weights(self.model)
        if self._state is None or not all(ops._same_index(e, w) for e, w in zip(self._state[0], ws)):
            self.refresh()
        return self._state[1]

    def csr(self, path=None):
        """The CSR of the kind's mode (rows = targets), looked up once per mode: the layer's own lookup."""
        mode = (path if path is not None else self.path()).csr_mode
        if mode not in self._csrs:
            self._csrs[mode] = csr_for(self._edge_index, self.n_rows, mode)
        return self._csrs[mode]

    @property
    def table_bytes(self):
        """Bytes of T -- and of the two score vectors on the GAT path (0 when no kernels answer: nothing is kept)."""
        path = self.path()
        return 0 if path is None else path.table_bytes(self.state(path))


class QueryEngine(_Engine):
    """predict(node_ids) -> [Q, C] for a trained network.Classify_node (log-probabilities) or network.Regress_node (raw values) over a
    data.SubgraphBatch, extra-node or cluster-node layout, with or without the de-duplicated feature table.  gat_kernels: a model of
    two GATConv layers is answered by the attention query kernel (off by default: its speed against the per-subgraph forward is
    not measured yet); it changes nothing for any other model.  sage_kernels: the same switch for a model of two SAGEConv layers
    (the mean-aggregation query kernel), off by default for the same reason.  gin_kernels: the same switch for a model of two GINConv
    layers with the reference's two-Linear ReLU MLP (the hops kernel with its dense product and the two-stage tail), off by default
    for the same reason.  gat_heads_kernels: the same switch for a model of two GATConv(heads, concat) layers with the same heads in
    2..8 (the per-head attention query kernel and its grouped tail); gat_kernels alone leaves such a model to its forward."""
    graph_level = False

    def __init__(self, model, batch, gat_kernels=False, sage_kernels=False, gin_kernels=False, gat_heads_kernels=False):
        self.batch = batch
        self.log_softmax = not isinstance(model, _regressors())
        g = batch.graph
        if g is None:
            raise ValueError("QueryEngine needs a SubgraphBatch on the GPU")
        self.graph = g
        self.n_rows = int(batch.n_rows)
        dev = batch.x.device
        n_nodes = int(batch.x_table.shape[0]) if batch.x_table is not None else None
        table = core_row_table(batch.node_id.cpu().numpy(), batch.core.cpu().numpy(), n_nodes)
        self._core_host = table
        self._core_row = torch.from_numpy(table).to(dev)
        self._subgraphs = {}    # the per-subgraph forward's inputs: s -> (x, edge_index, first row)
        # the GAT kernel ignores val and both modes have one pattern: no second CSR is built
        self._setup(model, (gat_kernels, sage_kernels, gin_kernels, gat_heads_kernels), batch.edge_index,
                    {m: g for m in (GCNPath.csr_mode, GATPath.csr_mode)})

    def _operand(self):
        b = self.batch
        if b.x_table is not None and b.row_index is not None:
            return b.x_table, b.row_index.index
        return b.x, None

    # -- queries --
    def predict(self, node_ids):
        """[Q, C] for original node ids (any order, repeats allowed).  ValueError names the first id that has no core row here."""
        ids = torch.as_tensor(node_ids, dtype=torch.int64).reshape(-1)
        miss = first_missing(self._core_host, ids.cpu().numpy())
        if miss is not None:
            raise ValueError(f"node {miss} has no core row in this batch")
        return self.predict_rows(self._core_row.index_select(0, ids.to(self._core_row.device)))

    def predict_rows(self, rows):
        """[Q, C] for union rows."""
        if self.model.training:
            raise RuntimeError("QueryEngine answers in eval mode only: call model.eval() (dropout has no place in a query)")
        dev = self.batch.x.device
        if torch.is_tensor(rows) and rows.is_cuda:
            rows = rows.to(torch.int64).reshape(-1).contiguous()
            bad = bool(rows.numel()) and (int(rows.min()) < 0 or int(rows.max()) >= self.n_rows)
        else:   # host ids: checked on the host, no device round trip before the launches
            host = np.asarray(rows.numpy() if torch.is_tensor(rows) else rows, dtype=np.int64).reshape(-1)
            bad = bool(host.size) and (int(host.min()) < 0 or int(host.max()) >= self.n_rows)
            rows = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
        if bad:
            raise ValueError(f"union rows must lie in [0, {self.n_rows})")
        path = self.path()
        with torch.no_grad():
            if path is not None:
                return self._predict_fused(rows, path)
            return self._predict_subgraphs(rows)

    def _predict_fused(self, rows, path):
        state = self.state(path)
        G = path.rows_hops(self.csr(path).f, state, self.model, rows, xrow=self._operand()[1])
        return path.node_tail(G, state, self.model, self.log_softmax)

    def subgraph(self, s):
        """(x, edge_index, first union row) of subgraph s as its own small graph, cut out once and kept; its CSR is built here too."""
        hit = self._subgraphs.get(s)
        if hit is None:
            b = self.batch
            r0, r1 = int(b.ptr[s]), int(b.ptr[s + 1])
            ei = b.edge_index
            m = (ei[0] >= r0) & (ei[0] < r1)
            hit = (b.x[r0:r1].contiguous(), (ei[:, m] - r0).contiguous(), r0)
            mode = _layer_mode(self.model)
            if mode is not None:
                csr_for(hit[1], r1 - r0, mode)
            self._subgraphs[s] = hit
        return hit

    def _predict_subgraphs(self, rows):
        host = rows.cpu().numpy()
        subs = np.searchsorted(self.batch.ptr, host, side="right") - 1
        C = int(self.model.lt1.weight.shape[0])
        out = torch.empty((len(host), C), dtype=torch.float32, device=rows.device)
        for s in np.unique(subs):
            x, ei, r0 = self.subgraph(int(s))
            y = self.model(x, ei)
            pick = torch.from_numpy(np.nonzero(subs == s)[0]).to(rows.device)
            out[pick] = y.index_select(0, rows[pick] - r0).float()
        return out


class GraphQueryEngine(_Engine):
    """predict(graph_ids) -> [Q, C] for a trained network.Classify_graph_gs / _gc (softmax probabilities, max pool) or
    network.Regress_graph_gs / _gc (raw values, mean pool) over a graph_data.GraphSet on the GPU.

    view: "gs" (the subgraph union: gs_x, gs_ptr, gs_edge_index; pooled rows = the rows where gs_mask is set), "gc" (the coarse
    graphs: gc_x, cluster_ptr, gc_edge_index) or "orig" (the uncoarsened graphs: x, node_ptr, edge_index -- the baseline); on "gc" and
    "orig" every row of a graph is pooled.  Default: "gs" for the *_gs classes, "gc" for the *_gc classes (whose forward pools every
    row: they do not take "gs").  max_window_rows: graphs with more rows than this -- or than the hops kernel's LDS window holds at the
    model's hidden size -- are answered through the per-row gather inside the same call.  gin_kernels: a model of two GINConv layers
    with the reference's two-Linear ReLU MLP is answered by the GIN graph-query pair (off by default, as QueryEngine's switch is); it
    changes nothing for any other model.  gat_kernels: the same switch for a model of two GATConv layers (heads = 1): the attention
    window launch in front of the GCN graph tail.  sage_kernels: the same switch for a model of two SAGEConv layers: the
    mean-plus-root window launch over the view's mean CSR in front of the GCN graph tail with K = 2H.

    The view's CSR, the per-graph pointers and the index of pooled rows are built here, once.  Any model the kernels do not
    take (ops.graph_query_supported, ops.gin_graph_query_supported behind gin_kernels, ops.gat_graph_query_supported behind
    gat_kernels, ops.sage_graph_query_supported behind sage_kernels) is answered by its own forward on gset.batch_ids(the unique ids, view)."""
    graph_level = True

    def __init__(self, model, gset, view=None, max_window_rows=None, gin_kernels=False, gat_kernels=False, sage_kernels=False):
        from . import network
        gs_cls = (network.Classify_graph_gs, network.Regress_graph_gs)
        gc_cls = (network.Classify_graph_gc, network.Regress_graph_gc)
        if not isinstance(model, gs_cls + gc_cls):
            raise TypeError("GraphQueryEngine needs one of network.Classify_graph_gs / _gc, Regress_graph_gs / _gc")
        self._gs_model = isinstance(model, gs_cls)
        view = view if view is not None else ("gs" if self._gs_model else "gc")
        if view not in ("gs", "gc", "orig"):
            raise ValueError(f"view must be 'gs', 'gc' or 'orig', not {view!r}")
        if view == "gs" and not self._gs_model:
            raise ValueError("a *_graph_gc model pools every row of its graph: it takes the views 'gc' and 'orig'")
        dev = gset.x.device
        if dev.type != "cuda":
            raise ValueError("GraphQueryEngine needs a GraphSet on the GPU")
        self.gset, self.view = gset, view
        self.classify = isinstance(model, (network.Classify_graph_gs, network.Classify_graph_gc))
        self.max_window_rows = None if max_window_rows is None else int(max_window_rows)
        ptr, x, mask = {"gs": (gset.gs_ptr, gset.gs_x, gset.gs_mask), "gc": (gset.cluster_ptr, gset.gc_x, None),
                        "orig": (gset.node_ptr, gset.x, None)}[view]
        ptr = np.asarray(ptr, dtype=np.int64)
        self.n_graphs, self.n_rows, self.x = len(ptr) - 1, int(ptr[-1]), x
        self._ptr = ptr
        self._whole = gset.batch(0, self.n_graphs, view)   # the view as ONE block-diagonal piece; the CSR cache is keyed on its edge tensor
        self.graph = csr_for(self._whole["edge_index"], self.n_rows, GCNPath.csr_mode)
        if mask is None:
            prow, pp = torch.arange(self.n_rows, dtype=torch.int64, device=dev), ptr
        else:
            prow = torch.nonzero(mask).flatten().to(torch.int64).contiguous()         # ascending: grouped by graph
            pp = np.searchsorted(prow.cpu().numpy(), ptr, side="left").astype(np.int64)
        self._prow, self._pp = prow, pp
        self._prow_host = prow.cpu().numpy()
        self._setup(model, (gat_kernels, sage_kernels, gin_kernels, False), self._whole["edge_index"], {GCNPath.csr_mode: self.graph})

    def _operand(self):
        return self.x, None

    def predict(self, graph_ids):
        """[Q, C] for graph ids (any order, repeats allowed, host or device).  ValueError names the first id outside [0, n_graphs)
        and the first graph without pooled rows."""
        if self.model.training:
            raise RuntimeError("GraphQueryEngine answers in eval mode only: call model.eval() (dropout has no place in a query)")
        ids = (graph_ids.detach().cpu().numpy() if torch.is_tensor(graph_ids) else np.asarray(graph_ids)).astype(np.int64).reshape(-1)
        bad = np.nonzero((ids < 0) | (ids >= self.n_graphs))[0]
        if bad.size:
            raise ValueError(f"graph {int(ids[bad[0]])} is outside [0, {self.n_graphs})")
        cnt = self._pp[ids + 1] - self._pp[ids]
        empty = np.nonzero(cnt == 0)[0]
        if empty.size:
            raise ValueError(f"graph {int(ids[empty[0]])} has no pooled rows in the view '{self.view}'")
        path = self.path()
        with torch.no_grad():
            if path is not None:
                return self._predict_fused(ids, cnt, path)
            return self._predict_forward(ids)

    def _predict_fused(self, ids, cnt, path):
        m, dev = self.model, self.x.device
        if ids.size == 0:
            return torch.empty((0, int(m.lt1.weight.shape[0])), dtype=torch.float32, device=dev)
        f, state = self.csr(path).f, self.state(path)
        Q = int(ids.size)
        # the launch's index arrays are made on the host, where the ids and the pointers are, and go up in ONE copy: no device glue
        pptr_h = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        P = int(pptr_h[-1])
        # pooled row j of query i is the view's pooled row pp[ids[i]] + (j - pptr[i])
        prow_h = self._prow_host[np.repeat(self._pp[ids] - pptr_h[:-1], cnt) + np.arange(P)]
        n_rows = self._ptr[ids + 1] - self._ptr[ids]
        seg_h = np.stack([self._ptr[ids], self._ptr[ids + 1]], 1).reshape(-1)
        packed = torch.from_numpy(np.concatenate([seg_h, pptr_h, prow_h])).to(dev)
        seg, pptr, prow = packed[:2 * Q].view(Q, 2), packed[2 * Q:3 * Q + 1], packed[3 * Q + 1:]
        limit = path.window_limit(state, m)
        if self.max_window_rows is not None:
            limit = min(limit, self.max_window_rows)
        large = n_rows > limit
        G = torch.empty((P, path.g_width(state, m)), dtype=torch.float32, device=dev)
        if not large.all():
            # a graph beyond max_rows is skipped by the launch itself: its rows of G are written by the per-row kernel below
            path.window_hops(f, state, m, seg, prow, pptr, int(n_rows[~large].max()), G)
        if large.any():   # the per-row kernel: correct for any size, the view being block-diagonal
            pos = torch.from_numpy(np.nonzero(np.repeat(large, cnt))[0]).to(dev)
            G.index_copy_(0, pos, path.rows_hops(f, state, m, prow.index_select(0, pos)))
        return path.graph_tail(G, pptr, state, m, "max" if self.classify else "mean", self.classify)

    def _predict_forward(self, ids):
        """The model's own forward on the unique graphs as one block-diagonal batch."""
        import types

        from .train import _cat_pieces
        uniq, inv = np.unique(ids, return_inverse=True)
        C = int(self.model.lt1.weight.shape[0])
        if uniq.size == 0:
            return torch.empty((0, C), dtype=torch.float32, device=self.x.device)
        piece = self.gset.batch_ids(uniq.tolist(), self.view)
        if self._gs_model:
            if piece["mask"] is None:   # "gc" / "orig": every row is pooled
                piece["mask"] = torch.ones(piece["x"].shape[0], dtype=torch.bool, device=self.x.device)
            b = _cat_pieces([piece], "gs", types)
            out = self.model(b, b["graph_of_masked"])
        else:
            out = self.model(_cat_pieces([piece], "gc", types)["gc"])
        return out.float().reshape(len(uniq), -1).index_select(0, torch.from_numpy(inv.reshape(-1)).to(out.device))


def _regressors():
    from . import network
    return (network.Regress_node,)


def _layer_mode(model):
    """The CSR mode the model's layers look up (pre-built per subgraph so that a timed forward finds it)."""
    from . import nn as fnn
    conv = model.conv[0] if len(model.conv) else None
    if isinstance(conv, fnn.GCNConv):
        return "gcn"
    if isinstance(conv, fnn.GATConv):
        return "gat"
    if isinstance(conv, fnn.GINConv):
        return "sum"
    if isinstance(conv, fnn.SAGEConv):
        return "mean"
    return None
