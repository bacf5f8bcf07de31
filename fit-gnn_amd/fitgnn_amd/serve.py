"""QueryEngine: predictions for node ids, computed on each node's two-hop receptive field inside its own subgraph.

FIT-GNN answers a node query by running the model on the ONE subgraph that holds the node (inference.py:668-688 of the reference)
and keeping one row.  For the reference's default model -- two GCNConv layers, ELU, lt1, eval mode -- row q of the block-diagonal
union needs only

    T     = X W0^T                                                     once per model, every table row (ops.Linear)
    h_j   = ELU(sum_{e' in row j} val[e'] T[xrow[col[e']]] + b0)        j in row q's columns
    g_q   = sum_{e in row q} val[e] h_{col[e]}                          ops.gcn_query_gather: one launch for any number of queries
    out_q = Wl ELU(W1 g_q + b1) + bl   (+ log_softmax)                  ops.gcn_query_tail:   one launch

The union is block-diagonal, so both hops stay inside the query's subgraph and the values are the per-subgraph forward's.

With gat_kernels=True a model of two GATConv layers (heads = 1) takes the same two launches, attention over both hops
(ops.gat_query_gather, then the same tail: sum beta = 1, so W1 (sum_j beta_j h_j) + b1 is conv1's output):

    T, a0s = T att_src0, a0d = T att_dst0                               once per set of weights, per table row
    u_s = W1^T att_src1, u_d = W1^T att_dst1                            (att . (W1 h) = (W1^T att) . h)
    h_r   = ELU(sum_k alpha_rk T[t(k)] + b0)                            alpha_r. = softmax_k lrelu(a0s[t(k)] + a0d[t(r)], slope0)
    g_q   = sum_j beta_j h_j                                            beta = softmax_j lrelu(u_s . h_j + u_d . h_q, slope1)

With sage_kernels=True a model of two SAGEConv layers takes two launches as well: its layer is a gather plus a root term, over the
union's mean CSR (no self loops added, val = 1 / max(deg, 1): what nn.SAGEConv.forward looks up), with t(r) the table row of union row r:

    T     = X [W_l0 ; W_r0]^T    [n_table, 2H]                          once per set of weights (one ops.Linear)
    h_r   = ELU(sum_{k in row r} val[k] T[t(col[k])][0:H] + T[t(r)][H:2H] + b_l0)
    G_q   = [sum_{j in row q} val[j] h_{col[j]} | h_q]                   ops.sage_query_gather
    out_q = Wl ELU([W_l1 | W_r1] G_q + b_l1) + bl   (+ log_softmax)      ops.gcn_query_tail, unchanged, with K = 2H

With gin_kernels=True a model of two GINConv layers whose nn is Linear, ReLU, Linear, ReLU (network._make_convs) takes two launches
of its own, over the union's sum CSR (no self loops added, val = 1: what nn.GINConv.forward looks up).  Only the first Linear of a
layer commutes with the aggregation; the second sits behind a ReLU and runs once per one-hop row of the query, inside the first launch:

    T     = X W0a^T    [n_table, Ha]                                    once per set of weights (one ops.Linear, no bias)
    a_r   = ReLU(sum_{k in row r} val[k] T[t(col[k])] + (1 + eps0) T[t(r)] + b0a)
    h_r   = ReLU(W0b a_r + b0b)                                         the dense product, per one-hop row
    s_q   = sum_{j in row q} val[j] h_{col[j]} + (1 + eps1) h_q         ops.gin_query_hops (eps read on the device)
    out_q = Wl ReLU(W1b ReLU(W1a s_q + b1a) + b1b) + bl  (+ log_softmax) ops.gin_query_tail

(the model's ELU after each conv is the identity on a ReLU output: the path holds only for an MLP that ends in ReLU).  Its latency
against the per-subgraph forward is not measured, so it is opt-in as the other two are.

Any other model (a GAT, SAGE or GIN model without its flag, a GIN model with another MLP, one or three layers, hidden sizes the
kernels do not take) is answered by that per-subgraph forward itself, each subgraph cut out of the union once and kept.

GraphQueryEngine: predictions for GRAPH ids of a graph_data.GraphSet (the reference's graph_cls / graph_reg tasks, inference.py:288-538:
the model on ONE graph's subgraph set, coarse graph or -- the baseline -- uncoarsened graph).  For two GCNConv layers every graph of a
predict() call shares two launches:

    T     = X W0^T                                                     once per set of weights, every row of the view
    h_r   = ELU(sum_{e' in row r} val[e'] T[col[e']] + b0)              EVERY row r of the graph, formed once, in LDS
    g_r   = sum_{e in row r} val[e] h_{col[e]}                          r among the graph's pooled rows     ops.gcn_graph_query_hops
    out   = Wl pool_r ELU(W1 g_r + b1) + bl   (softmax)                 max | mean over the pooled rows      ops.gcn_graph_query_tail

A graph is a contiguous, block-diagonal row range of its view, so the layer-0 rows of a graph of up to 160 rows at hidden 512 fit the
LDS window of one workgroup; calling the per-row gather on every pooled row would form each h_r once per entry that reaches it.  A
larger graph's pooled rows take that per-row gather all the same (correct for any size), into the same G in front of the one tail.

With gin_kernels=True a model of two GINConv layers (nn = Linear, ReLU, Linear, ReLU) takes two launches of its own over the view's sum
CSR (no self loops added, val = 1).  A GIN layer-0 row carries a dense Hb x Ha product behind a ReLU; the per-row kernel
(ops.gin_query_hops) forms it once per entry that reaches the row and once for the row itself, sum_r (deg(r) + 1) products for a graph
whose rows are all pooled, where the window forms each ONCE:

    T     = X W0a^T    [n_rows, Ha]                                     once per set of weights (one ops.Linear, no bias)
    a_r   = ReLU(sum_{k in row r} val[k] T[col[k]] + (1 + eps0) T[r] + b0a)     EVERY row r of the graph
    h_r   = ReLU(W0b a_r + b0b)                                         EVERY row r of the graph, formed once, in LDS
    s_r   = sum_{e in row r} val[e] h_{col[e]} + (1 + eps1) h_r         r among the graph's pooled rows     ops.gin_graph_query_hops
    out   = Wl pool_r ReLU(W1b ReLU(W1a s_r + b1a) + b1b) + bl  (softmax)                                   ops.gin_graph_query_tail

The window shares LDS with the product's two stages: ops.gin_graph_query_max_rows(Ha, Hb) rows, about 90 at 512 / 512 and about 450 at
64 / 64.  A larger graph's pooled rows take ops.gin_query_hops (the same s_r), into the same G in front of the one tail.  The path is
opt-in, as on the node engine; without the flag, and for any GIN model the kernels do not take, the model's own forward answers.

With gat_kernels=True a model of two GATConv layers (heads = 1) takes one launch of its own over the view's "gat" CSR (existing self
loops removed, one added per row) in front of the GCN graph tail, unchanged (sum beta = 1, as on the node engine).  The per-row kernel
(ops.gat_query_gather) re-forms h_j -- a softmax over row j and a gather of deg(j) table rows -- and its H-long score dot once per
entry that reaches j, sum_r (deg(r) + 1) layer-0 rows per graph; the window forms each ONCE and keeps its two dots beside it, so a
layer-1 score is two LDS scalar reads and an add:

    T, a0s, a0d, u_s, u_d                                               as on the node engine, once per set of the six weights
    h_r   = ELU(sum_k alpha_rk T[k] + b0)                               EVERY row r of the graph, formed once, in LDS
    ds_r  = u_s . h_r,  dd_r = u_d . h_r                                EVERY row r of the graph, behind the window
    g_r   = sum_j beta_j h_j,  beta = softmax_j lrelu(ds_j + dd_r, slope1)   r among the graph's pooled rows   ops.gat_graph_query_hops
    out   = Wl pool_r ELU(W1 g_r + b1) + bl   (softmax)                                                       ops.gcn_graph_query_tail

A wave holds a whole row (a score is a dot over all of H), so the window's row is H floats: ops.gat_graph_query_max_rows(H) rows, 79 at
hidden 512 and 620 at 64.  A larger graph's pooled rows take ops.gat_query_gather (the same g_r up to the summation order), into the
same G in front of the one tail.  Opt-in, as the node engine's switch is.

With sage_kernels=True a model of two SAGEConv layers takes one launch of its own over the view's mean CSR (no self loops added,
val = 1 / max(deg, 1)) in front of the GCN graph tail, unchanged, called with K = 2H.  The per-row kernel (ops.sage_query_gather)
re-forms h_c -- a gather of deg(c) + 1 table half-rows -- once per entry that reaches c and once more for c itself,
sum_r (deg(r) + 1) layer-0 rows per graph; the window forms each ONCE, and a pooled row's own h is a copy from it:

    T     = X [W_l0 ; W_r0]^T    [n_rows, 2H]                           once per set of the four weights (one ops.Linear)
    h_r   = ELU(sum_{k in row r} val[k] T[col[k]][0:H] + T[r][H:2H] + b_l0)     EVERY row r of the graph, formed once, in LDS
    G_r   = [sum_{e in row r} val[e] h_{col[e]} | h_r]                  r among the graph's pooled rows     ops.sage_graph_query_hops
    out   = Wl pool_r ELU([W_l1 | W_r1] G_r + b_l1) + bl   (softmax)                                        ops.gcn_graph_query_tail

The columns of h are independent, so the window's row is one 256-column slab: ops.sage_graph_query_max_rows(H) rows, 160 at hidden 512
and 640 at 64, as on the GCN path.  A larger graph's pooled rows take ops.sage_query_gather (the same [g | h] layout; g up to the
summation order), into the same G in front of the one tail.  Opt-in, as the node engine's switch is.
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


def gat_prepared_state(T, ws):
    """The GAT paths' state made from T = X W0^T and the six weights ws = [W0, att_src0, att_dst0, W1, att_src1, att_dst1]:
    ([(tensor, version)] of ws, a0s, a0d, u_s, u_d) with a0s / a0d = T att0 per table row (fitgnn_gat_scores_f32) and u = W1^T att1,
    formed in float64 and rounded once.  Both engines call it."""
    from . import _lib
    W0, as0, ad0, W1, as1, ad1 = ws
    n, H = T.shape
    with torch.no_grad():
        a0s = torch.empty(n, dtype=torch.float32, device=T.device)
        a0d = torch.empty(n, dtype=torch.float32, device=T.device)
        as0, ad0 = as0.detach().reshape(-1).contiguous(), ad0.detach().reshape(-1).contiguous()
        _lib.check(_lib.lib().fitgnn_gat_scores_f32(_lib.dptr(T), T.stride(0), n, H, _lib.dptr(as0), _lib.dptr(ad0), _lib.dptr(a0s),
                                                    _lib.dptr(a0d), _lib.stream_ptr(T.device)), "fitgnn_gat_scores_f32")
        W1d = W1.detach().double()
        u_s = (as1.detach().reshape(1, -1).double() @ W1d).reshape(-1).float().contiguous()
        u_d = (ad1.detach().reshape(1, -1).double() @ W1d).reshape(-1).float().contiguous()
    return ([(w, w._version) for w in ws], a0s, a0d, u_s, u_d)


def _gat_weights(model):
    c0, c1 = model.conv
    return [c0.lin.weight, c0.att_src, c0.att_dst, c1.lin.weight, c1.att_src, c1.att_dst]


def sage_prepared_state(X, ws, op_config):
    """The SAGE paths' state made from the table operand X and the four weights ws = [W_l0, W_r0, W_l1, W_r1]:
    ([(tensor, version)] of ws, T = X [W_l0 ; W_r0]^T [n_table, 2H] (one product), W1cat = [W_l1 | W_r1] [H2, 2H]).  Both engines call it."""
    Wl0, Wr0, Wl1, Wr1 = ws
    with torch.no_grad():
        T = ops.Linear.apply(X.float(), torch.cat([Wl0.detach(), Wr0.detach()], 0).contiguous(), op_config).contiguous()
        W1cat = torch.cat([Wl1.detach(), Wr1.detach()], 1).contiguous()
    return ([(w, w._version) for w in ws], T, W1cat)


def _sage_weights(model):
    c0, c1 = model.conv
    return [c0.lin_l.weight, c0.lin_r.weight, c1.lin_l.weight, c1.lin_r.weight]


class QueryEngine:
    """predict(node_ids) -> [Q, C] for a trained network.Classify_node (log-probabilities) or network.Regress_node (raw values) over a
    data.SubgraphBatch, extra-node or cluster-node layout, with or without the de-duplicated feature table.  gat_kernels: a model of
    two GATConv layers is answered by the attention query kernel (off by default: its speed against the per-subgraph forward is
    not measured yet); it changes nothing for any other model.  sage_kernels: the same switch for a model of two SAGEConv layers
    (the mean-aggregation query kernel), off by default for the same reason.  gin_kernels: the same switch for a model of two GINConv
    layers with the reference's two-Linear ReLU MLP (the hops kernel with its dense product and the two-stage tail), off by default
    for the same reason."""

    def __init__(self, model, batch, gat_kernels=False, sage_kernels=False, gin_kernels=False):
        self.model, self.batch = model, batch
        self.gat_kernels = bool(gat_kernels)
        self.sage_kernels = bool(sage_kernels)
        self.gin_kernels = bool(gin_kernels)
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
        self._T = None          # (W0, W0._version, T)
        self._subgraphs = {}    # the per-subgraph forward's inputs: s -> (x, edge_index, first row)
        self._fused = None      # (key of the model's layers and parameters, "gcn" | "gat" | "sage" | "gin" | None: the kernels that answer)
        self._gat = None        # the GAT path's prepared state: ([(tensor, version)] of the six weights it is made from, a0s, a0d, u_s, u_d)
        self._sage = None       # the SAGE path's prepared state: ([(tensor, version)] of the four weights it is made from, T, W1cat)
        self._mean = None       # the union's mean CSR (the SAGE path's pattern), looked up once
        self._gin = None        # the GIN path's prepared state: ((W0a, version), T)
        self._sum = None        # the union's sum CSR (the GIN path's pattern), looked up once

    # -- the table T = X W0^T --
    def _kind(self):
        """"gcn" (ops.query_supported), "gat" (gat_kernels and ops.gat_query_supported), "sage" (sage_kernels and
        ops.sage_query_supported), "gin" (gin_kernels and ops.gin_query_supported) or None, re-evaluated only when a layer or a parameter's storage, type or shape has changed."""
        m = self.model
        params = [p for c in m.conv for p in (getattr(getattr(c, "lin", None), "weight", None), getattr(c, "bias", None))]
        params += [m.lt1.weight, m.lt1.bias]
        if self.gat_kernels:
            params += [getattr(c, a, None) for c in m.conv for a in ("att_src", "att_dst")]
        if self.sage_kernels:
            params += [getattr(getattr(c, l, None), a, None) for c in m.conv for l in ("lin_l", "lin_r") for a in ("weight", "bias")]
        if self.gin_kernels:
            mlps = [getattr(c, "nn", None) for c in m.conv]
            subs = [list(n) if isinstance(n, torch.nn.Sequential) else [] for n in mlps]
            params += [getattr(l, a, None) for n in subs for l in n for a in ("weight", "bias")] + [getattr(c, "eps", None) for c in m.conv]
            params += [type(l) for n in subs for l in n]     # an activation swapped in place changes no parameter
        key = tuple(type(c) for c in m.conv) + tuple((p.data_ptr(), p.dtype, p.shape) if torch.is_tensor(p) else p for p in params)
        if self._fused is None or self._fused[0] != key:
            kind = "gcn" if ops.query_supported(m) else ("gat" if self.gat_kernels and ops.gat_query_supported(m) else None)
            if kind is None and self.sage_kernels and ops.sage_query_supported(m):
                kind = "sage"
            if kind is None and self.gin_kernels and ops.gin_query_supported(m):
                kind = "gin"
            self._fused = (key, kind)
        return self._fused[1]

    @property
    def fused(self):
        """The query kernels answer for the model (otherwise the per-subgraph forward does)."""
        return self._kind() is not None

    def _operand(self):
        b = self.batch
        if b.x_table is not None and b.row_index is not None:
            return b.x_table, b.row_index.index
        return b.x, None

    def refresh(self):
        """Remake T -- and, on the GAT path, the score vectors and W1^T att; on the SAGE path, [W_l1 | W_r1] -- from the model's
        current weights (done automatically when one of the weights they are made from changes)."""
        if self._kind() == "sage":
            return self._refresh_sage()
        if self._kind() == "gin":
            return self._refresh_gin()
        W0 = self.model.conv[0].lin.weight
        X, _ = self._operand()
        with torch.no_grad():
            T = ops.Linear.apply(X.float(), W0, self.model.op_config).contiguous()
        self._T = (W0, W0._version, T)
        if self._kind() == "gat":
            self._refresh_gat(T)
        return self

    def _gat_weights(self):
        return _gat_weights(self.model)

    def _refresh_gat(self, T):
        """a0s / a0d = T att0 per table row; u = W1^T att1 (gat_prepared_state)."""
        self._gat = gat_prepared_state(T, self._gat_weights())

    def _gat_state(self):
        """(T, a0s, a0d, u_s, u_d), remade when the storage or version of any of the six weights has changed."""
        ws = self._gat_weights()
        if self._gat is None or not all(ops._same_index(e, w) for e, w in zip(self._gat[0], ws)) or not ops._same_index(self._T, ws[0]):
            self.refresh()
        return (self._T[2],) + tuple(self._gat[1:])

    def _sage_weights(self):
        return _sage_weights(self.model)

    def _refresh_sage(self):
        """T = X [W_l0 ; W_r0]^T [n_table, 2H] (one product) and W1cat = [W_l1 | W_r1] [H2, 2H] (sage_prepared_state)."""
        self._sage = sage_prepared_state(self._operand()[0], self._sage_weights(), self.model.op_config)
        return self

    def _sage_state(self):
        """(T, W1cat), remade when the storage or version of any of the four weights has changed."""
        ws = self._sage_weights()
        if self._sage is None or not all(ops._same_index(e, w) for e, w in zip(self._sage[0], ws)):
            self._refresh_sage()
        return self._sage[1], self._sage[2]

    def _mean_csr(self):
        """The union's mean CSR (rows = targets, no self loops added, val = 1 / max(deg, 1)): nn.SAGEConv.forward's own lookup."""
        if self._mean is None:
            self._mean = csr_for(self.batch.edge_index, self.n_rows, "mean")
        return self._mean

    def _refresh_gin(self):
        """T = X W0a^T [n_table, Ha]: the first Linear of conv0's MLP, without its bias (the kernel adds it behind the aggregation)."""
        W0a = self.model.conv[0].nn[0].weight
        X, _ = self._operand()
        with torch.no_grad():
            T = ops.Linear.apply(X.float(), W0a, self.model.op_config).contiguous()
        self._gin = ((W0a, W0a._version), T)
        return self

    def _gin_state(self):
        """T, remade when the storage or version of W0a has changed; every other weight and both eps are read at every call."""
        if self._gin is None or not ops._same_index(self._gin[0], self.model.conv[0].nn[0].weight):
            self._refresh_gin()
        return self._gin[1]

    def _sum_csr(self):
        """The union's sum CSR (rows = targets, no self loops added, val = 1): nn.GINConv.forward's own lookup."""
        if self._sum is None:
            self._sum = csr_for(self.batch.edge_index, self.n_rows, "sum")
        return self._sum

    def _table(self):
        W0 = self.model.conv[0].lin.weight
        if not ops._same_index(self._T, W0):
            self.refresh()
        return self._T[2]

    @property
    def table_bytes(self):
        """Bytes of T -- [n_table, 2H] on the SAGE path, [n_table, Ha] on the GIN path -- and of the two score vectors on the GAT path (0 on the per-subgraph path,
        which keeps none)."""
        kind = self._kind()
        if kind is None:
            return 0
        if kind == "gat":
            T, a0s, a0d = self._gat_state()[:3]
            return int(T.numel()) * T.element_size() + int(a0s.numel() + a0d.numel()) * a0s.element_size()
        T = self._sage_state()[0] if kind == "sage" else self._gin_state() if kind == "gin" else self._table()
        return int(T.numel()) * T.element_size()

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
        with torch.no_grad():
            if self.fused:
                return self._predict_fused(rows)
            return self._predict_subgraphs(rows)

    def _predict_fused(self, rows):
        m, f = self.model, self.graph.f
        _, xrow = self._operand()
        if self._kind() == "gat":   # the same pattern in both CSR modes: existing self loops removed, one added per node
            T, a0s, a0d, u_s, u_d = self._gat_state()
            G = ops.gat_query_gather(f.rowptr, f.col, T, a0s, a0d, u_s, u_d, rows, xrow=xrow, b0=m.conv[0].bias,
                                     slope0=m.conv[0].negative_slope, slope1=m.conv[1].negative_slope)
            return ops.gcn_query_tail(G, m.conv[1].lin.weight, m.conv[1].bias, m.lt1.weight, m.lt1.bias, log_softmax=self.log_softmax)
        if self._kind() == "sage":   # G = [g_q | h_q]: the tail's K is 2H
            T, W1cat = self._sage_state()
            f = self._mean_csr().f
            G = ops.sage_query_gather(f.rowptr, f.col, f.val, T, rows, xrow=xrow, b0=m.conv[0].lin_l.bias)
            return ops.gcn_query_tail(G, W1cat, m.conv[1].lin_l.bias, m.lt1.weight, m.lt1.bias, log_softmax=self.log_softmax)
        if self._kind() == "gin":    # eps0 / eps1 stay on the device: the kernel reads them
            (_, _, l0b, _), (l1a, _, l1b, _) = m.conv[0].nn, m.conv[1].nn
            f = self._sum_csr().f
            G = ops.gin_query_hops(f.rowptr, f.col, f.val, self._gin_state(), m.conv[0].eps.detach(), l0b.weight, l0b.bias,
                                   m.conv[1].eps.detach(), rows, xrow=xrow, b0a=m.conv[0].nn[0].bias)
            return ops.gin_query_tail(G, l1a.weight, l1a.bias, l1b.weight, l1b.bias, m.lt1.weight, m.lt1.bias, log_softmax=self.log_softmax)
        G = ops.gcn_query_gather(f.rowptr, f.col, f.val, self._table(), rows, xrow=xrow, b0=m.conv[0].bias)
        return ops.gcn_query_tail(G, m.conv[1].lin.weight, m.conv[1].bias, m.lt1.weight, m.lt1.bias, log_softmax=self.log_softmax)

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


class GraphQueryEngine:
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
        self.model, self.gset, self.view = model, gset, view
        self.classify = isinstance(model, (network.Classify_graph_gs, network.Classify_graph_gc))
        self.max_window_rows = None if max_window_rows is None else int(max_window_rows)
        self.gin_kernels = bool(gin_kernels)
        self.gat_kernels = bool(gat_kernels)
        self.sage_kernels = bool(sage_kernels)
        ptr, x, mask = {"gs": (gset.gs_ptr, gset.gs_x, gset.gs_mask), "gc": (gset.cluster_ptr, gset.gc_x, None),
                        "orig": (gset.node_ptr, gset.x, None)}[view]
        ptr = np.asarray(ptr, dtype=np.int64)
        self.n_graphs, self.n_rows, self.x = len(ptr) - 1, int(ptr[-1]), x
        self._ptr = ptr
        self._whole = gset.batch(0, self.n_graphs, view)   # the view as ONE block-diagonal piece; the CSR cache is keyed on its edge tensor
        self.graph = csr_for(self._whole["edge_index"], self.n_rows, "gcn")
        if mask is None:
            prow, pp = torch.arange(self.n_rows, dtype=torch.int64, device=dev), ptr
        else:
            prow = torch.nonzero(mask).flatten().to(torch.int64).contiguous()         # ascending: grouped by graph
            pp = np.searchsorted(prow.cpu().numpy(), ptr, side="left").astype(np.int64)
        self._prow, self._pp = prow, pp
        self._prow_host = prow.cpu().numpy()
        self._T = None          # (W0, W0._version, T): W0 = conv[0].lin.weight, on the GIN path conv[0].nn[0].weight
        self._fused = None      # (key of the model's layers and parameters, "gcn" | "gat" | "sage" | "gin" | None: the kernels that answer)
        self._sum = None        # the view's sum CSR (the GIN path's pattern), looked up once
        self._gat = None        # the GAT path's prepared state: ([(tensor, version)] of the six weights, a0s, a0d, u_s, u_d)
        self._gat_graph = None  # the view's "gat" CSR (existing self loops removed, one added per row), looked up once
        self._sage = None       # the SAGE path's prepared state: ([(tensor, version)] of the four weights, T [n_rows, 2H], W1cat)
        self._mean = None       # the view's mean CSR (the SAGE path's pattern), looked up once

    def _kind(self):
        """"gcn" (ops.graph_query_supported), "gat" (gat_kernels and ops.gat_graph_query_supported), "sage" (sage_kernels and
        ops.sage_graph_query_supported), "gin" (gin_kernels and ops.gin_graph_query_supported) or None, re-evaluated only when a layer or a parameter's storage, type or shape has changed."""
        m = self.model
        params = [p for c in m.conv for p in (getattr(getattr(c, "lin", None), "weight", None), getattr(c, "bias", None))]
        params += [m.lt1.weight, m.lt1.bias]
        if self.gat_kernels:
            params += [getattr(c, a, None) for c in m.conv for a in ("att_src", "att_dst")]
        if self.sage_kernels:
            params += [getattr(getattr(c, l, None), a, None) for c in m.conv for l in ("lin_l", "lin_r") for a in ("weight", "bias")]
        if self.gin_kernels:
            mlps = [getattr(c, "nn", None) for c in m.conv]
            subs = [list(n) if isinstance(n, torch.nn.Sequential) else [] for n in mlps]
            params += [getattr(l, a, None) for n in subs for l in n for a in ("weight", "bias")] + [getattr(c, "eps", None) for c in m.conv]
            params += [type(l) for n in subs for l in n]     # an activation swapped in place changes no parameter
        key = tuple(type(c) for c in m.conv) + tuple((p.data_ptr(), p.dtype, p.shape) if torch.is_tensor(p) else p for p in params)
        if self._fused is None or self._fused[0] != key:
            kind = "gcn" if ops.graph_query_supported(m) else ("gat" if self.gat_kernels and ops.gat_graph_query_supported(m) else None)
            if kind is None and self.sage_kernels and ops.sage_graph_query_supported(m):
                kind = "sage"
            if kind is None and self.gin_kernels and ops.gin_graph_query_supported(m):
                kind = "gin"
            self._fused = (key, kind)
        return self._fused[1]

    @property
    def fused(self):
        """The graph-query kernels answer for the model (otherwise its own forward does)."""
        return self._kind() is not None

    def _w0(self):
        conv0 = self.model.conv[0]
        return conv0.nn[0].weight if self._kind() == "gin" else conv0.lin.weight

    def refresh(self):
        """Remake T = X W0^T (on the GIN path X W0a^T, without the bias: the kernel adds it behind the aggregation) and, on the GAT
        path, the score vectors and W1^T att; on the SAGE path T = X [W_l0 ; W_r0]^T and [W_l1 | W_r1] -- from the model's current
        weights (done automatically when the storage or version of a weight they are made from changes)."""
        if self._kind() == "sage":
            self._sage = sage_prepared_state(self.x, _sage_weights(self.model), self.model.op_config)
        elif self.fused:
            W0 = self._w0()
            with torch.no_grad():
                T = ops.Linear.apply(self.x.float(), W0, self.model.op_config).contiguous()
            self._T = (W0, W0._version, T)
            if self._kind() == "gat":
                self._gat = gat_prepared_state(T, _gat_weights(self.model))
        return self

    def _gat_state(self):
        """(T, a0s, a0d, u_s, u_d), remade when the storage or version of any of the six weights has changed."""
        ws = _gat_weights(self.model)
        if self._gat is None or not all(ops._same_index(e, w) for e, w in zip(self._gat[0], ws)) or not ops._same_index(self._T, ws[0]):
            self.refresh()
        return (self._T[2],) + tuple(self._gat[1:])

    def _sage_state(self):
        """(T, W1cat), remade when the storage or version of any of the four weights has changed."""
        ws = _sage_weights(self.model)
        if self._sage is None or not all(ops._same_index(e, w) for e, w in zip(self._sage[0], ws)):
            self.refresh()
        return self._sage[1], self._sage[2]

    def _mean_csr(self):
        """The view's mean CSR (rows = targets, no self loops added, val = 1 / max(deg, 1)): nn.SAGEConv.forward's own lookup."""
        if self._mean is None:
            self._mean = csr_for(self._whole["edge_index"], self.n_rows, "mean")
        return self._mean

    def _gat_csr(self):
        """The view's "gat" CSR (rows = targets, existing self loops removed, one added per row): nn.GATConv.forward's own lookup."""
        if self._gat_graph is None:
            self._gat_graph = csr_for(self._whole["edge_index"], self.n_rows, "gat")
        return self._gat_graph

    def _table(self):
        if not ops._same_index(self._T, self._w0()):
            self.refresh()
        return self._T[2]

    def _sum_csr(self):
        """The view's sum CSR (rows = targets, no self loops added, val = 1): nn.GINConv.forward's own lookup."""
        if self._sum is None:
            self._sum = csr_for(self._whole["edge_index"], self.n_rows, "sum")
        return self._sum

    @property
    def table_bytes(self):
        """Bytes of T -- [n_rows, Ha] on the GIN path, [n_rows, 2H] on the SAGE path -- and of the two score vectors on the GAT path (0
        when the model's own forward answers: it keeps none)."""
        if not self.fused:
            return 0
        if self._kind() == "sage":
            T = self._sage_state()[0]
            return int(T.numel()) * T.element_size()
        if self._kind() == "gat":
            T, a0s, a0d = self._gat_state()[:3]
            return int(T.numel()) * T.element_size() + int(a0s.numel() + a0d.numel()) * a0s.element_size()
        T = self._table()
        return int(T.numel()) * T.element_size()

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
        with torch.no_grad():
            if self.fused:
                return self._predict_fused(ids, cnt)
            return self._predict_forward(ids)

    def _predict_fused(self, ids, cnt):
        m, dev = self.model, self.x.device
        gin, gat, sage = self._kind() == "gin", self._kind() == "gat", self._kind() == "sage"
        f = self._sum_csr().f if gin else self._gat_csr().f if gat else self._mean_csr().f if sage else self.graph.f
        C = int(m.lt1.weight.shape[0])
        if ids.size == 0:
            return torch.empty((0, C), dtype=torch.float32, device=dev)
        if gat:
            T, a0s, a0d, u_s, u_d = self._gat_state()
        elif sage:
            T, W1cat = self._sage_state()
        else:
            T = self._table()
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
        pool = "max" if self.classify else "mean"
        if gin:    # eps0 / eps1 stay on the device: the kernels read them
            (l0a, _, l0b, _), (l1a, _, l1b, _) = m.conv[0].nn, m.conv[1].nn
            eps0, eps1 = m.conv[0].eps.detach(), m.conv[1].eps.detach()
            Hg = int(l0b.weight.shape[0])
            limit = ops.gin_graph_query_max_rows(int(T.shape[1]), Hg)
        elif sage:   # G = [g_r | h_r]: the tail's K is 2H
            Hg = int(T.shape[1])
            limit = ops.sage_graph_query_max_rows(Hg // 2)
            b0 = m.conv[0].lin_l.bias
        else:
            Hg = int(T.shape[1])
            limit = ops.gat_graph_query_max_rows(Hg) if gat else ops.graph_query_max_rows(Hg)
            b0 = m.conv[0].bias
            slopes = dict(slope0=m.conv[0].negative_slope, slope1=m.conv[1].negative_slope) if gat else None
        if self.max_window_rows is not None:
            limit = min(limit, self.max_window_rows)
        large = n_rows > limit
        G = torch.empty((P, Hg), dtype=torch.float32, device=dev)
        if not large.all():
            # a graph beyond max_rows is skipped by the launch itself: its rows of G are written by the per-row kernel below
            window = int(n_rows[~large].max())
            if gin:
                ops.gin_graph_query_hops(f.rowptr, f.col, f.val, T, eps0, l0b.weight, l0b.bias, eps1, seg, prow, pptr, window,
                                         b0a=l0a.bias, out=G)
            elif gat:
                ops.gat_graph_query_hops(f.rowptr, f.col, T, a0s, a0d, u_s, u_d, seg, prow, pptr, window, b0=b0, out=G, **slopes)
            elif sage:
                ops.sage_graph_query_hops(f.rowptr, f.col, f.val, T, seg, prow, pptr, window, b0=b0, out=G)
            else:
                ops.gcn_graph_query_hops(f.rowptr, f.col, f.val, T, seg, prow, pptr, window, b0=b0, out=G)
        if large.any():   # the per-row kernel: correct for any size, the view being block-diagonal
            pos = torch.from_numpy(np.nonzero(np.repeat(large, cnt))[0]).to(dev)
            rows = prow.index_select(0, pos)
            if gin:
                G.index_copy_(0, pos, ops.gin_query_hops(f.rowptr, f.col, f.val, T, eps0, l0b.weight, l0b.bias, eps1, rows, b0a=l0a.bias))
            elif gat:
                G.index_copy_(0, pos, ops.gat_query_gather(f.rowptr, f.col, T, a0s, a0d, u_s, u_d, rows, b0=b0, **slopes))
            elif sage:
                G.index_copy_(0, pos, ops.sage_query_gather(f.rowptr, f.col, f.val, T, rows, b0=b0))
            else:
                G.index_copy_(0, pos, ops.gcn_query_gather(f.rowptr, f.col, f.val, T, rows, b0=b0))
        if gin:
            return ops.gin_graph_query_tail(G, pptr, l1a.weight, l1a.bias, l1b.weight, l1b.bias, m.lt1.weight, m.lt1.bias, pool=pool,
                                            softmax=self.classify)
        if sage:
            return ops.gcn_graph_query_tail(G, pptr, W1cat, m.conv[1].lin_l.bias, m.lt1.weight, m.lt1.bias, pool=pool, softmax=self.classify)
        return ops.gcn_graph_query_tail(G, pptr, m.conv[1].lin.weight, m.conv[1].bias, m.lt1.weight, m.lt1.bias, pool=pool,
                                        softmax=self.classify)

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
