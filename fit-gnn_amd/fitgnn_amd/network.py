"""The six model classes of FIT-GNN's network.py, same surface, on fitgnn_amd.nn layers.

Kept from the reference (network.py:8-204): constructor takes the argparse Namespace (num_layers1,
layer_name, num_features, hidden, num_classes); attributes `.conv` (ModuleList) and `.lt1` (Linear);
`state_dict` keys `conv.{i}.*`, `lt1.*`; forward signatures and output activations:
    Classify_node(x, edge_index)      -> log_softmax            (:29-35)
    Regress_node(x, edge_index)       -> raw [N,1]               (:58-64)
    Classify_graph_gc(gc)             -> softmax(max-pool)       (:87-95)
    Regress_graph_gc(gc)              -> lt1(mean-pool)          (:158-166)
    Classify_graph_gs(set_gs, batch)  -> softmax(max-pool of masked subgraph rows)   (:118-135)
    Regress_graph_gs(set_gs, batch)   -> lt1(mean-pool of masked subgraph rows)      (:189-204)
Each layer is conv -> ELU -> dropout(p=0.5) (network.py:31-33); GCN layers run that as one GEMM plus one
SpMM with a fused epilogue.  The *_gs classes evaluate all subgraphs of a batch as ONE block-diagonal
pass instead of the reference's Python double loop (identical arithmetic: subgraphs share no edges).
"""
import collections

import torch
import torch.nn.functional as F
from torch import nn

from . import nn as fnn
from . import ops


def _make_convs(args):
    cls = getattr(fnn, args.layer_name, None)
    if cls is None:
        raise AttributeError(f"fitgnn_amd.nn has no layer '{args.layer_name}'")
    convs = nn.ModuleList()
    dims = [args.num_features] + [args.hidden] * args.num_layers1
    heads = int(getattr(args, "heads", 1)) if args.layer_name == "GATConv" else 1   # (an extension: the reference passes one head)
    if heads < 1:
        raise ValueError(f"heads = {heads}: a GATConv layer has at least one attention head")
    if args.hidden % heads != 0:
        raise ValueError(f"hidden = {args.hidden} is not a multiple of heads = {heads}: every GATConv layer is "
                         "GATConv(in, hidden // heads, heads=heads), its output hidden wide")
    for i in range(args.num_layers1):
        if args.layer_name == "GINConv":  # network.py:19-21: two-layer ReLU MLP, train_eps=True
            mlp = nn.Sequential(fnn.Linear(dims[i], args.hidden), nn.ReLU(), fnn.Linear(args.hidden, args.hidden), nn.ReLU())
            convs.append(cls(mlp, train_eps=True))
        elif heads > 1:
            convs.append(cls(dims[i], args.hidden // heads, heads=heads))
        else:
            convs.append(cls(dims[i], dims[i + 1]))
    return convs


def _one_head_gat(conv):
    """conv is a GATConv that runs the single-head kernels (ops.GATAggregate: fused epilogue, links, de-duplicated table, loss rows)."""
    return isinstance(conv, fnn.GATConv) and conv.heads == 1


# How a hidden layer runs conv -> ELU -> dropout (network.py:31-33) ...
_GCN = "gcn"                 # ops.FusedGCNLayer (GCNConv.forward_elu_dropout)
_GCN_NARROW = "gcn narrow"   # ops.FusedGCNLayerAggregatedInput: a narrow static input (QM9's 11 atom features), A_hat x formed once
_GCN_TABLE = "gcn table"     # ops.FusedGCNLayerDedup: layer 0 on the de-duplicated feature table
_GAT_TABLE = "gat table"     # a one-head GATConv.forward_elu_dropout on the table
_GAT = "gat"                 # GATConv.forward_elu_dropout: one head fused (ops.GATAggregate), more heads as torch operations
_PLAIN = "plain"             # conv, F.elu and F.dropout as they stand, for any layer class; an injected mask is ignored
_GCN_KINDS = (_GCN, _GCN_NARROW, _GCN_TABLE)
# ... and how the stack ends
_EMBED = "embed"                  # with its last layer: the embedding is the result
_HEAD = "head"                    # head(embedding)
_GCN_HEAD = "gcn + head"          # ops.FusedGCNLayerHead
_GCN_LOSS_ROWS = "gcn loss rows"  # ops.FusedGCNLastLayerRows
_GAT_LOSS_ROWS = "gat loss rows"  # ops.FusedGATLastLayerRows
_GCN_POOLED_ROWS = "gcn pooled rows"   # ops.FusedGCNLayerRows
_GCN_OUT_ROWS = "gcn out rows"    # (A_hat[rows] h) W^T, activation and head as torch operations

# What one forward runs, decided before any launch.  hidden: (kind, linked) per hidden layer -- every layer under _EMBED / _HEAD, all
# but the last otherwise; linked: the layer shares an ops.EpilogueLink with its one consumer (the next layer or the tail).  gather: a
# feature table is gathered to the union rows first (no layer 0 that reads it through the row index).
# embed_rules: the hidden layers run as embed() runs them -- a narrow-input first GCN layer as _GCN_NARROW, an attention layer as _GAT
# (its injected mask honoured).  Without (under a GCN tail with the head fused in, and under out_rows) a narrow first layer is a plain
# _GCN and an attention layer off the table is _PLAIN (its mask ignored): kept as found, wanted or not.
_Plan = collections.namedtuple("_Plan", "hidden tail gather embed_rules")


class _Base(nn.Module):
    out_dim_from_classes = True

    def __init__(self, args):
        super().__init__()
        self.num_layers = args.num_layers1
        self.conv = _make_convs(args)
        self.lt1 = nn.Linear(args.hidden, args.num_classes if self.out_dim_from_classes else 1)
        self.dropout_p = float(getattr(args, "dropout", 0.5))  # F.dropout's default p, which is what the reference uses
        self._inject_masks = None  # tests: list of uint8 masks, one per layer
        self.op_config = ops.DEFAULT

    def set_op_config(self, cfg):
        """Run this model's kernels under `cfg` (ops.OpConfig): GEMM policy, kernel A/B switches, profiling hooks, seed
        bank.  Per model: two models in one process keep their own."""
        self.op_config = cfg
        for m in self.modules():
            if isinstance(m, fnn._OpConfigured):
                m.op_config = cfg
        return self

    def reset_parameters(self):
        for m in self.conv:
            m.reset_parameters()
        self.lt1.reset_parameters()

    def _mask(self, i):
        """The dropout mask injected for layer i (tests), else None."""
        return self._inject_masks[i] if self._inject_masks is not None else None

    def _dropout(self, i):
        """(p, training, seed, mask) of layer i's dropout as the fused nodes take them; draws the layer's seed (ops.dropout_seed)."""
        mask = self._mask(i)
        return float(self.dropout_p), bool(self.training), ops.dropout_seed(self.op_config, self.training, self.dropout_p, mask), mask

    def _plan(self, x, x_index=None, out_rows=None, loss_rows=None, pooled_rows=None, head=True):
        """The _Plan of one forward over input x (x_index: x is a table), from what is known before any launch.  head=False: stop at
        the embedding (embed(); with pooled_rows, the last layer on those rows where that applies, else tail _EMBED)."""
        L, cfg, cuda, conv = self.num_layers, self.op_config, x.is_cuda, self.conv
        top = conv[L - 1] if L > 0 else None

        def head_fusable():
            return ops.head_fusable(self.lt1.in_features, self.lt1.out_features)

        def on_loss_rows():   # the last layer's dense part and the head on the loss rows alone: the hint, and shapes the row kernels take
            W = top.lin.weight
            return (loss_rows is not None and cfg.last_layer_on_loss_rows and loss_rows.numel() > 0 and W.shape[0] % 4 == 0
                    and W.shape[1] % 4 == 0 and ops.head_rows_supported(x.new_empty((1, W.shape[0])), self.lt1.weight))

        if out_rows is not None:
            if not isinstance(top, fnn.GCNConv):
                raise NotImplementedError("out_rows needs a GCNConv last layer")
            tail = _GCN_OUT_ROWS
        elif pooled_rows is not None:
            ok = (cfg.pooled_rows_last_layer and cuda and isinstance(top, fnn.GCNConv) and pooled_rows.dtype == torch.int64
                  and pooled_rows.numel() > 0 and top.lin.weight.shape[0] % 4 == 0 and all(isinstance(c, (fnn.GCNConv, fnn.GATConv)) for c in conv))
            tail = _GCN_POOLED_ROWS if ok else _EMBED
        elif not head:
            tail = _EMBED
        elif cuda and isinstance(top, fnn.GCNConv) and head_fusable():
            tail = _GCN_LOSS_ROWS if on_loss_rows() else _GCN_HEAD
        elif (cuda and _one_head_gat(top) and on_loss_rows() and head_fusable()
                and (L == 1 or isinstance(conv[L - 2], (fnn.GATConv, fnn.GCNConv)))):
            tail = _GAT_LOSS_ROWS
        else:
            tail = _HEAD
        embed_rules = tail not in (_GCN_HEAD, _GCN_LOSS_ROWS, _GCN_OUT_ROWS)
        table = x_index is not None and L > 1   # (a lone layer is the tail or reads gathered rows)

        def kind(i):
            c = conv[i]
            if not cuda:
                return _PLAIN
            if isinstance(c, fnn.GCNConv):
                if i == 0 and table:
                    return _GCN_TABLE
                return _GCN_NARROW if (i == 0 and embed_rules and ops.narrow_input_supported(x, c.lin.weight, cfg)) else _GCN
            if i == 0 and table and _one_head_gat(c) and (tail == _GCN_OUT_ROWS or not isinstance(conv[1], fnn.GCNConv)):
                return _GAT_TABLE
            return _GAT if (embed_rules and isinstance(c, fnn.GATConv)) else _PLAIN

        def linked(a, b, i):
            """Layer i of kind a and its consumer of kind b share a link: consecutive fused GCN layers (the backward GEMM dH @ W of layer
            i+1 applies layer i's ELU' / dropout' in its epilogue), and a one-head attention layer right below the aggregate-first
            attention tail (which hands them to that layer's adjoint aggregation).  None under out_rows."""
            if tail == _GCN_OUT_ROWS:
                return False
            if a in _GCN_KINDS:   # (the pooled-rows tail: only from a 4-column aligned layer below)
                return b in (_GCN, _GCN_HEAD, _GCN_LOSS_ROWS) or (b == _GCN_POOLED_ROWS and top.lin.weight.shape[1] % 4 == 0)
            return a in (_GAT, _GAT_TABLE) and b == _GAT_LOSS_ROWS and _one_head_gat(conv[i])

        kinds = [kind(i) for i in range(L if tail in (_EMBED, _HEAD) else L - 1)]
        hidden = tuple((a, linked(a, b, i)) for i, (a, b) in enumerate(zip(kinds, kinds[1:] + [tail])))
        gather = x_index is not None and not (kinds and kinds[0] in (_GCN_TABLE, _GAT_TABLE))
        return _Plan(hidden, tail, gather, embed_rules)

    def _hidden(self, plan, x, edge_index, x_index=None, first=0, last=None, link=None):
        """The layer loop: conv -> ELU -> dropout for the hidden layers first .. last - 1 of `plan` (default: all), seeds drawn in layer
        order.  Returns the result and the link its last layer recorded for the tail (None: the tail takes the plain gradient)."""
        cfg, p, training = self.op_config, self.dropout_p, self.training
        x = x.float()
        if plan.gather:
            x = x.index_select(0, x_index.index.long())  # materialise the union rows
        for i in range(first, len(plan.hidden) if last is None else last):
            conv, (how, linked) = self.conv[i], plan.hidden[i]
            nxt = ops.EpilogueLink() if linked else None
            if how == _GCN:
                x = conv.forward_elu_dropout(x, edge_index, p=p, training=training, mask=self._mask(i), link_in=link, link_out=nxt)
            elif how == _GCN_NARROW:
                ax = ops.aggregated_input(conv.graph(edge_index, x.shape[0]), x, cfg)
                x = ops.FusedGCNLayerAggregatedInput.apply(ax, conv.lin.weight, conv.bias, *self._dropout(i), nxt, cfg)
            elif how == _GCN_TABLE:
                g = conv.graph(edge_index, int(x_index.index.numel()))
                x = ops.FusedGCNLayerDedup.apply(x, conv.lin.weight, conv.bias, g, x_index, *self._dropout(i), nxt, cfg)
            elif how in (_GAT, _GAT_TABLE):
                x = conv.forward_elu_dropout(x, edge_index, p=p, training=training, mask=self._mask(i),
                                             x_index=x_index if how == _GAT_TABLE else None, link_out=nxt)
            else:
                x = F.dropout(F.elu(conv(x, edge_index)), p=p, training=training)
            link = nxt
        return x, link

    def prepare_static(self, x, edge_index, pooled_rows=None):
        """Form ahead of time what the layers keep per (graph, input) -- A_hat x of a narrow static input (ops.aggregated_input), the
        compact positions of the pooled rows (ops.FusedGCNLayerRows' backward) -- e.g. before the steps over a
        set of static batches are captured in hipGraphs: made lazily inside a step they would be captured and replayed with it."""
        if not (torch.is_tensor(x) and x.is_cuda):
            return
        # (A_hat x is kept per input TENSOR: an input of another dtype is converted anew every step, nothing to warm)
        hidden = self._plan(x, head=False).hidden
        if x.dtype == torch.float32 and hidden and hidden[0][0] == _GCN_NARROW:
            ops.aggregated_input(self.conv[0].graph(edge_index, x.shape[0]), x, self.op_config)
        if pooled_rows is not None and self._plan(x, pooled_rows=pooled_rows, head=False).tail == _GCN_POOLED_ROWS:
            ops.compact_positions(self.conv[self.num_layers - 1].graph(edge_index, x.shape[0]), pooled_rows)

    def embed(self, x, edge_index, x_index=None, first=0, link=None, last=None):
        """conv -> ELU -> dropout, layers first .. last - 1 (default: all; network.py:29-33).  link: the EpilogueLink recorded by the
        layer that produced x (consecutive fused GCN layers are linked: see ops.EpilogueLink; the stack is strictly sequential)."""
        return self._hidden(self._plan(x, head=False), x, edge_index, first=first, last=last, link=link)[0]

    def embed_pooled_rows(self, x, edge_index, rows):
        """embed() for a consumer that reads only `rows` of the result (the *_graph_gs models' pool over x[mask], network.py:129-131,
        :200-202): the last GCN layer aggregate-first on those rows, output compact [len(rows), hidden] (ops.FusedGCNLayerRows).
        None where that does not apply (the caller then embeds every row)."""
        plan = self._plan(x, pooled_rows=rows, head=False)
        if plan.tail != _GCN_POOLED_ROWS:
            return None
        h, link = self._hidden(plan, x, edge_index)
        top = self.conv[self.num_layers - 1]
        g = top.graph(edge_index, h.shape[0])
        return ops.FusedGCNLayerRows.apply(h, top.lin.weight, top.bias, g, *self._dropout(self.num_layers - 1), rows, self.op_config, link)

    def embed_and_head(self, x, edge_index, x_index=None, out_rows=None, loss_rows=None, compact_logits=False, forward_rows_only=False):
        """embed() followed by lt1; on the GPU the last GCN layer and the head form one autograd node.
        x_index (ops.RowIndex, optional): x is a de-duplicated table and union row r is table row x_index.index[r].
        out_rows (csr.RowSubset, optional): return the head's output on those rows only.  The last layer is then
        evaluated as (A_hat[rows] h) W^T -- aggregation first, on the kept rows, so that its GEMM, activation and the
        head run on len(rows) rows instead of all of them (same values on those rows: A (h W^T) = (A h) W^T).
        loss_rows (int64 index tensor, optional): the caller's promise that only these rows of the result reach its loss
        (run.py:193-204 keeps out[mask]), i.e. that the gradient it sends back is zero elsewhere; the head's weight and bias
        gradients are then reduced over those rows alone, and the head itself is evaluated on those rows alone (the result is
        zero on the others; the GCN layers still compute every row).
        compact_logits (with loss_rows): the caller accepts the result as [len(loss_rows), C] (the logits of those rows, in their
        order) when the last layer runs on the loss rows -- check the returned shape: other paths return all rows.
        forward_rows_only (with loss_rows, sorted ascending): the last layer's forward aggregation runs on the loss rows alone
        (A_hat[rows, :] h: the rows nobody reads are not computed at all -- the pruned step); ignored where the aggregate-first
        last layer does not apply."""
        plan = self._plan(x, x_index, out_rows=out_rows, loss_rows=loss_rows)
        x, link = self._hidden(plan, x, edge_index, x_index)
        if plan.tail == _HEAD:
            return self.head(x)
        L, cfg, lt1 = self.num_layers, self.op_config, self.lt1
        top = self.conv[L - 1]
        if plan.tail == _GCN_OUT_ROWS:
            agg = ops.SpMMRows.apply(x, out_rows, cfg)                   # [m, H_in]
            z = ops.Linear.apply(agg, top.lin.weight, cfg)
            if top.bias is not None:
                z = z + top.bias
            mask = self._mask(L - 1)
            z = F.elu(z)
            if mask is not None and self.training:
                z = z * mask.index_select(0, out_rows.rows).to(z.dtype) / (1.0 - self.dropout_p)
            else:
                z = F.dropout(z, p=self.dropout_p, training=self.training)
            return self.head(z)
        drop = self._dropout(L - 1)   # (the tail's draw comes last)
        if plan.tail == _GAT_LOSS_ROWS:
            # the last attention layer aggregate-first: its dense part on the loss rows only
            g = fnn.csr_for(edge_index, x.shape[0], "gat")
            return ops.FusedGATLastLayerRows.apply(x, top.lin.weight, top.att_src.view(-1), top.att_dst.view(-1), top.bias, lt1.weight, lt1.bias,
                                                   g, top.negative_slope, *drop, loss_rows, cfg, bool(compact_logits), link)
        g = top.graph(edge_index, x.shape[0])
        if plan.tail == _GCN_LOSS_ROWS:
            # aggregate first, then the dense part on the loss rows only; the previous layer's epilogue backward rides on the
            # backward SpMM's store (link).  forward_rows_only: A_hat[rows, :] and its tiles, built once per (graph, loss rows)
            fwd_sub = ops.rows_forward_subset(g, loss_rows) if forward_rows_only else None
            return ops.FusedGCNLastLayerRows.apply(x, top.lin.weight, top.bias, lt1.weight, lt1.bias, g, *drop, loss_rows, cfg, link,
                                                   bool(compact_logits), fwd_sub)
        return ops.FusedGCNLayerHead.apply(x, top.lin.weight, top.bias, lt1.weight, lt1.bias, g, *drop, link, cfg, loss_rows)

    def head(self, x):
        """lt1 (network.py:34): same parameters as nn.Linear, evaluated as mm + broadcast add."""
        if x.is_cuda:
            return ops.SmallLinear.apply(x, self.lt1.weight, self.lt1.bias, self.op_config)
        return self.lt1(x)


class Classify_node(_Base):
    def forward(self, x, edge_index, x_index=None):
        return F.log_softmax(self.embed_and_head(x, edge_index, x_index), dim=1)


class Regress_node(_Base):
    out_dim_from_classes = False

    def forward(self, x, edge_index, x_index=None):
        return self.embed_and_head(x, edge_index, x_index)


class APPNPNet(nn.Module):
    """The APPNP model north_star names beside GCN / GAT: Baselines/SGGC/APPNP/networks.py:7-27 (`Net`), same attributes
    (`lin1`, `lin2`, `prop1`) and forward: dropout -> lin1 -> ReLU -> dropout -> lin2 -> APPNP(K, alpha) -> log_softmax.
    args: num_features, hidden, num_classes, K (default 10), alpha (default 0.1) (networks.py:9-11).
    x_index (ops.RowIndex, optional): x is a de-duplicated feature table and union row r is table row x_index.index[r] -- the MLP
    is per node, so it runs on the table and its class-wide output is gathered to the union rows before the propagation (in
    training mode the copies of a node then share its dropout draw)."""

    def __init__(self, args):
        super().__init__()
        self.lin1 = fnn.Linear(args.num_features, args.hidden)
        self.lin2 = fnn.Linear(args.hidden, args.num_classes)
        self.prop1 = fnn.APPNP(int(getattr(args, "K", 10)), float(getattr(args, "alpha", 0.1)))
        self.dropout_p = float(getattr(args, "dropout", 0.5))
        self.op_config = ops.DEFAULT

    def set_op_config(self, cfg):
        self.op_config = cfg
        for m in self.modules():
            if isinstance(m, fnn._OpConfigured):
                m.op_config = cfg
        return self

    def reset_parameters(self):
        self.lin1.reset_parameters()
        self.lin2.reset_parameters()

    def logits(self, x, edge_index, x_index=None):
        """forward() without its log_softmax: a trainer whose loss reads a few rows (run.py:193-204 keeps out[mask]) takes the
        softmax and the NLL on those rows only (ops.SoftmaxNLL) instead of normalising every union row twice."""
        x = F.dropout(x.float(), p=self.dropout_p, training=self.training)
        x = F.relu(self.lin1(x))
        x = F.dropout(x, p=self.dropout_p, training=self.training)
        x = self.lin2(x)
        return self.prop1(x, edge_index, x_index=x_index)   # (the table's rows are gathered into the propagation's own layout there)

    def forward(self, x, edge_index, x_index=None):
        return F.log_softmax(self.logits(x, edge_index, x_index), dim=1)


class Classify_graph_gc(_Base):
    def forward(self, gc):
        x = self.embed(gc.x, gc.edge_index)
        return F.softmax(self.head(fnn.global_max_pool(x, gc.batch, getattr(gc, "num_graphs", None))), dim=1)


def _mean_pool_head(model, x, batch, size, rows=None):
    """lt1(global_mean_pool(x[rows])): one launch each way on the GPU (ops.MeanPoolHead) when the batch vector is sorted and the
    shapes allow it, else the pool followed by the head."""
    if (model.op_config.fused_pool_head and size is not None and ops.pool_head_supported(x, model.lt1.weight)
            and batch.dtype == torch.int64):
        pi = ops.pool_index(batch, size, rows, x.shape[0])
        if pi.sorted:
            return ops.MeanPoolHead.apply(x, pi, model.lt1.weight, model.lt1.bias, model.op_config)
    if rows is not None:
        return model.head(fnn.global_mean_pool(x, batch, size, rows=rows))
    return model.head(fnn.global_mean_pool(x, batch, size))


class Regress_graph_gc(_Base):
    out_dim_from_classes = False

    def forward(self, gc):
        x = self.embed(gc.x, gc.edge_index)
        return _mean_pool_head(self, x, gc.batch.to(torch.int64), getattr(gc, "num_graphs", None))


def _merge_subgraphs(set_gs, device):
    """Block-diagonal union of every subgraph of every graph in the batch (reference: nested Python loops,
    network.py:120-130); returns x, edge_index, row mask in the reference's concatenation order."""
    xs, eis, masks, off = [], [], [], 0
    for gs in set_gs:
        for g in gs:
            xs.append(g.x.to(device).float())
            eis.append(g.edge_index.to(device) + off)
            masks.append(g.mask.to(device))
            off += g.x.shape[0]
    return torch.cat(xs, 0), torch.cat(eis, 1), torch.cat(masks, 0)


def _gs_inputs(set_gs, batch_tensor):
    """Reference form (list of per-graph lists of subgraph Data, network.py:120-130) or the pre-merged union a
    fitgnn_amd.graph_data.GraphSet batch carries (dict with x, edge_index, mask)."""
    if isinstance(set_gs, dict):
        return set_gs["x"], set_gs["edge_index"], set_gs.get("mask_idx", set_gs["mask"]), set_gs.get("n_graphs")
    return _merge_subgraphs(set_gs, batch_tensor.device) + (None,)


def _pooled_rows_ok(set_gs, mask):
    """The pooled rows come as a precomputed int64 index (GraphSet batches) and the batch does not opt out."""
    return isinstance(set_gs, dict) and mask is not None and mask.dtype == torch.int64 and not set_gs.get("_no_pooled_rows", False)


def _take(x, mask):
    """x[mask] for a bool mask, or index_select for a precomputed index (no host sync: usable under graph capture)."""
    return x.index_select(0, mask) if mask.dtype == torch.int64 else x[mask]


def _pool_rows(pool, x, mask, batch_tensor, size):
    """pool(x[mask]) per graph (network.py:129-131, :200-202); a precomputed row index (GraphSet batches) is folded into the pool."""
    if mask.dtype == torch.int64 and x.is_cuda:
        return pool(x, batch_tensor.to(torch.int64), size, rows=mask)
    return pool(_take(x, mask), batch_tensor.to(torch.int64), size)


class Classify_graph_gs(_Base):
    def forward(self, set_gs, batch_tensor):
        x, ei, mask, size = _gs_inputs(set_gs, batch_tensor)
        hc = self.embed_pooled_rows(x, ei, mask) if _pooled_rows_ok(set_gs, mask) else None
        if hc is not None:   # the last layer on the pooled rows only: the pool runs over the compact rows
            x = self.head(fnn.global_max_pool(hc, batch_tensor.to(torch.int64), size))
        else:
            x = self.head(_pool_rows(fnn.global_max_pool, self.embed(x, ei), mask, batch_tensor, size))
        return F.softmax(x, dim=0 if x.dim() == 1 else 1)


class Regress_graph_gs(_Base):
    out_dim_from_classes = False

    def forward(self, set_gs, batch_tensor):
        x, ei, mask, size = _gs_inputs(set_gs, batch_tensor)
        hc = self.embed_pooled_rows(x, ei, mask) if _pooled_rows_ok(set_gs, mask) else None
        if hc is not None:   # the last layer on the pooled rows only: pool and head over the compact rows
            return _mean_pool_head(self, hc, batch_tensor.to(torch.int64), size)
        h = self.embed(x, ei)
        if mask.dtype == torch.int64 and h.is_cuda:   # a precomputed row index (GraphSet batches): pool and head in one launch
            return _mean_pool_head(self, h, batch_tensor.to(torch.int64), size, rows=mask)
        return self.head(_pool_rows(fnn.global_mean_pool, h, mask, batch_tensor, size))
