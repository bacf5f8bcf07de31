"""What every model of fitgnn_amd.network runs: the cases of tests/test_gpu_model_dispatch.py and the record each one leaves
(test infrastructure only; tests/golden/make_model_dispatch_golden.py writes the records to tests/golden/model_dispatch.json).

A record holds, for one (case, mode):
  nodes  the autograd nodes reachable from the model's output, depth first along grad_fn.next_functions in their order, every node
         once: the fitgnn_amd.ops Functions and AccumulateGrad (with the parameter's name);
  kinds  the launch kinds OpConfig.profile collected over forward and backward, in order;
  gemms  the kernel names OpConfig.profile_gemm collected;
  out, grads  sha256 of the output's bytes and (its first 16 hex digits) of every parameter gradient's bytes after one backward() of
         a fixed loss (nll_loss / l1_loss, reduction="sum") -- the kernels use no atomics, so a re-run reproduces the bits.
Every case runs once unrecorded first, so that what the layers keep per (graph, input) exists whatever ran before.
"""
import argparse
import hashlib
import types

import numpy as np
import torch

MODES = ("eval", "masks", "hashed")
HIDDEN = 64


def _case(model="Classify_node", layer="GCNConv", layers=2, features=24, classes=5, heads=1, swap=None, table=False, cfg=None, **hints):
    """swap: {i: the layer class conv[i] is replaced by} (a mixed stack).  hints: loss_rows / out_rows (True: the batch's train rows),
    compact_logits, forward_rows_only, wide_head (one class more than the fused head backward takes), no_pooled_rows."""
    return dict(model=model, layer=layer, layers=layers, features=features, classes=classes, heads=heads, swap=swap, table=table,
                cfg=cfg or {}, hints=hints)


def _cases():
    c = {}
    rows = dict(loss_rows=True, compact_logits=True)
    c["gcn2-plain"] = _case()
    c["gcn2-table-rows"] = _case(table=True, **rows)
    c["gcn2-table-rows-forward-only"] = _case(table=True, forward_rows_only=True, **rows)
    c["gcn2-table-rows-transform-first"] = _case(table=True, cfg=dict(last_layer_on_loss_rows=False), **rows)
    c["gcn2-table-rows-head-gradients-only"] = _case(table=True, cfg=dict(last_layer_on_loss_rows=False, compact_head_backward=False), **rows)
    for form, table in (("plain", False), ("table", True)):
        c[f"gcn2-{form}-out-rows"] = _case(table=table, out_rows=True)
        for L in (1, 3):
            c[f"gcn{L}-{form}-rows"] = _case(layers=L, table=table, loss_rows=True)
        for L in (2, 3):
            c[f"gat{L}-{form}"] = _case(layer="GATConv", layers=L, table=table)
            c[f"gat{L}-{form}-rows"] = _case(layer="GATConv", layers=L, table=table, **rows)
        c[f"gat2-heads4-{form}"] = _case(layer="GATConv", heads=4, table=table)
        c[f"sage2-{form}"] = _case(layer="SAGEConv", table=table)
        c[f"gin2-{form}"] = _case(layer="GINConv", table=table)
        c[f"gat-gcn-{form}"] = _case(layer="GATConv", swap={1: "GCNConv"}, table=table)
        c[f"gat-gcn-{form}-rows"] = _case(layer="GATConv", swap={1: "GCNConv"}, table=table, **rows)
        c[f"gcn-gat-{form}"] = _case(swap={1: "GATConv"}, table=table)
        c[f"gcn-gat-{form}-rows"] = _case(swap={1: "GATConv"}, table=table, **rows)
        c[f"gat-gcn-{form}-out-rows"] = _case(layer="GATConv", swap={1: "GCNConv"}, table=table, out_rows=True)
        c[f"gat-gat-gcn-{form}"] = _case(layer="GATConv", layers=3, swap={2: "GCNConv"}, table=table)
        c[f"gat-gat-gcn-{form}-rows"] = _case(layer="GATConv", layers=3, swap={2: "GCNConv"}, table=table, **rows)
        c[f"gcn-gcn-gat-{form}-rows"] = _case(layers=3, swap={2: "GATConv"}, table=table, **rows)
        c[f"gcn-gat-gat-{form}-rows"] = _case(layers=3, swap={1: "GATConv", 2: "GATConv"}, table=table, **rows)
    c["gat2-heads4-table-rows"] = _case(layer="GATConv", heads=4, table=True, **rows)
    c["sage2-table-rows"] = _case(layer="SAGEConv", table=True, **rows)
    c["gcn2-wide-head"] = _case(wide_head=True)
    c["gcn2-wide-head-table"] = _case(wide_head=True, table=True)
    c["gcn3-wide-head"] = _case(layers=3, wide_head=True)
    c["gcn2-regress-node"] = _case(model="Regress_node", classes=1)
    c["gcn2-narrow-input"] = _case(features=11)
    c["gcn2-narrow-input-regress-gc"] = _case(model="Regress_graph_gc", features=11, classes=1)
    c["classify-gc"] = _case(model="Classify_graph_gc", features=3, classes=2)
    for m, F, C in (("Classify_graph_gs", 3, 2), ("Regress_graph_gs", 11, 1)):
        n = m.split("_")[0].lower() + "-gs"
        c[f"{n}-gcn2"] = _case(model=m, features=F, classes=C)
        c[f"{n}-gcn3"] = _case(model=m, layers=3, features=F, classes=C)
        c[f"{n}-gcn2-no-pooled-rows"] = _case(model=m, features=F, classes=C, no_pooled_rows=True)
        c[f"{n}-gat2"] = _case(model=m, layer="GATConv", features=F, classes=C)
        c[f"{n}-gcn1-11-features"] = _case(model=m, layers=1, features=11, classes=C)
    return c


CASES = _cases()
_shared = {}


def _node_batch():
    if "node" not in _shared:
        from graph_fixtures import subgraph_batches
        from fitgnn_amd.csr import RowSubset

        batch, _ = subgraph_batches(seed=9)
        _shared["node"] = (batch, batch.x[:, :11].contiguous(), RowSubset(batch.graph, batch.train_idx))
    return _shared["node"]


def _graph_batch(features, kind):
    """Six graphs of fewer than 30 nodes each, as the one GraphSet batch a trainer would hand the model."""
    if (features, kind) not in _shared:
        from fitgnn_amd import graph_data, train

        if features not in _shared:   # (one coarsening serves the subgraph view and the coarse view)
            mol = (graph_data.synthetic_molecules if features == 11 else graph_data.synthetic_graph_classes)(6, seed=8)
            assert int(np.diff(mol["node_ptr"]).max()) < 30
            _shared[features] = graph_data.GraphSet(mol, ratio=0.5, extra_node=True, device="cuda")
        _shared[features, kind] = train._cat_pieces([_shared[features].batch(0, 6, kind)], kind, types)
    return _shared[features, kind]


def _model(case):
    from fitgnn_amd import network, ops
    from fitgnn_amd import nn as fnn

    classes = ops.head_max_classes_wide() + 1 if case["hints"].get("wide_head") else case["classes"]
    if case["hints"].get("wide_head"):
        assert not ops.head_fusable(HIDDEN, classes)
    args = argparse.Namespace(num_layers1=case["layers"], layer_name=case["layer"], num_features=case["features"], hidden=HIDDEN,
                              num_classes=classes, heads=case["heads"])
    torch.manual_seed(1)
    model = getattr(network, case["model"])(args)
    for i, cls in (case["swap"] or {}).items():
        model.conv[i] = getattr(fnn, cls)(HIDDEN, HIDDEN)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.normal_(std=0.1)
    return model.cuda(), classes


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _nodes(out, model):
    from fitgnn_amd import ops

    names = {id(p): k for k, p in model.named_parameters()}
    seen, found, stack = set(), [], [out.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        name = type(fn).__name__
        if name == "AccumulateGrad":
            found.append(f"AccumulateGrad({names.get(id(fn.variable), '?')})")
        elif name.endswith("Backward") and isinstance(getattr(ops, name[:-len("Backward")], None), type):
            found.append(name[:-len("Backward")])
        stack.extend(f for f, _ in reversed(fn.next_functions))
    return found


def record(name, mode):
    """Run CASES[name] in `mode` and return its record."""
    from fitgnn_amd import ops

    case, hints = CASES[name], CASES[name]["hints"]
    model, classes = _model(case)
    node_level = case["model"] in ("Classify_node", "Regress_node")
    if node_level:
        batch, x11, sub = _node_batch()
        n_rows, idx = batch.n_rows, batch.train_idx
    else:
        kind = "gs" if case["model"].endswith("_gs") else "gc"
        b = _graph_batch(case["features"], kind)
        if hints.get("no_pooled_rows"):
            b = dict(b, _no_pooled_rows=True)
        n_rows = int(b["x"].shape[0])
    model.train(mode != "eval")
    if mode == "masks":
        gen = torch.Generator().manual_seed(7)
        model._inject_masks = [(torch.rand(n_rows, HIDDEN, generator=gen) > 0.5).to(torch.uint8).cuda() for _ in range(case["layers"])]

    def run(cfg):
        model.set_op_config(cfg)
        model.zero_grad()
        torch.manual_seed(11)
        if node_level:
            kw = {}
            if hints.get("loss_rows"):
                kw = dict(loss_rows=idx, compact_logits=bool(hints.get("compact_logits")), forward_rows_only=bool(hints.get("forward_rows_only")))
            if hints.get("out_rows"):
                kw = dict(out_rows=sub)
            if case["table"]:
                out = model.embed_and_head(batch.x_table, batch.edge_index, batch.row_index, **kw)
            else:
                out = model.embed_and_head(x11 if case["features"] == 11 else batch.x, batch.edge_index, **kw)
            z = out if out.shape[0] == idx.numel() else out.index_select(0, idx)
            y = batch.y.index_select(0, idx)
            if case["model"] == "Regress_node":
                loss = torch.nn.functional.l1_loss(z.flatten(), y.float(), reduction="sum")
            else:
                loss = torch.nn.functional.nll_loss(torch.log_softmax(z, 1), y % classes, reduction="sum")
        else:
            out = model(b, b["graph_of_masked"]) if kind == "gs" else model(b["gc"])
            if case["model"].startswith("Regress"):
                loss = torch.nn.functional.l1_loss(out.flatten(), torch.arange(out.shape[0], device=out.device) * 0.5, reduction="sum")
            else:
                loss = torch.nn.functional.nll_loss(torch.log(out), torch.arange(out.shape[0], device=out.device) % classes, reduction="sum")
        loss.backward()
        torch.cuda.synchronize()
        return out

    run(ops.OpConfig(**case["cfg"]))
    cfg = ops.OpConfig(profile=[], profile_gemm=[], **case["cfg"])
    out = run(cfg)
    return dict(nodes=_nodes(out, model), kinds=[e[2] for e in cfg.profile], gemms=[e[2] for e in cfg.profile_gemm], out=_sha(out),
                grads={k: ("none" if p.grad is None else _sha(p.grad)[:16]) for k, p in model.named_parameters()})


def key(name, mode):
    return f"{name}/{mode}"
