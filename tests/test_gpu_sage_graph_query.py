"""GPU tier: fitgnn_amd.serve.GraphQueryEngine(model, gset, sage_kernels=True) for a model of two SAGEConv layers (random non-zero
biases) -- graph ids in, predictions out through fitgnn_sage_graph_query_hops_f32 and fitgnn_gcn_graph_query_tail_f32 with K = 2H --
against the float64 forward of tests/sage_graph_query_reference.model_forward (the oracle's sage_conv stack on the whole view, the
per-graph pool, the head, the softmax) and against the model's own forward on GraphSet.batch_ids, on the dozen-graph sets and the ids of
tests/test_gpu_graph_query.py; the split of one call between the window and the per-row kernel; the prepared state's refresh on in-place
weight updates; the default and the fallbacks, which stay the model's own forward; the torch.ops binding; inference.py --query_engine
--query_sage on the graph-level tasks.  1e-4 relative, as the project's other engine tests hold."""
import os

import numpy as np
import pytest
import torch

import sage_graph_query_reference as sgq
from test_gpu_gat_graph_query import _same_csv_rows
from test_gpu_graph_query import IDS, N_GRAPHS, ROOT, _forward, _gset, _model, _view, mods  # noqa: F401  (mods: the module-scoped fixture)
from test_gpu_query import rel

pytestmark = pytest.mark.gpu


def _sage_model(network, cls, F, hidden, layers=2, seed=0):
    return _model(network, cls, F, hidden, layer="SAGEConv", layers=layers, seed=seed)   # random non-zero biases


def _oracle(gorc, model, gset, view, ids):
    """float64: the SAGE stack on the whole (block-diagonal) view, per graph the pool over its pooled rows, the head, the softmax."""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    x, ptr, ei, mask = _view(gset, view)
    keep = np.ones(int(ptr[-1]), dtype=bool) if mask is None else mask.cpu().numpy()
    seg, prow, pptr = [], [], [0]
    for g in ids:
        rows = np.arange(int(ptr[g]), int(ptr[g + 1]))
        seg.append((int(ptr[g]), int(ptr[g + 1])))
        prow += rows[keep[rows]].tolist()
        pptr.append(len(prow))
    classify = type(model).__name__.startswith("Classify")
    out = sgq.model_forward(gorc, sd, x.cpu(), ei.cpu(), seg, np.array(prow), pptr, "max" if classify else "mean", classify)
    return torch.from_numpy(out)


def _check(mods, model, gset, view, ids=IDS, **kw):
    graph_data, network, ops, serve, gorc = mods
    eng = serve.GraphQueryEngine(model, gset, view=view, sage_kernels=True, **kw)
    assert eng.fused is True and eng._kind() == "sage" and ops.sage_graph_query_supported(model) and not ops.graph_query_supported(model)
    out = eng.predict(ids)
    C = model.lt1.weight.shape[0]
    assert out.shape == (len(ids), C) and out.dtype == torch.float32
    v = eng.view
    r_oracle = rel(out.cpu().double(), _oracle(gorc, model, gset, v, ids))
    r_model = rel(out.cpu().double(), _forward(model, gset, v, ids).cpu().double())
    print(f"sage graph query {type(model).__name__} {v}: rel to the oracle {r_oracle:.3g}, to the model's forward {r_model:.3g}")
    assert r_oracle <= 1e-4
    assert r_model <= 1e-4
    assert torch.equal(out[1], out[3]) and torch.equal(out[0], out[6])      # the repeated graphs
    assert torch.equal(eng.predict(torch.tensor(ids, device="cuda")), out)  # host and device ids: equal bits
    assert torch.equal(eng.predict(np.asarray(ids)), out)
    n_rows = int(_view(gset, v)[1][-1])
    assert eng.table_bytes == n_rows * 2 * model.conv[0].lin_l.weight.shape[0] * 4      # T [n_rows, 2H]
    return eng, out


@pytest.mark.parametrize("hidden", [64, 512])
@pytest.mark.parametrize("cls,kind,view", [("Classify_graph_gs", "cls", "gs"), ("Classify_graph_gc", "cls", "gc"),
                                           ("Regress_graph_gs", "mol", "gs"), ("Regress_graph_gc", "mol", "gc")], ids=str)
def test_every_model_class_on_its_default_view(mods, cls, kind, view, hidden):
    graph_data, network = mods[:2]
    gset = _gset(graph_data, kind)
    model = _sage_model(network, cls, gset.x.shape[1], hidden)
    eng, out = _check(mods, model, gset, None)
    assert eng.view == view
    if cls.startswith("Classify"):
        assert float((out.sum(1) - 1).abs().max()) <= 1e-5 and out.shape[1] == 5
    else:
        assert out.shape[1] == 1


@pytest.mark.parametrize("hidden", [64, 512])
def test_the_baseline_on_the_uncoarsened_graphs(mods, hidden):
    graph_data, network = mods[:2]
    gset = _gset(graph_data, "cls")
    _check(mods, _sage_model(network, "Classify_graph_gc", gset.x.shape[1], hidden), gset, "orig")
    gm = _gset(graph_data, "mol")
    _check(mods, _sage_model(network, "Regress_graph_gc", gm.x.shape[1], hidden), gm, "orig")


@pytest.mark.parametrize("extra_node,cluster_node", [(False, False), (True, False), (False, True)], ids=["plain", "extra", "cluster"])
def test_the_subgraph_view_in_every_layout(mods, extra_node, cluster_node):
    graph_data, network = mods[:2]
    gset = _gset(graph_data, "mol", extra_node=extra_node, cluster_node=cluster_node)
    if extra_node or cluster_node:
        assert not bool(gset.gs_mask.all()), "every row pooled: the layout adds no rows"
    _check(mods, _sage_model(network, "Regress_graph_gs", gset.x.shape[1], 64), gset, "gs")
    _check(mods, _sage_model(network, "Classify_graph_gs", gset.x.shape[1], 64), gset, "gs")


def test_max_window_rows_4_splits_a_call_between_the_window_and_the_per_row_kernel(mods):
    """Uncoarsened graphs of 4 to 18 nodes: max_window_rows=4 sends the graphs of four rows through the window and the others through
    ops.sage_query_gather on their pooled rows (the same [g | h] layout), in one call, into one G in front of one tail."""
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "small")
    n_rows = np.diff(np.asarray(gset.node_ptr))
    ids = list(range(N_GRAPHS))[::-1] + [3, 0]
    fits = torch.from_numpy(n_rows[ids] <= 4)
    assert bool(fits.any()) and not bool(fits.all()), n_rows
    for cls in ("Classify_graph_gc", "Regress_graph_gc"):
        model = _sage_model(network, cls, gset.x.shape[1], 64)
        eng = serve.GraphQueryEngine(model, gset, view="orig", max_window_rows=4, sage_kernels=True)
        out = eng.predict(ids)
        assert eng.fused and eng._kind() == "sage"
        assert rel(out.cpu().double(), _oracle(gorc, model, gset, "orig", ids)) <= 1e-4
        assert rel(out.cpu().double(), _forward(model, gset, "orig", ids).cpu().double()) <= 1e-4
        whole = serve.GraphQueryEngine(model, gset, view="orig", sage_kernels=True).predict(ids)     # every graph in the window
        assert torch.equal(out[fits], whole[fits])                                # the window's graphs: the same arithmetic, the same bits
        assert rel(out.cpu().double(), whole.cpu().double()) <= 1e-4
    # the subgraph view of the same set under max_window_rows=3: every graph has more rows, all of them take the per-row kernel
    model = _sage_model(network, "Classify_graph_gs", gset.x.shape[1], 64)
    assert int(np.diff(np.asarray(gset.gs_ptr)).min()) > 3
    out = serve.GraphQueryEngine(model, gset, max_window_rows=3, sage_kernels=True).predict(ids)
    assert rel(out.cpu().double(), _oracle(gorc, model, gset, "gs", ids)) <= 1e-4


WEIGHTS = ["conv0.lin_l.weight", "conv0.lin_r.weight", "conv0.lin_l.bias", "conv1.lin_l.weight", "conv1.lin_r.weight", "conv1.lin_l.bias",
           "lt1.bias"]


@pytest.mark.parametrize("which", WEIGHTS)
def test_weight_update_is_picked_up(mods, which):
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "mol")
    model = _sage_model(network, "Regress_graph_gs", gset.x.shape[1], 64)
    eng = serve.GraphQueryEngine(model, gset, sage_kernels=True)
    before = eng.predict(IDS).clone()
    c0, c1 = model.conv
    p = {"conv0.lin_l.weight": c0.lin_l.weight, "conv0.lin_r.weight": c0.lin_r.weight, "conv0.lin_l.bias": c0.lin_l.bias,
         "conv1.lin_l.weight": c1.lin_l.weight, "conv1.lin_r.weight": c1.lin_r.weight, "conv1.lin_l.bias": c1.lin_l.bias,
         "lt1.bias": model.lt1.bias}[which]
    with torch.no_grad():
        p.mul_(-1.5).add_(0.3)     # in place: same storage, new version
    after = eng.predict(IDS)
    assert eng.fused and rel(after.cpu().double(), _oracle(gorc, model, gset, "gs", IDS)) <= 1e-4
    assert not torch.equal(after, before)
    # nothing stale is left: an engine built after the update, and a forced refresh, give the same bits
    assert torch.equal(serve.GraphQueryEngine(model, gset, sage_kernels=True).predict(IDS), after)
    assert torch.equal(eng.refresh().predict(IDS), after)


def test_copied_and_replaced_weights_are_picked_up(mods):
    """copy_ keeps the storage and bumps the version; a replaced lin_r.weight is a new storage: both remake T and [W_l1 | W_r1]."""
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "cls")
    model = _sage_model(network, "Classify_graph_gs", gset.x.shape[1], 64)
    other = _sage_model(network, "Classify_graph_gs", gset.x.shape[1], 64, seed=5)
    eng = serve.GraphQueryEngine(model, gset, sage_kernels=True)
    outs = [eng.predict(IDS).clone()]
    with torch.no_grad():
        model.conv[0].lin_l.weight.copy_(other.conv[0].lin_l.weight)
    outs.append(eng.predict(IDS).clone())
    assert rel(outs[-1].cpu().double(), _oracle(gorc, model, gset, "gs", IDS)) <= 1e-4
    model.conv[0].lin_r.weight = torch.nn.Parameter(other.conv[0].lin_r.weight.detach().clone())
    outs.append(eng.predict(IDS).clone())
    assert eng.fused and eng._kind() == "sage"
    assert rel(outs[-1].cpu().double(), _oracle(gorc, model, gset, "gs", IDS)) <= 1e-4
    model.conv[1].lin_r.weight = torch.nn.Parameter(other.conv[1].lin_r.weight.detach().clone())
    outs.append(eng.predict(IDS).clone())
    assert rel(outs[-1].cpu().double(), _oracle(gorc, model, gset, "gs", IDS)) <= 1e-4
    assert all(not torch.equal(a, b) for a, b in zip(outs, outs[1:]))
    assert torch.equal(serve.GraphQueryEngine(model, gset, sage_kernels=True).predict(IDS), outs[-1])


def test_default_is_unchanged(mods):
    """Without the flag a SAGE model takes its own forward."""
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "mol")
    model = _sage_model(network, "Regress_graph_gs", gset.x.shape[1], 64)
    eng = serve.GraphQueryEngine(model, gset)
    assert eng.sage_kernels is False and eng.fused is False and eng._kind() is None and eng.table_bytes == 0
    assert rel(eng.predict(IDS).cpu().double(), _forward(model, gset, "gs", IDS).cpu().double()) <= 1e-4
    assert rel(eng.predict(IDS).cpu().double(), _oracle(gorc, model, gset, "gs", IDS)) <= 1e-4
    others = serve.GraphQueryEngine(model, gset, gin_kernels=True, gat_kernels=True)
    assert others.fused is False and others.table_bytes == 0


@pytest.mark.parametrize("layer", ["GCNConv", "GINConv", "GATConv"])
def test_other_models_ignore_the_flag(mods, layer):
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "cls")
    model = _model(network, "Classify_graph_gs", gset.x.shape[1], 64, layer=layer)
    own = {"GINConv": dict(gin_kernels=True), "GATConv": dict(gat_kernels=True)}.get(layer, {})
    a = serve.GraphQueryEngine(model, gset, **own)
    b = serve.GraphQueryEngine(model, gset, sage_kernels=True, **own)
    assert a.fused is True and b.fused is True and b._kind() == a._kind() == {"GCNConv": "gcn", "GINConv": "gin", "GATConv": "gat"}[layer]
    assert a.table_bytes == b.table_bytes and torch.equal(a.predict(IDS), b.predict(IDS))
    if own:   # and without its own flag the model takes its own forward, whatever sage_kernels says
        c = serve.GraphQueryEngine(model, gset, sage_kernels=True)
        assert c.fused is False and c.table_bytes == 0


def test_three_layers_fall_back(mods):
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "mol")
    model = _sage_model(network, "Regress_graph_gs", gset.x.shape[1], 64, layers=3)
    assert not ops.sage_graph_query_supported(model)
    eng = serve.GraphQueryEngine(model, gset, sage_kernels=True)
    assert eng.fused is False and eng.table_bytes == 0
    assert rel(eng.predict(IDS).cpu().double(), _forward(model, gset, "gs", IDS).cpu().double()) <= 1e-4


def test_a_model_without_the_second_bias_still_answers(mods):
    """lin_l.bias = None on conv 1: the tail takes b1 = NULL."""
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "mol")
    model = _sage_model(network, "Regress_graph_gs", gset.x.shape[1], 64)
    model.conv[1].lin_l.bias = None
    assert "conv.1.lin_l.bias" not in model.state_dict()
    eng = serve.GraphQueryEngine(model, gset, sage_kernels=True)
    out = eng.predict(IDS)
    assert rel(out.cpu().double(), _oracle(gorc, model, gset, "gs", IDS)) <= 1e-4
    assert rel(out.cpu().double(), _forward(model, gset, "gs", IDS).cpu().double()) <= 1e-4


def test_torch_ops_hold_the_launcher(mods):
    graph_data, network, ops, serve, gorc = mods
    from fitgnn_amd import torch_ops  # noqa: F401  (registers torch.ops.fitgnn)
    gset = _gset(graph_data, "cls", extra_node=True)
    model = _sage_model(network, "Classify_graph_gs", gset.x.shape[1], 64)
    eng = serve.GraphQueryEngine(model, gset, sage_kernels=True)
    f = eng.csr().f
    T, W1cat = eng.state()
    assert T.shape == (eng.n_rows, 128) and T.is_contiguous() and W1cat.shape == (64, 128) and W1cat.is_contiguous()
    ids = np.asarray(IDS)
    seg = torch.from_numpy(np.stack([eng._ptr[ids], eng._ptr[ids + 1]], 1)).cuda()
    cnt = torch.from_numpy(eng._pp[ids + 1] - eng._pp[ids]).cuda()
    pptr = torch.cat([cnt.new_zeros(1), torch.cumsum(cnt, 0)])
    prow = torch.cat([eng._prow[int(eng._pp[g]):int(eng._pp[g + 1])] for g in IDS])
    max_rows = int((seg[:, 1] - seg[:, 0]).max())
    b0 = model.conv[0].lin_l.bias.detach()
    G = torch.ops.fitgnn.sage_graph_query_hops(f.rowptr, f.col, f.val, T, seg, prow, pptr, max_rows, None, b0)
    assert G.shape == (prow.numel(), 128)
    assert torch.equal(G, ops.sage_graph_query_hops(f.rowptr, f.col, f.val, T, seg, prow, pptr, max_rows, b0=b0))
    assert not torch.equal(G, ops.sage_graph_query_hops(f.rowptr, f.col, f.val, T, seg, prow, pptr, max_rows))   # the bias counts
    Gn = ops.sage_query_gather(f.rowptr, f.col, f.val, T, prow, b0=b0)          # the per-row kernel: the same sage_row, the same h half
    assert torch.equal(G[:, 64:], Gn[:, 64:])
    tail = [p.detach() for p in (W1cat, model.conv[1].lin_l.bias, model.lt1.weight, model.lt1.bias)]
    assert torch.equal(ops.gcn_graph_query_tail(G, pptr, *tail, pool="max", softmax=True), eng.predict(IDS))
    assert ops.sage_graph_query_hops(f.rowptr, f.col, f.val, T, seg[:0], prow[:0], pptr[:1], 0).shape == (0, 128)   # P == 0: no launch
    mt = lambda t: t.to("meta")   # noqa: E731
    m = torch.ops.fitgnn.sage_graph_query_hops(mt(f.rowptr), mt(f.col), mt(f.val), mt(T), mt(seg), mt(prow), mt(pptr), max_rows, None, None)
    assert m.shape == G.shape and m.dtype == G.dtype and m.device.type == "meta"


def _inference_pair(tmp_path, task_csv, train, infer, line):
    """Train a SAGEConv checkpoint with main.py, then inference.py without the flags and with --query_engine --query_sage, each a
    process of its own (as a user starts it; see tests/test_gpu_query.py for why).  Returns the two printed lines starting with `line`
    and the CSV's rows."""
    import subprocess
    import sys

    import main as cli
    cli.main(train)
    inf = [sys.executable, os.path.join(ROOT, "fit-gnn_amd", "inference.py")] + infer
    outs = []
    for extra in ([], ["--query_engine", "--query_sage"]):
        r = subprocess.run(inf + extra, cwd=tmp_path, check=True, timeout=300, stdout=subprocess.PIPE, text=True)
        outs.append(r.stdout)
    shown = [ln for o in outs for ln in o.splitlines() if ln.startswith(line)]
    rows = open(os.path.join("inference_results", task_csv)).read().strip().split("\n")
    return shown, rows


def test_inference_cli_graph_regression_with_and_without_the_sage_engine(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "synthetic-qm9", "--n_graphs", "200", "--hidden", "64", "--seed", "0", "--extra_node", "--layer_name", "SAGEConv"]
    shown, rows = _inference_pair(
        tmp_path, "graph_reg.csv",
        common + ["--train_fitgnn", "--batch_size", "64", "--lr", "0.002", "--property", "0", "--epochs1", "3", "--epochs2", "3", "--output_dir", "q",
                  "--exp_setup", "Gs_train_2_Gs_infer"],
        common + ["--num_test_samples", "12", "--property", "0", "--exp_setup", "Gs_train_2_Gs_infer", "--path_gs", "save/graph_reg/q/"],
        "L1 loss:")
    assert len(shown) == 2
    la, lb = (float(s.split(":")[1]) for s in shown)
    assert abs(la - lb) <= 1e-4 * abs(la), shown
    _same_csv_rows(rows)


def test_inference_cli_graph_classification_with_and_without_the_sage_engine(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "synthetic-proteins", "--n_graphs", "200", "--hidden", "64", "--seed", "0", "--layer_name", "SAGEConv"]
    shown, rows = _inference_pair(
        tmp_path, "graph_cls.csv",
        common + ["--train_fitgnn", "--batch_size", "50", "--lr", "0.005", "--epochs1", "3", "--epochs2", "3", "--output_dir", "p",
                  "--exp_setup", "Gc_train_2_Gc_infer"],
        common + ["--num_test_samples", "12", "--exp_setup", "Gc_train_2_Gc_infer", "--path_gc", "save/graph_cls/p/", "--model_name_gc", "model.pt"],
        "Accuracy:")
    assert len(shown) == 2 and shown[0] == shown[1], shown
    _same_csv_rows(rows)
