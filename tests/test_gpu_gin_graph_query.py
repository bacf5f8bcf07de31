"""GPU tier: fitgnn_amd.serve.GraphQueryEngine(model, gset, gin_kernels=True) for a model of two GINConv layers (nn = Linear, ReLU,
Linear, ReLU; both eps non-zero, random non-zero biases) -- graph ids in, predictions out through fitgnn_gin_graph_query_hops_f32 and
fitgnn_gin_graph_query_tail_f32 -- against the float64 forward of tests/gin_graph_query_reference.model_forward (the oracle's GIN stack
on the whole view, the per-graph pool, the head, the softmax) and against the model's own forward on GraphSet.batch_ids, on the
dozen-graph sets and the ids of tests/test_gpu_graph_query.py; the split of one call between the window and the per-row kernel; the
table's refresh and the per-call reads on in-place weight updates; the default and the fallbacks, which stay the model's own forward;
the torch.ops bindings; inference.py --query_engine --query_gin on the graph-level tasks."""
import os

import numpy as np
import pytest
import torch

import gin_graph_query_reference as ggq
from test_gpu_graph_query import IDS, N_GRAPHS, ROOT, _forward, _gset, _model, _view, mods  # noqa: F401  (mods: the module-scoped fixture)
from test_gpu_query import rel

pytestmark = pytest.mark.gpu
EPS = (0.375, -0.625)   # the default 0 would hide a dropped eps


def _gin_model(network, cls, F, hidden, layers=2, seed=0):
    m = _model(network, cls, F, hidden, layer="GINConv", layers=layers, seed=seed)   # random non-zero biases
    with torch.no_grad():
        for c, e in zip(m.conv, EPS + (0.25,)):
            c.eps.fill_(e)
    return m


def _oracle(gorc, model, gset, view, ids):
    """float64: the GIN stack on the whole (block-diagonal) view, per graph the pool over its pooled rows, the head, the softmax."""
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
    out = ggq.model_forward(gorc, sd, x.cpu(), ei.cpu(), seg, np.array(prow), pptr, "max" if classify else "mean", classify)
    return torch.from_numpy(out)


def _check(mods, model, gset, view, ids=IDS, **kw):
    graph_data, network, ops, serve, gorc = mods
    eng = serve.GraphQueryEngine(model, gset, view=view, gin_kernels=True, **kw)
    assert eng.fused is True and eng._kind() == "gin" and ops.gin_graph_query_supported(model) and not ops.graph_query_supported(model)
    assert float(model.conv[0].eps.detach()) == EPS[0] and float(model.conv[1].eps.detach()) == EPS[1]
    out = eng.predict(ids)
    C = model.lt1.weight.shape[0]
    assert out.shape == (len(ids), C) and out.dtype == torch.float32
    v = eng.view
    r_oracle = rel(out.cpu().double(), _oracle(gorc, model, gset, v, ids))
    r_model = rel(out.cpu().double(), _forward(model, gset, v, ids).cpu().double())
    print(f"gin graph query {type(model).__name__} {v}: rel to the oracle {r_oracle:.3g}, to the model's forward {r_model:.3g}")
    assert r_oracle <= 1e-4
    assert r_model <= 1e-4
    assert torch.equal(out[1], out[3]) and torch.equal(out[0], out[6])      # the repeated graphs
    assert torch.equal(eng.predict(torch.tensor(ids, device="cuda")), out)  # host and device ids: equal bits
    assert torch.equal(eng.predict(np.asarray(ids)), out)
    n_rows = int(_view(gset, v)[1][-1])
    assert eng.table_bytes == n_rows * model.conv[0].nn[0].weight.shape[0] * 4
    return eng, out


@pytest.mark.parametrize("hidden", [64, 512])
@pytest.mark.parametrize("cls,kind,view", [("Classify_graph_gs", "cls", "gs"), ("Classify_graph_gc", "cls", "gc"),
                                           ("Regress_graph_gs", "mol", "gs"), ("Regress_graph_gc", "mol", "gc")], ids=str)
def test_every_model_class_on_its_default_view(mods, cls, kind, view, hidden):
    graph_data, network = mods[:2]
    gset = _gset(graph_data, kind)
    model = _gin_model(network, cls, gset.x.shape[1], hidden)
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
    _check(mods, _gin_model(network, "Classify_graph_gc", gset.x.shape[1], hidden), gset, "orig")
    gm = _gset(graph_data, "mol")
    _check(mods, _gin_model(network, "Regress_graph_gc", gm.x.shape[1], hidden), gm, "orig")


@pytest.mark.parametrize("extra_node,cluster_node", [(False, False), (True, False), (False, True)], ids=["plain", "extra", "cluster"])
def test_the_subgraph_view_in_every_layout(mods, extra_node, cluster_node):
    graph_data, network = mods[:2]
    gset = _gset(graph_data, "mol", extra_node=extra_node, cluster_node=cluster_node)
    if extra_node or cluster_node:
        assert not bool(gset.gs_mask.all()), "every row pooled: the layout adds no rows"
    _check(mods, _gin_model(network, "Regress_graph_gs", gset.x.shape[1], 64), gset, "gs")
    _check(mods, _gin_model(network, "Classify_graph_gs", gset.x.shape[1], 64), gset, "gs")


def test_max_window_rows_4_splits_a_call_between_the_window_and_the_per_row_kernel(mods):
    """Uncoarsened graphs of 4 to 18 nodes: max_window_rows=4 sends the graphs of four rows through the window and the others through
    ops.gin_query_hops on their pooled rows, in one call, into one G in front of one tail."""
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "small")
    n_rows = np.diff(np.asarray(gset.node_ptr))
    ids = list(range(N_GRAPHS))[::-1] + [3, 0]
    fits = torch.from_numpy(n_rows[ids] <= 4)
    assert bool(fits.any()) and not bool(fits.all()), n_rows
    for cls in ("Classify_graph_gc", "Regress_graph_gc"):
        model = _gin_model(network, cls, gset.x.shape[1], 64)
        eng = serve.GraphQueryEngine(model, gset, view="orig", max_window_rows=4, gin_kernels=True)
        out = eng.predict(ids)
        assert eng.fused and eng._kind() == "gin"
        assert rel(out.cpu().double(), _oracle(gorc, model, gset, "orig", ids)) <= 1e-4
        assert rel(out.cpu().double(), _forward(model, gset, "orig", ids).cpu().double()) <= 1e-4
        whole = serve.GraphQueryEngine(model, gset, view="orig", gin_kernels=True).predict(ids)     # every graph in the window
        assert torch.equal(out[fits], whole[fits])                                # the window's graphs: the same arithmetic, the same bits
        assert rel(out.cpu().double(), whole.cpu().double()) <= 1e-4
    # the subgraph view of the same set under max_window_rows=3: every graph has more rows, all of them take the per-row kernel
    model = _gin_model(network, "Classify_graph_gs", gset.x.shape[1], 64)
    assert int(np.diff(np.asarray(gset.gs_ptr)).min()) > 3
    out = serve.GraphQueryEngine(model, gset, max_window_rows=3, gin_kernels=True).predict(ids)
    assert rel(out.cpu().double(), _oracle(gorc, model, gset, "gs", ids)) <= 1e-4


@pytest.mark.parametrize("which", ["conv0.nn.0.weight", "conv1.nn.2.weight", "conv0.eps", "lt1.bias"])
def test_weight_update_is_picked_up(mods, which):
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "mol")
    model = _gin_model(network, "Regress_graph_gs", gset.x.shape[1], 64)
    eng = serve.GraphQueryEngine(model, gset, gin_kernels=True)
    before = eng.predict(IDS).clone()
    c0, c1 = model.conv
    p = {"conv0.nn.0.weight": c0.nn[0].weight, "conv1.nn.2.weight": c1.nn[2].weight, "conv0.eps": c0.eps, "lt1.bias": model.lt1.bias}[which]
    with torch.no_grad():
        p.mul_(-1.5).add_(0.3)     # in place: same storage, new version
    after = eng.predict(IDS)
    assert eng.fused and rel(after.cpu().double(), _oracle(gorc, model, gset, "gs", IDS)) <= 1e-4
    assert not torch.allclose(after, before, atol=1e-3)
    assert torch.equal(eng.refresh().predict(IDS), after)


def test_an_activation_swapped_later_is_noticed(mods):
    """The engine answered with the kernels; then the last ReLU of conv0's MLP is replaced: no parameter changes, the path must."""
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "mol")
    model = _gin_model(network, "Regress_graph_gs", gset.x.shape[1], 64)
    eng = serve.GraphQueryEngine(model, gset, gin_kernels=True)
    eng.predict(IDS)
    assert eng.fused is True
    model.conv[0].nn[3] = torch.nn.Tanh()
    assert eng.fused is False and eng.table_bytes == 0
    assert rel(eng.predict(IDS).cpu().double(), _forward(model, gset, "gs", IDS).cpu().double()) <= 1e-4


def test_default_is_unchanged(mods):
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "mol")
    model = _gin_model(network, "Regress_graph_gs", gset.x.shape[1], 64)
    eng = serve.GraphQueryEngine(model, gset)
    assert eng.gin_kernels is False and eng.fused is False and eng.table_bytes == 0
    assert rel(eng.predict(IDS).cpu().double(), _forward(model, gset, "gs", IDS).cpu().double()) <= 1e-4


def test_a_gcn_model_ignores_the_flag(mods):
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "cls")
    model = _model(network, "Classify_graph_gs", gset.x.shape[1], 64)
    a = serve.GraphQueryEngine(model, gset)
    b = serve.GraphQueryEngine(model, gset, gin_kernels=True)
    assert a.fused is True and b.fused is True and b._kind() == "gcn" and a.table_bytes == b.table_bytes
    assert torch.equal(a.predict(IDS), b.predict(IDS))


@pytest.mark.parametrize("kind", ["one layer", "hidden 40"])
def test_unsupported_models_fall_back(mods, kind):
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "mol")
    model = _gin_model(network, "Regress_graph_gs", gset.x.shape[1], 40 if kind == "hidden 40" else 64, layers=1 if kind == "one layer" else 2)
    assert not ops.gin_graph_query_supported(model)
    eng = serve.GraphQueryEngine(model, gset, gin_kernels=True)
    assert eng.fused is False and eng.table_bytes == 0
    out = eng.predict(IDS)
    assert rel(out.cpu().double(), _forward(model, gset, "gs", IDS).cpu().double()) <= 1e-4
    if kind == "hidden 40":
        assert rel(out.cpu().double(), _oracle(gorc, model, gset, "gs", IDS)) <= 1e-4


def test_refusals_are_unchanged(mods):
    graph_data, network, ops, serve, gorc = mods
    gset = _gset(graph_data, "mol")
    model = _gin_model(network, "Regress_graph_gs", gset.x.shape[1], 64)
    eng = serve.GraphQueryEngine(model, gset, gin_kernels=True)
    with pytest.raises(ValueError, match=r"graph 12\b"):
        eng.predict([3, 12, 13])
    with pytest.raises(ValueError, match=r"graph -1\b"):
        eng.predict(torch.tensor([3, -1], device="cuda"))
    assert eng.predict([]).shape == (0, 1)
    import copy
    bare = copy.copy(gset)          # a graph without pooled rows: its mask cleared on a copy of the set's attributes
    bare.gs_mask = gset.gs_mask.clone()
    bare.gs_mask[int(gset.gs_ptr[4]):int(gset.gs_ptr[5])] = False
    be = serve.GraphQueryEngine(model, bare, gin_kernels=True)
    assert be.fused and be.predict([3, 5]).shape == (2, 1)
    with pytest.raises(ValueError, match=r"graph 4\b.*no pooled rows"):
        be.predict([3, 4, 5])
    model.train()
    with pytest.raises(RuntimeError):
        eng.predict([3])
    model.eval()


def test_torch_ops_hold_the_two_launchers(mods):
    graph_data, network, ops, serve, gorc = mods
    from fitgnn_amd import torch_ops  # noqa: F401  (registers torch.ops.fitgnn)
    gset = _gset(graph_data, "cls", extra_node=True)
    model = _gin_model(network, "Classify_graph_gs", gset.x.shape[1], 64)
    eng = serve.GraphQueryEngine(model, gset, gin_kernels=True)
    f, T = eng.csr().f, eng.state()[0]
    assert T.shape == (eng.n_rows, 64) and T.is_contiguous() and bool((f.val == 1).all())
    ids = np.asarray(IDS)
    seg = torch.from_numpy(np.stack([eng._ptr[ids], eng._ptr[ids + 1]], 1)).cuda()
    cnt = torch.from_numpy(eng._pp[ids + 1] - eng._pp[ids]).cuda()
    pptr = torch.cat([cnt.new_zeros(1), torch.cumsum(cnt, 0)])
    prow = torch.cat([eng._prow[int(eng._pp[g]):int(eng._pp[g + 1])] for g in IDS])
    max_rows = int((seg[:, 1] - seg[:, 0]).max())
    c0, c1 = model.conv
    e0, e1 = c0.eps.detach(), c1.eps.detach()
    W0b, b0b, b0a = c0.nn[2].weight.detach(), c0.nn[2].bias.detach(), c0.nn[0].bias.detach()
    G = torch.ops.fitgnn.gin_graph_query_hops(f.rowptr, f.col, f.val, T, e0, W0b, b0b, e1, seg, prow, pptr, max_rows, None, b0a)
    assert G.shape == (prow.numel(), 64)
    assert torch.equal(G, ops.gin_graph_query_hops(f.rowptr, f.col, f.val, T, e0, W0b, b0b, e1, seg, prow, pptr, max_rows, b0a=b0a))
    tail = [p.detach() for p in (c1.nn[0].weight, c1.nn[0].bias, c1.nn[2].weight, c1.nn[2].bias, model.lt1.weight, model.lt1.bias)]
    y = torch.ops.fitgnn.gin_graph_query_tail(G, pptr, *tail, 0, True)
    assert torch.equal(y, ops.gin_graph_query_tail(G, pptr, *tail, pool="max", softmax=True)) and torch.equal(y, eng.predict(IDS))
    W1a, _, W1b, _, Wl, _ = tail
    assert torch.equal(torch.ops.fitgnn.gin_graph_query_tail(G, pptr, W1a, None, W1b, None, Wl, None, 1, False),
                       ops.gin_graph_query_tail(G, pptr, W1a, None, W1b, None, Wl, None, pool="mean"))
    mt = lambda t: t.to("meta")   # noqa: E731
    m = torch.ops.fitgnn.gin_graph_query_hops(mt(f.rowptr), mt(f.col), mt(f.val), mt(T), mt(e0), mt(W0b), None, mt(e1), mt(seg), mt(prow),
                                              mt(pptr), max_rows, None, None)
    assert m.shape == G.shape and m.dtype == G.dtype and m.device.type == "meta"
    my = torch.ops.fitgnn.gin_graph_query_tail(m, mt(pptr), mt(W1a), None, mt(W1b), None, mt(Wl), None, 0, True)
    assert my.shape == y.shape and my.dtype == y.dtype and my.device.type == "meta"


def _inference_pair(tmp_path, task_csv, train, infer, line):
    """Train a GINConv checkpoint with main.py, then inference.py without the flags and with --query_engine --query_gin, each a process
    of its own (as a user starts it; see tests/test_gpu_query.py for why).  Returns the two printed lines starting with `line` and
    the CSV's rows."""
    import subprocess
    import sys

    import main as cli
    cli.main(train)
    inf = [sys.executable, os.path.join(ROOT, "fit-gnn_amd", "inference.py")] + infer
    outs = []
    for extra in ([], ["--query_engine", "--query_gin"]):
        r = subprocess.run(inf + extra, cwd=tmp_path, check=True, timeout=300, stdout=subprocess.PIPE, text=True)
        outs.append(r.stdout)
    shown = [ln for o in outs for ln in o.splitlines() if ln.startswith(line)]
    rows = open(os.path.join("inference_results", task_csv)).read().strip().split("\n")
    return shown, rows


def _same_csv_rows(rows):
    assert len(rows) == 3 and rows[0].startswith("dataset,baseline,experiment,exp_setup")
    head, a, b = (r.split(",") for r in rows)
    assert len(a) == len(b) == len(head)
    la, lb = float(a[head.index("avg_loss")]), float(b[head.index("avg_loss")])
    assert abs(la - lb) <= 1e-4 * abs(la), (la, lb)
    assert a[:head.index("avg_inf_time")] == b[:head.index("avg_inf_time")] and a[-1] == b[-1]    # the accuracy column too


def test_inference_cli_graph_regression_with_and_without_the_gin_engine(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "synthetic-qm9", "--n_graphs", "200", "--hidden", "64", "--seed", "0", "--extra_node", "--layer_name", "GINConv"]
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


def test_inference_cli_graph_classification_with_and_without_the_gin_engine(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "synthetic-proteins", "--n_graphs", "200", "--hidden", "64", "--seed", "0", "--layer_name", "GINConv"]
    shown, rows = _inference_pair(
        tmp_path, "graph_cls.csv",
        common + ["--train_fitgnn", "--batch_size", "50", "--lr", "0.005", "--epochs1", "3", "--epochs2", "3", "--output_dir", "p",
                  "--exp_setup", "Gc_train_2_Gc_infer"],
        common + ["--num_test_samples", "12", "--exp_setup", "Gc_train_2_Gc_infer", "--path_gc", "save/graph_cls/p/", "--model_name_gc", "model.pt"],
        "Accuracy:")
    assert len(shown) == 2 and shown[0] == shown[1], shown
    _same_csv_rows(rows)
