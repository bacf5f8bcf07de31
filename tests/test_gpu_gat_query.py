"""GPU tier: fitgnn_amd.serve.QueryEngine(model, batch, gat_kernels=True) for a model of two GATConv layers -- node ids in,
predictions out through fitgnn_gat_query_gather_f32 and the GCN tail -- against the float64 oracle forward composed from
oracle.gnn_oracle.gat_conv and against the model's own whole-union forward, on the unions of tests/test_gpu_query.py (N = 60, four
clusters, seven classes); the prepared state's refresh on in-place weight updates; the default and the fallbacks, which stay the
per-subgraph forward; the torch.ops binding; inference.py --query_engine --query_attention."""
import os

import numpy as np
import pytest
import torch

import gat_query_reference as gq
from test_gpu_query import ROOT, SHAPES, _model, _union, mods, rel  # noqa: F401  (mods: the module-scoped fixture)

pytestmark = pytest.mark.gpu
SLOPE1 = 0.35   # a non-default negative_slope on the second layer


def _gat_model(network, F, hidden, cls="Classify_node", seed=0):
    m = _model(network, F, hidden, cls=cls, layer="GATConv", seed=seed)   # random non-zero biases
    m.conv[1].negative_slope = SLOPE1
    return m


def _oracle(gorc, model, batch, rows, classify=True):
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    slopes = (model.conv[0].negative_slope, model.conv[1].negative_slope)
    return gq.oracle_forward(gorc, sd, batch.x.cpu(), batch.edge_index.cpu(), slopes, log_softmax=classify)[rows.cpu()]


def _per_subgraph(model, batch, rows):
    """The per-subgraph forward of inference.py on `rows`."""
    ptr = batch.ptr
    ref = None
    with torch.no_grad():
        for s in range(len(ptr) - 1):
            r0, r1 = int(ptr[s]), int(ptr[s + 1])
            ei = batch.edge_index
            m = (ei[0] >= r0) & (ei[0] < r1)
            y = model(batch.x[r0:r1].contiguous(), (ei[:, m] - r0).contiguous())
            if ref is None:
                ref = torch.empty((len(rows), y.shape[1]), dtype=y.dtype, device=y.device)
            pick = (rows >= r0) & (rows < r1)
            ref[pick] = y[rows[pick] - r0]
    return ref


@pytest.mark.parametrize("dedup", [True, False], ids=["table", "rows"])
@pytest.mark.parametrize("F,hidden", SHAPES, ids=str)
@pytest.mark.parametrize("layout", ["extra", "cluster"])
def test_predict_every_core_node(mods, layout, F, hidden, dedup):
    fdata, network, ops, serve, gorc = mods
    batch = _union(fdata, layout, F, dedup=dedup)
    model = _gat_model(network, F, hidden)
    eng = serve.QueryEngine(model, batch, gat_kernels=True)
    assert eng.fused is True and ops.gat_query_supported(model) and not ops.query_supported(model)
    rows = torch.nonzero(batch.core).flatten()
    ids = batch.node_id[rows]
    perm = torch.randperm(len(ids), generator=torch.Generator().manual_seed(1)).cuda()
    ids, rows = ids[perm], rows[perm]     # unsorted
    out = eng.predict(ids)
    assert out.shape == (len(ids), 7) and out.dtype == torch.float32
    r_oracle = rel(out.cpu().double(), _oracle(gorc, model, batch, rows))
    with torch.no_grad():
        full = model(batch.x, batch.edge_index)[rows]
    r_model = rel(out.cpu().double(), full.cpu().double())
    print(f"gat query {layout} {(F, hidden)} dedup={dedup}: rel to the oracle {r_oracle:.3g}, to the model's forward {r_model:.3g}")
    assert r_oracle <= 1e-4
    assert r_model <= 1e-4
    assert torch.equal(eng.predict_rows(rows), out) and torch.equal(eng.predict(ids.cpu().tolist()), out)
    n_table = batch.x_table.shape[0] if dedup else batch.n_rows
    assert eng.table_bytes == n_table * (4 * hidden + 8)


def test_regress_node_values(mods):
    fdata, network, ops, serve, gorc = mods
    batch = _union(fdata, "extra", 12)
    model = _gat_model(network, 12, 64, cls="Regress_node")
    eng = serve.QueryEngine(model, batch, gat_kernels=True)
    rows = torch.nonzero(batch.core).flatten()
    out = eng.predict(batch.node_id[rows])
    assert out.shape == (len(rows), 1) and eng.fused
    assert rel(out.cpu().double(), _oracle(gorc, model, batch, rows, classify=False)) <= 1e-4


@pytest.mark.parametrize("which", ["conv0.att_dst", "conv1.att_src", "conv0.lin.weight"])
def test_weight_update_is_picked_up(mods, which):
    fdata, network, ops, serve, gorc = mods
    batch = _union(fdata, "extra", 12)
    model = _gat_model(network, 12, 64)
    eng = serve.QueryEngine(model, batch, gat_kernels=True)
    rows = torch.nonzero(batch.core).flatten()
    ids = batch.node_id[rows]
    before = eng.predict(ids).clone()
    p = {"conv0.att_dst": model.conv[0].att_dst, "conv1.att_src": model.conv[1].att_src, "conv0.lin.weight": model.conv[0].lin.weight}[which]
    with torch.no_grad():
        p.mul_(-1.5).add_(0.3)     # in place: same storage, new version
    after = eng.predict(ids)
    assert rel(after.cpu().double(), _oracle(gorc, model, batch, rows)) <= 1e-4
    assert not torch.allclose(after, before, atol=1e-3)
    assert torch.equal(eng.refresh().predict(ids), after)


def test_default_is_unchanged(mods):
    fdata, network, ops, serve, gorc = mods
    batch = _union(fdata, "extra", 12)
    model = _gat_model(network, 12, 64)
    eng = serve.QueryEngine(model, batch)
    assert eng.gat_kernels is False and eng.fused is False and eng.table_bytes == 0
    rows = torch.nonzero(batch.core).flatten()
    assert rel(eng.predict_rows(rows).cpu().double(), _per_subgraph(model, batch, rows).cpu().double()) <= 1e-4


def _unsupported(network, kind):
    from fitgnn_amd import nn as fnn
    if kind == "hidden 528":
        return _gat_model(network, 12, 528)
    if kind == "GAT + GCN":
        m = _gat_model(network, 12, 64)
        torch.manual_seed(3)
        m.conv[1] = fnn.GCNConv(64, 64).cuda()
        return m.eval()
    m = _model(network, 12, 64, layer="GATConv", layers=3)
    return m


@pytest.mark.parametrize("kind", ["hidden 528", "GAT + GCN", "three layers"])
def test_unsupported_models_fall_back(mods, kind):
    fdata, network, ops, serve, gorc = mods
    batch = _union(fdata, "extra", 12)
    model = _unsupported(network, kind)
    assert not ops.gat_query_supported(model)
    eng = serve.QueryEngine(model, batch, gat_kernels=True)
    assert eng.fused is False and eng.table_bytes == 0
    rows = torch.nonzero(batch.core).flatten().flip(0)
    out = eng.predict(batch.node_id[rows])
    assert rel(out.cpu().double(), _per_subgraph(model, batch, rows).cpu().double()) <= 1e-4


def test_a_gcn_model_ignores_the_flag(mods):
    fdata, network, ops, serve, gorc = mods
    batch = _union(fdata, "extra", 12)
    model = _model(network, 12, 64)
    rows = torch.nonzero(batch.core).flatten()
    a = serve.QueryEngine(model, batch)
    b = serve.QueryEngine(model, batch, gat_kernels=True)
    assert a.fused is True and b.fused is True and a.table_bytes == b.table_bytes
    assert torch.equal(a.predict_rows(rows), b.predict_rows(rows))


def test_torch_op_holds_the_launcher(mods):
    fdata, network, ops, serve, gorc = mods
    from fitgnn_amd import torch_ops  # noqa: F401  (registers torch.ops.fitgnn)
    batch = _union(fdata, "extra", 12)
    model = _gat_model(network, 12, 64)
    eng = serve.QueryEngine(model, batch, gat_kernels=True)
    f = batch.graph.f
    T, a0s, a0d, u_s, u_d = eng.state()
    rows = torch.nonzero(batch.core).flatten()
    xrow, b0 = batch.row_index.index, model.conv[0].bias
    G = torch.ops.fitgnn.gat_query_gather(f.rowptr, f.col, T, a0s, a0d, u_s, u_d, rows, xrow, b0, 0.2, SLOPE1)
    assert torch.equal(G, ops.gat_query_gather(f.rowptr, f.col, T, a0s, a0d, u_s, u_d, rows, xrow=xrow, b0=b0, slope0=0.2, slope1=SLOPE1))
    W1, b1, Wl, bl = model.conv[1].lin.weight, model.conv[1].bias, model.lt1.weight, model.lt1.bias
    assert torch.equal(torch.ops.fitgnn.gcn_query_tail(G, W1, b1, Wl, bl, True), eng.predict_rows(rows))
    G0 = torch.ops.fitgnn.gat_query_gather(f.rowptr, f.col, T, a0s, a0d, u_s, u_d, rows, xrow, None, 0.2, 0.2)
    assert torch.equal(G0, ops.gat_query_gather(f.rowptr, f.col, T, a0s, a0d, u_s, u_d, rows, xrow=xrow)) and not torch.equal(G0, G)
    mt = lambda t: t.to("meta")   # noqa: E731
    m = torch.ops.fitgnn.gat_query_gather(mt(f.rowptr), mt(f.col), mt(T), mt(a0s), mt(a0d), mt(u_s), mt(u_d), mt(rows), None, None, 0.2, 0.2)
    assert m.shape == G.shape and m.dtype == G.dtype and m.device.type == "meta"
    # u is W1^T att to half an ulp: float64 product, one rounding
    want = (model.conv[1].att_src.detach().double().reshape(1, -1) @ W1.detach().double()).reshape(-1)
    assert torch.equal(u_s, want.float())


def test_inference_cli_with_and_without_the_attention_engine(tmp_path, monkeypatch):
    """inference.py --layer_name GATConv on synthetic-cora with a checkpoint trained for 5 epochs here: --query_engine
    --query_attention gives the same hit count, the mean loss within 1e-4 relative, and the same CSV header and column count as the
    run without the two flags.  Each inference run is a process of its own (tests/test_gpu_query.py says why)."""
    import subprocess
    import sys

    monkeypatch.chdir(tmp_path)
    import main as cli

    common = ["--dataset", "synthetic-cora", "--hidden", "64", "--seed", "0", "--normalize_features", "--extra_node", "--layer_name", "GATConv"]
    cli.main(common + ["--runs", "1", "--output_dir", "f", "--train_fitgnn", "--exp_setup", "Gs_train_2_Gs_infer", "--coarsening_ratio", "0.5",
                       "--epochs1", "5", "--epochs2", "5"])
    inf = [sys.executable, os.path.join(ROOT, "fit-gnn_amd", "inference.py")] + common + ["--num_test_samples", "30", "--path_gs", "save/node_cls/f/"]
    outs = []
    for extra in ([], ["--query_engine", "--query_attention"]):
        r = subprocess.run(inf + extra, cwd=tmp_path, check=True, timeout=300, stdout=subprocess.PIPE, text=True)
        outs.append(r.stdout)
    hits = [ln for o in outs for ln in o.splitlines() if ln.startswith("Accuracy (FIT-GNN):")]
    assert len(hits) == 2 and hits[0] == hits[1], hits
    lines = open(os.path.join("inference_results", "node_cls.csv")).read().strip().split("\n")
    assert len(lines) == 3 and lines[0].startswith("dataset,baseline,experiment,exp_setup")
    head, a, b = (ln.split(",") for ln in lines)
    assert len(a) == len(b) == len(head)
    la, lb = float(a[head.index("avg_loss")]), float(b[head.index("avg_loss")])
    assert abs(la - lb) <= 1e-4 * abs(la), (la, lb)
