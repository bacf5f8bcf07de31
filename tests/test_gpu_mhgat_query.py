"""GPU tier: fitgnn_amd.serve.QueryEngine(model, batch, gat_heads_kernels=True) for a model of two GATConv(heads, concat) layers --
node ids in, predictions out through fitgnn_mhgat_query_gather_f32 and fitgnn_mhgat_query_tail_f32 -- against the float64 oracle
forward composed per head from oracle.gnn_oracle.gat_conv (tests/mhgat_query_reference.py) and against the per-subgraph forward, on
the union of tests/test_gpu_gat_heads.py (90 nodes, six subgraphs, its _args: 12 features, hidden 64, five classes) in the
extra-node layout and its cluster-node twin; the prepared state's refresh on in-place weight updates; the default and the
fallbacks, which stay the per-subgraph forward; inference.py --query_engine --query_attention_heads.

1e-4 of the largest value is the figure every engine test of tests/test_gpu_gat_query.py uses.

heads = 8 at hidden 64 has C1 = 8 output columns per head at layer 1; the tail's product runs in MFMA blocks of 16 columns
(fitgnn_mhgat_query_tail_f32 refuses C1 % 16 != 0, ops.mhgat_query_supported answers False), so that model is among the
fallbacks here and eight heads are answered by the kernels at hidden 128, the smallest hidden size at which they take eight."""
import os

import numpy as np
import pytest
import torch

import mhgat_query_reference as mq
from test_gpu_gat_heads import _args, _six_subgraph_batch
from test_gpu_gat_query import _per_subgraph
from test_gpu_query import ROOT, mods, rel  # noqa: F401  (mods: the module-scoped fixture)

pytestmark = pytest.mark.gpu
SLOPE1 = 0.35   # a non-default negative_slope on the second layer
FUSED = [(2, 64), (4, 64), (8, 128)]   # (heads, hidden)


def _batch(fdata, layout, dedup=True):
    """tests/test_gpu_gat_heads.py's union of six subgraphs (extra-node layout), or the same 90 nodes and clusters in the cluster-node
    layout (tests/test_gpu_query.py's construction)."""
    if layout == "extra":
        return _six_subgraph_batch(dedup=dedup)
    import scipy.sparse as sp

    N, K, F = 90, 6, 12
    rng = np.random.default_rng(5)
    ei = fdata.synthetic_graph(N, 220, seed=2)
    assign = rng.integers(0, K, size=N)
    assign[:K] = np.arange(K)
    X = rng.normal(size=(N, F)).astype(np.float32)
    y = rng.integers(0, 5, size=N)
    cu, cv = assign[ei[0]], assign[ei[1]]
    k = cu != cv
    adj = sp.csr_matrix((np.ones(int(k.sum())), (cu[k], cv[k])), shape=(K, K))
    sub = fdata.assemble_subgraphs_cluster(ei, N, assign, K, adj)
    X = np.concatenate([X, rng.normal(size=(K, F)).astype(np.float32)])   # stand-ins for the pooled rows C.X
    y = np.concatenate([y, np.zeros(K, dtype=y.dtype)])
    assert len(sub["ptr"]) - 1 == K
    return fdata.SubgraphBatch(sub, X, y, np.zeros(len(X), dtype=bool), device="cuda", dedup=dedup)


def _model(network, heads=4, hidden=64, cls="Classify_node", seed=0, **kw):
    torch.manual_seed(seed)
    m = getattr(network, cls)(_args(heads=heads, hidden=hidden, **kw)).cuda()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.normal_(0, 0.3)   # the default zero biases would hide a dropped bias
    m.conv[1].negative_slope = SLOPE1
    return m.eval()


def _oracle(gorc, model, batch, rows, classify=True):
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    slopes = (model.conv[0].negative_slope, model.conv[1].negative_slope)
    return mq.oracle_forward(gorc, sd, batch.x.cpu(), batch.edge_index.cpu(), model.conv[0].heads, slopes, log_softmax=classify)[rows.cpu()]


@pytest.mark.parametrize("dedup", [True, False], ids=["table", "rows"])
@pytest.mark.parametrize("heads,hidden", FUSED, ids=str)
@pytest.mark.parametrize("layout", ["extra", "cluster"])
def test_predict_every_core_node(mods, layout, heads, hidden, dedup):
    fdata, network, ops, serve, gorc = mods
    batch = _batch(fdata, layout, dedup=dedup)
    model = _model(network, heads, hidden)
    assert [c.heads for c in model.conv] == [heads, heads]
    eng = serve.QueryEngine(model, batch, gat_heads_kernels=True)
    assert eng.fused is True and eng.path().name == "gat_heads"
    assert ops.mhgat_query_supported(model) and not ops.gat_query_supported(model) and not ops.gat_graph_query_supported(model)
    rows = torch.nonzero(batch.core).flatten()
    ids = batch.node_id[rows]
    perm = torch.randperm(len(ids), generator=torch.Generator().manual_seed(1)).cuda()
    ids, rows = ids[perm], rows[perm]     # unsorted
    out = eng.predict(ids)
    assert out.shape == (len(ids), 5) and out.dtype == torch.float32
    r_oracle = rel(out.cpu().double(), _oracle(gorc, model, batch, rows))
    r_sub = rel(out.cpu().double(), _per_subgraph(model, batch, rows).cpu().double())
    print(f"mhgat query {layout} heads={heads} hidden={hidden} dedup={dedup}: rel to the oracle {r_oracle:.3g}, to the per-subgraph forward {r_sub:.3g}")
    assert r_oracle <= 1e-4
    assert r_sub <= 1e-4
    assert torch.equal(eng.predict_rows(rows), out) and torch.equal(eng.predict(ids.cpu().tolist()), out)
    n_table = batch.x_table.shape[0] if dedup else batch.n_rows
    assert eng.table_bytes == n_table * (4 * hidden + 8 * heads)
    # gat_kernels alone leaves the model to its forward
    assert serve.QueryEngine(model, batch, gat_kernels=True).fused is False


def test_regress_node_values(mods):
    fdata, network, ops, serve, gorc = mods
    batch = _batch(fdata, "extra")
    model = _model(network, 4, 64, cls="Regress_node")
    eng = serve.QueryEngine(model, batch, gat_heads_kernels=True)
    rows = torch.nonzero(batch.core).flatten()
    out = eng.predict(batch.node_id[rows])
    assert out.shape == (len(rows), 1) and eng.fused
    assert rel(out.cpu().double(), _oracle(gorc, model, batch, rows, classify=False)) <= 1e-4


@pytest.mark.parametrize("which", ["conv0.att_dst", "conv1.att_src", "conv0.lin.weight"])
def test_weight_update_is_picked_up(mods, which):
    fdata, network, ops, serve, gorc = mods
    batch = _batch(fdata, "extra")
    model = _model(network, 4, 64)
    eng = serve.QueryEngine(model, batch, gat_heads_kernels=True)
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


def test_prepared_state_is_the_per_head_products(mods):
    """U[hd] is W1[block hd]^T att1[hd] to half an ulp (float64 product, one rounding), a0s / a0d are [n_table, heads]."""
    fdata, network, ops, serve, gorc = mods
    batch = _batch(fdata, "extra")
    model = _model(network, 4, 64)
    T, a0s, a0d, U_s, U_d = serve.QueryEngine(model, batch, gat_heads_kernels=True).state()
    n = batch.x_table.shape[0]
    assert T.shape == (n, 64) and a0s.shape == a0d.shape == (n, 4) and U_s.shape == U_d.shape == (4, 64)
    W1 = model.conv[1].lin.weight.detach().cpu().numpy()
    assert np.array_equal(U_s.cpu().numpy(), mq.u_vectors(W1, model.conv[1].att_src.detach().cpu().numpy(), 4).astype(np.float32))
    assert np.array_equal(U_d.cpu().numpy(), mq.u_vectors(W1, model.conv[1].att_dst.detach().cpu().numpy(), 4).astype(np.float32))
    want = (T.double().view(n, 4, 16) * model.conv[0].att_src.detach().double().view(1, 4, 16)).sum(-1)
    assert rel(a0s.double(), want) <= 1e-5


def _fallback(network, kind):
    from fitgnn_amd import nn as fnn
    if kind == "flag off":
        return _model(network, 4, 64), {}
    flag = {"gat_heads_kernels": True}
    if kind == "heads = 1":
        return _model(network, 1, 64), flag
    if kind == "concat=False on layer 1":
        m = _model(network, 4, 64)
        torch.manual_seed(3)
        m.conv[1] = fnn.GATConv(64, 64, heads=4, concat=False).cuda()
        return m.eval(), flag
    if kind == "heads = 16":
        return _model(network, 16, 64), flag
    if kind == "heads = 8 at hidden 64":
        return _model(network, 8, 64), flag
    if kind == "hidden 528":
        return _model(network, 4, 528), flag
    return _model(network, 4, 64, num_layers1=3), flag


@pytest.mark.parametrize("kind", ["flag off", "heads = 1", "concat=False on layer 1", "heads = 16", "heads = 8 at hidden 64", "hidden 528",
                                  "three layers"])
def test_fallbacks_answer_with_the_per_subgraph_forward(mods, kind):
    fdata, network, ops, serve, gorc = mods
    batch = _batch(fdata, "extra")
    model, flags = _fallback(network, kind)
    assert ops.mhgat_query_supported(model) is (kind == "flag off")
    eng = serve.QueryEngine(model, batch, **flags)
    assert eng.fused is False and eng.table_bytes == 0
    rows = torch.nonzero(batch.core).flatten().flip(0)
    out = eng.predict(batch.node_id[rows])
    assert rel(out.cpu().double(), _per_subgraph(model, batch, rows).cpu().double()) <= 1e-4


def test_a_gcn_model_ignores_the_flag(mods):
    fdata, network, ops, serve, gorc = mods
    batch = _batch(fdata, "extra")
    torch.manual_seed(0)
    model = network.Classify_node(_args(layer_name="GCNConv")).cuda().eval()
    rows = torch.nonzero(batch.core).flatten()
    a = serve.QueryEngine(model, batch)
    b = serve.QueryEngine(model, batch, gat_heads_kernels=True)
    assert a.fused is True and b.fused is True and a.path().name == b.path().name == "gcn" and a.table_bytes == b.table_bytes
    assert torch.equal(a.predict_rows(rows), b.predict_rows(rows))


def test_the_graph_engine_keeps_its_fallback():
    from fitgnn_amd import network, serve
    torch.manual_seed(0)
    model = network.Classify_node(_args(heads=4)).cuda().eval()
    assert serve.GATHeadsPath().supported(model, graph=True) is False and serve.GATHeadsPath().supported(model, graph=False) is True
    assert [p.name for p in serve.PATHS] == ["gcn", "gat", "gat_heads", "sage", "gin"]


def test_inference_cli_with_and_without_the_heads_engine(tmp_path, monkeypatch):
    """inference.py --layer_name GATConv --heads 4 --hidden 64 on synthetic-cora with a checkpoint trained for 2 epochs here:
    --query_engine --query_attention_heads gives the same hit count, the mean loss within 1e-4 relative, and the same CSV header and
    column count as the run without the two flags.  Each inference run is a process of its own (tests/test_gpu_query.py says why)."""
    import subprocess
    import sys

    monkeypatch.chdir(tmp_path)
    import main as cli

    common = ["--dataset", "synthetic-cora", "--hidden", "64", "--heads", "4", "--seed", "0", "--normalize_features", "--extra_node",
              "--layer_name", "GATConv"]
    cli.main(common + ["--runs", "1", "--output_dir", "f", "--train_fitgnn", "--exp_setup", "Gs_train_2_Gs_infer", "--coarsening_ratio", "0.5",
                       "--epochs1", "2", "--epochs2", "2"])
    inf = [sys.executable, os.path.join(ROOT, "fit-gnn_amd", "inference.py")] + common + ["--num_test_samples", "30", "--path_gs", "save/node_cls/f/"]
    outs = []
    for extra in ([], ["--query_engine", "--query_attention_heads"]):
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
