"""GPU tier: fitgnn_amd.serve.QueryEngine(model, batch, sage_kernels=True) for a model of two SAGEConv layers -- node ids in,
predictions out through fitgnn_sage_query_gather_f32 and the GCN tail with K = 2H -- against the float64 forward composed from
oracle.gnn_oracle.sage_conv and against the model's own whole-union forward, on the unions of tests/test_gpu_query.py (N = 60, four
clusters, seven classes); a queried row without entries; the prepared state's refresh on in-place weight updates; the default and the
fallbacks, which stay the per-subgraph forward; the torch.ops binding; inference.py --query_engine --query_sage."""
import os

import numpy as np
import pytest
import torch

import sage_query_reference as sq
from test_gpu_gat_query import _per_subgraph
from test_gpu_query import N, N_CLUSTERS, ROOT, SHAPES, _model, _union, mods, rel  # noqa: F401  (mods: the module-scoped fixture)

pytestmark = pytest.mark.gpu


def _sage_model(network, F, hidden, cls="Classify_node", layers=2, seed=0):
    return _model(network, F, hidden, cls=cls, layer="SAGEConv", layers=layers, seed=seed)   # random non-zero biases


def _oracle(gorc, model, batch, rows, classify=True):
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    return sq.oracle_forward(gorc, sd, batch.x.cpu(), batch.edge_index.cpu(), log_softmax=classify)[rows.cpu()]


@pytest.mark.parametrize("dedup", [True, False], ids=["table", "rows"])
@pytest.mark.parametrize("F,hidden", SHAPES, ids=str)
@pytest.mark.parametrize("layout", ["extra", "cluster"])
def test_predict_every_core_node(mods, layout, F, hidden, dedup):
    fdata, network, ops, serve, gorc = mods
    batch = _union(fdata, layout, F, dedup=dedup)
    model = _sage_model(network, F, hidden)
    eng = serve.QueryEngine(model, batch, sage_kernels=True)
    assert eng.fused is True and eng._kind() == "sage" and ops.sage_query_supported(model) and not ops.query_supported(model)
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
    print(f"sage query {layout} {(F, hidden)} dedup={dedup}: rel to the oracle {r_oracle:.3g}, to the model's forward {r_model:.3g}")
    assert r_oracle <= 1e-4
    assert r_model <= 1e-4
    assert torch.equal(eng.predict_rows(rows), out) and torch.equal(eng.predict(ids.cpu().tolist()), out)
    n_table = batch.x_table.shape[0] if dedup else batch.n_rows
    assert eng.table_bytes == n_table * 2 * hidden * 4


def test_a_queried_row_without_entries(mods):
    """A core node all of whose edges are dropped before assembly: its row of the mean CSR is empty, g = 0, and the answer is
    Wl ELU(W_r1 h_q + b_l1) + bl with h_q = ELU(W_r0 x_q + b_l0)."""
    fdata, network, ops, serve, gorc = mods
    from fitgnn_amd.csr import csr_for
    rng = np.random.default_rng(5)
    ei = fdata.synthetic_graph(N, 150, seed=2)
    lone = 17
    ei = ei[:, (ei[0] != lone) & (ei[1] != lone)]
    assign = rng.integers(0, N_CLUSTERS, size=N)
    assign[:N_CLUSTERS] = np.arange(N_CLUSTERS)
    X = rng.normal(size=(N, 12)).astype(np.float32)
    sub = fdata.assemble_subgraphs(ei, N, assign, N_CLUSTERS, extra_node=True)
    batch = fdata.SubgraphBatch(sub, X, rng.integers(0, 7, size=N), np.zeros(N, dtype=bool), device="cuda")
    model = _sage_model(network, 12, 64)
    eng = serve.QueryEngine(model, batch, sage_kernels=True)
    rows = torch.nonzero(batch.core).flatten()
    ids = batch.node_id[rows]
    row = int(rows[ids == lone][0])
    f = csr_for(batch.edge_index, batch.n_rows, "mean").f
    assert int(f.rowptr[row + 1] - f.rowptr[row]) == 0 and eng.fused
    out = eng.predict(ids)
    assert rel(out.cpu().double(), _oracle(gorc, model, batch, rows)) <= 1e-4
    one = eng.predict([lone])
    assert torch.equal(one[0], out[ids == lone][0])
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    elu = torch.nn.functional.elu
    h = elu(torch.from_numpy(X[lone]).double() @ sd["conv.0.lin_r.weight"].t() + sd["conv.0.lin_l.bias"])
    y = elu(h @ sd["conv.1.lin_r.weight"].t() + sd["conv.1.lin_l.bias"]) @ sd["lt1.weight"].t() + sd["lt1.bias"]
    assert rel(one[0].cpu().double(), torch.log_softmax(y, 0)) <= 1e-4


def test_regress_node_values(mods):
    fdata, network, ops, serve, gorc = mods
    batch = _union(fdata, "extra", 12)
    model = _sage_model(network, 12, 64, cls="Regress_node")
    eng = serve.QueryEngine(model, batch, sage_kernels=True)
    rows = torch.nonzero(batch.core).flatten()
    out = eng.predict(batch.node_id[rows])
    assert out.shape == (len(rows), 1) and eng.fused
    assert rel(out.cpu().double(), _oracle(gorc, model, batch, rows, classify=False)) <= 1e-4


@pytest.mark.parametrize("which", ["conv0.lin_l.weight", "conv0.lin_r.weight", "conv1.lin_l.weight", "conv1.lin_r.weight", "lt1.bias"])
def test_weight_update_is_picked_up(mods, which):
    fdata, network, ops, serve, gorc = mods
    batch = _union(fdata, "extra", 12)
    model = _sage_model(network, 12, 64)
    eng = serve.QueryEngine(model, batch, sage_kernels=True)
    rows = torch.nonzero(batch.core).flatten()
    ids = batch.node_id[rows]
    before = eng.predict(ids).clone()
    c0, c1 = model.conv
    p = {"conv0.lin_l.weight": c0.lin_l.weight, "conv0.lin_r.weight": c0.lin_r.weight, "conv1.lin_l.weight": c1.lin_l.weight,
         "conv1.lin_r.weight": c1.lin_r.weight, "lt1.bias": model.lt1.bias}[which]
    with torch.no_grad():
        p.mul_(-1.5).add_(0.3)     # in place: same storage, new version
    after = eng.predict(ids)
    assert rel(after.cpu().double(), _oracle(gorc, model, batch, rows)) <= 1e-4
    assert not torch.allclose(after, before, atol=1e-3)
    assert torch.equal(eng.refresh().predict(ids), after)


def test_default_is_unchanged(mods):
    fdata, network, ops, serve, gorc = mods
    batch = _union(fdata, "extra", 12)
    model = _sage_model(network, 12, 64)
    eng = serve.QueryEngine(model, batch)
    assert eng.sage_kernels is False and eng.fused is False and eng.table_bytes == 0
    rows = torch.nonzero(batch.core).flatten()
    assert torch.equal(eng.predict_rows(rows), _per_subgraph(model, batch, rows).float())
    gat = serve.QueryEngine(model, batch, gat_kernels=True)     # the other flag changes nothing for a SAGE model
    assert gat.fused is False and gat.table_bytes == 0


@pytest.mark.parametrize("kind", ["hidden 40", "three layers"])
def test_unsupported_models_fall_back(mods, kind):
    fdata, network, ops, serve, gorc = mods
    batch = _union(fdata, "extra", 12)
    model = _sage_model(network, 12, 40) if kind == "hidden 40" else _sage_model(network, 12, 64, layers=3)
    assert not ops.sage_query_supported(model)
    eng = serve.QueryEngine(model, batch, sage_kernels=True)
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
    b = serve.QueryEngine(model, batch, sage_kernels=True)
    assert a.fused is True and b.fused is True and b._kind() == "gcn" and a.table_bytes == b.table_bytes
    assert torch.equal(a.predict_rows(rows), b.predict_rows(rows))


def test_torch_op_holds_the_launcher(mods):
    fdata, network, ops, serve, gorc = mods
    from fitgnn_amd import torch_ops  # noqa: F401  (registers torch.ops.fitgnn)
    batch = _union(fdata, "extra", 12)
    model = _sage_model(network, 12, 64)
    eng = serve.QueryEngine(model, batch, sage_kernels=True)
    f = eng.csr().f
    T, W1cat = eng.state()
    assert T.shape == (batch.x_table.shape[0], 128) and W1cat.shape == (64, 128) and W1cat.is_contiguous()
    rows = torch.nonzero(batch.core).flatten()
    xrow, b0 = batch.row_index.index, model.conv[0].lin_l.bias
    G = torch.ops.fitgnn.sage_query_gather(f.rowptr, f.col, f.val, T, rows, xrow, b0)
    assert G.shape == (len(rows), 128) and torch.equal(G, ops.sage_query_gather(f.rowptr, f.col, f.val, T, rows, xrow=xrow, b0=b0))
    y = torch.ops.fitgnn.gcn_query_tail(G, W1cat, model.conv[1].lin_l.bias, model.lt1.weight, model.lt1.bias, True)
    assert torch.equal(y, eng.predict_rows(rows))
    G0 = torch.ops.fitgnn.sage_query_gather(f.rowptr, f.col, f.val, T, rows, xrow, None)
    assert torch.equal(G0, ops.sage_query_gather(f.rowptr, f.col, f.val, T, rows, xrow=xrow)) and not torch.equal(G0, G)
    mt = lambda t: t.to("meta")   # noqa: E731
    m = torch.ops.fitgnn.sage_query_gather(mt(f.rowptr), mt(f.col), mt(f.val), mt(T), mt(rows), None, None)
    assert m.shape == G.shape and m.dtype == G.dtype and m.device.type == "meta"


def test_inference_cli_with_and_without_the_sage_engine(tmp_path, monkeypatch):
    """inference.py --layer_name SAGEConv on synthetic-cora with a checkpoint trained for 5 epochs here: --query_engine --query_sage
    gives the same hit count, the mean loss within 1e-4 relative, and the same CSV header and column count as the run without the
    two flags.  Each inference run is a process of its own (tests/test_gpu_query.py says why)."""
    import subprocess
    import sys

    monkeypatch.chdir(tmp_path)
    import main as cli

    common = ["--dataset", "synthetic-cora", "--hidden", "64", "--seed", "0", "--normalize_features", "--extra_node", "--layer_name", "SAGEConv"]
    cli.main(common + ["--runs", "1", "--output_dir", "f", "--train_fitgnn", "--exp_setup", "Gs_train_2_Gs_infer", "--coarsening_ratio", "0.5",
                       "--epochs1", "5", "--epochs2", "5"])
    inf = [sys.executable, os.path.join(ROOT, "fit-gnn_amd", "inference.py")] + common + ["--num_test_samples", "30", "--path_gs", "save/node_cls/f/"]
    outs = []
    for extra in ([], ["--query_engine", "--query_sage"]):
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
