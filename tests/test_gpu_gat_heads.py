"""GPU tier: multi-head GATConv (nn.GATConv(heads > 1), ops.GATHeadsAggregate) from the layer up to the command line.

The layer's tolerance is MEASURED, not fixed: on the same inputs the per-head composition of the single-head path -- `heads` calls of
ops.GATAggregate on column slices of h, the code this project already had -- is compared with the float64 reference
(tests/gat_heads_reference.py) first, and the multi-head path may be off by at most twice that plus 1e-6 of the largest reference
entry: both compute the same sums in another order, and a factor 2 covers reordering and nothing else.  The models are held to that
bound times their number of layers.  The figures are printed (pytest -s) and quoted in DESIGN.md section 4."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gat_heads_reference as ghr
import gat_reference as gr
from graph_fixtures import star_blocks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRADS = ("x", "lin.weight", "att_src", "att_dst", "bias")


# ---------------------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------------------
def _undirected(a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    k = a != b
    return torch.tensor(np.unique(np.concatenate([np.stack([a[k], b[k]]), np.stack([b[k], a[k]])], 1), axis=1), dtype=torch.long)


def _graph(kind):
    """(edge_index, n): a star of 300 leaves, a Barabasi-Albert (200, 3) graph, a union of stars of sizes [100, 7, 17, 3, 1, 64]."""
    if kind == "star":
        return _undirected(np.zeros(300), np.arange(1, 301)), 301
    if kind == "ba":
        rng = np.random.default_rng(7)
        n, m = 200, 3
        a, b, ends = [], [], list(range(m))
        for v in range(m, n):
            for t in set(rng.choice(ends, size=m).tolist()):
                a.append(v); b.append(t)
                ends += [v, t]
        return _undirected(a, b), n
    if kind == "stars":
        return star_blocks([100, 7, 17, 3, 1, 64], 1, seed=3)
    raise ValueError(kind)


GRAPHS = ["star", "ba", "stars"]
LAYERS = [(2, True), (8, True), (2, False), (8, False)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the layer three ways: multi-head kernels, per-head composition of the single-head path, float64
# ---------------------------------------------------------------------------------------------------------------------------------
def _per_head_composition(conv, x, ei):
    """The layer from `heads` calls of ops.GATAggregate on column slices of h (bias added outside): forward on leaf copies of the
    parameters, so that autograd gives the composition's own gradients."""
    from fitgnn_amd import ops
    from fitgnn_amd.csr import csr_for

    P = {k: v.detach().clone().requires_grad_(True) for k, v in conv.named_parameters()}
    Hd, C, cfg = conv.heads, conv.out_channels, conv.op_config
    g = csr_for(ei, x.shape[0], "gat")
    h = ops.Linear.apply(x, P["lin.weight"], cfg)
    a_s, a_d = P["att_src"].view(-1), P["att_dst"].view(-1)
    outs = []
    for k in range(Hd):
        sl = slice(k * C, (k + 1) * C)
        outs.append(ops.GATAggregate.apply(h[:, sl].contiguous(), a_s[sl], a_d[sl], None, g, conv.negative_slope, False, 0.0, False, 0,
                                           None, cfg))
    out = torch.cat(outs, dim=1) if conv.concat else torch.stack(outs, dim=0).mean(0)
    return out + P["bias"], P


def _measure(kind, heads, concat):
    """Errors (max |got - ref|) of both paths against float64 and the largest reference entry, per quantity."""
    from fitgnn_amd import nn as fnn

    ei, n = _graph(kind)
    torch.manual_seed(heads * 10 + concat)
    conv = fnn.GATConv(16, 8, heads=heads, concat=concat).cuda()
    with torch.no_grad():
        conv.bias.normal_()
    x = torch.randn(n, 16)
    gout = torch.randn(n, 8 * heads if concat else 8)
    eid = ei.cuda()

    xg = x.cuda().requires_grad_(True)
    out = conv(xg, eid)
    assert type(out.grad_fn).__name__ != "GATAggregateBackward"
    out.backward(gout.cuda())
    fused = dict(out=out.detach(), x=xg.grad, **{k: p.grad for k, p in conv.named_parameters()})

    xc = x.cuda().requires_grad_(True)
    out_c, Pc = _per_head_composition(conv, xc, eid)
    out_c.backward(gout.cuda())
    comp = dict(out=out_c.detach(), x=xc.grad, **{k: p.grad for k, p in Pc.items()})

    rowptr, col = gr.gat_csr(ei.numpy(), n)
    sd = {k: v.detach().cpu().double().numpy() for k, v in conv.state_dict().items()}
    a_s, a_d = sd["att_src"].reshape(-1), sd["att_dst"].reshape(-1)
    ref_out, mid = ghr.gat_heads_layer(x.double().numpy(), sd["lin.weight"], a_s, a_d, sd["bias"], rowptr, col, heads, concat=concat)
    g = ghr.gat_heads_layer_backward(x.double().numpy(), sd["lin.weight"], a_s, a_d, rowptr, col, mid, gout.double().numpy(), heads,
                                     concat=concat)
    ref = dict(out=ref_out, **dict(zip(GRADS, g)))
    rec = {}
    for q in ("out",) + GRADS:
        r = ref[q].reshape(-1)
        rec[q] = (float(np.abs(fused[q].cpu().double().numpy().reshape(-1) - r).max()),
                  float(np.abs(comp[q].cpu().double().numpy().reshape(-1) - r).max()), float(np.abs(r).max()))
    return rec


@pytest.fixture(scope="module")
def measured():
    """{(graph, heads, concat): {quantity: (error of the multi-head path, error of the per-head composition, max |ref|)}}: computed
    once for the layer tests and the bound of the model tests."""
    assert torch.cuda.is_available()
    return {(k, h, c): _measure(k, h, c) for k in GRAPHS for h, c in LAYERS}


@pytest.mark.parametrize("heads,concat", LAYERS, ids=[f"heads{h}-{'concat' if c else 'mean'}" for h, c in LAYERS])
@pytest.mark.parametrize("kind", GRAPHS)
def test_layer_against_float64_within_twice_the_per_head_compositions_error(measured, kind, heads, concat):
    rec = measured[(kind, heads, concat)]
    for q, (e_fused, e_comp, big) in rec.items():
        print(f"gat heads layer {kind} heads={heads} concat={concat} {q}: multi-head {e_fused:.3g}, per-head composition {e_comp:.3g}, "
              f"max |ref| {big:.3g}")
    for q, (e_fused, e_comp, big) in rec.items():
        assert e_fused <= 2 * e_comp + 1e-6 * big, (kind, heads, concat, q, e_fused, e_comp, big)


def _rel_bound(measured):
    """The largest relative allowance the layer tests grant: max over cases and quantities of (2 x composition error + 1e-6 max) / max."""
    return max((2 * e_comp + 1e-6 * big) / big for rec in measured.values() for (_, e_comp, big) in rec.values())


# ---------------------------------------------------------------------------------------------------------------------------------
# one head: the code it always ran
# ---------------------------------------------------------------------------------------------------------------------------------
def test_one_head_is_bit_identical_to_the_single_head_path():
    """GATConv(heads=1) (and concat=False at one head) runs ops.GATAggregate with the arguments it always passed: output and every
    gradient equal, bit for bit, a direct call of that Function on the same parameters; GATHeadsAggregate does not run."""
    from fitgnn_amd import nn as fnn
    from fitgnn_amd import ops
    from fitgnn_amd.csr import csr_for

    ei, n = _graph("stars")
    eid = ei.cuda()
    x = torch.randn(n, 16, generator=torch.Generator().manual_seed(1))
    gout = torch.randn(n, 32, generator=torch.Generator().manual_seed(2)).cuda()
    calls = []
    orig = ops.GATHeadsAggregate.forward
    ops.GATHeadsAggregate.forward = staticmethod(lambda *a, **k: calls.append(1) or orig(*a, **k))
    try:
        for kw in ({}, {"heads": 1}, {"heads": 1, "concat": False}):
            torch.manual_seed(4)
            conv = fnn.GATConv(16, 32, **kw).cuda()
            with torch.no_grad():
                conv.bias.normal_()
            xg = x.cuda().requires_grad_(True)
            out = conv(xg, eid)
            assert type(out.grad_fn).__name__ == "GATAggregateBackward"
            out.backward(gout)
            P = {k: v.detach().clone().requires_grad_(True) for k, v in conv.named_parameters()}
            xr = x.cuda().requires_grad_(True)
            h = ops.Linear.apply(xr.float(), P["lin.weight"], conv.op_config)
            ref = ops.GATAggregate.apply(h, P["att_src"].view(-1), P["att_dst"].view(-1), P["bias"], csr_for(eid, n, "gat"), 0.2,
                                         False, 0.0, False, 0, None, conv.op_config)
            ref.backward(gout)
            assert torch.equal(out, ref) and torch.equal(xg.grad, xr.grad), kw
            for k, p in conv.named_parameters():
                assert torch.equal(p.grad, P[k].grad), (kw, k)
            # the fused ELU / dropout form as well
            mask = (torch.rand(n, 32, generator=torch.Generator().manual_seed(3)) > 0.5).to(torch.uint8).cuda()
            z = conv.forward_elu_dropout(x.cuda(), eid, p=0.5, training=True, mask=mask)
            assert type(z.grad_fn).__name__ == "GATAggregateBackward"
    finally:
        ops.GATHeadsAggregate.forward = orig
    assert not calls


# ---------------------------------------------------------------------------------------------------------------------------------
# models against a float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def _dense_conv(x, sd, i, adj, heads, slope=0.2):
    """conv.i of the model in float64 torch on a dense adjacency (adj[i, j] = 1: j -> i, self loops in): masked softmax per head."""
    n = x.shape[0]
    h3 = (x @ sd[f"conv.{i}.lin.weight"].t()).view(n, heads, -1)
    a_s = (h3 * sd[f"conv.{i}.att_src"].view(1, heads, -1)).sum(-1)
    a_d = (h3 * sd[f"conv.{i}.att_dst"].view(1, heads, -1)).sum(-1)
    e = F.leaky_relu(a_s.unsqueeze(0) + a_d.unsqueeze(1), slope).masked_fill(adj.unsqueeze(2) == 0, float("-inf"))
    out = torch.einsum("ijh,jhc->ihc", torch.softmax(e, dim=1), h3).reshape(n, -1)
    return out + sd[f"conv.{i}.bias"]


def _dense_embed(x, sd, adj, heads, masks, p):
    for i in range(2):
        x = F.elu(_dense_conv(x, sd, i, adj, heads))
        if masks is not None:
            x = x * masks[i].double() / (1.0 - p)
    return x


def _adjacency(ei, n):
    rowptr, col = gr.gat_csr(ei.numpy(), n)
    adj = torch.zeros(n, n, dtype=torch.float64)
    adj[torch.from_numpy(gr.entry_rows(rowptr)), torch.from_numpy(col)] = 1.0
    return adj


def _args(**kw):
    base = dict(num_layers1=2, layer_name="GATConv", num_features=12, hidden=64, num_classes=5, heads=4)
    base.update(kw)
    return argparse.Namespace(**base)


def _check_model(got, ref, bound, what):
    for k, (a, b) in {k: (got[k], ref[k]) for k in ref}.items():
        a, b = a.detach().cpu().double().reshape(-1), b.detach().double().reshape(-1)
        err, big = float((a - b).abs().max()), float(b.abs().max())
        print(f"gat heads model {what} {k}: error {err:.3g} of max |ref| {big:.3g} (allowed {bound * big:.3g})")
        assert err <= bound * big, (what, k, err, big, bound)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "injected_masks"])
def test_classify_node_against_float64_and_on_a_deduplicated_table(measured, train):
    """Classify_node(GATConv, heads=4, hidden=64): log-probabilities, loss and every gradient against the float64 restatement, within
    the layer bound x 2 layers; under x_index (a de-duplicated table) the same values as on the materialised rows."""
    from fitgnn_amd import network, ops

    bound = 2 * _rel_bound(measured)
    ei, n = _graph("stars")
    eid = ei.cuda()
    torch.manual_seed(5)
    model = network.Classify_node(_args()).cuda()
    assert [c.heads for c in model.conv] == [4, 4]
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if name.endswith("bias"):
                prm.normal_(0, 0.3)
    N0 = n // 2
    idx = torch.randint(0, N0, (n,))
    idx[:N0] = torch.arange(N0)
    Xt = torch.randn(N0, 12)
    x = Xt[idx]
    y = torch.randint(0, 5, (n,))
    masks = [(torch.rand(n, 64) > 0.5).to(torch.uint8) for _ in range(2)] if train else None
    model.train(train)
    model._inject_masks = None if masks is None else [m.cuda() for m in masks]

    out = model(x.cuda(), eid)
    assert "GATHeadsAggregate" in repr(_functions(out.grad_fn))
    loss = F.nll_loss(out, y.cuda())
    loss.backward()
    got = dict(out=out, loss=loss, **{k: prm.grad.clone() for k, prm in model.named_parameters()})

    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    emb = _dense_embed(x.double(), sd, _adjacency(ei, n), 4, masks, 0.5)
    ref_out = F.log_softmax(emb @ sd["lt1.weight"].t() + sd["lt1.bias"], dim=1)
    ref_loss = F.nll_loss(ref_out, y)
    ref_loss.backward()
    ref = dict(out=ref_out, loss=ref_loss, **{k: v.grad for k, v in sd.items()})
    _check_model(got, ref, bound, "Classify_node " + ("train" if train else "eval"))

    model.zero_grad()
    out_t = model(Xt.cuda(), eid, x_index=ops.RowIndex(idx.cuda(), N0))
    F.nll_loss(out_t, y.cuda()).backward()
    assert torch.equal(out_t, out), "the de-duplicated table gives other values than its materialised rows"
    for k, prm in model.named_parameters():
        assert torch.equal(prm.grad, got[k]), k
    model._inject_masks = None


def _functions(fn):
    """Names of the autograd nodes below fn."""
    seen, todo = set(), [fn]
    while todo:
        f = todo.pop()
        if f is not None and f not in seen:
            seen.add(f)
            todo += [nxt for nxt, _ in f.next_functions]
    return {type(f).__name__ for f in seen}


@pytest.mark.parametrize("train", [False, True], ids=["eval", "injected_masks"])
def test_regress_graph_gs_against_float64(measured, train):
    """Regress_graph_gs(GATConv, heads=4, hidden=64) on a pre-merged union of six subgraphs of three graphs: outputs, L1 loss and
    every gradient against the float64 restatement, within the layer bound x 2 layers."""
    from fitgnn_amd import network

    bound = 2 * _rel_bound(measured)
    ei, n = _graph("stars")
    torch.manual_seed(6)
    model = network.Regress_graph_gs(_args()).cuda()
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if name.endswith("bias"):
                prm.normal_(0, 0.3)
    x = torch.randn(n, 12)
    ptr = np.concatenate([[0], np.cumsum([100, 7, 17, 3, 1, 64])])
    graph_of_block = np.array([0, 0, 1, 1, 2, 2])
    keep = torch.rand(n) < 0.6
    keep[torch.from_numpy(ptr[:-1])] = True                      # every subgraph contributes a row
    rows = torch.nonzero(keep).flatten()
    batch = torch.from_numpy(graph_of_block[np.searchsorted(ptr, rows.numpy(), side="right") - 1])
    tgt = torch.randn(3, 1)
    masks = [(torch.rand(n, 64) > 0.5).to(torch.uint8) for _ in range(2)] if train else None
    model.train(train)
    model._inject_masks = None if masks is None else [m.cuda() for m in masks]
    set_gs = dict(x=x.cuda(), edge_index=ei.cuda(), mask=keep.cuda(), mask_idx=rows.cuda(), n_graphs=3)
    out = model(set_gs, batch.cuda())
    loss = F.l1_loss(out, tgt.cuda())
    loss.backward()
    got = dict(out=out, loss=loss, **{k: prm.grad.clone() for k, prm in model.named_parameters()})

    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    emb = _dense_embed(x.double(), sd, _adjacency(ei, n), 4, masks, 0.5)[rows]
    pooled = torch.zeros(3, 64, dtype=torch.float64).index_add_(0, batch, emb) / torch.bincount(batch, minlength=3).double().unsqueeze(1)
    ref_out = pooled @ sd["lt1.weight"].t() + sd["lt1.bias"]
    ref_loss = F.l1_loss(ref_out, tgt.double())
    ref_loss.backward()
    ref = dict(out=ref_out, loss=ref_loss, **{k: v.grad for k, v in sd.items()})
    _check_model(got, ref, bound, "Regress_graph_gs " + ("train" if train else "eval"))
    model._inject_masks = None


# ---------------------------------------------------------------------------------------------------------------------------------
# trainer, serving, command line
# ---------------------------------------------------------------------------------------------------------------------------------
def _six_subgraph_batch(F_in=12, dedup=True):
    """A union of six cluster subgraphs with shared extra nodes (tests/test_gpu_query.py's construction) and a train mask."""
    from fitgnn_amd import data as fdata

    N, K = 90, 6
    rng = np.random.default_rng(5)
    ei = fdata.synthetic_graph(N, 220, seed=2)
    assign = rng.integers(0, K, size=N)
    assign[:K] = np.arange(K)
    X = rng.normal(size=(N, F_in)).astype(np.float32)
    y = rng.integers(0, 5, size=N)
    sub = fdata.assemble_subgraphs(ei, N, assign, K, extra_node=True)
    assert len(sub["ptr"]) - 1 == K
    return fdata.SubgraphBatch(sub, X, y, rng.random(N) < 0.5, device="cuda", dedup=dedup)


def test_gd_trainer_default_step_equals_the_eager_step():
    """Three GDTrainer steps with heads=4, dropout off: the default step and capture=False give the same losses and weights, bit
    for bit.  GDTrainer captures GCN-only and `logits` models, no GATConv model: both runs here are eager, so this shows that the
    multi-head step through the trainer (de-duplicated table gathered to rows, flat gradient buffer, fused loss) is reproducible and
    that the default takes no other path -- it shows nothing about hipGraph capture, which no test does for a multi-head step."""
    from fitgnn_amd import network, train

    batch = _six_subgraph_batch()
    runs = []
    for kw in ({}, {"capture": False}):
        torch.manual_seed(8)
        model = network.Classify_node(_args(dropout=0.0)).cuda()
        tr = train.GDTrainer(model, batch, lr=0.01, weight_decay=5e-4, **kw)
        losses = [float(tr.step()) for _ in range(3)]
        assert all(np.isfinite(losses)) and losses[2] != losses[0]
        runs.append((losses, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_query_engine_reports_not_fused_and_answers_with_the_models_forward():
    """QueryEngine(gat_kernels=True) on a heads=2 model: the attention query kernels take one score per row, so the engine is not
    fused and answers with the model's own per-subgraph forward -- the same launches on the same subgraphs: 1e-5 of the largest
    value allows another GEMM tile plan's rounding and nothing a wrong path would give."""
    from fitgnn_amd import network, ops, serve
    from test_gpu_gat_query import _per_subgraph

    batch = _six_subgraph_batch()
    torch.manual_seed(9)
    model = network.Classify_node(_args(heads=2)).cuda().eval()
    assert not ops.gat_query_supported(model) and not ops.gat_graph_query_supported(model)
    eng = serve.QueryEngine(model, batch, gat_kernels=True)
    assert eng.fused is False and eng.table_bytes == 0
    rows = torch.nonzero(batch.core).flatten()
    out = eng.predict(batch.node_id[rows])
    ref = _per_subgraph(model, batch, rows)
    assert out.shape == ref.shape == (len(rows), 5)
    assert float((out - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    one = network.Classify_node(_args(heads=1)).cuda().eval()
    assert ops.gat_query_supported(one)   # the single-head model keeps its kernels


def test_command_line_trains_four_heads_on_cora(tmp_path, monkeypatch):
    """main.py --layer_name GATConv --heads 4 --hidden 64 on the Cora files for 2 epochs: it runs, writes its results row, and the
    checkpoint's attention vectors are [1, 4, 16]."""
    sys.path.insert(0, os.path.join(ROOT, "fit-gnn_amd"))
    import main as cli

    raw = tmp_path / "dataset" / "cora"
    raw.mkdir(parents=True)
    os.symlink(os.path.join(ROOT, "tests", "golden", "cora_raw"), raw / "raw")
    monkeypatch.chdir(tmp_path)
    cli.main(["--dataset", "cora", "--data_root", str(tmp_path / "dataset"), "--runs", "1", "--seed", "0", "--layer_name", "GATConv",
              "--heads", "4", "--hidden", "64", "--output_dir", "h", "--train_fitgnn", "--exp_setup", "Gs_train_2_Gs_infer",
              "--extra_node", "--coarsening_ratio", "0.5", "--epochs1", "2", "--epochs2", "2"])
    rows = open("results/cora.csv").read().strip().split("\n")
    assert rows[0].startswith("dataset,coarsening_method,coarsening_ratio") and len(rows) == 2 and ",GATConv," in rows[1]
    sd = torch.load("save/node_cls/h/model.pt")
    assert tuple(sd["conv.0.att_src"].shape) == (1, 4, 16) and tuple(sd["conv.1.att_dst"].shape) == (1, 4, 16)
    assert tuple(sd["conv.0.lin.weight"].shape) == (64, 1433) and tuple(sd["lt1.weight"].shape) == (7, 64)
