#!/usr/bin/env python3
"""Latency of one node query through fitgnn_amd.serve.QueryEngine against the per-subgraph forward inference.py times without
--query_engine, on a workloads.py union (GPU only).

    python tools/query_latency.py --workload S-pubmed [--layer GATConv | SAGEConv | GINConv] [--hidden 512] [--samples 256] [--rounds 5] [--out FILE]

--layer GATConv: a two-layer GAT model through QueryEngine(gat_kernels=True) (fitgnn_gat_query_gather_f32 and the same tail).
--layer GATConv --heads N (2..8): the model with N attention heads per layer through QueryEngine(gat_heads_kernels=True)
(fitgnn_mhgat_query_gather_f32 and fitgnn_mhgat_query_tail_f32); writes profiles/query_latency_node_GATConv_heads<N>.json.
--layer SAGEConv: a two-layer SAGE model through QueryEngine(sage_kernels=True) (fitgnn_sage_query_gather_f32 over the mean CSR and the
same tail with K = 2H).
--layer GINConv: a two-layer GIN model through QueryEngine(gin_kernels=True) (fitgnn_gin_query_hops_f32 over the sum CSR, with a dense
H x H product per one-hop row, and fitgnn_gin_query_tail_f32).
Writes profiles/query_latency_<workload>.json (profiles/query_latency_<workload>_<layer>.json with --layer GATConv / SAGEConv / GINConv; or --out):
  (a) engine_single      median / p90 seconds of predict_rows([row]) per sampled core row, bracketed by device synchronisations as
                         inference.py brackets its forward;
  (b) subgraph_forward   the same rows through inference.timed_forward on the cached subgraph with its CSR pre-built -- measured TWICE
                         per row (b1 before the engine's turn, b2 after it) so that its own run-to-run spread is known;
                         (a), (b1), (b2) alternate row by row inside one process, after one untimed pass over every row;
  (c) engine_batch       queries per second at Q = --batch, and the gather kernel alone: sum_q sum_{j in row q} deg(j) * H * 4 bytes
                         (GATConv: + deg(q) rows for h_q; SAGEConv: sum_j deg(j) + deg(q) aggregate half-rows and deg(q) + 1 root
                         half-rows of 4 H bytes, 12 bytes of CSR per entry, 8 H bytes written per query; GINConv: sum_j deg(j) + 2 deg(q) + 1
                         table rows, 12 bytes of CSR per entry, 4 H bytes written and ceil((deg(q) + 1) / 16) passes over the 4 H H bytes of
                         W0b per query, which come from L2: gather_bytes counts them, so its rate is not an HBM rate) over its HIP-event time, next to
                         fitgnn_stream_copy_f32's rate in the same process.
The engine's answers are compared with the per-subgraph forward's on every sampled row (max relative difference is recorded).

    python tools/query_latency.py --task graph_reg | graph_cls [--layer GINConv | GATConv | SAGEConv] [--n_graphs 2000] [--view gs | gc | orig] [--hidden 512]
                                  [--samples 256] [--rounds 5] [--batch 1024] [--out FILE]

--task graph_reg / graph_cls: one GRAPH query through fitgnn_amd.serve.GraphQueryEngine (fitgnn_gcn_graph_query_hops_f32 and
fitgnn_gcn_graph_query_tail_f32) against the per-graph forward inference.py times without --query_engine, on a GraphSet of
graph_data.synthetic_molecules (graph_reg: Regress_graph_gs / _gc) or synthetic_graph_classes (graph_cls: Classify_graph_gs / _gc),
extra-node layout.  --layer GINConv: a two-layer GIN model through GraphQueryEngine(gin_kernels=True)
(fitgnn_gin_graph_query_hops_f32 over the sum CSR and fitgnn_gin_graph_query_tail_f32).  --layer GATConv: a two-layer GAT model through
GraphQueryEngine(gat_kernels=True) (fitgnn_gat_graph_query_hops_f32 over the "gat" CSR and fitgnn_gcn_graph_query_tail_f32).
--layer SAGEConv: a two-layer SAGE model through GraphQueryEngine(sage_kernels=True) (fitgnn_sage_graph_query_hops_f32 over the mean CSR
and fitgnn_gcn_graph_query_tail_f32 with K = 2H).  Writes profiles/query_latency_<task>_<view>.json
(profiles/query_latency_<task>_<view>_<layer>.json with --layer GINConv / GATConv / SAGEConv; or --out):
  (a) engine_single      predict([g]) per sampled graph, bracketed as above;
  (b) graph_forward      the model on the graph cut out of the set (gset.batch(g, g + 1, view), its CSR and pool index pre-built),
                         measured twice per graph around the engine's turn, after one untimed pass;
  (c) engine_batch       predict(ids) at Q = --batch (ids drawn with repeats) against the same graphs one forward each (the loop (b)
                         runs) and against ONE forward of the model on gset.batch_ids(the unique ids) pre-built;
  table_row_reads        counted, not timed: sum over the pooled rows r of sum_{c in row r} deg(c) (the per-row gather on every pooled
                         row) against sum over every row of the queried graphs of deg(r) (each layer-0 row formed once), and their ratio
                         (--layer GINConv / SAGEConv: plus the root row of every layer-0 row formed, on both sides);
  dense_rows             --layer GINConv, counted, not timed: the layer-0 rows that take the dense Hb x Ha product -- every row of the
                         view once (the window path) against sum over the pooled rows r of deg(r) + 1 (fitgnn_gin_query_hops_f32 on
                         every pooled row), and their ratio;
  attention_rows         --layer GATConv, counted, not timed: the layer-0 attention rows formed (a softmax, a gather and two score dots
                         each) -- every row of the view once (the window path) against sum over the pooled rows r of deg(r) + 1
                         (fitgnn_gat_query_gather_f32 on every pooled row, with one h_q per wave that has entries counted once), and
                         their ratio;
  sage_rows              --layer SAGEConv, counted, not timed: the layer-0 rows formed (a gather of deg + 1 table half-rows each) -- every
                         row of the view once (the window path) against sum over the pooled rows r of deg(r) + 1
                         (fitgnn_sage_query_gather_f32 on every pooled row), and their ratio."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fit-gnn_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


def _stats(t):
    import numpy as np
    t = np.asarray(t)
    return dict(median_us=round(float(np.median(t)) * 1e6, 2), p90_us=round(float(np.percentile(t, 90)) * 1e6, 2),
                mean_us=round(float(t.mean()) * 1e6, 2), n=int(t.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="S-pubmed")
    ap.add_argument("--layer", default="GCNConv", choices=["GCNConv", "GATConv", "SAGEConv", "GINConv"])
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--heads", type=int, default=1, help="--layer GATConv --task node: attention heads per layer (hidden // heads wide each)")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--task", default="node", choices=["node", "graph_reg", "graph_cls"])
    ap.add_argument("--n_graphs", type=int, default=2000)
    ap.add_argument("--view", default="gs", choices=["gs", "gc", "orig"])
    a = ap.parse_args()
    if a.heads != 1 and (a.layer != "GATConv" or a.task != "node"):
        ap.error("--heads goes with --layer GATConv --task node")
    if a.task != "node":
        return graph_main(a)

    import time

    import numpy as np
    import torch

    import inference
    from fitgnn_amd import _lib, network, serve, workloads
    from fitgnn_amd.csr import csr_for

    assert torch.cuda.is_available(), "query_latency.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    N, E, F, C, r = workloads.SHAPES[a.workload]
    wl = workloads.coarsen_workload(a.workload, dev)
    sub, _ = workloads.assemble(a.workload, torch.from_numpy(np.ascontiguousarray(wl["ei"])).to(dev),
                                torch.from_numpy(np.ascontiguousarray(wl["assign"])).to(dev), wl["n_clusters"])
    batch = workloads.batch_from_subgraphs(a.workload, sub, dev)
    del sub, wl
    margs = argparse.Namespace(num_layers1=2, layer_name=a.layer, num_features=F, hidden=a.hidden, num_classes=C, heads=a.heads)
    torch.manual_seed(2)
    model = network.Classify_node(margs).to(dev).eval()
    gat = a.layer == "GATConv"
    mh = gat and a.heads > 1
    sage = a.layer == "SAGEConv"
    gin = a.layer == "GINConv"
    engine = serve.QueryEngine(model, batch, gat_kernels=gat, sage_kernels=sage, gin_kernels=gin, gat_heads_kernels=mh)
    path = engine.path()
    assert path is not None and path.name == ("gat_heads" if mh else a.layer[:-4].lower())
    t0 = time.time()
    engine.refresh()
    torch.cuda.synchronize()
    t_table = time.time() - t0

    rng = np.random.default_rng(0)
    core_rows = torch.nonzero(batch.core).flatten().cpu().numpy()
    rows = core_rows[rng.permutation(len(core_rows))[: a.samples]]
    ptr, ei = batch.ptr, batch.edge_index
    subs = np.searchsorted(ptr, rows, side="right") - 1
    cache = {}
    for s in np.unique(subs):   # exactly inference.py's cache: the subgraph as its own graph, its CSR built outside the timed call
        r0, r1 = int(ptr[s]), int(ptr[s + 1])
        m = (ei[0] >= r0) & (ei[0] < r1)
        cache[int(s)] = (batch.x[r0:r1].contiguous(), (ei[:, m] - r0).contiguous(), r0)
        csr_for(cache[int(s)][1], r1 - r0, serve._layer_mode(model))

    def engine_once(row):
        torch.cuda.synchronize(dev)
        t = time.time()
        out = engine.predict_rows([row])
        torch.cuda.synchronize(dev)
        return out, time.time() - t

    def forward_once(row, s):
        x, e, r0 = cache[s]
        out, dt = inference.timed_forward(model, x, e, dev)
        return out[row - r0], dt

    worst = 0.0
    with torch.no_grad():
        for row, s in zip(rows.tolist(), subs.tolist()):   # untimed pass: every shape warmed, answers compared
            oa, _ = engine_once(row)
            ob, _ = forward_once(row, s)
            worst = max(worst, float((oa[0] - ob).abs().max() / ob.abs().max().clamp(min=1e-20)))
        ta, tb1, tb2 = [], [], []
        per_round = []
        for _ in range(a.rounds):
            ra, r1_, r2_ = [], [], []
            for row, s in zip(rows.tolist(), subs.tolist()):
                r1_.append(forward_once(row, s)[1])
                ra.append(engine_once(row)[1])
                r2_.append(forward_once(row, s)[1])
            per_round.append(dict(engine_median_us=round(float(np.median(ra)) * 1e6, 2), forward_first_median_us=round(float(np.median(r1_)) * 1e6, 2),
                                  forward_second_median_us=round(float(np.median(r2_)) * 1e6, 2)))
            ta += ra; tb1 += r1_; tb2 += r2_

        # (c) a batch of queries: the two launches end to end, and the gather kernel alone by HIP events
        qrows = torch.from_numpy(core_rows[rng.integers(0, len(core_rows), size=a.batch)]).to(dev)
        for _ in range(3):
            engine.predict_rows(qrows)
        torch.cuda.synchronize()
        reps = 20
        t = time.time()
        for _ in range(reps):
            engine.predict_rows(qrows)
        torch.cuda.synchronize()
        t_batch = (time.time() - t) / reps
        f, state = engine.csr().f, engine.state()
        T = state[0]
        xrow = batch.row_index.index if batch.row_index is not None else None
        G = torch.empty((a.batch, path.g_width(state, model)), dtype=torch.float32, device=dev)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record()
            path.rows_hops(f, state, model, qrows, xrow=xrow, out=G)
            e1.record()
        torch.cuda.synchronize()
        t_gather = float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])) * 1e-3
        deg = (f.rowptr[1:] - f.rowptr[:-1]).long()
        csum = torch.zeros(f.col.numel() + 1, dtype=torch.int64, device=dev)
        csum[1:] = torch.cumsum(deg.index_select(0, f.col.long()), 0)     # prefix sums of deg(col[e]) over the entries
        rp = f.rowptr.long()
        table_rows = int((csum[rp[qrows + 1]] - csum[rp[qrows]]).sum())
        if gat:   # every query also forms h_q from its own row
            table_rows += int(deg[qrows].sum())
        gather_bytes = table_rows * a.hidden * 4
        if sage:   # aggregate half-rows of the neighbours' rows and of row q itself, one root half-row per layer-0 row made
            dq = int(deg[qrows].sum())
            table_rows += dq
            gather_bytes = (table_rows + dq + a.batch) * a.hidden * 4 + 12 * table_rows + a.batch * 8 * a.hidden
        if gin:   # every layer-0 row made also reads its own table row; W0b once per tile of 16 items
            dq = int(deg[qrows].sum())
            tiles = int(((deg[qrows] + 1 + 15) // 16).sum())
            table_rows += 2 * dq + a.batch
            gather_bytes = table_rows * a.hidden * 4 + 12 * (table_rows - dq - a.batch) + a.batch * 4 * a.hidden + tiles * 4 * a.hidden * a.hidden
        n = 64 * 1024 * 1024
        src, dst = torch.empty(n, dtype=torch.float32, device=dev).normal_(), torch.empty(n, dtype=torch.float32, device=dev)
        cev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(10)]
        for e0, e1 in cev:
            e0.record()
            _lib.check(_lib.lib().fitgnn_stream_copy_f32(_lib.dptr(src), _lib.dptr(dst), n, _lib.stream_ptr(dev)), "fitgnn_stream_copy_f32")
            e1.record()
        torch.cuda.synchronize()
        t_copy = float(np.median([e0.elapsed_time(e1) for e0, e1 in cev][2:])) * 1e-3

    sa, s1, s2 = _stats(ta), _stats(tb1), _stats(tb2)
    base = min(s1["median_us"], s2["median_us"])
    spread = abs(s1["median_us"] - s2["median_us"])
    res = dict(workload=a.workload, layer=a.layer, heads=a.heads, hidden=a.hidden, classes=C, union_rows=int(batch.n_rows), nnz=int(batch.nnz), subgraphs=int(len(ptr) - 1),
               samples=int(len(rows)), rounds=a.rounds, device=torch.cuda.get_device_name(0),
               table=dict(rows=int(T.shape[0]), bytes=engine.table_bytes, build_s=round(t_table, 4)),
               engine_single=sa, subgraph_forward_first=s1, subgraph_forward_second=s2, per_round=per_round,
               subgraph_forward_spread_us=round(spread, 2), engine_below_forward_by_us=round(base - sa["median_us"], 2),
               engine_faster_beyond_spread=bool(base - sa["median_us"] > spread),
               max_rel_diff_engine_vs_forward=worst,
               engine_batch=dict(Q=a.batch, seconds=round(t_batch, 6), queries_per_s=round(a.batch / t_batch, 1),
                                 gather_kernel_s=round(t_gather, 6), gather_table_rows=table_rows, gather_bytes=gather_bytes,
                                 gather_GBps=round(gather_bytes / t_gather / 1e9, 1),
                                 stream_copy_GBps=round(2 * 4 * n / t_copy / 1e9, 1)))
    name = f"query_latency_node_GATConv_heads{a.heads}.json" if mh else f"query_latency_{a.workload}{'_' + a.layer if gat or sage or gin else ''}.json"
    out = a.out or os.path.join(ROOT, "profiles", name)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def graph_main(a):
    import time
    import types

    import numpy as np
    import torch

    from fitgnn_amd import graph_data, network, serve
    from fitgnn_amd.train import _cat_pieces

    assert torch.cuda.is_available(), "query_latency.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    reg = a.task == "graph_reg"
    mol = graph_data.synthetic_molecules(a.n_graphs, seed=0) if reg else graph_data.synthetic_graph_classes(a.n_graphs, seed=0)
    gset = graph_data.GraphSet(mol, ratio=0.5, extra_node=True, device=dev)
    gs = a.view == "gs"
    cls = ("Regress_graph_" if reg else "Classify_graph_") + ("gs" if gs else "gc")
    C = 1 if reg else int(mol["y"].max()) + 1
    gin, gat, sage = a.layer == "GINConv", a.layer == "GATConv", a.layer == "SAGEConv"
    margs = argparse.Namespace(num_layers1=2, layer_name=a.layer, num_features=int(gset.x.shape[1]), hidden=a.hidden, num_classes=C)
    torch.manual_seed(2)
    model = getattr(network, cls)(margs).to(dev).eval()
    engine = serve.GraphQueryEngine(model, gset, view=a.view, gin_kernels=gin, gat_kernels=gat, sage_kernels=sage)
    path = engine.path()
    assert path is not None and path.name == a.layer[:-4].lower()
    t0 = time.time()
    engine.refresh()
    torch.cuda.synchronize()
    t_table = time.time() - t0

    rng = np.random.default_rng(0)
    graphs = rng.permutation(gset.n_graphs)[: a.samples].tolist()
    kind = "gs" if gs else "gc"   # (how _cat_pieces shapes the batch: the "orig" view is a *_gc model's input too)
    cache = {g: _cat_pieces([gset.batch(g, g + 1, a.view)], kind, types) for g in graphs}   # inference.py's batch, built outside the timed call

    def call(b):
        return model(b, b["graph_of_masked"]) if gs else model(b["gc"])

    def engine_once(g):
        torch.cuda.synchronize(dev)
        t = time.time()
        out = engine.predict([g])
        torch.cuda.synchronize(dev)
        return out, time.time() - t

    def forward_once(g):
        torch.cuda.synchronize(dev)
        t = time.time()
        out = call(cache[g])
        torch.cuda.synchronize(dev)
        return out, time.time() - t

    worst = 0.0
    with torch.no_grad():
        for g in graphs:   # untimed pass: every shape warmed, answers compared
            oa, ob = engine_once(g)[0], forward_once(g)[0].reshape(1, -1)
            worst = max(worst, float((oa - ob).abs().max() / ob.abs().max().clamp(min=1e-20)))
        ta, tb1, tb2, per_round = [], [], [], []
        for _ in range(a.rounds):
            ra, r1_, r2_ = [], [], []
            for g in graphs:
                r1_.append(forward_once(g)[1])
                ra.append(engine_once(g)[1])
                r2_.append(forward_once(g)[1])
            per_round.append(dict(engine_median_us=round(float(np.median(ra)) * 1e6, 2), forward_first_median_us=round(float(np.median(r1_)) * 1e6, 2),
                                  forward_second_median_us=round(float(np.median(r2_)) * 1e6, 2)))
            ta += ra; tb1 += r1_; tb2 += r2_

        # (c) a batch of graph queries
        ids = rng.integers(0, gset.n_graphs, size=a.batch)
        ids_d = torch.from_numpy(ids).to(dev)
        uniq = np.unique(ids)
        whole = _cat_pieces([gset.batch_ids(uniq.tolist(), a.view)], kind, types)
        reps = 20

        def timed(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t = time.time()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return (time.time() - t) / reps

        t_batch = timed(lambda: engine.predict(ids_d))
        t_whole = timed(lambda: call(whole))

    # counted: table rows read by the per-row gather on every pooled row against every layer-0 row formed once
    f = engine.csr().f
    deg = (f.rowptr[1:] - f.rowptr[:-1]).long()
    csum = torch.zeros(f.col.numel() + 1, dtype=torch.int64, device=dev)
    csum[1:] = torch.cumsum(deg.index_select(0, f.col.long()), 0)
    rp = f.rowptr.long()
    prow = engine._prow
    per_row = int((csum[rp[prow + 1]] - csum[rp[prow]]).sum())
    once = int(deg.sum())
    if gin or sage:   # every layer-0 row formed also reads its own table row (SAGEConv: its root half-row)
        per_row += int(deg[prow].sum()) + int(prow.numel())
        once += int(engine.n_rows)

    sa, s1, s2 = _stats(ta), _stats(tb1), _stats(tb2)
    base = min(s1["median_us"], s2["median_us"])
    spread = abs(s1["median_us"] - s2["median_us"])
    res = dict(task=a.task, view=a.view, model=cls, layer=a.layer, hidden=a.hidden, classes=C, graphs=int(gset.n_graphs), view_rows=int(engine.n_rows),
               nnz=int(f.col.numel()), pooled_rows=int(prow.numel()), samples=len(graphs), rounds=a.rounds, device=torch.cuda.get_device_name(0),
               table=dict(rows=int(engine.n_rows), bytes=engine.table_bytes, build_s=round(t_table, 4)),
               engine_single=sa, graph_forward_first=s1, graph_forward_second=s2, per_round=per_round,
               graph_forward_spread_us=round(spread, 2), engine_below_forward_by_us=round(base - sa["median_us"], 2),
               engine_faster_beyond_spread=bool(base - sa["median_us"] > spread), max_rel_diff_engine_vs_forward=worst,
               engine_batch=dict(Q=a.batch, unique_graphs=int(len(uniq)), seconds=round(t_batch, 6), graphs_per_s=round(a.batch / t_batch, 1),
                                 one_forward_per_graph_s=round(a.batch * base * 1e-6, 6),
                                 one_forward_on_the_unique_graphs_s=round(t_whole, 6)),
               table_row_reads=dict(per_row_gather=per_row, each_row_once=once, ratio=round(per_row / max(once, 1), 3)))
    if gin or gat or sage:   # the layer-0 rows formed by the per-row kernel on every pooled row, against every row of the view once
        block, per_row_key = {"gin": ("dense_rows", "per_row_hops"), "gat": ("attention_rows", "per_row_gather"),
                              "sage": ("sage_rows", "per_row_gather")}[path.name]
        formed = int(deg[prow].sum()) + int(prow.numel())
        res[block] = {per_row_key: formed, "each_row_once": int(engine.n_rows), "ratio": round(formed / max(int(engine.n_rows), 1), 3),
                      "window_rows": int(path.window_limit(engine.state(), model)), "largest_graph_rows": int(np.diff(engine._ptr).max())}
    out = a.out or os.path.join(ROOT, "profiles", f"query_latency_{a.task}_{a.view}{'_' + a.layer if gin or gat or sage else ''}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
