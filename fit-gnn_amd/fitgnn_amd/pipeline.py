"""Node-level FIT-GNN pipeline behind main.py: dataset -> components -> coarsen -> Gc / Gs -> train -> infer.

Restates, on device-resident structures, what the reference does for `--task node_cls`:
    utils.coarsening_classification   utils.py:143-374   components, coarsen(), cluster map, subgraphs Gs
    utils.splits_classification       utils.py:612-643   fixed / random / few / ogbn_split masks
    utils.load_data_classification    utils.py:661-778   Gc features C.X, pooled labels and masks, Gc edges, Gs masks
    run.node_classification           run.py:329-506     exp_setup loops, best-val checkpoint, results CSV
    run.node_classification_baseline  run.py:832-902     full-graph baseline
The contraction step, pooling and all message passing run through libfitgnn_hip.so; index bookkeeping is
vectorised NumPy/torch instead of the reference's per-node Python loops.
"""
import os
import pickle
import time

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from . import coarsening, data as fdata, network
from .train import GDTrainer, MBTrainer, broadcast_parameters

SYNTHETIC_SHAPES = {  # name: (N, E, F, classes)   dataset_info.csv:4-7
    "synthetic-cora": (2708, 5278, 1433, 7),
    "synthetic-citeseer": (3327, 4552, 3703, 6),
    "synthetic-pubmed": (19717, 44324, 500, 3),
    "synthetic-physics": (34493, 247962, 8415, 5),
}


class NodeData:
    """The fields of a PyG `Data` object the node-level path reads."""

    def __init__(self, x, edge_index, y, train_mask=None, val_mask=None, test_mask=None):
        self.x, self.edge_index, self.y = x, edge_index, y
        self.num_nodes = x.shape[0]
        z = torch.zeros(self.num_nodes, dtype=torch.bool)
        self.train_mask = z.clone() if train_mask is None else train_mask
        self.val_mask = z.clone() if val_mask is None else val_mask
        self.test_mask = z.clone() if test_mask is None else test_mask


def load_planetoid(root, name):
    """Planetoid raw files ind.<name>.{x,tx,allx,y,ty,ally,graph,test.index} (the format torch_geometric's Planetoid
    downloads; the reference ships Cora/CiteSeer copies under Baselines/SGGC/APPNP/dataset/<name>/raw)."""
    def rd(suffix):
        with open(os.path.join(root, f"ind.{name}.{suffix}"), "rb") as f:
            return pickle.load(f, encoding="latin1")

    x, tx, allx, y, ty, ally, graph = (rd(s) for s in ("x", "tx", "allx", "y", "ty", "ally", "graph"))
    test_idx = np.loadtxt(os.path.join(root, f"ind.{name}.test.index"), dtype=np.int64)
    test_sorted = np.sort(test_idx)
    if name == "citeseer":  # isolated test nodes are missing from tx/ty: pad with zeros (PyG does the same)
        full = np.arange(test_sorted[0], test_sorted[-1] + 1)
        tx_ext = sp.lil_matrix((len(full), tx.shape[1]))
        tx_ext[test_sorted - test_sorted[0], :] = tx
        ty_ext = np.zeros((len(full), ty.shape[1]))
        ty_ext[test_sorted - test_sorted[0], :] = ty
        tx, ty = tx_ext, ty_ext
    feats = sp.vstack([allx, tx]).tolil()
    feats[test_idx, :] = feats[test_sorted, :]
    labels = np.vstack([ally, ty])
    labels[test_idx, :] = labels[test_sorted, :]
    N = feats.shape[0]
    src, dst = [], []
    for u, nbrs in graph.items():
        for v in nbrs:
            if u != v:
                src += [u, v]
                dst += [v, u]
    ei = np.unique(np.array([src, dst], dtype=np.int64), axis=1)
    ei = ei[:, (ei[0] < N) & (ei[1] < N)]
    yv = torch.from_numpy(labels.argmax(1).astype(np.int64))
    train = torch.zeros(N, dtype=torch.bool); val = train.clone(); test = train.clone()
    train[: y.shape[0]] = True
    val[y.shape[0]: y.shape[0] + 500] = True
    test[torch.from_numpy(test_idx)] = True
    return NodeData(torch.from_numpy(np.asarray(feats.todense(), dtype=np.float32)), ei, yv, train, val, test), int(labels.shape[1])


def synthetic_dataset(name, seed=0):
    """Seeded stand-in of a dataset's shape (no network access for the real files): preferential-attachment graph,
    labels = a noisy function of graph position so that the task is learnable, features = class centroid + noise."""
    N, E, Fdim, C = SYNTHETIC_SHAPES[name]
    rng = np.random.default_rng(seed)
    ei = fdata.synthetic_graph(N, E, seed=seed)
    W = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(N, N))
    lab = rng.integers(0, C, size=N)
    for _ in range(3):  # smooth labels over the graph so neighbours agree (homophily)
        onehot = np.eye(C)[lab]
        lab = np.asarray((W @ onehot) + 0.5 * onehot + 1e-3 * rng.random((N, C))).argmax(1)
    # bag-of-words features: 12 words per node, 70 % drawn from the class's own block of the vocabulary
    words = 12
    own = rng.random((N, words)) < 0.7
    blk = Fdim // C
    w_own = lab[:, None] * blk + rng.integers(0, blk, size=(N, words))
    w_any = rng.integers(0, Fdim, size=(N, words))
    w = np.where(own, w_own, w_any)
    X = np.zeros((N, Fdim), dtype=np.float32)
    X[np.repeat(np.arange(N), words), w.ravel()] = 1.0
    d = NodeData(torch.from_numpy(X), ei, torch.from_numpy(lab.astype(np.int64)))
    perm = rng.permutation(N)
    d.train_mask[perm[: 20 * C]] = True
    d.val_mask[perm[20 * C: 20 * C + 500]] = True
    d.test_mask[perm[20 * C + 500: 20 * C + 1500]] = True
    return d, C


def splits_classification(data, num_classes, exp, rng=None):
    """utils.py:612-643."""
    if exp == "fixed":
        return data
    g = torch.Generator().manual_seed(int(rng.integers(0, 2 ** 31))) if rng is not None else None
    idxs = []
    for c in range(num_classes):
        idx = (data.y.flatten() == c).nonzero().view(-1)
        idxs.append(idx[torch.randperm(idx.numel(), generator=g)])
    N = data.num_nodes
    if exp == "random":
        tr, va, te = (torch.cat([i[:20] for i in idxs]), torch.cat([i[20:50] for i in idxs]), torch.cat([i[50:] for i in idxs]))
    elif exp == "few":
        tr, va, te = (torch.cat([i[:5] for i in idxs]), torch.cat([i[5:10] for i in idxs]), torch.cat([i[10:] for i in idxs]))
    elif exp == "ogbn_split":
        p = torch.randperm(N, generator=g)
        tr, va, te = p[: int(0.08 * N)], p[int(0.08 * N): int(0.1 * N)], p[int(0.1 * N):]
    else:
        raise ValueError(exp)
    for name, idx in (("train_mask", tr), ("val_mask", va), ("test_mask", te)):
        m = torch.zeros(N, dtype=torch.bool)
        m[idx] = True
        setattr(data, name, m)
    return data


class Coarsened:
    """Result of coarsening_classification: per-component C / Gc and the global node -> cluster map."""
    pass


def coarsening_classification(args, data, coarsening_ratio, coarsening_method, device="cuda", batched=True):
    """utils.py:143-184: components sorted by size (descending, stable), coarsen() on every component with more
    than one node (Loukas r = 1 - --coarsening_ratio is passed by main.py:278), node -> cluster map from the
    level mapping dicts; single nodes are their own cluster.

    The matching methods (heavy_edge, algebraic_JC, variation_edges) take the node -> cluster map of utils.py:167-182: the
    row of the single non-zero in each column of C -- the same row the composed level dicts give for variation_neighborhoods,
    so one construction serves both.  affinity_GS is refused here: the reference maps it through its identity level dicts
    (every node its own meta-node), which no caller can use; coarsen() supports it.  The random methods (algebraic_JC) run
    coarsen() per component, which keeps the reference's np.random draw order (component by component, level by level)."""
    coarsening.check_method(coarsening_method)
    if coarsening_method == "affinity_GS":
        raise NotImplementedError("affinity_GS is supported by coarsening.coarsen() but not by the pipeline: the reference maps "
                                  "every node to its own meta-node for it (utils.py:182 on identity level dicts)")
    N = data.num_nodes
    ei = np.asarray(data.edge_index)
    W = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(N, N))
    W.data[:] = 1.0
    comps = coarsening.Graph(W).extract_components()
    comps = sorted(comps, key=lambda g: len(g.info["orig_idx"]), reverse=True)  # utils.py:146 (stable)
    out = Coarsened()
    out.components, out.C_list, out.Gc_list = comps, [], []   # *_list: components with > 10 nodes only (:164-166)
    out.all_C, out.all_Gc = [], []
    assign = np.zeros(N, dtype=np.int64)
    out.comp_cluster_off = []
    multi = [H for H in comps if len(H.info["orig_idx"]) > 1]
    if len(multi) > 4 and batched and coarsening_method not in coarsening.RANDOM_METHODS:
        # many components (Cora: 78, CiteSeer: 438): ONE batched contraction instead of a device round trip per component
        # (same per-component prelude, same kernels with one wavefront per component: identical partitions)
        idxs = [np.asarray(H.info["orig_idx"], dtype=np.int64) for H in multi]
        perm = np.concatenate(idxs)
        comp_off = np.concatenate([[0], np.cumsum([len(i) for i in idxs])])
        bc = coarsening.coarsen_batch(W[perm][:, perm], comp_off, r=coarsening_ratio, device=device, method=coarsening_method)
        per = {}
        for c, (H, idx) in enumerate(zip(multi, idxs)):
            b, e, cb, ce = int(comp_off[c]), int(comp_off[c + 1]), int(bc.cluster_off[c]), int(bc.cluster_off[c + 1])
            C = coarsening.CoarseningMatrix(sp.csc_matrix((bc.cval[b:e], (bc.assign[b:e] - cb, np.arange(e - b))), shape=(ce - cb, e - b)))
            per[id(H)] = (C, coarsening.Graph(bc.Wc[cb:ce, cb:ce].tocsr()))
    else:
        per = None
    off = 0
    for H in comps:
        idx = np.asarray(H.info["orig_idx"], dtype=np.int64)
        out.comp_cluster_off.append(off)
        if len(idx) > 1:
            if per is not None:
                C, Gc = per[id(H)]
            else:
                C, Gc, maps = coarsening.coarsen(H, r=coarsening_ratio, method=coarsening_method, device=device)
            a = sp.csc_matrix(C).indices.astype(np.int64)  # composed mapping dicts == row of C's single entry (== :167-180)
            assign[idx] = off + a
            off += C.shape[0]
            out.all_C.append(C); out.all_Gc.append(Gc)
            if len(idx) > 10:
                out.C_list.append(C); out.Gc_list.append(Gc)
        else:
            assign[idx] = off
            off += 1
            out.all_C.append(None); out.all_Gc.append(None)
    out.assign, out.n_clusters = assign, off
    return out


def dist_world():
    """(rank, world) of the initialised default process group, (0, 1) without one."""
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank(), torch.distributed.get_world_size()
    return 0, 1


def build_gs(args, data, co, device="cuda", float_targets=False, shard=None):
    """Subgraphs Gs (utils.py:186-267) + their masks (utils.py:683-703) as one block-diagonal SubgraphBatch.
    shard = (rank, world): keep only this rank's whole subgraphs of the union (data.shard_clusters: LPT over nnz';
    SURVEY §8e -- no edge crosses subgraphs, utils.py:248, and GD mode sums ONE loss over all of them, run.py:184-204)."""
    N, n = data.num_nodes, co.n_clusters
    x, y = data.x, data.y.flatten()
    masks = [data.train_mask, data.val_mask, data.test_mask]
    if getattr(args, "cluster_node", False):
        # new nodes carry the pooled features C.X of the neighbouring cluster (utils.py:160-161, :209), label 0, no mask
        Xc = torch.zeros((n, x.shape[1]), dtype=torch.float32)
        rows, cols = [], []
        for H, C, Gc, off in zip(co.components, co.all_C, co.all_Gc, co.comp_cluster_off):
            if C is None:
                continue
            idx = torch.as_tensor(np.asarray(H.info["orig_idx"], dtype=np.int64))
            Xc[off:off + C.shape[0]] = C.pool(x[idx].to(device)).cpu()
            coo = Gc.W.tocoo()
            rows.append(coo.row.astype(np.int64) + off); cols.append(coo.col.astype(np.int64) + off)
        r = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        c = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
        adj = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
        sub = fdata.assemble_subgraphs_cluster(data.edge_index, N, co.assign, n, adj)
        x = torch.cat([x.float(), Xc])
        y = torch.cat([y, torch.zeros(n, dtype=y.dtype)])
        masks = [torch.cat([m, torch.zeros(n, dtype=torch.bool)]) for m in masks]
    else:
        ei_dev = torch.as_tensor(np.asarray(data.edge_index)).to(device)
        # rows of a subgraph laid out star by star (an internal choice: per-node results do not depend on it; data.py)
        sub = fdata.assemble_subgraphs_torch(ei_dev, N, co.assign, n, extra_node=bool(getattr(args, "extra_node", False)),
                                             layout="star")
    if shard is not None and shard[1] > 1:
        owner = fdata.shard_clusters(None, fdata.cluster_nnz(sub), shard[1])   # the same on every rank
        sub = fdata.select_clusters(sub, np.nonzero(owner == shard[0])[0])
    batch = fdata.SubgraphBatch(sub, x, y, masks[0], device=device, float_targets=float_targets)
    core = batch.core
    batch.val_idx = torch.nonzero(masks[1].to(device)[batch.node_id] & core).flatten()
    batch.test_idx = torch.nonzero(masks[2].to(device)[batch.node_id] & core).flatten()
    return batch


def build_gc(args, data, co, device="cuda"):
    """The coarsened graph Gc of load_data_classification (utils.py:705-775): per component with > 10 nodes that holds
    train/val nodes: features C.X, label = argmax of pooled one-hot train (val) labels, mask = cluster holds labelled
    nodes of exactly one class, edges of Gc.W; smaller such components pass through uncoarsened."""
    n_classes = args.num_classes
    xs, tr_lab, tr_mask, va_lab, va_mask, rows, cols = [], [], [], [], [], [], []
    off, k_big = 0, 0
    y = data.y.flatten()
    onehot = torch.eye(n_classes)
    for H in co.components:
        idx = torch.as_tensor(np.asarray(H.info["orig_idx"], dtype=np.int64))
        big = len(idx) > 10
        C = Gc = None
        if big:
            C, Gc = co.C_list[k_big], co.Gc_list[k_big]  # utils.py:723-724: indexed by rank among big components
            k_big += 1
        tm, vm = data.train_mask[idx], data.val_mask[idx]
        if int(tm.sum()) + int(vm.sum()) == 0:
            continue
        if big:
            Xc = C.pool(data.x[idx].to(device)).cpu()
            tl = onehot[y[idx]].clone(); tl[~tm] = 0
            vl = onehot[y[idx]].clone(); vl[~vm] = 0
            ptl, pvl = torch.from_numpy(C.dot(tl.numpy())), torch.from_numpy(C.dot(vl.numpy()))
            for pooled, labs, masks in ((ptl, tr_lab, tr_mask), (pvl, va_lab, va_mask)):
                m = pooled.sum(1) > 0
                m &= ~((pooled > 0).sum(1) > 1)  # clusters mixing classes are not train (val) nodes (:728-730)
                labs.append(pooled.argmax(1))
                masks.append(m)
            coo = Gc.W.tocoo()
            n_c = Gc.N
        else:
            if not rows:
                raise Exception("The graph does not need coarsening.")  # utils.py:763
            Xc = data.x[idx]
            tr_lab.append(y[idx]); va_lab.append(y[idx]); tr_mask.append(tm); va_mask.append(vm)
            coo = H.W.tocoo()
            n_c = len(idx)
        xs.append(Xc.float())
        rows.append(coo.row.astype(np.int64) + off); cols.append(coo.col.astype(np.int64) + off)
        off += n_c
    gc = type("Gc", (), {})()
    gc.x = torch.cat(xs).to(device)
    if getattr(args, "normalize_features", False):
        gc.x = F.normalize(gc.x, p=1)  # run.py:334-335
    gc.edge_index = torch.from_numpy(np.stack([np.concatenate(rows), np.concatenate(cols)])).to(device)
    gc.train_labels, gc.val_labels = torch.cat(tr_lab).long().to(device), torch.cat(va_lab).long().to(device)
    gc.train_idx = torch.nonzero(torch.cat(tr_mask)).flatten().to(device)
    gc.val_idx = torch.nonzero(torch.cat(va_mask)).flatten().to(device)
    return gc


def _nll(model, x, ei, idx, labels, reduction):
    out = model(x, ei)
    return F.nll_loss(out.index_select(0, idx), labels.index_select(0, idx) if labels.numel() != idx.numel() else labels,
                      reduction=reduction), out


@torch.no_grad()
def infer_gs(model, batch, idx, reduction="mean"):
    """node_infer_Gs_GD (run.py:49-115): loss, accuracy and forward wall time over the subgraphs.  Under an initialised
    process group `batch` is this rank's shard: loss sums, hit counts and node counts are all-reduced, so every rank returns
    the figures of the whole union."""
    model.eval()
    torch.cuda.synchronize()
    t0 = time.time()
    out = model(batch.x, batch.edge_index)
    torch.cuda.synchronize()
    dt = time.time() - t0
    sel, y = out.index_select(0, idx), batch.y.index_select(0, idx)
    tot = torch.stack([F.nll_loss(sel, y, reduction="sum").double(), (sel.argmax(1) == y).sum().double(),
                       torch.tensor(float(idx.numel()), dtype=torch.float64, device=sel.device)])
    if dist_world()[1] > 1:
        torch.distributed.all_reduce(tot)
    n = max(float(tot[2]), 1.0)
    return float(tot[0]) / n, float(tot[1]) / n, dt


def _keep(model, ckpt, rank):
    """Best-val checkpoint (run.py:386-388): kept in memory on every rank (the validation loss is global, so all ranks keep
    the same epoch), written to `ckpt` by rank 0."""
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if rank == 0:
        torch.save(sd, ckpt)
    return sd


def node_classification(args, path, data, co, device="cuda", log=print):
    """run.node_classification (run.py:329-506) for exp_setup in {Gc_train_2_Gs_infer, Gs_train_2_Gs_infer,
    Gc_train_2_Gs_train}, gradient_method GD (one step per epoch over the union) or MB (one step per loader batch)."""
    if args.gradient_method not in ("GD", "MB"):
        raise ValueError(f"--gradient_method {args.gradient_method}: GD or MB")
    rank, world = dist_world()
    if world > 1 and args.gradient_method != "GD" and args.exp_setup != "Gc_train_2_Gs_infer":
        raise ValueError("--gradient_method MB steps once per loader batch, each step on the weights the previous batch left "
                         "(run.py:217-252): sequential by construction, single GPU only.  Data parallel runs use GD "
                         "(one loss over all subgraphs, run.py:184-204).")
    rng = np.random.default_rng(args.seed)
    data = splits_classification(data, args.num_classes, args.experiment, rng)
    # data parallel: every rank holds a shard of the ONE subgraph union; the Gc phase (one small graph) is
    # replicated -- same seeds, same data, same weights on every rank
    batch = build_gs(args, data, co, device, shard=(rank, world))
    gc = build_gc(args, data, co, device) if args.exp_setup != "Gs_train_2_Gs_infer" else None
    all_loss, all_acc, all_time = [], [], []
    ckpt = os.path.join(path, "model.pt")
    for run in range(args.runs):
        if args.seed is not None:
            torch.manual_seed(args.seed + run)
        model = network.Classify_node(args).to(device)
        model.reset_parameters()
        if world > 1:   # the replicated Gc phase and the all-reduced Gs phase both assume ONE set of weights
            broadcast_parameters(model)
        opt = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
        if args.exp_setup in ("Gc_train_2_Gs_infer", "Gc_train_2_Gs_train"):
            best = float("inf")
            for epoch in range(args.epochs1):  # node_train_Gc / node_val_Gc (run.py:26-47)
                model.train()
                opt.zero_grad()
                out = model(gc.x, gc.edge_index)
                loss = F.nll_loss(out.index_select(0, gc.train_idx), gc.train_labels.index_select(0, gc.train_idx),
                                  reduction=args.loss_reduction)
                loss.backward()
                opt.step()
                model.eval()
                with torch.no_grad():
                    out = model(gc.x, gc.edge_index)
                    vloss = float(F.nll_loss(out.index_select(0, gc.val_idx), gc.val_labels.index_select(0, gc.val_idx),
                                             reduction=args.loss_reduction))
                if vloss < best or epoch == 0:
                    best = vloss
                    best_sd = _keep(model, ckpt, rank)
            model.load_state_dict(best_sd)
            # drop the last epoch's autograd graph: while `loss` lives, the parameters' AccumulateGrad nodes stay bound to the stream
            # this phase ran on, and a trainer that captures its step on another stream would fork that stream into the capture
            # (train._accumulate_stream_guard detects it and falls back to eager steps; without the reference it does not arise)
            loss = out = None
        if args.exp_setup in ("Gs_train_2_Gs_infer", "Gc_train_2_Gs_train"):
            if args.gradient_method == "GD":
                # the extra nodes' last-layer outputs never reach the loss: evaluate that layer on the own nodes only
                trainer = GDTrainer(model, batch, lr=args.lr, weight_decay=args.weight_decay, reduction=args.loss_reduction,
                                    prune_unused_rows=True)
            else:
                trainer = MBTrainer(model, batch, batch_size=args.batch_size, lr=args.lr, weight_decay=args.weight_decay,
                                    reduction=args.loss_reduction, capture=True)  # launch-bound: replayed from hipGraphs
            if args.exp_setup == "Gc_train_2_Gs_train":
                trainer.opt.load_state_dict(opt.state_dict())  # the reference keeps ONE optimizer across both phases
            best = float("inf")
            for epoch in range(args.epochs2):
                trainer.step()
                vloss, vacc, _ = infer_gs(model, batch, batch.val_idx)
                if vloss < best or epoch == 0:
                    best = vloss
                    best_sd = _keep(model, ckpt, rank)
            model.load_state_dict(best_sd)
        tloss, tacc, ttime = infer_gs(model, batch, batch.test_idx)
        log(f"run {run + 1}: test_loss {tloss:.4f} test_acc {tacc:.4f} infer_time {ttime * 1e3:.2f} ms")
        all_loss.append(tloss); all_acc.append(tacc); all_time.append(ttime)
    return all_loss, all_acc, all_time


def node_classification_baseline(args, path, data, device="cuda", log=print):
    """run.node_classification_baseline (run.py:832-902): the 2-layer model on the full graph."""
    rng = np.random.default_rng(args.seed)
    data = splits_classification(data, args.num_classes, args.experiment, rng)
    x = data.x.to(device).float()
    ei = torch.as_tensor(np.asarray(data.edge_index)).to(device)
    y = data.y.flatten().to(device)
    tr, va, te = (torch.nonzero(m.to(device)).flatten() for m in (data.train_mask, data.val_mask, data.test_mask))
    all_loss, all_acc, all_time = [], [], []
    ckpt = os.path.join(path, "model.pt")
    for run in range(args.runs):
        if args.seed is not None:
            torch.manual_seed(args.seed + run)
        model = network.Classify_node(args).to(device)
        model.reset_parameters()
        opt = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
        best = float("inf")
        for epoch in range(args.epochs1):
            model.train()
            opt.zero_grad()
            out = model(x, ei)
            F.nll_loss(out.index_select(0, tr), y.index_select(0, tr), reduction=args.loss_reduction).backward()
            opt.step()
            model.eval()
            with torch.no_grad():
                out = model(x, ei)
                vloss = float(F.nll_loss(out.index_select(0, va), y.index_select(0, va), reduction=args.loss_reduction))
            if vloss < best or epoch == 0:
                best = vloss
                torch.save(model.state_dict(), ckpt)
        model.load_state_dict(torch.load(ckpt))
        model.eval()
        with torch.no_grad():
            torch.cuda.synchronize()
            t0 = time.time()
            out = model(x, ei)
            torch.cuda.synchronize()
            dt = time.time() - t0
            sel = out.index_select(0, te)
            tloss = float(F.nll_loss(sel, y.index_select(0, te)))
            tacc = float((sel.argmax(1) == y.index_select(0, te)).float().mean())
        log(f"run {run + 1}: test_loss {tloss:.4f} test_acc {tacc:.4f} infer_time {dt * 1e3:.2f} ms")
        all_loss.append(tloss); all_acc.append(tacc); all_time.append(dt)
    return all_loss, all_acc, all_time


def graph_method(args):
    """--coarsening_method for a graph-level task: variation_neighborhoods or a deterministic / in-order matching method
    (graph_data.GRAPH_MATCHING_METHODS); affinity_GS is refused as in coarsening_classification."""
    from . import graph_data

    m = getattr(args, "coarsening_method", "variation_neighborhoods")
    if m == "affinity_GS":
        raise NotImplementedError("affinity_GS is supported by coarsening.coarsen() but not by the pipeline (see "
                                  "coarsening_classification)")
    if m != "variation_neighborhoods" and m not in graph_data.GRAPH_MATCHING_METHODS:
        raise NotImplementedError(f"graph-level tasks coarsen with variation_neighborhoods, {', '.join(graph_data.GRAPH_MATCHING_METHODS)}; "
                                  f"not '{m}'")
    return m


def graph_regression(args, path, mol, device="cuda", log=print):
    """run.graph_regression (run.py:707-830) / run.graph_classification (run.py:575-706) on a graph_data.GraphSet:
    50/25/25 split of a random permutation (utils.py:23-39), {Regress,Classify}_graph_gc / _gs, L1 / cross-entropy
    loss, the four exp_setups, best-val checkpoint, and the reference's results row.  Returns best_test_loss
    (graph_cls: (best_test_loss, best_test_acc))."""
    from . import graph_data
    from .train import GraphTrainer

    gset = graph_data.GraphSet(mol, ratio=args.coarsening_ratio, extra_node=bool(args.extra_node), device=device,
                               cluster_node=bool(args.cluster_node), method=graph_method(args))
    G = gset.n_graphs
    gen = torch.Generator().manual_seed(0 if args.seed is None else args.seed)
    idx = torch.randperm(G, generator=gen).tolist()
    split = {"train": idx[: G // 2], "val": idx[G // 2: 3 * G // 4], "test": idx[3 * G // 4:]}
    cls_task = args.task == "graph_cls"
    if cls_task:
        model_gc, model_gs = network.Classify_graph_gc(args).to(device), network.Classify_graph_gs(args).to(device)
    else:
        args.num_classes = 1
        model_gc, model_gs = network.Regress_graph_gc(args).to(device), network.Regress_graph_gs(args).to(device)
    kw = dict(batch_size=args.batch_size, lr=args.lr, weight_decay=args.weight_decay, multi_prop=bool(args.multi_prop),
              prop=args.property, capture=True, task=args.task,   # launch-bound batch steps: replayed from hipGraphs
              truncate_targets=True)
    T = {}
    for m in ("gc", "gs"):   # one optimiser per model across all phases (run.py:718-719)
        model = model_gc if m == "gc" else model_gs
        # the training loaders reshuffle every epoch (run.py:710 shuffle=True) where that replays one captured step ("auto")
        T[(m, "train")] = GraphTrainer(model, gset, split["train"], kind=m, reshuffle="auto", **kw)
        for s in ("val", "test"):
            T[(m, s)] = GraphTrainer(model, gset, split[s], kind=m, share=T[(m, "train")], **kw)
    ckpt = os.path.join(path, "model.pt")
    best_val, best_test, best_acc = float("inf"), float("inf"), 0.0
    setup = args.exp_setup

    def consider(epoch, val, test, model):
        nonlocal best_val, best_test, best_acc
        if val < best_val or epoch == 0:
            best_val, best_test = val, test
            if cls_task and np.isfinite(test):
                best_acc = T[("gc" if model is model_gc and setup == "Gc_train_2_Gc_infer" else "gs", "test")].accuracy()
            torch.save(model.state_dict(), ckpt)

    if setup in ("Gc_train_2_Gs_train", "Gc_train_2_Gc_infer", "Gc_train_2_Gs_infer"):
        for epoch in range(args.epochs1):
            T[("gc", "train")].step()
            v = float(T[("gc", "val")].evaluate())
            if setup == "Gc_train_2_Gc_infer":
                consider(epoch, v, float(T[("gc", "test")].evaluate()), model_gc)
            elif setup == "Gc_train_2_Gs_infer":   # the Gs model is never loaded with the Gc weights here (run.py:769-784)
                consider(epoch, v, float(T[("gs", "test")].evaluate()), model_gc)
            else:
                consider(epoch, v, float("inf"), model_gc)
    if setup == "Gc_train_2_Gs_train":
        model_gs.load_state_dict(torch.load(ckpt))
        best_val = float("inf")
    if setup in ("Gc_train_2_Gs_train", "Gs_train_2_Gs_infer"):
        for epoch in range(args.epochs2):
            T[("gs", "train")].step()
            consider(epoch, float(T[("gs", "val")].evaluate()), float(T[("gs", "test")].evaluate()), model_gs)
    os.makedirs("results", exist_ok=True)
    fn = f"results/{args.dataset}.csv"
    if not os.path.exists(fn):
        with open(fn, "w") as f:
            f.write("dataset,coarsening_method,coarsening_ratio,exp_setup,layer_name,extra_nodes,cluster_node,community_used,hidden,"
                    "num_layers1,num_layers2,epochs1,epochs2,batch_size,lr,best_test_loss"
                    + (",best_test_acc" if cls_task else (",property_idx}" if args.multi_prop else "")) + "\n")
    tail = f",{best_acc}" if cls_task else (f",{args.property}" if args.multi_prop else "")
    with open(fn, "a") as f:
        f.write(f"{args.dataset},{args.coarsening_method},{args.coarsening_ratio},{args.exp_setup},{args.layer_name},{args.extra_node},"
                f"{args.cluster_node},{args.use_community_detection},{args.hidden},{args.num_layers1},{args.num_layers2},{args.epochs1},"
                f"{args.epochs2},{args.batch_size},{args.lr},{best_test}" + tail + "\n")
    log(f"best_test_loss: {best_test}" + (f"  best_test_acc: {best_acc}" if cls_task else ""))
    return (best_test, best_acc) if cls_task else best_test


# ---------------------------------------------------------------------------------------------
# node regression (chameleon / squirrel / crocodile shaped): run.node_regression, run.py:508-573
# ---------------------------------------------------------------------------------------------
SYNTHETIC_REG_SHAPES = {  # name: (N, E, F)   dataset_info.csv:8-10
    "synthetic-chameleon": (2277, 31396, 128),
    "synthetic-squirrel": (5201, 198423, 128),
    "synthetic-crocodile": (11631, 170845, 128),
}


def synthetic_regression_dataset(name, seed=0):
    """Seeded stand-in of a WikipediaNetwork node-regression dataset's shape (geom_gcn_preprocess=False: the target is
    the log of the page traffic, a float per node): target = a linear readout of the features averaged over the closed
    neighbourhood (what one propagation step can represent) plus noise."""
    N, E, Fdim = SYNTHETIC_REG_SHAPES[name]
    rng = np.random.default_rng(seed)
    ei = fdata.synthetic_graph(N, E, seed=seed)
    W = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(N, N))
    x = rng.standard_normal((N, Fdim)).astype(np.float32)
    deg = np.asarray(W.sum(1)).ravel()
    z = x[:, :16] @ rng.standard_normal(16)                            # a linear readout of the features ...
    z = (z + np.asarray(W @ z).ravel()) / (deg + 1)                # ... averaged over the closed neighbourhood
    y = (2.0 + 3.0 * (z - z.mean()) / z.std() + 0.1 * rng.standard_normal(N)).astype(np.float32)
    return NodeData(torch.from_numpy(x), ei, torch.from_numpy(y), None, None, None)


def splits_regression(data, train_ratio, val_ratio, rng):
    """utils.py:645-659: random node permutation cut at train_ratio / train_ratio + val_ratio."""
    if train_ratio + val_ratio >= 1:
        raise ValueError("train_ratio + val_ratio should be less than 1")
    N = data.x.shape[0]
    perm = torch.from_numpy(rng.permutation(N))
    n_tr, n_va = int(train_ratio * N), int(val_ratio * N)
    masks = []
    for idx in (perm[:n_tr], perm[n_tr:n_tr + n_va], perm[n_tr + n_va:]):
        m = torch.zeros(N, dtype=torch.bool)
        m[idx] = True
        masks.append(m)
    data.train_mask, data.val_mask, data.test_mask = masks
    return data


@torch.no_grad()
def infer_gs_regression(model, batch, idx):
    """node_infer_Gs_GD for node_reg (run.py:106-115): L1 over the selected nodes divided by the std of their labels."""
    model.eval()
    torch.cuda.synchronize()
    t0 = time.time()
    out = model(batch.x, batch.edge_index)
    torch.cuda.synchronize()
    dt = time.time() - t0
    sel, y = out.index_select(0, idx).flatten(), batch.y.index_select(0, idx).flatten()
    return float(F.l1_loss(sel, y) / y.std(unbiased=False)), 0.0, dt


def node_regression(args, path, data, co, device="cuda", log=print):
    """run.node_regression (run.py:508-573): Regress_node trained on Gs only (GD or MB), L1 loss, best-val checkpoint."""
    rng = np.random.default_rng(args.seed)
    data = splits_regression(data, args.train_ratio, args.val_ratio, rng)
    batch = build_gs(args, data, co, device, float_targets=True)   # plain / --extra_node / --cluster_node subgraphs
    all_loss, all_time = [], []
    ckpt = os.path.join(path, "model.pt")
    args.num_classes = 1
    for run in range(args.runs):
        if args.seed is not None:
            torch.manual_seed(args.seed + run)
        model = network.Regress_node(args).to(device)
        model.reset_parameters()
        if args.gradient_method == "GD":
            trainer = GDTrainer(model, batch, lr=args.lr, weight_decay=args.weight_decay, reduction=args.loss_reduction, task="node_reg")
        else:
            raise NotImplementedError("node regression: --gradient_method GD only")
        best = float("inf")
        for epoch in range(args.epochs2):
            trainer.step()
            vloss, _, _ = infer_gs_regression(model, batch, batch.val_idx)
            if vloss < best or epoch == 0:
                best = vloss
                torch.save(model.state_dict(), ckpt)
        model.load_state_dict(torch.load(ckpt))
        tloss, _, ttime = infer_gs_regression(model, batch, batch.test_idx)
        log(f"run {run + 1}: test_loss {tloss:.4f} infer_time {ttime * 1e3:.2f} ms")
        all_loss.append(tloss); all_time.append(ttime)
    top = sorted(all_loss)[:10]
    os.makedirs("results", exist_ok=True)
    fn = f"results/{args.dataset}.csv"
    if not os.path.exists(fn):
        with open(fn, "w") as f:
            f.write("dataset,coarsening_method,coarsening_ratio,layer_name,extra_nodes,cluster_node,community_used,hidden,runs,num_layers,"
                    "batch_size,lr,ave_time,top_10_loss,best_loss\n")
    with open(fn, "a") as f:
        f.write(f"{args.dataset},{args.coarsening_method},{args.coarsening_ratio},{args.layer_name},{args.extra_node},{args.cluster_node},"
                f"{args.use_community_detection},{args.hidden},{args.runs},{args.num_layers1},{args.batch_size},{args.lr},{np.mean(all_time)},"
                f"{np.mean(top)} +/- {np.std(top)},{top[0]}\n")
    log(f"top_10_loss: {np.mean(top)} +/- {np.std(top)}  best_loss: {top[0]}")
    return all_loss, all_time


def graph_baseline(args, path, mol, device="cuda", log=print):
    """run.graph_regression_baseline / graph_classification_baseline (run.py:967-1100): the *_graph_gc model on the
    UNCOARSENED graphs, gradients cleared per batch, float targets, best-val checkpoint, results/baseline row."""
    from . import graph_data
    from .train import GraphTrainer

    cls_task = args.task == "graph_cls"
    gset = graph_data.GraphSet(mol, ratio=0.5, extra_node=False, device=device)   # the contraction is unused here
    G = gset.n_graphs
    gen = torch.Generator().manual_seed(0 if args.seed is None else args.seed)
    idx = torch.randperm(G, generator=gen).tolist()
    split = {"train": idx[: G // 2], "val": idx[G // 2: 3 * G // 4], "test": idx[3 * G // 4:]}
    if not cls_task:
        args.num_classes = 1
    model = (network.Classify_graph_gc if cls_task else network.Regress_graph_gc)(args).to(device)
    kw = dict(kind="orig", batch_size=args.batch_size, lr=args.lr, weight_decay=args.weight_decay, multi_prop=bool(args.multi_prop),
              prop=args.property, task=args.task, truncate_targets=False, accumulate=False, capture=True)
    tr = GraphTrainer(model, gset, split["train"], **kw)
    va, te = (GraphTrainer(model, gset, split[s], share=tr, **kw) for s in ("val", "test"))
    ckpt = os.path.join(path, "model.pt")
    best_val, best_test, best_acc = float("inf"), float("inf"), 0.0
    for epoch in range(args.epochs1):
        tr.step()
        v, t = float(va.evaluate()), float(te.evaluate())
        if v < best_val or epoch == 0:
            best_val, best_test = v, t
            best_acc = te.accuracy() if cls_task else 0.0
            torch.save(model.state_dict(), ckpt)
    os.makedirs("results/baseline", exist_ok=True)
    fn = f"results/baseline/{args.dataset}.csv"
    if not os.path.exists(fn):
        with open(fn, "w") as f:
            f.write("dataset,layer_name,hidden,num_layers,epochs,batch_size,lr,best_test_loss" + (",best_test_acc" if cls_task else "") + "\n")
    with open(fn, "a") as f:
        f.write(f"{args.dataset},{args.layer_name},{args.hidden},{args.num_layers1},{args.epochs1},{args.batch_size},{args.lr},{best_test}"
                + (f",{best_acc}" if cls_task else "") + "\n")
    log(f"baseline best_test_loss: {best_test}" + (f"  best_test_acc: {best_acc}" if cls_task else ""))
    return (best_test, best_acc) if cls_task else best_test


def node_regression_baseline(args, path, data, device="cuda", log=print):
    """run.node_regression_baseline (run.py:904-965): Regress_node on the full graph, L1 loss, test loss / std(labels)."""
    rng = np.random.default_rng(args.seed)
    data = splits_regression(data, args.train_ratio, args.val_ratio, rng)
    x = data.x.to(device).float()
    ei = torch.as_tensor(np.asarray(data.edge_index)).to(device)
    y = data.y.flatten().to(device).float()
    tr, va, te = (torch.nonzero(m.to(device)).flatten() for m in (data.train_mask, data.val_mask, data.test_mask))
    args.num_classes = 1
    all_loss, all_time = [], []
    ckpt = os.path.join(path, "model.pt")
    for run in range(args.runs):
        if args.seed is not None:
            torch.manual_seed(args.seed + run)
        model = network.Regress_node(args).to(device)
        model.reset_parameters()
        opt = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
        best = float("inf")
        for epoch in range(args.epochs1):
            model.train()
            opt.zero_grad()
            out = model(x, ei).flatten()
            F.l1_loss(out.index_select(0, tr), y.index_select(0, tr), reduction=args.loss_reduction).backward()
            opt.step()
            model.eval()
            with torch.no_grad():
                vloss = float(F.l1_loss(model(x, ei).flatten().index_select(0, va), y.index_select(0, va), reduction=args.loss_reduction))
            if vloss < best or epoch == 0:
                best = vloss
                torch.save(model.state_dict(), ckpt)
        model.load_state_dict(torch.load(ckpt))
        model.eval()
        with torch.no_grad():
            torch.cuda.synchronize()
            t0 = time.time()
            out = model(x, ei).flatten()
            torch.cuda.synchronize()
            dt = time.time() - t0
            yt = y.index_select(0, te)
            tloss = float(F.l1_loss(out.index_select(0, te), yt) / yt.std())
        log(f"run {run + 1}: test_loss {tloss:.4f} infer_time {dt * 1e3:.2f} ms")
        all_loss.append(tloss); all_time.append(dt)
    top = sorted(all_loss)[:10]
    os.makedirs("results/baseline", exist_ok=True)
    fn = f"results/baseline/{args.dataset}.csv"
    if not os.path.exists(fn):
        with open(fn, "w") as f:
            f.write("dataset,experiment,layer_name,runs,num_layers,batch_size,lr,ave_time,top_10_loss,best_loss\n")
    with open(fn, "a") as f:
        f.write(f"{args.dataset},{args.experiment},{args.layer_name},{args.runs},{args.num_layers1},{args.batch_size},{args.lr},"
                f"{np.mean(all_time)},{np.mean(top)} +/- {np.std(top)},{top[0]}\n")
    return all_loss, all_time


# ---------------------------------------------------------------------------------------------
# --use_community_detection (main.py:247-267): keep the largest communities up to k nodes
# ---------------------------------------------------------------------------------------------
def detect_communities(edge_index, num_nodes, seed=0, iters=20, method="label_propagation"):
    """A node partition for --use_community_detection.  The reference calls leidenalg.find_partition(...,
    ModularityVertexPartition) on an igraph Graph (main.py:257-258); neither package exists here, and only the partition
    is consumed downstream.  method="label_propagation" (the default) is a substitute on the CPU: seeded label propagation
    (every node repeatedly adopts the most frequent label among its neighbours, ties to the smallest label, half of the
    nodes per sweep), vectorised with sort-based modes.  method="modularity" optimises what the reference optimises, on the
    GPU: community.modularity_communities (deterministic; seed and iters do not apply).  Returns int64 labels in
    0..n_comm-1."""
    if method == "modularity":
        from . import community
        return community.modularity_communities(edge_index, num_nodes)
    if method != "label_propagation":
        raise ValueError(f"detect_communities: unknown method {method!r} (label_propagation or modularity)")
    ei = np.asarray(edge_index)
    src, dst = ei[0].astype(np.int64), ei[1].astype(np.int64)
    N = int(num_nodes)
    rng = np.random.default_rng(seed)
    label = np.arange(N, dtype=np.int64)
    for it in range(iters):
        lab_src = label[src]
        order = np.lexsort((lab_src, dst))
        d, l = dst[order], lab_src[order]
        start = np.concatenate([[True], (d[1:] != d[:-1]) | (l[1:] != l[:-1])])
        run_id = np.cumsum(start) - 1
        cnt = np.bincount(run_id)
        rd, rl = d[start], l[start]
        best = np.lexsort((rl, -cnt, rd))              # per node: highest count, then smallest label
        first = np.concatenate([[True], rd[best][1:] != rd[best][:-1]])
        nodes, new = rd[best][first], rl[best][first]
        move = rng.random(len(nodes)) < 0.5            # half of the nodes per sweep: damps the oscillation of synchronous updates
        changed = int((label[nodes[move]] != new[move]).sum())
        label[nodes[move]] = new[move]
        if changed == 0 and it > 2:
            break
    _, label = np.unique(label, return_inverse=True)
    return label.astype(np.int64)


def merge_communities(data, labels, k):
    """utils.merge_communities (utils.py:132-141): communities largest first, taken whole while the node total stays <= k;
    the dataset becomes the subgraph induced by those nodes (renumbered in that order)."""
    sizes = np.bincount(labels)
    order = np.argsort(-sizes, kind="stable")
    keep, total = [], 0
    for c in order:
        if total + sizes[c] <= k:
            keep.append(np.nonzero(labels == c)[0])
            total += int(sizes[c])
            if total == k:
                break
    nodes = np.concatenate(keep) if keep else np.zeros(0, dtype=np.int64)
    new_id = np.full(data.num_nodes, -1, dtype=np.int64)
    new_id[nodes] = np.arange(len(nodes))
    ei = np.asarray(data.edge_index)
    m = (new_id[ei[0]] >= 0) & (new_id[ei[1]] >= 0)
    t = torch.from_numpy(nodes)
    return NodeData(data.x[t], np.stack([new_id[ei[0][m]], new_id[ei[1][m]]]), data.y[t], data.train_mask[t], data.val_mask[t],
                    data.test_mask[t])
