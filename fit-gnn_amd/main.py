#!/usr/bin/env python3
"""main.py -- FIT-GNN's training command line on the MI355X implementation.

Same flags, defaults and `store_true` semantics as the reference's main.py:176-208, same post-parse corrections
(arg_correction, main.py:117-129), same outputs: best-val `model.pt` under save/<task>/[baseline/]<output_dir>/ and a
row appended to results/<dataset>.csv (results/baseline/<dataset>.csv) with the reference's columns
(run.py:480-485, :883-887).  Tasks: node classification (GD / MB, all exp_setups), node regression, graph regression and
graph classification, each with its --baseline; datasets below.

Datasets: the reference downloads through torch_geometric / ogb, which are not available here.  Accepted:
  synthetic-{chameleon,squirrel,crocodile}   node-regression stand-ins (dataset_info.csv:8-10)
  synthetic-proteins         PROTEINS-shaped graph classification stand-in (--n_graphs graphs, 2 classes)
  synthetic-qm9              QM9-shaped graph regression stand-in (--n_graphs molecules of ~18 nodes, 19 targets)
  cora | citeseer | pubmed   Planetoid raw files `ind.<name>.*` under --data_root/<name>/raw (PyG's own layout)
  synthetic-{cora,citeseer,pubmed,physics}   seeded stand-ins of the same shape (dataset_info.csv)
Extra flags (not in the reference): --data_root, --device, --community_nodes, --community_method, --n_graphs, --dropout.

Data parallel (BASELINE.json config 4, "subgraph-batch DP on 8 x MI355X"; new functionality): launch one
process per GPU, e.g. `python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 main.py
--dataset ... --train_fitgnn --gradient_method GD`.  Rank 0 coarsens and broadcasts the partition; the subgraph union is
sharded by whole subgraphs (data.shard_clusters), gradients are all-reduced over RCCL once per GD step
(train.GDTrainer), validation / test figures are all-reduced sums; rank 0 writes model.pt and the results row.
MB mode is sequential by construction (run.py:217-252) and stays single-GPU.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402


# --coarsening_method values the node-level pipeline runs (coarsening.coarsen() also takes affinity_GS; the pipeline refuses it,
# pipeline.coarsening_classification).  Anything else fails here, at argument parsing: no method falls back to another.
COARSENING_METHODS = ('variation_neighborhoods', 'heavy_edge', 'algebraic_JC', 'variation_edges')


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--dataset', type=str, default='cora')
    p.add_argument('--experiment', type=str, default='fixed')
    p.add_argument('--runs', type=int, default=20)
    p.add_argument('--exp_setup', type=str, default='Gc_train_2_Gs_infer')
    p.add_argument('--hidden', type=int, default=512)
    p.add_argument('--layer_name', type=str, default='GCNConv')  # GCNConv, GATConv, SAGEConv, GINConv
    p.add_argument('--epochs1', type=int, default=100)
    p.add_argument('--epochs2', type=int, default=300)
    p.add_argument('--num_layers1', type=int, default=2)
    p.add_argument('--num_layers2', type=int, default=2)
    p.add_argument('--batch_size', type=int, default=128)
    p.add_argument('--train_ratio', type=float, default=0.3)
    p.add_argument('--val_ratio', type=float, default=0.2)
    p.add_argument('--early_stopping', type=int, default=10)
    p.add_argument('--extra_node', action='store_true')
    p.add_argument('--cluster_node', action='store_true')
    p.add_argument('--lr', type=float, default=0.01)
    p.add_argument('--weight_decay', type=float, default=0.0005)
    p.add_argument('--gradient_method', type=str, default='GD')
    p.add_argument('--use_community_detection', action='store_true')
    p.add_argument('--normalize_features', action='store_true')
    p.add_argument('--coarsening_ratio', type=float, default=0.5)
    p.add_argument('--coarsening_method', type=str, default='variation_neighborhoods', choices=COARSENING_METHODS)
    p.add_argument('--output_dir', type=str, required=True)
    p.add_argument('--task', type=str, default='node_cls')
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--multi_prop', action='store_true')
    p.add_argument('--loss_reduction', type=str, default='mean')
    p.add_argument('--property', type=int, default=0)
    p.add_argument('--train_fitgnn', action='store_true')
    p.add_argument('--run_intermediate_inference', action='store_true')
    p.add_argument('--intermediate_inference_freq', type=int, default=10)
    p.add_argument('--baseline', action='store_true')
    # not in the reference
    p.add_argument('--data_root', type=str, default='./dataset')
    p.add_argument('--device', type=str, default='cuda')
    p.add_argument('--community_nodes', type=int, default=165000)  # main.py:264 hard-codes 165000
    # modularity: community.modularity_communities on the GPU (what the reference's leidenalg call optimises); the default is the CPU substitute
    p.add_argument('--community_method', type=str, default='label_propagation', choices=['label_propagation', 'modularity'])
    p.add_argument('--n_graphs', type=int, default=2000)  # size of the synthetic-qm9 stand-in (QM9 itself: 130 831)
    p.add_argument('--dropout', type=float, default=0.5)  # the reference calls F.dropout with its default p = 0.5 (network.py:33)
    # attention heads of every --layer_name GATConv layer, each hidden / heads wide (the reference passes one head); other layers ignore it
    p.add_argument('--heads', type=int, default=1)
    return p


def arg_correction(args):
    """main.py:117-129."""
    if args.cluster_node:
        args.extra_node = False
    elif args.extra_node:
        args.cluster_node = False
    if args.experiment == 'fixed' and args.dataset in ('ogbn-products', 'dblp', 'Physics', 'WikiCS', 'Flickr'):
        args.experiment = 'random'
    if args.train_fitgnn:
        args.baseline = False
    if args.train_fitgnn is False:
        args.baseline = True
    return args


def process_dataset(args):
    from fitgnn_amd import pipeline

    name = args.dataset
    if name == 'synthetic-proteins':  # main.py:86-99: TU datasets are graph classification
        from fitgnn_amd import graph_data
        mol = graph_data.synthetic_graph_classes(args.n_graphs, seed=0 if args.seed is None else args.seed)
        args.task, args.multi_prop = 'graph_cls', False
        args.num_features, args.num_classes = mol["x"].shape[1], 2
        return mol, args
    if name == 'synthetic-qm9':  # QM9-shaped stand-in (main.py:105-108: task graph_reg, multi_prop forced on)
        from fitgnn_amd import graph_data
        mol = graph_data.synthetic_molecules(args.n_graphs, seed=0 if args.seed is None else args.seed)
        args.task, args.multi_prop = 'graph_reg', True
        args.num_features = mol["x"].shape[1]
        return mol, args
    if name in pipeline.SYNTHETIC_REG_SHAPES:  # main.py:71-85: WikipediaNetwork datasets are node regression
        data = pipeline.synthetic_regression_dataset(name, seed=0 if args.seed is None else args.seed)
        if args.normalize_features:
            data.x = torch.nn.functional.normalize(data.x, p=1)
        args.task, args.num_features, args.num_classes = 'node_reg', data.x.shape[1], 1
        return data, args
    if name in pipeline.SYNTHETIC_SHAPES:
        data, n_classes = pipeline.synthetic_dataset(name, seed=0 if args.seed is None else args.seed)
        if args.experiment == 'fixed':
            pass  # the generator already provides a 20-per-class / 500 / 1000 split
    elif name in ('cora', 'citeseer', 'pubmed'):
        root = os.path.join(args.data_root, name, 'raw')
        if not os.path.exists(os.path.join(root, f'ind.{name}.x')):
            raise FileNotFoundError(f"{root}/ind.{name}.* not found (no network access to download; point --data_root at a "
                                    f"directory holding <name>/raw, or use --dataset synthetic-{name})")
        data, n_classes = pipeline.load_planetoid(root, name)
    else:
        raise NotImplementedError(f"dataset '{name}' needs torch_geometric/ogb downloads, which this build does not have; "
                                  f"available: cora citeseer pubmed {' '.join(pipeline.SYNTHETIC_SHAPES)}")
    if args.normalize_features:
        data.x = torch.nn.functional.normalize(data.x, p=1)
    args.task = 'node_cls'
    args.num_features, args.num_classes = data.x.shape[1], n_classes
    return data, args


def write_results(args, all_loss, all_acc, all_time, baseline):
    top_acc = sorted(all_acc, reverse=True)[:10]
    top_loss = sorted(all_loss)[:10]
    os.makedirs('results/baseline', exist_ok=True)
    if baseline:
        fn = f"results/baseline/{args.dataset}.csv"
        header = 'dataset,experiment,layer_name,hidden,runs,num_layers,lr,ave_acc,ave_time,top_10_acc,best_acc,top_10_loss,best_loss\n'
        row = (f"{args.dataset},{args.experiment},{args.layer_name},{args.hidden},{args.runs},{args.num_layers1},{args.lr},"
               f"{np.mean(all_acc)} +/- {np.std(all_acc)},{np.mean(all_time)},{np.mean(top_acc)} +/- {np.std(top_acc)}, {top_acc[0]}, "
               f"{np.mean(top_loss)} +/- {np.std(top_loss)}, {top_loss[0]}\n")
    else:
        fn = f"results/{args.dataset}.csv"
        header = ('dataset,coarsening_method,coarsening_ratio,experiment,exp_setup,layer_name,extra_nodes,cluster_node,community_used,'
                  'hidden,runs,num_layers,batch_size,lr,ave_acc,ave_time,top_10_acc,best_acc,top_10_loss,best_loss\n')
        row = (f"{args.dataset},{args.coarsening_method},{args.coarsening_ratio},{args.experiment},{args.exp_setup},{args.layer_name},"
               f"{args.extra_node},{args.cluster_node},{args.use_community_detection},{args.hidden},{args.runs},{args.num_layers1},"
               f"{args.batch_size},{args.lr},{np.mean(all_acc)} +/- {np.std(all_acc)},{np.mean(all_time)},"
               f"{np.mean(top_acc)} +/- {np.std(top_acc)}, {top_acc[0]}, {np.mean(top_loss)} +/- {np.std(top_loss)}, {top_loss[0]}\n")
    if not os.path.exists(fn):
        with open(fn, 'w') as f:
            f.write(header)
    with open(fn, 'a') as f:
        f.write(row)
    tag = "BASELINE MODEL" if baseline else "FIT-GNN MODEL"
    print(f"############################### {tag} ###############################")
    for k in ("dataset", "experiment", "exp_setup", "layer_name", "hidden", "runs", "lr", "coarsening_ratio", "coarsening_method"):
        print(f"{k}: {getattr(args, k)}")
    print(f"ave_acc: {np.mean(all_acc)} +/- {np.std(all_acc)}")
    print(f"ave_time: {np.mean(all_time)}")
    print(f"best_acc: {top_acc[0]}")
    print(f"best_loss: {top_loss[0]}")
    print("#############################################################################")


def init_distributed(args):
    """One process per GPU under torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE in the environment): join the group
    (nccl = RCCL over xGMI; gloo when the box has fewer GPUs than ranks -- a rehearsal) and pin this rank's device.
    Returns (rank, world); (0, 1) when not launched that way."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0, 1
    rank, local = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    n_dev = torch.cuda.device_count()
    local %= max(n_dev, 1)
    torch.cuda.set_device(local)
    args.device = f"cuda:{local}"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    backend = os.environ.get("FITGNN_DIST_BACKEND", "nccl" if n_dev >= world else "gloo")
    if not torch.distributed.is_initialized():
        if backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=torch.device(args.device))
        else:
            torch.distributed.init_process_group(backend)
    return rank, world


def main(argv=None):
    args = build_parser().parse_args(argv)
    args = arg_correction(args)
    rank, world = init_distributed(args)
    if world > 1 and args.seed is None:
        # unseeded (the default, as in the reference): every rank would draw its own weights, splits and dropout seeds, while the
        # data-parallel step assumes ONE run replicated -- rank 0 draws the run's seed and every rank uses it
        box = [int(np.random.SeedSequence().generate_state(1)[0] % (2 ** 31))]
        torch.distributed.broadcast_object_list(box, src=0)
        args.seed = box[0]
        if rank == 0:
            print(f"data parallel run without --seed: rank 0 drew seed {args.seed} for every rank")
    if args.seed is not None:
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    data, args = process_dataset(args)
    from fitgnn_amd import pipeline

    if world > 1 and (args.baseline or args.task != 'node_cls'):
        raise NotImplementedError("data parallel runs cover the FIT-GNN node-classification path (--train_fitgnn, "
                                  "--gradient_method GD); launch baselines and the other tasks as one process")

    path = f"save/{args.task}/" + (f"baseline/{args.output_dir}/" if args.baseline else f"{args.output_dir}/")
    os.makedirs(path, exist_ok=True)
    if args.use_community_detection and args.task == 'node_cls':   # main.py:247-267
        labels = pipeline.detect_communities(data.edge_index, data.num_nodes, seed=0 if args.seed is None else args.seed,
                                             method=args.community_method)
        data = pipeline.merge_communities(data, labels, args.community_nodes)
        print(f"community detection: {int(labels.max()) + 1} communities, kept {data.num_nodes} nodes (<= {args.community_nodes})")
    if args.task == 'node_reg':
        if args.baseline:
            return pipeline.node_regression_baseline(args, path, data, device=args.device)
        co = pipeline.coarsening_classification(args, data, 1 - args.coarsening_ratio, args.coarsening_method, device=args.device)
        return pipeline.node_regression(args, path, data, co, device=args.device)
    if args.task in ('graph_reg', 'graph_cls'):
        if args.baseline:
            return pipeline.graph_baseline(args, path, data, device=args.device)
        return pipeline.graph_regression(args, path, data, device=args.device)
    if args.baseline:
        res = pipeline.node_classification_baseline(args, path, data, device=args.device)
        write_results(args, *res, baseline=True)
    else:
        co = None
        if rank == 0:
            co = pipeline.coarsening_classification(args, data, 1 - args.coarsening_ratio, args.coarsening_method,
                                                    device=args.device)  # main.py:278 passes 1 - rho as Loukas' r
            print(f"coarsened {data.num_nodes} nodes in {len(co.components)} components into {co.n_clusters} clusters")
        if world > 1:   # ONE partition for all ranks (the eigensolver's start vector is random: ranks would not agree)
            box = [co]
            torch.distributed.broadcast_object_list(box, src=0)
            co = box[0]
        res = pipeline.node_classification(args, path, data, co, device=args.device, log=print if rank == 0 else (lambda *a: None))
        if rank == 0:
            # main.py:279 `save(...)`: the subgraph union as a flat, memory-mappable artefact (fitgnn_amd.store)
            from fitgnn_amd import store
            store.save_gs(store.artefact_dir(f"./dataset/{args.dataset}/saved/{args.coarsening_method}", args),
                          pipeline.build_gs(args, pipeline.splits_classification(data, args.num_classes, args.experiment,
                                                                                 np.random.default_rng(args.seed)), co, args.device), co)
            write_results(args, *res, baseline=False)
        if world > 1:
            torch.distributed.barrier()
    return res


if __name__ == "__main__":
    main()
