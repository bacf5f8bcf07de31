#!/usr/bin/env python3
"""GPU-box tool: wall time and partition quality of the two --community_method paths on one synthetic graph of the S-products
class: planted communities of mixed sizes plus a power-law background, node ids shuffled, built with numpy under a seed.

  python tools/community_latency.py [--nodes 2000000] [--mean_degree 50] [--seed 0] [--out profiles/community_latency.json]

Records: the label-propagation path on the CPU (pipeline.detect_communities, the default method), the modularity path on the GPU
(community.modularity_communities: edge list on the host in, labels on the host out) as a plain run and again with a device
synchronise after every stage for its per-level split into sweeps / stats / aggregation, the levels and sweeps, both partitions'
modularity Q, and the size of the node set merge_communities would keep (--community_nodes).  Wall times are host clocks around work
that ends in a device synchronise or a host read."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fit-gnn_amd")):
    sys.path.insert(0, p)
import numpy as np, torch
from fitgnn_amd import community, pipeline


def make_graph(n, mean_degree, seed):
    """(edge_index int64[2, m] undirected pairs, planted labels).  70 % of the edges fall inside a planted community (sizes 50 .. 60 000,
    heavy-tailed), 30 % join endpoints drawn in proportion to Pareto weights: a few hubs of several thousand neighbours."""
    rng = np.random.default_rng(seed)
    sizes, total = [], 0
    while total < n:
        s = int(min(50 * (1.0 + rng.pareto(1.1)), 60000, n - total))
        sizes.append(s)
        total += s
    sizes = np.array(sizes, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    planted = np.repeat(np.arange(len(sizes)), sizes)
    m = n * mean_degree // 2
    m_in = int(0.7 * m)
    u = rng.integers(0, n, size=m_in)
    v = start[planted[u]] + (rng.random(m_in) * sizes[planted[u]]).astype(np.int64)
    wgt = 1.0 + rng.pareto(1.8, size=n)
    cdf = np.cumsum(wgt / wgt.sum())
    bu = np.minimum(np.searchsorted(cdf, rng.random(m - m_in)), n - 1)
    bv = np.minimum(np.searchsorted(cdf, rng.random(m - m_in)), n - 1)
    perm = rng.permutation(n)
    ei = np.stack([perm[np.concatenate([u, bu])], perm[np.concatenate([v, bv])]])
    lab = np.empty(n, dtype=np.int64)
    lab[perm] = planted
    return ei, lab


def symmetrise(ei, n):
    keep = ei[0] != ei[1]
    key = np.unique(np.concatenate([ei[0][keep] * n + ei[1][keep], ei[1][keep] * n + ei[0][keep]]))
    return np.stack([key // n, key % n])


def kept_nodes(labels, k):
    """merge_communities' rule on the sizes alone: largest first, whole communities while the total stays <= k."""
    total = 0
    for s in -np.sort(-np.bincount(labels), kind="stable"):
        if total + s <= k:
            total += int(s)
            if total == k:
                break
    return total


def describe(ei, n, labels, k):
    sizes = np.bincount(labels)
    return dict(communities=int(sizes.size), largest=int(sizes.max()), Q=community.modularity(ei, n, labels), kept_nodes=kept_nodes(labels, k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2000000)
    ap.add_argument("--mean_degree", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--community_nodes", type=int, default=165000)
    ap.add_argument("--skip_label_propagation", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "community_latency.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: the modularity path has no CPU form"
    t0 = time.perf_counter()
    und, planted = make_graph(a.nodes, a.mean_degree, a.seed)
    ei = symmetrise(und, a.nodes)                      # what main.py hands over: both directions, no duplicates
    del und
    deg = np.bincount(ei[0], minlength=a.nodes)
    res = dict(tool="tools/community_latency.py", device=torch.cuda.get_device_name(0), nodes=a.nodes, directed_edges=int(ei.shape[1]),
               mean_degree=float(deg.mean()), max_degree=int(deg.max()), seed=a.seed, community_nodes=a.community_nodes,
               build_graph_seconds=time.perf_counter() - t0)
    res["planted"] = describe(ei, a.nodes, planted, a.community_nodes)
    print(json.dumps(res), flush=True)

    small = make_graph(20000, 20, 1)[0]                # warm-up: code objects, torch's sort / unique plans
    community.modularity_communities(small, 20000)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lab = community.modularity_communities(ei, a.nodes)
    wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    lab2, info = community.modularity_communities(ei, a.nodes, return_info=True, _seconds=True)
    wall_sync = time.perf_counter() - t0
    assert lab.tobytes() == lab2.tobytes()
    levels = [dict(n=lv["n"], communities=lv["n_communities"], sweeps=lv["sweeps"], Q=lv["qnum"] / info["m2"] ** 2,
                   **{k + "_seconds": v for k, v in lv["seconds"].items()}) for lv in info["levels"]]
    res["modularity_gpu"] = dict(wall_seconds=wall, wall_seconds_with_stage_synchronises=wall_sync, levels=levels,
                                 n_levels=len(levels), n_sweeps=sum(lv["sweeps"] for lv in levels),
                                 sweeps_seconds=sum(lv["sweeps_seconds"] for lv in levels), stats_seconds=sum(lv["stats_seconds"] for lv in levels),
                                 aggregation_seconds=sum(lv["aggregation_seconds"] for lv in levels), **describe(ei, a.nodes, lab, a.community_nodes))
    print(json.dumps(res["modularity_gpu"]), flush=True)

    if not a.skip_label_propagation:
        t0 = time.perf_counter()
        lp = pipeline.detect_communities(ei, a.nodes, seed=a.seed)
        res["label_propagation_cpu"] = dict(wall_seconds=time.perf_counter() - t0, cpu_threads=torch.get_num_threads(),
                                            **describe(ei, a.nodes, lp, a.community_nodes))
        print(json.dumps(res["label_propagation_cpu"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
