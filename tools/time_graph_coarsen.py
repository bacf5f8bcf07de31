"""Wall time of coarsening every graph of synthetic_molecules(n) (the S-qm9 stand-in) with the matching methods:

  heavy_edge, variation_edges   coarsening.coarsen_batch (one batched level loop over all graphs; variation_edges with the
                                dense level-1 prelude GraphSet uses)
  algebraic_JC                  coarsening.coarsen_in_order (fitgnn_match_small's in-order chain) against the reference's
                                per-graph coarsen() loop; the loop is timed on the first --loop_graphs graphs and its
                                full-dataset figure is an EXTRAPOLATION (labelled so)

Prints one JSON line per measurement.  Usage: python tools/time_graph_coarsen.py [--n_graphs 130831] [--loop_graphs 2000]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fit-gnn_amd"))

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from fitgnn_amd import coarsening, graph_data  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n_graphs", type=int, default=130831)
    p.add_argument("--loop_graphs", type=int, default=2000)
    p.add_argument("--ratio", type=float, default=0.5)
    a = p.parse_args()
    mol = graph_data.synthetic_molecules(a.n_graphs, seed=0)
    off = np.asarray(mol["node_ptr"])
    N = int(off[-1])
    ei = mol["edge_index"]
    W = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(N, N))
    r = 1 - a.ratio
    base = dict(graphs=a.n_graphs, nodes=N, r=r, device=torch.cuda.get_device_name(0))
    # warm-up: library load, kernels' first launch
    coarsening.coarsen_batch(W[: off[50]][:, : off[50]], off[:51], r=r, method="heavy_edge")
    coarsening.coarsen_in_order(W[: off[50]][:, : off[50]], off[:51], r=r, method="algebraic_JC")
    for m, spectral in (("heavy_edge", "arpack"), ("variation_edges", "dense")):
        # variation_edges with the dense level-1 prelude: what GraphSet(method="variation_edges") runs
        co, t = timed(lambda: coarsening.coarsen_batch(W, off, r=r, method=m, spectral=spectral))
        print(json.dumps(dict(base, method=m, path="coarsen_batch", spectral=spectral if m == "variation_edges" else None,
                              seconds=round(t, 3), clusters=co.n_clusters)), flush=True)
    for m in ("algebraic_JC", "heavy_edge"):
        np.random.seed(0)
        co, t = timed(lambda: coarsening.coarsen_in_order(W, off, r=r, method=m))
        print(json.dumps(dict(base, method=m, path="coarsen_in_order", seconds=round(t, 3), clusters=co.n_clusters)), flush=True)
    g = min(a.loop_graphs, a.n_graphs)

    def loop():
        for c in range(g):
            b, e = int(off[c]), int(off[c + 1])
            coarsening.coarsen(coarsening.Graph(W[b:e, b:e]), r=r, method="algebraic_JC")

    np.random.seed(0)
    _, t = timed(loop)
    print(json.dumps(dict(base, method="algebraic_JC", path="per-graph coarsen() loop", graphs_timed=g, seconds=round(t, 3),
                          ms_per_graph=round(1e3 * t / g, 3), extrapolated_seconds_all_graphs=round(t / g * a.n_graphs, 1),
                          note="extrapolation from graphs_timed graphs")), flush=True)


if __name__ == "__main__":
    main()
