#!/usr/bin/env python3
"""GPU-box tool: wall-clock breakdown of one coarsen() call (host vs device stages).

  python tools/time_coarsen.py                                  # variation_neighborhoods on the S-pubmed graph, vs the C oracle
  python tools/time_coarsen.py --method heavy_edge [--graph cora_giant]
      a matching method: coarsen() wall time, then one level's device stages timed one by one (edge list, test vectors,
      proximity / cost, matching with its round count, assignment + lift)."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fit-gnn_amd")):
    sys.path.insert(0, p)
import numpy as np, scipy.sparse as sp, scipy.sparse.linalg as spla, torch
from fitgnn_amd import coarsening, data


def spubmed():
    N, E = 19717, 44324
    ei = data.synthetic_graph(N, E, seed=0)
    return sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(N, N))


def cora_giant():
    from fitgnn_amd import pipeline
    d, _ = pipeline.load_planetoid(os.path.join(ROOT, "tests", "golden", "cora_raw"), "cora")
    ei = np.asarray(d.edge_index)
    W = sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(d.num_nodes, d.num_nodes))
    W.data[:] = 1.0
    return max(coarsening.Graph(W).extract_components(), key=lambda g: g.N).W


def spectral(W):
    G = coarsening.Graph(W)
    offset = 2 * max(G.dw)
    T = offset * sp.eye(G.N, format="csc") - G.L
    lk, Uk = spla.eigsh(T, k=10, which="LM", tol=1e-5, v0=np.random.default_rng(0).standard_normal(G.N))
    return (offset - lk)[::-1].copy(), np.ascontiguousarray(Uk[:, ::-1])


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.time() - t0) * 1e3


def time_variation_neighborhoods(W):
    from oracle import coarsen_oracle as orc
    G = coarsening.Graph(W)
    lk, Uk = spectral(W)
    for rep in range(3):
        _, t_all = clock(lambda: coarsening.coarsen(coarsening.Graph(W), r=0.5, method="variation_neighborhoods", Uk=Uk.copy(), lk=lk.copy()))
        A = coarsening._spectral_level1(G, 10, Uk.copy(), lk.copy())
        res, t_level = clock(lambda: coarsening.contract_level(G, A, 0.5))
        _, t_lift = clock(lambda: coarsening.lift_adjacency(res))
        t0 = time.time()
        orc.coarsen_oracle(W, K=10, r=0.5, Uk=Uk.copy(), lk=lk.copy())
        t_orc = (time.time() - t0) * 1e3
        print(f"rep {rep}: coarsen() {t_all:.1f} ms | contract_level {t_level:.1f} ms, lift {t_lift:.1f} ms | C oracle (1 core) {t_orc:.1f} ms")


def time_matching(W, method, r=0.5):
    G = coarsening.Graph(W)
    kw = {}
    if method == "variation_edges":
        lk, Uk = spectral(W)
        kw = dict(Uk=Uk, lk=lk)
    for rep in range(3):
        np.random.seed(0)
        args = {k: v.copy() for k, v in kw.items()}
        (C, Gc, maps), t_all = clock(lambda: coarsening.coarsen(coarsening.Graph(W), r=r, method=method, **args))
        # one level, stage by stage (level 1 of the call above)
        el, t_el = clock(lambda: coarsening.EdgeList(G))
        t_vec = 0.0
        if method in coarsening.RANDOM_METHODS:
            X0 = np.random.randn(G.N, 10) / np.sqrt(G.N)
            X, t_vec = clock(lambda: coarsening.test_vectors(el, method, X0))
        if method == "variation_edges":
            A = coarsening._spectral_level1(G, 10, kw["Uk"].copy(), kw["lk"].copy())
            wgt, t_w = clock(lambda: -coarsening.edge_costs(el, A))
        else:
            wgt, t_w = clock(lambda: coarsening.proximity(el, method, X if method in coarsening.RANDOM_METHODS else None))
        res, t_m = clock(lambda: coarsening.greedy_matching(el, wgt, coarsening.match_keep(G.N, r)))
        _, t_lift = clock(lambda: coarsening.lift_adjacency(res))
        print(f"rep {rep}: {method} N={G.N} M={el.M}: coarsen() {t_all:.1f} ms, levels {len(maps)}, n={C.shape[0]} | level 1: "
              f"edge list {t_el:.2f} ms, test vectors {t_vec:.2f} ms, weights {t_w:.2f} ms, matching {t_m:.2f} ms "
              f"({res.rounds} rounds), assignment+lift {t_lift:.2f} ms", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", default="variation_neighborhoods")
    ap.add_argument("--graph", default="spubmed", choices=("spubmed", "cora_giant"))
    a = ap.parse_args()
    W = spubmed() if a.graph == "spubmed" else cora_giant()
    if a.method == "variation_neighborhoods":
        time_variation_neighborhoods(W)
    else:
        time_matching(W, a.method)
