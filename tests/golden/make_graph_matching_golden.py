#!/usr/bin/env python3
"""Generate tests/golden/graph_matching.npz from the *real* FIT-GNN reference: the graph-level loop of the matching methods.

Runs ONLY where the reference checkout is available (make_golden.py's pygsp stand-in; make_matching_golden.py's Tap, which
records every matching_greedy call and makes it use a stable argsort -- the project's tie rule, rank = (-weight, edge id)).

The input is a sequence of small connected graphs (a 2-node graph, a 3-node path, a star, K5, then ring-plus-chord
molecules, a few of them weighted).  For method in {heavy_edge, algebraic_JC} and r in {0.3, 0.5, 0.7}, np.random.seed(SEED)
once, then the unmodified reference's coarsen(G, K=10, r=r, method=m) on every graph in order -- what
coarsening_classification / coarsening_regression (utils.py:163-182, :378-411) do for one-component graphs, so algebraic_JC's
draws run on from one graph to the next -- and finally np.random.randn(NEXT): the stream's position after the loop.
Recorded per (method, r) and graph: C (the cluster of every node = the row of its column's non-zero, and that value), the
number of clusters, Gc.W (CSR), the applied levels (leading matching_greedy calls that took > 2 pairs: :131-135), and
min_rel_gap, the smallest relative gap between distinct weights of any of its levels (a near-tie where the device's rounding
of the test vectors may order two edges differently).  Re-run: `python tests/golden/make_graph_matching_golden.py`.
"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402  (the pygsp stand-in)
import make_matching_golden as mmg  # noqa: E402  (Tap: stable matching_greedy, per-level weights)

METHODS = ("heavy_edge", "algebraic_JC")
RATIOS = (0.3, 0.5, 0.7)
SEED = 0
K = 10
NEXT = 8
OUT = os.path.join(HERE, "graph_matching.npz")


def und(n, edges, w=None):
    e = np.array(edges, dtype=np.int64).reshape(-1, 2).T
    v = np.ones(e.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    A = sp.coo_matrix((v, (e[0], e[1])), shape=(n, n))
    W = (A + A.T).tocsr()
    W.sort_indices()
    return W


def graphs():
    rng = np.random.default_rng(2024)
    g = [und(2, [(0, 1)]), und(3, [(0, 1), (1, 2)]), und(9, [(0, i) for i in range(1, 9)]),
         und(5, [(i, j) for i in range(5) for j in range(i)])]
    while len(g) < 40:
        n = int(np.clip(np.rint(rng.normal(16, 6)), 4, 29))
        und_e = {(min(i, (i + 1) % n), max(i, (i + 1) % n)) for i in range(n)}
        for _ in range(int(rng.integers(1, 4))):
            a, b = (int(x) for x in rng.integers(0, n, size=2))
            if a != b:
                und_e.add((min(a, b), max(a, b)))
        e = sorted(und_e)
        w = rng.uniform(0.5, 2.0, size=len(e)) if len(g) % 5 == 0 else None
        g.append(und(n, e, w))
    return g


def main():
    if not hasattr(np, "Inf"):
        np.Inf = np.inf  # the reference predates numpy 2
    mg._install_pygsp_standin()
    sys.path.insert(0, mg.REF)
    from graph_coarsening import coarsening_utils as cu  # the unmodified reference module

    tap = mmg.Tap(cu)
    tap.stable = True
    gs = graphs()
    Wb = sp.block_diag(gs, format="csr")
    Wb.sort_indices()
    off = np.r_[0, np.cumsum([w.shape[0] for w in gs])].astype(np.int64)
    out = {"W_indptr": Wb.indptr.astype(np.int32), "W_indices": Wb.indices.astype(np.int32), "W_data": Wb.data, "comp_off": off}
    manifest = {"reference": "Roy-Shubhajit/FIT-GNN (graph_coarsening/coarsening_utils.py, utils.py:163-182)", "seed": SEED, "K": K,
                "graphs": len(gs), "nodes": int(off[-1]), "methods": list(METHODS), "ratios": list(RATIOS), "runs": []}
    for m in METHODS:
        for r in RATIOS:
            p = f"{m}_r{int(round(r * 100)):02d}_"
            np.random.seed(SEED)
            assign, cval, ncl, lvl, gap, rp, ci, cd = [], [], [], [], [], [], [], []
            for W in gs:
                tap.reset()
                C, Gc, _ = cu.coarsen(mg._Graph(W), K=K, r=r, method=m)
                C = sp.csc_matrix(C)
                assert np.array_equal(C.indptr, np.arange(W.shape[0] + 1))
                GW = sp.csr_matrix(Gc.W)
                GW.sort_indices()
                applied = 0
                for L in tap.levels:
                    if len(L["stable"]) <= 2:
                        break
                    applied += 1
                assign.append(C.indices.astype(np.int32))
                cval.append(C.data)
                ncl.append(C.shape[0])
                lvl.append(applied)
                gap.append(min(mmg.min_rel_gap(L["weights"]) for L in tap.levels))
                rp.append(GW.indptr.astype(np.int32))
                ci.append(GW.indices.astype(np.int32))
                cd.append(GW.data)
            nxt = np.random.randn(NEXT)
            out.update({p + "assign": np.concatenate(assign), p + "cval": np.concatenate(cval), p + "n": np.array(ncl, np.int64),
                        p + "levels": np.array(lvl, np.int64), p + "min_rel_gap": np.array(gap),
                        p + "gcw_indptr": np.concatenate(rp), p + "gcw_indices": np.concatenate(ci), p + "gcw_data": np.concatenate(cd),
                        p + "next_randn": nxt})
            near = int(np.count_nonzero(np.array(gap) < 1e-6))
            manifest["runs"].append({"method": m, "r": r, "clusters": int(sum(ncl)), "levels": int(sum(lvl)), "near_ties": near})
            print(m, r, "clusters", sum(ncl), "levels", sum(lvl), "near-tie graphs", near, flush=True)
    manifest["layout"] = ("W_* / comp_off: the block-diagonal input; per run <method>_r<pct>_: assign, cval (concatenated per graph, "
                          "cluster ids local to the graph), n, levels, min_rel_gap (per graph), gcw_indptr (n+1 per graph, "
                          "concatenated) / gcw_indices / gcw_data (Gc.W per graph, local ids), next_randn (np.random.randn(%d) after "
                          "the loop)" % NEXT)
    np.savez_compressed(OUT, **out)
    with open(os.path.join(HERE, "graph_matching_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
