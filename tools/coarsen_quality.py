#!/usr/bin/env python3
"""GPU-box tool: coarsening_quality() of every supported coarsen() method at one ratio, with the time of each stage.

  python tools/coarsen_quality.py [--graph cora_giant spubmed] [--r 0.5] [--kmax 30] [--spectral arpack|device]
  python tools/coarsen_quality.py --graph sproducts --methods heavy_edge --spectral device     # S-products size (2.45 M nodes)

Per (graph, method): the coarsen() time, then the metrics summary -- mean error_eigenvalue, error_subspace[kmax-1],
error_sintheta[kmax-1] -- and the stage times of coarsening_quality (the stream is synchronised between stages): eig_L, eig_Lc
(the two eigensolves), Lc (C L C^T on the device, CSR to the host), project (C U and C^T C U), gram (Y^T L Y), cross ((C U)^T Uc).
The fine eigenpairs are computed once per graph (they do not depend on the coarsening; eig_L is printed once) and injected.
coarsen() runs its own level-1 eigensolve (10 pairs) inside its time."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fit-gnn_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from fitgnn_amd import coarsening, data  # noqa: E402
from time_coarsen import cora_giant, spubmed  # noqa: E402


def sproducts():
    N, E = 2449029, 61859140
    ei = data.synthetic_graph(N, E, seed=0)
    return sp.csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(N, N))


GRAPHS = {"cora_giant": cora_giant, "spubmed": spubmed, "sproducts": sproducts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", nargs="+", default=["cora_giant", "spubmed"], choices=sorted(GRAPHS))
    ap.add_argument("--methods", nargs="+", default=list(coarsening.SUPPORTED_METHODS))
    ap.add_argument("--r", type=float, default=0.5)
    ap.add_argument("--kmax", type=int, default=30)
    ap.add_argument("--spectral", default="arpack", choices=("arpack", "device"))
    a = ap.parse_args()
    for gname in a.graph:
        t0 = time.perf_counter()
        W = GRAPHS[gname]()
        G = coarsening.Graph(W)
        print(f"== {gname}: N={G.N} nnz={W.nnz} (built in {time.perf_counter() - t0:.1f} s), r={a.r}, kmax={a.kmax}, "
              f"spectral={a.spectral}", flush=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if a.spectral == "device":
            lk, Uk = coarsening._lanczos_pairs(G.L, a.kmax)
        else:
            import scipy.sparse.linalg as spla
            lk, Uk = spla.eigsh(G.L, k=a.kmax, which="SM", tol=1e-3)
        torch.cuda.synchronize()
        print(f"eig_L {(time.perf_counter() - t0) * 1e3:.1f} ms (once per graph; injected as Uk / lk below)", flush=True)
        for method in a.methods:
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            C, _, _ = coarsening.coarsen(G, K=10, r=a.r, method=method, spectral=a.spectral)
            torch.cuda.synchronize()
            t_coarsen = time.perf_counter() - t0
            tm = {}
            met = coarsening.coarsening_quality(G, C, kmax=a.kmax, Uk=Uk, lk=lk, spectral=a.spectral, timings=tm)
            k = len(met["error_subspace"])
            st = " ".join(f"{s} {tm.get(s, 0.0) * 1e3:.1f}" for s in ("eig_Lc", "Lc", "project", "gram", "cross"))
            print(f"{method:24s} n={C.shape[0]:8d} coarsen {t_coarsen * 1e3:8.1f} ms | mean err_eig {np.mean(met['error_eigenvalue']):.4g} "
                  f"err_subspace[{k - 1}] {met['error_subspace'][k - 1]:.4g} err_sintheta[{k - 1}] {met['error_sintheta'][k - 1]:.4g} "
                  f"| ms: {st}", flush=True)


if __name__ == "__main__":
    main()
