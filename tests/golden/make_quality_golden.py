#!/usr/bin/env python3
"""Generate the coarsening_quality golden vectors under tests/golden/ from the *real* FIT-GNN reference.

Runs ONLY where the reference checkout is available (see make_golden.py, whose pygsp stand-in this file imports).  For every
case below it runs the unmodified `graph_coarsening.coarsening_utils.coarsening_quality(G, C, kmax, Uk, lk)` on the W and the
final C that coarsen_<graph>.npz already holds (the reference's variation_neighborhoods result at that ratio), with that
fixture's stored spectral pair (Uk, lk) injected -- copies: the reference overwrites lk[0] -- except where the case says
`inject: false` (then the reference's own eigsh of G.L runs, and the U, l it used are stored).

The coarse eigenpairs the reference used are recorded by wrapping, at module level, scipy.sparse.linalg.eigsh (which the
reference reaches as sp.sparse.linalg.eigsh) and graph_utils.eig (its dense branch, kmax > n / 2).  The tests inject them, so
that the comparison does not depend on the eigensolver's random start.

Output: quality_<graph>.npz + quality_manifest.json; per case, keys under the prefix r<pct>_k<kmax>_:
  Uc, lc (the coarse eigenpairs), U, l (only when not injected), and the metrics r, m, error_eigenvalue, angle_matrix,
  error_subspace, error_sintheta.  Re-run: `python tests/golden/make_quality_golden.py`.
"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402  (the pygsp stand-in)

# (graph, r, kmax, inject Uk/lk)
CASES = [
    ("cora_giant", 0.5, 10, True), ("cora_giant", 0.7, 10, True),
    ("ring100", 0.5, 10, True), ("ring100", 0.7, 10, True),
    ("ring100", 0.5, 5, True),     # Uk (10 columns) wider than kmax: U = Uk whole
    ("ring100", 0.3, 30, False),   # kmax = 30: the reference's own eigsh of G.L (U, l stored)
    ("star40", 0.5, 10, True), ("star40", 0.9, 10, True),     # r = 0.9: n = 5, dense branch, kmax clipped to n
    ("ba600w", 0.5, 10, True), ("ba600w", 0.7, 10, True),
    ("cora26", 0.5, 10, True),     # n = 13: kmax = 10 > n / 2, dense eig(Lc), Uc n x n
    ("cora26", 0.9, 10, True),     # n = 3
]
METRICS = ("r", "m", "error_eigenvalue", "angle_matrix", "error_subspace", "error_sintheta")


class Tap:
    """Records every eigsh / eig result the reference's coarsening_quality computes."""

    def __init__(self, cu):
        self.calls = []
        self.orig_eigsh = sp.linalg.eigsh
        self.orig_eig = cu.graph_utils.eig
        tap = self

        def eigsh(A, *a, **kw):
            l, U = tap.orig_eigsh(A, *a, **kw)
            tap.calls.append(("eigsh", np.array(U), np.array(l)))
            return l, U

        def eig(A, order="ascend"):
            U, l = tap.orig_eig(A, order)
            tap.calls.append(("eig", np.array(U), np.array(l)))
            return U, l

        sp.linalg.eigsh = eigsh
        spla.eigsh = eigsh
        cu.graph_utils.eig = eig


def main():
    mg._install_pygsp_standin()
    sys.path.insert(0, mg.REF)
    from graph_coarsening import coarsening_utils as cu  # the unmodified reference module

    tap = Tap(cu)
    manifest = {"reference": "Roy-Shubhajit/FIT-GNN (graph_coarsening/coarsening_utils.py:257-351 coarsening_quality)",
                "layout": "one npz per graph (inputs W, C, Uk, lk: coarsen_<graph>.npz); per case r<pct>_k<kmax>_{Uc,lc,[U,l],"
                          + ",".join(METRICS) + "}",
                "cases": []}
    outs = {}
    for name, r, kmax, inject in CASES:
        d = np.load(os.path.join(HERE, f"coarsen_{name}.npz"))
        N = len(d["W_indptr"]) - 1
        W = sp.csr_matrix((d["W_data"], d["W_indices"], d["W_indptr"]), shape=(N, N))
        rp = f"r{int(round(r * 100)):02d}_"
        C = sp.csc_matrix((d[rp + "C_data"], d[rp + "C_indices"], d[rp + "C_indptr"]), shape=tuple(d[rp + "C_shape"]))
        kw = {}
        if inject:
            kw = dict(Uk=d["Uk"].copy(), lk=d["lk"].copy())
        tap.calls = []
        met = cu.coarsening_quality(mg._Graph(W), C, kmax=kmax, **kw)
        p = f"{rp}k{kmax}_"
        out = outs.setdefault(name, {})
        if not inject:
            kind, U, l = tap.calls.pop(0)
            assert kind == "eigsh"
            out[p + "U"], out[p + "l"] = U, l
        assert len(tap.calls) == 1, tap.calls
        kind, Uc, lc = tap.calls[0]
        out[p + "Uc"], out[p + "lc"] = Uc, lc
        for k in METRICS:
            out[p + k] = np.asarray(met[k])
        n = C.shape[0]
        manifest["cases"].append({"name": name, "r": r, "kmax": kmax, "inject": inject, "N": int(N), "n": int(n),
                                  "coarse_eig": kind, "file": f"quality_{name}.npz"})
        print(name, r, kmax, "N", N, "n", n, kind, "m", met["m"], "angle", met["angle_matrix"].shape, flush=True)
    for name, out in outs.items():
        np.savez_compressed(os.path.join(HERE, f"quality_{name}.npz"), **out)
    with open(os.path.join(HERE, "quality_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
