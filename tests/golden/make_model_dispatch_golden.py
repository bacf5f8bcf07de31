#!/usr/bin/env python3
"""Record what every model of fitgnn_amd.network runs into tests/golden/model_dispatch.json (needs the MI355X).

For every case of tests/model_dispatch_cases.py in every mode (eval, injected masks, hashed dropout): the autograd nodes, the launch
kinds, the GEMM kernel names and the sha256 of the output and of every parameter gradient (the record's layout: that module's
docstring).  tests/test_gpu_model_dispatch.py holds the models to this file.

The bits rely on run-to-run determinism.  Run the maker twice, in two processes, and compare the files; a case whose bits differ
between the runs is named with --no-bits CASE (its record then keeps nodes, kinds and gemms only).

A change that MEANS to move a model onto other nodes, launches or bits re-records the file with this maker and says so; any other
change leaves the file alone.

    python tests/golden/make_model_dispatch_golden.py [--out PATH] [--no-bits CASE ...]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "fit-gnn_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "model_dispatch.json"))
    ap.add_argument("--no-bits", nargs="*", default=[], metavar="CASE")
    a = ap.parse_args()
    from model_dispatch_cases import CASES, MODES, key, record

    unknown = sorted(set(a.no_bits) - set(CASES))
    if unknown:
        raise SystemExit(f"--no-bits: no such case: {unknown}")
    records = {}
    for name in sorted(CASES):
        for mode in MODES:
            r = record(name, mode)
            if name in a.no_bits:
                del r["out"], r["grads"]
            records[key(name, mode)] = r
            print(key(name, mode), r["nodes"][0] if r["nodes"] else "-", len(r["kinds"]), "launches", flush=True)
    with open(a.out, "w") as f:
        json.dump({"records": records}, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
