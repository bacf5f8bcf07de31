#!/usr/bin/env python3
"""Generate tests/golden/cli_flags.json -- the command-line surface of the reference's main.py and inference.py.

    python tests/golden/make_cli_golden.py <checkout of Roy-Shubhajit/FIT-GNN>

Records, per `parser.add_argument(...)` line of each script: the flag name, its default (False for a store_true flag, None when
none is given), whether it is a store_true flag, and whether it is required.  Only these values are stored: no source.
tests/test_cli.py checks fit-gnn_amd/main.py's and inference.py's parsers against them.
"""
import ast
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def flags(path):
    src = open(path).read()
    out = {}
    for m in re.finditer(r"parser\.add_argument\((.*)\)", src):
        call = ast.parse("f(" + m.group(1).split("#")[0].rstrip().rstrip(")") + ")").body[0].value
        kw = {k.arg: k.value for k in call.keywords}
        default = ast.literal_eval(kw["default"]) if "default" in kw else (False if "action" in kw else None)
        out[call.args[0].value] = {"default": default, "flag": "action" in kw, "required": "required" in kw}
    return out


def main():
    ref = sys.argv[1]
    table = {name: flags(os.path.join(ref, name)) for name in ("main.py", "inference.py")}
    with open(os.path.join(HERE, "cli_flags.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in table.items()})


if __name__ == "__main__":
    main()
