#!/usr/bin/env python3
"""Cache-policy probe of the GCN step's HBM streams (fitgnn::NtStream, csrc/common.h).

    python tools/nt_probe.py build              # here or on the GPU box: one library per policy mix, fit-gnn_amd/lib/nt_probe/<name>/
    python tools/nt_probe.py run [--rounds 6]   # GPU box: the bench's default S-products step with every mix, in ONE process

Every library is the default build with spmm.o and lift_pool.o recompiled under `EXTRA=-DFITGNN_NT_STREAMS=<mask>`: the mask replaces
the default mix of the build (it is not or-ed into it), and the `default` row is the library the package builds.  `run` loads every
library, steps the bench's S-products trainer eagerly (no hipGraph), and records a HIP-event pair around every call into the library
(a launch kind = a call site of the step: its function and its occurrence within the step) and around the whole step.  The mixes take
turns in interleaved rounds, the order rotated every round; per round and mix: one untimed step, then --steps timed ones.  Printed:
per launch kind the median over rounds of each mix's mean time and its change against the mix `none` (no nt anywhere)."""
import argparse
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fit-gnn_amd")
LIBDIR = os.path.join(PKG, "lib")
PROBE_DIR = os.path.join(LIBDIR, "nt_probe")

# bit values as in csrc/common.h (fitgnn::NtStream)
BITS = {"out_table": 1 << 0, "out_plain": 1 << 1, "out_two_hop": 1 << 2, "win_plain": 1 << 3, "win_two_hop": 1 << 4, "prev": 1 << 5,
        "win_table": 1 << 6, "side_store": 1 << 7, "seg_load": 1 << 8, "seg_store": 1 << 9}
MIXES = {"none": 0}
MIXES.update(BITS)
MIXES["all_stores"] = BITS["out_table"] | BITS["out_plain"] | BITS["out_two_hop"] | BITS["side_store"] | BITS["seg_store"]
MIXES["all_but_table"] = sum(BITS.values()) & ~BITS["win_table"]
MIXES["all"] = sum(BITS.values())
POLICY_OBJS = ("spmm.o", "lift_pool.o")   # the objects whose code the mask changes


def build(jobs):
    from concurrent.futures import ThreadPoolExecutor

    subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), f"-j{jobs}"])

    def one(item):   # two objects per library: the libraries are built side by side
        name, mask = item
        d = os.path.join(PROBE_DIR, name)
        obj = os.path.join(d, "obj")
        shutil.rmtree(d, ignore_errors=True)
        shutil.copytree(os.path.join(LIBDIR, "obj"), obj)
        for o in POLICY_OBJS:
            os.remove(os.path.join(obj, o))
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j2", f"OBJ={obj}", f"OUT={os.path.join(d, 'libfitgnn_hip.so')}",
                               f"EXTRA=-DFITGNN_NT_STREAMS={mask:#x}"], stdout=subprocess.DEVNULL)
        shutil.rmtree(obj)
        print(f"built {name} (mask {mask:#05x})", flush=True)

    with ThreadPoolExecutor(max(1, jobs // 2)) as ex:
        list(ex.map(one, MIXES.items()))


class Timed:
    """The loaded library with a HIP-event pair around every call (on the current stream: the one the library launches on)."""

    def __init__(self, L, log):
        self._L, self._log = L, log

    def __getattr__(self, name):
        fn = getattr(self._L, name)
        if not name.startswith("fitgnn_"):
            return fn
        import torch

        def call(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self._log.append((name, e0, e1))
            return rc
        return call


def run(rounds, steps):
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    import argparse as ap_
    import numpy as np
    import torch

    from fitgnn_amd import _lib, network, ops, train, workloads

    dev = torch.device("cuda", 0)
    libs = {"default": None}
    libs.update({n: None for n in MIXES})
    for name in libs:
        _lib.LIB_PATH = os.path.join(LIBDIR, "libfitgnn_hip.so") if name == "default" else os.path.join(PROBE_DIR, name, "libfitgnn_hip.so")
        _lib._lib = None
        libs[name] = _lib.lib()
    _lib._lib = libs["default"]

    wname = "S-products"
    N, E, F, C, r = workloads.SHAPES[wname]
    wl = workloads.coarsen_workload(wname, dev)
    sub, _ = workloads.assemble(wname, torch.from_numpy(np.ascontiguousarray(wl["ei"])).to(dev),
                                torch.from_numpy(np.ascontiguousarray(wl["assign"])).to(dev), wl["n_clusters"])
    batch = workloads.batch_from_subgraphs(wname, sub, dev)
    del sub, wl
    margs = ap_.Namespace(num_layers1=2, layer_name="GCNConv", num_features=F, hidden=512, num_classes=C, dropout=0.5, K=10, alpha=0.1)
    torch.manual_seed(2)
    model = network.Classify_node(margs).to(dev)
    cfg = ops.OpConfig(gemm_precision="exact", fold_backward=False, dedup_gather=True, last_layer_on_loss_rows=True, compact_head_backward=True,
                       stream_kernel=False, compact_rows_kernel=True, two_hop_backward=True, appnp_blocks=True, appnp_sliced=True)
    tr = train.GDTrainer(model, batch, lr=0.01, weight_decay=5e-4, dedup=True, prune_unused_rows=False, op_config=cfg)
    tr.capture = False   # eager steps: every library call passes through Timed
    print(f"{wname}: union rows {batch.n_rows}, nnz' {batch.nnz}; {len(libs)} libraries, {rounds} rounds x {steps} steps each", flush=True)

    names = list(libs)
    per = {n: [] for n in names}   # per mix: one {kind: mean us} per round
    for rnd in range(rounds):
        order = names[rnd % len(names):] + names[:rnd % len(names)]
        for n in order:
            log = []
            _lib._lib = Timed(libs[n], log)
            tr.step()   # untimed
            torch.cuda.synchronize()
            log.clear()
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            step_logs = []
            s0.record()
            for _ in range(steps):
                log_before = len(log)
                tr.step()
                step_logs.append((log_before, len(log)))
            s1.record()
            torch.cuda.synchronize()
            kinds = {"step": s0.elapsed_time(s1) / steps * 1e3}
            acc = {}
            for a, b in step_logs:
                seen = {}
                for fname, e0, e1 in log[a:b]:
                    k = seen.get(fname, 0)
                    seen[fname] = k + 1
                    acc.setdefault(f"{fname}#{k}", []).append(e0.elapsed_time(e1) * 1e3)
            kinds.update({k: float(np.mean(v)) for k, v in acc.items()})
            per[n].append(kinds)
        _lib._lib = libs["default"]
        print(f"round {rnd}: " + ", ".join(f"{n} {per[n][-1]['step'] / 1e3:.2f}" for n in names) + " ms/step", flush=True)

    med = {n: {k: float(np.median([d[k] for d in per[n] if k in d])) for k in per[n][0]} for n in names}
    spread = {n: {k: (float(np.min([d[k] for d in per[n] if k in d])), float(np.max([d[k] for d in per[n] if k in d]))) for k in per[n][0]}
              for n in names}
    kinds = [k for k in med["none"] if med["none"][k] >= 20.0]   # launch kinds that move bytes (>= 20 us)
    kinds.sort(key=lambda k: -med["none"][k])
    print("\nmedian over rounds of the mean per launch kind (us); [min..max over rounds]; change vs `none`")
    for k in kinds:
        base = med["none"][k]
        print(f"\n{k}: none {base:9.1f} us [{spread['none'][k][0]:.1f}..{spread['none'][k][1]:.1f}]")
        for n in names:
            if n == "none" or k not in med[n]:
                continue
            d = med[n][k]
            print(f"    {n:14s} {d:9.1f} us [{spread[n][k][0]:.1f}..{spread[n][k][1]:.1f}]  {100.0 * (d - base) / base:+6.2f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["build", "run"])
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    if a.mode == "build":
        build(a.jobs)
    else:
        run(a.rounds, a.steps)


if __name__ == "__main__":
    main()
