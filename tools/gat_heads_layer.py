#!/usr/bin/env python3
"""One multi-head GATConv layer, forward + backward, on a workloads.py union (GPU only): the multi-head kernels (nn.GATConv(heads > 1)
-> ops.GATHeadsAggregate, csrc/gat_heads.hip) against the per-head composition of the single-head path (ops.Linear once, `heads`
calls of ops.GATAggregate on column slices of h, torch.cat).

    python tools/gat_heads_layer.py [--workload S-pubmed] [--in_channels 512] [--out_channels 64] [--heads 8] [--reps 20] [--rounds 6] [--out FILE]

Writes profiles/gat_heads_layer.json (or --out): HIP-event time per pass of both, `--rounds` alternating rounds of `--reps` passes after
five warm-up passes of each; the device launches (kernels and copies) of one pass of each under torch's profiler; the largest
relative difference of the two forward outputs."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "fit-gnn_amd")]
from fitgnn_amd import nn as fnn, ops, workloads   # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--workload", default="S-pubmed", choices=sorted(workloads.SHAPES))
    p.add_argument("--in_channels", type=int, default=512)
    p.add_argument("--out_channels", type=int, default=64)
    p.add_argument("--heads", type=int, default=8)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "gat_heads_layer.json"))
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "this tool times kernels: it needs the GPU"
    dev = torch.device("cuda")
    wl = workloads.coarsen_workload(a.workload, dev, spectral="device")
    sub, _ = workloads.assemble(a.workload, torch.from_numpy(wl["ei"]).to(dev), torch.from_numpy(wl["assign"]).to(dev), wl["n_clusters"])
    batch = workloads.batch_from_subgraphs(a.workload, sub, dev)
    ei, n = batch.edge_index, batch.n_rows
    g = batch.register_mode("gat")
    Hd, C = a.heads, a.out_channels
    torch.manual_seed(0)
    conv = fnn.GATConv(a.in_channels, C, heads=Hd).to(dev)
    x = torch.randn(n, a.in_channels, device=dev)
    gout = torch.randn(n, Hd * C, device=dev)
    cfg = conv.op_config

    def fused():
        xg = x.detach().requires_grad_(True)
        conv.zero_grad(set_to_none=True)
        out = conv(xg, ei)
        out.backward(gout)
        return out.detach()

    def composed():
        xg = x.detach().requires_grad_(True)
        conv.zero_grad(set_to_none=True)
        h = ops.Linear.apply(xg, conv.lin.weight, cfg)
        a_s, a_d = conv.att_src.view(-1), conv.att_dst.view(-1)
        outs = []
        for k in range(Hd):
            sl = slice(k * C, (k + 1) * C)
            outs.append(ops.GATAggregate.apply(h[:, sl].contiguous(), a_s[sl], a_d[sl], conv.bias[sl], g, conv.negative_slope, False, 0.0,
                                               False, 0, None, cfg))
        out = torch.cat(outs, 1)
        out.backward(gout)
        return out.detach()

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.reps

    for _ in range(5):
        o1, o2 = fused(), composed()
    torch.cuda.synchronize()
    diff = float((o1 - o2).abs().max() / o2.abs().max())
    t_f, t_c = [], []
    for _ in range(a.rounds):
        t_f.append(round(timed(fused), 4))
        t_c.append(round(timed(composed), 4))

    from torch.profiler import ProfilerActivity, profile
    launches = {}
    for label, fn in (("fused", fused), ("composed", composed)):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        launches[label] = len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA])

    res = dict(workload=a.workload, rows=n, nnz=g.nnz, device=torch.cuda.get_device_name(0),
               layer=f"GATConv({a.in_channels}, {C}, heads={Hd}), forward + backward on the whole union, both Linear products included",
               fused="nn.GATConv(heads > 1): ops.Linear, then ops.GATHeadsAggregate (csrc/gat_heads.hip)",
               composed="ops.Linear once, then `heads` x ops.GATAggregate on column slices of h, torch.cat",
               method=f"HIP events around {a.reps} passes, {a.rounds} alternating rounds after 5 warm-up passes of each",
               fused_ms=t_f, composed_ms=t_c, fused_ms_median=round(float(np.median(t_f)), 4),
               composed_ms_median=round(float(np.median(t_c)), 4), speedup=round(float(np.median(t_c) / np.median(t_f)), 2),
               device_launches_per_pass=launches, rel_output_difference=diff)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
