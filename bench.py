#!/usr/bin/env python3
"""bench.py -- edges aggregated/sec (GCN fwd+bwd) on coarsened subgraphs (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload S-products] [--layer GCNConv] [--shard K/N] [--dump-outputs DIR] [--full]

Workload (config.workload), default S-products = BASELINE.json configs[3], the north_star target: "ogbn-products
use_community_detection, subgraph-batch DP" on synthetic data of that shape: one community graph of
165 000 nodes (main.py:264) with mean degree 50 (assumed; E = 4 125 000), features U[0,1) row-L1-normalised F=100, 47
classes (main.py:243), coarsened by the HIP contraction step (variation_neighborhoods, r=0.5), one 1-hop "extra node"
subgraph per cluster (82.5 k subgraphs, 8.2 M union rows), all loader batches merged into ONE device-resident
block-diagonal CSR.  A step = one GD training epoch of run.py:177-215: forward over every subgraph (2-layer GCN,
hidden 512), one NLL loss, backward, Adam step (4 SpMM products over all nnz' entries: edges aggregated = 4 * nnz'; the two
backward products run as ONE two-hop launch).  The other configs
(--workload S-pubmed | S-physics | S-cora) are parity-test cases, selectable for A/B work; --workload S-qm9 is BASELINE.json
configs[4] (graph regression over 130 831 molecules: a step = one training epoch of 512 captured batch steps, bench_qm9 below);
--layer GATConv | APPNP times the same step with the other operators north_star names (per-kind rooflines of their own kernels).
--shard K/N steps ONE rank of an N-rank job alone on this GPU, the gradient all-reduce over RCCL in a group of one: the scaling
evidence a single MI355X can give (tools/shard_curve.py).

N>1 = data parallel, STRONG scaling: the ONE union is sharded by whole subgraphs (data.shard_clusters: LPT over
nnz'), every rank steps on its shard, one flat RCCL gradient all-reduce per step (train.GDTrainer).  Launch either
under torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE in the environment) or plainly as `python bench.py --gpus N`:
the parent then spawns N fresh children itself BEFORE it touches torch or the GPU and relays rank 0's line.

Prints ONE JSON line (rank 0): the metric (dense products in the reference's fp32 arithmetic: csrc/gemm_f32.hip), `roofline` for
the SpMM kernel over ALL FOUR products of the step (HIP events around each launch inside the timed region; per-launch entries
with the number of products they carry and their own compulsory bytes; `traffic` = HBM bytes per product from the committed PMC
passes) and at N>1 `allreduce_ms` and the ranks' nnz'.

A plain run does only what the headline needs: set-up, warm-up, the timed steps, --dump-outputs, the line.  --full adds what takes
runs of its own after the timed region: `ms_per_step_bf16x3` (the same step with the dense products as a 3 x bf16 split),
`ms_per_step_dense_on_all_rows`, `ms_per_step_pruned` / `value_pruned` (the last layer's forward aggregation on the loss rows alone:
fewer edges, its own count), `gemm_kernels` (HIP events over five more steps), `roofline.copy_ceiling_GBps` (the library's own
stream-copy kernel in this process), `t_assemble_s` as the assembly once more (else the first call's time), S-qm9's eager SpMM
roofline, and at N=1 `cpu_baseline` (the torch-CPU oracle of the same step on an evenly spaced sample of loader batches + the C
oracle of the contraction, on this host).  The others are null, empty or absent without it; `full` on the line says which kind
of run it was.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); measured copy ceiling is ~6300

# default (timed steps, warm-up steps) per workload; shapes: fitgnn_amd/workloads.py
DEFAULT_STEPS = {"S-products": (30, 5), "S-pubmed": (200, 20), "S-cora": (200, 20), "S-physics": (100, 10), "S-qm9": (5, 1)}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default per workload: S-products 30)")
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--workload", default="S-products", choices=sorted(DEFAULT_STEPS))
    ap.add_argument("--layer", default="GCNConv", choices=["GCNConv", "GATConv", "APPNP"],
                    help="the message-passing operator of the step (north_star: GCN / GAT / APPNP).  GCNConv = the headline; GATConv = "
                         "network.py's Classify_node with --layer_name GATConv (2 layers, heads 1); APPNP = the SGGC baseline's model "
                         "(Baselines/SGGC/APPNP/networks.py: 2-layer MLP, then K = 10 propagation steps on the class-wide signal).  "
                         "Secondary lines: same metric (SpMM products x nnz' per step), per-kernel rooflines for the operator's own kernels")
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--dropout", type=float, default=0.5, help="F.dropout's p (network.py:33: the default 0.5); 0 makes the step "
                    "deterministic across shardings (the dropout hash is keyed on a rank's own row numbers)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure what takes runs of its own: the re-timed variants of the step, the GEMM "
                         "kernels' events, the copy ceiling, the CPU baseline (see the --no-* options to skip some of them)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-bf16x3", action="store_true", help="--full: skip the re-timing of the step with the dense products as a 3 x bf16 split")
    ap.add_argument("--no-all-rows", action="store_true", help="--full: skip the re-timing with every dense operation over all union rows")
    ap.add_argument("--no-pruned", action="store_true", help="--full: skip the re-timing of the step with the last layer on the clusters' own nodes only")
    ap.add_argument("--fold", action="store_true", help="A/B: epilogue backward folded into the transposed SpMM (slower, see DESIGN.md)")
    ap.add_argument("--prune-unused-rows", action="store_true",
                    help="NOT the headline configuration: last layer only on the clusters' own nodes (the extra nodes' outputs "
                         "never reach the loss); the edge count of the metric is then the number actually aggregated")
    ap.add_argument("--no-dedup", action="store_true",
                    help="run layer 0's X@W^T on the materialised union rows (one copy per subgraph membership) instead of "
                         "the de-duplicated feature table")
    ap.add_argument("--no-dedup-gather", action="store_true",
                    help="A/B: layer 0 on the de-duplicated table through the LDS-window SpMM (row indirection) instead of the "
                         "direct-gather variant")
    ap.add_argument("--stream-kernel", action="store_true", help="A/B: the segment-streaming kernel (one wave per run of segments, no LDS) instead of the whole-subgraph kernel")
    ap.add_argument("--gpu-warm-seconds", type=float, default=None,
                    help="before the warm-up steps, keep the device busy with the library's stream-copy kernel until its rate settles (two "
                         "consecutive windows within 1 %%), at most this many seconds (default 12; 0 = off).  The first heavy process on a device "
                         "that sat idle runs every HBM-bound launch ~5 %% slower for its first seconds (DESIGN §0: 32.07 ms as the first process on a "
                         "freshly leased box, 30.25 as the second, 8 s later)")
    ap.add_argument("--reshuffle", default="off", choices=["off", "replay", "eager"],
                    help="S-qm9: re-draw the graph order before every epoch as the reference's DataLoader(shuffle=True) does (run.py:710). "
                         "replay: batches assembled on the device into fixed-capacity buffers, ONE captured step replayed for every batch "
                         "(graph_data.PaddedBatchPlan); eager: every batch's CSR rebuilt on the host, steps run eagerly; off (default): the "
                         "order is drawn once and each batch's captured step replayed")
    ap.add_argument("--round3-graph-step", action="store_true",
                    help="A/B (S-qm9): the batch step as round 3 had it -- first layer transform-first (its two SpMMs per step), pool / scale / "
                         "library product / bias add for the head, `grad += new` per tensor, loss.backward() from a ones fill")
    ap.add_argument("--no-appnp-sliced", action="store_true",
                    help="A/B (--layer APPNP): the whole-signal units kernel (one wavefront per <= 64-row unit, 24 KB of LDS buffers) and no "
                         "larger subgraph in LDS, instead of the column-sliced kernel (fitgnn_appnp_lds_f32)")
    ap.add_argument("--no-appnp-blocks", action="store_true",
                    help="A/B (--layer APPNP): the subgraphs beyond a wavefront's LDS on the per-step kernel (20 launches per step) instead of "
                         "one workgroup each for all K steps (fitgnn_appnp_blocks_f32)")
    ap.add_argument("--no-two-hop", action="store_true", help="A/B: the two backward SpMM products as two launches (dZ written and re-read)")
    ap.add_argument("--no-compact-rows", action="store_true", help="A/B: the compact backward operand through the tile / whole-subgraph kernels")
    ap.add_argument("--gemm-precision", default="exact", choices=["exact", "high", "highest"],
                    help="dense GEMM policy of the timed region (ops.OpConfig.gemm_precision): exact = the reference's arithmetic, "
                         "fp32 products and accumulation on the fp32 MFMA (csrc/gemm_f32.hip); high = 3 x bf16 split (rel err ~5e-6); "
                         "highest = the library's fp32 kernels")
    ap.add_argument("--shard", default=None, metavar="K/N",
                    help="ONE rank of an N-rank data-parallel job stepped alone on this GPU (scaling evidence a single MI355X can give): "
                         "rank K's shard (or `heaviest/N`) is built exactly as --gpus N builds it (workloads.shard_before_assembly), the loss "
                         "is scaled by the whole job's train count, and the gradient all-reduce runs for real over RCCL in a one-rank group "
                         "(the collective's launch path; no peer).  tools/shard_curve.py runs N = 1, 2, 4, 8 and fits the model of DESIGN 5")
    ap.add_argument("--spectral", default="device", choices=["device", "arpack"],
                    help="spectral prelude of the contraction (not timed): thick-restart Lanczos on the GPU, or ARPACK on the host")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (f32 / f64, at most 64 MB in "
                         "all): the loss, the updated parameters and Adam's moments.  The inputs depend on the arguments only, so two "
                         "builds run with the same arguments can be compared output for output")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = DEFAULT_STEPS[args.workload][0]
    if args.warmup is None:
        args.warmup = DEFAULT_STEPS[args.workload][1]
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


DUMP_BYTES = 63 << 20   # data of the --dump-outputs files (+ their .npy headers: under 64 MB in all)


def step_outputs(model, opt, loss):
    """What a caller of the timed step holds after it: the loss it returned, the model's updated parameters and the optimiser's
    moments (exp_avg carries the step's gradients; the Adam update itself is nearly g / |g| and hides their errors)."""
    import numpy as np

    out = {"loss": loss.detach().reshape(1).cpu().numpy()}
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    for n, p in named:
        out["param." + n] = p.detach().cpu().numpy()
    state = opt.state_dict()["state"]
    for i, (n, _) in enumerate(named):
        if i in state:
            for k in ("exp_avg", "exp_avg_sq"):
                out[f"adam_{k}.{n}"] = state[i][k].detach().cpu().numpy()
    return {k: np.asarray(v, dtype=np.float64 if v.dtype == np.float64 else np.float32) for k, v in out.items()}


def write_outputs(path, arrays, limit=DUMP_BYTES):
    """arrays -> path/<name>.npy.  Over `limit` bytes in all, every array is cut to the same fraction of its entries: a fixed sample
    (seeded by the array's name, ascending flat positions), so that two runs write the same positions."""
    import zlib

    import numpy as np

    os.makedirs(path, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    frac = min(1.0, limit / total) if total else 1.0
    for name, a in arrays.items():
        if frac < 1.0:
            k = int(a.size * frac)
            idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(a.size, k, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N fresh children (one per GPU) and relay rank 0's output.
    The parent has imported neither torch nor HIP at this point (a process that has initialised the GPU must never be the one
    that forks / execs the ranks)."""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   FITGNN_BENCH_CHILD="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    try:
        while procs and rc == 0:
            for p in list(procs):
                code = p.poll()
                if code is None:
                    continue
                procs.remove(p)
                if code != 0:
                    rc = code
            time.sleep(0.2)
    finally:
        for p in procs:   # a rank failed (or we were interrupted): stop exactly the children started here
            p.terminate()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
    return rc


PMC_FILE = "profiles/r04_pmc_bench_kernels.json"


def pmc_traffic(launches, run_cfg):
    """`traffic`: HBM bytes per SpMM product from the COMMITTED rocprofv3 --pmc passes of this command (PMC_FILE, written by
    tools/profile_round.sh + tools/summarize_pmc.py: FETCH_SIZE / WRITE_SIZE in passes of their own, (2 FETCH_SIZE + WRITE_SIZE) * 1024
    per the guide's gfx950 correction) -- counters cannot be read inside the timed run.  The file records the configuration its passes
    ran under (`config`) and which kernels make up each launch KIND of ops.OpConfig.profile (`kinds`); the figure is reported only when
    this run's configuration equals the recorded one and every launch kind of this step is listed, null otherwise (a rank's
    shard moves 1/N of these bytes; another hidden width or GEMM policy was not measured)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), PMC_FILE)
    try:
        with open(path) as fh:
            pmc = json.load(fh)
        rec = pmc["config"]
        if not launches or any(rec.get(k) != v for k, v in run_cfg.items()):
            raise KeyError("configuration differs from the PMC passes'")
        total, products = 0.0, 0
        for l in launches:
            b = sum(pmc["kernels"][k]["hbm_bytes_per_launch"] for k in pmc["kinds"][l["kind"]])
            l["pmc_hbm_bytes"] = b
            total += b
            products += l.get("products", 1)
        return {"traffic": total / products,
                "traffic_note": "mean HBM bytes per SpMM product over the step's launches, from %s (rocprofv3 --pmc passes of this command "
                                "and configuration at commit %s; per launch: launches[].pmc_hbm_bytes)" % (PMC_FILE, rec.get("commit", "?"))}
    except (OSError, KeyError, ValueError, TypeError):
        return {"traffic": None}


def _pruned_edges(tr, batch):
    """Edges aggregated by one pruned step: with the forward aggregation of the last layer on the loss rows alone (GDTrainer.prune_forward)
    layer 0's forward and both backward products still run over every entry (the backward's operand is zero outside the loss rows, every
    entry is multiplied); the older row-subset path runs both of layer 1's products on the own rows' entries."""
    sub_nnz = float(tr.sub.f.col.numel())
    return (3.0 * batch.nnz + sub_nnz) if getattr(tr, "prune_forward", False) else (2.0 * batch.nnz + 2.0 * sub_nnz)


def gpu_warm(device, max_seconds):
    """Bring an idle device to its steady clocks before anything is timed: 1-GiB stream copies (fitgnn_stream_copy_f32) in windows of
    12 copies (~4.5 ms) until a second has passed and three consecutive windows move bytes at the same rate (1 %), at most max_seconds.  Returns what it saw (for the line)."""
    import torch
    from fitgnn_amd import _lib

    if max_seconds <= 0:
        return None
    n = 1 << 28   # floats: 1 GiB
    src, dst = torch.empty(n, dtype=torch.float32, device=device), torch.empty(n, dtype=torch.float32, device=device)
    L, st = _lib.lib(), _lib.stream_ptr(device)
    rates, t_begin = [], time.perf_counter()
    while time.perf_counter() - t_begin < max_seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(12):
            _lib.check(L.fitgnn_stream_copy_f32(_lib.dptr(src), _lib.dptr(dst), n, st), "stream_copy")
        e1.record()
        torch.cuda.synchronize(device)
        rates.append(12 * 8.0 * n / (e0.elapsed_time(e1) * 1e-3) / 1e9)
        if time.perf_counter() - t_begin >= 1.0 and len(rates) >= 3 and abs(rates[-1] - rates[-2]) <= 0.01 * rates[-1] and abs(rates[-2] - rates[-3]) <= 0.01 * rates[-2]:
            break
    del src, dst
    return {"seconds": round(time.perf_counter() - t_begin, 2), "first_window_GBps": round(rates[0], 1), "last_window_GBps": round(rates[-1], 1),
            "windows": len(rates)}


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    for p in (ROOT, os.path.join(ROOT, "fit-gnn_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch

    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    n_dev = torch.cuda.device_count()
    local_rank %= max(n_dev, 1)   # rehearsal on a box with fewer GPUs than ranks (FITGNN_BENCH_BACKEND=gloo)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    backend = None
    emu = None   # (rank or "heaviest", ranks) of --shard
    if args.shard:
        if world != 1:
            raise SystemExit("--shard steps ONE rank of an N-rank job alone: run it with --gpus 1")
        k_s, n_s = args.shard.split("/")
        emu = (k_s if k_s == "heaviest" else int(k_s), int(n_s))
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        backend = "nccl"   # = RCCL: the same collectives GDTrainer issues at N ranks, in a group of one
        torch.distributed.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=device)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # nccl = RCCL over xGMI; gloo only to rehearse the multi-process path on a box with fewer GPUs than ranks
        backend = os.environ.get("FITGNN_BENCH_BACKEND", "nccl" if n_dev >= world else "gloo")
        if backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=device)
        else:
            torch.distributed.init_process_group(backend)

    from fitgnn_amd import data, network, ops, train, workloads

    warm_info = gpu_warm(device, 12.0 if args.gpu_warm_seconds is None else args.gpu_warm_seconds)
    if args.workload == "S-qm9":
        out = bench_qm9(args, device, world, rank, backend)
        out["gpu_warm"] = warm_info
        if rank == 0:
            print(json.dumps(out), flush=True)
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    N, E, F, C, r = workloads.SHAPES[args.workload]
    H = args.hidden
    info = dict(nodes=N, undirected_edges=E, features=F, classes=C)

    def bcast(t):
        """Broadcast a device tensor from rank 0 (through the host under gloo).  The buffer is made contiguous first: the collective
        ships memory, not indices, and the receiving ranks' buffers are row-major (synthetic_graph's edge array is a column-indexed
        NumPy view whose strides torch keeps: shipped as it lay, rank 1 received the edge list scrambled -- found in round 3 through
        the per-rank fingerprints below)."""
        t = t.contiguous()
        if backend == "gloo":
            h = t.cpu()
            torch.distributed.broadcast(h, 0)
            return h.to(device)
        torch.distributed.broadcast(t, 0)
        return t

    # ---- the ONE graph, coarsened once (rank 0), known to every rank -------------------------------------------------
    coarsen_inputs = None
    if rank == 0:
        wl = workloads.coarsen_workload(args.workload, device, spectral=args.spectral)
        coarsen_inputs = (wl["W"], wl["Uk"], wl["lk"], wl["r"])
        info.update(wl["timings"])
        ei_d = torch.from_numpy(np.ascontiguousarray(wl["ei"])).to(device)
        assign_d = torch.from_numpy(np.ascontiguousarray(wl["assign"])).to(device)
        head = torch.tensor([wl["ei"].shape[1], wl["n_clusters"]], dtype=torch.int64, device=device)
        # a fingerprint of the partition (the spectral prelude and the contraction are deterministic: every run of this workload
        # must print the same one)
        info["partition_fingerprint"] = int((wl["assign"].astype(np.int64) * (np.arange(N, dtype=np.int64) % 65521 + 1)).sum() % (2 ** 61 - 1))
        del wl
    else:
        head = torch.zeros(2, dtype=torch.int64, device=device)
    if world > 1:
        head = bcast(head)
        if rank != 0:
            ei_d = torch.empty((2, int(head[0])), dtype=torch.int64, device=device)
            assign_d = torch.empty(N, dtype=torch.int64, device=device)
        ei_d, assign_d = bcast(ei_d), bcast(assign_d)
    n_clusters = int(head[1])
    info["clusters"] = n_clusters

    # ---- this rank's subgraphs (device), the block-diagonal batch ---------------------------------------------------------
    # world > 1: the partition is sharded BEFORE anything is assembled (LPT over a weight every rank computes from the graph and
    # the partition: workloads.shard_before_assembly), and a rank assembles its own clusters only
    t4 = time.time()
    mine = None
    if world > 1:
        owner = workloads.shard_before_assembly(args.workload, ei_d, assign_d, n_clusters, world)
        mine = np.nonzero(owner == rank)[0]
        info["owner_fingerprint"] = int((owner * (np.arange(len(owner)) % 65521 + 1)).sum())   # the same on every rank, every run
    elif emu is not None:
        owner, w_c = workloads.shard_before_assembly(args.workload, ei_d, assign_d, n_clusters, emu[1], return_weights=True)
        loads = np.bincount(owner, weights=w_c.astype(np.float64), minlength=emu[1])
        k_emu = int(np.argmax(loads)) if emu[0] == "heaviest" else int(emu[0])
        mine = np.nonzero(owner == k_emu)[0]
        info["owner_fingerprint"] = int((owner * (np.arange(len(owner)) % 65521 + 1)).sum())
        info["emulated"] = {"rank": k_emu, "ranks": emu[1], "rank_weights": [int(v) for v in loads],
                            "share_of_weight": float(loads[k_emu] / loads.sum()), "clusters": int(len(mine))}
    sub, nnz_c = workloads.assemble(args.workload, ei_d, assign_d, n_clusters, clusters=mine)
    torch.cuda.synchronize()
    t5 = time.time()
    # [rows, nnz'] of this rank's shard + fingerprints of what it was built from (graph, partition, ownership): position-weighted
    # sums, so a permuted copy does not pass
    pos_e = torch.arange(ei_d.shape[1], device=device) % 1009 + 1
    mine_sizes = torch.tensor([float(sub["ptr"][-1]), float(nnz_c.sum()),
                               float(((ei_d[0] * 31 + ei_d[1] * 17) * pos_e).sum() % 1000003),
                               float((assign_d * (torch.arange(N, device=device) % 1009 + 1)).sum() % 1000003),
                               float(info.get("owner_fingerprint", 0)), float(sub["core"].sum())], device=device, dtype=torch.float64)
    if world > 1:
        per_rank = [torch.zeros_like(mine_sizes) for _ in range(world)]
        if backend == "gloo":
            host = [t.cpu() for t in per_rank]
            torch.distributed.all_gather(host, mine_sizes.cpu())
            per_rank = host
        else:
            torch.distributed.all_gather(per_rank, mine_sizes)
        for k in (2, 3, 4):   # every rank must have built its shard from the same graph, partition and ownership
            if len({float(t[k]) for t in per_rank}) != 1:
                raise RuntimeError(f"ranks disagree on their inputs (fingerprint {k}): {[float(t[k]) for t in per_rank]}")
        if int(sum(float(t[5]) for t in per_rank)) != N:
            raise RuntimeError("the shards' own nodes do not add up to the graph's nodes")
        info["shard_union_rows"] = [int(t[0]) for t in per_rank]
        info["shard_nnz_prime"] = [int(t[1]) for t in per_rank]
        info.update(union_rows=sum(info["shard_union_rows"]), nnz_prime=sum(info["shard_nnz_prime"]))
    else:
        info.update(union_rows=int(mine_sizes[0]), nnz_prime=int(mine_sizes[1]))
    # t_assemble_first_call_s: this process's FIRST assembly -- it includes the one-time paging-in of the library sort / unique / scan
    # kernels' code objects (0.2-0.8 s, box dependent); t_assemble_s (--full): the same assembly once more = what the algorithm takes
    info["t_assemble_first_call_s"] = round(t5 - t4, 3)
    info["t_assemble_s"] = info["t_assemble_first_call_s"]
    if args.full and world == 1 and emu is None and args.layer == "GCNConv":
        t_w = time.time()
        sub_w, _ = workloads.assemble(args.workload, ei_d, assign_d, n_clusters, clusters=mine)
        torch.cuda.synchronize()
        info["t_assemble_s"] = round(time.time() - t_w, 3)
        del sub_w
        t5 = time.time()
    del ei_d
    batch = workloads.batch_from_subgraphs(args.workload, sub, device)
    torch.cuda.synchronize()
    info["t_batch_csr_s"] = round(time.time() - t5, 2)
    del sub

    if args.layer == "GATConv":
        batch.register_mode("gat")   # the attention layers' CSR over the same star runs as the GCN one

    def make_trainer(precision, loss_rows_only=True, prune=None):
        margs = argparse.Namespace(num_layers1=2, layer_name="GCNConv" if args.layer == "APPNP" else args.layer, num_features=F, hidden=H,
                                   num_classes=C, dropout=args.dropout, K=10, alpha=0.1)
        torch.manual_seed(2)  # weight seed; identical on every rank
        model = (network.APPNPNet(margs) if args.layer == "APPNP" else network.Classify_node(margs)).to(device)
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        # loss_rows_only=False: the last layer transform-first with every dense operation over all union rows (the shape of the
        # reference's step); True (default): aggregate-first, the dense part on the rows that reach the loss -- see DESIGN §0
        cfg = ops.OpConfig(gemm_precision=precision, fold_backward=args.fold, dedup_gather=not args.no_dedup_gather,
                           last_layer_on_loss_rows=loss_rows_only, compact_head_backward=loss_rows_only,
                           stream_kernel=args.stream_kernel, compact_rows_kernel=not args.no_compact_rows,
                           two_hop_backward=not args.no_two_hop, appnp_blocks=not args.no_appnp_blocks,
                           appnp_sliced=not args.no_appnp_sliced)
        kw = {}
        if emu is not None:   # one rank of the N-rank job: the job's train count (every node is a train node), the dist path forced
            kw = dict(process_group=torch.distributed.group.WORLD, global_train_count=float(N))
        tr = train.GDTrainer(model, batch, lr=0.01, weight_decay=5e-4, dedup=not args.no_dedup,
                             prune_unused_rows=prune if prune is not None else args.prune_unused_rows, op_config=cfg, **kw)
        return tr, sd

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    def timed(tr, steps, warmup, per_step_events=None):
        for _ in range(warmup):
            tr.step()
        barrier()
        t0 = time.perf_counter()
        for i in range(steps):
            # HIP-event pairs around the SpMM launches of every 4th step of the timed region (each marker costs ~1 us); recorded
            # on the stream the kernels are launched on (ops.spmm_*: torch's current stream = the one handed to the C ABI)
            if per_step_events is not None and i % 4 == 0:
                tr.cfg.profile = []
                per_step_events.append(tr.cfg.profile)
            else:
                tr.cfg.profile = None
            loss = tr.step()
        tr.cfg.profile = None
        barrier()
        dt = torch.tensor([time.perf_counter() - t0], device=device, dtype=torch.float64)
        if world > 1:
            torch.distributed.all_reduce(dt, op=torch.distributed.ReduceOp.MAX)
        return float(dt.item()), loss

    trainer, sd0 = make_trainer(args.gemm_precision)
    step_events = []
    if world > 1 or emu is not None:
        trainer.comm_events = []
    dt, loss = timed(trainer, args.steps, args.warmup, step_events)
    if args.dump_outputs and rank == 0:   # before the profiled steps below move the weights on
        write_outputs(args.dump_outputs, step_outputs(trainer.model, trainer.opt, loss))
    loss_final = float(loss)
    if world > 1:   # every rank's share of the last timed step's loss (they add up to `loss`)
        share = trainer.local_loss.detach().to(torch.float64).view(1)
        shares = [torch.zeros(1, dtype=torch.float64) for _ in range(world)] if backend == "gloo" else [torch.zeros_like(share) for _ in range(world)]
        torch.distributed.all_gather(shares, share.cpu() if backend == "gloo" else share)
        info["loss_shares"] = [float(t) for t in shares]
    comm_ms = None
    if (world > 1 or emu is not None) and trainer.comm_events:
        torch.cuda.synchronize()
        comm_ms = float(np.mean([a.elapsed_time(b) for a, b in trainer.comm_events[args.warmup:]]))
    trainer.comm_events = None
    # --full: a few more steps, outside the timed region, with events around the hand-written GEMM launches (secondary figures:
    # their markers would cost the headline 1 %)
    gemm_events = []
    if args.full:
        trainer.cfg.profile_gemm = []
        for _ in range(min(args.steps, 5)):
            trainer.step()
        torch.cuda.synchronize()
        gemm_events, trainer.cfg.profile_gemm = trainer.cfg.profile_gemm, None

    edges_per_step = 4.0 * batch.nnz   # GCN / GAT: two layers x (aggregation forward + its adjoint backward)
    if args.layer == "APPNP":
        edges_per_step = 2.0 * 10 * batch.nnz   # K = 10 propagation steps forward + 10 backward, on the class-wide signal
    if trainer.sub is not None:   # layer 0 forward, both backward products over every entry + the loss rows' entries of A_hat (layer 1 forward)
        edges_per_step = _pruned_edges(trainer, batch)
    edges = torch.tensor([edges_per_step], device=device, dtype=torch.float64)
    if world > 1:
        torch.distributed.all_reduce(edges)
    edges_per_step_total = float(edges.item())

    def retime(precision, **kw):
        tr2, _ = make_trainer(precision, **kw)
        k2 = max(3, min(args.steps, 50))
        dt2, loss2 = timed(tr2, k2, max(2, min(args.warmup, 10)))
        e2 = edges_per_step_total
        if tr2.sub is not None:   # the pruned step aggregates fewer edges: its own count
            e2 = _pruned_edges(tr2, batch)
        return dict(ms_per_step=dt2 / k2 * 1e3, value=e2 * k2 / dt2, steps=k2, loss=float(loss2), edges_per_step=e2)

    secondary = args.full and emu is None and args.layer == "GCNConv"
    # secondary: the same step with the dense products as a 3 x bf16 split (narrower than the reference's fp32: never the headline)
    bf16x3 = retime("high") if (secondary and not args.no_bf16x3 and args.gemm_precision == "exact") else None
    # the same step with the last layer transform-first and every dense operation over all union rows
    all_rows = retime(args.gemm_precision, loss_rows_only=False) if (secondary and not args.no_all_rows) else None
    # the step a user of the drop-in gets when the last layer is evaluated only where its output is consumed (the clusters' own
    # nodes; run.py:193-204 discards the rest): fewer edges aggregated, labelled with its own count -- secondary, never `value`
    pruned = retime(args.gemm_precision, prune=True) if (secondary and world == 1 and not args.no_pruned and not args.prune_unused_rows) else None

    # ---- SpMM roofline, ALL launches of the step -------------------------------------------------------------------------------
    # one fp32 CSR SpMM moves 4H R (read X) + 4H R (write Y) + 8 nnz' + 4 (R + 1) bytes; `achieved` = that figure for
    # the step's SpMM launches / the sum of their mean HIP-event durations in the timed region (step-weighted: every launch counts
    # with its own time).  Next to it each launch's OWN compulsory bytes: layer 0's forward reads a de-duplicated table instead of
    # an [R x H] operand, the last layer's backward reads a compact operand and `prev` and lists a table row per CSR entry.
    R, nnz = batch.n_rows, batch.nnz
    n_loss, n_table = int(batch.train_idx.numel()), int(batch.x_table.shape[0]) if batch.x_table is not None else R
    bytes_spmm = 4 * H * R + 4 * H * R + 8 * nnz + 4 * (R + 1)
    csr_bytes = 8 * nnz + 4 * (R + 1)
    names = ["layer0_forward", "layer1_forward", "layer1_backward", "layer0_backward"]
    what = {"table": "operand = the de-duplicated table through a row indirection, bias / ELU / dropout in the store",
            "gather": "direct-gather variant on the de-duplicated table, bias / ELU / dropout in the store",
            "tile": "plain product (operand [R x H], bare store)",
            "compact_dz": "compact operand (loss rows + zero rows) through a row indirection, layer 0's ELU' / dropout' in the store, bias-gradient column sums",
            "compact": "compact operand (loss rows + zero rows) through a row indirection", "dz": "previous layer's ELU' / dropout' in the store"}
    own_bytes = {"table": 4 * H * R + 4 * H * n_table + csr_bytes + 4 * R + 4 * nnz,
                 "gather": 4 * H * R + 4 * H * n_table + csr_bytes + 4 * nnz,
                 "tile": bytes_spmm,
                 "compact_dz": 2 * 4 * H * R + 4 * H * n_loss + csr_bytes + 4 * R + 4 * nnz,
                 "compact": 4 * H * R + 4 * H * n_loss + csr_bytes + 4 * R + 4 * nnz,
                 "dz": 3 * 4 * H * R + csr_bytes}
    what["two_hop"] = ("BOTH backward products in one launch: dZ = (A_hat^T dAH) . layer 0's ELU' / dropout' from the compact operand, used "
                       "from registers, and A_hat^T dZ over it -- dZ is neither written nor read; bias-gradient column sums")
    own_bytes["two_hop"] = 2 * 4 * H * R + 3 * 4 * H * n_loss + 2 * (csr_bytes + 4 * nnz) + 4 * R
    products = {"two_hop": 2}   # SpMM products (the metric's unit: nnz' edges aggregated each) a launch of this kind carries
    launches, n_per_step = [], None
    n_launch = len(step_events[0]) if step_events else 0
    full_steps = [ev for ev in step_events if len(ev) == n_launch]
    kinds = [e[2] for e in full_steps[0]] if full_steps else []
    op_kernel = None
    if args.layer != "GCNConv" and step_events:
        # GAT / APPNP: every kernel of the operator, grouped by kind (ops._timed), with the compulsory bytes of ONE launch of that kind
        # (scores 4H R; aggregation = the §8(d) SpMM bytes; SDDMM reads both dense operands once and writes one value per
        # entry; the edge passes move 4-byte values per entry; APPNP's step is a C-wide SpMM with its teleport operand)
        Cw = C
        kind_bytes = {"gat_scores": 4 * H * R + 8 * R, "gat_edge_softmax": 8 * nnz + 4 * (R + 1) + 8 * R,
                      "gat_aggregate": bytes_spmm, "gat_aggregate_t": bytes_spmm, "gat_epilogue_bwd": 3 * 4 * H * R,
                      "gat_sddmm": 2 * 4 * H * R + 8 * nnz + 4 * (R + 1), "gat_softmax_bwd": 16 * nnz + 4 * (R + 1) + 12 * R,
                      "gat_transpose_edges": 28 * nnz + 4 * (R + 1) + 4 * R, "gat_rank1": 2 * 4 * H * R + 8 * R,
                      "appnp_step": 3 * 4 * Cw * R + 8 * nnz + 4 * (R + 1), "appnp_step_t": 4 * 4 * Cw * R + 8 * nnz + 4 * (R + 1)}
        plan = next(iter(getattr(batch.graph, "_appnp_plan", {}).values()), None) if args.layer == "APPNP" else None
        if plan is not None:   # the K steps in LDS for the rows in units (read z0 / write z_K once), the per-step kernel on the others' sub-matrix
            # (the larger ones one workgroup each: read the signal / write the result once -- the scratch signals between the steps are L2
            # traffic by design; backward also reads and writes its accumulator, which the algorithm does not need: not counted)
            r_u, r_o, nnz_o, r_b, nnz_b = plan.rows_in_units, plan.n_open, plan.nnz_open, plan.rows_in_blocks, plan.nnz_blocks
            r_l, nnz_l = plan.rows_in_lds_blocks, plan.nnz_lds_blocks
            kind_bytes.update({"appnp_units": 2 * 4 * Cw * r_u + 8 * (nnz - nnz_o - nnz_b - nnz_l) + 4 * (r_u + 1),
                               "appnp_units_t": 2 * 4 * Cw * r_u + 8 * (nnz - nnz_o - nnz_b - nnz_l) + 4 * (r_u + 1),
                               "appnp_lds_blocks": 2 * 4 * Cw * r_l + 8 * nnz_l + 4 * (r_l + 1),
                               "appnp_lds_blocks_t": 2 * 4 * Cw * r_l + 8 * nnz_l + 4 * (r_l + 1),
                               "appnp_blocks": 2 * 4 * Cw * r_b + 8 * nnz_b + 4 * (r_b + 1),
                               "appnp_blocks_t": 2 * 4 * Cw * r_b + 8 * nnz_b + 4 * (r_b + 1),
                               "appnp_step": 3 * 4 * Cw * r_o + 8 * nnz_o + 4 * (r_o + 1), "appnp_step_t": 4 * 4 * Cw * r_o + 8 * nnz_o + 4 * (r_o + 1)})
        per_kind = {}
        for ev in step_events:
            for a, b, kind in ev:
                per_kind.setdefault(kind, []).append(a.elapsed_time(b))
        n_steps_ev = max(len(step_events), 1)
        for kind, durs in per_kind.items():
            ms = float(np.mean(durs))
            kb = kind_bytes.get(kind, bytes_spmm)
            launches.append({"launch": kind, "kind": kind, "avg_us": ms * 1e3, "launches_per_step": len(durs) / n_steps_ev,
                             "us_per_step": float(np.sum(durs)) / n_steps_ev * 1e3, "launches_timed": len(durs),
                             "algorithmic_bytes": kb, "frac": kb / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS})
        launches.sort(key=lambda l: -l["us_per_step"])
        sum_ms = sum(l["us_per_step"] for l in launches) * 1e-3
        achieved = sum(l["algorithmic_bytes"] * l["launches_per_step"] for l in launches) / (sum_ms * 1e-3) / 1e9
        best = max(launches, key=lambda l: l["frac"])
        covers = ("every kernel of the %s operator in the step, step-weighted (sum of their compulsory bytes / sum of their launch times); "
                  "launches[0] is the dominant one" % args.layer)
        op_kernel = {"GATConv": "gat.hip (scores, edge softmax, SDDMM, softmax backward) + spmm_tile_kernel (aggregation, its adjoint) + "
                                "epilogue_bwd_kernel, H=%d, f32" % H,
                     "APPNP": "spmm_narrow_kernel (class-wide CSR SpMM with the teleport term in its store), %d columns, f32" % C}[args.layer]
    elif full_steps and trainer.sub is None and sum(products.get(k, 1) for k in kinds) == 4:
        pos_name = 0
        for pos, kind in enumerate(kinds):
            n_prod = products.get(kind, 1)
            ms = float(np.mean([ev[pos][0].elapsed_time(ev[pos][1]) for ev in full_steps]))
            launches.append({"launch": " + ".join(names[pos_name:pos_name + n_prod]), "kind": kind, "what": what.get(kind, kind), "avg_us": ms * 1e3,
                             "launches_timed": len(full_steps), "products": n_prod, "algorithmic_bytes": n_prod * bytes_spmm,
                             "frac": n_prod * bytes_spmm / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                             "own_compulsory_bytes": own_bytes.get(kind), "frac_own": (own_bytes[kind] / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS)
                             if kind in own_bytes else None})
            pos_name += n_prod
        sum_ms = sum(l["avg_us"] for l in launches) * 1e-3
        achieved = 4 * bytes_spmm / (sum_ms * 1e-3) / 1e9
        best = max(launches, key=lambda l: l["frac"])
        covers = ("all four SpMM products of the step (%d launches), step-weighted (4 x the §8(d) bytes / the sum of the mean launch times)"
                  % len(launches))
    else:   # A/B configurations whose step has another launch list: every recorded SpMM launch, formula bytes each
        durs = [a.elapsed_time(b) for ev in step_events for a, b, _ in ev]
        sum_ms = float(np.sum(durs)) if durs else float("nan")
        achieved = len(durs) * bytes_spmm / (sum_ms * 1e-3) / 1e9
        best = None
        covers = "every SpMM launch recorded in the timed region"
    # the hand-written MFMA GEMM kernels of the step (secondary): flops issued / mean HIP-event duration against the dense peak of
    # the pipe they run on (fp32 MFMA 157.3 TFLOP/s for the exact policy; bf16 2 500 for the split, three products per fp32 product)
    exact = args.gemm_precision == "exact"
    peak_tf = 157.3 if exact else 2500.0
    by_kernel = {}
    for a_ev, b_ev, name, flops in gemm_events:
        by_kernel.setdefault(name, []).append((a_ev.elapsed_time(b_ev), flops))
    gemm_summary = {name: {"launches_timed": len(v), "avg_launch_us": float(np.mean([d for d, _ in v])) * 1e3,
                           "bound": "mfma", "unit": "TFLOP/s (fp32 MFMA)" if name.startswith("gemm_f32") else "TFLOP/s (bf16, 3 products per fp32 product)",
                           "achieved": float(np.sum([f for _, f in v]) / (np.sum([d for d, _ in v]) * 1e-3) / 1e12),
                           "peak": 157.3 if name.startswith("gemm_f32") else 2500.0,
                           "frac": float(np.sum([f for _, f in v]) / (np.sum([d for d, _ in v]) * 1e-3) / 1e12 /
                                         (157.3 if name.startswith("gemm_f32") else 2500.0))}
                    for name, v in by_kernel.items()}
    gemm_ms_per_step = float(np.sum([d for v in by_kernel.values() for d, _ in v]) / max(min(args.steps, 5), 1)) if args.full else None
    copy_gbs = None
    if args.full:
        # device-to-device copy ceiling of this GPU, same process, after the timed region (read + write bytes / time)
        # (fitgnn_stream_copy_f32: one workgroup per 16-KiB chunk, 16-byte non-temporal accesses -- the fastest shape of
        # tools/microbench/copy_probe.hip; 2 x 4 GiB moved per launch, far beyond the 256-MiB Infinity Cache)
        from fitgnn_amd import _lib
        src = torch.rand(1 << 30, dtype=torch.float32, device=device)
        dst = torch.empty_like(src)
        copy = lambda: _lib.check(_lib.lib().fitgnn_stream_copy_f32(_lib.dptr(src), _lib.dptr(dst), src.numel(), _lib.stream_ptr(device)), "stream_copy")  # noqa: E731
        copy()
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record()
        for _ in range(5):
            copy()
        c1.record()
        torch.cuda.synchronize()
        copy_gbs = 5 * 2 * src.numel() * 4 / (c0.elapsed_time(c1) * 1e-3) / 1e9
        del src, dst

    run_cfg = dict(workload=args.workload, hidden=H, classes=C, gemm_precision=args.gemm_precision, two_hop=not args.no_two_hop,
                   dropout=args.dropout, dedup=not args.no_dedup, layer=args.layer)
    precision_text = {
        "exact": ("f32 everywhere: SpMM, epilogues, loss, Adam in f32; every dense product of the step in the reference's arithmetic -- fp32 "
                  "operands, exact fp32 products, fp32 accumulation on v_mfma_f32_32x32x2_f32 (hand-written csrc/gemm_f32.hip; measured "
                  "<= 3e-7 of the largest entry against fp64 = fp32 accumulation rounding, the library's own fp32 GEMM error); "
                  "ms_per_step_bf16x3 / value_bf16x3 = the same step with those products as a 3 x bf16 split (4-5e-6: secondary)"),
        "high": ("f32 storage and accumulation; the tall dense products as a 3 x bf16 split (hi.hi + hi.lo + lo.hi) on the bf16 MFMA pipe, "
                 "measured 4-5e-6 relative error vs fp64 (narrower than the reference's fp32)"),
        "highest": "f32 everywhere (library fp32 MFMA products)"}[args.gemm_precision]
    dense_text = {
        "exact": ("hand-written fp32-MFMA kernel csrc/gemm_f32.hip for x W^T, dH W (W read in place) and the split-k dH^T x with a "
                  "fixed-order sum; the few-column head on the loss rows by fitgnn_head_rows_f32; no library GEMM in the step"),
        "high": ("hand-written kernels gemm_nt.hip (X@W^T, dH@W with the previous layer's epilogue backward fused) and gemm_atb.hip "
                 "(dH^T@X, split-K with a fixed-order sum); layer 0's table zero-padded to K % 32 == 0; the few-column head on the loss "
                 "rows by fitgnn_head_rows_f32 (no library GEMM in the step)"),
        "highest": "hipBLASLt fp32 MFMA"}[args.gemm_precision]
    out = {
        "metric": "edges aggregated/sec (GCN fwd+bwd) on coarsened subgraphs",
        "value": edges_per_step_total * args.steps / dt, "unit": "edges/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "ms_per_step_bf16x3": None if bf16x3 is None else bf16x3["ms_per_step"],
        "value_bf16x3": None if bf16x3 is None else bf16x3["value"],
        "ms_per_step_dense_on_all_rows": None if all_rows is None else all_rows["ms_per_step"],
        "value_dense_on_all_rows": None if all_rows is None else all_rows["value"],
        "ms_per_step_pruned": None if pruned is None else pruned["ms_per_step"],
        "value_pruned": None if pruned is None else pruned["value"],
        "edges_per_step_pruned": None if pruned is None else pruned["edges_per_step"],
        "config": {"workload": f"{args.workload}: variation_neighborhoods r={r}, extra-node subgraphs, ONE block-diagonal union "
                               f"sharded over the ranks by whole subgraphs, " +
                               {"GCNConv": f"2-layer GCN hidden {H}", "GATConv": f"2-layer GAT (heads 1) hidden {H}, network.py --layer_name GATConv",
                                "APPNP": f"APPNP (Baselines/SGGC/APPNP/networks.py): MLP {F}-{H}-{C} on the de-duplicated table, K = 10, alpha = 0.1"}[args.layer] +
                               ", GD step + Adam",
                   "layer": args.layer,
                   "last_layer": ("aggregate-first: A_hat h over every row and edge, then x W^T / bias / ELU / dropout / head and the backward's "
                                  "weight-side products on the rows that reach the loss (every cluster's own nodes: "
                                  f"{n_loss} of {batch.n_rows} union rows); all four SpMMs of the step run over all "
                                  "nnz' edges; ms_per_step_dense_on_all_rows = the same step transform-first with every dense operation "
                                  "over all rows"),
                   "parallelism": f"dp{world}", "backend": backend, "ranks_in_group": world if world == 1 else torch.distributed.get_world_size(),
                   "precision": precision_text, "dense_gemm": dense_text, "dropout_p": args.dropout,
                   "layer0_features": f"de-duplicated table ({info['nodes']} rows) + row indirection in the SpMM" if trainer.dedup
                   else "materialised union rows",
                   "rank0_union_rows": R, "rank0_nnz_prime": batch.nnz,
                   **info},
        "roofline": {"kernel": op_kernel or (("spmm_block_kernel + spmm_tile_kernel (CSR SpMM: whole-subgraph kernel over the stars, LDS row windows over "
                                "the small ones; H=%d, f32)" if batch.graph.f.blocks is not None else
                                "spmm_tile_kernel (CSR SpMM, LDS row windows, H=%d, f32)") % H), "bound": "hbm", "achieved": achieved,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                     **pmc_traffic(launches if (world == 1 and emu is None and args.layer == "GCNConv") else None, run_cfg),
                     "covers": covers,
                     "algorithmic_bytes_per_launch": bytes_spmm, "spmm_ms_per_step": sum_ms if launches else None,
                     "launches": launches,
                     "best_launch": None if best is None else {"launch": best["launch"], "frac": best["frac"], "avg_us": best["avg_us"]},
                     "spmm_edges_per_s": (edges_per_step / (sum_ms * 1e-3)) if launches else None,
                     "copy_ceiling_GBps": copy_gbs, "frac_of_copy_ceiling": None if copy_gbs is None else achieved / copy_gbs},
        "run_config": run_cfg,
        "full": args.full,
        "gpu_warm": warm_info,
        "gemm_kernels": gemm_summary, "gemm_ms_per_step": gemm_ms_per_step,
        "loss": loss_final,
    }
    if world > 1 or emu is not None:
        out["allreduce_ms"] = comm_ms   # rank 0: compute-stream time per step inside GDTrainer._reduce_grads (the exposed part)
        out["allreduce_bytes"] = int(trainer.flat.buf.numel()) * 4
    if emu is not None:
        out["scaling"] = "strong (one rank of %d stepped alone: `value` is THIS shard's edges/s, not a job's)" % emu[1]
        out["config"]["parallelism"] = "rank %d of dp%d, alone on one GPU (RCCL group of one)" % (info["emulated"]["rank"], emu[1])
    if args.full and rank == 0 and world == 1 and emu is None and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(batch, sd0, 2, layer=args.layer)
        out["cpu_baseline"]["cpu_model"] = cpu_model()
        out["cpu_baseline"]["host_cores"] = os.cpu_count()
        # the contraction step of the same graph on the host: the C restatement (one core), next to the HIP time above
        from oracle import coarsen_oracle as corc
        Wc, Ukc, lkc, rc = coarsen_inputs
        t0 = time.time()
        corc.coarsen_oracle(Wc, K=10, r=rc, Uk=Ukc.copy(), lk=lkc.copy())
        out["cpu_baseline"]["coarsen_port_s"] = round(time.time() - t0, 3)
        out["cpu_baseline"]["coarsen_port_cores"] = 1
        out["cpu_baseline"]["coarsen_reference_probe"] = ("profiles/reference_probe_timings.json (reference Python, 8 cores: "
                                                          "17.97 s at PubMed size)")
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


def bench_qm9(args, device, world, rank, backend):
    """BASELINE.json configs[4] (QM9 graph regression, network.py:189-204 `Regress_graph_gs`, run.py:288-304 `graph_train_Gs`) on the
    QM9-shaped stand-in of SURVEY §8d: 130 831 molecules coarsened, pooled and assembled in ONE pass each, the training half (65 415
    graphs, utils.py:33) in loader batches of 128 (run.py:513).  A bench "step" = one training EPOCH = 512 batch steps (forward, L1 loss,
    backward, Adam; gradients never cleared inside the epoch, run.py:291), each replayed from a hipGraph captured once.
    value = 4 SpMM products x nnz' of every batch / epoch time."""
    import numpy as np
    import torch
    from fitgnn_amd import graph_data, network, ops, train

    n_graphs, H = 130_831, args.hidden
    t0 = time.time()
    mol = graph_data.synthetic_molecules(n_graphs, seed=0)
    t1 = time.time()
    gset = graph_data.GraphSet(mol, ratio=0.5, extra_node=True, device=device)
    torch.cuda.synchronize()
    t2 = time.time()
    graphs = list(range(n_graphs // 2))
    margs = argparse.Namespace(num_layers1=2, layer_name="GCNConv", num_features=11, hidden=H, num_classes=1, dropout=args.dropout)
    torch.manual_seed(2)
    model = network.Regress_graph_gs(margs).to(device)
    lean = not args.round3_graph_step
    cfg = ops.OpConfig(gemm_precision=args.gemm_precision, narrow_input_first=lean, fused_pool_head=lean)
    model.set_op_config(cfg)
    tr = train.GraphTrainer(model, gset, graphs, kind="gs", batch_size=128, lr=0.001, capture=(world == 1 and args.reshuffle != "eager"),
                            lean_step=lean, reshuffle=args.reshuffle != "off")
    cfg_step = model.op_config   # (the trainer's copy: + its gradient sink)
    torch.cuda.synchronize()
    t3 = time.time()
    rows = sum(int(b["x"].shape[0]) for b in tr.batches if b is not None)
    nnz = sum(int(b["edge_index"].shape[1]) + int(b["x"].shape[0]) for b in tr.batches if b is not None)

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        loss = tr.step()
    barrier()
    t_start = time.perf_counter()
    for _ in range(args.steps):
        loss = tr.step()
    barrier()
    dt = torch.tensor([time.perf_counter() - t_start], device=device, dtype=torch.float64)
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, step_outputs(model, tr.opt, loss))
    tot = torch.tensor([float(nnz), float(rows)], device=device, dtype=torch.float64)
    if world > 1:
        torch.distributed.all_reduce(dt, op=torch.distributed.ReduceOp.MAX)
        torch.distributed.all_reduce(tot)
    dt = float(dt.item())
    nnz_total, rows_total = float(tot[0]), float(tot[1])
    n_batches = len(tr.batches)
    # --full: the SpMM launches of one EAGER epoch's first batches (HIP events cannot be read back from inside a replayed hipGraph): their
    # mean duration against the §8(d) bytes of a batch -- these batches are ~10^4 rows: the launches are latency-, not bandwidth-bound
    launches, achieved = [], float("nan")
    if args.full and world == 1:
        import types
        ev_cfg = cfg.replace(profile=[])   # (no gradient sink: these passes run outside the trainer)
        model.set_op_config(ev_cfg)
        model.train()
        k_ev = min(16, n_batches)
        for b in tr.batches[:k_ev]:
            out_b = model(b, b["graph_of_masked"])
            out_b.sum().backward()
        torch.cuda.synchronize()
        model.set_op_config(cfg_step)
        tr.flat.zero()
        per_kind = {}
        for a, b_, kind in ev_cfg.profile:
            per_kind.setdefault(kind, []).append(a.elapsed_time(b_))
        r_b, nnz_b = rows / n_batches, nnz / n_batches
        bytes_spmm = 8 * H * r_b + 8 * nnz_b + 4 * (r_b + 1)
        for kind, durs in per_kind.items():
            ms = float(np.mean(durs))
            launches.append({"kind": kind, "avg_us": ms * 1e3, "launches_per_batch_step": len(durs) / k_ev, "algorithmic_bytes": bytes_spmm,
                             "frac": bytes_spmm / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS})
        sum_ms = sum(l["avg_us"] * l["launches_per_batch_step"] for l in launches) * 1e-3
        achieved = sum(l["algorithmic_bytes"] * l["launches_per_batch_step"] for l in launches) / max(sum_ms * 1e-3, 1e-12) / 1e9
    # SpMM products a batch step really runs: 4 transform-first; 2 with the first layer on the aggregated input (A_hat x of the 11 atom
    # features is formed once per batch, outside the timed region, and that layer's backward needs no aggregation: x takes no gradient)
    products = round(sum(l["launches_per_batch_step"] for l in launches)) if launches else (2 if lean else 4)
    out = {
        "metric": "edges aggregated/sec (GCN fwd+bwd) on coarsened subgraphs",
        "value": float(products) * nnz_total * args.steps / dt, "unit": "edges/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "spmm_products_per_batch_step": products,
        "value_at_the_reference_product_count": 4.0 * nnz_total * args.steps / dt,
        "graphs_per_s": len(graphs) * args.steps / dt, "batch_steps_per_epoch": n_batches, "us_per_batch_step": dt / args.steps / n_batches * 1e6,
        "config": {"workload": "S-qm9: 130 831 molecules (~18 nodes), variation_neighborhoods r=0.5 per molecule in one batched contraction, "
                               f"extra-node cluster subgraphs; Regress_graph_gs (2-layer GCN hidden {H}, mean pool of the masked rows, lt1), "
                               "a step = one training epoch over the 65 415 training graphs in batches of 128 (forward, L1 loss, backward, "
                               "Adam per batch; gradients accumulate inside the epoch as in run.py:291), every batch step replayed from a hipGraph"
                               + ("; first layer aggregate-first on A_hat x (formed once per batch), pool + head in one launch each way, weight "
                                  "gradients written where the optimiser kernel reads them" if lean else "; round 3's batch step (A/B)"),
                   "parallelism": f"dp{world}", "backend": backend, "graphs": n_graphs, "training_graphs": len(graphs),
                   "union_rows_per_epoch": int(rows_total), "nnz_prime_per_epoch": int(nnz_total), "dropout_p": args.dropout,
                   "captured": bool(tr.capture or tr._plan is not None), "reshuffle": args.reshuffle,
                   "padded_batch": (None if tr._plan is None else {"R_cap": tr._plan.R_cap, "E_cap": tr._plan.E_cap, "T_cap": tr._plan.T_cap,
                                                                   "mean_rows": rows / max(len(tr.batches), 1)}),
                   "t_molecules_s": round(t1 - t0, 2), "t_coarsen_pool_assemble_s": round(t2 - t1, 2),
                   "t_batches_and_capture_s": round(t3 - t2, 2)},
        "roofline": {"kernel": "spmm_tile_kernel (CSR SpMM, LDS row windows, H=%d, f32) on 128-molecule batches" % H, "bound": "hbm",
                     "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                     "covers": "the SpMM launches of the first 16 batch steps run eagerly after the timed region (a batch is ~10^4 rows: "
                               "the launches are latency-bound, and the epoch is bound by its launches per batch step)",
                     "launches": launches},
        "loss": float(loss),
        "full": args.full,
    }
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_qm9(gset, mol, model, tr)
        out["cpu_baseline"]["cpu_model"] = cpu_model()
        out["cpu_baseline"]["host_cores"] = os.cpu_count()
    return out


def cpu_baseline_qm9(gset, mol, model, tr, budget_s=15.0):
    """The oracle's literal restatement of network.py:189-204 (a conv stack per cluster subgraph) + L1 loss + backward, on the first
    loader batches of 128 molecules, as many as fit the budget."""
    import numpy as np
    import torch
    from oracle import gnn_oracle as gorc

    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    e_all = gset.gs_edge_index
    done, t_used, nnz_s = 0, 0.0, 0
    for bi in range(len(tr.batches)):
        g0 = bi * 128
        r_lo, r_hi = int(gset.gs_ptr[g0]), int(gset.gs_ptr[g0 + 128])
        keep = (e_all[0] >= r_lo) & (e_all[0] < r_hi)
        e = e_all[:, keep].cpu()
        set_gs = []
        for g in range(g0, g0 + 128):
            subs = []
            for c in range(int(gset.cluster_ptr[g]), int(gset.cluster_ptr[g + 1])):
                r0, r1 = int(gset.sub_ptr[c]), int(gset.sub_ptr[c + 1])
                k = (e[0] >= r0) & (e[0] < r1)
                subs.append(dict(x=gset.gs_x[r0:r1].cpu(), edge_index=e[:, k] - r0, mask=gset.gs_mask[r0:r1].cpu()))
            set_gs.append(subs)
        bt = torch.repeat_interleave(torch.arange(128), torch.from_numpy(np.diff(mol["node_ptr"][g0:g0 + 129])))
        tgt = torch.from_numpy(mol["y"][g0:g0 + 128]).long()[:, 0].view(-1, 1).float()
        t0 = time.time()
        params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        ref = gorc.regress_graph_gs_forward(params, set_gs, bt)
        torch.nn.functional.l1_loss(ref, tgt).backward()
        if bi > 0:   # the first batch warms the thread pools up
            t_used += time.time() - t0
            nnz_s += int(e.shape[1]) + (r_hi - r_lo)
            done += 1
        if t_used > budget_s or done >= 32:
            break
    return dict(value=4 * nnz_s / max(t_used, 1e-9), unit="edges/s", cores=torch.get_num_threads(), kind="port",
                sample=f"loader batches 1..{done} of {len(tr.batches)} (128 molecules each; literal per-subgraph loops of network.py:189-204), "
                       f"nnz' = {nnz_s}, 1 fwd+bwd each, {t_used:.2f} s")


def cpu_baseline(batch, sd, num_layers, budget_s=20.0, layer="GCNConv"):
    """The torch-CPU oracle of the same step (fwd + loss + bwd), timed on this host.  Sample = loader batches of the reference
    (run.py:336: 128 subgraphs each) drawn EVENLY SPACED over the loader's order -- the assembly lists large subgraphs first, so the
    first batches alone would be the densest ones -- as many as fit the time budget; the sample's rows and nnz' are reported."""
    import torch
    from oracle import gnn_oracle as gorc

    spans = batch.slice_batches(128)
    ei_all = batch.edge_index

    def gather(k):
        """host copies of k evenly spaced loader batches, rows renumbered to one block-diagonal sample"""
        pick = sorted({int(round(i * (len(spans) - 1) / max(k - 1, 1))) for i in range(k)})
        xs, ys, tms, es, off = [], [], [], [], 0
        for b in pick:
            r0, r1 = spans[b]
            keep = (ei_all[0] >= r0) & (ei_all[0] < r1)
            es.append((ei_all[:, keep] - r0 + off).cpu())
            xs.append(batch.x[r0:r1].cpu()); ys.append(batch.y[r0:r1].cpu()); tms.append(batch.train_mask[r0:r1].cpu())
            off += r1 - r0
        return torch.cat(xs), torch.cat(es, 1), torch.cat(ys), torch.cat(tms), len(pick)

    def run(sample):
        x, e, y, tm, _ = sample
        t0 = time.time()
        if layer == "GATConv":
            gorc.classify_node_gat_fwd_bwd(sd, x, e, y, num_layers=num_layers, train_mask=tm)
        elif layer == "APPNP":
            gorc.appnp_net_fwd_bwd(sd, x, e, y, K=10, alpha=0.1, train_mask=tm)
        else:
            gorc.classify_node_fwd_bwd(sd, x, e, y, num_layers=num_layers, train_mask=tm)
        return time.time() - t0, int(e.shape[1]) + int(x.shape[0])

    run(gather(min(2, len(spans))))  # warm-up (thread pools, allocator)
    k = min(8, len(spans))
    smp = gather(k)
    dt, nnz_s = run(smp)
    if dt < budget_s / 4 and k < len(spans):
        k = min(len(spans), 256, max(k + 1, int(k * (budget_s / 2) / max(dt, 1e-3))))
        smp = gather(k)
        dt, nnz_s = run(smp)
    per_step = 20 if layer == "APPNP" else 4   # SpMM products of one step (APPNP: K = 10 forward + 10 backward)
    return dict(value=per_step * nnz_s / dt, unit="edges/s", cores=torch.get_num_threads(), kind="port",
                sample=f"{smp[4]} of {len(spans)} loader batches (128 subgraphs each), evenly spaced over the loader's order: "
                       f"{int(smp[0].shape[0])} rows, nnz' = {nnz_s} ({nnz_s / max(batch.nnz, 1):.4f} of the union's), 1 fwd+bwd step, {dt:.2f} s")


if __name__ == "__main__":
    main()
