"""Modularity community detection on the MI355X for --use_community_detection (DESIGN §4 "Community detection").

The reference runs leidenalg.find_partition(..., ModularityVertexPartition) (main.py:257-258); neither igraph nor leidenalg
exists here and leidenalg is randomised, so this is the partition of a fully specified rule instead: a deterministic,
exact-integer multilevel Louvain scheme (synchronous half-sweeps, each accepted only if it raises the modularity) followed by a
split of every community into its connected pieces.  The sweeps, their statistics and the split are HIP kernels
(csrc/community.hip); relabelling and the aggregation P A P^T between levels are torch sorts and segment sums on the device.
tests/louvain_reference.py restates the rule on the CPU; the two agree bit for bit.  There is no CPU path.
"""
import ctypes
import time

import numpy as np
import torch

from . import _lib

_LIMIT = 2 ** 31


def _i32(t):
    return t.to(torch.int32).contiguous()


def _level0(edge_index, num_nodes, device):
    """Symmetrised, de-duplicated, loop-free CSR of the edge list with ascending columns (every weight 1): rowptr, col (int32)."""
    n = int(num_nodes)
    ei = torch.as_tensor(np.asarray(edge_index)).to(device=device, dtype=torch.int64).reshape(2, -1)
    src, dst = torch.cat([ei[0], ei[1]]), torch.cat([ei[1], ei[0]])
    keep = src != dst
    key = torch.unique(src[keep] * n + dst[keep])          # sorted: row-major, ascending columns
    if key.numel() >= _LIMIT:
        raise _lib.FitgnnError(f"modularity_communities: M2 = {key.numel()} directed edges; M2 and N must stay below 2^31")
    row, col = torch.div(key, n, rounding_mode="floor"), key % n
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
    rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    return _i32(rowptr), _i32(col)


def _number_by_smallest_member(comm):
    """int64 labels 0 .. n_c-1 in the order of every community's smallest member, and n_c."""
    n = comm.numel()
    sorted_c, perm = torch.sort(comm.to(torch.int64), stable=True)
    start = torch.ones(n, dtype=torch.bool, device=comm.device)
    start[1:] = sorted_c[1:] != sorted_c[:-1]
    smallest = perm[start]                                 # stable sort: a group's first node is its smallest
    n_c = int(smallest.numel())
    group_id = torch.empty(n_c, dtype=torch.int64, device=comm.device)
    group_id[torch.argsort(smallest)] = torch.arange(n_c, device=comm.device)
    labels = torch.empty(n, dtype=torch.int64, device=comm.device)
    labels[perm] = group_id[torch.cumsum(start, 0) - 1]
    return labels, n_c


def _aggregate(rowptr, col, w, labels, n_c):
    """P A P^T with the sums inside a community kept on the diagonal: rowptr, col, w (int32) and k of the next level."""
    n = rowptr.numel() - 1
    dev = rowptr.device
    row = torch.repeat_interleave(torch.arange(n, device=dev), (rowptr[1:] - rowptr[:-1]).to(torch.int64))
    key = labels[row] * n_c + labels[col.to(torch.int64)]
    ukey, inv = torch.unique(key, return_inverse=True)
    wsum = torch.zeros(ukey.numel(), dtype=torch.int64, device=dev)
    wsum.index_add_(0, inv, torch.ones_like(key) if w is None else w.to(torch.int64))
    r = torch.div(ukey, n_c, rounding_mode="floor")
    rp = torch.zeros(n_c + 1, dtype=torch.int64, device=dev)
    rp[1:] = torch.cumsum(torch.bincount(r, minlength=n_c), 0)
    k = torch.zeros(n_c, dtype=torch.int64, device=dev)
    k.index_add_(0, r, wsum)
    return _i32(rp), _i32(ukey % n_c), _i32(wsum), _i32(k)


class _Level:
    """The kernels' view of one level graph: buffers, row buckets and the sweep / stats calls."""

    def __init__(self, rowptr, col, w, k, m2):
        self.L = _lib.lib()
        self.rowptr, self.col, self.w, self.k, self.m2 = rowptr, col, w, k, int(m2)
        self.n = rowptr.numel() - 1
        self.dev = rowptr.device
        self.stream = _lib.stream_ptr(self.dev)
        self.max_row = int((rowptr[1:] - rowptr[:-1]).max()) if self.n else 0
        nbytes = self.L.fitgnn_louvain_sweep_workspace_bytes(self.n, self.max_row)
        if nbytes == 0:
            raise _lib.FitgnnError(f"fitgnn_louvain_sweep: N = {self.n}, longest row = {self.max_row} out of range")
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        self.counts = (ctypes.c_int32 * 4)()
        _lib.call("fitgnn_louvain_bucket_rows", rowptr, self.n, self.max_row, self.counts, self.work, nbytes, self.stream)
        self.out = torch.zeros(3, dtype=torch.int64, device=self.dev)

    def sweep(self, comm, tot, size, t, comm_out):
        _lib.call("fitgnn_louvain_sweep", self.rowptr, self.col, self.w, self.k, self.n, self.m2, comm, tot, size, int(t), self.counts, self.max_row,
                  comm_out, self.work, self.work.numel(), self.stream)

    def stats(self, comm, snapshot, tot, size):
        """tot / size of comm are written; returns (moved, Qnum) as Python ints: the one host read of a sweep."""
        _lib.call("fitgnn_louvain_stats", self.rowptr, self.col, self.w, self.k, self.n, self.m2, comm, snapshot, tot, size, self.out, self.stream)
        moved, sum_in, sum_tot2 = (int(v) for v in self.out.tolist())
        return moved, self.m2 * sum_in - sum_tot2

    def run(self, max_sweeps, seconds=None):
        """The sweeps of the level: (comm int32[n], sweeps run, last accepted Qnum)."""
        n, dev = self.n, self.dev
        comm = torch.arange(n, dtype=torch.int32, device=dev)
        buf = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(5)]
        tot, size, comm_new, tot_new, size_new = buf[0], buf[1], buf[2], buf[3], buf[4]
        _, accepted = self.stats(comm, comm, tot, size)     # the singletons
        sweeps = rejected = 0
        while sweeps < max_sweeps and rejected < 2:
            t0 = time.perf_counter()
            self.sweep(comm, tot, size, sweeps, comm_new)
            if seconds is not None:
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                seconds["sweeps"] += t1 - t0
                t0 = t1
            moved, q = self.stats(comm_new, comm, tot_new, size_new)
            if seconds is not None:
                seconds["stats"] += time.perf_counter() - t0
            sweeps += 1
            if moved > 0 and q > accepted:
                comm, comm_new, tot, tot_new, size, size_new = comm_new, comm, tot_new, tot, size_new, size
                accepted, rejected = q, 0
            else:
                rejected += 1
        return comm, sweeps, accepted


def connected_pieces(rowptr, col, comm):
    """int32 label[i] = the smallest node of i's connected component inside its community (fitgnn_louvain_components)."""
    L = _lib.lib()
    n = rowptr.numel() - 1
    dev = rowptr.device
    label = torch.empty(n, dtype=torch.int32, device=dev)
    nbytes = L.fitgnn_louvain_components_workspace_bytes(n)
    work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _lib.call("fitgnn_louvain_components", rowptr, col, n, comm, label, None, work, nbytes, _lib.stream_ptr(dev))
    return label


def modularity_communities(edge_index, num_nodes, max_levels=20, max_sweeps=64, split_disconnected=True, return_info=False,
                           device="cuda", _seconds=False):
    """int64 community labels (numpy), numbered by smallest member.  With return_info also a dict: m2, and per level the
    composed labels after the level, the sweeps run, the accepted Qnum, the level's nodes and communities (and, with _seconds,
    the wall time of its sweeps / stats / aggregation between device synchronisations)."""
    n = int(num_nodes)
    if n >= _LIMIT:
        raise _lib.FitgnnError(f"modularity_communities: N = {n}; M2 and N must stay below 2^31")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.FitgnnError("modularity_communities runs on the MI355X only (no CPU path exists)")
    rowptr0, col0 = _level0(edge_index, n, dev)
    m2 = int(col0.numel())
    rowptr, col, w, k = rowptr0, col0, None, _i32(rowptr0[1:] - rowptr0[:-1])
    composed = torch.arange(n, dtype=torch.int64, device=dev)
    levels = []
    for _ in range(max_levels if n else 0):
        seconds = dict(sweeps=0.0, stats=0.0, aggregation=0.0) if _seconds else None
        n_l = rowptr.numel() - 1
        comm, sweeps, accepted = _Level(rowptr, col, w, k, m2).run(max_sweeps, seconds)
        t0 = time.perf_counter()
        labels, n_c = _number_by_smallest_member(comm)
        composed = labels[composed]
        if n_c < n_l:
            rowptr, col, w, k = _aggregate(rowptr, col, w, labels, n_c)
        if _seconds:
            torch.cuda.synchronize(dev)
            seconds["aggregation"] = time.perf_counter() - t0
        levels.append(dict(labels=composed.cpu().numpy(), sweeps=sweeps, qnum=accepted, n=n_l, n_communities=n_c))
        if _seconds:
            levels[-1]["seconds"] = seconds
        if n_c == n_l:
            break
    final = composed
    if split_disconnected and n:
        final = _number_by_smallest_member(connected_pieces(rowptr0, col0, _i32(composed)))[0]
    final = final.cpu().numpy().astype(np.int64)
    return (final, dict(m2=m2, levels=levels)) if return_info else final


def modularity(edge_index, num_nodes, labels):
    """The exact modularity Qnum / M2^2 of a labelling of the symmetrised, de-duplicated, loop-free graph, computed on the host
    from integers: Qnum = M2 * (directed edges inside a community) - sum of tot[c]^2."""
    n = int(num_nodes)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    src, dst = np.concatenate([ei[0], ei[1]]), np.concatenate([ei[1], ei[0]])
    key = np.unique(src[src != dst] * n + dst[src != dst])
    m2 = int(key.size)
    if m2 == 0:
        return 0.0
    lab = np.unique(np.asarray(labels), return_inverse=True)[1].reshape(-1)
    row, col = key // n, key % n
    sum_in = int((lab[row] == lab[col]).sum())
    tot = np.bincount(lab[row], minlength=int(lab.max()) + 1)
    return (m2 * sum_in - sum(int(x) * int(x) for x in tot)) / (m2 * m2)
