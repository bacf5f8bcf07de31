"""Plain NumPy references of the assembly kernels (csrc/assemble.hip: fitgnn_induced_edges_count / _fill, fitgnn_batch_offsets,
fitgnn_batch_gather) and of the GCN normalisation (fitgnn_gcn_norm_csr_f32 in csrc/gcn_ops.hip), and the inputs of the GPU cases.

Every reference is a loop over the kernel's work items that can be read next to the kernel's comments.  None of them calls into
fitgnn_amd.  Each takes `slip=None`: the name of ONE mistake a kernel could make (SLIPS below).  The references proper are the
`slip=None` paths; tests/test_assemble_reference_cpu.py runs every slip on the inputs of the GPU cases and asserts that the expected
output changes, which is how a case shows that it would notice that mistake without a wrong kernel ever running on a GPU.

The second half of the file builds the inputs that tests/test_gpu_assemble_kernels.py launches the kernels on (the handmade member
index, the synthetic graph-level datasets, the CSR of the normalisation): both test files import them from here, so the CPU file
judges exactly the inputs the GPU file uses.
"""
import zlib

import numpy as np

I32_SENTINEL = 0x5A5A5A5A                 # what every integer output buffer holds before a launch
I64_SENTINEL = 0x5A5A5A5A5A5A5A5A
TILE_INTS = 8                             # fitgnn_tile_t: row_begin, row_end, win_begin, win_rows, nnz_begin, nnz_end, reserved[2]
TILE_ROWS = 16                            # rows of a tile that covers the rows past the batch

SLIPS = {
    # induced edges
    "first_chunk_only": "the chunk loop stops after the first 64 neighbours",
    "drop_lane_63": "the ballot prefix / total drops lane 63: a hit on the last lane of a chunk is lost",
    "no_hi_guard": "hit test without p < hi: a neighbour equal to the FOLLOWING run's first member counts",
    "ignore_inv": "inv ignored: key positions instead of the layout's rows",
    # batch kernels
    "find_first": "batch_find returns the first instead of the last graph among equal offsets",
    "tile_not_clipped": "the last tail tile is not clipped at R_cap",
    "tile_past_rcap": "a tail tile is emitted for r0 >= R_cap",
    "rowptr_rcap_missing": "rowptr[R_cap] is not written",
    "inv_cnt_no_clamp": "inv_cnt = 1 / cnt without the clamp to 1",
    "col_rebase_nnz": "columns re-based with o_nnz instead of o_row",
    "stale_left": "entries past the batch's totals are left as they were",
    "step_not_advanced": "step_idx is not advanced",
    # gcn normalisation
    "gcn_row_64": "only the first 64 entries of a row get a value",
    "gcn_ignore_w": "w ignored in val",
    "gcn_empty_dinv_one": "dinv of a row of non-positive degree taken as 1",
}


def _rng(*parts):
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


# ---------------------------------------------------------------------------------------------------------------------------------
# induced edges
# ---------------------------------------------------------------------------------------------------------------------------------
def find_member(key_node, lo, hi, y, slip=None):
    """Position of node y in the ascending run key_node[lo:hi], or None."""
    for p in range(lo, hi):
        if key_node[p] == y:
            return p
    if slip == "no_hi_guard" and hi < len(key_node) and key_node[hi] == y and all(key_node[p] < y for p in range(lo, hi)):
        return hi      # the lower bound of a y above the whole run is hi: unguarded, the next run's first member is compared
    return None


def induced_edges(adj_ptr, adj, row_node, row_cluster, cl_ptr, key_node, inv=None, slip=None):
    """(cnt int32 [n_rows], e_src, e_dst int64): row r = (cluster c, node x) walks x's adjacency list in order and emits (r, position
    of y in c's member run -- or inv[position]) for every entry y that is a member of c, a repeated entry as often as it occurs."""
    n_rows = len(row_node)
    cnt = np.zeros(n_rows, dtype=np.int32)
    e_src, e_dst = [], []
    for r in range(n_rows):
        x, c = int(row_node[r]), int(row_cluster[r])
        lo, hi = int(cl_ptr[c]), int(cl_ptr[c + 1])
        nbrs = adj[int(adj_ptr[x]):int(adj_ptr[x + 1])]
        if slip == "first_chunk_only":
            nbrs = nbrs[:64]
        for j, y in enumerate(nbrs):
            p = find_member(key_node, lo, hi, int(y), slip)
            if p is None:
                continue
            if slip == "drop_lane_63" and j % 64 == 63:
                continue
            e_src.append(r)
            e_dst.append(p if (inv is None or slip == "ignore_inv") else int(inv[p]))
            cnt[r] += 1
    return cnt, np.asarray(e_src, dtype=np.int64), np.asarray(e_dst, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# batch kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def batch_offsets(perm, step, B, g_row, g_nnz, g_tile, g_mem):
    """(off int32 [4, B + 1], gid int32 [B]) of the batch perm[step * B : step * B + B]: exclusive scans of the graphs' rows, CSR
    entries, tiles and pooled rows, off[k][B] the totals."""
    off = np.zeros((4, B + 1), dtype=np.int32)
    gid = np.zeros(B, dtype=np.int32)
    for i in range(B):
        g = int(perm[step * B + i])
        gid[i] = g
        for k, ptr in enumerate((g_row, g_nnz, g_tile, g_mem)):
            off[k, i + 1] = off[k, i] + (ptr[g + 1] - ptr[g])
    return off, gid


def offsets_state(step, loss_slot, loss_sum, slip=None):
    """The scalars fitgnn_batch_offsets hands over: (step_idx, loss_slot, loss_sum) after the launch.  loss_slot / loss_sum are float32
    scalars or None (NULL): only with both given is the slot added to the sum and cleared."""
    if loss_slot is not None and loss_sum is not None:
        loss_sum = np.float32(np.float32(loss_sum) + np.float32(loss_slot))
        loss_slot = np.float32(0)
    return (step if slip == "step_not_advanced" else step + 1), loss_slot, loss_sum


def batch_find(o, B, idx, slip=None):
    """The graph i of the batch whose range [o[i], o[i + 1]) holds idx: graphs with an empty range are stepped over."""
    hit = [i for i in range(B) if o[i] <= idx < o[i + 1]]
    assert len(hit) == 1
    i = hit[0]
    if slip == "find_first":
        while i > 0 and o[i - 1] == o[i]:
            i -= 1
    return i


def fresh_buffers(B, R_cap, E_cap, T_cap, M_cap, ld_ax, n_tgt, slack=5):
    """The output buffers of fitgnn_batch_gather before a launch: `slack` elements (rows of tiles) longer than their capacities, floats
    NaN, integers the sentinel.  An element that still holds this after the launch is "untouched"."""
    i32 = lambda n: np.full(n, I32_SENTINEL, dtype=np.int32)          # noqa: E731
    f32 = lambda n: np.full(n, np.nan, dtype=np.float32)              # noqa: E731
    return dict(rowptr=i32(R_cap + 1 + slack), col=i32(E_cap + slack), val=f32(E_cap + slack),
                tiles=np.full((T_cap + slack, TILE_INTS), I32_SENTINEL, dtype=np.int32), members=i32(M_cap + slack),
                seg_off=i32(B + 1 + slack), seg_of_row=i32(R_cap + slack), inv_cnt=f32(B + slack), ax=f32(R_cap * ld_ax + slack),
                tgt=f32(B * n_tgt + slack), members64=np.full(M_cap + slack, I64_SENTINEL, dtype=np.int64), cseg=i32(M_cap + slack),
                pos=i32(R_cap + slack))


def batch_gather(B, off, gid, D, R_cap, E_cap, T_cap, M_cap, K, ld_ax, n_tgt, zero_rows, bufs, optional=True, slip=None):
    """Every output buffer of fitgnn_batch_gather after the launch.  `D`: the dataset's arrays (batch_dataset below); `bufs`: the
    buffers as they were before the launch (fresh_buffers, or the result of an earlier step) -- the result is a copy in which every
    element the kernel must write is rewritten and every other one (the padding columns of ax when ld_ax > K, everything past a
    capacity) is left as it was.  optional=False: b_members64, b_cseg and b_pos are NULL (their buffers stay untouched)."""
    O = {k: v.copy() for k, v in bufs.items()}
    o_row, o_nnz, o_tile, o_mem = (off[k] for k in range(4))
    n_row, n_nnz, n_tile, n_mem = (int(off[k, B]) for k in range(4))
    stale = slip == "stale_left"
    zr = max(int(zero_rows), 1)
    for idx in range(R_cap + 1):               # rows: row pointer, pooled-row marker, position, the aggregated input
        if idx < n_row:
            i = batch_find(o_row, B, idx, slip)
            g = int(gid[i])
            src = int(D["g_row"][g]) + (idx - int(o_row[i]))
            O["rowptr"][idx] = o_nnz[i] + (D["rowptr"][src] - D["g_nnz"][g])
            pl = D["pooled"][src] != 0
            O["seg_of_row"][idx] = i if pl else -1
            if optional:
                O["pos"][idx] = o_mem[i] + D["mem_rank"][src] if pl else M_cap + idx % zr
            O["ax"][idx * ld_ax:idx * ld_ax + K] = D["ax"][src, :K]
        else:
            if idx < R_cap or slip != "rowptr_rcap_missing":
                O["rowptr"][idx] = n_nnz       # rows past the batch: no entries
            if idx < R_cap and not stale:
                O["seg_of_row"][idx] = -1
                if optional:
                    O["pos"][idx] = M_cap + idx % zr
                O["ax"][idx * ld_ax:idx * ld_ax + K] = 0.0
    for idx in range(E_cap):                   # CSR entries: columns re-based to the batch's rows
        if idx < n_nnz:
            i = batch_find(o_nnz, B, idx, slip)
            g = int(gid[i])
            src = int(D["g_nnz"][g]) + (idx - int(o_nnz[i]))
            base = o_nnz[i] if slip == "col_rebase_nnz" else o_row[i]
            O["col"][idx] = D["col"][src] - D["g_row"][g] + base
            O["val"][idx] = D["val"][src]
        elif not stale:
            O["col"][idx] = 0
            O["val"][idx] = 0.0
    for idx in range(T_cap):                   # row tiles: the graphs' own, then 16 rows to a tile over the rows past the batch
        t = np.zeros(TILE_INTS, dtype=np.int64)
        if idx < n_tile:
            i = batch_find(o_tile, B, idx, slip)
            g = int(gid[i])
            t[:] = D["tiles"][int(D["g_tile"][g]) + (idx - int(o_tile[i]))]
            dr, dn = int(o_row[i]) - int(D["g_row"][g]), int(o_nnz[i]) - int(D["g_nnz"][g])
            t[0] += dr; t[1] += dr; t[2] += dr
            t[4] += dn; t[5] += dn
        else:
            r0 = n_row + (idx - n_tile) * TILE_ROWS
            if r0 < R_cap or slip == "tile_past_rcap":
                end = r0 + TILE_ROWS if slip == "tile_not_clipped" else min(r0 + TILE_ROWS, R_cap)
                t[0], t[1], t[2], t[3], t[4], t[5] = r0, end, r0, end - r0, n_nnz, n_nnz
        O["tiles"][idx] = t
    for idx in range(M_cap):                   # pooled rows, grouped by graph
        m, sg = 0, -1
        if idx < n_mem:
            i = batch_find(o_mem, B, idx, slip)
            g = int(gid[i])
            m = int(D["mem"][int(D["g_mem"][g]) + (idx - int(o_mem[i]))]) - int(D["g_row"][g]) + int(o_row[i])
            sg = i
        elif stale:
            continue
        O["members"][idx] = m
        if optional:
            O["members64"][idx] = m
            O["cseg"][idx] = sg
    for idx in range(B + 1):                   # per graph: segment offsets, 1 / count, targets
        O["seg_off"][idx] = o_mem[idx]
        if idx < B:
            cnt = int(o_mem[idx + 1]) - int(o_mem[idx])
            with np.errstate(divide="ignore"):
                O["inv_cnt"][idx] = np.float32(1) / np.float32(cnt if (cnt > 0 or slip == "inv_cnt_no_clamp") else 1)
            O["tgt"][idx * n_tgt:(idx + 1) * n_tgt] = D["tgt"][int(gid[idx])]
    return O


def live_tiles_partition(tiles, R_cap, max_rows=TILE_ROWS):
    """True when the tiles with rows, in row order, are a partition of [0, R_cap) into windows of at most max_rows over their own
    rows."""
    t = np.asarray(tiles, dtype=np.int64)
    live = t[t[:, 1] > t[:, 0]]
    live = live[np.argsort(live[:, 0], kind="stable")]
    return bool(len(live) and live[0, 0] == 0 and live[-1, 1] == R_cap and np.array_equal(live[1:, 0], live[:-1, 1])
                and np.all(live[:, 1] - live[:, 0] <= max_rows) and np.array_equal(live[:, 2], live[:, 0])
                and np.array_equal(live[:, 3], live[:, 1] - live[:, 0]) and not t[:, 6:].any())


# ---------------------------------------------------------------------------------------------------------------------------------
# GCN normalisation
# ---------------------------------------------------------------------------------------------------------------------------------
def gcn_norm_csr(rowptr, col, w=None, slip=None):
    """(val [nnz], dinv [n], |terms| of val [nnz], |terms| of deg [n]) in float64: deg = row sum of w (row length when w is None),
    dinv = deg^-1/2 where deg > 0 and 0 elsewhere, val[e] = dinv[row] w[e] dinv[col[e]].  The two |terms| arrays are what the error
    bound is stated in: |dinv[row]| |w[e]| |dinv[col[e]]| per entry, and the row sum of |w| per row.  Entries a slip leaves
    unwritten are NaN."""
    n = len(rowptr) - 1
    nnz = int(rowptr[n])
    ww = np.ones(nnz, dtype=np.float64) if w is None else np.asarray(w, dtype=np.float64)
    deg, adeg = np.zeros(n), np.zeros(n)
    for i in range(n):
        for e in range(int(rowptr[i]), int(rowptr[i + 1])):
            deg[i] += ww[e]
            adeg[i] += abs(ww[e])
    dinv = np.zeros(n)
    for i in range(n):
        if deg[i] > 0:
            dinv[i] = deg[i] ** -0.5
        elif slip == "gcn_empty_dinv_one":
            dinv[i] = 1.0
    val, aval = np.full(nnz, np.nan), np.zeros(nnz)
    for i in range(n):
        for e in range(int(rowptr[i]), int(rowptr[i + 1])):
            if slip == "gcn_row_64" and e - int(rowptr[i]) >= 64:
                continue
            we = 1.0 if slip == "gcn_ignore_w" else ww[e]
            val[e] = dinv[i] * we * dinv[int(col[e])]
            aval[e] = abs(val[e])
    return val, dinv, aval, adeg


# =================================================================================================================================
# The inputs of the GPU cases
# =================================================================================================================================
# ---- induced edges: one handmade member index of 400 nodes ----
INDUCED_NODES = 400
INDUCED_N_ROWS = (1, 3, 4, 5, None)   # None: all rows; the last workgroup (four waves) then holds 1, 3, 4, 1 and 3 live waves


def induced_case():
    """Member runs (key_node, ascending inside a run):
         cluster 0 {5}; 1 {10, 11}; 2 {20, 21, 22}; 3 {21, 30 ... 128} (100 members); 4 empty; 5 {140 ... 396} (257 members).
       Node 21 is a member row of clusters 2 and 3 (an extra node of 3).  Nodes 0 ... 4 lie below every member, 397 ... 399 above.
       Adjacency lists (not symmetric, not sorted) of the nodes whose rows come first:
         146  127 entries: chunk 0 = 63 non-members then 140 (the ONLY hit, lane 63, and the run's first member); chunk 1 sparse
         21   [0, 20, 22, 21, 30, 128, 140, 150, 399]: as a row of cluster 2 the hits are 20, 22, 21; as a row of cluster 3 they are
              21 (first member), 30, 128 (last member); 140 is the first member of the run that follows 3's (cluster 4 is empty);
              150 a member of the following cluster only; 0 below, 399 above every member
         144  64 entries, all hits (200 ... 263)
         10   [11, 20, 5]: 20 is above cluster 1's run and the first member of the next one
         149  200 entries drawn from all 400 nodes with repeats
         140  none; 141 [142] (lane 0); 142 [150, 150] (the same neighbour twice); 143 63 entries 100 ... 162 (40 misses, 23 hits);
         145  65 entries: chunk 0 no hit (0 ... 63), chunk 1 = [396] (lane 0 of the second chunk, the run's last member)
         147  128 entries: chunk 0 = 141 then 63 non-members (only lane 0), chunk 1 all hits
         148  129 entries: chunk 0 all hits, chunk 1 none, chunk 2 = [397] (above every member: the search ends at hi == the end of
              key_node)
         5 [5, 10]; 11 []; 20 [21]; 22 [20, 21, 22, 30]
       every other member node: 0 to 5 random neighbours."""
    rng = _rng("induced")
    runs = [[5], [10, 11], [20, 21, 22], [21] + list(range(30, 129)), [], list(range(140, 397))]
    key_node = np.asarray([x for run in runs for x in run], dtype=np.int64)
    cl_ptr = np.concatenate([[0], np.cumsum([len(run) for run in runs])]).astype(np.int64)
    key_cluster = np.repeat(np.arange(len(runs)), [len(run) for run in runs]).astype(np.int64)
    non5 = np.arange(0, 140)
    lists = {x: list(rng.integers(0, INDUCED_NODES, size=rng.integers(0, 6))) for x in range(INDUCED_NODES)}
    lists.update({
        140: [], 141: [142], 142: [150, 150], 143: list(range(100, 163)), 144: list(range(200, 264)),
        145: list(range(0, 64)) + [396],
        146: list(non5[:63]) + [140] + [int(v) for v in rng.permutation(np.arange(100, 180))[:63]],
        147: [141] + list(non5[40:103]) + list(range(300, 364)),
        148: list(range(150, 214)) + list(range(64, 128)) + [397],
        149: [int(v) for v in rng.integers(0, INDUCED_NODES, size=200)],
        21: [0, 20, 22, 21, 30, 128, 140, 150, 399], 10: [11, 20, 5], 5: [5, 10], 11: [], 20: [21], 22: [20, 21, 22, 30],
    })
    adj_ptr = np.concatenate([[0], np.cumsum([len(lists[x]) for x in range(INDUCED_NODES)])]).astype(np.int64)
    adj = np.asarray([y for x in range(INDUCED_NODES) for y in lists[x]], dtype=np.int64)
    R = len(key_node)
    pos_of = {(int(key_cluster[p]), int(key_node[p])): p for p in range(R)}
    first = [pos_of[(5, 146)], pos_of[(3, 21)], pos_of[(5, 144)], pos_of[(1, 10)], pos_of[(5, 149)]]
    order = np.asarray(first + [p for p in range(R) if p not in first], dtype=np.int64)
    return dict(adj_ptr=adj_ptr, adj=adj, row_node=key_node[order].copy(), row_cluster=key_cluster[order].copy(), cl_ptr=cl_ptr,
                key_node=key_node, inv=rng.permutation(R).astype(np.int64), lengths=np.diff(adj_ptr))


def partitioned_graph():
    """(edge_index int64 [2, E] with both directions, N, assign, n_clusters, a subset of clusters) for the callers' path
    (data.assemble_subgraphs_torch): 600 nodes, 1 500 random undirected edges, node 0 a hub of degree >= 130 (three chunks of its
    adjacency list), one edge listed twice in both directions; a random partition into 100 clusters of which the last ten are
    singletons."""
    rng = _rng("partitioned")
    N, n = 600, 100
    a, b = rng.integers(0, N, size=1500), rng.integers(0, N, size=1500)
    hub = rng.permutation(np.arange(1, N))[:140]
    a, b = np.concatenate([a, np.zeros(140, dtype=np.int64)]), np.concatenate([b, hub])
    keep = a != b
    und = np.unique(np.stack([np.minimum(a, b)[keep], np.maximum(a, b)[keep]], 1), axis=0)
    und = np.concatenate([und, und[7:8]])                     # one duplicated edge
    ei = np.concatenate([und.T, und.T[::-1]], axis=1).astype(np.int64)
    assign = rng.integers(0, n - 10, size=N)
    assign[:n - 10] = np.arange(n - 10)                       # no empty cluster
    assign[N - 10:] = np.arange(n - 10, n)                    # singletons
    clusters = np.asarray(sorted(set(range(0, n, 3)) | {n - 2}), dtype=np.int64)
    return np.ascontiguousarray(ei), N, assign, n, clusters


def kernel_inputs_of(result, edge_index, N):
    """The induced-edge kernels' inputs behind one result of data.assemble_subgraphs_torch (NumPy dict): the adjacency lists in
    (src, dst) order, the rows in the layout's order, the member runs in ascending node order and, where the layout is not the sorted
    one, inv (key position -> row of the layout)."""
    src, dst = edge_index
    order = np.lexsort((dst, src))
    adj = dst[order].astype(np.int64)
    adj_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))]).astype(np.int64)
    ptr, node_id = np.asarray(result["ptr"], dtype=np.int64), np.asarray(result["node_id"], dtype=np.int64)
    row_cluster = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)).astype(np.int64)
    key_node, inv = node_id.copy(), np.arange(len(node_id), dtype=np.int64)
    for c in range(len(ptr) - 1):
        lo, hi = ptr[c], ptr[c + 1]
        rank = np.argsort(node_id[lo:hi], kind="stable")
        key_node[lo:hi] = node_id[lo:hi][rank]
        inv[lo:hi] = lo + rank
    if np.array_equal(inv, np.arange(len(node_id))):
        inv = None
    return dict(adj_ptr=adj_ptr, adj=adj, row_node=node_id, row_cluster=row_cluster, cl_ptr=ptr, key_node=key_node, inv=inv)


# ---- batch kernels: synthetic graph-level datasets ----
def batch_dataset(name, n_rows_of, K, ld_ax_g, n_tgt, unpooled=()):
    """A graph-level dataset as PaddedBatchPlan lays it out, built here from scratch: graph g has n_rows_of[g] rows, cut into tiles of
    1 to 16 rows; every row has 1 to 4 CSR entries whose columns lie inside its own tile (a tile's window is its own rows); about
    half of the rows are pooled, none in the graphs listed in `unpooled`.  Row ids, columns, tiles and pooled rows are GLOBAL (the
    dataset's rows), the four g_* arrays give each graph's ranges.  ax is [R, ld_ax_g] with NaN in the padding columns."""
    rng = _rng("dataset", name)
    G = len(n_rows_of)
    g_row = np.concatenate([[0], np.cumsum(n_rows_of)]).astype(np.int32)
    R = int(g_row[-1])
    rowptr, col, tiles, g_tile, g_nnz = [0], [], [], [0], [0]
    pooled = np.zeros(R, dtype=np.uint8)
    for g in range(G):
        r = int(g_row[g])
        while r < g_row[g + 1]:
            rows = int(min(rng.integers(1, TILE_ROWS + 1), g_row[g + 1] - r))
            nnz0 = rowptr[-1]
            for _ in range(rows):
                cols = np.unique(rng.integers(r, r + rows, size=rng.integers(1, 5)))   # ascending, distinct
                col.extend(int(c) for c in cols)
                rowptr.append(rowptr[-1] + len(cols))
            tiles.append([r, r + rows, r, rows, nnz0, rowptr[-1], 0, 0])
            r += rows
        g_tile.append(len(tiles))
        g_nnz.append(rowptr[-1])
        if g not in unpooled:
            pooled[g_row[g]:g_row[g + 1]] = rng.integers(0, 2, size=n_rows_of[g])
            pooled[rng.integers(g_row[g], g_row[g + 1])] = 1      # at least one
    mem = np.flatnonzero(pooled).astype(np.int32)
    g_mem = np.searchsorted(mem, g_row, side="left").astype(np.int32)
    mem_rank = np.full(R, I32_SENTINEL, dtype=np.int32)           # defined for pooled rows only
    graph_of_mem = np.searchsorted(g_row, mem, side="right") - 1
    mem_rank[mem] = np.arange(len(mem)) - g_mem[graph_of_mem]
    ax = np.full((R, ld_ax_g), np.nan, dtype=np.float32)
    ax[:, :K] = rng.normal(size=(R, K)).astype(np.float32)
    return dict(G=G, R=R, K=K, ld_ax_g=ld_ax_g, n_tgt=n_tgt, g_row=g_row, g_nnz=np.asarray(g_nnz, dtype=np.int32),
                g_tile=np.asarray(g_tile, dtype=np.int32), g_mem=g_mem, rowptr=np.asarray(rowptr, dtype=np.int32),
                col=np.asarray(col, dtype=np.int32), val=rng.uniform(0.1, 1.0, size=len(col)).astype(np.float32),
                tiles=np.asarray(tiles, dtype=np.int32), mem=mem, pooled=pooled, mem_rank=mem_rank, ax=ax,
                tgt=rng.normal(size=(G, n_tgt)).astype(np.float32))


SMALL_UNPOOLED = (3, 17, 29)
_DATASETS = {}


def dataset(name):
    """'k1' / 'k11': 40 graphs of 1 to 40 rows (graphs 3, 17 and 29 without pooled rows; K = 1 / 11 with ld_ax_g = 3 / 12 and
    n_tgt = 1 / 3); 'many': 2 200 graphs of 1 to 3 rows, the first 1 100 of one row, every eleventh without pooled rows."""
    if name not in _DATASETS:
        if name in ("k1", "k11"):
            sizes = _rng("sizes").integers(1, 41, size=40)
            sizes[[0, 3, 5]] = (1, 2, 40)
            K, ld, nt = (1, 3, 1) if name == "k1" else (11, 12, 3)
            _DATASETS[name] = batch_dataset(name, sizes, K, ld, nt, SMALL_UNPOOLED)
        else:
            sizes = np.concatenate([np.ones(1100, dtype=np.int64), _rng("many").integers(2, 4, size=1100)])
            _DATASETS[name] = batch_dataset(name, sizes, 1, 1, 1, tuple(range(0, 2200, 11)))
    return _DATASETS[name]


def totals(D, ids):
    """(n_row, n_nnz, n_tile, n_mem) of the batch of graphs `ids`."""
    ids = np.asarray(ids, dtype=np.int64)
    return tuple(int((D[k][ids + 1] - D[k][ids]).sum()) for k in ("g_row", "g_nnz", "g_tile", "g_mem"))


def capacities(tot, B, mode):
    """(R_cap, E_cap, T_cap, M_cap) of a capacity mode, from the batch's totals:
         exact    all four at the totals (M_cap 1 when the batch pools no row): no tail tile, rowptr[R_cap] still written
         r1 / r16 / r17   R_cap - n_row = 1 / 16 / 17 with T_cap exactly n_tile + ceil((R_cap - n_row) / 16); E_cap, M_cap a little over
         t_over   R_cap - n_row = 17 and T_cap seven tiles over what the tail needs (tiles with r0 >= R_cap)
         e_big / t_big / m_big   that capacity the largest of the five item counts that size the grid (R_cap + 1, E_cap, T_cap, M_cap,
                  B + 1), beyond the next multiple of 256."""
    n_row, n_nnz, n_tile, n_mem = tot
    if mode == "exact":
        return n_row, n_nnz, n_tile, max(n_mem, 1)
    dr = {"r1": 1, "r16": 16, "r17": 17}.get(mode, 17)
    R, E, M = n_row + dr, n_nnz + 3, n_mem + 2
    T = n_tile + (dr + TILE_ROWS - 1) // TILE_ROWS
    if mode == "t_over":
        T += 7
    big = (max(R + 1, E, T, M, B + 1) + 255) // 256 * 256 + 44
    if mode == "e_big":
        E = big
    elif mode == "t_big":
        T = big
    elif mode == "m_big":
        M = big
    return R, E, T, M


def pick(D, B, first_unpooled=True, last_unpooled=True, seed=0):
    """B graphs of D in a random order; with B >= 2 the first / the last is a graph without pooled rows when asked."""
    rng = _rng("pick", B, seed)
    un = [g for g in range(D["G"]) if D["g_mem"][g + 1] == D["g_mem"][g]]
    ids = [int(g) for g in rng.permutation(D["G"]) if g not in un[:2]][:B]
    if B >= 2 and first_unpooled:
        ids[0] = un[0]
    if B >= 2 and last_unpooled:
        ids[-1] = un[1]
    return ids


# name -> (dataset, B, ids, capacity mode, zero_rows, optional outputs given, ld_ax - K)
def batch_cases():
    cases = {}
    k1, k11, many = dataset("k1"), dataset("k11"), dataset("many")
    un = SMALL_UNPOOLED
    cases["B1-exact"] = ("k1", 1, [5], "exact", 256, True, 1)
    cases["B1-unpooled-r1"] = ("k11", 1, [un[0]], "r1", 1, True, 5)
    cases["B2-r16"] = ("k11", 2, [un[0], 7], "r16", 256, True, 0)
    cases["B2-unpooled-last-exact"] = ("k1", 2, [5, un[1]], "exact", 1, True, 0)
    cases["B5-r17"] = ("k11", 5, pick(k11, 5), "r17", 256, True, 5)
    cases["B5-t_over"] = ("k1", 5, pick(k1, 5, seed=1), "t_over", 1, True, 1)
    cases["B5-no-optional"] = ("k11", 5, pick(k11, 5, seed=2), "r17", 0, False, 1)
    cases["B16-exact"] = ("k11", 16, pick(k11, 16), "exact", 256, True, 0)
    cases["B16-r1"] = ("k1", 16, pick(k1, 16, seed=3), "r1", 256, True, 2)
    cases["B16-e_big"] = ("k11", 16, pick(k11, 16, seed=4), "e_big", 256, True, 1)
    cases["B16-t_big"] = ("k1", 16, pick(k1, 16, seed=5), "t_big", 256, True, 0)
    cases["B16-m_big"] = ("k11", 16, pick(k11, 16, seed=6), "m_big", 1, True, 0)
    cases["B1024-one-row-exact"] = ("many", 1024, list(range(1024)), "exact", 256, True, 0)
    cases["B1024-mixed-r17"] = ("many", 1024, [int(g) for g in _rng("b1024").permutation(many["G"])[:1024]], "r17", 256, True, 1)
    return cases


def three_steps():
    """(dataset, B, perm of 3 B graphs, capacities): the middle batch is the largest and the capacities are its totals with one row
    to spare, so the first and the last batch leave rows, entries, tiles and pooled rows of the middle one to overwrite."""
    D = dataset("k11")
    B = 5
    order = [int(g) for g in np.argsort(np.diff(D["g_row"]), kind="stable") if g not in SMALL_UNPOOLED]
    mid, small = order[-B:], order[:-B]
    perm = small[:B] + mid + [SMALL_UNPOOLED[0]] + small[B:2 * B - 2] + [SMALL_UNPOOLED[1]]
    assert len(perm) == 3 * B and len(set(perm)) == 3 * B
    caps = capacities(totals(D, mid), B, "r1")
    for s in range(3):
        assert all(t <= c for t, c in zip(totals(D, perm[s * B:(s + 1) * B]), caps))
    return "k11", B, perm, caps


def run_steps(D, B, perm, caps, ld_ax, zero_rows, losses, n_steps=3, refill_before=(0, 1), slip=None, optional=True):
    """What `n_steps` consecutive offsets + gather launches leave: a list of (step_idx, loss_slot, loss_sum, off, gid, buffers) after
    each step.  The buffers are refilled with the sentinels before the steps in `refill_before` only; losses[s] is what the step's loss
    kernel would have left in loss_slot before step s."""
    step, slot, lsum = 0, np.float32(0), np.float32(0)
    bufs, out = None, []
    for s in range(n_steps):
        if s in refill_before:
            bufs = fresh_buffers(B, *caps, ld_ax, D["n_tgt"])
        slot = np.float32(losses[s])
        off, gid = batch_offsets(perm, step, B, D["g_row"], D["g_nnz"], D["g_tile"], D["g_mem"])
        step, slot, lsum = offsets_state(step, slot, lsum, slip)
        bufs = batch_gather(B, off, gid, D, *caps, D["K"], ld_ax, D["n_tgt"], zero_rows, bufs, optional, slip)
        out.append((step, slot, lsum, off, gid, bufs))
    return out


# ---- GCN normalisation ----
GCN_LENGTHS = (3, 0, 1, 4, 5, 63, 64, 65, 68, 129, 300)
GCN_N_ROWS = (1, 4, 5, 256, 257)
GCN_EXACT_LENGTHS = (0, 1, 4, 16, 64, 256)


def gcn_case(n_rows):
    """rowptr of 257 rows -- GCN_LENGTHS, then lengths 0 to 6 -- cut to its first n_rows rows, with arbitrary columns below n_rows
    (rows 1 and every later empty row among them) and w uniform in [0.5, 2]."""
    rng = _rng("gcn", n_rows)
    lengths = np.concatenate([GCN_LENGTHS, _rng("gcn-lengths").integers(0, 7, size=257 - len(GCN_LENGTHS))])[:n_rows]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    nnz = int(rowptr[-1])
    col = rng.integers(0, n_rows, size=nnz).astype(np.int32)
    if n_rows >= 4:
        col[::7] = 1                                # an empty row as a column
    return rowptr, col, rng.uniform(0.5, 2.0, size=nnz).astype(np.float32)


def gcn_exact_case():
    """Row lengths 0, 1, 4, 16, 64, 256, three times over in mixed order, unweighted: every degree is 0 or a power of four, every dinv
    0 or a power of two, every val a product of two of them."""
    rng = _rng("gcn-exact")
    lengths = rng.permutation(np.repeat(GCN_EXACT_LENGTHS, 3))
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return rowptr, rng.integers(0, len(lengths), size=int(rowptr[-1])).astype(np.int32)


def gcn_nonpositive_case():
    """Five rows with signed weights: row 1 sums to exactly 0, row 3 to -1.5, rows 0, 2, 4 are positive; every row has entries in
    columns 1 and 3."""
    rowptr = np.asarray([0, 3, 7, 10, 12, 15], dtype=np.int32)
    col = np.asarray([0, 1, 3, 1, 0, 3, 2, 1, 2, 3, 3, 1, 4, 1, 3], dtype=np.int32)
    w = np.asarray([1.0, 2.0, 0.5, 1.5, -2.0, 1.0, -0.5, 0.25, 2.0, 1.0, -2.0, 0.5, 1.0, 1.0, 0.75], dtype=np.float32)
    return rowptr, col, w
