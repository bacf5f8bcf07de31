"""The references of tests/assemble_reference.py checked without a GPU, and the inputs of tests/test_gpu_assemble_kernels.py shown
to discriminate.

* induced_edges == data.assemble_subgraphs_torch on CPU tensors (the chunked torch path tests/test_host_logic.py ties to the NumPy
  and oracle constructions), element for element including order, over layout x extra_node x clusters.
* batch_offsets / batch_gather: the in-batch part == a brute-force build (scipy.sparse.block_diag of the chosen graphs' CSR blocks,
  the concatenated pooled-row lists, the row-stacked ax and tgt).
* gcn_norm_csr == oracle/gnn_oracle.gcn_norm in float64.
* Every slip of assemble_reference.SLIPS, applied to the REFERENCE, changes the expected output of the GPU cases that are said to
  catch it (expected_*_kills below, written from the construction of the cases), and every slip is caught by at least one case: a
  kernel making that mistake would fail that GPU case.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import assemble_reference as ar


def _differs(a, b):
    return not np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == "f")


# ---------------------------------------------------------------------------------------------------------------------------------
# the references against independent constructions
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subset", [False, True], ids=["all", "subset"])
@pytest.mark.parametrize("extra", [True, False], ids=["extra", "own"])
@pytest.mark.parametrize("layout", ["sorted", "star"])
def test_induced_edges_equal_the_cpu_torch_path(layout, extra, subset):
    from fitgnn_amd import data

    ei, N, assign, n, clusters = ar.partitioned_graph()
    res = data.assemble_subgraphs_torch(torch.from_numpy(ei), N, assign, n, extra_node=extra, layout=layout,
                                        clusters=clusters if subset else None, chunk_rows=257)
    res = {k: v.numpy() for k, v in res.items()}
    inp = ar.kernel_inputs_of(res, ei, N)
    assert (inp["inv"] is not None) == (layout == "star" and extra)   # (own nodes alone are ascending in both layouts)
    cnt, e_src, e_dst = ar.induced_edges(**inp)
    assert np.array_equal(np.stack([e_src, e_dst]), res["edge_index"])
    assert np.array_equal(cnt, np.bincount(res["edge_index"][0], minlength=len(inp["row_node"])))
    assert len(e_src) > 0
    assert np.diff(inp["adj_ptr"]).max() >= 130                       # the hub: three chunks
    if not subset and not extra:                                      # singleton clusters are there
        assert (np.diff(res["ptr"]) == 1).sum() >= 10


def _brute_batch(D, ids):
    """The batch of graphs `ids` built the long way round."""
    blocks, members, ax, tgt, pooled, row0 = [], [], [], [], [], 0
    for g in ids:
        r0, r1, e0 = int(D["g_row"][g]), int(D["g_row"][g + 1]), int(D["g_nnz"][g])
        rp = D["rowptr"][r0:r1 + 1].astype(np.int64) - e0
        blocks.append(sp.csr_matrix((D["val"][e0:e0 + rp[-1]], D["col"][e0:e0 + rp[-1]].astype(np.int64) - r0, rp), shape=(r1 - r0, r1 - r0)))
        members.append(D["mem"][D["g_mem"][g]:D["g_mem"][g + 1]].astype(np.int64) - r0 + row0)
        ax.append(D["ax"][r0:r1, :D["K"]])
        pooled.append(D["pooled"][r0:r1])
        tgt.append(D["tgt"][g])
        row0 += r1 - r0
    A = sp.block_diag(blocks, format="csr")
    A.sort_indices()
    return A, members, np.concatenate(ax), np.stack(tgt), np.concatenate(pooled)


@pytest.mark.parametrize("name", list(ar.batch_cases()))
def test_batch_reference_equals_a_brute_force_build(name):
    ds, B, ids, mode, zero_rows, optional, pad = ar.batch_cases()[name]
    D = ar.dataset(ds)
    caps = R_cap, E_cap, T_cap, M_cap = ar.capacities(ar.totals(D, ids), B, mode)
    ld_ax = D["K"] + pad
    perm = np.asarray([0] * B + list(ids), dtype=np.int64)             # the batch is step 1 of this permutation
    off, gid = ar.batch_offsets(perm, 1, B, D["g_row"], D["g_nnz"], D["g_tile"], D["g_mem"])
    assert np.array_equal(gid, ids) and tuple(off[:, B]) == ar.totals(D, ids)
    O = ar.batch_gather(B, off, gid, D, *caps, D["K"], ld_ax, D["n_tgt"], zero_rows, ar.fresh_buffers(B, *caps, ld_ax, D["n_tgt"]),
                        optional)
    A, members, ax, tgt, pooled = _brute_batch(D, ids)
    n_row, n_nnz, n_tile, n_mem = ar.totals(D, ids)
    assert A.shape[0] == n_row and A.nnz == n_nnz
    assert np.array_equal(O["rowptr"][:n_row + 1], A.indptr) and np.all(O["rowptr"][n_row:R_cap + 1] == n_nnz)
    assert np.array_equal(O["col"][:n_nnz], A.indices) and np.array_equal(O["val"][:n_nnz], A.data)
    allm = np.concatenate(members)
    assert np.array_equal(O["members"][:n_mem], allm) and np.array_equal(allm, np.flatnonzero(pooled))
    seg = np.repeat(np.arange(B), [len(m) for m in members])
    want_seg = np.full(n_row, -1)
    want_seg[allm] = seg
    assert np.array_equal(O["seg_of_row"][:n_row], want_seg)
    assert np.array_equal(O["seg_off"][:B + 1], np.concatenate([[0], np.cumsum([len(m) for m in members])]))
    assert np.array_equal(O["inv_cnt"][:B], (1.0 / np.maximum([len(m) for m in members], 1)).astype(np.float32))
    assert np.array_equal(O["ax"][:R_cap * ld_ax].reshape(R_cap, ld_ax)[:n_row, :D["K"]], ax)
    assert np.array_equal(O["tgt"][:B * D["n_tgt"]].reshape(B, -1), tgt)
    if optional:
        assert np.array_equal(O["members64"][:n_mem], allm) and np.array_equal(O["cseg"][:n_mem], seg)
        assert np.array_equal(O["pos"][:n_row][allm], np.arange(n_mem))
        rest = np.setdiff1d(np.arange(R_cap), allm)
        assert np.array_equal(O["pos"][rest], M_cap + rest % max(zero_rows, 1))
    else:
        assert np.all(O["members64"] == ar.I64_SENTINEL) and np.all(O["cseg"] == ar.I32_SENTINEL) and np.all(O["pos"] == ar.I32_SENTINEL)
    # the tiles: a partition of [0, R_cap) whose entry ranges are the row pointer's, empty past it; nothing past a capacity is written
    t = O["tiles"][:T_cap]
    assert ar.live_tiles_partition(t, R_cap)
    live = t[t[:, 1] > t[:, 0]]
    assert np.array_equal(live[:, 4], O["rowptr"][live[:, 0]]) and np.array_equal(live[:, 5], O["rowptr"][live[:, 1]])
    assert not t[t[:, 1] <= t[:, 0]].any()
    for k, cap in (("rowptr", R_cap + 1), ("col", E_cap), ("members", M_cap), ("seg_of_row", R_cap), ("seg_off", B + 1), ("cseg", M_cap)):
        assert np.all(O[k][cap:] == ar.I32_SENTINEL), k
    assert np.all(O["tiles"][T_cap:] == ar.I32_SENTINEL) and np.isnan(O["val"][E_cap:]).all() and np.isnan(O["ax"][R_cap * ld_ax:]).all()
    if pad:
        assert np.isnan(O["ax"][:R_cap * ld_ax].reshape(R_cap, ld_ax)[:, D["K"]:]).all()


def test_three_step_reference_leaves_nothing_of_the_larger_batch():
    ds, B, perm, caps = ar.three_steps()
    D = ar.dataset(ds)
    steps = ar.run_steps(D, B, perm, caps, D["K"] + 1, 256, losses=(3, 5, 7))
    assert [s[0] for s in steps] == [1, 2, 3] and [float(s[2]) for s in steps] == [3.0, 8.0, 15.0] and all(float(s[1]) == 0.0 for s in steps)
    tot = [ar.totals(D, perm[s * B:(s + 1) * B]) for s in range(3)]
    assert all(tot[1][k] > tot[0][k] and tot[1][k] > tot[2][k] for k in range(4))        # the middle batch is the largest
    alone = ar.run_steps(D, B, perm[2 * B:], caps, D["K"] + 1, 256, losses=(0,), n_steps=1)[0][5]
    for k, v in steps[2][5].items():                                                    # step 3 over step 2 == step 3 over sentinels
        assert not _differs(v, alone[k]), k


def test_gcn_reference_equals_the_oracle():
    from oracle import gnn_oracle

    rng = np.random.default_rng(5)
    n = 60
    a, b = rng.integers(0, n - 3, size=200), rng.integers(0, n - 3, size=200)            # (the last three nodes keep only their loop)
    keep = a != b
    ei = np.unique(np.concatenate([np.stack([a, b], 1)[keep], np.stack([b, a], 1)[keep]]), axis=0).T
    row, col, w = gnn_oracle.gcn_norm(torch.from_numpy(ei), n, torch.float64)
    # the kernel's CSR: rows = targets, columns = sources, self loops already in
    order = np.lexsort((row.numpy(), col.numpy()))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(col.numpy(), minlength=n))]).astype(np.int32)
    val, dinv, aval, adeg = ar.gcn_norm_csr(rowptr, row.numpy()[order].astype(np.int32), None)
    np.testing.assert_allclose(val, w.numpy()[order], rtol=1e-15, atol=0)
    np.testing.assert_allclose(dinv, np.diff(rowptr) ** -0.5, rtol=1e-15)
    assert np.array_equal(aval, np.abs(val)) and np.array_equal(adeg, np.diff(rowptr))


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs discriminate
# ---------------------------------------------------------------------------------------------------------------------------------
INDUCED_SLIPS = ("first_chunk_only", "drop_lane_63", "no_hi_guard", "ignore_inv")
BATCH_SLIPS = ("find_first", "tile_not_clipped", "tile_past_rcap", "rowptr_rcap_missing", "inv_cnt_no_clamp", "col_rebase_nnz", "stale_left")
GCN_SLIPS = ("gcn_row_64", "gcn_ignore_w", "gcn_empty_dinv_one")
_caught = {}       # slip -> the cases that catch it (filled by the tests below, read by the last one)


def _note(slip, case, changed, expected):
    if expected:
        assert changed, f"{case} does not notice: {ar.SLIPS[slip]}"
    if changed:
        _caught.setdefault(slip, []).append(case)


def expected_induced_kills(n_rows, with_inv):
    """Row 0 (node 146): its only first-chunk hit sits on lane 63 and its second chunk has hits; row 1 (node 21 in cluster 3) lists
    140, the first member of the run behind cluster 3's; inv is a random permutation of 363 positions."""
    kills = {"first_chunk_only", "drop_lane_63"}
    if n_rows is None or n_rows >= 3:
        kills.add("no_hi_guard")
    if with_inv:
        kills.add("ignore_inv")
    return kills


@pytest.mark.parametrize("with_inv", [False, True], ids=["key", "inv"])
@pytest.mark.parametrize("n_rows", ar.INDUCED_N_ROWS, ids=lambda v: f"rows{v}")
def test_induced_case_discriminates(n_rows, with_inv):
    c = ar.induced_case()
    assert set(c["lengths"][140:150]) == {0, 1, 2, 63, 64, 65, 127, 128, 129, 200}
    assert sorted(np.diff(c["cl_ptr"])) == [0, 1, 2, 3, 100, 257]
    n = len(c["row_node"]) if n_rows is None else n_rows
    args = (c["adj_ptr"], c["adj"], c["row_node"][:n], c["row_cluster"][:n], c["cl_ptr"], c["key_node"], c["inv"] if with_inv else None)
    ref = ar.induced_edges(*args)
    assert int(ref[0].sum()) == len(ref[1]) > 0
    kills = expected_induced_kills(n_rows, with_inv)
    for slip in INDUCED_SLIPS:
        got = ar.induced_edges(*args, slip=slip)
        _note(slip, f"induced-rows{n_rows}-{'inv' if with_inv else 'key'}", any(_differs(g, r) for g, r in zip(got, ref)), slip in kills)


def test_induced_case_holds_every_chunk_pattern():
    """Per 64-chunk of the lists of cluster 5's rows: no hit, only lane 0, only lane 63, all 64, a sparse pattern."""
    c = ar.induced_case()
    members = set(range(140, 397))
    seen = set()
    for x in range(140, 150):
        lst = c["adj"][c["adj_ptr"][x]:c["adj_ptr"][x + 1]]
        for b in range(0, len(lst), 64):
            hits = [j for j, y in enumerate(lst[b:b + 64]) if int(y) in members]
            seen.add("none" if not hits else "lane0" if hits == [0] else "lane63" if hits == [63] else "all" if len(hits) == 64 else "sparse")
    assert seen == {"none", "lane0", "lane63", "all", "sparse"}
    lst21 = [int(y) for y in c["adj"][c["adj_ptr"][21]:c["adj_ptr"][22]]]
    run3 = c["key_node"][c["cl_ptr"][3]:c["cl_ptr"][4]]
    assert min(lst21) < run3[0] and max(lst21) > run3[-1] and run3[0] in lst21 and run3[-1] in lst21
    assert c["key_node"][c["cl_ptr"][4]] == 140 and 140 in lst21 and c["cl_ptr"][4] == c["cl_ptr"][5]      # behind an empty cluster
    assert (c["key_node"] == 21).sum() == 2


def expected_batch_kills(name):
    ds, B, ids, mode, zero_rows, optional, pad = ar.batch_cases()[name]
    D = ar.dataset(ds)
    unpooled = [D["g_mem"][g + 1] == D["g_mem"][g] for g in ids]
    kills = {"rowptr_rcap_missing"}                                   # rowptr[R_cap] is an element of every case
    if any(u and not all(unpooled[i + 1:]) for i, u in enumerate(unpooled[:-1])):
        kills.add("find_first")                                       # pooled rows behind a graph that has none
    if any(unpooled):
        kills.add("inv_cnt_no_clamp")
    if mode != "exact":
        kills.add("stale_left")
        if mode != "r16":
            kills.add("tile_not_clipped")                             # 1 or 17 rows past the batch: the last tail tile holds one row
    if mode in ("t_over", "t_big"):
        kills.add("tile_past_rcap")
    tot = np.cumsum([ar.totals(D, [g])[:2] for g in ids], 0)
    if any(r != e for r, e in tot[:-1]):
        kills.add("col_rebase_nnz")                                   # a graph behind others whose rows and entries differ in number
    return kills


@pytest.mark.parametrize("name", list(ar.batch_cases()))
def test_batch_case_discriminates(name):
    ds, B, ids, mode, zero_rows, optional, pad = ar.batch_cases()[name]
    D = ar.dataset(ds)
    caps = ar.capacities(ar.totals(D, ids), B, mode)
    ld_ax = D["K"] + pad
    off, gid = ar.batch_offsets(np.asarray(ids, dtype=np.int64), 0, B, D["g_row"], D["g_nnz"], D["g_tile"], D["g_mem"])
    run = lambda slip: ar.batch_gather(B, off, gid, D, *caps, D["K"], ld_ax, D["n_tgt"], zero_rows,       # noqa: E731
                                       ar.fresh_buffers(B, *caps, ld_ax, D["n_tgt"]), optional, slip)
    ref = run(None)
    kills = expected_batch_kills(name)
    for slip in BATCH_SLIPS:
        got = run(slip)
        _note(slip, name, any(_differs(got[k], ref[k]) for k in ref), slip in kills)


def test_three_steps_discriminate():
    ds, B, perm, caps = ar.three_steps()
    D = ar.dataset(ds)
    ref = ar.run_steps(D, B, perm, caps, D["K"] + 1, 256, losses=(3, 5, 7))
    for slip in ("step_not_advanced", "stale_left", "find_first", "inv_cnt_no_clamp"):
        got = ar.run_steps(D, B, perm, caps, D["K"] + 1, 256, losses=(3, 5, 7), slip=slip)
        changed = any(g[0] != r[0] or any(_differs(g[5][k], r[5][k]) for k in r[5]) for g, r in zip(got, ref))
        _note(slip, "three-steps", changed, True)
    # stale entries: step 3 alone (written over what step 2 left, no sentinel in between) notices
    got = ar.run_steps(D, B, perm, caps, D["K"] + 1, 256, losses=(3, 5, 7), slip="stale_left")
    assert any(_differs(got[2][5][k], ref[2][5][k]) for k in ("col", "val", "members", "seg_of_row", "ax"))


def test_gcn_cases_discriminate():
    cases = {f"gcn-rows{n}": ar.gcn_case(n) for n in ar.GCN_N_ROWS}
    cases["gcn-exact"] = ar.gcn_exact_case() + (None,)
    cases["gcn-nonpositive"] = ar.gcn_nonpositive_case()
    for name, (rowptr, col, w) in cases.items():
        lengths = np.diff(rowptr)
        kills = set()
        if lengths.max() > 64:
            kills.add("gcn_row_64")
        if w is not None:
            kills.add("gcn_ignore_w")
        if name != "gcn-rows1":
            kills.add("gcn_empty_dinv_one")                           # an entry in the column of a row of degree <= 0
        ref = ar.gcn_norm_csr(rowptr, col, w)
        assert not np.isnan(ref[0]).any()
        for slip in GCN_SLIPS:
            got = ar.gcn_norm_csr(rowptr, col, w, slip)
            _note(slip, name, _differs(got[0], ref[0]) or _differs(got[1], ref[1]), slip in kills)
    assert set(np.diff(ar.gcn_case(257)[0])[:11]) == set(ar.GCN_LENGTHS)
    rowptr, col = ar.gcn_exact_case()
    assert set(np.diff(rowptr)) == set(ar.GCN_EXACT_LENGTHS)
    rowptr, col, w = ar.gcn_nonpositive_case()
    deg = np.add.reduceat(w.astype(np.float64), rowptr[:-1])
    assert deg[1] == 0 and deg[3] < 0 and (deg[[0, 2, 4]] > 0).all()


def test_every_slip_is_caught_by_some_gpu_case():
    """The union of what the cases above notice is the whole list (run on its own, this test goes through the cases itself)."""
    if set(ar.SLIPS) - set(_caught):
        for n_rows in ar.INDUCED_N_ROWS:
            test_induced_case_discriminates(n_rows, True)
        for name in ar.batch_cases():
            test_batch_case_discriminates(name)
        test_three_steps_discriminate()
        test_gcn_cases_discriminate()
    missing = [s for s in ar.SLIPS if s not in _caught]
    assert not missing, f"no GPU case notices: {[ar.SLIPS[s] for s in missing]}"
