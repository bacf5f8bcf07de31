"""GPU tier: the assembly kernels of csrc/assemble.hip (fitgnn_induced_edges_count / _fill, fitgnn_batch_offsets,
fitgnn_batch_gather) and the GCN normalisation of csrc/gcn_ops.hip (fitgnn_gcn_norm_csr_f32: gcn_deg_kernel, gcn_val_kernel) through
the C ABI against the plain references of tests/assemble_reference.py, with the helpers of tests/test_gpu_step_kernels.py.

Every output buffer is a few elements longer than its capacity and holds a sentinel before each launch (NaN in floats, 0x5A5A5A5A in
integers), so "written everywhere inside, nowhere outside" is part of every comparison; integer results are compared with
np.array_equal.  The inputs are built in tests/assemble_reference.py, and tests/test_assemble_reference_cpu.py shows on the same
inputs, without a GPU, that each of the mistakes listed there (assemble_reference.SLIPS) would change the expected output of at
least one case below.

Launcher -> branch -> tests that reach it:

| launcher | branch (from the launch code and the kernel) | tests |
|---|---|---|
| fitgnn_induced_edges_count | grid = ceil(64 n_rows / 256): n_rows = 1, 3, 4, 5, 363 (the last workgroup holds 1, 3, 4, 1, 3 live waves; `r >= n_rows` retires the others) | test_induced_edges[rows*] |
| (induced_edges_kernel<false>) | chunk loop: lists of 0 (no trip), 1, 2, 63, 64 (one full chunk), 65, 127, 128, 129 and 200 entries; `k < a1` on the last chunk | test_induced_edges (cluster 5's rows 140 ... 149) |
| | ballot per chunk: no hit, only lane 0, only lane 63, all 64, sparse; `total` over several chunks; lane 0 writes cnt | test_induced_edges |
| | find_member: runs of 1, 2, 3, 100, 257 members and an empty cluster between two others; y below every member, above every member (lo ends at hi: the `p < hi` guard, with the next run's first member equal to y, and at the very end of key_node), equal to the first / the last member, a member of the following cluster only; a node that is a row of two clusters | test_induced_edges (rows of node 21, 10, 5, 148) |
| | n_rows = 0 returns 0 and touches nothing; n_rows < 0, any NULL array refused | test_induced_edges_refusals |
| fitgnn_induced_edges_fill | the same grid and chunk loop with `out` from off[r]; prefix popcount below the lane (lane 0: none, lane 63: 63 bits); `out += popc(m)` between chunks; a neighbour listed twice is emitted twice; order = (row, position in the list) | test_induced_edges[*] |
| (induced_edges_kernel<true>) | inv NULL (key positions) / a random permutation | test_induced_edges[*-key / *-inv] |
| | nothing behind off[n_rows] written | test_induced_edges |
| | n_rows = 0, n_rows < 0, NULL arrays (inv may be NULL) | test_induced_edges_refusals |
| both, as data.assemble_subgraphs_torch calls them | layout sorted / star (inv) x extra_node x clusters None / a subset, on a 600-node graph with a hub of degree >= 130 (three chunks), a duplicated edge and singleton clusters: the CUDA path == the CPU path, torch.equal on every tensor | test_torch_path_equals_cpu_path |
| fitgnn_batch_offsets | B = 1, 2, 5, 16, 1024 (threads i >= B scan zeros; the 10 Hillis-Steele rounds at full width); off[k][B] by thread B - 1; gid | test_batch_case[*] |
| (batch_offsets_kernel) | step_idx read and advanced (0 -> 3), the batch taken at perm[step B] | test_three_steps_over_one_permutation |
| | loss_slot and loss_sum given: sum += slot, slot cleared; one of them NULL: the other untouched | test_three_steps_over_one_permutation, test_loss_hand_over_needs_both |
| | B = 0, 1025, NULL required arrays refused | test_batch_refusals |
| fitgnn_batch_gather | grid = ceil(max(R_cap + 1, E_cap, T_cap, M_cap, B + 1) / 256): each of the five the largest in turn (R_cap + 1 in most cases; E_cap, T_cap, M_cap: B16-e_big / t_big / m_big; B + 1 == R_cap + 1: B1024-one-row-exact) | test_batch_case[*] |
| (batch_gather_kernel) | rows: idx < n_row (batch_find over o_row, pooled / not, pos given / NULL, K = 1 / 11 columns, ld_ax_g > K, ld_ax >= K: padding untouched); n_row <= idx < R_cap (rowptr = n_nnz, seg_of_row = -1, pos = M_cap + idx % zero_rows with zero_rows 1 / 256, ax row zero); idx == R_cap (rowptr only), also with R_cap == n_row | test_batch_case[*] |
| | entries: idx < n_nnz (column re-based by o_row - g_row) / the zeros up to E_cap | test_batch_case[*] |
| | tiles: the graphs' own, moved by rows and entries; tail tiles of 16 rows: none (exact), one of 1 row (r1), one of 16 (r16), 16 + 1 (r17: the clip at R_cap), T_cap exactly n_tile + ceil((R_cap - n_row) / 16) and seven / many over it (r0 >= R_cap: all-zero tiles) | test_batch_case[*], test_assembled_batch_multiplies_like_the_host_built_one |
| | pooled rows: idx < n_mem with batch_find stepping over graphs without pooled rows (first, in the middle, last in the batch; a whole batch of one such graph) / 0 and -1 up to M_cap; members64, cseg NULL / given | test_batch_case[*], test_batch_case[B5-no-optional] |
| | per graph: seg_off (B + 1), inv_cnt with cnt = 0 clamped to 1, n_tgt = 1 / 3 targets | test_batch_case[*] |
| | every in-capacity element rewritten by every launch: a smaller batch over the remains of a larger one, no sentinel refill | test_three_steps_over_one_permutation |
| | the assembled tiles partition [0, R_cap); a product over them == the product over the host-built batch, zeros behind it | test_batch_case[*], test_assembled_batch_multiplies_like_the_host_built_one |
| | as graph_data.PaddedBatchPlan sizes it: T_cap covers caps[2] own tiles + the longest tail; the batch of the 16 smallest graphs assembled | test_plan_tile_capacity_covers_the_longest_tail |
| | B = 0, 1025; a capacity 0; K, n_tgt 0; ld_ax_g, ld_ax < K; b_pos with mem_rank NULL or zero_rows < 1; NULL required arrays | test_batch_refusals |
| fitgnn_gcn_norm_csr_f32 | gcn_deg_kernel: grid ceil(n / 256) with n = 1, 4, 5, 256 (one full workgroup), 257 (a second with one live thread); w NULL (row length) / given (running sum); d > 0 / d <= 0 (empty row, weights summing to 0 and below) | test_gcn_norm_weighted[n*], test_gcn_norm_exact, test_gcn_norm_nonpositive_degree |
| | gcn_val_kernel: grid ceil(64 n / 256) (n = 1, 5: one live wave in the last workgroup); rows of 0, 1, 3, 4, 5, 63, 64 entries (one trip at most), 65, 68, 129, 300 (the e += 64 stride: 2, 2, 3, 5 trips); w NULL / given; nothing behind nnz written | test_gcn_norm_weighted[n*], test_gcn_norm_exact |
| | two launches give the same bits | test_gcn_norm_weighted |
| | n_rows = 0 returns 0; n_rows < 0, NULL rowptr / col / val / dinv refused (w may be NULL) | test_gcn_norm_refusals |

The bound that is not bit-exact (u = 2^-24): the weighted normalisation.  gcn_deg_kernel adds a row's L weights into one running
fp32 sum: L - 1 roundings, each at most u of a partial sum that is at most the row's sum of |w|, so deg is within
(L - 1) u sum|w| = (L - 1) u c deg with c = sum|w| / |deg| (1 for the positive weights of the RANDOM case).  sqrtf and the division
1.0f / x are the correctly rounded IEEE operations (one rounding each), so dinv = deg^-1/2 carries a relative error of at most
e = ((L - 1) c / 2 + 2) u.  gcn_val_kernel forms (dinv[row] * w) * dinv[col]: two products, one rounding each, on top of the two
dinv errors carried in: |val - ref| <= k u |ref| with k = (L_row - 1) c_row / 2 + (L_col - 1) c_col / 2 + 6, and the sum of |terms|
of an entry is |ref| itself (one term).  Both bounds are multiplied by (1 + k u) for the products of the first-order terms.
Worst observed error / bound on one MI355X run (test_gcn_norm_weighted prints them with -s), n = 1 / 4 / 5 / 256 / 257:
val 0.28 / 0.19 / 0.36 / 0.46 / 0.39, dinv 0.33 / 0.26 / 0.48 / 0.66 / 0.62.
"""
import numpy as np
import pytest
import torch

import assemble_reference as ar
from test_gpu_step_kernels import E_BADARG, L, U, _call, _dev, _p, _rng, _run, _same, _strided, _within  # noqa: F401

pytestmark = pytest.mark.gpu

I32, I64, F32 = torch.int32, torch.int64, torch.float32


def _sent(n, dtype):
    """A device buffer of n elements holding the sentinel of its type."""
    if dtype == F32:
        return torch.full((n,), float("nan"), dtype=F32, device="cuda")
    return torch.full((n,), ar.I32_SENTINEL if dtype == I32 else ar.I64_SENTINEL, dtype=dtype, device="cuda")


def _host(t):
    return t.detach().cpu().numpy()


def _equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = np.array_equal(got, want, equal_nan=got.dtype.kind == "f")
    if not ok:
        bad = np.argwhere(~((got == want) | ((got != got) & (want != want)) if got.dtype.kind == "f" else got == want))
        raise AssertionError(f"{what}: {len(bad)} elements differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


# ---------------------------------------------------------------------------------------------------------------------------------
# induced edges
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def induced():
    c = ar.induced_case()
    dev = {k: _dev(c[k], I64) for k in ("adj_ptr", "adj", "row_node", "row_cluster", "cl_ptr", "key_node", "inv")}
    return c, dev


@pytest.mark.parametrize("with_inv", [False, True], ids=["key", "inv"])
@pytest.mark.parametrize("n_rows", ar.INDUCED_N_ROWS, ids=lambda v: f"rows{v}")
def test_induced_edges(L, induced, n_rows, with_inv):
    c, d = induced
    n = len(c["row_node"]) if n_rows is None else n_rows
    cnt_ref, src_ref, dst_ref = ar.induced_edges(c["adj_ptr"], c["adj"], c["row_node"][:n], c["row_cluster"][:n], c["cl_ptr"], c["key_node"],
                                                 c["inv"] if with_inv else None)
    head = (_p(L, d["adj_ptr"]), _p(L, d["adj"]), _p(L, d["row_node"]), _p(L, d["row_cluster"]), _p(L, d["cl_ptr"]), _p(L, d["key_node"]))
    cnt = _sent(n + 4, I32)
    _run(L, "fitgnn_induced_edges_count", *head, n, _p(L, cnt))
    _equal(_host(cnt), np.concatenate([cnt_ref, np.full(4, ar.I32_SENTINEL, dtype=np.int32)]), "cnt")
    off = np.concatenate([[0], np.cumsum(cnt_ref)]).astype(np.int64)          # the reference's scan: the fill is judged on its own
    n_e = int(off[-1])
    off_t = _dev(off, I64)
    e_src, e_dst = _sent(n_e + 4, I64), _sent(n_e + 4, I64)
    _run(L, "fitgnn_induced_edges_fill", *head, _p(L, d["inv"]) if with_inv else None, n, _p(L, off_t), _p(L, e_src), _p(L, e_dst))
    tail = np.full(4, ar.I64_SENTINEL, dtype=np.int64)
    _equal(_host(e_src), np.concatenate([src_ref, tail]), "e_src")
    _equal(_host(e_dst), np.concatenate([dst_ref, tail]), "e_dst")


def test_induced_edges_refusals(L, induced):
    c, d = induced
    names = ("adj_ptr", "adj", "row_node", "row_cluster", "cl_ptr", "key_node")
    head = [_p(L, d[k]) for k in names]
    cnt = _sent(8, I32)
    off_t = torch.zeros(8, dtype=I64, device="cuda")
    e_src, e_dst = _sent(8, I64), _sent(8, I64)
    assert _call(L, "fitgnn_induced_edges_count", *head, 0, _p(L, cnt)) == 0
    assert _call(L, "fitgnn_induced_edges_fill", *head, None, 0, _p(L, off_t), _p(L, e_src), _p(L, e_dst)) == 0
    assert _call(L, "fitgnn_induced_edges_count", *([None] * 6), 0, None) == 0                      # (n_rows = 0 is settled first)
    assert bool((cnt == ar.I32_SENTINEL).all()) and bool((e_src == ar.I64_SENTINEL).all()) and bool((e_dst == ar.I64_SENTINEL).all())
    assert _call(L, "fitgnn_induced_edges_count", *head, -1, _p(L, cnt)) == E_BADARG
    assert _call(L, "fitgnn_induced_edges_fill", *head, None, -1, _p(L, off_t), _p(L, e_src), _p(L, e_dst)) == E_BADARG
    for i in range(6):
        h = list(head)
        h[i] = None
        assert _call(L, "fitgnn_induced_edges_count", *h, 1, _p(L, cnt)) == E_BADARG, names[i]
        assert _call(L, "fitgnn_induced_edges_fill", *h, None, 1, _p(L, off_t), _p(L, e_src), _p(L, e_dst)) == E_BADARG, names[i]
    assert _call(L, "fitgnn_induced_edges_count", *head, 1, None) == E_BADARG
    for k in range(3):
        out = [_p(L, off_t), _p(L, e_src), _p(L, e_dst)]
        out[k] = None
        assert _call(L, "fitgnn_induced_edges_fill", *head, None, 1, *out) == E_BADARG
    assert bool((cnt == ar.I32_SENTINEL).all()) and bool((e_src == ar.I64_SENTINEL).all())


@pytest.mark.parametrize("subset", [False, True], ids=["all", "subset"])
@pytest.mark.parametrize("extra", [True, False], ids=["extra", "own"])
@pytest.mark.parametrize("layout", ["sorted", "star"])
def test_torch_path_equals_cpu_path(L, layout, extra, subset):
    from fitgnn_amd import data

    ei, N, assign, n, clusters = ar.partitioned_graph()
    kw = dict(extra_node=extra, layout=layout, clusters=clusters if subset else None)
    want = data.assemble_subgraphs_torch(torch.from_numpy(ei), N, assign, n, **kw)
    got = data.assemble_subgraphs_torch(torch.from_numpy(ei).cuda(), N, assign, n, **kw)
    assert set(got) == set(want) == {"ptr", "node_id", "core", "edge_index"} | ({"seg_start"} if layout == "star" else set())
    for k in want:
        assert got[k].is_cuda and torch.equal(got[k].cpu(), want[k]), k
    assert want["edge_index"].shape[1] > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# batch kernels
# ---------------------------------------------------------------------------------------------------------------------------------
_DTYPES = dict(g_row=I32, g_nnz=I32, g_tile=I32, g_mem=I32, rowptr=I32, col=I32, val=F32, tiles=I32, mem=I32, pooled=torch.uint8,
               mem_rank=I32, ax=F32, tgt=F32)
_BUF_DTYPES = dict(rowptr=I32, col=I32, val=F32, tiles=I32, members=I32, seg_off=I32, seg_of_row=I32, inv_cnt=F32, ax=F32, tgt=F32,
                   members64=I64, cseg=I32, pos=I32)
_dev_sets = {}


def _dataset(name):
    if name not in _dev_sets:
        D = ar.dataset(name)
        _dev_sets[name] = (D, {k: _dev(D[k], dt) for k, dt in _DTYPES.items()})
    return _dev_sets[name]


def _upload(bufs):
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in bufs.items()}


def _offsets(L, Dd, perm_t, step_t, B, off_t, gid_t, slot=None, lsum=None):
    return _call(L, "fitgnn_batch_offsets", _p(L, perm_t), _p(L, step_t), B, _p(L, Dd["g_row"]), _p(L, Dd["g_nnz"]), _p(L, Dd["g_tile"]),
                 _p(L, Dd["g_mem"]), _p(L, off_t), _p(L, gid_t), _p(L, slot), _p(L, lsum))


def _gather_args(L, D, Dd, B, off_t, gid_t, caps, ld_ax, zero_rows, bd, optional=True, over=None):
    """The argument list of fitgnn_batch_gather as a dict in ABI order (`over` replaces entries: the refusals)."""
    R_cap, E_cap, T_cap, M_cap = caps
    a = dict(B=B, off=_p(L, off_t), gid=_p(L, gid_t), g_row=_p(L, Dd["g_row"]), g_nnz=_p(L, Dd["g_nnz"]), g_tile=_p(L, Dd["g_tile"]),
             g_mem=_p(L, Dd["g_mem"]), rowptr=_p(L, Dd["rowptr"]), col=_p(L, Dd["col"]), val=_p(L, Dd["val"]), tiles=_p(L, Dd["tiles"]),
             mem=_p(L, Dd["mem"]), pooled=_p(L, Dd["pooled"]), ax=_p(L, Dd["ax"]), ld_ax_g=D["ld_ax_g"], tgt=_p(L, Dd["tgt"]),
             n_tgt=D["n_tgt"], K=D["K"], R_cap=R_cap, E_cap=E_cap, T_cap=T_cap, M_cap=M_cap, b_rowptr=_p(L, bd["rowptr"]),
             b_col=_p(L, bd["col"]), b_val=_p(L, bd["val"]), b_tiles=_p(L, bd["tiles"]), b_members=_p(L, bd["members"]),
             b_seg_off=_p(L, bd["seg_off"]), b_seg_of_row=_p(L, bd["seg_of_row"]), b_inv_cnt=_p(L, bd["inv_cnt"]), b_ax=_p(L, bd["ax"]),
             ld_ax=ld_ax, b_tgt=_p(L, bd["tgt"]), mem_rank=_p(L, Dd["mem_rank"]) if optional else None,
             b_members64=_p(L, bd["members64"]) if optional else None, b_cseg=_p(L, bd["cseg"]) if optional else None,
             b_pos=_p(L, bd["pos"]) if optional else None, zero_rows=zero_rows)
    assert set(over or ()) <= set(a), over
    a.update(over or {})
    return list(a.values())


def _check_buffers(bd, want, what):
    for k, w in want.items():
        _equal(_host(bd[k]), w, f"{what}: {k}")


@pytest.mark.parametrize("name", list(ar.batch_cases()))
def test_batch_case(L, name):
    from fitgnn_amd import ops

    ds, B, ids, mode, zero_rows, optional, pad = ar.batch_cases()[name]
    D, Dd = _dataset(ds)
    assert zero_rows in (0, 1, ops.ZERO_ROWS)
    caps = ar.capacities(ar.totals(D, ids), B, mode)
    ld_ax = D["K"] + pad
    perm = np.asarray(ids, dtype=np.int64)
    off_ref, gid_ref = ar.batch_offsets(perm, 0, B, D["g_row"], D["g_nnz"], D["g_tile"], D["g_mem"])
    perm_t, step_t = _dev(perm, I64), torch.zeros(1, dtype=I32, device="cuda")
    off_t, gid_t = _sent(4 * (B + 1) + 4, I32), _sent(B + 4, I32)
    assert _offsets(L, Dd, perm_t, step_t, B, off_t, gid_t) == 0
    pad4 = np.full(4, ar.I32_SENTINEL, dtype=np.int32)
    _equal(_host(off_t), np.concatenate([off_ref.reshape(-1), pad4]), "off")
    _equal(_host(gid_t), np.concatenate([gid_ref, pad4]), "gid")
    assert int(step_t) == 1
    bufs = ar.fresh_buffers(B, *caps, ld_ax, D["n_tgt"])
    bd = _upload(bufs)
    assert _call(L, "fitgnn_batch_gather", *_gather_args(L, D, Dd, B, off_t, gid_t, caps, ld_ax, zero_rows, bd, optional)) == 0
    want = ar.batch_gather(B, off_ref, gid_ref, D, *caps, D["K"], ld_ax, D["n_tgt"], zero_rows, bufs, optional)
    _check_buffers(bd, want, name)
    assert ar.live_tiles_partition(_host(bd["tiles"])[:caps[2]], caps[0])
    assert not np.isnan(_host(bd["val"])[:caps[1]]).any() and not np.isnan(_host(bd["inv_cnt"])[:B]).any()


def test_three_steps_over_one_permutation(L):
    """Three consecutive offsets + gather steps on one permutation, the middle batch the largest, the buffers NOT refilled between steps
    2 and 3: step_idx goes 0 -> 3, the loss slot is added to the sum and cleared each time (small integers: exact), and after step 3
    the buffers are what step 3 alone leaves -- nothing of step 2."""
    ds, B, perm, caps = ar.three_steps()
    D, Dd = _dataset(ds)
    ld_ax, zero_rows, losses = D["K"] + 1, 256, (3, 5, 7)
    ref = ar.run_steps(D, B, perm, caps, ld_ax, zero_rows, losses)
    perm_t, step_t = _dev(np.asarray(perm), I64), torch.zeros(1, dtype=I32, device="cuda")
    slot, lsum = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    off_t, gid_t = _sent(4 * (B + 1) + 4, I32), _sent(B + 4, I32)
    bd = None
    for s in range(3):
        if s < 2:
            bd = _upload(ar.fresh_buffers(B, *caps, ld_ax, D["n_tgt"]))
        slot.fill_(float(losses[s]))                                              # what the step's loss kernel left
        assert _offsets(L, Dd, perm_t, step_t, B, off_t, gid_t, slot, lsum) == 0
        assert _call(L, "fitgnn_batch_gather", *_gather_args(L, D, Dd, B, off_t, gid_t, caps, ld_ax, zero_rows, bd)) == 0
        step, r_slot, r_sum, off_ref, gid_ref, want = ref[s]
        assert int(step_t) == step == s + 1
        assert float(slot) == float(r_slot) == 0.0 and float(lsum) == float(r_sum) == float(sum(losses[:s + 1]))
        _equal(_host(off_t)[:4 * (B + 1)], off_ref.reshape(-1), f"step {s}: off")
        _equal(_host(gid_t)[:B], gid_ref, f"step {s}: gid")
        _check_buffers(bd, want, f"step {s}")
    alone = ar.run_steps(D, B, perm[2 * B:], caps, ld_ax, zero_rows, (0,), n_steps=1)[0][5]
    _check_buffers(bd, alone, "step 3 against step 3 alone")


def test_loss_hand_over_needs_both(L):
    D, Dd = _dataset("k1")
    B = 2
    perm_t = _dev(np.asarray([4, 6, 8, 9]), I64)
    off_t, gid_t = _sent(4 * (B + 1), I32), _sent(B, I32)
    for give_slot in (True, False):
        step_t = torch.zeros(1, dtype=I32, device="cuda")
        slot, lsum = torch.full((1,), 3.0, device="cuda"), torch.full((1,), 5.0, device="cuda")
        assert _offsets(L, Dd, perm_t, step_t, B, off_t, gid_t, slot if give_slot else None, None if give_slot else lsum) == 0
        assert int(step_t) == 1 and float(slot) == 3.0 and float(lsum) == 5.0
    assert _offsets(L, Dd, perm_t, step_t, B, off_t, gid_t, slot, lsum) == 0
    assert int(step_t) == 2 and float(slot) == 0.0 and float(lsum) == 8.0
    _equal(_host(gid_t), np.asarray([8, 9], dtype=np.int32), "gid of step 1")


def _graph(rowptr, col, val, tiles, n, nnz, window_rows):
    """A CSRGraph over given device arrays and contiguous-window tiles (what PaddedBatchPlan hands the layers)."""
    from fitgnn_amd.csr import CSRGraph, _Side

    side = _Side(rowptr, col)
    side.val, side.tiles, side.n_tiles = val, tiles, int(tiles.shape[0])
    g = object.__new__(CSRGraph)
    g.device, g.n, g.mode, g.nnz = rowptr.device, n, "gcn", nnz
    g.planned, g.gather, g.split_large, g.block_limit = False, False, False, None
    g.fold_ok, g.f, g.t = False, side, side
    g.dinv, g.seg, g.range_seg, g.window_rows, g.ptr = None, None, None, window_rows, None
    return g


@pytest.mark.parametrize("name", ["B16-exact", "B5-t_over", "B16-r1"])
def test_assembled_batch_multiplies_like_the_host_built_one(L, name):
    """ops.spmm_graph over the assembled CSR and tiles (R_cap rows, the tail tiles and the all-zero tiles included) == the product over
    the host-built batch (its own rows, entries and tiles only) bit for bit, and the rows past the batch are WRITTEN: zeros over NaN."""
    from fitgnn_amd import ops

    ds, B, ids, mode, zero_rows, optional, pad = ar.batch_cases()[name]
    D, Dd = _dataset(ds)
    caps = R_cap, E_cap, T_cap, M_cap = ar.capacities(ar.totals(D, ids), B, mode)
    ld_ax = D["K"] + pad
    n_row, n_nnz, n_tile, n_mem = ar.totals(D, ids)
    perm_t, step_t = _dev(np.asarray(ids), I64), torch.zeros(1, dtype=I32, device="cuda")
    off_t, gid_t = _sent(4 * (B + 1), I32), _sent(B, I32)
    bd = _upload(ar.fresh_buffers(B, *caps, ld_ax, D["n_tgt"]))
    assert _offsets(L, Dd, perm_t, step_t, B, off_t, gid_t) == 0
    assert _call(L, "fitgnn_batch_gather", *_gather_args(L, D, Dd, B, off_t, gid_t, caps, ld_ax, zero_rows, bd)) == 0
    off_ref, gid_ref = ar.batch_offsets(np.asarray(ids), 0, B, D["g_row"], D["g_nnz"], D["g_tile"], D["g_mem"])
    host = ar.batch_gather(B, off_ref, gid_ref, D, *caps, D["K"], ld_ax, D["n_tgt"], zero_rows, ar.fresh_buffers(B, *caps, ld_ax, D["n_tgt"]))
    window = int(L.lib().fitgnn_spmm_default_window_rows())
    g_dev = _graph(bd["rowptr"][:R_cap + 1], bd["col"][:E_cap], bd["val"][:E_cap], bd["tiles"][:T_cap], R_cap, E_cap, window)
    g_host = _graph(_dev(host["rowptr"][:n_row + 1], I32), _dev(host["col"][:n_nnz], I32), _dev(host["val"][:n_nnz], F32),
                    _dev(host["tiles"][:n_tile], I32), n_row, n_nnz, window)
    X = torch.randn(R_cap, 64, device="cuda")
    Y = ops.spmm_graph(g_dev, X, out=torch.full((R_cap, 64), float("nan"), device="cuda"))
    Yh = ops.spmm_graph(g_host, X[:n_row].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(Y[:n_row], Yh) and not bool(torch.isnan(Yh).any()) and float(Yh.abs().max()) > 0
    assert bool((Y[n_row:] == 0).all())
    A = torch.zeros(n_row, n_row, dtype=torch.float64)
    rp = host["rowptr"][:n_row + 1]
    rows = np.repeat(np.arange(n_row), np.diff(rp))
    A.index_put_((torch.from_numpy(rows), torch.from_numpy(host["col"][:n_nnz].astype(np.int64))), torch.from_numpy(host["val"][:n_nnz].astype(np.float64)), accumulate=True)
    ref = A @ X[:n_row].double().cpu()
    absref = A.abs() @ X[:n_row].double().cpu().abs()
    _within(_host(Yh), ref.numpy(), 4 * U * absref.numpy(), "the host-built product against float64 (at most 4 entries a row)")


def test_plan_tile_capacity_covers_the_longest_tail(L):
    """graph_data.PaddedBatchPlan's T_cap: a batch that fits has at most caps[2] tiles of its own and at least B rows, so the rows past
    it need at most ceil((R_cap - B) / 16) tiles more; the batch with the fewest rows -- the longest tail -- is assembled and its
    tiles still partition [0, R_cap)."""
    from fitgnn_amd import graph_data

    mol = graph_data.synthetic_molecules(96, seed=9)
    gset = graph_data.GraphSet(mol, ratio=0.5, extra_node=True, device="cuda")
    B = 16
    plan = graph_data.PaddedBatchPlan(gset, B, lambda y: y[:, 2:3].long().float())
    assert int(plan.caps[2]) + (plan.R_cap - B + ar.TILE_ROWS - 1) // ar.TILE_ROWS <= plan.T_cap
    ids = np.argsort(plan.sizes[:, 0], kind="stable")[:B]
    assert plan.fits(ids[None, :]).all()
    plan.set_epoch(ids)
    plan.assemble()
    torch.cuda.synchronize()
    n_row, n_tile = int(plan.sizes[ids, 0].sum()), int(plan.sizes[ids, 2].sum())
    t = _host(plan.b_tiles)
    assert ar.live_tiles_partition(t, plan.R_cap, max_rows=max(int(plan.graph.window_rows), ar.TILE_ROWS))
    tail = (plan.R_cap - n_row + ar.TILE_ROWS - 1) // ar.TILE_ROWS
    assert int((t[:, 1] > t[:, 0]).sum()) == n_tile + tail and not t[n_tile + tail:].any()
    assert int(plan.b_rowptr[plan.R_cap]) == int(plan.b_rowptr[n_row]) == int(plan.sizes[ids, 1].sum())


def test_batch_refusals(L):
    ds, B, ids, mode, zero_rows, optional, pad = ar.batch_cases()["B5-r17"]
    D, Dd = _dataset(ds)
    caps = ar.capacities(ar.totals(D, ids), B, mode)
    ld_ax = D["K"] + pad
    perm_t, step_t = _dev(np.asarray(ids), I64), torch.zeros(1, dtype=I32, device="cuda")
    off_t, gid_t = _sent(4 * 1026, I32), _sent(1025, I32)
    for bad_B in (0, 1025, -1):
        assert _offsets(L, Dd, perm_t, step_t, bad_B, off_t, gid_t) == E_BADARG
    base = [_p(L, perm_t), _p(L, step_t), B, _p(L, Dd["g_row"]), _p(L, Dd["g_nnz"]), _p(L, Dd["g_tile"]), _p(L, Dd["g_mem"]), _p(L, off_t), _p(L, gid_t)]
    for i in (0, 1, 3, 4, 5, 6, 7, 8):
        a = list(base)
        a[i] = None
        assert _call(L, "fitgnn_batch_offsets", *a, None, None) == E_BADARG, i
    assert int(step_t) == 0 and bool((off_t == ar.I32_SENTINEL).all()) and bool((gid_t == ar.I32_SENTINEL).all())
    assert _offsets(L, Dd, perm_t, step_t, B, off_t, gid_t) == 0
    bufs = ar.fresh_buffers(B, *caps, ld_ax, D["n_tgt"])
    bd = _upload(bufs)
    args = lambda **over: _gather_args(L, D, Dd, B, off_t, gid_t, caps, ld_ax, 256, bd, over=over)   # noqa: E731
    for over in (dict(B=0), dict(B=1025), dict(R_cap=0), dict(E_cap=0), dict(T_cap=0), dict(M_cap=0), dict(K=0), dict(n_tgt=0),
                 dict(ld_ax=D["K"] - 1), dict(ld_ax_g=D["K"] - 1), dict(mem_rank=None), dict(zero_rows=0), dict(zero_rows=-3)):
        assert _call(L, "fitgnn_batch_gather", *args(**over)) == E_BADARG, over
    required = ("off", "gid", "g_row", "g_nnz", "g_tile", "g_mem", "rowptr", "col", "val", "tiles", "mem", "pooled", "ax", "tgt", "b_rowptr",
                "b_col", "b_val", "b_tiles", "b_members", "b_seg_off", "b_seg_of_row", "b_inv_cnt", "b_ax", "b_tgt")
    for k in required:
        assert _call(L, "fitgnn_batch_gather", *args(**{k: None})) == E_BADARG, k
    _check_buffers(bd, bufs, "a refused call writes nothing")
    # mem_rank NULL and zero_rows 0 are fine without b_pos
    assert _call(L, "fitgnn_batch_gather", *args(mem_rank=None, b_pos=None, zero_rows=0)) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# GCN normalisation
# ---------------------------------------------------------------------------------------------------------------------------------
def _gcn(L, rowptr, col, w, n=None):
    n = len(rowptr) - 1 if n is None else n
    nnz = int(rowptr[n])
    rp, cc = _dev(rowptr, I32), _dev(col if len(col) else np.zeros(1), I32)
    wt = None if w is None else _dev(w if len(w) else np.zeros(1), F32)
    val, dinv = _sent(nnz + 4, F32), _sent(n + 4, F32)
    _run(L, "fitgnn_gcn_norm_csr_f32", _p(L, rp), _p(L, cc), _p(L, wt), _p(L, val), _p(L, dinv), n)
    v, d = _host(val), _host(dinv)
    assert np.isnan(v[nnz:]).all() and np.isnan(d[n:]).all(), "written behind nnz / n_rows"
    return v[:nnz], d[:n]


def _gcn_bounds(rowptr, col, w):
    """(val64, dinv64, bound on val, bound on dinv): the derivation in the module docstring."""
    val, dinv, aval, adeg = ar.gcn_norm_csr(rowptr, col, w)
    Ln = np.diff(rowptr).astype(np.float64)
    deg = 1.0 / np.where(dinv > 0, dinv, 1.0) ** 2
    c = np.where(dinv > 0, adeg / deg, 0.0)
    e = (np.maximum(Ln - 1, 0) * c / 2 + 2)                        # roundings behind dinv: the sum (halved by the root), sqrt, 1 / x
    rows = np.repeat(np.arange(len(Ln)), np.diff(rowptr))
    k = e[rows] + e[col] + 2                                       # the two products
    return val, dinv, k * U * aval * (1 + k * U), e * U * dinv * (1 + e * U)


@pytest.mark.parametrize("n", ar.GCN_N_ROWS, ids=lambda v: f"n{v}")
def test_gcn_norm_weighted(L, n, capsys):
    rowptr, col, w = ar.gcn_case(n)
    v, d = _gcn(L, rowptr, col, w)
    val, dinv, bv, bd = _gcn_bounds(rowptr, col, w)
    assert not np.isnan(v).any() and not np.isnan(d).any()
    with np.errstate(invalid="ignore", divide="ignore"):
        rv, rd = np.abs(v - val) / bv, np.abs(d - dinv) / bd
    with capsys.disabled():
        print(f"\n[gcn_norm weighted n={n}] worst error / bound: val {np.nanmax(rv) if len(rv) else 0.0:.3f}, dinv {np.nanmax(rd):.3f}")
    _within(d, dinv, bd, "dinv")
    _within(v, val, bv, "val")
    empty = np.diff(rowptr) == 0
    assert np.all(d[empty] == 0) and np.all(v[empty[col]] == 0)   # an empty row: dinv 0, and 0 in its column
    v2, d2 = _gcn(L, rowptr, col, w)
    assert np.array_equal(v, v2) and np.array_equal(d, d2)         # fixed order
    # the unweighted launch on the same pattern (w NULL: the row length as degree)
    vu, du = _gcn(L, rowptr, col, None)
    valu, dinvu, bvu, bdu = _gcn_bounds(rowptr, col, None)
    _within(du, dinvu, 2 * U * dinvu * (1 + 2 * U), "dinv, unweighted (an exact degree: sqrt and 1 / x)")
    _within(vu, valu, 6 * U * np.abs(valu) * (1 + 6 * U), "val, unweighted")


def test_gcn_norm_exact(L):
    rowptr, col = ar.gcn_exact_case()
    v, d = _gcn(L, rowptr, col, None)
    val, dinv, _, _ = ar.gcn_norm_csr(rowptr, col, None)
    assert set(np.unique(dinv)) == {0.0, 1.0, 0.5, 0.25, 0.125, 0.0625}
    _same(d, dinv, "dinv")
    _same(v, val, "val")


def test_gcn_norm_nonpositive_degree(L):
    rowptr, col, w = ar.gcn_nonpositive_case()
    v, d = _gcn(L, rowptr, col, w)
    val, dinv, bv, bd = _gcn_bounds(rowptr, col, w)
    assert not np.isnan(v).any() and not np.isnan(d).any()
    assert d[1] == 0 and d[3] == 0 and np.all(d[[0, 2, 4]] > 0)
    rows = np.repeat(np.arange(5), np.diff(rowptr))
    dead = np.isin(rows, (1, 3)) | np.isin(col, (1, 3))
    assert np.all(v[dead] == 0) and np.all(v[~dead] != 0) and (~dead).sum() >= 3
    _within(d, dinv, bd, "dinv")
    _within(v, val, bv, "val")


def test_gcn_norm_refusals(L):
    rowptr, col, w = ar.gcn_case(5)
    rp, cc, wt = _dev(rowptr, I32), _dev(col, I32), _dev(w, F32)
    val, dinv = _sent(len(col) + 4, F32), _sent(9, F32)
    good = [_p(L, rp), _p(L, cc), _p(L, wt), _p(L, val), _p(L, dinv)]
    assert _call(L, "fitgnn_gcn_norm_csr_f32", *good, 0) == 0
    assert _call(L, "fitgnn_gcn_norm_csr_f32", None, None, None, None, None, 0) == 0
    assert _call(L, "fitgnn_gcn_norm_csr_f32", *good, -1) == E_BADARG
    for i in (0, 1, 3, 4):
        a = list(good)
        a[i] = None
        assert _call(L, "fitgnn_gcn_norm_csr_f32", *a, 5) == E_BADARG, i
    assert bool(torch.isnan(val).all()) and bool(torch.isnan(dinv).all())
