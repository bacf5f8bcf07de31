"""GPU tier: the modularity community detection (csrc/community.hip, fitgnn_amd/community.py) against the CPU restatement of its
rule (tests/louvain_reference.py).  Everything is integer, so every comparison is for equality."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph
import torch

import community_graphs as graphs
import louvain_reference as ref
from fitgnn_amd import community, pipeline

pytestmark = pytest.mark.gpu

ROW_LENGTHS = (0, 1, 128, 129, 4096, 4097)   # every side of the sweep's two branch boundaries, and the rows without work


def _csr_from_dict(entries, n):
    """Symmetric {(i, j): w} (diagonal allowed) -> rowptr, col, w with ascending columns."""
    keys = sorted(entries)
    row = np.array([i for i, _ in keys], dtype=np.int64)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=rowptr[1:])
    return rowptr, np.array([j for _, j in keys], dtype=np.int64), np.array([entries[k] for k in keys], dtype=np.int64)


def _stars_graph():
    """Four hubs whose rows hold 128, 129, 4096 and 4097 entries (a diagonal entry, cross edges to other hubs, leaves), leaves with
    and without diagonal entries and a few leaf-leaf cross edges, one node with a diagonal entry only and one with no entry."""
    rng = np.random.default_rng(11)
    entries = {}

    def add(i, j, w):
        entries[(i, j)] = w
        entries[(j, i)] = w

    hubs = [0, 1, 2, 3]
    want = dict(zip(hubs, (128, 129, 4096, 4097)))
    for a, b in ((0, 1), (1, 2), (2, 3), (0, 3)):
        add(a, b, int(rng.integers(1, 6)))
    nxt, leaves_of = 4, {}
    for h in hubs:
        add(h, h, 2 * int(rng.integers(1, 6)))
        n_leaves = want[h] - 3                              # the diagonal and two hub-hub edges are in the row already
        leaves_of[h] = np.arange(nxt, nxt + n_leaves)
        for l in leaves_of[h]:
            add(h, int(l), int(rng.integers(1, 6)))
        nxt += n_leaves
    for l in rng.choice(np.arange(4, nxt), size=600, replace=False):       # leaves that were communities at a lower level
        add(int(l), int(l), 2 * int(rng.integers(1, 4)))
    for h, g in ((0, 2), (1, 3), (2, 3), (0, 1)):                          # cross edges between stars
        for a, b in zip(rng.choice(leaves_of[h], 40, replace=False), rng.choice(leaves_of[g], 40, replace=False)):
            add(int(a), int(b), int(rng.integers(1, 4)))
    add(nxt, nxt, 6)                                        # a diagonal entry only: never moves
    n = nxt + 2                                             # the last node has no entry at all
    rowptr, col, w = _csr_from_dict(entries, n)
    d = np.diff(rowptr)
    assert set(ROW_LENGTHS) <= set(d.tolist()) and n <= 9000, sorted(set(d.tolist()))
    # a non-trivial labelling: a third of the nodes in 40 large communities, the rest scattered over ids (mostly singletons and
    # pairs), so that a hub's table meets thousands of distinct keys
    comm = rng.integers(0, n, size=n)
    big = rng.random(n) < 0.33
    comm[big] = rng.integers(0, 40, size=int(big.sum())) * 7
    return rowptr, col, w, comm


class _Device:
    """A level graph on the device with the kernels' calls, and the reference's view of the same arrays."""

    def __init__(self, rowptr, col, w):
        self.host = (rowptr, col, w)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()   # noqa: E731
        self.k = np.array(ref.degrees(rowptr, w), dtype=np.int64)
        self.level = community._Level(i32(rowptr), i32(col), i32(w), i32(self.k), int(self.k.sum()))
        self.i32 = i32

    def sweep_and_stats(self, comm, t):
        """comm_out of sweep t, then tot / size / (moved, sum in, sum tot^2) of comm_out against comm."""
        n = len(comm)
        tot, size = ref.community_totals(self.k.tolist(), [int(c) for c in comm])
        d_comm, out = self.i32(comm), torch.full((n,), -7, dtype=torch.int32, device="cuda")
        self.level.sweep(d_comm, self.i32(tot), self.i32(size), t, out)
        tot2, size2 = torch.empty_like(out), torch.empty_like(out)
        self.level.stats(out, d_comm, tot2, size2)
        return out.cpu().numpy(), tot2.cpu().numpy(), size2.cpu().numpy(), self.level.out.cpu().numpy()


@pytest.fixture(scope="module")
def stars():
    rowptr, col, w, comm = _stars_graph()
    return _Device(rowptr, col, w), comm


@pytest.mark.parametrize("t", [0, 1])
def test_sweep_and_stats_equal_the_reference_at_every_branch(stars, t):
    dev, comm = stars
    rowptr, col, w = dev.host
    counts = list(dev.level.counts)
    assert counts[0] > 0 and counts[1] == 2 and counts[2] == 1 and counts[3] == 4097, counts    # 129 and 4096 | 4097
    want = ref.sweep(rowptr, col, w, comm, t)
    got, tot, size, out = dev.sweep_and_stats(comm, t)
    moved_rows = {int(np.diff(rowptr)[i]) for i in np.nonzero(np.array(want) != comm)[0]}
    print("sweep t=%d: %d nodes move, among them rows of length %s" % (t, int((np.array(want) != comm).sum()), sorted(moved_rows)[-4:]))
    assert np.array_equal(got, np.array(want))
    r_tot, r_size, r_moved, r_in, r_tot2 = ref.stats(rowptr, col, w, want, comm)
    assert np.array_equal(tot, np.array(r_tot)) and np.array_equal(size, np.array(r_size))
    assert out.tolist() == [r_moved, r_in, r_tot2] and r_moved > 0


def test_two_singletons_do_not_swap():
    """Nodes 0 and 2 are adjacent singletons, both active in sweep 0: only the larger one moves."""
    rowptr, col, w = _csr_from_dict({(0, 2): 1, (2, 0): 1, (1, 3): 1, (3, 1): 1}, 4)
    dev = _Device(rowptr, col, w)
    comm = np.arange(4)
    got = dev.sweep_and_stats(comm, 0)[0]
    assert got.tolist() == [0, 1, 0, 3] == ref.sweep(rowptr, col, w, comm, 0)
    got = dev.sweep_and_stats(comm, 1)[0]
    assert got.tolist() == [0, 1, 2, 1] == ref.sweep(rowptr, col, w, comm, 1)


@pytest.mark.parametrize("id_a,id_b", [(1, 3), (5, 3), (1, 7), (5, 7), (7, 5)])
def test_a_score_tie_goes_to_the_smaller_id(id_a, id_b):
    """Node 0 sees the communities {1, 5} and {3, 7} with equal weight and equal totals, under several community ids: it joins
    the one with the smaller id, whichever node carries it."""
    e = {}
    for a, b in ((0, 1), (0, 3), (1, 5), (3, 7)):
        e[(a, b)] = e[(b, a)] = 1
    rowptr, col, w = _csr_from_dict(e, 8)
    comm = np.array([0, id_a, 2, id_b, 4, id_a, 6, id_b])
    want = ref.sweep(rowptr, col, w, comm, 0)
    assert want[0] == min(id_a, id_b)
    assert _Device(rowptr, col, w).sweep_and_stats(comm, 0)[0].tolist() == want


@pytest.mark.parametrize("comm", graphs.NEAR_LIMIT_COMMS, ids=["singletons", "pairs", "crossed"])
def test_scores_next_to_the_int64_limit(comm):
    """M2 = 2^31 - 2: the products of a score reach 2^61, the sum of tot^2 almost 2^62."""
    rowptr, col, w = graphs.near_limit()
    dev = _Device(rowptr, col, w)
    for t in (0, 1):
        want = ref.sweep(rowptr, col, w, comm, t)
        got, tot, size, out = dev.sweep_and_stats(comm, t)
        assert got.tolist() == want
        r_tot, r_size, r_moved, r_in, r_tot2 = ref.stats(rowptr, col, w, want, comm)
        assert tot.tolist() == r_tot and size.tolist() == r_size and out.tolist() == [r_moved, r_in, r_tot2]
        assert r_tot2 > 2 ** 59


RUN_GRAPHS = {"planted4": graphs.planted4, "ring64": graphs.ring, "sbm1200": graphs.sbm, "gnm": graphs.gnm, "double_star": graphs.double_star}


@pytest.fixture(scope="module")
def reference_runs():
    return {name: ref.modularity_communities(*make(), return_info=True) for name, make in RUN_GRAPHS.items()}


@pytest.mark.parametrize("name", list(RUN_GRAPHS))
def test_full_run_equals_the_reference_at_every_level(reference_runs, name):
    ei, n = RUN_GRAPHS[name]()
    want, want_info = reference_runs[name]
    got, info = community.modularity_communities(ei, n, return_info=True)
    print(name, "levels (sweeps, communities):", [(l["sweeps"], l["n_communities"]) for l in info["levels"]])
    assert info["m2"] == want_info["m2"] and len(info["levels"]) == len(want_info["levels"])
    for lv, (a, b) in enumerate(zip(info["levels"], want_info["levels"])):
        assert (a["sweeps"], a["qnum"], a["n"], a["n_communities"]) == (b["sweeps"], b["qnum"], b["n"], b["n_communities"]), lv
        assert np.array_equal(a["labels"], b["labels"]), lv
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert community.modularity(ei, n, got) == ref.modularity(ei, n, want)


def test_the_runs_reach_weighted_levels(reference_runs):
    assert all(len(info["levels"]) >= 2 for _, info in reference_runs.values())
    assert max(len(info["levels"]) for _, info in reference_runs.values()) >= 3


def test_components_equal_scipy():
    """A community in two far pieces, a 2 000-node path (ids shuffled) in one community, a path cut by a foreign node, isolated nodes."""
    rng = np.random.default_rng(2)
    path = rng.permutation(2000)
    src, dst = [path[:-1]], [path[1:]]
    blob_a, blob_b = np.arange(2000, 2030), np.arange(2030, 2060)               # one community, no edge between the two
    for blob in (blob_a, blob_b):
        src.append(blob[:-1]); dst.append(blob[1:])
    cut = np.arange(2060, 2071)                                                 # 2065 belongs elsewhere: two pieces
    src.append(cut[:-1]); dst.append(cut[1:])
    n = 2080                                                                    # 2071 .. 2079 isolated
    ei = np.stack([np.concatenate(src), np.concatenate(dst)])
    comm = np.zeros(n, dtype=np.int64)
    comm[2000:2060], comm[2060:2071], comm[2065], comm[2071:] = 1, 2, 3, 1
    rowptr, col, _ = ref.level0_graph(ei, n)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()   # noqa: E731
    label = community.connected_pieces(i32(rowptr), i32(col), i32(comm)).cpu().numpy()
    same = comm[ei[0]] == comm[ei[1]]
    g = sp.coo_matrix((np.ones(int(same.sum())), (ei[0][same], ei[1][same])), shape=(n, n))
    n_comp, cc = csgraph.connected_components(g, directed=False)
    smallest = np.full(n_comp, n)
    np.minimum.at(smallest, cc, np.arange(n))
    assert np.array_equal(label, smallest[cc])                                  # the smallest member of every piece
    assert n_comp == 15                 # the path, two blobs, three pieces of the cut path, nine isolated nodes
    by_smallest = np.unique(smallest[cc], return_inverse=True)[1]
    assert np.array_equal(community._number_by_smallest_member(torch.from_numpy(label).cuda())[0].cpu().numpy(), by_smallest)
    assert np.array_equal(np.array(ref.split_components(rowptr, col, comm.tolist())), by_smallest)


def test_two_runs_give_identical_bytes():
    ei, n = graphs.gnm()
    a, ia = community.modularity_communities(ei, n, return_info=True)
    b, ib = community.modularity_communities(ei, n, return_info=True)
    assert a.tobytes() == b.tobytes()
    assert [(l["sweeps"], l["qnum"], l["labels"].tobytes()) for l in ia["levels"]] == [(l["sweeps"], l["qnum"], l["labels"].tobytes())
                                                                                      for l in ib["levels"]]


def test_pipeline_keeps_the_planted_blocks():
    """detect_communities(method="modularity") + merge_communities on planted4: 60 fits, 40 and 25 do not, 10 fits, as the host
    test expects of the true partition."""
    ei, n = graphs.planted4()
    truth = np.repeat(np.arange(4), graphs.PLANTED4_SIZES)
    lab = pipeline.detect_communities(ei, n, method="modularity")
    data = pipeline.NodeData(torch.arange(n).float().view(-1, 1), ei, torch.from_numpy(truth))
    out = pipeline.merge_communities(data, lab, 75)
    assert out.num_nodes == 70 and out.x.flatten().tolist() == list(range(60)) + list(range(125, 135))
    assert int(out.edge_index.max()) < 70 and out.y.tolist() == [0] * 60 + [3] * 10
