"""CPU tier: tests/louvain_reference.py, the restatement the GPU community detection is compared with bit for bit, is itself a
sound modularity optimiser: its partitions are as good as networkx's Louvain where the structure is clear, within a stated factor
of it elsewhere, never worse than the label-propagation substitute, monotone from level to level, connected and exact in int64."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph

import community_graphs as graphs
import louvain_reference as ref

try:
    import networkx as nx
except ImportError:          # the comparisons with networkx are skipped, the rest is not
    nx = None

NAMES = ["planted4", "karate", "ring64", "ba600", "caveman", "sbm1200", "star", "gnm"]


def _from_nx(g):
    return np.array(list(g.edges()), dtype=np.int64).T, g.number_of_nodes()


def _build(name):
    if name == "planted4":
        return graphs.planted4()
    if name == "ring64":
        return graphs.ring(64)
    if nx is None:
        pytest.skip("networkx is not installed")
    if name == "karate":
        return _from_nx(nx.karate_club_graph())
    if name == "ba600":
        return _from_nx(nx.barabasi_albert_graph(600, 3, seed=1))
    if name == "caveman":
        return _from_nx(nx.connected_caveman_graph(12, 8))
    if name == "sbm1200":
        p = (np.full((8, 8), 0.004) + np.eye(8) * (0.084 - 0.004)).tolist()
        return _from_nx(nx.stochastic_block_model([150] * 8, p, seed=3))
    if name == "star":
        return _from_nx(nx.star_graph(300))
    return _from_nx(nx.gnm_random_graph(400, 1600, seed=5))


_cache = {}


def _run(name):
    """(edge_index, n, labels, info, labels without the split): computed once per graph and shared, never changed."""
    if name not in _cache:
        ei, n = _build(name)
        labels, info = ref.modularity_communities(ei, n, return_info=True)
        _cache[name] = (ei, n, labels, info, ref.modularity_communities(ei, n, split_disconnected=False))
    return _cache[name]


def _louvain_q(name):
    ei, n = _run(name)[:2]
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(ei.T.tolist())
    qs = []
    for seed in range(5):
        lab = np.zeros(n, dtype=np.int64)
        for c, members in enumerate(nx.community.louvain_communities(g, seed=seed)):
            lab[list(members)] = c
        qs.append(ref.modularity(ei, n, lab))
    return qs


@pytest.mark.skipif(nx is None, reason="networkx is not installed")
@pytest.mark.parametrize("name", ["planted4", "ring64", "caveman", "sbm1200", "star"])
def test_as_good_as_networkx_louvain_on_clear_structure(name):
    ei, n, labels = _run(name)[:3]
    q, qs = ref.modularity(ei, n, labels), _louvain_q(name)
    print(name, "Q = %.6f, networkx Louvain seeds 0..4: best %.6f worst %.6f" % (q, max(qs), min(qs)))
    assert q >= max(qs) - 1e-12


@pytest.mark.skipif(nx is None, reason="networkx is not installed")
@pytest.mark.parametrize("name", ["karate", "ba600", "gnm"])
def test_within_085_of_networkx_louvain_elsewhere(name):
    ei, n, labels = _run(name)[:3]
    q, qs = ref.modularity(ei, n, labels), _louvain_q(name)
    print(name, "Q = %.6f, networkx Louvain seeds 0..4: best %.6f worst %.6f, ratio to the worst %.4f" % (q, max(qs), min(qs), q / min(qs)))
    assert q >= 0.85 * min(qs)


@pytest.mark.parametrize("name", NAMES)
def test_never_below_the_label_propagation_substitute(name):
    from fitgnn_amd import pipeline

    ei, n, labels = _run(name)[:3]
    sym = np.unique(np.concatenate([ei, ei[::-1]], axis=1), axis=1)
    q_sub = ref.modularity(ei, n, pipeline.detect_communities(sym, n, seed=1))
    q = ref.modularity(ei, n, labels)
    print(name, "Q = %.6f, label propagation %.6f" % (q, q_sub))
    assert q >= q_sub


@pytest.mark.parametrize("name", NAMES)
def test_levels_split_connectivity_and_numbering(name):
    ei, n, labels, info, unsplit = _run(name)
    m2 = info["m2"]
    q_levels = [lv["qnum"] / (m2 * m2) for lv in info["levels"]]
    assert all(b >= a for a, b in zip(q_levels, q_levels[1:])), q_levels        # accepted Qnum / M2^2 never decreases
    for lv in info["levels"]:                                                   # ... and is the modularity of the level's labels
        assert lv["qnum"] / (m2 * m2) == ref.modularity(ei, n, lv["labels"])
    assert np.array_equal(info["levels"][-1]["labels"], unsplit)
    assert ref.modularity(ei, n, labels) >= ref.modularity(ei, n, unsplit)      # the split never lowers Q
    same = labels[ei[0]] == labels[ei[1]]
    g = sp.coo_matrix((np.ones(int(same.sum())), (ei[0][same], ei[1][same])), shape=(n, n))
    n_comp, cc = csgraph.connected_components(g, directed=False)
    assert n_comp == int(labels.max()) + 1                                      # every final community is connected:
    assert len(set(zip(cc.tolist(), labels.tolist()))) == n_comp                # pieces and communities coincide
    for lab in (labels, unsplit):                                               # numbered by smallest member
        first = [int(np.nonzero(lab == c)[0][0]) for c in range(int(lab.max()) + 1)]
        assert first == sorted(first) and lab.dtype == np.int64


def _int64_scores(rowptr, col, w, comm, t):
    """The scores of sweep t in numpy int64, overflow checked: {(i, c): s}."""
    n = len(rowptr) - 1
    k = np.add.reduceat(np.append(w, 0), rowptr[:-1]) * (np.diff(rowptr) > 0)
    m2 = np.int64(k.sum())
    tot = np.zeros(n, dtype=np.int64)
    np.add.at(tot, comm, k)
    out = {}
    with np.errstate(over="raise"):
        for i in range(n):
            if (i + t) % 2:
                continue
            js, ws = col[rowptr[i]:rowptr[i + 1]], w[rowptr[i]:rowptr[i + 1]]
            off = js != i
            if not off.any():
                continue
            cs, inv = np.unique(comm[js[off]], return_inverse=True)
            acc = np.zeros(len(cs), dtype=np.int64)
            np.add.at(acc, inv, ws[off])
            a = comm[i]
            out[(i, int(a))] = int(m2 * (acc[cs == a].sum()) - k[i] * (tot[a] - k[i]))
            for c, x in zip(cs, acc):
                if c != a:
                    out[(i, int(c))] = int(np.multiply(m2, x, dtype=np.int64) - np.multiply(k[i], tot[c], dtype=np.int64))
    return out


@pytest.mark.parametrize("name", NAMES + ["near_limit"])
def test_python_ints_agree_with_int64(name):
    if name == "near_limit":
        rowptr, col, w = graphs.near_limit()
        assert sum(ref.degrees(rowptr, w)) == 2 ** 31 - 2
        comms = graphs.NEAR_LIMIT_COMMS
    else:
        ei, n = _build(name)
        rowptr, col, w = ref.level0_graph(ei, n)
        comms = [np.arange(n), np.array(ref.run_level(rowptr, col, w, max_sweeps=3)[0])]
    for comm in comms:
        for t in (0, 1):
            scores = []
            ref.sweep(rowptr, col, w, comm, t, scores=scores)
            want = _int64_scores(rowptr, col, w, comm, t)
            got = {(i, c): s for i, c, s in scores}
            assert scores and all(abs(s) < 2 ** 63 for s in got.values())
            assert all(want[key] == s for key, s in got.items())       # every score the rule evaluates fits int64 unchanged
        _, _, _, sum_in, sum_tot2 = ref.stats(rowptr, col, w, comm, comm)
        m2 = sum(ref.degrees(rowptr, w))
        assert m2 * sum_in < 2 ** 63 and sum_tot2 <= m2 * m2 < 2 ** 62
