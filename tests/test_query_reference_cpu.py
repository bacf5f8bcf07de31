"""CPU tier of the node-query path (fitgnn_amd/serve.py, csrc/query.hip): the float64 references of tests/query_reference.py against
the whole-union forward of the oracle, the host half of QueryEngine (node id -> core row), the launchers' argument refusals and the
exactness of the EXACT inputs the GPU test sends through the kernels."""
import numpy as np
import pytest
import torch

import query_reference as qr
from graph_fixtures import star_blocks
from oracle import gnn_oracle as gorc


def _model(rng, F, H, C):
    g = lambda *s: rng.normal(0, 0.4, size=s)   # noqa: E731
    return dict(W0=g(H, F), b0=g(H), W1=g(H, H), b1=g(H), Wl=g(C, H), bl=g(C))


def _oracle_rows(m, x, ei, rows):
    sd = {"conv.0.lin.weight": m["W0"], "conv.0.bias": m["b0"], "conv.1.lin.weight": m["W1"], "conv.1.bias": m["b1"],
          "lt1.weight": m["Wl"], "lt1.bias": m["bl"]}
    sd = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    out = gorc.classify_node_forward(sd, torch.from_numpy(x).double(), ei, 2)
    return out.numpy()[rows]


def _shared_extra_nodes(sizes, centres):
    """node_id of a star_blocks union read as --extra_node subgraphs: a block's leaves are its own nodes, its centres are copies
    of other blocks' leaves (extra nodes), and the same leaf serves as a centre of SEVERAL blocks."""
    offs = np.concatenate([[0], np.cumsum(sizes)])
    if len(sizes) == 1:   # one subgraph: every row its own node
        return np.arange(offs[-1], dtype=np.int64), np.ones(offs[-1], dtype=bool), int(offs[-1])
    node_id, core, nxt = np.zeros(offs[-1], dtype=np.int64), np.zeros(offs[-1], dtype=bool), 0
    leaves = []
    for b, s in enumerate(sizes):
        c = min(centres, max(s - 1, 0))
        ids = np.arange(nxt, nxt + s - c)
        node_id[offs[b] + c:offs[b + 1]] = ids
        core[offs[b] + c:offs[b + 1]] = True
        leaves.append(ids)
        nxt += s - c
    for b, s in enumerate(sizes):
        donor = max((k for k in range(len(sizes)) if k != b), key=lambda k: len(leaves[k]))   # the largest other block lends its leaves
        for h in range(min(centres, max(s - 1, 0))):
            node_id[offs[b] + h] = leaves[donor][h % len(leaves[donor])]
    return node_id, core, nxt


@pytest.mark.parametrize("sizes,centres,table", [((7, 12, 5, 9), 1, False), ((7, 12, 5, 9), 2, True), ((1, 3, 30, 2, 16), 2, True),
                                                 ((40,), 3, False)], ids=str)
def test_reference_equals_the_whole_union_forward(sizes, centres, table):
    """gather + tail on chosen rows == classify_node_forward in float64 on the whole union, on those rows, to 1e-12; with `table`
    the operand is a de-duplicated node table whose rows the shared extra nodes reference from several subgraphs."""
    rng = np.random.default_rng(len(sizes) * 10 + centres)
    ei, n = star_blocks(list(sizes), centres, seed=3, extra=0.05)
    F, H, C = 6, 16, 5
    m = _model(rng, F, H, C)
    node_id, core, n_nodes = _shared_extra_nodes(list(sizes), centres)
    if len(sizes) >= 3:
        assert len(np.unique(node_id[~core])) < (~core).sum()   # an extra node really is shared between subgraphs
    X = rng.normal(size=(n_nodes, F))
    x_union = X[node_id]
    rowptr, col, val = qr.gcn_csr(ei.numpy(), n)
    rows = np.concatenate([np.nonzero(core)[0][::2], [0, n - 1, 0]])   # unsorted, with duplicates and an extra row
    if table:
        G = qr.gather(rowptr, col, val, X @ m["W0"].T, rows, xrow=node_id, b0=m["b0"])
    else:
        G = qr.gather(rowptr, col, val, x_union @ m["W0"].T, rows, b0=m["b0"])
    out = qr.tail(G, m["W1"], m["b1"], m["Wl"], m["bl"], log_softmax=True)
    ref = _oracle_rows(m, x_union, ei, rows)
    assert np.abs(out - ref).max() <= 1e-12
    dense = qr.dense_forward(x_union, ei.numpy(), m["W0"], m["b0"], m["W1"], m["b1"], m["Wl"], m["bl"])[rows]
    assert np.abs(dense - ref).max() <= 1e-12


def test_core_row_table_on_a_hand_made_batch():
    from fitgnn_amd.serve import core_row_table, first_missing

    #          sub 0: own 4, 2 + extra 7   sub 1: own 7 + extra 2, 4    sub 2: own 0 + extra 7
    node_id = [4, 2, 7, 7, 2, 4, 0, 7]
    core = [1, 1, 0, 1, 0, 0, 1, 0]
    t = core_row_table(node_id, core, n_nodes=9)
    assert t.dtype == np.int64 and t.tolist() == [6, -1, 1, -1, 0, -1, -1, 3, -1]
    assert core_row_table(node_id, core).tolist() == [6, -1, 1, -1, 0, -1, -1, 3]      # sized by the largest id seen
    assert first_missing(t, [4, 7, 0, 2, 7]) is None
    assert first_missing(t, [4, 5, 1]) == 5          # the FIRST id without a core row
    assert first_missing(t, [0, 9]) == 9 and first_missing(t, [-1]) == -1   # outside the table
    assert first_missing(t, []) is None
    # a shard: sub 1 alone -- its extra nodes 2 and 4 have no core row there
    t1 = core_row_table(node_id[3:6], core[3:6], n_nodes=9)
    assert t1.tolist() == [-1] * 7 + [0, -1] and first_missing(t1, [7, 2]) == 2


def test_launchers_refuse_bad_arguments_without_touching_the_gpu():
    from fitgnn_amd import _lib
    L = _lib.lib()
    g = L.fitgnn_gcn_query_gather_f32
    #        rowptr col  val   T    ldt  xrow  b0    rows  Q   H    G    ldg  stream
    assert g(None, None, None, None, 512, None, None, None, -1, 512, None, 512, None) == -1    # Q < 0
    assert g(None, None, None, None, 512, None, None, None, 4, 510, None, 512, None) == -1     # H % 4 != 0
    assert g(None, None, None, None, 508, None, None, None, 4, 512, None, 512, None) == -1     # ldt < H
    assert g(None, None, None, None, 512, None, None, None, 4, 512, None, 508, None) == -1     # ldg < H
    assert g(None, None, None, None, 514, None, None, None, 4, 512, None, 512, None) == -3     # ldt % 4 != 0
    assert g(None, None, None, None, 512, None, None, None, 0, 512, None, 512, None) == 0      # nothing to do
    assert g(None, None, None, None, 512, None, None, None, 4, 512, None, 512, None) == -1     # NULL pointers, refused not dereferenced
    t = L.fitgnn_gcn_query_tail_f32
    #        G    ldg  Q   W1    b1    Wl    bl    H    H2   C  out   ldo lsm stream
    assert t(None, 512, -1, None, None, None, None, 512, 512, 7, None, 7, 0, None) == -1        # Q < 0
    assert t(None, 512, 4, None, None, None, None, 510, 512, 7, None, 7, 0, None) == -1         # H % 4 != 0
    assert t(None, 512, 4, None, None, None, None, 512, 520, 7, None, 7, 0, None) == -1         # H2 % 16 != 0
    assert t(None, 508, 4, None, None, None, None, 512, 512, 7, None, 7, 0, None) == -1         # ldg < H
    assert t(None, 512, 4, None, None, None, None, 512, 512, 7, None, 6, 0, None) == -1         # ldo < C
    assert t(None, 512, 0, None, None, None, None, 512, 512, 7, None, 7, 1, None) == 0          # nothing to do
    assert t(None, 512, 4, None, None, None, None, 512, 512, 7, None, 7, 1, None) == -1         # NULL pointers
    assert t(None, 512, 4, None, None, None, None, 512, 4096, 7, None, 7, 0, None) == -1        # z of the tile beyond 160 KiB of LDS
    lds = L.fitgnn_gcn_query_tail_lds_bytes
    # z [16 x (H2 + 4)] + the W1 stage [256 x 36] + the G stage [16 x 36] + the logits [16 x C]
    assert lds(512, 47) == (16 * 516 + 256 * 36 + 16 * 36 + 16 * 47) * 4
    assert lds(512, 48) <= 160 * 1024 and lds(0, 7) == 0
    assert lds(4096, 7) > 160 * 1024


def _exactness_watch():
    seen = {"n": 0}

    def watch(name, a):
        a = np.asarray(a, dtype=np.float64)
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), f"{name} does not survive float32"
        if name == "pre":
            assert np.all((a >= 0) | (a <= -32)), "a pre-activation inside (-32, 0): fp32 ELU would round"
        seen["n"] += 1
    return watch, seen


@pytest.mark.parametrize("case", qr.EXACT_GATHER_CASES, ids=str)
def test_exact_gather_inputs_are_exact(case):
    c = qr.exact_gather_case(*case)
    watch, seen = _exactness_watch()
    G = qr.gather(c["rowptr"], c["col"], c["val"], c["T"], c["rows"], xrow=c["xrow"], b0=c["b0"], watch=watch, f32_elu=True)
    assert seen["n"] > 1000 and np.isfinite(G).all()
    deg = np.diff(c["rowptr"])
    assert sorted(set(deg[c["rows"]].tolist())) == sorted(qr.GATHER_QUERY_DEGS)
    assert set(qr.GATHER_NEIGHBOUR_DEGS) <= set(deg[c["col"][c["rowptr"][11]:c["rowptr"][12]]].tolist())   # the 130-entry query meets them all
    if c["xrow"] is not None:
        assert c["xrow"][c["col"]].max() == c["T"].shape[0] - 1
    if c["b0"] is not None:
        assert (G < 0).any() and (G > 0).any()    # both ELU branches reach the output


@pytest.mark.parametrize("case", qr.EXACT_TAIL_CASES, ids=str)
def test_exact_tail_inputs_are_exact(case):
    c = qr.exact_tail_case(*case)
    watch, seen = _exactness_watch()
    out = qr.tail(c["G"], c["W1"], c["b1"], c["Wl"], c["bl"], watch=watch, f32_elu=True)
    assert seen["n"] > case[0] and np.isfinite(out).all()
