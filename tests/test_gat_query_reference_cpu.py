"""CPU tier of the attention query path (csrc/query.hip gat_query_hops_kernel, fitgnn_amd/serve.py with gat_kernels=True): the
float64 reference of tests/gat_query_reference.py against a two-layer GAT forward composed from the oracle, the exactness of the
EXACT inputs the GPU test sends through the kernel, the launcher's argument refusals and ops.gat_query_supported's host logic."""
import argparse

import numpy as np
import pytest
import torch

import gat_query_reference as gq
import query_reference as qr
from oracle import gnn_oracle as gorc


def _graph(kind):
    """(edge_index [2, E] with source row 0 and target row 1, n): self loops on some nodes already, and no symmetry assumed."""
    rng = np.random.default_rng({"random": 1, "isolated": 2, "hub": 3}[kind])
    if kind == "random":
        n = 23
        e = rng.integers(0, n, size=(2, 70))
    elif kind == "isolated":   # node 5 has no edge at all, node 6 only a self loop, node 7 only outgoing edges
        n = 17
        e = rng.integers(0, n, size=(2, 40))
        e = e[:, (e != 5).all(0) & (e != 6).all(0) & (e[1] != 7)]
        e = np.concatenate([e, [[6, 7, 7], [6, 1, 2]]], axis=1)
    else:                      # node 0 hears every node, and a few random edges
        n = 70
        e = np.concatenate([np.stack([np.arange(n), np.zeros(n, dtype=np.int64)]), rng.integers(0, n, size=(2, 60))], axis=1)
    e = np.concatenate([e, np.stack([np.arange(0, n, 3)] * 2)], axis=1)   # existing self loops: replaced by exactly one
    return e.astype(np.int64), n


@pytest.mark.parametrize("kind", ["random", "isolated", "hub"])
def test_reference_equals_the_oracle_forward(kind):
    """gather (attention over both hops, layer 1 before its Linear, scores through W1^T att) + query_reference.tail == ELU(gat_conv)
    twice + head + log_softmax in float64, to 1e-12 relative: the identities att . (W1 h) = (W1^T att) . h and sum beta = 1, and that
    the pattern's rows are the targets."""
    ei, n = _graph(kind)
    rng = np.random.default_rng(n)
    F, H, H2, C = 6, 16, 32, 5
    g = lambda *s: rng.normal(0, 0.6, size=s)   # noqa: E731
    sd = {"conv.0.lin.weight": g(H, F), "conv.0.att_src": g(1, 1, H), "conv.0.att_dst": g(1, 1, H), "conv.0.bias": g(H),
          "conv.1.lin.weight": g(H2, H), "conv.1.att_src": g(1, 1, H2), "conv.1.att_dst": g(1, 1, H2), "conv.1.bias": g(H2),
          "lt1.weight": g(C, H2), "lt1.bias": g(C)}
    X = rng.normal(size=(n, F))
    slopes = (0.2, 0.35)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    ref = gq.oracle_forward(gorc, tsd, torch.from_numpy(X), torch.from_numpy(ei), slopes).numpy()
    rowptr, col, _ = qr.gcn_csr(ei, n)
    T = X @ sd["conv.0.lin.weight"].T
    W1 = sd["conv.1.lin.weight"]
    rows = np.concatenate([np.arange(n)[::-1], [0, 0]])
    G = gq.gather(rowptr, col, T, T @ sd["conv.0.att_src"].reshape(-1), T @ sd["conv.0.att_dst"].reshape(-1),
                  W1.T @ sd["conv.1.att_src"].reshape(-1), W1.T @ sd["conv.1.att_dst"].reshape(-1), rows, b0=sd["conv.0.bias"],
                  slope0=slopes[0], slope1=slopes[1])
    out = qr.tail(G, W1, sd["conv.1.bias"], sd["lt1.weight"], sd["lt1.bias"], log_softmax=True)
    assert np.abs(out - ref[rows]).max() <= 1e-12 * np.abs(ref).max()
    # the same through a de-duplicated table: rows 2 k and 2 k + 1 of a doubled table hold node k
    xrow = 2 * np.arange(n) + (np.arange(n) % 2)
    T2 = np.repeat(T, 2, axis=0)
    G2 = gq.gather(rowptr, col, T2, T2 @ sd["conv.0.att_src"].reshape(-1), T2 @ sd["conv.0.att_dst"].reshape(-1),
                   W1.T @ sd["conv.1.att_src"].reshape(-1), W1.T @ sd["conv.1.att_dst"].reshape(-1), rows, xrow=xrow, b0=sd["conv.0.bias"],
                   slope0=slopes[0], slope1=slopes[1])
    assert np.abs(G2 - G).max() <= 1e-12 * np.abs(G).max()


def _exactness_watch():
    seen = {"n": 0, "names": set()}

    def watch(name, a):
        a = np.asarray(a, dtype=np.float64)
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), f"{name} does not survive float32"
        if name == "pre":
            assert np.all((a >= 0) | (a <= -32)), "a pre-activation inside (-32, 0): fp32 ELU would round"
        if name in ("arg", "x_arg"):
            assert np.all((a == 0) | (a <= -104)), "an exp argument inside (-104, 0): expf would round"
        seen["n"] += 1
        seen["names"].add(name)
    return watch, seen


@pytest.mark.parametrize("case", gq.EXACT_GATHER_CASES, ids=str)
@pytest.mark.parametrize("gen", sorted(gq.EXACT_GENERATORS))
def test_exact_inputs_are_exact(gen, case):
    c = gq.EXACT_GENERATORS[gen](*case)
    watch, seen = _exactness_watch()
    G = gq.run(c, watch=watch, f32_elu=True)
    assert seen["n"] > 1000 and np.isfinite(G).all()
    assert {"s", "e", "arg", "p", "l", "a", "inv", "pre", "h", "dot", "cq", "cj", "f", "x", "L", "P", "g"} <= seen["names"]
    # what rounds to float32 exactly is also what float64 gives without the rounding of exp, up to exp's underflow (< 1e-200)
    assert np.abs(gq.run(c) - G).max() <= 1e-12
    deg = np.diff(c["rowptr"])
    q_degs = gq.UNIFORM_QUERY_DEGS if gen == "uniform" else qr.GATHER_QUERY_DEGS
    n_degs = gq.UNIFORM_NEIGHBOUR_DEGS if gen == "uniform" else qr.GATHER_NEIGHBOUR_DEGS
    assert deg[c["rows"]].tolist() == q_degs and np.all(G[np.array(q_degs) == 0] == 0)
    met = set()
    for q in c["rows"]:
        met |= set(deg[c["col"][c["rowptr"][q]:c["rowptr"][q + 1]]].tolist())
    assert set(n_degs) <= met, "a neighbour degree no query meets"
    if c["xrow"] is not None:
        assert c["xrow"][c["col"]].max() == c["T"].shape[0] - 1
    if c["b0"] is not None:
        assert (G < 0).any() and (G > 0).any()    # both ELU branches reach the output
    if gen == "selector":
        f = []
        gq.run(c, watch=lambda name, a: f.append(float(a)) if name == "f" else None, f32_elu=True)
        assert min(f) < 0 and max(f) >= 0 and len(set(f)) > 8      # layer-1 scores on both sides of the LeakyReLU
        # a dropped, doubled or misplaced entry shows: pointing one winner elsewhere changes the result
        d = dict(c)
        d["a_src0"] = c["a_src0"][::-1].copy()
        assert np.abs(gq.run(d, f32_elu=True) - G).max() > 0


def test_launcher_refuses_bad_arguments_without_touching_the_gpu():
    from fitgnn_amd import _lib
    g = _lib.lib().fitgnn_gat_query_gather_f32
    #        rowptr col   T    ldt  xrow  a_s   a_d   b0   sl0  u_s   u_d   sl1  rows  Q   H    G    ldg  stream
    for H in (0, 6, 516):
        assert g(None, None, None, 520, None, None, None, None, 0.2, None, None, 0.2, None, 4, H, None, 520, None) == -1    # bad H
    assert g(None, None, None, 512, None, None, None, None, 0.2, None, None, 0.2, None, -1, 512, None, 512, None) == -1     # Q < 0
    assert g(None, None, None, 508, None, None, None, None, 0.2, None, None, 0.2, None, 4, 512, None, 512, None) == -1      # ldt < H
    assert g(None, None, None, 512, None, None, None, None, 0.2, None, None, 0.2, None, 4, 512, None, 508, None) == -1      # ldg < H
    assert g(None, None, None, 514, None, None, None, None, 0.2, None, None, 0.2, None, 4, 512, None, 512, None) == -3      # ldt % 4 != 0
    assert g(None, None, None, 512, None, None, None, None, 0.2, None, None, 0.2, None, 4, 512, None, 518, None) == -3      # ldg % 4 != 0
    assert g(None, None, None, 512, None, None, None, None, 0.2, None, None, 0.2, None, 0, 512, None, 512, None) == 0       # nothing to do
    assert g(None, None, None, 512, None, None, None, None, 0.2, None, None, 0.2, None, 4, 512, None, 512, None) == -1      # NULL pointers


def _model(layer="GATConv", layers=2, hidden=64, F=12):
    from fitgnn_amd import network
    args = argparse.Namespace(num_layers1=layers, layer_name=layer, num_features=F, hidden=hidden, num_classes=7)
    torch.manual_seed(0)
    return network.Classify_node(args).eval()


def test_gat_query_supported_refuses_on_the_host():
    """What ops.gat_query_supported decides before any device is needed: the layer types and count come first, and parameters that
    are not on the GPU are refused (so a CPU model never reaches the launcher)."""
    from fitgnn_amd import ops
    assert ops.gat_query_supported(_model()) is False                       # two GATConv layers, but on the CPU
    assert ops.gat_query_supported(_model(layer="GCNConv")) is False
    assert ops.gat_query_supported(_model(layers=3)) is False
    assert ops.gat_query_supported(_model(layers=1)) is False
    assert ops.gat_query_supported(torch.nn.Linear(3, 3)) is False          # no conv stack at all
