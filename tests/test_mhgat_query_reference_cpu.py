"""CPU tier of the multi-head attention query path (csrc/query.hip mhgat_hops_kernel and mhgat_tail_kernel,
fitgnn_amd/serve.py with gat_heads_kernels=True): the float64 reference of tests/mhgat_query_reference.py against a two-layer
multi-head GAT forward composed from the oracle, against the single-head reference when the heads share their scores, the exactness of
the EXACT inputs the GPU test sends through the kernel, what the selector case selects, and ops.mhgat_query_supported's host logic."""
import argparse

import numpy as np
import pytest
import torch

import gat_query_reference as gq
import mhgat_query_reference as mq
import query_reference as qr
from oracle import gnn_oracle as gorc
from test_gat_query_reference_cpu import _exactness_watch, _graph


def _grouped_tail(G, W1, b1, Wl, bl, heads, log_softmax=True):
    """z[n] = ELU(W1[n, :] . G[hd1(n) H : (hd1(n) + 1) H] + b1[n]), the head, the log-softmax: the issue's formula, directly."""
    H2, H = W1.shape
    C1 = H2 // heads
    z = np.concatenate([G[:, g * H:(g + 1) * H] @ W1[g * C1:(g + 1) * C1].T for g in range(heads)], axis=1) + b1
    y = qr.elu(z) @ Wl.T + bl
    if log_softmax:
        y = y - y.max(1, keepdims=True)
        y = y - np.log(np.exp(y).sum(1, keepdims=True))
    return y


@pytest.mark.parametrize("heads", [2, 3])
@pytest.mark.parametrize("kind", ["random", "isolated", "hub"])
def test_reference_equals_the_oracle_forward(kind, heads):
    """gather (every head's attention over both hops, layer 1 before its Linear, scores through W1[block]^T att) + the grouped tail
    == ELU(concat of gat_conv per head) twice + head + log_softmax in float64, to 1e-12 relative: att . (W1 h)[block hd] =
    (W1[block hd]^T att) . h and sum_j beta^{hd}_j = 1.  The grouped tail is also query_reference.tail on the block-expanded W1."""
    ei, n = _graph(kind)
    rng = np.random.default_rng(n + heads)
    F, C0, C1, C = 6, 8, 16, 5
    H, H2 = heads * C0, heads * C1
    g = lambda *s: rng.normal(0, 0.6, size=s)   # noqa: E731
    sd = {"conv.0.lin.weight": g(H, F), "conv.0.att_src": g(1, heads, C0), "conv.0.att_dst": g(1, heads, C0), "conv.0.bias": g(H),
          "conv.1.lin.weight": g(H2, H), "conv.1.att_src": g(1, heads, C1), "conv.1.att_dst": g(1, heads, C1), "conv.1.bias": g(H2),
          "lt1.weight": g(C, H2), "lt1.bias": g(C)}
    X = rng.normal(size=(n, F))
    slopes = (0.2, 0.35)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    ref = mq.oracle_forward(gorc, tsd, torch.from_numpy(X), torch.from_numpy(ei), heads, slopes).numpy()
    rowptr, col, _ = qr.gcn_csr(ei, n)
    T = X @ sd["conv.0.lin.weight"].T
    W1 = sd["conv.1.lin.weight"]
    rows = np.concatenate([np.arange(n)[::-1], [0, 0]])
    scores = lambda T, att: (T.reshape(len(T), heads, C0) * sd[att].reshape(1, heads, C0)).sum(-1)   # noqa: E731
    U_s, U_d = mq.u_vectors(W1, sd["conv.1.att_src"], heads), mq.u_vectors(W1, sd["conv.1.att_dst"], heads)
    G = mq.gather(rowptr, col, T, scores(T, "conv.0.att_src"), scores(T, "conv.0.att_dst"), U_s, U_d, rows, b0=sd["conv.0.bias"],
                  slope0=slopes[0], slope1=slopes[1])
    out = _grouped_tail(G, W1, sd["conv.1.bias"], sd["lt1.weight"], sd["lt1.bias"], heads)
    assert np.abs(out - ref[rows]).max() <= 1e-12 * np.abs(ref).max()
    big = qr.tail(G, mq.tail_expanded(W1, heads), sd["conv.1.bias"], sd["lt1.weight"], sd["lt1.bias"], log_softmax=True)
    assert np.abs(big - out).max() <= 1e-12 * np.abs(ref).max()
    # the same through a de-duplicated table: rows 2 k and 2 k + 1 of a doubled table hold node k
    xrow = 2 * np.arange(n) + (np.arange(n) % 2)
    T2 = np.repeat(T, 2, axis=0)
    G2 = mq.gather(rowptr, col, T2, scores(T2, "conv.0.att_src"), scores(T2, "conv.0.att_dst"), U_s, U_d, rows, xrow=xrow,
                   b0=sd["conv.0.bias"], slope0=slopes[0], slope1=slopes[1])
    assert np.abs(G2 - G).max() <= 1e-12 * np.abs(G).max()


def _shared(c, g=0):
    """The case with head g's layer-0 scores in every head."""
    d = dict(c)
    heads = c["heads"]
    d["a_src0"] = np.repeat(c["a_src0"][:, g:g + 1], heads, axis=1)
    d["a_dst0"] = np.repeat(c["a_dst0"][:, g:g + 1], heads, axis=1)
    return d


@pytest.mark.parametrize("heads,H", [(2, 8), (4, 64), (5, 260)])
def test_shared_scores_equal_the_single_head_reference(heads, H):
    """With `heads` copies of one head's layer-0 scores every block of G is gat_query_reference.gather's with that block's
    (U_s[hd], U_d[hd]), exactly: the same operations in the same order.  The bound is the same sum of the same terms."""
    rng = np.random.default_rng([heads, H, 31])
    rowptr, col, _, xrow, n_rows = qr.query_csr(rng, [0, 1, 3, 4, 9, 17], [0, 1, 2, 5, 70], 19, True, pow2_val=False)
    nt = 19
    c = dict(rowptr=rowptr, col=col, xrow=xrow, T=rng.normal(size=(nt, H)), b0=rng.normal(size=H), a_src0=rng.normal(size=(nt, heads)),
             a_dst0=rng.normal(size=(nt, heads)), U_src=rng.normal(size=(heads, H)) / np.sqrt(H), U_dst=rng.normal(size=(heads, H)) / np.sqrt(H),
             slope0=0.2, slope1=0.3, rows=np.arange(6, dtype=np.int64), n_rows=n_rows, heads=heads)
    d = _shared(c, 1)
    G, B = mq.run(d, sums=True)
    for g in range(heads):
        Gs, Bs = gq.run(mq.single_head_case(d, g, scores_of=1), sums=True)
        assert np.array_equal(G[:, g * H:(g + 1) * H], Gs), g
        assert np.all(np.abs(B[:, g * H:(g + 1) * H] - Bs) <= 1e-12 * Bs), g    # (float64 sums of the same terms in another order)
    assert not np.array_equal(mq.run(c), G)     # and the heads' own scores give something else


@pytest.mark.parametrize("case", mq.EXACT_GATHER_CASES, ids=str)
@pytest.mark.parametrize("gen", sorted(mq.EXACT_GENERATORS))
def test_exact_inputs_are_exact(gen, case):
    c = mq.EXACT_GENERATORS[gen](*case)
    heads, H = case[:2]
    watch, seen = _exactness_watch()
    G = mq.run(c, watch=watch, f32_elu=True)
    assert seen["n"] > 1000 and np.isfinite(G).all() and G.shape == (len(c["rows"]), heads * H)
    assert {"s", "e", "arg", "p", "l", "a", "inv", "pre", "h", "dot", "cq", "cj", "f", "x", "L", "P", "g"} <= seen["names"]
    # what rounds to float32 exactly is also what float64 gives without the rounding of exp, up to exp's underflow (< 1e-200)
    assert np.abs(mq.run(c) - G).max() <= 1e-12
    for k in ("T", "a_src0", "a_dst0", "U_src", "U_dst"):
        assert c[k].dtype == np.float32, k
    deg = np.diff(c["rowptr"])
    q_degs = mq.UNIFORM_QUERY_DEGS if gen == "uniform" else qr.GATHER_QUERY_DEGS
    n_degs = mq.UNIFORM_NEIGHBOUR_DEGS if gen == "uniform" else qr.GATHER_NEIGHBOUR_DEGS
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
        mq.run(c, watch=lambda name, a: f.append(float(a)) if name == "f" else None, f32_elu=True)
        assert min(f) < 0 and max(f) >= 0 and len(set(f)) > 8      # layer-1 scores on both sides of the LeakyReLU
        d = dict(c)
        d["a_src0"] = c["a_src0"][::-1].copy()
        assert np.abs(mq.run(d, f32_elu=True) - G).max() > 0


@pytest.mark.parametrize("case", mq.EXACT_GATHER_CASES, ids=str)
def test_selector_case_tells_the_heads_apart(case):
    """At least two heads of some query select different entry sets, and a kernel that took head 0's layer-0 weights for every
    column, or head 0's beta for every block, would not return the selector case's G: every block past the first differs."""
    c = mq.exact_selector_case(*case)
    heads, H = case[:2]
    sel = mq.selected_entries(c, f32_elu=True)
    n_q = 1 + max(q for q, _ in sel)
    assert any(len({sel[(q, g)] for g in range(heads)}) >= 2 for q in range(n_q))
    assert sum(sel[(q, 0)] != sel[(q, 1)] for q in range(n_q)) >= n_q // 2
    G = mq.run(c, f32_elu=True)
    # head 0's layer-0 scores in every head
    wrong0 = mq.run(_shared(c, 0), f32_elu=True)
    # head 0's layer-1 weights on every block: block g of G would be the single-head result of (U_s[0], U_d[0])
    d = dict(c)
    d["U_src"], d["U_dst"] = np.repeat(c["U_src"][:1], heads, 0), np.repeat(c["U_dst"][:1], heads, 0)
    wrong1 = mq.run(d, f32_elu=True)
    for g in range(1, heads):
        blk = slice(g * H, (g + 1) * H)
        assert not np.array_equal(wrong0[:, blk], G[:, blk]), g
        if g % 2 == 1:   # (the even heads share head 0's group: their layer-1 selection is head 0's by construction)
            assert not np.array_equal(wrong1[:, blk], G[:, blk]), g


def test_tail_expanded_places_the_blocks():
    W1 = np.arange(1, 6 * 4 + 1, dtype=np.float32).reshape(6, 4)
    big = mq.tail_expanded(W1, 3)
    assert big.shape == (6, 12) and big.dtype == np.float32 and np.count_nonzero(big) == 24
    for n in range(6):
        assert np.array_equal(big[n, (n // 2) * 4:(n // 2 + 1) * 4], W1[n])


def _model(heads=4, layers=2, hidden=64, F=12, layer="GATConv"):
    from fitgnn_amd import network
    args = argparse.Namespace(num_layers1=layers, layer_name=layer, num_features=F, hidden=hidden, num_classes=7, heads=heads)
    torch.manual_seed(0)
    return network.Classify_node(args).eval()


def test_mhgat_query_supported_refuses_on_the_host():
    """What ops.mhgat_query_supported decides before any device is needed: layer types, count, heads and concat come first, and
    parameters that are not on the GPU are refused (so a CPU model never reaches the launcher)."""
    from fitgnn_amd import ops
    assert ops.mhgat_query_supported(_model()) is False                     # two GATConv(heads = 4) layers, but on the CPU
    assert ops.mhgat_query_supported(_model(heads=1)) is False
    assert ops.mhgat_query_supported(_model(heads=16)) is False
    assert ops.mhgat_query_supported(_model(layer="GCNConv")) is False
    assert ops.mhgat_query_supported(_model(layers=3)) is False
    assert ops.mhgat_query_supported(torch.nn.Linear(3, 3)) is False        # no conv stack at all
    m = _model()
    m.conv[1].concat = False
    assert ops.mhgat_query_supported(m) is False
