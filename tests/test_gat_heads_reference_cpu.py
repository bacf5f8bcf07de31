"""CPU tier: tests/gat_heads_reference.py (the float64 statements the multi-head GPU tests compare against) is tied to what is already
pinned: at one head it is gat_reference.gat_layer and its backward; at several heads it is the column-wise concatenation (or, with
concat=False, the mean) of oracle.gnn_oracle.gat_conv run once per head on that head's slice of W, att and bias; and its backward
is torch-CPU float64 autograd of a dense restatement of the layer."""
import numpy as np
import pytest
import torch

import gat_heads_reference as ghr
import gat_reference as gr
from oracle import gnn_oracle as gorc


def _graph(n, m, seed):
    """A random undirected graph without repeated edges, some self loops in the input (GATConv replaces them), one isolated node."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n - 1, size=m), rng.integers(0, n - 1, size=m)
    ei = np.unique(np.concatenate([np.stack([a, b]), np.stack([b, a])], 1), axis=1)
    return torch.tensor(ei, dtype=torch.long)


def _params(n, fin, heads, C, concat, seed):
    rng = np.random.default_rng(seed)
    return dict(x=rng.standard_normal((n, fin)), W=rng.standard_normal((heads * C, fin)) / np.sqrt(fin),
                att_src=rng.standard_normal(heads * C), att_dst=rng.standard_normal(heads * C),
                bias=rng.standard_normal(heads * C if concat else C))


@pytest.mark.parametrize("C", [1, 5, 8])
def test_one_head_is_the_single_head_reference(C):
    n = 40
    ei = _graph(n, 90, C)
    rowptr, col = gr.gat_csr(ei.numpy(), n)
    P = _params(n, 6, 1, C, True, C)
    out, mid = ghr.gat_heads_layer(P["x"], P["W"], P["att_src"], P["att_dst"], P["bias"], rowptr, col, heads=1)
    ref, rmid = gr.gat_layer(P["x"], P["W"], P["att_src"], P["att_dst"], P["bias"], rowptr, col)
    assert np.allclose(out, ref, rtol=0, atol=1e-13)
    assert np.allclose(mid["alpha"][:, 0], rmid["alpha"], rtol=0, atol=1e-15)
    dout = np.random.default_rng(1).standard_normal(out.shape)
    got = ghr.gat_heads_layer_backward(P["x"], P["W"], P["att_src"], P["att_dst"], rowptr, col, mid, dout, heads=1)
    want = gr.gat_layer_backward(P["x"], P["W"], P["att_src"], P["att_dst"], rowptr, col, rmid, dout)
    for g, w in zip(got, want):
        assert np.allclose(g, w, rtol=0, atol=1e-12 * max(1.0, np.abs(w).max()))


def _oracle_heads(P, ei, heads, C):
    """One gnn_oracle.gat_conv run per head on that head's slices, without bias: a list of [n, C] tensors."""
    x = torch.from_numpy(P["x"])
    outs = []
    for k in range(heads):
        sl = slice(k * C, (k + 1) * C)
        outs.append(gorc.gat_conv(x, ei, torch.from_numpy(P["W"][sl]), torch.from_numpy(P["att_src"][sl]),
                                  torch.from_numpy(P["att_dst"][sl]), None))
    return outs


@pytest.mark.parametrize("heads", [2, 3, 8])
def test_concat_is_the_per_head_oracle_side_by_side(heads):
    n, C = 50, 4
    ei = _graph(n, 120, heads)
    rowptr, col = gr.gat_csr(ei.numpy(), n)
    P = _params(n, 7, heads, C, True, heads)
    out, _ = ghr.gat_heads_layer(P["x"], P["W"], P["att_src"], P["att_dst"], P["bias"], rowptr, col, heads=heads)
    ref = torch.cat(_oracle_heads(P, ei, heads, C), dim=1).numpy() + P["bias"]
    assert np.abs(out - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("heads", [2, 3, 8])
def test_mean_is_the_mean_of_the_per_head_oracle_plus_bias(heads):
    n, C = 50, 4
    ei = _graph(n, 120, 10 + heads)
    rowptr, col = gr.gat_csr(ei.numpy(), n)
    P = _params(n, 7, heads, C, False, heads)
    out, _ = ghr.gat_heads_layer(P["x"], P["W"], P["att_src"], P["att_dst"], P["bias"], rowptr, col, heads=heads, concat=False)
    ref = torch.stack(_oracle_heads(P, ei, heads, C), dim=0).mean(0).numpy() + P["bias"]
    assert out.shape == (n, C)
    assert np.abs(out - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def _dense_layer(x, W, att_src, att_dst, bias, adj, heads, concat, slope):
    """The layer on a dense 0 / 1 adjacency (adj[i, j] = 1: j -> i, self loops included) in torch: masked softmax over j per head."""
    n = x.shape[0]
    h3 = (x @ W.t()).view(n, heads, -1)
    a_s = (h3 * att_src.view(1, heads, -1)).sum(-1)
    a_d = (h3 * att_dst.view(1, heads, -1)).sum(-1)
    e = torch.nn.functional.leaky_relu(a_s.unsqueeze(0) + a_d.unsqueeze(1), slope)          # [i, j, hd]
    e = e.masked_fill(adj.unsqueeze(2) == 0, float("-inf"))
    alpha = torch.softmax(e, dim=1)
    out = torch.einsum("ijh,jhc->ihc", alpha, h3)
    out = out.reshape(n, -1) if concat else out.mean(1)
    return out + bias


@pytest.mark.parametrize("heads,concat", [(1, True), (2, True), (3, True), (8, True), (2, False), (8, False)])
def test_backward_is_float64_autograd_of_a_dense_restatement(heads, concat):
    n, C, slope = 30, 3, 0.2
    ei = _graph(n, 70, 20 + heads)
    rowptr, col = gr.gat_csr(ei.numpy(), n)
    adj = torch.zeros(n, n, dtype=torch.float64)
    adj[torch.from_numpy(gr.entry_rows(rowptr)), torch.from_numpy(col)] = 1.0
    P = _params(n, 5, heads, C, concat, 30 + heads)
    T = {k: torch.from_numpy(v).requires_grad_(True) for k, v in P.items()}
    ref = _dense_layer(T["x"], T["W"], T["att_src"], T["att_dst"], T["bias"], adj, heads, concat, slope)
    out, mid = ghr.gat_heads_layer(P["x"], P["W"], P["att_src"], P["att_dst"], P["bias"], rowptr, col, heads=heads, concat=concat,
                                   slope=slope)
    assert np.abs(out - ref.detach().numpy()).max() <= 1e-12 * max(1.0, float(ref.detach().abs().max()))
    dout = np.random.default_rng(2).standard_normal(out.shape)
    ref.backward(torch.from_numpy(dout))
    got = ghr.gat_heads_layer_backward(P["x"], P["W"], P["att_src"], P["att_dst"], rowptr, col, mid, dout, heads=heads, concat=concat,
                                       slope=slope)
    for g, k in zip(got, ("x", "W", "att_src", "att_dst", "bias")):
        w = T[k].grad.numpy()
        assert np.abs(g - w).max() <= 1e-11 * max(1.0, np.abs(w).max()), k


def test_helpers_report_the_condition_sums():
    """The condition sums are the same operations on absolute values: equal to the result where every term is positive."""
    rng = np.random.default_rng(3)
    rowptr, col = np.array([0, 2, 2, 5]), np.array([0, 2, 1, 0, 2])
    heads, C = 2, 3
    h, d = np.abs(rng.standard_normal((3, heads * C))), np.abs(rng.standard_normal((3, heads * C)))
    att = np.abs(rng.standard_normal(heads * C))
    a, _, ca, _ = ghr.scores(h, att, att, heads)
    assert np.allclose(a, ca)
    v, cv = ghr.sddmm(rowptr, col, d, h, heads)
    assert v.shape == (5, heads) and np.allclose(v, cv)
    alpha = np.abs(rng.standard_normal((5, heads)))
    y, cy = ghr.aggregate(rowptr, col, alpha, h)
    assert np.allclose(y, cy) and np.all(y[1] == 0)
    assert np.allclose(ghr.column_sum(rowptr, col, alpha)[1], alpha[2])
