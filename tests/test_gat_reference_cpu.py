"""The float64 GAT references of tests/gat_reference.py, composed into a layer, against oracle.gnn_oracle.gat_conv and its autograd
in float64 (CPU): the references the GPU kernel tests (tests/test_gpu_gat_kernels.py) trust are themselves checked here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gat_reference as gr
from oracle import gnn_oracle as gorc


def _graph(kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "star":   # a hub row of 600 entries, leaves of 2
        n = 601
        a = np.zeros(600, dtype=np.int64); b = np.arange(1, 601)
    elif kind == "isolated":   # nodes 0..9 have no edge: their rows are the self loop alone
        n = 80
        a = rng.integers(10, n, size=200); b = rng.integers(10, n, size=200)
    else:   # random, with explicit self loops (dropped, then one added per node)
        n = 120
        a = rng.integers(0, n, size=400); b = rng.integers(0, n, size=400)
        a[:5] = b[:5]
    ei = np.unique(np.concatenate([np.stack([a, b]), np.stack([b, a])], 1), axis=1)
    return torch.tensor(ei, dtype=torch.long), n


@pytest.mark.parametrize("kind", ["random", "star", "isolated"])
@pytest.mark.parametrize("slope", [0.2, 0.0])
def test_reference_layer_equals_the_oracle_and_its_autograd(kind, slope):
    ei, n = _graph(kind, seed=3)
    torch.manual_seed(1)
    K, C = 12, 9
    x = torch.randn(n, K, dtype=torch.float64, requires_grad=True)
    W = torch.randn(C, K, dtype=torch.float64, requires_grad=True)
    att_s = torch.randn(C, dtype=torch.float64, requires_grad=True)
    att_d = torch.randn(C, dtype=torch.float64, requires_grad=True)
    b = torch.randn(C, dtype=torch.float64, requires_grad=True)
    ref = gorc.gat_conv(x, ei, W, att_s, att_d, b, negative_slope=slope)
    dout = torch.randn(n, C, dtype=torch.float64)
    ref.backward(dout)

    rowptr, col = gr.gat_csr(ei.numpy(), n)
    args = [t.detach().numpy() for t in (x, W, att_s, att_d)]
    out, mid = gr.gat_layer(*args, b.detach().numpy(), rowptr, col, slope)
    np.testing.assert_allclose(out, ref.detach().numpy(), rtol=1e-12, atol=1e-12)
    grads = gr.gat_layer_backward(*args, rowptr, col, mid, dout.numpy(), slope)
    for got, want in zip(grads, (x.grad, W.grad, att_s.grad, att_d.grad, b.grad)):
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-10, atol=1e-10)


def test_leaky_relu_gradient_at_zero_is_the_slope():
    """The softmax backward takes the slope where s == 0 exactly, as F.leaky_relu's autograd does."""
    s = torch.tensor([-1.0, 0.0, 2.0], dtype=torch.float64, requires_grad=True)
    F.leaky_relu(s, 0.25).sum().backward()
    assert s.grad.tolist() == gr.leaky_relu_grad(s.detach().numpy(), 0.25).tolist() == [0.25, 0.25, 1.0]


def test_softmax_backward_is_the_jacobian_product():
    """ds = J^T dalpha for alpha = softmax(LeakyReLU(s)) of every row, by autograd on the scores themselves."""
    rng = np.random.default_rng(0)
    lens = np.array([1, 2, 8, 9, 65, 3])
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    n = len(lens)
    col = rng.integers(0, n, size=rowptr[-1])
    a_src, a_dst = rng.standard_normal(n), rng.standard_normal(n)
    a_src[0], a_dst[0] = 0.5, -0.5   # s == 0 on every entry of row 0 whose column is 0
    dalpha = rng.standard_normal(rowptr[-1])
    alpha = gr.edge_softmax(rowptr, col, a_src, a_dst, 0.2)
    ds, da_dst = gr.softmax_bwd(rowptr, col, a_src, a_dst, alpha, dalpha, 0.2)
    s = torch.tensor(gr.edge_scores(rowptr, col, a_src, a_dst), requires_grad=True)
    e = F.leaky_relu(s, 0.2)
    rows = torch.from_numpy(gr.entry_rows(rowptr))
    parts = [torch.softmax(e[rowptr[i]:rowptr[i + 1]], 0) for i in range(n)]
    (torch.cat(parts) * torch.from_numpy(dalpha)).sum().backward()
    np.testing.assert_allclose(torch.cat(parts).detach().numpy(), alpha, rtol=1e-14)
    np.testing.assert_allclose(ds, s.grad.numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(da_dst, torch.zeros(n, dtype=torch.float64).index_add_(0, rows, s.grad).numpy(), rtol=1e-12, atol=1e-14)


def test_sddmm_and_row_sum_on_selected_rows():
    rng = np.random.default_rng(2)
    rowptr = np.array([0, 3, 3, 7, 8])
    col = rng.integers(0, 4, size=8)
    h, dout = rng.standard_normal((4, 5)), rng.standard_normal((4, 5))
    full, cond = gr.sddmm(rowptr, col, dout, h)
    assert np.allclose(full, [dout[r] @ h[c] for r, c in zip(gr.entry_rows(rowptr), col)])
    assert np.all(cond >= np.abs(full))
    sel = np.array([3, 0])
    part, _ = gr.sddmm(rowptr, col, dout[sel], h, sel=sel)
    on = np.zeros(8, dtype=bool); on[0:3] = on[7:8] = True
    assert np.allclose(part[on], full[on], rtol=1e-14, atol=0) and np.isnan(part[~on]).all()
    y, ya = gr.row_sum(rowptr, full)
    assert np.allclose(y, [full[0:3].sum(), 0.0, full[3:7].sum(), full[7]]) and np.all(ya >= np.abs(y))
