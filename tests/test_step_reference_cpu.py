"""The float64 references of tests/step_reference.py against torch's own float64 operations and autograd (CPU), and the dropout-hash
replica against literal values of csrc/common.h: the references the GPU kernel tests (tests/test_gpu_step_kernels.py) trust are
themselves checked here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import step_reference as sr

D = torch.float64


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_allclose(a, b, rtol=tol, atol=tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# the hash replica
# ---------------------------------------------------------------------------------------------------------------------------------
# (seed, group) -> dropout_bits(seed, group): printed by a host build of a ten-line C++ program that includes csrc/common.h and
# calls fitgnn::dropout_bits on these arguments (hipcc, no device code).  Groups above 2^32 exercise the high word's multiplier.
HASH_LITERALS = [
    (0x0000000000000000, 0x0, 0x929AE26000000000),
    (0x0000000000000000, 0x1, 0x3FB01A8C11FD02EB),
    (0x0000000000000000, 0x3039, 0xBBCB75FE0F8066CA),
    (0x0000000000000000, 0x100000003, 0x24F92EF101E95D13),
    (0x0000000000000001, 0x1, 0x3FB01A8CB19FEA7C),
    (0x9E3779B97F4A7C15, 0x0, 0x25B6F7C14BC0FBEB),
    (0x9E3779B97F4A7C15, 0x3039, 0x538A006D2FC0BD72),
    (0x9E3779B97F4A7C15, 0x100000003, 0xAE79AE4D4CBF75E3),
    (0xFFFFFFFF00000001, 0x1, 0xB35C9A78B19FEA7C),
    (0xFFFFFFFF00000001, 0x100000003, 0x83902560E5E9DD3B),
]


@pytest.mark.parametrize("seed,group,bits", HASH_LITERALS)
def test_dropout_bits_replica_matches_common_h(seed, group, bits):
    assert int(sr.dropout_bits(seed, np.array([group], dtype=np.uint64))[0]) == bits


def test_fmix32_and_threshold_literals():
    assert int(sr.fmix32(0x12345678)) == 0xE37CD1BC
    assert [sr.dropout_threshold(p) for p in (0.5, 0.3, 0.1)] == [32768, 19660, 6553]


def test_dropout_keep_takes_group_and_sub_index_from_the_flat_index():
    seed, H, p = 0x9E3779B97F4A7C15, 12, 0.5
    rows, cols = np.meshgrid(np.arange(7), np.arange(H), indexing="ij")
    keep = sr.dropout_keep(seed, rows, cols, H, p)
    idx = (rows * H + cols).astype(np.uint64)
    bits = sr.dropout_bits(seed, idx >> np.uint64(2))
    want = ((bits >> ((idx & np.uint64(3)) * np.uint64(16))) & np.uint64(0xFFFF)) >= np.uint64(32768)
    assert np.array_equal(keep, want)
    # the same decision for the same flat index, whatever the row width says about rows
    assert np.array_equal(sr.dropout_keep(seed, 0, np.arange(7 * H), 7 * H, p), keep.reshape(-1))
    assert np.array_equal(sr.keep_matrix(seed, [3, 0], H, p), keep[[3, 0]])
    assert 0.3 < keep.mean() < 0.7


def test_resolve_seed_reads_the_device_word_only_with_both_flags():
    words = {0x1000: 77}
    assert sr.resolve_seed(0x1000, sr.EPI_SEED_DEVICE | sr.EPI_DROPOUT, words.__getitem__) == 77
    assert sr.resolve_seed(0x1000, sr.EPI_DROPOUT, words.__getitem__) == 0x1000
    assert sr.resolve_seed(0x1000, sr.EPI_SEED_DEVICE, words.__getitem__) == 0x1000


# ---------------------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 47, 65])
def test_softmax_nll_matches_torch_and_its_autograd(C):
    rng = np.random.default_rng(C)
    z = rng.normal(0, 3, size=(40, C))
    z[5] *= 20.0
    idx = rng.permutation(40)[:23]
    labels = rng.integers(0, C, size=23)
    scale = 0.125
    loss, dz, lse = sr.softmax_nll(z, idx, labels, scale)
    zt = torch.tensor(z, dtype=D, requires_grad=True)
    lt = F.nll_loss(F.log_softmax(zt[torch.tensor(idx)], 1), torch.tensor(labels), reduction="sum") * scale
    lt.backward()
    _close(loss, lt.item())
    _close(dz, zt.grad.numpy())
    _close(lse, torch.logsumexp(zt.detach()[torch.tensor(idx)], 1).numpy())
    assert np.all(dz[np.setdiff1d(np.arange(40), idx)] == 0)


def test_softmax_nll_refuses_repeated_rows():
    with pytest.raises(AssertionError):
        sr.softmax_nll(np.zeros((4, 3)), [1, 1], [0, 0], 1.0)


def test_l1_loss_matches_torch_and_its_autograd_with_ties():
    rng = np.random.default_rng(1)
    out = rng.integers(-3, 4, size=300) / 4.0
    tgt = rng.integers(-3, 4, size=300) / 4.0
    assert np.any(out == tgt)
    loss, grad = sr.l1_loss(out, tgt, 0.25)
    ot = torch.tensor(out, dtype=D, requires_grad=True)
    lt = F.l1_loss(ot, torch.tensor(tgt, dtype=D), reduction="sum") * 0.25
    lt.backward()
    _close(loss, lt.item())
    _close(grad, ot.grad.numpy())
    assert np.all(grad[out == tgt] == 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_adam_matches_torch_optim_adam_over_50_steps(wd):
    rng = np.random.default_rng(2)
    p0 = rng.normal(size=64)
    grads = rng.normal(size=(50, 64)) * np.linspace(1e-3, 10, 64)
    pt = torch.tensor(p0, dtype=D, requires_grad=True)
    opt = torch.optim.Adam([pt], lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(64), np.zeros(64)
    for t in range(50):
        # the gradient arrives in two parts (the accumulated buffer and this backward's own), as fitgnn_adam_step_acc_f32 takes it
        half = grads[t] / 4
        p, g, m, v = sr.adam(p, grads[t] - half, half, m, v, t, 0.01, 0.9, 0.999, 1e-8, wd)
        _close(g, grads[t], 1e-15)
        pt.grad = torch.tensor(grads[t], dtype=D)
        opt.step()
    _close(p, pt.detach().numpy(), 1e-12)
    st = opt.state[pt]
    _close(m, st["exp_avg"].numpy(), 1e-12)
    _close(v, st["exp_avg_sq"].numpy(), 1e-12)


# ---------------------------------------------------------------------------------------------------------------------------------
# epilogue, head, narrow-K layer
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", [0, sr.EPI_BIAS, sr.EPI_ELU, sr.EPI_DROPOUT, sr.EPI_BIAS | sr.EPI_ELU | sr.EPI_DROPOUT])
def test_epilogue_forward_and_backward_match_torch_autograd(epi):
    rng = np.random.default_rng(epi)
    n, H, p = 30, 12, 0.3
    z = rng.normal(size=(n, H)); b = rng.normal(size=H)
    keep = sr.keep_matrix(1234, np.arange(n), H, p)
    zt = torch.tensor(z, dtype=D, requires_grad=True); bt = torch.tensor(b, dtype=D, requires_grad=True)
    y = zt + bt if epi & sr.EPI_BIAS else zt
    if epi & sr.EPI_ELU:
        y = F.elu(y)
    if epi & sr.EPI_DROPOUT:   # dropout by the replica's mask: kept entries scaled by 1 / (1 - p) with p the fp32 value
        y = y * torch.tensor(keep, dtype=D) / (1.0 - float(np.float32(p)))
    ref = sr.epilogue_fwd(z, b, epi, p, keep)
    _close(ref, y.detach().numpy())
    g = rng.normal(size=(n, H))
    y.backward(torch.tensor(g, dtype=D))
    dZ, db, _ = sr.epilogue_bwd(g, ref, epi, p, keep)
    _close(dZ, zt.grad.numpy(), 1e-10)
    if epi & sr.EPI_BIAS:
        _close(db, bt.grad.numpy(), 1e-10)


def test_head_backward_and_linear_match_torch_autograd():
    rng = np.random.default_rng(5)
    n, H, C, p = 25, 16, 5, 0.25
    z = rng.normal(size=(n, H)); Wl = rng.normal(size=(C, H)); bl = rng.normal(size=C)
    keep = sr.keep_matrix(99, np.arange(n), H, p)
    epi = sr.EPI_ELU | sr.EPI_DROPOUT
    zt = torch.tensor(z, dtype=D, requires_grad=True)
    Wt = torch.tensor(Wl, dtype=D, requires_grad=True); bt = torch.tensor(bl, dtype=D, requires_grad=True)
    out = F.elu(zt) * torch.tensor(keep, dtype=D) / (1.0 - float(np.float32(p)))
    y = out @ Wt.t() + bt
    o = sr.epilogue_fwd(z, None, epi, p, keep)
    y_ref, _ = sr.head_rows(o, Wl, bl)
    _close(y_ref, y.detach().numpy())
    dy = rng.normal(size=(n, C))
    y.backward(torch.tensor(dy, dtype=D))
    dZ, db, dWl, _, _ = sr.epilogue_bwd_head(dy, Wl, o, epi, p, keep)
    _close(dZ, zt.grad.numpy(), 1e-10)
    _close(dWl, Wt.grad.numpy(), 1e-10)
    _close(sr.colsum(dy)[0], bt.grad.numpy())
    sel = np.array([7, 2, 19])
    dy_s, o_s = sr.select_rows(sel, False, dy, o)
    assert np.array_equal(o_s, o[sel])
    assert np.array_equal(sr.select_rows(sel, True, dy)[0], dy[:3])


@pytest.mark.parametrize("epi", [0, sr.EPI_BIAS | sr.EPI_ELU, sr.EPI_BIAS | sr.EPI_ELU | sr.EPI_DROPOUT])
def test_dense_narrow_k_and_narrow_atb_match_a_linear_layer_and_its_autograd(epi):
    rng = np.random.default_rng(7)
    n, K, H, p = 33, 11, 16, 0.5
    a = rng.normal(size=(n, K)); W = rng.normal(size=(H, K)); b = rng.normal(size=H)
    keep = sr.keep_matrix(5, np.arange(n), H, p)
    Wt = torch.tensor(W, dtype=D, requires_grad=True); bt = torch.tensor(b, dtype=D, requires_grad=True)
    y = torch.tensor(a, dtype=D) @ Wt.t() + (bt if epi & sr.EPI_BIAS else 0.0)
    if epi & sr.EPI_ELU:
        y = F.elu(y)
    if epi & sr.EPI_DROPOUT:
        y = y * torch.tensor(keep, dtype=D) / (1.0 - p)
    out, _, _ = sr.dense_narrow_k(a, W, b, epi, p, keep)
    _close(out, y.detach().numpy())
    d = rng.normal(size=(n, H))
    y.backward(torch.tensor(d, dtype=D))
    dW, db, _, _ = sr.narrow_atb(d, a, prev=out, epi=epi & ~sr.EPI_BIAS, p=p, keep=keep)
    _close(dW, Wt.grad.numpy(), 1e-10)
    if epi & sr.EPI_BIAS:
        _close(db, bt.grad.numpy(), 1e-10)
    dW0, db0, _, _ = sr.narrow_atb(d, a)
    _close(dW0, d.T @ a); _close(db0, d.sum(0))
