"""The float64 references of tests/pool_reference.py against torch's own float64 operations and autograd (CPU), and the max pool's
tie / -inf / NaN rule on hand-written segments: the references the GPU kernel tests (tests/test_gpu_pool_kernels.py) trust are
themselves checked here."""
import numpy as np
import pytest
import torch

import pool_reference as pr

D = torch.float64
NAN, INF = float("nan"), float("inf")


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_allclose(a, b, rtol=tol, atol=tol)


def _index(rng, lengths, n_rows, distinct=False):
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    members = rng.permutation(n_rows)[:off[-1]] if distinct else rng.integers(0, n_rows, size=off[-1])
    return off, members.astype(np.int64)


def _seg_ids(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


LENGTHS = [0, 1, 3, 4, 5, 17, 0, 40]


@pytest.mark.parametrize("distinct", [False, True])
def test_segment_sum_and_expand_against_index_add(distinct):
    rng = np.random.default_rng(1)
    off, members = _index(rng, LENGTHS, 90, distinct)
    X = torch.from_numpy(rng.normal(size=(90, 7))).requires_grad_(True)
    seg = torch.from_numpy(_seg_ids(off))
    out = torch.zeros(len(LENGTHS), 7, dtype=D).index_add_(0, seg, X[torch.from_numpy(members)])
    _close(pr.segment_sum(off, members, X.detach().numpy()), out.detach().numpy())
    if distinct:   # the adjoint of a sum (times a per-segment scale) over disjoint segments is segment_expand
        g = torch.from_numpy(rng.normal(size=(len(LENGTHS), 7)))
        scale = torch.from_numpy(rng.uniform(0.5, 2.0, size=len(LENGTHS)))
        (out * scale[:, None] * g).sum().backward()
        seg_of_row = np.full(90, -1, dtype=np.int64)
        seg_of_row[members] = seg.numpy()
        _close(pr.segment_expand(g.numpy(), seg_of_row, scale.numpy()), X.grad.numpy())
        _close(pr.segment_expand(g.numpy(), seg_of_row, None), pr.segment_expand(g.numpy(), seg_of_row, np.ones(len(LENGTHS))))
        assert np.all(pr.segment_expand(g.numpy(), seg_of_row, None)[seg_of_row < 0] == 0)


def test_segment_max_against_amax_and_autograd():
    rng = np.random.default_rng(2)
    off, members = _index(rng, LENGTHS, 90, distinct=True)
    X = torch.from_numpy(rng.normal(size=(90, 6))).requires_grad_(True)   # continuous values: no ties, amax's gradient is one-hot
    seg = torch.from_numpy(_seg_ids(off))
    sel = X[torch.from_numpy(members)]
    ref = torch.full((len(LENGTHS), 6), -INF, dtype=D).scatter_reduce(0, seg[:, None].expand_as(sel), sel, reduce="amax", include_self=True)
    out, arg = pr.segment_max(off, members, X.detach().numpy())
    assert np.array_equal(out, ref.detach().numpy())
    empty = np.diff(off) == 0
    assert np.all(arg[empty] == -1) and np.all(out[empty] == -INF) and np.all(arg[~empty] >= 0)
    g = rng.normal(size=out.shape)
    (torch.where(torch.isfinite(ref), ref, torch.zeros((), dtype=D)) * torch.from_numpy(g)).sum().backward()
    _close(pr.segment_max_bwd(g, arg, 90), X.grad.numpy())
    # members None: the segments are row ranges
    out2, arg2 = pr.segment_max(off, None, X.detach().numpy())
    for s in range(len(LENGTHS)):
        rows = np.arange(off[s], off[s + 1])
        if rows.size:
            assert np.array_equal(out2[s], X.detach().numpy()[rows].max(0))
            assert np.array_equal(arg2[s], rows[X.detach().numpy()[rows].argmax(0)])


def test_segment_max_rule_on_ties_inf_and_nan():
    #            col 0: tie of two   col 1: tie of three   col 2: all -inf   col 3: NaN first   col 4: NaN middle   col 5: NaN last
    X = np.array([[1.0, 5.0, -INF, 0.0, NAN, 7.0],      # row 0
                  [2.0, 5.0, -INF, 4.0, NAN, 8.0],      # row 1
                  [0.0, 1.0, -INF, 3.0, 0.0, NAN],      # row 2
                  [2.0, 5.0, -INF, NAN, 1.0, 1.0],      # row 3
                  [9.0, 9.0, 9.0, 9.0, 9.0, 9.0]])      # row 4: no segment's member
    off = np.array([0, 4, 4, 5])
    members = np.array([3, 1, 0, 2, 2])                # segment 0 = rows 3, 1, 0, 2 in that order; segment 1 empty; segment 2 = row 2
    out, arg = pr.segment_max(off, members, X)
    # ties go to the first member in SEGMENT order (row 3), not to the smallest row id (row 1 / row 0)
    assert out[0].tolist()[:3] == [2.0, 5.0, -INF] and arg[0].tolist()[:3] == [3, 3, 3]
    assert np.all(np.isnan(out[0, 3:]))
    assert arg[0].tolist()[3:] == [3, 1, 2]            # the first NaN member in segment order (of rows 1 and 0 in column 4: row 1)
    assert np.all(out[1] == -INF) and np.all(arg[1] == -1)
    assert np.array_equal(out[2], X[2], equal_nan=True) and np.all(arg[2] == 2)
    # the same NaN pattern as torch's amax over the same members
    t = torch.from_numpy(X[members[:4]])
    assert np.array_equal(np.isnan(out[0]), torch.isnan(t.amax(0)).numpy())
    # the backward puts g on exactly the arg rows; a segment without members writes nothing
    g = np.arange(1.0, 19.0).reshape(3, 6)
    dst = pr.segment_max_bwd(g[:2], arg[:2], 5)
    want = np.zeros((5, 6))
    for c in range(6):
        want[arg[0, c], c] = g[0, c]
    assert np.array_equal(dst, want) and np.count_nonzero(dst) == 6
    with pytest.raises(AssertionError):
        pr.segment_max_bwd(g, arg, 5)                  # segments 0 and 2 share row 2 as a maximum: not disjoint


@pytest.mark.parametrize("with_bias", [False, True])
def test_pool_head_and_its_backward_against_autograd(with_bias):
    rng = np.random.default_rng(3)
    lengths = [0, 1, 9, 2, 30]
    n_rows, F, C = 60, 8, 3
    off, members = _index(rng, lengths, n_rows, distinct=True)
    seg = torch.from_numpy(_seg_ids(off))
    X = torch.from_numpy(rng.normal(size=(n_rows, F))).requires_grad_(True)
    W = torch.from_numpy(rng.normal(size=(C, F))).requires_grad_(True)
    b = torch.from_numpy(rng.normal(size=C)).requires_grad_(True) if with_bias else None
    inv = 1.0 / np.maximum(np.diff(off), 1)
    pooled_t = torch.zeros(len(lengths), F, dtype=D).index_add_(0, seg, X[torch.from_numpy(members)]) * torch.from_numpy(inv)[:, None]
    y_t = pooled_t @ W.t() + (b if with_bias else 0.0)
    pooled, y = pr.pool_head(off, members, X.detach().numpy(), inv, W.detach().numpy(), None if b is None else b.detach().numpy())
    _close(pooled, pooled_t.detach().numpy())
    _close(y, y_t.detach().numpy())
    dy = rng.normal(size=y.shape)
    (y_t * torch.from_numpy(dy)).sum().backward()
    seg_of_row = np.full(n_rows, -1, dtype=np.int64)
    seg_of_row[members] = seg.numpy()
    dx, dW, db = pr.pool_head_bwd(dy, W.detach().numpy(), pooled, seg_of_row, inv)
    _close(dx, X.grad.numpy())
    _close(dW, W.grad.numpy())
    if with_bias:
        _close(db, b.grad.numpy())
    assert np.all(dx[seg_of_row < 0] == 0)


def test_sum_leading():
    part = np.random.default_rng(4).normal(size=(91, 12))
    _close(pr.sum_leading(part), torch.from_numpy(part).sum(0).numpy())
    _close(pr.sum_leading(part[:1]), part[0])
