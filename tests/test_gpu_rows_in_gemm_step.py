"""GPU tier: the step's use of the exact product's row lists (OpConfig.rows_in_gemm), and the column-sum partials of the
whole-subgraph kernel without a fill.

1. FusedGCNLastLayerRows and FusedGCNLayerRows, forward and backward, with rows_in_gemm on (the products read the kept rows where they
   lie in A_hat X) and off (they read a gathered copy): outputs and every gradient torch.equal, at dropout 0.5 and 0, on a
   block-diagonal batch split into large and padding block records.
2. The two-hop backward and spmm_graph_dz with their partial buffers poisoned with NaN (FITGNN_POISON's switch): db is finite and
   torch.equal to the run whose partial buffers were zero-filled -- the kernel writes the row of every record, a padding record's
   as zeros; the extra row of the two-hop pass is zeroed where no row lies outside the blocks.
"""
import numpy as np
import pytest
import torch
from graph_fixtures import star_blocks

from test_gpu_step_kernels import L  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [100, 7, 17, 300, 3, 3, 64, 33, 2, 1000, 5, 5, 40]


def _split_graph(sizes=SIZES, centres=2, seed=11):
    """A batch of stars whose blocks beyond 16 rows run on the whole-subgraph kernel: its record table is padded per XCD."""
    from fitgnn_amd import csr
    ei, n = star_blocks(sizes, centres, seed=seed)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    g = csr.CSRGraph(ei.cuda(), n, mode="gcn", ptr=ptr, block_limit=4096)
    for side in (g.f, g.t):
        assert side.blocks is not None
        live = int((side.blocks[:, 1] > side.blocks[:, 0]).sum())
        assert 0 < live < int(side.blocks.shape[0]), "the batch has large and padding block records"
    return g, n


@pytest.mark.parametrize("p", [0.5, 0.0])
def test_fused_rows_layers_read_the_aggregate_in_place(L, p):
    from fitgnn_amd import ops
    g, n = _split_graph()
    K, H, C = 64, 256, 47
    torch.manual_seed(5)
    rows = torch.randperm(n).cuda()[: n // 3].sort().values
    labels = torch.randint(0, C, (rows.numel(),)).cuda()
    base = [torch.randn(n, K).cuda(), torch.randn(H, K).cuda() / 8, torch.randn(H).cuda(), torch.randn(C, H).cuda() / 8, torch.randn(C).cuda()]
    G = torch.randn(rows.numel(), H).cuda()
    last, mid = [], []
    for through in (True, False):
        cfg = ops.OpConfig(rows_in_gemm=through)
        X, W, b, Wl, bl = (t.clone().requires_grad_(True) for t in base)
        y = ops.FusedGCNLastLayerRows.apply(X, W, b, Wl, bl, g, p, True, 1234, None, rows, cfg, None, True)
        loss = torch.nn.functional.cross_entropy(y, labels)
        loss.backward()
        last.append([y.detach(), loss.detach()] + [t.grad for t in (X, W, b, Wl, bl)])
        X, W, b = (t.clone().requires_grad_(True) for t in base[:3])
        out = ops.FusedGCNLayerRows.apply(X, W, b, g, p, True, 1234, None, rows, cfg)
        (out * G).sum().backward()
        mid.append([out.detach()] + [t.grad for t in (X, W, b)])
    for name, u, v in zip(("logits", "loss", "dX", "dW", "db", "dWl", "dbl"), *last):
        assert torch.equal(u, v), f"FusedGCNLastLayerRows {name}"
    for name, u, v in zip(("out", "dX", "dW", "db"), *mid):
        assert torch.equal(u, v), f"FusedGCNLayerRows {name}"
    assert (last[0][0] != 0).any().item() and (mid[0][0] != 0).any().item() and torch.isfinite(last[0][3]).all().item()


@pytest.mark.parametrize("H", [512, 96])
@pytest.mark.parametrize("sizes,loss", [(SIZES, "centres"), (SIZES, "random"), ([70] * 20, "centres")])
def test_column_sum_partials_need_no_fill(L, monkeypatch, H, sizes, loss):
    from fitgnn_amd import ops
    from fitgnn_amd._lib import EPI_DROPOUT, EPI_ELU
    g, n = _split_graph(sizes, centres=2, seed=H + len(sizes))
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    torch.manual_seed(H + n)
    if loss == "centres":
        rows = torch.cat([torch.arange(2) + int(o) for o in ptr[:-1]]).cuda().sort().values
    else:
        rows = torch.randperm(n).cuda()[: n // 3].sort().values
    k = int(rows.numel())
    Xc = torch.cat([torch.randn(k, H).cuda(), torch.zeros(ops.ZERO_ROWS, H).cuda()])
    X = torch.randn(n, H).cuda()
    prev = torch.randn(n, H).cuda() * (torch.rand(n, H).cuda() > 0.3)
    pos = ops._compact_positions(g, rows)
    flags, p, seed = EPI_ELU | EPI_DROPOUT, 0.5, 77
    cfg = ops.OpConfig()

    def run():
        link = ops.EpilogueLink()
        link.record(True, p, seed, None, True, g=g)
        assert ops.two_hop_supported(g, link, Xc, prev, cfg)
        Y, db = ops.spmm_two_hop_blocks(g, Xc, prev, rows, pos, link, cfg=cfg)
        dZ, db2 = ops.spmm_graph_dz(g, X, prev, flags, p=p, seed=seed, want_db=True, cfg=cfg)
        return Y, db, dZ, db2

    scratch = ops._scratch
    monkeypatch.setattr(ops, "_scratch", lambda shape, device: torch.zeros(shape, dtype=torch.float32, device=device))   # zero-filled partials
    want = run()
    monkeypatch.setattr(ops, "_scratch", scratch)
    monkeypatch.setattr(ops, "_POISON", True)
    got = run()
    for name, u, v in zip(("two-hop Y", "two-hop db", "dZ", "dz db"), got, want):
        assert torch.isfinite(u).all().item(), f"{name}: a row of the partials was not written"
        assert torch.equal(u, v), name
    if len(sizes) == 20:   # every row in a block: the extra partial row of the two-hop pass has no rows to sum
        assert ops._two_hop_block_index(g, rows, pos)["tile_zt"].numel() == 0
