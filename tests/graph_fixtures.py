"""Graph builders shared by the GPU test modules (test infrastructure only)."""
import numpy as np
import torch


def star_blocks(sizes, centres, seed, extra=0.02):
    """Block-diagonal batch of star-shaped subgraphs: in every block the first `centres` rows link to all the others
    (--extra_node subgraphs, utils.py:235-239), plus a few random leaf -- leaf edges."""
    rng = np.random.default_rng(seed)
    src, dst, off = [], [], 0
    for s in sizes:
        c = min(centres, max(s - 1, 0))
        for h in range(c):
            leaves = np.arange(c, s)
            src += [off + h] * len(leaves) + (off + leaves).tolist()
            dst += (off + leaves).tolist() + [off + h] * len(leaves)
        m = int(extra * s * s)
        if m and s > 2:
            a, b = rng.integers(0, s, size=m), rng.integers(0, s, size=m)
            k = a != b
            src += (off + a[k]).tolist() + (off + b[k]).tolist()
            dst += (off + b[k]).tolist() + (off + a[k]).tolist()
        off += s
    return torch.tensor(np.unique(np.array([src, dst]), axis=1), dtype=torch.long), off


def subgraph_batches(seed=0):
    """A small Gs: 40 clusters over a 400-node graph with extra nodes, as loader batches of 8 subgraphs."""
    from fitgnn_amd import data as fdata

    ei = fdata.synthetic_graph(400, 900, seed=seed)
    rng = np.random.default_rng(seed)
    assign = rng.integers(0, 40, size=400); assign[:40] = np.arange(40)
    sub = fdata.assemble_subgraphs(ei, 400, assign, 40, extra_node=True)
    X = torch.from_numpy(rng.standard_normal((400, 24)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, 4, size=400))
    tm = torch.from_numpy(rng.random(400) < 0.3)
    batch = fdata.SubgraphBatch(sub, X, y, tm, device="cuda")
    cpu = []
    for r0, r1 in batch.slice_batches(8):
        e = batch.edge_index.cpu()
        k = (e[0] >= r0) & (e[0] < r1)
        cpu.append(dict(x=batch.x[r0:r1].cpu(), edge_index=e[:, k] - r0, y=batch.y[r0:r1].cpu(), train_mask=batch.train_mask[r0:r1].cpu()))
    return batch, cpu
