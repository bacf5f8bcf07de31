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
