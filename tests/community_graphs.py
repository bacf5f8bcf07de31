"""numpy-built graphs shared by the community detection tests (no networkx, no product import): (edge_index, num_nodes)."""
import numpy as np


def planted4():
    """The construction of test_host_logic.py::test_community_detection_substitute_and_merge: four dense blocks of 60, 40, 25 and
    10 nodes joined by three single edges."""
    rng = np.random.default_rng(0)
    sizes, edges, off = [60, 40, 25, 10], [], 0
    for s in sizes:
        a = rng.integers(0, s, size=6 * s); b = rng.integers(0, s, size=6 * s)
        k = a != b
        edges.append(np.stack([a[k] + off, b[k] + off])); off += s
    ei = np.concatenate(edges + [np.array([[0, 60, 100], [60, 100, 125]])], axis=1)
    return np.unique(np.concatenate([ei, ei[::-1]], axis=1), axis=1), off


PLANTED4_SIZES = [60, 40, 25, 10]


def ring(n=64):
    i = np.arange(n)
    return np.stack([i, (i + 1) % n]), n


def sbm(blocks=8, size=150, p_in=0.084, p_out=0.004, seed=3):
    rng = np.random.default_rng(seed)
    n = blocks * size
    iu, ju = np.triu_indices(n, 1)
    p = np.where(iu // size == ju // size, p_in, p_out)
    keep = rng.random(iu.size) < p
    return np.stack([iu[keep], ju[keep]]), n


def gnm(n=400, m=1600, seed=5):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    pick = rng.choice(iu.size, size=m, replace=False)
    return np.stack([iu[pick], ju[pick]]), n


def double_star(leaves=4096):
    """Hubs 0 and 1, joined, each adjacent to every leaf: both rows hold leaves + 1 > 4096 entries."""
    leaf = np.arange(2, leaves + 2)
    src = np.concatenate([[0], np.zeros(leaves, dtype=np.int64), np.ones(leaves, dtype=np.int64)])
    dst = np.concatenate([[1], leaf, leaf])
    return np.stack([src, dst]), leaves + 2


def near_limit():
    """A hand-made level graph (rowptr, col, w) of four nodes whose weights bring M2 to 2^31 - 2: the largest products a score
    and the statistics can meet."""
    big = 2 ** 28
    e = {(0, 1): big, (1, 0): big, (2, 3): big, (3, 2): big, (0, 0): 2 * big - 4, (2, 2): 2 * big, (1, 2): 1, (2, 1): 1}
    keys = sorted(e)
    rowptr = np.zeros(5, dtype=np.int64)
    np.cumsum(np.bincount([i for i, _ in keys], minlength=4), out=rowptr[1:])
    return rowptr, np.array([j for _, j in keys], dtype=np.int64), np.array([e[k] for k in keys], dtype=np.int64)


NEAR_LIMIT_COMMS = [np.arange(4), np.array([0, 0, 2, 2]), np.array([3, 1, 1, 3])]
