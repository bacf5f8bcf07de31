"""CPU restatement of the modularity community rule of csrc/community.hip / fitgnn_amd/community.py ("Community
detection"): numpy for the graph plumbing, plain loops and Python ints for the rule itself, read literally.  It imports nothing of
the product, so the GPU path can be compared with it bit for bit.

A level graph is (rowptr, col, w): a CSR with ascending columns and integer weights >= 1; from level 1 on a diagonal entry holds
the weight inside the community.  k_i is the row sum (diagonal included), M2 the sum of all k_i.
"""
import numpy as np


def level0_graph(edge_index, num_nodes):
    """Symmetrised, de-duplicated edge list without self-loops as a CSR with ascending columns, every weight 1."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    n = int(num_nodes)
    src = np.concatenate([ei[0], ei[1]])
    dst = np.concatenate([ei[1], ei[0]])
    keep = src != dst
    key = np.unique(src[keep] * n + dst[keep])
    row, col = key // n, key % n
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=rowptr[1:])
    return rowptr, col.astype(np.int64), np.ones(len(col), dtype=np.int64)


def degrees(rowptr, w):
    return [int(sum(int(x) for x in w[rowptr[i]:rowptr[i + 1]])) for i in range(len(rowptr) - 1)]


def community_totals(k, comm):
    n = len(k)
    tot, size = [0] * n, [0] * n
    for i in range(n):
        tot[comm[i]] += k[i]
        size[comm[i]] += 1
    return tot, size


def sweep(rowptr, col, w, comm, t, scores=None):
    """One sweep t from the snapshot comm: the new community of every node.  scores (a list) receives (i, c, s(c)) for every
    score evaluated, as Python ints."""
    n = len(rowptr) - 1
    comm = [int(c) for c in comm]
    k = degrees(rowptr, w)
    m2 = sum(k)
    tot, size = community_totals(k, comm)
    out = list(comm)
    for i in range(n):
        if (i + t) % 2:
            continue
        a = comm[i]
        acc = {}
        for p in range(int(rowptr[i]), int(rowptr[i + 1])):
            j = int(col[p])
            if j != i:
                acc[comm[j]] = acc.get(comm[j], 0) + int(w[p])
        if not acc:                                    # no off-diagonal entry: never moves
            continue
        s_a = m2 * acc.get(a, 0) - k[i] * (tot[a] - k[i])
        if scores is not None:
            scores.append((i, a, s_a))
        best, best_s = None, None
        for c in sorted(acc):                          # ascending ids: a tie keeps the smaller one
            if c == a or (size[a] == 1 and size[c] == 1 and c > a):
                continue
            s = m2 * acc[c] - k[i] * tot[c]
            if scores is not None:
                scores.append((i, c, s))
            if best is None or s > best_s:
                best, best_s = c, s
        if best is not None and best_s > s_a:
            out[i] = best
    return out


def stats(rowptr, col, w, comm, snapshot):
    """tot[], size[], moved, sum of in[c], sum of tot[c]^2 of the labelling comm (moved: against snapshot)."""
    n = len(rowptr) - 1
    comm = [int(c) for c in comm]
    k = degrees(rowptr, w)
    tot, size = community_totals(k, comm)
    moved = sum(1 for i in range(n) if comm[i] != int(snapshot[i]))
    sum_in = 0
    for i in range(n):
        for p in range(int(rowptr[i]), int(rowptr[i + 1])):
            if comm[int(col[p])] == comm[i]:
                sum_in += int(w[p])
    return tot, size, moved, sum_in, sum(x * x for x in tot)


def qnum(rowptr, col, w, comm):
    _, _, _, sum_in, sum_tot2 = stats(rowptr, col, w, comm, comm)
    return sum(degrees(rowptr, w)) * sum_in - sum_tot2


def run_level(rowptr, col, w, max_sweeps=64):
    """The sweeps of one level: (comm, sweeps run, last accepted Qnum)."""
    n = len(rowptr) - 1
    m2 = sum(degrees(rowptr, w))
    comm = list(range(n))
    accepted = qnum(rowptr, col, w, comm)
    sweeps, rejected = 0, 0
    while sweeps < max_sweeps and rejected < 2:
        new = sweep(rowptr, col, w, comm, sweeps)
        _, _, moved, sum_in, sum_tot2 = stats(rowptr, col, w, new, comm)
        q = m2 * sum_in - sum_tot2
        sweeps += 1
        if moved > 0 and q > accepted:
            comm, accepted, rejected = new, q, 0
        else:
            rejected += 1
    return comm, sweeps, accepted


def number_by_smallest_member(comm):
    """Labels 0 .. n_c-1 in the order of every community's smallest member."""
    new_id, out = {}, []
    for c in comm:
        c = int(c)
        if c not in new_id:
            new_id[c] = len(new_id)
        out.append(new_id[c])
    return out, len(new_id)


def aggregate(rowptr, col, w, labels, n_c):
    """P A P^T with the sums inside a community kept on the diagonal."""
    n = len(rowptr) - 1
    rows = [dict() for _ in range(n_c)]
    for i in range(n):
        r = rows[labels[i]]
        for p in range(int(rowptr[i]), int(rowptr[i + 1])):
            c = labels[int(col[p])]
            r[c] = r.get(c, 0) + int(w[p])
    rp, cc, ww = [0], [], []
    for r in rows:
        for c in sorted(r):
            cc.append(c)
            ww.append(r[c])
        rp.append(len(cc))
    return np.array(rp, dtype=np.int64), np.array(cc, dtype=np.int64), np.array(ww, dtype=np.int64)


def split_components(rowptr, col, labels):
    """Every community split into the connected components of its induced subgraph; numbered by smallest member."""
    n = len(rowptr) - 1
    piece = [-1] * n
    for s in range(n):
        if piece[s] >= 0:
            continue
        piece[s] = s
        stack = [s]
        while stack:
            i = stack.pop()
            for p in range(int(rowptr[i]), int(rowptr[i + 1])):
                j = int(col[p])
                if piece[j] < 0 and labels[j] == labels[i]:
                    piece[j] = s
                    stack.append(j)
    return number_by_smallest_member(piece)[0]


def modularity_communities(edge_index, num_nodes, max_levels=20, max_sweeps=64, split_disconnected=True, return_info=False):
    rowptr0, col0, w0 = level0_graph(edge_index, num_nodes)
    n = int(num_nodes)
    m2 = int(len(col0))
    if m2 >= 2 ** 31 or n >= 2 ** 31:
        raise ValueError("M2 and N must stay below 2^31")
    rowptr, col, w = rowptr0, col0, w0
    composed = list(range(n))
    levels = []
    for _ in range(max_levels):
        n_l = len(rowptr) - 1
        comm, sweeps, accepted = run_level(rowptr, col, w, max_sweeps)
        labels, n_c = number_by_smallest_member(comm)
        composed = [labels[c] for c in composed]
        levels.append(dict(labels=np.array(composed, dtype=np.int64), sweeps=sweeps, qnum=accepted, n=n_l, n_communities=n_c))
        if n_c == n_l:
            break
        rowptr, col, w = aggregate(rowptr, col, w, labels, n_c)
    final = split_components(rowptr0, col0, composed) if split_disconnected else composed
    final = np.array(final, dtype=np.int64)
    return (final, dict(m2=m2, levels=levels)) if return_info else final


def modularity(edge_index, num_nodes, labels):
    """Exact Qnum / M2^2 of a labelling of the level-0 graph."""
    rowptr, col, w = level0_graph(edge_index, num_nodes)
    m2 = int(len(col))
    if m2 == 0:
        return 0.0
    lab = number_by_smallest_member(np.asarray(labels).tolist())[0]
    return qnum(rowptr, col, w, lab) / (m2 * m2)
