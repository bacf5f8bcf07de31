"""Plain float64 NumPy statements of the small per-step kernels of csrc/gcn_ops.hip (test infrastructure only): the loss kernels,
the flat Adam update, the output head on the loss rows, the narrow column sum, the dense pass over a few input columns and its
backward, the backward of the bias / ELU / dropout epilogue, and a replica of the counter-based dropout hash of csrc/common.h.

Each helper returns the float64 result of the kernel's operation, plus, where a tolerance needs it, the per-entry condition
sum |terms|.  tests/test_step_reference_cpu.py checks them against torch's own float64 operations and autograd.
"""
import numpy as np

EPI_BIAS, EPI_ELU, EPI_DROPOUT, EPI_SEED_DEVICE = 1, 2, 4, 8
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------------
# the dropout hash (common.h: fmix32, dropout_bits, dropout_threshold, dropout_keep, resolve_seed)
# ---------------------------------------------------------------------------------------------------------------------------------
def fmix32(h):
    """murmur3's 32-bit finaliser on uint64 arrays holding uint32 values."""
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    return h ^ (h >> np.uint64(16))


def dropout_bits(seed, group):
    """The 64 hash bits of a group of four consecutive elements (group = flat index >> 2) under a 64-bit seed."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    group = np.asarray(group, dtype=np.uint64)
    g = ((group & M32) * np.uint64(0x9E3779B1) + (group >> np.uint64(32)) * np.uint64(0x85EBCA77)) & M32
    lo = fmix32(g ^ np.uint64(seed & M32))
    hi = fmix32(((g + np.uint64(0x7F4A7C15)) & M32) ^ np.uint64(seed >> 32) ^ np.uint64(0x68E31DA4))
    return (hi << np.uint64(32)) | lo


def dropout_threshold(p):
    """(uint32)(p * 65536.0f): p is the fp32 value the kernel receives."""
    return int(np.float32(p) * np.float32(65536.0))


def resolve_seed(seed_arg, epi, read_word):
    """The seed a kernel uses: with FITGNN_EPI_SEED_DEVICE and FITGNN_EPI_DROPOUT both set, seed_arg is the address of a device word
    holding it (read_word(address) returns that word), else the seed itself."""
    return int(read_word(seed_arg)) if (epi & EPI_SEED_DEVICE) and (epi & EPI_DROPOUT) else int(seed_arg)


def dropout_keep(seed, row, col, H, p):
    """Keep decision of element (row, col) of a [rows x H] matrix: group (row * H + col) >> 2, sub-index (row * H + col) & 3, kept
    iff that sub-index's 16 bits are >= floor(p * 65536)."""
    idx = np.asarray(row, dtype=np.uint64) * np.uint64(H) + np.asarray(col, dtype=np.uint64)
    bits = dropout_bits(seed, idx >> np.uint64(2))
    sub = (idx & np.uint64(3)) * np.uint64(16)
    return ((bits >> sub) & np.uint64(0xFFFF)) >= np.uint64(dropout_threshold(p))


def keep_matrix(seed, rows, H, p):
    """[len(rows) x H] keep decisions of the ORIGINAL rows `rows` (a compact matrix's row i is original row rows[i])."""
    rows = np.asarray(rows, dtype=np.int64)
    return dropout_keep(seed, rows[:, None], np.arange(H)[None, :], H, p)


# ---------------------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------------------
def softmax_nll(z, idx, labels, scale):
    """loss = scale * sum_t (lse(z[idx[t]]) - z[idx[t], labels[t]]) and dz = (softmax - onehot) * scale on the selected rows, zero
    elsewhere.  The rows of idx must be distinct (the kernel writes, not adds, each selected row's gradient).  Also returns the
    lse of every selected row (for the tolerances)."""
    z = np.asarray(z, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    assert np.unique(idx).size == idx.size, "softmax_nll: idx must not repeat a row"
    zs = z[idx]
    m = zs.max(1, keepdims=True) if zs.size else np.zeros((0, 1))
    lse = (m + np.log(np.exp(zs - m).sum(1, keepdims=True)))[:, 0] if zs.size else np.zeros(0)
    t = np.arange(idx.size)
    loss = float(((lse - zs[t, labels]) * scale).sum())
    dz = np.zeros_like(z)
    sm = np.exp(zs - lse[:, None])
    sm[t, labels] -= 1.0
    dz[idx] = sm * scale
    return loss, dz, lse


def l1_loss(out, tgt, scale):
    """loss = scale * sum |out - tgt| and its gradient scale * sign(out - tgt), 0 where out == tgt (torch's sign(0))."""
    d = np.asarray(out, dtype=np.float64) - np.asarray(tgt, dtype=np.float64)
    return float(scale * np.abs(d).sum()), scale * np.sign(d)


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------------
def adam(p, g_acc, g_new, m, v, t, lr, b1, b2, eps, wd):
    """One torch.optim.Adam step (amsgrad=False, maximize=False) in float64 from a state whose step count is t (the step taken is
    t + 1): g = g_acc (+ g_new), g += wd * p, m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
    p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps) with bc = 1 - beta^(t + 1).  The betas are used as given: pass the fp32-rounded
    values a kernel receives to state what it should compute.  Returns (p, g, m, v) -- g is the gradient accumulated from g_acc and
    g_new, before the weight decay."""
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    p, g, m, v = f(p), f(g_acc), f(m), f(v)
    if g_new is not None:
        g = g + f(g_new)
    b1, b2, lr, eps, wd = float(b1), float(b2), float(lr), float(eps), float(wd)
    step = float(t) + 1.0
    gk = g + wd * p
    m = b1 * m + (1.0 - b1) * gk
    v = b2 * v + (1.0 - b2) * gk * gk
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return p, g, m, v


# ---------------------------------------------------------------------------------------------------------------------------------
# the bias / ELU / dropout epilogue
# ---------------------------------------------------------------------------------------------------------------------------------
def keep_of(epi, keep, shape):
    return np.ones(shape, dtype=bool) if not (epi & EPI_DROPOUT) else np.broadcast_to(np.asarray(keep, dtype=bool), shape)


def epilogue_fwd(z, bias, epi, p=0.0, keep=None):
    """dropout(ELU(z + bias)) as the SpMM kernels' store epilogue: ELU with expm1, kept entries scaled by 1 / (1 - p)."""
    y = np.asarray(z, dtype=np.float64)
    if epi & EPI_BIAS:
        y = y + np.asarray(bias, dtype=np.float64)[None, :]
    if epi & EPI_ELU:
        y = np.where(y > 0, y, np.expm1(np.minimum(y, 0.0)))
    if epi & EPI_DROPOUT:
        y = np.where(keep_of(epi, keep, y.shape), y * (1.0 / (1.0 - float(np.float32(p)))), 0.0)
    return y


def epilogue_bwd_factor(out, epi, p=0.0, keep=None):
    """d out / d z of the epilogue, from the forward's output `out`: dropout' (kept: 1 / (1 - p), else 0) times ELU' (1 above
    zero, exp(z) = e + 1 below, e the pre-dropout ELU output = out * (1 - p))."""
    out = np.asarray(out, dtype=np.float64)
    f = np.ones_like(out)
    pf = float(np.float32(p))
    if epi & EPI_DROPOUT:
        f = np.where(keep_of(epi, keep, out.shape), 1.0 / (1.0 - pf), 0.0)
    if epi & EPI_ELU:
        e = out * ((1.0 - pf) if epi & EPI_DROPOUT else 1.0)
        f = f * np.where(e > 0, 1.0, e + 1.0)
    return f


def epilogue_bwd(dOut, out, epi, p=0.0, keep=None):
    """(dZ, db, cond): dZ = dOut * d out / d z, db = column sums of dZ, cond = column sums of |dZ|."""
    dZ = np.asarray(dOut, dtype=np.float64) * epilogue_bwd_factor(out, epi, p, keep)
    return dZ, dZ.sum(0), np.abs(dZ).sum(0)


def epilogue_bwd_head(dy, Wl, out, epi, p=0.0, keep=None):
    """The backward through the output head y = out Wl^T and the epilogue: dOut = dy Wl, dZ as epilogue_bwd, db = column sums of
    dZ, dWl = dy^T out.  Returns (dZ, db, dWl, dOut_cond, dWl_cond) with the conditions sum |terms| of dOut and dWl."""
    dy, Wl, out = (np.asarray(a, dtype=np.float64) for a in (dy, Wl, out))
    dOut = dy @ Wl
    dZ, db, db_cond = epilogue_bwd(dOut, out, epi, p, keep)
    return dZ, db, dy.T @ out, np.abs(dy) @ np.abs(Wl), np.abs(dy).T @ np.abs(out)


def select_rows(sel, compact_in, *arrays):
    """The rows an epilogue-backward launch over selected rows reads: row i is original row sel[i], or row i of an already compact
    input (compact_in)."""
    return tuple(np.asarray(a)[:len(sel)] if compact_in else np.asarray(a)[np.asarray(sel, dtype=np.int64)] for a in arrays)


# ---------------------------------------------------------------------------------------------------------------------------------
# the output head, the narrow column sum, the dense pass over a few input columns and its backward
# ---------------------------------------------------------------------------------------------------------------------------------
def head_rows(out_rows, Wl, bl):
    """y = out_rows Wl^T + bl for the selected rows (out_rows [n x H]), and the condition sum_h |out Wl| + |bl|."""
    o, W = np.asarray(out_rows, dtype=np.float64), np.asarray(Wl, dtype=np.float64)
    b = np.zeros(W.shape[0]) if bl is None else np.asarray(bl, dtype=np.float64)
    return o @ W.T + b, np.abs(o) @ np.abs(W).T + np.abs(b)


def colsum(x):
    """Column sums of x and their condition sum |x|."""
    x = np.asarray(x, dtype=np.float64)
    return x.sum(0), np.abs(x).sum(0)


def dense_narrow_k(a, W, bias, epi, p=0.0, keep=None):
    """out = dropout(ELU(a W^T + bias)) with a [n x K], W [H x K]; also returns the pre-epilogue product and its condition."""
    a, W = np.asarray(a, dtype=np.float64), np.asarray(W, dtype=np.float64)
    z = a @ W.T
    return epilogue_fwd(z, bias, epi, p, keep), z, np.abs(a) @ np.abs(W).T


def narrow_atb(d, a, prev=None, epi=0, p=0.0, keep=None):
    """dW = dZ^T a ([H x K]) and db = column sums of dZ, where dZ = d, or with `prev` (the layer's forward output) d times the
    epilogue's derivative under the forward's flags.  Returns (dW, db, dW_cond, db_cond)."""
    d, a = np.asarray(d, dtype=np.float64), np.asarray(a, dtype=np.float64)
    dZ = d if prev is None else d * epilogue_bwd_factor(prev, epi, p, keep)
    return dZ.T @ a, dZ.sum(0), np.abs(dZ).T @ np.abs(a), np.abs(dZ).sum(0)
