"""Plain float64 NumPy statements of the SpMM kernels of csrc/spmm.hip (test infrastructure only): the product Y = A X[xrow] with zero
operand rows, its forward and backward store epilogues (tests/step_reference.py states those; they are reused, not restated), the
column sums of dZ per tile / block / range, the error bounds of the kernels' summation order, and builders for every descriptor the
entry points take, so that a test chooses its tiling and is not limited to what the host planners emit.

A pattern is (rowptr, col, val): row r holds the entries rowptr[r] ... rowptr[r + 1] - 1, columns ascending and distinct within a
row; a row may be empty.  val is what the kernel receives (float32), taken to float64 exactly.

Bounds (u = 2^-24, first order, no allowance on top):
* a row of len entries is ONE fmaf chain in CSR order in every kernel (padded entries add exact zeros; the gather kernel's fast path
  takes the first four entries first, a chain of the same length):      |Y - ref| <= len u S,   S = |A| |X|   (`row_bound`)
* backward epilogue at p = 0.5 (the scale 2 and e = prev / 2 are exact): two roundings, e + 1 and the product:
  |dZ - ref| <= |factor| row_bound + 2 u |dZ|                            (`dz_bound`)
* col_part: a lane adds its wave's rows in order, then the four waves are added:  sum of the dZ bounds + (rows_of_the_wave + 3) u
  sum |dZ|; one wave owns a whole range of the stream / rows-compact forms (rows - 1 additions, no cross-wave sum)  (`colsum_bound`)

EXACT inputs: X and prev integers in [-8, 8] over 8, val = +- 2^-ceil(log2 max(len, 1)) (sum |val| <= 1 per row), bias integers
over 8, p = 0.5.  Every partial sum of a row is a multiple of 2^-(3 + ceil(log2 len)) of magnitude <= 1: an fp32 number while len <=
2^20, in ANY order.  dZ = 2 Y (e + 1) adds 3 fraction bits (e + 1 has 4, the scale takes one back) at magnitude <= 3.  A column sum is
exact in any order while (sum |dZ|) 2^q < 2^24, q the largest fraction-bit count among its terms (`colsum_is_exact`, evaluated per
column by the tests: the columns it does not certify are held to the bound).  tests/test_spmm_reference_cpu.py evaluates the row lengths
of the GPU module in fp32 in three orders and requires the float64 result bit for bit.
"""
import numpy as np

import appnp_reference as ar
import step_reference as sr

U = 2.0 ** -24
NO_ROW = 0x7FFFFFFF
TILE_INTS = BLOCK_INTS = 8

# row lengths of the GPU module's cases: the tile kernel's group-of-four tails, its eight-at-a-time path (>= 16 entries in a 64-entry
# chunk) with tails of 0 and 7, a second chunk that is itself short (65, 80: 1, 16 entries) or long (300)
TILE_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 23, 24, 63, 64, 65, 80, 300]


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------------
def exact_values(rng, lengths):
    """+- 2^-ceil(log2 max(len, 1)) per entry."""
    lengths = np.asarray(lengths, dtype=np.int64)
    ln = np.maximum(np.repeat(lengths, lengths), 1)
    return (rng.choice([-1.0, 1.0], size=len(ln)) * 2.0 ** -np.ceil(np.log2(ln))).astype(np.float32)


def random_values(rng, nnz):
    """Uniform in +-[0.05, 1]."""
    return (rng.choice([-1.0, 1.0], size=nnz) * rng.uniform(0.05, 1.0, size=nnz)).astype(np.float32)


def make_csr(row_lengths, n_cols, rng, exact=False, lo=None, hi=None, cols=None):
    """(rowptr int32, col int32, val float32) with the given row lengths (0 allowed).  Row r draws len distinct columns from
    [lo[r], hi[r]) (default [0, n_cols)), ascending; cols {row: columns} places a row's columns by hand (sorted here).
    exact: val = +- 2^-ceil(log2 max(len, 1)); else uniform in +-[0.05, 1]."""
    lengths = np.asarray(row_lengths, dtype=np.int64).copy()
    n = len(lengths)
    lo = np.zeros(n, dtype=np.int64) if lo is None else np.broadcast_to(np.asarray(lo, dtype=np.int64), (n,))
    hi = np.full(n, n_cols, dtype=np.int64) if hi is None else np.broadcast_to(np.asarray(hi, dtype=np.int64), (n,))
    cols = {} if cols is None else cols
    out = []
    for r in range(n):
        if r in cols:
            c = np.unique(np.asarray(cols[r], dtype=np.int64))
            lengths[r] = len(c)
        else:
            assert lengths[r] <= hi[r] - lo[r], f"row {r}: {lengths[r]} distinct columns do not fit [{lo[r]}, {hi[r]})"
            c = np.sort(lo[r] + rng.permutation(hi[r] - lo[r])[:lengths[r]])
        assert len(c) == 0 or (c[0] >= 0 and c[-1] < n_cols)
        out.append(c)
    col = np.concatenate(out) if out else np.zeros(0, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lengths)])
    val = exact_values(rng, lengths) if exact else random_values(rng, len(col))
    return rowptr.astype(np.int32), col.astype(np.int32), val


def exact_signal(rng, shape):
    """Integers in [-8, 8] over 8."""
    return (rng.integers(-8, 9, size=shape) / 8.0).astype(np.float32)


def cycle(values, n, start=0):
    return np.array([values[(start + i) % len(values)] for i in range(n)], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the product and its epilogues
# ---------------------------------------------------------------------------------------------------------------------------------
def operand(X, n_cols, xrow=None, zero_from=-1):
    """[n_cols, H] float64: the operand row of every pattern column -- X[xrow[c]] (xrow None: X[c]), zeros where that row index is >=
    zero_from (zero_from < 0: nowhere; such rows need not exist in X)."""
    X = _f64(X)
    idx = np.arange(n_cols, dtype=np.int64) if xrow is None else np.asarray(xrow, dtype=np.int64)[:n_cols]
    zero = (idx >= zero_from) if zero_from >= 0 else np.zeros(len(idx), dtype=bool)
    out = np.zeros((len(idx), X.shape[1]))
    out[~zero] = X[idx[~zero]]
    return out


def spmm(rowptr, col, val, X, xrow=None, zero_from=-1, n_cols=None):
    """(Y, S): Y = A @ X[xrow] in float64 with operand rows >= zero_from read as zero, and S = |A| @ |X[xrow]|, the magnitude every
    entry's error bound scales with.  For the compact-operand entry points pass xcol as col (it names operand rows) and zero_from."""
    col = np.asarray(col, dtype=np.int64)
    if n_cols is None:
        n_cols = len(xrow) if xrow is not None else max(int(col.max()) + 1 if len(col) else 0, 0 if zero_from >= 0 else np.shape(X)[0])
    Xe = operand(X, n_cols, xrow, zero_from)
    return ar.spmv(rowptr, col, _f64(val), Xe), ar.spmv(rowptr, col, np.abs(_f64(val)), np.abs(Xe))


def row_bound(rowptr, S):
    """len u S per entry."""
    return np.diff(np.asarray(rowptr, dtype=np.int64))[:, None] * U * _f64(S)


def forward(Y, bias, epi, p=0.0, keep=None):
    """dropout(ELU(Y + bias)) (step_reference.epilogue_fwd); the dropout hash index is row * H + col, H the logical width."""
    return sr.epilogue_fwd(Y, bias, epi, p, keep)


def keep_by_hash(seed, rows, H, p=0.5):
    return sr.keep_matrix(seed, rows, H, p)


def backward(Y, prev, epi, p=0.0, keep=None):
    """(dZ, factor): dZ = Y * d out / d z of the forward's epilogue, from the forward's output prev (step_reference)."""
    f = sr.epilogue_bwd_factor(prev, epi, p, keep)
    return _f64(Y) * f, f


def dz_bound(factor, eY, dZ):
    """|factor| eY + 2 u |dZ|: the product's error through the factor, then the roundings of e + 1 and of the product (p = 0.5)."""
    return np.abs(factor) * eY + 2 * U * np.abs(dZ)


def colsums(dZ, ranges):
    """(sums, abs sums) [n_ranges, H] of dZ's rows per [r0, r1) of `ranges` (an empty range: zeros)."""
    dZ = _f64(dZ)
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    s = np.zeros((len(r), dZ.shape[1]))
    a = np.zeros_like(s)
    for i, (r0, r1) in enumerate(r):
        s[i], a[i] = dZ[r0:r1].sum(0), np.abs(dZ[r0:r1]).sum(0)
    return s, a


def colsum_bound(dz_bounds, abs_sums, ranges, rows_of_wave):
    """Sum of the dZ bounds of each range + (rows_of_wave + 3) u sum |dZ|; rows_of_wave: per range, the largest number of rows one
    wave adds (the cross-wave sum is the + 3; a single-wave kernel passes its rows - 4)."""
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    b = np.stack([_f64(dz_bounds)[r0:r1].sum(0) for r0, r1 in r]) if len(r) else np.zeros((0, np.shape(dz_bounds)[1]))
    return b + (np.asarray(rows_of_wave, dtype=np.float64).reshape(-1, 1) + 3) * U * abs_sums


def colsum_is_exact(abs_sums, max_len):
    """Per column: every partial sum of the range's dZ, in any order, is an fp32 number -- (sum |dZ|) 2^q < 2^24 with q = 3 +
    ceil(log2 max_len) + 3 the fraction bits of an EXACT dZ (module docstring)."""
    q = 6 + int(np.ceil(np.log2(max(int(max_len), 1))))
    return _f64(abs_sums) * 2.0 ** q < 2.0 ** 24


def chain_f32(rowptr, col, val, Xe, order="csr"):
    """The rows' sums with every product-and-add rounded once to fp32 (an fmaf chain: the product enters the addition unrounded), the
    entries taken in `order`: 'csr', 'reverse' or 'first4' (entries 4 ... first, then 0 ... 3 -- no kernel's order, a third one)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    lens = np.diff(rowptr)
    n = len(lens)
    col = np.asarray(col, dtype=np.int64)
    v64, X64 = _f64(np.asarray(val, dtype=np.float32)), _f64(np.asarray(Xe, dtype=np.float32))
    acc = np.zeros((n, X64.shape[1]), dtype=np.float32)
    for j in range(int(lens.max()) if n else 0):
        rows = np.nonzero(lens > j)[0]
        if order == "reverse":
            k = lens[rows] - 1 - j
        elif order == "first4":
            k = np.where(lens[rows] > 4, (j + 4) % lens[rows], j)
        else:
            k = np.full(len(rows), j)
        e = rowptr[rows] + k
        acc[rows] = (v64[e][:, None] * X64[col[e]] + acc[rows].astype(np.float64)).astype(np.float32)   # one rounding: fmaf
    return acc


# ---------------------------------------------------------------------------------------------------------------------------------
# descriptors
# ---------------------------------------------------------------------------------------------------------------------------------
def tile_records(rowptr, specs):
    """fitgnn_tile_t records [T, 8] int32 from specs (row_begin, row_end, win_begin, win_rows[, listed]); a spec None is an empty
    record (row_begin == row_end, no window), legal padding anywhere in the array."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    out = np.zeros((len(specs), TILE_INTS), dtype=np.int32)
    for i, s in enumerate(specs):
        if s is None:
            continue
        r0, r1, w0, wn = s[:4]
        out[i] = [r0, r1, w0, wn, rowptr[r0], rowptr[r1], s[4] if len(s) > 4 else 0, 0]
    return out


def pack_tiles(ptr, max_rows):
    """(row_begin, row_end, win_begin, win_rows) of fitgnn_make_tiles_host: consecutive blocks packed while they fit max_rows rows, a
    larger block cut into max_rows-row pieces; the window is the tile's own rows."""
    ptr = [int(v) for v in ptr]
    out, b, nb = [], 0, len(ptr) - 1
    while b < nb:
        start, size = ptr[b], ptr[b + 1] - ptr[b]
        if size > max_rows:
            out += [(s, min(s + max_rows, start + size), s, min(s + max_rows, start + size) - s) for s in range(start, start + size, max_rows)]
            b += 1
            continue
        e = b + 1
        while e < nb and ptr[e + 1] - start <= max_rows:
            e += 1
        out.append((start, ptr[e], start, ptr[e] - start))
        b = e
    return out


def block_records(rowptr, ranges, long_row=None, long_rows=None):
    """(fitgnn_block_t records [B, 8] int32, long_rows int32): one record per [r0, r1) of `ranges` in the order given (None: an empty
    record).  A block's long rows are its rows of more than long_row entries, ascending (fitgnn_split_blocks_host), or, with
    long_rows {range index: rows}, the rows listed by hand."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    lens = np.diff(rowptr)
    out = np.zeros((len(ranges), BLOCK_INTS), dtype=np.int32)
    longs = []
    for i, rg in enumerate(ranges):
        if rg is None:
            continue
        r0, r1 = int(rg[0]), int(rg[1])
        if long_rows is not None and i in long_rows:
            mine = sorted(int(v) for v in long_rows[i])
        elif long_row is not None:
            mine = [r for r in range(r0, r1) if lens[r] > long_row]
        else:
            mine = []
        assert all(r0 <= r < r1 for r in mine)
        out[i] = [r0, r1, rowptr[r0], rowptr[r1], len(longs), len(mine), 0, 0]
        longs += mine
    return out, np.asarray(longs, dtype=np.int32)


def split_blocks(ptr, rowptr, cap, limit, long_row):
    """(tiles4, blocks, long_rows) of fitgnn_split_blocks_host: blocks of cap < rows <= limit become records (input order), the
    maximal runs of the others are packed into tiles."""
    ptr = [int(v) for v in ptr]
    large = [cap < ptr[b + 1] - ptr[b] <= limit for b in range(len(ptr) - 1)]
    tiles, ranges, b = [], [], 0
    while b < len(large):
        if large[b]:
            ranges.append((ptr[b], ptr[b + 1]))
            b += 1
            continue
        e = b
        while e < len(large) and not large[e]:
            e += 1
        tiles += pack_tiles(ptr[b:e + 1], cap)
        b = e
    blocks, longs = block_records(rowptr, ranges, long_row)
    return tiles, blocks, longs


def segments(seg_sizes, segs_per_range):
    """(seg_ptr int32 [n_seg + 1], range_seg int32 [n_ranges + 1]): segments of the given row counts (each >= 1: its first row is its
    hub), cut into ranges of the given numbers of whole segments (0: an empty range)."""
    seg_ptr = np.concatenate([[0], np.cumsum(seg_sizes)]).astype(np.int32)
    range_seg = np.concatenate([[0], np.cumsum(segs_per_range)]).astype(np.int32)
    assert range_seg[-1] == len(seg_sizes) and all(s >= 1 for s in seg_sizes)
    return seg_ptr, range_seg


def plan_windows(rowptr, col, specs):
    """A hand-made plan for fitgnn_spmm_csr_f32's lcol / win_cols form.  specs: (row_begin, row_end, window) per tile with window
    either (win_begin, win_rows) -- contiguous -- or a list of operand rows -- listed (reserved[0] = 1, win_begin = its offset in
    win_cols); None: an empty record.  Returns (tiles [T, 8], win_cols, lcol): lcol[e] is the LDS slot of entry e's operand row in its
    tile's window, or -(col + 1) when the window does not hold it.  Entries of rows no tile covers keep -(col + 1)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    lcol = -(col + 1)
    win_cols, recs = [], []
    for s in specs:
        if s is None:
            recs.append(None)
            continue
        r0, r1, w = s
        e0, e1 = rowptr[r0], rowptr[r1]
        c = col[e0:e1]
        if isinstance(w, tuple):
            w0, wn = w
            slot = np.where((c >= w0) & (c < w0 + wn), c - w0, -1)
            recs.append((r0, r1, w0, wn, 0))
        else:
            w = [int(v) for v in w]
            where = {v: i for i, v in reversed(list(enumerate(w)))}
            slot = np.array([where.get(int(v), -1) for v in c], dtype=np.int64)
            recs.append((r0, r1, len(win_cols), len(w), 1))
            win_cols += w
        lcol[e0:e1] = np.where(slot >= 0, slot, -(c + 1))
    return tile_records(rowptr, recs), np.asarray(win_cols if win_cols else [0], dtype=np.int32), lcol.astype(np.int32)


def resolve_lcol(tiles, win_cols, lcol, rowptr):
    """The operand row every planned entry resolves to: win_cols[win_begin + slot] (listed) or win_begin + slot (contiguous) for a
    slot >= 0, -(lcol + 1) otherwise; -1 for entries of rows no tile covers."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    out = np.full(len(lcol), -1, dtype=np.int64)
    for t in np.asarray(tiles).reshape(-1, TILE_INTS):
        for e in range(rowptr[t[0]], rowptr[t[1]]):
            s = int(lcol[e])
            out[e] = -(s + 1) if s < 0 else (int(win_cols[t[2] + s]) if t[6] else int(t[2]) + s)
            assert s < 0 or s < t[3], "a slot beyond the tile's window"
    return out
