"""GPU tier: every SpMM kernel of csrc/spmm.hip through the C ABI against the float64 references of tests/spmm_reference.py, with the helpers
of tests/test_gpu_step_kernels.py.  Patterns, tilings, block records, segments and plans are made by hand (spmm_reference's builders):
rows of 0 entries, windows of any size, listed windows, ld > H, unaligned operands, empty records, more long rows than are carried --
what the ABI promises and csr.CSRGraph(mode="gcn") never produces.  Two kinds of input:
EXACT (X, prev integers in [-8, 8] over 8, val = +- 2^-ceil(log2 max(len, 1)), bias integers over 8, p = 0.5: every fp32 partial result
is exact -- tests/test_spmm_reference_cpu.py) must come back bit for bit, in any summation order; with ELU in a forward epilogue only the
entries with z > 0 are exact, the others are held to the bound; a column sum is compared bit for bit where spmm_reference.colsum_is_exact
certifies it (all of them in these shapes but some sums over the 300-leaf star of the two-hop tests).
RANDOM (normal X, val uniform in +-[0.05, 1]) is held per entry to a bound of first order in u = 2^-24, never to a fraction of the
output's largest value.  Every output (Y, ZT, col_part where the header says every element is written) is NaN before the launch and
followed by guard elements; rows no record covers and the columns H .. ld must still be NaN; operands are strided views with NaN
padding, the zero rows of a compact operand or table are NaN in memory (a kernel that loads one poisons its result).

Launcher -> branch -> tests that reach it (H: 4 one slab, 36 dead lanes in a slab, 256 exactly one slab, 260 a second slab with one
live lane, 512 two slabs; VEC = 1: H = 1, 7, 33 and H = 64 with X and Y one float into their buffers):

| launcher | branch (from the launch code and the kernel) | tests |
|---|---|---|
| fitgnn_spmm_csr_f32, launch<4> / launch<1> | spmm_tile_kernel<VEC, 4, 16, PLAIN, NOEPI>: no flag, window <= 16 (w16, w5, w2), no lcol / win_cols / xrow | test_tile_product[*-w16 / w5 / w2] |
| | <VEC, 4, 16, PLAIN>: an epilogue flag on the same launch | test_tile_forward_epilogues[*-w16-*] |
| | <VEC, 4, 16, !PLAIN>: lcol over contiguous windows (w16-planned), listed windows (reserved[0] = 1) with lcol slots, -(col + 1) misses and slots beyond the clamped window (w16-listed), xrow alone (w16-xrow), zero rows inside and outside the windows (w16-xrow-zero), xrow with listed windows (w16-listed-xrow-zero) | test_tile_product[*-w16-planned / -listed / -xrow / -xrow-zero / -listed-xrow-zero], test_tile_forward_epilogues[*-w16-listed-xrow-zero-*] |
| | <VEC, 8, 32, !PLAIN>: windows 17 (w17), 40 with a plan and a table (w40-listed-xrow-zero), 96 (w96), window_rows = 200 clamped to 96 (w200) | test_tile_product[*-w17 / w40-* / w96 / w200], test_tile_forward_epilogues[*-w40-*] |
| | hipFuncSetAttribute: a 96-row window at VEC = 4 is 98 KiB of LDS (+ 24 KiB of CSR slice); at VEC = 1 it stays below 64 KiB | test_tile_product[H4 ... H512-w96 / w200] against [H1 ... H64-unaligned-w96] |
| | n_tiles = 1, 8, 9 and all (the first nine records hold three empty ones; blocks beyond n_tiles return); rows of no tile stay NaN | test_tile_product |
| | a tile's win_rows beyond the launched window (clamped, misses from memory); a tile of 2 w + 3 rows (row pointers beyond rp_rows from memory); a tile with more entries than lds_rows * MPR (entries beyond n_meta from memory, in one chunk with staged ones); tiles of 1, 2, 3 rows | _tile_layout: every tile test |
| | row lengths 0, 1, 2, 3, 4, 5, 15, 16, 17, 23, 24, 63, 64, 65, 80, 300: the group-of-four tail at 1, 2, 3; the kLongRow eight-at-a-time path with tails of 0 and 7 then groups of four; a second 64-entry chunk, short (65, 80) or long (300) | _tile_pattern: every tile test |
| | groups of four that are all hits, all misses, mixed (rows placed inside / half inside / outside their window) | _tile_pattern |
| | forward flags: bias, ELU, both, dropout by mask, by hash with the seed by value and by pointer | test_tile_forward_epilogues |
| | FITGNN_SPMM_GATHER with xrow_zero_from >= 0: the flag is dropped, the tile kernel runs | test_gather_with_zero_rows_runs_the_tile_kernel |
| | refusals: FITGNN_EPI_BACKWARD on the forward entry, win_cols without lcol, window_rows < 0 | test_tile_refusals |
| fitgnn_spmm_csr_f32 + FITGNN_SPMM_GATHER, spmm_gather_kernel<4 / 1> | fast path (<= 63 rows and <= 64 entries per wave): 2, 3, 8 and 63 rows per wave (the qa / qb ping-pong with and without a tail), rows of 0, 1, 4, 5, 9, 10, 64 entries, an empty row first in its wave, one last with lo == 64 | test_gather_product, test_gather_forward_epilogues |
| | general path: 64 rows per wave; 65 ... 71 entries per wave with rows of 3, 4, 5, 61, 64, 65, 67 entries | the same |
| | tiles of 1, 2, 3 rows (waves that return); xrow; VEC 4 / 1; empty records; the forward epilogues | the same |
| fitgnn_spmm_csr_dz_f32 | <4, 16, PLAIN>, <4, 16, !PLAIN>, <4, 8, 32> with FITGNN_EPI_BACKWARD: ELU, dropout, both; mask, hash by value, by pointer; col_part given / NULL; the partial rows of empty records 0 | test_tile_dz |
| | a window of two rows: the LDS is sized for write_col_part's scratch, not the window | test_tile_dz[*-w2-*] |
| | H % 4 != 0, a bias flag, prev unaligned -> FITGNN_E_BADARG; X / Y unaligned -> FITGNN_E_ALIGN | test_tile_refusals |
| fitgnn_spmm_csr_blocks_f32 | spmm_block_kernel<false, false, NOEPI> (plain), <true, false> (xrow, with and without xcol) without a flag | test_blocks_product |
| | <false, false>, <true, false> with the forward epilogue | test_blocks_forward_epilogues |
| | blocks of 1, 15, 16, 17, 33, 200 rows; a block of empty rows at row 0 (nnz_begin == nnz_end == 0: the staging load is guarded) and one in the middle; empty records; n_blocks = 1, 9, all; rows of no block stay NaN | _block_pattern, BLOCK_ORDER: every blocks test |
| | n_long = 0, 1, 4, 6 (two long rows not carried: short rows of 65 entries); long rows of 65 and 300 entries before, inside and after the block (gather_long on both sides, a 64-entry chunk ending inside a piece) | the same |
| | a piece of 180 entries (beyond kBlkMeta: resolved in the row loop, some at a carried row, some at a zero row); short-row entries into another piece (gathered) and at a carried long row (pinned slot) | the same |
| | xrow_zero_from: zero rows as window rows, as gathered entries, as a carried long row (row 90) | test_blocks_product[*-xrow-zero / -xrow-xcol-zero], test_blocks_dz |
| fitgnn_spmm_csr_blocks_dz_f32 | <false, true>, <true, true>; col_part per block, rows of empty records left alone | test_blocks_dz |
| | H = 7, xcol without xrow, FITGNN_EPI_BACKWARD on the forward entry, prev unaligned -> FITGNN_E_BADARG; H = 36 accepted; X unaligned -> FITGNN_E_ALIGN | test_blocks_refusals |
| fitgnn_spmm_csr_stream_f32 | spmm_stream_kernel<false, false, true>, <false, false, false>, <true, false, true>, <true, false, false> | test_stream_forward[*-plain / plain-epi, plain-hash / xrow / xrow-epi, xrow-hash] |
| | segments of 1, 2, 3, 5, 70 rows; ranges of one segment, of 130 (a second seg_ptr batch) and 200 rows (three row-pointer / xrow batches, groups of four across them), an empty range; 5 and 10 waves (n_ranges n_slabs % 4 != 0) | _stream_layout: every stream test |
| | hubs of 3, 64, 65, 130, 200 entries left of, inside and right of their segment; a hub tile reload in hub_gather and in hub_take; leaves of 1, 2, 4, 5, 9 entries (own, the hub's, others); a leaf right after 130 hub entries (k + 3 >= 128: re-base); leaves across the current / next entry tiles | _stream_pattern |
| fitgnn_spmm_csr_stream_dz_f32 | <false, true, false>, <true, true, false>; col_part: one row per range, every element written, the empty range exactly 0 | test_stream_dz |
| | xrow or xcol alone, nnz == 0, H = 7, prev unaligned -> FITGNN_E_BADARG; X unaligned -> FITGNN_E_ALIGN | test_stream_refusals |
| fitgnn_spmm_rows_compact_f32 / _dz_f32 | spmm_rows_compact_kernel<false> / <true>: n_rows = 1, 31, 32, 33, 200 (ranges of 32 rows, a partial last one); ranges of 0, 64, 65, 200 entries (entry tiles, rows across them); empty rows first and last in a range; the same operand row in consecutive rows (cached), again after another row and after a zero row; entries >= zero_from, a row of them only | test_rows_compact |
| | zero_from = 0 | test_rows_compact_every_row_zero |
| | 262 145 rows: 33 per range (a last group of one row); 524 289 rows: 65 per range, the range's second row-pointer batch (i >= 64: 33 rows per range never reach it) | test_rows_compact_many_rows |
| | nnz == 0 with NULL and with one-element xcol / val: no launch, Y's H columns and col_part exactly 0 | test_rows_compact_without_entries |
| | col_part per range against fitgnn_spmm_rows_compact_parts | test_rows_compact, _parts |
| | every refusal of spmm_rows_impl | test_rows_compact_refusals |
| fitgnn_two_hop_rows_f32 | table rows in any order with repeats; rows of 0, 1, 3, 5, 64, 65, 200 entries with no, some, only loss columns; zcol = 0x7fffffff and >= zero_from; ELU / dropout / both, mask / hash; H = 260 (the dead lanes' clamped column); ldz > H; refusals | test_two_hop_rows, test_two_hop_rows_refusals |
| fitgnn_spmm_two_hop_blocks_f32 | spmm_block_kernel<true, false, true, true>: stars of 3, 40, 300 leaves, leaf -- leaf edges inside a piece, across pieces, across blocks, rows of no block (NaN); loss rows: the centres (hub slot), centres and leaves (a row with two loss columns in the table), none in a block; simple rows made in the window; col_part per block; index from ops._two_hop_block_index | test_two_hop_blocks, test_two_hop_blocks_refusals |
| "same bits" (header) | tile (windows 16 and 40), gather general path, blocks, stream, rows-compact on one RANDOM pattern; their dz forms; two-hop == rows-compact-dz + blocks; two launches of every kernel | test_same_bits_across_kernels, test_same_bits_across_dz_kernels, test_two_hop_blocks, test_two_hop_rows, the random cases |

Bounds (u = 2^-24, derived in tests/spmm_reference.py, no allowance on top).  Row: len u S, S = |A| |X|.  Forward epilogue: + u |y| for the
bias, test_gpu_step_kernels._elu_bound below zero, the scale 2 exact.  Backward epilogue: |factor| len u S + 2 u |dZ|.  col_part: the sum
of the dZ bounds + (rows of a wave + 3) u sum |dZ| with ceil(rows / 4) rows per wave (tile), 4 per piece + 1 (blocks), 4 per piece
(two-hop), rows - 4 (stream, rows-compact: one wave, no cross-wave sum).  Two-hop Y: |P| (dZ bound) + len u |P| |dZ|.
Worst observed error / bound over all entries of one MI355X run (a row of one entry is a single rounding and reaches u on its own):
* products: tile 0.998, gather 0.997, blocks 0.999, stream 0.999, rows-compact 0.996; the fp32 fmaf-chain emulation in CSR order of
  tests/test_spmm_reference_cpu.py: 0.97
* forward epilogue: tile 0.99, gather 1.00, blocks 0.99, stream 1.00
* dZ: tile 0.88, blocks 0.84, stream 0.81, rows-compact 0.81, two-hop rows 0.81; two-hop blocks Y 0.51
* col_part: tile 0.33, blocks 0.19, stream 0.19, rows-compact 0.29, two-hop 0.17

Arithmetic-only changes to a scratch copy of spmm.hip (none moves an address), this module and tests/test_gpu_spmm.py run once per
change on one MI355X -- failed tests of the 584 here / of the 223 there:
* (a) spmm_tile_kernel: the padded entries of a last group weighted like its first entry instead of 0:      242 / 121
* (b) epilogue_value, backward: d * (e + 1) without the e > 0 test:                                          141 / 16
* (c) spmm_block_kernel: gather_long's fma skipped when bound == blk.row_begin (a long row's entries left of its block dropped):
                                                                                                             124 / 0  (the 1e-4 check and the bit comparisons there miss it: no planner output has such entries)
* (d) spmm_rows_compact_kernel, `cached = c` in the zero-row branch:                                         0 / 0    -- no result changes: c >= zero_from there, so the next
  selection entry never equals `cached` and reloads its row; the change costs a load, not a bit.  The nearby change that does keep a
  stale row across a zero-row entry -- the zero-row branch clears xc and leaves `cached` as it is:          48 / 9   (16 of test_rows_compact, 20 of
  test_two_hop_rows' bit comparison, 12 of test_two_hop_blocks': rows such as {3}, {12}, {3})
* (e) write_col_part: three of the four waves added:                                                         108 / 23
"""
import types

import numpy as np
import pytest
import torch

import spmm_reference as R
import step_reference as sr
from test_gpu_step_kernels import (E_ALIGN, E_BADARG, L, U, _call, _dev, _dropout, _elu_bound, _exact, _np, _offset_copy, _p, _rng,  # noqa: F401
                                   _run, _same, _strided, _within)

pytestmark = pytest.mark.gpu

NAN = float("nan")
GATHER = 0x100
WORST = {}
GUARD = 8
VEC4_H = [4, 36, 256, 260, 512]
# (H, floats X and Y sit into their buffers): VEC = 1 by width, and by an unaligned operand at a width the vector path would take
VEC1_H = [(1, 0), (7, 0), (33, 0), (64, 1)]
SHAPES = [(H, 0) for H in VEC4_H] + VEC1_H
SHAPE_IDS = [f"H{H}" + ("-unaligned" if o else "") for H, o in SHAPES]


def _bounded(family, got, ref, bound, what):
    """_within, and the worst error / bound ratio of the family printed (run with -s) for the module docstring."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"[ratio] {family}: {what}: {ratio:.3g} (family worst {WORST[family]:.3g})")
    _within(got, ref, bound, what)


def _eq(a, b):
    """Bit equality of two outputs of the same launch shape (their untouched NaN padding compares equal)."""
    return torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))


def _i32(a):
    return _dev(np.asarray(a), torch.int32)


def _ld(H, off):
    """Leading dimensions (X, Y) above H: multiples of 4 where H is one (the scalar path is then taken for the pointer alone), odd
    ones otherwise."""
    return (H + 4, H + 8) if H % 4 == 0 else (H + 3, H + 6)


def _out(n, H, ld, off=0):
    """A NaN output [n, ld] `off` floats into its buffer, GUARD NaN elements behind it: (buffer, [n, ld] view)."""
    buf = torch.full((off + n * ld + GUARD,), NAN, dtype=torch.float32, device="cuda")
    return buf, buf[off:off + n * ld].view(n, ld)


def _operand(X, ld, off=0, nan_rows=0):
    """_strided with NaN padding, `nan_rows` rows of NaN behind the operand (zero rows a kernel must not load)."""
    X = np.asarray(X, dtype=np.float32)
    if nan_rows:
        X = np.concatenate([X, np.full((nan_rows, X.shape[1]), np.nan, np.float32)])
    return _strided(X, ld, off)


def _rows_of(records):
    """Row mask helper: the rows [r0, r1) of descriptor records (columns 0, 1)."""
    return [(int(r[0]), int(r[1])) for r in np.asarray(records).reshape(-1, 8) if r[1] > r[0]]


def _mask(n, ranges):
    m = np.zeros(n, dtype=bool)
    for a, b in ranges:
        m[a:b] = True
    return m


def _check_out(buf, full, H, off, touched, what):
    """Guards, row padding and the rows no record covers still NaN; returns the touched rows' H columns (float64), none of them NaN."""
    assert torch.isnan(buf[-GUARD:]).all().item() and torch.isnan(buf[:off]).all().item(), f"{what}: wrote outside the output"
    g = _np(full)
    assert np.isnan(g[:, H:]).all(), f"{what}: wrote into the columns H .. ld"
    assert np.isnan(g[~touched, :H]).all(), f"{what}: a row no record covers was written"
    got = g[touched, :H]
    assert not np.isnan(got).any(), f"{what}: a covered row was not written (or read a NaN)"
    return got


def _fwd_bound(Y, eY, bias, epi):
    """Forward epilogue at p = 0.5 on a product known to within eY: one rounding for the bias; ELU below zero: the __expf bound of
    test_gpu_step_kernels; the dropout scale 2 is exact."""
    b = np.zeros(Y.shape[1]) if not (epi & sr.EPI_BIAS) else np.asarray(bias, dtype=np.float64)
    y = Y + b[None, :]
    ey = eY + (U * np.abs(y) if epi & sr.EPI_BIAS else 0.0)
    scale = 2.0 if epi & sr.EPI_DROPOUT else 1.0
    return np.where(y <= 0, _elu_bound(y, ey, scale), scale * ey) if epi & sr.EPI_ELU else scale * ey


def _verify_forward(got, Y, eY, bias, epi, keep, exact, family, what):
    keep = np.ones(Y.shape, dtype=bool) if keep is None else keep
    ref = R.forward(Y, bias, epi, 0.5, keep)
    if epi & sr.EPI_DROPOUT:
        assert np.all(got[~keep] == 0), f"{what}: a dropped element is not zero"
    if not exact:
        _bounded(family, got, ref, np.where(keep, _fwd_bound(Y, eY, bias, epi), 0.0), what)
        return
    if epi & sr.EPI_ELU:                                       # only z > 0 is exact: __expf below
        z = Y + (np.asarray(bias, dtype=np.float64)[None, :] if epi & sr.EPI_BIAS else 0.0)
        sure = (z > 0) | ~keep
        _same(got[sure], ref[sure], what + " (z > 0)")
        _within(got[~sure], ref[~sure], _fwd_bound(Y, 0.0 * Y, bias, epi)[~sure], what + " (z <= 0)")
    else:
        _same(got, ref, what)


FWD_EPIS = {"none": (0, "none"), "bias": (sr.EPI_BIAS, "none"), "elu": (sr.EPI_ELU, "none"), "bias_elu": (sr.EPI_BIAS | sr.EPI_ELU, "none"),
            "mask": (0, "mask"), "bias_elu_mask": (sr.EPI_BIAS | sr.EPI_ELU, "mask"), "elu_hash": (sr.EPI_ELU, "hash"),
            "bias_hash_ptr": (sr.EPI_BIAS, "hash_ptr"), "bias_elu_hash_ptr": (sr.EPI_BIAS | sr.EPI_ELU, "hash_ptr")}
BWD_EPIS = {"elu": (sr.EPI_ELU, "none"), "mask": (0, "mask"), "hash": (0, "hash"), "elu_mask": (sr.EPI_ELU, "mask"),
            "elu_hash": (sr.EPI_ELU, "hash"), "elu_hash_ptr": (sr.EPI_ELU, "hash_ptr")}


class Epi:
    """One epilogue form on the device: flags, seed argument, mask, bias, the keep matrix of all rows."""

    def __init__(self, rng, name, n, H, exact, table=FWD_EPIS):
        flags, drop = table[name]
        d_flags, self.seed, self.mask, self.word, keep = _dropout(drop, n, H, rng)
        self.flags = flags | d_flags
        self.keep = keep(np.arange(n))
        self.bias = None
        if flags & sr.EPI_BIAS:
            self.bias = (rng.integers(-8, 9, size=H) / 8.0).astype(np.float32) if exact else rng.normal(size=H).astype(np.float32)
        self.bias_d = None if self.bias is None else _dev(self.bias)

    def rows(self, touched):
        return None if self.keep is None else self.keep[touched]


class Data:
    """A pattern with its operand on the host (float64 reference, magnitude, row bound) and on the device.
    table: (n_tab, zero_from) -- X is a de-duplicated table of n_tab rows behind xrow, rows >= zero_from are zero rows (NaN in memory: a
    kernel that loads one poisons its result); compact: the pattern's columns ARE operand rows (rows-compact form)."""

    def __init__(self, rng, csr, H, exact, off=0, table=None, compact_zero_from=None, n_cols=None):
        self.rowptr, self.col, self.val = csr
        self.n, self.H, self.off, self.exact = len(self.rowptr) - 1, H, off, exact
        self.nnz = int(self.rowptr[-1])
        self.lens = np.diff(self.rowptr.astype(np.int64))
        self.n_cols = self.n if n_cols is None else n_cols
        self.ldx, self.ldy = _ld(H, off)
        mk = (lambda s: R.exact_signal(rng, s)) if exact else (lambda s: rng.normal(size=s).astype(np.float32))
        self.xrow, self.zero_from, nan_rows = None, -1, 0
        if compact_zero_from is not None:
            self.zero_from, nan_rows = compact_zero_from, 3
            self.X = mk((max(compact_zero_from, 1), H))
            self.Y, self.S = R.spmm(self.rowptr, self.col, self.val, self.X, zero_from=compact_zero_from, n_cols=compact_zero_from + 3)
        elif table is not None:
            n_tab, zf = table
            self.xrow = rng.integers(0, n_tab, size=self.n_cols)
            self.zero_from = zf
            live = n_tab if zf < 0 else zf
            nan_rows = n_tab - live
            self.X = mk((live, H))
            self.Y, self.S = R.spmm(self.rowptr, self.col, self.val, self.X, xrow=self.xrow, zero_from=zf)
        else:
            self.X = mk((self.n_cols, H))
            self.Y, self.S = R.spmm(self.rowptr, self.col, self.val, self.X, n_cols=self.n_cols)
        self.eY = R.row_bound(self.rowptr, self.S)
        self.Xd = _operand(self.X, self.ldx, off, nan_rows)
        pad = self.nnz == 0
        self.rp_d, self.col_d = _i32(self.rowptr), _i32([0] if pad else self.col)
        self.val_d = _dev(np.zeros(1, np.float32) if pad else self.val)
        self.xrow_d = None if self.xrow is None else _i32(self.xrow)
        self.xcol_d = None if self.xrow is None else _i32(self.xrow[self.col] if self.nnz else [0])

    def csr_ptrs(self, L):
        return _p(L, self.rp_d), _p(L, self.col_d), _p(L, self.val_d)

    def prev(self, rng):
        """The forward's output of the layer below, [n, H] contiguous: integers over 8 (EXACT) or an ELU / dropout image."""
        if self.exact:
            return R.exact_signal(rng, (self.n, self.H))
        z = rng.normal(size=(self.n, self.H))
        return (np.where(z > 0, z, np.expm1(z)) * 2.0 * (rng.random((self.n, self.H)) < 0.8)).astype(np.float32)


def _valid_tiles(tiles, D, win_cols=None, n_operand=None):
    """Every index a launch will form lies inside its array (checked on the host before anything runs on the device)."""
    n_operand = D.n_cols if n_operand is None else n_operand
    for t in np.asarray(tiles).reshape(-1, 8):
        assert 0 <= t[0] <= t[1] <= D.n and t[4] == D.rowptr[t[0]] and t[5] == D.rowptr[t[1]] and t[7] == 0
        if t[6]:
            assert win_cols is not None and 0 <= t[2] and t[2] + t[3] <= len(win_cols)
        else:
            assert 0 <= t[2] and t[2] + t[3] <= n_operand
    if win_cols is not None:
        assert np.all((np.asarray(win_cols) >= 0) & (np.asarray(win_cols) < n_operand))
    assert D.nnz == 0 or (D.col.min() >= 0 and D.col.max() < n_operand)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tile kernel: fitgnn_spmm_csr_f32 / fitgnn_spmm_csr_dz_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def _tile_layout(w, n):
    """Row ranges of a hand-made tiling for a launch window of w rows: (r0, r1, win_begin, win_rows) or None (an empty record).
    The first nine records hold two empty ones; the last 7 rows belong to no tile."""
    specs = [(0, w, 0, w), None, (w, 3 * w + 3, w + 1, w),             # more rows than the window: row pointers beyond rp_rows from memory
             (3 * w + 3, 3 * w + 8, 2 * w, w + 24),                    # win_rows beyond the launched window: clamped, misses from memory
             (3 * w + 8, 3 * w + 9, 3 * w + 8, 1), None,               # one row: three waves without a row
             (3 * w + 9, 3 * w + 11, 3 * w + 9, 2), (3 * w + 11, 3 * w + 14, 3 * w + 10, 3), None]
    r = 3 * w + 14
    assert r < n - 7
    while r < n - 7:
        e = min(r + 2 * w, n - 7)
        specs.append((r, e, max(r - 3, 0), min(w, n - max(r - 3, 0))))
        r = e
    return specs


def _tile_pattern(rng, n, specs, exact, hits=True):
    """Row lengths cycle through TILE_LENGTHS (shifted per tile, so every tile kind meets many of them).  Rows of at most 16 entries:
    every third draws inside its tile's window (groups that are all hits), every third half inside / half outside (mixed groups), the
    others anywhere (misses, a few hits); longer rows anywhere."""
    lengths = R.cycle(R.TILE_LENGTHS, n)
    cols = {}
    for s in (s for s in specs if s is not None):
        r0, r1, w0, wn = s[:4]
        lengths[r0:r1] = R.cycle(R.TILE_LENGTHS, r1 - r0, start=r0 % 5)
    lengths = np.minimum(lengths, n)
    for s in (s for s in specs if s is not None):
        r0, r1, w0, wn = s[:4]
        inside = np.arange(w0, w0 + wn)
        outside = np.setdiff1d(np.arange(n), inside)
        for r in range(r0, r1):
            ln = int(lengths[r])
            if not hits or ln > 16 or ln == 0 or r % 3 == 2:
                continue
            k = min(ln, wn) if r % 3 == 0 else min(ln // 2, wn)
            cols[r] = np.concatenate([rng.permutation(inside)[:k], rng.permutation(outside)[:ln - k]])
    return R.make_csr(lengths, n, rng, exact=exact, cols=cols), lengths


def _launch_tile(L, D, tiles, n_tiles, window, epi=None, lcol=None, win_cols=None, use_xrow=True, gather=False, prev=None, col_part=None):
    """fitgnn_spmm_csr_f32 (prev None) or fitgnn_spmm_csr_dz_f32: (rc, output buffer, [n, ldy] view)."""
    buf, Y = _out(D.n, D.H, D.ldy, D.off)
    xr = D.xrow_d if use_xrow else None
    flags = (epi.flags if epi else 0) | (GATHER if gather else 0)
    seed, mask = (epi.seed, epi.mask) if epi else (0, None)
    head = (*D.csr_ptrs(L), _p(L, D.Xd), D.ldx, _p(L, Y), D.ldy, D.n, D.H, _p(L, tiles), n_tiles, _p(L, lcol), _p(L, win_cols), _p(L, xr),
            D.zero_from if xr is not None else -1, window)
    if prev is None:
        rc = _call(L, "fitgnn_spmm_csr_f32", *head, _p(L, epi.bias_d) if epi else None, flags, 0.5, seed, _p(L, mask))
    else:
        rc = _call(L, "fitgnn_spmm_csr_dz_f32", *head, _p(L, prev), flags, 0.5, seed, _p(L, mask), _p(L, col_part))
    return rc, buf, Y


# variant -> (launch window, plan: None / "contiguous" / "listed", operand table (n_tab, zero_from) or None)
TILE_VARIANTS = {
    "w16": (16, None, None),                      # <4, 16, PLAIN, NOEPI> / <4, 16, PLAIN> by the epilogue
    "w2": (2, None, None),                        # 60 rows; backward form: a window smaller than write_col_part's scratch
    "w5": (5, None, None),                        # a window below 16 rows that is not a multiple of 4
    "w16-planned": (16, "contiguous", None),      # <4, 16, !PLAIN>: lcol over contiguous windows
    "w16-listed": (16, "listed", None),           # ... listed windows, -(col + 1) misses, slots beyond a clamped window
    "w16-xrow": (16, None, (150, -1)),            # ... xrow alone, contiguous windows
    "w16-xrow-zero": (16, None, (150, 100)),      # ... zero rows inside and outside the windows
    "w16-listed-xrow-zero": (16, "listed", (150, 100)),
    "w17": (17, None, None),                      # <8, 32, !PLAIN>: the smallest window of the large instantiation
    "w40-listed-xrow-zero": (40, "listed", (150, 100)),
    "w96": (96, None, None),                      # VEC = 4: 98 KiB of window, above 64 KiB of LDS (hipFuncSetAttribute)
    "w200": (200, None, None),                    # window_rows above the maximum: the launcher clamps it to 96
}


def _tile_case(rng, H, off, variant, exact):
    w, plan, table = TILE_VARIANTS[variant]
    lw = min(w, 96)
    n = 60 if lw < 5 else 340 if lw <= 40 else 460
    specs = _tile_layout(lw, n)
    csr, _ = _tile_pattern(rng, n, specs, exact)
    D = Data(rng, csr, H, exact, off, table=table)
    lcol = win_cols = None
    if plan is None:
        tiles = R.tile_records(D.rowptr, specs)
    else:
        pspecs = []
        for i, s in enumerate(specs):
            if s is None:
                pspecs.append(None)
            elif plan == "contiguous" or i % 2 == 0:
                pspecs.append((s[0], s[1], (s[2], s[3])))
            else:        # the rows' own columns in random order, up to 8 beyond the launched window, and two rows nothing references
                used = np.unique(D.col[D.rowptr[s[0]]:D.rowptr[s[1]]])
                pspecs.append((s[0], s[1], [int(v) for v in rng.permutation(used)[:lw + 6]] + [0, n - 1]))
        tiles, win_cols, lcol = R.plan_windows(D.rowptr, D.col, pspecs)
        assert np.array_equal(R.resolve_lcol(tiles, win_cols, lcol, D.rowptr)[:D.rowptr[n - 7]], D.col[:D.rowptr[n - 7]])
        assert (lcol < 0).any() and (plan != "listed" or (lcol >= lw).any())
    _valid_tiles(tiles, D, win_cols)
    return D, tiles, _i32(tiles), None if lcol is None else _i32(lcol), None if win_cols is None else _i32(win_cols), w


# every variant at three widths (one slab with dead lanes, two slabs, the scalar path), every width at three variants
TILE_PRODUCT_CASES = [(H, o, v) for (H, o) in SHAPES for v in TILE_VARIANTS
                      if (H, o) in ((36, 0), (260, 0), (33, 0)) or v in ("w16", "w16-listed-xrow-zero", "w96")]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("H,off,variant", TILE_PRODUCT_CASES, ids=lambda v: str(v))
def test_tile_product(L, H, off, variant, exact):
    rng = _rng("tile", H, off, variant, exact)
    D, tiles, tiles_d, lcol, win_cols, w = _tile_case(rng, H, off, variant, exact)
    assert len(tiles) > 9 and (tiles[:9, 1] == tiles[:9, 0]).sum() == 3
    lw = min(w, 96)
    assert (D.rowptr[tiles[:, 1]] - D.rowptr[tiles[:, 0]]).max() > lw * (16 if lw <= 16 else 32)     # entries beyond the staged slice (lds_rows * MPR)
    for n_tiles in (1, 8, 9, len(tiles)):
        rc, buf, Y = _launch_tile(L, D, tiles_d, n_tiles, w, lcol=lcol, win_cols=win_cols)
        L.check(rc, "fitgnn_spmm_csr_f32")
        touched = _mask(D.n, _rows_of(tiles[:n_tiles]))
        got = _check_out(buf, Y, H, off, touched, f"Y ({n_tiles} tiles)")
        if exact:
            _same(got, D.Y[touched], f"Y ({n_tiles} tiles)")
        else:
            _bounded("tile", got, D.Y[touched], D.eY[touched], f"Y ({n_tiles} tiles)")
    if not exact:
        rc, _, Y2 = _launch_tile(L, D, tiles_d, len(tiles), w, lcol=lcol, win_cols=win_cols)
        assert _eq(Y, Y2), "two launches on the same input differ"


EPI_SHAPES = [(36, 0), (260, 0), (33, 0), (64, 1)]
TILE_EPI_CASES = [(*EPI_SHAPES[(i + j) % 4], v, e) for i, e in enumerate(k for k in FWD_EPIS if k != "none")
                  for j, v in enumerate(["w16", "w16-listed-xrow-zero", "w40-listed-xrow-zero"])]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("H,off,variant,epi_name", TILE_EPI_CASES, ids=lambda v: str(v))
def test_tile_forward_epilogues(L, H, off, variant, epi_name, exact):
    """<4 | 1, 16, PLAIN> (an epilogue flag on contiguous windows), <.., 16, !PLAIN> and <.., 8, 32> with every forward flag form."""
    rng = _rng("tile_epi", H, off, variant, epi_name, exact)
    D, tiles, tiles_d, lcol, win_cols, w = _tile_case(rng, H, off, variant, exact)
    epi = Epi(rng, epi_name, D.n, H, exact)
    rc, buf, Y = _launch_tile(L, D, tiles_d, len(tiles), w, epi, lcol, win_cols)
    L.check(rc, "fitgnn_spmm_csr_f32")
    touched = _mask(D.n, _rows_of(tiles))
    got = _check_out(buf, Y, H, off, touched, "Y")
    _verify_forward(got, D.Y[touched], D.eY[touched], epi.bias, epi.flags, epi.rows(touched), exact, "tile forward epilogue", f"Y ({epi_name})")


def _rows_of_wave_tile(tiles):
    return -(-(tiles[:, 1] - tiles[:, 0]) // 4)


def _verify_dz(got, D, prev, epi, touched, family, what):
    """dZ of the touched rows against the reference; returns (dZ reference, its bound) over ALL rows for the column sums."""
    keep = epi.keep
    dZ, f = R.backward(D.Y, prev, epi.flags, 0.5, keep)
    bound = R.dz_bound(f, D.eY, dZ)
    if epi.flags & sr.EPI_DROPOUT:
        assert np.all(got[~keep[touched]] == 0), f"{what}: a dropped element is not zero"
    if D.exact:
        _same(got, dZ[touched], what)
    else:
        _bounded(family, got, dZ[touched], bound[touched], what)
    return dZ, bound


def _verify_col_part(cp_buf, cp, D, dZ, bound, ranges, rows_of_wave, written, family, what, untouched=0.0):
    """col_part [parts, H]: the rows in `written` against the column sums of their range (bit for bit where colsum_is_exact certifies
    the column, else within colsum_bound); the other rows still hold what the caller put there; the guard behind it intact."""
    assert torch.isnan(cp_buf[-GUARD:]).all().item(), f"{what}: wrote past the end of col_part"
    got = _np(cp)
    rg = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    s, a = R.colsums(dZ, rg)
    written = np.asarray(written, dtype=bool)
    rest = got[~written]
    assert np.all(np.isnan(rest)) if np.isnan(untouched) else np.all(rest == untouched), f"{what}: a partial row of no record was written"
    assert not np.isnan(got[written]).any(), f"{what}: a partial row was not written"
    b = R.colsum_bound(bound, a, rg, rows_of_wave)
    if D.exact:
        sure = np.stack([R.colsum_is_exact(a[i], D.lens[r0:r1].max() if r1 > r0 else 1) for i, (r0, r1) in enumerate(rg)]) if len(rg) else a > 0
        assert not written.any() or sure[written].mean() > 0.9
        _same(got[written][sure[written]], s[written][sure[written]], what)
        _within(got[written][~sure[written]], s[written][~sure[written]], b[written][~sure[written]], what)
    else:
        _bounded(family, got[written], s[written], b[written], what)


def _col_part(parts, H, fill):
    buf = torch.full((parts * H + GUARD,), NAN, dtype=torch.float32, device="cuda")
    buf[:parts * H] = fill
    return buf, buf[:parts * H].view(parts, H)


DZ_H = [4, 36, 260, 512]
TILE_DZ_CASES = [(DZ_H[(i + j) % 4], v, e) for i, e in enumerate(BWD_EPIS)
                 for j, v in enumerate(["w16", "w2", "w16-listed-xrow-zero", "w40-listed-xrow-zero", "w96"])]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("H,variant,epi_name", TILE_DZ_CASES, ids=lambda v: str(v))
def test_tile_dz(L, H, variant, epi_name, exact):
    """fitgnn_spmm_csr_dz_f32: <4, 16, PLAIN>, <4, 16, !PLAIN>, <4, 8, 32> with the backward store; w2: a window of two rows, smaller than
    write_col_part's scratch (the launcher sizes the LDS for it).  col_part rows of empty records come back as the zeros the caller put
    there (the tile kernel stores the zero sums of a record without rows)."""
    rng = _rng("tile_dz", H, variant, epi_name, exact)
    D, tiles, tiles_d, lcol, win_cols, w = _tile_case(rng, H, 0, variant, exact)
    prev = D.prev(rng)
    prev_d = _dev(prev)
    epi = Epi(rng, epi_name, D.n, H, exact, BWD_EPIS)
    touched = _mask(D.n, _rows_of(tiles))
    cp_buf, cp = _col_part(len(tiles), H, 0.0)
    rc, buf, Y = _launch_tile(L, D, tiles_d, len(tiles), w, epi, lcol, win_cols, prev=prev_d, col_part=cp)
    L.check(rc, "fitgnn_spmm_csr_dz_f32")
    got = _check_out(buf, Y, H, 0, touched, "dZ")
    dZ, bound = _verify_dz(got, D, prev, epi, touched, "tile dz", f"dZ ({epi_name})")
    _verify_col_part(cp_buf, cp, D, dZ, bound, tiles[:, :2], _rows_of_wave_tile(tiles), tiles[:, 1] > tiles[:, 0], "tile col_part", "col_part")
    rc, buf2, Y2 = _launch_tile(L, D, tiles_d, len(tiles), w, epi, lcol, win_cols, prev=prev_d, col_part=None)   # col_part NULL
    L.check(rc, "fitgnn_spmm_csr_dz_f32")
    assert _eq(Y, Y2), "dZ depends on col_part being given"


def test_tile_refusals(L):
    rng = _rng("tile_refusals")
    specs = [(0, 8, 0, 8)]
    D = Data(rng, R.make_csr([1, 2, 3, 0, 4, 5, 1, 1], 8, rng, exact=True), 8, True)
    tiles = _i32(R.tile_records(D.rowptr, specs))
    prev = _dev(D.prev(rng))
    epi = Epi(rng, "elu", 8, 8, True, BWD_EPIS)
    assert _launch_tile(L, D, tiles, 1, 0, epi, prev=prev)[0] == 0
    assert _launch_tile(L, D, tiles, 1, 0, epi, prev=_offset_copy(D.prev(rng), 1))[0] == E_BADARG      # prev not 16-byte aligned
    D1 = Data(rng, (D.rowptr, D.col, D.val), 8, True, off=1)
    assert _launch_tile(L, D1, tiles, 1, 0, epi, prev=prev)[0] == E_ALIGN                               # X / Y one float into their buffers
    D7 = Data(rng, (D.rowptr, D.col, D.val), 7, True)
    assert _launch_tile(L, D7, tiles, 1, 0, Epi(rng, "elu", 8, 7, True, BWD_EPIS), prev=prev)[0] == E_BADARG    # H % 4 != 0
    assert _launch_tile(L, D, tiles, 1, 0, Epi(rng, "bias", 8, 8, True), prev=prev)[0] == E_BADARG       # no bias in the backward form
    bwd = types.SimpleNamespace(flags=0x10, seed=0, mask=None, bias_d=None)
    assert _launch_tile(L, D, tiles, 1, 0, bwd)[0] == E_BADARG                                           # FITGNN_EPI_BACKWARD on the forward entry
    lcol = _i32(np.zeros(D.nnz))
    assert _launch_tile(L, D, tiles, 1, 0, win_cols=lcol)[0] == E_BADARG                                 # win_cols without lcol
    assert _launch_tile(L, D, tiles, 1, -1)[0] == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the direct-gather kernel: fitgnn_spmm_csr_f32 with FITGNN_SPMM_GATHER
# ---------------------------------------------------------------------------------------------------------------------------------
def _gather_layout():
    """(lengths, tile specs, rows of the general-path tiles).  A wave owns ceil(rows / 4) consecutive rows of its tile; the fast path
    needs <= 63 rows and <= 64 entries per wave."""
    parts = [("fast-even", [0, 1, 4, 5, 9, 0, 1, 4]),                                   # two rows per wave; an empty row first, one last
             ("fast-odd", [5, 0, 1, 0, 9, 4, 1, 1, 1, 4, 4, 0]),                        # three rows per wave: the qa / qb tail
             ("fast-full", [9, 9, 9, 9, 9, 9, 10, 0] + [0, 0, 0, 64, 0, 0, 0, 0] + [1] * 8 + [8] * 8),   # 64 entries, the last row empty: lo == 64
             ("one", [5]), ("two", [0, 9]), ("three", [4, 1, 0]),                       # waves without a row
             ("gap", [3, 3]),                                                           # rows of no tile
             ("general-entries", [3, 64, 67, 4, 5, 65, 4, 61]),                         # 67, 71, 70, 65 entries per wave
             ("general-rows", list(R.cycle([0, 1, 2, 0, 3], 256))),                     # 64 rows per wave
             ("fast-63", list(R.cycle([1, 0, 2, 0, 1], 252))),                          # 63 rows per wave, 50 / 51 entries
             ("gap", [1, 0, 2])]
    lengths, specs, general, r = [], [], [], 0
    for name, ln in parts:
        if name != "gap":
            specs.append((r, r + len(ln), r, min(len(ln), 16)))
            if name.startswith("general"):
                general.append((r, r + len(ln)))
        if name in ("one", "fast-odd"):
            specs.append(None)
        lengths += ln
        r += len(ln)
    return np.asarray(lengths, dtype=np.int64), specs, general


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("table", [None, (150, -1)], ids=["plain", "xrow"])
@pytest.mark.parametrize("H,off", SHAPES, ids=SHAPE_IDS)
def test_gather_product(L, H, off, table, exact):
    rng = _rng("gather", H, off, table, exact)
    lengths, specs, general = _gather_layout()
    D = Data(rng, R.make_csr(lengths, len(lengths), rng, exact=exact), H, exact, off, table=table)
    tiles = R.tile_records(D.rowptr, specs)
    _valid_tiles(tiles, D)
    tiles_d = _i32(tiles)
    touched = _mask(D.n, _rows_of(tiles))
    assert not touched.all()
    rc, buf, Y = _launch_tile(L, D, tiles_d, len(tiles), 0, gather=True)
    L.check(rc, "fitgnn_spmm_csr_f32")
    got = _check_out(buf, Y, H, off, touched, "Y")
    if exact:
        _same(got, D.Y[touched], "Y")
    else:
        _bounded("gather", got, D.Y[touched], D.eY[touched], "Y")
        rc, _, Y2 = _launch_tile(L, D, tiles_d, len(tiles), 0, gather=True)
        assert _eq(Y, Y2), "two launches on the same input differ"
        rc, _, Yt = _launch_tile(L, D, tiles_d, len(tiles), 0)                        # the tile kernel on the same records
        L.check(rc, "fitgnn_spmm_csr_f32")
        g = torch.from_numpy(_mask(D.n, general)).cuda()
        assert _eq(Y[g], Yt[g]), "the gather kernel's general path and the tile kernel differ in bits"


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("epi_name", ["bias", "bias_elu_mask", "elu_hash", "bias_elu_hash_ptr"])
@pytest.mark.parametrize("H,off", [(36, 0), (260, 0), (33, 0)], ids=["H36", "H260", "H33"])
def test_gather_forward_epilogues(L, H, off, epi_name, exact):
    rng = _rng("gather_epi", H, off, epi_name, exact)
    lengths, specs, _ = _gather_layout()
    D = Data(rng, R.make_csr(lengths, len(lengths), rng, exact=exact), H, exact, off)
    tiles = R.tile_records(D.rowptr, specs)
    epi = Epi(rng, epi_name, D.n, H, exact)
    rc, buf, Y = _launch_tile(L, D, _i32(tiles), len(tiles), 0, epi, gather=True)
    L.check(rc, "fitgnn_spmm_csr_f32")
    touched = _mask(D.n, _rows_of(tiles))
    got = _check_out(buf, Y, H, off, touched, "Y")
    _verify_forward(got, D.Y[touched], D.eY[touched], epi.bias, epi.flags, epi.rows(touched), exact, "gather forward epilogue", f"Y ({epi_name})")


@pytest.mark.parametrize("H,off", [(36, 0), (33, 0)], ids=["H36", "H33"])
def test_gather_with_zero_rows_runs_the_tile_kernel(L, H, off):
    """FITGNN_SPMM_GATHER with xrow_zero_from >= 0: the gather kernel knows no zero rows (it would load them: NaN here), the launcher
    drops the flag."""
    rng = _rng("gather_zero", H, off)
    lengths, specs, _ = _gather_layout()
    D = Data(rng, R.make_csr(lengths, len(lengths), rng, exact=True), H, True, off, table=(150, 100))
    tiles = R.tile_records(D.rowptr, specs)
    rc, buf, Y = _launch_tile(L, D, _i32(tiles), len(tiles), 0, gather=True)
    L.check(rc, "fitgnn_spmm_csr_f32")
    touched = _mask(D.n, _rows_of(tiles))
    _same(_check_out(buf, Y, H, off, touched, "Y"), D.Y[touched], "Y")


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole-subgraph kernel: fitgnn_spmm_csr_blocks_f32 / _dz_f32
# ---------------------------------------------------------------------------------------------------------------------------------
BLOCK_N = 360
# an empty block at row 0 (nnz_begin == nnz_end == 0), blocks of 1, 15, 16, 17, 33, 200 rows, empty rows in the middle, 33, 20; rows 350 ... 359: no block
BLOCK_RANGES = [(0, 5), (5, 6), (6, 21), (21, 37), (37, 54), (54, 87), (87, 287), (287, 297), (297, 330), (330, 350)]
BLOCK_LONG = {6: [90, 100, 150, 200, 250, 286], 8: [300], 9: [331, 335, 340, 349]}     # n_long 6 (two not carried), 1, 4; the others 0
BLOCK_ORDER = [6, None, 0, 3, 9, None, 1, 2, 7, 4, 5, 8]                               # records: n_blocks = 1 is the 200-row block alone
DENSE_PIECE = (87 + 48, 87 + 64)                                                       # a piece of 12-entry rows: 180 entries > kBlkMeta


def _block_pattern(rng, exact):
    n = BLOCK_N
    cols = {}
    every = np.arange(n)
    for b, (r0, r1) in enumerate(BLOCK_RANGES + [(350, 360)]):
        longs = BLOCK_LONG.get(b, [])
        hub = longs[0] if longs else None
        inside = np.arange(r0, r1)
        for r in range(r0, r1):
            if b in (0, 7):
                cols[r] = []                                                             # blocks of empty rows
            elif r in (90, 200):
                cols[r] = rng.permutation(every)[:300]                                   # 300 entries: before, inside and after the block
            elif r in longs:                                                             # 65 entries: 20 before, 25 inside (as many as fit), 20 after
                k = min(25, r1 - r0)
                cols[r] = np.concatenate([rng.permutation(np.arange(0, r0))[:20], rng.permutation(inside)[:k],
                                          rng.permutation(np.arange(r1, n))[:45 - k]])
            elif DENSE_PIECE[0] <= r < DENSE_PIECE[1]:
                cols[r] = np.concatenate([[90, 200], rng.permutation(np.setdiff1d(every, [90, 200]))[:10]])
            else:
                ln = [0, 1, 2, 3, 4, 5, 9][(r + b) % 7]
                pool = every if r % 4 == 1 else inside                                   # anywhere / the block (other pieces: gathered)
                c = list(rng.permutation(pool)[:min(ln, len(pool))])
                if hub is not None and r % 2 == 0 and ln:
                    c[0] = hub                                                           # a carried long row: the pinned slot
                cols[r] = c
    return R.make_csr(np.zeros(n, dtype=np.int64), n, rng, exact=exact, cols=cols)


def _fix_xrow(D, rng, fixes):
    """Give chosen pattern columns a chosen table row and redo the reference."""
    for c, t in fixes.items():
        D.xrow[c] = t
    D.Y, D.S = R.spmm(D.rowptr, D.col, D.val, D.X, xrow=D.xrow, zero_from=D.zero_from)
    D.eY = R.row_bound(D.rowptr, D.S)
    D.xrow_d, D.xcol_d = _i32(D.xrow), _i32(D.xrow[D.col])


def _block_case(rng, H, exact, table):
    D = Data(rng, _block_pattern(rng, exact), H, exact, table=table)
    if table is not None and table[1] >= 0:
        _fix_xrow(D, rng, {90: table[0] - 1, 100: 0})                                    # a carried long row that is a zero row, one that is not
    assert D.rowptr[5] == 0 and D.lens[DENSE_PIECE[0]:DENSE_PIECE[1]].sum() > 128 and D.lens[90] == 300 and D.lens[286] == 65
    ranges = [None if b is None else BLOCK_RANGES[b] for b in BLOCK_ORDER]
    longs = {i: BLOCK_LONG[b] for i, b in enumerate(BLOCK_ORDER) if b in BLOCK_LONG}
    blocks, long_rows = R.block_records(D.rowptr, ranges, long_rows=longs)
    assert blocks[0, 5] == 6 and np.all((long_rows >= 0) & (long_rows < D.n)) and blocks[2].tolist()[:4] == [0, 5, 0, 0]
    return D, blocks, _i32(blocks), _i32(long_rows)


def _launch_blocks(L, D, blocks_d, n_blocks, long_d, epi=None, use_xcol=True, prev=None, col_part=None):
    buf, Y = _out(D.n, D.H, D.ldy, D.off)
    flags = epi.flags if epi else 0
    seed, mask = (epi.seed, epi.mask) if epi else (0, None)
    head = (*D.csr_ptrs(L), _p(L, D.Xd), D.ldx, _p(L, Y), D.ldy, D.n, D.H, _p(L, blocks_d), n_blocks, _p(L, long_d), _p(L, D.xrow_d),
            _p(L, D.xcol_d if use_xcol else None), D.zero_from)
    if prev is None:
        rc = _call(L, "fitgnn_spmm_csr_blocks_f32", *head, _p(L, epi.bias_d) if epi else None, flags, 0.5, seed, _p(L, mask))
    else:
        rc = _call(L, "fitgnn_spmm_csr_blocks_dz_f32", *head, _p(L, prev), flags, 0.5, seed, _p(L, mask), _p(L, col_part))
    return rc, buf, Y


BLOCK_TABLES = {"plain": (None, True), "xrow": ((200, -1), False), "xrow-xcol": ((200, -1), True), "xrow-zero": ((200, 150), False),
                "xrow-xcol-zero": ((200, 150), True)}


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("form", list(BLOCK_TABLES))
@pytest.mark.parametrize("H", VEC4_H)
def test_blocks_product(L, H, form, exact):
    """<false, false, NOEPI> (plain) and <true, false> (a table) without an epilogue flag."""
    rng = _rng("blocks", H, form, exact)
    table, use_xcol = BLOCK_TABLES[form]
    D, blocks, blocks_d, long_d = _block_case(rng, H, exact, table)
    for n_blocks in (1, 9, len(blocks)):
        rc, buf, Y = _launch_blocks(L, D, blocks_d, n_blocks, long_d, use_xcol=use_xcol)
        L.check(rc, "fitgnn_spmm_csr_blocks_f32")
        touched = _mask(D.n, _rows_of(blocks[:n_blocks]))
        got = _check_out(buf, Y, H, 0, touched, f"Y ({n_blocks} records)")
        if exact:
            _same(got, D.Y[touched], f"Y ({n_blocks} records)")
        else:
            _bounded("blocks", got, D.Y[touched], D.eY[touched], f"Y ({n_blocks} records)")
    if not exact:
        rc, _, Y2 = _launch_blocks(L, D, blocks_d, len(blocks), long_d, use_xcol=use_xcol)
        assert _eq(Y, Y2), "two launches on the same input differ"


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("epi_name", ["bias", "bias_elu_mask", "elu_hash", "bias_elu_hash_ptr"])
@pytest.mark.parametrize("form", ["plain", "xrow-xcol-zero"])
@pytest.mark.parametrize("H", [36, 260])
def test_blocks_forward_epilogues(L, H, form, epi_name, exact):
    """<false, false> and <true, false> with the forward epilogue."""
    rng = _rng("blocks_epi", H, form, epi_name, exact)
    table, use_xcol = BLOCK_TABLES[form]
    D, blocks, blocks_d, long_d = _block_case(rng, H, exact, table)
    epi = Epi(rng, epi_name, D.n, H, exact)
    rc, buf, Y = _launch_blocks(L, D, blocks_d, len(blocks), long_d, epi, use_xcol)
    L.check(rc, "fitgnn_spmm_csr_blocks_f32")
    touched = _mask(D.n, _rows_of(blocks))
    got = _check_out(buf, Y, H, 0, touched, "Y")
    _verify_forward(got, D.Y[touched], D.eY[touched], epi.bias, epi.flags, epi.rows(touched), exact, "blocks forward epilogue", f"Y ({epi_name})")


BLOCKS_DZ_CASES = [(DZ_H[(i + j) % 4], f, e) for i, e in enumerate(BWD_EPIS) for j, f in enumerate(["plain", "xrow-zero", "xrow-xcol-zero"])]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("H,form,epi_name", BLOCKS_DZ_CASES, ids=lambda v: str(v))
def test_blocks_dz(L, H, form, epi_name, exact):
    """<false, true> and <true, true>; col_part per block, the rows of empty records left as the caller zeroed them."""
    rng = _rng("blocks_dz", H, form, epi_name, exact)
    table, use_xcol = BLOCK_TABLES[form]
    D, blocks, blocks_d, long_d = _block_case(rng, H, exact, table)
    prev = D.prev(rng)
    prev_d = _dev(prev)
    epi = Epi(rng, epi_name, D.n, H, exact, BWD_EPIS)
    touched = _mask(D.n, _rows_of(blocks))
    cp_buf, cp = _col_part(len(blocks), H, 0.0)
    rc, buf, Y = _launch_blocks(L, D, blocks_d, len(blocks), long_d, epi, use_xcol, prev_d, cp)
    L.check(rc, "fitgnn_spmm_csr_blocks_dz_f32")
    got = _check_out(buf, Y, H, 0, touched, "dZ")
    dZ, bound = _verify_dz(got, D, prev, epi, touched, "blocks dz", f"dZ ({epi_name})")
    rows = blocks[:, 1] - blocks[:, 0]
    _verify_col_part(cp_buf, cp, D, dZ, bound, blocks[:, :2], 4 * -(-rows // 16) + 1, rows > 0, "blocks col_part", "col_part")
    rc, _, Y2 = _launch_blocks(L, D, blocks_d, len(blocks), long_d, epi, use_xcol, prev_d, None)
    L.check(rc, "fitgnn_spmm_csr_blocks_dz_f32")
    assert _eq(Y, Y2), "dZ depends on col_part being given"


def test_blocks_refusals(L):
    rng = _rng("blocks_refusals")
    csr = R.make_csr([1, 2, 3, 0, 4, 5, 1, 1], 8, rng, exact=True)
    blocks = lambda D: _i32(R.block_records(D.rowptr, [(0, 8)])[0])   # noqa: E731
    D = Data(rng, csr, 36, True)
    assert _launch_blocks(L, D, blocks(D), 1, None)[0] == 0                                              # H = 36: a multiple of 4
    D7 = Data(rng, csr, 7, True)
    assert _launch_blocks(L, D7, blocks(D7), 1, None)[0] == E_BADARG
    D1 = Data(rng, csr, 36, True, off=1)
    assert _launch_blocks(L, D1, blocks(D1), 1, None)[0] == E_ALIGN
    D.xcol_d = D.col_d
    assert _launch_blocks(L, D, blocks(D), 1, None)[0] == E_BADARG                                       # xcol without xrow
    D.xcol_d = None
    epi = Epi(rng, "elu", 8, 36, True, BWD_EPIS)
    assert _launch_blocks(L, D, blocks(D), 1, None, epi, prev=_offset_copy(D.prev(rng), 1))[0] == E_BADARG
    assert _launch_blocks(L, D, blocks(D), 1, None, types.SimpleNamespace(flags=0x10, seed=0, mask=None, bias_d=None))[0] == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the segment-streaming kernel: fitgnn_spmm_csr_stream_f32 / _dz_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def _stream_layout():
    """(segment sizes, segments per range): a range of one 5-row segment; an empty range; 130 segments of 1 / 2 rows (a second seg_ptr
    batch; 200 rows: three row-pointer batches); one 70-row segment; hubs alone / with one leaf / with 130 entries before their leaves."""
    many = [1 if i % 13 < 6 else 2 for i in range(130)]
    assert sum(many) == 200
    return [5] + many + [70] + [1, 2, 5, 3], [1, 0, 130, 1, 4]


def _stream_pattern(rng, exact):
    sizes, per_range = _stream_layout()
    seg_ptr, range_seg = R.segments(sizes, per_range)
    n = int(seg_ptr[-1])
    every = np.arange(n)
    hub_len = {0: 3, 205: 200, 275: 64, 276: 65, 278: 130, 283: 3}
    cols = {}
    for s in range(len(sizes)):
        h, e = int(seg_ptr[s]), int(seg_ptr[s + 1])
        left, inside, right = np.arange(0, h), np.arange(h, e), np.arange(e, n)
        ln = hub_len.get(h, [1, 2, 3, 4][s % 4])
        take_in = inside if ln >= 64 else rng.permutation(inside)[:max(ln // 2, 1)]       # a big hub references every row of its segment
        rest = ln - len(take_in)
        n_right = min(len(right), max(rest // 4, 1 if rest else 0))
        n_left = min(len(left), rest - n_right)
        cols[h] = np.concatenate([rng.permutation(left)[:n_left], take_in, rng.permutation(right)[:n_right + (rest - n_right - n_left)]])
        for r in range(h + 1, e):                                                          # leaves: own entry, the hub's, others
            ln = [1, 2, 4, 5, 9][r % 5]
            c = [r] if r % 2 == 0 else []
            c += [h] if r % 3 != 0 else []
            c = c[:ln]
            cols[r] = np.concatenate([c, rng.permutation(np.setdiff1d(every, c))[:ln - len(c)]]).astype(np.int64)
    csr = R.make_csr(np.zeros(n, dtype=np.int64), n, rng, exact=exact, cols=cols)
    lens = np.diff(csr[0])
    assert lens[205] == 200 and lens[278] == 130 and lens[275] == 64 and lens[276] == 65 and lens[0] == 3
    return csr, seg_ptr, range_seg


def _launch_stream(L, D, seg_d, n_seg, rs_d, n_ranges, epi=None, prev=None, col_part=None, xrow="both", nnz=None):
    buf, Y = _out(D.n, D.H, D.ldy, D.off)
    flags = epi.flags if epi else 0
    seed, mask = (epi.seed, epi.mask) if epi else (0, None)
    xr = D.xrow_d if xrow in ("both", "xrow") else None
    xc = D.xcol_d if xrow in ("both", "xcol") else None
    head = (*D.csr_ptrs(L), D.nnz if nnz is None else nnz, _p(L, D.Xd), D.ldx, _p(L, Y), D.ldy, D.n, D.H, _p(L, seg_d), n_seg, _p(L, rs_d), n_ranges,
            _p(L, xr), _p(L, xc))
    if prev is None:
        rc = _call(L, "fitgnn_spmm_csr_stream_f32", *head, _p(L, epi.bias_d) if epi else None, flags, 0.5, seed, _p(L, mask))
    else:
        rc = _call(L, "fitgnn_spmm_csr_stream_dz_f32", *head, _p(L, prev), flags, 0.5, seed, _p(L, mask), _p(L, col_part))
    return rc, buf, Y


def _valid_stream(D, seg_ptr, range_seg):
    assert seg_ptr[0] == 0 and seg_ptr[-1] == D.n and np.all(np.diff(seg_ptr) >= 1) and range_seg[0] == 0 and range_seg[-1] == len(seg_ptr) - 1
    assert np.all(np.diff(range_seg) >= 0) and D.nnz > 0 and D.col.min() >= 0 and D.col.max() < D.n_cols


# (table, epilogue): the six instantiations <XROW, BWD, NOEPI>; the dz forms are test_stream_dz
STREAM_FORMS = {"plain": (None, "none"), "plain-epi": (None, "bias_elu_mask"), "plain-hash": (None, "bias_elu_hash_ptr"),
                "xrow": ((150, -1), "none"), "xrow-epi": ((150, -1), "bias_elu_mask"), "xrow-hash": ((150, -1), "elu_hash")}


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("form", list(STREAM_FORMS))
@pytest.mark.parametrize("H", VEC4_H)
def test_stream_forward(L, H, form, exact):
    rng = _rng("stream", H, form, exact)
    table, epi_name = STREAM_FORMS[form]
    csr, seg_ptr, range_seg = _stream_pattern(rng, exact)
    D = Data(rng, csr, H, exact, table=table)
    _valid_stream(D, seg_ptr, range_seg)
    n_ranges = len(range_seg) - 1
    assert (n_ranges * -(-H // 256)) % 4 != 0
    epi = None if epi_name == "none" else Epi(rng, epi_name, D.n, H, exact)
    seg_d, rs_d = _i32(seg_ptr), _i32(range_seg)
    rc, buf, Y = _launch_stream(L, D, seg_d, len(seg_ptr) - 1, rs_d, n_ranges, epi)
    L.check(rc, "fitgnn_spmm_csr_stream_f32")
    touched = np.ones(D.n, dtype=bool)
    got = _check_out(buf, Y, H, 0, touched, "Y")
    if epi is None:
        if exact:
            _same(got, D.Y, "Y")
        else:
            _bounded("stream", got, D.Y, D.eY, "Y")
    else:
        _verify_forward(got, D.Y, D.eY, epi.bias, epi.flags, epi.keep, exact, "stream forward epilogue", f"Y ({epi_name})")
    if not exact:
        rc, _, Y2 = _launch_stream(L, D, seg_d, len(seg_ptr) - 1, rs_d, n_ranges, epi)
        assert _eq(Y, Y2), "two launches on the same input differ"


STREAM_DZ_CASES = [(DZ_H[(i + j) % 4], t, e) for i, e in enumerate(BWD_EPIS) for j, t in enumerate([None, (150, -1)])]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("H,table,epi_name", STREAM_DZ_CASES, ids=lambda v: str(v))
def test_stream_dz(L, H, table, epi_name, exact):
    """<false, true, false> and <true, true, false>; col_part: one row per range, every element written, an empty range exactly 0."""
    rng = _rng("stream_dz", H, table, epi_name, exact)
    csr, seg_ptr, range_seg = _stream_pattern(rng, exact)
    D = Data(rng, csr, H, exact, table=table)
    _valid_stream(D, seg_ptr, range_seg)
    n_ranges = len(range_seg) - 1
    prev = D.prev(rng)
    prev_d = _dev(prev)
    epi = Epi(rng, epi_name, D.n, H, exact, BWD_EPIS)
    cp_buf, cp = _col_part(n_ranges, H, NAN)
    seg_d, rs_d = _i32(seg_ptr), _i32(range_seg)
    rc, buf, Y = _launch_stream(L, D, seg_d, len(seg_ptr) - 1, rs_d, n_ranges, epi, prev_d, cp)
    L.check(rc, "fitgnn_spmm_csr_stream_dz_f32")
    touched = np.ones(D.n, dtype=bool)
    got = _check_out(buf, Y, H, 0, touched, "dZ")
    dZ, bound = _verify_dz(got, D, prev, epi, touched, "stream dz", f"dZ ({epi_name})")
    ranges = np.stack([seg_ptr[range_seg[:-1]], seg_ptr[range_seg[1:]]], 1)
    _verify_col_part(cp_buf, cp, D, dZ, bound, ranges, ranges[:, 1] - ranges[:, 0] - 4, np.ones(n_ranges, dtype=bool), "stream col_part", "col_part")
    assert torch.all(cp[1] == 0).item(), "the empty range's partial row is not exactly 0"
    rc, _, Y2 = _launch_stream(L, D, seg_d, len(seg_ptr) - 1, rs_d, n_ranges, epi, prev_d, None)
    assert _eq(Y, Y2), "dZ depends on col_part being given"


def test_stream_refusals(L):
    rng = _rng("stream_refusals")
    csr = R.make_csr([1, 2, 3, 0, 4, 5, 1, 1], 8, rng, exact=True)
    seg, rs = _i32([0, 3, 8]), _i32([0, 1, 2])
    D = Data(rng, csr, 36, True, table=(8, -1))
    run = lambda D, **kw: _launch_stream(L, D, seg, 2, rs, 2, **kw)[0]   # noqa: E731
    assert run(D) == 0 and run(D, xrow="neither") == 0
    assert run(D, xrow="xrow") == E_BADARG and run(D, xrow="xcol") == E_BADARG                         # one of the two alone
    assert run(D, nnz=0) == E_BADARG
    assert run(Data(rng, csr, 7, True)) == E_BADARG
    assert run(Data(rng, csr, 36, True, off=1)) == E_ALIGN
    epi = Epi(rng, "elu", 8, 36, True, BWD_EPIS)
    assert run(D, epi=epi, prev=_offset_copy(D.prev(rng), 1)) == E_BADARG
    assert run(D, epi=types.SimpleNamespace(flags=0x10, seed=0, mask=None, bias_d=None)) == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the row-streaming kernel on a compact operand: fitgnn_spmm_rows_compact_f32 / _dz_f32
# ---------------------------------------------------------------------------------------------------------------------------------
ZF = 12   # operand rows 0 ... 11 are the selection, 12 ... 14 rows of zeros (NaN in memory)


def _compact_pattern(rng, n, exact):
    """Ranges of 32 rows with 0, 64, 65 and 200 entries, then rows that name the same operand row again and again, a zero row between
    them, a row of zero rows only; 15 operand ids, so repeats are the rule.  Other n: random rows of 0 ... 9 entries."""
    ids = np.arange(ZF + 3)
    lens = rng.integers(0, 10, size=n)
    lens[rng.random(n) < 0.2] = 0
    cols = {}
    if n == 200:
        lens[0:32] = 0
        lens[32:64] = 2
        lens[64:96] = 2
        lens[70] = 3
        lens[96:128] = [0] + [7] * 20 + [6] * 10 + [0]
        for r, c in zip(range(128, 140), [[3], [3], [3], [5], [3], [12], [3], [13, 14], [3], [12, 3], [3], [0, 3, 11, 12, 14]]):
            cols[r] = c
        lens[159], lens[160], lens[191], lens[199] = 0, 0, 0, 0                            # empty rows at the ends of ranges
    csr = R.make_csr(lens, len(ids), rng, exact=exact, cols=cols)
    if n == 200:
        e = csr[0][[0, 32, 64, 96, 128]]
        assert np.diff(e).tolist() == [0, 64, 65, 200]
    return csr


def _launch_compact(L, D, prev=None, epi=None, col_part=None, null_csr=False, **over):
    buf, Y = _out(D.n, D.H, D.ldy, D.off)
    a = dict(nnz=D.nnz, ldx=D.ldx, zero_from=D.zero_from, n=D.n, H=D.H)
    a.update(over)
    rp, xc, vl = D.csr_ptrs(L)
    if null_csr:
        xc = vl = None
    head = (rp, xc, vl, a["nnz"], _p(L, D.Xd), a["ldx"], a["zero_from"], _p(L, Y), D.ldy, a["n"], a["H"])
    if prev is None:
        rc = _call(L, "fitgnn_spmm_rows_compact_f32", *head)
    else:
        rc = _call(L, "fitgnn_spmm_rows_compact_dz_f32", *head, _p(L, prev), epi.flags, over.get("p", 0.5), epi.seed, _p(L, epi.mask), _p(L, col_part))
    return rc, buf, Y


def _parts(L, n):
    """(ranges [parts, 2], rows per range) as rows_plan cuts n rows."""
    parts = int(L.lib().fitgnn_spmm_rows_compact_parts(n))
    per = max(-(-n // 8192), 32)
    assert parts == -(-n // per)
    b = np.minimum(np.arange(parts + 1, dtype=np.int64) * per, n)
    return np.stack([b[:-1], b[1:]], 1), per


def _compact_check(L, D, rng, epi_name, what):
    """Forward, then the dz form with col_part, on one Data."""
    assert D.nnz == 0 or (D.col.min() >= 0 and D.col.max() < D.zero_from + 3)
    touched = np.ones(D.n, dtype=bool)
    rc, buf, Y = _launch_compact(L, D)
    L.check(rc, "fitgnn_spmm_rows_compact_f32")
    got = _check_out(buf, Y, D.H, 0, touched, what + ": Y")
    if D.exact:
        _same(got, D.Y, what + ": Y")
    else:
        _bounded("rows-compact", got, D.Y, D.eY, what + ": Y")
    prev = D.prev(rng)
    prev_d = _dev(prev)
    epi = Epi(rng, epi_name, D.n, D.H, D.exact, BWD_EPIS)
    ranges, _ = _parts(L, D.n)
    cp_buf, cp = _col_part(len(ranges), D.H, NAN)
    rc, buf, Z = _launch_compact(L, D, prev_d, epi, cp)
    L.check(rc, "fitgnn_spmm_rows_compact_dz_f32")
    got = _check_out(buf, Z, D.H, 0, touched, what + ": dZ")
    dZ, bound = _verify_dz(got, D, prev, epi, touched, "rows-compact dz", what + f": dZ ({epi_name})")
    _verify_col_part(cp_buf, cp, D, dZ, bound, ranges, ranges[:, 1] - ranges[:, 0] - 4, np.ones(len(ranges), dtype=bool), "rows-compact col_part",
                     what + ": col_part")
    return Y, Z


COMPACT_CASES = [(H, n, ["elu", "elu_mask", "hash", "elu_hash_ptr"][(i + j) % 4]) for i, H in enumerate(VEC4_H) for j, n in enumerate([1, 31, 32, 33, 200])]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("H,n,epi_name", COMPACT_CASES, ids=lambda v: str(v))
def test_rows_compact(L, H, n, epi_name, exact):
    rng = _rng("compact", H, n, epi_name, exact)
    D = Data(rng, _compact_pattern(rng, n, exact), H, exact, compact_zero_from=ZF)
    Y, Z = _compact_check(L, D, rng, epi_name, f"n = {n}")
    if not exact:
        assert _eq(Y, _launch_compact(L, D)[2]), "two launches on the same input differ"


@pytest.mark.parametrize("H", [4, 260])
def test_rows_compact_every_row_zero(L, H):
    """zero_from = 0: every operand row is a row of zeros (none of them may be loaded: NaN in memory)."""
    rng = _rng("compact_zero", H)
    csr = R.make_csr(rng.integers(0, 4, size=70), 3, rng, exact=True)
    D = Data(rng, csr, H, True, compact_zero_from=0)
    Y, Z = _compact_check(L, D, rng, "elu_hash", "zero_from = 0")
    assert torch.all(Y[:, :H] == 0).item() and torch.all(Z[:, :H] == 0).item()


@pytest.mark.parametrize("n", [262145, 524289])
def test_rows_compact_many_rows(L, n):
    """H = 4, three entries per row.  262 145 rows: rows_plan gives 33 rows per range (a last group of one row, ranges that start at
    any row modulo 4); 524 289 rows: 65 per range, the second row-pointer batch of a range (i >= 64)."""
    rng = _rng("compact_many", n)
    zf = 1000
    base = rng.integers(0, zf - 4, size=n)
    col = (base[:, None] + np.array([0, 3, 7])[None, :]).reshape(-1).astype(np.int32)        # ascending, up to zf + 2: some zero rows
    rowptr = (3 * np.arange(n + 1)).astype(np.int32)
    val = R.exact_values(rng, np.full(n, 3))
    D = Data(rng, (rowptr, col, val), 4, True, compact_zero_from=zf)
    assert _parts(L, n)[1] == (33 if n == 262145 else 65)
    _compact_check(L, D, rng, "elu_hash", f"n = {n}")


@pytest.mark.parametrize("null_csr", [True, False], ids=["null", "one-element"])
@pytest.mark.parametrize("H,n", [(4, 1), (36, 33), (260, 70)])
def test_rows_compact_without_entries(L, H, n, null_csr):
    """nnz == 0: no kernel runs (it would load xcol[0] / val[0]); Y's H columns exactly 0, the padding untouched, col_part exactly 0."""
    rng = _rng("compact_empty", H, n)
    D = Data(rng, (np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)), H, True, compact_zero_from=ZF)
    rc, buf, Y = _launch_compact(L, D, null_csr=null_csr)
    L.check(rc, "fitgnn_spmm_rows_compact_f32")
    got = _check_out(buf, Y, H, 0, np.ones(n, dtype=bool), "Y")
    assert np.all(got == 0)
    epi = Epi(rng, "elu_hash", n, H, True, BWD_EPIS)
    parts = len(_parts(L, n)[0])
    cp_buf, cp = _col_part(parts, H, NAN)
    rc, buf, Z = _launch_compact(L, D, _dev(D.prev(rng)), epi, cp, null_csr=null_csr)
    L.check(rc, "fitgnn_spmm_rows_compact_dz_f32")
    assert np.all(_check_out(buf, Z, H, 0, np.ones(n, dtype=bool), "dZ") == 0)
    assert torch.all(cp == 0).item() and torch.isnan(cp_buf[-GUARD:]).all().item()


def test_rows_compact_refusals(L):
    rng = _rng("compact_refusals")
    D = Data(rng, _compact_pattern(rng, 33, True), 36, True, compact_zero_from=ZF)
    prev = _dev(D.prev(rng))
    epi = Epi(rng, "elu_hash", 33, 36, True, BWD_EPIS)
    run = lambda D=D, **kw: _launch_compact(L, D, **kw)[0]   # noqa: E731
    assert run() == 0 and run(prev=prev, epi=epi) == 0
    assert run(n=-1) == E_BADARG and run(nnz=-1) == E_BADARG and run(nnz=1 << 31) == E_BADARG and run(zero_from=-1) == E_BADARG
    assert run(n=0) == 0 and run(H=0) == 0
    assert run(null_csr=True) == E_BADARG                                                               # NULL xcol / val with nnz > 0
    assert run(H=34) == E_BADARG and run(ldx=32) == E_BADARG and run(ldx=37) == E_BADARG
    assert run(Data(rng, (D.rowptr, D.col, D.val), 36, True, off=1, compact_zero_from=ZF)) == E_ALIGN
    assert run(prev=prev, epi=epi, p=1.0) == E_BADARG
    assert run(prev=_offset_copy(D.prev(rng), 1), epi=epi) == E_BADARG
    assert run(prev=prev, epi=types.SimpleNamespace(flags=sr.EPI_BIAS, seed=0, mask=None)) == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the two-hop side table: fitgnn_two_hop_rows_f32
# ---------------------------------------------------------------------------------------------------------------------------------
TWO_HOP_ROWS_CASES = [(H, ["elu", "mask", "elu_mask", "elu_hash", "elu_hash_ptr"][(i + j) % 5]) for i, H in enumerate(VEC4_H) for j in range(2)]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("H,epi_name", TWO_HOP_ROWS_CASES, ids=lambda v: str(v))
def test_two_hop_rows(L, H, epi_name, exact):
    """Rows of 0, 1, 64, 65, 200 entries of which none, some or all are loss rows (zcol < zero_from); the others carry a table row >=
    zero_from or 0x7fffffff.  Table rows in any order, with repeats; ldz > H; H = 260: the dead lanes of the second slab read the
    clamped column group of `prev` and, were they to index it, a mask.  Same bits as the rows-compact dz kernel on those rows."""
    rng = _rng("two_hop_rows", H, epi_name, exact)
    n, zf = 45, 40
    lens = R.cycle([0, 1, 64, 65, 200, 3, 5], n)
    rowptr, col, val = R.make_csr(lens, 260, rng, exact=exact)
    kind = np.repeat(np.arange(n) % 3, lens)                                                # per row: no loss column, some, all
    loss = np.where(kind == 0, False, np.where(kind == 1, rng.random(len(col)) < 0.5, True))
    other = np.where(rng.random(len(col)) < 0.5, R.NO_ROW, zf + rng.integers(0, 100, size=len(col)))
    zcol = np.where(loss, rng.integers(0, zf, size=len(col)), other).astype(np.int32)
    D = Data(rng, (rowptr, np.minimum(zcol, zf + 2).astype(np.int32), val), H, exact, compact_zero_from=zf)
    prev = D.prev(rng)
    epi = Epi(rng, epi_name, n, H, exact, BWD_EPIS)
    rows = np.concatenate([rng.permutation(n), [7, 7, 0, n - 1]])
    ldz = H + 8
    buf, ZT = _out(len(rows), H, ldz)
    rows_d, zcol_d, prev_d = _dev(rows, torch.int64), _i32(zcol), _dev(prev)
    args = (_p(L, D.rp_d), _p(L, zcol_d), _p(L, D.val_d), _p(L, D.Xd), D.ldx, zf, _p(L, rows_d), len(rows), _p(L, prev_d), H, epi.flags, 0.5,
            epi.seed, _p(L, epi.mask), _p(L, ZT), ldz)
    _run(L, "fitgnn_two_hop_rows_f32", *args)
    got = _check_out(buf, ZT, H, 0, np.ones(len(rows), dtype=bool), "ZT")
    dZ, f = R.backward(D.Y, prev, epi.flags, 0.5, epi.keep)
    if exact:
        _same(got, dZ[rows], "ZT")
    else:
        _bounded("two-hop rows", got, dZ[rows], R.dz_bound(f, D.eY, dZ)[rows], "ZT")
    rc, _, Z = _launch_compact(L, D, prev_d, epi, None)
    L.check(rc, "fitgnn_spmm_rows_compact_dz_f32")
    assert torch.equal(ZT[:, :H], Z[torch.from_numpy(rows).cuda(), :H]), "the side table and the rows-compact dz kernel differ in bits"


def test_two_hop_rows_refusals(L):
    rng = _rng("two_hop_rows_refusals")
    D = Data(rng, R.make_csr([1, 2, 3, 0], 6, rng, exact=True), 8, True, compact_zero_from=6)
    prev, rows = _dev(D.prev(rng)), _dev(np.arange(4), torch.int64)
    ZT = torch.zeros(4, 8, device="cuda")

    def run(H=8, flags=0, zf=6, ldz=8, zt=ZT, pv=prev):
        return _call(L, "fitgnn_two_hop_rows_f32", *D.csr_ptrs(L), _p(L, D.Xd), D.ldx, zf, _p(L, rows), 4, _p(L, pv), H, flags, 0.5, 0, None,
                     _p(L, zt), ldz)

    assert run() == 0
    assert run(H=6) == E_BADARG and run(zf=-1) == E_BADARG and run(ldz=4) == E_BADARG
    assert run(flags=sr.EPI_BIAS) == E_BADARG and run(flags=0x10) == E_BADARG
    assert run(zt=_offset_copy(np.zeros((4, 8), np.float32), 1)) == E_ALIGN and run(pv=_offset_copy(D.prev(rng), 1)) == E_ALIGN


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels the header calls "same bits", on one RANDOM pattern none of the planners would emit
# ---------------------------------------------------------------------------------------------------------------------------------
def _common_case(rng, H):
    n = 330
    lens = np.minimum(R.cycle(R.TILE_LENGTHS, n, start=3), n)
    lens[:256] = np.minimum(lens[:256], 24)                                                 # 64 rows per wave of the first tile: the gather kernel's general path
    D = Data(rng, R.make_csr(lens, n, rng), H, False)
    tiles = R.tile_records(D.rowptr, [(0, 256, 0, 16), None, (256, 300, 250, 40), (300, n, 300, 30)])
    blocks, long_rows = R.block_records(D.rowptr, [(200, n), None, (0, 100), (100, 200)], long_row=64)
    seg_ptr, range_seg = R.segments([20] * 16 + [10], [3, 0, 10, 4])
    return D, tiles, blocks, long_rows, seg_ptr, range_seg


@pytest.mark.parametrize("H", [36, 260])
def test_same_bits_across_kernels(L, H):
    rng = _rng("same_bits", H)
    D, tiles, blocks, long_rows, seg_ptr, range_seg = _common_case(rng, H)
    _valid_tiles(tiles, D)
    _valid_stream(D, seg_ptr, range_seg)
    tiles_d = _i32(tiles)
    outs = {}
    rc, _, outs["tile"] = _launch_tile(L, D, tiles_d, len(tiles), 0)
    L.check(rc, "tile")
    rc, _, outs["tile, window 40"] = _launch_tile(L, D, tiles_d, len(tiles), 40)
    L.check(rc, "tile, window 40")
    rc, _, g = _launch_tile(L, D, tiles_d, len(tiles), 0, gather=True)
    L.check(rc, "gather")
    rc, _, outs["blocks"] = _launch_blocks(L, D, _i32(blocks), len(blocks), _i32(long_rows))
    L.check(rc, "blocks")
    rc, _, outs["stream"] = _launch_stream(L, D, _i32(seg_ptr), len(seg_ptr) - 1, _i32(range_seg), len(range_seg) - 1, xrow="neither")
    L.check(rc, "stream")
    D.zero_from = D.n                                                                        # the plain operand as a compact one without zero rows
    rc, _, outs["rows-compact"] = _launch_compact(L, D)
    D.zero_from = -1
    L.check(rc, "rows-compact")
    ref = outs["tile"]
    assert not torch.isnan(ref[:, :H]).any().item()
    _bounded("same-bits input", _np(ref[:, :H]), D.Y, D.eY, "tile")
    for name, Y in outs.items():
        assert torch.equal(Y[:, :H], ref[:, :H]), f"{name} and the tile kernel differ in bits"
    assert torch.equal(g[:256, :H], ref[:256, :H]), "the gather kernel's general path and the tile kernel differ in bits"
    assert not torch.isnan(g[:, :H]).any().item()


@pytest.mark.parametrize("epi_name", ["elu_mask", "elu_hash"])
@pytest.mark.parametrize("H", [36, 260])
def test_same_bits_across_dz_kernels(L, H, epi_name):
    rng = _rng("same_bits_dz", H, epi_name)
    D, tiles, blocks, long_rows, seg_ptr, range_seg = _common_case(rng, H)
    prev_d = _dev(D.prev(rng))
    epi = Epi(rng, epi_name, D.n, H, False, BWD_EPIS)
    outs = {}
    rc, _, outs["tile"] = _launch_tile(L, D, _i32(tiles), len(tiles), 0, epi, prev=prev_d)
    L.check(rc, "tile")
    rc, _, outs["blocks"] = _launch_blocks(L, D, _i32(blocks), len(blocks), _i32(long_rows), epi, prev=prev_d)
    L.check(rc, "blocks")
    rc, _, outs["stream"] = _launch_stream(L, D, _i32(seg_ptr), len(seg_ptr) - 1, _i32(range_seg), len(range_seg) - 1, epi, prev_d, xrow="neither")
    L.check(rc, "stream")
    D.zero_from = D.n
    rc, _, outs["rows-compact"] = _launch_compact(L, D, prev_d, epi)
    D.zero_from = -1
    L.check(rc, "rows-compact")
    ref = outs["tile"]
    assert not torch.isnan(ref[:, :H]).any().item()
    for name, Y in outs.items():
        assert torch.equal(Y[:, :H], ref[:, :H]), f"{name} and the tile kernel differ in bits (dz form)"


# ---------------------------------------------------------------------------------------------------------------------------------
# the two-hop backward on the whole-subgraph kernel: fitgnn_spmm_two_hop_blocks_f32
# ---------------------------------------------------------------------------------------------------------------------------------
STARS = [(0, 4), (4, 45), (45, 346)]          # centre first, then its 3, 40 and 300 leaves; rows 346 ... 355 belong to no block
TWO_HOP_N = 356
LOSS_ROWS = {"centres": [45, 0, 4], "mixed": [4, 7, 30, 100, 200, 59, 346, 2], "outside": [346, 350]}


def _star_pattern(rng, exact):
    """A symmetric pattern, star by star: a self loop on every row but the 300-leaf centre, centre -- leaf, leaf -- leaf edges inside a
    piece (58, 59), across pieces (5, 30), (50, 200) and across blocks (2, 20), (10, 100), and edges to rows of no block."""
    und = {(r, r) for r in range(TWO_HOP_N) if r != 45}
    for c, e in STARS:
        und |= {(c, r) for r in range(c + 1, e)}
    und |= {(58, 59), (5, 30), (50, 200), (2, 20), (10, 100), (346, 7), (350, 345), (347, 348), (346, 30)}
    cols = {r: [] for r in range(TWO_HOP_N)}
    for a, b in und:
        cols[a].append(b)
        cols[b].append(a)
    return R.make_csr(np.zeros(TWO_HOP_N, dtype=np.int64), TWO_HOP_N, rng, exact=exact, cols=cols)


TWO_HOP_CASES = [(H, loss, ["elu_mask", "elu_hash", "mask", "elu_hash_ptr", "elu", "hash"][(i + 3 * j) % 6])
                 for i, loss in enumerate(LOSS_ROWS) for j, H in enumerate([36, 260])]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("H,loss,epi_name", TWO_HOP_CASES, ids=lambda v: str(v))
def test_two_hop_blocks(L, H, loss, epi_name, exact):
    """Y = P dZ on the blocks' rows with dZ = (P Xc_dense) . f(prev) made in the LDS windows (simple rows) or read from the side table;
    col_part: the column sums of dZ per block.  The same bits as fitgnn_spmm_rows_compact_dz_f32 followed by
    fitgnn_spmm_csr_blocks_f32."""
    from fitgnn_amd import ops

    rng = _rng("two_hop_blocks", H, loss, epi_name, exact)
    n = TWO_HOP_N
    rowptr, col, val = _star_pattern(rng, exact)
    lens = np.diff(rowptr.astype(np.int64))
    rows = np.asarray(LOSS_ROWS[loss], dtype=np.int64)
    n_sel = len(rows)
    pos = n_sel + np.arange(n) % 256
    pos[rows] = np.arange(n_sel)
    blocks, long_rows = R.block_records(rowptr, [STARS[2], None, STARS[0], STARS[1]], long_rows={0: [45], 2: [0], 3: [4]})
    dev = lambda a, dt: _dev(np.asarray(a), dt)   # noqa: E731
    side = types.SimpleNamespace(rowptr=dev(rowptr, torch.int32), col=dev(col, torch.int32), val=_dev(val), blocks=dev(blocks[[0, 2, 3]], torch.int32),
                                 long_rows=dev(long_rows, torch.int32))
    # (the index is built from the non-empty records; long_off / n_long of a record are the same in both arrays)
    g = types.SimpleNamespace(t=side, n=n)
    ix = ops._two_hop_block_index(g, dev(rows, torch.int64), dev(pos, torch.int32))
    zrow, zcol, zt_rows = (ix[k].cpu().numpy() for k in ("zrow", "zcol", "zt_rows"))
    row_p = ix["row_p"].cpu().numpy()
    in_block = _mask(n, STARS)
    assert (zrow[in_block] == -1).sum() > 250, "most leaves are simple rows: their dZ is made in the window"
    assert np.array_equal(zt_rows[:n_sel], rows) and np.all(zrow[~in_block] >= 0)
    if loss == "centres":                       # a centre that is a loss row: its leaves take its compact row from the hub slot
        assert zrow[45] == 0 and np.all(row_p[46:346] == 0) and np.all(zrow[46:346][lens[46:346] == 2] == -1)
    if loss == "mixed":                         # row 5 has the loss columns 4 and 30: its dZ is not one product, it sits in the table
        assert zrow[5] >= n_sel and zrow[58] == -1 and row_p[58] == pos[59]
    if loss == "outside":                       # (row 7 is read by row 346, a row of no block: it sits in the table)
        assert zrow[7] >= n_sel and row_p[7] == 0 and (row_p[in_block] == ops.NO_ROW).sum() > 300

    mk = (lambda s: R.exact_signal(rng, s)) if exact else (lambda s: rng.normal(size=s).astype(np.float32))
    Xc = mk((n_sel, H))
    Xdense = np.zeros((n, H))
    Xdense[rows] = Xc
    D = types.SimpleNamespace(n=n, H=H, exact=exact)
    prev = Data.prev(D, rng)
    epi = Epi(rng, epi_name, n, H, exact, BWD_EPIS)
    U1, S1 = R.spmm(rowptr, col, val, Xdense)
    dZ, f = R.backward(U1, prev, epi.flags, 0.5, epi.keep)
    dzb = R.dz_bound(f, R.row_bound(rowptr, S1), dZ)
    Y, S2 = R.spmm(rowptr, col, val, dZ)
    absP = R.spmm(rowptr, col, np.abs(val), dzb)[0]
    bound = absP + R.row_bound(rowptr, S2)

    ldx, ldz, ldy = H + 4, H + 8, H + 8
    Xc_d = _operand(Xc, ldx, 0, nan_rows=3)     # rows >= n_sel are rows of zeros: never loaded
    prev_d = _dev(prev)
    zbuf, ZT = _out(len(zt_rows), H, ldz)
    _run(L, "fitgnn_two_hop_rows_f32", _p(L, side.rowptr), _p(L, ix["zcol"]), _p(L, side.val), _p(L, Xc_d), ldx, n_sel, _p(L, ix["zt_rows"]), len(zt_rows),
         _p(L, prev_d), H, epi.flags, 0.5, epi.seed, _p(L, epi.mask), _p(L, ZT), ldz)
    zt = _check_out(zbuf, ZT, H, 0, np.ones(len(zt_rows), dtype=bool), "ZT")
    if exact:
        _same(zt, dZ[zt_rows], "ZT")
    else:
        _bounded("two-hop rows", zt, dZ[zt_rows], dzb[zt_rows], "ZT")
    blocks_d = _i32(blocks)
    ybuf, Yd = _out(n, H, ldy)
    cp_buf, cp = _col_part(len(blocks), H, 0.0)
    _run(L, "fitgnn_spmm_two_hop_blocks_f32", _p(L, side.rowptr), _p(L, side.col), _p(L, side.val), _p(L, ZT), ldz, _p(L, Yd), ldy, n, H, _p(L, blocks_d),
         len(blocks), _p(L, side.long_rows), _p(L, ix["zrow"]), _p(L, ix["zcol"]), _p(L, prev_d), _p(L, Xc_d), ldx, n_sel, _p(L, ix["row_p"]),
         _p(L, ix["row_w"]), epi.flags, 0.5, epi.seed, _p(L, epi.mask), _p(L, cp))
    got = _check_out(ybuf, Yd, H, 0, in_block, "Y")            # the rows outside the blocks: still NaN
    if exact:
        # a term val[e] dZ[col[e]] is a multiple of 2^-(log2 1/|val| + 6 + ceil(log2 len(col[e]))); exact in any order while the sum of
        # the magnitudes, in that unit, stays below 2^24
        qe = np.log2(1.0 / np.abs(val.astype(np.float64))) + 6 + np.ceil(np.log2(np.maximum(lens[col], 1)))
        Q = np.array([qe[rowptr[r]:rowptr[r + 1]].max() if lens[r] else 0.0 for r in range(n)])
        sure = (S2 * 2.0 ** Q[:, None] < 2.0 ** 24)[in_block]
        assert sure.mean() > 0.95
        _same(got[sure], Y[in_block][sure], "Y")
        _within(got[~sure], Y[in_block][~sure], bound[in_block][~sure], "Y (the terms of the 300-leaf centre)")
    else:
        _bounded("two-hop blocks", got, Y[in_block], bound[in_block], "Y")
    D.lens = lens
    pieces = -(-(blocks[:, 1] - blocks[:, 0]) // 16)
    _verify_col_part(cp_buf, cp, D, dZ, dzb, blocks[:, :2], 4 * pieces, blocks[:, 1] > blocks[:, 0], "two-hop col_part", "col_part")
    # the same bits as the two launches it replaces
    xcol_d = _i32(pos[col])
    Dc = types.SimpleNamespace(n=n, H=H, ldx=ldx, ldy=ldy, off=0, nnz=len(col), zero_from=n_sel, Xd=Xc_d,
                               csr_ptrs=lambda L: (_p(L, side.rowptr), _p(L, xcol_d), _p(L, side.val)))
    rc, _, Zfull = _launch_compact(L, Dc, prev_d, epi, None)
    L.check(rc, "fitgnn_spmm_rows_compact_dz_f32")
    Zc = Zfull[:, :H].contiguous()
    assert torch.equal(ZT[:, :H], Zc[ix["zt_rows"]]), "the side table and the rows-compact dz kernel differ in bits"
    Y2 = torch.full((n, H), NAN, device="cuda")
    _run(L, "fitgnn_spmm_csr_blocks_f32", _p(L, side.rowptr), _p(L, side.col), _p(L, side.val), _p(L, Zc), H, _p(L, Y2), H, n, H, _p(L, blocks_d),
         len(blocks), _p(L, side.long_rows), None, None, -1, None, 0, 0.0, 0, None)
    m = torch.from_numpy(in_block).cuda()
    assert torch.equal(Yd[m][:, :H], Y2[m]), "the two-hop launch and rows-compact-dz followed by blocks differ in bits"


def test_two_hop_blocks_refusals(L):
    z = [None] * 3
    f = lambda **kw: _call(L, "fitgnn_spmm_two_hop_blocks_f32", *z, None, 512, None, 512, kw.get("n", 8), kw.get("H", 512), None, kw.get("nb", 1), None,   # noqa: E731
                           None, None, None, None, 512, kw.get("zf", 0), None, None, 0, 0.0, 0, None, None)
    assert f(nb=0) == 0 and f(n=0) == 0 and f() == E_BADARG and f(zf=-1) == E_BADARG and f(n=-1) == E_BADARG
