"""Direct parity tests of the uncoded single-vector products of vexcl_amd/csrc/spmv.hip -- `csr_stream_kernel`, `csr_stream2_kernel`,
`csr_scalar_kernel`, `hell_kernel`, `sell_kernel`, `sell_pair_kernel` --, of the fills that feed them (`hell_analyze` / `hell_fill` in
misc.hip, `sell_fill_kernel`) and of the builders of their traversals (`build_order`, `vexhip_csr_traversal_i32`), through the C ABI
(`vexcl_amd.lib()`, `vexcl_amd._capi`) with torch tensors as device buffers.

What runs where
  * test_csr_*: `vexhip_spmv_csr_f64_i32`, `_f32_i32`, `_f64_i64` and the two `_ordered_` entries under the variant words 0..7 (second and
    first form, non-temporal loads, XCD swizzle), with col / val views off a 16-byte boundary (the scalar kernel), with a NULL traversal
    and three hand-made ones in units of 256-row blocks, on 1 .. 8 * 256 + 1 rows with empty rows and blocks, a row of 4500 entries,
    rows that span exactly one LDS tile, and ptr[0] = 0, 1, 2, 3, 4, 7.
  * test_hell_analyze_and_fill_*, test_hell_width_rule_edges: `vexhip_hell_analyze_i32` and `vexhip_hell_fill_*` against
    `oracle.hell_width` / `oracle.hell_build`, array for array, into buffers of exactly the size the header states, between guards.
  * test_hell_products_*: `vexhip_spmv_hell_*` under the variant words 0..15, ELL widths 1..9 and 12, with a tail, without one, tail only,
    the empty part, an odd pitch and unaligned ELL arrays; `vexhip_spmv_hell_ordered_*` with hand-made traversals of 512-row blocks.
  * test_sell_*: `vexhip_sell_bytes`, `vexhip_sell_fill_*` against `oracle.sell_pair_slots` for every row of every slice, and
    `vexhip_spmv_sell_*`: the pair kernel, `sell_kernel<W>` (under `vexhip_spmv_sell8_set_variant(1)`), the looping kernel.
  * test_order_builders_*: the smallest banded matrix for which the builders return a traversal, and four that they must decline.
  * test_generators_references_and_host_restatements (no GPU): pins everything the GPU tests take for granted.
The module has no `pytestmark`: the last test has to run without a GPU, so every GPU test carries the `gpu` mark itself.

Why the comparisons are exact
  spmv.hip is compiled with -ffp-contract=off and folds a row in storage order -- the ELL part in CSR order, then the CSR tail -- as
  `oracle.spmv_csr` does; padding adds +0 to a sum that started at +0.  Every y is therefore compared with `np.array_equal` against the
  oracle in the matrix's own type.  No tolerance in those comparisons.

The independent check
  The oracle shares its summation order with the kernels, so every result is also held against products and row sums in np.longdouble
  (fp64) / float64 (fp32): |y - y_hp| <= g (|alpha| sum_j |a_ij x_j| + |y0_i|), g = (L+2)u / (1 - (L+2)u), L the row length, u = 2^-53 /
  2^-24: the standard bound of a recursive sum of L rounded products followed by one scaling and one addition.  Derived, not measured.

Canaries
  x is a view at an odd element offset of a larger tensor, surrounded by NaN; every element of x that no entry references is NaN (the last
  column of every matrix is such an element).  y is a view with 64 sentinel elements on either side, compared as bytes after every call;
  before a `=` call y itself holds the sentinel, so a row block that no workgroup visits shows.  col / val carry slack entries in front
  of ptr[0] and behind ptr[n] (the staged CSR kernels read from ptr[0] & ~3, the first form multiplies what it reads there): the slack
  columns point at the NaN last element of x, the slack values are NaN.  All of these addresses lie inside live allocations.

Traversals
  No product is launched with a traversal that was not checked on the host first (`visit_once`): every block of [0, nb) exactly once,
  every other entry -1.  The hand-made ones are arithmetic strips with a ragged last plane and a ragged last tile, the blocks in reverse
  as an explicit map, and a map of 2 nb + 3 entries with a -1 hole in every other place.

Variant words are set inside `try` and put back in `finally`: -1 for the CSR and HELL words, 0 for the SELL word (their defaults)."""
import contextlib
import ctypes
from fractions import Fraction

import numpy as np
import pytest

gpu = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
HP = {np.float64: np.longdouble, np.float32: np.float64}          # the type of the independent reference
UNIT = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
MODES = ((1.0, False), (-0.75, True))                             # (alpha, append)
GUARD = 64                                                        # sentinel elements on either side of every y and every filled buffer
SENTINEL = 12345.0
SLACK = 8                                                         # col / val entries behind ptr[n]

CSR_BLOCK, CSR_TILE, SLICE = 256, 2048, 512
CSR_SIZES = (1, 2, 255, 256, 257, 3 * 256 + 77, 8 * 256 + 1)      # 8 * 256 + 1: 9 blocks, the swizzled grid of 16 has blocks >= nb
CSR_STRUCTURES = ("ragged", "no_entries", "long_row", "tile_edges")
CSR_LEADS = (0, 1, 2, 3, 4, 7)                                    # ptr[0]
CSR_WORDS = tuple(range(8))                                       # bit 0 non-temporal, bit 1 swizzle, bit 2 the first form
CSR_WORDS_OFFSET = (0, 4, 7)                                      # at ptr[0] != 0: both forms, and the first form with both bits
LONG_ROW = 4500                                                   # more than two LDS tiles of 2048 entries

ROW_SIZES = (1, 2, 3, 511, 512, 513, 1023, 3 * 512 + 77)
ELL_WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12)                      # 1..8 unrolled; 9 and 12 take the loop
HELL_WORDS = tuple(range(16))                                     # bit 0 non-temporal, bit 1 swizzle, bits 2..3 rows per lane 1 / 2 / 4 / "3 -> 4"
HELL_WORDS_FALLBACK = (0, 7, 11, 15)                              # odd pitch / unaligned arrays: every rows-per-lane word must fall back to 1
UNUSED_EVERY, UNUSED_AT = 11, 5                                   # no entry in a column c with c % 11 == 5: x is NaN there

ORDER_FAR = 131072                                                # 2 * 65536, a multiple of 512
ORDER_N = 4 * ORDER_FAR + 513                                     # above 8 * 65536; ragged last plane and last tile
ORDER_DIAGONALS = (-ORDER_FAR, -512, 0, ORDER_FAR)
ORDER_MODES = (0, 1, 2, 101, 107)

every_dtype = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)


# ---------------------------------------------------------------------------------------------------------------------------
# matrices: CSR with ptr[0] = 0, values kept in float64 and rounded to the type under test; the last column is never used
# ---------------------------------------------------------------------------------------------------------------------------
class Mat:
    def __init__(self, name, n, m, ptr, col, val):
        self.name, self.n, self.m = name, int(n), int(m)
        self.ptr = np.ascontiguousarray(ptr, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        self.lens = np.diff(self.ptr.astype(np.int64))
        self.rows = np.repeat(np.arange(self.n, dtype=np.int64), self.lens)
        self.pos = np.arange(len(self.col), dtype=np.int64) - np.repeat(self.ptr[:-1].astype(np.int64), self.lens)
        self._csr = {}

    def csr(self, dtype):
        key = np.dtype(dtype).name
        if key not in self._csr:
            self._csr[key] = (self.ptr, self.col, np.ascontiguousarray(self.val.astype(dtype)))
        return self._csr[key]


def _uniform(oracle, seed, count):
    return oracle.random_f64(seed, max(1, count))[:count] - 0.5


def _from_lens(oracle, name, n, m, lens, col_of, seed):
    """Rows of the given lengths; col_of(rows, pos) gives the column of entry `pos` of row `rows`; columns sorted inside a row."""
    lens = np.asarray(lens, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    pos = np.arange(ptr[-1], dtype=np.int64) - np.repeat(ptr[:-1], lens)
    col = col_of(rows, pos)
    col = col[np.lexsort((col, rows))]
    return Mat(name, n, m, ptr, col, _uniform(oracle, seed, len(col)))


_MATS = {}


def _cached(name, make):
    if name not in _MATS:
        _MATS[name] = make()
        assert _MATS[name].name == name
    return _MATS[name]


def csr_matrix(oracle, n, structure):
    """ragged: 0..5 entries a row, first and last row empty, rows 256..511 empty where they exist (n = 257: its one-row second block);
    no_entries; long_row: one row of 4500 entries among rows of 1 or 2; tile_edges: rows 0 and 1 hold 2048 entries each -- with ptr[0]
    a multiple of 4 they begin and end exactly on a tile boundary --, the others 1 or 0."""
    name = "csr_%s_n%d" % (structure, n)

    def make():
        i = np.arange(n, dtype=np.int64)
        if structure == "no_entries":
            return _from_lens(oracle, name, n, 9, np.zeros(n), lambda r, p: r, 500 + n)
        if structure == "ragged":
            mm = max(n, 8)
            lens = (oracle.random_f64(510 + n, n) * 6).astype(np.int64)
            if n == 1:
                lens[:] = 3
            elif n == 2:
                lens[:] = (0, 2)
            else:
                lens[0] = lens[-1] = 0
                lens[CSR_BLOCK:2 * CSR_BLOCK] = 0
            return _from_lens(oracle, name, n, mm + 1, lens, lambda r, p: (r * 7 + p * 13) % mm, 520 + n)
        if structure == "long_row":
            mm, at = LONG_ROW + 100, min(n - 1, 100)
            lens = 1 + (i % 3 == 0)
            lens[at] = LONG_ROW
            return _from_lens(oracle, name, n, mm + 1, lens, lambda r, p: np.where(r == at, p + 50, (r * 7 + p * 13) % mm), 530 + n)
        assert structure == "tile_edges"
        mm = CSR_TILE + 52
        lens = np.where(i % 5 == 0, 0, 1)
        lens[:2] = CSR_TILE
        return _from_lens(oracle, name, n, mm + 1, lens, lambda r, p: np.where(r < 2, p + r, (r * 7) % mm), 540 + n)
    return _cached(name, make)


def holes(oracle, n, w):
    """n x (n + w + 2) band of the w + 2 diagonals 0 .. w + 1, each entry kept with probability 0.85, none in a column c with c % 11 == 5
    (x is NaN there, next to columns that are read).  Row 0 keeps every entry -- with a forced ELL width w it has a tail --, the last row
    of n > 1 loses its first three: padding.  Adjacent rows read adjacent columns, so the SELL fill finds pairs."""
    name = "holes_n%d_w%d" % (n, w)

    def make():
        nd = w + 2
        keep = oracle.random_f64(600 + 13 * w + n % 97, n * nd).reshape(n, nd) < 0.85
        keep[0] = True
        if n > 1:
            keep[-1, :3] = False
        cols = np.arange(n, dtype=np.int64)[:, None] + np.arange(nd)[None, :]
        keep &= cols % UNUSED_EVERY != UNUSED_AT
        ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
        return Mat(name, n, n + nd, ptr, cols[keep], _uniform(oracle, 700 + 13 * w + n % 97, int(keep.sum())))
    return _cached(name, make)


def truncated(mat, w):
    """The first w entries of every row: the ELL part alone, a matrix without a tail."""
    name = mat.name + "_first%d" % w

    def make():
        keep = mat.pos < w
        return Mat(name, mat.n, mat.m, np.concatenate([[0], np.cumsum(np.minimum(mat.lens, w))]), mat.col[keep], mat.val[keep])
    return _cached(name, make)


def equal_rows(oracle, n, w):
    """Every row holds w entries: the width rule gives w and no tail."""
    name = "equal_n%d_w%d" % (n, w)
    return _cached(name, lambda: _from_lens(oracle, name, n, n + w + 1, np.full(n, w), lambda r, p: r + p, 800 + n + w))


def pad_edges(oracle):
    """Five rows, ELL width 2, columns 0..9 (largest ELL column 9).  Row 1 holds column 0 alone in its ELL column (row 0 is on another
    diagonal): a 16-byte load for the empty half would start at x[-1]: code -2.  Row 2 holds column 9 alone in its ELL column: the load
    would end at x[10]: -2 in row 3.  The other two empty halves may be loaded: -1.  Row 4 has no partner (n is odd): row 5 is -1."""
    name = "pad_edges"
    rows = ((3,), (0,), (9,), (5,), (6, 7))
    lens = [len(r) for r in rows]
    col = np.concatenate([np.array(r) for r in rows])
    return _cached(name, lambda: Mat(name, 5, 11, np.concatenate([[0], np.cumsum(lens)]), col, _uniform(oracle, 810, len(col))))


def unpaired(oracle):
    """513 rows of two entries, even rows on the diagonals 0 and 5, odd rows on 2 and 9: no diagonal is shared, the merged list of a row
    pair is longer than the width 2, the fill keeps the plain packing, and no lane of any wave has two adjacent columns in an ELL column:
    the `ballot == 0` branch of sell_pair_kernel."""
    name = "unpaired"
    n = SLICE + 1
    return _cached(name, lambda: _from_lens(oracle, name, n, n + 10, np.full(n, 2),
                                            lambda r, p: r + np.where(r % 2 == 0, 5 * p, 2 + 7 * p), 820))


def diagonal_matrix(oracle, name, n, diagonals, keep=None):
    """Constant value per diagonal; keep: which rows hold the first and the last diagonal (default: all that reach a column)."""
    def make():
        d = np.asarray(diagonals, dtype=np.int64)
        cols = np.arange(n, dtype=np.int64)[:, None] + d[None, :]
        ok = (cols >= 0) & (cols < n)
        if keep is not None:
            ok[:, 0] &= keep
            ok[:, -1] &= keep
        vals = np.broadcast_to(_uniform(oracle, 900 + len(d), len(d))[None, :], ok.shape)
        return Mat(name, n, n + 1, np.concatenate([[0], np.cumsum(ok.sum(axis=1))]), cols[ok], vals[ok])
    return _cached(name, make)


def order_matrix(oracle):
    return diagonal_matrix(oracle, "order_positive", ORDER_N, ORDER_DIAGONALS)


def order_negatives(oracle):
    """(matrix, why the builders decline it)."""
    n = ORDER_N
    return (
        (diagonal_matrix(oracle, "order_small", 8 * 65536 - 1, ORDER_DIAGONALS), "n below 8 * 65536"),
        (diagonal_matrix(oracle, "order_misaligned", n, (-ORDER_FAR - 256, -512, 0, ORDER_FAR + 256)), "far diagonal no multiple of 512"),
        (diagonal_matrix(oracle, "order_sparse_far", n, ORDER_DIAGONALS, keep=np.arange(n) % 3 == 0), "far diagonal in a third of the rows"),
    )


# ---------------------------------------------------------------------------------------------------------------------------
# host restatements: width rule, storages, traversals
# ---------------------------------------------------------------------------------------------------------------------------
def host_width(lens):
    """hybrid_ell.inl:103-110: the smallest w below the largest row length with 3 * #(rows wider than w) < n, else that length."""
    lens = np.sort(np.asarray(lens, dtype=np.int64))
    n, maxw = len(lens), int(lens[-1]) if len(lens) else 0
    for w in np.unique(np.concatenate([[0], lens])):              # the count of wider rows changes only at a length some row has
        if w < maxw and 3 * (n - np.searchsorted(lens, w, side="right")) < n:
            return int(w)
    return maxw


def width_edges():
    """name -> row lengths.  The library counts lengths in a histogram whose last bucket, 4096, collects every longer row."""
    return {
        "all_equal": [5] * 100,
        "third_wider": [7] * 33 + [4] * 66,                       # 3 * 33 < 99 fails: width 7
        "under_a_third_wider": [7] * 32 + [4] * 67,               # 3 * 32 < 99: width 4
        "one_row": [3],
        "rows_5000_6000_7000": [5000, 6000, 7000],
        "two_4096_one_4097": [10, 4096, 4097, 4096, 20],
        "ties_above_4096": [4100, 5000, 30, 4200, 6000, 5000, 4300, 2, 1],
    }


WIDTH_EDGE_RESULTS = {"all_equal": 5, "third_wider": 7, "under_a_third_wider": 4, "one_row": 3, "rows_5000_6000_7000": 7000,
                      "two_4096_one_4097": 4096, "ties_above_4096": 5000}


def ell_split(mat, w):
    """(entries of the ELL part, largest ELL column or -1, tail entries) for a forced ELL width w."""
    ell = mat.pos < w
    return ell, (int(mat.col[ell].max()) if ell.any() else -1), int((~ell).sum())


_SELL = {}


def sell_expected(oracle, mat, w):
    """Columns (ns, w, 512) with the padding codes -1 / -2, and the CSR entry behind every slot (-1: padding), from
    `oracle.sell_pair_slots` for every row pair of every slice."""
    key = (mat.name.split("_first")[0], w)                         # (a truncated matrix has the same ELL part)
    if key not in _SELL:
        ns = (mat.n + SLICE - 1) // SLICE
        cols, ent = np.full((ns, w, SLICE), -1, dtype=np.int32), np.full((ns, w, SLICE), -1, dtype=np.int64)
        max_col = ell_split(mat, w)[1]
        for row0 in range(0, mat.n, 2):
            out = oracle.sell_pair_slots(mat.ptr, mat.col, row0, w, max_col)
            for q in (0, 1):
                for j, e in enumerate(out[q]):
                    if e == "unsafe":
                        cols[row0 // SLICE, j, row0 % SLICE + q] = -2
                    elif e != "safe":
                        cols[row0 // SLICE, j, row0 % SLICE + q], ent[row0 // SLICE, j, row0 % SLICE + q] = mat.col[e], e
        _SELL[key] = (cols, ent)
    return _SELL[key]


def sell_buffer(oracle, mat, w, dtype):
    """The bytes of the SELL-512 buffer: per slice its w * 512 columns, then its w * 512 values."""
    cols, ent = sell_expected(oracle, mat, w)
    val = mat.csr(dtype)[2]
    vals = np.where(ent >= 0, val[np.maximum(ent, 0)] if len(val) else dtype(0), dtype(0)).astype(dtype)
    return b"".join(cols[s].tobytes() + vals[s].tobytes() for s in range(cols.shape[0]))


def strip_visits(grid, chunk, planes, plane_blocks, nb):
    """The block of every workgroup of a strip traversal, -1 where the workgroup returns (traversal.hpp traversal_slice restated)."""
    b = np.arange(grid, dtype=np.int64)
    k, q = b & 7, b >> 3
    r, i = q // chunk, q % chunk
    tile, p = r // planes, r % planes
    l = tile * (8 * chunk) + k * chunk + i
    lb = p * plane_blocks + l
    return np.where((l < plane_blocks) & (lb < nb), lb, -1)


def strip_geometry(nb):
    """(grid_blocks, chunk, planes, plane_blocks) of hand-made strips over nb blocks whose last plane and last tile are ragged where nb
    allows it: three planes of one- or two-block strips, from 8 blocks on two planes of strips of two blocks."""
    planes = 2 if nb >= 8 else 3 if nb >= 3 else 1
    plane_blocks = (nb + planes - 1) // planes
    chunk = 2 if plane_blocks >= 4 else 1
    tiles = (plane_blocks + 8 * chunk - 1) // (8 * chunk)
    return tiles * planes * 8 * chunk, chunk, planes, plane_blocks


def holey_map(nb):
    """2 nb + 3 workgroups for nb blocks: the blocks in reverse at the odd places, -1 everywhere else."""
    m = np.full(2 * nb + 3, -1, dtype=np.int32)
    m[1:2 * nb:2] = np.arange(nb - 1, -1, -1)
    return m


def visit_once(visited, nb):
    """Every block of [0, nb) exactly once, every other entry -1, nothing >= nb: what a traversal must satisfy before a launch."""
    visited = np.asarray(visited, dtype=np.int64)
    real = visited[visited >= 0]
    return bool(len(real) == nb and np.array_equal(np.sort(real), np.arange(nb)) and np.all(visited[visited < 0] == -1)
                and len(visited) < 2 ** 31)


def builder_strips(n, rows_per_block, far, forced_chunk=None):
    """What the header promises for a banded matrix whose far diagonal is `far`: planes of far / rows_per_block blocks, every XCD a strip
    of an eighth of a plane but at most 32 Ki rows, tiles of 8 strips, plane after plane."""
    plane_blocks = far // rows_per_block
    nb = (n + rows_per_block - 1) // rows_per_block
    chunk = forced_chunk or max(1, min(32768 // rows_per_block, plane_blocks // 8))
    planes = (nb + plane_blocks - 1) // plane_blocks
    tiles = (plane_blocks + 8 * chunk - 1) // (8 * chunk)
    return tiles * planes * 8 * chunk, chunk, planes, plane_blocks


def builder_map_blocks(n, mode):
    """grid_blocks of the two explicit maps over 512-row blocks: mode 1 deals an eighth of the blocks to every XCD (8 * ceil(nb / 8)
    places); mode 2 walks tiles of 64 Ki rows = 128 blocks, plane after plane (tiles * planes * 128 places)."""
    nb, plane_blocks = (n + SLICE - 1) // SLICE, ORDER_FAR // SLICE
    if mode == 1:
        return 8 * ((nb + 7) // 8)
    return ((plane_blocks + 127) // 128) * ((nb + plane_blocks - 1) // plane_blocks) * 128


# ---------------------------------------------------------------------------------------------------------------------------
# right-hand side, start vector and references of one matrix in one type, computed once and shared by every test
# ---------------------------------------------------------------------------------------------------------------------------
def segment_sums(a, ptr):
    """Row sums of the entries a; an empty row sums to 0 (np.add.reduceat alone would return the NEXT row's first entry)."""
    lens = np.diff(ptr.astype(np.int64))
    out = np.zeros(len(lens), dtype=a.dtype)
    full = lens > 0
    if full.any():
        out[full] = np.add.reduceat(a, ptr[:-1].astype(np.int64)[full])
    return out


class Case:
    def __init__(self, oracle, mat, dtype):
        self.mat, self.dtype = mat, dtype
        ptr, col, val = mat.csr(dtype)
        used = np.zeros(mat.m, dtype=bool)
        used[col] = True
        assert not used[-1]                                           # the slack columns point here
        seed = 1000 + 17 * mat.n + 3 * mat.m + len(mat.col) % 1000
        self.x = _uniform(oracle, seed, mat.m).astype(dtype)
        self.x[~used] = np.nan                                        # no entry reads these
        self.y0 = _uniform(oracle, seed + 50, mat.n).astype(dtype)
        hp = HP[dtype]
        prod = val.astype(hp) * self.x.astype(hp)[col]
        self.sum, self.abs_sum = segment_sums(prod, ptr), segment_sums(np.abs(prod), ptr)
        lu = (mat.lens + 2).astype(hp) * hp(UNIT[dtype])
        self.gamma = lu / (1 - lu)
        self._ref = {}

    def reference(self, oracle, mode):
        """oracle.spmv_csr in the matrix's own type.  `=` starts from the sentinel: every row must be written."""
        if mode not in self._ref:
            alpha, append = mode
            ptr, col, val = self.mat.csr(self.dtype)
            y = self.y0.copy() if append else np.full(self.mat.n, SENTINEL, dtype=self.dtype)
            self._ref[mode] = oracle.spmv_csr(ptr, col, val, self.x, y, alpha, append)
        return self._ref[mode]

    def high_precision(self, mode):
        """(y_hp, bound): products and row sums in HP, and g (|alpha| sum |a x| + |y0|)."""
        alpha, append = mode
        hp = HP[self.dtype]
        y, scale = hp(alpha) * self.sum, hp(abs(alpha)) * self.abs_sum
        if append:
            y, scale = y + self.y0.astype(hp), scale + np.abs(self.y0.astype(hp))
        return y, self.gamma * scale

    def within_bound(self, y, mode):
        y_hp, bound = self.high_precision(mode)
        return bool(np.all(np.abs(y.astype(HP[self.dtype]) - y_hp) <= bound))


_CASES = {}


def case_of(oracle, mat, dtype):
    key = (mat.name, np.dtype(dtype).name)
    if key not in _CASES:
        _CASES[key] = Case(oracle, mat, dtype)
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------------------
# the CPU test
# ---------------------------------------------------------------------------------------------------------------------------
def _exact(v):
    """A float32 / float64 / longdouble scalar as a Fraction (a longdouble is the sum of two doubles)."""
    hi = float(v)
    return Fraction(hi) + Fraction(float(v - type(v)(hi)))


def _check_structure(mat):
    assert mat.ptr[0] == 0 and mat.ptr[-1] == len(mat.col) == len(mat.val) and np.all(mat.lens >= 0), mat.name
    assert len(mat.col) == 0 or (mat.col.min() >= 0 and mat.col.max() < mat.m - 1), mat.name         # the last column stays unused
    inner = mat.pos > 0
    assert np.all(np.diff(mat.col.astype(np.int64))[inner[1:]] > 0), mat.name + ": columns do not ascend inside a row"
    assert np.all(np.abs(mat.val) <= 0.5) and np.all(mat.val != 0), mat.name


def all_block_counts():
    csr = {(n + CSR_BLOCK - 1) // CSR_BLOCK for n in CSR_SIZES}
    rows = {(n + SLICE - 1) // SLICE for n in ROW_SIZES + (5, SLICE + 1)}
    return sorted(csr | rows)


def test_generators_references_and_host_restatements(oracle):
    """Without a GPU: every generated matrix has the promised structure; y_hp equals a plain loop in exact rational arithmetic on the
    two smallest matrices; `oracle.spmv_csr` lies within the derived bound on every matrix of the file, in both types; the width rule,
    the strip geometry and every hand-made traversal are what the GPU tests assume; and the parametrisations have the stated sizes."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no wider than double here: no independent fp64 reference"
    # how much the GPU tests cover
    assert (len(CSR_SIZES), len(CSR_STRUCTURES), len(CSR_LEADS), len(CSR_WORDS)) == (7, 4, 6, 8) and set(CSR_WORDS_OFFSET) <= set(CSR_WORDS)
    assert {w & 4 for w in CSR_WORDS_OFFSET} == {0, 4} and {(n + 255) // 256 for n in CSR_SIZES} == {1, 2, 4, 9}
    assert (len(ROW_SIZES), len(ELL_WIDTHS), len(HELL_WORDS)) == (8, 10, 16) and {w > 8 for w in ELL_WIDTHS} == {False, True}
    assert {(w >> 2) & 3 for w in HELL_WORDS_FALLBACK} == {0, 1, 2, 3} and set(range(1, 9)) <= set(ELL_WIDTHS)
    assert len(DTYPES) == 2 and len(MODES) == 2 and len(ORDER_MODES) == 5 and len(width_edges()) == 7 == len(WIDTH_EDGE_RESULTS)

    mats = {}
    for n in CSR_SIZES:
        for structure in CSR_STRUCTURES:
            A = mats.setdefault("csr_%s_n%d" % (structure, n), csr_matrix(oracle, n, structure))
            assert A.n == n and len(A.col) <= 8000, A.name
        A = csr_matrix(oracle, n, "ragged")
        assert len(A.col) > 0 and A.lens.max() <= 5 and (n <= 2 or (A.lens[0] == 0 and A.lens[-1] == 0))
        assert n <= CSR_BLOCK or np.all(A.lens[CSR_BLOCK:2 * CSR_BLOCK] == 0)
        assert n < 2 * CSR_BLOCK or (A.lens[2 * CSR_BLOCK:].max() == 5 and np.any(A.lens[1:CSR_BLOCK] == 0))
        assert len(csr_matrix(oracle, n, "no_entries").col) == 0
        A = csr_matrix(oracle, n, "long_row")
        assert A.lens.max() == LONG_ROW > 2 * CSR_TILE and np.count_nonzero(A.lens > 2) == 1
        A = csr_matrix(oracle, n, "tile_edges")
        assert A.ptr[1] == CSR_TILE and (n == 1 or A.ptr[2] == 2 * CSR_TILE) and (n <= 2 or A.lens[2:].max() <= 1)
    for n in ROW_SIZES:
        for w in ELL_WIDTHS:
            A = mats.setdefault("holes_n%d_w%d" % (n, w), holes(oracle, n, w))
            T = mats.setdefault(A.name + "_first%d" % w, truncated(A, w))
            ell, max_col, tail = ell_split(A, w)
            assert tail > 0 and A.lens[0] > w and A.lens.max() <= w + 2, (A.name, tail)
            assert n < 511 or (np.count_nonzero(A.lens < w) > (10 if w > 2 else 0) and np.count_nonzero(A.lens > w) > 10), A.name
            assert T.lens.max() == w and np.array_equal(T.col, A.col[ell]) and ell_split(T, w)[2] == 0
            used = np.bincount(A.col, minlength=A.m) > 0
            assert not used[UNUSED_AT::UNUSED_EVERY].any() and not used[-1]
    A = mats.setdefault("pad_edges", pad_edges(oracle))
    cols, ent = sell_expected(oracle, A, 2)
    assert cols.shape == (1, 2, SLICE) and ell_split(A, 2)[1:] == (9, 0)
    assert cols[0, :, :6].T.tolist() == [[-2, 3], [0, -1], [-1, 9], [5, -2], [6, 7], [-1, -1]] and np.all(cols[0, :, 6:] == -1), cols[0, :, :6].T
    A = mats.setdefault("unpaired", unpaired(oracle))
    cols, ent = sell_expected(oracle, A, 2)
    c0, c1 = cols[0, :, 0::2].astype(np.int64), cols[0, :, 1::2].astype(np.int64)
    assert np.all(c0 >= 0) and np.all(c1 >= 0) and not np.any(c1 == c0 + 1)       # both halves real, never adjacent: no 16-byte load
    assert cols[1, :, 0].tolist() == [SLICE, SLICE + 5] and np.all(cols[1, :, 1] < 0)
    for n, w in ((100, 5), (1613, 9)):
        A = mats.setdefault("equal_n%d_w%d" % (n, w), equal_rows(oracle, n, w))
        assert host_width(A.lens) == w
    for A in mats.values():
        _check_structure(A)
    big = [order_matrix(oracle)] + [A for A, _ in order_negatives(oracle)]
    for A in big:
        _check_structure(A)
        assert host_width(A.lens) == oracle.hell_width(A.ptr) == (2 if A is big[3] else 4) and A.lens.max() == 4, A.name
    A = big[0]
    assert 1.8e6 < len(A.col) < 2.1e6
    far = A.col.astype(np.int64) - A.rows
    assert A.n == ORDER_N >= 8 * 65536 and ORDER_FAR == 2 * 65536 and ORDER_FAR % SLICE == 0 and set(np.unique(far)) == set(ORDER_DIAGONALS)
    assert 2 * np.count_nonzero(far == -ORDER_FAR) >= A.n and big[1].n < 8 * 65536 and (ORDER_FAR + 256) % SLICE != 0
    assert set(np.unique(big[2].col.astype(np.int64) - big[2].rows)) == {-ORDER_FAR - 256, -512, 0, ORDER_FAR + 256}
    assert all(2 * np.count_nonzero(big[3].col.astype(np.int64) - big[3].rows == d) < big[3].n for d in (-ORDER_FAR, ORDER_FAR))

    # the width rule
    for name, lens in width_edges().items():
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        assert host_width(lens) == oracle.hell_width(ptr) == WIDTH_EDGE_RESULTS[name], (name, host_width(lens), oracle.hell_width(ptr))
    for A in mats.values():
        assert host_width(A.lens) == oracle.hell_width(A.ptr), A.name

    # traversals: the hand-made ones visit every block once and have live guards; the builders' strips as restated
    for nb in all_block_counts():
        grid, chunk, planes, plane_blocks = strip_geometry(nb)
        visited = strip_visits(grid, chunk, planes, plane_blocks, nb)
        assert visit_once(visited, nb) and np.any(visited < 0) and grid % 8 == 0, nb
        assert visit_once(np.arange(nb - 1, -1, -1), nb) and visit_once(holey_map(nb), nb) and len(holey_map(nb)) > nb
    assert all_block_counts() == [1, 2, 4, 9] and strip_geometry(9) == (32, 2, 2, 5) and strip_geometry(4) == (24, 1, 3, 2)
    assert not visit_once([0, 1, 1], 3) and not visit_once([0, 2, -1], 3) and not visit_once([0, 1, 2, 3], 3) and not visit_once([0, 1, 2, -2], 3)
    assert builder_strips(ORDER_N, SLICE, ORDER_FAR) == (1280, 32, 5, 256)
    assert builder_strips(ORDER_N, SLICE, ORDER_FAR, 1) == (1280, 1, 5, 256)
    assert builder_strips(ORDER_N, SLICE, ORDER_FAR, 7) == (1400, 7, 5, 256)           # 5 tiles of 56 blocks: the last one ragged
    assert builder_strips(ORDER_N, CSR_BLOCK, ORDER_FAR) == (2560, 64, 5, 512)
    assert builder_strips(ORDER_N, CSR_BLOCK, ORDER_FAR + 256) == (4096, 64, 4, 513)    # two tiles: 513 = 512 + 1
    assert (builder_map_blocks(ORDER_N, 1), builder_map_blocks(ORDER_N, 2)) == (1032, 1280)
    for rpb, far, chunk in ((SLICE, ORDER_FAR, None), (SLICE, ORDER_FAR, 1), (SLICE, ORDER_FAR, 7), (CSR_BLOCK, ORDER_FAR, None),
                            (CSR_BLOCK, ORDER_FAR + 256, None)):
        nb = (ORDER_N + rpb - 1) // rpb
        visited = strip_visits(*builder_strips(ORDER_N, rpb, far, chunk), nb)
        assert visit_once(visited, nb) and np.any(visited < 0), (rpb, far, chunk)     # ragged: some workgroups return

    # y_hp against a plain loop in exact arithmetic, on the two smallest matrices
    for A in (holes(oracle, 1, 12), holes(oracle, 2, 12)):
        for dtype in DTYPES:
            C = case_of(oracle, A, dtype)
            ptr, col, val = A.csr(dtype)
            eps = Fraction(float(np.finfo(HP[dtype]).eps))
            for mode in MODES:
                y_hp, bound = C.high_precision(mode)
                for i in range(A.n):
                    s, a = Fraction(0), Fraction(0)
                    for j in range(ptr[i], ptr[i + 1]):
                        p = _exact(val[j]) * _exact(C.x[col[j]])
                        s, a = s + p, a + abs(p)
                    y = Fraction(mode[0]) * s + (_exact(C.y0[i]) if mode[1] else 0)
                    scale = abs(Fraction(mode[0])) * a + (abs(_exact(C.y0[i])) if mode[1] else 0)
                    assert abs(_exact(y_hp[i]) - y) <= 16 * eps * scale, (A.name, dtype, mode, i)
                    g = (A.lens[i] + 2) * Fraction(UNIT[dtype])
                    assert abs(_exact(bound[i]) - g / (1 - g) * scale) <= 16 * eps * g * scale

    # the oracle within the derived bound, everywhere
    for A in list(mats.values()) + [big[0]]:
        for dtype in DTYPES:
            C = case_of(oracle, A, dtype)
            used = np.bincount(A.col, minlength=A.m) > 0
            assert np.all(np.isnan(C.x[~used])) and np.all(np.isfinite(C.x[used])) and np.isnan(C.x[-1])
            for mode in MODES:
                y = C.reference(oracle, mode)
                assert y.dtype == dtype and np.all(np.isfinite(y)) and not np.any(y == SENTINEL), (A.name, dtype, mode)
                assert C.within_bound(y, mode), (A.name, np.dtype(dtype).name, mode)
    _CASES.pop((big[0].name, "float32"), None)                        # (only this test needs it)


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def G(request):
    import torch                                        # before libvexhip.so: the process settles on torch's HIP runtime

    class NS:
        pass
    g = NS()
    g.torch, g.L, g.dev = torch, request.getfixturevalue("built_lib"), torch.device("cuda:0")
    g.up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(g.dev)
    g.stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(g.dev).cuda_stream)
    return g


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _real(dtype):
    return ctypes.c_double if dtype == np.float64 else ctypes.c_float


def _sfx(dtype):
    return "f64" if dtype == np.float64 else "f32"


@contextlib.contextmanager
def variant_word(setter, word, default):
    try:
        setter(word)
        yield
    finally:
        setter(default)


class Vectors:
    """x and y of a case on the device: x at an odd element offset between NaN; y between sentinels, at an odd element offset (never
    16-byte aligned) or, with y_offset = 0, at an even one (16-byte aligned for fp64, 8-byte for fp32: the vector branch of store_pair)."""

    def __init__(self, G, C, y_offset=1):
        self.G, self.C = G, C
        n, m, dtype = C.mat.n, C.mat.m, C.dtype
        xbuf = np.full(m + 8, np.nan, dtype=dtype)
        xbuf[3:3 + m] = C.x
        self.xbuf = G.up(xbuf)
        self.x = self.xbuf[3:3 + m]
        self.y_at = GUARD + y_offset
        self.start, self.start_dev = {}, {}
        for mode in MODES:
            ybuf = np.full(n + 2 * GUARD + 2, SENTINEL, dtype=dtype)
            if mode[1]:
                ybuf[self.y_at:self.y_at + n] = C.y0
            self.start[mode], self.start_dev[mode] = ybuf, G.up(ybuf)
        size = np.dtype(dtype).itemsize
        assert self.xbuf.data_ptr() % 16 == 0 and self.start_dev[MODES[0]].data_ptr() % 16 == 0
        assert self.x.data_ptr() % (2 * size) == size
        assert (self.start_dev[MODES[0]].data_ptr() + self.y_at * size) % (2 * size) == y_offset * size

    def run(self, call, mode):
        """call(x, y, alpha, append); returns the whole y tensor on the host."""
        ybuf = self.start_dev[mode].clone()
        call(self.x, ybuf[self.y_at:self.y_at + self.C.mat.n], mode[0], mode[1])
        return ybuf.cpu().numpy()


def first_difference(got, want):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return "no difference" if len(bad) == 0 else "first differing row %d of %d (%d differ): got %r, want %r" % (
        bad[0], len(got), len(bad), got[bad[0]], want[bad[0]])


def check_run(oracle, V, out, mode, what):
    """Every result finite, equal to the oracle bit for bit, within the derived bound of the high-precision result; every other byte
    of the tensor unchanged."""
    C, n = V.C, V.C.mat.n
    sl = slice(V.y_at, V.y_at + n)
    got, want = out[sl], C.reference(oracle, mode)
    assert np.all(np.isfinite(got)), what + ("not finite: row %d" % np.flatnonzero(~np.isfinite(got))[0],)
    assert np.array_equal(got, want), what + (first_difference(got, want),)
    assert C.within_bound(got, mode), what + ("outside the bound of the high-precision reference",)
    rest = out.copy()
    rest[sl] = V.start[mode][sl]
    assert rest.tobytes() == V.start[mode].tobytes(), what + ("a guard element changed",)


def check_all(oracle, V, calls, what):
    """In both modes: the first call is checked in full; every other one must leave the same bytes in the whole tensor, and says what
    differs if it does not."""
    for mode in MODES:
        first = None
        for name, call in calls:
            out = V.run(call, mode)
            if first is None:
                check_run(oracle, V, out, mode, what + (mode, name))
                first = out
            elif out.tobytes() != first.tobytes():
                check_run(oracle, V, out, mode, what + (mode, name))
                raise AssertionError(what + (mode, name, "differs from " + calls[0][0]))


def checked_traversal(G, name, visited, nb, fields, order=None):
    """A vexhip_traversal for a launch -- only if its visits, restated on the host, pass `visit_once`."""
    from vexcl_amd import _capi
    assert visit_once(visited, nb), (name, nb, "not a traversal: no launch")
    assert int(fields[0]) == len(visited)
    return _capi.Traversal(*[int(f) for f in fields], None if order is None else order.data_ptr())


def hand_made_traversals(G, nb):
    """[(name, traversal)], and the device maps to keep alive."""
    geo = strip_geometry(nb)
    rev, holey = np.arange(nb - 1, -1, -1, dtype=np.int32), holey_map(nb)
    d_rev, d_holey = G.up(rev), G.up(holey)
    return [("strips", checked_traversal(G, "strips", strip_visits(*geo, nb), nb, geo)),
            ("reversed map", checked_traversal(G, "reversed map", rev, nb, (nb, 0, 0, 0), d_rev)),
            ("map with holes", checked_traversal(G, "map with holes", holey, nb, (len(holey), 0, 0, 0), d_holey))], (d_rev, d_holey)


def guarded(G, count, np_dtype, junk):
    """A device buffer of exactly `count` elements between two guards of GUARD elements; returns (whole tensor, view, host copy)."""
    host = np.full(count + 2 * GUARD, junk, dtype=np_dtype)
    host[:GUARD] = host[GUARD + count:] = 77
    whole = G.up(host)
    return whole, whole[GUARD:GUARD + count], host


def check_guarded(whole, host, expected, what):
    got = whole.cpu().numpy()
    count = len(host) - 2 * GUARD
    assert got[:GUARD].tobytes() == host[:GUARD].tobytes() and got[GUARD + count:].tobytes() == host[GUARD + count:].tobytes(), what + ("guard changed",)
    body = got[GUARD:GUARD + count]
    assert body.tobytes() == np.ascontiguousarray(expected).tobytes(), what + (
        "first differing element %d" % np.flatnonzero(body.view(np.uint8) != np.frombuffer(np.ascontiguousarray(expected).tobytes(), dtype=np.uint8))[0],)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. CSR
# ---------------------------------------------------------------------------------------------------------------------------
def csr_device(G, mat, dtype, lead, wide=False, unaligned=False):
    """(ptr, col, val) on the device with ptr[0] = lead: `lead` slack entries in front, SLACK behind; slack columns point at the NaN last
    element of x, slack values are NaN.  unaligned: col and val are views one element into their allocations."""
    ptr, col, val = mat.csr(dtype)
    it = np.int64 if wide else np.int32
    off = 1 if unaligned else 0
    c = np.concatenate([np.full(off + lead, mat.m - 1), col, np.full(SLACK, mat.m - 1)]).astype(it)
    v = np.concatenate([np.full(off + lead, np.nan), val, np.full(SLACK, np.nan)]).astype(dtype)
    dp, cbuf, vbuf = G.up((ptr.astype(np.int64) + lead).astype(it)), G.up(c), G.up(v)
    dc, dv = cbuf[off:], vbuf[off:]
    assert cbuf.data_ptr() % 16 == 0 and vbuf.data_ptr() % 16 == 0 and (dc.data_ptr() % 16 != 0) == unaligned == (dv.data_ptr() % 16 != 0)
    return dp, dc, dv


def csr_call(G, dtype, wide, n, D, trav=None):
    L = G.L
    name = "spmv_csr_%s%s_%s" % ("ordered_" if trav is not None else "", _sfx(dtype), "i64" if wide else "i32")
    entry, real = getattr(L, name), _real(dtype)

    def call(x, y, alpha, append):
        args = (0, G.stream(), n, real(alpha), int(append), _vp(D[0]), _vp(D[1]), _vp(D[2]), _vp(x), _vp(y))
        entry(*args) if trav is None else entry(*args, ctypes.byref(trav))
    return call


def check_csr(G, oracle, mat, dtype, wide):
    L = G.L
    V = Vectors(G, case_of(oracle, mat, dtype))
    nb = (mat.n + CSR_BLOCK - 1) // CSR_BLOCK
    travs, keep_alive = ([], None) if wide else hand_made_traversals(G, nb)       # (the 64-bit entry takes no traversal)
    launches = 0
    for lead in CSR_LEADS:
        D = csr_device(G, mat, dtype, lead, wide)
        calls = [("NULL traversal", csr_call(G, dtype, wide, mat.n, D))] + [(name, csr_call(G, dtype, wide, mat.n, D, t)) for name, t in travs]
        for word in (CSR_WORDS if lead == 0 else CSR_WORDS_OFFSET):
            with variant_word(L.spmv_csr_set_variant, word, -1):
                check_all(oracle, V, calls, (mat.name, _sfx(dtype), "ptr[0] = %d" % lead, "word %d" % word))
            launches += len(calls)
    D = csr_device(G, mat, dtype, 3, wide, unaligned=True)                            # the scalar kernel; a traversal is not looked at
    calls = [("NULL traversal", csr_call(G, dtype, wide, mat.n, D))] + [(name, csr_call(G, dtype, wide, mat.n, D, t)) for name, t in travs[:1]]
    check_all(oracle, V, calls, (mat.name, _sfx(dtype), "unaligned col / val"))
    return launches


@gpu
@every_dtype
@pytest.mark.parametrize("n", CSR_SIZES)
def test_csr_every_form_structure_and_traversal(G, oracle, dtype, n):
    """The 32-bit entries: words 0..7 x (NULL, strips, reversed map, map with holes) at ptr[0] = 0, words 0, 4, 7 at ptr[0] = 1, 2, 3, 4, 7,
    and the scalar kernel, on the four structures; `=` and `+= alpha`."""
    for structure in CSR_STRUCTURES:
        launches = check_csr(G, oracle, csr_matrix(oracle, n, structure), dtype, wide=False)
        assert launches == 4 * (len(CSR_WORDS) + (len(CSR_LEADS) - 1) * len(CSR_WORDS_OFFSET))


@gpu
@pytest.mark.parametrize("n", CSR_SIZES)
def test_csr_64_bit_columns(G, oracle, n):
    """`vexhip_spmv_csr_f64_i64` runs the same kernels with 64-bit row pointers and columns: the same words, offsets and structures."""
    for structure in CSR_STRUCTURES:
        launches = check_csr(G, oracle, csr_matrix(oracle, n, structure), np.float64, wide=True)
        assert launches == len(CSR_WORDS) + (len(CSR_LEADS) - 1) * len(CSR_WORDS_OFFSET)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. hybrid ELL
# ---------------------------------------------------------------------------------------------------------------------------
def analyze(G, ptr):
    w, tail = ctypes.c_int64(-1), ctypes.c_int64(-1)
    d = G.up(np.asarray(ptr, dtype=np.int32))
    G.L.hell_analyze_i32(0, G.stream(), len(ptr) - 1, _vp(d), ctypes.byref(w), ctypes.byref(tail))
    return int(w.value), int(tail.value)


@gpu
def test_hell_width_rule_edges(G, oracle):
    """`vexhip_hell_analyze_i32` against the reference rule, restated on the host and pinned against `oracle.hell_width` by the CPU test:
    all rows equal, exactly a third of the rows wider (and one row fewer), one row, and rows beyond the histogram's last bucket."""
    for name, lens in width_edges().items():
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        w = host_width(lens)
        assert w == WIDTH_EDGE_RESULTS[name] == oracle.hell_width(ptr)
        assert analyze(G, ptr) == (w, int(np.maximum(np.asarray(lens) - w, 0).sum())), name


def fill_matrices(oracle):
    """Width by the rule: with a tail (bands with holes, a ragged CSR matrix with a 4500-entry row) and without one (equal rows)."""
    return [holes(oracle, n, w) for n, w in ((1, 3), (2, 12), (513, 5), (3 * 512 + 77, 9))] + [
        equal_rows(oracle, 100, 5), equal_rows(oracle, 1613, 9), csr_matrix(oracle, 257, "long_row"), csr_matrix(oracle, 845, "ragged")]


@gpu
@every_dtype
def test_hell_analyze_and_fill_match_the_oracle_layout(G, oracle, dtype):
    """Width, tail count, ELL columns and values with the -1 / 0 padding of short rows and of rows n .. pitch - 1, tail pointers, columns
    and values, array for array; the caller's buffers are exactly as large as the header says and lie between guards.  Without a tail
    the fill runs with csr_ptr = NULL."""
    fill = getattr(G.L, "hell_fill_%s_i32" % _sfx(dtype))
    tails = set()
    for mat in fill_matrices(oracle):
        ptr, col, val = mat.csr(dtype)
        H = oracle.hell_build(ptr, col, val.astype(np.float64))
        w, tail, pitch = H["width"], H["tail"], H["pitch"]
        assert w == host_width(mat.lens) and pitch == (mat.n + 15) // 16 * 16 and tail == ell_split(mat, w)[2]
        assert analyze(G, ptr) == (w, tail), mat.name
        dp, dc, dv = G.up(ptr), G.up(np.concatenate([col, [0]]).astype(np.int32)), G.up(np.concatenate([val, [0]]).astype(dtype))
        ec = guarded(G, pitch * w, np.int32, 55)
        ev = guarded(G, pitch * w, dtype, 55)
        if tail:
            cp, cc, cv = guarded(G, mat.n + 1, np.int32, 55), guarded(G, tail, np.int32, 55), guarded(G, tail, dtype, 55)
        else:
            cp = cc = cv = (None, None, None)
        fill(0, G.stream(), mat.n, _vp(dp), _vp(dc), _vp(dv), w, pitch, _vp(ec[1]), _vp(ev[1]), _vp(cp[1]), _vp(cc[1]), _vp(cv[1]))
        G.torch.cuda.synchronize()
        what = (mat.name, _sfx(dtype), w, tail)
        assert np.all(H["ell_col"].reshape(w, pitch)[:, mat.n:] == -1) and np.all(H["ell_val"].reshape(w, pitch)[:, mat.n:] == 0)
        check_guarded(ec[0], ec[2], H["ell_col"], what + ("ell_col",))
        check_guarded(ev[0], ev[2], H["ell_val"].astype(dtype), what + ("ell_val",))
        if tail:
            check_guarded(cp[0], cp[2], H["csr_ptr"], what + ("csr_ptr",))
            check_guarded(cc[0], cc[2], H["csr_col"], what + ("csr_col",))
            check_guarded(cv[0], cv[2], H["csr_val"].astype(dtype), what + ("csr_val",))
        tails.add(tail > 0)
    assert tails == {False, True}


class HellStorage:
    """The hybrid-ELL arrays of a matrix for a forced ELL width, built by `oracle.hell_build` on the host (the library's fill is under test
    elsewhere), on the device at a chosen pitch and element offset."""

    def __init__(self, G, oracle, mat, dtype, w, pitch=None, offset=0):
        ptr, col, val = mat.csr(dtype)
        H = oracle.hell_build(ptr, col, val.astype(np.float64), width=w)
        self.n, self.w, self.tail = mat.n, w, H["tail"]
        self.pitch = H["pitch"] if pitch is None else pitch
        ec, ev = np.full(self.pitch * w, -1, dtype=np.int32), np.zeros(self.pitch * w, dtype=dtype)
        for j in range(w):
            ec[j * self.pitch:j * self.pitch + mat.n] = H["ell_col"][j * H["pitch"]:j * H["pitch"] + mat.n]
            ev[j * self.pitch:j * self.pitch + mat.n] = H["ell_val"][j * H["pitch"]:j * H["pitch"] + mat.n]
        self._ec, self._ev = G.up(np.concatenate([np.full(offset, -1, dtype=np.int32), ec])), G.up(np.concatenate([np.zeros(offset, dtype=dtype), ev]))
        self.ec, self.ev = (self._ec[offset:], self._ev[offset:]) if w else (None, None)
        assert self._ec.data_ptr() % 16 == 0 and self._ev.data_ptr() % 16 == 0
        if self.tail:
            self.cp, self.cc, self.cv = G.up(H["csr_ptr"]), G.up(H["csr_col"]), G.up(H["csr_val"].astype(dtype))
        else:
            self.cp = self.cc = self.cv = None

    @classmethod
    def of_device_arrays(cls, n, w, pitch, ec, ev):
        """Arrays that are on the device already, without a tail."""
        self = cls.__new__(cls)
        self.n, self.w, self.tail, self.pitch, self.ec, self.ev, self.cp, self.cc, self.cv = n, w, 0, pitch, ec, ev, None, None, None
        return self

    def call(self, G, dtype, trav=None):
        entry = getattr(G.L, "spmv_hell_%s%s_i32" % ("ordered_" if trav is not None else "", _sfx(dtype)))
        real = _real(dtype)

        def call(x, y, alpha, append):
            args = (0, G.stream(), self.n, real(alpha), int(append), self.w, self.pitch, _vp(self.ec), _vp(self.ev),
                    _vp(self.cp), _vp(self.cc), _vp(self.cv), _vp(x), _vp(y))
            entry(*args) if trav is None else entry(*args, ctypes.byref(trav))
        return call


def odd_pitch(n):
    p = n + 1
    return p if p % 16 else p + 1


@gpu
@every_dtype
@pytest.mark.parametrize("n", ROW_SIZES)
def test_hell_products_every_word_width_and_layout(G, oracle, dtype, n):
    """Words 0..15 x ELL widths 1..9 and 12 x (with a tail, without: csr_ptr = NULL); per width the odd pitch and the unaligned arrays
    (one row per lane whatever the word says), the ordered product with the hand-made traversals of 512-row blocks and its refusal of
    unaligned arrays; once per n the tail alone (width 0) and the empty part."""
    from vexcl_amd import _capi
    L = G.L
    travs, keep_alive = hand_made_traversals(G, (n + SLICE - 1) // SLICE)
    for w in ELL_WIDTHS:
        full = holes(oracle, n, w)
        for mat in (full, truncated(full, w)):
            V = Vectors(G, case_of(oracle, mat, dtype))
            S = HellStorage(G, oracle, mat, dtype, w)
            assert (S.tail > 0) == (mat is full) and S.pitch % 16 == 0
            what = (mat.name, _sfx(dtype), "width %d" % w)
            plain = [("plain", S.call(G, dtype))]
            for word in HELL_WORDS:
                with variant_word(L.spmv_hell_set_variant, word, -1):
                    check_all(oracle, V, plain, what + ("word %d" % word,))
            check_all(oracle, V, plain + [(name, S.call(G, dtype, t)) for name, t in travs], what + ("ordered",))
            P, U = HellStorage(G, oracle, mat, dtype, w, pitch=odd_pitch(n)), HellStorage(G, oracle, mat, dtype, w, offset=1)
            assert P.pitch % 16 != 0 and P.pitch >= n and U.ec.data_ptr() % 16 != 0 and U.ev.data_ptr() % 16 != 0
            for word in HELL_WORDS_FALLBACK:
                with variant_word(L.spmv_hell_set_variant, word, -1):
                    check_all(oracle, V, [("odd pitch", P.call(G, dtype)), ("unaligned", U.call(G, dtype))], what + ("word %d" % word,))
            for R in (P, U):                                          # the ordered product needs vector loads: an error code, not a launch
                for mode in MODES:
                    ybuf = V.start_dev[mode].clone()
                    with pytest.raises(_capi.Error, match="aligned ELL arrays"):
                        R.call(G, dtype, travs[0][1])(V.x, ybuf[V.y_at:V.y_at + n], *mode)
                    assert ybuf.cpu().numpy().tobytes() == V.start[mode].tobytes(), what + ("a refused call wrote to y",)
    # the tail alone: ELL width 0, the whole matrix in the CSR part
    mat = holes(oracle, n, 5)
    V = Vectors(G, case_of(oracle, mat, dtype))
    S = HellStorage(G, oracle, mat, dtype, 0)
    assert S.tail == len(mat.col) and S.ec is None
    for word in (0, 7, 15):
        with variant_word(L.spmv_hell_set_variant, word, -1):
            check_all(oracle, V, [("tail only", S.call(G, dtype))], (mat.name, _sfx(dtype), "width 0", "word %d" % word))
    # the empty part: `=` writes zeros, `+=` leaves y byte-identical
    S.cp = S.cc = S.cv = None
    for mode in MODES:
        out = V.run(S.call(G, dtype), mode)
        want = V.start[mode].copy()
        if not mode[1]:
            want[V.y_at:V.y_at + n] = 0
        assert out.tobytes() == want.tobytes(), (n, _sfx(dtype), "empty part", mode)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. SELL-512
# ---------------------------------------------------------------------------------------------------------------------------
def sell_fill_checked(G, oracle, mat, dtype, w):
    """`vexhip_sell_fill_*` into a buffer of exactly `vexhip_sell_bytes` bytes between guards, compared byte for byte with the layout
    restated from `oracle.sell_pair_slots`; returns the filled buffer (16-byte aligned)."""
    L = G.L
    size = np.dtype(dtype).itemsize
    ptr, col, val = mat.csr(dtype)
    want = np.frombuffer(sell_buffer(oracle, mat, w, dtype), dtype=np.uint8)
    nbytes = L.sell_bytes(mat.n, w, size)
    assert nbytes == len(want) == (mat.n + SLICE - 1) // SLICE * SLICE * w * (4 + size)
    whole, view, host = guarded(G, nbytes, np.uint8, 0x5a)
    assert view.data_ptr() % 16 == 0
    dp, dc, dv = G.up(ptr), G.up(np.concatenate([col, [0]]).astype(np.int32)), G.up(np.concatenate([val, [0]]).astype(dtype))
    getattr(L, "sell_fill_%s_i32" % _sfx(dtype))(0, G.stream(), mat.n, _vp(dp), _vp(dc), _vp(dv), w, _vp(view))
    G.torch.cuda.synchronize()
    check_guarded(whole, host, want, (mat.name, _sfx(dtype), "SELL fill, width %d" % w))
    return whole, view


def sell_call(G, dtype, n, w, sell, tail, trav=None):
    entry, real = getattr(G.L, "spmv_sell_%s_i32" % _sfx(dtype)), _real(dtype)

    def call(x, y, alpha, append):
        entry(0, G.stream(), n, real(alpha), int(append), w, _vp(sell), _vp(tail[0]), _vp(tail[1]), _vp(tail[2]), _vp(x), _vp(y),
              None if trav is None else ctypes.byref(trav))
    return call


def tail_of(G, oracle, mat, dtype, w):
    ptr, col, val = mat.csr(dtype)
    H = oracle.hell_build(ptr, col, val.astype(np.float64), width=w)
    return (G.up(H["csr_ptr"]), G.up(H["csr_col"]), G.up(H["csr_val"].astype(dtype))) if H["tail"] else (None, None, None)


def check_sell_products(G, oracle, mat, dtype, w, sell, travs):
    """Pair kernel and `sell_kernel<W>` (w <= 8) or the looping kernel (w > 8), NULL and hand-made traversals, y at an odd and at an even
    element offset (the scalar and the 16-byte branch of store_pair)."""
    L = G.L
    tail = tail_of(G, oracle, mat, dtype, w)
    calls = [("NULL traversal", sell_call(G, dtype, mat.n, w, sell, tail))] + [(name, sell_call(G, dtype, mat.n, w, sell, tail, t)) for name, t in travs]
    forms = 0
    for y_offset in (1, 0):
        V = Vectors(G, case_of(oracle, mat, dtype), y_offset)
        for word in ((0, 1) if w <= 8 else (0,)):
            with variant_word(L.spmv_sell8_set_variant, word, 0):
                check_all(oracle, V, calls, (mat.name, _sfx(dtype), "width %d" % w, "y offset %d" % y_offset, "SELL word %d" % word))
            forms += 1
    return tail[0] is not None, forms


@gpu
@every_dtype
@pytest.mark.parametrize("n", ROW_SIZES)
def test_sell_fill_and_products_every_width(G, oracle, dtype, n):
    """Per ELL width 1..9 and 12: the fill against the restated layout, every row of every slice (padding rows of the last slice: negative
    columns, value 0), then the products on the filled buffer with the CSR tail and, on the matrix cut to its ELL part, without one."""
    travs, keep_alive = hand_made_traversals(G, (n + SLICE - 1) // SLICE)
    seen = set()
    for w in ELL_WIDTHS:
        full = holes(oracle, n, w)
        cols, ent = sell_expected(oracle, full, w)
        rows_in_last = n - (n - 1) // SLICE * SLICE
        assert np.all(cols[-1, :, rows_in_last:] < 0) and np.all(ent[-1, :, rows_in_last:] == -1)
        whole, sell = sell_fill_checked(G, oracle, full, dtype, w)
        for mat in (full, truncated(full, w)):
            has_tail, forms = check_sell_products(G, oracle, mat, dtype, w, sell, travs)
            assert has_tail == (mat is full) and forms == (4 if w <= 8 else 2)
            seen.add((w, has_tail))
    assert seen == {(w, t) for w in ELL_WIDTHS for t in (False, True)}


@gpu
@every_dtype
def test_sell_padding_codes_at_both_ends_of_x(G, oracle, dtype):
    """-2 next to a lone column 0 of an odd row and next to a lone largest column of an even row, -1 for the missing partner of the last
    row of an odd n; and 513 rows in which no lane of any wave has a pair: sell_pair_kernel skips its 16-byte load (`ballot == 0`)."""
    for mat, w in ((pad_edges(oracle), 2), (unpaired(oracle), 2), (unpaired(oracle), 1)):
        cols, _ = sell_expected(oracle, mat, w)
        assert mat.name != "pad_edges" or (np.count_nonzero(cols == -2) == 2 and np.count_nonzero(cols[0, :, :5] == -1) == 2)
        whole, sell = sell_fill_checked(G, oracle, mat, dtype, w)
        travs, keep_alive = hand_made_traversals(G, (mat.n + SLICE - 1) // SLICE)
        has_tail, forms = check_sell_products(G, oracle, mat, dtype, w, sell, travs)
        assert has_tail == (w == 1) and forms == 4


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the order builders
# ---------------------------------------------------------------------------------------------------------------------------
class BigStorages:
    """CSR, hybrid ELL (width 4, no tail) and SELL-512 buffers of a banded matrix on the device, filled by the library (the fills are
    under test above, at sizes where every element is compared)."""

    def __init__(self, G, mat, w, sell_types=DTYPES):
        L, n = G.L, mat.n
        self.n, self.w, self.pitch = n, w, (n + 15) // 16 * 16
        ptr, col, val = mat.csr(np.float64)
        self.ptr, self.col, self.val = G.up(ptr), G.up(np.concatenate([col, np.full(SLACK, mat.m - 1)]).astype(np.int32)), G.up(np.concatenate([val, np.full(SLACK, np.nan)]))
        self.ec = G.torch.empty(self.pitch * w, dtype=G.torch.int32, device=G.dev)
        self.ev = G.torch.empty(self.pitch * w, dtype=G.torch.float64, device=G.dev)
        L.hell_fill_f64_i32(0, G.stream(), n, _vp(self.ptr), _vp(self.col), _vp(self.val), w, self.pitch, _vp(self.ec), _vp(self.ev), None, None, None)
        self.sell = {}
        for dtype in sell_types:
            size = np.dtype(dtype).itemsize
            buf = G.torch.empty(L.sell_bytes(n, w, size), dtype=G.torch.uint8, device=G.dev)
            v = self.val if dtype == np.float64 else self.val.to(G.torch.float32)
            getattr(L, "sell_fill_%s_i32" % _sfx(dtype))(0, G.stream(), n, _vp(self.ptr), _vp(self.col), _vp(v), w, _vp(buf))
            assert buf.data_ptr() % 16 == 0
            self.sell[dtype] = buf
        self.capacity = int(L.hell_order_capacity(n))
        G.torch.cuda.synchronize()

    def build(self, G, which, mode):
        """(traversal, map tensor) from `vexhip_hell_order_i32` ("hell"), `vexhip_sell_order_i32` (a value type) or
        `vexhip_csr_traversal_i32` ("csr")."""
        from vexcl_amd import _capi
        L, out = G.L, _capi.Traversal(-1, -1, -1, -1, None)
        order = G.torch.full((self.capacity,), -7, dtype=G.torch.int32, device=G.dev)
        if which == "csr":
            L.csr_traversal_i32(0, G.stream(), self.n, _vp(self.ptr), _vp(self.col), CSR_BLOCK, ctypes.byref(out))
        elif which == "hell":
            L.hell_order_i32(0, G.stream(), self.n, self.w, self.pitch, _vp(self.ec), mode, _vp(order), self.capacity, ctypes.byref(out))
        else:
            L.sell_order_i32(0, G.stream(), self.n, self.w, np.dtype(which).itemsize, _vp(self.sell[which]), mode, _vp(order), self.capacity, ctypes.byref(out))
        return out, order


def checked_built_traversal(S, out, order, expect, rows_per_block, what):
    """The returned struct as restated, the visits -- downloaded (a map) or restated (strips) -- pass `visit_once`, the grid fits the
    capacity: only then may a product be launched with it."""
    nb = (S.n + rows_per_block - 1) // rows_per_block
    got = (int(out.grid_blocks), int(out.chunk), int(out.planes), int(out.plane_blocks))
    assert got == expect and 0 < got[0] <= S.capacity, what + (got, expect)
    if expect[1] == 0:
        assert out.order == order.data_ptr(), what
        visited = order[:got[0]].cpu().numpy()
    else:
        assert not out.order, what
        visited = strip_visits(*got, nb)
    assert visit_once(visited, nb), what + ("not a traversal: no launch",)
    return out


@gpu
def test_order_builders_on_the_smallest_matrix_that_turns_them_on(G, oracle):
    """Diagonals -131072, -512, 0, +131072 on 4 * 131072 + 513 rows.  Per builder and mode: the struct, the visit-once check on the host,
    the capacity, and only then the ordered product, bit for bit against the plain product of the same storage and the oracle."""
    mat = order_matrix(oracle)
    S = BigStorages(G, mat, 4)
    V = Vectors(G, case_of(oracle, mat, np.float64))
    hell = HellStorage.of_device_arrays(S.n, 4, S.pitch, S.ec, S.ev)
    no_tail = (None, None, None)
    built = 0
    for mode in ORDER_MODES:
        expect = (builder_map_blocks(S.n, mode), 0, 0, 0) if mode in (1, 2) else builder_strips(S.n, SLICE, ORDER_FAR, mode - 100 if mode >= 100 else None)
        out, order = S.build(G, "hell", mode)
        t = checked_built_traversal(S, out, order, expect, SLICE, ("hell_order", mode))
        check_all(oracle, V, [("plain", hell.call(G, np.float64)), ("ordered", hell.call(G, np.float64, t))], ("hell", "mode %d" % mode))
        for dtype in DTYPES:
            out, order = S.build(G, dtype, mode)
            t = checked_built_traversal(S, out, order, expect, SLICE, ("sell_order", _sfx(dtype), mode))
            Vd = V if dtype == np.float64 else Vectors(G, Case(oracle, mat, dtype))
            check_all(oracle, Vd, [("plain", sell_call(G, dtype, S.n, 4, S.sell[dtype], no_tail)),
                                   ("ordered", sell_call(G, dtype, S.n, 4, S.sell[dtype], no_tail, t))], ("sell", _sfx(dtype), "mode %d" % mode))
            built += 1
        built += 1
    out, order = S.build(G, "csr", 0)
    t = checked_built_traversal(S, out, order, builder_strips(S.n, CSR_BLOCK, ORDER_FAR), CSR_BLOCK, ("csr_traversal",))
    D = (S.ptr, S.col, S.val)
    check_all(oracle, V, [("plain", csr_call(G, np.float64, False, S.n, D)), ("ordered", csr_call(G, np.float64, False, S.n, D, t))], ("csr",))
    assert built == 3 * len(ORDER_MODES)


@gpu
def test_order_builders_decline(G, oracle):
    """grid_blocks == 0 (plain order) below 8 * 65536 rows, for a far diagonal that is no multiple of the block's 512 rows, for a far
    diagonal in fewer than half the rows, and for ELL width 33 (the positive matrix, stored 33 wide: 29 columns of padding).  The CSR
    builder counts 256-row blocks: 131072 + 256 is a multiple of those, and it returns the restated strips there."""
    def declined(S, what, csr_expect=None):
        for which in ("hell",) + DTYPES:
            for mode in ORDER_MODES:
                out, _ = S.build(G, which, mode)
                assert (out.grid_blocks, out.chunk, out.planes, out.plane_blocks, out.order) == (0, 0, 0, 0, None), what + (which, mode)
        if csr_expect is not None:
            out, order = S.build(G, "csr", 0)
            if csr_expect:
                checked_built_traversal(S, out, order, csr_expect, CSR_BLOCK, what + ("csr",))
            else:
                assert (out.grid_blocks, out.chunk, out.planes, out.plane_blocks, out.order) == (0, 0, 0, 0, None), what + ("csr",)

    small, misaligned, sparse_far = order_negatives(oracle)
    declined(BigStorages(G, small[0], 4), (small[1],), csr_expect=())
    declined(BigStorages(G, misaligned[0], 4), (misaligned[1],), csr_expect=builder_strips(ORDER_N, CSR_BLOCK, ORDER_FAR + 256))
    declined(BigStorages(G, sparse_far[0], 4), (sparse_far[1],), csr_expect=())
    declined(BigStorages(G, order_matrix(oracle), 33), ("width 33",))
