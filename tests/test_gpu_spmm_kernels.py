"""Direct parity tests of the multi-right-hand-side SELL products of vexcl_amd/csrc/spmm.hip: `spmm_sell_kernel` (32-bit columns),
`spmm_coded_kernel<..., VCODED = false>` (diagonal codes, stored values) and `<..., VCODED = true>` (diagonal and value codes), fp64 and fp32, NR = 1..4
right-hand sides per launch and the split of 5..8 right-hand sides into two passes, the unrolled widths 3, 5, 7, 9 and the looping
branch, with and without a CSR tail, and the slice-dictionary forms of the two coded kernels.

What runs where
  * test_full_bands_*, test_bands_with_holes_*, test_unstructured_*: `ops.SlicedELL(..., codes=False)`, `(..., value_codes=False)`
    and `(...)` driven through `mul_multi`, i.e. `vexhip_spmm_sell_*`, `_sell8_*`, `_sell8v_*`, with the storage's traversal,
    with NULL, and with two hand-made traversals (arithmetic strips; an explicit map of the slices in reverse): the set-up
    gives matrices this small an empty traversal, and the kernels' `traversal_block` would otherwise only see plain order.
  * test_dictionary_forms_*: `ops.SpMat(..., direct=False, march=False)` on 65 slices whose code blocks repeat; the test reads
    `A.info` and calls `vexhip_spmm_sell8_dict_*` / `vexhip_spmm_sell8v_dict_*` itself (traversal `&info.traversal`, NULL, the hand-made two),
    and makes the same product through `A.apply_multi` (`vexhip_spmat_apply_multi_*`).
  * test_generated_matrices_and_references (no GPU): pins the generators, the high-precision reference and the oracle.
Every test asserts the storage the library chose (format, ELL width, tail entries, diagonals, values, dictionary blocks): the
expected figures are restated on the host from the hybrid-ELL width rule (`oracle.hell_width`) and the first `width` entries of
every row.  Only the set-up code of the library builds the storages, so only the products are under test.

Why the comparisons are exact
  spmm.hip is compiled with -ffp-contract=off and folds a row in storage order -- the ELL part in CSR order, then the CSR tail --
  as the single-vector kernels and `oracle.spmv_csr` do; padding adds +0 to a sum that started at +0.  Every Y_k is therefore
  compared with `np.array_equal` against the oracle in the matrix's own type and against the single-vector product of the same
  storage (`S.mul` / `A.apply`).  No tolerance in those comparisons.

The independent check
  The oracle shares its summation order with the kernels, so every result is also held against products and row sums in
  np.longdouble (fp64) / float64 (fp32): |y - y_hp| <= g (|alpha| sum_j |a_ij x_j| + |y0_i|), g = (L+2)u / (1 - (L+2)u), L the row
  length (ELL + tail), u = 2^-53 / 2^-24.  That is the standard bound of a recursive sum of L rounded products followed by one
  scaling and one addition; it is derived, not measured, and the CPU test holds the oracle to it as well.

Canaries
  Every x and y is a view at an ODD element offset of a larger tensor (8-byte / 4-byte aligned, never 16-byte aligned).  x is
  surrounded by NaN, and every element of x that no entry of the matrix uses is NaN: a padded lane that multiplies a stray x
  shows as a non-finite result.  y has 64 sentinel elements on either side, compared as bytes after every call, and the results
  of right-hand sides that were NOT passed must keep their bytes too: a store past row n - 1 or to a wrong vector shows there.
  All of these addresses lie inside live allocations.

Rows n = 1 and 2 use the diagonals 0 .. w-1 of an n x (n + w - 1) matrix, so that every width exists there too and
`SlicedELL` never sees an empty ELL part; no size is skipped for any storage."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

DTYPES = (np.float64, np.float32)
HP = {np.float64: np.longdouble, np.float32: np.float64}          # the type of the independent reference
UNIT = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
MODES = ((1.0, False), (-0.75, True))                             # (alpha, append)
MAX_NRHS = 8                                                      # nrhs = 1..8: NR = 1..4 and the passes 4+1 .. 4+4
GUARD = 64                                                        # sentinel elements on either side of every y
SENTINEL = 12345.0
EXTRA_COLS = 8                                                    # columns behind the band that only the extra entries use
SLICE = 512

UNROLLED, LOOPED = (3, 5, 7, 9), (4, 12)
BAND_SIZES = (1, 2, 511, 512, 513, 3 * 512 + 77)
HOLES_N = 3 * 512 + 77
HOLES_UNROLLED = (-700, -3, -1, 0, 2, 9, 40, 41)                  # 8 diagonals kept with probability 0.8: ELL width 7
HOLES_LOOPED = (-700, -3, -1, 0, 2, 9, 40)                        # 7 diagonals: ELL width 6, the looping branch
HOLES_WIDTH = {"unrolled": 7, "looped": 6}
DICT_N = 64 * 512 + 77                                            # 65 slices: make_dictionary looks from 64 slices on
DICT_DIAGONALS = {4: 6, 5: 7, 7: 10, 8: 12, 9: 13, 12: 18}        # ELL width -> diagonals of the period-3 pattern
DICT_WIDTHS = {"sell8": (5, 7, 4, 8), "sell8v": (5, 7, 4, 8, 9, 12)}   # stored values: a dictionary up to width 8 only

STORAGES = {"sell32": {"codes": False}, "sell8": {"value_codes": False}, "sell8v": {}}

every_dtype = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
every_storage = pytest.mark.parametrize("storage", tuple(STORAGES))


# ---------------------------------------------------------------------------------------------------------------------------
# matrices: CSR with ascending columns, values kept in float64 and rounded to the type under test
# ---------------------------------------------------------------------------------------------------------------------------
class Mat:
    def __init__(self, name, n, m, ptr, col, val, tail_rows=()):
        self.name, self.n, self.m = name, int(n), int(m)
        self.ptr = np.ascontiguousarray(ptr, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        self.tail_rows = tuple(int(r) for r in tail_rows)         # rows that got three extra entries behind the band
        self.lens = np.diff(self.ptr.astype(np.int64))
        self.rows = np.repeat(np.arange(self.n, dtype=np.int64), self.lens)
        self._csr = {}

    def csr(self, dtype):
        key = np.dtype(dtype).name
        if key not in self._csr:
            self._csr[key] = (self.ptr, self.col, np.ascontiguousarray(self.val.astype(dtype)))
        return self._csr[key]

    def expected_storage(self, oracle, dtype):
        """What the set-up must report: the hybrid-ELL width, the entries past it, and the distinct diagonals / values (as bit
        patterns of `dtype`) among the first `width` entries of every row."""
        w = oracle.hell_width(self.ptr)
        pos = np.arange(len(self.col), dtype=np.int64) - np.repeat(self.ptr[:-1].astype(np.int64), self.lens)
        ell = pos < w
        bits = self.csr(dtype)[2][ell].view(np.uint64 if dtype == np.float64 else np.uint32)
        return {"width": int(w), "tail_nnz": int((~ell).sum()),
                "ndeltas": len(np.unique(self.col[ell].astype(np.int64) - self.rows[ell])), "nvalues": len(np.unique(bits))}


def _uniform(oracle, seed, count):
    return oracle.random_f64(seed, max(1, count))[:count] - 0.5


def _from_mask(oracle, name, n, m, diagonals, keep, constant, seed):
    """Row i holds diagonal k (column i + diagonals[k]) where keep[i, k] and the column lies in [0, m).  constant: one value
    per diagonal (value codes), else a random value per entry."""
    d = np.asarray(diagonals, dtype=np.int64)
    assert np.all(np.diff(d) > 0)
    cols = np.arange(n, dtype=np.int64)[:, None] + d[None, :]
    ok = keep & (cols >= 0) & (cols < m)
    vals = (np.broadcast_to(_uniform(oracle, seed, len(d))[None, :], ok.shape) if constant
            else _uniform(oracle, seed, n * len(d)).reshape(n, len(d)))
    ptr = np.concatenate([[0], np.cumsum(ok.sum(axis=1))])
    return Mat(name, n, m, ptr, cols[ok], vals[ok])


def band_diagonals(n, w):
    """The band's diagonals and the number of columns: centred for n >= 511; 0 .. w-1 of an n x (n + w - 1) matrix for n = 1, 2."""
    return (np.arange(w), n + w - 1) if n <= 2 else (np.arange(w) - w // 2, n)


_MATS = {}


def _cached(name, make):
    if name not in _MATS:
        _MATS[name] = make()
        assert _MATS[name].name == name
    return _MATS[name]


def full_band(oracle, n, w, constant):
    name = "band_n%d_w%d_%s" % (n, w, "constant" if constant else "random")
    d, m = band_diagonals(n, w)
    return _cached(name, lambda: _from_mask(oracle, name, n, m, d, np.ones((n, w), dtype=bool), constant, 100 + w))


def holes_random(oracle, which, constant):
    """Row i keeps each in-range diagonal with probability 0.8: neighbouring rows hold different diagonals in one ELL column
    and short rows are padded; diagonal -700 makes i + delta leave the slice."""
    name = "holes_%s_%s" % (which, "constant" if constant else "random")
    d = HOLES_UNROLLED if which == "unrolled" else HOLES_LOOPED

    def make():
        keep = oracle.random_f64(200 + len(d), HOLES_N * len(d)).reshape(HOLES_N, len(d)) < 0.8
        return _from_mask(oracle, name, HOLES_N, HOLES_N, d, keep, constant, 210 + len(d))
    return _cached(name, make)


def holes_periodic(oracle, w, constant):
    """Row i keeps diagonal number k iff (i + k) % 3 != 0, on 65 slices: 512 % 3 = 2, so the interior slices repeat with
    period 3 -- a handful of distinct code blocks, well under blocks * 4 <= slices.  3q diagonals give rows of 2q entries,
    3q + 1 diagonals rows of 2q and 2q + 1 entries: ELL width 2q and 2q + 1 by the hybrid-ELL rule."""
    name = "periodic_w%d_%s" % (w, "constant" if constant else "random")
    nd = DICT_DIAGONALS[w]

    def make():
        keep = (np.arange(DICT_N)[:, None] + np.arange(nd)[None, :]) % 3 != 0
        return _from_mask(oracle, name, DICT_N, DICT_N, np.arange(nd) - nd // 2, keep, constant, 300 + w)
    return _cached(name, make)


def tail_rows_of(base, width):
    """About 40 rows for the extra entries: row 0, the last row, an odd row whose (even) partner is short, rows on both sides
    of slice boundaries; all inside the first two and the last two slices, so that the slices in between keep repeating."""
    n = base.n
    odd = np.concatenate([np.arange(17, 2 * SLICE, 2), np.arange(1, 17, 2)])      # (an all-equal interior: a clipped first row)
    short_partner = int(odd[base.lens[odd - 1] < width][0])
    last = (n - 1) // SLICE * SLICE                                   # first row of the ragged last slice
    rows = {0, 1, 2, 3, 6, 9, 255, 256, 300, 509, 510, 511, 512, 513, 514, 700, 701, 1000, 1022, 1023, short_partner,
            last - SLICE, last - SLICE + 1, last - 258, last - 3, last - 2, last - 1, last, last + 1, last + 2, last + 3, last + 30,
            last + 31, n - 8, n - 7, n - 4, n - 3, n - 2, n - 1}
    return sorted(r for r in rows if 0 <= r < n), short_partner


def with_tail(oracle, base, width):
    """Three extra entries in each of about 40 rows, at columns behind every band column: in a row that is full they land in
    the CSR tail, and the ELL part stays the band."""
    name = base.name + "_tail"

    def make():
        rows, _ = tail_rows_of(base, width)
        extra_val = _uniform(oracle, 400 + base.n % 97, 3 * len(rows)).reshape(len(rows), 3)
        lens = base.lens.copy()
        lens[rows] += 3
        ptr = np.concatenate([[0], np.cumsum(lens)])
        col, val = np.empty(ptr[-1], dtype=np.int64), np.empty(ptr[-1], dtype=np.float64)
        own = np.ones(ptr[-1], dtype=bool)
        for k, r in enumerate(rows):
            e = ptr[r + 1]
            own[e - 3:e] = False
            col[e - 3:e] = base.m + np.array([r % 3, 3 + r % 2, 5 + r % 3])
            val[e - 3:e] = extra_val[k]
        col[own], val[own] = base.col, base.val
        return Mat(name, base.n, base.m + EXTRA_COLS, ptr, col, val, tail_rows=rows)
    return _cached(name, make)


EMPTY_SLICE = (SLICE, 2 * SLICE)                                      # rows 512..1023: one whole slice


def with_empty_rows(base):
    name = base.name + "_empty_rows"

    def make():
        keep_row = np.ones(base.n, dtype=bool)
        keep_row[EMPTY_SLICE[0]:EMPTY_SLICE[1]] = False
        keep_row[base.n - 5:] = False
        lens = np.where(keep_row, base.lens, 0)
        keep = np.repeat(keep_row, base.lens)
        return Mat(name, base.n, base.m, np.concatenate([[0], np.cumsum(lens)]), base.col[keep], base.val[keep])
    return _cached(name, make)


UNUSED_EVERY, UNUSED_AT = 11, 5


def with_unused_columns(base):
    """Every entry in a column c with c % 11 == 5 removed: x is NaN there (Case), right next to columns that are read.  A lane
    whose row is padded beside a real entry of its partner row loads exactly such a neighbour in the 16-byte load of
    gather_pair, and has to mask it."""
    name = base.name + "_unused_columns"

    def make():
        keep = base.col % UNUSED_EVERY != UNUSED_AT
        lens = np.bincount(base.rows[keep], minlength=base.n)
        return Mat(name, base.n, base.m, np.concatenate([[0], np.cumsum(lens)]), base.col[keep], base.val[keep])
    return _cached(name, make)


def unstructured(oracle, which):
    name = "unstructured_" + which
    n, m, per_row = {"square": (1613, 1613, 16), "wide": (1613, 2500, 6)}[which]
    return _cached(name, lambda: Mat(name, n, m, *oracle.random_matrix(77 + per_row, n, m, per_row)))


def band_matrices(oracle, constant):
    return [full_band(oracle, n, w, constant) for w in UNROLLED + LOOPED for n in BAND_SIZES]


def holes_matrices(oracle, constant):
    out = []
    for which in ("unrolled", "looped"):
        base = holes_random(oracle, which, constant)
        out += [base, with_tail(oracle, base, HOLES_WIDTH[which]), with_empty_rows(base)]
    return out + unused_column_matrices(oracle, constant)


def unused_column_matrices(oracle, constant):
    """ELL widths 5 (with a tail) and 7 (without): the unrolled branch, where gather_pair runs."""
    return [with_unused_columns(holes_random(oracle, "looped", constant)), with_unused_columns(full_band(oracle, HOLES_N, 7, constant))]


def dictionary_matrices(oracle, storage):
    out = []
    for w in DICT_WIDTHS[storage]:
        base = holes_periodic(oracle, w, storage == "sell8v")
        out += [(w, base), (w, with_tail(oracle, base, w))]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# right-hand sides and references, computed once per (matrix, type) and shared by every test
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
    """Eight right-hand sides and start vectors of one matrix in one type, the oracle's results and the high-precision ones."""

    def __init__(self, oracle, mat, dtype):
        self.mat, self.dtype = mat, dtype
        ptr, col, val = mat.csr(dtype)
        used = np.zeros(mat.m, dtype=bool)
        used[col] = True
        seed = 1000 + 17 * mat.n + 3 * mat.m + len(mat.col) % 1000
        self.x, self.y0 = [], []
        for k in range(MAX_NRHS):
            x = _uniform(oracle, seed + k, mat.m).astype(dtype)
            x[~used] = np.nan                                         # no entry reads these
            self.x.append(x)
            self.y0.append(_uniform(oracle, seed + 50 + k, mat.n).astype(dtype))
        hp = HP[dtype]
        self.sum, self.abs_sum = [], []
        for x in self.x:
            prod = val.astype(hp) * x.astype(hp)[col]
            self.sum.append(segment_sums(prod, ptr))
            self.abs_sum.append(segment_sums(np.abs(prod), ptr))
        lu = (mat.lens + 2).astype(hp) * hp(UNIT[dtype])
        self.gamma = lu / (1 - lu)
        self._ref = {}

    def x_of(self, k, alias):
        return self.x[0] if alias and k == 2 else self.x[k]          # alias: the same vector is right-hand side 0 and 2

    def reference(self, oracle, k, mode, alias=False):
        """oracle.spmv_csr in the matrix's own type.  `=` starts from NaN: every row must be written."""
        key = (k, mode, alias and k == 2)
        if key not in self._ref:
            alpha, append = mode
            ptr, col, val = self.mat.csr(self.dtype)
            y = self.y0[k].copy() if append else np.full(self.mat.n, np.nan, dtype=self.dtype)
            self._ref[key] = oracle.spmv_csr(ptr, col, val, self.x_of(k, alias), y, alpha, append)
        return self._ref[key]

    def high_precision(self, k, mode, alias=False):
        """(y_hp, bound): products and row sums in HP, and g (|alpha| sum |a x| + |y0|)."""
        alpha, append = mode
        hp = HP[self.dtype]
        j = 0 if alias and k == 2 else k
        y = hp(alpha) * self.sum[j]
        scale = hp(abs(alpha)) * self.abs_sum[j]
        if append:
            y = y + self.y0[k].astype(hp)
            scale = scale + np.abs(self.y0[k].astype(hp))
        return y, self.gamma * scale

    def within_bound(self, y, k, mode, alias=False):
        y_hp, bound = self.high_precision(k, mode, alias)
        return bool(np.all(np.abs(y.astype(HP[self.dtype]) - y_hp) <= bound))


_CASES = {}


def case_of(oracle, mat, dtype):
    key = (mat.name, np.dtype(dtype).name)
    if key not in _CASES:
        _CASES[key] = Case(oracle, mat, dtype)
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------------------
# the CPU test: generators, high-precision reference, oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _exact(v):
    """A float32 / float64 / longdouble scalar as a Fraction (a longdouble is the sum of two doubles)."""
    hi = float(v)
    return Fraction(hi) + Fraction(float(v - type(v)(hi)))


def _check_structure(mat):
    assert mat.ptr[0] == 0 and mat.ptr[-1] == len(mat.col) == len(mat.val) and np.all(mat.lens >= 0), mat.name
    assert len(mat.col) == 0 or (mat.col.min() >= 0 and mat.col.max() < mat.m), mat.name
    inner = np.ones(len(mat.col), dtype=bool)
    inner[mat.ptr[:-1][mat.lens > 0]] = False                         # first entry of every row
    assert np.all(np.diff(mat.col.astype(np.int64))[inner[1:]] > 0), mat.name + ": columns do not ascend inside a row"
    assert np.all(np.abs(mat.val) <= 1.0) and np.all(mat.val != 0), mat.name


def test_generated_matrices_and_references(oracle):
    """Pins the helpers of this file without a GPU: every generated matrix has ascending columns inside [0, m), the promised
    widths, hole patterns and tail rows; y_hp equals a plain Python double loop (in exact rational arithmetic) on the two
    smallest matrices; `oracle.spmv_csr` lies within the derived bound on every matrix of the file, in both types."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no wider than double here: no independent fp64 reference"
    mats = {}
    for constant in (False, True):
        for w in UNROLLED + LOOPED:
            for n in BAND_SIZES:
                A = full_band(oracle, n, w, constant)
                d, m = band_diagonals(n, w)
                want = np.arange(n)[:, None] + d[None, :]
                assert (A.n, A.m) == (n, m) and np.array_equal(A.col, want[(want >= 0) & (want < m)]), A.name
                exp = A.expected_storage(oracle, np.float64)
                assert exp == {"width": w, "tail_nnz": 0, "ndeltas": w, "nvalues": w if constant else len(A.col)}, (A.name, exp)
                mats[A.name] = A
        for which, diagonals in (("unrolled", HOLES_UNROLLED), ("looped", HOLES_LOOPED)):
            A = holes_random(oracle, which, constant)
            w = HOLES_WIDTH[which]
            exp = A.expected_storage(oracle, np.float64)
            assert exp["width"] == w and exp["ndeltas"] == len(diagonals) and exp["tail_nnz"] == int(np.maximum(A.lens - w, 0).sum()) > 0, exp
            delta = A.col - A.rows
            assert set(np.unique(delta)) == set(diagonals)
            in_range = sum(int(((np.arange(A.n) + d >= 0) & (np.arange(A.n) + d < A.n)).sum()) for d in diagonals)
            assert 0.77 < len(A.col) / in_range < 0.83                # probability 0.8
            even, odd = np.arange(0, A.n - 1, 2), np.arange(1, A.n, 2)
            first = lambda r: np.where(A.lens[r] > 0, delta[np.minimum(A.ptr[r], len(delta) - 1)], 10 ** 6)
            assert np.count_nonzero(first(even) != first(odd)) > 100  # neighbouring rows: different diagonals in one ELL column
            assert np.count_nonzero(A.lens < w) > 100                 # padded rows
            assert np.any(A.rows + delta < A.rows // SLICE * SLICE)   # a column that leaves the slice
            E = with_empty_rows(A)
            assert np.all(E.lens[EMPTY_SLICE[0]:EMPTY_SLICE[1]] == 0) and np.all(E.lens[-5:] == 0) and E.lens[-6] > 0
            gone = (A.rows >= EMPTY_SLICE[0]) & (A.rows < EMPTY_SLICE[1]) | (A.rows >= A.n - 5)
            assert np.array_equal(E.col, A.col[~gone]) and np.array_equal(E.val, A.val[~gone])
            assert E.expected_storage(oracle, np.float64)["width"] in (w, w - 1)
            mats.update({A.name: A, E.name: E})
            mats[with_tail(oracle, A, w).name] = with_tail(oracle, A, w)
        for A, w in zip(unused_column_matrices(oracle, constant), (5, 7)):
            exp = A.expected_storage(oracle, np.float64)
            assert exp["width"] == w and w in UNROLLED and exp["ndeltas"] <= 254, (A.name, exp)
            used = np.bincount(A.col, minlength=A.m) > 0
            assert not used[UNUSED_AT::UNUSED_EVERY].any() and used.sum() == A.m - len(used[UNUSED_AT::UNUSED_EVERY])
            assert np.count_nonzero((A.col + 1) % UNUSED_EVERY == UNUSED_AT) > 100      # entries whose right neighbour in x is NaN
            assert np.count_nonzero((A.col - 1) % UNUSED_EVERY == UNUSED_AT) > 100      # ... and whose left neighbour is
            x = case_of(oracle, A, np.float32).x[3]
            assert np.all(np.isnan(x[~used])) and np.all(np.isfinite(x[used]))
            mats[A.name] = A
        for w, nd in DICT_DIAGONALS.items():
            A = holes_periodic(oracle, w, constant)
            d = np.arange(nd) - nd // 2
            i, k = np.meshgrid(np.arange(A.n), np.arange(nd), indexing="ij")
            keep = ((i + k) % 3 != 0) & (i + d[k] >= 0) & (i + d[k] < A.n)
            assert np.array_equal(A.col, (i + d[k])[keep]), A.name
            exp = A.expected_storage(oracle, np.float64)
            assert exp["width"] == w and exp["tail_nnz"] == 0 and exp["ndeltas"] == nd, (A.name, exp)
            assert exp["nvalues"] == (nd if constant else len(A.col)) and (constant or exp["nvalues"] > 255)
            assert (A.n + SLICE - 1) // SLICE == 65 and A.n % SLICE != 0
            mats.update({A.name: A, with_tail(oracle, A, w).name: with_tail(oracle, A, w)})
    for which in ("square", "wide"):
        A = unstructured(oracle, which)
        exp = A.expected_storage(oracle, np.float64)
        assert exp["tail_nnz"] > 0 and exp["ndeltas"] > 254 and exp["width"] == {"square": 10, "wide": 4}[which], exp
        mats[A.name] = A
    assert unstructured(oracle, "wide").m > unstructured(oracle, "wide").n

    for A in mats.values():
        _check_structure(A)
        if not A.tail_rows:
            continue
        base = mats[A.name[:-len("_tail")]]                           # the promised tail rows
        w = base.expected_storage(oracle, np.float64)["width"]
        rows, short_partner = tail_rows_of(base, w)
        assert list(A.tail_rows) == rows and 35 <= len(rows) <= 45 and A.m == base.m + EXTRA_COLS
        assert {0, A.n - 1, SLICE - 1, SLICE, short_partner} <= set(rows)
        assert short_partner % 2 == 1 and base.lens[short_partner - 1] < w
        assert np.array_equal(A.lens - base.lens, np.isin(np.arange(A.n), rows) * 3)
        extra = A.col >= base.m
        assert np.array_equal(np.flatnonzero(np.bincount(A.rows[extra], minlength=A.n)), rows) and extra.sum() == 3 * len(rows)
        assert np.array_equal(A.col[~extra], base.col) and base.col.max() < base.m
        exp = A.expected_storage(oracle, np.float64)
        assert exp["width"] == w and exp["ndeltas"] <= 254, (A.name, exp)          # the ELL part stays the band's width, still coded
        assert exp["tail_nnz"] >= base.expected_storage(oracle, np.float64)["tail_nnz"] + 3 * np.count_nonzero(base.lens[rows] >= w) > 0
        slices = {r // SLICE for r in rows}
        assert slices <= {0, 1, (A.n - 1) // SLICE - 1, (A.n - 1) // SLICE}        # the slices in between keep repeating

    for ns in (1, 2, 3, 4, 65):                                       # the hand-made strips visit every slice once; the guards are live
        visited = strip_slices(ns)
        assert np.array_equal(np.sort(visited[visited >= 0]), np.arange(ns)) and np.any(visited < 0), ns
    assert strip_geometry(65) == (96, 2, 3, 22)                       # ragged last plane (66 > 65), ragged last tile (32 > 22)

    # y_hp against a plain double loop in exact arithmetic, on the two smallest matrices (one row, two rows; 12 entries a row)
    for A in (full_band(oracle, 1, 12, False), full_band(oracle, 2, 12, False)):
        for dtype in DTYPES:
            C = case_of(oracle, A, dtype)
            ptr, col, val = A.csr(dtype)
            eps = Fraction(float(np.finfo(HP[dtype]).eps))
            for k in (0, 5):
                for mode in MODES:
                    y_hp, bound = C.high_precision(k, mode)
                    for i in range(A.n):
                        s, a = Fraction(0), Fraction(0)
                        for j in range(ptr[i], ptr[i + 1]):
                            p = _exact(val[j]) * _exact(C.x[k][col[j]])
                            s, a = s + p, a + abs(p)
                        y = Fraction(mode[0]) * s + (_exact(C.y0[k][i]) if mode[1] else 0)
                        scale = abs(Fraction(mode[0])) * a + (abs(_exact(C.y0[k][i])) if mode[1] else 0)
                        assert abs(_exact(y_hp[i]) - y) <= 16 * eps * scale, (A.name, dtype, k, mode, i)
                        g = (A.lens[i] + 2) * Fraction(UNIT[dtype])
                        assert abs(_exact(bound[i]) - g / (1 - g) * scale) <= 16 * eps * g * scale

    # the oracle within the derived bound, everywhere
    for A in mats.values():
        for dtype in DTYPES:
            C = case_of(oracle, A, dtype)
            for k in range(MAX_NRHS):
                for mode in MODES:
                    y = C.reference(oracle, k, mode)
                    assert y.dtype == dtype and np.all(np.isfinite(y)), (A.name, dtype, k, mode)
                    assert C.within_bound(y, k, mode), (A.name, np.dtype(dtype).name, k, mode)
            for mode in MODES:
                assert C.within_bound(C.reference(oracle, 2, mode, alias=True), 2, mode, alias=True)


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
    from vexcl_amd import ops
    g.ops = ops
    g.up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(g.dev)
    return g


def _even(v):
    return v + v % 2


class Vectors:
    """The right-hand sides and results of a case on the device: views at odd element offsets of two large tensors, x between
    NaN, y between sentinels."""

    def __init__(self, G, C):
        self.G, self.C = G, C
        n, m, dtype = C.mat.n, C.mat.m, C.dtype
        xs, ys = _even(m + 6), _even(n + 2 * GUARD + 2)
        self.x_at = [k * xs + 3 for k in range(MAX_NRHS)]
        self.y_at = [k * ys + GUARD + 1 for k in range(MAX_NRHS)]
        xbuf = np.full(MAX_NRHS * xs, np.nan, dtype=dtype)
        for k in range(MAX_NRHS):
            xbuf[self.x_at[k]:self.x_at[k] + m] = C.x[k]
        self.xbuf = G.up(xbuf)
        self.x = [self.xbuf[o:o + m] for o in self.x_at]
        self.start, self.start_dev = {}, {}
        for mode in MODES:
            ybuf = np.full(MAX_NRHS * ys, SENTINEL, dtype=dtype)
            for k in range(MAX_NRHS):
                ybuf[self.y_at[k]:self.y_at[k] + n] = C.y0[k] if mode[1] else np.nan
            self.start[mode], self.start_dev[mode] = ybuf, G.up(ybuf)
        size = np.dtype(dtype).itemsize
        assert self.xbuf.data_ptr() % 16 == 0 and self.start_dev[MODES[0]].data_ptr() % 16 == 0
        assert all(x.data_ptr() % size == 0 and x.data_ptr() % 16 != 0 and x.data_ptr() % (2 * size) == size for x in self.x)
        assert all(o % 2 == 1 and o >= GUARD for o in self.y_at) and ys - n >= 2 * GUARD

    def run(self, call, nrhs, mode, alias=False):
        """call(xs, ys, alpha, append) on the first nrhs vectors; returns the whole y tensor on the host."""
        n = self.C.mat.n
        ybuf = self.start_dev[mode].clone()
        ys = [ybuf[o:o + n] for o in self.y_at[:nrhs]]
        assert all(y.data_ptr() % 16 != 0 for y in ys)
        xs = list(self.x[:nrhs])
        if alias:
            assert nrhs >= 3
            xs[2] = xs[0]
        call(xs, ys, mode[0], mode[1])
        return ybuf.cpu().numpy()


def first_difference(got, want):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return "no difference" if len(bad) == 0 else "first differing row %d of %d (%d differ): got %r, want %r" % (
        bad[0], len(got), len(bad), got[bad[0]], want[bad[0]])


def check_run(oracle, V, out, nrhs, mode, what, alias=False, single=None):
    """Every result finite, equal to the oracle bit for bit (and to the single-vector products `single`), within the derived
    bound of the high-precision result; every other byte of the tensor -- sentinels, results that were not asked for -- unchanged."""
    C, n = V.C, V.C.mat.n
    rest = out.copy()
    for k in range(nrhs):
        sl = slice(V.y_at[k], V.y_at[k] + n)
        got, want = out[sl], C.reference(oracle, k, mode, alias)
        assert np.all(np.isfinite(got)), what + (k, "not finite: row %d" % np.flatnonzero(~np.isfinite(got))[0])
        assert np.array_equal(got, want), what + (k, first_difference(got, want))
        assert C.within_bound(got, k, mode, alias), what + (k, "outside the bound of the high-precision reference")
        if single is not None and not (alias and k == 2):
            assert np.array_equal(got, single[sl]), what + (k, "differs from the single-vector product", first_difference(got, single[sl]))
        rest[sl] = V.start[mode][sl]
    assert rest.tobytes() == V.start[mode].tobytes(), what + ("bytes outside the %d results changed: element %d" % (
        nrhs, np.flatnonzero(rest.view(np.uint8).reshape(len(rest), -1) != V.start[mode].view(np.uint8).reshape(len(rest), -1))[0]),)


def singles(oracle, V, apply, what):
    """The eight single-vector products of the same storage, one tensor per mode; checked like every other run."""
    out = {}
    for mode in MODES:
        out[mode] = V.run(lambda xs, ys, alpha, append: [apply(x, y, alpha, append) for x, y in zip(xs, ys)], MAX_NRHS, mode)
        check_run(oracle, V, out[mode], MAX_NRHS, mode, what + ("single", mode))
    return out


def strip_geometry(ns):
    """(grid_blocks, chunk, planes, plane_blocks) of a strip traversal over ns slices whose last plane and last tile are ragged
    where ns allows it."""
    planes = 3 if ns >= 3 else 1
    plane_blocks = (ns + planes - 1) // planes
    chunk = 2 if plane_blocks >= 4 else 1
    tiles = (plane_blocks + 8 * chunk - 1) // (8 * chunk)
    return tiles * planes * 8 * chunk, chunk, planes, plane_blocks


def strip_slices(ns):
    """The slice of every workgroup of that traversal, -1 where the workgroup returns (traversal.hpp traversal_slice restated)."""
    grid, chunk, planes, plane_blocks = strip_geometry(ns)
    b = np.arange(grid, dtype=np.int64)
    k, q = b & 7, b >> 3
    r, i = q // chunk, q % chunk
    tile, p = r // planes, r % planes
    l = tile * (8 * chunk) + k * chunk + i
    lb = p * plane_blocks + l
    return np.where((l < plane_blocks) & (lb < ns), lb, -1)


def hand_made_traversals(G, n):
    """Two traversals the set-up would not choose for matrices this small (it returns 0 blocks: plain order), so that the
    kernels' `traversal_block` runs in each of its forms: arithmetic strips, and an explicit map (the slices in reverse).  Any
    permutation of the slices is a correct traversal (include/vexhip.h); both visit every slice exactly once."""
    from vexcl_amd import _capi
    ns = (n + SLICE - 1) // SLICE
    visited = strip_slices(ns)
    assert np.array_equal(np.sort(visited[visited >= 0]), np.arange(ns)) and len(visited) == strip_geometry(ns)[0]
    order = G.up(np.arange(ns - 1, -1, -1, dtype=np.int32))
    strips = _capi.Traversal(*strip_geometry(ns), None)
    mapped = _capi.Traversal(ns, 0, 0, 0, order.data_ptr())
    return (("strips", strips), ("reversed map", mapped)), order          # (the caller keeps `order` alive)


def check_all(oracle, V, calls, nrhs, mode, what, single):
    """The first call is checked in full (check_run); every other one must leave the same bytes in the whole tensor, and says
    what differs if it does not."""
    first = None
    for name, call in calls:
        out = V.run(call, nrhs, mode)
        if first is None:
            check_run(oracle, V, out, nrhs, mode, what + (nrhs, mode, name), single=single)
            first = out
        elif out.tobytes() != first.tobytes():
            check_run(oracle, V, out, nrhs, mode, what + (nrhs, mode, name), single=single)
            raise AssertionError(what + (nrhs, mode, name, "differs from " + calls[0][0]))


def sliced_ell(G, oracle, mat, dtype, storage):
    """The storage built by the library's own set-up code, and asserted: a change in storage selection fails here."""
    ptr, col, val = mat.csr(dtype)
    S = G.ops.SlicedELL(G.up(ptr), G.up(col), G.up(val), **STORAGES[storage])
    exp = mat.expected_storage(oracle, dtype)
    got = {"width": S.width, "tail_nnz": S.tail_nnz, "ndeltas": S.ndeltas if storage != "sell32" else exp["ndeltas"],
           "nvalues": S.nvalues if storage == "sell8v" else exp["nvalues"]}
    assert got == exp, (mat.name, storage, got, exp)
    assert (S.deltas is not None) == (storage != "sell32") and (S.values is not None) == (storage == "sell8v"), (mat.name, storage)
    assert (S.csr_ptr is not None) == (exp["tail_nnz"] > 0)
    return S, exp


def check_sliced_ell(G, oracle, mat, dtype, storage, alias=False):
    S, exp = sliced_ell(G, oracle, mat, dtype, storage)
    V = Vectors(G, case_of(oracle, mat, dtype))
    what = (mat.name, storage, np.dtype(dtype).name)
    single = singles(oracle, V, S.mul, what)
    own = (S.trav, S.order_grid)
    hand_made, keep_alive = hand_made_traversals(G, mat.n)

    def through(trav, tiled):                                          # mul_multi hands on S.trav when tiled and S.order_grid > 0
        def call(xs, ys, alpha, append):
            S.trav, S.order_grid = (own if trav is None else (trav, int(trav.grid_blocks)))
            try:
                S.mul_multi(xs, ys, alpha, append, tiled=tiled)
            finally:
                S.trav, S.order_grid = own
        return call

    calls = [("the storage's traversal", through(None, True)), ("NULL traversal", through(None, False))]
    calls += [(name, through(trav, True)) for name, trav in hand_made]
    for mode in MODES:
        for nrhs in range(1, MAX_NRHS + 1):
            check_all(oracle, V, calls, nrhs, mode, what, single[mode])
            if alias and nrhs >= 3:
                out = V.run(lambda xs, ys, alpha, append: S.mul_multi(xs, ys, alpha, append), nrhs, mode, alias=True)
                check_run(oracle, V, out, nrhs, mode, what + (nrhs, mode, "x[2] is x[0]"), alias=True, single=single[mode])
    return exp


@pytest.mark.gpu
@every_dtype
@every_storage
def test_full_bands_every_width_and_ragged_size(G, oracle, storage, dtype):
    """Full bands of the unrolled widths 3, 5, 7, 9 and of 4 and 12 (loop) on n = 1, 2, 511, 512, 513 and 3 * 512 + 77 rows:
    the lane's second row, or all of a slice but its first rows, does not exist.  nrhs = 1..8, `=` and `+= alpha`."""
    widths = set()
    mats = band_matrices(oracle, storage == "sell8v")
    for mat in mats:
        exp = check_sliced_ell(G, oracle, mat, dtype, storage, alias=mat is mats[-1] or mat.n == 2 and mat.m == 4)
        assert exp["tail_nnz"] == 0
        widths.add(exp["width"])
    assert widths == set(UNROLLED + LOOPED)


@pytest.mark.gpu
@every_dtype
@every_storage
def test_bands_with_holes_tails_and_empty_rows(G, oracle, storage, dtype):
    """Random holes (ELL width 7: every branch of gather_pair -- two diagonals in one lane, one row padded, the 16-byte load
    next to a padding code -- and width 6: the loop), the same with about 40 rows of three extra entries behind the band (CSR
    tail, m = n + 8), with an empty slice and five empty last rows (widths 6 and 5), and with every eleventh column unused and
    NaN in x (widths 5 and 7): there the masked half of a 16-byte load IS NaN."""
    seen = set()
    for mat in holes_matrices(oracle, storage == "sell8v"):
        exp = check_sliced_ell(G, oracle, mat, dtype, storage, alias=bool(mat.tail_rows))
        seen.add((exp["width"] in UNROLLED, exp["tail_nnz"] > 0))
    assert seen == {(True, True), (False, True), (True, False)}


@pytest.mark.gpu
@every_dtype
def test_unstructured_matrices_with_32_bit_columns(G, oracle, dtype):
    """oracle.random_matrix 1613 x 1613 (up to 15 entries a row: width 10 and a tail) and 1613 x 2500 (width 4, non-square:
    every unused element of x is NaN) through the 32-bit-column kernel."""
    for which in ("square", "wide"):
        exp = check_sliced_ell(G, oracle, unstructured(oracle, which), dtype, "sell32", alias=which == "wide")
        assert exp["tail_nnz"] > 0 and exp["ndeltas"] > 254


def _vp(v):
    return ctypes.c_void_p(v)


@pytest.mark.gpu
@every_dtype
@pytest.mark.parametrize("storage", ("sell8", "sell8v"))
def test_dictionary_forms_through_the_entry_points_and_apply_multi(G, oracle, storage, dtype):
    """65 slices whose code blocks repeat with period 3, with and without a CSR tail: `vexhip_spmm_sell8_dict_*` (codes from
    the pool, values from the slice; widths 5, 7 and 4, 8) and `vexhip_spmm_sell8v_dict_*` (whole slices from the pool; also 9
    and 12) called with the addresses of `A.info`, traversal `&info.traversal`, NULL, hand-made strips and a hand-made map, against the
    oracle, against
    `A.apply_multi` and against `A.apply`, bit for bit."""
    torch, L = G.torch, G.L
    f64 = dtype == np.float64
    entry = getattr(L, "spmm_%s_dict_%s_i32" % (storage, "f64" if f64 else "f32"))
    real = ctypes.c_double if f64 else ctypes.c_float
    stream = ctypes.c_void_p(torch.cuda.current_stream(G.dev).cuda_stream)
    seen = set()
    for w, mat in dictionary_matrices(oracle, storage):
        ptr, col, val = mat.csr(dtype)
        dp, dc, dv = G.up(ptr), G.up(col), G.up(val)
        A = G.ops.SpMat(dp, dc, dv, n_cols=mat.m, direct=False, march=False)
        info, exp = A.info, mat.expected_storage(oracle, dtype)
        what = (mat.name, storage, np.dtype(dtype).name)
        assert A.storage == storage and not A.direct and A.march is None and A.plane is None, what + (A.storage, A.reason)
        got = {"width": int(info.ell_width), "tail_nnz": int(info.tail_nnz), "ndeltas": int(info.ndeltas),
               "nvalues": int(info.nvalues) if storage == "sell8v" else exp["nvalues"]}
        assert got == exp and exp["width"] == w, what + (got, exp)
        assert (exp["tail_nnz"] > 0) == bool(mat.tail_rows)
        assert 0 < A.dictionary_blocks <= 65 // 4 and info.slice_blocks and info.code_pool and info.deltas, what + (A.dictionary_blocks,)
        assert bool(info.values) == (storage == "sell8v") and (info.sell == info.code_pool) == (storage == "sell8v")
        assert info.rows == mat.n and bool(info.csr_ptr) == (exp["tail_nnz"] > 0)
        csr_ptr = info.csr_ptr if info.tail_nnz else None             # as apply_multi passes it
        V = Vectors(G, case_of(oracle, mat, dtype))
        single = singles(oracle, V, A.apply, what)

        def direct(trav):
            def call(xs, ys, alpha, append):
                k = len(xs)
                xp = (ctypes.c_void_p * k)(*[x.data_ptr() for x in xs])
                yp = (ctypes.c_void_p * k)(*[y.data_ptr() for y in ys])
                head = (0, stream, mat.n, k, real(alpha), int(append), w)
                tail = (_vp(info.deltas),) + ((_vp(info.values),) if storage == "sell8v" else ()) + (
                    _vp(csr_ptr), _vp(info.csr_col), _vp(info.csr_val), xp, yp, trav)
                if storage == "sell8v":
                    entry(*head, _vp(info.code_pool), _vp(info.slice_blocks), *tail)
                else:
                    entry(*head, _vp(info.sell), _vp(info.code_pool), _vp(info.slice_blocks), *tail)
            return call

        hand_made, keep_alive = hand_made_traversals(G, mat.n)
        calls = [("&info.traversal", direct(ctypes.byref(info.traversal))), ("NULL traversal", direct(None)),
                 ("apply_multi", lambda xs, ys, alpha, append: A.apply_multi(xs, ys, alpha, append))]
        calls += [(name, direct(ctypes.byref(trav))) for name, trav in hand_made]
        for mode in MODES:
            for nrhs in range(1, MAX_NRHS + 1):
                check_all(oracle, V, calls, nrhs, mode, what, single[mode])
                if nrhs in (3, 7) and mat.tail_rows:
                    out = V.run(direct(ctypes.byref(info.traversal)), nrhs, mode, alias=True)
                    check_run(oracle, V, out, nrhs, mode, what + (nrhs, mode, "x[2] is x[0]"), alias=True, single=single[mode])
        seen.add((w, exp["tail_nnz"] > 0))
        del A
    assert seen == {(w, t) for w in DICT_WIDTHS[storage] for t in (False, True)}
