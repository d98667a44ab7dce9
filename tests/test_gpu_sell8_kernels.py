"""Direct parity tests of the coded SELL-512 storages of vexcl_amd/csrc/sell8.hip -- diagonal codes (SELL8), diagonal and value codes
(SELL8V), the slice dictionary and the march product -- through the C ABI (`vexcl_amd.lib()`, `vexcl_amd._capi`) with torch tensors as
device buffers.

What runs where
  * test_analyses_*: `vexhip_sell8_analyze_i32`, `vexhip_sell8v_analyze_f64_i32` / `_f32_i32` (`collect_kernel<diagonal_keys>`,
    `collect_kernel<value_keys<V>>`, `upload_table`) against `tables()`; the limits 254 / 255 diagonals and 255 / 256 values with every row
    holding all of them (the per-workgroup check decides) and spread over the rows (only the merged set decides), more than 1024
    diagonals, the value whose bits are all ones, a matrix without entries; `analyze_fused_kernel`, which shares their `collector`,
    through `vexhip_spmat_create_*` on ordinary matrices and at the same limits.
  * test_fills_*: `vexhip_sell8_fill_*` / `vexhip_sell8v_fill_*` (`coded_fill_kernel` over the storage policies
    `stored_values<V>` / `coded_values<V>`, staged and not, `ell_max_col_kernel`) for the ELL widths 1..9 and 12 on every family of matrices below, byte for byte against `encode_sell8` /
    `encode_sell8v`; `vexhip_slice_dictionary` on the filled buffers.
  * test_products_streamed_*: `vexhip_spmv_sell8_*` and `vexhip_spmv_sell8v_*` under the variant words 0 and 1:
    `sell8_pair_kernel<W, VCODED, false>` (widths 1..8, word 0), `sell8_kernel<W>` and `sell8v_kernel<W>` (word 1; `sell8v_kernel<9>`
    under either word) and their loops (widths 9, 12 / 12), with a NULL traversal, arithmetic strips with holes, the slices in
    reverse as an explicit map and a map with a -1 in every other place, with and without a CSR tail.
  * test_products_strip_order_*: the same entries and `vexhip_spmv_sell8_dict_*` / `vexhip_spmv_sell8v_dict_*` on 47 slices with a
    NULL traversal and strips of 2 and 4 slices: `sell8_pair_kernel<3, false, DICT>`, `<7, true, DICT>`, the `blocks` branch of
    `sell8_kernel` (3, 12) and of `sell8v_kernel` (7, 9).  (`sell8_pair_kernel<W, true, true>` for W = 1, 2, 3, 7, 8 is also the
    reference of every march test.)
  * test_march_*: `vexhip_sell8_march_plan` against `march_plan_host`, its declines, and `vexhip_spmv_sell8v_march_*`
    (`sell8_march_kernel<W>`, W = 1, 2, 3, 7, 8) with `run` written into the plan.
  * test_halo_*: `sell8_pair_halo_kernel<double, W, VCODED, DICT>`, the pair product as one device's whole product step, alone in one
    process: `vexhip_spmat_create_f64_i32` with the storage pinned (SELL8 / SELL8V, no march, plane or grid plan, with and without
    a slice dictionary; checked from `vexhip_spmat_get_info` and against the encoders) on a stored strip as
    `vexcl_amd.distributed.halo_extended_csr` builds it (`Strip`, `strip_matrix`), `vexhip_dist_spmv_create_halo_pull` without a window
    and with VEXHIP_PULL_EVENTS -- no flag is raised or waited for; a VEXHIP_PULL_FLAGS plan would wait for a flag nobody raises and
    is never created here --, `vexhip_dist_spmv_apply_pull` with x and the two ghost ranges as three canaried device arrays.  All 32
    instantiations (widths 1..8, both value forms, streamed and from a dictionary); strips with one, two and three edge slices per
    side, shorter than two reaches, with a neighbour on one side only and with none; the +-1 diagonals across both seams inside one
    lane; reach equal to the ghost range; three products on one plan with the vectors rewritten in place.  The expected bits are
    `oracle.spmv_csr` on the stored matrix with x_ext = [x_below | x | x_above], own rows; without a neighbour also
    `vexhip_spmat_apply_f64` of the same handle.
  * test_generators_encoders_and_host_models (no GPU): pins everything the GPU tests take for granted.
The module has no `pytestmark`: the last test has to run without a GPU, so every GPU test carries the `gpu` mark itself.

Why the comparisons are exact
  sell8.hip is compiled with -ffp-contract=off and folds a row in CSR order -- the ELL part, then the CSR tail -- as `oracle.spmv_csr`
  does; padding adds +0 to a sum that started at +0.  Every y is compared with `np.array_equal` against the oracle in the matrix's own
  type.  The fills write every byte of their buffer, so a filled buffer is compared as bytes, whole, with the host restatement: the
  word / lane packing of include/vexhip.h ("slice layout"), the merge and the plain-packing fallback of csrc/pairing.hpp, `pad_code`
  (255: the partner's 16-byte load may cover the empty half; 254: that load would leave x), +0 (SELL8) or value code 255 (SELL8V) for
  padding, the rows behind the last one of a ragged slice as empty rows.  A wrong 254 / 255 changes no result -- the kernel replaces
  what it loaded by 0 -- it only reads outside x: nothing but this comparison sees it.

The independent check
  The oracle shares its summation order with the kernels, so every result is also held against products and row sums in np.longdouble
  (fp64) / float64 (fp32): |y - y_hp| <= g (|alpha| sum_j |a_ij x_j| + |y0_i|), g = (L+2)u / (1 - (L+2)u), L the row length, u = 2^-53 /
  2^-24: the bound of a recursive sum of L rounded products followed by one scaling and one addition.  Derived, not measured.  It
  assumes that no product underflows: where a subnormal matrix value (the value pools hold one) meets an element of x, that element
  is +-0.25 and the product is exact.

Canaries
  x is a view into a larger NaN-filled tensor and holds exactly max_col + 1 elements (max_col: the largest ELL column, which is also
  the largest column of the matrix); every element of x that no entry references is NaN, and so is everything behind x_last.  y has 64
  sentinel elements on either side, compared as bytes after every call; before a `=` call y itself holds the sentinel, so a slice that
  no workgroup visits shows.  Filled buffers, tables, dictionaries sit between guards of 64 elements.  All of these addresses lie
  inside live allocations.  The halo tests keep x (exactly the own rows) and each ghost range (exactly `halo` elements, 16-byte
  aligned) in NaN-filled tensors of their own; after every plan `timed_out` is 0.

Launch geometry
  No product is launched before `visit_once` has shown on the host that its geometry -- the traversal (`strip_visits`, a restatement
  of traversal.hpp `traversal_slice`) and, for the march product, the traversal together with `run` (`march_visits`, a restatement
  of sell8.hip `march_run`) -- visits every slice exactly once and that every other place is a hole.  For the halo role
  `halo_geometry` shows the same of `halo_visits` (the kernel's inner / lower edge / upper edge order and its short-strip rule), and
  that no workgroup reads a ghost range it is not told to need.

Left out
  `sell8v_runs_*` (reachable through vexhip_spmat only), spmm.hip; the flags of the halo role (tests/test_gpu_distributed.py); the plane
  and grid products and their plans have a file of their own, tests/test_gpu_plane_grid_kernels.py.  The `_dict` products with
  explicit maps, and `sell8_pair_kernel<W, *, true>` at the widths not named above.
  The march plan looks at diagonals and slice numbers only: that a SELL8 matrix (stored values) is not given to
  the march product is the caller's business (vexhip_spmat asks for a plan for value-coded storage only) and is not tested here.
  The plan orders diagonals of equal magnitude as std::sort leaves them; the test matrices have no diagonal set for which that order
  decides anything (`march_plan_host` checks both orders), and their far diagonals differ in magnitude.  `run` depends on the
  device's CU count: every test writes its own.

The variant word is process-wide: it is set inside `try` and put back to 0 in `finally`."""
import contextlib
import ctypes
import zlib

import numpy as np
import pytest

gpu = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
HP = {np.float64: np.longdouble, np.float32: np.float64}          # the type of the independent reference
UNIT = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
BITS = {np.float64: np.uint64, np.float32: np.uint32}
MODES = ((1.0, False), (-0.75, True))                             # (alpha, append)
GUARD = 64                                                        # sentinel elements on either side of every y and every written buffer
SENTINEL = 12345.0
SLACK = 8                                                         # col / val entries behind ptr[n]
INT_MAX = 2 ** 31 - 1

SLICE, PAD, PAD_UNSAFE = 512, 255, 254
WAVE_CAP, HASH_SLOTS = 1024, 1024
SIZES = (1, 2, 511, 512, 513, 3 * 512 + 77)
N13, N47 = 12 * 512 + 77, 46 * 512 + 77                           # 13 and 47 slices, the last one ragged
WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12)
FEW_WIDTHS = (1, 3, 8, 12)                                        # products at the sizes below 513; the analyses
FAMILIES = ("bands", "holes", "crossed", "tails", "long_row", "unsorted", "empty", "pools", "wide", "narrow")
LONG_ROW = 1500
LEAD = 5                                                          # ptr[0] of the `empty` family's second run
MARCH_RUNS = (1, 2, 3, 5, 13, 64)
STRIPS47 = {2: (80, 2, 5, 10), 4: (160, 4, 5, 10)}                # chunk -> (grid_blocks, chunk, planes, plane_blocks) over 47 slices

SUB32, SUB64 = 2.0 ** -140, 2.0 ** -1060                          # subnormal in float32 / in float64 (which float32 rounds to +0)

every_dtype = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
every_family = pytest.mark.parametrize("fam", FAMILIES)


# ---------------------------------------------------------------------------------------------------------------------------
# matrices: CSR with ptr[0] = 0; the values of a matrix come in several schemes, kept in float64 and rounded to the type under test
# ---------------------------------------------------------------------------------------------------------------------------
def pool_values(k):
    """k distinct float64 values: 3 and 255 with -0.0 and a float32 subnormal, 255 with +0.0 and a float64 subnormal too; 5 and 7
    (the schemes of the other families) without a subnormal, 7 with both zeros."""
    if k == 1:
        return np.array([-1.25])
    if k in (5, 7):
        return np.array([0.625, -1.25, 0.3125, 1.5, -0.875, -0.0, 0.0][:k])
    head = [0.625, -0.0, SUB32] if k < 255 else [0.0, -0.0, SUB32, SUB64]
    j = np.arange(k - len(head))
    return np.concatenate([head, (j + 3) / 512.0 * np.where(j % 2 == 0, 1.0, -1.0)])       # (exact in float32)


VALUE_SCHEMES = {"pool1": (1, 5, 3), "pool3": (3, 5, 3), "pool255": (255, 5, 3), "hash7": (7, 5, 3), "diag5": (5, 0, 1)}   # pool size, row and entry multiplier


class Mat:
    def __init__(self, oracle, name, n, ptr, col, kidx):
        self.o, self.name, self.n = oracle, name, int(n)
        self.ptr = np.ascontiguousarray(ptr, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.kidx = np.ascontiguousarray(kidx, dtype=np.int64)         # which diagonal of its generator an entry is (extras: beyond them)
        self.m = int(self.col.max()) + 1 if len(self.col) else 1        # x holds exactly this many elements
        self.lens = np.diff(self.ptr.astype(np.int64))
        self.rows = np.repeat(np.arange(self.n, dtype=np.int64), self.lens)
        self.pos = np.arange(len(self.col), dtype=np.int64) - np.repeat(self.ptr[:-1].astype(np.int64), self.lens)
        self._val, self._slots, self.part_of = {}, {}, None              # part_of: (matrix, mask) of a matrix cut out of another one

    def values(self, scheme):
        if scheme not in self._val:
            if self.part_of is not None:
                v = self.part_of[0].values(scheme)[self.part_of[1]]
            elif scheme == "random":
                v = self.o.random_f64(zlib.crc32(self.name.encode()) % 100000, max(1, len(self.col)))[:len(self.col)] - 0.5
            else:
                k, a, b = VALUE_SCHEMES[scheme]
                v = pool_values(k)[(self.rows * a + self.kidx * b) % k]
            self._val[scheme] = np.ascontiguousarray(v, dtype=np.float64)
        return self._val[scheme]

    def csr(self, dtype, scheme):
        return self.ptr, self.col, np.ascontiguousarray(self.values(scheme).astype(dtype))

    def max_col(self, w):
        ell = self.pos < w
        return int(self.col[ell].max()) if ell.any() else -1

    def slots(self, w):
        """`pair_slots` of the ELL part at width w (the layout does not depend on the values)."""
        if w not in self._slots:
            self._slots[w] = pair_slots(self.ptr, self.col, w, self.max_col(w))
        return self._slots[w]


_MATS = {}


def _cached(name, make):
    if name not in _MATS:
        _MATS[name] = make()
        assert _MATS[name].name == name
    return _MATS[name]


def assemble(oracle, name, n, diags, keep, mcut, extras=None, shuffle=None):
    """Row i holds the columns i + diags[i, k] (diags: (nd,) or (n, nd)) where keep[i, k] and 0 <= column < mcut, in ascending k;
    extras(lens, m) -> (rows, columns) appended behind the rows' entries; shuffle: a seed -- column order shuffled inside the rows."""
    i = np.arange(n, dtype=np.int64)[:, None]
    diags = np.asarray(diags, dtype=np.int64)
    cols = i + (diags if diags.ndim == 2 else diags[None, :])
    ok = np.broadcast_to(keep, cols.shape) & (cols >= 0) & (cols < mcut)
    rows, col = np.broadcast_to(i, cols.shape)[ok], cols[ok]
    kidx = np.broadcast_to(np.arange(cols.shape[1])[None, :], cols.shape)[ok]
    key = np.arange(len(col), dtype=np.float64)
    if extras is not None and len(col):
        xr, xc = extras(ok.sum(axis=1), int(col.max()) + 1)
        rows, col = np.concatenate([rows, xr]), np.concatenate([col, xc])
        kidx = np.concatenate([kidx, cols.shape[1] + np.arange(len(xr))])
        key = np.concatenate([key, 1e9 + np.arange(len(xr))])
    if shuffle is not None:
        key = oracle.random_f64(shuffle, max(1, len(col)))[:len(col)]
    order = np.lexsort((key, rows))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return Mat(oracle, name, n, ptr, col[order], kidx[order])


def band(w):
    """w diagonals around 0: -1, 0, 1 adjacent, the others three apart."""
    k = np.arange(w) - w // 2
    return np.where(np.abs(k) <= 1, k, 3 * k)


def tail_extras(w, long_row=False):
    """Entries behind the ELL part of rows that hold exactly w entries (so they are a tail and their diagonals are never coded):
    1..3 in every fifth such row, or LONG_ROW in one row (row 300 where it is such a row)."""
    def extras(lens, m):
        full = np.flatnonzero(lens == w)
        if long_row:
            full = full[np.argmin(np.abs(full - 300))][None] if len(full) else full
            count = np.full(len(full), LONG_ROW)
        else:
            full = full[full % 5 == 2]
            count = 1 + full % 3
        rows = np.repeat(full, count)
        e = np.arange(len(rows)) - np.repeat(np.cumsum(count) - count, count)
        return rows, (rows * 7 + 13 * e) % m
    return extras


def family(oracle, fam, n, w):
    """bands: w full diagonals; every interior pair is `same`; the band leaves the matrix in the first and the last rows (254 next to
    column 0 and next to max_col).  holes: diagonals kept with probability 0.8 (merged pairs, 255).  crossed: two pairs in three hold
    the diagonals 4k in the even and 4k + 2 in the odd row: the merged list exceeds w, plain packing, two diagonals in one lane.
    tails / long_row: a band with entries behind the ELL part; the 1500 of long_row push one wave's piece beyond WAVE_CAP.  unsorted:
    holes with the column order shuffled inside the rows.  empty: leading empty rows, empty rows among full ones, rows 512..1023
    empty.  pools: a band for the value schemes pool1 / pool3 / pool255.  wide: max_col > n - 1 (columns behind the band); narrow:
    max_col < n - 1 (from 16 rows on)."""
    name = "%s_n%d_w%d" % (fam, n, w)

    def make():
        D, i = band(w), np.arange(n, dtype=np.int64)
        keep, mcut, extras, shuffle = np.ones((n, w), dtype=bool), n, None, None
        seed = 3000 + 97 * w + n % 89
        if fam in ("holes", "unsorted"):
            keep = oracle.random_f64(seed, n * w).reshape(n, w) < 0.8
            keep[0, w // 2] = True
            shuffle = seed + 1 if fam == "unsorted" else None
        elif fam == "crossed":
            k = np.arange(w)
            D = np.where((((i // 2) % 3 != 0) & (i % 2 == 1))[:, None], (4 * k + 2)[None, :], (4 * k)[None, :])
            mcut = n + 4 * w + 3
        elif fam in ("tails", "long_row"):
            extras = tail_extras(w, fam == "long_row")
        elif fam == "empty":
            lead = min(130, n // 2)
            rows = (i >= lead) & (i % 3 != 1) & ~((i >= 512) & (i < 1024))
            rows[n - 1] = True
            keep = keep & rows[:, None]
        elif fam == "wide":
            D, mcut = D + 3 * (w // 2) + 2, n + 6 * w + 8
        elif fam == "narrow" and n >= 16:
            D = D - 3 * (w // 2) - 7
        else:
            assert fam in ("bands", "pools", "narrow"), fam
        return assemble(oracle, name, n, D, keep, mcut, extras, shuffle)
    return _cached(name, make)


def diag_matrix(oracle, name, n, diagonals, mcut=None, tails=True):
    """The given diagonals in every row that reaches a column (0 <= column < mcut, default n), one value per diagonal under the
    scheme diag5 -- the slices repeat --, and a CSR tail in every fifth full row."""
    w = len(diagonals)
    return _cached(name, lambda: assemble(oracle, name, n, np.asarray(diagonals), np.ones((n, w), dtype=bool), mcut or n,
                                          tail_extras(w) if tails else None))


MARCH_SETS = {                                                       # name -> (diagonals, columns behind the band)
    "w1": ((0,), 0),                                                 # no far diagonal, x_last = n - 1
    "w2": ((-2048, -3), 0),                                          # one far diagonal, x_last = n - 4 < n - 1
    "w3": ((0, 1, 2560), 2560),                                      # one far diagonal, x_last > n - 1
    "w7": ((-2048, -600, -1, 0, 1, 600, 2560), 2560),                # two, a near window of three slices: the ring wraps
    "w8": ((-2048, -700, -1, 0, 1, 2, 700, 2560), 2560),
}
MARCH_EXPECT = {"w1": (0, 0, []), "w2": (-3, 0, [-2048]), "w3": (0, 1, [2560]), "w7": (-600, 600, [-2048, 2560]),
                "w8": (-700, 700, [-2048, 2560])}                    # lo, hi, far
MARCH_W9 = (-2048, -700, -1, 0, 1, 2, 3, 700, 2560)


def march_matrix(oracle, which, n=N13):
    D, behind = MARCH_SETS[which] if which in MARCH_SETS else (MARCH_W9, 2560)
    return diag_matrix(oracle, "march_%s_n%d" % (which, n), n, D, n + behind)


def dict_matrix(oracle, w, n=N13):
    return diag_matrix(oracle, "dict_n%d_w%d" % (n, w), n, band(w))


def truncated(mat, w):
    """The first w entries of every row: the ELL part alone, a matrix without a tail and with the same storage."""
    name = mat.name + "_first%d" % w

    def make():
        keep = mat.pos < w
        cut = Mat(mat.o, name, mat.n, np.concatenate([[0], np.cumsum(np.minimum(mat.lens, w))]), mat.col[keep], mat.kidx[keep])
        cut.part_of = (mat, keep)
        return cut
    return _cached(name, make)


def fill_schemes(fam):
    """[(storage, value scheme)] a family is filled with."""
    if fam == "pools":
        return [("sell8v", "pool1"), ("sell8v", "pool3"), ("sell8v", "pool255"), ("sell8", "pool3")]
    return [("sell8", "random"), ("sell8v", "hash7")]


def product_widths(n):
    return WIDTHS if n >= 513 else FEW_WIDTHS


# ---------------------------------------------------------------------------------------------------------------------------
# host restatements: tables, tail, pair placement, the two encoders and their inverse
# ---------------------------------------------------------------------------------------------------------------------------
def tables(ptr, col, val, w):
    """(sorted diagonals, values sorted by bit pattern as unsigned integers, largest column) of the first w entries of every row."""
    p = ptr.astype(np.int64)
    lens = np.diff(p)
    rows = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    ell = np.arange(p[0], p[-1]) - np.repeat(p[:-1], lens) < w
    c, v = col[p[0]:p[-1]][ell].astype(np.int64), val[p[0]:p[-1]][ell]
    bits = np.unique(np.ascontiguousarray(v).view(BITS[v.dtype.type]))
    return np.unique(c - rows[ell]), bits, (int(c.max()) if len(c) else -1)


def split_tail(ptr, col, val, w):
    """The CSR tail the products are given: the entries from position w on of every row (ptr[0] = 0)."""
    lens = np.diff(ptr.astype(np.int64))
    pos = np.arange(ptr[-1], dtype=np.int64) - np.repeat(ptr[:-1].astype(np.int64), lens)
    tp = np.concatenate([[0], np.cumsum(np.maximum(lens - w, 0))]).astype(np.int32)
    return tp, np.ascontiguousarray(col[pos >= w]), np.ascontiguousarray(val[pos >= w])


def pair_slots(ptr, col, w, max_col):
    """csrc/pairing.hpp restated.  ent[r, j]: the CSR entry in ELL column j of row r (-1: none) for the ns * 512 rows of the storage
    (the rows behind the last one are empty); pad[r, j]: the code of an empty place -- 255, or 254 where the place's partner holds
    column c in row half q and x[c - q], x[c - q + 1] is not inside x[0 .. max_col] --; kinds: pairs with entries that are `same` (equal
    diagonal lists), merged otherwise, plain-packed."""
    n = len(ptr) - 1
    R = (n + SLICE - 1) // SLICE * SLICE
    ent, pad = np.full((R, w), -1, dtype=np.int64), np.full((R, w), PAD, dtype=np.uint8)
    kinds = {"same": 0, "merged": 0, "plain": 0}
    # pairs whose rows hold the same diagonals in the same order, all at once: entry k of both in column k, as the merge places them
    p64, c64 = ptr.astype(np.int64), col.astype(np.int64)
    lens_w = np.concatenate([np.minimum(np.diff(p64), w), [0]])
    begin = np.concatenate([p64[:-1], [0]])
    even = np.arange(0, n, 2)
    cand = even[(lens_w[even] == lens_w[even + 1]) & (lens_w[even] > 0)]
    count = lens_w[cand]
    which = np.repeat(np.arange(len(cand)), count)
    k = np.arange(len(which)) - np.repeat(np.cumsum(count) - count, count)
    e0, e1 = begin[cand][which] + k, begin[cand + 1][which] + k
    differ = np.bincount(which[c64[e0] + 1 != c64[e1]], minlength=len(cand)) > 0
    ok = ~differ[which]
    ent[cand[which][ok], k[ok]], ent[cand[which][ok] + 1, k[ok]] = e0[ok], e1[ok]
    kinds["same"] = int(np.count_nonzero(~differ))
    done = np.zeros(n + 1, dtype=bool)
    done[cand[~differ]] = True
    p, c = p64.tolist(), col.tolist()
    for r0 in np.flatnonzero(~done[:n:2]) * 2:
        r0 = int(r0)
        b0, b1, n1 = p[r0], 0, 0
        n0 = min(p[r0 + 1] - b0, w)
        if r0 + 1 < n:
            b1 = p[r0 + 1]
            n1 = min(p[r0 + 2] - b1, w)
        if n0 == 0 and n1 == 0:
            continue
        d0, d1 = [c[b0 + k] - r0 for k in range(n0)], [c[b1 + k] - r0 - 1 for k in range(n1)]
        pa = pb = merged = 0
        while pa < n0 or pb < n1:                                     # pair_merge::init
            if pa < n0 and pb < n1:
                if d0[pa] == d1[pb]:
                    pa += 1
                    pb += 1
                elif d0[pa] < d1[pb]:
                    pa += 1
                else:
                    pb += 1
            elif pa < n0:
                pa += 1
            else:
                pb += 1
            merged += 1
        aligned = merged <= w
        kinds["same" if d0 == d1 else "merged" if aligned else "plain"] += 1
        pa = pb = 0
        for j in range(w):                                            # pair_merge::next
            k0 = k1 = -1
            h0, h1 = pa < n0, pb < n1
            if not aligned:
                if h0:
                    k0, pa = pa, pa + 1
                if h1:
                    k1, pb = pb, pb + 1
            elif h0 and h1:
                da, db = d0[pa], d1[pb]
                if da <= db:
                    k0, pa = pa, pa + 1
                if db <= da:
                    k1, pb = pb, pb + 1
            elif h0:
                k0, pa = pa, pa + 1
            elif h1:
                k1, pb = pb, pb + 1
            if k0 >= 0:
                ent[r0, j] = b0 + k0
                if k1 < 0:
                    first = c[b0 + k0]                                # the partner is half 0: its load starts at its own column
                    pad[r0 + 1, j] = PAD if first >= 0 and first + 1 <= max_col else PAD_UNSAFE
            if k1 >= 0:
                ent[r0 + 1, j] = b1 + k1
                if k0 < 0:
                    first = c[b1 + k1] - 1
                    pad[r0, j] = PAD if first >= 0 and first + 1 <= max_col else PAD_UNSAFE
    return ent, pad, kinds


def pack_codes(codes):
    """(ns * 512, w) bytes -> (ns, ceil(w/2) * 1024): word [jp][t] = {(2jp, 2t), (2jp, 2t+1), (2jp+1, 2t), (2jp+1, 2t+1)}; the column
    behind an odd w is 255."""
    R, w = codes.shape
    ns, wp = R // SLICE, (w + 1) // 2
    full = np.full((ns, SLICE // 2, 2, 2 * wp), PAD, dtype=np.uint8)                       # [slice][t][q][j]
    full[..., :w] = codes.reshape(ns, SLICE // 2, 2, w)
    return np.ascontiguousarray(full.reshape(ns, SLICE // 2, 2, wp, 2).transpose(0, 3, 1, 4, 2)).reshape(ns, wp * 1024)   # [slice][jp][t][jj][q]


def unpack_codes(block, w):
    ns, wp = block.shape[0], (w + 1) // 2
    full = block.reshape(ns, wp, SLICE // 2, 2, 2).transpose(0, 2, 4, 1, 3)                  # [slice][t][q][jp][jj]
    return np.ascontiguousarray(full).reshape(ns * SLICE, 2 * wp)[:, :w]


def _coded(ptr, col, w, deltas, max_col, slots):
    ent, pad, _ = slots if slots is not None else pair_slots(ptr, col, w, max_col)
    real = ent >= 0
    e = np.maximum(ent, 0)
    diag = col.astype(np.int64)[e] - np.arange(ent.shape[0], dtype=np.int64)[:, None] if len(col) else np.zeros_like(ent)
    code = np.searchsorted(deltas, diag)
    assert len(deltas) <= PAD_UNSAFE and np.all(np.asarray(deltas)[np.minimum(code, len(deltas) - 1)][real] == diag[real]), "a diagonal is not in the table"
    return real, e, np.where(real, code, pad).astype(np.uint8)


def encode_sell8(ptr, col, val, w, deltas, max_col, dtype, slots=None):
    """The whole SELL8 buffer (`vexhip_sell8_bytes`) as bytes: per slice ceil(w/2) KiB of codes, then w * 512 values, j-major."""
    real, e, codes = _coded(ptr, col, w, deltas, max_col, slots)
    ns = codes.shape[0] // SLICE
    v = np.where(real, val.astype(dtype)[e] if len(val) else dtype(0), dtype(0)).astype(dtype)          # padding: +0
    vals = np.ascontiguousarray(v.reshape(ns, SLICE, w).transpose(0, 2, 1)).reshape(ns, -1)
    return np.concatenate([pack_codes(codes), vals.view(np.uint8).reshape(ns, -1)], axis=1).reshape(-1)


def encode_sell8v(ptr, col, val, w, deltas, max_col, dtype, values, slots=None):
    """The whole SELL8V buffer (`vexhip_sell8v_bytes`): per slice ceil(w/2) KiB of diagonal codes, then as many of value codes (255
    for padding).  values: the table, bit patterns as unsigned integers, ascending."""
    real, e, codes = _coded(ptr, col, w, deltas, max_col, slots)
    bits = np.ascontiguousarray(val.astype(dtype)).view(BITS[dtype])[e] if len(val) else np.zeros_like(e, dtype=BITS[dtype])
    vc = np.searchsorted(values, bits)
    assert len(values) <= PAD and np.all(np.asarray(values)[np.minimum(vc, len(values) - 1)][real] == bits[real]), "a value is not in the table"
    return np.concatenate([pack_codes(codes), pack_codes(np.where(real, vc, PAD).astype(np.uint8))], axis=1).reshape(-1)


def decode(buf, n, w, deltas, dtype, values=None):
    """(columns, values) of the real entries of a buffer, row after row in ELL column order: the inverse of the encoders."""
    ns, wp = (n + SLICE - 1) // SLICE, (w + 1) // 2
    sl = np.asarray(buf, dtype=np.uint8).reshape(ns, -1)
    codes = unpack_codes(sl[:, :wp * 1024], w)
    real = codes < PAD_UNSAFE
    cols = np.arange(ns * SLICE, dtype=np.int64)[:, None] + np.asarray(deltas, dtype=np.int64)[np.minimum(codes, len(deltas) - 1)]
    if values is None:
        vals = np.ascontiguousarray(sl[:, wp * 1024:]).view(dtype).reshape(ns, w, SLICE).transpose(0, 2, 1).reshape(ns * SLICE, w)
        assert np.all(vals[~real].view(BITS[dtype]) == 0)                                  # +0, not -0
    else:
        vc = unpack_codes(sl[:, wp * 1024:], w)
        assert np.all(vc[~real] == PAD)
        vals = np.asarray(values).view(dtype)[np.minimum(vc, len(values) - 1)]
    return cols[real], vals[real]


def first_appearance(blocks):
    """(number of every row of `blocks` in order of first appearance, the rows that introduce a number)."""
    seen, ids, reps = {}, [], []
    for s in range(blocks.shape[0]):
        key = blocks[s].tobytes()
        if key not in seen:
            seen[key] = len(reps)
            reps.append(s)
        ids.append(seen[key])
    return np.array(ids, dtype=np.int32), reps


# ---------------------------------------------------------------------------------------------------------------------------
# host models of the launch geometry and of the march plan
# ---------------------------------------------------------------------------------------------------------------------------
def strip_visits(grid, chunk, planes, plane_blocks, nb):
    """traversal.hpp traversal_slice, strip form: the slice of every workgroup, -1 where it returns."""
    b = np.arange(grid, dtype=np.int64)
    k, q = b & 7, b >> 3
    r, i = q // chunk, q % chunk
    tile, p = r // planes, r % planes
    l = tile * (8 * chunk) + k * chunk + i
    lb = p * plane_blocks + l
    return np.where((l < plane_blocks) & (lb < nb), lb, -1)


def strip_geometry(nb):
    """(grid_blocks, chunk, planes, plane_blocks) of hand-made strips with holes (8 * chunk > plane_blocks) and a ragged last plane
    where nb allows it."""
    planes = 2 if nb >= 8 else 3 if nb >= 3 else 1
    plane_blocks = (nb + planes - 1) // planes
    chunk = 2 if plane_blocks >= 4 else 1
    tiles = (plane_blocks + 8 * chunk - 1) // (8 * chunk)
    return tiles * planes * 8 * chunk, chunk, planes, plane_blocks


def holey_map(nb):
    m = np.full(2 * nb + 3, -1, dtype=np.int32)
    m[1:2 * nb:2] = np.arange(nb - 1, -1, -1)
    return m


def march_visits(nb, run, strips=None):
    """sell8.hip march_run and march_launch's grid: the slices of every workgroup one after the other, -1 for a workgroup without
    any (a hole of the strip order)."""
    out = []
    if strips is None:
        grid = (nb + run - 1) // run
        runs = [(mb * run, min(run, nb - mb * run)) for mb in range(grid)]
    else:
        grid_blocks, chunk, planes, plane_blocks = strips
        assert chunk % run == 0 and grid_blocks % run == 0
        runs, rpc = [], chunk // run
        for mb in range(grid_blocks // run):
            k, q = mb & 7, mb >> 3
            r, ri = q // rpc, q % rpc
            tile, p = r // planes, r % planes
            l = tile * (8 * chunk) + k * chunk + ri * run
            first = p * plane_blocks + l
            runs.append((first, min(run, plane_blocks - l, nb - first)))
    for first, count in runs:
        out.extend(range(first, first + count) if count > 0 else [-1])
    return np.array(out, dtype=np.int64), runs


def visit_once(visited, nb):
    """Every slice of [0, nb) exactly once, every other entry -1, nothing >= nb: what a launch geometry must satisfy."""
    visited = np.asarray(visited, dtype=np.int64)
    real = visited[visited >= 0]
    return bool(len(real) == nb and np.array_equal(np.sort(real), np.arange(nb)) and np.all(visited[visited < 0] == -1)
                and len(visited) < 2 ** 31)


def march_span_bytes(lo, hi, vb):
    """Bytes of x the near diagonals lo..hi cover, on even elements, rounded up to whole slices."""
    slb = SLICE * vb
    return ((((hi + 1) & ~1) - (lo & ~1)) * vb + slb - 1) // slb * slb


def march_lds_bytes(lo, hi, vb):
    """Ring (span + 2 slices) + mirror (span) + two far slots + the diagonal and value tables."""
    return 2 * march_span_bytes(lo, hi, vb) + 4 * SLICE * vb + 1024 + 256 * vb


def march_plan_host(deltas, blocks, value_bytes, x_last, explicit_order=False):
    """include/vexhip.h on vexhip_sell8_march_plan: None where it declines, else (lo, hi, far)."""
    deltas, ns = [int(d) for d in deltas], len(blocks)
    if not 1 <= len(deltas) <= 254 or ns < 8 or x_last < 0 or explicit_order:
        return None
    if 2 * int(np.count_nonzero(np.diff(np.asarray(blocks)))) > ns:
        return None
    plans = []
    for tie in (1, -1):                                               # diagonals of equal magnitude in either order
        lo = hi = 0
        by_abs = sorted(deltas, key=lambda d: (abs(d), tie * d))
        for d in by_abs:
            nlo, nhi = min(lo, d), max(hi, d)
            if nhi - nlo > 1 << 20 or march_lds_bytes(nlo, nhi, value_bytes) > 48 * 1024:
                break
            if march_span_bytes(nlo, nhi, value_bytes) // value_bytes + SLICE > 2048:
                break
            lo, hi = nlo, nhi
        plans.append((lo, hi, [d for d in by_abs if d < lo or d > hi]))
    if len(plans[0][2]) > 2 and len(plans[1][2]) > 2:
        return None                                                   # a third far diagonal
    assert plans[0] == plans[1], "the order of diagonals of equal magnitude decides: not a test matrix"
    return plans[0]


# ---------------------------------------------------------------------------------------------------------------------------
# right-hand side, start vector and references of one matrix in one type, computed once and shared by every test
# ---------------------------------------------------------------------------------------------------------------------------
def segment_sums(a, ptr):
    lens = np.diff(ptr.astype(np.int64))
    out = np.zeros(len(lens), dtype=a.dtype)
    full = lens > 0
    if full.any():
        out[full] = np.add.reduceat(a, ptr[:-1].astype(np.int64)[full])
    return out


class Case:
    def __init__(self, oracle, mat, dtype, scheme, salt=0):
        self.mat, self.dtype, self.scheme = mat, dtype, scheme
        ptr, col, val = mat.csr(dtype, scheme)
        used = np.zeros(mat.m, dtype=bool)
        used[col] = True
        seed = 1000 + 17 * mat.n + 3 * mat.m + len(mat.col) % 1000 + 7919 * salt    # salt: further vectors for the same matrix
        self.x = (oracle.random_f64(seed, mat.m) - 0.5).astype(dtype)
        tiny = (val != 0) & (np.abs(val) < np.finfo(dtype).tiny)
        self.x[col[tiny]] = np.copysign(dtype(0.25), self.x[col[tiny]])   # a subnormal value meets a power of two: its product is exact (the bound assumes no underflow)
        self.x[~used] = np.nan                                        # no entry reads these
        self.y0 = (oracle.random_f64(seed + 50, mat.n) - 0.5).astype(dtype)
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
            ptr, col, val = self.mat.csr(self.dtype, self.scheme)
            y = self.y0.copy() if append else np.full(self.mat.n, SENTINEL, dtype=self.dtype)
            self._ref[mode] = oracle.spmv_csr(ptr, col, val, self.x, y, alpha, append)
        return self._ref[mode]

    def within_bound(self, y, mode):
        alpha, append = mode
        hp = HP[self.dtype]
        y_hp, scale = hp(alpha) * self.sum, hp(abs(alpha)) * self.abs_sum
        if append:
            y_hp, scale = y_hp + self.y0.astype(hp), scale + np.abs(self.y0.astype(hp))
        return bool(np.all(np.abs(y.astype(hp) - y_hp) <= self.gamma * scale))


_CASES = {}


def case_of(oracle, mat, dtype, scheme, salt=0):
    key = (mat.name, np.dtype(dtype).name, scheme) + ((salt,) if salt else ())
    if key not in _CASES:
        _CASES[key] = Case(oracle, mat, dtype, scheme, salt)
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------------------
# the halo role of the pair product: stored strips, their matrices, the kernel's block-to-slice mapping
# ---------------------------------------------------------------------------------------------------------------------------
class Strip:
    """One device's strip as vexcl_amd.distributed.halo_extended_csr stores it: `lo` empty rows in front of the own rows where there
    is a lower neighbour, `hi` empty rows behind them where there is an upper one (a ghost range of `halo` rows each), columns counted
    from the first element of the lower ghost range.  reach: the largest |diagonal| of its matrices."""

    def __init__(self, name, halo, rows, lower, upper, reach):
        self.name, self.halo, self.rows, self.lower, self.upper, self.reach = name, halo, rows, lower, upper, reach
        self.lo, self.hi = halo * lower, halo * upper
        self.n = self.lo + rows + self.hi                               # rows (and columns) of the stored matrix
        self.ns, self.edge = rows // SLICE, (reach + SLICE - 1) // SLICE
        assert rows % SLICE == 0 and halo % SLICE == 0 and rows % halo == 0 and 0 < reach <= halo

    def own(self, a):
        return a[self.lo:self.lo + self.rows]


STRIPS = {s.name: s for s in (
    Strip("seams", 512, 4 * 512, True, True, 1),                      # the +-1 diagonals straddle both seams inside one lane
    Strip("reach_is_halo", 512, 4 * 512, True, True, 512),            # pairs of the inner slices end at the last own element; the ghost ranges' first and last elements
    Strip("edge2", 1024, 4 * 1024, True, True, 513),                  # two edge slices per side, four inner ones
    Strip("short513", 1024, 1024, True, True, 513),                   # ns < 2 edge: every slice needs both ghost ranges
    Strip("short1024", 1024, 1024, True, True, 1024),
    Strip("edge3", 1536, 1536, True, True, 1025),                     # edge = ns = 3
    Strip("lower", 512, 4 * 512, True, False, 512),                   # x and y moved by the lower ghost range
    Strip("upper", 512, 4 * 512, False, True, 512),                   # ... and not moved
    Strip("alone", 512, 4 * 512, False, False, 512),                  # every slice inner: the plain pair product
    Strip("dict", 512, 64 * 512, True, True, 512),                    # 66 stored slices that repeat: the DICT forms
)}
HALO_FAMILIES = ("bands", "holes", "crossed")
PULL_EVENTS = 2                                                       # VEXHIP_PULL_EVENTS (include/vexhip.h): the only order a one-process test may ask for
HALO_EXPECT = {                                                       # per workgroup: (own slice, needs the lower, the upper ghost range)
    "seams": [(1, False, False), (2, False, False), (0, True, False), (3, False, True)],
    "reach_is_halo": [(1, False, False), (2, False, False), (0, True, False), (3, False, True)],
    "edge2": [(2, False, False), (3, False, False), (4, False, False), (5, False, False), (0, True, False), (1, True, False), (6, False, True), (7, False, True)],
    "short513": [(0, True, True), (1, True, True)],
    "short1024": [(0, True, True), (1, True, True)],
    "edge3": [(0, True, True), (1, True, True), (2, True, True)],
    "lower": [(1, False, False), (2, False, False), (3, False, False), (0, True, False)],
    "upper": [(0, False, False), (1, False, False), (2, False, False), (3, False, True)],
    "alone": [(0, False, False), (1, False, False), (2, False, False), (3, False, False)],
    "dict": [(s, False, False) for s in range(1, 63)] + [(0, True, False), (63, False, True)],
}


def halo_visits(ns, edge, has_lo, has_hi):
    """sell8.hip sell8_pair_halo_kernel, workgroup -> (own slice, need_lo, need_hi): the inner slices first, then the lower edge, then
    the upper edge; in a strip shorter than two reaches a slice may need both ghost ranges."""
    elo = min(edge, ns) if has_lo else 0
    ehi = min(edge, ns - elo) if has_hi else 0
    inner = ns - elo - ehi
    out = []
    for b in range(ns):
        need_lo = need_hi = False
        if b < inner:
            so = b + elo
        elif b < inner + elo:
            so, need_lo = b - inner, True
        else:
            so, need_hi = ns - ehi + (b - inner - elo), True
        if has_lo and has_hi and ns < 2 * edge:
            need_lo, need_hi = need_lo or so < edge, need_hi or so >= ns - edge
        out.append((so, need_lo, need_hi))
    return out


def halo_diagonals(fam, w, reach):
    """(diagonals of the even rows, of the odd rows), ascending, the largest magnitude `reach`.  crossed: the odd rows' are the even
    rows' + 2 -- disjoint sets, so a pair's merged list exceeds w."""
    if reach == 1:
        assert w <= (1 if fam == "crossed" else 3)
        return (np.array([-1]), np.array([1])) if fam == "crossed" else (np.sort([-1, 1, 0][:w]),) * 2
    assert reach >= 16
    if fam == "crossed":
        even = np.sort([-reach, reach - 2, 0, -4, 4, -8, 8, 12][:w])
        return even, even + 2
    return (np.sort([-reach, reach, 0, -1, 1, -3, 3, 6][:w]),) * 2


def strip_matrix(oracle, strip, fam, w):
    """The stored matrix of a strip, one of three of the file's families with the strip's reach.  bands: every own row holds the w
    diagonals (pairs on one diagonal).  holes: every third row keeps a diagonal with probability 0.8, the same rows in every slice
    (255 / 254 beside an entry; more than a third of all stored rows stay full: no CSR tail).  crossed: in two pairs of three the odd
    row holds other diagonals than the even one (plain packing: two diagonals in one lane).  The ghost rows are empty; a diagonal
    that leaves the stored columns (no neighbour on that side) is cut."""
    name = "strip_%s_%s_w%d" % (strip.name, fam, w)

    def make():
        i = np.arange(strip.n, dtype=np.int64)
        even, odd = halo_diagonals(fam, w, strip.reach)
        D = np.where((((i // 2) % 3 != 0) & (i % 2 == 1))[:, None], odd[None, :], even[None, :])
        keep = np.ones((SLICE, w), dtype=bool)
        if fam == "holes":
            keep = oracle.random_f64(5000 + 31 * w, SLICE * w).reshape(SLICE, w) < 0.8
            keep[np.arange(SLICE) % 3 != 0] = True
        own = (i >= strip.lo) & (i < strip.lo + strip.rows)
        return assemble(oracle, name, strip.n, D, keep[i % SLICE] & own[:, None], strip.n)
    return _cached(name, make)


def halo_schemes(kind, use_dict):
    """The value scheme of a strip's matrix: stored values are random; value codes take seven values, or -- where the slices
    have to repeat -- one value per diagonal."""
    return "random" if kind == "sell8" else "diag5" if use_dict else "hash7"


def halo_families(strip, w):
    """The families a strip is tested with at width w: `holes` only where the own rows are more than half of the stored ones (the
    hybrid-ELL rule takes the full width while a third of ALL stored rows are full; fewer, and the rows with holes make a CSR tail),
    `crossed` at reach 1 only with one column."""
    fams = [f for f in HALO_FAMILIES if not (f == "holes" and 2 * strip.rows < strip.n)]
    return [f for f in fams if not (f == "crossed" and strip.reach == 1 and w > 1)]


def halo_cases():
    """(strip, ELL width, slice dictionary) of every GPU test of the halo role."""
    out = [(STRIPS["edge2"], w, False) for w in range(1, 9)] + [(STRIPS["dict"], w, True) for w in range(1, 9)]
    out += [(STRIPS["seams"], 3, False), (STRIPS["seams"], 1, False)]
    return out + [(s, 7, False) for name, s in STRIPS.items() if name not in ("seams", "edge2", "dict")]


def gather_kinds(codes, slices):
    """Per lane and ELL column of the given stored slices, from the codes (rows x w): (both rows on one diagonal, padding beside
    an entry, two different diagonals) -- the three ways through gather_pair that load something."""
    rows = (np.asarray(slices, dtype=np.int64)[:, None] * SLICE + np.arange(0, SLICE, 2)[None, :]).reshape(-1)
    c0, c1 = codes[rows].astype(np.int64), codes[rows + 1].astype(np.int64)
    m0, m1 = c0 < PAD_UNSAFE, c1 < PAD_UNSAFE
    return int(np.count_nonzero(m0 & m1 & (c0 == c1))), int(np.count_nonzero(m0 ^ m1)), int(np.count_nonzero(m0 & m1 & (c0 != c1)))


def halo_geometry(strip, mat):
    """The launch of a strip's product restated and checked on the host -- no product is launched before this has passed: every own
    slice exactly once; a workgroup reads a ghost range only where `halo_visits` says so (anything else would leave x); the inner
    slices stay inside the own range even with their 16-byte pairs.  Returns the inner slices in stored numbering."""
    visits = halo_visits(strip.ns, strip.edge, strip.lower, strip.upper)
    assert visit_once([so for so, _, _ in visits], strip.ns), (strip.name, "not every own slice once: no launch")
    first, last = np.full(strip.n // SLICE, strip.n, dtype=np.int64), np.full(strip.n // SLICE, -1, dtype=np.int64)
    np.minimum.at(first, mat.rows // SLICE, mat.col)
    np.maximum.at(last, mat.rows // SLICE, mat.col)
    inner = []
    for so, need_lo, need_hi in visits:
        sl = so + strip.lo // SLICE
        assert (need_lo or first[sl] >= strip.lo) and (need_hi or last[sl] < strip.lo + strip.rows), (strip.name, so, "reads a ghost range it does not wait for")
        assert not (need_lo and not strip.lower) and not (need_hi and not strip.upper), (strip.name, so)
        if not (need_lo or need_hi):
            # a pair is x[i + d], x[i + d + 1] of the lane's even row i: beside a ghost range it must stay inside the own range (where
            # the stored x ends instead, the 254 codes keep it inside: the encoders' business)
            assert not strip.lower or sl * SLICE - strip.reach >= strip.lo, (strip.name, so)
            assert not strip.upper or sl * SLICE + SLICE - 1 + strip.reach < strip.lo + strip.rows, (strip.name, so)
            inner.append(sl)
    return inner


# ---------------------------------------------------------------------------------------------------------------------------
# matrices of the analysis limits
# ---------------------------------------------------------------------------------------------------------------------------
def spread_index(n, count):
    """One number of [0, count) per row; the 256 rows a workgroup of the analyses takes hold at most 36 different ones."""
    r = np.arange(n, dtype=np.int64)
    return (36 * (r // 256) + r % 36) % count


def limit_diagonals(oracle, count, spread):
    """(ptr, col, w): `count` diagonals -- all of them in each of 300 rows, or one per row over 2048 (7680 for 1080) rows."""
    if not spread:
        n = 300
        col = (np.arange(n, dtype=np.int64)[:, None] + np.arange(count)[None, :]).reshape(-1)
        return np.arange(n + 1, dtype=np.int32) * count, col.astype(np.int32), count + 5
    n = 2048 if count <= 288 else 256 * 30
    d = spread_index(n, count) if count <= 288 else 36 * (np.arange(n) // 256) + np.arange(n) % 36
    return np.arange(n + 1, dtype=np.int32), (np.arange(n) + d).astype(np.int32), 1


def limit_values(count, spread, dtype):
    """(ptr, val, w): `count` distinct values, placed like the diagonals."""
    pool = ((np.arange(count) + 1) / 512.0).astype(dtype)
    if not spread:
        return np.arange(301, dtype=np.int32) * count, np.tile(pool, 300), count + 5
    return np.arange(2049, dtype=np.int32), pool[spread_index(2048, count)], 1


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
def sell8_variant(L, word):
    try:
        L.spmv_sell8_set_variant(word)
        yield
    finally:
        L.spmv_sell8_set_variant(0)


class Vectors:
    """x and y of a case on the device: x, exactly mat.m elements, at element offset x_offset (3: off every boundary; 4: 16-byte
    aligned) of a NaN-filled tensor; y between sentinels at an odd element offset (never 16-byte aligned) or, with y_offset = 0, at an
    even one (16-byte aligned for fp64, 8-byte for fp32: the vector branch of store_pair, the hot loop of the march kernel)."""

    def __init__(self, G, C, y_offset=1, x_offset=3):
        self.G, self.C = G, C
        n, m, dtype = C.mat.n, C.mat.m, C.dtype
        xbuf = np.full(m + 8, np.nan, dtype=dtype)
        xbuf[x_offset:x_offset + m] = C.x
        self.xbuf = G.up(xbuf)
        self.x = self.xbuf[x_offset:x_offset + m]
        self.y_at = GUARD + y_offset
        self.start, self.start_dev = {}, {}
        for mode in MODES:
            ybuf = np.full(n + 2 * GUARD + 2, SENTINEL, dtype=dtype)
            if mode[1]:
                ybuf[self.y_at:self.y_at + n] = C.y0
            self.start[mode], self.start_dev[mode] = ybuf, G.up(ybuf)
        size = np.dtype(dtype).itemsize
        assert self.xbuf.data_ptr() % 16 == 0 and self.start_dev[MODES[0]].data_ptr() % 16 == 0
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


def checked_traversal(name, visited, nb, fields, order=None):
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
    return [("strips", checked_traversal("strips", strip_visits(*geo, nb), nb, geo)),
            ("reversed map", checked_traversal("reversed map", rev, nb, (nb, 0, 0, 0), d_rev)),
            ("map with holes", checked_traversal("map with holes", holey, nb, (len(holey), 0, 0, 0), d_holey))], (d_rev, d_holey)


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
    body, want = got[GUARD:GUARD + count].view(np.uint8), np.ascontiguousarray(expected).view(np.uint8).reshape(-1)
    assert body.tobytes() == want.tobytes(), what + ("first differing byte %d of %d" % (np.flatnonzero(body != want)[0], len(want)),)


def table256(entries, pad, np_dtype):
    out = np.full(256, pad, dtype=np_dtype)
    out[:len(entries)] = entries
    return out


def device_csr(G, ptr, col, val, lead=0):
    """(ptr, col, val) on the device with ptr[0] = lead: `lead` slack entries in front, SLACK behind (column 0, value NaN)."""
    c = np.concatenate([np.zeros(lead), col, np.zeros(SLACK)]).astype(np.int32)
    v = np.concatenate([np.full(lead, np.nan), val, np.full(SLACK, np.nan)]).astype(val.dtype)
    return G.up((ptr.astype(np.int64) + lead).astype(np.int32)), G.up(c), G.up(v)


class Storage:
    """A matrix filled into a SELL8 / SELL8V buffer of exactly the stated size between guards by `vexhip_sell8_fill_*` /
    `vexhip_sell8v_fill_*` with the host's tables, and compared byte for byte with the encoder before anything uses it."""

    def __init__(self, G, oracle, mat, dtype, scheme, w, kind, lead=0):
        from vexcl_amd import _capi
        L, size = G.L, np.dtype(dtype).itemsize
        self.mat, self.dtype, self.scheme, self.w, self.kind, self.n = mat, dtype, scheme, w, kind, mat.n
        self.what = (mat.name, _sfx(dtype), scheme, kind, "width %d" % w, "ptr[0] = %d" % lead)
        ptr, col, val = mat.csr(dtype, scheme)
        self.deltas, self.values, self.max_col = tables(ptr, col, val, w)
        assert self.max_col == mat.max_col(w)
        if kind == "sell8":
            self.expected = encode_sell8(ptr, col, val, w, self.deltas, self.max_col, dtype, mat.slots(w))
            nbytes = L.sell8_bytes(mat.n, w, size)
        else:
            self.expected = encode_sell8v(ptr, col, val, w, self.deltas, self.max_col, dtype, self.values, mat.slots(w))
            nbytes = L.sell8v_bytes(mat.n, w)
        self.ns = (mat.n + SLICE - 1) // SLICE
        assert nbytes == len(self.expected) == self.ns * ((w + 1) // 2 * 1024 + (w * SLICE * size if kind == "sell8" else (w + 1) // 2 * 1024)), self.what
        self.d_deltas = G.up(table256(self.deltas, INT_MAX, np.int32))
        self.d_values = G.up(table256(self.values.view(dtype), 0, dtype)) if len(self.values) <= PAD else None
        self.whole, self.buf, self.host = guarded(G, nbytes, np.uint8, 0x5a)
        assert self.buf.data_ptr() % 16 == 0
        self.trav = _capi.Traversal(-1, -1, -1, -1, None)
        self.csr = device_csr(G, ptr, col, val, lead)
        self.fill(G)
        G.torch.cuda.synchronize()
        assert L.sell8_last_fill_max_col() == self.max_col, self.what
        assert (self.trav.grid_blocks, self.trav.chunk, self.trav.planes, self.trav.plane_blocks, self.trav.order) == (0, 0, 0, 0, None), self.what
        check_guarded(self.whole, self.host, self.expected, self.what + ("fill",))
        self._tails = {}

    def fill(self, G, d_deltas=None, ndeltas=None, d_values=None, nvalues=None):
        L, (dp, dc, dv) = G.L, self.csr
        dd, nd = d_deltas if d_deltas is not None else self.d_deltas, len(self.deltas) if ndeltas is None else ndeltas
        if self.kind == "sell8":
            getattr(L, "sell8_fill_%s_i32" % _sfx(self.dtype))(0, G.stream(), self.n, _vp(dp), _vp(dc), _vp(dv), self.w, _vp(dd), nd, _vp(self.buf), ctypes.byref(self.trav))
        else:
            dvl, nv = d_values if d_values is not None else self.d_values, len(self.values) if nvalues is None else nvalues
            getattr(L, "sell8v_fill_%s_i32" % _sfx(self.dtype))(0, G.stream(), self.n, _vp(dp), _vp(dc), _vp(dv), self.w, _vp(dd), nd, _vp(dvl), nv, _vp(self.buf),
                                                                ctypes.byref(self.trav))

    def tail(self, G, mat):
        """The CSR tail of `mat` (the filled matrix, or its ELL part alone) on the device; (None, None, None) where there is none."""
        if mat.name not in self._tails:
            tp, tc, tv = split_tail(*mat.csr(self.dtype, self.scheme), self.w)
            self._tails[mat.name] = (G.up(tp), G.up(np.concatenate([tc, np.zeros(SLACK, dtype=np.int32)])),
                                     G.up(np.concatenate([tv, np.full(SLACK, np.nan, dtype=self.dtype)]))) if len(tc) else (None, None, None)
        return self._tails[mat.name]

    def dictionary(self, G):
        """`vexhip_slice_dictionary` on the filled buffer -- the code part of every slice (SELL8) or the whole slice (SELL8V) -- with
        room for one block per slice: the numbers in order of first appearance and the representatives, as computed from the
        encoder's bytes."""
        L, wp = G.L, (self.w + 1) // 2
        code_bytes = wp * (1024 if self.kind == "sell8" else 2048)
        stride = len(self.expected) // self.ns
        assert (code_bytes == stride) == (self.kind == "sell8v")
        slices = self.expected.reshape(self.ns, stride)[:, :code_bytes]
        ids, reps = first_appearance(slices)
        bw, self.blocks, bh = guarded(G, self.ns, np.int32, -9)
        pw, self.pool, ph = guarded(G, self.ns * code_bytes, np.uint8, 0x3c)
        nb = ctypes.c_int64(-5)
        L.slice_dictionary(0, G.stream(), self.ns, stride, code_bytes, _vp(self.buf), self.ns, _vp(self.blocks), _vp(self.pool), ctypes.byref(nb))
        G.torch.cuda.synchronize()
        assert nb.value == len(reps), self.what + (nb.value, len(reps))
        check_guarded(bw, bh, ids, self.what + ("slice numbers",))
        check_guarded(pw, ph, np.concatenate([slices[reps].reshape(-1), np.full((self.ns - len(reps)) * code_bytes, 0x3c, dtype=np.uint8)]), self.what + ("pool",))
        self.ids, self.keep = ids, (bw, pw)
        return len(reps)

    def call(self, G, mat, trav=None, use_dict=False, march=None):
        """x, y, alpha, append -> one product of `mat` (the filled matrix or its ELL part alone) on this storage."""
        L, real, sfx, tail = G.L, _real(self.dtype), _sfx(self.dtype), self.tail(G, mat)
        tr = None if trav is None else ctypes.byref(trav)

        def call(x, y, alpha, append):
            head = (0, G.stream(), self.n, real(alpha), int(append), self.w)
            rest = (_vp(tail[0]), _vp(tail[1]), _vp(tail[2]), _vp(x), _vp(y), tr)
            if self.kind == "sell8" and not use_dict:
                getattr(L, "spmv_sell8_%s_i32" % sfx)(*head, _vp(self.buf), _vp(self.d_deltas), *rest)
            elif self.kind == "sell8":
                getattr(L, "spmv_sell8_dict_%s_i32" % sfx)(*head, _vp(self.buf), _vp(self.pool), _vp(self.blocks), _vp(self.d_deltas), *rest)
            elif not use_dict:
                getattr(L, "spmv_sell8v_%s_i32" % sfx)(*head, _vp(self.buf), _vp(self.d_deltas), _vp(self.d_values), *rest)
            elif march is None:
                getattr(L, "spmv_sell8v_dict_%s_i32" % sfx)(*head, _vp(self.pool), _vp(self.blocks), _vp(self.d_deltas), _vp(self.d_values), *rest)
            else:
                getattr(L, "spmv_sell8v_march_%s_i32" % sfx)(*head, _vp(self.pool), _vp(self.blocks), _vp(self.d_deltas), _vp(self.d_values), *rest, ctypes.byref(march))
        return call


def still_the_encoders(S, what):
    """A product test first asserts that its buffer (still) equals the encoder's."""
    check_guarded(S.whole, S.host, S.expected, what + ("the storage is not the encoder's",))


def with_and_without_tail(mat, w):
    return [mat] + ([truncated(mat, w)] if mat.lens.max() > w else [])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. analyses
# ---------------------------------------------------------------------------------------------------------------------------
def analyze_diagonals(G, ptr, col, w):
    """(ndeltas, the 256 table entries); the table sits between guards and starts as junk."""
    L = G.L
    whole, view, host = guarded(G, 256, np.int32, -3)
    nd = ctypes.c_int(-5)
    dp, dc, _ = device_csr(G, ptr, col, np.zeros(len(col)))
    L.sell8_analyze_i32(0, G.stream(), len(ptr) - 1, _vp(dp), _vp(dc), w, _vp(view), ctypes.byref(nd))
    G.torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert got[:GUARD].tobytes() == host[:GUARD].tobytes() and got[GUARD + 256:].tobytes() == host[GUARD + 256:].tobytes(), "guard changed"
    return nd.value, got[GUARD:GUARD + 256]


def analyze_values(G, ptr, val, w):
    L, dtype = G.L, val.dtype.type
    whole, view, host = guarded(G, 256, dtype, -3)
    nv = ctypes.c_int(-5)
    dp, _, dv = device_csr(G, ptr, np.zeros(len(val)), val)
    getattr(L, "sell8v_analyze_%s_i32" % _sfx(dtype))(0, G.stream(), len(ptr) - 1, _vp(dp), _vp(dv), w, _vp(view), ctypes.byref(nv))
    G.torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert got[:GUARD].tobytes() == host[:GUARD].tobytes() and got[GUARD + 256:].tobytes() == host[GUARD + 256:].tobytes(), "guard changed"
    return nv.value, got[GUARD:GUARD + 256].view(BITS[dtype])


def untouched(table, np_dtype):
    return table.tobytes() == np.full(256, -3, dtype=np_dtype).tobytes()


def analysis_matrices(oracle):
    return [family(oracle, fam, n, 12) for fam, n in (("holes", SIZES[-1]), ("tails", SIZES[-1]), ("unsorted", 513), ("empty", SIZES[-1]), ("crossed", 511),
                                                       ("bands", 1), ("pools", SIZES[-1]))]


@gpu
@every_dtype
@pytest.mark.parametrize("which", range(7))
def test_analyses_tables_counts_and_pads(G, oracle, dtype, which):
    """The diagonal table, the value table, their counts and the pads behind the last entry (INT_MAX / 0.0) for the first w entries of
    every row, w = 1, 3, 8, 12 -- matrices of width 12 with tails, unsorted rows, empty rows and slices."""
    assert len(analysis_matrices(oracle)) == 7
    for mat in analysis_matrices(oracle)[which:which + 1]:
        for scheme in ("pool255", "hash7"):
            ptr, col, val = mat.csr(dtype, scheme)
            for w in FEW_WIDTHS:
                deltas, values, _ = tables(ptr, col, val, w)
                nd, table = analyze_diagonals(G, ptr, col, w)
                assert nd == len(deltas) and np.array_equal(table, table256(deltas, INT_MAX, np.int32)), (mat.name, w, nd, len(deltas))
                nv, vtable = analyze_values(G, ptr, val, w)
                assert nv == len(values) and np.array_equal(vtable, table256(values, 0, BITS[dtype])), (mat.name, scheme, w, nv, len(values))


@gpu
def test_analyses_limits(G, oracle):
    """254 diagonals are coded and 255 are not; 255 values are coded and 256 are not -- with all of them in every row (a workgroup
    sees them all) and spread so that no workgroup sees more than 36 (only the merged set decides); 1080 diagonals overflow the global
    set; the value whose bits are all ones, and a matrix without entries, have no table.  A declined analysis leaves the table alone."""
    for spread in (False, True):
        for count in (254, 255):
            ptr, col, w = limit_diagonals(oracle, count, spread)
            nd, table = analyze_diagonals(G, ptr, col, w)
            if count == 254:
                assert nd == 254 and np.array_equal(table, table256(np.arange(254), INT_MAX, np.int32)), (spread, nd)
            else:
                assert nd == -1 and untouched(table, np.int32), (spread, nd)
        for dtype in DTYPES:
            for count in (255, 256):
                ptr, val, w = limit_values(count, spread, dtype)
                nv, table = analyze_values(G, ptr, val, w)
                if count == 255:
                    assert nv == 255 and np.array_equal(table, table256(np.unique(val.view(BITS[dtype])), 0, BITS[dtype])), (spread, dtype, nv)
                else:
                    assert nv == -1 and untouched(table, dtype), (spread, dtype, nv)
    ptr, col, w = limit_diagonals(oracle, 1080, True)
    nd, table = analyze_diagonals(G, ptr, col, w)
    assert nd == -1 and untouched(table, np.int32), nd
    for dtype in DTYPES:
        val = ((np.arange(10) + 1) / 8.0).astype(dtype)
        val.view(BITS[dtype])[3] = ~BITS[dtype](0)
        nv, table = analyze_values(G, np.arange(11, dtype=np.int32), val, 1)
        assert nv == -1 and untouched(table, dtype), (dtype, nv)
        nv, table = analyze_values(G, np.zeros(11, dtype=np.int32), np.zeros(0, dtype=dtype), 4)
        assert nv == -1 and untouched(table, dtype), (dtype, nv)
    nd, table = analyze_diagonals(G, np.zeros(11, dtype=np.int32), np.zeros(0, dtype=np.int32), 4)
    assert nd == -1 and untouched(table, np.int32), nd


def fused_matrices(oracle):
    """(ptr, col, float64 values, the storage vexhip_spmat must choose) -- one per storage."""
    A = family(oracle, "tails", SIZES[-1], 5)
    ptr, col, w = limit_diagonals(oracle, 255, True)
    return [(A.ptr, A.col, A.values("hash7"), "sell8v"), (A.ptr, A.col, A.values("random"), "sell8"),
            (ptr, col, oracle.random_f64(77, len(col)) - 0.5, "sell32")]


def fused_limit_matrices(oracle, dtype):
    """(name, ptr, col, values of `dtype`, the row length the hybrid-ELL width must cover): the matrices of `test_analyses_limits`
    as whole matrices -- 254 / 255 diagonals over three values; 255 / 256 values, spread over one diagonal, all of them in every
    row (which then holds as many diagonals: neither is coded), and all of them in every two rows of 128 diagonals (a workgroup
    sees them all and the diagonals stay coded); the value whose bits are all ones."""
    out = []
    for count in (254, 255):
        for spread in (False, True):
            ptr, col, _ = limit_diagonals(oracle, count, spread)
            out.append(("%d diagonals%s" % (count, ", spread" if spread else ""), ptr, col, ((col % 3 + 1) / 4.0).astype(dtype), 1 if spread else count))
    for count in (255, 256):
        for spread in (False, True):
            ptr, val, _ = limit_values(count, spread, dtype)
            rows = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
            col = (rows + np.arange(len(val)) - ptr[:-1][rows]).astype(np.int32)               # entry k of row r: column r + k
            out.append(("%d values%s" % (count, ", spread" if spread else ""), ptr, col, val, 1 if spread else count))
        pool = ((np.arange(count) + 1) / 512.0).astype(dtype)
        k = np.arange(300 * 128, dtype=np.int64)
        out.append(("%d values, in every two rows" % count, np.arange(301, dtype=np.int32) * 128, (k // 128 + k % 128).astype(np.int32), pool[k % count], 128))
    val = ((np.arange(10) + 1) / 8.0).astype(dtype)
    val.view(BITS[dtype])[3] = ~BITS[dtype](0)
    out.append(("all-ones value", np.arange(11, dtype=np.int32), np.arange(10, dtype=np.int32), val, 1))
    return out


def check_fused(G, oracle, ptr, col, val, storage=None, row_length=None):
    """One matrix through vexhip_spmat_create_*: what its fused analysis left in the handle against the separate analyses at
    info.ell_width.  storage: the storage it must choose, where the case names one."""
    from vexcl_amd import _capi
    L, dtype = G.L, val.dtype.type
    assert row_length is None or oracle.hell_width(ptr) >= row_length, (oracle.hell_width(ptr), row_length)
    dp, dc, dv = device_csr(G, ptr, col, val)
    h = ctypes.c_void_p()
    getattr(L, "spmat_create_%s_i32" % _sfx(dtype))(0, G.stream(), len(ptr) - 1, _vp(dp), _vp(dc), _vp(dv), _capi.SPMAT_AUTO, 0, ctypes.byref(h))
    try:
        info = _capi.SpMatInfo()
        L.spmat_get_info(h, ctypes.byref(info))
        w = int(info.ell_width)
        assert w == oracle.hell_width(ptr) and (storage is None or _capi.SPMAT_NAMES[info.format] == storage), (storage, info.format, w)
        nd, table = analyze_diagonals(G, ptr, col, w)
        nv, vtable = analyze_values(G, ptr, val, w)
        if not (nd > 0 and nv > 0):
            nv = -1                                                # (value codes only where the diagonals have codes and the values fit)
        assert (info.ndeltas, info.nvalues) == (nd, nv), (storage, info.ndeltas, nd, info.nvalues, nv)
        assert bool(info.deltas) == (nd > 0) and bool(info.values) == (nv > 0)
        assert storage is None or (nd > 0, nv > 0) == (storage != "sell32", storage == "sell8v"), (storage, nd, nv)
        if nd > 0:
            got = np.empty(256, dtype=np.int32)
            L.memcpy_d2h(0, got.ctypes.data, info.deltas, got.nbytes, G.stream(), 1)
            assert np.array_equal(got, table), storage
        if nv > 0:
            got = np.empty(256, dtype=BITS[dtype])
            L.memcpy_d2h(0, got.ctypes.data, info.values, got.nbytes, G.stream(), 1)
            assert np.array_equal(got, vtable), storage
        return nd, nv
    finally:
        L.spmat_destroy(h)


@gpu
@every_dtype
def test_fused_analysis_reports_what_the_separate_analyses_do(G, oracle, dtype):
    """`analyze_fused_kernel` (vexhip_spmat_create_*): ndeltas, nvalues and both tables as `vexhip_sell8_analyze_i32` and
    `vexhip_sell8v_analyze_*` give them at info.ell_width, for a value-coded matrix, one with stored values and one with 32-bit
    columns -- and at the limits of both sets (fused_limit_matrices), where the verdicts are known as well."""
    for ptr, col, val64, storage in fused_matrices(oracle):
        check_fused(G, oracle, ptr, col, val64.astype(dtype), storage)
    verdicts = {name: check_fused(G, oracle, ptr, col, val, None, row_length) for name, ptr, col, val, row_length in fused_limit_matrices(oracle, dtype)}
    assert verdicts == {"254 diagonals": (254, 3), "254 diagonals, spread": (254, 3), "255 diagonals": (-1, -1), "255 diagonals, spread": (-1, -1),
                        "255 values": (-1, -1), "255 values, spread": (1, 255), "255 values, in every two rows": (128, 255),
                        "256 values": (-1, -1), "256 values, spread": (1, -1), "256 values, in every two rows": (128, -1),
                        "all-ones value": (1, -1)}, verdicts


# ---------------------------------------------------------------------------------------------------------------------------
# 2. fills and the slice dictionary
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@every_dtype
@every_family
def test_fills_every_width_byte_for_byte(G, oracle, dtype, fam):
    """Per family, size and ELL width 1..9, 12: both fills into a buffer of exactly the stated size between guards, compared as bytes
    with the encoders; the largest ELL column; the empty traversal.  Staged (w <= 8) and not; the family `empty` also with ptr[0] = 5."""
    fills = 0
    for n in SIZES:
        for w in WIDTHS:
            mat = family(oracle, fam, n, w)
            for kind, scheme in fill_schemes(fam):
                for lead in ((0, LEAD) if fam == "empty" else (0,)):
                    Storage(G, oracle, mat, dtype, scheme, w, kind, lead)
                    fills += 1
    assert fills == len(SIZES) * len(WIDTHS) * len(fill_schemes(fam)) * (2 if fam == "empty" else 1)


@gpu
@every_dtype
def test_fills_refuse_a_table_that_lacks_a_diagonal_or_a_value(G, oracle, dtype):
    """A table without one of the matrix's diagonals, or without one of its values, is an error with the documented text -- in the
    staged fill and in the walk through global memory."""
    from vexcl_amd import _capi
    for w in (5, 9):
        mat = family(oracle, "holes", 513, w)
        for kind, text in (("sell8", "SELL8 fill: the matrix uses a diagonal that is not in the table"),
                           ("sell8v", "SELL8V fill: a diagonal or a value of the matrix is not in its table")):
            S = Storage(G, oracle, mat, dtype, "hash7", w, kind)
            for drop in range(len(S.deltas)):
                with pytest.raises(_capi.Error, match=text):
                    S.fill(G, G.up(table256(np.delete(S.deltas, drop), INT_MAX, np.int32)), len(S.deltas) - 1)
                assert text in G.L.last_error().decode()
            if kind == "sell8v":
                for drop in (0, len(S.values) - 1):
                    with pytest.raises(_capi.Error, match=text):
                        S.fill(G, d_values=G.up(table256(np.delete(S.values, drop).view(dtype), 0, dtype)), nvalues=len(S.values) - 1)
                    assert text in G.L.last_error().decode()
            S.fill(G)                                                  # and the full tables again: the encoder's bytes
            G.torch.cuda.synchronize()
            still_the_encoders(S, S.what)


def dictionary_cases(oracle):
    """(matrix, ELL width, scheme of the SELL8 storage): repeating slices for every width, and slices that are all different."""
    return [(dict_matrix(oracle, w), w, "random") for w in WIDTHS] + [(family(oracle, "holes", SIZES[-1], 5), 5, "random"), (march_matrix(oracle, "w7"), 7, "diag5")]


@gpu
@every_dtype
@pytest.mark.parametrize("part", range(4))
def test_slice_dictionary_numbers_and_pool(G, oracle, dtype, part):
    """13-slice matrices whose inner slices repeat (few blocks) and a matrix whose slices all differ (a block per slice): the code
    part alone for SELL8 -- stored values differ from slice to slice --, the whole slice for SELL8V."""
    assert len(dictionary_cases(oracle)) == 12
    for mat, w, scheme in dictionary_cases(oracle)[part::4]:
        blocks8 = Storage(G, oracle, mat, dtype, scheme, w, "sell8").dictionary(G)
        blocks8v = Storage(G, oracle, mat, dtype, "diag5", w, "sell8v").dictionary(G)
        ns = (mat.n + SLICE - 1) // SLICE
        if mat.name.startswith("holes"):
            assert blocks8 == blocks8v == ns == 4
        else:
            assert 2 <= blocks8 <= blocks8v <= 6 and ns == 13, (mat.name, blocks8, blocks8v)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. products
# ---------------------------------------------------------------------------------------------------------------------------
def check_products(G, oracle, S, travs, use_dict, words=(0, 1)):
    """The products of one storage, with and without the CSR tail: every traversal with y off every 16-byte boundary, the NULL
    traversal also with y and x aligned; under each variant word."""
    still_the_encoders(S, S.what)
    launches = 0
    for mat in with_and_without_tail(S.mat, S.w):
        C = case_of(oracle, mat, S.dtype, S.scheme)
        assert mat.m == S.max_col + 1, S.what                           # x holds exactly max_col + 1 elements
        calls = [("NULL traversal", S.call(G, mat, None, use_dict))] + [(name, S.call(G, mat, t, use_dict)) for name, t in travs]
        for V, some in ((Vectors(G, C, 1, 3), calls), (Vectors(G, C, 0, 4), calls[:1])):
            for word in words:
                with sell8_variant(G.L, word):
                    check_all(oracle, V, some, S.what + (mat.name, "y offset %d" % (V.y_at - GUARD), "word %d" % word, "dict" if use_dict else "streamed"))
                launches += len(some)
    return launches


@gpu
@every_dtype
@every_family
@pytest.mark.parametrize("sizes", (SIZES[:4], SIZES[4:]), ids=("to512", "from513"))
def test_products_streamed_every_width_and_traversal(G, oracle, dtype, fam, sizes):
    """`vexhip_spmv_sell8_*` and `vexhip_spmv_sell8v_*` on the fills' buffers: sell8_pair_kernel<W, *, false> (word 0, W <= 8),
    sell8_kernel<W> / sell8v_kernel<W> (word 1; sell8v_kernel<9> under both) and the loops (9 / 12; 12)."""
    seen = set()
    for n in sizes:
        travs, keep_alive = hand_made_traversals(G, (n + SLICE - 1) // SLICE)
        for w in product_widths(n):
            mat = family(oracle, fam, n, w)
            for kind, scheme in fill_schemes(fam)[-2:]:
                S = Storage(G, oracle, mat, dtype, scheme, w, kind)
                assert check_products(G, oracle, S, travs, False) > 0
                seen.add((kind, w))
    assert seen == {(k, w) for k in ("sell8", "sell8v") for w in product_widths(sizes[0])}


def strips47(chunk):
    geo = STRIPS47[chunk]
    return checked_traversal("strips of %d" % chunk, strip_visits(*geo, 47), 47, geo)


STRIP_CASES = ((3, "sell8", "random"), (7, "sell8v", "diag5"), (9, "sell8v", "diag5"), (12, "sell8", "random"))


@gpu
@every_dtype
@pytest.mark.parametrize("case", STRIP_CASES, ids=lambda c: "w%d-%s" % c[:2])
def test_products_strip_order_on_47_slices(G, oracle, dtype, case):
    """Strips of 2 and of 4 slices over planes of 10 (8 * chunk > 10: holes in every tile; the last plane holds 7) on 47 slices:
    the pair kernel's `s < 0` branch with and without a dictionary, and the early return of the per-entry kernels."""
    w, kind, scheme = case
    S = Storage(G, oracle, dict_matrix(oracle, w, N47), dtype, scheme, w, kind)
    S.dictionary(G)
    travs = [("strips of %d" % c, strips47(c)) for c in (2, 4)]
    for use_dict in (False, True):
        assert check_products(G, oracle, S, travs, use_dict) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the march product
# ---------------------------------------------------------------------------------------------------------------------------
def device_plan(G, S, x_last, trav=None):
    from vexcl_amd import _capi
    out = _capi.March(-1, -1, -1, -1, -1, -1, (-1, -1, -1))
    G.L.sell8_march_plan(0, G.stream(), _vp(S.d_deltas), len(S.deltas), _vp(S.blocks), S.ns, np.dtype(S.dtype).itemsize,
                         None if trav is None else ctypes.byref(trav), x_last, ctypes.byref(out))
    return out


def plan_fields(p):
    return (p.lo, p.hi, p.usable, p.x_last, p.nfar, list(p.far)[:p.nfar])


def checked_plan(G, S, which, trav=None):
    """The device's plan equals the host restatement (and what the sets are named for); returns it."""
    plan = device_plan(G, S, S.max_col, trav)
    host = march_plan_host(S.deltas, S.ids, np.dtype(S.dtype).itemsize, S.max_col)
    assert host is not None and host == MARCH_EXPECT[which], (which, host)
    assert plan_fields(plan) == (host[0], host[1], 1, S.max_col, len(host[2]), host[2]) and plan.run >= 2 and plan.far[2] == 0, (which, plan_fields(plan), host)
    return plan


def with_run(plan, run):
    from vexcl_amd import _capi
    return _capi.March(plan.lo, plan.hi, run, plan.usable, plan.x_last, plan.nfar, tuple(plan.far))


def check_march(G, oracle, S, plan, runs, trav, strips, what):
    """`vexhip_spmv_sell8v_march_*` for every run, against the `_dict` product of the same traversal (checked in full against the
    oracle and the bound): with and without the CSR tail, y aligned (the hot loop) and not (`kend = 0`), x at both alignments."""
    still_the_encoders(S, S.what)
    for run in runs:
        assert visit_once(march_visits(S.ns, run, strips)[0], S.ns), what + ("run %d: not every slice once: no launch" % run,)
    for mat in with_and_without_tail(S.mat, S.w):
        C = case_of(oracle, mat, S.dtype, S.scheme)
        assert mat.m == S.max_col + 1 == plan.x_last + 1
        calls = [("dict", S.call(G, mat, trav, True))] + [("march, run %d" % r, S.call(G, mat, trav, True, with_run(plan, r))) for r in runs]
        for y_offset in (0, 1):
            for x_offset in (3, 4):
                check_all(oracle, Vectors(G, C, y_offset, x_offset), calls, what + (mat.name, "y offset %d" % y_offset, "x offset %d" % x_offset))
        with sell8_variant(G.L, 2):                                    # word 2: the march entry behaves as `_dict`
            check_all(oracle, Vectors(G, C, 0, 4), [calls[0], ("march entry under word 2", calls[-1][1])], what + (mat.name, "word 2"))


@gpu
@every_dtype
@pytest.mark.parametrize("which", sorted(MARCH_SETS))
def test_march_plan_and_product_on_13_slices(G, oracle, dtype, which):
    """Widths 1, 2, 3, 7, 8; no, one and two far diagonals; x_last below, at and above n - 1; a near window of three slices; runs
    of 1, 2, 3, 5, 13 and 64 slices in plain order."""
    mat = march_matrix(oracle, which)
    w = len(MARCH_SETS[which][0])
    S = Storage(G, oracle, mat, dtype, "diag5", w, "sell8v")
    S.dictionary(G)
    plan = checked_plan(G, S, which)
    check_march(G, oracle, S, plan, MARCH_RUNS, None, None, S.what)


@gpu
@every_dtype
@pytest.mark.parametrize("which", ("w3", "w7"))
def test_march_product_in_strip_order_on_47_slices(G, oracle, dtype, which):
    """The strip form of march_run: every divisor of the strip length as run, strips of 2 and 4 over planes of 10 slices -- runs cut
    short by the plane end (10 = 2 * 4 + 2) and by the matrix end (the last plane holds 7 slices), workgroups without a slice."""
    mat = march_matrix(oracle, which, N47)
    S = Storage(G, oracle, mat, dtype, "diag5", len(MARCH_SETS[which][0]), "sell8v")
    S.dictionary(G)
    for chunk in (2, 4):
        trav = strips47(chunk)
        plan = checked_plan(G, S, which, trav)
        assert chunk % plan.run == 0
        check_march(G, oracle, S, plan, [r for r in (1, 2, 4) if chunk % r == 0], trav, STRIPS47[chunk], S.what + ("strips of %d" % chunk,))


@gpu
def test_march_plan_declines_and_width_9_is_refused(G, oracle):
    """Fewer than 8 slices, slice numbers that alternate, a third far diagonal and an explicit order are declined (a zeroed plan); the
    march entry refuses ELL width 9 with the documented error and writes nothing."""
    from vexcl_amd import _capi
    L = G.L

    def plan(deltas, blocks, order=None):
        out = _capi.March(-1, -1, -1, -1, -1, -1, (-1, -1, -1))
        d, b = G.up(table256(deltas, INT_MAX, np.int32)), G.up(np.asarray(blocks, dtype=np.int32))
        trav = None if order is None else ctypes.byref(_capi.Traversal(len(blocks), 0, 0, 0, order.data_ptr()))
        L.sell8_march_plan(0, G.stream(), _vp(d), len(deltas), _vp(b), len(blocks), 8, trav, 10 ** 6, ctypes.byref(out))
        host = march_plan_host(deltas, blocks, 8, 10 ** 6, order is not None)
        return (out.lo, out.hi, out.run, out.usable, out.x_last, out.nfar, list(out.far)), host
    zero = (0, 0, 0, 0, 0, 0, [0, 0, 0])
    near, steady = (-512, -1, 0, 1, 512), [0] + [1] * 11 + [2]
    got, host = plan(near, steady)
    assert got[3] == 1 and host == (-512, 512, []) and got[:2] == (-512, 512) and got[5] == 0
    assert plan(near, steady[:7]) == (zero, None)
    assert plan(near, [0, 1] * 6 + [0]) == (zero, None)
    assert plan(near, [0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0])[0][3] == 1          # 6 changes in 13 slices: still taken
    assert plan((-4096, -2048, 0, 2048), steady) == (zero, None)
    order = G.up(np.arange(13, dtype=np.int32))
    assert plan(near, steady, order) == (zero, None)

    mat = march_matrix(oracle, "w9")
    S = Storage(G, oracle, mat, np.float64, "diag5", 9, "sell8v")
    S.dictionary(G)
    p = device_plan(G, S, S.max_col)
    assert p.usable == 1 and (p.lo, p.hi, p.nfar) == (-700, 700, 2)
    for m in with_and_without_tail(mat, 9):
        V = Vectors(G, case_of(oracle, m, np.float64, "diag5"), 0, 4)
        for mode in MODES:
            ybuf = V.start_dev[mode].clone()
            with pytest.raises(_capi.Error, match=r"march kernels cover ELL widths 1\.\.8"):
                S.call(G, m, None, True, with_run(p, 4))(V.x, ybuf[V.y_at:V.y_at + m.n], *mode)
            assert ybuf.cpu().numpy().tobytes() == V.start[mode].tobytes(), "a refused call wrote to y"
        check_all(oracle, V, [("dict", S.call(G, m, None, True))], S.what + (m.name,))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the halo role of the pair product, in one process
# ---------------------------------------------------------------------------------------------------------------------------
class HaloPlan:
    """A strip's matrix as a vexhip_spmat in the storage the test names -- checked from vexhip_spmat_get_info and, where the handle
    keeps its slices, byte for byte against the encoder -- and its pull plan without a window (VEXHIP_PULL_EVENTS: no flag is raised
    or waited for, the launch is sell8_pair_halo_kernel alone)."""

    def __init__(self, G, oracle, strip, mat, kind, w, use_dict):
        from vexcl_amd import _capi
        L = G.L
        self.G, self.strip, self.mat, self.kind, self.w = G, strip, mat, kind, w
        self.scheme = halo_schemes(kind, use_dict)
        self.what = (strip.name, mat.name, kind, "width %d" % w, "dictionary" if use_dict else "streamed")
        self.inner = halo_geometry(strip, mat)                          # before anything is launched
        ptr, col, val = mat.csr(np.float64, self.scheme)
        assert mat.n == strip.n and oracle.hell_width(ptr) == w == mat.lens.max(), self.what
        self.csr = device_csr(G, ptr, col, val)
        self.h, self.plan = ctypes.c_void_p(), ctypes.c_void_p()
        flags = _capi.SPMAT_NO_MARCH | _capi.SPMAT_NO_PLANE | (0 if use_dict else _capi.SPMAT_NO_DICTIONARY)
        L.spmat_create_f64_i32(0, G.stream(), mat.n, _vp(self.csr[0]), _vp(self.csr[1]), _vp(self.csr[2]),
                               _capi.SPMAT_SELL8 if kind == "sell8" else _capi.SPMAT_SELL8V, flags, ctypes.byref(self.h))
        try:
            info = _capi.SpMatInfo()
            L.spmat_get_info(self.h, ctypes.byref(info))
            assert _capi.SPMAT_NAMES[info.format] == kind and info.tail_nnz == 0 and info.ell_width == w and info.rows == mat.n, self.what + (info.format, info.tail_nnz, info.ell_width)
            assert (info.dictionary_blocks > 0) == use_dict and bool(info.slice_blocks) == use_dict, self.what + (info.dictionary_blocks,)
            assert info.plane.usable == 0 and info.grid.usable == 0 and info.march.usable == 0, self.what
            deltas, values, max_col = tables(ptr, col, val, w)
            assert info.ndeltas == len(deltas) and np.abs(deltas).max() == strip.reach, self.what
            self.codes = _coded(ptr, col, w, deltas, max_col, mat.slots(w))[2]
            want = encode_sell8(ptr, col, val, w, deltas, max_col, np.float64, mat.slots(w)) if kind == "sell8" else \
                encode_sell8v(ptr, col, val, w, deltas, max_col, np.float64, values, mat.slots(w))

            def fetch(address, count, np_dtype):
                got = np.empty(count, dtype=np_dtype)
                L.memcpy_d2h(0, got.ctypes.data, address, got.nbytes, G.stream(), 1)
                return got
            if info.sell_bytes:                                         # (a value-coded matrix with a dictionary keeps its pool only)
                assert info.sell_bytes == len(want) and fetch(info.sell, len(want), np.uint8).tobytes() == want.tobytes(), self.what + ("the stored slices are not the encoder's",)
            else:
                assert kind == "sell8v" and use_dict, self.what
            if use_dict:                                                # the blocks in order of first appearance, as vexhip_slice_dictionary numbers them
                ns, code_bytes = mat.n // SLICE, (w + 1) // 2 * (1024 if kind == "sell8" else 2048)
                slices = want.reshape(ns, -1)[:, :code_bytes]
                ids, reps = first_appearance(slices)
                assert info.dictionary_blocks == len(reps) and np.array_equal(fetch(info.slice_blocks, ns, np.int32), ids), self.what + (info.dictionary_blocks, len(reps))
                assert fetch(info.code_pool, len(reps) * code_bytes, np.uint8).tobytes() == slices[reps].tobytes(), self.what + ("the pool is not the encoder's",)
            L.dist_spmv_create_halo_pull(None, self.h, strip.rows, strip.halo, 0 if strip.lower else -1, 1 if strip.upper else -1,
                                         PULL_EVENTS, ctypes.byref(self.plan))
        except BaseException:
            self.close()
            raise

    def kinds(self):
        """gather_kinds of the slices that take the inner gather."""
        return gather_kinds(self.codes, self.inner)

    def apply(self, x, y, alpha, append, below, above):
        self.G.L.dist_spmv_apply_pull(self.plan, self.G.stream(), float(alpha), int(append), _vp(x), _vp(y), _vp(below), _vp(above))

    def apply_plain(self, x, y, alpha, append):
        self.G.L.spmat_apply_f64(self.h, self.G.stream(), float(alpha), int(append), _vp(x), _vp(y))

    def timed_out(self):
        t, transport, direct = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        self.G.L.dist_spmv_status(self.plan, ctypes.byref(t), ctypes.byref(transport), ctypes.byref(direct))
        return t.value

    def close(self):
        if self.plan:
            self.G.L.dist_spmv_destroy(self.plan)
        if self.h:
            self.G.L.spmat_destroy(self.h)
        self.plan, self.h = ctypes.c_void_p(), ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class HaloVectors:
    """x, the two ghost ranges and y of a strip on the device.  x: exactly the own rows, at element 3 of a NaN-filled tensor; the
    ghost ranges: exactly `halo` elements at element 2 (16-byte aligned, as apply_pull requires) of NaN-filled tensors of their own;
    y between sentinels, off (y_offset = 1) or on a 16-byte boundary.  `load` rewrites all of them in place from a case of the
    stored matrix: x_ext = [x_below | x | x_above], NaN wherever no entry reads."""

    def __init__(self, G, strip, y_offset=1):
        self.G, self.strip, self.y_at = G, strip, GUARD + y_offset

        def canary(count, at):
            whole = G.up(np.full(count + 8, np.nan))
            assert (whole.data_ptr() + 8 * at) % 16 == 8 * (at % 2)
            return whole, whole[at:at + count]
        self.xbuf, self.x = canary(strip.rows, 3)
        self.bbuf, self.below = canary(strip.halo, 2) if strip.lower else (None, None)
        self.abuf, self.above = canary(strip.halo, 2) if strip.upper else (None, None)
        self.ybuf = G.up(np.full(strip.rows + 2 * GUARD + 2, SENTINEL))
        assert self.ybuf.data_ptr() % 16 == 0

    def load(self, C):
        s, up = self.strip, self.G.up
        x_ext = np.full(s.n, np.nan)
        x_ext[:len(C.x)] = C.x
        for whole, at, part in ((self.xbuf, 3, s.own(x_ext)), (self.bbuf, 2, x_ext[:s.lo]), (self.abuf, 2, x_ext[s.lo + s.rows:])):
            if whole is not None:
                host = np.full(len(part) + 8, np.nan)
                host[at:at + len(part)] = part
                whole.copy_(up(host))
        self.C, self.start = C, {}
        for mode in MODES:
            ybuf = np.full(s.rows + 2 * GUARD + 2, SENTINEL)
            if mode[1]:
                ybuf[self.y_at:self.y_at + s.rows] = s.own(C.y0)
            self.start[mode] = ybuf

    def run(self, P, mode, plain=False):
        """One product in place; returns the whole y tensor on the host."""
        self.ybuf.copy_(self.G.up(self.start[mode]))
        y = self.ybuf[self.y_at:self.y_at + self.strip.rows]
        if plain:
            P.apply_plain(self.x, y, *mode)
        else:
            P.apply(self.x, y, *mode, self.below, self.above)
        return self.ybuf.cpu().numpy()


def check_halo(oracle, P, V, what):
    """Both modes: every own row finite, the oracle's bits (its product on the stored matrix, own rows), within the derived bound;
    every other byte of the y tensor unchanged; without a neighbour also the bytes of vexhip_spmat_apply_f64."""
    s, C = P.strip, V.C
    own = slice(V.y_at, V.y_at + s.rows)
    for mode in MODES:
        out, ref = V.run(P, mode), C.reference(oracle, mode)
        got, want = out[own], s.own(ref)
        assert np.all(np.isfinite(got)), what + (mode, "not finite: row %d" % np.flatnonzero(~np.isfinite(got))[0])
        assert np.array_equal(got, want), what + (mode, first_difference(got, want))
        whole = ref.copy()
        whole[s.lo:s.lo + s.rows] = got
        assert C.within_bound(whole, mode), what + (mode, "outside the bound of the high-precision reference")
        rest = out.copy()
        rest[own] = V.start[mode][own]
        assert rest.tobytes() == V.start[mode].tobytes(), what + (mode, "a guard element changed")
        if not (s.lower or s.upper):
            assert V.run(P, mode, plain=True).tobytes() == out.tobytes(), what + (mode, "differs from vexhip_spmat_apply_f64")
    assert P.timed_out() == 0, what


def check_strip(G, oracle, strip, w, use_dict, kinds, y_offsets=(1,)):
    """Every family of the strip at width w, in both value forms; returns the gather kinds of the inner slices, summed."""
    seen = np.zeros(3, dtype=np.int64)
    for fam in halo_families(strip, w):
        mat = strip_matrix(oracle, strip, fam, w)
        for kind in kinds:
            with HaloPlan(G, oracle, strip, mat, kind, w, use_dict) as P:
                for y_offset in y_offsets:
                    V = HaloVectors(G, strip, y_offset)
                    V.load(case_of(oracle, mat, np.float64, P.scheme))
                    check_halo(oracle, P, V, P.what + ("y offset %d" % y_offset,))
                k = np.array(P.kinds())
                assert k[HALO_FAMILIES.index(fam)] > 0 or not P.inner, P.what + (k.tolist(), "the family no longer takes its way through the inner gather")
                seen += k
    return seen


every_width = pytest.mark.parametrize("w", range(1, 9))
both_forms = pytest.mark.parametrize("kind", ("sell8", "sell8v"))


@gpu
@every_width
@both_forms
def test_halo_every_width_streamed(G, oracle, w, kind):
    """sell8_pair_halo_kernel<double, W, VCODED, false>, W = 1..8, on a strip with two edge slices per side and four inner ones
    (reach 513 in ghost ranges of 1024): all three gathers in the inner slices, both ghost ranges through the translated access."""
    seen = check_strip(G, oracle, STRIPS["edge2"], w, False, (kind,))
    assert np.all(seen > 0), (w, kind, seen.tolist())


@gpu
@every_width
@both_forms
def test_halo_every_width_with_a_dictionary(G, oracle, w, kind):
    """sell8_pair_halo_kernel<double, W, VCODED, true> on 66 stored slices whose code blocks repeat (ns >= 64, 4 blocks <= ns)."""
    seen = check_strip(G, oracle, STRIPS["dict"], w, True, (kind,))
    assert np.all(seen > 0), (w, kind, seen.tolist())


@gpu
@pytest.mark.parametrize("name", [n for n in STRIPS if n not in ("edge2", "dict")])
def test_halo_geometries(G, oracle, name):
    """The other strips at width 7 (reach 1: widths 3 and 1), y off and on a 16-byte boundary: the seams inside one lane, reach equal
    to the ghost range, strips shorter than two reaches, a neighbour on one side only and none (then also against
    vexhip_spmat_apply_f64)."""
    strip = STRIPS[name]
    seen = sum(check_strip(G, oracle, strip, w, False, ("sell8", "sell8v"), (1, 0)) for s, w, _ in halo_cases() if s is strip)
    assert strip.ns < 2 * strip.edge or np.all(seen > 0), (name, seen.tolist())


@gpu
@both_forms
def test_halo_repeated_products_on_one_plan(G, oracle, kind):
    """Three products back to back on one plan, x and both ghost ranges rewritten in place in between."""
    strip, w = STRIPS["reach_is_halo"], 7
    mat = strip_matrix(oracle, strip, "holes", w)
    with HaloPlan(G, oracle, strip, mat, kind, w, False) as P:
        V = HaloVectors(G, strip)
        for salt in (0, 1, 2):
            V.load(case_of(oracle, mat, np.float64, P.scheme, salt))
            check_halo(oracle, P, V, P.what + ("vectors %d" % salt,))


# ---------------------------------------------------------------------------------------------------------------------------
# the CPU test
# ---------------------------------------------------------------------------------------------------------------------------
def every_storage_case(oracle):
    """(matrix, ELL width, value schemes) of every storage a GPU test fills."""
    for fam in FAMILIES:
        for n in SIZES:
            for w in WIDTHS:
                yield family(oracle, fam, n, w), w, sorted({s for _, s in fill_schemes(fam)})
    for w in WIDTHS:
        yield dict_matrix(oracle, w), w, ["random", "diag5"]
    for w in (3, 7, 9, 12):
        yield dict_matrix(oracle, w, N47), w, ["random", "diag5"]
    for which in sorted(MARCH_SETS) + ["w9"]:
        yield march_matrix(oracle, which), len(MARCH_SETS[which][0]) if which in MARCH_SETS else 9, ["diag5"]
    for which in ("w3", "w7"):
        yield march_matrix(oracle, which, N47), len(MARCH_SETS[which][0]), ["diag5"]


def oracle_slots(oracle, mat, w):
    """`pair_slots` from `oracle.sell_pair_slots`, pair after pair."""
    R = (mat.n + SLICE - 1) // SLICE * SLICE
    ent, pad = np.full((R, w), -1, dtype=np.int64), np.full((R, w), PAD, dtype=np.uint8)
    max_col = mat.max_col(w)
    for r0 in range(0, mat.n, 2):
        out = oracle.sell_pair_slots(mat.ptr, mat.col, r0, w, max_col)
        for q in (0, 1):
            for j, e in enumerate(out[q]):
                if e == "unsafe":
                    pad[r0 + q, j] = PAD_UNSAFE
                elif e != "safe":
                    ent[r0 + q, j] = e
    return ent, pad


def test_generators_encoders_and_host_models(oracle):
    """Without a GPU: every family contains what it is named for; the encoders' placement equals `oracle.sell_pair_slots` for every
    pair of every matrix a GPU test fills, and decode(encode(A)) = A; the traversal and march-run models visit every slice once for
    every geometry used and refuse what is no traversal; the plan restatement gives what the march sets are named for; and
    `oracle.spmv_csr` lies within the derived bound on every matrix, in both types."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no wider than double here: no independent fp64 reference"
    assert len(FAMILIES) == 10 and len(SIZES) == 6 and len(WIDTHS) == 10 and set(range(1, 10)) <= set(WIDTHS) and N13 == 6221 and N47 == 23629
    assert {(n + SLICE - 1) // SLICE for n in SIZES} == {1, 2, 4} and (N13 + 511) // 512 == 13 and (N47 + 511) // 512 == 47

    # the families: structure counts over all sizes and widths
    stats = {fam: {"same": 0, "merged": 0, "plain": 0, 254: 0, 255: 0, "tail": 0} for fam in FAMILIES}
    cases = list(every_storage_case(oracle))
    assert len({(m.name, w) for m, w, _ in cases}) == len(cases) == 600 + 10 + 4 + 6 + 2
    for mat, w, schemes in cases:
        assert mat.ptr[0] == 0 and mat.ptr[-1] == len(mat.col) and len(mat.col) > 0 and mat.col.min() >= 0, mat.name
        assert mat.max_col(w) == mat.m - 1, (mat.name, "the largest column is not in the ELL part")
        ent, pad, kinds = mat.slots(w)
        oent, opad = oracle_slots(oracle, mat, w)
        assert np.array_equal(ent, oent) and np.array_equal(pad, opad), (mat.name, w, "placement differs from oracle.sell_pair_slots")
        assert np.all(pad[ent >= 0] == PAD) and np.all(ent[mat.n:] == -1) and np.all(pad[mat.n + (mat.n & 1):] == PAD), mat.name
        ell = mat.pos < w
        assert np.array_equal(np.sort(ent[ent >= 0]), np.flatnonzero(ell)), (mat.name, "not every ELL entry exactly once")
        fam = mat.name.split("_n")[0]
        if fam in stats:
            for k in kinds:
                stats[fam][k] += kinds[k]
            stats[fam][254] += int(np.count_nonzero(pad == PAD_UNSAFE))
            partner_real = (ent >= 0).reshape(-1, 2, w)[:, ::-1, :].reshape(-1, w)
            stats[fam][255] += int(np.count_nonzero((pad == PAD) & (ent < 0) & partner_real))        # 255 next to an entry
            stats[fam]["tail"] += int(np.count_nonzero(~ell))
        # decode(encode(A)) = A, in both storages where the values have a table
        for scheme in schemes:
            for dtype in DTYPES:
                ptr, col, val = mat.csr(dtype, scheme)
                deltas, values, max_col = tables(ptr, col, val, w)
                assert 1 <= len(deltas) <= 254 and max_col == mat.m - 1
                buf = encode_sell8(ptr, col, val, w, deltas, max_col, dtype, mat.slots(w))
                c, v = decode(buf, mat.n, w, deltas, dtype)
                assert np.array_equal(c, col[ell]) and v.tobytes() == val[ell].tobytes(), (mat.name, w, scheme)
                if scheme != "random":
                    assert 1 <= len(values) <= 255
                    buf = encode_sell8v(ptr, col, val, w, deltas, max_col, dtype, values, mat.slots(w))
                    c, v = decode(buf, mat.n, w, deltas, dtype, values)
                    assert np.array_equal(c, col[ell]) and v.tobytes() == val[ell].tobytes(), (mat.name, w, scheme)
                tp, tc, tv = split_tail(ptr, col, val, w)
                assert tp[-1] == len(tc) == np.count_nonzero(~ell) and np.array_equal(tc, col[~ell]) and np.array_equal(np.diff(tp), np.maximum(mat.lens - w, 0))
    assert stats["bands"]["same"] > 1000 and stats["bands"][254] > 0 and stats["bands"]["tail"] == 0, stats["bands"]
    assert stats["holes"]["merged"] > 1000 and stats["holes"][255] > 1000 and stats["holes"]["plain"] == 0, stats["holes"]
    assert stats["crossed"]["plain"] > 1000 and stats["crossed"]["same"] > 500, stats["crossed"]
    assert stats["tails"]["tail"] > 1000 and stats["long_row"]["tail"] >= 30 * LONG_ROW, (stats["tails"], stats["long_row"])
    assert stats["unsorted"]["merged"] > 0 and stats["unsorted"]["plain"] > 0 and stats["empty"][254] > 0 and stats["empty"]["same"] > 0, (stats["unsorted"], stats["empty"])
    assert all(s[255] > 0 for s in stats.values()), stats
    for w in WIDTHS:
        A = family(oracle, "bands", SIZES[-1], w)
        pad = A.slots(w)[1]
        assert w == 1 or (pad[0, 0] == PAD_UNSAFE and pad[A.n, :].tolist().count(PAD_UNSAFE) == 1), (w, "254 next to column 0 and next to max_col")
        A = family(oracle, "long_row", SIZES[-1], w)
        at = int(np.argmax(A.lens))
        assert A.lens[at] == w + LONG_ROW and A.ptr[at // 128 * 128 + 128] - A.ptr[at // 128 * 128] > WAVE_CAP and at == 300
        assert w > 8 or np.all(np.diff(A.ptr.astype(np.int64)[::128])[np.arange(len(A.ptr[::128]) - 1) != at // 128] <= WAVE_CAP)     # its neighbours stage
        A = family(oracle, "tails", SIZES[-1], w)
        assert np.count_nonzero(A.lens > w) > 100 and A.lens.max() <= w + 3
        A = family(oracle, "unsorted", SIZES[-1], w)
        assert w < 3 or np.any(np.diff(A.col.astype(np.int64))[A.pos[1:] > 0] < 0)
        A = family(oracle, "empty", SIZES[-1], w)
        assert np.all(A.lens[:130] == 0) and np.all(A.lens[512:1024] == 0) and A.lens[131] > 0 and A.lens[133] == 0 and A.lens[-1] > 0
        assert family(oracle, "wide", SIZES[-1], w).m > SIZES[-1] and family(oracle, "narrow", SIZES[-1], w).m < SIZES[-1]
        assert family(oracle, "crossed", SIZES[-1], w).m > SIZES[-1]
    A = family(oracle, "pools", SIZES[-1], 12)
    for scheme, count in (("pool1", 1), ("pool3", 3), ("pool255", 255), ("hash7", 7), ("diag5", 5)):
        v = A.values(scheme)
        assert len(np.unique(v.view(np.uint64))) == count and len(np.unique(v.astype(np.float32).view(np.uint32))) == count - (scheme == "pool255"), scheme
        assert scheme in ("pool1", "diag5") or (np.any(v.view(np.uint64) == 1 << 63) and np.any(v == (0.0 if scheme == "hash7" else SUB32)))
        assert scheme != "pool255" or (np.any(v.view(np.uint64) == 0) and np.any(v == SUB64))
    assert np.float32(SUB32) != 0 and np.float32(SUB32) < np.finfo(np.float32).tiny and 0 < SUB64 < np.finfo(np.float64).tiny and np.float32(SUB64) == 0

    # the limit matrices of the analyses
    for count in (254, 255):
        ptr, col, w = limit_diagonals(oracle, count, False)
        assert len(tables(ptr, col, np.zeros(len(col)), w)[0]) == count and w > count
        ptr, col, w = limit_diagonals(oracle, count, True)
        d = col.astype(np.int64) - np.arange(len(col))
        assert len(np.unique(d)) == count and w == 1 and max(len(np.unique(d[k:k + 256])) for k in range(0, len(d), 256)) <= 40
    ptr, col, w = limit_diagonals(oracle, 1080, True)
    d = col.astype(np.int64) - np.arange(len(col))
    assert len(np.unique(d)) == 1080 > HASH_SLOTS and max(len(np.unique(d[k:k + 256])) for k in range(0, len(d), 256)) <= 40
    for dtype in DTYPES:
        for count in (255, 256):
            for spread in (False, True):
                ptr, val, w = limit_values(count, spread, dtype)
                assert len(np.unique(val.view(BITS[dtype]))) == count and val.dtype == dtype
                assert not spread or max(len(np.unique(val[k:k + 256])) for k in range(0, len(val), 256)) <= 40
    for ptr, col, val, storage in fused_matrices(oracle):
        w = oracle.hell_width(ptr)
        deltas, values, _ = tables(ptr, col, val, w)
        assert (len(deltas) <= 254, len(values) <= 255) == {"sell8v": (True, True), "sell8": (True, False), "sell32": (False, False)}[storage]
    for dtype in DTYPES:
        for name, ptr, col, val, row_length in fused_limit_matrices(oracle, dtype):
            w = oracle.hell_width(ptr)
            deltas, values, _ = tables(ptr, col, val, w)
            assert w == row_length == np.diff(ptr).max() and val.dtype == dtype and len(col) == len(val) == ptr[-1], name
            assert "%d diagonals" % len(deltas) in name or "%d values" % len(values) in name or "all-ones" in name, (name, len(deltas), len(values))

    # launch geometry
    for nb in (1, 2, 4, 13):
        geo = strip_geometry(nb)
        visited = strip_visits(*geo, nb)
        assert visit_once(visited, nb) and np.any(visited < 0) and geo[0] % 8 == 0 and 8 * geo[1] > geo[3], nb
        assert visit_once(np.arange(nb - 1, -1, -1), nb) and visit_once(holey_map(nb), nb) and np.all(holey_map(nb)[::2] == -1)
    assert strip_geometry(13) == (32, 2, 2, 7)
    for chunk, geo in STRIPS47.items():
        visited = strip_visits(*geo, 47)
        assert visit_once(visited, 47) and geo[0] == 5 * 8 * chunk and 8 * chunk > geo[3] and np.count_nonzero(visited < 0) == geo[0] - 47
        for run in (r for r in (1, 2, 4) if chunk % r == 0):
            visited, runs = march_visits(47, run, geo)
            assert visit_once(visited, 47) and len(runs) == geo[0] // run, (chunk, run)
            assert any(c <= 0 for _, c in runs)
        assert not visit_once(march_visits(47, 2, (geo[0], chunk, 5, 9))[0], 47)
    runs4 = march_visits(47, 4, STRIPS47[4])[1]
    assert (8, 2) in runs4 and (44, 3) in runs4 and (12, -2) in runs4      # cut by the plane end, by the matrix end, a workgroup without a slice
    for ns in (13, 47):
        for run in MARCH_RUNS:
            visited, runs = march_visits(ns, run)
            assert visit_once(visited, ns) and len(runs) == (ns + run - 1) // run and all(c > 0 for _, c in runs)
    assert not visit_once([0, 1, 1], 3) and not visit_once([0, 2, -1], 3) and not visit_once([0, 1, 2, 3], 3) and not visit_once([0, 1, 2, -2], 3)

    # the halo role: the kernel's block-to-slice mapping against hand-written expectations, and every strip's matrices -- full
    # width without a CSR tail, the intended reach, slices that repeat where a dictionary is wanted, every launch's geometry, and
    # the three kinds of gather in the slices that take the inner gather
    assert sorted(HALO_EXPECT) == sorted(STRIPS) and {s for s, _, _ in halo_cases()} == set(STRIPS.values())
    for name, strip in STRIPS.items():
        visits = halo_visits(strip.ns, strip.edge, strip.lower, strip.upper)
        assert visits == HALO_EXPECT[name] and visit_once([so for so, _, _ in visits], strip.ns), name
    assert halo_visits(5, 2, True, False) == [(2, False, False), (3, False, False), (4, False, False), (0, True, False), (1, True, False)]
    assert halo_visits(3, 2, True, True) == [(0, True, False), (1, True, True), (2, False, True)]      # elo = 2, ehi = 1; the short-strip rule: slice 1 is within two slices of both ends
    assert halo_visits(1, 1, True, True) == [(0, True, True)] and halo_visits(2, 3, False, True) == [(0, False, True), (1, False, True)]
    codes = np.full((2 * SLICE, 2), PAD, dtype=np.uint8)
    codes[SLICE:SLICE + 4] = [[3, 255], [3, 4], [254, 7], [9, 8]]          # lane 0: one diagonal | 255 beside an entry; lane 1: 254 beside an entry | two diagonals
    assert gather_kinds(codes, [1]) == (1, 2, 1) and gather_kinds(codes, [0]) == (0, 0, 0)
    halo_checked = 0
    for strip, w, use_dict in halo_cases():
        seen = np.zeros(3, dtype=np.int64)
        fams = halo_families(strip, w)
        assert "bands" in fams and ("crossed" in fams or strip.reach == 1) and ("holes" in fams) == (2 * strip.rows >= strip.n), (strip.name, w, fams)
        for fam in fams:
            mat = strip_matrix(oracle, strip, fam, w)
            inner = halo_geometry(strip, mat)
            assert len(inner) == max(0, strip.ns - strip.edge * (strip.lower + strip.upper)), (mat.name, inner)
            assert mat.n == strip.n and oracle.hell_width(mat.ptr) == w == mat.lens.max(), (mat.name, oracle.hell_width(mat.ptr))
            assert np.all(mat.lens[:strip.lo] == 0) and np.all(mat.lens[strip.lo + strip.rows:] == 0) and mat.col.max() < strip.n
            if fam == "bands" and w > 1:                                                      # how far into the ghost ranges the entries reach
                assert mat.col.min() == max(0, strip.lo - strip.reach) and mat.col.max() == min(strip.n - 1, strip.lo + strip.rows - 1 + strip.reach), mat.name
                assert strip.reach < strip.halo or (mat.col.min() == 0 and mat.col.max() == strip.n - 1), mat.name      # ... to their first and last elements
            for kind in ("sell8", "sell8v"):
                ptr, col, val = mat.csr(np.float64, halo_schemes(kind, use_dict))
                deltas, values, max_col = tables(ptr, col, val, w)
                assert np.abs(deltas).max() == strip.reach and len(deltas) <= 254 and (kind == "sell8" or len(values) <= 255), (mat.name, kind)
                if use_dict:
                    buf = encode_sell8v(ptr, col, val, w, deltas, max_col, np.float64, values, mat.slots(w)) if kind == "sell8v" else \
                        encode_sell8(ptr, col, val, w, deltas, max_col, np.float64, mat.slots(w)).reshape(strip.n // SLICE, -1)[:, :(w + 1) // 2 * 1024]
                    reps = first_appearance(buf.reshape(strip.n // SLICE, -1))[1]
                    assert strip.n // SLICE >= 64 and 2 <= len(reps) and 4 * len(reps) <= strip.n // SLICE, (mat.name, kind, len(reps))
            k = np.array(gather_kinds(_coded(ptr, col, w, deltas, max_col, mat.slots(w))[2], inner))
            assert not inner or k[HALO_FAMILIES.index(fam)] > 0, (mat.name, k.tolist())
            seen += k
            halo_checked += 1
        assert strip.ns < 2 * strip.edge or strip.reach == 1 or np.all(seen > 0), (strip.name, w, seen.tolist())
    assert halo_checked == 16 * 3 + 2 + 3 + 3 * 2 + 4 * 3
    seams = strip_matrix(oracle, STRIPS["seams"], "bands", 3)                 # the +-1 diagonals cross both seams inside one lane
    lo, end = STRIPS["seams"].lo, STRIPS["seams"].lo + STRIPS["seams"].rows
    assert seams.col[seams.ptr[lo]] == lo - 1 and seams.col[seams.ptr[end - 1] - 1] == end - 1 and seams.col[seams.ptr[end] - 1] == end

    # the plan restatement
    assert (march_span_bytes(0, 0, 8), march_span_bytes(-600, 600, 8), march_span_bytes(-1, 1, 4), march_lds_bytes(-600, 600, 8)) == (0, 12288, 2048, 44032)
    for which, (D, behind) in MARCH_SETS.items():
        for n in (N13, N47) if which in ("w3", "w7") else (N13,):
            A = march_matrix(oracle, which, n)
            w = len(D)
            ptr, col, val = A.csr(np.float64, "diag5")
            deltas, values, max_col = tables(ptr, col, val, w)
            assert deltas.tolist() == sorted(D) and A.lens.max() > w and max_col == A.m - 1
            assert (max_col > n - 1, max_col < n - 1) == (behind > 0, which == "w2")
            buf = encode_sell8v(ptr, col, val, w, deltas, max_col, np.float64, values, A.slots(w))
            ids, reps = first_appearance(buf.reshape((n + 511) // 512, -1))
            for vb in (8, 4):
                assert march_plan_host(deltas, ids, vb, max_col) == MARCH_EXPECT[which], which
            assert 2 * np.count_nonzero(np.diff(ids)) <= len(ids) and len(reps) <= 6
    lo, hi, far = MARCH_EXPECT["w7"]
    assert march_span_bytes(lo, hi, 8) == 3 * 4096 and len(far) == 2 and abs(far[0]) != abs(far[1])       # wider than a slice: the ring wraps
    assert march_plan_host((0,), [0] * 7, 8, 5) is None and march_plan_host((0,), [0, 1] * 6 + [0], 8, 5) is None
    assert march_plan_host((-4096, -2048, 0, 2048), [0] * 13, 8, 5) is None and march_plan_host((0,), [0] * 13, 8, 5, True) is None
    assert march_plan_host((-1024, 0, 513), [0] * 13, 8, 5) == (0, 513, [-1024]) and march_plan_host((-1024, 0, 512), [0] * 13, 8, 5) == (-1024, 512, [])

    # the oracle within the derived bound, on every matrix a product runs on
    checked = 0
    for mat, w, schemes in cases:
        if mat.name.split("_n")[0] in FAMILIES and w not in product_widths(mat.n):
            continue
        for m in with_and_without_tail(mat, w):
            for scheme in schemes:
                for dtype in DTYPES:
                    C = case_of(oracle, m, dtype, scheme)
                    used = np.bincount(m.col, minlength=m.m) > 0
                    assert len(C.x) == m.m and np.all(np.isnan(C.x[~used])) and np.all(np.isfinite(C.x[used])) and used[-1]
                    for mode in MODES:
                        y = C.reference(oracle, mode)
                        assert y.dtype == dtype and np.all(np.isfinite(y)) and not np.any(y == SENTINEL), (m.name, dtype, mode)
                        assert C.within_bound(y, mode), (m.name, np.dtype(dtype).name, scheme, mode)
                        checked += 1
    assert checked > 3000
