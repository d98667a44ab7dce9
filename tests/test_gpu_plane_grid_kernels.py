"""Direct parity tests of the plane and grid products -- vexcl_amd/csrc/plane.hip (`plane_walk`), plane32.hip (`plane32_walk`), grid.hip and
grid32.hip (both `grid_walk<V, ...>` of grid_walk.hpp), all four over the shared pieces of walk.hpp -- and of their plans, through the C ABI (`vexcl_amd.lib()`, `vexcl_amd._capi`) with torch tensors as device buffers.

What runs where
  * test_grid_products_on_hand_built_plans: `vexhip_spmv_sell8v_grid_f64` / `_f32` on plans filled by hand -- the geometry of
    `vexhip_sell8_grid_geometry` for the device's CU count with the fields under test overridden (depth, segments, threads, hot class,
    flat, store policy), tables encoded on the host from the header text -- for every case of GRID_CASES: `sell8_grid_kernel<0 | 1, AUX,
    256 | 512>` and `sell8_grid_f32_kernel<0 | 1, AUX>`, the fast groups, the slow steps, the `run == 64` continuation, the `cpx`
    dealing of flat plans, hand-cut segments.  No set-up code of the library is in the loop.
  * test_grid_store_policies_and_fp32_depths: the four store policies (every AUX) and VEXHIP_GRID32_DEPTH 1, 4, unset.
  * test_plane_products_on_hand_built_plans: `vexhip_spmv_sell8v_plane_f64_i32` / `_f32_i32` for PLANE_CASES in both forms of `decode`
    -- class tables (`table_pitch > 0`) and hand-packed SELL-512 code blocks (`table_pitch == 0`) of every width 1..8 --:
    `sell8_plane_kernel<2 | 4, 0 | 1, AUX, false, FLAT 0 | 1>`, `sell8_plane_f32_kernel<0 | 1, AUX>`.
  * test_plane_store_policies_and_fp32_depths: plan policies 0..3 (fp64), VEXHIP_PLANE_STORE 0..3 and VEXHIP_PLANE32_DEPTH (fp32).
  * test_alignment_of_x_and_y: x and y 8-byte but not 16-byte aligned (fp64 grid), at every 4-byte residue (fp32), refused by the fp64 plane product.
  * test_refusals_launch_nothing: every documented refusal returns its error and leaves y and its sentinels alone.
  * test_plans_called_directly, test_grid_plan_declines, test_plane_plan_declines, test_grid_plan_size_rules_at_two_to_the_23_rows,
    test_one_pass_build_limits: `vexhip_sell8_plane_plan`, `vexhip_sell8_grid_plan` (`grid_line_hash / table / verify_kernel`) on storage
    built by `vexhip_spmat_create_*`, field by field and byte by byte against `plane_plan_host` / `grid_plan_host`, the library's code
    blocks through `unpack_blocks`; the declines, the grid plan's size rules on matrices of 2^23 rows made on the device; the limits of
    the one-pass build (`grid_build_kernel`).
  * test_host_models_generators_and_geometries (no GPU): pins everything the GPU tests take for granted.
The module has no `pytestmark`: the last test has to run without a GPU, so every GPU test carries the `gpu` mark itself.

Why the comparisons are exact
  The four files are compiled with -ffp-contract=off.  A row's entries are folded in position order {-P, -nx, -1, 0, +1, +nx, +P}, which is
  the storage order of the CSR rows here, products rounded before they are added, the scale applied to the sum: the loop of
  `oracle.spmv_csr`.  A position without an entry adds a * (+0): a is entry 255 of the value table, +0.0, and x is replaced by a number
  whose exponent field is 0 and whose sign is +, so the term is +0 whatever x holds.  A sum that started at +0 is either not zero --
  adding +0 changes nothing -- or it is +0: (+0) + (-0) and an exact cancellation both give +0 under round-to-nearest, so a stored -0.0
  (whose product is -0 or +0) leaves +0 behind in the CSR loop too, and (+0) + (+0) = +0.  Every y is compared with `np.array_equal`
  (`equal_nan`) against the oracle in the matrix's own type.

The independent check
  The oracle shares its summation order with the kernels, so every finite result is also held against products and row sums in
  np.longdouble (fp64) / float64 (fp32): |y - y_hp| <= g (|alpha| sum_j |a_ij x_j| + |y0_i|), g = (L+2)u / (1 - (L+2)u), L <= 7, u = 2^-53 /
  2^-24: the bound of a recursive sum of L rounded products followed by one scaling and one addition.  Derived, not measured.  It assumes
  that no product underflows: where a subnormal matrix value meets an element of x, that element is +-0.25.

Canaries
  x is a view of exactly x_last + 1 elements inside a NaN-filled tensor; every element of x that no entry references is NaN (every
  third one +-Inf); a few elements that a stored 0.0 references are +-Inf, so those rows are NaN as in the CSR loop: the rows that are
  not finite must be exactly the ones the host predicts.  y sits between 64 sentinel elements on either side, compared as bytes after
  every call; before a `=` call y itself holds the sentinel, so a line no workgroup visits shows.  Class tables, line classes, code
  blocks, value and diagonal tables sit between guards.  All of these addresses lie inside live allocations.

Launch geometry
  The fast loops address x and y through buffer resources without a range check.  No product is launched before the host has shown,
  with restatements of `grid_launch` / `grid_workgroups` / `plane_launch` / `plane_workgroups` and of the `zh` rule of the walks, that
  every (plane, line, segment) is owned by exactly one workgroup (`visit_once`) and that every element a fast step of that workgroup
  may request or store lies inside x and y (`addresses_inside`).  depth, tile, threads, segments, pitch and store policy are not
  restated: they come from `vexhip_sell8_grid_geometry` / `vexhip_sell8_plane_geometry`, pinned in tests/test_capi_exports.py.

Left out
  `sell8v_runs_*`; the HALO forms of all four kernels (tests/test_gpu_distributed.py); the ZM = 2 addend (reachable through
  `vexhip_spmat_apply_axpby_*` only: tests/test_gpu_spmv.py test_product_with_a_vector_added_is_bit_identical).  The products of the
  plans of 2^23 rows are not run (the 208^3 case of tests/test_gpu_spmv.py does that at such a size).  The blocks the products run on
  are deliberately ones the library's fill would not produce (gaps, pad codes in the middle of a row); the packer is held against
  `oracle.sell_pair_slots` on the blocks that the fill does produce, and the unpacker against the library's own blocks.

The environment switches (VEXHIP_PLANE_FORCE, VEXHIP_GRID32_DEPTH, VEXHIP_PLANE32_DEPTH, VEXHIP_PLANE_STORE) are set inside `try` and
removed in `finally`, each time followed by `vexhip_reload_env`."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
HP = {np.float64: np.longdouble, np.float32: np.float64}          # the type of the independent reference
UNIT = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
BITS = {np.float64: np.uint64, np.float32: np.uint32}
MODES = ((1.0, False), (-0.75, True))                             # (alpha, append)
GUARD = 64                                                        # sentinel elements on either side of every y and every table
SENTINEL = 12345.0
ABSENT = 255                                                      # table byte of a position without an entry
INT_MAX = 2 ** 31 - 1
PL = 512                                                          # points per line of the plane product
SUB = {np.float64: 2.0 ** -1060, np.float32: 2.0 ** -140}         # a subnormal of either type
ZERO, MINUS_ZERO, SUBN = 8, 1, 2                                  # codes of the stored 0.0, of -0.0 and of the subnormal in the pool

every_dtype = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)


# ---------------------------------------------------------------------------------------------------------------------------
# matrices by grid line
# ---------------------------------------------------------------------------------------------------------------------------
def value_pool(dtype):
    """The value of every code: -0.0, a subnormal, repeated magnitudes, a stored +0.0; 16 more for the families with many classes."""
    head = [0.625, -0.0, SUB[dtype], -1.25, 1.25, 0.3125, 1.5, -0.875, 0.0, 2.5, -0.625]
    return np.array(head + [(j + 3) / 64.0 * (1 if j % 2 else -1) for j in range(16)], dtype=dtype)


def offsets(nx, ny):
    return np.array([-nx * ny, -nx, -1, 0, 1, nx, nx * ny], dtype=np.int64)


class GridMat:
    """An nx x ny x nz grid + `extra` lines (a ragged last plane).  want[line, position, row]: the value code wanted there (255: none);
    what would leave [0, x_last] is dropped, then equal lines form a class, numbered in order of first appearance."""

    def __init__(self, name, nx, ny, nz, extra, want, x_extra=0):
        self.name, self.nx, self.ny, self.extra = name, nx, ny, extra
        self.lines = ny * nz + extra
        self.nz = (self.lines + ny - 1) // ny
        self.n = self.lines * nx
        self.x_last = self.n - 1 + x_extra
        off = offsets(nx, ny)
        want = np.ascontiguousarray(want, dtype=np.uint8)
        assert want.shape == (self.lines, 7, nx)
        i = (np.arange(self.lines, dtype=np.int64)[:, None, None] * nx + np.arange(nx, dtype=np.int64)[None, None, :]) + off[None, :, None]
        want[(i < 0) | (i > self.x_last)] = ABSENT
        flat_lines = want.reshape(self.lines, 7 * nx)
        _, first, inverse = np.unique(flat_lines, axis=0, return_index=True, return_inverse=True)
        rank = np.argsort(np.argsort(first))                          # unique's number -> order of first appearance
        self.line_class = rank[inverse.reshape(-1)].astype(np.int32)
        self.classes = np.ascontiguousarray(flat_lines[np.sort(first)].reshape(-1, 7, nx))
        self.uses = np.bincount(self.line_class, minlength=len(self.classes))
        self._csr = {}

    def csr(self, dtype):
        """(ptr, col, val): the entries of a row in position order."""
        if dtype not in self._csr:
            sig = self.classes[self.line_class].transpose(0, 2, 1).reshape(self.n, 7)
            has = sig != ABSENT
            rows, pos = np.nonzero(has)
            col = (rows + offsets(self.nx, self.ny)[pos]).astype(np.int32)
            ptr = np.concatenate([[0], np.cumsum(has.sum(axis=1))]).astype(np.int32)
            self._csr[dtype] = (ptr, col, np.ascontiguousarray(value_pool(dtype)[sig[has]]))
        return self._csr[dtype]

    def hot(self, which):
        """A class number: 'most' = the first most frequent, 'least' = the first least frequent, 'unused' = one no line uses."""
        return {"most": int(np.argmax(self.uses)), "least": int(np.argmin(self.uses)), "unused": len(self.classes)}[which]

    def tables(self, pitch, hot):
        """(line_class[lines], table[classes][7][pitch]) as include/vexhip.h describes them; a hot class no line uses is an empty class."""
        ncls = max(len(self.classes), hot + 1)
        table = np.full((ncls, 7, pitch), ABSENT, dtype=np.uint8)
        table[:len(self.classes), :, :self.nx] = self.classes
        return self.line_class.copy(), table


def decode_tables(line_class, table, nx, ny, values):
    """The storage by grid line back to CSR."""
    sig = table[line_class][:, :, :nx].transpose(0, 2, 1).reshape(-1, 7)
    has = sig != ABSENT
    rows, pos = np.nonzero(has)
    return (np.concatenate([[0], np.cumsum(has.sum(axis=1))]).astype(np.int32), (rows + offsets(nx, ny)[pos]).astype(np.int32),
            np.ascontiguousarray(values[sig[has]]))


_MATS = {}
BAND = (3, 5, 10, 6, MINUS_ZERO, 7, 4)                              # a value code per position; -0.0 at +1


def _rand(seed, shape):
    return np.random.default_rng(seed).random(shape)


def grid_matrix(fam, nx, ny, nz, extra=0, x_extra=0):
    """bench: the benchmark's operator -- identity rows on the boundary, seven points inside: two classes.  natural: every neighbour
    inside the grid, a stored 0.0 at +P in plane 1, the subnormal at +1 in the lines y = 1: nine classes or more.  natural9: the same
    without the two extras: exactly nine on a whole grid.  bands: all seven positions in every row (+-1 crosses the line ends).
    bands5: the same without +-nx (a flat plan).  striped: bands whose centre value depends on the plane (three classes that cycle).
    pairs: bands whose centre value depends on the line's parity (the two lines of a tile differ).  alternate: ... on the plane's
    parity (a line changes between the hot and the other class inside a fast run).  holes: five classes with random
    entries removed, a row without entries, a row with +-P only.  diag: the centre alone (one class).  many<k>: the centre and +1 with
    k different pairs of centre values in the rows 0 and 1 (k classes).  ids: bands with such a pair per line (as many classes as lines)."""
    key = (fam, nx, ny, nz, extra, x_extra)
    if key in _MATS:
        return _MATS[key]
    lines = ny * nz + extra
    nzz = (lines + ny - 1) // ny
    ln = np.arange(lines)
    yy, zz, r = (ln % ny)[:, None, None], (ln // ny)[:, None, None], np.arange(nx)[None, None, :]
    p = np.arange(7)[None, :, None]
    want = np.full((lines, 7, nx), ABSENT, dtype=np.uint8)
    band = np.broadcast_to(np.array(BAND, dtype=np.uint8)[None, :, None], want.shape)
    if fam == "bench":
        inner = (r > 0) & (r < nx - 1) & (yy > 0) & (yy < ny - 1) & (zz > 0) & (zz < nzz - 1)
        want[:] = np.where(inner, np.where(p == 3, 9, 10), np.where(p == 3, 4, ABSENT))
    elif fam in ("natural", "natural9"):
        there = [zz > 0, yy > 0, r > 0, r >= 0, r < nx - 1, yy < ny - 1, zz < nzz - 1]
        code = np.array([0, 3, 5, 9, 5, 3, 0], dtype=np.uint8)
        for k in range(7):
            want[:, k, :] = np.where(np.broadcast_to(there[k], (lines, 1, nx))[:, 0, :], code[k], ABSENT)
        if fam == "natural":
            want[:, 6, :] = np.where((zz[:, 0, :] == 1) & (want[:, 6, :] != ABSENT), ZERO, want[:, 6, :])
            want[:, 4, :] = np.where((yy[:, 0, :] == 1) & (want[:, 4, :] != ABSENT), SUBN, want[:, 4, :])
    elif fam in ("bands", "bands5", "striped", "pairs", "alternate"):
        want[:] = band
        if fam == "bands5":
            want[:, (1, 5), :] = ABSENT
        if fam == "striped":
            want[:, 3, :] = np.array([0, 3, 5], dtype=np.uint8)[zz[:, 0, :] % 3]
        if fam == "alternate":
            want[:, 3, :] = np.array([6, 9], dtype=np.uint8)[zz[:, 0, :] % 2]
        if fam == "pairs":
            want[:, 3, :] = np.array([6, 9], dtype=np.uint8)[yy[:, 0, :] % 2]
    elif fam == "holes":
        K = 5
        cls = np.where(_rand(11, (K, 7, nx)) < 0.65, np.array(BAND, dtype=np.uint8)[None, :, None], ABSENT).astype(np.uint8)
        cls[:, 6, :] = np.where(cls[:, 6, :] != ABSENT, np.where(np.arange(nx) % 5 == 0, ZERO, 4), ABSENT)      # stored zeros at +P
        cls[:, 2, :] = np.where(cls[:, 2, :] != ABSENT, np.where(np.arange(nx) % 7 == 3, SUBN, 10), ABSENT)     # the subnormal at -1
        cls[0, :, 3] = ABSENT                                                                                   # an empty row
        cls[1, :, 4] = ABSENT
        cls[1, 0, 4] = cls[1, 6, 4] = 3                                                                         # +-P only
        want[:] = cls[(ln % ny + 2 * (ln // ny % 7 == 3)) % K]               # a class per line of the plane, others in the planes 3, 10, ..
    elif fam == "diag":
        want[:, 3, :] = 6
    elif fam == "ids":                                             # all seven positions, every line a class of its own (up to 256 lines)
        want[:] = band
        want[:, 3, 0] = 11 + ln % 16
        want[:, 3, 1] = 11 + (ln // 16) % 16
    elif fam.startswith("many"):
        k = int(fam[4:])
        want[:, 3, :] = 6
        want[:, 4, :nx - 1] = 10
        want[:, 3, 0] = 11 + (ln % k) % 16
        want[:, 3, 1] = 11 + (ln % k) // 16
    else:
        raise KeyError(fam)
    _MATS[key] = GridMat("%s_%dx%dx%d+%d+%d" % key, nx, ny, nz, extra, want, x_extra)
    return _MATS[key]


def limited_matrix(w, ny, nz, extra=0, x_extra=0):
    """512-point lines whose rows hold at most w entries (the code blocks of width w): four classes, a random subset per row."""
    key = ("limited", w, ny, nz, extra, x_extra)
    if key not in _MATS:
        lines = ny * nz + extra
        rank = np.argsort(np.argsort(_rand(100 + w, (4, 7, PL)), axis=1), axis=1)
        cls = np.where(rank < w, np.array(BAND, dtype=np.uint8)[None, :, None], ABSENT).astype(np.uint8)
        cls[:, 6, :] = np.where(cls[:, 6, :] != ABSENT, np.where(np.arange(PL) % 5 == 0, ZERO, 4), ABSENT)
        ln = np.arange(lines)
        _MATS[key] = GridMat("limited%d_%dx%d+%d+%d" % key[1:], PL, ny, nz, extra, cls[ln % ny % 2 + 2 * (ln // ny % 7 == 3)], x_extra)
    return _MATS[key]


# ---------------------------------------------------------------------------------------------------------------------------
# SELL-512 code blocks of the plane product (table_pitch == 0): ceil(w/2) KiB of diagonal codes, then as many value codes; the codes
# of ELL column j of row r: word (j >> 1) * 256 + (r >> 1), half j & 1, byte r & 1
# ---------------------------------------------------------------------------------------------------------------------------
def pack_blocks(classes, w, seed=5, fill_like=False):
    """One code block per class; the diagonal code of a position IS the position (the table holds all seven diagonals, sorted).  A row's
    entries ascend by position but sit in a random subset of the w columns: 254 / 255 in the gaps, with value codes that look valid; the
    unused half-word of an odd width holds codes that look valid too.  fill_like: the block as the library's fill leaves it where the two
    rows of a lane need no merging -- entries packed to the left, 255 for both codes of every other place (the CPU test holds such
    blocks against `oracle.sell_pair_slots`)."""
    ncls, _, nx = classes.shape
    assert nx == PL and 1 <= w <= 8
    wp = (w + 1) // 2
    dc = np.full((ncls, 2 * wp, PL), 254, dtype=np.uint8)
    dc[:, :, 1::2] = 255
    dc[:, 1::2, :] ^= 1                                             # pads: 254 and 255 in both rows of a pair and both halves
    vc = np.full((ncls, 2 * wp, PL), 5, dtype=np.uint8)              # (ignored behind a pad)
    if fill_like:
        dc[:], vc[:] = 255, 255
    rng = np.random.default_rng(seed)
    for c in range(ncls):
        for r in range(PL):
            pos = np.flatnonzero(classes[c, :, r] != ABSENT)
            assert len(pos) <= w, "a row of %d entries does not fit width %d" % (len(pos), w)
            cols = np.arange(len(pos)) if fill_like else np.sort(rng.permutation(w)[:len(pos)])
            dc[c, cols, r], vc[c, cols, r] = pos, classes[c, pos, r]
    if w % 2 and not fill_like:
        dc[:, w, :], vc[:, w, :] = 3, 6                              # looks like a diagonal entry: the kernel must not read it
    def words(a):                                                    # [class][column][row] -> [class][column pair][lane][half][byte]
        return np.ascontiguousarray(a.reshape(ncls, wp, 2, 256, 2).transpose(0, 1, 3, 2, 4)).reshape(ncls, wp * 1024)
    return np.ascontiguousarray(np.concatenate([words(dc), words(vc)], axis=1))


def oracle_block(oracle, mat, line, w):
    """The code block of the 512 rows of a line of a matrix as `oracle.sell_pair_slots` places their entries -- 255 for a place that is
    safe to load through, 254 for one that is not, value code 255 behind either, 255 in the unused half of an odd width -- byte by byte
    by the formula of include/vexhip.h."""
    ptr, col, _ = mat.csr(np.float64)
    sig = mat.classes[mat.line_class].transpose(0, 2, 1).reshape(mat.n, 7)
    vcode = sig[sig != ABSENT]
    off = offsets(PL, mat.ny).tolist()
    wp = (w + 1) // 2
    out = np.full(wp * 2048, 255, dtype=np.uint8)
    for r0 in range(line * PL, line * PL + PL, 2):
        slots = oracle.sell_pair_slots(ptr, col, r0, w, int(col.max()))
        for q in (0, 1):
            r = r0 + q - line * PL
            for j, e in enumerate(slots[q]):
                at = ((j >> 1) * 256 + (r >> 1)) * 4 + (j & 1) * 2 + (r & 1)
                if e == "unsafe":
                    out[at] = 254
                elif e != "safe":
                    out[at], out[wp * 1024 + at] = off.index(int(col[e]) - (r0 + q)), vcode[e]
    return out


def unpack_blocks(pool, w, pos_of=tuple(range(7))):
    """[class][7][512] class tables from code blocks, by the layout of include/vexhip.h; -1 where a row's positions do not ascend.
    pos_of: the position of every diagonal code (the blocks packed here hold all seven diagonals: the code is the position)."""
    wp = (w + 1) // 2
    ncls = pool.shape[0]
    out = np.full((ncls, 7, PL), ABSENT, dtype=np.int64)
    for c in range(ncls):
        for r in range(PL):
            last = -1
            for j in range(w):
                at = ((j >> 1) * 256 + (r >> 1)) * 4 + (j & 1) * 2 + (r & 1)
                d, v = int(pool[c, at]), int(pool[c, wp * 1024 + at])
                if d >= 254:
                    continue
                d = pos_of[d]
                out[c, d, r] = v if d > last else -1
                last = max(last, d)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# launch geometry restated: who owns what, and what a fast step may touch
# ---------------------------------------------------------------------------------------------------------------------------
class Launch:
    """The walks of one launch.  rows_per_lane 2 (fp64) | 4 (fp32); tile: lines per workgroup (grid: 2); segs / seg_len: the grid's
    segments (plane: one of 512); flat_walk: the kernel requests no lines above / below a tile."""

    def __init__(self, kind, nx, ny, nz, lines, x_last, depth, tile, segs, seg_len, threads, rows_per_lane, flat_walk, cpx_rule):
        self.kind, self.nx, self.ny, self.nz, self.lines, self.x_last = kind, nx, ny, nz, lines, x_last
        self.depth, self.tile, self.segs, self.seg_len, self.threads, self.rpl, self.flat_walk = depth, tile, segs, seg_len, threads, rows_per_lane, flat_walk
        self.n = lines * nx
        self.ytiles = (ny + 1) // 2 if kind == "grid" else ny // tile
        self.tiles = self.ytiles * segs
        self.tpx = (self.tiles + 7) // 8
        self.chunks = (nz + depth - 1) // depth
        self.cpx = (self.chunks + 7) // 8 if cpx_rule else 0          # grid_workgroups: flat plans deal walks, not tiles, to the XCDs
        self.workgroups = 8 * self.cpx * self.tiles if self.cpx else 8 * self.tpx * self.chunks

    def owner(self, b):
        """blockIdx -> (tile, chunk), or None where the workgroup leaves at once."""
        xcd, q = b & 7, b >> 3
        zc = q // self.tpx
        tile = xcd * self.tpx + (q - zc * self.tpx)
        if self.cpx:
            w = q // self.tiles
            tile, zc = q - w * self.tiles, xcd * self.cpx + w
        if tile >= self.tiles or zc * self.depth >= self.nz:
            return None
        return tile, zc

    def tile_geometry(self, tile):
        ytile, seg = divmod(tile, self.segs)
        y0 = self.tile * ytile
        nl = min(self.ny - y0, self.tile)
        row0 = seg * self.seg_len
        return y0, nl, row0, min(self.nx - row0, self.seg_len)

    def zh(self, tile, zc, append):
        """Planes [z, zh) of the walk may take fast steps (the rule of the four walks, restated)."""
        y0, _, row0, _ = self.tile_geometry(tile)
        zend = min(zc * self.depth + self.depth, self.nz)
        TY = self.tile
        if self.kind == "plane":
            xlines = (self.x_last + 1) // PL
            if xlines - 1 - TY - y0 < 0 or self.lines - TY - y0 < 0:
                return 0
            a = (xlines - 1 - TY - y0) // self.ny - 3
            bb = (self.lines - TY - y0) // self.ny - (1 if append else 0)
            return min(zend, a + 1, bb + 1)
        over = row0 + self.rpl * self.threads + 1
        xl_in = (self.x_last - over) // self.nx if self.x_last - over >= 0 else -1
        yl_in = (self.n - 1 - over) // self.nx if self.n - 1 - over >= 0 else -1

        def end_for(limit, ahead, line):
            v = limit - y0 - line
            return 0 if v < 0 else v // self.ny - ahead + 1
        e = min(end_for(xl_in, 3, TY), end_for(self.lines - 1, 0, TY - 1))
        if append:
            e = min(e, end_for(yl_in, 1, TY - 1))
        return min(zend, max(e, 0))


def visit_once(la):
    """Every (plane, line, segment) is owned by exactly one workgroup, every row of a line by one segment and one lane."""
    count = np.zeros((la.nz, la.tiles), dtype=np.int64)
    for b in range(la.workgroups):
        own = la.owner(b)
        if own is not None:
            tile, zc = own
            count[zc * la.depth:min(zc * la.depth + la.depth, la.nz), tile] += 1
    rows = np.zeros(la.nx, dtype=np.int64)
    lines = np.zeros(la.ny, dtype=np.int64)
    for tile in range(la.tiles):
        y0, nl, row0, ln = la.tile_geometry(tile)
        if ln <= 0 or nl <= 0 or ln > la.rpl * la.threads or row0 % 2:
            return False
        if y0 == 0:
            rows[row0:row0 + ln] += 1
        if row0 == 0:
            lines[y0:y0 + nl] += 1
    return bool((count == 1).all() and (rows == 1).all() and (lines == 1).all())


def addresses_inside(la, append):
    """Every element a fast step may request lies in x[0 .. x_last], every one it stores (or, '+=', reads one plane ahead) in y[0 .. n-1]:
    for every plane below `zh` of every walk, whatever classes the lines have.  Returns the number of such planes (-1: a request outside)."""
    fast = 0
    span = la.rpl * la.threads
    for tile in range(la.tiles):
        y0, nl, row0, ln = la.tile_geometry(tile)
        for zc in range(la.chunks):
            for z in range(zc * la.depth, la.zh(tile, zc, append)):
                at = lambda plane, line: (plane * la.ny + y0 + line) * la.nx + row0
                xs = [at(z + 3, 0), at(z + 3, la.tile - 1) + span - 1,                      # the centre lines three planes ahead
                      at(z + 2, 0) - 1, at(z + 2, la.tile - 1) + span]                      # the edge elements two planes ahead
                if not la.flat_walk:
                    xs += [at(z + 2, -1), at(z + 2, la.tile) + span - 1]                    # the lines above and below the tile
                ys = [at(z, 0), at(z, nl - 1) + ln - 1]
                if la.kind == "plane":
                    ys = [at(z, 0), at(z, la.tile - 1) + span - 1]
                if append:
                    ys += [at(z + 1, 0), at(z + 1, la.tile - 1) + span - 1]
                if min(xs) < 0 or max(xs) > la.x_last or min(ys) < 0 or max(ys) > la.n - 1:
                    return -1
                fast += 1
    return fast


def walk_features(la, line_class, hot, append):
    """The walks restated (which planes run in fast groups, which class is decoded when): {'fast': steps in groups of four, 'mixed': groups in which
    a line changes between the hot and the other class, 'run64': a look that found 64 planes, 'others': the most classes decoded within one walk, 'slow': slow steps}."""
    out = {"fast": 0, "run64": 0, "others": 0, "slow": 0, "mixed": 0}
    for tile in range(la.tiles):
        y0, nl, _, _ = la.tile_geometry(tile)
        look = nl if la.kind == "grid" else la.tile
        for zc in range(la.chunks):
            z, zend, zh, other, decoded = zc * la.depth, min(zc * la.depth + la.depth, la.nz), la.zh(tile, zc, append), -1, 0
            while z < zend:
                run = 0
                while run < 64 and z + run < zh and all(line_class[(z + run) * la.ny + y0 + l] in (hot, other) for l in range(look)):
                    run += 1
                if run >= 4:
                    out["mixed"] += sum(len({line_class[(z + k) * la.ny + y0 + l] == hot for k in range(run & ~3)}) == 2 for l in range(look))
                    out["fast"] += run & ~3
                    z += run & ~3
                    if run == 64:
                        out["run64"] += 1
                        continue
                if z >= zend:
                    break
                for l in range(look):
                    li = z * la.ny + y0 + l
                    if li < la.lines and line_class[li] not in (hot, other):
                        other, decoded = int(line_class[li]), decoded + 1
                out["slow"] += 1
                z += 1
            out["others"] = max(out["others"], decoded)
    return out


def f32_threads(segment_rows):
    return max(64, min(256, ((segment_rows + 3) // 4 + 63) // 64 * 64))


def grid_launch_of(g, mat, dtype, depth32=None):
    """The launch the grid product makes of a plan: fp64 walks the plan's depth with the plan's lanes; fp32 chooses lanes and depth itself
    (depth32: the value of VEXHIP_GRID32_DEPTH; None: unknown here -- the caller checks every depth)."""
    f64 = dtype == np.float64
    depth = g.depth if f64 else min(depth32, mat.nz)
    threads = g.threads if f64 else f32_threads(g.segment_rows)
    return Launch("grid", g.nx, g.lines_per_plane, g.planes, mat.lines, g.x_last, depth, 2, g.segments, g.segment_rows, threads, 2 if f64 else 4,
                  bool(g.flat), bool(g.flat))


def plane_launch_of(p, mat, dtype, depth32=None):
    f64 = dtype == np.float64
    tile = p.tile if f64 else 2
    return Launch("plane", PL, p.lines_per_plane, p.planes, mat.lines, p.x_last, p.depth if f64 else min(depth32, p.planes), tile, 1, PL, 256 if f64 else 128,
                  2 if f64 else 4, bool(f64 and p.flat and tile == 2), False)


def host_grid_check(g, n):
    """vexhip_sell8_grid_check restated (the CPU test holds the two against each other on every case)."""
    return bool(g.nx >= 8 and n > 0 and n % g.nx == 0 and g.lines_per_plane >= 2 and g.depth >= 1 and g.planes >= 1 and g.segments >= 1
                and 2 <= g.segment_rows <= 1024 and g.segment_rows % 2 == 0 and g.segments * g.segment_rows >= g.nx
                and 64 <= g.threads <= 512 and g.threads % 64 == 0 and 2 * g.threads >= g.segment_rows
                and (g.segments - 1) * g.segment_rows + 2 * g.threads <= g.pitch and g.pitch % 16 == 0
                and (n // g.nx + g.lines_per_plane - 1) // g.lines_per_plane == g.planes
                and (g.depth + 4) * g.lines_per_plane * g.nx * 8 < 2 ** 32)


def host_plane_check(p, n, w, f64):
    """plane.hpp plane_check restated, without the pointers."""
    tile = p.tile if f64 else 2
    return bool(p.usable and n > 0 and n % PL == 0 and 1 <= w <= 8 and (p.table_pitch == 0 or p.table_pitch >= PL + 2)
                and tile in (2, 4) and p.lines_per_plane >= 4 and p.lines_per_plane % tile == 0 and p.depth >= 1 and p.planes >= 1
                and (p.x_last + 1) % PL == 0 and (not f64 or (p.depth + 4) * p.lines_per_plane * 4096 < 2 ** 32) and p.x_last + 1 >= n)


# ---------------------------------------------------------------------------------------------------------------------------
# the fixed lists of geometries
# ---------------------------------------------------------------------------------------------------------------------------
def GC(name, fam, nx, ny, nz, extra=0, xk=None, hot="most", flat=0, **over):
    """A grid case; xk: x is longer than y, x_last = n - 1 + xk * nx + 3; over: fields of the plan written over the geometry's."""
    return (name, fam, nx, ny, nz, extra, xk, hot, flat, over)


GRID_CASES = (
    [GC("nx%d" % nx, "natural", nx, 3, 24, depth=8) for nx in (8, 9, 10, 11, 125, 130, 255, 256, 257, 514)]
    + [GC("nx1023", "bench", 1023, 2, 24, depth=8),
       GC("cut20", "bands", 20, 4, 24, depth=8, segments=3, segment_rows=8, threads=64),
       GC("cut300", "natural", 300, 3, 24, depth=8, segments=2, segment_rows=150, threads=128),
       GC("cut514", "bands", 514, 2, 24, depth=8, segments=2, segment_rows=258, threads=192)]
    + [GC("ny%d" % ny, "natural", 41, ny, 24, depth=8) for ny in (2, 3, 5, 17)]
    + [GC("nz%d-d%d" % (nz, d), "bench", 9, 4, nz, depth=d) for nz in (1, 2, 3) for d in (1, 4)]
    + [GC("nz9-d%d" % d, "natural", 9, 5, 9, depth=d) for d in (1, 3, 4, 7, 9)]
    + [GC("nz70-d70", "bench", 128, 4, 70, depth=70), GC("nz70-d4", "bands", 128, 4, 70, depth=4)]
    + [GC("ragged%d" % e, "bands", 9, 5, 24, extra=e, depth=8) for e in (1, 4)]
    + [GC("xlong%d" % k, "bands", 9, 5, 24, xk=k, depth=8) for k in (0, 1, 2)]
    + [GC("flat%d" % f, "bands5", 12, 4, 70, flat=f, depth=4) for f in (1, 0)]
    + [GC("hot-%s" % h, "natural", 9, 5, 24, hot=h, depth=8) for h in ("least", "unused")]
    + [GC("classes1", "diag", 9, 4, 24, depth=8), GC("classes2", "bench", 9, 4, 24, depth=8), GC("classes9", "natural9", 9, 3, 24, depth=8),
       GC("classes128", "many128", 9, 8, 17, depth=9)]
    + [GC("striped", "striped", 9, 4, 12, hot="unused", depth=12), GC("pairs", "pairs", 9, 4, 9, hot="unused", depth=9),
       GC("alternate", "alternate", 41, 5, 24, depth=8), GC("holes", "holes", 130, 5, 24, extra=1, depth=8), GC("holes-long", "holes", 125, 5, 24, xk=1, depth=8)])
GRID_IDS = [c[0] for c in GRID_CASES]
# the cases that take slow steps only (few planes, walks shorter than four planes, a class that changes with every plane); every other
# case takes fast steps in both types, '=' and '+=' (the CPU test holds the restated walks to that)
GRID_SLOW_ONLY = ("nz1-d1", "nz1-d4", "nz2-d1", "nz2-d4", "nz3-d1", "nz3-d4", "nz9-d1", "nz9-d3", "nz9-d4", "nz9-d7", "nz9-d9", "striped", "pairs", "classes128")


def PC(name, fam, ny, nz, extra=0, xk=0, hot="most", flat=0, form=0, **over):
    """A plane case; xk: x is longer than y by xk lines; form: 0 = class tables, w = code blocks of width w; fam 'limited': at most w
    entries per row."""
    return (name, fam, ny, nz, extra, xk, hot, flat, form, over)


PLANE_CASES = (
    [PC("ny4-t%d" % t, "bench", 4, 24, tile=t, depth=8) for t in (2, 4)] + [PC("ny8-t%d" % t, "natural", 8, 24, tile=t, depth=8) for t in (2, 4)]
    + [PC("ny18", "natural", 18, 15, tile=2, depth=5), PC("ny6", "bench", 6, 9, tile=2, depth=3)]
    + [PC("nz%d-d%d" % (nz, d), "bench", 4, nz, depth=d) for nz in (1, 2, 3) for d in (1, 4)]
    + [PC("nz9-d%d" % d, "natural", 4, 9, depth=d) for d in (1, 3, 4, 7, 9)]
    + [PC("nz70-d70", "bench", 4, 70, depth=70), PC("nz70-d4", "bands", 4, 70, depth=4)]
    + [PC("ragged%d" % e, "bands", 4, 24, extra=e, depth=8) for e in (1, 3)]
    + [PC("xlong%d" % k, "bands", 4, 24, xk=k, depth=8) for k in (1, 5)]
    + [PC("flat%d-t%d" % (f, t), "bands5", 4, 24, flat=f, tile=t, depth=8) for f, t in ((1, 2), (0, 2), (1, 4))]
    + [PC("hot-%s" % h, "natural", 8, 24, hot=h, depth=8) for h in ("least", "unused")]
    + [PC("striped", "striped", 4, 12, hot="unused", depth=12), PC("pairs", "pairs", 4, 9, hot="unused", depth=9), PC("holes", "holes", 4, 24, extra=1, depth=8),
       PC("alternate", "alternate", 4, 24, depth=8)]
    + [PC("blocks-w%d" % w, "limited", 4, 24, extra=(w % 2), xk=(w % 3), form=w, depth=8, tile=2 + 2 * (w % 2)) for w in range(1, 9)]
    + [PC("blocks-natural", "natural", 4, 24, form=7, depth=8), PC("blocks-nz70", "bench", 4, 70, form=8, depth=70),
       PC("blocks-striped", "striped", 4, 12, hot="unused", form=7, depth=12), PC("blocks-alternate", "alternate", 4, 24, form=7, depth=8)])
PLANE_IDS = [c[0] for c in PLANE_CASES]
PLANE_SLOW_ONLY = ("ny6", "nz1-d1", "nz1-d4", "nz2-d1", "nz2-d4", "nz3-d1", "nz3-d4", "nz9-d1", "nz9-d3", "nz9-d4", "nz9-d7", "nz9-d9", "striped", "pairs",
                   "blocks-striped")


def grid_case_matrix(case):
    _, fam, nx, ny, nz, extra, xk, _, _, _ = case
    return grid_matrix(fam, nx, ny, nz, extra, 0 if xk is None else xk * nx + 3)


def plane_case_matrix(case):
    _, fam, ny, nz, extra, xk, _, _, form, _ = case
    if fam == "limited":
        return limited_matrix(form, ny, nz, extra, xk * PL)
    return grid_matrix(fam, PL, ny, nz, extra, xk * PL)


def fill_grid(L, cus, mat, case):
    """The plan of a grid case: the library's geometry for `cus` compute units, the case's fields written over it."""
    from vexcl_amd import _capi
    g = _capi.Grid()
    L.sell8_grid_geometry(cus, mat.nx, mat.ny, mat.nz, ctypes.byref(g))
    assert g.depth >= 1 and g.usable == 0 and not g.table and not g.line_class
    for k, v in case[9].items():
        setattr(g, k, v)
    g.hot_class = mat.hot(case[7])
    g.classes = max(len(mat.classes), g.hot_class + 1)
    g.usable, g.flat, g.x_last = 1, case[8], mat.x_last
    return g


def fill_plane(L, cus, mat, case):
    from vexcl_amd import _capi
    p = _capi.Plane()
    L.sell8_plane_geometry(cus, mat.ny, mat.nz, ctypes.byref(p))
    assert p.depth >= 1 and p.usable == 0
    for k, v in case[9].items():
        setattr(p, k, v)
    p.hot_block = mat.hot(case[6])
    p.usable, p.flat, p.x_last = 1, case[7], mat.x_last
    p.table_pitch = 0 if case[8] else 528
    return p


# ---------------------------------------------------------------------------------------------------------------------------
# a case's vectors and references
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    _all = {}

    def __init__(self, oracle, mat, dtype):
        self.mat, self.dtype = mat, dtype
        ptr, col, val = mat.csr(dtype)
        self.csr = (ptr, col, val)
        n, m = mat.n, mat.x_last + 1
        seed = 1 + sum(map(ord, mat.name)) % 9973
        x = (oracle.random_f64(seed, m) - 0.5).astype(dtype)
        sub = (np.abs(val) < np.finfo(dtype).tiny) & (val != 0)
        x[col[sub]] = np.where(col[sub] % 2 == 0, 0.25, -0.25)
        zero_cols = np.unique(col[val == 0])
        x[zero_cols[3::41][:6]] = np.inf
        x[zero_cols[7::53][:3]] = -np.inf
        referenced = np.zeros(m, dtype=bool)
        referenced[col] = True
        free = np.flatnonzero(~referenced)
        x[free] = np.nan
        x[free[::3]] = np.inf
        x[free[1::6]] = -np.inf
        self.x, self.unreferenced = x, len(free)
        self.y0 = (oracle.random_f64(seed + 1, n) - 0.5).astype(dtype)
        rows = np.repeat(np.arange(n), np.diff(ptr))
        self.bad_rows = np.unique(rows[~np.isfinite(x[col])])           # the rows the host predicts not to be finite
        self.empty_rows = int((np.diff(ptr) == 0).sum())
        self._ref = {}
        hp = HP[dtype]
        with np.errstate(invalid="ignore"):
            prod = val.astype(hp) * x[col].astype(hp)
        prod[~np.isfinite(prod)] = 0
        full = np.diff(ptr) > 0
        self.hp_sum, self.hp_abs = np.zeros(n, dtype=hp), np.zeros(n, dtype=hp)
        if len(prod):
            self.hp_sum[full] = np.add.reduceat(prod, ptr[:-1][full])
            self.hp_abs[full] = np.add.reduceat(np.abs(prod), ptr[:-1][full])

    @classmethod
    def of(cls, oracle, mat, dtype):
        key = (mat.name, dtype)
        if key not in cls._all:
            cls._all[key] = cls(oracle, mat, dtype)
        return cls._all[key]

    def reference(self, oracle, mode):
        if mode not in self._ref:
            alpha, append = mode
            ptr, col, val = self.csr
            self._ref[mode] = oracle.spmv_csr(ptr, col, val, self.x, y=self.y0.copy() if append else None, alpha=alpha, append=append)
        return self._ref[mode]

    def within_bound(self, got, mode):
        alpha, append = mode
        hp, u = HP[self.dtype], UNIT[self.dtype]
        g = 9 * u / (1 - 9 * u)                                        # L + 2 with L = 7
        want = hp(alpha) * self.hp_sum + (self.y0.astype(hp) if append else 0)
        bound = g * (abs(alpha) * self.hp_abs + (np.abs(self.y0.astype(hp)) if append else 0))
        ok = np.ones(len(got), dtype=bool)
        ok[self.bad_rows] = False
        return bool(np.all(np.abs(got[ok].astype(hp) - want[ok]) <= bound[ok]))


def first_difference(got, want):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return "no difference" if len(bad) == 0 else "first differing row %d of %d (%d differ): got %r, want %r" % (
        bad[0], len(got), len(bad), got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def G(request):
    import torch                                        # before libvexhip.so: the process settles on torch's HIP runtime
    from vexcl_amd import _capi

    class NS:
        pass
    g = NS()
    g.torch, g.L, g.dev = torch, request.getfixturevalue("built_lib"), torch.device("cuda:0")
    g.up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(g.dev)
    g.stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(g.dev).cuda_stream)
    props = _capi.DeviceProps()
    g.L.device_get_props(0, ctypes.byref(props))
    g.cus = int(props.compute_units)
    return g


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _real(dtype):
    return ctypes.c_double if dtype == np.float64 else ctypes.c_float


def _sfx(dtype):
    return "f64" if dtype == np.float64 else "f32"


@contextlib.contextmanager
def environment(L, **settings):
    """Switches of the library for the calls inside; removed, and the snapshot retaken, on the way out."""
    try:
        for k, v in settings.items():
            if v is not None:
                os.environ[k] = str(v)
        L.reload_env()
        yield
    finally:
        for k in settings:
            os.environ.pop(k, None)
        L.reload_env()


def guarded(G, host_array):
    """A device copy of the array between two guards of GUARD elements: (whole tensor, view, host copy of the whole)."""
    flat = np.ascontiguousarray(host_array).reshape(-1)
    host = np.concatenate([np.full(GUARD, 77, dtype=flat.dtype), flat, np.full(GUARD, 77, dtype=flat.dtype)])
    whole = G.up(host)
    return whole, whole[GUARD:GUARD + len(flat)], host


class Vectors:
    """x, exactly x_last + 1 elements, at element offset 4 + x_shift of a NaN-filled tensor; y between sentinels at element offset
    GUARD + y_shift.  Shift 0: 16-byte aligned."""

    def __init__(self, G, C, x_shift=0, y_shift=0):
        self.G, self.C = G, C
        n, m, dtype = C.mat.n, len(C.x), C.dtype
        xbuf = np.full(m + 16, np.nan, dtype=dtype)
        xbuf[4 + x_shift:4 + x_shift + m] = C.x
        self.xbuf = G.up(xbuf)
        self.x = self.xbuf[4 + x_shift:4 + x_shift + m]
        self.y_at = GUARD + y_shift
        self.start, self.start_dev = {}, {}
        for mode in MODES:
            ybuf = np.full(n + 2 * GUARD + 8, SENTINEL, dtype=dtype)
            if mode[1]:
                ybuf[self.y_at:self.y_at + n] = C.y0
            self.start[mode], self.start_dev[mode] = ybuf, G.up(ybuf)
        size = np.dtype(dtype).itemsize
        assert self.xbuf.data_ptr() % 16 == 0 and self.x.data_ptr() % 16 == (x_shift * size) % 16
        assert self.start_dev[MODES[0]].data_ptr() % 16 == 0

    def run(self, call, mode):
        """call(x, y, alpha, append); returns the whole y tensor on the host."""
        ybuf = self.start_dev[mode].clone()
        call(self.x, ybuf[self.y_at:self.y_at + self.C.mat.n], mode[0], mode[1])
        return ybuf.cpu().numpy()

    def untouched(self, raw_call, text, what):
        """raw_call(x, y, alpha, append) -> (status, message): refused with `text`, y and its sentinels as they were."""
        for mode in MODES:
            ybuf = self.start_dev[mode].clone()
            rc, message = raw_call(self.x, ybuf[self.y_at:self.y_at + self.C.mat.n], mode[0], mode[1])
            assert rc != 0 and text in message, what + (mode, rc, message)
            assert ybuf.cpu().numpy().tobytes() == self.start[mode].tobytes(), what + (mode, "a refused call wrote")


def check_run(oracle, V, out, mode, what):
    """Equal to the oracle bit for bit (NaN where it is NaN), not finite exactly in the rows the host predicts, within the derived bound
    of the high-precision result elsewhere; every other byte of the tensor unchanged."""
    C, n = V.C, V.C.mat.n
    sl = slice(V.y_at, V.y_at + n)
    got, want = out[sl], C.reference(oracle, mode)
    assert np.array_equal(got, want, equal_nan=True), what + (first_difference(got, want),)
    assert np.array_equal(np.flatnonzero(~np.isfinite(got)), C.bad_rows), what + ("%d rows are not finite, %d predicted" % ((~np.isfinite(got)).sum(), len(C.bad_rows)),)
    assert C.within_bound(got, mode), what + ("outside the bound of the high-precision reference",)
    rest = out.copy()
    rest[sl] = V.start[mode][sl]
    assert rest.tobytes() == V.start[mode].tobytes(), what + ("a sentinel changed",)


def check_all(oracle, V, call, what):
    outs = {}
    for mode in MODES:
        outs[mode] = V.run(call, mode)
        check_run(oracle, V, outs[mode], mode, what + (mode,))
    return outs


def check_guards(tables, what):
    for whole, _, host in tables:
        assert whole.cpu().numpy().tobytes() == host.tobytes(), what + ("a table or its guard changed",)


def table256(entries, pad, np_dtype):
    out = np.full(256, pad, dtype=np_dtype)
    out[:len(entries)] = entries
    return out


def launches_to_check(make_launch, mat, dtype, depth32):
    """The launches a call may make: one, or -- fp32 with the library's own depth, which is not exported for the grid -- every depth."""
    if dtype == np.float64 or depth32 is not None:
        return [make_launch(depth32)]
    return [make_launch(d) for d in range(1, mat.nz + 1)]


def host_checks(launches, what):
    """`visit_once` and `addresses_inside`, for '=' and '+=': no product is launched unless both hold."""
    for la in launches:
        assert visit_once(la), what + ("depth %d" % la.depth, "not every line is owned by exactly one workgroup: no launch")
        for append in (False, True):
            assert addresses_inside(la, append) >= 0, what + ("depth %d" % la.depth, "a fast step would leave the arrays: no launch")


class GridRun:
    """A grid case on the device: the plan filled by hand, its tables between guards, the host checks done."""

    def __init__(self, G, oracle, case, dtype, depth32=None, **more):
        from vexcl_amd import _capi
        self.G, self.case, self.dtype, self.mat = G, case, dtype, grid_case_matrix(case)
        mat = self.mat
        self.C = Case.of(oracle, mat, dtype)
        self.g = g = fill_grid(G.L, G.cus, mat, case)
        for k, v in more.items():
            setattr(g, k, v)
        self.what = (case[0], np.dtype(dtype).name, "depth32 %r" % depth32)
        line_class, table = mat.tables(g.pitch, g.hot_class)
        self.tables = [guarded(G, line_class), guarded(G, table), guarded(G, table256(value_pool(dtype), 0.0, dtype))]
        g.line_class, g.table = self.tables[0][1].data_ptr(), self.tables[1][1].data_ptr()
        assert host_grid_check(g, mat.n) and g.x_last + 1 >= mat.n, self.what
        G.L.sell8_grid_check(ctypes.byref(g), mat.n)
        if dtype == np.float32:
            assert (min(depth32 or 1, mat.nz) + 4) * mat.ny * mat.nx * 4 < 2 ** 32
        host_checks(launches_to_check(lambda d: grid_launch_of(g, mat, dtype, d), mat, dtype, depth32), self.what)
        self.fn = getattr(G.L, "spmv_sell8v_grid_" + _sfx(dtype))
        self.raw = getattr(G.L.cdll, "vexhip_spmv_sell8v_grid_" + _sfx(dtype))

    def call(self, x, y, alpha, append):
        self.fn(0, self.G.stream(), self.mat.n, _real(self.dtype)(alpha), int(append), _vp(self.tables[2][1]), _vp(x), _vp(y), ctypes.byref(self.g))

    def raw_call(self, g=None, n=None, values=True):
        def call(x, y, alpha, append):
            rc = self.raw(0, self.G.stream(), self.mat.n if n is None else n, _real(self.dtype)(alpha), int(append),
                          _vp(self.tables[2][1]) if values else None, _vp(x), _vp(y), ctypes.byref(self.g if g is None else g))
            return rc, self.G.L.last_error().decode(errors="replace")
        return call


class PlaneRun:
    """A plane case on the device in the form the case names: class tables + line classes, or hand-packed code blocks + block numbers."""

    def __init__(self, G, oracle, case, dtype, depth32=None, check=True, **more):
        self.G, self.case, self.dtype, self.mat = G, case, dtype, plane_case_matrix(case)
        mat = self.mat
        self.C = Case.of(oracle, mat, dtype)
        self.p = p = fill_plane(G.L, G.cus, mat, case)
        for k, v in more.items():
            setattr(p, k, v)
        self.w = case[8] if case[8] else 7
        self.what = (case[0], np.dtype(dtype).name, "depth32 %r" % depth32)
        line_class, table = mat.tables(p.table_pitch or PL, p.hot_block)
        pool = pack_blocks(table[:, :, :PL], self.w) if case[8] else table
        deltas = table256(np.sort(offsets(PL, mat.ny)), INT_MAX, np.int32)
        self.tables = [guarded(G, line_class), guarded(G, pool), guarded(G, table256(value_pool(dtype), 0.0, dtype)), guarded(G, deltas)]
        self.fn = getattr(G.L, "spmv_sell8v_plane_%s_i32" % _sfx(dtype))
        self.raw = getattr(G.L.cdll, "vexhip_spmv_sell8v_plane_%s_i32" % _sfx(dtype))
        if check:
            assert host_plane_check(p, mat.n, self.w, dtype == np.float64), self.what
            if dtype == np.float32 and depth32 is None:
                depth32 = int(G.L.sell8_plane_f32_depth(G.cus, mat.ny, mat.nz))
                assert depth32 >= 1
            host_checks([plane_launch_of(p, mat, dtype, depth32)], self.what)

    def call(self, x, y, alpha, append):
        t = self.tables
        self.fn(0, self.G.stream(), self.mat.n, _real(self.dtype)(alpha), int(append), self.w, _vp(t[1][1]), _vp(t[0][1]), _vp(t[3][1]), _vp(t[2][1]),
                _vp(x), _vp(y), ctypes.byref(self.p))

    def raw_call(self, p=None, n=None, w=None, pool=True):
        def call(x, y, alpha, append):
            t = self.tables
            rc = self.raw(0, self.G.stream(), self.mat.n if n is None else n, _real(self.dtype)(alpha), int(append), self.w if w is None else w,
                          _vp(t[1][1]) if pool else None, _vp(t[0][1]), _vp(t[3][1]), _vp(t[2][1]), _vp(x), _vp(y), ctypes.byref(self.p if p is None else p))
            return rc, self.G.L.last_error().decode(errors="replace")
        return call


def copy_of(plan, **fields):
    other = type(plan)()
    ctypes.memmove(ctypes.byref(other), ctypes.byref(plan), ctypes.sizeof(plan))
    for k, v in fields.items():
        setattr(other, k, v)
    return other


def case_named(cases, name):
    return [c for c in cases if c[0] == name][0]


# ---------------------------------------------------------------------------------------------------------------------------
# products on hand-built plans
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@every_dtype
@pytest.mark.parametrize("case", GRID_CASES, ids=GRID_IDS)
def test_grid_products_on_hand_built_plans(G, oracle, dtype, case):
    """fp64 walks the depth written into the plan; fp32 takes its depth from VEXHIP_GRID32_DEPTH, set to the same number."""
    depth32 = case[9].get("depth") if dtype == np.float32 else None
    with environment(G.L, VEXHIP_GRID32_DEPTH=depth32):
        R = GridRun(G, oracle, case, dtype, depth32)
        outs = check_all(oracle, Vectors(G, R.C), R.call, R.what)
        check_guards(R.tables, R.what)
        if case[0] == "flat1":                                       # the same matrix walked as a flat plan and not: the same bytes
            R0 = GridRun(G, oracle, case_named(GRID_CASES, "flat0"), dtype, depth32)
            assert R0.C is R.C
            for mode in MODES:
                assert Vectors(G, R0.C).run(R0.call, mode).tobytes() == outs[mode].tobytes(), R.what + (mode, "flat = 0 differs")


@gpu
@every_dtype
def test_grid_store_policies_and_fp32_depths(G, oracle, dtype):
    for name in ("nx130", "nx514", "holes"):
        case = case_named(GRID_CASES, name)
        for policy in range(4):
            for depth32 in ((None,) if dtype == np.float64 else (1, 4, None)):
                with environment(G.L, VEXHIP_GRID32_DEPTH=depth32):
                    R = GridRun(G, oracle, case, dtype, depth32, store_policy=policy)
                    check_all(oracle, Vectors(G, R.C), R.call, R.what + ("policy %d" % policy,))


@gpu
@every_dtype
@pytest.mark.parametrize("case", PLANE_CASES, ids=PLANE_IDS)
def test_plane_products_on_hand_built_plans(G, oracle, dtype, case):
    """fp64 walks the plan's depth and tile; fp32 takes tiles of two lines and its depth from VEXHIP_PLANE32_DEPTH, set to the plan's."""
    depth32 = case[9].get("depth") if dtype == np.float32 else None
    with environment(G.L, VEXHIP_PLANE32_DEPTH=depth32):
        if case[0] == "ny6":                                         # six lines per plane: tiles of four must be refused, tiles of two run
            R4 = PlaneRun(G, oracle, case, np.float64, check=False, tile=4)
            assert not host_plane_check(R4.p, R4.mat.n, R4.w, True)
            Vectors(G, R4.C).untouched(R4.raw_call(), "bad plane plan", R4.what)
        R = PlaneRun(G, oracle, case, dtype, depth32)
        outs = check_all(oracle, Vectors(G, R.C), R.call, R.what)
        check_guards(R.tables, R.what)
        if case[0] == "flat1-t2":
            R0 = PlaneRun(G, oracle, case_named(PLANE_CASES, "flat0-t2"), dtype, depth32)
            for mode in MODES:
                assert Vectors(G, R0.C).run(R0.call, mode).tobytes() == outs[mode].tobytes(), R.what + (mode, "flat = 0 differs")


@gpu
@every_dtype
def test_plane_store_policies_and_fp32_depths(G, oracle, dtype):
    """The fp64 product takes the policy from the plan; the fp32 product reads VEXHIP_PLANE_STORE at the launch."""
    for name in ("ny8-t2", "ny8-t4", "flat1-t2", "blocks-w5", "holes"):
        case = case_named(PLANE_CASES, name)
        for policy in range(4):
            for depth32 in ((None,) if dtype == np.float64 else (1, 4, None)):
                with environment(G.L, VEXHIP_PLANE32_DEPTH=depth32, VEXHIP_PLANE_STORE=policy if dtype == np.float32 else None):
                    R = PlaneRun(G, oracle, case, dtype, depth32, store_policy=policy)
                    check_all(oracle, Vectors(G, R.C), R.call, R.what + ("policy %d" % policy,))


@gpu
@every_dtype
def test_alignment_of_x_and_y(G, oracle, dtype):
    """fp64 grid: x, y and both one element off (8-byte, not 16-byte aligned); fp32 grid and plane: every 4-byte residue; the fp64 plane
    product refuses such vectors and writes nothing."""
    shifts = (1,) if dtype == np.float64 else (1, 2, 3)
    for name in ("nx9", "nx125", "nx130", "cut300", "holes"):
        R = GridRun(G, oracle, case_named(GRID_CASES, name), dtype, 4 if dtype == np.float32 else None)
        with environment(G.L, VEXHIP_GRID32_DEPTH=4 if dtype == np.float32 else None):
            for s in shifts:
                for xs, ys in ((s, 0), (0, s), (s, s)):
                    check_all(oracle, Vectors(G, R.C, xs, ys), R.call, R.what + ("x shift %d" % xs, "y shift %d" % ys))
    for name in ("ny8-t2", "blocks-w5"):
        R = PlaneRun(G, oracle, case_named(PLANE_CASES, name), dtype, 4 if dtype == np.float32 else None)
        with environment(G.L, VEXHIP_PLANE32_DEPTH=4 if dtype == np.float32 else None):
            for s in shifts:
                for xs, ys in ((s, 0), (0, s), (s, s)):
                    V = Vectors(G, R.C, xs, ys)
                    if dtype == np.float64:
                        V.untouched(R.raw_call(), "must be 16-byte aligned", R.what + (xs, ys))
                    else:
                        check_all(oracle, V, R.call, R.what + ("x shift %d" % xs, "y shift %d" % ys))


@gpu
@every_dtype
def test_refusals_launch_nothing(G, oracle, dtype):
    R = GridRun(G, oracle, case_named(GRID_CASES, "nx130"), dtype, 4 if dtype == np.float32 else None)
    V, g, n = Vectors(G, R.C), R.g, R.mat.n
    for text, call in (("bad grid product arguments", R.raw_call(copy_of(g, usable=0))),
                       ("bad grid product arguments", R.raw_call(copy_of(g, table=None))),
                       ("bad grid product arguments", R.raw_call(copy_of(g, line_class=None))),
                       ("bad grid product arguments", R.raw_call(values=False)),
                       ("bad grid plan", R.raw_call(n=n - 1)),                               # n no multiple of nx
                       ("bad grid plan", R.raw_call(copy_of(g, planes=g.planes + 1))),
                       ("bad grid plan", R.raw_call(n=n - g.nx * g.lines_per_plane)),         # planes inconsistent with n
                       ("bad grid plan", R.raw_call(copy_of(g, pitch=2 * g.threads - 16))),
                       ("bad grid plan", R.raw_call(copy_of(g, threads=96))),
                       ("bad grid plan", R.raw_call(copy_of(g, segment_rows=g.segment_rows - 1))),
                       ("bad grid plan", R.raw_call(copy_of(g, depth=0))),
                       ("bad grid plan", R.raw_call(copy_of(g, x_last=n - 2)))):
        V.untouched(call, text, R.what + (text,))
    R = PlaneRun(G, oracle, case_named(PLANE_CASES, "ny8-t2"), dtype, 4 if dtype == np.float32 else None)
    V, p, n = Vectors(G, R.C), R.p, R.mat.n
    refusals = [("bad plane product arguments", R.raw_call(copy_of(p, usable=0))),
                ("bad plane product arguments", R.raw_call(pool=False)),
                ("bad plane product geometry", R.raw_call(n=n - 1)),
                ("bad plane product geometry", R.raw_call(w=9)),
                ("bad plane product geometry", R.raw_call(w=0)),
                ("bad plane plan (table pitch)", R.raw_call(copy_of(p, table_pitch=513))),
                ("bad plane plan", R.raw_call(copy_of(p, x_last=p.x_last - 1))),
                ("bad plane plan", R.raw_call(copy_of(p, depth=0))),
                ("bad plane plan", R.raw_call(copy_of(p, lines_per_plane=2)))]
    if dtype == np.float64:
        refusals.append(("bad plane plan", R.raw_call(copy_of(p, tile=3))))
    with environment(G.L, VEXHIP_PLANE32_DEPTH=4 if dtype == np.float32 else None):
        for text, call in refusals:
            V.untouched(call, text, R.what + (text,))


# ---------------------------------------------------------------------------------------------------------------------------
# the plans restated
# ---------------------------------------------------------------------------------------------------------------------------
def csr_signatures(ptr, col, val, nx, far):
    """(sig[n][7], ascending): the code of every row's value at every position -- values numbered by bit pattern as unsigned integers,
    the order of the value table of the SELL-512 storage -- and whether every row's positions ascend."""
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    d = col.astype(np.int64) - rows
    pos = np.full(len(d), -1, dtype=np.int64)
    for p, o in enumerate((-far, -nx, -1, 0, 1, nx, far)):
        pos[d == o] = p
    assert (pos >= 0).all()
    bits = np.ascontiguousarray(val).view(BITS[val.dtype.type])
    code = np.searchsorted(np.unique(bits), bits)
    same_row = rows[1:] == rows[:-1]
    ascending = bool(np.all(pos[1:][same_row] > pos[:-1][same_row]))
    sig = np.full((n, 7), ABSENT, dtype=np.uint8)
    sig[rows, pos] = code
    return sig, ascending


def first_appearance(keys):
    """Numbers in order of first appearance for the rows of a 2-D array: (number per row, representatives' indices)."""
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    rank = np.argsort(np.argsort(first))
    return rank[inverse.reshape(-1)].astype(np.int32), np.sort(first)


def grid_diagonals_host(L, diagonals, rows):
    """grid.hip grid_diagonals from the header text: (nx, far) or None."""
    mags = sorted({abs(int(d)) for d in diagonals if d != 0})
    if len(mags) == 2 and mags[0] == 1:
        W = mags[1]
        if W < 16 or rows % W or W > 2 ** 30:
            return None
        nx = int(L.sell8_grid_virtual_line(W))
        return (nx, W) if nx >= 8 else None
    if len(mags) != 3 or mags[0] != 1:
        return None
    nx, far = mags[1], mags[2]
    if nx < 8 or far % nx or far // nx < 2 or rows % nx or far > 2 ** 30:
        return None
    return nx, far


def grid_plan_host(L, ptr, col, val, x_last, ell_width, tail_nnz, value_bytes=None, force=True, threshold=2 ** 23):
    """vexhip_sell8_grid_plan from the header text: None where it declines, else the fields the text defines.  threshold: the rows below
    which the plan declines without FORCE (the CPU test lowers it to reach the two size rules behind it on small examples)."""
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    diagonals = np.unique(col.astype(np.int64) - rows)
    if (value_bytes or val.dtype.itemsize) not in (4, 8) or not 4 <= len(diagonals) <= 7:
        return None
    if not 1 <= ell_width <= 8 or tail_nnz or n < 8 or (n < threshold and not force):
        return None
    if x_last + 1 < n or x_last >= 2 ** 31:
        return None
    geo = grid_diagonals_host(L, diagonals, n)
    if geo is None:
        return None
    nx, far = geo
    ny, lines = far // nx, n // nx
    nz = (lines + ny - 1) // ny
    if nz < 4 and not force:
        return None
    sig, ascending = csr_signatures(ptr, col, val, nx, far)
    if not ascending:
        return None
    by_line = np.ascontiguousarray(sig.reshape(lines, nx, 7).transpose(0, 2, 1)).reshape(lines, 7 * nx)
    line_class, reps = first_appearance(by_line)
    if len(reps) > 128:
        return None
    uses = np.bincount(line_class)
    hot = int(np.argmax(uses))
    if (lines - uses[hot]) * 4 > lines and not force:
        return None
    return {"nx": nx, "lines_per_plane": ny, "planes": nz, "hot_class": hot, "classes": len(reps), "x_last": x_last,
            "flat": int(-nx not in diagonals and nx not in diagonals), "line_class": line_class, "table": by_line[reps].reshape(-1, 7, nx)}


def plane_plan_host(ptr, col, val, x_last, ell_width, tail_nnz, blocks, dictionary_blocks, value_bytes=None, force=True):
    """vexhip_sell8_plane_plan from the header text (the blocks and their numbers are the dictionary's): None where it declines."""
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    diagonals = np.unique(col.astype(np.int64) - rows)
    nslices = n // PL
    if (value_bytes or val.dtype.itemsize) not in (4, 8) or not 2 <= len(diagonals) <= 7 or not 1 <= dictionary_blocks <= 128:
        return None
    if not 1 <= ell_width <= 8 or tail_nnz or n != nslices * PL or (nslices < 64 and not force):
        return None
    if x_last < 0 or (x_last + 1) % PL or x_last + 1 < n:
        return None
    fars = {abs(int(d)) for d in diagonals} - {0, 1, PL}
    if len(fars) != 1:
        return None
    far = fars.pop()
    if far < 4 * PL or far % (2 * PL) or far > 2 ** 30:
        return None
    ny = far // PL
    nz = (nslices + ny - 1) // ny
    if nz < 4 and not force:
        return None
    if not csr_signatures(ptr, col, val, PL, far)[1]:
        return None
    if blocks.min() < 0 or blocks.max() >= dictionary_blocks:
        return None
    uses = np.bincount(blocks, minlength=dictionary_blocks)
    hot = int(np.argmax(uses))
    if (nslices - uses[hot]) * 16 > nslices and not force:
        return None
    return {"lines_per_plane": ny, "planes": nz, "hot_block": hot, "x_last": x_last, "flat": int(PL not in diagonals and -PL not in diagonals),
            "table_pitch": 0}


# ---------------------------------------------------------------------------------------------------------------------------
# the plans called directly on storage the library built
# ---------------------------------------------------------------------------------------------------------------------------
class Built:
    """The SELL-512 value-coded storage of a CSR matrix from vexhip_spmat_create_* (no one-pass build, no plans of its own).  The arrays
    are numpy arrays or, for the matrices of 2^23 rows, torch tensors made on the device (fp64, 32-bit row pointers)."""

    def __init__(self, G, ptr, col, val, flags=0, fmt=None, p64=False):
        from vexcl_amd import _capi
        self.G, self.csr = G, (ptr, col, val)
        if isinstance(val, np.ndarray):
            self.dtype = val.dtype.type
            self.dev = (G.up(ptr.astype(np.int64) if p64 else ptr), G.up(col), G.up(val))
        else:
            self.dtype, self.dev = np.float64, (ptr, col, val)
        self.value_bytes = np.dtype(self.dtype).itemsize
        self.A = ctypes.c_void_p()
        fn = getattr(G.L, "spmat_create_%s_%s" % (_sfx(self.dtype), "p64" if p64 else "i32"))
        fn(0, G.stream(), len(ptr) - 1, _vp(self.dev[0]), _vp(self.dev[1]), _vp(self.dev[2]), _capi.SPMAT_SELL8V if fmt is None else fmt,
           flags, ctypes.byref(self.A))
        self.info = _capi.SpMatInfo()
        G.L.spmat_get_info(self.A, ctypes.byref(self.info))
        G.torch.cuda.synchronize()

    def close(self):
        if self.A:
            self.G.L.spmat_destroy(self.A)
            self.A = ctypes.c_void_p()

    def read(self, address, count, np_dtype):
        host = np.empty(count, dtype=np_dtype)
        self.G.L.memcpy_d2h(0, ctypes.c_void_p(host.ctypes.data), ctypes.c_void_p(address), host.nbytes, None, 1)
        return host

    def apply(self, x, y, alpha, append):
        dtype = self.dtype
        getattr(self.G.L, "spmat_apply_" + _sfx(dtype))(self.A, self.G.stream(), _real(dtype)(alpha), int(append), _vp(x), _vp(y))


def plan_flags(dictionary=True):
    from vexcl_amd import _capi
    return _capi.SPMAT_NO_GRID_BUILD | _capi.SPMAT_NO_MARCH | _capi.SPMAT_NO_PLANE | (0 if dictionary else _capi.SPMAT_NO_DICTIONARY)


def call_grid_plan(G, B, x_last, with_blocks=True, **over):
    from vexcl_amd import _capi
    i = B.info
    g = _capi.Grid()
    blocks = i.slice_blocks if with_blocks else None
    codes = (i.code_pool or i.sell) if blocks else i.sell
    a = dict(ndeltas=i.ndeltas, ell_width=i.ell_width, rows=i.rows, tail_nnz=i.tail_nnz, value_bytes=B.value_bytes, x_last=x_last)
    a.update(over)
    G.L.sell8_grid_plan(0, G.stream(), i.deltas, a["ndeltas"], codes, blocks, a["ell_width"], a["rows"], a["tail_nnz"], a["value_bytes"], a["x_last"], ctypes.byref(g))
    return g


def call_plane_plan(G, B, x_last, **over):
    from vexcl_amd import _capi
    i = B.info
    p = _capi.Plane()
    a = dict(ndeltas=i.ndeltas, blocks=i.slice_blocks, nslices=i.rows // PL, dictionary_blocks=i.dictionary_blocks, ell_width=i.ell_width, rows=i.rows,
             tail_nnz=i.tail_nnz, value_bytes=B.value_bytes, x_last=x_last)
    a.update(over)
    G.L.sell8_plane_plan(0, G.stream(), i.deltas, a["ndeltas"], a["blocks"], a["nslices"], i.code_pool or i.sell, a["dictionary_blocks"], a["ell_width"],
                         a["rows"], a["tail_nnz"], a["value_bytes"], a["x_last"], ctypes.byref(p))
    return p


def plan_matrices():
    """(name, matrix, a dictionary is expected, the plane plan applies).  The library keeps a slice dictionary from 64 slices on where at
    most a quarter of them are distinct: 128-point lines in planes of four make every slice a plane."""
    return [("natural 20x5x6", grid_matrix("natural", 20, 5, 6), False, False), ("bands 130x5x9+1", grid_matrix("bands", 130, 5, 9, 1), False, False),
            ("bands 514x3x4", grid_matrix("bands", 514, 3, 4), False, False), ("ids 9x8x16", grid_matrix("ids", 9, 8, 16), False, False),
            ("natural 128x4x64", grid_matrix("natural", 128, 4, 64), True, False), ("striped 128x4x66", grid_matrix("striped", 128, 4, 66), True, False),
            ("natural 512x4x16", grid_matrix("natural", PL, 4, 16), True, True), ("bench 512x6x11", grid_matrix("bench", PL, 6, 11), True, True),
            ("bands5 512x4x16", grid_matrix("bands5", PL, 4, 16), True, True)]


def check_grid_plan(G, oracle, B, mat, dtype, model, with_blocks, what):
    """The plan of the library against the model, its tables read back whole, the product on it, the release."""
    from vexcl_amd import _capi
    i = B.info
    g = call_grid_plan(G, B, mat.x_last, with_blocks)
    assert g.usable == 1 and g.reserved == 0, what
    for k in ("nx", "lines_per_plane", "planes", "hot_class", "classes", "x_last", "flat"):
        assert getattr(g, k) == model[k], what + (k, getattr(g, k), model[k])
    geo = _capi.Grid()
    G.L.sell8_grid_geometry(G.cus, g.nx, g.lines_per_plane, g.planes, ctypes.byref(geo))
    for k in ("depth", "segments", "segment_rows", "threads", "pitch", "store_policy"):
        assert getattr(g, k) == getattr(geo, k), what + (k,)
    table = np.full((g.classes, 7, g.pitch), ABSENT, dtype=np.uint8)
    table[:, :, :g.nx] = model["table"]
    assert B.read(g.line_class, mat.lines, np.int32).tobytes() == model["line_class"].tobytes(), what + ("line_class",)
    assert B.read(g.table, table.size, np.uint8).tobytes() == table.tobytes(), what + ("table",)
    host_checks(launches_to_check(lambda d: grid_launch_of(g, mat, dtype, d), mat, dtype, None), what)
    fn = getattr(G.L, "spmv_sell8v_grid_" + _sfx(dtype))
    check_all(oracle, Vectors(G, Case.of(oracle, mat, dtype)),
              lambda x, y, alpha, append: fn(0, G.stream(), mat.n, _real(dtype)(alpha), int(append), i.values, _vp(x), _vp(y), ctypes.byref(g)), what)
    G.L.sell8_grid_release(0, ctypes.byref(g))
    assert bytes(g) == bytes(ctypes.sizeof(g)), what + ("release left something",)
    G.L.sell8_grid_release(0, ctypes.byref(g))


@gpu
@every_dtype
@pytest.mark.parametrize("which", range(9))
def test_plans_called_directly(G, oracle, dtype, which):
    """Every field the host models define; line_class and table read back whole, pitch padding included; the product on the returned
    plan; release zeroes the struct and may be repeated."""
    from vexcl_amd import _capi
    assert len(plan_matrices()) == 9
    name, mat, has_dictionary, want_plane = plan_matrices()[which]
    ptr, col, val = mat.csr(dtype)
    assert int(col.max()) == mat.x_last
    with environment(G.L, VEXHIP_PLANE_FORCE=1):
        for dictionary in (True, False):
            B = Built(G, ptr, col, val, plan_flags(dictionary))
            try:
                i = B.info
                what = (name, np.dtype(dtype).name, "dictionary %r" % dictionary)
                assert _capi.SPMAT_NAMES[i.format] == "sell8v" and not i.grid.usable and not i.plane.usable and not i.march.usable, what + (i.reason,)
                assert bool(i.slice_blocks) == (dictionary and has_dictionary) and i.tail_nnz == 0, what
                model = grid_plan_host(G.L, ptr, col, val, mat.x_last, int(i.ell_width), int(i.tail_nnz))
                assert model is not None, what
                check_grid_plan(G, oracle, B, mat, dtype, model, bool(i.slice_blocks), what)
                if not i.slice_blocks or mat.nx != PL:
                    continue
                blocks = B.read(i.slice_blocks, mat.n // PL, np.int32)
                # the library's own code blocks through the unpacker: the block of every slice holds the class table of its line
                w = int(i.ell_width)
                pool = B.read(i.code_pool or i.sell, int(i.dictionary_blocks) * (w + 1) // 2 * 2048, np.uint8).reshape(int(i.dictionary_blocks), -1)
                pos_of = [offsets(PL, mat.ny).tolist().index(int(d)) for d in B.read(i.deltas, int(i.ndeltas), np.int32)]
                assert np.array_equal(unpack_blocks(pool, w, pos_of)[blocks], model["table"][model["line_class"]]), what + ("code blocks",)
                assert np.array_equal(blocks, first_appearance(blocks[:, None])[0]), what + ("the dictionary does not number by first appearance",)
                pm = plane_plan_host(ptr, col, val, mat.x_last, int(i.ell_width), int(i.tail_nnz), blocks, int(i.dictionary_blocks))
                assert (pm is not None) == want_plane, what
                p = call_plane_plan(G, B, mat.x_last)
                assert p.usable == 1 and p.reserved == 0, what
                for k in pm:
                    assert getattr(p, k) == pm[k], what + (k, getattr(p, k), pm[k])
                geo = _capi.Plane()
                G.L.sell8_plane_geometry(G.cus, p.lines_per_plane, p.planes, ctypes.byref(geo))
                for k in ("depth", "tile", "store_policy"):
                    assert getattr(p, k) == getattr(geo, k), what + (k,)
                assert host_plane_check(p, mat.n, int(i.ell_width), dtype == np.float64), what
                host_checks([plane_launch_of(p, mat, dtype, int(G.L.sell8_plane_f32_depth(G.cus, p.lines_per_plane, p.planes)))], what)
                fn = getattr(G.L, "spmv_sell8v_plane_%s_i32" % _sfx(dtype))
                check_all(oracle, Vectors(G, Case.of(oracle, mat, dtype)),
                          lambda x, y, alpha, append: fn(0, G.stream(), mat.n, _real(dtype)(alpha), int(append), i.ell_width, i.code_pool or i.sell,
                                                         i.slice_blocks, i.deltas, i.values, _vp(x), _vp(y), ctypes.byref(p)), what + ("plane",))
            finally:
                B.close()


def band_csr(n, diagonals, mcut=None, values=None, dtype=np.float64):
    """Every diagonal in every row whose column lies in [0, mcut), in the order given; one value per diagonal."""
    i = np.arange(n, dtype=np.int64)[:, None]
    cols = i + np.asarray(diagonals, dtype=np.int64)[None, :]
    ok = (cols >= 0) & (cols < (mcut or n))
    vals = np.broadcast_to(np.asarray(values if values is not None else [(k + 2) / 8.0 for k in range(len(diagonals))], dtype=dtype)[None, :], cols.shape)
    return np.concatenate([[0], np.cumsum(ok.sum(axis=1))]).astype(np.int32), cols[ok].astype(np.int32), np.ascontiguousarray(vals[ok])


def declined(plan):
    """usable = 0, and then the whole struct is zero."""
    return not plan.usable and bytes(plan) == bytes(ctypes.sizeof(plan))


def product_is_the_csr_loop(G, oracle, B, csr):
    x = oracle.random_f64(3, int(csr[1].max()) + 1)
    y = G.up(np.zeros(len(csr[0]) - 1))
    B.apply(G.up(x), y, 1.0, False)
    assert np.array_equal(y.cpu().numpy(), oracle.spmv_csr(*csr, x))


@gpu
def test_grid_plan_declines(G, oracle):
    """One structural reason each, under VEXHIP_PLANE_FORCE: the plan is accepted as the matrix stands and declined for that reason alone."""
    P, nx = 20 * 5, 20
    seven = (-P, -nx, -1, 0, 1, nx, P)
    n = P * 6
    with contextlib.ExitStack() as stack, environment(G.L, VEXHIP_PLANE_FORCE=1):
        def built(csr):
            B = Built(G, *csr, plan_flags())
            stack.callback(B.close)
            return B
        B = built(band_csr(n, seven))
        g = call_grid_plan(G, B, n - 1)
        assert g.usable == 1 and B.info.tail_nnz == 0
        G.L.sell8_grid_release(0, ctypes.byref(g))
        for reason, a in (("value_bytes = 2", dict(x_last=n - 1, value_bytes=2)), ("a CSR tail", dict(x_last=n - 1, tail_nnz=1)),
                          ("x shorter than the rows", dict(x_last=n - 2)), ("ndeltas < 4", dict(x_last=n - 1, ndeltas=3))):
            assert declined(call_grid_plan(G, B, **a)), reason
        for reason, csr in (("an eighth diagonal", band_csr(n, (-P, -nx, -2, -1, 0, 1, nx, P))),
                            ("a far diagonal that is no multiple of nx", band_csr(n, (-P - 7, -nx, -1, 0, 1, nx, P + 7))),
                            ("fewer than four diagonals", band_csr(n, (-1, 0, 1))),
                            ("rows that do not fill whole lines", band_csr(n + 7, seven)),
                            ("a row whose entries descend by position", band_csr(n, seven[::-1]))):
            B = built(csr)
            assert B.info.tail_nnz == 0, reason
            assert declined(call_grid_plan(G, B, int(csr[1].max()))), reason
            assert grid_plan_host(G.L, *csr, int(csr[1].max()), int(B.info.ell_width), 0) is None, reason
            product_is_the_csr_loop(G, oracle, B, csr)
        for lines, usable in ((128, True), (129, False)):                         # classes: 128 accepted, 129 declined
            mat = grid_matrix("ids", 9, 8, 16, lines - 128)
            B = built(mat.csr(np.float64))
            g = call_grid_plan(G, B, mat.x_last)
            assert len(mat.classes) == lines and bool(g.usable) == usable, (lines, g.usable, g.classes)
            assert g.classes == 128 if usable else declined(g), (lines, g.classes)
            G.L.sell8_grid_release(0, ctypes.byref(g))


@gpu
def test_plane_plan_declines(G, oracle):
    """One structural reason each under VEXHIP_PLANE_FORCE; then the three size rules without it, each on a matrix that the plan takes
    with it."""
    n5 = PL * 4 * 16
    seven512 = (-4 * PL, -PL, -1, 0, 1, PL, 4 * PL)
    with contextlib.ExitStack() as stack:
        def built(csr):
            B = Built(G, *csr, plan_flags())
            stack.callback(B.close)
            return B
        with environment(G.L, VEXHIP_PLANE_FORCE=1):
            B64 = built(band_csr(n5, seven512))
            assert B64.info.slice_blocks and B64.info.tail_nnz == 0
            assert call_plane_plan(G, B64, n5 - 1).usable == 1
            bad_blocks = G.up(np.full(n5 // PL, int(B64.info.dictionary_blocks), dtype=np.int32))
            for reason, a in (("value_bytes = 2", dict(x_last=n5 - 1, value_bytes=2)), ("a CSR tail", dict(x_last=n5 - 1, tail_nnz=1)),
                              ("x_last + 1 no multiple of 512", dict(x_last=n5 - 1 + 100)), ("ndeltas < 2", dict(x_last=n5 - 1, ndeltas=1)),
                              ("rows that do not fill whole lines", dict(x_last=n5 - 1, rows=n5 - 1)),
                              ("129 blocks", dict(x_last=n5 - 1, dictionary_blocks=129)),
                              ("a block number out of range", dict(x_last=n5 - 1, blocks=bad_blocks.data_ptr()))):
                assert declined(call_plane_plan(G, B64, **a)), reason
            for reason, csr in (("an eighth diagonal", band_csr(n5, (-4 * PL, -PL, -2, -1, 0, 1, PL, 4 * PL))),
                                ("a far diagonal that is no multiple of 1024", band_csr(n5, (-3 * PL, -PL, -1, 0, 1, PL, 3 * PL))),
                                ("a row whose entries descend by position", band_csr(n5, seven512[::-1]))):
                B = built(csr)
                assert B.info.tail_nnz == 0 and B.info.slice_blocks, reason
                assert declined(call_plane_plan(G, B, n5 - 1)), reason
                product_is_the_csr_loop(G, oracle, B, csr)
            # (the centre and +P with x long enough for every row to hold both: all slices are one block, nothing but the size decides)
            Bs = built(band_csr(n5, (0, 4 * PL), n5 + 4 * PL))
            B3 = built(band_csr(PL * 32 * 3, (0, 32 * PL), PL * 32 * 4))
            pairs = grid_matrix("pairs", PL, 4, 16)                                # half of the slices off the hot block
            Bp = built(pairs.csr(np.float64))
            assert Bs.info.slice_blocks and B3.info.slice_blocks and Bp.info.slice_blocks and Bs.info.dictionary_blocks == 1
            size_cases = (("fewer than 64 slices", Bs, dict(x_last=67 * PL - 1, nslices=63, rows=63 * PL)),
                          ("fewer than 4 planes", B3, dict(x_last=128 * PL - 1)),
                          ("more than 1/16 of the slices off the hot block", Bp, dict(x_last=pairs.x_last)))
            for reason, B, a in size_cases:
                assert call_plane_plan(G, B, **a).usable == 1, reason
        with environment(G.L):
            assert call_plane_plan(G, Bs, n5 + 4 * PL - 1).usable == 1
            for reason, B, a in size_cases:
                assert declined(call_plane_plan(G, B, **a)), reason


def device_band(G, n, diagonals, values, nx=None, centre=None):
    """`band_csr` made on the device (fp64, columns below n); centre: the two values of the centre entry in the lines (of nx rows) of
    even and of odd number."""
    t = G.torch
    i = t.arange(n, device=G.dev, dtype=t.int64)[:, None]
    cols = i + t.tensor(diagonals, device=G.dev, dtype=t.int64)[None, :]
    ok = (cols >= 0) & (cols < n)
    vals = t.tensor(values, device=G.dev, dtype=t.float64)[None, :].expand(n, -1).clone()
    if centre is not None:
        vals[:, list(diagonals).index(0)] = t.tensor(centre, device=G.dev, dtype=t.float64)[(i[:, 0] // nx) % 2]
    ptr = t.zeros(n + 1, device=G.dev, dtype=t.int32)
    ptr[1:] = t.cumsum(ok.sum(dim=1), 0).to(t.int32)
    return ptr, cols[ok].to(t.int32), vals[ok]


@gpu
def test_grid_plan_size_rules_at_two_to_the_23_rows(G):
    """Without VEXHIP_PLANE_FORCE the grid plan looks at no matrix below 2^23 rows, so that is the smallest size at which its other
    two size rules show: fewer than 4 planes, and more than 1/4 of the lines off the hot class.  Each matrix is made on the device, is
    taken under FORCE, and is declined without it; a matrix of 2^23 rows without either fault is taken, and declined one plane short."""
    nx, ny, nz = PL, 4, 4096
    n = nx * ny * nz
    assert n == 2 ** 23
    seven = (-nx * ny, -nx, -1, 0, 1, nx, nx * ny)
    values = [(k + 2) / 8.0 for k in range(7)]
    with contextlib.ExitStack() as stack:
        def built(*csr):
            B = Built(G, *csr, plan_flags())
            stack.callback(B.close)
            assert B.info.tail_nnz == 0 and B.info.ell_width == 7 and B.info.rows == csr[0].numel() - 1
            return B
        plain = built(*device_band(G, n, seven, values))
        pairs = built(*device_band(G, n, seven, values, nx, (1.5, 2.5)))
        nx3, ny3 = 1024, 2731
        n3 = nx3 * ny3 * 3
        assert n3 >= 2 ** 23 and n3 - nx3 * 3 < 2 ** 23                    # (the smallest three-plane grid of 1024-point lines above the threshold)
        three = built(*device_band(G, n3, (-nx3 * ny3, -nx3, -1, 0, 1, nx3, nx3 * ny3), values))
        small = grid_plan_host(G.L, *band_csr(8 * 4 * 6, (-32, -8, -1, 0, 1, 8, 32)), 8 * 4 * 6 - 1, 7, 0)      # the same classes on a grid of 8 x 4 x 6
        for force in (True, False):
            with environment(G.L, VEXHIP_PLANE_FORCE=1 if force else None):
                g = call_grid_plan(G, plain, n - 1)
                assert g.usable == 1 and (g.nx, g.lines_per_plane, g.planes, g.classes, g.flat) == (nx, ny, nz, small["classes"], 0), (force, g.usable, g.classes)
                assert 4 * (ny * nz - 8) >= 3 * ny * nz                      # (eight lines of the first and the last plane are off the hot class)
                G.L.sell8_grid_release(0, ctypes.byref(g))
                g = call_grid_plan(G, plain, n - 1, rows=n - nx * ny)
                assert bool(g.usable) == force, "one plane short of 2^23 rows"
                G.L.sell8_grid_release(0, ctypes.byref(g))
                g = call_grid_plan(G, pairs, n - 1)
                assert bool(g.usable) == force and (declined(g) or g.classes > small["classes"]), "half of the lines off the hot class"
                G.L.sell8_grid_release(0, ctypes.byref(g))
                g = call_grid_plan(G, three, n3 - 1)
                assert bool(g.usable) == force and (declined(g) or g.planes == 3), "fewer than 4 planes"
                G.L.sell8_grid_release(0, ctypes.byref(g))


@gpu
@every_dtype
@pytest.mark.parametrize("p64", (False, True), ids=("ptr32", "ptr64"))
def test_one_pass_build_limits(G, oracle, dtype, p64):
    """grid_build through vexhip_spmat_create_*: 254 distinct values and 128 classes are stored by grid line, 255 and 129 are given up (the
    SELL-512 set-up takes over); the product equals the CSR loop either way."""
    from vexcl_amd import _capi
    base = grid_matrix("bands", 256, 4, 5)
    ptr, col, val = base.csr(dtype)
    centre = col == np.repeat(np.arange(base.n), np.diff(ptr))

    def many_values(k):                                              # k distinct values: six of the band and k - 6 on the diagonal, by row of the line
        v = val.copy()
        v[centre] = (3.0 + (np.arange(base.n) % 256 % (k - 6)) / 512.0).astype(dtype)
        assert len(np.unique(v.view(BITS[dtype]))) == k
        return ptr, col, v

    def many_classes(lines):
        mat = grid_matrix("ids", 9, 8, 16, lines - 128)
        assert len(mat.classes) == lines
        return mat.csr(dtype)

    with environment(G.L, VEXHIP_PLANE_FORCE=1):
        for csr, direct in ((many_values(254), True), (many_values(255), False), (many_classes(128), True), (many_classes(129), False)):
            B = Built(G, *csr, flags=0, fmt=_capi.SPMAT_AUTO, p64=p64)
            try:
                i = B.info
                assert bool(i.grid.usable and not i.sell and not i.code_pool) == direct, (direct, i.reason)
                m = int(csr[1].max()) + 1
                x, y0 = (oracle.random_f64(5, m) - 0.5).astype(dtype), (oracle.random_f64(6, len(csr[0]) - 1) - 0.5).astype(dtype)
                for alpha, append in MODES:
                    y = G.up(y0.copy())
                    B.apply(G.up(x), y, alpha, append)
                    want = oracle.spmv_csr(*csr, x, y=y0.copy() if append else None, alpha=alpha, append=append)
                    assert np.array_equal(y.cpu().numpy(), want), (direct, alpha)
            finally:
                B.close()


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_host_models_generators_and_geometries(oracle, built_lib):
    """Everything the GPU tests take for granted: generator -> CSR -> tables -> CSR; the packer against its unpacker; the plan models
    on examples computed by hand; `vexhip_sell8_grid_check`, the host checks, `visit_once` and `addresses_inside` on every listed
    case for several device sizes; every family holds what it is named for; the oracle lies within the derived bound."""
    from vexcl_amd import _capi
    L = built_lib
    assert ctypes.sizeof(_capi.Plane) == 48 and ctypes.sizeof(_capi.Grid) == 80
    assert len(set(GRID_IDS)) == len(GRID_IDS) and len(set(PLANE_IDS)) == len(PLANE_IDS)
    for dtype in DTYPES:
        pool = value_pool(dtype)
        assert len(np.unique(pool.view(BITS[dtype]))) == len(pool) == 27 and pool[ZERO] == 0 and np.signbit(pool[MINUS_ZERO]) and not np.signbit(pool[ZERO])
        assert 0 < pool[SUBN] < np.finfo(dtype).tiny

    # ---- generator -> CSR -> tables -> CSR, in columns, values and order
    seen = {}
    for mat in [grid_case_matrix(c) for c in GRID_CASES] + [plane_case_matrix(c) for c in PLANE_CASES] + [m[1] for m in plan_matrices()]:
        if mat.name in seen:
            continue
        seen[mat.name] = mat
        for dtype in DTYPES:
            ptr, col, val = mat.csr(dtype)
            assert ptr[-1] == len(col) == len(val) and (len(col) == 0 or (col.min() >= 0 and col.max() <= mat.x_last)), mat.name
            rows = np.repeat(np.arange(mat.n), np.diff(ptr))
            d = col - rows
            same = rows[1:] == rows[:-1]
            assert np.all(d[1:][same] > d[:-1][same]), (mat.name, "a row's entries do not ascend")
            for hot in ("most", "unused"):
                lc, table = mat.tables(528 if mat.nx <= 512 else 1040, mat.hot(hot))
                assert table.shape[0] == max(len(mat.classes), mat.hot(hot) + 1) and (table[:, :, mat.nx:] == ABSENT).all()
                back = decode_tables(lc, table, mat.nx, mat.ny, table256(value_pool(dtype), 0.0, dtype))
                assert all(np.array_equal(a, b) for a, b in zip(back, (ptr, col, val))) and back[2].tobytes() == val.tobytes(), mat.name
        assert np.array_equal(np.unique(mat.line_class, return_index=True)[1], np.sort(np.unique(mat.line_class, return_index=True)[1])), mat.name
        firsts = [int(np.flatnonzero(mat.line_class == c)[0]) for c in range(len(mat.classes))]
        assert firsts == sorted(firsts) and mat.uses.min() >= 1, (mat.name, "classes are not numbered by first appearance")

    # ---- the families hold what they are named for
    assert len(grid_matrix("bench", 9, 4, 9).classes) == 2 and len(grid_matrix("diag", 9, 4, 9).classes) == 1
    assert len(grid_matrix("natural9", 9, 3, 9).classes) == 9 and len(grid_matrix("natural", 9, 5, 9).classes) >= 9
    assert len(grid_matrix("many128", 9, 8, 17).classes) == 128 and len(grid_matrix("many129", 9, 8, 17).classes) == 129
    for mat in (grid_case_matrix(case_named(GRID_CASES, "holes")), grid_case_matrix(case_named(GRID_CASES, "holes-long")),
                plane_case_matrix(case_named(PLANE_CASES, "holes"))):
        for dtype in DTYPES:
            C = Case.of(oracle, mat, dtype)
            lens = np.diff(C.csr[0])
            assert set(range(8)) == set(np.unique(lens).tolist()) and C.empty_rows > 0 and C.unreferenced > 0, (mat.name, np.unique(lens))
            rows = np.repeat(np.arange(mat.n), lens)
            far_only = np.zeros(mat.n, dtype=bool)
            far_only[rows] = True
            far_only[rows[np.abs(C.csr[1] - rows) != mat.nx * mat.ny]] = False
            assert far_only.any(), (mat.name, "no row with +-P only")
    for mat in seen.values():
        for dtype in DTYPES:
            C = Case.of(oracle, mat, dtype)
            ptr, col, val = C.csr
            sub = (np.abs(val) < np.finfo(dtype).tiny) & (val != 0)
            xs, free = C.x[col[sub]], C.x[np.setdiff1d(np.arange(len(C.x)), col)]
            assert np.all((np.abs(xs) == 0.25) | ~np.isfinite(xs)) and not np.isfinite(free).any() and (len(free) < 3 or np.isnan(free).any()), mat.name
            for mode in MODES:
                want = C.reference(oracle, mode)
                assert np.array_equal(np.flatnonzero(~np.isfinite(want)), C.bad_rows), (mat.name, "the host predicts other rows not to be finite than the CSR loop gives")
                assert C.within_bound(want, mode), (mat.name, mode, "the oracle is outside the derived bound")
            if mat.name.startswith(("natural_", "holes", "limited")):
                assert len(C.bad_rows) > 0 and np.isnan(C.reference(oracle, MODES[0])).any(), (mat.name, "no stored zero meets an Inf: the canary is vacuous")

    # ---- the code-block packer against its unpacker and the layout of the header
    for w in range(1, 9):
        mat = limited_matrix(w, 4, 24, w % 2, (w % 3) * PL)
        assert np.diff(mat.csr(np.float64)[0]).max() == min(w, 7), (w, "no row fills the width")
        _, table = mat.tables(PL, mat.hot("unused"))
        pool = pack_blocks(table[:, :, :PL], w)
        assert pool.shape == (len(mat.classes) + 1, (w + 1) // 2 * 2048)
        assert np.array_equal(unpack_blocks(pool, w), table[:, :, :PL]), (w, "the unpacked blocks are not the class tables")
        codes = pool[:, :(w + 1) // 2 * 1024]
        assert (codes == 254).any() and (codes == 255).any()
        if w % 2:
            assert (pool.reshape(len(pool), 2, -1, 256, 2, 2)[:, 0, -1, :, 1, :] == 3).all() and (pool.reshape(len(pool), 2, -1, 256, 2, 2)[:, 1, -1, :, 1, :] == 6).all()
    # blocks the library's fill would produce -- the two rows of every lane hold the same diagonals, or the second one more -- against
    # `oracle.sell_pair_slots`: a line of full bands (widths 7 and 8), a line with the centre in every row and +P in the odd ones (2, 3)
    want = np.full((4 * 6, 7, PL), ABSENT, dtype=np.uint8)
    want[:, 3, :] = 9
    want[:, 6, 1::2] = 4
    for mat, widths, lines in ((grid_matrix("bands", PL, 4, 6), (7, 8), (9, 14)), (GridMat("centre and +P", PL, 4, 6, 0, want), (2, 3), (0, 9, 23))):
        for line in lines:
            cls = mat.classes[mat.line_class[line]][None]
            for w in widths:
                mine = pack_blocks(cls, w, fill_like=True)[0]
                assert mine.tobytes() == oracle_block(oracle, mat, line, w).tobytes(), (mat.name, line, w, "the packed block is not what oracle.sell_pair_slots places")
                assert np.array_equal(unpack_blocks(mine[None], w), cls)
    one = np.full((1, 7, PL), ABSENT, dtype=np.uint8)
    one[0, 3, :] = 9
    one[0, 6, 5] = 4                                                 # row 5: the centre (position 3, value code 9) and +P (position 6, value code 4)
    pool = pack_blocks(one, 2)
    word = pool[0].view(np.uint32)[5 >> 1]
    assert [(word >> s) & 255 for s in (8, 24)] == [3, 6] and [(pool[0].view(np.uint32)[256 + 2] >> s) & 255 for s in (8, 24)] == [9, 4]

    # ---- the plan models on examples computed by hand
    # 8 x 2 x 2 grid, centre 1.5 everywhere, +1 inside the lines (0.25), +-8 and +-16 where they exist: lines 0..3 differ -> 4 classes
    ptr, col, val = band_csr(32, (-16, -8, -1, 0, 1, 8, 16), values=[0.5, 0.25, 2.0, 1.5, 2.0, 0.25, 0.5])
    model = grid_plan_host(L, ptr, col, val, 31, 7, 0)
    assert model is not None and (model["nx"], model["lines_per_plane"], model["planes"], model["classes"], model["hot_class"], model["flat"]) == (8, 2, 2, 4, 0, 0)
    assert model["line_class"].tolist() == [0, 1, 2, 3] and model["table"].shape == (4, 7, 8)
    # value codes by bit pattern: 0.25 < 0.5 < 1.5 < 2.0 -> 0, 1, 2, 3; row 0 of line 0 has no -16, -8, -1
    assert model["table"][0, :, 0].tolist() == [255, 255, 255, 2, 3, 0, 1] and model["table"][3, :, 7].tolist() == [1, 0, 3, 2, 255, 255, 255]
    ptr, col, val = band_csr(8 * 2 * 6, (-16, -8, -1, 0, 1, 8, 16))
    model = grid_plan_host(L, ptr, col, val, 95, 7, 0)
    assert model["classes"] == 5 and model["line_class"].tolist() == [0, 1, 2, 2, 2, 2, 2, 2, 2, 2, 3, 4] and model["hot_class"] == 2
    assert grid_plan_host(L, ptr, col, val, 95, 7, 0, force=False) is None and grid_plan_host(L, ptr, col, val, 95, 7, 3) is None
    # the two size rules behind the row threshold, which is lowered to reach them: 4 of 12 lines off the hot class are more than a
    # quarter, 4 of 16 are not; three planes are too few
    assert grid_plan_host(L, ptr, col, val, 95, 7, 0, force=False, threshold=0) is None
    csr16 = band_csr(8 * 2 * 8, (-16, -8, -1, 0, 1, 8, 16))
    assert grid_plan_host(L, *csr16, 127, 7, 0, force=False, threshold=0)["hot_class"] == 2
    # (the centre, +1, +8 and +64 with x long enough for every row to hold all four: one class, nothing but the planes decides)
    csr3, csr4 = band_csr(8 * 8 * 3, (0, 1, 8, 64), 8 * 8 * 4), band_csr(8 * 8 * 4, (0, 1, 8, 64), 8 * 8 * 5)
    assert grid_plan_host(L, *csr3, 255, 4, 0, force=False, threshold=0) is None and grid_plan_host(L, *csr3, 255, 4, 0)["planes"] == 3
    four = grid_plan_host(L, *csr4, 319, 4, 0, force=False, threshold=0)
    assert (four["planes"], four["classes"]) == (4, 1)
    assert grid_plan_host(L, ptr, col, val, 94, 7, 0) is None and grid_plan_host(L, ptr, col, val, 95, 9, 0) is None
    assert grid_plan_host(L, *band_csr(96, (-16, -8, -2, -1, 0, 1, 8, 16)), 95, 8, 0) is None
    assert grid_plan_host(L, *band_csr(96, (-17, -8, -1, 0, 1, 8, 17)), 95, 7, 0) is None
    assert grid_plan_host(L, *band_csr(96, (16, 8, 1, 0, -1, -8, -16)), 95, 7, 0) is None
    assert grid_plan_host(L, *band_csr(96, (-1, 0, 1)), 95, 3, 0) is None and grid_plan_host(L, *band_csr(100, (-16, -8, -1, 0, 1, 8, 16)), 99, 7, 0) is None
    flat = grid_plan_host(L, *band_csr(2048 * 3, (-2048, -1, 0, 1, 2048)), 2048 * 3 - 1, 5, 0)
    assert flat is not None and (flat["nx"], flat["lines_per_plane"], flat["flat"]) == (512, 4, 1)
    n = PL * 4 * 5
    csr = band_csr(n, (-4 * PL, -PL, -1, 0, 1, PL, 4 * PL))
    blocks = np.array([0, 1, 1, 1] + [2] * 12 + [3, 3, 3, 4], dtype=np.int32)
    pm = plane_plan_host(*csr, n - 1, 7, 0, blocks, 5)
    assert pm == {"lines_per_plane": 4, "planes": 5, "hot_block": 2, "x_last": n - 1, "flat": 0, "table_pitch": 0}
    assert plane_plan_host(*csr, n - 1, 7, 0, blocks, 5, force=False) is None and plane_plan_host(*csr, n + 99, 7, 0, blocks, 5) is None
    assert plane_plan_host(*csr, n - 1, 7, 1, blocks, 5) is None and plane_plan_host(*csr, n - 1, 7, 0, blocks, 4) is None
    assert plane_plan_host(*band_csr(n, (-3 * PL, -PL, -1, 0, 1, PL, 3 * PL)), n - 1, 7, 0, blocks, 5) is None
    assert plane_plan_host(*band_csr(n, (0,)), n - 1, 1, 0, blocks, 5) is None
    tie = plane_plan_host(*csr, n - 1, 7, 0, np.array([1, 1, 0, 0] * 5, dtype=np.int32), 2)
    assert tie["hot_block"] == 0                                     # the first most frequent

    # ---- every listed geometry: the library's check, the host's, visit_once and the addresses, for several device sizes
    features = {"fast": 0, "run64": 0, "others": 0, "cpx": 0, "idle": 0, "slow": 0, "maxt512": 0, "tile4": 0, "flatwalk": 0}
    for cus in (256, 304, 64, 1):
        for case in GRID_CASES:
            mat = grid_case_matrix(case)
            g = fill_grid(L, cus, mat, case)
            g.line_class = g.table = 1                               # (not looked at by the check)
            L.sell8_grid_check(ctypes.byref(g), mat.n)
            assert host_grid_check(g, mat.n), case[0]
            for dtype in DTYPES:
                d32 = case[9].get("depth")
                launches = launches_to_check(lambda d: grid_launch_of(g, mat, dtype, d), mat, dtype, d32) + ([] if dtype == np.float64 else
                                                                                                              launches_to_check(lambda d: grid_launch_of(g, mat, dtype, d), mat, dtype, None))
                host_checks(launches, (case[0], cus, np.dtype(dtype).name))
                if cus == 256:
                    la = launches[0]
                    f = walk_features(la, mat.line_class, g.hot_class, False)
                    for k in ("fast", "run64", "slow"):
                        features[k] += f[k]
                    features["others"] = max(features["others"], f["others"])
                    features["cpx"] = max(features["cpx"], la.cpx)
                    features["idle"] += sum(la.owner(b) is None for b in range(la.workgroups))
                    features["maxt512"] += la.threads > 256
                    fa = walk_features(la, mat.line_class, g.hot_class, True)
                    assert (f["fast"] > 0 and fa["fast"] > 0) != (case[0] in GRID_SLOW_ONLY), (case[0], np.dtype(dtype).name, f, fa, "fast steps")
                    if case[0] == "nz70-d70":
                        assert f["run64"] > 0, "no look finds 64 planes"
                    if case[0] == "alternate":
                        assert f["mixed"] > 0 and fa["mixed"] > 0, "no fast group in which a line changes class"
                    if case[0] == "flat1":
                        assert la.cpx == 3 and la.chunks == 18
                    if case[0] == "striped":
                        assert f["others"] >= 3 and f["fast"] == 0
                    if case[0] == "ny17":
                        assert la.tpx == 2
        for case in PLANE_CASES:
            mat = plane_case_matrix(case)
            p = fill_plane(L, cus, mat, case)
            for dtype in DTYPES:
                f64 = dtype == np.float64
                assert host_plane_check(p, mat.n, case[8] or 7, f64), case[0]
                d32 = case[9].get("depth")
                la = plane_launch_of(p, mat, dtype, d32)
                host_checks([la], (case[0], cus, np.dtype(dtype).name))
                if not f64:
                    host_checks([plane_launch_of(p, mat, dtype, d) for d in range(1, mat.nz + 1)], (case[0], cus, "every fp32 depth"))
                if cus == 256:
                    f = walk_features(la, mat.line_class, p.hot_block, True)
                    assert (f["fast"] > 0) != (case[0] in PLANE_SLOW_ONLY), (case[0], np.dtype(dtype).name, f, "fast steps")
                    features["tile4"] += la.tile == 4
                    features["flatwalk"] += la.flat_walk
                    if case[0] in ("nz70-d70", "blocks-nz70"):
                        assert f["run64"] > 0
                    if case[0] in ("striped", "blocks-striped"):
                        assert f["others"] >= 3
                    if case[0] in ("alternate", "blocks-alternate"):
                        assert f["mixed"] > 0, "no fast group in which a line changes class"
                    if case[0] == "ny18":
                        assert la.tpx == 2 and la.tiles == 9
    assert features["fast"] > 0 and features["run64"] > 0 and features["others"] >= 3 and features["cpx"] > 1 and features["idle"] > 0, features
    assert features["maxt512"] > 0 and features["tile4"] > 0 and features["flatwalk"] > 0 and features["slow"] > 0, features
    # a plan the host must stop: x too short for the fast steps the walk would take if zh ignored it is caught by the models themselves
    mat = grid_matrix("bands", 9, 5, 9)
    la = Launch("grid", 9, 5, 9, mat.lines, mat.x_last, 4, 2, 1, 10, 64, 2, False, False)
    assert visit_once(la) and addresses_inside(la, True) > 0
    la.zh = lambda tile, zc, append: min(zc * 4 + 4, 9)               # fast steps to the end of every walk: the last planes leave x
    assert addresses_inside(la, False) == -1
    la = Launch("grid", 9, 5, 9, mat.lines, mat.x_last, 4, 2, 2, 4, 64, 2, False, False)      # two segments of four rows do not cover nine
    assert not visit_once(la)
