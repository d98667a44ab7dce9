"""Direct parity tests of the compressed-stencil product, `vexhip_spmv_ccsr_f64/_f32` (vexcl_amd/csrc/ccsr.hip), in every
form it ships: the pair form (rows per lane 0, the default) and `ccsr_kernel<RPL = 1, 2, 4, 8>`, with the unique-row tables in
LDS and in global memory, in plain order and in the strip traversal.

vex::SpMatCCSR hands every float / double operator of 32768 rows or more to vexhip_spmat, and every CCSR case of the C++ suite is
that large: without this file the kernels below run in no test, although the class keeps them for small operators, operators
of 2^31 entries or more, columns outside [0, n), storages without diagonal codes and after an out-of-memory in the hand-over.

Reference: the operator expanded on the host (row i = table row idx[i], columns i + col[j], entries in table order) through
`oracle.spmv_csr`.  ccsr.hip is compiled with -ffp-contract=off and folds a row's entries in table order, so every comparison
is `np.array_equal` -- no tolerance anywhere in this file.  The expansion itself is pinned by a plain Python loop (CPU)."""
import contextlib
import ctypes

import numpy as np
import pytest

FORMS = (0, 1, 2, 4, 8)                                  # vexhip_spmv_ccsr_set_rows_per_lane: 0 = pair form
DTYPES = (np.float64, np.float32)
MODES = ((1.0, 0), (2.5, 0), (-0.5, 1))                  # (alpha, append)
KTABLE = 1024                                            # ccsr.hip: unique rows / entries staged in LDS at most

every_form = pytest.mark.parametrize("rpl", FORMS, ids=lambda r: "pair" if r == 0 else "rpl%d" % r)
every_dtype = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
every_mode = pytest.mark.parametrize("mode", MODES, ids=lambda m: "alpha%g_%s" % (m[0], "append" if m[1] else "set"))


# ---------------------------------------------------------------------------------------------------------------------------
# operators: (n, idx uint32[n], row uint32[m + 1], col int32[entries], val float64[entries])
# ---------------------------------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, idx, row, col, val):
        self.name, self.n = name, len(idx)
        self.idx = np.ascontiguousarray(idx, dtype=np.uint32)
        self.row = np.ascontiguousarray(row, dtype=np.uint32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        self.m, self.entries = len(self.row) - 1, len(self.col)
        assert self.row[0] == 0 and self.row[-1] == self.entries and np.all(np.diff(self.row.astype(np.int64)) >= 0)
        assert self.n == 0 or int(self.idx.max()) < self.m
        self._csr = {}

    def in_lds(self):
        return self.m <= KTABLE and self.entries <= KTABLE

    def csr(self, dtype):
        """Row i = table row idx[i] with columns i + col[j], entries in table order; every column inside [0, n) (asserted: the
        kernel relies on it)."""
        key = np.dtype(dtype).name
        if key not in self._csr:
            row = self.row.astype(np.int64)
            first = row[self.idx]
            lens = row[self.idx + 1] - first
            ptr = np.concatenate([[0], np.cumsum(lens)])
            nnz = int(ptr[-1])
            assert nnz < 2 ** 31
            rows = np.repeat(np.arange(self.n, dtype=np.int64), lens)
            pos = np.arange(nnz, dtype=np.int64) - np.repeat(ptr[:-1], lens) + np.repeat(first, lens)
            ccol = rows + self.col[pos]
            assert nnz == 0 or (ccol.min() >= 0 and ccol.max() < self.n), "operator %s leaves [0, n)" % self.name
            self._csr[key] = (ptr.astype(np.int32), ccol.astype(np.int32), np.ascontiguousarray(self.val.astype(dtype)[pos]))
        return self._csr[key]


def _table(rows_offsets, oracle, seed):
    """Unique-row tables from a list of offset lists; values uniform in (-0.5, 0.5), none a power of two."""
    row = np.concatenate([[0], np.cumsum([len(r) for r in rows_offsets])])
    col = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows_offsets]) if row[-1] else np.zeros(0, dtype=np.int64)
    val = oracle.random_f64(seed, max(1, int(row[-1])))[:int(row[-1])] - 0.5
    return row, col, val


def _offsets(oracle, seed, count, reach, with_zero):
    """`count` distinct offsets within +-reach in a shuffled (not ascending) order, with or without offset 0."""
    pool = np.array([o for o in range(-reach, reach + 1) if o != 0])
    order = np.argsort(oracle.random_f64(seed, len(pool)), kind="stable")
    pick = list(pool[order[:count - (1 if with_zero else 0)]])
    if with_zero:
        pick.insert(len(pick) // 2, 0)
    assert len(pick) == count and len(set(pick)) == count
    return pick


def _iid_and_runs(oracle, seed, n, choices):
    """Positions drawn from `choices`: independent draws in the first half (neighbouring rows mostly differ: p0 != p1), runs of
    1 to 300 equal draws in the second half (whole waves with p0 == p1)."""
    choices = np.asarray(choices)
    u = oracle.random_f64(seed, max(1, n))
    out = choices[np.minimum((u * len(choices)).astype(np.int64), len(choices) - 1)][:n]
    half = n // 2
    if n - half > 1:
        lens = 1 + (oracle.random_f64(seed + 1, n - half) * 300).astype(np.int64)
        starts = np.repeat(np.arange(n - half), lens)[:n - half]
        out[half:] = out[half:][starts]
    return out


def _fitting_idx(oracle, seed, n, rows_offsets):
    """For every row i one of the unique rows whose offsets all stay inside [0, n), uniformly among those (the empty row and
    the identity row always fit)."""
    lo = np.array([min(r) if len(r) else 0 for r in rows_offsets])
    hi = np.array([max(r) if len(r) else 0 for r in rows_offsets])
    i = np.arange(n)[:, None]
    fits = (i + lo[None, :] >= 0) & (i + hi[None, :] < n)
    count = fits.sum(axis=1)
    assert np.all(count > 0)
    k = np.minimum((oracle.random_f64(seed, n) * count).astype(np.int64), count - 1)
    return np.argmax((np.cumsum(fits, axis=1) == (k + 1)[:, None]) & fits, axis=1)


_OPS = {}


def _cached(name, make):
    if name not in _OPS:
        _OPS[name] = make()
    return _OPS[name]


# Unique rows of length 0, 1, 7, 8, 9, 16, 17 (the kernels take entries eight at a time) behind the identity row 0 that the
# margins use; rows 2 (1 entry), 3 (7 entries) and 5 (9 entries) have no offset 0.
EDGE_LENGTHS = (1, 0, 1, 7, 8, 9, 16, 17)
EDGE_WITH_ZERO = (True, False, False, False, True, False, True, True)
EDGE_REACH = 40


def edge_operator(oracle, n=10007):
    def make():
        offs = [[0]] + [_offsets(oracle, 100 + r, EDGE_LENGTHS[r], EDGE_REACH, EDGE_WITH_ZERO[r]) if EDGE_LENGTHS[r] else []
                        for r in range(1, len(EDGE_LENGTHS))]
        row, col, val = _table(offs, oracle, 7)
        idx = _iid_and_runs(oracle, 11, n, np.arange(len(offs)))
        idx[:EDGE_REACH] = 0
        idx[n - EDGE_REACH:] = 0                       # identity-only margins keep every i + col[j] inside [0, n)
        return Op("edges%d" % n, idx, row, col, val)
    return _cached("edges%d" % n, make)


RAGGED_SIZES = (1, 2, 3, 511, 512, 513, 1023, 2049, 100003)
RAGGED_ROWS = ([0], [-1, 0, 1], [1], [-2, -1], [], [-5, 3, -1, 4, 2, -3, 5, 1, -4])


def ragged_operator(oracle, n):
    def make():
        row, col, val = _table(RAGGED_ROWS, oracle, 21)
        return Op("ragged%d" % n, _fitting_idx(oracle, 1000 + n, n, RAGGED_ROWS), row, col, val)
    return _cached("ragged%d" % n, make)


def many_rows_operator(oracle, trimmed):
    """m = 1500 unique rows of 1 to 3 entries (tables in global memory); trimmed to the leading rows that fit KTABLE entries."""
    def make():
        m, n, reach = 1500, 20011, 3
        lens = 1 + (oracle.random_f64(31, m) * 3).astype(np.int64)
        offs = [[0]] + [_offsets(oracle, 2000 + r, int(lens[r]), reach, r % 2 == 0) for r in range(1, m)]
        if trimmed:
            keep = int(np.searchsorted(np.cumsum([len(o) for o in offs]), KTABLE, side="right"))
            offs = offs[:keep]
        row, col, val = _table(offs, oracle, 33)
        idx = _iid_and_runs(oracle, 35, n, np.arange(len(offs)))
        idx[:reach] = 0
        idx[n - reach:] = 0
        return Op("many_rows_%s" % ("lds" if trimmed else "global"), idx, row, col, val)
    return _cached("many%d" % trimmed, make)


def long_row_operator(oracle, trimmed):
    """One unique row of 1100 entries with offsets within +-600 (more entries than KTABLE); trimmed to 1000 entries."""
    def make():
        n, reach = 20011, 600
        offs = [[0], _offsets(oracle, 41, 1000 if trimmed else 1100, reach, False), [-2, 0, 7]]
        row, col, val = _table(offs, oracle, 43)
        idx = _iid_and_runs(oracle, 45, n, np.array([0, 1, 1, 2]))
        idx[:reach] = 0
        idx[n - reach:] = 0
        return Op("long_row_%s" % ("lds" if trimmed else "global"), idx, row, col, val)
    return _cached("long%d" % trimmed, make)


def seven_point_operator(far, n, nx=512):
    """7-point operator on lines of nx points, far = points per plane; boundary points and the first and last plane use the
    identity row."""
    def make():
        assert far % nx == 0
        ny = far // nx
        row = [0, 1, 8]
        col = [0, -far, -nx, -1, 0, 1, nx, far]
        val = [1.0, -0.3125, 0.41, -0.77, 5.3, 0.19, -0.6, 0.23]
        i = np.arange(n)
        x, y = i % nx, (i // nx) % ny
        inner = (i >= far) & (i < n - far) & (x > 0) & (x < nx - 1) & (y > 0) & (y < ny - 1)
        return Op("seven_point_%d_%d" % (far, n), inner.astype(np.uint32), row, col, val)
    return _cached("seven%d_%d" % (far, n), make)


# ---------------------------------------------------------------------------------------------------------------------------
# host restatement of the launch geometry (ccsr.hip: launch_ccsr / spmv_ccsr and strip_block)
# ---------------------------------------------------------------------------------------------------------------------------
def rows_per_block(rpl):
    return 512 if rpl == 0 else 256 * rpl


def strip_geometry(rpl, far, n):
    """None in plain order, else (chunk, planes, plane_blocks, tiles) of the strip traversal."""
    rows = rows_per_block(rpl)
    if not (far >= 131072 and far % rows == 0 and n >= 524288):
        return None
    nb = (n + rows - 1) // rows
    plane_blocks = far // rows
    chunk = max(1, min(64 * 512 // rows, plane_blocks // 8))
    planes = (nb + plane_blocks - 1) // plane_blocks
    tiles = (plane_blocks + 8 * chunk - 1) // (8 * chunk)
    return chunk, planes, plane_blocks, tiles


def strip_blocks(rpl, far, n):
    """The logical block of every workgroup of the launch (strip_block), -1 where the workgroup returns."""
    chunk, planes, plane_blocks, tiles = strip_geometry(rpl, far, n)
    nb = (n + rows_per_block(rpl) - 1) // rows_per_block(rpl)
    b = np.arange(tiles * planes * 8 * chunk, dtype=np.int64)
    k, q = b & 7, b >> 3
    r, i = q // chunk, q % chunk
    tile, p = r // planes, r % planes
    l = tile * (8 * chunk) + k * chunk + i
    lb = p * plane_blocks + l
    return np.where((l < plane_blocks) & (lb < nb), lb, -1)


STRIP_A = (131072, 5 * 131072 + 777)          # ragged last plane, ragged last block
STRIP_B = (512 * 300, 4 * 512 * 300 + 1)      # plane_blocks is not a multiple of 8 * chunk: the `l < plane_blocks` guard is live


@every_form
@pytest.mark.parametrize("case", (STRIP_A, STRIP_B), ids=("far131072", "far153600"))
def test_strip_traversal_is_on_and_visits_every_block_once(rpl, case):
    """The condition of the strip traversal restated on the host: it is ON for every form in both cases.  (153600 = 75 * 2048,
    so the RPL = 8 form, 2048 rows per block, takes the traversal in the second case too -- with 75 blocks per plane and
    chunk 9.)  The restated `strip_block` maps the launch onto every logical block exactly once; in the second case the
    blocks of a plane do not fill its last tile for every form but RPL = 1 (600 blocks = 8 chunks of 75), so some workgroups
    of the grid return at the `l < plane_blocks` guard."""
    far, n = case
    geo = strip_geometry(rpl, far, n)
    assert geo is not None and strip_geometry(rpl, 0, n) is None
    chunk, planes, plane_blocks, tiles = geo
    lb = strip_blocks(rpl, far, n)
    nb = (n + rows_per_block(rpl) - 1) // rows_per_block(rpl)
    assert np.array_equal(np.sort(lb[lb >= 0]), np.arange(nb))
    assert planes * plane_blocks > nb                                    # ragged last plane
    assert n % rows_per_block(rpl) != 0                                  # ragged last block
    if case == STRIP_B:
        assert (plane_blocks % (8 * chunk) != 0) == (rpl != 1)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
def vectors(oracle, op, dtype):
    x = (oracle.random_f64(5000 + op.n, max(1, op.n))[:op.n] - 0.5).astype(dtype)
    y0 = (oracle.random_f64(6000 + op.n, max(1, op.n))[:op.n] - 0.5).astype(dtype)
    return x, y0


def reference(oracle, op, dtype, x, y0, alpha, append):
    ptr, col, val = op.csr(dtype)
    if op.n == 0:
        return np.zeros(0, dtype=dtype)
    y = y0.copy() if append else np.full(op.n, np.nan, dtype=dtype)
    return oracle.spmv_csr(ptr, col, val, x, y, alpha, bool(append))


def plain_loop(op, dtype, x, y0, alpha, append):
    """s = 0; for j in table order: s = s + val[j] * x[i + col[j]]; y = alpha * s (+ y0) -- scalar arithmetic in `dtype`."""
    t = np.dtype(dtype).type
    val = op.val.astype(dtype)
    out = np.empty(op.n, dtype=dtype)
    for i in range(op.n):
        s = t(0)
        for j in range(int(op.row[op.idx[i]]), int(op.row[op.idx[i] + 1])):
            s = s + val[j] * x[i + int(op.col[j])]
        y = t(alpha) * s
        out[i] = y0[i] + y if append else y
    return out


@every_dtype
def test_host_expansion_through_the_oracle_equals_the_plain_loop(oracle, dtype):
    """Pins the reference of this file without a GPU: expansion + oracle.spmv_csr == the loop of the kernel's contract, bit for
    bit, in the arithmetic of `dtype`."""
    ops = [edge_operator(oracle, 397), ragged_operator(oracle, 3), ragged_operator(oracle, 513)]
    for op in ops:
        x, y0 = vectors(oracle, op, dtype)
        assert x.dtype == dtype
        for alpha, append in MODES:
            want = plain_loop(op, dtype, x, y0, alpha, append)
            got = reference(oracle, op, dtype, x, y0, alpha, append)
            assert got.dtype == dtype and np.array_equal(got, want), (op.name, alpha, append)
    lens = np.diff(ops[0].row.astype(np.int64))
    assert sorted(set(lens[ops[0].idx])) == [0, 1, 7, 8, 9, 16, 17]      # every length is in use
    zero_free = [r for r in range(ops[0].m) if lens[r] and 0 not in ops[0].col[ops[0].row[r]:ops[0].row[r + 1]]]
    assert len(zero_free) >= 2


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
    return g


@contextlib.contextmanager
def form(L, rpl):
    L.spmv_ccsr_set_rows_per_lane(rpl)
    try:
        yield
    finally:
        L.spmv_ccsr_set_rows_per_lane(0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


Y_GUARD = 12345.0


class Device:
    """The operator and its vectors on the device.  Every array is a view into a larger buffer, so that a view can start one
    element later (idx at 4 mod 8, y at 8 mod 16 for double / 4 mod 8 for float, x moved by one element); x is surrounded by
    NaN and y by a guard value that must survive."""

    def __init__(self, G, op, dtype, x, idx_off=0, x_off=0, y_off=0):
        torch = G.torch
        self.G, self.op, self.dtype, self.n = G, op, dtype, op.n
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(G.dev)
        ibuf = np.zeros(op.n + 4, dtype=np.int32)
        self.i0 = 2 + idx_off
        ibuf[self.i0:self.i0 + op.n] = op.idx.view(np.int32)
        self.ibuf = up(ibuf)
        self.idx = self.ibuf[self.i0:self.i0 + op.n]
        xbuf = np.full(op.n + 6, np.nan, dtype=dtype)
        self.x0 = 2 + x_off
        xbuf[self.x0:self.x0 + op.n] = x
        self.xbuf = up(xbuf)
        self.x = self.xbuf[self.x0:self.x0 + op.n]
        self.y0 = 2 + y_off
        self.row, self.col, self.val = up(op.row.view(np.int32)), up(op.col), up(op.val.astype(dtype))
        assert self.ibuf.data_ptr() % 16 == 0 and self.xbuf.data_ptr() % 16 == 0
        assert (self.idx.data_ptr() % 8 == 4) == bool(idx_off)
        assert (self.x.data_ptr() % (2 * x.itemsize) != 0) == bool(x_off)

    def product(self, y_init, alpha, append, far=0):
        torch, op = self.G.torch, self.op
        ybuf = np.full(op.n + 6, Y_GUARD, dtype=self.dtype)
        ybuf[self.y0:self.y0 + op.n] = y_init
        dy = torch.from_numpy(ybuf).to(self.G.dev)
        y = dy[self.y0:self.y0 + op.n]
        assert dy.data_ptr() % 16 == 0 and (y.data_ptr() % (2 * ybuf.itemsize) != 0) == (self.y0 != 2)
        fn = self.G.L.spmv_ccsr_f64 if self.dtype == np.float64 else self.G.L.spmv_ccsr_f32
        fn(0, None, op.n, alpha, int(append), _p(self.idx), op.m, _p(self.row), _p(self.col), _p(self.val), op.entries, far,
           _p(self.x), _p(y))
        out = dy.cpu().numpy()
        assert np.all(out[:self.y0] == Y_GUARD) and np.all(out[self.y0 + op.n:] == Y_GUARD), "a store outside y"
        return out[self.y0:self.y0 + op.n].copy()


def first_difference(got, want):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return "no difference" if len(bad) == 0 else "first differing index %d of %d (%d differ): got %r, want %r" % (
        bad[0], len(got), len(bad), got[bad[0]], want[bad[0]])


def check_operator(G, oracle, op, dtype, mode, far=0, offsets=(0, 0, 0), x=None):
    """One product against the oracle; SET starts from NaN in every row (each must be written), APPEND from random y0 (a row
    written twice changes bits).  Returns the result."""
    alpha, append = mode
    x0, y0 = vectors(oracle, op, dtype)
    x = x0 if x is None else x
    want = reference(oracle, op, dtype, x, y0, alpha, append)
    dev = Device(G, op, dtype, x, *offsets)
    got = dev.product(y0 if append else np.full(op.n, np.nan, dtype=dtype), alpha, append, far)
    assert np.array_equal(got, want, equal_nan=True), (op.name, np.dtype(dtype).name, mode, far, offsets, first_difference(got, want))
    return got


@pytest.mark.gpu
@every_mode
@every_dtype
@every_form
def test_row_lengths_at_the_eight_at_a_time_edges(G, oracle, rpl, dtype, mode):
    """Unique rows of 0, 1, 7, 8, 9, 16 and 17 entries, three of them without offset 0, drawn at random per row (pairs with
    p0 != p1) and in runs (p0 == p1 across whole waves), on an odd number of rows."""
    op = edge_operator(oracle)
    assert op.n % 2 == 1 and op.in_lds()
    with form(G.L, rpl):
        got = check_operator(G, oracle, op, dtype, mode)
    assert np.all(np.isfinite(got))
    pairs = op.idx[0:op.n - 1:2] == op.idx[1:op.n:2]
    assert pairs.any() and (~pairs).any()


@pytest.mark.gpu
@every_mode
@every_dtype
@every_form
def test_ragged_sizes(G, oracle, rpl, dtype, mode):
    """Sizes around the block sizes of every form, odd sizes (the last lane of the pair form owns one row) and 1, 2, 3 rows."""
    with form(G.L, rpl):
        for n in RAGGED_SIZES:
            op = ragged_operator(oracle, n)
            got = check_operator(G, oracle, op, dtype, mode)
            assert np.all(np.isfinite(got)), n


@pytest.mark.gpu
@every_mode
@every_dtype
@every_form
def test_tables_in_global_memory_and_in_lds(G, oracle, rpl, dtype, mode):
    """m > 1024 unique rows, and a unique row of more than 1024 entries: the instantiations that read the tables from global
    memory; the same operators trimmed to the LDS instantiation."""
    with form(G.L, rpl):
        for make in (many_rows_operator, long_row_operator):
            big, small = make(oracle, False), make(oracle, True)
            assert not big.in_lds() and small.in_lds()
            check_operator(G, oracle, big, dtype, mode)
            check_operator(G, oracle, small, dtype, mode)
    assert many_rows_operator(oracle, False).m == 1500 and long_row_operator(oracle, False).entries > 1100


@pytest.mark.gpu
@every_mode
@every_dtype
@every_form
def test_views_that_are_not_16_byte_aligned(G, oracle, rpl, dtype, mode):
    """idx at 4 mod 8 (no 8-byte position loads), y at one element past a 16-byte boundary (no vector stores), x moved by one
    element: each alone and all together give the bits of the aligned run (which are the oracle's)."""
    op = edge_operator(oracle, 10008)                  # an even size too: every lane of the pair form owns two rows
    with form(G.L, rpl):
        base = check_operator(G, oracle, op, dtype, mode)
        for offsets in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            got = check_operator(G, oracle, op, dtype, mode, offsets=offsets)
            assert np.array_equal(got, base), (offsets, first_difference(got, base))
        odd = edge_operator(oracle)
        base = check_operator(G, oracle, odd, dtype, mode)
        assert np.array_equal(check_operator(G, oracle, odd, dtype, mode, offsets=(1, 1, 1)), base)


@pytest.mark.gpu
@every_mode
@every_dtype
@every_form
@pytest.mark.parametrize("case", (STRIP_A, STRIP_B), ids=("far131072", "far153600"))
def test_strip_traversal_equals_plain_order(G, oracle, case, rpl, dtype, mode):
    """7-point operator whose far offset is a plane of 131072 / 153600 points: with far_offset passed the launch walks the
    blocks in strips (ON for every form in both cases: test_strip_traversal_is_on_and_visits_every_block_once restates the
    condition), with far_offset = 0 in plain order; both equal the oracle and so each other.  A block skipped leaves NaN
    (SET) and a block visited twice adds twice (APPEND)."""
    far, n = case
    assert strip_geometry(rpl, far, n) is not None and strip_geometry(rpl, 0, n) is None
    op = seven_point_operator(far, n)
    with form(G.L, rpl):
        strips = check_operator(G, oracle, op, dtype, mode, far=far)
        plain = check_operator(G, oracle, op, dtype, mode, far=0)
    assert np.array_equal(strips, plain)


@pytest.mark.gpu
@every_mode
@every_dtype
@every_form
def test_nan_and_inf_stay_in_the_rows_that_reference_them(G, oracle, rpl, dtype, mode):
    """Padding lanes of a group of eight read x[i] (x[i], x[i + 1] in the pair form) and must not add it: NaN and +-Inf are
    planted at exactly those positions of rows whose unique row has no offset 0 and a length that is not a multiple of 8, and
    at a few positions rows do reference.  Bits of the oracle (NaN == NaN); rows that reference no planted position are finite."""
    op = edge_operator(oracle)
    lens = np.diff(op.row.astype(np.int64))
    zero_free = [r for r in range(op.m) if lens[r] % 8 and 0 not in op.col[op.row[r]:op.row[r + 1]]]
    assert len(zero_free) >= 2
    rows = np.flatnonzero(np.isin(op.idx, zero_free))
    rows = rows[(rows > 2 * EDGE_REACH) & (rows < op.n - 2 * EDGE_REACH)]
    rows = rows[::max(1, len(rows) // 24)][:24]
    planted = np.unique(np.concatenate([rows, rows + 1, [op.n // 3, op.n // 2 + 1, op.n - 1, 0]]))
    x, _ = vectors(oracle, op, dtype)
    x = x.copy()
    x[planted] = np.resize(np.array([np.nan, np.inf, -np.inf], dtype=dtype), len(planted))
    ptr, col, _ = op.csr(dtype)
    touched = np.zeros(op.n, dtype=bool)
    touched[np.repeat(np.arange(op.n), np.diff(ptr))[np.isin(col, planted)]] = True
    assert (~touched[rows]).any(), "no planted row is free of planted columns: the case would show nothing"
    with form(G.L, rpl):
        got = check_operator(G, oracle, op, dtype, mode, x=x)
    assert np.all(np.isfinite(got[~touched]))
    assert not np.all(np.isfinite(got[touched]))


@pytest.mark.gpu
@every_dtype
@every_form
def test_no_rows_is_a_no_op(G, rpl, dtype):
    """n = 0 returns 0 without looking at an argument and without a launch."""
    torch = G.torch
    y = torch.full((8,), Y_GUARD, dtype=torch.float64 if dtype == np.float64 else torch.float32, device=G.dev)
    fn = G.L.spmv_ccsr_f64 if dtype == np.float64 else G.L.spmv_ccsr_f32
    with form(G.L, rpl):
        for append in (0, 1):
            fn(0, None, 0, 2.5, append, None, 0, None, None, None, 0, 0, None, None)
            fn(0, None, 0, 2.5, append, None, 0, None, None, None, 0, 131072, None, _p(y))
    assert np.all(y.cpu().numpy() == Y_GUARD)
