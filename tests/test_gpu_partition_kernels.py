"""Direct parity tests of the kernels every multi-device product rests on, called through the C ABI with torch tensors as device
buffers:

  * `vexhip_csr_split_sizes_i32`, `vexhip_csr_split_{f64,f32}_i32` (vexcl_amd/csrc/split.hip): one strip -> local part, row-subset
    remote part, sorted ghost set;
  * `vexhip_csr_extend_halo_i32` (same file): the strip with its ghost planes;
  * `vexhip_spmv_csr_rows_{f64,f32}_i32` (`csr_rows_kernel`, spmv.hip): the remote product;
  * `vexhip_gather_{f64,f32}_i32` (`gather_kernel`): the owner-side pack;
  * and all of them composed to the product of every rank of a world, in one process.

References: `oracle.split_rows` (the host set-up of the reference, spmat.hpp:291-378), `oracle.spmv_split` (its five-phase apply)
and `oracle.spmv_csr`.  Integers are compared with `np.array_equal`, values as raw bits; spmv.hip is compiled with
-ffp-contract=off and folds a row in CSR order like the oracle's loop, so the products are compared exactly too -- there is no
tolerance anywhere in this file.  Every output buffer ends in GUARD elements that hold a sentinel and must keep it."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 16
SENTINEL = {np.dtype(np.int32): np.int32(-1515870811), np.dtype(np.float64): np.float64(12345.0), np.dtype(np.float32): np.float32(12345.0)}
BITS = {np.dtype(np.float64): np.int64, np.dtype(np.float32): np.int32, np.dtype(np.int32): np.int32}

SCAN_TILE = 4096                  # scan.hip: cfg<int>::TILE = SBLOCK * VN * SK = 256 * 4 * 4 elements per workgroup
SCAN_LOOKBACK_TILES = 64          # scan.hip scan_impl: integer scans of this many tiles or more take the single-pass kernel
SORT_TILE = 12288                 # sort.hip: tile_keys<unsigned, 0>() = UB * (48 KiB / 4 / UB), UB = 768
SPLIT_BLOCKS_PER_CU = 16          # split.hip grid_for and the gather launch: at most cus * 16 workgroups of 256
ROWS_BLOCKS_PER_CU = 32           # spmv.hip spmv_csr_rows: at most cus * 32 workgroups of 256
BLOCK = 256

WORLDS = (1, 2, 3, 5, 8)


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def G(request):
    import torch                                        # before libvexhip.so: the process settles on torch's HIP runtime
    import vexcl_amd
    from vexcl_amd._capi import DeviceProps

    class NS:
        pass
    g = NS()
    g.torch, g.L, g.dev = torch, request.getfixturevalue("built_lib"), torch.device("cuda:0")
    g.ops, g.Error = vexcl_amd.ops, vexcl_amd.Error
    props = DeviceProps()
    g.L.device_get_props(0, ctypes.byref(props))
    g.cus = int(props.compute_units)
    assert g.cus > 0
    return g


def _p(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def up(G, a):
    return G.torch.from_numpy(np.ascontiguousarray(a)).to(G.dev)


def guarded(G, count, dtype):
    """`count` elements and GUARD more, all holding the sentinel: an element the call does not write shows, too."""
    return up(G, np.full(count + GUARD, SENTINEL[np.dtype(dtype)], dtype=dtype))


def payload(buf, count, what):
    out = buf.cpu().numpy()
    assert len(out) == count + GUARD
    assert np.all(out[count:] == SENTINEL[out.dtype]), "a store behind %s" % what
    return out[:count].copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(BITS[a.dtype]), b.view(BITS[b.dtype]))


class Split:
    """One call of sizes() and one of split() on a strip (row pointers from 0, GLOBAL columns), every output allocated as
    include/vexhip.h says plus the guard.  The device tensors stay alive in `self.d` for the products built on them."""

    def __init__(self, G, ptr, col, val, c0, c1):
        torch, L = G.torch, G.L
        n = len(ptr) - 1
        dtype = np.dtype(val.dtype)
        src = (up(G, ptr.astype(np.int32)), up(G, col.astype(np.int32)), up(G, val))
        sizes = (ctypes.c_int64 * 4)(-5, -5, -5, -5)
        L.csr_split_sizes_i32(0, None, n, _p(src[0]), _p(src[1]), int(c0), int(c1), sizes)
        self.first = [int(s) for s in sizes]
        lnnz, rnnz, nr = self.first[:3]
        assert min(lnnz, rnnz, nr) >= 0 and lnnz + rnnz == len(col) and nr <= n
        b = dict(lptr=guarded(G, n + 1, np.int32), lcol=guarded(G, lnnz, np.int32), lval=guarded(G, lnnz, dtype),
                 rem_rows=guarded(G, nr, np.int32), rem_ptr=guarded(G, nr + 1, np.int32), rem_col=guarded(G, rnnz, np.int32),
                 rem_val=guarded(G, rnnz, dtype), ghosts=guarded(G, rnnz, np.int32))
        fn = L.csr_split_f64_i32 if dtype == np.float64 else L.csr_split_f32_i32
        fn(0, None, n, _p(src[0]), _p(src[1]), _p(src[2]), int(c0), int(c1), sizes, _p(b["lptr"]), _p(b["lcol"]), _p(b["lval"]),
           _p(b["rem_rows"]), _p(b["rem_ptr"]), _p(b["rem_col"]), _p(b["rem_val"]), _p(b["ghosts"]))
        torch.cuda.synchronize()
        self.sizes = [int(s) for s in sizes]
        self.n, self.lnnz, self.rnnz, self.nr = n, lnnz, rnnz, nr
        self.ng = self.sizes[3]
        assert 0 <= self.ng <= rnnz
        count = dict(lptr=n + 1, lcol=lnnz, lval=lnnz, rem_rows=nr, rem_ptr=nr + 1, rem_col=rnnz, rem_val=rnnz, ghosts=rnnz)
        self.h = {k: payload(b[k], count[k], k) for k in b}
        self.h["ghosts"] = self.h["ghosts"][:self.ng]
        self.d = {k: b[k][:count[k]] for k in b}
        self.d["ghosts"] = self.d["ghosts"][:self.ng]
        self.src = src
        # the strip itself is an input
        assert np.array_equal(src[0].cpu().numpy(), ptr) and np.array_equal(src[1].cpu().numpy(), col) and same_bits(src[2].cpu().numpy(), val)


def host_split(ptr, col, val, c0, c1):
    """The layout of `oracle.split_rows` for ONE strip and an explicit column range (the hand-made strips below have no
    partition); check_split pins it to the oracle wherever both apply."""
    n = len(ptr) - 1
    c = col.astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(ptr.astype(np.int64)))
    is_loc = (c >= c0) & (c < c1)
    ghosts = np.unique(c[~is_loc])

    def rowptr(mask):
        return np.concatenate([[0], np.cumsum(np.bincount(rows[mask], minlength=n))]).astype(np.int32)

    return dict(loc=(rowptr(is_loc), (c[is_loc] - c0).astype(np.int32), val[is_loc].copy()),
                rem=(rowptr(~is_loc), np.searchsorted(ghosts, c[~is_loc]).astype(np.int32), val[~is_loc].copy()), ghosts=ghosts)


def check_split(G, ptr, col, val, c0, c1, want=None):
    """Splits on the device and compares every array with `want` (a device entry of oracle.split_rows; default: host_split)."""
    mine = host_split(ptr, col, val, c0, c1)
    if want is None:
        want = mine
    else:
        for k in ("loc", "rem"):
            assert all(np.array_equal(a, b) for a, b in zip(mine[k][:2], want[k][:2])) and same_bits(mine[k][2], want[k][2])
        assert np.array_equal(mine["ghosts"], want["ghosts"])
    s = Split(G, ptr, col, val, c0, c1)
    lptr, lcol, lval = want["loc"]
    rptr_full, rcol, rval = want["rem"]
    ghosts = np.asarray(want["ghosts"], dtype=np.int64)
    rows = np.flatnonzero(np.diff(rptr_full.astype(np.int64))).astype(np.int32)
    where = (len(ptr) - 1, len(col), c0, c1)
    assert s.first == [len(lcol), len(rcol), len(rows), -1], where
    assert s.sizes == [len(lcol), len(rcol), len(rows), len(ghosts)], where
    assert len(ghosts) == 0 or (np.all(np.diff(ghosts) > 0) and len(rcol) > 0)
    assert np.array_equal(s.h["lptr"], lptr), where                       # n == 0: [0]
    assert np.array_equal(s.h["lcol"], lcol), where
    assert same_bits(s.h["lval"], lval), where
    assert np.array_equal(s.h["ghosts"].astype(np.int64), ghosts), where
    assert np.array_equal(s.h["rem_rows"], rows), where
    assert np.array_equal(s.h["rem_ptr"], np.concatenate([rptr_full[rows], [len(rcol)]]).astype(np.int32)), where   # no remote entry: [0]
    assert np.array_equal(s.h["rem_col"], rcol), where
    assert same_bits(s.h["rem_val"], rval), where
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# matrices: name -> (ptr, col, val, columns)
# ---------------------------------------------------------------------------------------------------------------------------
def _from_rows(rows, val_of):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if ptr[-1] else np.zeros(0, dtype=np.int32)
    return ptr, col, val_of(len(col))


def _two_far_columns(oracle):
    """Row i = columns 0, i, m - 1 (rows 0 and m - 1 hold their far column twice): every row of every strip reaches a ghost,
    and the ghost set is {0}, {m - 1} or both."""
    m = 1024
    return _from_rows([[0, i, m - 1] for i in range(m)], lambda k: oracle.random_f64(71, k) - 0.5) + (m,)


def _unsorted_duplicates(oracle):
    """Rows of random_matrix in descending column order, with the row's smallest and largest column once more in front."""
    ptr, col, _ = oracle.random_matrix(13, 1024, 1024, 16)
    rows = []
    for i in range(1024):
        r = list(col[ptr[i]:ptr[i + 1]][::-1])
        rows.append(r[-1:] + r[:1] + r)
    return _from_rows(rows, lambda k: oracle.random_f64(73, k) - 0.5) + (1024,)


def _lower_triangle(oracle):
    ptr, col, val = oracle.poisson3d(12)
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    keep = col <= rows
    return np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32), col[keep].copy(), val[keep].copy(), n


def _special_values_f32(oracle):
    ptr, col, val = oracle.random_matrix(3, 1024, 1024, 16)
    val = (val - 0.5).astype(np.float32)
    special = np.array([0x7FC00123, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x80000100], dtype=np.uint32).view(np.float32)
    assert np.isnan(special[:2]).all() and np.isinf(special[2:4]).all() and np.signbit(special[4]) and special[4] == 0 and 0 < special[5] < 1e-44
    at = (np.arange(7 * 40) * 53) % len(val)
    val[at] = np.resize(special, len(at))
    return ptr, col, val, 1024


MATRICES = {
    "random_1024": lambda o: o.random_matrix(1, 1024, 1024, 16) + (1024,),
    "random_1024x2048": lambda o: o.random_matrix(2, 1024, 2048, 16) + (2048,),
    "random_40_empty_tail": lambda o: o.random_matrix(4, 40, 40, 6, empty_tail=3) + (40,),
    "random_40x100_empty_tail": lambda o: o.random_matrix(5, 40, 100, 6, empty_tail=3) + (100,),
    "poisson_12": lambda o: o.poisson3d(12) + (12 ** 3,),
    "poisson_12_lower": _lower_triangle,
    "two_far_columns": _two_far_columns,
    "unsorted_duplicates": _unsorted_duplicates,
    "special_values_f32": _special_values_f32,
}
SPLIT_CASES = [(name, w) for name in MATRICES for w in ((8,) if name.startswith("random_40") else WORLDS)]
_CACHE = {}


def matrix(oracle, name):
    key = ("matrix", name)
    if key not in _CACHE:
        ptr, col, val, m = MATRICES[name](oracle)
        assert ptr.dtype == np.int32 and col.dtype == np.int32 and len(col) == ptr[-1] == len(val)
        assert len(col) == 0 or (col.min() >= 0 and col.max() < m)
        _CACHE[key] = (ptr, col, val, m)
    return _CACHE[key]


def split_world(G, oracle, name, world):
    """(oracle.split_rows of the matrix, the checked device split of every rank); computed once."""
    key = ("split", name, world)
    if key not in _CACHE:
        ptr, col, val, m = matrix(oracle, name)
        S = oracle.split_rows(ptr, col, val, m, world)
        assert S["part"] == oracle.partition(len(ptr) - 1, world) and S["col_part"] == oracle.partition(m, world)
        ranks = []
        for d, D in enumerate(S["devs"]):
            (r0, r1), (c0, c1) = D["rows"], D["cols"]
            j0, j1 = int(ptr[r0]), int(ptr[r1])
            ranks.append(check_split(G, ptr[r0:r1 + 1] - ptr[r0], col[j0:j1], val[j0:j1], c0, c1, want=D))
        _CACHE[key] = (S, ranks)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the split
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,world", SPLIT_CASES, ids=["%s-world%d" % c for c in SPLIT_CASES])
def test_split_of_every_rank_equals_the_host_set_up(G, oracle, name, world):
    S, ranks = split_world(G, oracle, name, world)
    ptr, col, val, m = matrix(oracle, name)
    assert sum(s.lnnz + s.rnnz for s in ranks) == len(col) and sum(s.n for s in ranks) == len(ptr) - 1
    if world == 1:
        assert ranks[0].sizes == [len(col), 0, 0, 0]
    if name.startswith("random_40"):
        assert any(s.n == 0 for s in ranks), "no empty strip in this partition"
        assert any(s.n > 0 and s.rnnz > 0 for s in ranks)
    if name == "two_far_columns" and world > 1:
        assert all(s.nr == s.n and 1 <= s.ng <= 2 for s in ranks)
    if name == "unsorted_duplicates" and world > 1:
        assert all(s.ng < s.rnnz for s in ranks)                 # columns repeat in the remote part
    if name == "poisson_12_lower" and world > 1:
        assert ranks[0].rnnz == 0 and all(s.rnnz > 0 for s in ranks[1:])      # one-sided coupling


def _strip(rows, dtype=np.float64):
    return _from_rows(rows, lambda k: (np.arange(k) * 0.37 - 1.25).astype(dtype))


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("float64", "float32"))
def test_hand_made_strips(G, dtype):
    """The ABI with explicit col_begin / col_end, independent of any partition."""
    # the half-open range [c0, c1): columns c0 - 1, c0, c1 - 1, c1 in both orders and one per row
    c0, c1 = 32, 64
    s = check_split(G, *_strip([[31, 32, 63, 64], [64, 63, 32, 31], [31], [32], [63], [64], [], [64, 64, 31, 31, 32]], dtype), c0, c1)
    assert s.sizes == [7, 10, 5, 2] and list(s.h["ghosts"]) == [31, 64] and list(s.h["rem_rows"]) == [0, 1, 2, 5, 7]
    assert list(s.h["lcol"]) == [0, 31, 31, 0, 0, 31, 0] and list(s.h["rem_col"]) == [0, 1, 1, 0, 0, 1, 1, 1, 0, 0]
    # an empty range: every entry is remote
    for c in (0, 48):
        s = check_split(G, *_strip([[0, 47, 48, 49], [], [48], [100, 0]], dtype), c, c)
        assert s.sizes == [0, 7, 3, 5] and not s.h["lptr"].any()
    # every entry local: rem_ptr is the row pointer of a matrix without rows
    s = check_split(G, *_strip([[5, 3], [], [7, 7, 0]], dtype), 0, 8)
    assert s.sizes == [5, 0, 0, 0] and list(s.h["rem_ptr"]) == [0]
    # every entry remote
    s = check_split(G, *_strip([[5, 3], [], [9, 9, 0]], dtype), 6, 9)
    assert s.sizes == [0, 5, 2, 4] and list(s.h["lptr"]) == [0, 0, 0, 0]
    # rows without entries: col and val are empty tensors (NULL)
    s = check_split(G, *_strip([[], [], []], dtype), 0, 4)
    assert s.sizes == [0, 0, 0, 0] and list(s.h["lptr"]) == [0, 0, 0, 0] and list(s.h["rem_ptr"]) == [0]
    # no rows
    for c0, c1 in ((0, 4), (16, 16)):
        s = check_split(G, *_strip([], dtype), c0, c1)
        assert s.sizes == [0, 0, 0, 0] and list(s.h["lptr"]) == [0] and list(s.h["rem_ptr"]) == [0]
    # the top of the signed range: the sort and the rank search meet 2^31 - 1
    top = 2 ** 31 - 1
    c0, c1 = 2 ** 31 - 48, 2 ** 31 - 16
    s = check_split(G, *_strip([[top, c0, 0], [c1, c1 - 1, c0 - 1, 5], [top, top, c1], [c0 + 1]], dtype), c0, c1)
    assert list(s.h["ghosts"].astype(np.int64)) == [0, 5, c0 - 1, c1, top] and list(s.h["rem_col"]) == [4, 0, 3, 2, 1, 4, 4, 3]


def test_split_refuses_a_reversed_column_range(G):
    """col_end < col_begin is refused by sizes() and by both split() entry points, each called directly with buffers a valid
    range [7, 8) would need; nothing is written."""
    ptr, col, val = _strip([[1, 2], [3]])
    with pytest.raises(G.Error):
        Split(G, ptr, col, val, 8, 7)                         # raises in sizes()
    dptr, dcol = up(G, ptr), up(G, col)
    for dtype, fn in ((np.float64, G.L.csr_split_f64_i32), (np.float32, G.L.csr_split_f32_i32)):
        dval = up(G, val.astype(dtype))
        sizes = (ctypes.c_int64 * 4)(-5, -5, -5, -5)
        ints = [guarded(G, 3, np.int32) for _ in range(6)]    # lptr, lcol, rem_rows, rem_ptr, rem_col, ghosts
        vals = [guarded(G, 3, dtype) for _ in range(2)]       # lval, rem_val
        with pytest.raises(G.Error):
            fn(0, None, 2, _p(dptr), _p(dcol), _p(dval), 8, 7, sizes, _p(ints[0]), _p(ints[1]), _p(vals[0]),
               _p(ints[2]), _p(ints[3]), _p(ints[4]), _p(vals[1]), _p(ints[5]))
        G.torch.cuda.synchronize()
        assert list(sizes) == [-5, -5, -5, -5]
        for b in ints + vals:
            assert np.all(b.cpu().numpy() == SENTINEL[np.dtype(b.cpu().numpy().dtype)])


def random_strip(oracle, seed, n, local, remote, c0, c1, m):
    """n rows, exactly `local` entries inside [c0, c1) and `remote` outside, dealt to the rows at random (rows without entries,
    unsorted and repeated columns)."""
    total = local + remote
    is_rem = np.zeros(total, dtype=bool)
    is_rem[np.argsort(oracle.random_f64(seed, max(1, total))[:total], kind="stable")[:remote]] = True
    inside = c0 + (oracle.random_f64(seed + 1, max(1, total))[:total] * (c1 - c0)).astype(np.int64)
    outside = (oracle.random_f64(seed + 2, max(1, total))[:total] * (m - (c1 - c0))).astype(np.int64)
    outside = np.where(outside >= c0, outside + (c1 - c0), outside)
    col = np.where(is_rem, outside, inside).astype(np.int32)
    rows = np.sort((oracle.random_f64(seed + 3, max(1, total))[:total] * n).astype(np.int64))
    rows[-1:] = n - 1                                         # the last row is never empty
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    val = oracle.random_f64(seed + 4, max(1, total))[:total] - 0.5
    assert ((col >= c0) & (col < c1)).sum() == local and col.min() >= 0 and col.max() < m
    return ptr, col, val


SCAN_EDGES = (SCAN_TILE - 1, SCAN_TILE, (SCAN_LOOKBACK_TILES - 1) * SCAN_TILE - 1, (SCAN_LOOKBACK_TILES - 1) * SCAN_TILE)


@pytest.mark.parametrize("n", SCAN_EDGES)
def test_row_counts_on_both_sides_of_a_scan_tile(G, oracle, n):
    """The row pointers are exclusive scans of n + 1 counts: n + 1 = one tile / one tile and an element, and 63 tiles / 63 tiles
    and an element (from 64 tiles on the scan is the single-pass kernel).  The compacted row list must keep its last row."""
    assert (n + 1) % SCAN_TILE in (0, 1)
    ptr, col, val = random_strip(oracle, 100 + n, n, 2 * n, n // 2, 1000, 3000, 5000)
    col[-1] = 4999                                            # the last row has a remote entry
    assert ptr[-1] > ptr[-2] and ptr[-1] == len(col)
    s = check_split(G, ptr, col, val, 1000, 3000)
    assert s.h["rem_rows"][-1] == n - 1 and 0 < s.nr < n


@pytest.mark.parametrize("remote", (SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 3 * SORT_TILE - 1, SCAN_TILE - 1, SCAN_TILE))
def test_remote_entries_on_both_sides_of_a_sort_tile(G, oracle, remote):
    """The ghost set sorts `remote nnz` keys (tiles of 12288) and scans remote nnz + 1 run flags (tiles of 4096)."""
    ptr, col, val = random_strip(oracle, 200 + remote, 3000, 5000, remote, 4096, 8192, 20000)
    s = check_split(G, ptr, col, val, 4096, 8192)
    assert s.rnnz == remote and s.ng < remote


def test_a_second_trip_of_every_grid_stride_loop(G, oracle):
    """cus * 16 * 256 + 257 rows with about 3 entries each, half of them remote: more rows and more remote entries than
    one trip of the largest grid of split.hip covers (its loops run over rows or over remote entries)."""
    one_trip = G.cus * SPLIT_BLOCKS_PER_CU * BLOCK
    n = one_trip + BLOCK + 1
    ptr, col, val = random_strip(oracle, 300, n, 3 * n // 2, 3 * n // 2, n // 4, 3 * n // 4, n)
    s = check_split(G, ptr, col, val, n // 4, 3 * n // 4)
    assert s.rnnz > one_trip and s.nr > one_trip // 2 and (n + 1) > SCAN_LOOKBACK_TILES * SCAN_TILE


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the strip with its ghost planes
# ---------------------------------------------------------------------------------------------------------------------------
def check_extend(G, ptr, col, col_begin, lo, hi):
    n, nnz = len(ptr) - 1, len(col)
    want_ptr = np.concatenate([np.zeros(lo, dtype=np.int32), ptr, np.full(hi, ptr[n], dtype=np.int32)]).astype(np.int32)
    ext = col.astype(np.int64) - (col_begin - lo)
    want_bad = int(((ext < 0) | (ext >= lo + n + hi)).sum())
    dptr, dcol = up(G, ptr.astype(np.int32)), up(G, col.astype(np.int32))
    ptr_ext, col_ext = guarded(G, lo + n + hi + 1, np.int32), guarded(G, nnz, np.int32)
    bad = ctypes.c_int64(-5)
    G.L.csr_extend_halo_i32(0, None, n, nnz, _p(dptr), _p(dcol), col_begin, lo, hi, _p(ptr_ext), _p(col_ext), ctypes.byref(bad))
    G.torch.cuda.synchronize()
    assert np.array_equal(payload(ptr_ext, lo + n + hi + 1, "ptr_ext"), want_ptr), (n, nnz, col_begin, lo, hi)
    assert np.array_equal(payload(col_ext, nnz, "col_ext"), ext.astype(np.int32)), (n, nnz, col_begin, lo, hi)
    assert bad.value == want_bad, (n, nnz, col_begin, lo, hi)
    assert np.array_equal(dptr.cpu().numpy(), ptr) and np.array_equal(dcol.cpu().numpy(), col)
    return want_bad


def test_extend_halo_of_a_stencil_strip(G):
    """A strip of the 7-point operator between its two ghost planes: nothing out of range; without one of the planes, the
    entries that reach it are counted."""
    from test_gpu_distributed import _stencil_strip
    nx, ny, planes, world = 16, 8, 4, 3
    P = nx * ny
    for rank in range(world):
        r0, r1 = rank * planes * P, (rank + 1) * planes * P
        ptr, col, _ = (t.cpu().numpy() for t in _stencil_strip(G.torch, nx, ny, planes * world, r0, r1, G.dev))
        full = (0 if rank == 0 else P, 0 if rank == world - 1 else P)
        assert check_extend(G, ptr, col, r0, *full) == 0
        reach = (nx - 2) * (ny - 2)                              # inner points of a plane
        for lo in {0, full[0]}:
            for hi in {0, full[1]}:
                assert check_extend(G, ptr, col, r0, lo, hi) == reach * ((lo < full[0]) + (hi < full[1]))


def test_extend_halo_edges(G, oracle):
    ptr, col, _ = _strip([[], [200, 199, 100, 99], [], [150]])
    # the four edges: the last valid and the first invalid column on each side (lo = 20, n = 4, hi = 76: columns 100 .. 199)
    assert check_extend(G, ptr, col, 120, 20, 76) == 2
    assert check_extend(G, ptr, col, 100, 0, 96) == 2           # a first-rank shape: lo == 0
    assert check_extend(G, ptr, col, 0, 0, 196) == 1            # col_begin == 0
    assert check_extend(G, ptr, col, 99, 0, 0) == 3
    # no entries
    ptr0 = np.zeros(6, dtype=np.int32)
    for lo, hi in ((0, 0), (7, 0), (0, 7), (7, 7)):
        assert check_extend(G, ptr0, np.zeros(0, dtype=np.int32), 7, lo, hi) == 0
    assert check_extend(G, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), 0, 0, 0) == 0
    # several workgroups add to the counter: one entry in 1000 lies outside, on alternating sides
    n, lo, hi, begin = 40000, 300, 500, 1000
    nnz = G.cus * SPLIT_BLOCKS_PER_CU * BLOCK + 1000 * BLOCK + 3            # a second trip of the loop too
    ptr = np.concatenate([[0], np.sort((oracle.random_f64(51, n) * nnz).astype(np.int64))[1:], [nnz]]).astype(np.int32)
    col = (begin - lo) + (oracle.random_f64(52, nnz) * (lo + n + hi)).astype(np.int64)
    out = np.arange(500, nnz, 1000)
    col[out] = np.where(out % 2000 < 1000, begin - lo - 1 - (out % 7), begin + n + hi + (out % 5))
    assert check_extend(G, ptr, col.astype(np.int32), begin, lo, hi) == len(out) and len(out) > BLOCK


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the row-subset product and the gather
# ---------------------------------------------------------------------------------------------------------------------------
def nonzero_hash(oracle, seed, n, dtype):
    y = (oracle.random_f64(seed, max(1, n))[:n] - 0.5).astype(dtype)
    y[y == 0] = 0.25
    return y


def subset_of(ptr, col, val, rows):
    """(compact row pointers, columns, values) of the listed rows (ascending), and the full-height CSR that has entries in
    those rows only."""
    n = len(ptr) - 1
    listed = np.zeros(n, dtype=bool)
    listed[rows] = True
    widths = np.diff(ptr.astype(np.int64))
    keep = np.repeat(listed, widths)
    cptr = np.concatenate([[0], np.cumsum(widths[rows])]).astype(np.int32)
    fptr = np.concatenate([[0], np.cumsum(np.where(listed, widths, 0))]).astype(np.int32)
    return cptr, np.ascontiguousarray(col[keep]), np.ascontiguousarray(val[keep]), fptr


def check_rows_product(G, oracle, ptr, col, val, rows, x, y0, alpha):
    dtype = val.dtype
    rows = np.asarray(rows, dtype=np.int32)
    cptr, ccol, cval, fptr = subset_of(ptr, col, val, rows)
    want = oracle.spmv_csr(fptr, ccol, cval, x, y0.copy(), alpha, True)
    y = guarded(G, len(y0), dtype)
    y[:len(y0)] = up(G, y0)
    d = [up(G, a) for a in (rows, cptr, ccol, cval, x)]
    fn = G.L.spmv_csr_rows_f64_i32 if dtype == np.float64 else G.L.spmv_csr_rows_f32_i32
    fn(0, None, len(rows), alpha, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), _p(d[4]), _p(y))
    got = payload(y, len(y0), "y")
    assert np.array_equal(got, want, equal_nan=True), (len(rows), alpha, np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])
    unlisted = np.ones(len(y0), dtype=bool)
    unlisted[rows] = False
    assert same_bits(got[unlisted], y0[unlisted])
    return got, cptr


@pytest.mark.parametrize("alpha", (1.0, -1.0, 1.5))
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("float64", "float32"))
def test_row_subset_product(G, oracle, dtype, alpha):
    """y[rows[k]] = y0[rows[k]] + alpha * (the row folded in CSR order), every other element of y and the guard untouched:
    exact for integer-valued inputs (every partial sum is exact) and for hash-valued reals (same order, no contraction)."""
    n, m = 301, 200
    ptr, col, hval = oracle.random_matrix(7, n, m, 9, empty_tail=4)
    widths = np.diff(ptr)
    empty, full = np.flatnonzero(widths == 0), np.flatnonzero(widths > 0)
    assert len(empty) > 4 and widths[n - 1] == 0
    last = int(full[-1])
    subsets = {"every row": np.arange(n), "one row": [int(full[len(full) // 2])], "first and last": [0, n - 1], "first and last with entries": [0, last],
               "rows without entries": empty, "a mix": np.sort(np.concatenate([full[::3], empty[::2]]))}
    ival = (oracle.random_i32(8, len(col), -8, 8)).astype(dtype)
    inputs = {"integers": (ival, oracle.random_i32(9, m, -16, 16).astype(dtype), (oracle.random_i32(10, n, 1, 50) * np.where(np.arange(n) % 2, 1, -1)).astype(dtype)),
              "hash": ((hval - 0.5).astype(dtype), nonzero_hash(oracle, 11, m, dtype), nonzero_hash(oracle, 12, n, dtype))}
    for val, x, y0 in inputs.values():
        assert not (y0 == 0).any()
        for rows in subsets.values():
            got, cptr = check_rows_product(G, oracle, ptr, col, val, rows, x, y0, alpha)
    # the oracle route against a plain loop in the arithmetic of dtype
    val, x, y0 = inputs["hash"]
    rows = subsets["a mix"]
    got, cptr = check_rows_product(G, oracle, ptr, col, val, rows, x, y0, alpha)
    t = np.dtype(dtype).type
    loop = y0.copy()
    for r in rows:
        s = t(0)
        for j in range(int(ptr[r]), int(ptr[r + 1])):
            s = s + val[j] * x[col[j]]
        loop[r] = y0[r] + t(alpha) * s
    assert same_bits(got, loop)
    # a NaN in x shows in the rows that reference it and in no other
    xn = x.copy()
    xn[17] = np.nan
    got, _ = check_rows_product(G, oracle, ptr, col, val, np.arange(n), xn, y0, alpha)
    touched = np.zeros(n, dtype=bool)
    touched[np.repeat(np.arange(n), widths)[col == 17]] = True
    assert touched.any() and not touched.all() and np.isnan(got[touched]).all() and np.isfinite(got[~touched]).all()
    # no rows: nothing is read, nothing written
    y = guarded(G, 8, dtype)
    fn = G.L.spmv_csr_rows_f64_i32 if dtype == np.float64 else G.L.spmv_csr_rows_f32_i32
    fn(0, None, 0, alpha, None, None, None, None, None, _p(y))
    fn(0, None, 0, alpha, None, None, None, None, None, None)
    assert np.all(y.cpu().numpy() == SENTINEL[np.dtype(dtype)])


def test_row_subset_product_takes_a_second_trip(G, oracle):
    """More listed rows than cus * 32 * 256 (one trip of the launch), 1 or 2 entries each, every second row of y listed."""
    nr = G.cus * ROWS_BLOCKS_PER_CU * BLOCK + BLOCK + 1
    n, m = 2 * nr, 1000
    widths = np.zeros(n, dtype=np.int64)
    widths[1::2] = 1 + (oracle.random_u32(21, nr) & 1)
    ptr = np.concatenate([[0], np.cumsum(widths)]).astype(np.int32)
    nnz = int(ptr[-1])
    col = oracle.random_i32(22, nnz, 0, m - 1)
    val = oracle.random_f64(23, nnz) - 0.5
    x, y0 = nonzero_hash(oracle, 24, m, np.float64), nonzero_hash(oracle, 25, n, np.float64)
    rows = np.arange(1, n, 2)
    assert len(rows) == nr > G.cus * ROWS_BLOCKS_PER_CU * BLOCK
    check_rows_product(G, oracle, ptr, col, val, rows, x, y0, 1.5)


def random_bits(oracle, seed, n, dtype):
    """Any bit pattern is a value to a gather: NaNs with payloads, infinities, denormals, both zeros."""
    words = oracle.random_u32(seed, max(1, 2 * n))
    return words[:2 * n].view(np.float64).copy() if dtype == np.float64 else words[:n].view(np.float32).copy()


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("float64", "float32"))
def test_gather(G, oracle, dtype):
    """dst[i] = src[idx[i]], bit for bit, for identity, reversed, all-same and random-with-repeats indices; sizes around a
    workgroup and one beyond a trip of the grid (cus * 16 workgroups of 256); the guard after dst survives."""
    fn = G.L.gather_f64_i32 if dtype == np.float64 else G.L.gather_f32_i32
    for n in (0, 1, BLOCK - 1, BLOCK, BLOCK + 1, G.cus * SPLIT_BLOCKS_PER_CU * BLOCK + BLOCK + 1):
        src = random_bits(oracle, 31 + n % 97, max(n, 1) + 5, dtype)
        dsrc = up(G, src)
        patterns = {"identity": np.arange(n), "reversed": np.arange(n)[::-1], "all the same": np.full(n, len(src) - 1),
                    "random with repeats": oracle.random_i32(33, max(n, 1), 0, len(src) - 1)[:n] // 2 * 2}
        for name, idx in patterns.items():
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            dst, didx = guarded(G, n, dtype), up(G, idx)
            fn(0, None, n, _p(didx), _p(dsrc), _p(dst))
            assert same_bits(payload(dst, n, "dst"), src[idx]), (n, name)
            if n in (BLOCK + 1,):                                # the wrapper the composed product uses
                assert same_bits(G.ops.gather(up(G, idx), dsrc).cpu().numpy(), src[idx])
        assert same_bits(dsrc.cpu().numpy(), src)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the composed product: every rank of a world in one process
# ---------------------------------------------------------------------------------------------------------------------------
def reference_product(oracle, S, x, y, alpha, append):
    """oracle.spmv_split (fp64); for fp32 the same five phases composed from oracle.spmv_csr on the parts."""
    if x.dtype == np.float64:
        return oracle.spmv_split(S, x, y, alpha, append)
    cpart = S["col_part"]
    for d, D in enumerate(S["devs"]):
        r0, r1 = D["rows"]
        yl = np.ascontiguousarray(y[r0:r1])
        p, c, v = D["loc"]
        if len(v):
            oracle.spmv_csr(p, c, v, np.ascontiguousarray(x[cpart[d]:cpart[d + 1]]), yl, alpha, append)
        elif not append:
            yl[:] = 0
        p, c, v = D["rem"]
        if len(v):
            oracle.spmv_csr(p, c, v, np.ascontiguousarray(x[D["ghosts"]]), yl, alpha, True)
        y[r0:r1] = yl
    return y


PRODUCT_CASES = [(name, w) for name, w in SPLIT_CASES if w > 1]


@pytest.mark.parametrize("fmt", ("auto", "csr"))
@pytest.mark.parametrize("name,world", PRODUCT_CASES, ids=["%s-world%d" % c for c in PRODUCT_CASES])
def test_product_of_all_ranks_equals_the_five_phase_apply(G, oracle, name, world, fmt):
    """Local part (ops.SpMat on the device split) + ghost values packed by their owners (ops.gather) + remote part
    (ops.RowSubsetCSR on the device split), rank by rank: the bits of oracle.spmv_split.  (Not of the unsplit product: the
    remote sum is added separately, which moves the last bit of about one row in ten.)"""
    torch, ops = G.torch, G.ops
    S, ranks = split_world(G, oracle, name, world)               # every array of the split is checked in there
    ptr, col, val, m = matrix(oracle, name)
    n, dtype = len(ptr) - 1, val.dtype
    part, cpart = S["part"], S["col_part"]
    x, y0 = nonzero_hash(oracle, 41, m, dtype), nonzero_hash(oracle, 42, n, dtype)
    dx = up(G, x)
    locs = [ops.SpMat(s.d["lptr"], s.d["lcol"], s.d["lval"], n_cols=cpart[d + 1] - cpart[d], fmt=fmt) if s.lnnz else None
            for d, s in enumerate(ranks)]
    for alpha, append in ((1.5, True), (1.0, False)):
        start = y0.copy() if append else np.full(n, np.nan, dtype=dtype)
        want = reference_product(oracle, S, x, start.copy(), alpha, append)
        ybuf = guarded(G, n, dtype)
        ybuf[:n] = up(G, start)
        for d, s in enumerate(ranks):
            if s.n == 0:
                continue
            y = ybuf[part[d]:part[d + 1]]
            if locs[d] is not None:
                locs[d].apply(dx[cpart[d]:cpart[d + 1]], y, alpha, append)
            elif not append:
                y.zero_()
            if s.nr == 0:
                continue
            pieces = []
            for o in range(world):                               # the owners pack what this rank needs, in ghost order
                mine = s.h["ghosts"][(s.h["ghosts"] >= cpart[o]) & (s.h["ghosts"] < cpart[o + 1])]
                if len(mine):
                    assert o != d
                    pieces.append(ops.gather(up(G, (mine - cpart[o]).astype(np.int32)), dx[cpart[o]:cpart[o + 1]]))
            ghost = torch.cat(pieces)
            assert ghost.numel() == s.ng
            ops.RowSubsetCSR(s.d["rem_rows"], s.d["rem_ptr"], s.d["rem_col"], s.d["rem_val"]).apply(ghost, y, alpha)
        got = payload(ybuf, n, "y")
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
        assert len(bad) == 0, (alpha, append, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
        if dtype == np.float64:
            assert same_bits(got, want)
