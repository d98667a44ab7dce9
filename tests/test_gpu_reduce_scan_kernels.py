"""Direct parity tests of the two primitives everything else rests on, called through the C ABI with torch tensors as device
buffers:

  * `vexhip_reduce`, `vexhip_reduce_dot`, `vexhip_reduce_finish` (vexcl_amd/csrc/reduce.hip: `reduce_stage1`, `reduce_stage2`);
  * `vexhip_scan` (vexcl_amd/csrc/scan.hip: `tile_sum_kernel` / `tile_scan_kernel`, the reduce-then-scan recursion, and
    `lookback_scan_kernel` in every form `vexhip_scan_set_lookback` accepts).

References: numpy on the host.  Integers are compared with `np.array_equal` on raw bits, sums and scans mod 2^k (signed types
are scanned as unsigned).  Floats are compared bit for bit as well: every float SUM, dot and scan input is integer-valued with
sum |x| below 2^24 (f32) or 2^53 (f64), so that every partial sum in every association order is exact -- each test asserts
that bound on its own input before it calls the kernel.  MIN and MAX return an element of the input, whatever the order.  The
one tolerance in this file is `test_ill_conditioned_sum`, whose bound is derived from the kernel's addition path in its
docstring.  Every output buffer (reduce `out` and `tmp`, scan `out` and `tmp`) is exactly as large as include/vexhip.h says and
ends in GUARD elements of sentinel bytes that must survive."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 16
SENTINEL_BYTE = 0xA5              # as a float: a small normal number, not a NaN

RBLOCK = 256                      # reduce.hip:15  lanes of a workgroup of either stage
RGROUPS_PER_CU = 8                # reduce.hip:161 stage1_groups(): at most 8 workgroups per CU ...
RGROUP_ELEMS = 4 * RBLOCK         # reduce.hip:165 ... and at most one per 1024 elements
SBLOCK = 256                      # scan.hip:18    lanes of a workgroup of the reduce-then-scan kernels
SK = 4                            # scan.hip:20    16-byte vectors per lane per tile; cfg<T>::TILE = SBLOCK * VN * SK (scan.hip:24)
LOOKBACK_TILES = 64               # scan.hip:355   integer scans of this many small tiles or more take the single-pass kernel
LOOKBACK_FORMS = {2: (8, 256), 3: (16, 256), 4: (16, 512), 5: (8, 1024), 6: (16, 1024), 7: (32, 256)}   # scan.hip:319 (vectors per lane, lanes)
LOOKBACK_AUTO = {4: 7, 8: 3}      # scan.hip:321   form 1 = auto: by element size
WAVE = 64                         # the look-back walk reads 64 predecessors per step (scan.hip:239-257)

SUM, SUM_KAHAN, MIN, MAX, MIN_MAX = range(5)       # include/vexhip.h, vexcl_amd/_capi.py
OPS = {"SUM": SUM, "SUM_Kahan": SUM_KAHAN, "MIN": MIN, "MAX": MAX, "MIN_MAX": MIN_MAX}


class Ty:
    def __init__(self, name, code, dtype, carrier, unsigned):
        self.name, self.code, self.np, self.carrier, self.uns = name, code, np.dtype(dtype), np.dtype(carrier), np.dtype(unsigned)
        self.size = self.np.itemsize
        self.VN = 16 // self.size                   # elements of a 16-byte load (reduce.hip:93, scan.hip:23)
        self.TILE = SBLOCK * self.VN * SK           # 4096 for 4-byte types, 2048 for 8-byte types
        self.is_float = self.np.kind == "f"
        if self.is_float:
            self.hi, self.lo = self.np.type(np.finfo(self.np).max), self.np.type(-np.finfo(self.np).max)
            self.exact = 2.0 ** (np.finfo(self.np).nmant + 1)          # 2^24, 2^53
        else:
            self.hi, self.lo = self.np.type(np.iinfo(self.np).max), self.np.type(np.iinfo(self.np).min)

    def __repr__(self):
        return self.name


# torch has no arithmetic (and old versions no tensors) of uint32 / uint64: the device buffer of a type is a tensor of its carrier
F64 = Ty("f64", 0, np.float64, np.float64, np.uint64)
F32 = Ty("f32", 1, np.float32, np.float32, np.uint32)
I32 = Ty("i32", 2, np.int32, np.int32, np.uint32)
U32 = Ty("u32", 3, np.uint32, np.int32, np.uint32)
I64 = Ty("i64", 4, np.int64, np.int64, np.uint64)
U64 = Ty("u64", 5, np.uint64, np.int64, np.uint64)
TYPES = (F64, F32, I32, U32, I64, U64)
FLOATS, INTS = (F64, F32), (I32, U32, I64, U64)
by_name = pytest.mark.parametrize("t", TYPES, ids=repr)


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def G(request):
    import torch                                        # before libvexhip.so: the process settles on torch's HIP runtime
    from vexcl_amd._capi import DeviceProps

    class NS:
        pass
    g = NS()
    g.torch, g.L, g.dev = torch, request.getfixturevalue("built_lib"), torch.device("cuda:0")
    props = DeviceProps()
    g.L.device_get_props(0, ctypes.byref(props))
    g.cus = int(props.compute_units)
    assert g.cus > 0
    g.rtmp = int(g.L.reduce_tmp_bytes())
    g.tdtype = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32,
                np.dtype(np.int64): torch.int64}
    return g


def _p(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def up(G, t, a):
    d = G.torch.from_numpy(np.ascontiguousarray(a).view(t.carrier)).to(G.dev)
    assert d.data_ptr() & 15 == 0
    return d


def down(t, d):
    return d.cpu().numpy().view(t.np)


def misaligned(G, t, a):
    """The `[1:]` view of a tensor one element longer: 4 or 8 bytes off a 16-byte boundary."""
    d = up(G, t, np.concatenate([a[:1] if len(a) else np.zeros(1, t.np), a]))[1:]
    assert d.data_ptr() & 15 != 0 and d.numel() == len(a)
    return d


def guarded(G, t, count, lead=0):
    """`lead` + `count` + GUARD elements, every byte the sentinel; returns (buffer, the view of `count` elements)."""
    fill = np.full(t.size, SENTINEL_BYTE, np.uint8).view(t.carrier)[0].item()
    buf = G.torch.full((lead + count + GUARD,), fill, dtype=G.tdtype[t.carrier], device=G.dev)
    return buf, buf[lead:lead + count]


def guard_ok(t, buf, count, what, lead=0):
    for part in (buf[:lead], buf[lead + count:]):
        assert np.all(part.cpu().numpy().view(np.uint8) == SENTINEL_BYTE), "a store outside %s" % what


def payload(t, buf, count, what, lead=0):
    guard_ok(t, buf, count, what, lead)
    return down(t, buf[lead:lead + count]).copy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def reduce(G, t, op, d, n, dot_with=None, finish=False):
    """One call of vexhip_reduce / vexhip_reduce_dot / vexhip_reduce_finish on the first n elements (finish: n partials) of d;
    `out` holds exactly the results and `tmp` exactly vexhip_reduce_tmp_bytes, each followed by the guard."""
    nout = 2 if op == MIN_MAX else 1
    out, outv = guarded(G, t, nout)
    if finish:
        G.L.reduce_finish(0, None, op, t.code, _p(d), n, _p(outv))
    else:
        tmp, tmpv = guarded(G, t, G.rtmp // t.size)
        if dot_with is None:
            G.L.reduce(0, None, op, t.code, _p(d), n, _p(outv), _p(tmpv))
        else:
            assert op == SUM
            G.L.reduce_dot(0, None, t.code, _p(d), _p(dot_with), n, _p(outv), _p(tmpv))
        guard_ok(t, tmp, G.rtmp // t.size, "the reduce tmp")
    return payload(t, out, nout, "the reduce out")


def scan(G, t, d, n, exclusive, init=None, in_place=False, out_lead=0, tmp_lead=0, want_tmp=False):
    """One call of vexhip_scan; `tmp` holds exactly vexhip_scan_tmp_bytes(dtype, n) behind `tmp_lead` elements, `out` exactly n
    behind `out_lead`, each followed by the guard.  init None = a NULL init_host."""
    nbytes = int(G.L.scan_tmp_bytes(t.code, n))
    assert nbytes % t.size == 0 and nbytes > 0
    tmp, tmpv = guarded(G, t, nbytes // t.size, tmp_lead)
    out, outv = guarded(G, t, n, out_lead)
    src = d[:n]
    if in_place:
        outv.copy_(src)
        src = outv
    host = None if init is None else np.array([init], dtype=t.np)
    G.L.scan(0, None, t.code, int(exclusive), None if host is None else ctypes.c_void_p(host.ctypes.data), _p(src), _p(outv), n, _p(tmpv))
    got = payload(t, out, n, "the scan out", out_lead)
    guard_ok(t, tmp, nbytes // t.size, "the scan tmp", tmp_lead)
    return (got, tmpv) if want_tmp else got


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and host references (no device needed: the inputs are checked on the host before a kernel sees them)
# ---------------------------------------------------------------------------------------------------------------------------
def words(oracle, seed, n):
    return oracle.random_u32(seed, max(1, n))[:n]


def any_bits(oracle, t, seed, n):
    """Integers over the whole range of the type: 64-bit values above 2^53 included."""
    assert not t.is_float
    return words(oracle, seed, n * (t.size // 4)).view(t.np).copy()


def small_ints(oracle, t, seed, n):
    """One element in four is -2, -1, 1 or 2, the others +0: sum |x| is about 0.375 n."""
    w = words(oracle, seed, n)
    return np.where((w & 3) == 0, np.array([-2, -1, 1, 2])[(w >> 2) & 3], 0).astype(t.np)


def zero_one(oracle, t, seed, n):
    """A 0/1 vector of density 1/4: sum |x| is about n / 4."""
    return ((words(oracle, seed, n) & 3) == 0).astype(t.np)


def distinct_reals(oracle, t, seed, n):
    x = ((oracle.random_f64(seed, max(1, n))[:n] - 0.5) * 1e3).astype(t.np)
    x[x == 0] = t.np.type(0.25)                      # no zeros: which of +0 and -0 a MIN returns is not asserted
    return x


def sum_input(oracle, t, seed, n):
    return small_ints(oracle, t, seed, n) if t.is_float else any_bits(oracle, t, seed, n)


def minmax_input(oracle, t, seed, n):
    return distinct_reals(oracle, t, seed, n) if t.is_float else any_bits(oracle, t, seed, n)


def assert_exact(t, *terms):
    """Integer-valued and sum of magnitudes below 2^24 / 2^53: every partial sum in any order is exact."""
    total = 0.0
    for x in terms:
        x = np.atleast_1d(np.asarray(x, dtype=np.float64))
        assert np.array_equal(x, np.rint(x))
        total += float(np.abs(x).sum())
    assert total < t.exact, (t, total)
    return total


def want_sum(t, x, y=None):
    """sum(x) or sum(x * y): exact for floats (bound asserted), mod 2^k for integers."""
    if t.is_float:
        p = x.astype(np.float64) if y is None else x.astype(np.float64) * y.astype(np.float64)
        assert_exact(t, p)
        return np.array([p.sum()], dtype=np.float64).astype(t.np)
    u = x.view(t.uns) if y is None else x.view(t.uns) * y.view(t.uns)
    return np.array([u.sum(dtype=t.uns)], dtype=t.uns).view(t.np)


def want_reduce(t, op, x):
    if op in (SUM, SUM_KAHAN):
        return want_sum(t, x)
    lo = x.min() if len(x) else t.hi                 # reductor.hpp:113-115 initial() of MIN
    hi = x.max() if len(x) else t.lo                 # reductor.hpp:89-91 initial() of MAX
    return np.array({MIN: [lo], MAX: [hi], MIN_MAX: [lo, hi]}[op], dtype=t.np)


def want_scan(t, x, exclusive, init=0, inclusive=None):
    """The prefix sums of x (`inclusive`: its precomputed inclusive scan in t.uns / float64)."""
    if t.is_float:
        assert_exact(t, x, init if exclusive else 0)
        c = np.cumsum(x, dtype=np.float64) if inclusive is None else inclusive
        if exclusive:
            c = np.concatenate([[0.0], c[:-1]]) + np.float64(init)
        return c.astype(t.np)
    c = np.cumsum(x.view(t.uns), dtype=t.uns) if inclusive is None else inclusive
    if exclusive:
        c = np.concatenate([np.zeros(1, t.uns), c[:-1]]) + np.array([init], dtype=t.np).view(t.uns)
    return c.astype(t.uns).view(t.np)


def reduce_sizes(cus, t):
    """Both sides of every edge of reduce_stage1 and of the group count min(8 CUs, ceil(n / 1024))."""
    nthreads = RGROUPS_PER_CU * cus * RBLOCK
    sat, one = RGROUPS_PER_CU * cus * RGROUP_ELEMS, nthreads * t.VN     # the group count saturates / one vector per lane
    return sorted({0, 1, t.VN - 1, t.VN, t.VN + 1, 1023, 1024, 1025, sat - 1, sat, sat + 1,
                   one - 1, one, one + 1, one + t.VN, one + t.VN + 1,         # nv = nthreads: no two-load trip; + 1: lane 0 takes one
                   2 * one - 1, 2 * one, 2 * one + 1, 2 * one + t.VN,         # a single load after the two-load trip
                   3 * one + 257 * t.VN + t.VN - 1})                          # a second two-load trip of 257 lanes, ragged, a scalar tail


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------------
# reduce
# ---------------------------------------------------------------------------------------------------------------------------
@by_name
def test_reduce_every_op_at_every_edge_size(G, oracle, t):
    """(1) SUM, SUM_Kahan (exact on exact inputs), MIN, MAX and MIN_MAX at 0, 1, around a 16-byte vector, around 1 -> 2 groups,
    around the saturation of the group count, and around every trip count of the two-load loop, the single-load loop and the
    scalar tail."""
    sizes = reduce_sizes(G.cus, t)
    xs, xm = sum_input(oracle, t, 11, sizes[-1]), minmax_input(oracle, t, 12, sizes[-1])
    if not t.is_float:
        assert (xs.view(t.uns) >> (8 * t.size - 1)).any() and xs.view(t.uns).max() > 2 ** (8 * t.size - 2)
    ds, dm = up(G, t, xs), up(G, t, xm)
    for n in sizes:
        for name, op in OPS.items():
            x, d = (xs, ds) if op in (SUM, SUM_KAHAN) else (xm, dm)
            want = want_reduce(t, op, x[:n])
            got = reduce(G, t, op, d[:n], n)
            assert same_bits(got, want), (t, name, n, got, want)
    assert same_bits(down(t, ds), xs) and same_bits(down(t, dm), xm)


def plant_size(cus, t):
    """Every lane takes the two-load trip, half of the lanes a single load after it, and VN - 1 elements are left to the tail."""
    nthreads = RGROUPS_PER_CU * cus * RBLOCK
    return nthreads, 2 * nthreads * t.VN + (nthreads // 2) * t.VN + t.VN - 1


@by_name
def test_reduce_finds_an_element_planted_anywhere(G, oracle, t):
    """(2) A unique minimum / maximum, and the one non-zero element of a sum, at: 0, 1, VN - 1, VN, the last vector of the
    first load, the first of the second load, the last full vector, the first tail element, n - 1."""
    nthreads, n = plant_size(G.cus, t)
    nv = n // t.VN
    assert nv > 2 * nthreads and nv % nthreads and n % t.VN
    at = sorted({0, 1, t.VN - 1, t.VN, nthreads * t.VN - 1, nthreads * t.VN, nv * t.VN - 1, nv * t.VN, n - 1})   # VN == 2: 7 of them
    assert max(at) == n - 1
    if t.is_float:
        base, low, high = distinct_reals(oracle, t, 21, n), t.np.type(-1e30), t.np.type(1e30)
    else:                                             # the middle half of the range
        base = ((any_bits(oracle, t, 21, n).view(t.uns) >> 2) + (t.uns.type(1) << (8 * t.size - 2))).astype(t.uns)
        base = (base if t.np == t.uns else base - (t.uns.type(1) << (8 * t.size - 1))).view(t.np)
        low, high = t.np.type(int(t.lo) + 5), t.np.type(int(t.hi) - 7)
    assert low < base.min() and base.max() < high
    d, zeros = up(G, t, base), up(G, t, np.zeros(n, t.np))
    host = base.copy()

    def poke(buf, pos, v):
        buf[pos:pos + 1].copy_(up(G, t, np.array([v], dtype=t.np)))

    for k, pos in enumerate(at):
        poke(d, pos, low)
        host[pos] = low
        assert same_bits(reduce(G, t, MIN, d, n), np.array([low])), (t, pos)
        assert same_bits(reduce(G, t, MIN_MAX, d, n), np.array([low, host.max()])), (t, pos)
        poke(d, pos, high)
        host[pos] = high
        assert same_bits(reduce(G, t, MAX, d, n), np.array([high])), (t, pos)
        assert same_bits(reduce(G, t, MIN_MAX, d, n), np.array([host.min(), high])), (t, pos)
        poke(d, pos, base[pos])
        host[pos] = base[pos]
        weight = t.np.type(3 + 2 * k)
        if t.is_float:
            assert_exact(t, weight)
        poke(zeros, pos, weight)
        for op in (SUM, SUM_KAHAN):
            assert same_bits(reduce(G, t, op, zeros, n), np.array([weight])), (t, pos, op)
        poke(zeros, pos, t.np.type(0))
    assert same_bits(down(t, d), base)


def test_reduce_i64_sum_of_40_bit_values_is_the_integer_sum(G, oracle):
    """(2) n values below 2^40 with n * 2^40 < 2^63: the sum does not wrap, so a dropped or doubled element moves it."""
    _, n = plant_size(G.cus, I64)
    assert n << 40 < 2 ** 63
    x = (any_bits(oracle, U64, 23, n) & np.uint64(2 ** 40 - 1)).view(np.int64)
    want = sum(x.tolist())                             # Python integers
    assert want == int(x.sum(dtype=np.int64)) < 2 ** 63
    d = up(G, I64, x)
    for op in (SUM, SUM_KAHAN):
        assert int(reduce(G, I64, op, d, n)[0]) == want


@by_name
def test_reduce_of_misaligned_operands_takes_the_scalar_path(G, oracle, t):
    """(3) `in` 4 / 8 bytes off a 16-byte boundary (vec_ok == 0: every lane strides by single elements), every op; the dot
    product with only a, only b and both off the boundary.  Two trips of the scalar loop and a ragged rest."""
    n = 2 * RGROUPS_PER_CU * G.cus * RBLOCK + 777
    xs, xm = sum_input(oracle, t, 31, n), minmax_input(oracle, t, 32, n)
    ds, dm = misaligned(G, t, xs), misaligned(G, t, xm)
    for name, op in OPS.items():
        x, d = (xs, ds) if op in (SUM, SUM_KAHAN) else (xm, dm)
        want = want_reduce(t, op, x)
        assert same_bits(reduce(G, t, op, d, n), want), (t, name)
    a, b = dot_inputs(oracle, t, 33, n)
    want = want_sum(t, a, b)
    al, bl = (up(G, t, a), misaligned(G, t, a)), (up(G, t, b), misaligned(G, t, b))
    for i, j in ((1, 0), (0, 1), (1, 1), (0, 0)):
        assert same_bits(reduce(G, t, SUM, al[i], n, dot_with=bl[j]), want), (t, i, j)


def dot_inputs(oracle, t, seed, n):
    """Floats: a sparse in {-2 .. 2}, b in {-3 .. 3}: every product and every partial sum is exact (want_sum asserts the
    bound).  Integers: the whole range, the product and the sum mod 2^k."""
    if not t.is_float:
        return any_bits(oracle, t, seed, n), any_bits(oracle, t, seed + 1000, n)
    return small_ints(oracle, t, seed, n), ((words(oracle, seed + 1000, n) >> 4) % 7).astype(np.int64).astype(t.np) - t.np.type(3)


@by_name
def test_reduce_dot_of_every_type(G, oracle, t):
    """(4) sum(a * b) at 0, 1, a vector and an element, two groups, the first two-load trip, and the ragged size of (1)."""
    sizes = reduce_sizes(G.cus, t)
    one = RGROUPS_PER_CU * G.cus * RBLOCK * t.VN
    a, b = dot_inputs(oracle, t, 41, sizes[-1])
    da, db = up(G, t, a), up(G, t, b)
    for n in (0, 1, t.VN + 1, 1025, one + t.VN + 1, 2 * one + t.VN, sizes[-1]):
        assert n in sizes
        want = want_sum(t, a[:n], b[:n])
        assert same_bits(reduce(G, t, SUM, da[:n], n, dot_with=db[:n]), want), (t, n)
    assert same_bits(down(t, da), a) and same_bits(down(t, db), b)


@by_name
def test_reduce_finish_folds_partials(G, oracle, t):
    """(5) vexhip_reduce_finish on 0, 1, 2, 255, 256, 257 and 2048 partials (0, 1 and several trips of a stage-2 lane).
    MIN_MAX partials are interleaved (lo, hi) pairs; the lo and the hi entries here are unrelated numbers, so a fold that mixes
    them shows.  No partials: the identity (0, `highest`, `lowest`)."""
    for nparts in (0, 1, 2, 255, 256, 257, 2048):
        for name, op in OPS.items():
            width = 2 if op == MIN_MAX else 1
            p = (sum_input if op in (SUM, SUM_KAHAN) else minmax_input)(oracle, t, 51 + op, nparts * width)
            if op == MIN_MAX:                          # every lo entry above every hi entry
                s = np.sort(p)
                p[0::2], p[1::2] = s[nparts:][::-1], s[:nparts]
                want = np.array([s[nparts], s[nparts - 1]] if nparts else [t.hi, t.lo], dtype=t.np)
                assert nparts == 0 or (want[0] == p[0::2].min() and want[1] == p[1::2].max())
            else:
                want = want_reduce(t, op, p)
            got = reduce(G, t, op, up(G, t, p) if nparts else None, nparts, finish=True)
            assert same_bits(got, want), (t, name, nparts, got, want)
        identity = {SUM: [0], SUM_KAHAN: [0], MIN: [t.hi], MAX: [t.lo], MIN_MAX: [t.hi, t.lo]}
        if nparts == 0:
            for op, v in identity.items():
                assert same_bits(reduce(G, t, op, None, 0, finish=True), np.array(v, dtype=t.np))
                assert same_bits(reduce(G, t, op, None, 0), np.array(v, dtype=t.np))


def test_reduce_geometry(G):
    groups, block = ctypes.c_int(-1), ctypes.c_int(-1)
    G.L.reduce_num_groups(0, ctypes.byref(groups), ctypes.byref(block))
    assert (groups.value, block.value) == (RGROUPS_PER_CU * G.cus, RBLOCK)
    assert RGROUPS_PER_CU * G.cus * 16 <= G.rtmp                # a MIN_MAX partial of an 8-byte type per group


@pytest.mark.parametrize("t", FLOATS, ids=repr)
def test_reduce_special_values(G, oracle, t):
    """(6) What the reference does (vexcl/reductor.hpp): MIN starts from numeric_limits::max() (:113-115), MAX from lowest()
    (:89-91), and the functors are `prm1 < prm2 ? prm1 : prm2` (:119) and `prm1 > prm2 ? prm1 : prm2` (:95) with the accumulator
    as prm1 (:527, :376, :433).  On inputs without NaN that is the same function as the `x < s ? x : s` of reduce.hip up to the
    sign of a zero: infinities are ordinary values, an empty input gives the start value, and a MAX of nothing but -inf gives
    lowest() (lowest() > -inf keeps the start value) -- in both.  With a NaN the reference's form has no answer of its own:
    `s < NaN` is false, so the NaN REPLACES the accumulator, and the next element (`NaN < x` is false too) replaces the NaN,
    dropping everything folded before it.  A lane that sees 1, NaN, 5 ends with 5; whether a NaN or a minimum survives depends on
    which lane, workgroup and fold step meets it, i.e. on the launch geometry of the device it runs on.  There is nothing
    there to reproduce, so reduce.hip keeps the one form with an order-independent answer, pinned here: a NaN never enters the
    accumulator, MIN / MAX are the minimum / maximum of the elements that are not NaN, and of nothing (all NaN) the start value.
    Which of +0.0 and -0.0 wins is not asserted (the inputs hold no zero)."""
    nan, inf = t.np.type(np.nan), t.np.type(np.inf)
    for n in (1, 5, 1025, 4 * 1024 + 3, RGROUPS_PER_CU * G.cus * RBLOCK * t.VN + t.VN + 1):
        base = distinct_reals(oracle, t, 61, n)
        cases = {"finite": base}
        for where in sorted({0, n // 2, n - 1}):
            for name, v in (("nan", nan), ("+inf", inf), ("-inf", -inf)):
                x = base.copy()
                x[where] = v
                cases["%s at %d" % (name, where)] = x
        x = base.copy()
        x[::2] = nan                                   # every second element, the last vector and the tail included
        cases["every second a nan"] = x
        x = base.copy()
        x[1::3], x[2::3] = inf, -inf
        cases["both infinities"] = x
        for name, v in (("all nan", nan), ("all +inf", inf), ("all -inf", -inf)):
            cases[name] = np.full(n, v, dtype=t.np)
        for name, x in cases.items():
            ok = x[~np.isnan(x)]                       # the start value takes part: a MAX of nothing but -inf is lowest()
            lo = min(ok.min(), t.hi) if len(ok) else t.hi
            hi = max(ok.max(), t.lo) if len(ok) else t.lo
            d = up(G, t, x)
            for d_in in (d, misaligned(G, t, x)):
                assert same_bits(reduce(G, t, MIN, d_in, n), np.array([lo])), (t, n, name)
                assert same_bits(reduce(G, t, MAX, d_in, n), np.array([hi])), (t, n, name)
                assert same_bits(reduce(G, t, MIN_MAX, d_in, n), np.array([lo, hi])), (t, n, name)
    # the fold of partials follows the same rule
    p = np.array([nan, 3, 2, nan, inf, -7, nan, nan], dtype=t.np)
    assert same_bits(reduce(G, t, MIN, up(G, t, p), 8, finish=True), np.array([-7], dtype=t.np))
    assert same_bits(reduce(G, t, MAX, up(G, t, p), 8, finish=True), np.array([inf], dtype=t.np))
    assert same_bits(reduce(G, t, MIN_MAX, up(G, t, p), 4, finish=True), np.array([2, 3], dtype=t.np))     # lo of (nan, 2, inf, nan), hi of (3, nan, -7, nan)


@pytest.mark.parametrize("t", FLOATS, ids=repr)
def test_ill_conditioned_sum(G, oracle, t):
    """The one tolerance of this file: SUM and SUM_Kahan of (U - 0.5) * 1e8 (vector_arithmetics.cpp:72-96) against math.fsum,
    which is the correctly rounded sum of the stored values (for f64 oracle.sum_kahan must agree with it to Kahan's 2 u S1).

    u = 2^-53 (f64), 2^-24 (f32); S1 = sum |x|.  Every partial sum is at most S1 in magnitude, so one rounded addition
    contributes at most u S1.  The path of an element through reduce.hip:
      * stage 1, per lane: m additions, m = VN * ceil(nv / nthreads) + 1 (its vectors and at most one tail element), nv = n / VN,
        nthreads = groups * 256.  SUM: m u S1.  SUM_Kahan: the compensated recurrence, 2 u S1 whatever m (Kahan / Goldberg,
        (2 u + O(m u^2)) S1);
      * the fold of a workgroup (block_fold): 6 shuffle steps and RWAVES - 1 = 3 LDS merges: 9 u S1;
      * stage 2: ceil(groups / 256) merges per lane, then the same fold: (ceil(groups / 256) + 9) u S1.
    Bound: (m + F) u S1 for SUM and (2 + F) u S1 for SUM_Kahan, F = 18 + ceil(groups / 256), both times (1 + 1e-3) for the
    second-order terms ((m + F)^2 u^2 < 1e-3 u), plus u |S| for the reference's own rounding.  Nothing here was fitted to what
    the kernel returns."""
    n = (1 << 20) + 3
    x = ((oracle.random_f64(n, n) - 0.5) * 1e8).astype(t.np)
    exact = math.fsum(float(v) for v in x)
    u = 1.0 / t.exact
    assert u == (2.0 ** -53 if t is F64 else 2.0 ** -24)
    s1 = math.fsum(abs(float(v)) for v in x)
    if t is F64:
        assert abs(oracle.sum_kahan(x) - exact) <= 2 * u * s1
    groups = min(RGROUPS_PER_CU * G.cus, (n + RGROUP_ELEMS - 1) // RGROUP_ELEMS)
    nthreads, nv = groups * RBLOCK, n // t.VN
    m = {"vector": t.VN * ((nv + nthreads - 1) // nthreads) + 1, "scalar": (n + nthreads - 1) // nthreads}
    F = 18 + (groups + RBLOCK - 1) // RBLOCK
    assert (m["vector"] + F) ** 2 * u < 1e-3
    operands = {"vector": up(G, t, x), "scalar": misaligned(G, t, x)}     # misaligned: a lane adds ceil(n / nthreads) single elements
    for name, op in (("SUM", SUM), ("SUM_Kahan", SUM_KAHAN)):
        for path, d_in in operands.items():
            bound = ((m[path] if op == SUM else 2) + F) * u * s1 * (1 + 1e-3) + u * abs(exact)
            got = float(reduce(G, t, op, d_in, n)[0])
            print("%s %s n=%d: |error| = %.3e, bound = %.3e" % (t, name, n, abs(got - exact), bound))
            assert abs(got - exact) <= bound, (t, name, got, exact, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# scan
# ---------------------------------------------------------------------------------------------------------------------------
def scan_input(oracle, t, seed, n):
    return small_ints(oracle, t, seed, n) if t.is_float else any_bits(oracle, t, seed, n)


def wrap_init(t):
    return t.np.type(-3) if t.np.kind == "i" else t.np.type(int(t.hi) - 2)       # 2^k - 3 as bits: the first sums wrap


@by_name
def test_scan_every_type_and_placement(G, oracle, t):
    """(7) Inclusive and exclusive, out of place and in place, around a 16-byte vector, around one tile, three tiles, and on
    both sides of the 64 small tiles from which integers take the look-back kernel (floats: reduce-then-scan throughout).
    Exclusive: init 0, small, one that wraps the running sum (integers) / a larger one (floats), and a NULL init_host (= 0);
    inclusive: a non-NULL init_host is ignored."""
    sizes = sorted({1, t.VN - 1, t.VN + 1, t.TILE - 1, t.TILE, t.TILE + 1, 2 * t.TILE + 3,
                    (LOOKBACK_TILES - 1) * t.TILE, (LOOKBACK_TILES - 1) * t.TILE + 1, LOOKBACK_TILES * t.TILE + 5})
    base = scan_input(oracle, t, 71, sizes[-1])
    d = up(G, t, base)
    inits = [t.np.type(0), t.np.type(7), t.np.type(1000) if t.is_float else wrap_init(t)]
    for n in sizes:
        x = base[:n]
        inc = np.cumsum(x, dtype=np.float64) if t.is_float else np.cumsum(x.view(t.uns), dtype=t.uns)
        for in_place in (False, True):
            where = (t, n, in_place)
            want = want_scan(t, x, False, inclusive=inc)
            assert same_bits(scan(G, t, d, n, False, None, in_place), want), where
            assert same_bits(scan(G, t, d, n, False, t.np.type(7), in_place), want), where
            assert same_bits(scan(G, t, d, n, True, None, in_place), want_scan(t, x, True, 0, inclusive=inc)), where
            for init in inits:
                assert same_bits(scan(G, t, d, n, True, init, in_place), want_scan(t, x, True, init, inclusive=inc)), where + (init,)
    assert same_bits(down(t, d), base)


FORM_CASES = [(t, form) for t in (U32, U64) for form in (1, 2, 3, 4, 5, 6, 7)]


def lookback_data(G, oracle, t):
    """The longest input of (8), its device copy and its inclusive scan, made once per type."""
    def make():
        n = 100 * max(v * b for v, b in LOOKBACK_FORMS.values()) * t.VN + 3
        x = any_bits(oracle, t, 81, n)
        return x, up(G, t, x), np.cumsum(x.view(t.uns), dtype=t.uns)
    return cached(("lookback", t.name), make)


@pytest.mark.parametrize("t,form", FORM_CASES, ids=["%s-form%d" % c for c in FORM_CASES])
def test_scan_every_lookback_form(G, oracle, t, form):
    """(8) Every form of the single-pass kernel against the host prefix sum and against form 0 (reduce-then-scan) on the same
    input, inclusive and exclusive.  Sizes: one tile of the form -1 / +0 / +1 and 5 tiles + 17 (below 64 SMALL tiles these
    still take reduce-then-scan, whatever the form: asserted through the ticket word), 64 small tiles -1 / +0 / +1 (the first
    sizes of the look-back kernel; they end in a tile short of one element, a full tile, and a tile of one element), and
    100 tiles + 3: more than 64 predecessors, so the walk's second window (`base -= kWave`) is reachable -- whether a tile
    walks that far depends on how far its predecessors have got when it looks, which a test cannot force.
    The ticket word ws[0] counts the workgroups that took a tile: it tells which kernel ran.  `tmp` is exactly
    vexhip_scan_tmp_bytes and guarded, which checks the extent of the hipMemsetAsync for every form."""
    vectors, lanes = LOOKBACK_FORMS[LOOKBACK_AUTO[t.size] if form == 1 else form]
    tile = vectors * lanes * t.VN
    base, d, inc = lookback_data(G, oracle, t)
    edge = LOOKBACK_TILES * t.TILE
    assert edge % tile == 0
    sizes = sorted({tile - 1, tile, tile + 1, 5 * tile + 17, edge - 1, edge, edge + 1, 100 * tile + 3})
    assert sizes[-1] <= len(base) and 100 * tile + 3 > (WAVE + 1) * tile
    init = wrap_init(t)
    try:
        for n in sizes:
            want = (want_scan(t, base[:n], False, inclusive=inc[:n]), want_scan(t, base[:n], True, init, inclusive=inc[:n]))
            G.L.scan_set_lookback(0)
            for exclusive in (False, True):
                assert same_bits(scan(G, t, d, n, exclusive, init), want[exclusive]), (t, "form 0", n, exclusive)
            G.L.scan_set_lookback(form)
            for exclusive in (False, True):
                for in_place in (False, True):
                    got, tmp = scan(G, t, d, n, exclusive, init, in_place, want_tmp=True)
                    assert same_bits(got, want[exclusive]), (t, form, n, exclusive, in_place)
                    ticket = int(tmp[:8 // t.size].cpu().numpy().view(np.uint64)[0])
                    if (n + t.TILE - 1) // t.TILE >= LOOKBACK_TILES:
                        assert ticket == (n + tile - 1) // tile, (t, form, n, ticket)       # every tile of this form was taken once
                    else:
                        assert ticket != (n + tile - 1) // tile, (t, form, n, ticket)       # not the look-back kernel
    finally:
        G.L.scan_set_lookback(1)
    assert same_bits(down(t, d), base)


@pytest.mark.parametrize("t,n", ((F64, 2048 ** 2 + 2049), (F32, 4096 ** 2 + 4097)), ids=("f64", "f32"))
def test_scan_three_levels_of_reduce_then_scan(G, oracle, t, n):
    """(9) More than TILE^2 elements: the tile sums need a scan of more than one tile of tile sums.  A 0/1 vector of density
    1/4 (sum about n / 4 < 2^24): the float32 prefix sums are exact, asserted against a float64 and a float32 host scan."""
    assert n > t.TILE ** 2 and t.TILE in (2048, 4096)
    x = zero_one(oracle, t, 91, n)
    init = t.np.type(1000)
    assert assert_exact(t, x, init) > n / 5
    inc = np.cumsum(x, dtype=np.float64)
    assert same_bits(np.cumsum(x, dtype=t.np), inc.astype(t.np))          # the host reference alone: exact in either precision
    d = up(G, t, x)
    assert same_bits(scan(G, t, d, n, False), want_scan(t, x, False, inclusive=inc))
    assert same_bits(scan(G, t, d, n, True, init), want_scan(t, x, True, init, inclusive=inc))
    assert same_bits(down(t, d), x)


@by_name
def test_scan_of_misaligned_operands(G, oracle, t):
    """(10) `in`, `out` or both 4 / 8 bytes off a 16-byte boundary: load_vec / store_vec go element by element.  Integers at
    64 tiles + 5 (the look-back kernel) and 3 tiles + 1 (reduce-then-scan), floats at 3 tiles + 1."""
    sizes = (3 * t.TILE + 1,) if t.is_float else (3 * t.TILE + 1, LOOKBACK_TILES * t.TILE + 5)
    x = scan_input(oracle, t, 101, sizes[-1])
    init = t.np.type(7)
    operands = (up(G, t, x), misaligned(G, t, x))
    for n in sizes:
        inc = np.cumsum(x[:n], dtype=np.float64) if t.is_float else np.cumsum(x[:n].view(t.uns), dtype=t.uns)
        want = (want_scan(t, x[:n], False, inclusive=inc), want_scan(t, x[:n], True, init, inclusive=inc))
        for mis_in, mis_out in ((1, 0), (0, 1), (1, 1)):
            for exclusive in (False, True):
                got = scan(G, t, operands[mis_in], n, exclusive, init, out_lead=mis_out)
                assert same_bits(got, want[exclusive]), (t, n, mis_in, mis_out, exclusive)
    assert same_bits(down(t, operands[1]), x)


def test_scan_u32_with_tmp_off_by_four_bytes(G, oracle):
    """(10) The status words of the look-back kernel are 8-byte atomics: a tmp that is not 8-byte aligned silently takes
    reduce-then-scan (scan.hip:355) and must give the same answer, inside the same vexhip_scan_tmp_bytes."""
    t, n = U32, LOOKBACK_TILES * U32.TILE + 5
    x = any_bits(oracle, t, 103, n)
    d = up(G, t, x)
    for exclusive in (False, True):
        got, tmp = scan(G, t, d, n, exclusive, t.np.type(7), tmp_lead=1, want_tmp=True)
        assert tmp.data_ptr() & 7 == 4
        assert same_bits(got, want_scan(t, x, exclusive, t.np.type(7))), exclusive


def test_float_scan_is_deterministic(G, oracle):
    """(11) The same ill-conditioned f64 input scanned five times: identical bits (floats never take the look-back kernel,
    whose association order depends on timing)."""
    n = 70 * F64.TILE + 5
    x = (oracle.random_f64(111, n) - 0.5) * 1e8
    d = up(G, F64, x)
    first = scan(G, F64, d, n, False)
    for rep in range(4):
        assert same_bits(scan(G, F64, d, n, False), first), rep
