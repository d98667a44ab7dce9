"""Direct parity tests of the stencil convolution, `vexhip_stencil_conv_f64/_f32` (vexcl_amd/csrc/stencil.hip), called
through the C ABI: the LDS kernel (interior tiles with aligned 16-byte loads, edge tiles through `read_x`, vector and scalar
stores) and the direct-read kernel of stencils wider than LDS, in double and in float.

Reference, from the contract in include/vexhip.h:  out[i] = beta*y[i] + alpha * sum_j s[j] * X(i + j - lhalo), where X is x
padded with the halo buffer where has_left / has_right is set and with the edge element otherwise, evaluated over
`sliding_window_view`.  stencil.hip allows FMA contraction, so order and rounding of the sum are not pinned; hence

* EXACT inputs (the bulk): s in [-3, 3], x / xrem / y0 in [-7, 7], alpha in {1, 3, 0.5}, beta in {0, 1, -2}, all integers but
  alpha = 0.5.  Every partial sum is an integer below 9000 * 21 * 3 + 14 < 2^24: exact in float and double in any order, with
  or without FMA (alpha = 0.5 gives half-integers, still exact).  Compared with `np.array_equal`.
* REAL inputs (widths <= 64): reference in np.longdouble, bound  |got - ref| <= g * (|alpha| * sum_j |s[j] X_j| + |beta y0[i]|),
  g = k u / (1 - k u), k = width + 3, u = 2^-53 or 2^-24 -- the standard bound of a recursive sum of `width` products plus the
  two scalings; derived, not measured.  A one-tap error is orders of magnitude above it.

The padded-window reference itself is pinned by a loop that restates `read_x` (CPU)."""
import ctypes

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

DTYPES = (np.float64, np.float32)
GEOMETRIES = ((0, 0), (1, 1), (0, 16), (16, 0), (10, 10), (23, 40), (7, 8))     # (lhalo, rhalo); (7, 8) and (10, 10): odd and even lhalo
SIZES = (1, 2, 3, 5, 1023, 1024, 1025, 4099, 3 * 1024 + 500, 1 << 20)
HALOS = ((0, 0), (1, 0), (0, 1), (1, 1))                                         # (has_left, has_right)
ALPHAS, BETAS = (1.0, 3.0, 0.5), (0.0, 1.0, -2.0)
SCALINGS = tuple((a, b) for a in ALPHAS for b in BETAS)
DIAGONAL = ((1.0, 0.0), (3.0, 1.0), (0.5, -2.0))
CTILE, CI = 1024, 4                                                              # stencil.hip: outputs per workgroup / per lane

every_dtype = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
every_geometry = pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "l%d_r%d" % g)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
def padded(x, xrem, lhalo, rhalo, has_left, has_right):
    """X(-lhalo) ... X(n - 1 + rhalo): the halo buffer holds lhalo values of the left neighbour, then rhalo of the right one."""
    left = xrem[:lhalo] if has_left else np.full(lhalo, x[0], dtype=x.dtype)
    right = xrem[lhalo:lhalo + rhalo] if has_right else np.full(rhalo, x[-1], dtype=x.dtype)
    return np.concatenate([left, x, right])


def window_sums(s, X, acc):
    """sum_j s[j] * X[i + j] for every i, in the arithmetic of `acc`, over the sliding windows (in slabs of rows: a product
    with the whole view would copy n * width elements)."""
    width = len(s)
    W = sliding_window_view(X.astype(acc), width)
    sa = s.astype(acc)
    out = np.empty(W.shape[0], dtype=acc)
    step = max(1, (1 << 22) // width)
    for r in range(0, W.shape[0], step):
        out[r:r + step] = W[r:r + step] @ sa
    return out


def reference_exact(s, x, xrem, y0, lhalo, rhalo, has_left, has_right, alpha, beta, conv=None):
    """For integer inputs: every operation below is exact in float64."""
    if conv is None:
        conv = window_sums(s, padded(x, xrem, lhalo, rhalo, has_left, has_right), np.float64)
    assert np.all(np.abs(conv) * 3 + 14 < 2 ** 24)
    return alpha * conv + (beta * y0.astype(np.float64) if beta != 0 else 0.0)


def read_x_loop(s, x, xrem, y0, lhalo, rhalo, has_left, has_right, alpha, beta):
    """The contract restated as a loop: `read_x` of the header comment, indices clamped to [0, n - 1] without a neighbour."""
    n = len(x)
    out = np.empty(n, dtype=np.float64)
    for i in range(n):
        acc = 0.0
        for j in range(lhalo + rhalo + 1):
            g = i + j - lhalo
            if 0 <= g < n:
                v = x[g]
            elif g < 0:
                v = xrem[lhalo + g] if has_left else x[max(0, min(n - 1, g))]
            else:
                v = xrem[lhalo + (g - n)] if has_right else x[max(0, min(n - 1, g))]
            acc += float(s[j]) * float(v)
        out[i] = alpha * acc + (beta * float(y0[i]) if beta != 0 else 0.0)
    return out


def exact_inputs(oracle, n, lhalo, rhalo, seed=0):
    """Integers: s in [-3, 3]; x, xrem, y0 in [-7, 7]; no halo value equals the edge element it stands in for."""
    width = lhalo + rhalo + 1
    key = 1000003 * n + 1009 * lhalo + rhalo + 7919 * seed
    s = oracle.random_i32(key + 1, width, -3, 3)
    x = oracle.random_i32(key + 2, n, -7, 7)
    y0 = oracle.random_i32(key + 3, n, -7, 7)
    xrem = oracle.random_i32(key + 4, width - 1, -7, 7)
    for part, edge in ((slice(0, lhalo), int(x[0])), (slice(lhalo, lhalo + rhalo), int(x[-1]))):
        xrem[part] = np.where(xrem[part] == edge, edge + 3 if edge + 3 <= 7 else edge - 3, xrem[part])
    return s, x, xrem, y0


def real_inputs(oracle, n, lhalo, rhalo, dtype):
    width = lhalo + rhalo + 1
    key = 2000003 * n + 1013 * lhalo + rhalo
    s = (oracle.random_f64(key + 1, width) - 0.5).astype(dtype)
    x = oracle.random_f64(key + 2, n).astype(dtype)
    y0 = (oracle.random_f64(key + 3, n) - 0.5).astype(dtype)
    xrem = (oracle.random_f64(key + 4, max(1, width - 1))[:width - 1] + 1.0).astype(dtype)
    return s, x, xrem, y0


def test_padded_window_reference_equals_the_read_x_loop(oracle):
    """Pins the reference of this file without a GPU, on sizes that include n < lhalo and n < rhalo."""
    for n, lhalo, rhalo in ((1, 0, 0), (1, 2, 3), (2, 5, 1), (3, 1, 6), (7, 3, 3), (40, 23, 40), (40, 37, 5), (19, 0, 16), (19, 16, 0)):
        s, x, xrem, y0 = exact_inputs(oracle, n, lhalo, rhalo)
        assert len(xrem) == lhalo + rhalo and s.min() >= -3 and s.max() <= 3 and np.abs(x).max() <= 7
        for has_left, has_right in HALOS:
            if has_left and lhalo:
                assert np.all(xrem[:lhalo] != x[0])
            if has_right and rhalo:
                assert np.all(xrem[lhalo:] != x[-1])
            for alpha, beta in DIAGONAL + ((1.0, -2.0),):
                want = read_x_loop(s, x, xrem, y0, lhalo, rhalo, has_left, has_right, alpha, beta)
                got = reference_exact(s, x, xrem, y0, lhalo, rhalo, has_left, has_right, alpha, beta)
                assert np.array_equal(got, want), (n, lhalo, rhalo, has_left, has_right, alpha, beta)
                wide = window_sums(s, padded(x, xrem, lhalo, rhalo, has_left, has_right), np.longdouble)
                assert np.array_equal((alpha * wide + (beta * y0 if beta != 0 else 0)).astype(np.float64), want)


def lds_bytes(dtype, lhalo, rhalo):
    """stencil.hip `lds_elems`: the kernel stages in LDS when this is at most 64 KiB, else every lane reads x directly."""
    span = CTILE + lhalo + rhalo + CI
    return np.dtype(dtype).itemsize * ((lhalo + rhalo + 1) + span + span // 16 + 2)


def test_widths_lie_on_both_sides_of_the_lds_threshold():
    kib64 = 64 * 1024
    assert lds_bytes(np.float64, 1500, 1499) <= kib64 < lds_bytes(np.float64, 2000, 1999)
    assert lds_bytes(np.float32, 3500, 3499) <= kib64 < lds_bytes(np.float32, 4000, 3999)
    assert lds_bytes(np.float64, 4500, 4499) > kib64 and lds_bytes(np.float32, 4500, 4499) > kib64
    assert all(lds_bytes(np.float64, l, r) <= kib64 for l, r in GEOMETRIES)


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


Y_GUARD = 12345.0


def convolve(G, dtype, s, x, xrem, y_init, lhalo, rhalo, has_left, has_right, alpha, beta, x_off=0, y_off=0):
    """One call.  x, s and the halo buffer are surrounded by NaN, and so is the half of the halo buffer that has no neighbour
    (it must not be read); y is surrounded by a guard value that must survive.  xrem is NULL without a neighbour.  x_off /
    y_off = 1 move the view one element past a 16-byte boundary."""
    torch = G.torch
    n = len(x)

    item = np.dtype(dtype).itemsize

    def framed(a, off, fill):
        """The buffer on the device and the address of a inside it (base + offset: an empty view of a torch tensor, the halo
        buffer of a one-point stencil, reports address 0, and the library rightly refuses a NULL halo buffer with a neighbour)."""
        buf = np.full(len(a) + 6, fill, dtype=dtype)
        buf[off:off + len(a)] = a
        t = torch.from_numpy(buf).to(G.dev)
        assert t.data_ptr() % 16 == 0
        return t, t.data_ptr() + off * item

    xbuf, px = framed(x, 2 + x_off, np.nan)
    sbuf, ps = framed(s, 2, np.nan)
    assert (px % (2 * item) != 0) == bool(x_off)
    rbuf, prem = None, None
    if has_left or has_right:
        h = np.asarray(xrem, dtype=dtype).copy()
        if not has_left:
            h[:lhalo] = np.nan
        if not has_right:
            h[lhalo:] = np.nan
        rbuf, prem = framed(h, 2, np.nan)
    ybuf, py = framed(y_init, 2 + y_off, Y_GUARD)
    assert (py % (2 * item) != 0) == bool(y_off)
    fn = G.L.stencil_conv_f64 if dtype == np.float64 else G.L.stencil_conv_f32
    vp = ctypes.c_void_p
    fn(0, None, n, int(has_left), int(has_right), lhalo, rhalo, vp(ps), vp(px), None if prem is None else vp(prem), vp(py),
       beta, alpha)
    out = ybuf.cpu().numpy()
    o = 2 + y_off
    assert np.all(out[:o] == Y_GUARD) and np.all(out[o + n:] == Y_GUARD), "a store outside y"
    return out[o:o + n].copy()


def first_difference(got, want):
    bad = np.flatnonzero(~(got == want))
    return "no difference" if len(bad) == 0 else "first differing index %d of %d (%d differ): got %r, want %r" % (
        bad[0], len(got), len(bad), got[bad[0]], want[bad[0]])


def check_exact(G, oracle, dtype, n, lhalo, rhalo, halos=HALOS, scalings=SCALINGS, x_off=0, y_off=0, seed=0):
    """Integer inputs against the exact reference; with beta = 0, y starts as NaN (a set must not read y).  Returns the
    results in call order."""
    s, x, xrem, y0 = exact_inputs(oracle, n, lhalo, rhalo, seed)
    results = []
    for has_left, has_right in halos:
        conv = window_sums(s, padded(x, xrem, lhalo, rhalo, has_left, has_right), np.float64)
        for alpha, beta in scalings:
            want = reference_exact(s, x, xrem, y0, lhalo, rhalo, has_left, has_right, alpha, beta, conv).astype(dtype)
            y_init = y0.astype(dtype) if beta != 0 else np.full(n, np.nan, dtype=dtype)
            got = convolve(G, dtype, s.astype(dtype), x.astype(dtype), xrem.astype(dtype), y_init, lhalo, rhalo,
                           has_left, has_right, alpha, beta, x_off, y_off)
            assert np.array_equal(got, want), (np.dtype(dtype).name, n, lhalo, rhalo, has_left, has_right, alpha, beta, x_off, y_off,
                                               first_difference(got, want))
            results.append(got)
    return results


def sizes_for(lhalo, rhalo):
    """SIZES plus sizes below either halo."""
    extra = {h - 1 for h in (lhalo, rhalo) if h > 1} | {h // 2 for h in (lhalo, rhalo) if h > 3}
    return tuple(sorted(set(SIZES) | extra))


def has_interior_tile(n, lhalo, rhalo):
    """stencil.hip: a tile whose inputs all lie in the local segment takes the aligned 16-byte loads."""
    span = CTILE + lhalo + rhalo
    for g0 in range(0, n, CTILE):
        first = g0 - lhalo
        if first >= 1 and (first & ~1) + 2 * ((span + CI + 2) // 2) <= n:
            return True
    return False


@pytest.mark.gpu
@every_geometry
@every_dtype
def test_exact_inputs_every_size_and_halo(G, oracle, dtype, geometry):
    """Every size (one lane, tiles that end one short of / at / one past 1024, ragged last tiles, interior tiles, segments
    shorter than a halo) x all four (has_left, has_right) x every (alpha, beta); the largest size with three scalings."""
    lhalo, rhalo = geometry
    assert all(has_interior_tile(n, lhalo, rhalo) for n in (4099, 3 * 1024 + 500, 1 << 20))
    assert not has_interior_tile(1025, lhalo, rhalo)
    for n in sizes_for(lhalo, rhalo):
        check_exact(G, oracle, dtype, n, lhalo, rhalo, scalings=DIAGONAL if n >= (1 << 20) else SCALINGS)
    if lhalo > 1 or rhalo > 1:
        assert min(sizes_for(lhalo, rhalo)) < max(lhalo, rhalo)


WIDE = ((3000, 1500), (4000, 2000), (7000, 3500), (8000, 4000), (9000, 4500))     # (width, centre)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", WIDE, ids=lambda w: "width%d" % w[0])
@every_dtype
def test_exact_inputs_on_both_sides_of_the_lds_threshold(G, oracle, dtype, wide):
    """Widths 3000 / 4000 straddle the 64 KiB of LDS for double, 7000 / 8000 for float, 9000 (centre 4500) is direct-read for
    both: the staged kernel at its largest and the kernel in which every lane reads x through `read_x`.  Segments of 5 and
    2500 points are shorter than either halo."""
    width, centre = wide
    lhalo, rhalo = centre, width - 1 - centre
    staged = lds_bytes(dtype, lhalo, rhalo) <= 64 * 1024
    assert staged == (width <= (3000 if dtype == np.float64 else 7000))
    for n in (5, 2500):
        check_exact(G, oracle, dtype, n, lhalo, rhalo, scalings=DIAGONAL)


@pytest.mark.gpu
@every_geometry
@every_dtype
def test_real_inputs_within_the_derived_bound(G, oracle, dtype, geometry):
    """Nothing depends on integer data: oracle.random_f64 values (cast for float) against the np.longdouble reference, within
    g * (|alpha| * sum_j |s[j] X_j| + |beta y0[i]|), g = k u / (1 - k u), k = width + 3."""
    lhalo, rhalo = geometry
    width = lhalo + rhalo + 1
    assert width <= 64 and np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    u = np.longdouble(2.0) ** (-53 if dtype == np.float64 else -24)
    gamma = (width + 3) * u / (1 - (width + 3) * u)
    for n in (5, 1023, 1025, 3 * 1024 + 500, 4099):
        s, x, xrem, y0 = real_inputs(oracle, n, lhalo, rhalo, dtype)
        for has_left, has_right in HALOS:
            X = padded(x, xrem, lhalo, rhalo, has_left, has_right)
            conv = window_sums(s, X, np.longdouble)
            scale = window_sums(np.abs(s), np.abs(X), np.longdouble)
            for alpha, beta in DIAGONAL + ((1.0, -2.0),):
                ref = alpha * conv + (beta * y0.astype(np.longdouble) if beta != 0 else 0)
                bound = gamma * (abs(alpha) * scale + abs(beta) * np.abs(y0.astype(np.longdouble)))
                y_init = y0 if beta != 0 else np.full(n, np.nan, dtype=dtype)
                got = convolve(G, dtype, s, x, xrem, y_init, lhalo, rhalo, has_left, has_right, alpha, beta)
                err = np.abs(got.astype(np.longdouble) - ref)
                worst = int(np.argmax(err - bound))
                assert np.all(err <= bound), (np.dtype(dtype).name, n, lhalo, rhalo, has_left, has_right, alpha, beta,
                                              "index %d: error %g, bound %g" % (worst, err[worst], bound[worst]))


@pytest.mark.gpu
@every_dtype
def test_beta_zero_ignores_what_y_held(G, oracle, dtype):
    """beta == 0 is a set: y prefilled with NaN comes back without one, on the vector store path (y aligned, n % 4 == 0) and on
    the scalar one (y moved by one element; n % 4 != 0), staged and direct-read."""
    for n, lhalo, rhalo in ((4096, 10, 10), (4098, 10, 10), (1024, 7, 8), (700, 2000, 1999)):
        for y_off in (0, 1):
            for got in check_exact(G, oracle, dtype, n, lhalo, rhalo, scalings=((1.0, 0.0), (0.5, 0.0)), y_off=y_off):
                assert not np.isnan(got).any()


@pytest.mark.gpu
@every_dtype
def test_beta_nonzero_on_the_vector_and_the_scalar_store_path(G, oracle, dtype):
    """beta != 0 reads y: through 16-byte pairs when y is aligned and the lane's four outputs exist, else element by element
    (y moved by one element; the last lanes of n % 4 != 0).  Both give the exact result, so the same bits; with halos."""
    for n in (4096, 4098, 1027):
        for lhalo, rhalo in ((10, 10), (7, 8)):
            scalings = tuple((a, b) for a in ALPHAS for b in BETAS if b != 0)
            aligned = check_exact(G, oracle, dtype, n, lhalo, rhalo, scalings=scalings)
            moved = check_exact(G, oracle, dtype, n, lhalo, rhalo, scalings=scalings, y_off=1)
            assert all(np.array_equal(a, b) for a, b in zip(aligned, moved))


@pytest.mark.gpu
@every_dtype
def test_x_moved_by_one_element_gives_the_same_bits(G, oracle, dtype):
    """An x that is not 16-byte aligned fails the alignment test of the interior load: those tiles are staged through `read_x`
    instead.  Same LDS contents, same arithmetic: the bits of the aligned run, for integer and for real-valued inputs."""
    for n in (4099, 3 * 1024 + 500, 8192):
        for lhalo, rhalo in ((10, 10), (7, 8), (23, 40)):
            assert has_interior_tile(n, lhalo, rhalo)
            aligned = check_exact(G, oracle, dtype, n, lhalo, rhalo, scalings=DIAGONAL)
            moved = check_exact(G, oracle, dtype, n, lhalo, rhalo, scalings=DIAGONAL, x_off=1)
            assert all(np.array_equal(a, b) for a, b in zip(aligned, moved))
            s, x, xrem, y0 = real_inputs(oracle, n, lhalo, rhalo, dtype)
            for has_left, has_right in HALOS:
                a = convolve(G, dtype, s, x, xrem, y0, lhalo, rhalo, has_left, has_right, 0.5, -2.0)
                b = convolve(G, dtype, s, x, xrem, y0, lhalo, rhalo, has_left, has_right, 0.5, -2.0, x_off=1)
                assert np.array_equal(a, b), (n, lhalo, rhalo, has_left, has_right, first_difference(b, a))
