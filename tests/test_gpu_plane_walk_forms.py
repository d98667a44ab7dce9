"""The two walks of the fp64 plane product with tiles of two lines (vexcl_amd/csrc/plane.hip): `plane_walk`, selected by
VEXHIP_PLANE_WALK=0, and `plane_walk_ahead`, selected by 1 or by nothing -- the walk that requests the classes of its lines a group
of four planes ahead through scalar loads, its first x requests before its tables, and decodes the first plane's class before the
first look.  Every case runs under both through the C ABI on a plan filled by hand (the machinery of test_gpu_plane_grid_kernels.py:
matrices by grid line, canaries in x, sentinels around y, guarded tables) and must give the bits of `oracle.spmv_csr` and of the
other walk.

What is placed on purpose
  * walks that end 1 plane before, at and after a multiple of 64 planes (63 .. 130 planes, whole and cut at 64 and 65), so that every
    residue of (planes mod 4) and the look past the last plane occur;
  * walks of 1 .. 9 planes cut at 1, 4 and not at all (no group of four fits / exactly one / one and a rest);
  * a line whose class changes exactly at the planes 63, 64, 65 and 128; a third class in the middle of a run of groups (a slow step, a
    decode, fast steps again); a plan whose hot class no line uses; a single class; a first plane whose two lines differ;
  * a ragged last plane (1 and 3 lines), x longer than y (1 and 5 lines);
  * the addend forms: none, y itself ('+='), another array, x itself (the last two through `vexhip_spmat_apply_axpby_f64` on a
    matrix the library stored itself).

The host model
  `ahead_walk` restates plane_walk_ahead for one workgroup: which planes take fast steps, which slow ones, every class word it reads
  and every decode.  Before any launch `ahead_requests_inside` shows with it that every request and every store of the new walk lies
  inside x, y and the class array (the fast steps address x and y through buffer resources without a range check); the checks of
  test_gpu_plane_grid_kernels.py (`visit_once`, `addresses_inside`) cover the launch and the other walk.  The model is pinned by
  test_host_model_of_the_walk, which needs no GPU: a walk reads every class word of its planes once, plus the look four planes past
  its end (clamped to the last line), and the benchmark's operator takes no slow step before the planes that `zh` excludes."""
import collections
import os

import numpy as np
import pytest

import test_gpu_plane_grid_kernels as K
from test_gpu_plane_grid_kernels import G          # noqa: F401 -- the module-scoped device fixture

gpu = pytest.mark.gpu
PL, ABSENT = K.PL, K.ABSENT
WALKS = (0, 1)

# a line's seven value codes by class of the palette: every position / the centre alone / another centre / no +-P
PALETTE = (K.BAND, (ABSENT, ABSENT, ABSENT, 4, ABSENT, ABSENT, ABSENT), K.BAND[:3] + (9,) + K.BAND[4:], (ABSENT,) + K.BAND[1:3] + (0,) + K.BAND[4:6] + (ABSENT,))


def _changes(z, y):        # line 1 changes class exactly at the planes 63, 64, 65 and 128
    return 2 if (y == 1 and (z == 63 or 65 <= z < 128)) else 0


def _third(z, y):          # planes 8 .. 15 and 30 .. of line 0 use a second class, plane 21 a third one in the middle of a run
    return 3 if (y == 0 and z == 21) else 2 if (y == 0 and (8 <= z < 16 or z >= 30)) else 0


def _halves(z, y):         # two classes, neither of them the plan's hot one
    return 2 if z >= 20 else 0


def _first(z, y):          # the two lines of the first tile differ in the first plane
    return (1 if y % 2 == 0 else 2) if z == 0 else 0


PLACED = {"changes": _changes, "third": _third, "halves": _halves, "first": _first}


def placed_matrix(fam, ny, nz, extra=0, xk=0):
    """A GridMat whose line (z, y) has the class PLACED[fam](z, y) of the palette, registered where `K.plane_case_matrix` finds it."""
    key = (fam, PL, ny, nz, extra, xk * PL)
    if key not in K._MATS:
        lines = ny * nz + extra
        ln = np.arange(lines)
        which = np.array([PLACED[fam](int(l // ny), int(l % ny)) for l in ln])
        want = np.broadcast_to(np.array(PALETTE, dtype=np.uint8)[which][:, :, None], (lines, 7, PL)).copy()
        K._MATS[key] = K.GridMat("%s_%dx%dx%d+%d+%d" % key, PL, ny, nz, extra, want, xk * PL)
    return K._MATS[key]


def WC(name, fam, ny, nz, depth, extra=0, xk=0, hot="most"):
    return K.PC(name, fam, ny, nz, extra=extra, xk=xk, hot=hot, tile=2, depth=depth)


WINDOW_CASES = [WC("nz%d-d%d" % (nz, d), "bench", (4, 6)[nz % 2], nz, d) for nz in (63, 64, 65, 127, 128, 129, 130) for d in sorted({nz, 64, 65})]
SHORT_CASES = [WC("nz%d-d%d" % (nz, d), ("bench", "natural")[nz % 2], 4, nz, d) for nz in (1, 2, 3, 4, 5, 9) for d in sorted({1, 4, nz})]
PLACED_CASES = [WC("changes", "changes", 4, 140, 140), WC("third", "third", 6, 70, 70), WC("hot-unused", "halves", 4, 40, 40, hot="unused"),
                WC("single", "diag", 4, 66, 66), WC("first", "first", 4, 24, 24), WC("ny18", "bench", 18, 65, 65), WC("ny18-natural", "natural", 18, 9, 5)]
END_CASES = ([WC("ragged%d" % e, "bands", 4, 66, 66, extra=e) for e in (1, 3)] + [WC("ragged%d-cut" % e, "bench", 6, 21, 8, extra=e) for e in (1, 3)]
             + [WC("xlong%d" % k, "bands", 4, 66, 66, xk=k) for k in (1, 5)] + [WC("xlong1-ragged1", "bands", 6, 9, 9, extra=1, xk=1)])
CASES = WINDOW_CASES + SHORT_CASES + PLACED_CASES + END_CASES


def case_matrix(case):
    _, fam, ny, nz, extra, xk = case[:6]
    return placed_matrix(fam, ny, nz, extra, xk) if fam in PLACED else K.plane_case_matrix(case)


# ---------------------------------------------------------------------------------------------------------------------------
# plane_walk_ahead restated
# ---------------------------------------------------------------------------------------------------------------------------
def ahead_walk(la, line_class, hot, tile, zc, append):
    """One workgroup's walk: (steps [(kind, plane)], class words read [line index], decodes of another class)."""
    y0 = la.tile_geometry(tile)[0]
    ny, lines = la.ny, la.lines
    z, zend, zh = zc * la.depth, min(zc * la.depth + la.depth, la.nz), la.zh(tile, zc, append)
    reads = []

    def request(zz):
        at = [min(zz * ny + y0 + l, lines - 1) for l in (0, 1)]
        reads.extend(at)
        return [int(line_class[a]) for a in at]
    cw = [request(z + i) for i in range(4)]
    other, decodes = -1, 0
    for l in (1, 0):
        if cw[0][l] != hot and z * ny + y0 + l < lines:
            other = cw[0][l]
    decodes += other >= 0
    steps = []
    while z < zend:
        while z + 4 <= zh and all(c in (hot, other) for plane in cw for c in plane):
            steps += [("fast", z + i) for i in range(4)]
            cw = [request(z + 4 + i) for i in range(4)]
            z += 4
        if z >= zend:
            break
        for l in (0, 1):
            if z * ny + y0 + l < lines and cw[0][l] not in (hot, other):
                other, decodes = cw[0][l], decodes + 1
        steps.append(("slow", z))
        z += 1
        cw = cw[1:] + [request(z + 3)]
    return steps, reads, decodes


def ahead_requests_inside(la, line_class, hot, append):
    """Every element the new walk requests lies in x[0 .. x_last], every one it stores (or reads as the addend) in y[0 .. n - 1], every
    class word in the class array; every plane of every walk is stepped through once.  Returns {'fast', 'slow', 'decodes'} (None: not so)."""
    xlines, ny, n = (la.x_last + 1) // PL, la.ny, la.lines * PL
    out = collections.Counter()
    for tile in range(la.tiles):
        y0 = la.tile_geometry(tile)[0]
        for zc in range(la.chunks):
            steps, reads, decodes = ahead_walk(la, line_class, hot, tile, zc, append)
            z0, zend = zc * la.depth, min(zc * la.depth + la.depth, la.nz)
            if [z for _, z in steps] != list(range(z0, zend)) or min(reads) < 0 or max(reads) > la.lines - 1:
                return None
            xs, ys = [], []
            clamp = lambda zz, w: min(max(zz * ny + y0 - 1 + w, 0), xlines - 1)               # line_of: window line w of plane zz
            for w in range(4):                                                                  # fill_registers, rotate_by_copy: whole lines, clamped
                for zz in range(z0 - 1, zend + 3):
                    xs += [clamp(zz, w) * PL, clamp(zz, w) * PL + PL - 1]
            for kind, z in steps:
                at = lambda plane, line: (plane * ny + y0 + line) * PL
                if kind == "fast":
                    xs += [at(z + 3, 0), at(z + 3, 1) + PL - 1, at(z + 2, 0) - 1, at(z + 2, 1) + PL, at(z + 2, -1), at(z + 2, 2) + PL - 1]
                    ys += [at(z, 0), at(z, 1) + PL - 1] + ([at(z + 1, 0), at(z + 1, 1) + PL - 1] if append else [])
                else:
                    ys += [e for l in (0, 1) if z * ny + y0 + l < la.lines for e in (at(z, l), at(z, l) + PL - 1)]
                    if append:                                                                  # yold: clamped to the lines of y
                        ys += [min(max((z + 1) * ny + y0 + l, 0), la.lines - 1) * PL for l in (0, 1)]
            if min(xs) < 0 or max(xs) > la.x_last or (ys and (min(ys) < 0 or max(ys) > n - 1)):
                return None
            out["fast"] += sum(k == "fast" for k, _ in steps)
            out["slow"] += sum(k == "slow" for k, _ in steps)
            out["decodes"] += decodes
    return out


class Run(K.PlaneRun):
    """A case of this file on the device: the plan filled by hand, tables between guards, the host checks of both walks done."""

    def __init__(self, G, oracle, case):
        case_matrix(case)                                            # (registers a placed matrix before PlaneRun looks it up)
        K.PlaneRun.__init__(self, G, oracle, case, np.float64)
        la = K.plane_launch_of(self.p, self.mat, np.float64)
        assert la.tile == 2 and not la.flat_walk
        for append in (False, True):
            self.model = ahead_requests_inside(la, self.mat.line_class, self.p.hot_block, append)
            assert self.model is not None, self.what + ("the new walk would leave the arrays: no launch",)


def both_walks(G, oracle, R):
    """Both walks on the same vectors: each equal to the oracle bit for bit with its sentinels intact (`K.check_all`), and to each other."""
    V = K.Vectors(G, R.C)
    outs = {}
    for walk in WALKS:
        with K.environment(G.L, VEXHIP_PLANE_WALK=walk):
            outs[walk] = K.check_all(oracle, V, R.call, R.what + ("walk %d" % walk,))
    for mode in K.MODES:
        assert outs[0][mode].tobytes() == outs[1][mode].tobytes(), R.what + (mode, "the two walks differ")
    K.check_guards(R.tables, R.what)


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_both_walks_on_hand_built_plans(G, oracle, case):
    both_walks(G, oracle, Run(G, oracle, case))


# the matrix as SELL-512 code blocks (csrc/plane.hpp decode_block: an ELL width below 8, an odd number of column pairs, padding codes):
# the block-form cases of test_gpu_plane_grid_kernels.py that have tiles of two lines -- 4 lines x 24 planes, walks of 8 planes
BLOCK_CASES = [c for c in K.PLANE_CASES if c[0].startswith("blocks-w") and c[9]["tile"] == 2]


@gpu
@pytest.mark.parametrize("case", BLOCK_CASES, ids=[c[0] for c in BLOCK_CASES])
def test_both_walks_on_code_blocks(G, oracle, case):
    assert case[8] > 0 and [c[0] for c in BLOCK_CASES] == ["blocks-w2", "blocks-w4", "blocks-w6", "blocks-w8"]
    both_walks(G, oracle, Run(G, oracle, case))


@gpu
def test_unset_selects_the_new_walk_and_other_shapes_ignore_the_switch(G, oracle):
    """Unset is 1 (the same bytes, whatever they are, is all a product can show); tiles of four and flat plans have one walk."""
    R = Run(G, oracle, WC("nz65-d65", "bench", 4, 65, 65))
    V = K.Vectors(G, R.C)
    os.environ.pop("VEXHIP_PLANE_WALK", None)
    G.L.reload_env()
    K.check_all(oracle, V, R.call, R.what + ("unset",))
    for name in ("ny8-t4", "flat1-t2"):
        R = K.PlaneRun(G, oracle, K.case_named(K.PLANE_CASES, name), np.float64)
        for walk in WALKS:
            with K.environment(G.L, VEXHIP_PLANE_WALK=walk):
                K.check_all(oracle, K.Vectors(G, R.C), R.call, R.what + ("walk %d" % walk,))


@gpu
@pytest.mark.parametrize("shape", ((4, 9, 9), (6, 65, 65), (4, 66, 16)), ids=lambda s: "ny%d-nz%d-d%d" % s)
def test_addend_forms(G, oracle, shape):
    """y = alpha A x + beta z with z another array (the walk's ZM = 1 with its own array) and z = x (ZM = 2), and the plain product, on a
    matrix the library stored itself, under both walks."""
    from vexcl_amd import ops
    ny, nz, depth = shape
    mat = K.grid_matrix("natural", PL, ny, nz)
    C = K.Case.of(oracle, mat, np.float64)
    ptr, col, val = C.csr
    x, zv = C.x, C.y0
    with np.errstate(invalid="ignore"):
        want = {"plain": oracle.spmv_csr(ptr, col, val, x, alpha=-0.75),
                "array": -0.5 * zv + oracle.spmv_csr(ptr, col, val, x, alpha=1.5),
                "x": 2.0 * x[:mat.n] + oracle.spmv_csr(ptr, col, val, x, alpha=-1.0)}
    dx, dz = G.up(x), G.up(zv)
    got = {}
    for walk in WALKS:
        with K.environment(G.L, VEXHIP_PLANE_FORCE=1, VEXHIP_PLANE_DEPTH=depth, VEXHIP_PLANE_WALK=walk):
            A = ops.SpMat(G.up(ptr), G.up(col), G.up(val))
            assert A.plane is not None and A.plane["tile"] == 2 and A.plane["depth"] == depth and not A.plane["flat"], (A.plane, A.storage)
            ybuf = G.up(np.full(mat.n + 2 * K.GUARD, K.SENTINEL))
            y = ybuf[K.GUARD:K.GUARD + mat.n]
            for form in ("plain", "array", "x"):
                if form == "plain":
                    A.apply(dx, y, -0.75, False)
                elif form == "array":
                    A.apply_axpby(dx, y, 1.5, dz, -0.5)
                else:
                    assert len(x) == mat.n
                    A.apply_axpby(dx, y, -1.0, dx, 2.0)
                out = ybuf.cpu().numpy()
                got[walk, form] = out[K.GUARD:K.GUARD + mat.n].copy()
                assert np.array_equal(got[walk, form], want[form], equal_nan=True), (shape, walk, form, K.first_difference(got[walk, form], want[form]))
                assert (out[:K.GUARD] == K.SENTINEL).all() and (out[-K.GUARD:] == K.SENTINEL).all(), (shape, walk, form, "a sentinel changed")
    for form in ("plain", "array", "x"):
        assert got[0, form].tobytes() == got[1, form].tobytes(), (shape, form, "the two walks differ")


def test_host_model_of_the_walk(built_lib):
    """No GPU: the model that the GPU tests rely on.  A walk reads the class words of its planes once each and looks four planes past its
    end; the benchmark's operator takes slow steps only in the planes that `zh` excludes; the placed cases contain what their names say."""
    def launch(case):
        mat = case_matrix(case)
        p = K.fill_plane(built_lib, 256, mat, case)
        return mat, p, K.plane_launch_of(p, mat, np.float64)
    # a 64-plane walk: 2 x 64 class words, each once, + the look past the end (2 x 4 words, clamped to the last line)
    mat, p, la = launch(WC("nz64-d64", "bench", 18, 64, 64))         # (18 lines per plane: the interior class is the hot one, as at 512^3)
    assert p.hot_block == int(mat.line_class[la.ny + 1]) != int(mat.line_class[0])
    for tile in range(la.tiles):
        steps, reads, decodes = ahead_walk(la, mat.line_class, p.hot_block, tile, 0, False)
        count = collections.Counter(reads)
        inside = [tile * 2 + l + z * la.ny for z in range(64) for l in (0, 1)]
        assert len(reads) == 2 * (64 + 4) and all(count[i] == (1 if i != la.lines - 1 else count[i]) for i in inside) and set(count) <= set(inside) | {la.lines - 1}
        assert count[la.lines - 1] == 2 * 4 + (la.lines - 1 in inside)
        # plane 0 is of the boundary class, decoded before the first look: fast steps from plane 0 up to zh, in groups of four
        zh = la.zh(tile, 0, False)
        assert decodes == 1 and [k for k, _ in steps] == ["fast"] * (zh // 4 * 4) + ["slow"] * (64 - zh // 4 * 4), (tile, zh, steps)
    # walks cut at 64: the second one starts in the interior, with the hot class, and decodes the boundary class in its last plane
    mat, p, la = launch(WC("nz130-d64", "bench", 18, 130, 64))
    assert la.chunks == 3 and ahead_walk(la, mat.line_class, p.hot_block, 1, 1, False)[2] == 0 and ahead_walk(la, mat.line_class, p.hot_block, 1, 2, False)[2] == 1
    seen = {}
    for case in CASES:
        mat, p, la = launch(case)
        assert K.visit_once(la), case[0]
        for append in (False, True):
            assert K.addresses_inside(la, append) >= 0, case[0]
            seen[case[0], append] = ahead_requests_inside(la, mat.line_class, p.hot_block, append)
            assert seen[case[0], append] is not None, case[0]
            assert seen[case[0], append]["fast"] + seen[case[0], append]["slow"] == la.nz * la.tiles
    assert all(seen[c[0], False]["fast"] == 0 for c in SHORT_CASES if min(c[3], c[9]["depth"]) < 4 + 3)
    assert all(seen[c[0], False]["fast"] > 0 for c in WINDOW_CASES + PLACED_CASES + END_CASES if c[0] != "ny18-natural")
    # the third class: a slow step at plane 21 and the decodes around it, fast steps behind it
    mat, p, la = launch(case_of("third"))
    steps, _, decodes = ahead_walk(la, mat.line_class, p.hot_block, 0, 0, False)
    kinds = dict((z, k) for k, z in steps)
    assert kinds[21] == "slow" and "fast" in [kinds[z] for z in range(8, 21)] and "fast" in [kinds[z] for z in range(22, 30)] and "fast" in [kinds[z] for z in range(30, 66)], steps
    assert decodes >= 3 and len({int(mat.line_class[z * la.ny]) for z in (7, 8, 21, 22, 30)}) == 3, decodes
    # the line that changes at 63, 64, 65, 128: its second class is decoded in a slow step at plane 63 (the other class was plane 0's
    # until then); from there on the line alternates between the hot and the other class inside groups of fast steps
    mat, p, la = launch(case_of("changes"))
    steps, _, _ = ahead_walk(la, mat.line_class, p.hot_block, 0, 0, False)
    kinds = dict((z, k) for k, z in steps)
    assert kinds[63] == "slow" and all(kinds[z] == "fast" for z in (64, 65, 66, 127, 128, 129)), steps
    assert [int(mat.line_class[z * 4 + 1]) == p.hot_block for z in (62, 63, 64, 65, 127, 128)] == [True, False, True, False, False, True]
    # no line uses the hot class: every line goes through the other one, a slow step where it changes
    mat, p, la = launch(case_of("hot-unused"))
    assert p.hot_block == len(mat.classes) and seen["hot-unused", False]["fast"] > 0 and seen["hot-unused", False]["decodes"] >= 2 * la.tiles
    mat, p, la = launch(case_of("single"))
    assert len(mat.classes) == 1 and seen["single", False]["decodes"] == 0
    mat, p, la = launch(case_of("first"))
    assert mat.line_class[0] != mat.line_class[1] and ahead_walk(la, mat.line_class, p.hot_block, 0, 0, False)[0][0] == ("slow", 0)


def case_of(name):
    return [c for c in CASES if c[0] == name][0]
