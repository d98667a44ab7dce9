// The walk of the GRID products (grid.hip: double, grid32.hip: float): a workgroup owns TWO adjacent grid lines of ANY length (one
// segment of them) and walks through the planes; lane t owns rows R t .. R t + R - 1 of its segment, R = 16 / sizeof(V) (walk.hpp).
// What the value type changes is the number of rows behind a lane -- the rows of s_other, the bytes of an element in edge_b, line_b
// and `over`, how many rows a lane at the end of its line stores -- and nothing else.
#pragma once
#include "halo.hpp"
#include "walk.hpp"
#include "grid.hpp"

#include <algorithm>

namespace vexhip {
namespace {

// MAXT: lanes of a workgroup at most (the lane-private rows of s_other)
// HALO (round 6; halo.hpp, the PULL form only; double only): the launch is one device's whole product step.  x and y are addressed in the numbering of
// the STORED grid, whose plane z0 - 1 / z1 (where the device has a neighbour) is a ghost plane: read from the neighbour's x in place
// (H.lo / H.hi), behind its "x is final" flag where flags order the launches.  The walks are the plan's; the two that touch a ghost
// plane are dispatched last and wait before they start.
// ZM: the addend of the result (walk.hpp add_addend): 0 none, 1 beta times the array zs ('+=': zs = y, beta = 1), 2 beta times x itself (from the registers)
template <typename V, int ZM, int STORE_AUX, int MAXT, bool HALO>
__device__ __forceinline__
void grid_walk(const V *__restrict__ x, V *__restrict__ y, V alpha, const V *__restrict__ zs, V beta,
        const int *__restrict__ line_class, const unsigned char *__restrict__ table, const V *__restrict__ values, const grid_dev &gd,
        const halo_dev &H, [[maybe_unused]] const unsigned long long step)
{
    static_assert(!HALO || sizeof(V) == 8, "the ghost planes of a one-launch step are doubles");
    typedef vec_of<V> VEC;
    constexpr int TY = 2, R = rows_of<V>, VB = (int)sizeof(V);
    // LDS: the value table and the decoded values of the OTHER class, lane-private ([position * R + row][lane]: conflict-free)
    __shared__ V s_value[256];
    __shared__ V s_other[7 * R][MAXT];

    const int t = threadIdx.x;
    const unsigned b = blockIdx.x, xcd = b & 7u, q = b >> 3;
    int zc = (int)(q / (unsigned)gd.tpx);
    int tile = (int)xcd * gd.tpx + (int)(q - (unsigned)zc * (unsigned)gd.tpx);
    if (gd.cpx) { const int w = (int)(q / (unsigned)gd.tiles); tile = (int)(q - (unsigned)w * (unsigned)gd.tiles); zc = (int)xcd * gd.cpx + w; }      // (grid.hpp)
    if (tile >= gd.tiles) return;                                   // the whole workgroup
    const int ytile = tile / gd.segs, seg = tile - ytile * gd.segs;
    const int y0 = TY * ytile;
    const int nl = gd.ny - y0 < TY ? gd.ny - y0 : TY;               // lines of the tile inside a plane (odd ny: the last tile has one)
    const int row0 = seg * gd.seg_len;
    const int len = gd.nx - row0 < gd.seg_len ? gd.nx - row0 : gd.seg_len;
    int z, zend_;
    [[maybe_unused]] bool ghost_bad = false;
    [[maybe_unused]] __shared__ int s_flag;
    if constexpr (HALO) {
        // the walks of the planes [z0, z1), the first and the last of them -- which touch a ghost plane -- dispatched behind the others
        const int nch = (H.z1 - H.z0 + gd.depth - 1) / gd.depth;
        const int c = nch > 1 ? (zc + 1) % nch : 0;
        z = H.z0 + c * gd.depth; zend_ = z + gd.depth < H.z1 ? z + gd.depth : H.z1;
        if (zc >= nch || z >= zend_) return;
        ghost_bad = !halo_wait(H, step, H.lo && z == H.z0, H.hi && zend_ == H.z1, &s_flag);
    } else {
        z = zc * gd.depth;
        zend_ = z + gd.depth < gd.nz ? z + gd.depth : gd.nz;
        if (z >= zend_) return;
    }
    const int zend = zend_;
    const int nx = gd.nx, ny = gd.ny;
    // HALO: the elements of x and y that exist are those of the planes [z0, z1)
    const long long own_lo = HALO ? (long long)H.z0 * ny * nx : 0;
    const long long lines = HALO ? (long long)H.z1 * ny : gd.lines, x_last = HALO ? (long long)H.z1 * ny * nx - 1 : gd.x_last, n = HALO ? (long long)H.z1 * ny * nx : gd.n;
    const unsigned lane_b = 16u * (unsigned)t;
    const int nv = len - R * t < 0 ? 0 : (len - R * t > R ? R : len - R * t);      // rows of this lane inside the segment: it stores that many
    // the element beyond either end of the wave's 64 R rows of a segment: lane 63 reads the one behind them, every other lane the
    // one in front (lane 0 uses it; one cache line for the rest) -- byte offset from the start of the segment
    const int edge_b = (t >> 6) * 1024 + ((t & 63) == 63 ? 1024 : -VB);

    for (int i = t; i < 256; i += (int)blockDim.x) s_value[i] = values[i];
    __syncthreads();

    // ---- a line class -> values (into s_other) and validity (returned) of this lane's rows at the seven positions ----
    // (four rows per lane: lanes beyond the end of the line read the last bytes of the position row -- padding, 255 -- and a lane may
    //  start at any even byte: row0 is even)
    const int tb_off = R == 2 ? row0 + R * t : (row0 + R * t < gd.pitch - R ? row0 + R * t : gd.pitch - R);
    auto decode = [&](int cls) -> unsigned {
        return decode_table<true>(table + (long long)cls * 7 * gd.pitch + tb_off, gd.pitch, s_value, s_other, t);
    };

    const int hot = gd.hot;
    V aH[7][R];                                 // the hot class: values ...
    unsigned long long mH[7][R];                // ... and the lanes with an entry, per position and row
    take_hot(decode(hot), s_other, t, aH, mH);
    unsigned bitsO = 0;
    int other = -1;                             // what s_other holds now is the hot class's: never asked for
    const line_terms<V, 7 * R, MAXT> terms = {aH, mH, s_other, hot, other, bitsO, t, alpha, beta};

    // clamped requests (prologue, slow steps): line `l` of the tile's window (0 = the line above the tile, 1 .. TY = the tile,
    // TY + 1 = the line below) in plane zz, element by element.  What lies outside x is never referenced by an entry; what is
    // loaded in its place is multiplied by +0.0 behind a mask
    auto elem = [&](long long i) -> V {
        if constexpr (HALO) {
            // an element of the plane below / above the device's planes: the neighbour's boundary plane of x, where it lies
            const long long plane = (long long)ny * nx;
            if (i < own_lo) { const long long j = i - (own_lo - plane); if (H.lo && j >= 0) return ghost_bad ? __builtin_nan("") : H.lo[j]; }
            else if (i > x_last) { const long long j = i - (x_last + 1); if (H.hi && j < plane) return ghost_bad ? __builtin_nan("") : H.hi[j]; }
            i = i < own_lo ? own_lo : i;
        }
        i = i < 0 ? 0 : i; i = i > x_last ? x_last : i; return x[i];
    };
    auto ld = [&](int zz, int l) -> VEC {
        const long long i = ((long long)zz * ny + (y0 - 1 + l)) * nx + row0 + R * t;
        VEC r;
#pragma unroll
        for (int k = 0; k < R; ++k) r[k] = elem(i + k);
        return r;
    };
    auto edge = [&](int zz, int l) -> V {
        return elem(((long long)zz * ny + (y0 - 1 + l)) * nx + row0 + edge_b / VB);
    };
    auto yold = [&](int zz, int l) -> VEC {
        const long long i = ((long long)zz * ny + (y0 + l)) * nx + row0 + R * t;
        VEC r;
#pragma unroll
        for (int k = 0; k < R; ++k) { long long j = i + k; j = j < own_lo ? own_lo : j; j = j > n - 1 ? n - 1 : j; r[k] = zs[j]; }
        return r;
    };

    // ---- the registers of the walk (walk.hpp), filled for plane z ----
    VEC Cs[4][TY], Hs[2][2], Yo[TY];
    V Es[2][TY];
    const unsigned line_b = (unsigned)nx * (unsigned)VB;              // bytes from a line to the next
    const unsigned plane_b32 = (unsigned)ny * line_b;                 // ... to the same line of the next plane (the plan: (depth + 4) of them < 2^32)
    const int z_first = z;
    // buffer resources of the fast loop: x from the segment of the line above the tile in the workgroup's first plane, y from
    // the tile's first line in that plane.  No range check (the scalar offset that moves with the planes takes no part in it):
    // the fast loop only runs where every request of every lane lies inside the arrays (zh below)
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<V *>(x + (((long long)z_first * ny + (y0 - 1)) * nx + row0)), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(y + (((long long)z_first * ny + y0) * nx + row0), 0, -1, 0x00020000);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(const_cast<V *>(ZM == 1 ? zs : x) + (((long long)z_first * ny + y0) * nx + row0), 0, -1, 0x00020000);
    // gd.flat (round 6): no entry at +-nx anywhere -- a 5-point operator on a 2-D grid, its rows cut into virtual lines: the lines above
    // and below the tile are never requested (two of the six 16-byte requests of a step)
    const bool flat = gd.flat != 0;                                   // uniform
    fill_registers<ZM>(Cs, Hs, Es, Yo, z, !flat, ld, edge, yold);

    // fast steps: every request lies inside the arrays.  A lane may sit beyond the end of its line (it stores nothing, but it
    // requests): `over` = the furthest element, from the start of a line, that a lane of this workgroup asks for
    int zh = zend;
    {
        const long long over = row0 + R * (long long)blockDim.x + 1;
        const long long xl_in = x_last - over >= 0 ? (x_last - over) / nx : -1;       // largest line all of whose requests are inside x
        const long long yl_in = n - 1 - over >= 0 ? (n - 1 - over) / nx : -1;         // ... inside y ('+=' reads the old y one plane ahead)
        // largest z with (z + ahead) * ny + y0 + line <= limit, + 1
        auto end_for = [&](long long limit, int ahead, int line) -> long long { const long long v = limit - y0 - line; return v < 0 ? 0 : v / ny - ahead + 1; };
        long long e = end_for(xl_in, 3, TY);                                           // x: planes up to z + 3, lines up to the one below the tile
        e = std::min(e, end_for(lines - 1, 0, TY - 1));                               // y: both lines exist
        if (ZM == 1) e = std::min(e, end_for(yl_in, 1, TY - 1));
        zh = zh < e ? zh : (int)(e < 0 ? 0 : e);
    }

    while (z < zend) {
        unsigned long long use_hot[TY];
        const int run = fast_run(line_class, ny, y0, nl, z, zh, hot, other, t, use_hot);
        if (run >= 4) {
            // xo: plane z + 2, the line above the tile; yo: plane z, the tile's first line; both relative to the workgroup's first plane
            unsigned xo = (unsigned)((z + 2 - z_first) * plane_b32), yo = (unsigned)((z - z_first) * plane_b32);
            auto fast_step = [&](VEC (&P)[TY], VEC (&C)[TY], VEC (&N)[TY], VEC (&Hl)[2], V (&E)[TY]) {
                VEC o[TY];
#pragma unroll
                for (int l = 0; l < TY; ++l) {
                    V xs[R][7], s[R] = {};
                    stencil_x(P, C, N, Hl, E, l, xs);
                    if (use_hot[l] & 1ull) hot_sums(s, aH, mH, xs); else other_sums(s, s_other, t, bitsO, xs);      // uniform
                    o[l] = add_addend<ZM>(alpha, s, beta, Yo[l], C[l]);
                }
#pragma unroll
                for (int l = 0; l < TY; ++l) use_hot[l] >>= 1;
#pragma unroll
                for (int l = 0; l < TY; ++l)
                    if (l < nl) {                  // uniform; written once, not read again by this kernel
                        if (nv == R) store16<STORE_AUX>(o[l], ry, (int)lane_b, yo + l * line_b);
                        // the lane at the end of the line.  (nv > 0 here, not only row by row inside: the lanes beyond the line then skip
                        // ONE branch -- without it the fp32 fast loop is 100 instructions longer and 384^3 runs 8 % slower)
                        else if (nv > 0) store_rows<STORE_AUX>(o[l], nv, ry, (int)lane_b, yo + l * line_b);
                    }
                if (ZM == 1) {
#pragma unroll
                    for (int l = 0; l < TY; ++l) Yo[l] = load16<V>(rz, (int)lane_b, yo + plane_b32 + l * line_b);
                }
                if (!flat) {
                    Hl[0] = load16<V>(rx, (int)lane_b, xo);
                    Hl[1] = load16<V>(rx, (int)lane_b, xo + (TY + 1) * line_b);
                }
#pragma unroll
                for (int l = 0; l < TY; ++l) {
                    P[l] = load16<V>(rx, (int)lane_b, xo + plane_b32 + (l + 1) * line_b);
                    E[l] = load_edge<V>(rx, edge_b + VB, xo + (l + 1) * line_b - (unsigned)VB);
                }
                xo += plane_b32; yo += plane_b32; ++z;
            };
            for (int g = run >> 2; g > 0; --g) fast_group(fast_step, Cs, Hs, Es);
            if (run == 64) continue;                                      // look again: the run may go on
        }
        if (z >= zend) break;
        // ---- a slow step: a line needs another class decoded, the last planes (clamped requests), the ragged last plane, what
        // a run leaves over after its groups of four ----
#pragma unroll
        for (int l = 0; l < TY; ++l) {
            const long long li = (long long)z * ny + (y0 + l);
            if (l < nl && li < lines) {                                   // uniform
                const VEC o = line_result<ZM>(terms, __builtin_amdgcn_readfirstlane(line_class[li]), decode, Cs, Hs, Es, Yo, l);
                V *yr = y + li * nx + row0 + R * t;
#pragma unroll
                for (int r = 0; r < R; ++r) if (r < nv) { const V e = o[r]; __builtin_nontemporal_store(e, yr + r); }
            }
        }
        rotate_by_copy<ZM>(Cs, Hs, Es, Yo, z, !flat, ld, edge, yold);
        ++z;
    }
}

} // namespace
} // namespace vexhip
