// What the plane products share (plane.hip: fp64, two rows per lane; plane32.hip: fp32, four rows per lane): the geometry a launch
// is given, how the host assembles it, the numbering of the seven stencil positions, and the device pieces of a walk on 512-point
// lines: the decode of a SELL-512 code block, blockIdx -> tile and planes, the bound of the fast steps, the clamped requests of a
// walk with no ghost plane in reach.
#pragma once
#include "launch.hpp"
#include "walk.hpp"

namespace vexhip {
namespace {

constexpr int PL_ROWS = 512;
constexpr unsigned PL_PAD_FIRST = 254;      // codes 254 / 255 are padding (sell8.hip)

struct plane_dev {
    long long nslices;       // 512-row lines of the matrix
    long long xlines;        // lines of x that may be loaded whole: (x_last + 1) / 512
    long long x_last;
    int ny;                  // lines per plane
    int nz;                  // planes: ceil(nslices / ny)
    int depth;               // planes per workgroup
    int tiles;               // ny / tile height
    int tpx;                 // tiles per XCD: ceil(tiles / 8)
    int hot;                 // dictionary block decoded into registers with scalar masks
    int w;                   // ELL width (<= 8)
    int far;                 // 512 * ny
    int pitch;               // 0: `pool` holds SELL-512 code blocks; > 0: class tables of the grid storage ([class][7 positions][pitch] value codes, grid.hip)
};


// diagonal -> position 0..6 in {-far, -512, -1, 0, 1, 512, far} (the plan has checked that it is one of them)
__device__ __forceinline__ int position_of(int d, int far) {
    return d == 0 ? 3 : d == -1 ? 2 : d == 1 ? 4 : d == -PL_ROWS ? 1 : d == PL_ROWS ? 5 : d == -far ? 0 : 6;
}

// ---- a dictionary block -> values (into s_other) and validity (returned) of the lane's R rows at the seven positions ----
// A code block: per pair of ELL columns 256 words of diagonal codes, then as many of value codes; word i holds rows 2i, 2i + 1 of both
// columns, so a lane reads R / 2 adjacent words per column pair.  s_slot: per diagonal code R times its position.  Row 7 R of s_other
// takes what padding "writes".  w: the ELL width, wp = (w + 1) / 2 its column pairs (the walk computes it once: with the shift inside
// here the fp64 walks of tile 2 spill 40 - 44 bytes more)
template <typename V, int ROWS, int LANES>
__device__ __forceinline__ unsigned decode_block(const char *pool, int blk, int w, int wp, const int *s_slot, const V *s_value, V (&s_other)[ROWS][LANES], int t) {
    constexpr int R = rows_of<V>, H = R / 2;
    static_assert(ROWS == 7 * R + 1, "seven positions of R rows and the padding row");
    const unsigned *cw = reinterpret_cast<const unsigned *>(pool + (long long)blk * ((long long)wp * 2048)) + H * t;
    unsigned dcw[4 * H], vcw[4 * H];        // diagonal codes, value codes: a word per pair of ELL columns and pair of rows
#pragma unroll
    for (int i = 0; i < 4 * H; ++i) { const int u = i / H, h = i % H; dcw[i] = u < wp ? cw[u * 256 + h] : 0xffffffffu; vcw[i] = u < wp ? cw[(wp + u) * 256 + h] : 0u; }
#pragma unroll
    for (int p = 0; p < 7 * R; ++p) s_other[p][t] = 0;
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        unsigned cword[H], vword[H];
#pragma unroll
        for (int h = 0; h < H; ++h) { cword[h] = dcw[(j >> 1) * H + h] >> (16 * (j & 1)); vword[h] = vcw[(j >> 1) * H + h] >> (16 * (j & 1)); }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const unsigned code = j < w ? (cword[r >> 1] >> (8 * (r & 1))) & 255u : 255u;
            const bool real = code < PL_PAD_FIRST;
            const int slot = real ? s_slot[code] + r : 7 * R;
            s_other[slot][t] = s_value[real ? (vword[r >> 1] >> (8 * (r & 1))) & 255u : 255u];      // entry 255 of the table is 0.0
            bits |= (real ? 1u : 0u) << slot;
        }
    }
    return bits & ((1u << (7 * R)) - 1u);
}

// ---- blockIdx -> (XCD, chunk, tile of the XCD): tiles are dealt to XCDs in contiguous ranges (plane_workgroups) ----
// tile_lines: lines per tile; y0: the first of the tile's lines; zc: the chunk.  false: no tile for this workgroup
__device__ __forceinline__ bool plane_tile(const plane_dev &pd, unsigned b, int tile_lines, int &y0, int &zc) {
    const unsigned xcd = b & 7u, q = b >> 3;
    zc = (int)(q / (unsigned)pd.tpx);
    const int tile = (int)xcd * pd.tpx + (int)(q - (unsigned)zc * (unsigned)pd.tpx);
    y0 = tile_lines * tile;
    return tile < pd.tiles;
}
// ... and the planes [z, zend) of chunk zc in a launch without ghost planes.  false: nothing to walk.  (Two functions, two returns in
// the walks: as one, the ahead walk with ZM = 2 grew by 67 instructions inside its fast loop.)
__device__ __forceinline__ bool plane_chunk(const plane_dev &pd, int zc, int &z, int &zend) {
    z = zc * pd.depth;
    zend = z + pd.depth < pd.nz ? z + pd.depth : pd.nz;
    return z < zend;
}

// ---- the end of the fast steps: they need nothing clamped ----
// x has the lines [.., line_hi), y (and an addend array) the lines [.., yline_hi).  a: the largest z with (z + 3) ny + y0 + TY <=
// line_hi - 1 -- planes up to z + 3 inside x, the line below the tile included; bb: the largest z with z ny + y0 + TY - 1 <=
// yline_hi - 1 -- all lines of the tile inside y; old_y: the addend array is requested one plane ahead (inside y also when x is
// longer than y)
__device__ __forceinline__ int fast_limit(int zend, int ny, int y0, int tile_lines, int line_hi, int yline_hi, bool old_y) {
    const int a = (line_hi - 1 - tile_lines - y0) / ny - 3, bb = (yline_hi - tile_lines - y0) / ny - (old_y ? 1 : 0);
    if (line_hi - 1 - tile_lines - y0 < 0 || yline_hi - tile_lines - y0 < 0) return 0;
    int zh = zend;
    zh = zh < a + 1 ? zh : a + 1; zh = zh < bb + 1 ? zh : bb + 1;
    return zh;
}

// ---- clamped requests (prologue, slow steps) of a walk with no ghost plane in reach ----
// Line `l` of the tile's window (0 = the line above the tile, 1 .. TY = the tile, TY + 1 = the line below) in plane zz.  The lines of
// x that exist are [line_lo, line_hi), those of y and the addend array [line_lo, yline_hi).  A line outside x is never referenced
// by an entry; what is loaded in its place is multiplied by +0.0 behind a mask.
// edge_b: the element beyond either end of the wave's 64 R rows of a line: lane 63 reads the one behind them, every other lane the
// one in front (lane 0 uses it; one cache line for the rest) -- byte offset from the start of the line
template <typename V>
struct clamped_requests {
    typedef vec_of<V> VEC;
    typedef VEC __attribute__((aligned(sizeof(V) == 8 ? 16 : 4))) LDVEC;      // (a quad of floats may start at any element)
    const V *x, *zs;
    int ny, y0, line_lo, line_hi, yline_hi;
    long long x_last;
    unsigned lane_b;
    int edge_b;
    __device__ __forceinline__ int line_of(int zz, int l) const {
        int li = zz * ny + (y0 - 1 + l);
        li = li < line_lo ? line_lo : li; li = li >= line_hi ? line_hi - 1 : li;
        return li;
    }
    __device__ __forceinline__ VEC ld(int zz, int l) const {
        return *reinterpret_cast<const LDVEC *>(reinterpret_cast<const char *>(x + (long long)line_of(zz, l) * PL_ROWS) + lane_b);
    }
    __device__ __forceinline__ V edge(int zz, int l) const {
        long long i = (long long)line_of(zz, l) * PL_ROWS + (edge_b >> (sizeof(V) == 8 ? 3 : 2));
        const long long a = (long long)line_lo * PL_ROWS;
        i = i < a ? a : i; i = i > x_last ? x_last : i;
        return x[i];
    }
    __device__ __forceinline__ VEC yold(int zz, int l) const {
        int li = zz * ny + (y0 + l);
        li = li < line_lo ? line_lo : li; li = li >= yline_hi ? yline_hi - 1 : li;
        return *reinterpret_cast<const LDVEC *>(reinterpret_cast<const char *>(zs + (long long)li * PL_ROWS) + lane_b);
    }
};
__device__ __forceinline__ int edge_offset(int t, int elem_b) { return (t >> 6) * 1024 + ((t & 63) == 63 ? 1024 : -elem_b); }

// The requirements of a launch on a matrix of `rows` rows.  tile: lines per workgroup of the kernel (0: the plan's); line_bytes: > 0: the PLAN's
// depth is walked and must fit 32-bit byte offsets with such lines (0: the launch chooses its own); align16: of x and y (fp64; fp32: no rule)
inline int plane_check(const vexhip_plane *plane, int tile, int line_bytes, int64_t rows, int64_t w, bool tables, const void *x, const void *y, bool align16) {
    VEXHIP_REQUIRE(plane && plane->usable && tables && x && y, "bad plane product arguments");
    VEXHIP_REQUIRE(rows > 0 && rows % PL_ROWS == 0 && w >= 1 && w <= 8, "bad plane product geometry");
    VEXHIP_REQUIRE(plane->table_pitch == 0 || plane->table_pitch >= PL_ROWS + 2, "bad plane plan (table pitch)");
    if (!tile) tile = plane->tile;
    VEXHIP_REQUIRE((tile == 2 || tile == 4) && plane->lines_per_plane >= 4 && plane->lines_per_plane % tile == 0 && plane->depth >= 1 && plane->planes >= 1
                   && (plane->x_last + 1) % PL_ROWS == 0 && ((long long)plane->depth + 4) * plane->lines_per_plane * line_bytes < (1ll << 32), "bad plane plan");
    VEXHIP_REQUIRE(!align16 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0, "plane product: x and y must be 16-byte aligned");
    return 0;
}

// the launch struct of a plan; rows: those the launch addresses (a one-launch step: of the stored grid)
inline plane_dev plane_launch(const vexhip_plane &plane, long long rows, long long w, int tile, int depth) {
    plane_dev pd;
    pd.nslices = rows / PL_ROWS; pd.xlines = (plane.x_last + 1) / PL_ROWS; pd.x_last = plane.x_last;
    pd.ny = plane.lines_per_plane; pd.nz = plane.planes; pd.depth = depth;
    pd.tiles = pd.ny / tile; pd.tpx = (pd.tiles + 7) / 8; pd.hot = plane.hot_block; pd.w = (int)w; pd.far = pd.ny * PL_ROWS;
    pd.pitch = plane.table_pitch;
    return pd;
}

// Workgroups of a launch that walks `planes` planes pd.depth at a time, blockIdx -> (XCD, chunk, tile of the XCD), with short_chunks more walks
// per tile and `first` workgroups in front of the walks (plane.hip's one-launch step: the chunks next to the ghost planes, the push workgroups)
inline int plane_workgroups(const plane_dev &pd, long long planes, long long short_chunks, long long first, unsigned *grid) {
    const long long n = first + 8ll * pd.tpx * ((planes + pd.depth - 1) / pd.depth + short_chunks);
    VEXHIP_REQUIRE(n < (1ll << 31), "matrix too large for one launch");
    *grid = (unsigned)n;
    return 0;
}

} // namespace
} // namespace vexhip
