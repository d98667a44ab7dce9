// What the plane products share (plane.hip: fp64, two rows per lane; plane32.hip: fp32, four rows per lane): the geometry a launch
// is given, how the host assembles it, and the numbering of the seven stencil positions.
#pragma once
#include "launch.hpp"

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
