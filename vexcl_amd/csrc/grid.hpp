// What the grid products share (grid.hip: fp64, two rows per lane; grid32.hip: fp32, four rows per lane): the geometry a launch is given
// and how the host assembles it.
#pragma once
#include "launch.hpp"

namespace vexhip {
namespace {

struct grid_dev {
    long long lines;         // grid lines of the matrix: rows / nx
    long long x_last;        // largest valid index of x
    long long n;             // rows
    int nx, ny, nz;          // line length, lines per plane, planes: ceil(lines / ny)
    int depth;               // planes per workgroup
    int segs, seg_len;       // segments per line, rows per segment (even, <= 512)
    int tiles, tpx;          // ceil(ny / 2) * segs, and per XCD: ceil(tiles / 8)
    int hot;                 // line class decoded into registers with scalar masks
    int pitch;               // bytes per position row of a class table (>= segs * 512, padded with 255)
    int flat;                // no entry at +-nx in any line (a 2-D operator on virtual lines): the lines above / below a tile are not requested
    int cpx;                 // 0: an XCD owns TILES (all walks of a tile share its L2: the lines between neighbouring tiles);  > 0 (flat plans:
                             // a row of a 2-D grid has a handful of tiles -- six for 12 000 points -- and nothing to share between them): an XCD
                             // owns cpx consecutive WALKS of every tile, blockIdx -> (xcd, walk, tile)
};

// The requirements of a launch on a matrix of `rows` rows.  whole_x: the plan's x_last must cover the rows (false: a one-launch step, whose x is
// the device's segment)
inline int grid_check(const vexhip_grid *g, int64_t rows, const void *values, const void *x, const void *y, bool whole_x) {
    VEXHIP_REQUIRE(g && g->usable && g->line_class && g->table && values && x && y, "bad grid product arguments");
    if (int rc = vexhip_sell8_grid_check(g, rows)) return rc;
    VEXHIP_REQUIRE(!whole_x || g->x_last + 1 >= rows, "bad grid plan");
    return 0;
}

// the launch struct of a plan with the plan's walks (cpx: grid_workgroups); rows: those the launch addresses (a one-launch step: of the stored grid)
inline grid_dev grid_launch(const vexhip_grid &g, long long rows) {
    grid_dev gd;
    gd.lines = rows / g.nx; gd.x_last = g.x_last; gd.n = rows;
    gd.nx = g.nx; gd.ny = g.lines_per_plane; gd.nz = g.planes; gd.depth = g.depth;
    gd.segs = g.segments; gd.seg_len = g.segment_rows;
    gd.tiles = (gd.ny + 1) / 2 * gd.segs; gd.tpx = (gd.tiles + 7) / 8; gd.hot = g.hot_class; gd.pitch = g.pitch; gd.flat = g.flat;
    return gd;
}

// Workgroups of a launch that walks `planes` planes gd.depth at a time, and who owns what (gd.cpx: see above)
inline int grid_workgroups(grid_dev &gd, long long planes, unsigned *grid) {
    const long long chunks = (planes + gd.depth - 1) / gd.depth;
    gd.cpx = gd.flat ? (int)((chunks + 7) / 8) : 0;
    const long long n = gd.cpx ? 8ll * gd.cpx * gd.tiles : 8ll * gd.tpx * chunks;
    VEXHIP_REQUIRE(n < (1ll << 31), "matrix too large for one launch");
    *grid = (unsigned)n;
    return 0;
}

} // namespace
} // namespace vexhip
