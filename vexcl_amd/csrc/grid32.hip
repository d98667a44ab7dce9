// The GRID product for fp32 (round 5): y (=|+=) alpha * A * x for a matrix stored by grid line (grid.hip: a class per line, a
// table of value codes per class and position) whose lines have ANY length -- the walk of the fp64 grid product with FOUR rows
// per lane, as plane32.hip does it for 512-point lines: every request is 16 bytes per lane (at 4-byte addresses: lines start
// at any element), a wave covers 256 rows of a segment, workgroups are 1 .. 4 waves.  Until this kernel float matrices on
// grids other than 512-point lines took the pair product of the SELL-512 storage and ran SLOWER than the same matrix in
// double (384^3: 0.248 ms against 0.183; 640^3: 1.39 against 0.87).  Now 384^3 0.10 ms, 500^3 0.23, 640^3 0.54, 700^3 0.69 - 0.73
// (profiles/r05_fp32_sizes.json): 0.47 - 0.56 of the HBM peak by the bytes that must move -- a line of 384 floats fills 96 of
// the 128 lanes of its two waves, one of 640 fills 160 of 192: the lanes beyond the line still request.
// Semantics: the reference's ELL product (/root/reference/vexcl/spmat/hybrid_ell.inl:238-269: entries in storage order,
// products rounded before they are added, the scale applied to the sum); bit-identical to the fp32 CSR loop
// (spmat/csr.inl:163-170).  Compiled with -ffp-contract=off.
#include "common.hpp"
#include "grid_walk.hpp"
#include "storage.hpp"

#include <algorithm>
#include <cstdlib>

namespace vexhip {
namespace {

constexpr int G32_MAXT = 256;              // lanes of a workgroup at most: 1024 rows of a segment

// ZM: the addend of the result (walk.hpp add_addend): 0 none, 1 beta times the array zs ('+=': zs = y, beta = 1), 2 beta times x itself (from the registers)
template <int ZM, int STORE_AUX>
__global__ __launch_bounds__(G32_MAXT)             // 199 registers, two waves per SIMD (capped at 168 for three, with 15 spilled: the same times)
void sell8_grid_f32_kernel(const float *__restrict__ x, float *__restrict__ y, float alpha, const float *__restrict__ zs, float beta,
        const int *__restrict__ line_class, const unsigned char *__restrict__ table, const float *__restrict__ values, grid_dev gd)
{
    grid_walk<float, ZM, STORE_AUX, G32_MAXT, false>(x, y, alpha, zs, beta, line_class, table, values, gd, halo_dev(), 0ull);
}

} // namespace
} // namespace vexhip

using namespace vexhip;

extern "C" {

int vexhip_spmv_sell8v_grid_f32(int dev, void *stream, int64_t n, float alpha, int append, const float *values,
        const float *x, float *y, const vexhip_grid *g)
{ return grid_apply<float>(dev, stream, n, alpha, append, values, x, y, g); }

} // extern "C"

namespace vexhip {
// Planes per workgroup of the fp32 grid product (host arithmetic only) for workgroups of `threads` lanes on `tiles` tiles and nz planes.
// A workgroup is 1 .. 4 waves (four rows per lane) and a CU holds eight waves of this kernel.  Measured (ms by walk depth,
// profiles/r05_fp32_sizes.json): the best launch is ONE round of workgroups that just fills the CUs -- 384^3 (192 tiles x 2 waves)
// 96 / 77 / 64 / 48 planes = 0.120 / 0.103 / 0.136 / 0.115 (3 / 3.75 / 4.5 / 6 workgroups per CU), 500^3 125 / 100 / 63 = 0.217 /
// 0.304 / 0.228 (3.9 / 4.9 / 7.8), 512^3 128 / 86 / 64 = 0.214 / 0.244 / 0.259 (4 / 6 / 8) -- a little more than one round is the
// worst.  Workgroups of three and four waves (two per CU, 1.25 .. 2 tiles per CU) cannot do that: many short walks, at least
// eight per CU, as the fp64 grid product does it (640^3: 320 / 160 / 80 planes = 0.697 / 0.595 / 0.524).
static long long grid32_depth(long long cus, long long tiles, int threads, long long nz)
{
    const long long resident = std::max(1, 8 / (threads / 64));
    const long long cmax = std::max(1ll, nz / 16);
    long long chunks = std::min(cmax, resident * cus / tiles);
    if (resident < 3 || chunks < 1 || tiles * chunks * 20 < resident * cus * 17) {
        double best = 0;
        chunks = 1;
        for (long long c = 1; c <= cmax; ++c) {
            const long long per_cu = (tiles * c + cus - 1) / cus;
            if (per_cu < 8 && c < cmax) continue;
            const double est = (double)per_cu * (double)((nz + c - 1) / c + 6);
            if (best == 0 || est < best) { best = est; chunks = c; }
            if (per_cu > 24) break;
        }
    }
    return (nz + chunks - 1) / chunks;
}

// y = alpha A x + [zm 1: beta zs | zm 2: beta x] through the fp32 grid product (spmat.hip vexhip_spmat_apply_axpby_f32)
int grid_apply_axpby(int dev, void *stream, int64_t n, float alpha, int zm, const float *zs, float beta, const float *values,
        const float *x, float *y, const vexhip_grid *g)
{
    if (int rc = grid_check(g, n, values, x, y, true)) return rc;
    VEXHIP_REQUIRE(zm == 0 || zm == 2 || (zm == 1 && zs), "grid product: the addend must be a vector");
    VEXHIP_SET_DEVICE(dev);
    grid_dev gd = grid_launch(*g, n);
    const int threads = std::max(64, std::min(G32_MAXT, ((g->segment_rows + 3) / 4 + 63) / 64 * 64));
    gd.depth = (int)grid32_depth(std::max(1, info(dev).cus), gd.tiles, threads, gd.nz);       // this product's own walks, not the plan's (the fp64 kernel's)
    if (const char *e = env(ENV_VEXHIP_GRID32_DEPTH)) if (std::atoi(e) > 0) gd.depth = std::min(std::atoi(e), (int)gd.nz);
    VEXHIP_REQUIRE(((long long)gd.depth + 4) * gd.ny * gd.nx * 4 < (1ll << 32), "bad grid plan");
    unsigned grid;
    if (int rc = grid_workgroups(gd, gd.nz, &grid)) return rc;
    const unsigned char *tb = static_cast<const unsigned char *>(g->table);
    with_launch_forms(zm, g->store_policy, [&](auto ZM, auto AUX) {       // (the policy was read when the plan was made: grid.hip grid_fill_plan)
        sell8_grid_f32_kernel<ZM(), AUX()><<<grid, (unsigned)threads, 0, as_stream(stream)>>>(x, y, alpha, zs, beta, g->line_class, tb, values, gd);
    });
    VEXHIP_LAUNCH_CHECK();
    return 0;
}

} // namespace vexhip

VEXHIP_WARM_TU(grid32)
