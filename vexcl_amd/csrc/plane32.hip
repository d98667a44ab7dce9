// The PLANE product for fp32 (round 5): y (=|+=) alpha * A * x for value-coded SELL-512 storage with a slice dictionary whose
// diagonals are those of a 7-point operator on a grid with 512-point lines -- the storage, the plan and the walk of plane.hip,
// with FOUR rows per lane: a 512-point line of floats is 2 KB = 128 lanes x 16 bytes, so a workgroup is two waves, owns two
// adjacent grid lines and walks through the planes.  Every request is 16 bytes per lane as in the fp64 kernel (the march
// product, which float matrices took until now, moves x in 8-byte pairs through the LDS: 0.289 ms at 512^3, 0.46 of the HBM
// peak by the bytes that must move -- profiles/r05_fp32.json).  The +-512 / +-P neighbours of a lane's rows are quads the lane
// loaded itself; of the +-1 neighbours only the first and the last of the four rows look at another lane (one DPP shift
// each), the element beyond either end of a wave's 256 rows is a 4-byte load of lane 0 / lane 63.
// Semantics: the reference's ELL product (/root/reference/vexcl/spmat/hybrid_ell.inl:238-269: the row's entries in storage
// order, products rounded before they are added, the scale applied to the sum); results bit-identical to the CSR loop
// (spmat/csr.inl:163-170) in fp32.  Compiled with -ffp-contract=off.
#include "common.hpp"
#include "halo.hpp"
#include "walk.hpp"
#include "plane.hpp"
#include "storage.hpp"

#include <algorithm>
#include <cstdlib>

namespace vexhip {
namespace {

constexpr int P32_LANES = 128;             // lanes of a workgroup: 4 rows each
constexpr int P32_LINE_B = PL_ROWS * 4;    // bytes of a line

// HALO (round 6; halo.hpp, the PULL form only): the launch is one device's whole product step, as in grid.hip -- x and y addressed in
// the numbering of the STORED grid, the plane below z0 / above z1 - 1 read from the neighbour's x in place (H.lo / H.hi point at
// floats here), the two walks that touch a ghost plane dispatched last.
// ZM: the addend of the result (plane.hip): 0 none, 1 beta times the array zs ('+=': zs = y, beta = 1), 2 beta times x itself (from the registers)
template <int ZM, int STORE_AUX, bool HALO>
__device__ __forceinline__
void plane32_walk(const float *__restrict__ x, float *__restrict__ y, float alpha, const float *__restrict__ zs, float beta,
        const int *__restrict__ blocks, const char *__restrict__ pool, const int *__restrict__ deltas, const float *__restrict__ values,
        const plane_dev &pd, const halo_dev &H, [[maybe_unused]] const unsigned long long step)
{
    constexpr int TY = 2;
    // LDS: per diagonal code its position (x 4), the value table, and the decoded values of the OTHER block, lane-private
    // ([position * 4 + row][lane]; row 28 takes what padding "writes")
    __shared__ int s_slot[256];
    __shared__ float s_value[256];
    __shared__ float s_other[29][P32_LANES];

    const int t = threadIdx.x;
    int y0, zc, z, zend_;
    if (!plane_tile(pd, blockIdx.x, TY, y0, zc)) return;           // the whole workgroup
    [[maybe_unused]] bool ghost_bad = false;
    [[maybe_unused]] __shared__ int s_flag;
    if constexpr (HALO) {
        const int nch = (H.z1 - H.z0 + pd.depth - 1) / pd.depth;
        const int c = nch > 1 ? (zc + 1) % nch : 0;               // the first and the last walk touch a ghost plane: dispatched behind the others
        z = H.z0 + c * pd.depth; zend_ = z + pd.depth < H.z1 ? z + pd.depth : H.z1;
        if (zc >= nch || z >= zend_) return;
        ghost_bad = !halo_wait(H, step, H.lo && z == H.z0, H.hi && zend_ == H.z1, &s_flag);
    } else if (!plane_chunk(pd, zc, z, zend_)) return;
    const int zend = zend_;
    const int ny = pd.ny;
    // HALO: the lines of x and y that exist are those of the planes [z0, z1)
    const int line_lo = HALO ? H.z0 * ny : 0;
    const int nslices = HALO ? H.z1 * ny : (int)pd.nslices, xlines = HALO ? H.z1 * ny : (int)pd.xlines;
    const unsigned lane_b = 16u * (unsigned)t;
    const int edge_b = edge_offset(t, 4);

    for (int i = t; i < 256; i += P32_LANES) { s_slot[i] = 4 * position_of(deltas[i], pd.far); s_value[i] = values[i]; }
    __syncthreads();

    // a dictionary block, or a class of the matrix stored by grid line (grid.hip) -> values (into s_other) and validity (returned)
    const int wp = (pd.w + 1) >> 1;
    auto decode = [&](int blk) -> unsigned {
        return pd.pitch > 0 ? decode_table<false>(pool + (long long)blk * 7 * pd.pitch + 4 * t, pd.pitch, s_value, s_other, t)
                            : decode_block(pool, blk, pd.w, wp, s_slot, s_value, s_other, t);
    };

    const int hot = pd.hot;
    float aH[7][4];                             // the hot block: values ...
    unsigned long long mH[7][4];                // ... and the lanes with an entry, per position and row.  (56 scalar registers: the
    // compiler keeps some of them in lanes of vector registers, 40 v_readlane per line.  Measured at 512^3: these masks 0.2066 ms,
    // the lane's own 28 validity bits in a vector register 0.2085, NO masks at all 0.2035 -- the product is not bound by them.)
    take_hot(decode(hot), s_other, t, aH, mH);
    unsigned bitsO = 0;
    int other = -1;                             // what s_other holds now is the hot block's: never asked for
    const line_terms<float, 29, P32_LANES> terms = {aH, mH, s_other, hot, other, bitsO, t, alpha, beta};

    // clamped requests (plane.hpp); the ghost planes in front of them
    const clamped_requests<float> own = {x, zs, ny, y0, line_lo, xlines, nslices, HALO ? (long long)xlines * PL_ROWS - 1 : pd.x_last, lane_b, edge_b};
    auto ld = [&](int zz, int l) -> f4 {
        if constexpr (HALO) {
            const int li = zz * ny + (y0 - 1 + l);                                   // uniform
            if (li < line_lo || li >= xlines) {
                const bool below = li < line_lo;
                const int gl = below ? li - (line_lo - ny) : li - xlines;            // line of the ghost plane
                const float *g = reinterpret_cast<const float *>(below ? H.lo : H.hi);
                f4 r = {0.0f, 0.0f, 0.0f, 0.0f};
                if (!g || gl < 0 || gl >= ny || l == 0 || l == TY + 1) return r;     // no neighbour there / not the adjacent plane / the line above or below the tile IN a ghost plane: never referenced
                if (ghost_bad) { r.x = r.y = r.z = r.w = __builtin_nanf(""); return r; }
                return *reinterpret_cast<const f4u *>(reinterpret_cast<const char *>(g + (long long)gl * PL_ROWS) + lane_b);
            }
        }
        return own.ld(zz, l);
    };
    auto edge = [&](int zz, int l) -> float {
        if constexpr (HALO) {
            const int li = zz * ny + (y0 - 1 + l);
            if (li < line_lo || li >= xlines) return 0.0f;                           // the +-1 neighbours inside a ghost line: no row of this device has them
        }
        return own.edge(zz, l);
    };
    auto yold = [&](int zz, int l) -> f4 { return own.yold(zz, l); };

    // ---- the registers of the walk (walk.hpp), filled for plane z ----
    f4 Cs[4][TY], Hs[2][2], Yo[TY];
    float Es[2][TY];
    const unsigned plane_b32 = (unsigned)ny * (unsigned)P32_LINE_B;    // bytes from a line to the same line of the next plane
    const int z_first = z;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(x + ((long long)z_first * ny + (y0 - 1)) * PL_ROWS), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(y + ((long long)z_first * ny + y0) * PL_ROWS, 0, -1, 0x00020000);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(ZM == 1 ? zs : x) + ((long long)z_first * ny + y0) * PL_ROWS, 0, -1, 0x00020000);
    fill_registers<ZM>(Cs, Hs, Es, Yo, z, true, ld, edge, yold);

    const int zh = fast_limit(zend, ny, y0, TY, xlines, nslices, ZM == 1);

    while (z < zend) {
        unsigned long long use_hot[TY];
        const int run = fast_run(blocks, ny, y0, TY, z, zh, hot, other, t, use_hot);
        if (run >= 4) {
            // xo: plane z + 2, the line above the tile; yo: plane z, the tile's first line; both relative to the workgroup's first plane
            unsigned xo = (unsigned)((z + 2 - z_first) * plane_b32), yo = (unsigned)((z - z_first) * plane_b32);
            auto fast_step = [&](f4 (&P)[TY], f4 (&C)[TY], f4 (&N)[TY], f4 (&Hl)[2], float (&E)[TY]) {
                f4 o[TY];
#pragma unroll
                for (int l = 0; l < TY; ++l) {
                    float xs[4][7], s[4] = {};
                    stencil_x(P, C, N, Hl, E, l, xs);
                    if (use_hot[l] & 1ull) hot_sums(s, aH, mH, xs); else other_sums(s, s_other, t, bitsO, xs);      // uniform
                    o[l] = add_addend<ZM>(alpha, s, beta, Yo[l], C[l]);
                }
#pragma unroll
                for (int l = 0; l < TY; ++l) use_hot[l] >>= 1;
#pragma unroll
                for (int l = 0; l < TY; ++l) store16<STORE_AUX>(o[l], ry, (int)lane_b, yo + l * P32_LINE_B);       // written once, not read again by this kernel
                if (ZM == 1) {
#pragma unroll
                    for (int l = 0; l < TY; ++l) Yo[l] = load16<float>(rz, (int)lane_b, yo + plane_b32 + l * P32_LINE_B);
                }
                Hl[0] = load16<float>(rx, (int)lane_b, xo);
                Hl[1] = load16<float>(rx, (int)lane_b, xo + (TY + 1) * P32_LINE_B);
#pragma unroll
                for (int l = 0; l < TY; ++l) {
                    P[l] = load16<float>(rx, (int)lane_b, xo + plane_b32 + (l + 1) * P32_LINE_B);
                    E[l] = load_edge<float>(rx, edge_b + 4, xo + (l + 1) * P32_LINE_B - 4u);
                }
                xo += plane_b32; yo += plane_b32; ++z;
            };
            for (int g = run >> 2; g > 0; --g) fast_group(fast_step, Cs, Hs, Es);
            if (run == 64) continue;                                      // look again: the run may go on
        }
        if (z >= zend) break;
        // ---- a slow step: a line needs another block decoded, the last planes (clamped requests), the ragged last plane, what
        // a run leaves over after its groups of four ----
#pragma unroll
        for (int l = 0; l < TY; ++l) {
            const int li = z * ny + (y0 + l);
            if (li < nslices) {                                           // uniform
                const f4 o = line_result<ZM>(terms, __builtin_amdgcn_readfirstlane(blocks[li]), decode, Cs, Hs, Es, Yo, l);
                *reinterpret_cast<f4u *>(reinterpret_cast<char *>(y + (long long)li * PL_ROWS) + lane_b) = o;
            }
        }
        rotate_by_copy<ZM>(Cs, Hs, Es, Yo, z, true, ld, edge, yold);
        ++z;
    }
}

template <int ZM, int STORE_AUX, bool HALO = false>
__global__ __launch_bounds__(P32_LANES)
void sell8_plane_f32_kernel(const float *__restrict__ x, float *__restrict__ y, float alpha, const float *__restrict__ zs, float beta,
        const int *__restrict__ blocks, const char *__restrict__ pool, const int *__restrict__ deltas, const float *__restrict__ values,
        plane_dev pd, halo_dev H)
{
    if constexpr (!HALO) {
        plane32_walk<ZM, STORE_AUX, false>(x, y, alpha, zs, beta, blocks, pool, deltas, values, pd, H, 0ull);
    } else {
        const unsigned long long step = *H.step;
        halo_announce(H, step);
        plane32_walk<ZM, STORE_AUX, true>(x, y, alpha, zs, beta, blocks, pool, deltas, values, pd, H, step);
        halo_finish(H, step);
    }
}

} // namespace
} // namespace vexhip

using namespace vexhip;

extern "C" {

// Planes per workgroup of the fp32 plane product (host arithmetic only, exported so that the choice can be checked without a device):
// a workgroup is two waves and six of them fit a CU: about two rounds of workgroups (512^3: depth 512 / 256 / 128 / 64 / 43 / 32 / 16 =
// 0.315 / 0.239 / 0.214 / 0.213 / 0.207 / 0.214 / 0.221 ms, profiles/r05_fp32_plane.txt); no walk shorter than 8 planes.  The kernel
// forms byte offsets inside a walk in 32 bits: the depth is halved until (depth + 4) planes of 2048-byte lines fit -- checked on the
// depth chosen HERE, not on the fp64 plan's (round 6: ny = 8192, nz = 256 passed the fp64 check at depth 64 and walked 256 planes).
// 0: no depth fits.
int64_t vexhip_sell8_plane_f32_depth(int cus, int64_t lines_per_plane, int64_t planes)
{
    if (lines_per_plane < 2 || planes < 1) return 0;
    const long long c = std::max(1, cus), tiles = lines_per_plane / 2;
    const long long chunks = std::max(1ll, std::min<long long>(planes / 8, (12 * c + tiles / 2) / tiles));
    long long depth = (planes + chunks - 1) / chunks;
    if (const char *e = env(ENV_VEXHIP_PLANE32_DEPTH)) if (std::atoi(e) > 0) depth = std::min<long long>(std::atoi(e), planes);
    while ((depth + 4) * lines_per_plane * P32_LINE_B >= (1ll << 32) && depth > 8) depth = (depth + 1) / 2;
    return (depth + 4) * lines_per_plane * P32_LINE_B < (1ll << 32) ? depth : 0;
}

int vexhip_spmv_sell8v_plane_f32_i32(int dev, void *stream, int64_t n, float alpha, int append, int64_t w, const void *pool,
        const int32_t *blocks, const int32_t *deltas, const float *values, const float *x, float *y, const vexhip_plane *plane)
{ return plane_apply<float>(dev, stream, n, alpha, append, w, pool, blocks, deltas, values, x, y, plane); }

} // extern "C"

namespace vexhip {
// the two launches below: the product on a matrix of n rows, or (HALO; else H is not looked at) one device's step, which has '=' and '+=' only
template <bool HALO>
static int plane32_run(int dev, hipStream_t s, int64_t n, float alpha, int zm, const float *zs, float beta, int64_t w, const void *pool, const int32_t *blocks,
        const int32_t *deltas, const float *values, const float *x, float *y, const vexhip_plane *plane, const halo_dev &H)
{
    // (x and y may start at any element: 16-byte requests at 4-byte addresses are served, a matrix stored by grid line has no
    //  other product to fall back on)
    if (int rc = plane_check(plane, 2, 0, n, w, pool && blocks && deltas && values, x, y, false)) return rc;
    if (HALO) { if (int rc = check_halo_step(H, plane->planes, (long long)plane->lines_per_plane * PL_ROWS, true)) return rc; }
    VEXHIP_REQUIRE(zm == 0 || (zm == 2 && !HALO) || (zm == 1 && zs), "plane product: the addend must be a vector");
    VEXHIP_SET_DEVICE(dev);
    const int planes = HALO ? H.z1 - H.z0 : plane->planes;      // the depth is chosen for the planes THIS launch walks
    const int depth = (int)vexhip_sell8_plane_f32_depth(std::max(1, info(dev).cus), plane->lines_per_plane, planes);
    VEXHIP_REQUIRE(depth > 0, "fp32 plane product: a walk of this grid does not fit 32-bit byte offsets");
    const plane_dev pd = plane_launch(*plane, n, w, 2, depth);
    unsigned grid;
    if (int rc = plane_workgroups(pd, planes, 0, 0, &grid)) return rc;
    const long long off = HALO ? (long long)H.z0 * pd.far : 0;      // a step: the kernel addresses x and y in the numbering of the stored grid
    const char *cpool = static_cast<const char *>(pool);
    if constexpr (HALO) {       // '=' and '+=' only; the stores of a step always take policy 1 (immediate 18)
        auto kernel = zm ? sell8_plane_f32_kernel<1, 18, true> : sell8_plane_f32_kernel<0, 18, true>;
        kernel<<<grid, P32_LANES, 0, s>>>(x - off, y - off, alpha, zs ? zs - off : nullptr, beta, blocks, cpool, deltas, values, pd, H);
    } else {
        // VEXHIP_PLANE_STORE is read HERE, at the launch (the other three products read it when the plan is made); unset: policy 1, whatever
        // the plan holds for the fp64 kernel
        int store_kind = 1;
        if (const char *e = env(ENV_VEXHIP_PLANE_STORE)) store_kind = std::max(0, std::min(3, std::atoi(e)));
        with_launch_forms(zm, store_kind, [&](auto ZM, auto AUX) {
            sell8_plane_f32_kernel<ZM(), AUX()><<<grid, P32_LANES, 0, s>>>(x, y, alpha, zs, beta, blocks, cpool, deltas, values, pd, H);
        });
    }
    VEXHIP_LAUNCH_CHECK();
    return 0;
}

// y = alpha A x + [zm 1: beta zs | zm 2: beta x] through the fp32 plane product (spmat.hip vexhip_spmat_apply_axpby_f32)
int plane_apply_axpby(int dev, void *stream, int64_t n, float alpha, int zm, const float *zs, float beta, int64_t w, const void *pool,
        const int32_t *blocks, const int32_t *deltas, const float *values, const float *x, float *y, const vexhip_plane *plane)
{ return plane32_run<false>(dev, as_stream(stream), n, alpha, zm, zs, beta, w, pool, blocks, deltas, values, x, y, plane, halo_dev()); }

// One device's product step in one launch for a float matrix on 512-point lines (halo.hpp, the pull form): the fp32 plane product over
// the planes [H.z0, H.z1) of the stored grid of n_ext rows; x and y are the device's own segments.
int plane_apply_halo(int dev, hipStream_t s, int64_t n_ext, float alpha, int append, int64_t w, const void *pool, const int32_t *blocks,
        const int32_t *deltas, const float *values, const float *x, float *y, const vexhip_plane *plane, halo_dev H)
{ return plane32_run<true>(dev, s, n_ext, alpha, append ? 1 : 0, append ? y : nullptr, append ? 1.0f : 0.0f, w, pool, blocks, deltas, values, x, y, plane, H); }
} // namespace vexhip

VEXHIP_WARM_TU(plane32)
