// The PLANE product (round 4): y (=|+=) alpha * A * x for value-coded SELL-512 storage with a slice dictionary whose diagonals
// are those of a 7-point operator on a grid with 512-point lines -- {0, +-1, +-512, +-P}, P = 512 * (lines per plane).
// This is the headline kernel of vex::SpMat on the 512^3 Poisson matrix; semantics are the reference's ELL product
// (/root/reference/vexcl/spmat/hybrid_ell.inl:238-269: the row's entries in storage order, products rounded before they are
// added, the scale applied to the sum), results bit-identical to the CSR loop (spmat/csr.inl:163-170).
//
// What it does differently from the march product (sell8.hip), and why (profiles/r04_pm_proto.json):
//   * the march product walks a run of consecutive slices and keeps the +-512 window in an LDS ring; the +-P diagonals are
//     two more 16-byte requests per lane and slice that other workgroups satisfy from HBM a second and third time whenever
//     the three touches of a line do not meet in one L2 (1.21 x the read traffic, L2 hit 58 %), and every x element crosses
//     the LDS (55 % busy, 39 % of it bank conflicts).
//   * here a workgroup owns TWO adjacent grid lines and walks through the PLANES.  Lane t owns rows 2t, 2t + 1 of both lines in
//     every plane, so the +-512 neighbours (the line above / below) and the +-P neighbours (the same line one plane back /
//     ahead) of its rows are 16-byte pairs THE SAME LANE loaded itself: they stay in registers.  Only the +-1 neighbours
//     belong to other lanes: one DPP wave shift each; the element beyond either end of a wave's 128 rows is a scalar load.
//     No LDS, no barrier.  Per plane step a lane requests 4 pairs (two centre lines, the halo line above and below) and stores
//     2: every x line is requested twice instead of three times, and the halo lines are the centre lines of the neighbouring
//     tile, which the same XCD works on at the same plane (tiles are dealt to XCDs in contiguous ranges).
//   * the matrix enters as it does in the march product: 4 bytes per slice (its dictionary block) + the pool of distinct code
//     blocks.  A lane decodes a block into values and validity of its two rows at the seven diagonal positions; the block
//     that most slices use (the plan's `hot` block) keeps them in registers with scalar lane masks, one other block sits
//     next to it and is re-decoded when a line needs a third one (boundary planes / lines: < 1/16 of the slices, the plan
//     checks).  Rows need not be pair-aligned: x comes by diagonal position, not by ELL column.
// The plan (vexhip_sell8_plane_plan) validates every dictionary block on the host -- diagonals in the set, positions ascending
// within a row (so that position order IS storage order) -- and declines otherwise; the march and pair products remain.
// Compiled with -ffp-contract=off.
#include "common.hpp"
#include "walk.hpp"
#include "halo.hpp"
#include "plane.hpp"
#include "storage.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace vexhip {
namespace {

constexpr int PL_LINE_B = PL_ROWS * 8;             // bytes of a line

// One workgroup's piece of a push: elements [j * per, (j + 1) * per) of the rank's first (down) or last boundary plane of x go into
// the neighbour's window in 16-byte pieces; the workgroup is counted (if `counted`), and the one that brings the count to `target`
// raises `arrive` at the neighbour.  s_flag: one LDS word of the caller.
__device__ __forceinline__ void push_piece(const double *__restrict__ x, int far, const halo_dev &H, unsigned long long step, bool down, int j,
        int per, unsigned target, bool counted, int *s_flag)
{
    const int t = threadIdx.x;
    if (t == 0) *s_flag = spin_until(down ? H.sent_lo : H.sent_hi, step - 1ull, H.err, H.ticks, 0) ? 1 : 0;   // the neighbour has read the previous share
    __syncthreads();
    if (!*s_flag) return;                                                    // uniform; a neighbour that does not answer is not written to
    const double *src = x + (down ? (long long)H.z0 * far : (long long)(H.z1 - 1) * far);
    double *dst = down ? H.dst_lo : H.dst_hi;
    const int i0 = j * per, i1 = i0 + per < H.halo ? i0 + per : H.halo;
    for (int i = i0 + 2 * t; i < i1; i += 512)
        *reinterpret_cast<d2 *>(dst + i) = *reinterpret_cast<const d2 *>(src + i);
    // The window is UNCACHED memory (here and through the peer mapping): its stores go past every cache, and a wave's
    // stores have been performed at the destination once its store counter is back at zero -- so the flag may follow
    // behind `s_waitcnt vmcnt(0)` + a barrier + a relaxed count of the workgroups, with NO release fence.  A fence at
    // agent or system scope writes back the XCD's L2, which at this moment is full of the product's freshly stored y:
    // with ACQ_REL counts and a system fence in front of the flag the push of 4 MB took ~50 us of a 120 us step
    // (tools/r05_dist_step.py, VEXHIP_HALO_NO_PUSH against the default; profiles/r05_dist_step_*.json).
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0 && counted) {
        unsigned *cnt = H.done + (down ? 1 : 2);
        const unsigned old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1u == target) {
            __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (H.release) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");       // a window in cached memory (diagnostic): the model-correct hand-off
            __hip_atomic_store(down ? H.peer_arrive_lo : H.peer_arrive_hi, step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// HALO (round 5, halo.hpp): the launch is one rank's whole product step.  x and y are addressed in the numbering of the STORED
// grid, whose plane z0 - 1 / z1 (if the rank has a neighbour there) is a ghost plane: its lines are read from the rank's window
// (H.lo / H.hi) behind the owner's `arrive` flag; the first workgroups of the launch copy the rank's own boundary planes to the
// neighbours.  (`consumed` is raised and the step number advanced by halo_signal_kernel behind this launch: a kernel boundary
// orders every workgroup's reads of the ghost planes before the owners may overwrite them.)
// (the walk of one workgroup; the kernel below adds what follows it in a HALO launch)
// ZM, the addend of the result (round 6): 0 none (y = alpha A x); 1 an array `zs` scaled by beta (y = alpha A x + beta zs: '+=' is zs = y,
// beta = 1; a residual b - A x is zs = b, alpha = -1); 2 beta times x ITSELF, taken from the registers that hold the centre lines (y = x + 2 A x
// moves not a byte more than y = A x).
// FLAT (round 6): no block has an entry at +-512 -- a 5-point operator on a 2-D grid whose rows are virtual 512-point lines (grid.hip
// grid_diagonals): the lines above / below the tile are never requested (two of a step's six 16-byte requests).  A template flag: the
// instantiations of the 3-D operators -- the headline's -- are what they were.
template <int TY, int ZM, int STORE_AUX, bool HALO, bool FLAT = false>
__device__ __forceinline__
void plane_walk(const double *__restrict__ x, double *__restrict__ y, double alpha, const double *__restrict__ zs, double beta,
        const int *__restrict__ blocks, const char *__restrict__ pool, const int *__restrict__ deltas, const double *__restrict__ values,
        const plane_dev &pd, const halo_dev &H, [[maybe_unused]] const unsigned long long step_in)
{
    // LDS: per diagonal code its position (x 2), the value table, and the decoded values of the OTHER block, lane-private
    // ([position * 2 + row][lane]: consecutive lanes, consecutive 8-byte words -- conflict-free; row 14 takes what padding
    // "writes").  33 KiB: four workgroups per CU.
    __shared__ int s_slot[256];
    __shared__ double s_value[256];
    __shared__ double s_other[15][256];

    const int t = threadIdx.x;
    unsigned b = blockIdx.x;
    [[maybe_unused]] unsigned long long step = 0;
    [[maybe_unused]] __shared__ int s_flag[2];
    [[maybe_unused]] unsigned long long dbg_t0 = 0, dbg_flag = 0, dbg_data = 0;
    if constexpr (HALO) {
        if (H.debug) dbg_t0 = wall_clock64();
        step = step_in;
        halo_announce(H, step);
        const unsigned npush = H.pull ? 0u : (H.dst_lo ? (unsigned)H.push_blocks : 0u) + (H.dst_hi ? (unsigned)H.push_blocks : 0u);
        if (b < npush) {
            // ---- a dedicated push workgroup: every one of the push_blocks per side is counted, whether a piece is left for it or not ----
            const bool down = H.dst_lo && b < (unsigned)H.push_blocks;           // the FIRST plane goes to the lower neighbour
            const unsigned j = down ? b : b - (H.dst_lo ? (unsigned)H.push_blocks : 0u);
            const int per = ((H.halo + H.push_blocks - 1) / H.push_blocks + 511) / 512 * 512;
            push_piece(x, pd.far, H, step, down, (int)j, per, (unsigned)H.push_blocks, true, &s_flag[0]);
            if (H.debug && t == 0) { unsigned long long *d = H.debug + 6ull * blockIdx.x; d[0] = dbg_t0; d[1] = 0; d[2] = 0; d[3] = wall_clock64(); d[4] = ~0ull; d[5] = down ? 0ull : 1ull; }
            return;
        }
        b -= npush;
    }
    int y0, zc, z, zend;
    if (!plane_tile(pd, b, TY, y0, zc)) return;                     // the whole workgroup
    [[maybe_unused]] bool second = false;
    [[maybe_unused]] int z2 = 0, zend2 = 0;
    if constexpr (HALO) {
        // chunks of the planes [z0, z1): the planes next to a ghost plane form SHORT chunks of their own, dispatched behind the
        // main chunks -- they wait for the neighbour's share and read it from uncached memory (slow: few requests in flight)
        // while the main chunks, which never touch a ghost plane, stream the bulk of the strip
        const int mid0 = H.z0 + H.lo_planes, mid1 = H.z1 - H.hi_planes;
        const int nmain = (mid1 - mid0 + pd.depth - 1) / pd.depth;
        if (zc < nmain) { z = mid0 + zc * pd.depth; zend = z + pd.depth < mid1 ? z + pd.depth : mid1; }
        else if (H.hi_planes && zc == nmain) { z = mid1; zend = H.z1; }
        else if (H.lo_two_pass && mid0 - H.z0 >= 2) {
            // the chunk next to the LOWER ghost plane needs that plane for its FIRST plane: it walks the planes above it first and
            // comes back for plane z0 in a second pass, when the neighbour's share has arrived (the push of a plane takes 45 us and
            // more: tools/r05_halo_timeline.py) -- one plane of work behind the flag instead of the whole chunk
            z = H.z0 + 1; zend = mid0; second = true; z2 = H.z0; zend2 = H.z0 + 1;
        } else { z = H.z0; zend = mid0; }
        if (z >= zend) return;
    } else if (!plane_chunk(pd, zc, z, zend)) return;
    [[maybe_unused]] const int z_first0 = z, mid_end = zend;
    if constexpr (HALO) {
        // push_blocks == 0: NO dedicated push workgroups -- the first 2 x 256 product workgroups each copy 1024 elements of a
        // boundary plane before they start their walk.  Stores into the uncached window complete one after the other per wave
        // (32 of them per lane took the 32 dedicated workgroups 45 us on some boxes and 84 us on others: tools/r05_halo_timeline.py);
        // two per lane from 2048 waves at once are done in a few microseconds, and the neighbours' ghost flags rise that early.
        if (!H.pull && H.push_blocks == 0 && b < 512u) {
            const bool down = b < 256u;
            double *dst = down ? H.dst_lo : H.dst_hi;
            if (dst) {                                                           // uniform; only the workgroups that have a piece are counted
                const int per = ((H.halo + 255) / 256 + 511) / 512 * 512, j = (int)(b & 255u);
                push_piece(x, pd.far, H, step, down, j, per, (unsigned)((H.halo + per - 1) / per), j * per < H.halo, &s_flag[0]);
                __syncthreads();                                                 // s_flag is used again by the ghost waits
            }
        }
    }
    const int ny = pd.ny;
    const unsigned lane_b = 16u * (unsigned)t;
    const int edge_b = edge_offset(t, 8);

    s_slot[t] = 2 * position_of(deltas[t], pd.far); s_value[t] = values[t];
    __syncthreads();

    // a dictionary block, or a class of the matrix stored by grid line (grid.hip) -> values (into s_other) and validity (returned)
    const int wp = (pd.w + 1) >> 1;
    auto decode = [&](int blk) -> unsigned {
        return pd.pitch > 0 ? decode_table<false>(pool + (long long)blk * 7 * pd.pitch + 2 * t, pd.pitch, s_value, s_other, t)
                            : decode_block(pool, blk, pd.w, wp, s_slot, s_value, s_other, t);
    };

    const int hot = pd.hot;
    double aH[7][2];                            // the hot block: values ...
    unsigned long long mH[7][2];                // ... and the lanes with an entry, per position and row
    take_hot(decode(hot), s_other, t, aH, mH);
    unsigned bitsO = 0;
    int other = -1;                             // what s_other holds now is the hot block's: never asked for
    const line_terms<double, 15, 256> terms = {aH, mH, s_other, hot, other, bitsO, t, alpha, beta};

    // clamped requests (plane.hpp).  HALO: the lines of x and y that exist are those of the planes [z0, z1); the plane below / above
    // them is the ghost plane
    const int line_lo = HALO ? H.z0 * ny : 0, line_hi = HALO ? H.z1 * ny : (int)pd.xlines;       // x: [line_lo, line_hi)
    const int yline_hi = HALO ? H.z1 * ny : (int)pd.nslices;
    const clamped_requests<double> own = {x, zs, ny, y0, line_lo, line_hi, yline_hi, HALO ? (long long)line_hi * PL_ROWS - 1 : pd.x_last, lane_b, edge_b};
    [[maybe_unused]] bool got_lo = false, got_hi = false, ghost_bad = false;
    auto ld = [&](int zz, int l) -> d2 {
        if constexpr (HALO) {
            const int li = zz * ny + (y0 - 1 + l);                                   // uniform
            if (li < line_lo || li >= line_hi) {
                const bool below = li < line_lo;
                const int gl = below ? li - (line_lo - ny) : li - line_hi;           // line of the ghost plane
                const double *g = below ? H.lo : H.hi;
                d2 r = {0.0, 0.0};
                if (!g || gl < 0 || gl >= ny || l == 0 || l == TY + 1) return r;     // no neighbour there / not the adjacent plane / the line above or below the tile IN a ghost plane: never referenced by an entry
                bool &got = below ? got_lo : got_hi;
                if (!got && H.pull != 2) {
                    // the first line of this ghost plane the workgroup needs: has the owner's share of THIS product arrived?
                    // (PULL: is the owner's x final?  pull == 2: the host has ordered the streams, there is nothing to wait for)
                    if (t == 0) s_flag[below ? 0 : 1] = spin_until(below ? H.arrive_lo : H.arrive_hi, step, H.err, H.ticks, H.acquire) ? 1 : 0;
                    __syncthreads();
                    if (!s_flag[below ? 0 : 1]) ghost_bad = true;
                    // (no fence per lane: the ghost planes are UNCACHED memory -- nothing of them is ever held in a cache -- and
                    //  lane 0 has acquired at system scope inside spin_until in front of the barrier; a system-scope acquire by
                    //  every lane of every workgroup doubled the time of the whole product: 55 -> 119 us)
                    got = true;
                    if (H.debug && !dbg_flag) dbg_flag = wall_clock64();
                }
                if (ghost_bad) { r.x = r.y = __builtin_nan(""); return r; }         // never numbers from stale ghosts (comm.hip)
                if (H.debug && !dbg_data) {                                          // diagnostics: how long the first ghost line takes to arrive
                    const d2 v = *reinterpret_cast<const d2 *>(reinterpret_cast<const char *>(g + (long long)gl * PL_ROWS) + lane_b);
                    asm volatile("s_waitcnt vmcnt(0)" :: "v"(v.x), "v"(v.y) : "memory");
                    dbg_data = wall_clock64();
                    return v;
                }
                return *reinterpret_cast<const d2 *>(reinterpret_cast<const char *>(g + (long long)gl * PL_ROWS) + lane_b);
            }
        }
        return own.ld(zz, l);
    };
    auto edge = [&](int zz, int l) -> double {
        if constexpr (HALO) {
            const int li = zz * ny + (y0 - 1 + l);
            if (li < line_lo || li >= line_hi) return 0.0;                           // the +-1 neighbours inside a ghost line: no row of this rank has them
        }
        return own.edge(zz, l);
    };
    auto yold = [&](int zz, int l) -> d2 { return own.yold(zz, l); };

    // ---- the registers of the walk (walk.hpp), filled for plane z; which block a line uses is known for up to 64 planes ahead
    // (fast_run: one look at blocks[] per entry) ----
    constexpr int NPASS = HALO ? 2 : 1;
    for (int pass = 0; pass < NPASS; ++pass) {
    if constexpr (HALO) if (pass == 1) { if (!second) break; z = z2; zend = zend2; }
    d2 Cs[4][TY], Hs[2][2], Yo[TY];
    double Es[2][TY];
    const unsigned plane_b32 = (unsigned)ny * (unsigned)PL_LINE_B;     // bytes from a line to the same line of the next plane (the plan: (depth + 4) of them < 2^32)
    const int z_first = z;
    // buffer resources of the fast loop: x from the line above the tile in the workgroup's first plane, y from the tile's first
    // line in that plane (no range check: the fast loop only runs where every request lies inside the arrays)
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double *>(x + ((long long)z_first * ny + (y0 - 1)) * PL_ROWS), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(y + ((long long)z_first * ny + y0) * PL_ROWS, 0, -1, 0x00020000);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(ZM == 1 ? zs : x) + ((long long)z_first * ny + y0) * PL_ROWS, 0, -1, 0x00020000);
    fill_registers<ZM>(Cs, Hs, Es, Yo, z, !FLAT, ld, edge, yold);

    const int zh = fast_limit(zend, ny, y0, TY, line_hi, yline_hi, ZM == 1);

    while (z < zend) {
        unsigned long long use_hot[TY];
        const int run = fast_run(blocks, ny, y0, TY, z, zh, hot, other, t, use_hot);
        if (run >= 4) {
            // Buffer addressing: a resource per array (scalar), the lane's byte offset (ONE vector register for the whole
            // kernel) and a scalar offset that moves with the planes -- no 64-bit vector address arithmetic, which cost a dozen
            // registers and, re-using the registers of requests still in flight, forced early waits.  xo: plane z + 2, the
            // line above the tile; yo: plane z, the tile's first line; both relative to the workgroup's first plane.
            unsigned xo = (unsigned)((z + 2 - z_first) * plane_b32), yo = (unsigned)((z - z_first) * plane_b32);
            auto fast_step = [&](d2 (&P)[TY], d2 (&C)[TY], d2 (&N)[TY], d2 (&Hl)[2], double (&E)[TY]) {
                d2 o[TY];
#pragma unroll
                for (int l = 0; l < TY; ++l) {
                    double xs[2][7], s[2] = {};
                    stencil_x(P, C, N, Hl, E, l, xs);
                    if (use_hot[l] & 1ull) hot_sums(s, aH, mH, xs); else other_sums(s, s_other, t, bitsO, xs);      // uniform
                    o[l] = add_addend<ZM>(alpha, s, beta, Yo[l], C[l]);
                }
#pragma unroll
                for (int l = 0; l < TY; ++l) use_hot[l] >>= 1;
#pragma unroll
                for (int l = 0; l < TY; ++l) store16<STORE_AUX>(o[l], ry, (int)lane_b, yo + l * PL_LINE_B);       // written once, not read again by this kernel
                if (ZM == 1) {
#pragma unroll
                    for (int l = 0; l < TY; ++l) Yo[l] = load16<double>(rz, (int)lane_b, yo + plane_b32 + l * PL_LINE_B);
                }
                if constexpr (!FLAT) {
                    Hl[0] = load16<double>(rx, (int)lane_b, xo);
                    Hl[1] = load16<double>(rx, (int)lane_b, xo + (TY + 1) * PL_LINE_B);
                }
#pragma unroll
                for (int l = 0; l < TY; ++l) {
                    P[l] = load16<double>(rx, (int)lane_b, xo + plane_b32 + (l + 1) * PL_LINE_B);
                    E[l] = load_edge<double>(rx, edge_b + 8, xo + (l + 1) * PL_LINE_B - 8u);
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
            if (li < yline_hi) {                                          // uniform
                const d2 o = line_result<ZM>(terms, __builtin_amdgcn_readfirstlane(blocks[li]), decode, Cs, Hs, Es, Yo, l);
                __builtin_nontemporal_store(o, reinterpret_cast<d2 *>(reinterpret_cast<char *>(y + (long long)li * PL_ROWS) + lane_b));
            }
        }
        rotate_by_copy<ZM>(Cs, Hs, Es, Yo, z, !FLAT, ld, edge, yold);
        ++z;
    }
    }       // pass
    if constexpr (HALO) {
        if (H.debug && t == 0) {
            unsigned long long *d = H.debug + 6ull * blockIdx.x;
            d[0] = dbg_t0; d[1] = dbg_flag; d[2] = dbg_data; d[3] = wall_clock64(); d[4] = (unsigned long long)(second ? z2 : z_first0); d[5] = (unsigned long long)(second ? mid_end : zend);
        }
    }
}

#ifndef VEXHIP_HALO_WAVES
#define VEXHIP_HALO_WAVES 2
#endif
template <int TY, int ZM, int STORE_AUX, bool HALO = false, bool FLAT = false>
__global__ __launch_bounds__(256, (TY == 2 && !HALO) ? 4 : (HALO ? VEXHIP_HALO_WAVES : 2))       // (HALO: a few registers more than 128)
void sell8_plane_kernel(const double *__restrict__ x, double *__restrict__ y, double alpha, const double *__restrict__ zs, double beta,
        const int *__restrict__ blocks, const char *__restrict__ pool, const int *__restrict__ deltas, const double *__restrict__ values,
        plane_dev pd, halo_dev H)
{
    if constexpr (!HALO) {
        plane_walk<TY, ZM, STORE_AUX, false, FLAT>(x, y, alpha, zs, beta, blocks, pool, deltas, values, pd, H, 0ull);
    } else {
        const unsigned long long step = *H.step;
        plane_walk<TY, ZM, STORE_AUX, true>(x, y, alpha, zs, beta, blocks, pool, deltas, values, pd, H, step);
        halo_finish(H, step);          // the launch's last workgroup raises `consumed` and advances the step number (halo.hpp)
    }
}

// The walk of the headline shape -- tiles of two lines, no ghost planes, not flat -- with no stretch in which a workgroup has no request
// in flight (one walk per CU is all that is resident there: a walk that waits leaves the CU's share of HBM idle).  The steps, the sums
// and their order are those of plane_walk; what differs is WHEN things are asked for:
//   * the walk's first x requests and the classes of its first four planes go out first, the tables are read behind them;
//   * where the first plane uses a class other than the hot one, that class is decoded before the first look, so plane 0 of a grid --
//     all boundary lines -- takes fast steps;
//   * the classes of the tile's lines come through SCALAR loads, requested at the top of a group of four steps for the four planes
//     behind it (cw[]) and looked at when the group is done.  Scalar loads are counted apart from the vector requests, so no look waits
//     for an x request or a store (plane_walk's look-up every 64 planes is two dependent vector loads behind a full drain), and they
//     cost no vector register: the kernel sits at its 128, and a class kept in a vector register for the 64 steps of a window was
//     spilled and came back through the vector memory pipeline, behind every request of the walk.  Every class word is read once per
//     walk; a slow step takes its classes from the same registers, and a change of the other class needs nothing re-read.
// The last three planes of a grid still take slow steps (their requests would leave x): the rule `zh` of plane_walk.
// VEXHIP_PLANE_WALK=0 keeps plane_walk for this shape (tools/plane_walk_ab.py times the two in one process).
template <int ZM, int STORE_AUX>
__device__ __forceinline__
void plane_walk_ahead(const double *__restrict__ x, double *__restrict__ y, double alpha, const double *__restrict__ zs, double beta,
        const int *__restrict__ blocks, const char *__restrict__ pool, const int *__restrict__ deltas, const double *__restrict__ values,
        const plane_dev &pd)
{
    constexpr int TY = 2;
    __shared__ int s_slot[256];
    __shared__ double s_value[256];
    __shared__ double s_other[15][256];

    const int t = threadIdx.x;
    int y0, zc, z, zend;
    if (!plane_tile(pd, blockIdx.x, TY, y0, zc)) return;           // the whole workgroup
    if (!plane_chunk(pd, zc, z, zend)) return;
    const int ny = pd.ny;
    const int nslices = (int)pd.nslices, xlines = (int)pd.xlines;
    const unsigned lane_b = 16u * (unsigned)t;
    const int edge_b = edge_offset(t, 8);
    const clamped_requests<double> own = {x, zs, ny, y0, 0, xlines, nslices, pd.x_last, lane_b, edge_b};
    auto ld = [&](int zz, int l) { return own.ld(zz, l); };
    auto edge = [&](int zz, int l) { return own.edge(zz, l); };
    auto yold = [&](int zz, int l) { return own.yold(zz, l); };

    d2 Cs[4][TY], Hs[2][2], Yo[TY];
    double Es[2][TY];
    const unsigned plane_b32 = (unsigned)ny * (unsigned)PL_LINE_B;
    const int z_first = z;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double *>(x + ((long long)z_first * ny + (y0 - 1)) * PL_ROWS), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(y + ((long long)z_first * ny + y0) * PL_ROWS, 0, -1, 0x00020000);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(ZM == 1 ? zs : x) + ((long long)z_first * ny + y0) * PL_ROWS, 0, -1, 0x00020000);
    const int zh = fast_limit(zend, ny, y0, TY, xlines, nslices, ZM == 1);

    // ---- what depends on the geometry alone goes out first: the registers of plane z, the classes of the first four planes ----
    fill_registers<ZM>(Cs, Hs, Es, Yo, z, true, ld, edge, yold);
    // cw[i][l]: the class of tile line l in plane z + i (uniform: scalar loads; past the last line: the last line's, never looked at)
    int cw[4][TY];
    auto class_of = [&](int zz, int l) -> int {
        const int li = zz * ny + (y0 + l);
        return __builtin_amdgcn_readfirstlane(blocks[li < nslices ? li : nslices - 1]);
    };
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int l = 0; l < TY; ++l) cw[i][l] = class_of(z + i, l);

    // ---- the tables, behind the requests ----
    s_slot[t] = 2 * position_of(deltas[t], pd.far); s_value[t] = values[t];
    __syncthreads();
    const int wp = (pd.w + 1) >> 1;
    auto decode = [&](int blk) -> unsigned {
        return pd.pitch > 0 ? decode_table<false>(pool + (long long)blk * 7 * pd.pitch + 2 * t, pd.pitch, s_value, s_other, t)
                            : decode_block(pool, blk, pd.w, wp, s_slot, s_value, s_other, t);
    };
    const int hot = pd.hot;
    double aH[7][2];
    unsigned long long mH[7][2];
    take_hot(decode(hot), s_other, t, aH, mH);
    unsigned bitsO = 0;
    int other = -1;
    const line_terms<double, 15, 256> terms = {aH, mH, s_other, hot, other, bitsO, t, alpha, beta};
    // the first plane's first class that is not the hot one becomes the other class now
#pragma unroll
    for (int l = TY - 1; l >= 0; --l)
        if (cw[0][l] != hot && z * ny + (y0 + l) < nslices) other = cw[0][l];
    if (other >= 0) bitsO = decode(other);

    // the look: can the planes z .. z + 3 take a group of four fast steps -- all below zh, every line of the hot or the other class?
    unsigned use_hot = 0;                               // bit 4 l + i: line l of plane z + i uses the hot class
    auto look = [&]() -> bool {
        bool fast = z + 4 <= zh;
        use_hot = 0;
#pragma unroll
        for (int l = 0; l < TY; ++l)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                fast = fast && (cw[i][l] == hot || cw[i][l] == other);
                use_hot |= (cw[i][l] == hot ? 1u : 0u) << (4 * l + i);
            }
        return fast;
    };
    while (z < zend) {
        if (look()) {
            // A run of groups is entered with nothing outstanding (the prologue and a slow step have consumed what they requested last):
            // said here, so that the waits inside the loop count the loop's own requests and not, for every group, the fewer ones that
            // follow a request of a slow step.
            __builtin_amdgcn_s_waitcnt(0x0f70);             // vmcnt(0)
            do {
                // the classes of the four planes behind the group: requested now, looked at when the group is done
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int l = 0; l < TY; ++l) cw[i][l] = class_of(z + 4 + i, l);
                unsigned xo = (unsigned)((z + 2 - z_first) * plane_b32), yo = (unsigned)((z - z_first) * plane_b32);
                auto fast_step = [&](d2 (&P)[TY], d2 (&C)[TY], d2 (&N)[TY], d2 (&Hl)[2], double (&E)[TY]) {
                    d2 o[TY];
#pragma unroll
                    for (int l = 0; l < TY; ++l) {
                        double xs[2][7], sm[2] = {};
                        stencil_x(P, C, N, Hl, E, l, xs);
                        if (use_hot & (1u << (4 * l))) hot_sums(sm, aH, mH, xs); else other_sums(sm, s_other, t, bitsO, xs);      // uniform
                        o[l] = add_addend<ZM>(alpha, sm, beta, Yo[l], C[l]);
                    }
                    use_hot >>= 1;
#pragma unroll
                    for (int l = 0; l < TY; ++l) store16<STORE_AUX>(o[l], ry, (int)lane_b, yo + l * PL_LINE_B);
                    if (ZM == 1) {
#pragma unroll
                        for (int l = 0; l < TY; ++l) Yo[l] = load16<double>(rz, (int)lane_b, yo + plane_b32 + l * PL_LINE_B);
                    }
                    Hl[0] = load16<double>(rx, (int)lane_b, xo);
                    Hl[1] = load16<double>(rx, (int)lane_b, xo + (TY + 1) * PL_LINE_B);
#pragma unroll
                    for (int l = 0; l < TY; ++l) {
                        P[l] = load16<double>(rx, (int)lane_b, xo + plane_b32 + (l + 1) * PL_LINE_B);
                        E[l] = load_edge<double>(rx, edge_b + 8, xo + (l + 1) * PL_LINE_B - 8u);
                    }
                    xo += plane_b32; yo += plane_b32; ++z;
                };
                fast_group(fast_step, Cs, Hs, Es);
            } while (look());
            if (z >= zend) break;
        }
        // ---- a slow step, as in plane_walk; the classes come from cw[0] ----
#pragma unroll
        for (int l = 0; l < TY; ++l) {
            const int li = z * ny + (y0 + l);
            if (li < nslices) {                                           // uniform
                const d2 o = line_result<ZM>(terms, cw[0][l], decode, Cs, Hs, Es, Yo, l);
                __builtin_nontemporal_store(o, reinterpret_cast<d2 *>(reinterpret_cast<char *>(y + (long long)li * PL_ROWS) + lane_b));
            }
        }
        rotate_by_copy<ZM>(Cs, Hs, Es, Yo, z, true, ld, edge, yold);
        ++z;
#pragma unroll
        for (int l = 0; l < TY; ++l) {
#pragma unroll
            for (int i = 0; i < 3; ++i) cw[i][l] = cw[i + 1][l];
            cw[3][l] = class_of(z + 3, l);
        }
    }
}

// (a namespace of its own, the kernel's name kept: profiles and the counter passes of bench.py find the headline kernel by that name)
namespace ahead {
template <int ZM, int STORE_AUX>
__global__ __launch_bounds__(256, 4)
void sell8_plane_kernel(const double *__restrict__ x, double *__restrict__ y, double alpha, const double *__restrict__ zs, double beta,
        const int *__restrict__ blocks, const char *__restrict__ pool, const int *__restrict__ deltas, const double *__restrict__ values,
        plane_dev pd)
{
    plane_walk_ahead<ZM, STORE_AUX>(x, y, alpha, zs, beta, blocks, pool, deltas, values, pd);
}
} // namespace ahead

// The yardstick of the plane / march products (bench.py roofline.device_copy_hand): x copied to y with one 16-byte pair per lane,
// no loop, non-temporal stores -- the same HBM traffic as the product (x once, y once) and nothing else to do.  6.23 TB/s at
// 512^3 elements on the box where the library's copy (torch) reaches 4.94 (profiles/r04_pm_proto.json).
__global__ __launch_bounds__(256)
void stream_copy_kernel(const double *__restrict__ x, double *__restrict__ y, long long npairs, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < npairs) __builtin_nontemporal_store(reinterpret_cast<const d2 *>(x)[i], reinterpret_cast<d2 *>(y) + i);
    else if (i == npairs && (n & 1)) y[n - 1] = x[n - 1];
}

// behind a HALO launch: the ghost planes of product `step` have been read -- the owners may write the next ones
__global__ void halo_signal_kernel(halo_dev H) {
    const unsigned long long step = *H.step;
    if (H.consumed_lo) __hip_atomic_store(H.consumed_lo, step, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (H.consumed_hi) __hip_atomic_store(H.consumed_hi, step, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (H.pull == 1) {
        // PULL: the neighbours read this rank's boundary planes of x IN PLACE -- the stream must not go on (to a kernel that may
        // overwrite x) before they say they have (a pushed share is a copy: there the next push waits instead)
        if (H.sent_lo) (void)spin_until(H.sent_lo, step, H.err, H.ticks, 0);
        if (H.sent_hi) (void)spin_until(H.sent_hi, step, H.err, H.ticks, 0);
    }
    *H.step = step + 1ull;
}

} // namespace
} // namespace vexhip

namespace vexhip {
// y = alpha A x + [zm 1: beta zs | zm 2: beta x] through the plane product (spmat.hip vexhip_spmat_apply_axpby_f64; the exported
// vexhip_spmv_sell8v_plane_f64_i32 is zm = append, zs = y, beta = 1)
int plane_apply_axpby(int dev, void *stream, int64_t n, double alpha, int zm, const double *zs, double beta, int64_t w, const void *pool,
        const int32_t *blocks, const int32_t *deltas, const double *values, const double *x, double *y, const vexhip_plane *plane)
{
    if (int rc = plane_check(plane, 0, PL_LINE_B, n, w, pool && blocks && deltas && values, x, y, true)) return rc;      // the plan's tile, the plan's depth
    VEXHIP_REQUIRE(zm == 0 || zm == 2 || (zm == 1 && zs && (reinterpret_cast<uintptr_t>(zs) & 15) == 0), "plane product: the addend must be a 16-byte aligned vector");
    VEXHIP_SET_DEVICE(dev);
    const plane_dev pd = plane_launch(*plane, n, w, plane->tile, plane->depth);
    unsigned grid;
    if (int rc = plane_workgroups(pd, pd.nz, 0, 0, &grid)) return rc;
    const char *cpool = static_cast<const char *>(pool);
    const char *walk = env(ENV_VEXHIP_PLANE_WALK);                           // 0: plane_walk for every shape; 1 / unset: plane_walk_ahead where it exists
    const bool ahead = plane->tile == 2 && !plane->flat && !(walk && std::atoi(walk) == 0);
    with_launch_forms(zm, plane->store_policy, [&](auto ZM, auto AUX) {      // (the plan's policy: plane_geometry_with; the flat walk exists for tiles of two only)
        if (ahead) {
            ahead::sell8_plane_kernel<ZM(), AUX()><<<grid, 256, 0, as_stream(stream)>>>(x, y, alpha, zs, beta, blocks, cpool, deltas, values, pd);
            return;
        }
        auto kernel = plane->tile == 4 ? sell8_plane_kernel<4, ZM(), AUX()> : plane->flat ? sell8_plane_kernel<2, ZM(), AUX(), false, true> : sell8_plane_kernel<2, ZM(), AUX()>;
        kernel<<<grid, 256, 0, as_stream(stream)>>>(x, y, alpha, zs, beta, blocks, cpool, deltas, values, pd, halo_dev());
    });
    VEXHIP_LAUNCH_CHECK();
    return 0;
}

} // namespace vexhip

using namespace vexhip;

// lines per workgroup (2 or 4), planes per workgroup, store policy of a plane plan; false: the walk does not fit 32-bit offsets
static bool plane_geometry_with(long long cus, long long ny, long long nz, int hot, vexhip_plane *out);
static bool plane_geometry(int dev, long long ny, long long nz, int hot, vexhip_plane *out)
{
    return plane_geometry_with(std::max(1, info(dev).cus), ny, nz, hot, out);
}
// (host arithmetic only: vexhip_sell8_plane_geometry exposes it so that the choice of walks can be checked without a device)
static bool plane_geometry_with(long long cus, long long ny, long long nz, int hot, vexhip_plane *out)
{
    cus = std::max(1ll, cus);
    auto depth_for = [&](long long tl) {
        const long long tiles = ny / tl;
        long long chunks = std::max(1ll, std::min(nz / 8, (cus + tiles / 2) / tiles));
        // Round 5 -- ONE workgroup per CU, all of them resident and in step, is the best a launch can do (512 lines per plane:
        // walks of 512 / 256 / 128 / 64 / 43 planes = 0.377 / 0.385 / 0.387 / 0.387 / 0.385 ms) -- but only where the tiles come out
        // as one per CU.  Planes of 640 lines are 1.25 tiles per CU: with one walk per tile a quarter of the CUs do twice the work
        // of the others (0.850 ms for 512 x 640 x 640; walks of 80 planes: 0.621).  So unless the workgroups above number
        // 0.95 .. 1 per CU: many short walks, at least six per CU for the dispatcher to even out, the fewest rounds of
        // (planes per walk + 6) -- the rule of the grid product (grid.hip).  Measured, plan before -> after
        // (profiles/r05_plane_shapes.json): 512 x 640 x 640 0.850 -> 0.621 ms, 512 x 768 x 512 0.768 -> 0.626, 512 x 384 x 768
        // 0.492 -> 0.431, 512 x 320 x 1024 0.702 -> 0.52, 512 x 1024 x 256 0.434 -> 0.428.
        if (tiles * chunks > cus || tiles * chunks * 20 < cus * 19) {
            double best = 0;
            const long long cmax = std::max(1ll, nz / 16);
            for (long long c = 1; c <= cmax; ++c) {
                const long long per_cu = (tiles * c + cus - 1) / cus;
                if (per_cu < 6 && c < cmax) continue;
                const double est = (double)per_cu * (double)((nz + c - 1) / c + 6);
                if (best == 0 || est <= best * 1.01) { if (best == 0 || est < best) best = est; chunks = c; }
                if (per_cu > 24) break;
            }
        }
        // SHORT walks (a rank's strip of a partitioned grid: 64 planes at 512^3 / 8) want two workgroups per CU: the start and the
        // end of a walk -- four planes requested before the first row is stored, the last planes clamped -- are a tenth of a
        // 64-plane walk and overlap with the other workgroup's steady state: 56.6 -> 47.0 us for 16.8 M rows (depth 22 / 16 / 11:
        // 50.0 / 50.8 / 52.4; tools/r05_dist_step.py, "local part alone").  Long walks lose 2 % that way (512 planes, round 4).
        if (chunks == 1 && nz >= 32 && nz <= 192 && tiles * 2 <= 2 * cus) chunks = 2;
        return (nz + chunks - 1) / chunks;
    };
    long long tile = 2;
    if (const char *e = env(ENV_VEXHIP_PLANE_TILE)) tile = (std::atoi(e) == 4 && ny % 4 == 0) ? 4 : 2;
    long long depth = depth_for(tile);
    if (const char *e = env(ENV_VEXHIP_PLANE_DEPTH)) depth = std::max(1, std::atoi(e));
    depth = std::min(depth, nz);
    while ((depth + 4) * ny * PL_LINE_B >= (1ll << 32) && depth > 8) depth = (depth + 1) / 2;      // 32-bit byte offsets inside a workgroup's walk
    if ((depth + 4) * ny * PL_LINE_B >= (1ll << 32)) return false;
    out->lines_per_plane = (int32_t)ny; out->planes = (int32_t)nz; out->depth = (int32_t)depth; out->hot_block = hot; out->tile = (int32_t)tile;
    // cache policy of the y stores (launch.hpp with_launch_forms: the policies and their measurements); VEXHIP_PLANE_STORE overrides
    out->store_policy = tile == 4 ? 2 : 1;
    if (const char *e = env(ENV_VEXHIP_PLANE_STORE)) out->store_policy = std::max(0, std::min(3, std::atoi(e)));
    return true;
}

namespace vexhip {
// The plane plan of a matrix stored by grid line (grid.hip grid_build) whose lines are 512 points long: the plane kernel reads the
// class tables instead of SELL-512 code blocks (table_pitch > 0); a line IS a slice, its class takes the place of its block.
// The build has checked what the plan checks on dictionary blocks (diagonals, positions ascending, few lines off the hot class).
int plane_plan_from_grid(int dev, const vexhip_grid *grid, int64_t rows, vexhip_plane *out)
{
    VEXHIP_REQUIRE(grid && out, "NULL argument");
    std::memset(out, 0, sizeof(*out));
    const bool force = env(ENV_VEXHIP_PLANE_FORCE) != nullptr;
    if (!grid->usable || grid->nx != PL_ROWS || grid->segments != 1 || rows % PL_ROWS != 0) return 0;
    const long long ny = grid->lines_per_plane, nz = grid->planes;
    if (ny < 4 || ny % 2 != 0 || (nz < 4 && !force) || (rows / PL_ROWS < 64 && !force)) return 0;
    if ((grid->x_last + 1) % PL_ROWS != 0 || grid->x_last + 1 < rows) return 0;
    if (!plane_geometry(dev, ny, nz, grid->hot_class, out)) return 0;
    out->table_pitch = grid->pitch;
    out->flat = grid->flat;
    out->x_last = grid->x_last; out->usable = 1;
    return 0;
}
} // namespace vexhip

namespace vexhip {
// One rank's product step in one launch (halo.hpp): the plane product over the planes [H.z0, H.z1) of the stored grid of n_ext
// rows, x and y being the rank's own segments (their element 0 is row H.z0 * far of the stored grid); ghost planes from the
// window, boundary planes pushed by the first workgroups; then the kernel that raises `consumed` and advances the step number.
int plane_apply_halo(int dev, hipStream_t s, int64_t n_ext, double alpha, int append, int64_t w, const void *pool, const int32_t *blocks,
        const int32_t *deltas, const double *values, const double *x, double *y, const vexhip_plane *plane, halo_dev H)
{
    // (the kernel of the step is the one for tiles of two lines whatever the plan's tile; the depth checked is the plan's, the one walked is chosen below)
    if (int rc = plane_check(plane, 2, PL_LINE_B, n_ext, w, pool && blocks && deltas && values, x, y, true)) return rc;
    if (int rc = check_halo_step(H, plane->planes, (long long)plane->lines_per_plane * PL_ROWS, false)) return rc;
    VEXHIP_SET_DEVICE(dev);
    const int nzr = H.z1 - H.z0;
    int edge_planes = 8;
    if (const char *e = env(ENV_VEXHIP_HALO_EDGE_PLANES)) edge_planes = std::max(1, std::atoi(e));
    int lo_planes = edge_planes, hi_planes = edge_planes;
    if (const char *e = env(ENV_VEXHIP_HALO_LO_PLANES)) lo_planes = std::max(1, std::atoi(e));
    if (const char *e = env(ENV_VEXHIP_HALO_HI_PLANES)) hi_planes = std::max(1, std::atoi(e));
    H.lo_planes = H.lo ? std::min(lo_planes, nzr) : 0;
    H.hi_planes = H.hi ? std::min(hi_planes, nzr - H.lo_planes) : 0;
    const int mid = nzr - H.lo_planes - H.hi_planes;
    int depth = std::max(1, mid);         // ONE main chunk (two of 25 planes beside the short chunks: 88-90 us against 76 for the step)
    if (const char *e = env(ENV_VEXHIP_HALO_DEPTH)) depth = std::max(1, std::atoi(e));
    const plane_dev pd = plane_launch(*plane, n_ext, w, 2, depth);
    const long long npush = H.pull ? 0 : (H.dst_lo ? H.push_blocks : 0) + (H.dst_hi ? H.push_blocks : 0);
    unsigned grid;
    if (int rc = plane_workgroups(pd, mid, (H.lo_planes ? 1 : 0) + (H.hi_planes ? 1 : 0), npush, &grid)) return rc;
    VEXHIP_REQUIRE(H.pull || H.push_blocks > 0 || grid - npush >= 512 || !(H.dst_lo || H.dst_hi), "too few workgroups to push the boundary planes");
    const double *xe = x - (long long)H.z0 * pd.far;          // the kernel addresses x and y in the numbering of the stored grid
    double *ye = y - (long long)H.z0 * pd.far;
    const char *cpool = static_cast<const char *>(pool);
    auto kernel = append ? sell8_plane_kernel<2, 1, 18, true> : sell8_plane_kernel<2, 0, 18, true>;      // '=' and '+=' only; the stores of a step always take policy 1 (immediate 18)
    kernel<<<grid, 256, 0, s>>>(xe, ye, alpha, append ? ye : nullptr, append ? 1.0 : 0.0, blocks, cpool, deltas, values, pd, H);
    VEXHIP_LAUNCH_CHECK();
    if (H.pull != 2 && !H.one_launch) {   // (events: the host advances nothing on the device -- there are no flags to number; one_launch: the last workgroup has done it)
        halo_signal_kernel<<<1, 1, 0, s>>>(H);
        VEXHIP_LAUNCH_CHECK();
    }
    return 0;
}
} // namespace vexhip

extern "C" {

int vexhip_sell8_plane_geometry(int cus, int64_t lines_per_plane, int64_t planes, vexhip_plane *out)
{
    VEXHIP_REQUIRE(out, "NULL output");
    std::memset(out, 0, sizeof(*out));
    reload_env();
    VEXHIP_REQUIRE(lines_per_plane >= 4 && lines_per_plane % 2 == 0 && lines_per_plane < (1ll << 30) && planes >= 1 && planes < (1ll << 30), "bad grid");
    if (!plane_geometry_with(cus, lines_per_plane, planes, 0, out)) { std::memset(out, 0, sizeof(*out)); return 0; }      // depth = 0: no geometry
    return 0;
}

int vexhip_sell8_plane_plan(int dev, void *stream, const int32_t *deltas, int ndeltas, const int32_t *blocks, int64_t nslices,
        const void *pool, int64_t dictionary_blocks, int64_t ell_width, int64_t rows, int64_t tail_nnz, int value_bytes,
        int64_t x_last, vexhip_plane *out)
{
    VEXHIP_REQUIRE(out, "NULL output");
    std::memset(out, 0, sizeof(*out));
    reload_env();
    const bool force = env(ENV_VEXHIP_PLANE_FORCE) != nullptr;          // tests: small grids, many blocks
    if ((value_bytes != 8 && value_bytes != 4) || !deltas || !blocks || !pool || ndeltas < 2 || ndeltas > 7 || dictionary_blocks < 1 || dictionary_blocks > 128) return 0;
    if (ell_width < 1 || ell_width > 8 || tail_nnz != 0 || rows != nslices * PL_ROWS || (nslices < 64 && !force)) return 0;
    if (x_last < 0 || (x_last + 1) % PL_ROWS != 0 || x_last + 1 < rows) return 0;
    VEXHIP_SET_DEVICE(dev);
    hipStream_t s = as_stream(stream);
    const int wp = (int)((ell_width + 1) / 2);
    const size_t code_bytes = (size_t)wp * 2048;
    std::vector<int> table((size_t)ndeltas), id((size_t)nslices);
    std::vector<unsigned> codes((size_t)dictionary_blocks * code_bytes / 4);
    VEXHIP_TRY(hipMemcpyAsync(table.data(), deltas, sizeof(int) * (size_t)ndeltas, hipMemcpyDeviceToHost, s));
    VEXHIP_TRY(hipMemcpyAsync(id.data(), blocks, sizeof(int) * (size_t)nslices, hipMemcpyDeviceToHost, s));
    VEXHIP_TRY(hipMemcpyAsync(codes.data(), pool, (size_t)dictionary_blocks * code_bytes, hipMemcpyDeviceToHost, s));
    VEXHIP_TRY(hipStreamSynchronize(s));
    // the diagonals: {0, +-1, +-512} and one far pair +-P, P a multiple of 1024 (two lines per workgroup)
    long long far = 0;
    for (int d : table) {
        const long long a = std::llabs((long long)d);
        if (a == 0 || a == 1 || a == PL_ROWS) continue;
        if (far == 0) far = a;
        if (a != far) return 0;
    }
    if (far < 4 * PL_ROWS || far % (2 * PL_ROWS) != 0 || far > (1ll << 30)) return 0;
    const long long ny = far / PL_ROWS, nz = (nslices + ny - 1) / ny;
    if (nz < 4 && !force) return 0;
    auto position = [&](int d) { return d == 0 ? 3 : d == -1 ? 2 : d == 1 ? 4 : d == -PL_ROWS ? 1 : d == PL_ROWS ? 5 : d == -far ? 0 : 6; };
    // every row of every dictionary block: positions strictly ascending along the ELL columns (position order = storage order)
    for (int64_t blk = 0; blk < dictionary_blocks; ++blk) {
        const unsigned *cw = codes.data() + (size_t)blk * code_bytes / 4;
        for (int t = 0; t < 256; ++t)
            for (int r = 0; r < 2; ++r) {
                int last = -1;
                for (int j = 0; j < (int)ell_width; ++j) {
                    const unsigned cword = cw[(size_t)(j >> 1) * 256 + t] >> (16 * (j & 1));
                    const unsigned code = (cword >> (8 * r)) & 255u;
                    if (code >= PL_PAD_FIRST) continue;
                    if ((int)code >= ndeltas) return 0;
                    const int p = position(table[code]);
                    if (p <= last) return 0;
                    last = p;
                }
            }
    }
    // the hot block; lines that use another one must be few (each change of the other block is a decode: two dependent loads)
    std::vector<int64_t> uses((size_t)dictionary_blocks, 0);
    for (int64_t k = 0; k < nslices; ++k) {
        if (id[(size_t)k] < 0 || id[(size_t)k] >= dictionary_blocks) return 0;
        ++uses[(size_t)id[(size_t)k]];
    }
    const int hot = (int)(std::max_element(uses.begin(), uses.end()) - uses.begin());
    if ((nslices - uses[(size_t)hot]) * 16 > nslices && !force) return 0;
    // Lines per workgroup (2 or 4) and planes per workgroup.  Measured at 512^3 (profiles/r04_plane_sweep*.json, r04_plane_offsets.json;
    // march product 0.466 ms beside them): FEW, LONG workgroups win -- with every request two steps ahead a wave hides the memory
    // latency by itself, and every workgroup re-reads the 4 planes around its range: tile 2 x depth 128 / 256 / 512 = 0.393 /
    // 0.389 / 0.381 ms, tile 4 x depth 128 / 256 = 0.409 / 0.388 ms (tile 4 x 512: half the CUs idle, 0.57).  Tile 4 halves the
    // halo requests (HBM read 1.04 x instead of 1.14 x of x at depth 128) but needs 164 registers and is not faster.  So: two
    // lines, about one workgroup per CU.  The time also depends on where x and y lie relative to each other (0.378 - 0.41 ms for
    // the same kernel, r04_plane_offsets.json; the copy kernel and the march product do not show it).
    if (!plane_geometry(dev, ny, nz, hot, out)) return 0;
    out->flat = 1;
    for (int d : table) if (std::llabs((long long)d) == PL_ROWS) out->flat = 0;
    out->x_last = x_last; out->usable = 1;
    return 0;
}

int vexhip_spmv_sell8v_plane_f64_i32(int dev, void *stream, int64_t n, double alpha, int append, int64_t w, const void *pool,
        const int32_t *blocks, const int32_t *deltas, const double *values, const double *x, double *y, const vexhip_plane *plane)
{ return plane_apply<double>(dev, stream, n, alpha, append, w, pool, blocks, deltas, values, x, y, plane); }

int vexhip_stream_copy_f64(int dev, void *stream, const double *x, double *y, int64_t n)
{
    VEXHIP_REQUIRE(n >= 0 && (n == 0 || (x && y)), "bad copy arguments");
    VEXHIP_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0, "stream copy: x and y must be 16-byte aligned");
    if (n == 0) return 0;
    VEXHIP_SET_DEVICE(dev);
    const long long npairs = n / 2, grid = (npairs + 1 + 255) / 256;
    VEXHIP_REQUIRE(grid < (1ll << 31), "vector too large for one launch");
    stream_copy_kernel<<<(unsigned)grid, 256, 0, as_stream(stream)>>>(x, y, npairs, (long long)n);
    VEXHIP_LAUNCH_CHECK();
    return 0;
}

} // extern "C"

VEXHIP_WARM_TU(plane)
