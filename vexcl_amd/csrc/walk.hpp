// The device side that the four grid-line products share (plane.hip, plane32.hip, grid_walk.hpp): a workgroup owns TY adjacent grid
// lines and walks through the planes; a lane owns R = 16 / sizeof(V) adjacent rows of each line as ONE 16-byte vector (fp64: a pair,
// fp32: a quad).  Here stand, once: the lane's requests, the table form of a decode, x at the seven stencil positions and the sums
// over them, the look-ahead that bounds a run of fast steps, and the two rotations of the walk's registers.  What differs between
// the walks stays with them: where a line lies (512-point lines / any length), the clamped requests, the ghost planes.
#pragma once
#include "lanes.hpp"

namespace vexhip {
namespace {

// ---- a lane's 16 bytes ----
template <typename V> struct lane_vec;
template <> struct lane_vec<double> { typedef d2 vec; };
template <> struct lane_vec<float> { typedef f4 vec; };
template <typename V> using vec_of = typename lane_vec<V>::vec;
template <typename V> constexpr int rows_of = 16 / (int)sizeof(V);

// buffer requests of the fast steps: the lane's byte offset `voff`, a scalar offset `soff` that moves with the planes
template <typename V>
__device__ __forceinline__ vec_of<V> load16(__amdgpu_buffer_rsrc_t rs, int voff, unsigned soff) {
    return __builtin_bit_cast(vec_of<V>, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, (int)soff, 0));
}
template <int AUX, typename VEC>
__device__ __forceinline__ void store16(VEC v, __amdgpu_buffer_rsrc_t rs, int voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), rs, voff, (int)soff, AUX);
}
// the element beyond either end of a wave's rows (one element wide)
template <typename V>
__device__ __forceinline__ V load_edge(__amdgpu_buffer_rsrc_t rs, int voff, unsigned soff) {
    if constexpr (sizeof(V) == 8) return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, (int)soff, 0));
    else return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b32(rs, voff, (int)soff, 0));
}
// the first nv (< R) rows of a lane at the end of its line, one by one
template <int AUX, typename VEC>
__device__ __forceinline__ void store_rows(VEC v, int nv, __amdgpu_buffer_rsrc_t rs, int voff, unsigned soff) {
    constexpr int R = (int)(sizeof(VEC) / sizeof(v.x));
#pragma unroll
    for (int r = 0; r < R - 1; ++r)
        if (r < nv) {
            const auto e = v[r];                 // (a copy: __builtin_bit_cast of the element expression itself reads element 0)
            if constexpr (sizeof(e) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, e), rs, voff + 8 * r, (int)soff, AUX);
            else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, e), rs, voff + 4 * r, (int)soff, AUX);
        }
}

// ---- a class / line table -> values and validity of the lane's R rows at the seven positions ----
// tb: the lane's R value codes of position 0 (one byte per row, 255 = no entry; position p lies p * pitch bytes on).  The values go
// into s_other ([position * R + row][lane]: lane-private, conflict-free), the validity bits are returned.  HALVES: the codes are
// read as 2-byte pieces (a lane of grid32.hip may start at any even byte).
template <bool HALVES, typename V, int ROWS, int LANES>
__device__ __forceinline__ unsigned decode_table(const void *tb, int pitch, const V *s_value, V (&s_other)[ROWS][LANES], int t) {
    constexpr int R = rows_of<V>;
    unsigned bits = 0;
#pragma unroll
    for (int p = 0; p < 7; ++p) {
        const char *at = static_cast<const char *>(tb) + (long long)p * pitch;
        unsigned codes;
        if constexpr (R == 2) codes = *reinterpret_cast<const unsigned short *>(at);
        else if constexpr (HALVES) { const unsigned short *h = reinterpret_cast<const unsigned short *>(at); codes = (unsigned)h[0] | ((unsigned)h[1] << 16); }
        else codes = *reinterpret_cast<const unsigned *>(at);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const unsigned code = (codes >> (8 * r)) & 255u;
            s_other[R * p + r][t] = s_value[code];                // entry 255 of the value table is 0.0
            bits |= (code != 255u ? 1u : 0u) << (R * p + r);
        }
    }
    return bits;
}
// what a decode left in s_other becomes the HOT block / class: values in registers, the lanes with an entry as scalar masks
template <typename V, int R, int ROWS, int LANES>
__device__ __forceinline__ void take_hot(unsigned bits, const V (&s_other)[ROWS][LANES], int t, V (&aH)[7][R], unsigned long long (&mH)[7][R]) {
#pragma unroll
    for (int p = 0; p < 7; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            aH[p][r] = s_other[R * p + r][t];
            mH[p][r] = __builtin_amdgcn_ballot_w64((bits >> (R * p + r)) & 1u);
        }
}

// ---- x at the seven positions {-far, -line, -1, 0, +1, +line, +far} of the lane's R rows of tile line l ----
// P, C, N: the tile's centre lines in the planes behind, at and ahead of the step's; H: the lines above and below the tile; E: per
// centre line the lane's edge element.  Only the first and the last row look at another lane (one DPP shift each).
template <int TY, typename VEC, typename V, int R>
__device__ __forceinline__ void stencil_x(const VEC (&P)[TY], const VEC (&C)[TY], const VEC (&N)[TY], const VEC (&H)[2], const V (&E)[TY], int l, V (&xs)[R][7]) {
    const VEC c = C[l], up = l == 0 ? H[0] : C[l > 0 ? l - 1 : 0], dn = l == TY - 1 ? H[1] : C[l < TY - 1 ? l + 1 : 0], pv = P[l], nx = N[l];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        xs[r][0] = pv[r]; xs[r][1] = up[r];
        xs[r][2] = r == 0 ? shift_from_lower_lane(c[R - 1], E[l]) : c[r > 0 ? r - 1 : 0];
        xs[r][3] = c[r];
        xs[r][4] = r == R - 1 ? shift_from_upper_lane(c[0], E[l]) : c[r < R - 1 ? r + 1 : 0];
        xs[r][5] = dn[r]; xs[r][6] = nx[r];
    }
}
// the rows' sums, entries in position order (= storage order), products rounded before they are added
template <typename V, int R>
__device__ __forceinline__ void hot_sums(V (&s)[R], const V (&aH)[7][R], const unsigned long long (&mH)[7][R], const V (&xs)[R][7]) {
#pragma unroll
    for (int p = 0; p < 7; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] += aH[p][r] * keep_lanes(xs[r][p], mH[p][r]);
}
template <typename V, int R, int ROWS, int LANES>
__device__ __forceinline__ void other_sums(V (&s)[R], const V (&s_other)[ROWS][LANES], int t, unsigned bits, const V (&xs)[R][7]) {
#pragma unroll
    for (int p = 0; p < 7; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] += s_other[R * p + r][t] * keep_bit(xs[r][p], bits, R * p + r);
}
// alpha times the sums, plus the addend.  ZM: 0 none, 1 beta times an array (yo: the lane's rows of it; '+=' is the old y, beta = 1),
// 2 beta times x itself (c: the centre line, from the registers)
template <int ZM, typename VEC, typename V, int R>
__device__ __forceinline__ VEC add_addend(V alpha, const V (&s)[R], V beta, const VEC &yo, const VEC &c) {
    VEC o;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        o[r] = alpha * s[r];
        if (ZM == 1) o[r] = beta * yo[r] + o[r];
        if (ZM == 2) o[r] = beta * c[r] + o[r];
    }
    return o;
}
// What the result of a line needs beside x: the hot class / block in registers, one other class in s_other (which one, and its validity
// bits: they change under a walk's slow steps), the scale and the addend.  The walks keep the arrays.
template <typename V, int ROWS, int LANES>
struct line_terms {
    static constexpr int R = rows_of<V>;
    const V (&aH)[7][R];
    const unsigned long long (&mH)[7][R];
    const V (&s_other)[ROWS][LANES];
    const int hot;
    int &other;
    unsigned &bitsO;
    const int t;
    const V alpha, beta;
};
// The line of a slow step, the lane's vector to store: its class is the hot one, the other one, or becomes the other one now (`decode`
// fills s_other).  (The class is decided behind the stencil, as the walks had it: decided in front of it, the fp64 kernels allocate otherwise.)
template <int ZM, int TY, typename V, int ROWS, int LANES, typename VEC, typename DECODE>
__device__ __forceinline__ VEC line_result(const line_terms<V, ROWS, LANES> &terms, int cls, DECODE &&decode,
        const VEC (&Cs)[4][TY], const VEC (&Hs)[2][2], const V (&Es)[2][TY], const VEC (&Yo)[TY], int l) {
    constexpr int R = rows_of<V>;
    V xs[R][7], s[R] = {};
    stencil_x(Cs[0], Cs[1], Cs[2], Hs[0], Es[0], l, xs);
    if (cls == terms.hot) hot_sums(s, terms.aH, terms.mH, xs);
    else {
        if (cls != terms.other) { terms.bitsO = decode(cls); terms.other = cls; }
        other_sums(s, terms.s_other, terms.t, terms.bitsO, xs);
    }
    return add_addend<ZM>(terms.alpha, s, terms.beta, Yo[l], Cs[1][l]);
}

// ---- the look-ahead: how many of the planes z, z + 1, ... (<= 64, below zh) can take fast steps ----
// One look at the classes (blocks[] / line_class[]) of the tile's nl live lines, line0 = that of its first line in plane 0: a plane
// can when every line uses the hot class or the other one.  use_hot[l], bit k: line l of plane z + k uses the hot class.
template <int TY>
__device__ __forceinline__ int fast_run(const int *__restrict__ classes, int ny, int line0, int nl, int z, int zh, int hot, int other, int t,
        unsigned long long (&use_hot)[TY]) {
    const int k = t & 63, zz = z + k;
    const bool in = zz < zh;
    bool ok = in;
#pragma unroll
    for (int l = 0; l < TY; ++l) {
        const int bk = (in && l < nl) ? classes[(long long)zz * ny + (line0 + l)] : hot;
        ok = ok && (bk == hot || bk == other);
        use_hot[l] = __builtin_amdgcn_ballot_w64(bk == hot);
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
    return ~m ? __builtin_ctzll(~m) : 64;
}

// ---- the registers of a walk at the top of the step for plane z, and their rotations ----
// Cs[0..3]: the tile's centre lines in planes z-1, z, z+1, z+2;  Hs[0..1]: the lines above and below the tile in planes z, z+1;
// Es[0..1]: per centre line the edge element of this lane (lane 0: the one in front of the wave's rows, lane 63: the one behind)
// in planes z, z+1.  A step consumes plane z-1's centres and plane z's halos and edges and requests into the SAME registers
// what plays that role three (centres) or two planes later: every request has two steps to arrive.  The fast loop runs
// GROUPS of four steps with the names rotated: after four steps every name is back in place and no register is copied (a
// copy behind a request makes the step wait for it: the one-step form of this loop ran 8 % slower).  It contains no memory
// instruction other than these requests and the stores, so that the waits of a step count what the step before requested.
template <typename STEP, typename VEC, typename V, int TY>
__device__ __forceinline__ void fast_group(STEP &&step, VEC (&Cs)[4][TY], VEC (&Hs)[2][2], V (&Es)[2][TY]) {
    step(Cs[0], Cs[1], Cs[2], Hs[0], Es[0]);
    step(Cs[1], Cs[2], Cs[3], Hs[1], Es[1]);
    step(Cs[2], Cs[3], Cs[0], Hs[0], Es[0]);
    step(Cs[3], Cs[0], Cs[1], Hs[1], Es[1]);
}
// The walk's clamped requests fill the registers before the first step and behind a slow step, where the names are rotated by copies:
// ld(plane, line of the tile's window: 0 = the line above the tile, 1 .. TY = the tile, TY + 1 = the line below), edge(plane, line),
// yold(plane, tile line).  halo_lines: the lines above / below the tile are requested at all (a flat operator never reads them)
template <int ZM, typename VEC, typename V, int TY, typename LD, typename EDGE, typename YOLD>
__device__ __forceinline__ void fill_registers(VEC (&Cs)[4][TY], VEC (&Hs)[2][2], V (&Es)[2][TY], VEC (&Yo)[TY], int z, bool halo_lines,
        LD &&ld, EDGE &&edge, YOLD &&yold) {
#pragma unroll
    for (int l = 0; l < TY; ++l) { Cs[0][l] = ld(z - 1, l + 1); Cs[1][l] = ld(z, l + 1); Cs[2][l] = ld(z + 1, l + 1); Cs[3][l] = ld(z + 2, l + 1); }
    const VEC zero = {};
    Hs[0][0] = Hs[0][1] = Hs[1][0] = Hs[1][1] = zero;
    if (halo_lines) { Hs[0][0] = ld(z, 0); Hs[0][1] = ld(z, TY + 1); Hs[1][0] = ld(z + 1, 0); Hs[1][1] = ld(z + 1, TY + 1); }
#pragma unroll
    for (int l = 0; l < TY; ++l) {
        Es[0][l] = edge(z, l + 1); Es[1][l] = edge(z + 1, l + 1);
        if (ZM == 1) Yo[l] = yold(z, l);
    }
}
template <int ZM, typename VEC, typename V, int TY, typename LD, typename EDGE, typename YOLD>
__device__ __forceinline__ void rotate_by_copy(VEC (&Cs)[4][TY], VEC (&Hs)[2][2], V (&Es)[2][TY], VEC (&Yo)[TY], int z, bool halo_lines,
        LD &&ld, EDGE &&edge, YOLD &&yold) {
#pragma unroll
    for (int l = 0; l < TY; ++l) {
        Cs[0][l] = Cs[1][l]; Cs[1][l] = Cs[2][l]; Cs[2][l] = Cs[3][l]; Cs[3][l] = ld(z + 3, l + 1);
        Es[0][l] = Es[1][l]; Es[1][l] = edge(z + 2, l + 1);
        if (ZM == 1) Yo[l] = yold(z + 1, l);
    }
#pragma unroll
    for (int l = 0; l < 2; ++l) { Hs[0][l] = Hs[1][l]; if (halo_lines) Hs[1][l] = ld(z + 2, (TY + 1) * l); }
}

} // namespace
} // namespace vexhip
