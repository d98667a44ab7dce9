// Device-side knowledge of the SELL-512 storages that their product kernels share (spmv.hip, sell8.hip, spmm.hip): a slice is the 512
// rows of one workgroup, a lane owns rows 2t and 2t + 1 of it.  The coded storages (layouts: sell8.hip) keep a one-byte diagonal code --
// and, value-coded, a one-byte value code -- per entry, four to a word:  word [j >> 1] of a lane holds ELL columns j and j + 1 of its
// two rows.  What has one user stays with that user.
#pragma once
#include <hip/hip_runtime.h>

namespace vexhip {
namespace {

constexpr int SLICE_ROWS = 512;
// codes from here on are padding (a table holds at most 254 diagonals); 254 itself is the padding whose partner must not use the
// 16-byte load (gather_pair), 255 the padding that such a load may cover
constexpr unsigned PAD_UNSAFE = 254;
constexpr unsigned PAD = 255;

template <typename V> struct vec2 { typedef V type __attribute__((ext_vector_type(2))); };

// code of ELL column j, row q of the lane: in the one word that holds columns j and j ^ 1, or in the lane's words of a slice
__device__ __forceinline__ unsigned code_of(unsigned word, int j, int q) { return (word >> (16 * (j & 1) + 8 * q)) & 255u; }
template <int N>
__device__ __forceinline__ unsigned code_of(const unsigned (&c)[N], int j, int q) { return code_of(c[j >> 1], j, q); }

// One of the lane's code words: blocks of the dictionary pool (DICT) live in L1 / L2 and take cached loads, streamed slices are
// read once: non-temporal loads.  (The loop over a lane's words stays in the kernel: inside a helper the pair kernels compile to
// another schedule, 0.551 -> 0.560 ms for the fp32 dictionary product at 512^3: profiles/slices_header_ab.json.)
template <bool DICT>
__device__ __forceinline__ unsigned load_code(const unsigned *p)
{
    if constexpr (DICT) return *p;
    else return __builtin_nontemporal_load(p);
}

// x for the two rows of a lane in one ELL column of a diagonal-coded slice (why and what was measured: sell8.hip, "PAIR kernels",
// above sell8_pair_kernel): ONE 16-byte load when both rows sit on the same diagonal or one of them is padding that allows it
// (code 255), an 8-byte load per real entry otherwise; padding reads as 0.  c0 / c1: the two rows' codes,
// d: s_delta[c0 is real ? c0 : c1], looked up once per column by the caller; safe: a harmless address, the diagonal table.
template <typename V>
__device__ __forceinline__ void gather_pair(const V *__restrict__ x, long long i, unsigned c0, unsigned c1, int d,
        const int *s_delta, const int *__restrict__ safe, V &x0, V &x1)
{
    typedef typename vec2<V>::type V2;
    const bool m0 = c0 < PAD_UNSAFE, m1 = c1 < PAD_UNSAFE;
    const bool pair = (c0 == c1) || (c0 == PAD && m1) || (c1 == PAD && m0);
    const bool use16 = pair && (m0 || m1);
    V2 p = {V(0), V(0)};
    if (__builtin_amdgcn_ballot_w64(use16) != 0) {          // skipped only when no lane of the wave has a pair here
        const V *px = use16 ? x + (i + d) : reinterpret_cast<const V *>(safe);
        __builtin_memcpy(&p, px, sizeof(V2));
    }
    x0 = p.x; x1 = p.y;
    if (!pair) {                                            // different diagonals in one lane, or a 16-byte load that would leave x
        if (m0) x0 = x[i + s_delta[c0]];
        if (m1) x1 = x[i + 1 + s_delta[c1]];
    }
    x0 = m0 ? x0 : V(0);
    x1 = m1 ? x1 : V(0);
}

// The CSR tail (rows wider than the ELL width) of a lane's two rows i, i + 1 for NR right-hand sides: sum[k][q] += A(i + q, :) xs[k],
// entries in CSR order.  xs: the NR vectors (X: a pointer to pointers to V, restrict-qualified or not); a single-vector kernel
// passes &x and &sum.
template <typename V, int NR = 1, typename X>
__device__ __forceinline__ void add_csr_tail(long long n, long long i, const int *__restrict__ csr_ptr, const int *__restrict__ csr_col,
        const V *__restrict__ csr_val, X xs, V (*sum)[2])
{
    if (!csr_ptr) return;
#pragma unroll
    for (int q = 0; q < 2; ++q)
        if (i + q < n)
            for (int j = csr_ptr[i + q], e = csr_ptr[i + q + 1]; j < e; ++j) {
                const int c = csr_col[j]; const V v = csr_val[j];
#pragma unroll
                for (int k = 0; k < NR; ++k) sum[k][q] += v * xs[k][c];
            }
}

} // namespace
} // namespace vexhip
