// Multi-right-hand-side products  Y_k (+)= alpha * A * X_k,  k < nrhs, for the
// SELL-512 and SELL8 storage of spmv.hip / sell8.hip: `SpMat * multivector`
// (reference: vexcl/spmat.hpp:388-398 applies the product component by
// component, streaming the matrix nrhs times).
//
// The matrix stream (9-12 B per entry) dominates a product's HBM traffic, the
// x/y vectors are 16 B per ROW.  One launch therefore reads every slice ONCE and
// reuses each (column, value) pair for up to four right-hand sides held in
// registers: for the 7-point Poisson matrix two right-hand sides cost 1.18x the
// bytes of one instead of 2x.  Per right-hand side the arithmetic and its order
// are exactly the single-vector kernels' (this file is compiled with
// -ffp-contract=off too), so every Y_k is bit-identical to the separate product.
#include "common.hpp"
#include "traversal.hpp"
#include "storage.hpp"
#include "dispatch.hpp"
#include "slices.hpp"

namespace vexhip {
namespace {

constexpr int MAX_NR = 4;

typedef int int2v __attribute__((ext_vector_type(2)));

template <typename V> struct rhs_set { const V *x[MAX_NR]; V *y[MAX_NR]; };

template <typename V, int NR>
__device__ __forceinline__ void tail_and_store(long long n, long long i, V alpha, int append,
        const int *__restrict__ csr_ptr, const int *__restrict__ csr_col, const V *__restrict__ csr_val,
        const rhs_set<V> &io, V (&sum)[NR][2])
{
    add_csr_tail<V, NR>(n, i, csr_ptr, csr_col, csr_val, io.x, sum);
#pragma unroll
    for (int k = 0; k < NR; ++k)
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (i + q < n) {
                V o = alpha * sum[k][q];
                if (append) o = io.y[k][i + q] + o;
                io.y[k][i + q] = o;
            }
}

// ---- SELL8 and SELL8V: 1-byte diagonal codes; matrix values stored in the slice or (VCODED) as 1-byte value codes (layouts: sell8.hip) ----
// `values` is unused by the stored-value form, `pool` by the value-coded one, whose whole storage is the pool when it has a dictionary.
template <typename V, int W, int NR, bool VCODED>
__global__ __launch_bounds__(256)
void spmm_coded_kernel(long long n, long long nslices, V alpha, int append, int ell_w,
        const char *__restrict__ buf, const int *__restrict__ deltas, const V *__restrict__ values,
        const int *__restrict__ csr_ptr, const int *__restrict__ csr_col, const V *__restrict__ csr_val,
        rhs_set<V> io, trav_dev trav, const char *__restrict__ pool, const int *__restrict__ blocks)
{
    __shared__ int s_delta[256];
    __shared__ V s_value[VCODED ? 256 : 1];
    s_delta[threadIdx.x] = deltas[threadIdx.x];
    if constexpr (VCODED) s_value[threadIdx.x] = values[threadIdx.x];
    __syncthreads();

    const long long s = traversal_block(trav, nslices);
    if (s < 0) return;
    const int t = threadIdx.x;
    const long long i = s * SLICE_ROWS + 2 * t;
    const int w = W > 0 ? W : ell_w;
    const int wp = (w + 1) / 2;
    const long long code_bytes = (long long)wp * (VCODED ? 2048 : 1024);
    const char *slice = buf + s * (VCODED ? code_bytes : code_bytes + (long long)w * SLICE_ROWS * sizeof(V));
    // slice dictionary (sell8.hip): the codes of slice s are block blocks[s] of the pool of distinct code blocks; stored values stay in the
    // slice, a value-coded storage is its pool and arrives as buf
    const char *codes;
    if constexpr (VCODED) codes = buf + (blocks ? (long long)blocks[s] : s) * code_bytes;
    else codes = blocks ? pool + (long long)blocks[s] * code_bytes : slice;
    const unsigned *cw = reinterpret_cast<const unsigned *>(codes) + t;
    const V *vp = reinterpret_cast<const V *>(slice + code_bytes) + 2 * t;             // stored values
    const unsigned *vw = cw + wp * 256;                                                // value codes
    typedef typename vec2<V>::type V2;

    V sum[NR][2];
#pragma unroll
    for (int k = 0; k < NR; ++k) { sum[k][0] = V(0); sum[k][1] = V(0); }

    if constexpr (W > 0) {
        constexpr int WP = (W + 1) / 2;
        unsigned c[WP], vc[VCODED ? WP : 1];
#pragma unroll
        for (int jp = 0; jp < WP; ++jp) {
            if (blocks) { c[jp] = load_code<true>(cw + jp * 256); if constexpr (VCODED) vc[jp] = load_code<true>(vw + jp * 256); }
            else { c[jp] = load_code<false>(cw + jp * 256); if constexpr (VCODED) vc[jp] = load_code<false>(vw + jp * 256); }
        }
        // the matrix values: the slice's pairs as loaded, or looked up in s_value below
        V2 v[VCODED ? 1 : W]; V a[VCODED ? W : 1][2];
        if constexpr (!VCODED) {
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = __builtin_nontemporal_load(reinterpret_cast<const V2 *>(vp + j * SLICE_ROWS));
        }
        auto value = [&](int j, int q) -> V { if constexpr (VCODED) return a[j][q]; else return v[j][q]; };
        int d[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const unsigned c0 = code_of(c, j, 0), c1 = code_of(c, j, 1);
            d[j] = s_delta[c0 < PAD_UNSAFE ? c0 : c1];
            if constexpr (VCODED) {
                a[j][0] = s_value[c0 < PAD_UNSAFE ? code_of(vc, j, 0) : 255u];          // entry 255 is 0.0
                a[j][1] = s_value[c1 < PAD_UNSAFE ? code_of(vc, j, 1) : 255u];
            }
        }
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            V xv[W][2];
#pragma unroll
            for (int j = 0; j < W; ++j)
                gather_pair<V>(io.x[k], i, code_of(c, j, 0), code_of(c, j, 1), d[j], s_delta, deltas, xv[j][0], xv[j][1]);
            // padding: matrix value 0, gathered value 0 -- sum + (+-0) == sum bit for bit (the sum starts at +0)
#pragma unroll
            for (int j = 0; j < W; ++j)
#pragma unroll
                for (int q = 0; q < 2; ++q) sum[k][q] += value(j, q) * xv[j][q];
        }
    } else {
        for (int j = 0; j < w; ++j) {
            const unsigned cword = cw[(j >> 1) * 256];
            unsigned vword = 0; V2 vv = {V(0), V(0)};
            if constexpr (VCODED) vword = vw[(j >> 1) * 256];
            else vv = *reinterpret_cast<const V2 *>(vp + (long long)j * SLICE_ROWS);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const unsigned code = code_of(cword, j, q);
                if (code < PAD_UNSAFE) {
                    const long long cidx = i + q + s_delta[code];
                    V v;
                    if constexpr (VCODED) v = s_value[code_of(vword, j, q)];
                    else v = vv[q];
#pragma unroll
                    for (int k = 0; k < NR; ++k) sum[k][q] += v * io.x[k][cidx];
                }
            }
        }
    }
    tail_and_store<V, NR>(n, i, alpha, append, csr_ptr, csr_col, csr_val, io, sum);
}

// ---- SELL-512 with 32-bit columns (layout: spmv.hip) ---------------------------------------
template <typename V, int W, int NR>
__global__ __launch_bounds__(256)
void spmm_sell_kernel(long long n, long long nslices, V alpha, int append, int ell_w,
        const char *__restrict__ sell,
        const int *__restrict__ csr_ptr, const int *__restrict__ csr_col, const V *__restrict__ csr_val,
        rhs_set<V> io, trav_dev trav)
{
    const long long s = traversal_block(trav, nslices);
    if (s < 0) return;
    const int r = 2 * threadIdx.x;
    const long long i = s * SLICE_ROWS + r;
    const int w = W > 0 ? W : ell_w;
    const char *slice = sell + s * ((long long)w * SLICE_ROWS * (4 + (long long)sizeof(V)));
    const int *cp = reinterpret_cast<const int *>(slice) + r;
    const V *vp = reinterpret_cast<const V *>(slice + (long long)w * SLICE_ROWS * 4) + r;
    typedef typename vec2<V>::type V2;

    V sum[NR][2];
#pragma unroll
    for (int k = 0; k < NR; ++k) { sum[k][0] = V(0); sum[k][1] = V(0); }

    if constexpr (W > 0) {
        int2v c[W]; V2 v[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            c[j] = __builtin_nontemporal_load(reinterpret_cast<const int2v *>(cp + j * SLICE_ROWS));
            v[j] = __builtin_nontemporal_load(reinterpret_cast<const V2 *>(vp + j * SLICE_ROWS));
        }
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            V xv[W][2];
#pragma unroll
            for (int j = 0; j < W; ++j)
#pragma unroll
                for (int q = 0; q < 2; ++q) xv[j][q] = (c[j][q] >= 0) ? io.x[k][c[j][q]] : V(0);
#pragma unroll
            for (int j = 0; j < W; ++j)
#pragma unroll
                for (int q = 0; q < 2; ++q) if (c[j][q] >= 0) sum[k][q] += v[j][q] * xv[j][q];
        }
    } else {
        for (int j = 0; j < w; ++j) {
            const int2v c = *reinterpret_cast<const int2v *>(cp + (long long)j * SLICE_ROWS);
            const V2 v = *reinterpret_cast<const V2 *>(vp + (long long)j * SLICE_ROWS);
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (c[q] >= 0) {
#pragma unroll
                    for (int k = 0; k < NR; ++k) sum[k][q] += v[q] * io.x[k][c[q]];
                }
        }
    }
    tail_and_store<V, NR>(n, i, alpha, append, csr_ptr, csr_col, csr_val, io, sum);
}

// CODES: 0 = 32-bit columns, 1 = diagonal codes, 2 = diagonal and value codes
template <typename V, int CODES, int NR>
void launch(hipStream_t s, long long grid, long long n, long long ns, V alpha, int append, int w, const char *buf,
        const int *deltas, const V *values, const int *cp, const int *cc, const V *cv, const rhs_set<V> &io, const trav_dev &t,
        const char *pool, const int *blocks)
{
    with_width_of<3, 5, 7, 9>(w, [&](auto W) {    // unrolled for the usual stencil widths (1-D, 2-D 5/9-point, 3-D 7-point); any other width loops
        if constexpr (CODES > 0) spmm_coded_kernel<V, W(), NR, CODES == 2><<<(unsigned)grid, 256, 0, s>>>(n, ns, alpha, append, w, buf, deltas, values, cp, cc, cv, io, t, pool, blocks);
        else spmm_sell_kernel<V, W(), NR><<<(unsigned)grid, 256, 0, s>>>(n, ns, alpha, append, w, buf, cp, cc, cv, io, t);
    });
}

} // namespace

// nrhs products in passes of up to MAX_NR right-hand sides (storage.hpp)
template <typename V, int CODES>
int spmm(int dev, void *stream, int64_t n, int nrhs, V alpha, int append, int64_t w, const void *buf, const int *deltas, const V *values,
        const int *cp, const int *cc, const V *cv, const V *const *x, V *const *y, const vexhip_traversal *tr, const int *blocks, const void *pool_)
{
    VEXHIP_REQUIRE(n >= 0 && w >= 1 && w < (1 << 20) && nrhs >= 1, "bad SpMM geometry");
    if (n == 0) return 0;
    VEXHIP_REQUIRE(buf && x && y && (CODES == 0 || deltas) && (CODES != 2 || values) && (reinterpret_cast<uintptr_t>(buf) & 15) == 0,
            "NULL argument or misaligned matrix buffer");
    for (int k = 0; k < nrhs; ++k) VEXHIP_REQUIRE(x[k] && y[k], "NULL right-hand side or result");
    VEXHIP_SET_DEVICE(dev);
    hipStream_t s = as_stream(stream);
    const long long ns = (n + SLICE_ROWS - 1) / SLICE_ROWS;
    long long grid = 0;
    const trav_dev t = make_traversal(tr, ns, &grid);
    VEXHIP_REQUIRE(grid < (1ll << 31), "matrix too large for one launch");
    const char *b = static_cast<const char *>(buf), *pool = static_cast<const char *>(pool_);
    for (int k0 = 0; k0 < nrhs; k0 += MAX_NR) {
        const int nr = nrhs - k0 < MAX_NR ? nrhs - k0 : MAX_NR;
        rhs_set<V> io;
        for (int k = 0; k < MAX_NR; ++k) { io.x[k] = x[k0 + (k < nr ? k : 0)]; io.y[k] = y[k0 + (k < nr ? k : 0)]; }
        with_width<MAX_NR>(nr, [&](auto NR) {
            if constexpr (NR() > 0)             // nr is 1..MAX_NR
                launch<V, CODES, NR()>(s, grid, n, ns, alpha, append, (int)w, b, deltas, values, cp, cc, cv, io, t, pool, blocks);
        });
        VEXHIP_LAUNCH_CHECK();
    }
    return 0;
}

#define VEXHIP_INSTANTIATE(V, CODES) template int spmm<V, CODES>(int, void *, int64_t, int, V, int, int64_t, const void *, const int *, const V *, const int *, const int *, const V *, \
        const V *const *, V *const *, const vexhip_traversal *, const int *, const void *);
VEXHIP_INSTANTIATE(double, 0) VEXHIP_INSTANTIATE(double, 1) VEXHIP_INSTANTIATE(double, 2) VEXHIP_INSTANTIATE(float, 0) VEXHIP_INSTANTIATE(float, 1) VEXHIP_INSTANTIATE(float, 2)
#undef VEXHIP_INSTANTIATE

} // namespace vexhip

using namespace vexhip;

extern "C" {

int vexhip_spmm_sell8_f64_i32(int dev, void *stream, int64_t n, int nrhs, double alpha, int append, int64_t w,
        const void *buf, const int32_t *deltas, const int32_t *cp, const int32_t *cc, const double *cv,
        const double *const *x, double *const *y, const vexhip_traversal *traversal)
{ return spmm<double, 1>(dev, stream, n, nrhs, alpha, append, w, buf, deltas, nullptr, cp, cc, cv, x, y, traversal); }

int vexhip_spmm_sell8_f32_i32(int dev, void *stream, int64_t n, int nrhs, float alpha, int append, int64_t w,
        const void *buf, const int32_t *deltas, const int32_t *cp, const int32_t *cc, const float *cv,
        const float *const *x, float *const *y, const vexhip_traversal *traversal)
{ return spmm<float, 1>(dev, stream, n, nrhs, alpha, append, w, buf, deltas, nullptr, cp, cc, cv, x, y, traversal); }

int vexhip_spmm_sell_f64_i32(int dev, void *stream, int64_t n, int nrhs, double alpha, int append, int64_t w,
        const void *sell, const int32_t *cp, const int32_t *cc, const double *cv,
        const double *const *x, double *const *y, const vexhip_traversal *traversal)
{ return spmm<double, 0>(dev, stream, n, nrhs, alpha, append, w, sell, nullptr, nullptr, cp, cc, cv, x, y, traversal); }

int vexhip_spmm_sell_f32_i32(int dev, void *stream, int64_t n, int nrhs, float alpha, int append, int64_t w,
        const void *sell, const int32_t *cp, const int32_t *cc, const float *cv,
        const float *const *x, float *const *y, const vexhip_traversal *traversal)
{ return spmm<float, 0>(dev, stream, n, nrhs, alpha, append, w, sell, nullptr, nullptr, cp, cc, cv, x, y, traversal); }

int vexhip_spmm_sell8v_f64_i32(int dev, void *stream, int64_t n, int nrhs, double alpha, int append, int64_t w,
        const void *buf, const int32_t *deltas, const double *values, const int32_t *cp, const int32_t *cc, const double *cv,
        const double *const *x, double *const *y, const vexhip_traversal *traversal)
{ return spmm<double, 2>(dev, stream, n, nrhs, alpha, append, w, buf, deltas, values, cp, cc, cv, x, y, traversal); }

int vexhip_spmm_sell8v_f32_i32(int dev, void *stream, int64_t n, int nrhs, float alpha, int append, int64_t w,
        const void *buf, const int32_t *deltas, const float *values, const int32_t *cp, const int32_t *cc, const float *cv,
        const float *const *x, float *const *y, const vexhip_traversal *traversal)
{ return spmm<float, 2>(dev, stream, n, nrhs, alpha, append, w, buf, deltas, values, cp, cc, cv, x, y, traversal); }

int vexhip_spmm_sell8_dict_f64_i32(int dev, void *stream, int64_t n, int nrhs, double alpha, int append, int64_t w,
        const void *buf, const void *pool, const int32_t *blocks, const int32_t *deltas, const int32_t *cp, const int32_t *cc, const double *cv,
        const double *const *x, double *const *y, const vexhip_traversal *traversal)
{ return spmm<double, 1>(dev, stream, n, nrhs, alpha, append, w, buf, deltas, nullptr, cp, cc, cv, x, y, traversal, blocks, pool); }

int vexhip_spmm_sell8_dict_f32_i32(int dev, void *stream, int64_t n, int nrhs, float alpha, int append, int64_t w,
        const void *buf, const void *pool, const int32_t *blocks, const int32_t *deltas, const int32_t *cp, const int32_t *cc, const float *cv,
        const float *const *x, float *const *y, const vexhip_traversal *traversal)
{ return spmm<float, 1>(dev, stream, n, nrhs, alpha, append, w, buf, deltas, nullptr, cp, cc, cv, x, y, traversal, blocks, pool); }

int vexhip_spmm_sell8v_dict_f64_i32(int dev, void *stream, int64_t n, int nrhs, double alpha, int append, int64_t w,
        const void *pool, const int32_t *blocks, const int32_t *deltas, const double *values, const int32_t *cp, const int32_t *cc, const double *cv,
        const double *const *x, double *const *y, const vexhip_traversal *traversal)
{ return spmm<double, 2>(dev, stream, n, nrhs, alpha, append, w, pool, deltas, values, cp, cc, cv, x, y, traversal, blocks); }

int vexhip_spmm_sell8v_dict_f32_i32(int dev, void *stream, int64_t n, int nrhs, float alpha, int append, int64_t w,
        const void *pool, const int32_t *blocks, const int32_t *deltas, const float *values, const int32_t *cp, const int32_t *cc, const float *cv,
        const float *const *x, float *const *y, const vexhip_traversal *traversal)
{ return spmm<float, 2>(dev, stream, n, nrhs, alpha, append, w, pool, deltas, values, cp, cc, cv, x, y, traversal, blocks); }

} // extern "C"

VEXHIP_WARM_TU(spmm)
