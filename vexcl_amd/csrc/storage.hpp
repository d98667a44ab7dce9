// The typed interface between the translation units of libvexhip.so: what spmat.hip (the one place that decides how a matrix is
// stored and which product it launches) and comm.hip call in their sibling files.  V = double | float (values), P = int32_t |
// long long (row pointers; columns are 32-bit).  The templates are defined, and explicitly instantiated for the combinations in use,
// in the file named above each group; the extern "C" functions of include/vexhip.h are one-line calls of these.
#pragma once
#include "common.hpp"
#include "halo.hpp"
#include "traversal.hpp"

namespace vexhip {

extern int g_sell8_variant;            // sell8.hip (vexhip_spmv_sell8_set_variant): 0 = pair kernels (default), 1 = one gather per entry, 2 = no march

// ---- misc.hip: the hybrid-ELL rule; ell_col == NULL fills the CSR tail alone ----
template <typename P> int hell_analyze(int dev, void *stream, int64_t n, const P *ptr, int64_t *ell_width, int64_t *tail_nnz);
template <typename V, typename P>
int hell_fill(int dev, void *stream, int64_t n, const P *ptr, const int *col, const V *val, int64_t w, int64_t pitch, int *ell_col, V *ell_val,
        int *csr_ptr, int *csr_col, V *csr_val);

// ---- sell8.hip: set-up of the coded storages ----
template <typename P> int sell8_analyze(int dev, void *stream, int64_t n, const P *ptr, const int32_t *col, int64_t w, int32_t *deltas, int *ndeltas);
template <typename V, typename P> int sell8v_analyze(int dev, void *stream, int64_t n, const P *ptr, const V *val, int64_t w, V *values, int *nvalues);
// diagonals + values + the largest ELL column (*max_col; -1: none) in one pass over the CSR arrays
template <typename V, typename P>
int analyze_fused(int dev, void *stream, int64_t n, const P *ptr, const int *col, const V *val, int64_t w, int32_t *deltas, int *ndeltas, V *values, int *nvalues,
        int64_t *max_col);
// known_max_col: the largest ELL column where the caller knows it (-1: the fill looks for it); *max_col (may be NULL): the largest column stored
template <typename V, typename P>
int sell8v_fill(int dev, void *stream, int64_t n, const P *ptr, const int *col, const V *val, int64_t w, const int *deltas, int ndeltas, const V *values, int nvalues,
        void *buf, vexhip_traversal *trav, int64_t known_max_col, int64_t *max_col);
template <typename V, typename P>
int sell8_fill(int dev, void *stream, int64_t n, const P *ptr, const int *col, const V *val, int64_t w, const int *deltas, int ndeltas, void *buf, vexhip_traversal *trav,
        int64_t known_max_col, int64_t *max_col);
template <typename P> int csr_traversal(int dev, void *stream, int64_t n, const P *ptr, const int32_t *col, int rows_per_block, vexhip_traversal *traversal);
int slice_dictionary(int dev, void *stream, int64_t nslices, int64_t stride_bytes, int64_t slice_bytes, const void *buf, int64_t max_blocks, int32_t *blocks, void *pool,
        int64_t *nblocks);
template <typename V> int sell8v_runs_plan(int dev, void *stream, const void *pool, int64_t nblocks, int64_t w, const int *deltas, const V *values, int **desc_out);

// ---- sell8.hip: products (pool + blocks: a slice dictionary; march: the march plan where usable) ----
template <typename V>
int spmv_sell8(int dev, void *stream, int64_t n, V alpha, int append, int64_t w, const void *buf, const int *deltas, const int *cp, const int *cc, const V *cv,
        const V *x, V *y, const vexhip_traversal *tr, const void *pool = nullptr, const int *blocks = nullptr, addend add = {});
template <typename V>
int spmv_sell8v(int dev, void *stream, int64_t n, V alpha, int append, int64_t w, const void *buf, const int *deltas, const V *values, const int *cp, const int *cc,
        const V *cv, const V *x, V *y, const vexhip_traversal *tr, const int *blocks = nullptr, const vexhip_march *march = nullptr, addend add = {});
template <typename V>
int sell8v_runs_apply(int dev, void *stream, int64_t n, V alpha, int append, int64_t w, const void *pool, const int *blocks, const int *deltas, const V *values,
        const int *cp, const int *cc, const V *cv, const V *x, V *y, const vexhip_traversal *tr, const int *desc, long long x_last, addend add = {});
int sell8_apply_halo(int dev, hipStream_t s, long long own_rows, double alpha, int append, int w, bool vcoded, const void *buf, const void *pool,
        const int *blocks, const int *deltas, const double *values, const double *x, double *y, halo_dev H);

// ---- spmv.hip: 32-bit columns and CSR (I: row pointers and columns of one width; spmv_csr_wide: 64-bit row pointers, 32-bit columns) ----
template <typename V, typename P> int sell_fill(int dev, void *stream, int64_t n, const P *ptr, const int *col, const V *val, int64_t w, void *sell);
template <typename V>
int spmv_sell(int dev, void *stream, int64_t n, V alpha, int append, int64_t w, const void *sell, const int *cp, const int *cc, const V *cv, const V *x, V *y,
        const vexhip_traversal *tr, addend add = {});
template <typename V, typename I>
int spmv_csr(int dev, void *stream, int64_t n, V alpha, int append, const I *ptr, const I *col, const V *val, const V *x, V *y, const vexhip_traversal *tr = nullptr,
        addend add = {});
template <typename V>
int spmv_csr_wide(int dev, void *stream, int64_t n, V alpha, int append, const long long *ptr, const int32_t *col, const V *val, const V *x, V *y,
        const vexhip_traversal *tr, addend add = {});

// ---- spmm.hip: several right-hand sides; CODES: 0 = 32-bit columns, 1 = diagonal codes, 2 = diagonal and value codes ----
template <typename V, int CODES>
int spmm(int dev, void *stream, int64_t n, int nrhs, V alpha, int append, int64_t w, const void *buf, const int *deltas, const V *values, const int *cp, const int *cc,
        const V *cv, const V *const *x, V *const *y, const vexhip_traversal *tr, const int *blocks = nullptr, const void *pool = nullptr);

// ---- grid.hip / grid32.hip, plane.hip / plane32.hip: a matrix stored by grid line ----
template <typename V, typename P>
int grid_build(int dev, void *stream, int64_t rows, const P *ptr, const int32_t *col, const V *val, int32_t *deltas, V *values, int *ndeltas, int *nvalues,
        int64_t *ell_width, int64_t *x_last, vexhip_grid *out, int64_t min_cols);
int plane_plan_from_grid(int dev, const vexhip_grid *grid, int64_t rows, vexhip_plane *out);
// y = alpha A x + [zm 0: nothing | zm 1: beta zs | zm 2: beta x]
int plane_apply_axpby(int dev, void *stream, int64_t n, double alpha, int zm, const double *zs, double beta, int64_t w, const void *pool, const int32_t *blocks,
        const int32_t *deltas, const double *values, const double *x, double *y, const vexhip_plane *plane);
int plane_apply_axpby(int dev, void *stream, int64_t n, float alpha, int zm, const float *zs, float beta, int64_t w, const void *pool, const int32_t *blocks,
        const int32_t *deltas, const float *values, const float *x, float *y, const vexhip_plane *plane);
int grid_apply_axpby(int dev, void *stream, int64_t n, double alpha, int zm, const double *zs, double beta, const double *values, const double *x, double *y,
        const vexhip_grid *g);
int grid_apply_axpby(int dev, void *stream, int64_t n, float alpha, int zm, const float *zs, float beta, const float *values, const float *x, float *y,
        const vexhip_grid *g);
// y (=|+=) alpha A x: the addend is y itself
template <typename V>
inline int plane_apply(int dev, void *stream, int64_t n, V alpha, int append, int64_t w, const void *pool, const int32_t *blocks, const int32_t *deltas, const V *values,
        const V *x, V *y, const vexhip_plane *plane)
{ return plane_apply_axpby(dev, stream, n, alpha, append ? 1 : 0, y, V(1), w, pool, blocks, deltas, values, x, y, plane); }
template <typename V>
inline int grid_apply(int dev, void *stream, int64_t n, V alpha, int append, const V *values, const V *x, V *y, const vexhip_grid *g)
{ return grid_apply_axpby(dev, stream, n, alpha, append ? 1 : 0, y, V(1), values, x, y, g); }
// one rank's product step in one launch (halo.hpp)
int plane_apply_halo(int dev, hipStream_t s, int64_t n_ext, double alpha, int append, int64_t w, const void *pool, const int32_t *blocks, const int32_t *deltas,
        const double *values, const double *x, double *y, const vexhip_plane *plane, halo_dev H);
int plane_apply_halo(int dev, hipStream_t s, int64_t n_ext, float alpha, int append, int64_t w, const void *pool, const int32_t *blocks, const int32_t *deltas,
        const float *values, const float *x, float *y, const vexhip_plane *plane, halo_dev H);
int grid_apply_halo(int dev, hipStream_t s, int64_t n_ext, double alpha, int append, const double *values, const double *x, double *y, const vexhip_grid *g, halo_dev H);

// ---- spmat.hip: the stored strip of a rank as the operand of the one-launch step (comm.hip) ----
int spmat_halo_geometry(const vexhip_spmat *h, int *planes, int *lines_per_plane, int *line_length, int *value_type);
int spmat_halo_general(const vexhip_spmat *h, int64_t halo, int64_t rows_ext, int *reach, int *value_type);
int spmat_device(const vexhip_spmat *h, int *dev);
int spmat_apply_halo(const vexhip_spmat *h, hipStream_t s, double alpha, int append, const void *x, void *y, const halo_dev &H);

} // namespace vexhip
