// The jumping-knowledge step (see bmp_jk.hip) over a TILE TABLE: the VAR instances of jk_step_fwd / jk_step_bwd<D, NG> of
// bmp_wtile_jk.h, for batches in the encoder layout (bmp/enclayout.py, with or without de-duplication) and for the fixed-shape
// batch (bmp.packed.StaticPairBatch), which the whole-tile entries of bmp_jk.hip cannot take.  One workgroup of 512 threads per
// table entry of 1..4 live 32-row blocks, the same two [128][d + 4] LDS tiles; the waves of a dead block skip their products.
// 2 directions x 2 update widths x 2 widths = 8 kernels, none of which spills.
#include "bmp_kernels.h"
#include "bmp_wtile_jk.h"

#define JKT_FWD_ARGS const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,                 \
                     const float* __restrict__ val, const float* __restrict__ WTp, const float* __restrict__ bE,             \
                     const float* __restrict__ WsTp, const float* __restrict__ bs, const float* __restrict__ AUp,            \
                     const float* __restrict__ bU, float* __restrict__ m, float* __restrict__ out, WgTable tt
#define JKT_BWD_ARGS const float* __restrict__ dout, const float* __restrict__ out, const int* __restrict__ ptrT,           \
                     const int* __restrict__ colT, const float* __restrict__ valT, const float* __restrict__ Wnp,            \
                     const float* __restrict__ Wsp, const float* __restrict__ Unp, float* __restrict__ dh,                   \
                     float* __restrict__ gda, WgTable tt

template <int D> __global__ __launch_bounds__(512) void k_jk_step1_table_fwd(JKT_FWD_ARGS) {
    jk_step_fwd<D, 1, true>(h, ptr, col, val, WTp, bE, WsTp, bs, AUp, bU, m, out, tt);
}
template <int D> __global__ __launch_bounds__(512) void k_jk_step2_table_fwd(JKT_FWD_ARGS) {
    jk_step_fwd<D, 2, true>(h, ptr, col, val, WTp, bE, WsTp, bs, AUp, bU, m, out, tt);
}
template <int D> __global__ __launch_bounds__(512) void k_jk_step1_table_bwd(JKT_BWD_ARGS) {
    jk_step_bwd<D, 1, true>(dout, out, ptrT, colT, valT, Wnp, Wsp, Unp, dh, gda, tt);
}
template <int D> __global__ __launch_bounds__(512) void k_jk_step2_table_bwd(JKT_BWD_ARGS) {
    jk_step_bwd<D, 2, true>(dout, out, ptrT, colT, valT, Wnp, Wsp, Unp, dh, gda, tt);
}

extern "C" int bmp_jk_step_table_supported(int d) { return bmp_jk_step_supported(d); }

// bmp_jk_step_tile_fwd over a tile table: n_tiles table entries, mt_rows rows in the arrays; tile_stride 0 (dense rows) or the
// fixed stride of the table's tiles, whose dead rows are then cleared in m and out.
extern "C" int bmp_jk_step_table_fwd(int ng, const float* h, int n_tiles, int d, const int* csr_ptr, const int* csr_col,
                                     const float* csr_val, const float* WTp, const float* bE, const float* WsTp, const float* bs,
                                     const float* AUp, const float* bU, float* m, float* out, const int* mt_row0, const int* mt_nblk,
                                     int mt_rows, int tile_stride, hipStream_t st) {
    BMP_REQUIRE(bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, tile_stride, WT_R));
    if (int rc = jk_fwd_check(bmp_jk_step_table_supported(d), ng, h, n_tiles, csr_ptr, WTp, bE, WsTp, bs, AUp, bU, m, out)) return rc;
    const WgTable tt = {mt_row0, mt_nblk, mt_rows, tile_stride};
    if (ng == 1)
        WT_LAUNCH(k_jk_step1_table_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, WTp, bE, WsTp, bs, AUp, bU, m, out, tt);
    else
        WT_LAUNCH(k_jk_step2_table_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, WTp, bE, WsTp, bs, AUp, bU, m, out, tt);
    return 0;
}

// ... and its backward: the dead rows of a fixed-stride table are cleared in dh and gda.
extern "C" int bmp_jk_step_table_bwd(int ng, const float* dout, const float* out, int n_tiles, int d, const int* csrT_ptr,
                                     const int* csrT_col, const float* csrT_val, const float* Wnat_p, const float* Ws_p,
                                     const float* Unat_p, float* dh, float* gda, const int* mt_row0, const int* mt_nblk, int mt_rows,
                                     int tile_stride, hipStream_t st) {
    BMP_REQUIRE(bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, tile_stride, WT_R));
    if (int rc = jk_bwd_check(bmp_jk_step_table_supported(d), ng, dout, out, n_tiles, csrT_ptr, Wnat_p, Ws_p, Unat_p, dh, gda)) return rc;
    const WgTable tt = {mt_row0, mt_nblk, mt_rows, tile_stride};
    if (ng == 1)
        WT_LAUNCH(k_jk_step1_table_bwd, d, n_tiles, wt_lds_bytes(d), st, dout, out, csrT_ptr, csrT_col, csrT_val, Wnat_p, Ws_p, Unat_p, dh, gda, tt);
    else
        WT_LAUNCH(k_jk_step2_table_bwd, d, n_tiles, wt_lds_bytes(d), st, dout, out, csrT_ptr, csrT_col, csrT_val, Wnat_p, Ws_p, Unat_p, dh, gda, tt);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// 'mean' over a ROW COUNT (a tile-table batch's rows are no multiple of 128 and have no sides to look up): the two bodies above
// over n4 = n_rows d / 4 units with c_t = ct = 1 / T for every t.
template <int T>
__global__ __launch_bounds__(JK_TPB) void k_jk_mean_fwd(JkIn h, size_t n4, float ct, float* __restrict__ y) {
    float c[T];
#pragma unroll
    for (int t = 0; t < T; ++t) c[t] = ct;
    const size_t stride = (size_t)gridDim.x * JK_TPB;
    for (size_t u = (size_t)blockIdx.x * JK_TPB + threadIdx.x; u < n4; u += stride) reinterpret_cast<f32x4*>(y)[u] = jk_comb_unit<T>(h, u, c);
}
template <int T>
__global__ __launch_bounds__(JK_TPB) void k_jk_mean_bwd(const float* __restrict__ dy, size_t n4, float ct, JkOut dh) {
    float c[T];
#pragma unroll
    for (int t = 0; t < T; ++t) c[t] = ct;
    const size_t stride = (size_t)gridDim.x * JK_TPB;
    for (size_t u = (size_t)blockIdx.x * JK_TPB + threadIdx.x; u < n4; u += stride)
        jk_scale_unit<T>(dh, u, reinterpret_cast<const f32x4*>(dy)[u], c);
}

// 'mean' on a row count: h, T host pointers to the step outputs [n_rows x d]; y [n_rows x d] = (1 / T) sum_t h[t].  No access
// goes past row n_rows.
extern "C" int bmp_jk_mean_fwd(const float* const* h, int T, int n_rows, int d, float* y, hipStream_t st) {
    BMP_REQUIRE(h && T >= 1 && T <= JK_MAXT && n_rows > 0 && d > 0 && d % 4 == 0 && y && jk_aligned(y));
    JkIn in = {};
    for (int t = 0; t < T; ++t) {
        BMP_REQUIRE(h[t] && jk_aligned(h[t]));
        in.p[t] = h[t];
    }
    const size_t n4 = (size_t)n_rows * (d / 4);
#define JK_CASE(TT) case TT: hipLaunchKernelGGL((k_jk_mean_fwd<TT>), dim3(jk_blocks(n4)), dim3(JK_TPB), 0, st, in, n4, 1.0f / (float)T, y); break;
    JK_T_SWITCH(T, JK_CASE)
#undef JK_CASE
    BMP_LAUNCH_CHECK();
    return 0;
}

// ... and its backward: dh[t] [n_rows x d] = dy / T for every t.
extern "C" int bmp_jk_mean_bwd(const float* dy, int T, int n_rows, int d, float* const* dh, hipStream_t st) {
    BMP_REQUIRE(dy && jk_aligned(dy) && dh && T >= 1 && T <= JK_MAXT && n_rows > 0 && d > 0 && d % 4 == 0);
    JkOut out = {};
    for (int t = 0; t < T; ++t) {
        BMP_REQUIRE(dh[t] && jk_aligned(dh[t]));
        out.p[t] = dh[t];
    }
    const size_t n4 = (size_t)n_rows * (d / 4);
#define JK_CASE(TT) case TT: hipLaunchKernelGGL((k_jk_mean_bwd<TT>), dim3(jk_blocks(n4)), dim3(JK_TPB), 0, st, dy, n4, 1.0f / (float)T, out); break;
    JK_T_SWITCH(T, JK_CASE)
#undef JK_CASE
    BMP_LAUNCH_CHECK();
    return 0;
}
