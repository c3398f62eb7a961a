// The GIN layer (see bmp_gin.hip) over a TILE TABLE: the VAR instances of gin_layer_fwd / gin_layer_bwd<D> of bmp_wtile_gin.h,
// for batches in the encoder layout (bmp/enclayout.py, with or without de-duplication) and for the fixed-shape batch
// (bmp.packed.StaticPairBatch), which the whole-tile entries of bmp_gin.hip cannot take.  One workgroup of 512 threads per table
// entry of 1..4 live 32-row blocks, the same two [128][d + 4] LDS tiles; the waves of a dead block skip their products.  The
// forward takes s == t == null (a uniform branch) and then keeps nothing for a backward.
// 2 directions x 2 widths = 4 kernels, none of which spills.
#include "bmp_kernels.h"
#include "bmp_wtile_gin.h"

template <int D>
__global__ __launch_bounds__(512) void k_gin_table_fwd(const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,
                                                       const float* __restrict__ val, const float* __restrict__ W1p,
                                                       const float* __restrict__ b1, const float* __restrict__ W2p,
                                                       const float* __restrict__ b2, const float* __restrict__ keep,
                                                       float* __restrict__ s, float* __restrict__ t, float* __restrict__ out, WgTable tt) {
    gin_layer_fwd<D, true>(h, ptr, col, val, W1p, b1, W2p, b2, keep, s, t, out, tt);
}

template <int D>
__global__ __launch_bounds__(512) void k_gin_table_bwd(const float* __restrict__ dout, const float* __restrict__ out,
                                                       const float* __restrict__ keep, const float* __restrict__ t,
                                                       const int* __restrict__ ptrT, const int* __restrict__ colT,
                                                       const float* __restrict__ valT, const float* __restrict__ W2np,
                                                       const float* __restrict__ W1np, float* __restrict__ dp2,
                                                       float* __restrict__ dp1, float* __restrict__ dh, WgTable tt) {
    gin_layer_bwd<D, true>(dout, out, keep, t, ptrT, colT, valT, W2np, W1np, dp2, dp1, dh, tt);
}

extern "C" int bmp_gin_layer_table_supported(int d) { return bmp_gin_layer_supported(d); }

// bmp_gin_layer_tile_fwd over a tile table: n_tiles table entries, mt_rows rows in the arrays; tile_stride 0 (dense rows) or the
// fixed stride of the table's tiles, whose dead rows are then cleared in s, t and out.  s and t both null: forward only.
extern "C" int bmp_gin_layer_table_fwd(const float* h, int n_tiles, int d, const int* csr_ptr, const int* csr_col, const float* csr_val,
                                       const float* W1p, const float* b1, const float* W2p, const float* b2, const float* keep,
                                       float* s, float* t, float* out, const int* mt_row0, const int* mt_nblk, int mt_rows,
                                       int tile_stride, hipStream_t st) {
    BMP_REQUIRE(bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, tile_stride, WT_R));
    if (int rc = gin_fwd_check(bmp_gin_layer_table_supported(d), (s == nullptr) == (t == nullptr), h, n_tiles, csr_ptr, W1p, b1, W2p, b2,
                               keep, s, t, out))
        return rc;
    const WgTable tt = {mt_row0, mt_nblk, mt_rows, tile_stride};
    WT_LAUNCH(k_gin_table_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, W1p, b1, W2p, b2, keep, s, t, out, tt);
    return 0;
}

// ... and its backward: the dead rows of a fixed-stride table are cleared in dp2, dp1 and dh.
extern "C" int bmp_gin_layer_table_bwd(const float* dout, const float* out, const float* keep, const float* t, int n_tiles, int d,
                                       const int* csrT_ptr, const int* csrT_col, const float* csrT_val, const float* W2np,
                                       const float* W1np, float* dp2, float* dp1, float* dh, const int* mt_row0, const int* mt_nblk,
                                       int mt_rows, int tile_stride, hipStream_t st) {
    BMP_REQUIRE(bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, tile_stride, WT_R));
    if (int rc = gin_bwd_check(bmp_gin_layer_table_supported(d), dout, out, keep, t, n_tiles, csrT_ptr, W2np, W1np, dp2, dp1, dh)) return rc;
    const WgTable tt = {mt_row0, mt_nblk, mt_rows, tile_stride};
    WT_LAUNCH(k_gin_table_bwd, d, n_tiles, wt_lds_bytes(d), st, dout, out, keep, t, csrT_ptr, csrT_col, csrT_val, W2np, W1np, dp2, dp1, dh, tt);
    return 0;
}
