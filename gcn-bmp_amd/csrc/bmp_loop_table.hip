// The self-loop GGNN step (see bmp_loop.hip) over a TILE TABLE: the VAR instances of wg_step_fwd / wg_step_bwd<D, FIRST,
// WG_SELF_LOOP> of bmp_wtile_gru.h, for batches in the encoder layout (bmp/enclayout.py, with or without de-duplication) and for
// the fixed-shape batch (bmp.packed.StaticPairBatch), which the whole-tile entries of bmp_loop.hip cannot take.  One workgroup of
// 512 threads per table entry of 1..4 live 32-row blocks, the same two [128][d + 4] LDS tiles; the waves of a dead block skip
// their products.  2 directions x 2 call forms x 2 widths = 8 kernels, none of which spills.
#include "bmp_wtile_gru.h"

#define LOOPT_FWD_ARGS const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col, const float* __restrict__ val,           \
                       const float* __restrict__ WTp, const float* __restrict__ bE, const float* __restrict__ WsTp, const float* __restrict__ bs,      \
                       const float* __restrict__ ATp, const float* __restrict__ UcTp, const float* __restrict__ b, float* __restrict__ m,              \
                       float* __restrict__ rz, float* __restrict__ c, float* __restrict__ hout, WgTable tt
#define LOOPT_BWD_ARGS const float* __restrict__ dhout, const float* __restrict__ h, const float* __restrict__ rz, const float* __restrict__ c,        \
                       const int* __restrict__ ptrT, const int* __restrict__ colT, const float* __restrict__ valT, const float* __restrict__ Wnp,      \
                       const float* __restrict__ Wsp, const float* __restrict__ Anp, const float* __restrict__ Ucp, float* __restrict__ dh,            \
                       float* __restrict__ gda, float* __restrict__ rh, WgTable tt

template <int D> __global__ __launch_bounds__(512) void k_loop_step_first_table_fwd(LOOPT_FWD_ARGS) {
    wg_step_fwd<D, true, WG_SELF_LOOP, true>(h, ptr, col, val, EdgeSeg{}, WTp, bE, WsTp, bs, ATp, UcTp, b, m, rz, c, hout, tt);
}
template <int D> __global__ __launch_bounds__(512) void k_loop_step_later_table_fwd(LOOPT_FWD_ARGS) {
    wg_step_fwd<D, false, WG_SELF_LOOP, true>(h, ptr, col, val, EdgeSeg{}, WTp, bE, WsTp, bs, ATp, UcTp, b, m, rz, c, hout, tt);
}
template <int D> __global__ __launch_bounds__(512) void k_loop_step_first_table_bwd(LOOPT_BWD_ARGS) {
    wg_step_bwd<D, true, WG_SELF_LOOP, true>(dhout, h, rz, c, ptrT, colT, valT, EdgeSeg{}, Wnp, Wsp, Anp, Ucp, dh, gda, rh, tt);
}
template <int D> __global__ __launch_bounds__(512) void k_loop_step_later_table_bwd(LOOPT_BWD_ARGS) {
    wg_step_bwd<D, false, WG_SELF_LOOP, true>(dhout, h, rz, c, ptrT, colT, valT, EdgeSeg{}, Wnp, Wsp, Anp, Ucp, dh, gda, rh, tt);
}

extern "C" int bmp_ggnn_loop_step_supported(int d);           // bmp_loop.hip
extern "C" int bmp_ggnn_loop_step_table_supported(int d) { return bmp_ggnn_loop_step_supported(d); }

// bmp_ggnn_loop_step_tile_fwd over a tile table: n_tiles table entries, mt_rows rows in the arrays; tile_stride 0 (dense rows) or
// the fixed stride of the table's tiles, whose dead rows are then cleared in m, rz, c and hout.
extern "C" int bmp_ggnn_loop_step_table_fwd(const float* h, int n_tiles, int d, int first, const int* csr_ptr, const int* csr_col,
                                            const float* csr_val, const float* WTp, const float* bE, const float* WsTp, const float* bs,
                                            const float* ATp, const float* UcTp, const float* b, float* m, float* rz, float* c,
                                            float* hout, const int* mt_row0, const int* mt_nblk, int mt_rows, int tile_stride,
                                            hipStream_t st) {
    BMP_REQUIRE(bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, tile_stride, WT_R));
    BMP_REQUIRE(bE && bs && (((uintptr_t)bE | (uintptr_t)bs) & 15) == 0);
    if (int rc = wg_fwd_check(bmp_ggnn_loop_step_table_supported(d), h, n_tiles, first, csr_ptr, WTp, WsTp, ATp, UcTp, b, m, rz, c, hout)) return rc;
    const WgTable tt = {mt_row0, mt_nblk, mt_rows, tile_stride};
    if (first)
        WT_LAUNCH(k_loop_step_first_table_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, WTp, bE, WsTp, bs, ATp, UcTp, b, m, rz, c, hout, tt);
    else
        WT_LAUNCH(k_loop_step_later_table_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, WTp, bE, WsTp, bs, ATp, UcTp, b, m, rz, c, hout, tt);
    return 0;
}

// ... and its backward: the dead rows of a fixed-stride table are cleared in dh, gda and rh.
extern "C" int bmp_ggnn_loop_step_table_bwd(const float* dhout, const float* h, const float* rz, const float* c, int n_tiles, int d,
                                            int first, const int* csrT_ptr, const int* csrT_col, const float* csrT_val,
                                            const float* Wnat_p, const float* Ws_p, const float* A_p, const float* Uc_p, float* dh,
                                            float* gda, float* rh, const int* mt_row0, const int* mt_nblk, int mt_rows, int tile_stride,
                                            hipStream_t st) {
    BMP_REQUIRE(bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, tile_stride, WT_R));
    if (int rc = wg_bwd_check(bmp_ggnn_loop_step_table_supported(d), dhout, h, rz, c, n_tiles, first, csrT_ptr, Wnat_p, Ws_p, A_p, Uc_p, dh, gda, rh)) return rc;
    const WgTable tt = {mt_row0, mt_nblk, mt_rows, tile_stride};
    if (first)
        WT_LAUNCH(k_loop_step_first_table_bwd, d, n_tiles, wt_lds_bytes(d), st, dhout, h, rz, c, csrT_ptr, csrT_col, csrT_val, Wnat_p, Ws_p, A_p, Uc_p, dh, gda, rh, tt);
    else
        WT_LAUNCH(k_loop_step_later_table_bwd, d, n_tiles, wt_lds_bytes(d), st, dhout, h, rz, c, csrT_ptr, csrT_col, csrT_val, Wnat_p, Ws_p, A_p, Uc_p, dh, gda, rh, tt);
    return 0;
}
