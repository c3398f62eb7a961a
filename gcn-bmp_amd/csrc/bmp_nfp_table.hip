// The NFP layer and its softmax readout (see bmp_nfp.hip) over a TILE TABLE: the VAR instances of the four bodies of
// bmp_wtile_nfp.h, for batches in the encoder layout (bmp/enclayout.py, with or without de-duplication) and for the fixed-shape
// batch (bmp.packed.StaticPairBatch), which the whole-tile entries of bmp_nfp.hip cannot take.  One workgroup of 512 threads per
// table entry of 1..4 live 32-row blocks, the LDS of the whole-tile forms; the rows behind an entry's live rows rank as class 0
// without being loaded, and the waves of a ranked block without live rows skip their products.  The layer forward takes
// fv == null (a uniform branch) and then keeps nothing for a backward.
// 2 entries x 2 directions x 2 widths = 8 kernels, none of which spills.
#include "bmp_kernels.h"
#include "bmp_wtile_nfp.h"

template <int D>
__global__ __launch_bounds__(512) void k_nfp_table_fwd(const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col,
                                                       const float* __restrict__ val, const float* __restrict__ self_w,
                                                       const int* __restrict__ cls, const float* __restrict__ WTp,
                                                       const float* __restrict__ B, float* __restrict__ fv, float* __restrict__ out,
                                                       WgTable tt) {
    nfp_layer_fwd<D, true>(h, ptr, col, val, self_w, cls, WTp, B, fv, out, tt);
}

template <int D>
__global__ __launch_bounds__(512) void k_nfp_table_bwd(const float* __restrict__ dout, const float* __restrict__ out,
                                                       const int* __restrict__ ptrT, const int* __restrict__ colT,
                                                       const float* __restrict__ valT, const float* __restrict__ self_w,
                                                       const int* __restrict__ cls, const float* __restrict__ row_w,
                                                       const float* __restrict__ Wnp, float* __restrict__ dpre, float* __restrict__ dh,
                                                       WgTable tt) {
    nfp_layer_bwd<D, true>(dout, out, ptrT, colT, valT, self_w, cls, row_w, Wnp, dpre, dh, tt);
}

template <int D>
__global__ __launch_bounds__(512) void k_nfp_readout_table_fwd(const float* __restrict__ h, int o, const float* __restrict__ WoTp,
                                                               const float* __restrict__ bo, const float* __restrict__ row_w,
                                                               const int* __restrict__ row_mol, float* __restrict__ sout,
                                                               float* __restrict__ g, int accumulate, WgTable tt) {
    nfp_readout_fwd<D, true>(h, o, WoTp, bo, row_w, row_mol, sout, g, accumulate, tt);
}

template <int D>
__global__ __launch_bounds__(512) void k_nfp_readout_table_bwd(const float* __restrict__ dg, const float* __restrict__ s, int o,
                                                               const float* __restrict__ Wnp, const float* __restrict__ row_w,
                                                               const int* __restrict__ row_mol, float* __restrict__ dz,
                                                               float* __restrict__ dh, WgTable tt) {
    nfp_readout_bwd<D, true>(dg, s, o, Wnp, row_w, row_mol, dz, dh, tt);
}

extern "C" int bmp_nfp_layer_table_supported(int d) { return bmp_nfp_layer_supported(d); }
extern "C" int bmp_nfp_readout_table_supported(int d, int o) { return bmp_nfp_readout_tile_supported(d, o); }

// bmp_nfp_layer_tile_fwd over a tile table: n_tiles table entries, mt_rows rows in the arrays; tile_stride 0 (dense rows) or the
// fixed stride of the table's tiles, whose dead rows are then cleared in fv and out.  fv null: forward only.
extern "C" int bmp_nfp_layer_table_fwd(const float* h, int n_tiles, int d, const int* csr_ptr, const int* csr_col, const float* csr_val,
                                       const float* self_w, const int* deg_class, const float* WTp, const float* B, float* fv,
                                       float* out, const int* mt_row0, const int* mt_nblk, int mt_rows, int tile_stride,
                                       hipStream_t st) {
    BMP_REQUIRE(bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, tile_stride, WT_R));
    if (int rc = nfp_layer_fwd_check(bmp_nfp_layer_table_supported(d), true, h, n_tiles, csr_ptr, self_w, deg_class, WTp, B, fv, out))
        return rc;
    BMP_REQUIRE(((uintptr_t)out & 15) == 0);                  // (the clear of a fixed stride's dead rows stores 16 bytes)
    const WgTable tt = {mt_row0, mt_nblk, mt_rows, tile_stride};
    WT_LAUNCH(k_nfp_table_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, self_w, deg_class, WTp, B, fv, out, tt);
    return 0;
}

// ... and its backward: the dead rows of a fixed-stride table are cleared in dpre and dh.  row_w: the weight whose zeros leave
// with dpre == 0 -- the batch's row_w, or on the encoder layout the liveness weight of bmp_nfp_rows_enc.
extern "C" int bmp_nfp_layer_table_bwd(const float* dout, const float* out, int n_tiles, int d, const int* csrT_ptr, const int* csrT_col,
                                       const float* csrT_val, const float* self_w, const int* deg_class, const float* row_w,
                                       const float* Wnp, float* dpre, float* dh, const int* mt_row0, const int* mt_nblk, int mt_rows,
                                       int tile_stride, hipStream_t st) {
    BMP_REQUIRE(bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, tile_stride, WT_R));
    if (int rc = nfp_layer_bwd_check(bmp_nfp_layer_table_supported(d), dout, out, n_tiles, csrT_ptr, self_w, deg_class, row_w, Wnp, dpre, dh))
        return rc;
    const WgTable tt = {mt_row0, mt_nblk, mt_rows, tile_stride};
    WT_LAUNCH(k_nfp_table_bwd, d, n_tiles, wt_lds_bytes(d), st, dout, out, csrT_ptr, csrT_col, csrT_val, self_w, deg_class, row_w, Wnp,
              dpre, dh, tt);
    return 0;
}

// bmp_nfp_readout_tile_fwd over a tile table; a fixed stride's dead rows are cleared in s.
extern "C" int bmp_nfp_readout_table_fwd(const float* h, int n_tiles, int d, int o, const float* WoTp, const float* b, const float* row_w,
                                         const int* row_mol, float* s, float* g, int accumulate, const int* mt_row0,
                                         const int* mt_nblk, int mt_rows, int tile_stride, hipStream_t st) {
    BMP_REQUIRE(bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, tile_stride, WT_R));
    if (int rc = nfp_readout_fwd_check(bmp_nfp_readout_table_supported(d, o), h, n_tiles, WoTp, b, row_w, row_mol, s, g)) return rc;
    BMP_REQUIRE(((uintptr_t)s & 15) == 0);
    const WgTable tt = {mt_row0, mt_nblk, mt_rows, tile_stride};
    const size_t lds = (size_t)WT_R * (d + 4 + NFP_LDZ) * sizeof(float);
    WT_LAUNCH(k_nfp_readout_table_fwd, d, n_tiles, lds, st, h, o, WoTp, b, row_w, row_mol, s, g, accumulate, tt);
    return 0;
}

// ... and its backward: a fixed stride's dead rows are cleared in the dz workspace (the first mt_rows x o floats of ws) and in
// dh; dW_o and db then sum over all mt_rows rows.  ws: bmp_nfp_readout_bwd_ws_floats(mt_rows, d, o) floats.
extern "C" int bmp_nfp_readout_table_bwd(const float* dg, const float* h, const float* s, int n_tiles, int d, int o, const float* Wnp,
                                         const float* row_w, const int* row_mol, float* dh, float* dWT, float* db, float* ws,
                                         size_t ws_floats, const int* mt_row0, const int* mt_nblk, int mt_rows, int tile_stride,
                                         hipStream_t st) {
    BMP_REQUIRE(bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, tile_stride, WT_R));
    if (int rc = nfp_readout_bwd_check(bmp_nfp_readout_table_supported(d, o), dg, h, s, n_tiles, Wnp, row_w, row_mol, dh, dWT, db, ws))
        return rc;
    BMP_REQUIRE((((uintptr_t)ws | (uintptr_t)dh) & 15) == 0 && (mt_rows & 7) == 0);
    BMP_REQUIRE(ws_floats >= bmp_nfp_readout_bwd_ws_floats(mt_rows, d, o));
    const WgTable tt = {mt_row0, mt_nblk, mt_rows, tile_stride};
    const size_t lds = (size_t)WT_R * NFP_LDZ * sizeof(float);
    WT_LAUNCH(k_nfp_readout_table_bwd, d, n_tiles, lds, st, dg, s, o, Wnp, row_w, row_mol, ws, dh, tt);
    return nfp_readout_wgrad(h, mt_rows, d, o, dWT, db, ws, st);
}
