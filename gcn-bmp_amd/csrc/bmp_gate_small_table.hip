// The d = 32 fuse-gate / simple-gate GGNN step over a TILE TABLE: the VAR instances of the kernels of bmp_gate_small.h, for
// batches in the encoder layout (bmp/enclayout.py, with or without de-duplication) and for the fixed-shape batch
// (bmp.packed.StaticPairBatch), which the whole-tile entries of bmp_gate_small.hip cannot take.
#include "bmp_gate_small.h"

// The same step over a tile table: n_tiles table entries of 1..4 live 32-row blocks, mt_rows rows in the arrays; tile_stride 0
// (dense rows) or the fixed stride of the table's tiles, whose dead rows are then cleared in m, act and hout.
extern "C" int bmp_ggnn_gate_step_small_table_fwd(int kind, const float* h, int n_tiles, int d, const int* csr_ptr, const int* csr_col,
                                                  const float* csr_val, const float* WTp, const float* bE, const float* AUp,
                                                  const float* bU, const float* keep, float* m, float* act, float* hout,
                                                  const int* mt_row0, const int* mt_nblk, int mt_rows, int tile_stride, hipStream_t st) {
    BMP_REQUIRE(bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, tile_stride, FS_R));
    return gs_fwd<true>(kind, h, n_tiles, d, csr_ptr, csr_col, csr_val, WTp, bE, AUp, bU, keep, m, act, hout, mt_row0, mt_nblk, tile_stride, st);
}

// ... and its backward: the dead rows of a fixed-stride table are cleared in dh and gda.
extern "C" int bmp_ggnn_gate_step_small_table_bwd(int kind, const float* dhout, const float* h, const float* m, const float* act,
                                                  const float* keep, int n_tiles, int d, const int* csrT_ptr, const int* csrT_col,
                                                  const float* csrT_val, const float* Wnat_p, const float* Unat_p, float* dh, float* gda,
                                                  const int* mt_row0, const int* mt_nblk, int mt_rows, int tile_stride, hipStream_t st) {
    BMP_REQUIRE(bmp_tile_table_ok(mt_row0, mt_nblk, mt_rows, tile_stride, FS_R));
    return gs_bwd<true>(kind, dhout, h, m, act, keep, n_tiles, d, csrT_ptr, csrT_col, csrT_val, Wnat_p, Unat_p, dh, gda, mt_row0, mt_nblk,
                  tile_stride, st);
}
