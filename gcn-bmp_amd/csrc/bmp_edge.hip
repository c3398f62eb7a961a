// GGNN propagation step with the edge-network message -- EdgeNetwork of models/ggnn.py:657-720 behind GGNN.update's
// 'edge_network' branch (:245-248), always built without hidden layers (:95).  The network is affine in the adjacency vector of an
// atom pair, so with W_e[p, q] = output_layer.W[p d + q, e] and B[p, q] = output_layer.b[p d + q]
//   m_i = sum_e W_e . agg_e(i) + B . S,   agg_e = the neighbour sum over the bonds of type e,
//                                         S = the sum of h over ALL A padded positions of the atom's molecule
//       = the row_w-weighted sum over the molecule's rows (the virtual pad row with its multiplicity A - n),
//   out = GRU([h, m]) as in bmp_loop.hip (state folded into the h-part; `first`: no r gate, no U term).
// No bias enters the message: the per-edge bias of bmp_ggnn_step_* and the self loop's b_s have no counterpart here.
//
// The kernels' body is wg_step_fwd / wg_step_bwd<D, FIRST, WG_EDGE_NET> of bmp_wtile_gru.h, the one the self-loop kernels
// (bmp_loop.hip) run, with the fifth message operand changed: the tile of S rows in place of the tile of h, and in the backward
// Q_r = row_w[r] T_mol(r), T = the molecule's sum of dm, where the self-loop kernel has dm.  This file holds the kernels and the
// C entries.  Whole tiles whose molecules never straddle a tile.
#include "bmp_wtile_gru.h"

#define EDGE_FWD_ARGS const float* __restrict__ h, const int* __restrict__ ptr, const int* __restrict__ col, const float* __restrict__ val,            \
                      EdgeSeg sg, const float* __restrict__ WTp, const float* __restrict__ BTp, const float* __restrict__ ATp,                         \
                      const float* __restrict__ UcTp, const float* __restrict__ b, float* __restrict__ m, float* __restrict__ rz,                      \
                      float* __restrict__ c, float* __restrict__ hout
#define EDGE_BWD_ARGS const float* __restrict__ dhout, const float* __restrict__ h, const float* __restrict__ rz, const float* __restrict__ c,         \
                      const int* __restrict__ ptrT, const int* __restrict__ colT, const float* __restrict__ valT, EdgeSeg sg,                          \
                      const float* __restrict__ Wnp, const float* __restrict__ Bp, const float* __restrict__ Anp, const float* __restrict__ Ucp,       \
                      float* __restrict__ dh, float* __restrict__ gda, float* __restrict__ rh

template <int D> __global__ __launch_bounds__(512) void k_edge_step_first_tile_fwd(EDGE_FWD_ARGS) {
    wg_step_fwd<D, true, WG_EDGE_NET>(h, ptr, col, val, sg, WTp, nullptr, BTp, nullptr, ATp, UcTp, b, m, rz, c, hout);
}
template <int D> __global__ __launch_bounds__(512) void k_edge_step_later_tile_fwd(EDGE_FWD_ARGS) {
    wg_step_fwd<D, false, WG_EDGE_NET>(h, ptr, col, val, sg, WTp, nullptr, BTp, nullptr, ATp, UcTp, b, m, rz, c, hout);
}
template <int D> __global__ __launch_bounds__(512) void k_edge_step_first_tile_bwd(EDGE_BWD_ARGS) {
    wg_step_bwd<D, true, WG_EDGE_NET>(dhout, h, rz, c, ptrT, colT, valT, sg, Wnp, Bp, Anp, Ucp, dh, gda, rh);
}
template <int D> __global__ __launch_bounds__(512) void k_edge_step_later_tile_bwd(EDGE_BWD_ARGS) {
    wg_step_bwd<D, false, WG_EDGE_NET>(dhout, h, rz, c, ptrT, colT, valT, sg, Wnp, Bp, Anp, Ucp, dh, gda, rh);
}

extern "C" int bmp_ggnn_edge_step_supported(int d) { return d == 64 || d == 128; }

// WTp [4d x d] (row e d + q, column p: W_e[p, q]), ATp [2d x 3d], UcTp [d x d], b [3d]: as bmp_ggnn_step_fwd takes them;
// BTp [d x d] = B^T (K-major), K4-packed.  row_w [N], row_mol [N] (-1: a row of no molecule), mol_row0 / mol_nrows [n_mols]: the
// batch's segments.  Saves m [N x d], rz [N x 2d] and c [N x d], all three null for forward-only evaluation.  N = 128 n_tiles.
extern "C" int bmp_ggnn_edge_step_tile_fwd(const float* h, int n_tiles, int d, int first, const int* csr_ptr, const int* csr_col,
                                           const float* csr_val, const float* row_w, const int* row_mol, const int* mol_row0,
                                           const int* mol_nrows, int n_mols, const float* WTp, const float* BTp, const float* ATp,
                                           const float* UcTp, const float* b, float* m, float* rz, float* c, float* hout,
                                           hipStream_t st) {
    BMP_REQUIRE(row_w && row_mol && mol_row0 && mol_nrows && n_mols > 0);
    if (int rc = wg_fwd_check(bmp_ggnn_edge_step_supported(d), h, n_tiles, first, csr_ptr, WTp, BTp, ATp, UcTp, b, m, rz, c, hout)) return rc;
    const EdgeSeg sg{row_w, row_mol, mol_row0, mol_nrows, n_mols};
    if (first)
        WT_LAUNCH(k_edge_step_first_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, sg, WTp, BTp, ATp, UcTp, b, m, rz, c, hout);
    else
        WT_LAUNCH(k_edge_step_later_tile_fwd, d, n_tiles, wt_lds_bytes(d), st, h, csr_ptr, csr_col, csr_val, sg, WTp, BTp, ATp, UcTp, b, m, rz, c, hout);
    return 0;
}
// Wnat_p [d x 4d], A_p [3d x 2d], Uc_p [d x d]: as bmp_ggnn_step_bwd takes them; B_p [d x d] = B in the reference layout
// [out x in], K4-packed.  Writes dh [N x d], gda [N x 8d] = [G_0 .. G_3 | Q | da_r | da_z | da_c] and, for later calls,
// rh [N x d] = r * h; first != 0: the da_r block is written as zeros, rh is not written (and may be null).
extern "C" int bmp_ggnn_edge_step_tile_bwd(const float* dhout, const float* h, const float* rz, const float* c, int n_tiles, int d,
                                           int first, const int* csrT_ptr, const int* csrT_col, const float* csrT_val,
                                           const float* row_w, const int* row_mol, const int* mol_row0, const int* mol_nrows,
                                           int n_mols, const float* Wnat_p, const float* B_p, const float* A_p, const float* Uc_p,
                                           float* dh, float* gda, float* rh, hipStream_t st) {
    BMP_REQUIRE(row_w && row_mol && mol_row0 && mol_nrows && n_mols > 0);
    if (int rc = wg_bwd_check(bmp_ggnn_edge_step_supported(d), dhout, h, rz, c, n_tiles, first, csrT_ptr, Wnat_p, B_p, A_p, Uc_p, dh, gda, rh)) return rc;
    const EdgeSeg sg{row_w, row_mol, mol_row0, mol_nrows, n_mols};
    if (first)
        WT_LAUNCH(k_edge_step_first_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dhout, h, rz, c, csrT_ptr, csrT_col, csrT_val, sg, Wnat_p, B_p, A_p, Uc_p, dh, gda, rh);
    else
        WT_LAUNCH(k_edge_step_later_tile_bwd, d, n_tiles, wt_lds_bytes(d), st, dhout, h, rz, c, csrT_ptr, csrT_col, csrT_val, sg, Wnat_p, B_p, A_p, Uc_p, dh, gda, rh);
    return 0;
}
